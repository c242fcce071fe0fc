// mesh_components.hip -- connected components of a ragged mesh batch (include/rfd_components.h), gfx950.
//
// The six rules are written out in the header and restated in tests/components_f64.py; every f64 expression below is
// evaluated as written (the library is built with -ffp-contract=off).  The prefix sums and the grouping of the faces by
// component between the kernels are the host module's; what is here is one thread per face / vertex / mesh, and for the
// measures sixteen lanes per component, as in mesh_decimate.hip: lane j adds the component's faces j, j + 16, ... in order
// and a halving tree of wave shuffles adds the sixteen partial sums.  No floating-point atomics.
//
// The labelling is a lock-free union-find over the V global vertex indices.  parent[i] = i on entry; one thread per valid
// face unites (a, b) and (a, c); unite(u, v) finds both roots and links the LARGER root under the SMALLER with one
// agent-scope compare-and-swap on parent[larger] that expects parent[larger] == larger, and after a failed swap goes on
// from the value the swap returned.
//
// Termination.  The swap replaces the root x by a smaller index, once; the only other store to parent[x], find()'s path
//   halving, replaces a parent by that parent's parent, smaller still: a parent is always
//   <= its child, and strictly less unless the child is a root.  So find() descends strictly, and every retry of unite()
//   strictly lowers u + v (the larger root is replaced by its new parent, which is smaller; the other only descends).  No
//   thread waits for another thread, wave or workgroup.  Both loops carry an explicit bound of V steps on top of that, and
//   find() stops at a parent that is not below its child, so not even a corrupted array can spin or lead outside it.
// Determinism.  The fixed point is unique: two vertices end in one tree exactly if a chain of valid faces joins them, and
//   since every link points to a smaller index the root of a set is its smallest index -- whatever the order of execution,
//   the grid or the XCD placement.  rfd_components_flatten then gives every vertex that root, and everything after it is
//   computed from the roots alone.
// Memory.  Parents are read with agent-scope relaxed atomic loads, never with plain loads: a plain load may be served from
//   a stale L1 line or kept in a register.  A stale parent is still an ancestor (a link is only ever replaced by a link to
//   an ancestor), so it costs steps and never correctness; the swap itself acts on the true value.  Flattening is a
//   launch of its own: the kernel boundary makes every link visible.  Path halving stays because it pays: linking by
//   index, not by rank, leaves chains as long as a mesh's sweep is deep (DESIGN.md section 3 has the times).
#include <stdint.h>

#include "mesh_batch.h"
#include "../../include/rfd_components.h"

namespace {

constexpr int CMP_THREADS = 256;
constexpr int COMP_LANES = 16;                         // partial sums of a component (rule 4)
constexpr int COMPS_PER_BLOCK = CMP_THREADS / COMP_LANES;
constexpr int WALK = 4;                                // faces of a lane whose loads are in flight together

__device__ __forceinline__ int load_parent(const int *parent, int i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x (0 <= x < V): descends strictly, V steps at most.  Path halving on the way: parent[x] = parent[parent[x]]
// by a relaxed atomic store.  It writes to a non-root only, which the swap of unite() never changes again, and what it
// writes is an ancestor of x below x, so every statement above holds with it; two racing stores leave either ancestor.
__device__ __forceinline__ int find_root(int *parent, int x, int V) {
  for (int step = 0; step < V; ++step) {
    const int p = load_parent(parent, x);
    if ((unsigned)p >= (unsigned)x) break;             // p == x: a root (anything else is not a parent: stop here too)
    const int g = load_parent(parent, p);
    if ((unsigned)g >= (unsigned)p) {                  // p is the root
      x = p;
      break;
    }
    __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
  }
  return x;
}

__device__ __forceinline__ void unite(int *parent, int u, int v, int V) {
  for (int step = 0; step < V; ++step) {
    u = find_root(parent, u, V), v = find_root(parent, v, V);
    if (u == v) return;
    if (u > v) {
      const int s = u;
      u = v, v = s;
    }
    int seen = v;                                      // u < v: v goes under u if it is still a root
    if (__hip_atomic_compare_exchange_strong(parent + v, &seen, u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return;
    if ((unsigned)seen >= (unsigned)v) return;         // not a parent of v: a corrupted array
    v = seen;                                          // somebody linked v first: on from its new parent, below v
  }
}

// the three global corners of face f, or false for an invalid face (rule 1)
__device__ __forceinline__ bool global_corners(const int *__restrict__ faces, const int *__restrict__ tend,
                                               const int *__restrict__ vend, int K, int V, long f, int &a, int &b,
                                               int &c) {
  const int k = segment_of(tend, K, (int)f);
  const int v0 = vend[k], nv = vend[k + 1] - v0;
  const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  if ((unsigned)ia >= (unsigned)nv || (unsigned)ib >= (unsigned)nv || (unsigned)ic >= (unsigned)nv) return false;
  a = v0 + ia, b = v0 + ib, c = v0 + ic;
  return a >= 0 && (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V;
}

__global__ __launch_bounds__(CMP_THREADS) void union_kernel(int F, int K, int V, const int *__restrict__ faces,
                                                            const int *__restrict__ tend, const int *__restrict__ vend,
                                                            int *parent) {
  const long f = (long)blockIdx.x * CMP_THREADS + threadIdx.x;
  if (f >= F) return;
  int a, b, c;
  if (!global_corners(faces, tend, vend, K, V, f, a, b, c)) return;
  unite(parent, a, b, V);
  unite(parent, a, c, V);
}

__global__ __launch_bounds__(CMP_THREADS) void flatten_kernel(int V, int *parent, int *root) {
  const long i = (long)blockIdx.x * CMP_THREADS + threadIdx.x;
  if (i >= V) return;
  root[i] = find_root(parent, (int)i, V);
}

__global__ __launch_bounds__(CMP_THREADS) void face_roots_kernel(int F, int K, int V, const int *__restrict__ faces,
                                                                 const int *__restrict__ tend,
                                                                 const int *__restrict__ vend,
                                                                 const int *__restrict__ root, int *__restrict__ froot,
                                                                 int *__restrict__ corner, int *__restrict__ is_root,
                                                                 int *__restrict__ named) {
  const long f = (long)blockIdx.x * CMP_THREADS + threadIdx.x;
  if (f >= F) return;
  int a = -1, b = -1, c = -1, r = -1;
  if (global_corners(faces, tend, vend, K, V, f, a, b, c)) {
    r = root[a];
    if ((unsigned)r >= (unsigned)V) r = -1;
  } else {
    a = b = c = -1;
  }
  if (r < 0) a = b = c = -1;
  froot[f] = r;
  corner[3 * f] = a, corner[3 * f + 1] = b, corner[3 * f + 2] = c;
  if (r < 0) return;
  is_root[r] = 1;                                      // several faces may name a root or a vertex: they all store the same word
  named[a] = 1, named[b] = 1, named[c] = 1;
}

__global__ __launch_bounds__(CMP_THREADS) void labels_kernel(int F, int K, int V, const int *__restrict__ froot,
                                                             const int *__restrict__ root, const int *__restrict__ named,
                                                             const int *__restrict__ rincl, const int *__restrict__ tend,
                                                             const int *__restrict__ cbase, int *__restrict__ glabel,
                                                             int *__restrict__ llabel, int *__restrict__ vlabel) {
  const long i = (long)blockIdx.x * CMP_THREADS + threadIdx.x;
  if (i < F) {
    const int r = froot[i];
    int g = -1, l = -1;
    if ((unsigned)r < (unsigned)V) {
      g = rincl[r] - 1;
      l = g - cbase[segment_of(tend, K, (int)i)];
    }
    glabel[i] = g, llabel[i] = l;
  }
  if (i < V) {
    const int r = root[i];
    vlabel[i] = named[i] && (unsigned)r < (unsigned)V ? rincl[r] - 1 : -1;
  }
}

// rule 4: COMP_LANES lanes per component
template <typename T>
__global__ __launch_bounds__(CMP_THREADS) void measure_kernel(int C, int F, int V, const void *__restrict__ vertices,
                                                              const int *__restrict__ corner,
                                                              const int *__restrict__ rowptr, const int *__restrict__ col,
                                                              int *__restrict__ faces, double *__restrict__ area,
                                                              double *__restrict__ volume, double *__restrict__ lo,
                                                              double *__restrict__ hi) {
  const int lane = threadIdx.x % COMP_LANES;
  const long comp = (long)blockIdx.x * COMPS_PER_BLOCK + threadIdx.x / COMP_LANES;
  int begin = 0, end = 0;
  if (comp < C) begin = max(rowptr[comp], 0), end = min(rowptr[comp + 1], F);      // col has F entries
  double sa = 0.0, st = 0.0;
  double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  // A lane's faces come WALK at a time: their three levels of loads (face, corners, vertices) are issued together, and the
  // terms are then added in the faces' order, so the sums keep their shape.  (One face at a time, a component of 50 000
  // faces is 3 200 round trips to memory per lane: DESIGN.md section 3 has the times.)
  for (int base = begin + lane; base < end; base += COMP_LANES * WALK) {
    int f[WALK], i0[WALK], i1[WALK], i2[WALK];
    bool ok[WALK];
#pragma unroll
    for (int u = 0; u < WALK; ++u) {
      const int at = base + u * COMP_LANES;
      f[u] = at < end ? col[at] : -1;
      ok[u] = (unsigned)f[u] < (unsigned)F;
    }
#pragma unroll
    for (int u = 0; u < WALK; ++u) {
      const long row = ok[u] ? f[u] : 0;
      i0[u] = corner[3 * row], i1[u] = corner[3 * row + 1], i2[u] = corner[3 * row + 2];
      ok[u] = ok[u] && (unsigned)i0[u] < (unsigned)V && (unsigned)i1[u] < (unsigned)V && (unsigned)i2[u] < (unsigned)V;
    }
    D3 p0[WALK], p1[WALK], p2[WALK];
#pragma unroll
    for (int u = 0; u < WALK; ++u) {
      p0[u] = ld3<T>(vertices, (size_t)(ok[u] ? i0[u] : 0)), p1[u] = ld3<T>(vertices, (size_t)(ok[u] ? i1[u] : 0));
      p2[u] = ld3<T>(vertices, (size_t)(ok[u] ? i2[u] : 0));
    }
#pragma unroll
    for (int u = 0; u < WALK; ++u) {
      if (!ok[u]) continue;
      const D3 n = cross(sub(p1[u], p0[u]), sub(p2[u], p0[u]));
      const double L = sqrt(dot(n, n));
      const double a = usable_length(L) ? 0.5 * L : 0.0;
      double t = dot(p0[u], cross(p1[u], p2[u]));
      if (!finite_f64(t)) t = 0.0;
      sa = sa + a;
      st = st + t;
      const double q[9] = {p0[u].x, p0[u].y, p0[u].z, p1[u].x, p1[u].y, p1[u].z, p2[u].x, p2[u].y, p2[u].z};
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        if (!finite_f64(q[j])) continue;
        mn[j % 3] = fmin(mn[j % 3], q[j]);
        mx[j % 3] = fmax(mx[j % 3], q[j]);
      }
    }
  }
  // 16 -> 8 -> 4 -> 2 -> 1: lane j takes lane j + step of its own group of sixteen (what the upper lanes fetch is unused)
#pragma unroll
  for (int step = COMP_LANES / 2; step >= 1; step >>= 1) {
    sa = sa + __shfl_down(sa, step, COMP_LANES);
    st = st + __shfl_down(st, step, COMP_LANES);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      mn[j] = fmin(mn[j], __shfl_down(mn[j], step, COMP_LANES));
      mx[j] = fmax(mx[j], __shfl_down(mx[j], step, COMP_LANES));
    }
  }
  if (lane != 0 || comp >= C) return;
  faces[comp] = max(end - begin, 0);
  area[comp] = sa;
  volume[comp] = st / 6.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) lo[3 * comp + j] = mn[j], hi[3 * comp + j] = mx[j];
}

__device__ __forceinline__ double measure_of(int measure, int c, const int *__restrict__ faces,
                                             const double *__restrict__ area, const double *__restrict__ volume) {
  return measure == RFD_COMPONENTS_BY_FACES ? (double)faces[c] : measure == RFD_COMPONENTS_BY_AREA ? area[c]
                                                                                                    : fabs(volume[c]);
}

// rule 5: one thread per mesh
__global__ __launch_bounds__(CMP_THREADS) void select_kernel(int K, int C, int measure, int largest_only, double t,
                                                             int drop_cavities, const int *__restrict__ cbase,
                                                             const int *__restrict__ faces,
                                                             const double *__restrict__ area,
                                                             const double *__restrict__ volume,
                                                             unsigned char *__restrict__ keep_comp,
                                                             int *__restrict__ kept) {
  const long k = (long)blockIdx.x * CMP_THREADS + threadIdx.x;
  if (k >= K) return;
  const int c0 = max(cbase[k], 0), c1 = min(cbase[k + 1], C);
  int count = 0;
  if (c1 > c0) {
    int best = c0;
    double mb = measure_of(measure, c0, faces, area, volume);
    for (int c = c0 + 1; c < c1; ++c) {
      const double m = measure_of(measure, c, faces, area, volume);
      if (m > mb) best = c, mb = m;
    }
    const double bar = t * mb, vb = volume[best];
    for (int c = c0; c < c1; ++c) {
      bool keep = c == best;
      if (!keep && !largest_only) keep = measure_of(measure, c, faces, area, volume) >= bar;
      if (keep && drop_cavities && c != best && volume[c] * vb < 0.0) keep = false;
      keep_comp[c] = keep ? 1 : 0;
      count += keep ? 1 : 0;
    }
  }
  kept[k] = count;
}

__global__ __launch_bounds__(CMP_THREADS) void mark_kernel(int F, int C, int V, const int *__restrict__ glabel,
                                                           const int *__restrict__ corner,
                                                           const unsigned char *__restrict__ keep_comp,
                                                           unsigned char *__restrict__ keep, int *__restrict__ used) {
  const long f = (long)blockIdx.x * CMP_THREADS + threadIdx.x;
  if (f >= F) return;
  const int g = glabel[f];
  const bool stays = (unsigned)g < (unsigned)C && keep_comp[g];
  keep[f] = stays ? 1 : 0;
  if (!stays) return;
  for (int c = 0; c < 3; ++c) {
    const int i = corner[3 * f + c];
    if ((unsigned)i < (unsigned)V) used[i] = 1;        // several faces may name a vertex: they all store the same word
  }
}

// rule 6 for the vertices: W is an unsigned word of the vertices' width, so the copy is bit for bit
template <typename W>
__global__ __launch_bounds__(CMP_THREADS) void gather_vertices_kernel(int V, int V2, const void *__restrict__ vertices,
                                                                      const int *__restrict__ used,
                                                                      const int *__restrict__ vincl,
                                                                      void *__restrict__ v2) {
  const long i = (long)blockIdx.x * CMP_THREADS + threadIdx.x;
  if (i >= V || !used[i]) return;
  const long at = vincl[i] - 1;
  if (at < 0 || at >= V2) return;
  const W *__restrict__ from = static_cast<const W *>(vertices) + 3 * i;
  W *__restrict__ to = static_cast<W *>(v2) + 3 * at;
  to[0] = from[0], to[1] = from[1], to[2] = from[2];
}

bool indexable(int F) { return F > 0 && (long)F * 3 <= INT_MAX; }

}  // namespace

RFD_API int rfd_components_union(int F, int K, int V, const int *faces, const int *tend, const int *vend, int *parent,
                                 void *stream) {
  if (!indexable(F) || K <= 0 || V <= 0) return rfd_invalid("rfd_components_union: K > 0, V > 0, 0 < 3 F < 2^31");
  if (!faces || !tend || !vend || !parent) return MESH_NULL("rfd_components_union");
  union_kernel<<<blocks_of(F, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(F, K, V, faces, tend, vend, parent);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_flatten(int V, int *parent, int *root, void *stream) {
  if (V <= 0) return rfd_invalid("rfd_components_flatten: V must be positive");
  if (!parent || !root) return MESH_NULL("rfd_components_flatten");
  flatten_kernel<<<blocks_of(V, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(V, parent, root);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_face_roots(int F, int K, int V, const int *faces, const int *tend, const int *vend,
                                      const int *root, int *froot, int *corner, int *is_root, int *named, void *stream) {
  if (!indexable(F) || K <= 0 || V <= 0) return rfd_invalid("rfd_components_face_roots: K > 0, V > 0, 0 < 3 F < 2^31");
  if (!faces || !tend || !vend || !root || !froot || !corner || !is_root || !named)
    return MESH_NULL("rfd_components_face_roots");
  face_roots_kernel<<<blocks_of(F, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(F, K, V, faces, tend, vend, root,
                                                                                        froot, corner, is_root, named);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_labels(int F, int K, int V, const int *froot, const int *root, const int *named,
                                  const int *rincl, const int *tend, const int *cbase, int *glabel, int *llabel,
                                  int *vlabel, void *stream) {
  if (F <= 0 || K <= 0 || V <= 0) return rfd_invalid("rfd_components_labels: counts must be positive");
  if (!froot || !root || !named || !rincl || !tend || !cbase || !glabel || !llabel || !vlabel)
    return MESH_NULL("rfd_components_labels");
  labels_kernel<<<blocks_of(F > V ? F : V, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(
      F, K, V, froot, root, named, rincl, tend, cbase, glabel, llabel, vlabel);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_measure(int C, int F, int V, int v_is_f32, const void *vertices, const int *corner,
                                   const int *rowptr, const int *col, int *faces, double *area, double *volume,
                                   double *lo, double *hi, void *stream) {
  if (C <= 0 || V <= 0 || !indexable(F)) return rfd_invalid("rfd_components_measure: C > 0, V > 0, 0 < 3 F < 2^31");
  if (!vertices || !corner || !rowptr || !col || !faces || !area || !volume || !lo || !hi)
    return MESH_NULL("rfd_components_measure");
  const unsigned grid = blocks_of(C, COMPS_PER_BLOCK);
  if (v_is_f32)
    measure_kernel<float><<<grid, CMP_THREADS, 0, (hipStream_t)stream>>>(C, F, V, vertices, corner, rowptr, col, faces,
                                                                         area, volume, lo, hi);
  else
    measure_kernel<double><<<grid, CMP_THREADS, 0, (hipStream_t)stream>>>(C, F, V, vertices, corner, rowptr, col, faces,
                                                                          area, volume, lo, hi);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_select(int K, int C, int measure, int largest_only, double t, int drop_cavities,
                                  const int *cbase, const int *faces, const double *area, const double *volume,
                                  unsigned char *keep_comp, int *kept, void *stream) {
  if (K <= 0 || C <= 0) return rfd_invalid("rfd_components_select: counts must be positive");
  if (measure != RFD_COMPONENTS_BY_FACES && measure != RFD_COMPONENTS_BY_AREA && measure != RFD_COMPONENTS_BY_ABS_VOLUME)
    return rfd_invalid("rfd_components_select: measure must be faces (0), area (1) or abs_volume (2)");
  if (!largest_only && !(t >= 0.0 && t <= 1.0)) return rfd_invalid("rfd_components_select: the fraction t must be in [0, 1]");
  if (!cbase || !faces || !area || !volume || !keep_comp || !kept) return MESH_NULL("rfd_components_select");
  select_kernel<<<blocks_of(K, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(
      K, C, measure, largest_only, largest_only ? 1.0 : t, drop_cavities, cbase, faces, area, volume, keep_comp, kept);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_mark(int F, int C, int V, const int *glabel, const int *corner,
                                const unsigned char *keep_comp, unsigned char *keep, int *used, void *stream) {
  if (!indexable(F) || C <= 0 || V <= 0) return rfd_invalid("rfd_components_mark: C > 0, V > 0, 0 < 3 F < 2^31");
  if (!glabel || !corner || !keep_comp || !keep || !used) return MESH_NULL("rfd_components_mark");
  mark_kernel<<<blocks_of(F, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(F, C, V, glabel, corner, keep_comp, keep,
                                                                                  used);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_compact_faces(int F, int K, int V, const int *tend, const int *corner,
                                         const unsigned char *keep, const int *fincl, const int *vincl, const int *vend2,
                                         int *f2, void *stream) {
  if (!indexable(F) || K <= 0 || V <= 0)
    return rfd_invalid("rfd_components_compact_faces: K > 0, V > 0, 0 < 3 F < 2^31");
  if (!tend || !corner || !keep || !fincl || !vincl || !vend2 || !f2) return MESH_NULL("rfd_components_compact_faces");
  compact_faces_kernel<CMP_THREADS><<<blocks_of(F, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(
      F, K, V, corner, tend, nullptr, nullptr, keep, fincl, vincl, vend2, f2);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_components_gather_vertices(int V, int V2, int v_is_f32, const void *vertices, const int *used,
                                           const int *vincl, void *v2, void *stream) {
  if (V <= 0 || V2 <= 0) return rfd_invalid("rfd_components_gather_vertices: counts must be positive");
  if (!vertices || !used || !vincl || !v2) return MESH_NULL("rfd_components_gather_vertices");
  if (v_is_f32)
    gather_vertices_kernel<uint32_t><<<blocks_of(V, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(V, V2, vertices,
                                                                                                        used, vincl, v2);
  else
    gather_vertices_kernel<uint64_t><<<blocks_of(V, CMP_THREADS), CMP_THREADS, 0, (hipStream_t)stream>>>(V, V2, vertices,
                                                                                                        used, vincl, v2);
  RFD_CHECK_LAUNCH();
  return 0;
}
