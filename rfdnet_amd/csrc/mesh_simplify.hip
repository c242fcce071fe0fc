// mesh_simplify.hip -- quadric edge collapse in parallel rounds (include/rfd_simplify.h), gfx950.
//
// Rules S0-S7 are written out in the header and restated in tests/simplify_f64.py; every f64 expression below is
// evaluated as written (the library is built with -ffp-contract=off), so costs, and with them the order of the
// collapses, are the restatement's bit for bit.  The grouping between the kernels (stable sorts, prefix sums) is the
// host module's.  The hot kernel is one thread per edge: an edge walks the corner rows of its two ends (about six faces
// each on a marching-cubes mesh), gathers their positions and tests every face; these are scattered 8-byte loads with
// some sixty f64 operations per face, no reuse a tile could hold, and rows too short to share among lanes, so a wave
// simply keeps 64 independent walks in flight.  Integer atomicMin only (S4's minima).  Every index read from memory is
// checked against its array before it is used: a corner row in walk(), the one place that reads one for the checks of
// S1 and S3.  The mesh of an item, the f64 helpers and S7's kernel are mesh_batch.h's, shared with mesh_decimate.hip.
#include "mesh_batch.h"
#include "../../include/rfd_simplify.h"

namespace {

constexpr int SIM_THREADS = 256;

struct Tri {
  int i[3];
};
// the working face f, or -1 -1 -1 if it is dead or names something outside the batch
__device__ __forceinline__ Tri ld_face(const int *__restrict__ face, int f, int V) {
  Tri t = {{face[3 * (size_t)f], face[3 * (size_t)f + 1], face[3 * (size_t)f + 2]}};
  if ((unsigned)t.i[0] >= (unsigned)V || (unsigned)t.i[1] >= (unsigned)V || (unsigned)t.i[2] >= (unsigned)V)
    t.i[0] = t.i[1] = t.i[2] = -1;
  return t;
}
__device__ __forceinline__ bool holds(Tri t, int v) { return t.i[0] == v || t.i[1] == v || t.i[2] == v; }

// the working mesh: V positions, F working faces and the corner rows of the round (col has 3 F entries)
struct Star {
  int V, F;
  const int *face;
  const double *pos;
  const int *rowptr, *col;
};
// The alive faces at the corners of vertex v, in ascending order of the row: body(t, s) sees the face and the slot s of
// the corner in it and answers whether the walk stops there; -> whether it was stopped.  The one place where a corner
// row is read: the row is clamped to col, the corner checked against 3 F, the face's indices against V (ld_face).
template <typename Body>
__device__ __forceinline__ bool walk(const Star &m, int v, Body body) {
  const int begin = max(m.rowptr[v], 0), end = min(m.rowptr[v + 1], 3 * m.F);
  for (int at = begin; at < end; ++at) {
    const int corner = m.col[at];
    if ((unsigned)corner >= 3u * (unsigned)m.F) continue;
    const int f = corner / 3;
    const Tri t = ld_face(m.face, f, m.V);
    if (t.i[0] >= 0 && body(t, corner - 3 * f)) return true;
  }
  return false;
}

// S0, first half: one thread per vertex and per face
template <typename T>
__global__ __launch_bounds__(SIM_THREADS) void init_kernel(int V, int F, int K, const void *__restrict__ vertices,
                                                           const int *__restrict__ faces, const int *__restrict__ vend,
                                                           const int *__restrict__ tend, const int *__restrict__ n_faces,
                                                           double *__restrict__ pos, unsigned char *__restrict__ nonfinite,
                                                           int *__restrict__ face) {
  const long i = (long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i < V) {
    const T *q = static_cast<const T *>(vertices) + i * 3;
    const double x = (double)q[0], y = (double)q[1], z = (double)q[2];
    pos[3 * i] = x, pos[3 * i + 1] = y, pos[3 * i + 2] = z;
    nonfinite[i] = (finite_f64(x) && finite_f64(y) && finite_f64(z)) ? 0 : 1;
  }
  if (i < F) {
    const int k = segment_of(tend, K, (int)i);
    const int v0 = vend[k], nv = vend[k + 1] - v0;
    const int a = faces[3 * i], b = faces[3 * i + 1], c = faces[3 * i + 2];
    const bool part = tend[k + 1] - tend[k] > n_faces[k];
    const bool ok = part && v0 >= 0 && nv >= 0 && (long)v0 + nv <= V && (unsigned)a < (unsigned)nv &&
                    (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv && a != b && b != c && a != c;
    face[3 * i] = ok ? v0 + a : -1;
    face[3 * i + 1] = ok ? v0 + b : -1;
    face[3 * i + 2] = ok ? v0 + c : -1;
  }
}

// S1: one thread per vertex adds its corners in order
__global__ __launch_bounds__(SIM_THREADS) void quadrics_kernel(int V, int F, const double *__restrict__ pos,
                                                               const int *__restrict__ face,
                                                               const int *__restrict__ rowptr, const int *__restrict__ col,
                                                               double *__restrict__ Q) {
  const long v = (long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (v >= V) return;
  double acc[10];
#pragma unroll
  for (int t = 0; t < 10; ++t) acc[t] = 0.0;
  walk(Star{V, F, face, pos, rowptr, col}, (int)v, [&](Tri t, int) {
    const D3 p0 = ld3<double>(pos, t.i[0]), p1 = ld3<double>(pos, t.i[1]), p2 = ld3<double>(pos, t.i[2]);
    const auto [m, w, usable] = face_plane(p0, p1, p2);
    if (!usable) return false;
    const double d = -dot(m, p0);
    const double gx = w * m.x, gy = w * m.y, gz = w * m.z, e = w * d;
    acc[0] = acc[0] + gx * m.x;
    acc[1] = acc[1] + gx * m.y;
    acc[2] = acc[2] + gx * m.z;
    acc[3] = acc[3] + gy * m.y;
    acc[4] = acc[4] + gy * m.z;
    acc[5] = acc[5] + gz * m.z;
    acc[6] = acc[6] + e * m.x;
    acc[7] = acc[7] + e * m.y;
    acc[8] = acc[8] + e * m.z;
    acc[9] = acc[9] + e * d;
    return false;
  });
#pragma unroll
  for (int t = 0; t < 10; ++t) Q[10 * v + t] = acc[t];
}

// S0, second half: the slot at the head of a run of equal keys is the run's edge
__global__ __launch_bounds__(SIM_THREADS) void edges_kernel(int V, int F, const long long *__restrict__ skey,
                                                            const int *__restrict__ horder, const int *__restrict__ face,
                                                            int *__restrict__ ea, int *__restrict__ eb,
                                                            int *__restrict__ eface, int *__restrict__ eapex,
                                                            unsigned char *__restrict__ efrozen,
                                                            unsigned char *__restrict__ vfrozen) {
  const long n = 3l * F;
  const long i = (long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i >= n) return;
  int a = -1, b = -1, f0 = -1, f1 = -1, c0 = -1, c1 = -1;
  bool frozen = true;
  const long long key = skey[i];
  const bool head = key >= 0 && key < (long long)V * V && (i == 0 || skey[i - 1] != key);
  if (head) {
    a = (int)(key / V), b = (int)(key % V);
    long run = 1;
    while (i + run < n && skey[i + run] == key) ++run;
    if (run == 2) {
      const int h0 = horder[i], h1 = horder[i + 1];
      if ((unsigned)h0 < 3u * (unsigned)F && (unsigned)h1 < 3u * (unsigned)F) {
        const int g0 = h0 / 3, s0 = h0 - 3 * g0, g1 = h1 / 3, s1 = h1 - 3 * g1;
        const Tri t0 = ld_face(face, g0, V), t1 = ld_face(face, g1, V);
        const bool fits = t0.i[0] >= 0 && t1.i[0] >= 0 && g0 != g1 && holds(t0, a) && holds(t0, b) && holds(t1, a) &&
                          holds(t1, b);
        if (fits && (t0.i[s0] == a) != (t1.i[s1] == a)) {          // opposite directions along the edge
          frozen = false;
          f0 = g0, f1 = g1, c0 = t0.i[(s0 + 2) % 3], c1 = t1.i[(s1 + 2) % 3];
        }
      }
    }
    if (frozen) vfrozen[a] = 1, vfrozen[b] = 1;          // several edges may name a vertex: they all store the same byte
  }
  ea[i] = a, eb[i] = b;
  eface[2 * i] = f0, eface[2 * i + 1] = f1;
  eapex[2 * i] = c0, eapex[2 * i + 1] = c1;
  efrozen[i] = frozen ? 1 : 0;
}

struct Quadric {
  double axx, axy, axz, ayy, ayz, azz, bx, by, bz, c;
};
__device__ __forceinline__ double quadric_cost(const Quadric &q, D3 p) {
  const double hx = (q.axx * p.x + q.axy * p.y) + q.axz * p.z;
  const double hy = (q.axy * p.x + q.ayy * p.y) + q.ayz * p.z;
  const double hz = (q.axz * p.x + q.ayz * p.y) + q.azz * p.z;
  return (((p.x * hx + p.y * hy) + p.z * hz) + 2.0 * ((q.bx * p.x + q.by * p.y) + q.bz * p.z)) + q.c;
}

// S3's flip guard for the faces of `moved` that do not hold `other`; true = rejected
__device__ bool star_flips(Star m, int moved, int other, D3 p) {
  const D3 o = ld3<double>(m.pos, moved);
  return walk(m, moved, [&](Tri t, int s) {
    if (t.i[s] != moved || holds(t, other)) return false;
    const D3 q1 = ld3<double>(m.pos, t.i[(s + 1) % 3]), q2 = ld3<double>(m.pos, t.i[(s + 2) % 3]);
    const D3 k = cross(sub(q1, o), sub(q2, o));
    const double Lk = sqrt(dot(k, k));
    const D3 d1 = sub(q1, p), d2 = sub(q2, p);
    const double l1 = sqrt(dot(d1, d1)), l2 = sqrt(dot(d2, d2));
    if (!usable_length(l1) || !usable_length(l2)) return true;
    const D3 u1 = {d1.x / l1, d1.y / l1, d1.z / l1}, u2 = {d2.x / l2, d2.y / l2, d2.z / l2};
    if (fabs(dot(u1, u2)) > 0.999) return true;
    const D3 n = cross(u1, u2);
    const double Ln = sqrt(dot(n, n));
    if (!usable_length(Ln)) return true;
    return usable_length(Lk) && dot(n, k) < 0.2 * (Ln * Lk);
  });
}

// does some alive face of v hold w?
__device__ bool adjacent(const Star &m, int v, int w) {
  return walk(m, v, [&](Tri t, int) { return holds(t, v) && holds(t, w); });
}

// does a face of v without `other` hold both c0 and c1?
__device__ bool holds_both_apexes(const Star &m, int v, int other, int c0, int c1) {
  return walk(m, v, [&](Tri t, int) { return holds(t, v) && !holds(t, other) && holds(t, c0) && holds(t, c1); });
}

// S3's link condition; true = holds
__device__ bool link_ok(Star m, int a, int b, int c0, int c1) {
  if (c0 == c1) return false;
  const bool pinched = walk(m, a, [&](Tri t, int) {
    if (!holds(t, a) || holds(t, b)) return false;
    for (int s = 0; s < 3; ++s) {
      const int w = t.i[s];
      if (w == a || w == c0 || w == c1) continue;
      if (adjacent(m, b, w)) return true;
    }
    return false;
  });
  return !pinched && !(holds_both_apexes(m, a, b, c0, c1) && holds_both_apexes(m, b, a, c0, c1));
}

// S2 and S3: one thread per edge slot
__global__ __launch_bounds__(SIM_THREADS) void edge_costs_kernel(
    int V, int F, int K, const int *__restrict__ vend, const int *__restrict__ ea, const int *__restrict__ eb,
    const int *__restrict__ eapex, const unsigned char *__restrict__ efrozen, const unsigned char *__restrict__ vfrozen,
    const int *__restrict__ face, const double *__restrict__ pos, const double *__restrict__ Q,
    const int *__restrict__ rowptr, const int *__restrict__ col, double *__restrict__ cost, double *__restrict__ epos,
    unsigned char *__restrict__ legal, int *__restrict__ emesh) {
  const long i = (long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i >= 3l * F) return;
  const double inf = __longlong_as_double(0x7ff0000000000000ll);
  double best = inf;
  D3 p = {0.0, 0.0, 0.0};
  bool ok = false;
  const int a = ea[i], b = eb[i], c0 = eapex[2 * i], c1 = eapex[2 * i + 1];
  if ((unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && a < b && (unsigned)c0 < (unsigned)V &&
      (unsigned)c1 < (unsigned)V && !efrozen[i] && !vfrozen[a] && !vfrozen[b]) {
    const double *qa = Q + 10 * (size_t)a, *qb = Q + 10 * (size_t)b;
    const Quadric q = {qa[0] + qb[0], qa[1] + qb[1], qa[2] + qb[2], qa[3] + qb[3], qa[4] + qb[4],
                       qa[5] + qb[5], qa[6] + qb[6], qa[7] + qb[7], qa[8] + qb[8], qa[9] + qb[9]};
    const D3 pa = ld3<double>(pos, a), pb = ld3<double>(pos, b);
    const D3 mid = {(pa.x + pb.x) * 0.5, (pa.y + pb.y) * 0.5, (pa.z + pb.z) * 0.5};
    const D3 t = sub(pb, pa);
    const double len2 = dot(t, t);
    const Adjugate3 adj = adjugate(q.axx, q.axy, q.axz, q.ayy, q.ayz, q.azz);
    if (adj.det != 0.0 && finite_f64(adj.det)) {
      const D3 y = solve(adj, -q.bx, -q.by, -q.bz);
      if (finite_f64(y.x) && finite_f64(y.y) && finite_f64(y.z)) {
        const D3 s = sub(y, mid);
        if (dot(s, s) <= len2) {
          const double c = quadric_cost(q, y);
          if (c < best) best = c, p = y;
        }
      }
    }
    const D3 rest[3] = {mid, pa, pb};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double c = quadric_cost(q, rest[j]);
      if (c < best) best = c, p = rest[j];
    }
    const Star m = {V, F, face, pos, rowptr, col};
    ok = best < inf && link_ok(m, a, b, c0, c1) && !star_flips(m, a, b, p) && !star_flips(m, b, a, p);
  }
  cost[i] = ok ? best + 0.0 : inf;          // -0 + 0 = +0: one zero for the sort
  epos[3 * i] = p.x, epos[3 * i + 1] = p.y, epos[3 * i + 2] = p.z;
  legal[i] = ok ? 1 : 0;
  emesh[i] = ok ? segment_of(vend, K, a) : K;
}

__global__ __launch_bounds__(SIM_THREADS) void vertex_min_kernel(int V, int F, int pass, const int *__restrict__ ea,
                                                                 const int *__restrict__ eb,
                                                                 const unsigned char *__restrict__ legal,
                                                                 const int *__restrict__ rank,
                                                                 const int *__restrict__ other, int *__restrict__ vmin) {
  const long i = (long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i >= 3l * F) return;
  const int a = ea[i], b = eb[i];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V) return;
  if (pass == 0) {
    if (!legal[i]) return;
    atomicMin(vmin + a, rank[i]);
    atomicMin(vmin + b, rank[i]);
  } else {
    atomicMin(vmin + a, other[b]);
    atomicMin(vmin + b, other[a]);
  }
}

__global__ __launch_bounds__(SIM_THREADS) void select_kernel(int V, int F, const int *__restrict__ ea,
                                                             const int *__restrict__ eb,
                                                             const unsigned char *__restrict__ legal,
                                                             const int *__restrict__ rank, const int *__restrict__ m2,
                                                             unsigned char *__restrict__ sel) {
  const long i = (long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i >= 3l * F) return;
  const int a = ea[i], b = eb[i];
  bool s = false;
  if ((unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && legal[i]) s = rank[i] == m2[a] && rank[i] == m2[b];
  sel[i] = s ? 1 : 0;
}

// S5: one thread per kept edge; the stars of kept edges are disjoint, so nobody else touches what it writes
__global__ __launch_bounds__(SIM_THREADS) void apply_kernel(int V, int F, const unsigned char *__restrict__ keep,
                                                            const int *__restrict__ ea, const int *__restrict__ eb,
                                                            const int *__restrict__ eface,
                                                            const double *__restrict__ epos,
                                                            const int *__restrict__ rowptr, const int *__restrict__ col,
                                                            double *__restrict__ pos, double *__restrict__ Q,
                                                            int *__restrict__ face) {
  const long i = (long)blockIdx.x * SIM_THREADS + threadIdx.x;
  if (i >= 3l * F || !keep[i]) return;
  const int a = ea[i], b = eb[i], f0 = eface[2 * i], f1 = eface[2 * i + 1];
  if ((unsigned)a >= (unsigned)V || (unsigned)b >= (unsigned)V || (unsigned)f0 >= (unsigned)F ||
      (unsigned)f1 >= (unsigned)F)
    return;
  for (int t = 0; t < 3; ++t) pos[3 * (size_t)a + t] = epos[3 * i + t];
  for (int t = 0; t < 10; ++t) Q[10 * (size_t)a + t] = Q[10 * (size_t)a + t] + Q[10 * (size_t)b + t];
  const int begin = max(rowptr[b], 0), end = min(rowptr[b + 1], 3 * F);
  for (int at = begin; at < end; ++at) {
    const int corner = col[at];
    if ((unsigned)corner >= 3u * (unsigned)F) continue;
    if (face[corner] == b) face[corner] = a;
  }
  for (int t = 0; t < 3; ++t) face[3 * (size_t)f0 + t] = -1, face[3 * (size_t)f1 + t] = -1;
}

int check_sizes(const char *msg, int V, int F) {
  if (V <= 0 || F <= 0 || (long)F * 3 > INT_MAX) return rfd_invalid(msg);
  return 0;
}

}  // namespace

RFD_API int rfd_simplify_init(int V, int F, int K, int v_is_f32, const void *vertices, const int *faces, const int *vend,
                              const int *tend, const int *n_faces, double *pos, unsigned char *nonfinite, int *face,
                              void *stream) {
  if (int rc = check_sizes("rfd_simplify_init: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (K <= 0) return rfd_invalid("rfd_simplify_init: K must be positive");
  if (!vertices || !faces || !vend || !tend || !n_faces || !pos || !nonfinite || !face)
    return MESH_NULL("rfd_simplify_init");
  const unsigned grid = blocks_of(V > F ? V : F, SIM_THREADS);
  if (v_is_f32)
    init_kernel<float><<<grid, SIM_THREADS, 0, (hipStream_t)stream>>>(V, F, K, vertices, faces, vend, tend, n_faces, pos,
                                                                      nonfinite, face);
  else
    init_kernel<double><<<grid, SIM_THREADS, 0, (hipStream_t)stream>>>(V, F, K, vertices, faces, vend, tend, n_faces, pos,
                                                                       nonfinite, face);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_simplify_quadrics(int V, int F, const double *pos, const int *face, const int *rowptr, const int *col,
                                  double *Q, void *stream) {
  if (int rc = check_sizes("rfd_simplify_quadrics: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (!pos || !face || !rowptr || !col || !Q) return MESH_NULL("rfd_simplify_quadrics");
  quadrics_kernel<<<blocks_of(V, SIM_THREADS), SIM_THREADS, 0, (hipStream_t)stream>>>(V, F, pos, face, rowptr, col, Q);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_simplify_edges(int V, int F, const long long *skey, const int *horder, const int *face, int *ea, int *eb,
                               int *eface, int *eapex, unsigned char *efrozen, unsigned char *vfrozen, void *stream) {
  if (int rc = check_sizes("rfd_simplify_edges: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (!skey || !horder || !face || !ea || !eb || !eface || !eapex || !efrozen || !vfrozen)
    return MESH_NULL("rfd_simplify_edges");
  edges_kernel<<<blocks_of(3l * F, SIM_THREADS), SIM_THREADS, 0, (hipStream_t)stream>>>(V, F, skey, horder, face, ea, eb,
                                                                                        eface, eapex, efrozen, vfrozen);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_simplify_edge_costs(int V, int F, int K, const int *vend, const int *ea, const int *eb, const int *eapex,
                                    const unsigned char *efrozen, const unsigned char *vfrozen, const int *face,
                                    const double *pos, const double *Q, const int *rowptr, const int *col, double *cost,
                                    double *epos, unsigned char *legal, int *emesh, void *stream) {
  if (int rc = check_sizes("rfd_simplify_edge_costs: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (K <= 0) return rfd_invalid("rfd_simplify_edge_costs: K must be positive");
  if (!vend || !ea || !eb || !eapex || !efrozen || !vfrozen || !face || !pos || !Q || !rowptr || !col || !cost || !epos ||
      !legal || !emesh)
    return MESH_NULL("rfd_simplify_edge_costs");
  edge_costs_kernel<<<blocks_of(3l * F, SIM_THREADS), SIM_THREADS, 0, (hipStream_t)stream>>>(
      V, F, K, vend, ea, eb, eapex, efrozen, vfrozen, face, pos, Q, rowptr, col, cost, epos, legal, emesh);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_simplify_vertex_min(int V, int F, int pass, const int *ea, const int *eb, const unsigned char *legal,
                                    const int *rank, const int *other, int *vmin, void *stream) {
  if (int rc = check_sizes("rfd_simplify_vertex_min: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (pass != 0 && pass != 1) return rfd_invalid("rfd_simplify_vertex_min: pass is 0 or 1");
  if (!ea || !eb || !vmin || (pass == 0 && (!legal || !rank)) || (pass == 1 && !other))
    return MESH_NULL("rfd_simplify_vertex_min");
  vertex_min_kernel<<<blocks_of(3l * F, SIM_THREADS), SIM_THREADS, 0, (hipStream_t)stream>>>(V, F, pass, ea, eb, legal,
                                                                                             rank, other, vmin);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_simplify_select(int V, int F, const int *ea, const int *eb, const unsigned char *legal, const int *rank,
                                const int *m2, unsigned char *sel, void *stream) {
  if (int rc = check_sizes("rfd_simplify_select: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (!ea || !eb || !legal || !rank || !m2 || !sel) return MESH_NULL("rfd_simplify_select");
  select_kernel<<<blocks_of(3l * F, SIM_THREADS), SIM_THREADS, 0, (hipStream_t)stream>>>(V, F, ea, eb, legal, rank, m2,
                                                                                         sel);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_simplify_apply(int V, int F, const unsigned char *keep, const int *ea, const int *eb, const int *eface,
                               const double *epos, const int *rowptr, const int *col, double *pos, double *Q, int *face,
                               void *stream) {
  if (int rc = check_sizes("rfd_simplify_apply: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (!keep || !ea || !eb || !eface || !epos || !rowptr || !col || !pos || !Q || !face) return MESH_NULL("rfd_simplify_apply");
  apply_kernel<<<blocks_of(3l * F, SIM_THREADS), SIM_THREADS, 0, (hipStream_t)stream>>>(V, F, keep, ea, eb, eface, epos,
                                                                                        rowptr, col, pos, Q, face);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_simplify_compact_faces(int V, int F, int K, const int *faces, const int *face, const int *vend,
                                       const int *tend, const unsigned char *takes_part, const unsigned char *keep,
                                       const int *fincl, const int *vincl, const int *vend2, int *f2, void *stream) {
  if (int rc = check_sizes("rfd_simplify_compact_faces: V > 0 and 0 < 3 F < 2^31", V, F)) return rc;
  if (K <= 0) return rfd_invalid("rfd_simplify_compact_faces: K must be positive");
  if (!faces || !face || !vend || !tend || !takes_part || !keep || !fincl || !vincl || !vend2 || !f2)
    return MESH_NULL("rfd_simplify_compact_faces");
  compact_faces_kernel<SIM_THREADS><<<blocks_of(F, SIM_THREADS), SIM_THREADS, 0, (hipStream_t)stream>>>(
      F, K, V, face, tend, takes_part, faces, keep, fincl, vincl, vend2, f2);                       // S7
  RFD_CHECK_LAUNCH();
  return 0;
}
