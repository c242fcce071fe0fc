// mesh_decimate.hip -- vertex clustering with a quadric-placed representative per cell (include/rfd_decimate.h), gfx950.
//
// The five rules are written out in the header and restated in tests/decimate_f64.py; every f64 expression below is
// evaluated as written (the library is built with -ffp-contract=off), so a cell index is the numpy one bit for bit and a
// position differs from it by the last place of a quotient or a root at most.  The grouping between the kernels (stable
// sorts, unique, prefix sums) is the host module's; what is here is one thread per vertex / face / run, and for the hot
// kernel sixteen lanes per cell: lane j adds the cell's corners j, j + 16, ... in order and a halving tree of wave
// shuffles adds the sixteen partial sums, the same shape at every grid size and in every batch.  No atomics at all.
// The mesh of an item, the f64 helpers and rule 5's kernel are mesh_batch.h's, shared with mesh_simplify.hip.
#include "mesh_batch.h"
#include "../../include/rfd_decimate.h"

namespace {

constexpr int DEC_THREADS = 256;
constexpr int CELL_LANES = 16;                         // partial sums of a cell (rule 3)
constexpr int CELLS_PER_BLOCK = DEC_THREADS / CELL_LANES;
constexpr int MAX_CELLS = 1290;                        // 1290^3 < 2^31 <= 1291^3

// rule 1: clamp(floor((x - lo) * inv_h), 0, cells - 1), decided in f64 before the conversion to an integer
__device__ __forceinline__ int cell_index(double x, double lo, double inv_h, int cells) {
  const double t = floor((x - lo) * inv_h);
  return (int)fmin(fmax(t, 0.0), (double)(cells - 1));
}

template <typename T>
__global__ __launch_bounds__(DEC_THREADS) void vertex_keys_kernel(int V, int K, int cells, const void *__restrict__ vertices,
                                                                  const int *__restrict__ vend,
                                                                  const double *__restrict__ lo,
                                                                  const double *__restrict__ inv_h, int *__restrict__ key) {
  const long i = (long)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (i >= V) return;
  const int k = segment_of(vend, K, (int)i);
  const D3 p = ld3<T>(vertices, (size_t)i);
  int out = K * cells * cells * cells;               // no cell
  if (finite_f64(p.x) && finite_f64(p.y) && finite_f64(p.z)) {
    const double ih = inv_h[k];
    const int ix = cell_index(p.x, lo[3 * k], ih, cells), iy = cell_index(p.y, lo[3 * k + 1], ih, cells),
              iz = cell_index(p.z, lo[3 * k + 2], ih, cells);
    out = k * cells * cells * cells + (iz * cells + iy) * cells + ix;
  }
  key[i] = out;
}

// rule 4, first half: one thread per face
__global__ __launch_bounds__(DEC_THREADS) void face_remap_kernel(int F, int K, int C, const int *__restrict__ faces,
                                                                 const int *__restrict__ tend, const int *__restrict__ vend,
                                                                 const int *__restrict__ vcell, int *__restrict__ fcell,
                                                                 long long *__restrict__ pair, int *__restrict__ top,
                                                                 unsigned char *__restrict__ alive) {
  const long f = (long)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (f >= F) return;
  const int k = segment_of(tend, K, (int)f);
  const int v0 = vend[k], nv = vend[k + 1] - v0;
  const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  int a = -1, b = -1, c = -1;
  if ((unsigned)ia < (unsigned)nv && (unsigned)ib < (unsigned)nv && (unsigned)ic < (unsigned)nv) {
    a = vcell[v0 + ia], b = vcell[v0 + ib], c = vcell[v0 + ic];
    if (a >= C) a = -1;                                // the host's table holds -1 .. C-1; nothing else leaves here
    if (b >= C) b = -1;
    if (c >= C) c = -1;
  }
  fcell[3 * f] = a, fcell[3 * f + 1] = b, fcell[3 * f + 2] = c;
  const bool ok = a >= 0 && b >= 0 && c >= 0 && a != b && b != c && a != c;
  const int lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = (int)(((long)a + b + c) - lo - hi);
  pair[f] = ok ? (long long)lo * C + mid : 0;
  top[f] = ok ? hi : 0;
  alive[f] = ok ? 1 : 0;
}

// rule 4, second half: the thread at the head of a run of equal candidate sets counts the run
__global__ __launch_bounds__(DEC_THREADS) void parity_kernel(int n, int C, int F, const long long *__restrict__ s_pair,
                                                             const int *__restrict__ s_top, const int *__restrict__ s_face,
                                                             const int *__restrict__ fcell, unsigned char *__restrict__ keep,
                                                             int *__restrict__ used) {
  const long i = (long)blockIdx.x * DEC_THREADS + threadIdx.x;
  if (i >= n) return;
  const long long p = s_pair[i];
  const int t = s_top[i];
  if (i > 0 && s_pair[i - 1] == p && s_top[i - 1] == t) return;
  long run = 1;
  while (i + run < n && s_pair[i + run] == p && s_top[i + run] == t) ++run;
  if (!(run & 1)) return;
  const int f = s_face[i];
  if ((unsigned)f >= (unsigned)F) return;
  keep[f] = 1;
  for (int c = 0; c < 3; ++c) {
    const int cell = fcell[3 * (long)f + c];
    if ((unsigned)cell < (unsigned)C) used[cell] = 1;  // several runs may name a cell: they all store the same word
  }
}

constexpr int N_SUMS = 13;                             // Axx Axy Axz Ayy Ayz Azz, bx by bz, W, sx sy sz

// rule 3: CELL_LANES lanes per cell
template <typename T>
__global__ __launch_bounds__(DEC_THREADS) void cell_solve_kernel(
    int C, int K, int F, int cells, const void *__restrict__ vertices, const int *__restrict__ faces,
    const int *__restrict__ vend, const int *__restrict__ cellkey, const int *__restrict__ rowptr,
    const int *__restrict__ col, const int *__restrict__ dst, const double *__restrict__ lo, const double *__restrict__ h,
    double regularise, float *__restrict__ out) {
  const int lane = threadIdx.x % CELL_LANES;
  const long cell = (long)blockIdx.x * CELLS_PER_BLOCK + threadIdx.x / CELL_LANES;
  int row = -1, begin = 0, end = 0, v0 = 0, nv = 0;
  D3 g = {0.0, 0.0, 0.0};
  double hk = 0.0;
  if (cell < C) {
    row = dst[cell];
    const int key = cellkey[cell], per = cells * cells * cells;
    const int k = key / per;
    if (row >= 0 && key >= 0 && k < K) {
      const int r = key - k * per;
      const int ix = r % cells, iy = (r / cells) % cells, iz = r / (cells * cells);
      hk = h[k];
      g = {lo[3 * k] + ((double)ix + 0.5) * hk, lo[3 * k + 1] + ((double)iy + 0.5) * hk,
           lo[3 * k + 2] + ((double)iz + 0.5) * hk};
      v0 = vend[k], nv = vend[k + 1] - v0;
      begin = max(rowptr[cell], 0), end = min(rowptr[cell + 1], 3 * F);     // col has 3 F entries
    } else {
      row = -1;
    }
  }
  double acc[N_SUMS];
#pragma unroll
  for (int t = 0; t < N_SUMS; ++t) acc[t] = 0.0;
  for (int at = begin + lane; at < end; at += CELL_LANES) {
    const int corner = col[at];
    if ((unsigned)corner >= 3u * (unsigned)F) continue;
    const int f = corner / 3, c = corner - 3 * f;
    const int i0 = faces[3 * (long)f], i1 = faces[3 * (long)f + 1], i2 = faces[3 * (long)f + 2];
    if ((unsigned)i0 >= (unsigned)nv || (unsigned)i1 >= (unsigned)nv || (unsigned)i2 >= (unsigned)nv) continue;
    const D3 p0 = ld3<T>(vertices, (size_t)(v0 + i0)), p1 = ld3<T>(vertices, (size_t)(v0 + i1)),
             p2 = ld3<T>(vertices, (size_t)(v0 + i2));
    const auto [m, w, usable] = face_plane(p0, p1, p2);
    if (!usable) continue;
    const double d = -dot(m, sub(p0, g));
    const double wx = w * m.x, wy = w * m.y, wz = w * m.z, wd = -(w * d);
    acc[0] = acc[0] + wx * m.x;
    acc[1] = acc[1] + wx * m.y;
    acc[2] = acc[2] + wx * m.z;
    acc[3] = acc[3] + wy * m.y;
    acc[4] = acc[4] + wy * m.z;
    acc[5] = acc[5] + wz * m.z;
    acc[6] = acc[6] + wd * m.x;
    acc[7] = acc[7] + wd * m.y;
    acc[8] = acc[8] + wd * m.z;
    acc[9] = acc[9] + w;
    const D3 q = sub(c == 0 ? p0 : c == 1 ? p1 : p2, g);
    acc[10] = acc[10] + w * q.x;
    acc[11] = acc[11] + w * q.y;
    acc[12] = acc[12] + w * q.z;
  }
  // 16 -> 8 -> 4 -> 2 -> 1: lane j takes lane j + step of its own group of sixteen (what the upper lanes fetch is unused)
#pragma unroll
  for (int step = CELL_LANES / 2; step >= 1; step >>= 1) {
#pragma unroll
    for (int t = 0; t < N_SUMS; ++t) acc[t] = acc[t] + __shfl_down(acc[t], step, CELL_LANES);
  }
  if (lane != 0 || row < 0) return;
  double y[3] = {0.0, 0.0, 0.0};
  const double W = acc[9];
  if (W != 0.0) {
    const double l = regularise * W;
    const double axx = acc[0] + l, axy = acc[1], axz = acc[2], ayy = acc[3] + l, ayz = acc[4], azz = acc[5] + l;
    const double bx = acc[6] + l * (acc[10] / W), by = acc[7] + l * (acc[11] / W), bz = acc[8] + l * (acc[12] / W);
    const D3 s = solve(adjugate(axx, axy, axz, ayy, ayz, azz), bx, by, bz);
    y[0] = s.x, y[1] = s.y, y[2] = s.z;
  }
  const double half = 0.5 * hk;
  const double centre[3] = {g.x, g.y, g.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double ya = finite_f64(y[a]) ? y[a] : 0.0;
    ya = fmin(fmax(ya, -half), half);
    out[3 * (long)row + a] = (float)(centre[a] + ya);
  }
}

int check_batch(int n, int K, int cells) {
  if (n <= 0 || K <= 0) return rfd_invalid("decimate: counts must be positive");
  if (cells < 1 || cells > MAX_CELLS || (long long)K * cells * cells * cells >= (1ll << 31))
    return rfd_invalid("decimate: cells >= 1 and K cells^3 < 2^31");
  return 0;
}

}  // namespace

RFD_API int rfd_decimate_vertex_keys(int V, int K, int cells, int v_is_f32, const void *vertices, const int *vend,
                                     const double *lo, const double *inv_h, int *key, void *stream) {
  if (int rc = check_batch(V, K, cells)) return rc;
  if (!vertices || !vend || !lo || !inv_h || !key) return MESH_NULL("rfd_decimate_vertex_keys");
  if (v_is_f32)
    vertex_keys_kernel<float><<<blocks_of(V, DEC_THREADS), DEC_THREADS, 0, (hipStream_t)stream>>>(
        V, K, cells, vertices, vend, lo, inv_h, key);
  else
    vertex_keys_kernel<double><<<blocks_of(V, DEC_THREADS), DEC_THREADS, 0, (hipStream_t)stream>>>(
        V, K, cells, vertices, vend, lo, inv_h, key);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_decimate_face_remap(int F, int K, int C, const int *faces, const int *tend, const int *vend,
                                    const int *vcell, int *fcell, long long *pair, int *top, unsigned char *alive,
                                    void *stream) {
  if (F <= 0 || K <= 0 || C <= 0) return rfd_invalid("rfd_decimate_face_remap: counts must be positive");
  if (!faces || !tend || !vend || !vcell || !fcell || !pair || !top || !alive)
    return MESH_NULL("rfd_decimate_face_remap");
  face_remap_kernel<<<blocks_of(F, DEC_THREADS), DEC_THREADS, 0, (hipStream_t)stream>>>(F, K, C, faces, tend, vend, vcell,
                                                                                        fcell, pair, top, alive);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_decimate_parity(int n, int C, int F, const long long *s_pair, const int *s_top, const int *s_face,
                                const int *fcell, unsigned char *keep, int *used, void *stream) {
  if (n <= 0 || C <= 0 || F <= 0) return rfd_invalid("rfd_decimate_parity: counts must be positive");
  if (!s_pair || !s_top || !s_face || !fcell || !keep || !used) return MESH_NULL("rfd_decimate_parity");
  parity_kernel<<<blocks_of(n, DEC_THREADS), DEC_THREADS, 0, (hipStream_t)stream>>>(n, C, F, s_pair, s_top, s_face, fcell,
                                                                                    keep, used);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_decimate_cell_solve(int C, int K, int F, int cells, int v_is_f32, const void *vertices, const int *faces,
                                    const int *vend, const int *cellkey, const int *rowptr, const int *col,
                                    const int *dst, const double *lo, const double *h, double regularise, float *out,
                                    void *stream) {
  if (int rc = check_batch(C, K, cells)) return rc;
  if (F <= 0 || (long)F * 3 > INT_MAX) return rfd_invalid("rfd_decimate_cell_solve: 0 < 3 F < 2^31");
  if (!(regularise >= 0.0)) return rfd_invalid("rfd_decimate_cell_solve: regularise must be >= 0");
  if (!vertices || !faces || !vend || !cellkey || !rowptr || !col || !dst || !lo || !h || !out)
    return MESH_NULL("rfd_decimate_cell_solve");
  const unsigned grid = blocks_of(C, CELLS_PER_BLOCK);
  if (v_is_f32)
    cell_solve_kernel<float><<<grid, DEC_THREADS, 0, (hipStream_t)stream>>>(C, K, F, cells, vertices, faces, vend, cellkey,
                                                                            rowptr, col, dst, lo, h, regularise, out);
  else
    cell_solve_kernel<double><<<grid, DEC_THREADS, 0, (hipStream_t)stream>>>(C, K, F, cells, vertices, faces, vend, cellkey,
                                                                             rowptr, col, dst, lo, h, regularise, out);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_decimate_compact_faces(int F, int K, const int *tend, const int *fcell, const unsigned char *keep,
                                       const int *fincl, const int *vincl, const int *vend2, int *f2, void *stream) {
  if (F <= 0 || K <= 0) return rfd_invalid("rfd_decimate_compact_faces: counts must be positive");
  if (!tend || !fcell || !keep || !fincl || !vincl || !vend2 || !f2)
    return MESH_NULL("rfd_decimate_compact_faces");
  // rule 5.  The entry has no cell count to check fcell against: what face_remap_kernel left there is -1 .. C - 1, so
  // the sign is the check that matters
  compact_faces_kernel<DEC_THREADS><<<blocks_of(F, DEC_THREADS), DEC_THREADS, 0, (hipStream_t)stream>>>(
      F, K, INT_MAX, fcell, tend, nullptr, nullptr, keep, fincl, vincl, vend2, f2);
  RFD_CHECK_LAUNCH();
  return 0;
}
