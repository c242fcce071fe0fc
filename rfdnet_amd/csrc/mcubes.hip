// mcubes.hip -- batched marching cubes on padded occupancy grids (gfx950).
//
// Replaces the per-proposal CPU call `mcubes.marching_cubes(np.pad(occ_hat, 1,
// constant_values=-1e6), threshold)` of Generator3D.extract_mesh
// (models/iscnet/modules/generator.py:157-161).  PyMCubes 0.1.2 is a
// third-party dependency that is not vendored in the reference: its published
// algorithm (table-driven marching cubes, one shared vertex per crossed lattice
// edge placed by linear interpolation, indexed triangles) is restated, and its
// OUTPUT CONVENTIONS are read back from the meshes the reference ships under
// demo/outputs/ (tests/golden/F_MC.npz, tests/test_mcubes_golden.py): the case
// table (tools/gen_mc_tables.py), triangles in x-major cell order and table order,
// vertices numbered by (high end point of their edge in x-major order, axis).
// Given a grid this kernel emits the same vertex and face arrays as the library
// (faces identical, vertices to double rounding).  Not observable in those meshes
// and therefore an assumption: a value EXACTLY equal to the iso level counts as
// below it (`<=`).
//
// All K proposals are processed by the same launches; the -1e6 padding shell is
// virtual (never materialised).  Three passes over K*D^3 lattice points
// (D = n + 2), workgroup = a run of MC_RUN consecutive points of one proposal.
// The only per-point state kept in HBM is ONE byte -- the cube index of the cell whose FAR
// corner (corner 6) is the point; a point owns the vertices of the three edges that END in it,
// see above -- plus a sparse int32 vertex base for points that own a vertex; prefix sums are
// two-level (per-workgroup sums -> tiny scan by the caller -> in-workgroup scan recomputed
// where needed), so no dense int32 count / scan arrays are written or read:
//   classify : point -> code byte; workgroup -> (#vertices, #triangles)
//   vertices : one vertex per crossed edge, index = workgroup base + in-workgroup scan;
//              leaves that index in vbase[point] for the triangle pass
//   triangles: table lookup, vertex index via the owner point's vbase
// HBM traffic per point: 4 B of grid + 1 B written (classify), 1 B read twice (emit),
// vs 4 + 9 written, 2 x 16 for scans / differences and 13 read in the dense-array version.
// Vertex coordinates are in padded-grid index space (grid point i of the
// original grid sits at i + 1), double precision like the reference's float64
// grid.
#include "common.h"
#include "mc_tables.h"

namespace {

__constant__ signed char c_ntri[256];
__constant__ signed char c_tri[256][3 * MC_MAX_TRIS];
__constant__ signed char c_owner[12][4];
bool g_tables_uploaded[64] = {false};

constexpr int MC_BLOCK = 256;
constexpr int MC_PTS = 4;                    // consecutive lattice points per thread
constexpr int MC_RUN = MC_BLOCK * MC_PTS;     // points per workgroup = unit of the two-level scan

// Largest float <= iso: for a float v, ((double)v <= iso) == (v <= float_floor(iso)).
__device__ __forceinline__ float float_floor(double iso) {
  float t = (float)iso;
  if ((double)t > iso) {
    if (t == 0.f) t = -0.f;  // step from +0 to the largest negative subnormal below
    t = __uint_as_float(__float_as_uint(t) + (t > 0.f ? -1 : 1));
  }
  return t;
}

struct GridView {
  const float *g;  // [n][n][n] of this proposal
  int n, D;
  float pad;
  // branch-free: clamp the address, select the padding value afterwards (lets the compiler
  // issue all corner loads of a thread back to back)
  __device__ __forceinline__ float at(int i, int j, int k) const {
    const bool in = i > 0 && j > 0 && k > 0 && i < D - 1 && j < D - 1 && k < D - 1;
    const int ci = min(max(i - 1, 0), n - 1), cj = min(max(j - 1, 0), n - 1),
              ck = min(max(k - 1, 0), n - 1);
    float v = g[(unsigned)((ci * n + cj) * n + ck)];
    asm("" : "+v"(v));  // keep the load unconditional (else it is sunk under a branch on `in`)
    return in ? v : pad;
  }
};

struct Point {
  int i, j, k;
  __device__ __forceinline__ Point(unsigned e, unsigned D) {
    const unsigned r = e / D;
    k = (int)(e - r * D);
    i = (int)(r / D);
    j = (int)(r - (unsigned)i * D);
  }
};

// Exclusive scan of x over the workgroup (MC_BLOCK threads); *total = sum over the workgroup.
__device__ __forceinline__ int block_scan(int x, int *total) {
  __shared__ int wsum[MC_BLOCK / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = x;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(inc, d);
    if (lane >= d) inc += y;
  }
  __syncthreads();  // wsum may still be read by a previous call
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int q = 0; q < MC_BLOCK / 64; ++q) {
    if (q < w) off += wsum[q];
    tot += wsum[q];
  }
  *total = tot;
  return off + inc - x;
}

// crossed edges ENDING in the cell's far corner (x: edge 6 = corners 7-6, y: edge 5 = 5-6,
// z: edge 10 = 2-6), from the cube index
__device__ __forceinline__ unsigned edge_bits(unsigned ci) {
  const unsigned c6 = ci >> 6;
  return (((ci >> 7) ^ c6) & 1u) | ((((ci >> 5) ^ c6) & 1u) << 1) | ((((ci >> 2) ^ c6) & 1u) << 2);
}

// code[point] = cube index of the cell whose FAR corner is the point, over the padded lattice
// extended by one more virtual padding layer (cells hanging over the near faces see only
// padding: index 255, no triangles, no edges -- the same result as "no such cell").
// A workgroup owns a run of MC_RUN consecutive points, four per thread: the 32 corner loads
// of a thread are independent and the per-run scan covers 4x the points (these passes were
// bound by workgroup latency x rounds, not by bandwidth).  In the emit kernels thread t owns
// the points 4t .. 4t+3 so that the scan order is the point order.
__global__ __launch_bounds__(MC_BLOCK) void mc_classify_kernel(
    int n, float pad, double iso, const float *__restrict__ grids,
    unsigned char *__restrict__ code, int *__restrict__ vsum, int *__restrict__ tsum) {
  const int D = n + 2;
  const unsigned per = (unsigned)D * D * D;
  const int kp = blockIdx.y;
  const float thr = float_floor(iso);
  // only the run TOTALS are needed here, so lanes take consecutive points (coalesced loads)
  const unsigned e = blockIdx.x * MC_RUN + threadIdx.x;
  GridView G{grids + (size_t)kp * n * n * n, n, D, pad};
  // Bourke corner numbering
  const int cx[8] = {0, 1, 1, 0, 0, 1, 1, 0}, cy[8] = {0, 0, 1, 1, 0, 0, 1, 1},
            cz[8] = {0, 0, 0, 0, 1, 1, 1, 1};
  int cnt = 0;
#pragma unroll
  for (int p = 0; p < MC_PTS; ++p) {
    const unsigned ep = e + p * MC_BLOCK;
    if (ep < per) {
      const Point P(ep, D);
      float v[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = G.at(P.i - 1 + cx[c], P.j - 1 + cy[c], P.k - 1 + cz[c]);
      unsigned ci = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) ci |= (v[c] <= thr ? 1u : 0u) << c;
      code[(size_t)kp * per + ep] = (unsigned char)ci;
      cnt += __popc(edge_bits(ci)) | ((int)c_ntri[ci] << 16);
    }
  }
  // per-run totals: vertices in the low half, triangles in the high half (<= 3072 / 5120)
  int total;
  block_scan(cnt, &total);
  if (threadIdx.x == 0) {
    vsum[(size_t)kp * gridDim.x + blockIdx.x] = total & 0xffff;
    tsum[(size_t)kp * gridDim.x + blockIdx.x] = total >> 16;
  }
}

// Phase 1 (thread per 4 points): scan the vertex counts, leave each owner's first vertex index
// in vbase and list the owners in LDS.  Phase 2 (thread per VERTEX): interpolate and store --
// the surface touches ~5 % of the points, so a thread-per-point emit leaves most lanes idle.
__global__ __launch_bounds__(MC_BLOCK) void mc_vertices_kernel(
    int n, float pad, double iso, const float *__restrict__ grids,
    const unsigned char *__restrict__ code, const int *__restrict__ vblock,
    int *__restrict__ vbase, double *__restrict__ verts, double va, double vc) {
  __shared__ unsigned short owner[MC_RUN * 3];
  __shared__ unsigned short first[MC_RUN];
  __shared__ unsigned char sbits[MC_RUN];
  const int D = n + 2;
  const unsigned per = (unsigned)D * D * D;
  const int kp = blockIdx.y;
  const unsigned e0 = blockIdx.x * MC_RUN, e = e0 + threadIdx.x * MC_PTS;
  unsigned bits[MC_PTS];
  int mine = 0;
#pragma unroll
  for (int p = 0; p < MC_PTS; ++p) {
    bits[p] = e + p < per ? edge_bits(code[(size_t)kp * per + e + p]) : 0u;
    mine += __popc(bits[p]);
  }
  int total;
  int off = block_scan(mine, &total);
  if (total == 0) return;
  const int base = vblock[(size_t)kp * gridDim.x + blockIdx.x];
#pragma unroll
  for (int p = 0; p < MC_PTS; ++p) {
    const int c = threadIdx.x * MC_PTS + p;
    first[c] = (unsigned short)off;
    sbits[c] = (unsigned char)bits[p];
    if (bits[p]) {
      vbase[(size_t)kp * per + e + p] = base + off;
      for (int q = 0; q < __popc(bits[p]); ++q) owner[off + q] = (unsigned short)c;
      off += __popc(bits[p]);
    }
  }
  __syncthreads();
  GridView G{grids + (size_t)kp * n * n * n, n, D, pad};
  for (int t = threadIdx.x; t < total; t += MC_BLOCK) {
    const int c = owner[t];
    int q = t - first[c];
    unsigned b = sbits[c];
    while (q--) b &= b - 1;          // drop the q lowest crossed edges
    const int a = __ffs(b) - 1;      // axis of this vertex
    const Point P(e0 + c, D);
    const double fhi = (double)G.at(P.i, P.j, P.k);
    const double flo = (double)G.at(P.i - (a == 0), P.j - (a == 1), P.k - (a == 2));
    // the library's interpolation, `(x2 - x1) * (iso - f1) / (f2 - f1) + x1`, walks the x edge
    // from its high end (edge 6 = corners 6 -> 7) and the y / z edges from their low end
    // (edges 5 and 10 = corners 5 -> 6, 2 -> 6); equal up to the last bit of a double
    const double xhi = (double)(a == 0 ? P.i : a == 1 ? P.j : P.k), xlo = xhi - 1.0;
    const double x1 = a == 0 ? xhi : xlo, x2 = a == 0 ? xlo : xhi;
    const double f1 = a == 0 ? fhi : flo, f2 = a == 0 ? flo : fhi;
    const double x = (f2 == f1) ? (x2 + x1) / 2 : (x2 - x1) * (iso - f1) / (f2 - f1) + x1;
    double *o = verts + (size_t)(base + t) * 3;
    // stored coordinate = va * (padded-grid index coordinate) + vc, ONE rounding (va = 1, vc = 0: the library's plain
    // output; Generator3D.extract_mesh's four steps of generator.py:163-168 collapse to one such map)
    o[0] = __builtin_fma(va, a == 0 ? x : (double)P.i, vc);
    o[1] = __builtin_fma(va, a == 1 ? x : (double)P.j, vc);
    o[2] = __builtin_fma(va, a == 2 ? x : (double)P.k, vc);
  }
}

// Same two phases for the triangles (thread per TRIANGLE in phase 2).
__global__ __launch_bounds__(MC_BLOCK) void mc_triangles_kernel(
    int n, const unsigned char *__restrict__ code, const int *__restrict__ vblock,
    const int *__restrict__ tblock, const int *__restrict__ vbase, int *__restrict__ tris) {
  __shared__ unsigned short owner[MC_RUN * MC_MAX_TRIS];
  __shared__ unsigned short first[MC_RUN];
  __shared__ unsigned char sci[MC_RUN];
  const int D = n + 2;
  const unsigned per = (unsigned)D * D * D;
  const int kp = blockIdx.y;
  const unsigned char *pc = code + (size_t)kp * per;
  const unsigned e0 = blockIdx.x * MC_RUN, e = e0 + threadIdx.x * MC_PTS;
  unsigned ci[MC_PTS];
  int mine = 0;
#pragma unroll
  for (int p = 0; p < MC_PTS; ++p) {
    ci[p] = e + p < per ? pc[e + p] : 255u;
    mine += c_ntri[ci[p]];
  }
  int total;
  int off = block_scan(mine, &total);
  if (total == 0) return;
#pragma unroll
  for (int p = 0; p < MC_PTS; ++p) {
    const int c = threadIdx.x * MC_PTS + p;
    const int nt = c_ntri[ci[p]];
    first[c] = (unsigned short)off;
    sci[c] = (unsigned char)ci[p];
    for (int q = 0; q < nt; ++q) owner[off + q] = (unsigned short)c;
    off += nt;
  }
  __syncthreads();
  const int base = tblock[(size_t)kp * gridDim.x + blockIdx.x];
  const int v0 = vblock[(size_t)kp * gridDim.x];  // first vertex of this proposal
  const int *pv = vbase + (size_t)kp * per;
  for (int t = threadIdx.x; t < total; t += MC_BLOCK) {
    const int c = owner[t];
    const int q = t - first[c];
    const unsigned cc = sci[c];
    const unsigned ec = e0 + c;
    int idx[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int ed = c_tri[cc][3 * q + r];
      const unsigned op = (unsigned)((int)ec + (c_owner[ed][0] * D + c_owner[ed][1]) * D + c_owner[ed][2]);
      const unsigned ob = edge_bits(pc[op]);
      const int axis = c_owner[ed][3];
      idx[r] = pv[op] + __popc(ob & ((1u << axis) - 1u)) - v0;
    }
    int *o = tris + (size_t)(base + t) * 3;
    o[0] = idx[0];
    o[1] = idx[1];
    o[2] = idx[2];
  }
}

int upload_tables() {
  int dev = 0;
  RFD_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || g_tables_uploaded[dev]) return 0;
  RFD_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_ntri), MC_NTRI, sizeof(MC_NTRI)));
  RFD_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_tri), MC_TRI, sizeof(MC_TRI)));
  RFD_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_owner), MC_EDGE_OWNER, sizeof(MC_EDGE_OWNER)));
  g_tables_uploaded[dev] = true;
  return 0;
}

}  // namespace

RFD_API int rfd_mc_blocks(int n) {
  const size_t per = (size_t)(n + 2) * (n + 2) * (n + 2);
  return (int)((per + MC_RUN - 1) / MC_RUN);
}

// grids [K][n][n][n] f32; code [K][D^3] u8 (D = n+2); vsum / tsum [K][rfd_mc_blocks(n)] i32
RFD_API int rfd_mc_classify(int K, int n, float pad_value, double iso, const float *grids,
                            unsigned char *code, int *vsum, int *tsum, void *stream) {
  if (K <= 0 || n <= 0) return 0;
  int rc = upload_tables();
  if (rc) return rc;
  hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)rfd_mc_blocks(n), K), dim3(MC_BLOCK), 0,
                     (hipStream_t)stream, n, pad_value, iso, grids, code, vsum, tsum);
  RFD_CHECK_LAUNCH();
  return 0;
}

// vblock / tblock: EXCLUSIVE prefix sums of vsum / tsum over the flattened [K][blocks]
// arrays.  vbase [K][D^3] i32 scratch (written where a point owns a vertex).  verts [NV][3]
// f64 (padded-grid index coordinates), tris [NT][3] i32 with vertex indices LOCAL to each
// proposal.
// rfd_mc_emit_affine: the stored vertices are va * v + vc (what a caller would otherwise do in a second pass over the
// 24 B / vertex buffer); va = 1, vc = 0 is the identity map.
RFD_API int rfd_mc_emit_affine(int K, int n, float pad_value, double iso, const float *grids,
                               const unsigned char *code, const int *vblock, const int *tblock,
                               int *vbase, double *verts, int *tris, double va, double vc, void *stream) {
  if (K <= 0 || n <= 0) return 0;
  int rc = upload_tables();
  if (rc) return rc;
  const dim3 grid((unsigned)rfd_mc_blocks(n), K);
  hipLaunchKernelGGL(mc_vertices_kernel, grid, dim3(MC_BLOCK), 0, (hipStream_t)stream, n,
                     pad_value, iso, grids, code, vblock, vbase, verts, va, vc);
  RFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(mc_triangles_kernel, grid, dim3(MC_BLOCK), 0, (hipStream_t)stream, n, code,
                     vblock, tblock, vbase, tris);
  RFD_CHECK_LAUNCH();
  return 0;
}
