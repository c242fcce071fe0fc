// mesh_refine.hip -- the small kernels of the batched mesh refinement (Generator3D.refine_mesh, generator.py:226-289), gfx950.
//
// The reference moves the vertices of ONE mesh by RMSprop on
//   mean_f (sigmoid(l(q_f)) - tau)^2 + 0.01 mean_f |nf_f - nt_f|^2,     q_f = a random point of face f,
//   nf = face normal, nt = -grad sigmoid(l)(q) / (|.| + 1e-10)
// and differentiates nt by autograd with create_graph.  The decoder is piecewise linear in q (fc_p, eval-mode CBN, ReLU, 1x1
// convolutions), so the Hessian of l is zero and the double backward needs the logit l (decoder kernels), its gradient g
// (csrc/occ_normals.hip) and the derivatives of the sigmoid only.  Per step, for ALL meshes of a scene at once:
//   refine_sample         q per face, written in the two layouts the two decoder kernels read
//   (decode, normals)     l and g, unchanged entry points
//   refine_face_backward  d loss / d (the face's three corners), [F][3][3]
//   refine_vertex_step    per vertex: sum of its corners' gradients in ascending (face, corner) order through a CSR built once
//                         by the host (no atomics: deterministic, independent of what else is in the launch), then RMSprop
// The terms of a corner gradient are fp32; their sum -- within the corner and over a vertex's corners -- is carried in f64 and
// rounded to fp32 once per vertex.  A zero-area face (i, i, j) is why: its normal term is ~1e10 times the value term and cancels
// EXACTLY between the two corners that name vertex i; in fp32 the value term (and every other face's share of that vertex) would
// be absorbed before the cancellation and the vertex would see a zero gradient where the float64 loop sees a step.
// A mesh is described by offsets: faces fend[k] .. fend[k+1]-1 (indices local to the mesh), vertices vend[k] .. vend[k+1]-1,
// decoder tiles tprefix[k] .. tprefix[k+1]-1 (128 query slots each; tprefix[k+1] - tprefix[k] >= ceil(faces / 128)).
// Everything else is fp32, one rounding per written operation (the library is built with -ffp-contract=off).
#include "mesh_batch.h"
#include "rfd_occ.h"

namespace {

constexpr float REFINE_EPS = 1e-10f;             // generator.py:267, :276

struct Face {
  int slot;           // decoder query slot
  int i0, i1, i2;     // global vertex indices
  int n_faces;        // of the mesh
  bool ok;            // indices inside the mesh's vertex range and the slot inside its tiles
};

__device__ __forceinline__ Face load_face(int f, int K, const int *__restrict__ faces, const int *__restrict__ fend,
                                          const int *__restrict__ vend, const int *__restrict__ tprefix) {
  Face fc;
  const int k = segment_of(fend, K, f);         // the mesh of face f
  const int f0 = fend[k], v0 = vend[k], nv = vend[k + 1] - v0;
  fc.n_faces = fend[k + 1] - f0;
  const int j = f - f0;                          // >= 0: segment_of chose k with fend[k] <= f
  const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
  fc.ok = (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv &&
          j < (tprefix[k + 1] - tprefix[k]) * RFD_OCC_TILE;
  fc.slot = tprefix[k] * RFD_OCC_TILE + j;
  fc.i0 = v0 + a;
  fc.i1 = v0 + b;
  fc.i2 = v0 + c;
  return fc;
}

struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 ld3(const float *__restrict__ p, size_t i) { return {p[i * 3], p[i * 3 + 1], p[i * 3 + 2]}; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 mul(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 divs(V3 a, float s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ void st3(float *__restrict__ p, size_t i, V3 a) {
  p[i * 3] = a.x;
  p[i * 3 + 1] = a.y;
  p[i * 3 + 2] = a.z;
}

// q = (e0 v0 + e1 v1) + e2 v2 per face: compact f64 [F][3] (what rfd_occ_normals_w8 reads, with fend as its per-mesh offsets)
// and f32 at the face's slot of the mesh's 128-point tiles (rfd_occ_decode_w8); a face with an index outside its mesh: zeros
__global__ __launch_bounds__(256) void refine_sample_kernel(int F, int K, const float *__restrict__ verts,
                                                           const int *__restrict__ faces, const int *__restrict__ fend,
                                                           const int *__restrict__ vend, const int *__restrict__ tprefix,
                                                           const float *__restrict__ eps, double *__restrict__ qd,
                                                           float *__restrict__ qt) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const Face fc = load_face(f, K, faces, fend, vend, tprefix);
  V3 q = {0.f, 0.f, 0.f};
  if (fc.ok) {
    const V3 e = ld3(eps, f);
    q = add(add(mul(e.x, ld3(verts, fc.i0)), mul(e.y, ld3(verts, fc.i1))), mul(e.z, ld3(verts, fc.i2)));
    st3(qt, fc.slot, q);
  }
  qd[(size_t)f * 3] = (double)q.x;
  qd[(size_t)f * 3 + 1] = (double)q.y;
  qd[(size_t)f * 3 + 2] = (double)q.z;
}

// d loss / d corners of every face, cg [F][3][3] f64 (the file header; DESIGN.md section 3 has the derivation)
__global__ __launch_bounds__(256) void refine_face_backward_kernel(
    int F, int K, const float *__restrict__ verts, const int *__restrict__ faces, const int *__restrict__ fend,
    const int *__restrict__ vend, const int *__restrict__ tprefix, const float *__restrict__ eps,
    const float *__restrict__ logits, const float *__restrict__ grad, float tau, double *__restrict__ cg) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  const Face fc = load_face(f, K, faces, fend, vend, tprefix);
  double *out = cg + (size_t)f * 9;
#pragma unroll
  for (int i = 0; i < 9; ++i) out[i] = 0.0;
  if (fc.ok) {
    const V3 p0 = ld3(verts, fc.i0), p1 = ld3(verts, fc.i1), p2 = ld3(verts, fc.i2);
    const V3 e = ld3(eps, f), g = ld3(grad, f);
    const float l = logits[fc.slot];
    const float nF = (float)fc.n_faces;
    // face normal nf = c / (|c| + eps)
    const V3 a = sub(p1, p0), b = sub(p2, p1), c = cross(a, b);
    const float r = __builtin_sqrtf(dot(c, c)), re = r + REFINE_EPS;
    const V3 nf = divs(c, re);
    // target normal nt = -s' g / (s' |g| + eps): the gradient of sigmoid(l) is s' g
    const float s = 1.f / (1.f + expf(-l));
    const float s1 = s * (1.f - s), s2 = s1 * (1.f - 2.f * s);
    const float m = s1 * __builtin_sqrtf(dot(g, g)) + REFINE_EPS;
    const V3 nt = divs(mul(-s1, g), m);
    const V3 d = sub(nf, nt);
    // through q: the value term, and nt's dependence on q through s' alone (g is locally constant)
    const float c2 = 0.02f / nF;
    const float coef = 2.f * (s - tau) * s1 / nF + c2 * dot(d, g) * s2 * (REFINE_EPS / (m * m));
    const V3 gq = mul(coef, g);
    // through the face normal: w = d loss / d c, the norm's derivative taken as 0 at c = 0 (as torch does)
    const V3 u = mul(c2, d);
    V3 w = divs(u, re);
    if (r > 0.f) w = add(w, mul(-dot(u, c) / (re * re), divs(c, r)));
    const V3 da = cross(b, w), db = cross(w, a);
    // G0 = e0 gq - da, G1 = e1 gq + da - db, G2 = e2 gq + db: fp32 terms, summed in f64
    const V3 q0 = mul(e.x, gq), q1 = mul(e.y, gq), q2 = mul(e.z, gq);
    const float t0[3] = {q0.x, q0.y, q0.z}, t1[3] = {q1.x, q1.y, q1.z}, t2[3] = {q2.x, q2.y, q2.z};
    const float fa[3] = {da.x, da.y, da.z}, fb[3] = {db.x, db.y, db.z};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      out[j] = (double)t0[j] - (double)fa[j];
      out[3 + j] = ((double)t1[j] + (double)fa[j]) - (double)fb[j];
      out[6 + j] = (double)t2[j] + (double)fb[j];
    }
  }
}

// per vertex: G = sum of cg[col[rowptr[v] .. rowptr[v+1]-1]] in that order, then torch.optim.RMSprop's defaults with
// lr = 1e-4 (generator.py:252): sq = 0.99 sq + 0.01 G^2, v -= 1e-4 G / (sqrt(sq) + 1e-8).  G = 0 leaves v bit-unchanged.
__global__ __launch_bounds__(256) void refine_vertex_step_kernel(int V, const int *__restrict__ rowptr,
                                                                const int *__restrict__ col, int n_corners,
                                                                const double *__restrict__ cg, float *__restrict__ verts,
                                                                float *__restrict__ sq, float *__restrict__ gout) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int b = rowptr[v], e = rowptr[v + 1];
  if (b < 0) b = 0;
  if (e > n_corners) e = n_corners;
  double gx = 0.0, gy = 0.0, gz = 0.0;
  for (int i = b; i < e; ++i) {
    const int cn = col[i];
    if ((unsigned)cn < (unsigned)n_corners) {
      gx += cg[(size_t)cn * 3];
      gy += cg[(size_t)cn * 3 + 1];
      gz += cg[(size_t)cn * 3 + 2];
    }
  }
  const float g3[3] = {(float)gx, (float)gy, (float)gz};
  if (gout) st3(gout, v, V3{g3[0], g3[1], g3[2]});
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const size_t i = (size_t)v * 3 + j;
    const float q = 0.99f * sq[i] + 0.01f * g3[j] * g3[j];
    sq[i] = q;
    verts[i] = verts[i] - 1e-4f * (g3[j] / (__builtin_sqrtf(q) + 1e-8f));
  }
}

// ---- Dirichlet(1/2, 1/2, 1/2) rows on the device: z_i^2 / sum z_j^2 of three standard normals (z^2 / 2 ~ Gamma(1/2)), the
// normals by Box-Muller from a counter-based hash of (seed, step, row): same distribution as np.random.dirichlet, not its stream
__device__ __forceinline__ unsigned long long mix64(unsigned long long x) {          // splitmix64's finaliser
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

__global__ __launch_bounds__(256) void refine_dirichlet_kernel(int n, unsigned long long seed, int step,
                                                              float *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = mix64(seed + 0x9e3779b97f4a7c15ull * (unsigned long long)(step + 1));
  const unsigned long long h0 = mix64(key ^ (0xd1b54a32d192ed03ull * (unsigned long long)(i + 1)));
  const unsigned long long h1 = mix64(h0 + 0x9e3779b97f4a7c15ull);
  const float k24 = 1.f / 16777216.f;
  const float ua = (float)((unsigned)(h0 >> 40) + 1u) * k24, ub = (float)((unsigned)(h0 >> 8) & 0xffffffu) * k24;    // (0, 1], [0, 1)
  const float uc = (float)((unsigned)(h1 >> 40) + 1u) * k24, ud = (float)((unsigned)(h1 >> 8) & 0xffffffu) * k24;
  const float ra = __builtin_sqrtf(-2.f * logf(ua)), rc = __builtin_sqrtf(-2.f * logf(uc));
  float sn, cs;
  sincospif(2.f * ub, &sn, &cs);
  const float z0 = ra * cs, z1 = ra * sn, z2 = rc * cospif(2.f * ud);
  const float a = z0 * z0, b = z1 * z1, c = z2 * z2;
  const float t = (a + b) + c;
  V3 e = {1.f / 3.f, 1.f / 3.f, 1.f / 3.f};
  if (t > 0.f) e = {a / t, b / t, c / t};
  st3(out, i, e);
}

}  // namespace

RFD_API int rfd_refine_sample(int F, int K, const float *verts, const int *faces, const int *fend, const int *vend,
                              const int *tprefix, const float *eps, double *qd, float *qt, void *stream) {
  if (F < 0 || K <= 0 || !verts || !faces || !fend || !vend || !tprefix || !eps || !qd || !qt)
    return rfd_invalid("rfd_refine_sample: arguments");
  if (F == 0) return 0;
  hipLaunchKernelGGL(refine_sample_kernel, dim3(ceil_div(F, 256)), dim3(256), 0, (hipStream_t)stream, F, K, verts, faces,
                     fend, vend, tprefix, eps, qd, qt);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_refine_face_backward(int F, int K, const float *verts, const int *faces, const int *fend, const int *vend,
                                     const int *tprefix, const float *eps, const float *logits, const float *grad,
                                     float tau, double *cg, void *stream) {
  if (F < 0 || K <= 0 || !verts || !faces || !fend || !vend || !tprefix || !eps || !logits || !grad || !cg)
    return rfd_invalid("rfd_refine_face_backward: arguments");
  if (F == 0) return 0;
  hipLaunchKernelGGL(refine_face_backward_kernel, dim3(ceil_div(F, 256)), dim3(256), 0, (hipStream_t)stream, F, K, verts,
                     faces, fend, vend, tprefix, eps, logits, grad, tau, cg);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_refine_vertex_step(int V, const int *rowptr, const int *col, int n_corners, const double *cg, float *verts,
                                   float *sq, float *gout, void *stream) {
  if (V < 0 || n_corners < 0 || !rowptr || !col || !cg || !verts || !sq)
    return rfd_invalid("rfd_refine_vertex_step: arguments");
  if (V == 0) return 0;
  hipLaunchKernelGGL(refine_vertex_step_kernel, dim3(ceil_div(V, 256)), dim3(256), 0, (hipStream_t)stream, V, rowptr, col,
                     n_corners, cg, verts, sq, gout);
  RFD_CHECK_LAUNCH();
  return 0;
}

RFD_API int rfd_refine_dirichlet(int n, unsigned long long seed, int step, float *out, void *stream) {
  if (n < 0 || step < 0 || !out) return rfd_invalid("rfd_refine_dirichlet: arguments");
  if (n == 0) return 0;
  hipLaunchKernelGGL(refine_dirichlet_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, n, seed, step, out);
  RFD_CHECK_LAUNCH();
  return 0;
}
