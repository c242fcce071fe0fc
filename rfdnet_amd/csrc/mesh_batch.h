// mesh_batch.h -- what the stages over a flat ragged mesh batch (v, f, vend, tend) share: mesh_decimate.hip and
// mesh_simplify.hip all of it, mesh_refine.hip (fp32, other operations) the segment search alone.
//
// Here: the mesh of a vertex or face, the f64 vector helpers, the plane of a face, the symmetric 3x3 adjugate solve, the
// face compaction both thinning stages end with, and the launchers' grid size and null-argument refusal.  NOT here: what a
// caller makes of a plane (decimate's thirteen sums are taken about the cell centre, simplify's ten are absolute, with
// opposite signs of the offset term) and the guards around a solve (they differ too).  Every f64 expression is evaluated as
// written (the library is built with -ffp-contract=off): the parenthesisation of dot() and the operand order of cross() are
// part of what the float64 restatements in tests/ are compared with bit for bit.
//
// The device functions are __forceinline__, as in split_f16.h, and everything is in an anonymous namespace: an including
// file compiles to what it would with its own copy of this text, and gets the kernel only if it launches it.
#pragma once
#include <limits.h>

#include "common.h"

namespace {

// the segment of item i: the last k with off[k] <= i (empty segments repeat an offset); 0 <= i < off[K]
__device__ __forceinline__ int segment_of(const int *__restrict__ off, int K, int i) {
  int lo = 0, hi = K;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool finite_f64(double v) { return (__double2hiint(v) & 0x7ff00000) != 0x7ff00000; }
__device__ __forceinline__ bool usable_length(double L) { return L != 0.0 && finite_f64(L); }

struct D3 {
  double x, y, z;
};
template <typename T>
__device__ __forceinline__ D3 ld3(const void *__restrict__ p, size_t i) {
  const T *q = static_cast<const T *>(p) + i * 3;
  return {(double)q[0], (double)q[1], (double)q[2]};
}
__device__ __forceinline__ D3 sub(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 u, D3 v) {
  return {u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
}

// the plane of face (p0, p1, p2): n = (p1 - p0) x (p2 - p0), unit normal m = n / |n|, weight w = |n| / 2 (the area);
// m and w mean nothing unless |n| is usable.  (Handing m and w back through references cost cell_solve_kernel 6 VGPRs.)
struct Plane {
  D3 m;
  double w;
  bool usable;
};
__device__ __forceinline__ Plane face_plane(D3 p0, D3 p1, D3 p2) {
  const D3 n = cross(sub(p1, p0), sub(p2, p0));
  const double L = sqrt(dot(n, n));
  return {{n.x / L, n.y / L, n.z / L}, 0.5 * L, usable_length(L)};
}

// the adjugate of the symmetric matrix (axx axy axz; axy ayy ayz; axz ayz azz) and its determinant; whether det can be
// divided by is the caller's question
struct Adjugate3 {
  double c00, c01, c02, c11, c12, c22, det;
};
__device__ __forceinline__ Adjugate3 adjugate(double axx, double axy, double axz, double ayy, double ayz, double azz) {
  Adjugate3 a;
  a.c00 = ayy * azz - ayz * ayz, a.c01 = axz * ayz - axy * azz, a.c02 = axy * ayz - axz * ayy;
  a.c11 = axx * azz - axz * axz, a.c12 = axy * axz - axx * ayz, a.c22 = axx * ayy - axy * axy;
  a.det = (axx * a.c00 + axy * a.c01) + axz * a.c02;
  return a;
}
// A^-1 r, row by row
__device__ __forceinline__ D3 solve(const Adjugate3 &a, double rx, double ry, double rz) {
  return {((a.c00 * rx + a.c01 * ry) + a.c02 * rz) / a.det, ((a.c01 * rx + a.c11 * ry) + a.c12 * rz) / a.det,
          ((a.c02 * rx + a.c12 * ry) + a.c22 * rz) / a.det};
}

// The last step of a thinning stage, one thread per face: the kept face f becomes row fincl[f] - 1 of f2, and its corner c,
// which names row id[3 f + c] of a table of `rows` survivors-to-be, is renumbered through vincl and made local to its mesh
// (vend2: the new vertex offsets).  An id outside the table gives -1.  takes_part (may be null: every mesh does) [K]: a
// mesh that takes no part keeps faces[3 f + c], its face as it went in.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void compact_faces_kernel(int F, int K, int rows, const int *__restrict__ id,
                                                                const int *__restrict__ tend,
                                                                const unsigned char *__restrict__ takes_part,
                                                                const int *__restrict__ faces,
                                                                const unsigned char *__restrict__ keep,
                                                                const int *__restrict__ fincl, const int *__restrict__ vincl,
                                                                const int *__restrict__ vend2, int *__restrict__ f2) {
  const long f = (long)blockIdx.x * THREADS + threadIdx.x;
  if (f >= F || !keep[f]) return;
  const int k = segment_of(tend, K, (int)f);
  const long at = fincl[f] - 1;                        // >= 0: keep[f] is counted in fincl[f]
  if (at < 0 || at >= F) return;
  const bool part = !takes_part || takes_part[k];
  const int *__restrict__ from = part ? id : faces;
  for (int c = 0; c < 3; ++c) {
    int out = from[3 * f + c];
    if (part) out = (unsigned)out < (unsigned)rows ? (vincl[out] - 1) - vend2[k] : -1;
    f2[3 * at + c] = out;
  }
}

// ---- launchers
static inline unsigned blocks_of(long n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

// what a launcher answers to a null pointer; `who` is its name, a string literal
#define MESH_NULL(who) rfd_invalid(who ": a null argument")
