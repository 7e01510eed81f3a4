// Quaternion product map of one quaternion (reference transformers/quatprod.py), forward, inverse and the VJP of both,
// shared by the stand-alone kernels (transformers.hip, backward.hip).
//
// Quaternions are 4 contiguous features, scalar LAST: (x, y, z, w) = x i + y j + z k + w, with the Hamilton product
//   (a (x) b).xyz = a.w b.xyz + b.w a.xyz + a.xyz x b.xyz,      (a (x) b).w = a.w b.w - a.xyz . b.xyz
// so the identity quaternion is (0, 0, 0, 1).  With q = p / |p| the normalised parameter quaternion
//   forward: y = q (x) x,          inverse: x = conj(q) (x) y,          conj(a) = (-a.xyz, a.w).
// Left multiplication by a unit quaternion is an orthogonal 4 x 4 matrix L(q), and L(conj(q)) = L(q)^T: the map preserves
// |x| and volume (log|det J| = 0 -- the kernels write the zero, nothing is computed for it), and it is linear in x, so
// T(-x) = -T(x).
//
// VJP.  <a (x) b, g> = <b, conj(a) (x) g> = <a, g (x) conj(b)>, so with g the cotangent of the output
//   forward: gx = conj(q) (x) g,   gq = g (x) conj(x)
//   inverse: gy = q (x) g,         gq = conj(g (x) conj(y)) = y (x) conj(g)
// and through the normalisation q = p / |p|:  gp = (gq - q (q . gq)) / |p|.  The cotangent of the log-det multiplies a
// constant and contributes nothing.
//
// p = 0 is 0 / 0 in the reference (NaN); here too: nothing special-cases it, every output of that quaternion is NaN.
//
// T is the element type of the kernel: float kernels compute in fp64 with the ~1 ulp helpers of fp64_fast.h (their
// results are rounded to float: the identity parameters return x bit for bit), double kernels with IEEE division and
// square root (|p| = 1 gives 1 / |p| = 1 and q = p exactly).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fp64_fast.h"

namespace tfep {

// One quaternion as 16-byte pieces (one float4, or two double2) when the row starts on a 16-byte boundary -- every
// quaternion of the row does then --, else element by element (column slices of a mixed transformer's parameters).
template <typename T> struct alignas(16) QuatPack { T v[16 / sizeof(T)]; };

template <typename T> __device__ __forceinline__ bool quat_aligned(const void* row) { return ((uintptr_t)row & 15) == 0; }

template <typename T>
__device__ __forceinline__ void quat_load(const T* __restrict__ row, int q, bool packed, double (&out)[4]) {
    constexpr int N = 16 / (int)sizeof(T), PIECES = 4 / N;
    if (packed) {
        const QuatPack<T>* src = reinterpret_cast<const QuatPack<T>*>(row) + (int64_t)q * PIECES;
#pragma unroll
        for (int k = 0; k < PIECES; ++k) {
            const QuatPack<T> piece = src[k];
#pragma unroll
            for (int i = 0; i < N; ++i) out[k * N + i] = (double)piece.v[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = (double)row[(int64_t)q * 4 + i];
    }
}

template <typename T>
__device__ __forceinline__ void quat_store(T* __restrict__ row, int q, bool packed, const double (&in)[4]) {
    constexpr int N = 16 / (int)sizeof(T), PIECES = 4 / N;
    if (packed) {
        QuatPack<T>* dst = reinterpret_cast<QuatPack<T>*>(row) + (int64_t)q * PIECES;
#pragma unroll
        for (int k = 0; k < PIECES; ++k) {
            QuatPack<T> piece;
#pragma unroll
            for (int i = 0; i < N; ++i) piece.v[i] = (T)in[k * N + i];
            dst[k] = piece;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) row[(int64_t)q * 4 + i] = (T)in[i];
    }
}

// 1 / |p| from |p|^2
template <typename T> __device__ __forceinline__ double quat_inv_norm(double n2);
template <> __device__ __forceinline__ double quat_inv_norm<float>(double n2) { return fast_rcp64(fast_sqrt64(n2)); }
template <> __device__ __forceinline__ double quat_inv_norm<double>(double n2) { return 1.0 / ::sqrt(n2); }

// q = p / |p| as p * (1 / |p|): one reciprocal per quaternion, and |p| = 1 gives q = p exactly in the double kernels.
template <typename T>
__device__ __forceinline__ void quat_normalize(const double (&p)[4], double (&q)[4], double& inv_norm) {
    const double n2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3];
    inv_norm = quat_inv_norm<T>(n2);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = p[i] * inv_norm;
}

// out = a (x) b, with the vector part of a (CONJ_A) or of b (CONJ_B) negated first
template <bool CONJ_A, bool CONJ_B>
__device__ __forceinline__ void quat_mul(const double (&a)[4], const double (&b)[4], double (&out)[4]) {
    const double sa = CONJ_A ? -1.0 : 1.0, sb = CONJ_B ? -1.0 : 1.0;
    const double ax = sa * a[0], ay = sa * a[1], az = sa * a[2], aw = a[3];
    const double bx = sb * b[0], by = sb * b[1], bz = sb * b[2], bw = b[3];
    out[0] = aw * bx + ax * bw + ay * bz - az * by;
    out[1] = aw * by - ax * bz + ay * bw + az * bx;
    out[2] = aw * bz + ax * by - ay * bx + az * bw;
    out[3] = aw * bw - ax * bx - ay * by - az * bz;
}

// xv: the quaternion, pv: the raw parameter quaternion; yv: the image.
template <typename T, bool INVERSE>
__device__ __forceinline__ void quatprod_element(const double (&xv)[4], const double (&pv)[4], double (&yv)[4]) {
    double q[4], inv_norm;
    quat_normalize<T>(pv, q, inv_norm);
    quat_mul<INVERSE, false>(q, xv, yv);
}

// Reverse mode through quatprod_element: gv is the cotangent of the image; writes the cotangents of the input quaternion
// (gxv) and of the raw parameter quaternion (gpv).
template <typename T, bool INVERSE>
__device__ __forceinline__ void quatprod_vjp_element(const double (&xv)[4], const double (&pv)[4], const double (&gv)[4],
                                                     double (&gxv)[4], double (&gpv)[4]) {
    double q[4], gq[4], inv_norm;
    quat_normalize<T>(pv, q, inv_norm);
    quat_mul<!INVERSE, false>(q, gv, gxv);                       // L(q)^T g forward, L(q) g inverse
    if (INVERSE)
        quat_mul<false, true>(xv, gv, gq);                       // y (x) conj(g)
    else
        quat_mul<false, true>(gv, xv, gq);                       // g (x) conj(x)
    const double dot = q[0] * gq[0] + q[1] * gq[1] + q[2] * gq[2] + q[3] * gq[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) gpv[i] = (gq[i] - q[i] * dot) * inv_norm;
}

}  // namespace tfep
