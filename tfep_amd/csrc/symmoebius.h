// Symmetrized Moebius map of one d-vector (reference transformers/moebius.py:481-629), forward, inverse and the VJP of
// both, shared by the stand-alone kernels (transformers.hip, backward.hip).
//
// With u = max_radius / (1 + |w|) w (the unit-sphere rescaling), r2 = |u|^2, p = x . u and t2 = p^2 / |x|^2 = (xhat . u)^2
// the two Moebius images of the reference add up to a multiple of (1 + r2) x - 2 p u, and its analytic inverse
// (moebius.py:554-602: the solution in the plane of w and x) to a multiple of (1 - r2) x + 2 p u.  Both directions are
//   y = (alpha x + beta p u) / sqrt(H),   |y| = |x|
//   forward: alpha = 1 + r2, beta = -2, H = (1 - r2)^2 + 4 (r2 - t2)      (= alpha^2 - 4 t2: the reference's 4 q + (1 - r2)^2)
//            log|det J| = log((1 - r2)(1 + r2)^(d-1)) - d/2 log H                                       (moebius.py:608-629)
//   inverse: alpha = 1 - r2, beta = +2, H = (1 - r2)^2 + 4 t2             (= alpha^2 + 4 t2)
//            log|det J| = log((1 - r2)^(d-1) (1 + r2)) - d/2 log H
// The inverse log-det is minus the forward formula at the solution x', whose 4 q' + (1 - r2)^2 is
// (1 + r2)^2 (1 - r2)^2 / H: the form above has no cancellation.  1 - r2 >= 1 - max_radius^2 > 0, so H > 0.
//
// Degenerate inputs: w = 0 gives u = 0, y = x and log-det 0 in BOTH directions, and x parallel to w is a fixed
// direction -- the closed form has no 0 / 0 where the reference's inverse divides by |w| and by the norm of the
// component of x orthogonal to w.  x = 0 gives NaN (the reference divides by |x| too).  The VJP at w = 0 takes the
// gradient of |w| as 0, like torch.
//
// T is the element type of the kernel: float kernels compute in fp64 with the ~1 ulp helpers of fp64_fast.h (their
// results are rounded to float), double kernels with IEEE division, square root and logarithm (SymMath<T>, fp64_fast.h).
#pragma once
#include <hip/hip_runtime.h>

#include "fp64_fast.h"
#include "moebius.h"

namespace tfep {

__device__ __forceinline__ double sym_powi(double a, int n) {      // a^n, n = 1 .. MOEBIUS_MAX_DIM - 1
    double out = a;
#pragma unroll
    for (int i = 1; i < MOEBIUS_MAX_DIM - 1; ++i)
        if (i < n) out *= a;
    return out;
}

// xv: the point, wv: the raw parameter vector; yv: the image.  Returns log|det J| of the direction taken.
template <typename T, bool INVERSE>
__device__ __forceinline__ double symmoebius_vector(const double (&xv)[MOEBIUS_MAX_DIM], const double (&wv)[MOEBIUS_MAX_DIM],
                                                    int dim, double max_radius, double (&yv)[MOEBIUS_MAX_DIM]) {
    using M = SymMath<T>;
    double wn2 = 0.0, xn2 = 0.0, xw = 0.0;
#pragma unroll
    for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
        if (i < dim) {
            wn2 += wv[i] * wv[i];
            xn2 += xv[i] * xv[i];
            xw += xv[i] * wv[i];
        }
    const double s = max_radius * M::rcp(1.0 + M::sqrt(wn2));      // moebius.py:531-535
    const double r2 = s * s * wn2, p = s * xw;
    const double t2 = p * p * M::rcp(xn2);
    const double c1 = 1.0 - r2, c2 = 1.0 + r2;
    const double alpha = INVERSE ? c1 : c2, beta = INVERSE ? 2.0 : -2.0;
    const double H = c1 * c1 + 4.0 * (INVERSE ? t2 : r2 - t2);
    const double k = M::rcp(M::sqrt(H)), bps = beta * p * s;
#pragma unroll
    for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
        if (i < dim) yv[i] = k * (alpha * xv[i] + bps * wv[i]);
    const double numer = INVERSE ? sym_powi(c1, dim - 1) * c2 : c1 * sym_powi(c2, dim - 1);
    return M::log(numer) - 0.5 * dim * M::log(H);
}

// Reverse mode through symmoebius_vector: gyv / gl are the cotangents of the image and of the log-det; writes the
// cotangents of the point (gxv) and of the raw parameter vector (gwv).
template <typename T, bool INVERSE>
__device__ __forceinline__ void symmoebius_vjp_vector(const double (&xv)[MOEBIUS_MAX_DIM], const double (&wv)[MOEBIUS_MAX_DIM],
                                                      int dim, double max_radius, const double (&gyv)[MOEBIUS_MAX_DIM],
                                                      double gl, double (&gxv)[MOEBIUS_MAX_DIM], double (&gwv)[MOEBIUS_MAX_DIM]) {
    using M = SymMath<T>;
    double wn2 = 0.0, xn2 = 0.0, xw = 0.0, gx_ = 0.0, gw_ = 0.0;      // gx_ = gy . x, gw_ = gy . w
#pragma unroll
    for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
        if (i < dim) {
            wn2 += wv[i] * wv[i];
            xn2 += xv[i] * xv[i];
            xw += xv[i] * wv[i];
            gx_ += gyv[i] * xv[i];
            gw_ += gyv[i] * wv[i];
        }
    const double wn = M::sqrt(wn2), inv_1pw = M::rcp(1.0 + wn);
    const double s = max_radius * inv_1pw;
    const double r2 = s * s * wn2, p = s * xw;
    const double inv_xn2 = M::rcp(xn2);
    const double t2 = p * p * inv_xn2;
    const double c1 = 1.0 - r2, c2 = 1.0 + r2;
    const double alpha = INVERSE ? c1 : c2, beta = INVERSE ? 2.0 : -2.0;
    const double H = c1 * c1 + 4.0 * (INVERSE ? t2 : r2 - t2);
    const double inv_H = M::rcp(H), k = M::rcp(M::sqrt(H));
    const double inv_c1 = M::rcp(c1), inv_c2 = M::rcp(c2);
    // y = k z, z = alpha x + beta p u, u = s w:  zb = k gy
    const double gz = alpha * gx_ + beta * p * s * gw_;             // gy . z
    const double Hb = -0.5 * k * gz * inv_H - 0.5 * dim * gl * inv_H;   // k = H^(-1/2); ldj has -d/2 log H
    const double alphab = k * gx_;
    double pb = beta * k * s * gw_;                                    // zb . (beta u)
    // log-det numerator and H in c1, c2, r2, t2
    double c1b = 2.0 * c1 * Hb, c2b, r2b, t2b;
    if (INVERSE) {
        c1b += alphab + (dim - 1) * gl * inv_c1;
        c2b = gl * inv_c2;
        r2b = 0.0;
        t2b = 4.0 * Hb;
    } else {
        c1b += gl * inv_c1;
        c2b = alphab + (dim - 1) * gl * inv_c2;
        r2b = 4.0 * Hb;
        t2b = -4.0 * Hb;
    }
    r2b += c2b - c1b;
    pb += t2b * 2.0 * p * inv_xn2;                                      // t2 = p^2 / |x|^2
    const double xn2b = -t2b * t2 * inv_xn2;
    // p = s (x . w), r2 = s^2 |w|^2, u = s w (through z: ub = beta p zb):  the cotangent of s, then of |w|
    const double sb = pb * xw + 2.0 * r2b * s * wn2 + beta * p * k * gw_;
    const double wnb = -sb * s * inv_1pw;
    const double wn2b = r2b * s * s + (wn > 0.0 ? 0.5 * wnb * M::rcp(wn) : 0.0);
    const double ak = alpha * k, bpsk = beta * p * s * k, pbs = pb * s;
#pragma unroll
    for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
        if (i < dim) {
            gxv[i] = ak * gyv[i] + pbs * wv[i] + 2.0 * xn2b * xv[i];
            gwv[i] = bpsk * gyv[i] + pbs * xv[i] + 2.0 * wn2b * wv[i];
        }
}

}  // namespace tfep
