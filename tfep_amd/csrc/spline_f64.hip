// float64 RQ spline kernels: forward, inverse and VJP on double tensors.  Same launch shape as the float32 spline
// (transformers.hip / backward.hip): one wavefront per sample row, its 64 lanes walk the features with unit stride, the
// log-derivative is summed with the wave butterfly (no atomics: bit-reproducible and independent of the batch the row sits
// in).  The other float64 transformers are the float32 kernels' double instantiations (transformers.hip, backward.hip).
//
// Numerics: everything in fp64 from double parameters, with the library exp / log / log1p / sqrt and IEEE divisions (no
// polynomial exponentials, no hardware-seeded reciprocals: the float32 kernels' shortcuts are accurate to ~1e-11, which is
// coarse next to the float64 reference).  The spline follows the reference's rules: strict '>' in the bin search, linear
// continuation along the boundary slope outside the domain (transformers/spline.py:567-650).
#include "common.h"
#include "spline_f64.h"

namespace tfep {
namespace {

constexpr int RPB = 4;   // rows (waves) per block of 256 threads

inline unsigned row_blocks64(int B) { return (unsigned)((B + RPB - 1) / RPB); }

__device__ inline void store_ldj64(double* ldj, int b, double total, int accumulate) {
    if ((threadIdx.x & 63) == 0) ldj[b] = accumulate ? ldj[b] + total : total;
}


template <int KMAX, bool INVERSE>
__global__ void __launch_bounds__(256) spline64_kernel(const double* __restrict__ x, int64_t ldx,
                                                       const double* __restrict__ params, tfep_param_layout L, Spline64 a,
                                                       double* __restrict__ y, int64_t ldy, double* __restrict__ ldj,
                                                       int accumulate, int B, int D) {
    const int b = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const double* xr = x + (int64_t)b * ldx;
    const double* pr = params + (int64_t)b * L.ld;
    double* yr = y + (int64_t)b * ldy;
    double acc = 0.0;
    for (int f = lane; f < D; f += 64) {
        double w[KMAX], h[KMAX], sraw[KMAX + 1], last, last2, ld;
        load_element64<KMAX>(pr + f * L.stride_f, L.stride_p, a, w, h, sraw, last, last2);
        yr[f] = rq_spline_element_f64<KMAX, INVERSE>(w, h, sraw, last, last2, a, a.x0[f], a.xf[f], a.y0[f], a.yf[f], xr[f],
                                                     &ld);
        acc += ld;
    }
    acc = wave_sum(acc);
    if (ldj) store_ldj64(ldj, b, INVERSE ? -acc : acc, accumulate);
}

// Reverse mode through rq_spline_element_f64<KMAX, false> (FORWARD map), every layout.  The same derivation as the float32
// VJP (backward.hip: rq_spline_backward) in IEEE fp64 arithmetic.  Writes the gradients of the raw widths / heights / knot
// slopes, of `last` / `last2` and of the input.
template <int KMAX>
__device__ inline void rq_spline_backward_f64(double (&pw)[KMAX], double (&ph)[KMAX], const double (&sraw)[KMAX + 1],
                                              double last, double last2, const Spline64& a, double x0f, double xff,
                                              double y0f, double yff, double vin, double gy, double gl,
                                              double (&guw)[KMAX], double (&guh)[KMAX], double (&gus)[KMAX + 1],
                                              double* glast, double* glast2, double* gxin) {
    const int K = a.K;
    const double mb = a.min_bin;
    const bool learn = a.learn_lower || a.learn_upper;
    double x0, y0, W, H;
    domain64(a, last, last2, x0f, xff, y0f, yff, x0, y0, W, H);
    double gx0 = 0.0, gy0 = 0.0, gWt = 0.0, gHt = 0.0;   // grads w.r.t. x0', y0' and direct terms of W, H
    double v = vin;
    if (a.circular) v = py_mod(v - x0 + last, xff - x0) + x0;
    softmax64(pw, K);
    softmax64(ph, K);

    double kx = x0, ky = y0, bw = 0.0, bh = 0.0;
    int kbin = -1;
    bool found = false;
    const bool lower_tail = !(v > x0);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K && !found) {
            const double wk = pw[k] * W + mb, hk = ph[k] * H + mb;
            if (v > kx + wk) {
                kx += wk;
                ky += hk;
            } else {
                found = true;
                bw = wk;
                bh = hk;
                kbin = k;
            }
        }

    double gw[KMAX], gh[KMAX], gd[KMAX + 1];      // grads w.r.t. bin widths, heights, knot slopes (values)
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        gw[k] = 0.0;
        gh[k] = 0.0;
        gd[k] = 0.0;
    }
    gd[KMAX] = 0.0;
    double gv;
    int ja = -1, jb2 = -1;                         // the (at most two) knots whose slope enters the element
    double sga = 0.0, sgb = 0.0;                   // and the derivatives of their softplus
    if (lower_tail || !found) {
        // y = y_b + d (v - x_b), ld = log d
        double rs = sraw[0];
        int jb = 0;
        if (!lower_tail) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k == K - 1) rs = sraw[k + 1];
            jb = K;
        }
        const double d = softplus64(rs + a.slope_offset) + a.min_slope;
        const double bx = lower_tail ? x0 : kx;
        const double gdb = gy * (v - bx) + gl / d;
        ja = jb;
        sga = softplus64_grad(rs + a.slope_offset);
        // boundary knot: (x0', y0') below, (x0' + W + K mb, y0' + H + K mb) above
        gx0 = -gy * d;
        gy0 = gy;
        if (!lower_tail) {
            gWt = -gy * d;
            gHt = gy;
        }
#pragma unroll
        for (int j = 0; j <= KMAX; ++j)
            if (j == jb) gd[j] = gdb;
        gv = gy * d;
    } else {
        double rs0 = sraw[0], rs1 = sraw[0];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k == kbin) {
                rs0 = sraw[k];
                rs1 = sraw[k + 1];
            }
        const double dk = softplus64(rs0 + a.slope_offset) + a.min_slope;
        const double dk1 = softplus64(rs1 + a.slope_offset) + a.min_slope;
        ja = kbin;
        jb2 = kbin + 1;
        sga = softplus64_grad(rs0 + a.slope_offset);
        sgb = softplus64_grad(rs1 + a.slope_offset);
        const double s = bh / bw, t = dk1 + dk - 2.0 * s;
        const double eps = (v - kx) / bw, om = 1.0 - eps, e1 = eps * om;
        const double A = s * eps * eps + dk * e1;
        const double Dn = s + t * e1;
        const double Q = dk1 * eps * eps + 2.0 * s * e1 + dk * om * om;
        const double dy_dA = bh / Dn, dy_dDn = -bh * A / (Dn * Dn);
        const double gs = gy * (dy_dA * eps * eps + dy_dDn * (1.0 - 2.0 * e1)) +
                          gl * (2.0 / s + 2.0 * e1 / Q - 2.0 * (1.0 - 2.0 * e1) / Dn);
        const double geps = gy * (dy_dA * (2.0 * s * eps + dk * (1.0 - 2.0 * eps)) + dy_dDn * t * (1.0 - 2.0 * eps)) +
                            gl * ((2.0 * dk1 * eps + 2.0 * s * (1.0 - 2.0 * eps) - 2.0 * dk * om) / Q -
                                  2.0 * t * (1.0 - 2.0 * eps) / Dn);
        const double gdk = gy * (dy_dA * e1 + dy_dDn * e1) + gl * (om * om / Q - 2.0 * e1 / Dn);
        const double gdk1 = gy * (dy_dDn * e1) + gl * (eps * eps / Q - 2.0 * e1 / Dn);
        const double gh_bin = gy * A / Dn + gs / bw;
        const double gw_bin = -gs * s / bw - geps * eps / bw;
        const double gxk = -geps / bw;
        gv = geps / bw;
        gx0 = gxk;
        gy0 = gy;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            if (k < kbin) {
                gw[k] = gxk;
                gh[k] = gy;
            } else if (k == kbin) {
                gw[k] = gw_bin;
                gh[k] = gh_bin;
            }
        }
#pragma unroll
        for (int j = 0; j <= KMAX; ++j) {
            if (j == kbin) gd[j] = gdk;
            if (j == kbin + 1) gd[j] = gdk1;
        }
    }

    // softmax backward: w_k = p_k W + mb
    double dotw = 0.0, doth = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        dotw += pw[k] * gw[k];
        doth += ph[k] * gh[k];
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        guw[k] = pw[k] * W * (gw[k] - dotw);
        guh[k] = ph[k] * H * (gh[k] - doth);
    }
    // softplus backward
#pragma unroll
    for (int j = 0; j <= KMAX; ++j) gus[j] = j == ja ? gd[j] * sga : (j == jb2 ? gd[j] * sgb : 0.0);
    *glast = a.circular ? gv : 0.0;
    *glast2 = 0.0;
    if (learn) {
        // W = W0 e^last, H = H0 e^last; w_k = p_k W + mb
        double gW = dotw + gWt, gH = doth + gHt;
        if (a.learn_lower && a.learn_upper) {
            *glast2 = gx0 + gy0;
        } else if (a.learn_lower) {      // x0' = xf - W - K mb, y0' = yf - H - K mb
            gW -= gx0;
            gH -= gy0;
        }
        *glast = gW * W + gH * H;
    }
    *gxin = gv;
}

template <int KMAX>
__global__ void __launch_bounds__(256) spline64_backward_kernel(const double* __restrict__ x, int64_t ldx,
                                                                const double* __restrict__ params, tfep_param_layout L,
                                                                Spline64 a, const double* __restrict__ gy, int64_t ldgy,
                                                                const double* __restrict__ gldj,
                                                                double* __restrict__ gparams, tfep_param_layout GL,
                                                                double* __restrict__ gx, int64_t ldgx, int B, int D) {
    const int b = blockIdx.x * RPB + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const int K = a.K, P = a.P;
    const double gl = gldj ? gldj[b] : 0.0;
    for (int f = lane; f < D; f += 64) {
        const double* pf = params + (int64_t)b * L.ld + f * L.stride_f;
        double* gp = gparams + (int64_t)b * GL.ld + f * GL.stride_f;
        const int64_t gsp = GL.stride_p;
        double w[KMAX], h[KMAX], sraw[KMAX + 1], last, last2;
        load_element64<KMAX>(pf, L.stride_p, a, w, h, sraw, last, last2);
        double guw[KMAX], guh[KMAX], gus[KMAX + 1], glast, glast2, gxin;
        rq_spline_backward_f64<KMAX>(w, h, sraw, last, last2, a, a.x0[f], a.xf[f], a.y0[f], a.yf[f], x[(int64_t)b * ldx + f],
                                     gy[(int64_t)b * ldgy + f], gl, guw, guh, gus, &glast, &glast2, &gxin);
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if (k < K) {
                gp[k * gsp] = guw[k];
                gp[(K + k) * gsp] = guh[k];
            }
        // knot K of a circular spline shares the parameter of knot 0; identity boundary slopes have no parameter
        double g0 = gus[0];
#pragma unroll
        for (int j = 0; j <= KMAX; ++j)
            if (j == K && a.circular && !a.identity) g0 += gus[j];
#pragma unroll
        for (int j = 0; j <= KMAX; ++j) {
            if (j > K) continue;
            if (a.circular && !a.identity && j == K) continue;
            const int pi = slope_param64(j, K, a.circular, a.identity);
            if (pi >= 0) gp[pi * gsp] = j == 0 ? g0 : gus[j];
        }
        if (a.circular || a.learn_lower || a.learn_upper) gp[(P - 1) * gsp] = glast;
        if (a.learn_lower && a.learn_upper) gp[(P - 2) * gsp] = glast2;
        gx[(int64_t)b * ldgx + f] = gxin;
    }
}


template <bool INVERSE>
int launch_spline64(const double* x, int64_t ldx, const double* params, tfep_param_layout L, const tfep_spline_desc_f64* desc,
                    double* y, int64_t ldy, double* ldj, int accumulate, int B, int D, void* stream) {
    Spline64 a;
    int rc = make_spline64(desc, &a);
    if (rc) return rc;
    TFEP_REQUIRE(B >= 0 && D >= 0, "spline_f64: negative size");
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(x && params && y, "spline_f64: x/params/y must be non-NULL");
    hipStream_t s = (hipStream_t)stream;
    if (a.K <= 8)
        spline64_kernel<8, INVERSE><<<row_blocks64(B), 256, 0, s>>>(x, ldx, params, L, a, y, ldy, ldj, accumulate, B, D);
    else if (a.K <= 16)
        spline64_kernel<16, INVERSE><<<row_blocks64(B), 256, 0, s>>>(x, ldx, params, L, a, y, ldy, ldj, accumulate, B, D);
    else
        spline64_kernel<32, INVERSE><<<row_blocks64(B), 256, 0, s>>>(x, ldx, params, L, a, y, ldy, ldj, accumulate, B, D);
    return check_launch("spline64_kernel");
}

}  // namespace
}  // namespace tfep

using namespace tfep;

extern "C" {

int tfep_spline_n_parameters_per_feature_f64(const tfep_spline_desc_f64* d) {
    Spline64 a;
    int rc = make_spline64(d, &a);
    return rc ? rc : a.P;
}

int tfep_spline_forward_f64(const double* x, int64_t ldx, const double* params, tfep_param_layout layout,
                            const tfep_spline_desc_f64* desc, double* y, int64_t ldy, double* log_det_J, int accumulate,
                            int B, int D, void* stream) {
    return launch_spline64<false>(x, ldx, params, layout, desc, y, ldy, log_det_J, accumulate, B, D, stream);
}

int tfep_spline_inverse_f64(const double* y, int64_t ldy, const double* params, tfep_param_layout layout,
                            const tfep_spline_desc_f64* desc, double* x, int64_t ldx, double* log_det_J, int accumulate,
                            int B, int D, void* stream) {
    return launch_spline64<true>(y, ldy, params, layout, desc, x, ldx, log_det_J, accumulate, B, D, stream);
}

int tfep_spline_backward_f64(const double* x, int64_t ldx, const double* params, tfep_param_layout layout,
                             const tfep_spline_desc_f64* desc, const double* gy, int64_t ldgy, const double* g_log_det_J,
                             double* gparams, tfep_param_layout glayout, double* gx, int64_t ldgx, int B, int D,
                             void* stream) {
    Spline64 a;
    int rc = make_spline64(desc, &a);
    if (rc) return rc;
    TFEP_REQUIRE(B >= 0 && D >= 0, "spline_backward_f64: negative size");
    if (B == 0 || D == 0) return TFEP_OK;
    TFEP_REQUIRE(x && params && gy && gparams && gx, "spline_backward_f64: NULL pointer");
    hipStream_t s = (hipStream_t)stream;
    if (a.K <= 8)
        spline64_backward_kernel<8><<<row_blocks64(B), 256, 0, s>>>(x, ldx, params, layout, a, gy, ldgy, g_log_det_J, gparams,
                                                                    glayout, gx, ldgx, B, D);
    else if (a.K <= 16)
        spline64_backward_kernel<16><<<row_blocks64(B), 256, 0, s>>>(x, ldx, params, layout, a, gy, ldgy, g_log_det_J, gparams,
                                                                     glayout, gx, ldgx, B, D);
    else
        spline64_backward_kernel<32><<<row_blocks64(B), 256, 0, s>>>(x, ldx, params, layout, a, gy, ldgy, g_log_det_J, gparams,
                                                                     glayout, gx, ldgx, B, D);
    return check_launch("spline64_backward_kernel");
}

}  // extern "C"
