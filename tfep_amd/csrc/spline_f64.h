// float64 RQ spline: descriptor view, parameter loading and the element map, shared by the standalone float64 spline
// kernels (spline_f64.hip) and the float64 blocked inverse (inverse_block_f64.hip).
#pragma once

#include "common.h"

#include <math.h>

namespace tfep {

// ---------------------------------------------------------------- RQ spline (spline.py)
struct Spline64 {
    const double *x0, *xf, *y0, *yf;
    int K, P;
    bool circular, identity, learn_lower, learn_upper;
    double min_bin, min_slope, slope_offset;   // slope_offset = log(exp(1 - min_slope) - 1), spline.py:414
};

// Parameter position of the raw slope of knot j (spline.py:359-380); -1: the constant 0 of an identity boundary slope.
__host__ __device__ inline int slope_param64(int j, int K, bool circular, bool identity) {
    if (identity) {
        if (j == 0 || j == K) return -1;
        return 2 * K + j - 1;
    }
    if (circular && j == K) return 2 * K;
    return 2 * K + j;
}

__host__ __device__ inline int n_params64(int K, bool circular, bool identity, bool ll, bool lu) {
    int n = 3 * K + 1;          // spline.py:165-182
    if (ll) n += 1;
    if (lu) n += 1;
    if (identity) n -= circular ? 1 : 2;
    return n;
}

// torch softplus (beta 1, threshold 20) and its derivative
__device__ inline double softplus64(double z) { return z > 20.0 ? z : log1p(exp(z)); }
__device__ inline double softplus64_grad(double z) {
    if (z > 20.0) return 1.0;
    if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
    const double e = exp(z);
    return e / (1.0 + e);
}

// The P parameters of one element, expanded: K raw widths, K raw heights, K + 1 raw knot slopes, `last` / `last2` =
// parameters P - 1 / P - 2 (circular shift; log-scale and shift of a learnable domain), 0 where unused.
template <int KMAX>
__device__ inline void load_element64(const double* pf, int64_t sp, const Spline64& a, double (&w)[KMAX],
                                      double (&h)[KMAX], double (&sraw)[KMAX + 1], double& last, double& last2) {
    const int K = a.K;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        w[k] = 0.0;
        h[k] = 0.0;
        if (k < K) {
            w[k] = pf[k * sp];
            h[k] = pf[(K + k) * sp];
        }
    }
#pragma unroll
    for (int j = 0; j <= KMAX; ++j) {
        sraw[j] = 0.0;
        if (j <= K) {
            const int pi = slope_param64(j, K, a.circular, a.identity);
            if (pi >= 0) sraw[j] = pf[pi * sp];
        }
    }
    last = (a.circular || a.learn_lower || a.learn_upper) ? pf[(a.P - 1) * sp] : 0.0;
    last2 = (a.learn_lower && a.learn_upper) ? pf[(a.P - 2) * sp] : 0.0;
}

// Domain of the element after the learnable bounds (spline.py:384-410).
__device__ inline void domain64(const Spline64& a, double last, double last2, double x0f, double xff, double y0f, double yff,
                                double& x0, double& y0, double& W, double& H) {
    const double mi = a.K * a.min_bin;
    x0 = x0f;
    y0 = y0f;
    W = xff - x0f - mi;
    H = yff - y0f - mi;
    if (a.learn_lower || a.learn_upper) {
        const double scale = exp(last);
        W *= scale;
        H *= scale;
        if (a.learn_lower && a.learn_upper) {
            x0 += last2;
            y0 += last2;
        } else if (a.learn_lower) {
            x0 = xff - W - mi;
            y0 = yff - H - mi;
        }
    }
}

// softmax in place: p[k] = exp(u[k] - max) / sum (spline.py:394-395)
template <int KMAX>
__device__ inline void softmax64(double (&u)[KMAX], int K) {
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
        if (k < K) m = fmax(m, u[k]);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        u[k] = k < K ? exp(u[k] - m) : 0.0;
        s += u[k];
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) u[k] = u[k] / s;
}

// One element of the forward (INVERSE = false) or inverse map; w / h are overwritten by their softmax.  Returns the mapped
// value; *logd receives log(dy/dx) of the FORWARD map at the point (the caller negates it for the inverse).
template <int KMAX, bool INVERSE>
__device__ inline double rq_spline_element_f64(double (&w)[KMAX], double (&h)[KMAX], const double (&sraw)[KMAX + 1],
                                               double last, double last2, const Spline64& a, double x0f, double xff,
                                               double y0f, double yff, double vin, double* logd) {
    const int K = a.K;
    const double mb = a.min_bin;
    double x0, y0, W, H;
    domain64(a, last, last2, x0f, xff, y0f, yff, x0, y0, W, H);
    double v = vin;
    if (a.circular && !INVERSE) v = py_mod(v - x0 + last, xff - x0) + x0;      // spline.py:236-238
    softmax64(w, K);
    softmax64(h, K);

    // bin search: strict '>' (spline.py:622-625); v <= first knot -> lower tail, past the last knot -> upper tail
    double kx = x0, ky = y0, bw = 0.0, bh = 0.0, rs0 = sraw[0], rs1 = sraw[0], rs_last = sraw[0];
    bool found = false;
    const bool lower_tail = !(v > (INVERSE ? y0 : x0));
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
        if (k < K) {
            const double wk = w[k] * W + mb;
            const double hk = h[k] * H + mb;
            if (!found) {
                const double upper = INVERSE ? ky + hk : kx + wk;
                if (v > upper) {
                    kx += wk;
                    ky += hk;
                } else {
                    found = true;
                    bw = wk;
                    bh = hk;
                    rs0 = sraw[k];
                    rs1 = sraw[k + 1];
                }
            }
            if (k == K - 1) rs_last = sraw[k + 1];
        }
    }

    double out, ld;
    if (lower_tail || !found) {
        // linear continuation along the boundary slope (the reference's sentinel knots, spline.py:599-614)
        const double d = softplus64((lower_tail ? sraw[0] : rs_last) + a.slope_offset) + a.min_slope;
        const double bx = lower_tail ? x0 : kx, by = lower_tail ? y0 : ky;
        out = INVERSE ? bx + (v - by) / d : by + d * (v - bx);
        ld = log(d);
    } else {
        const double dk = softplus64(rs0 + a.slope_offset) + a.min_slope;
        const double dk1 = softplus64(rs1 + a.slope_offset) + a.min_slope;
        const double s = bh / bw;                                  // spline.py:643
        const double t = dk1 + dk - 2.0 * s;
        double eps;
        if (INVERSE) {                                             // spline.py:521-536
            const double ym = v - ky;
            const double qa = bh * (s - dk) + ym * t;
            const double qb = bh * dk - ym * t;
            const double qc = -s * ym;
            eps = 2.0 * qc / (-qb - sqrt(qb * qb - 4.0 * qa * qc));
            out = eps * bw + kx;
        } else {                                                   // spline.py:485-494
            eps = (v - kx) / bw;
            const double e1 = eps * (1.0 - eps);
            out = ky + bh * (s * eps * eps + dk * e1) / (s + t * e1);
        }
        const double e1 = eps * (1.0 - eps);                       // spline.py:556-558
        const double om = 1.0 - eps;
        const double num = s * s * (dk1 * eps * eps + 2.0 * s * e1 + dk * om * om);
        const double den = s + t * e1;
        ld = log(num / (den * den));
    }
    if (a.circular && INVERSE) out = py_mod(out - x0 - last, xff - x0) + x0;   // spline.py:257-259
    *logd = ld;
    return out;
}

// Host-side view and validation of a tfep_spline_desc_f64 (the rules of make_spline_args).
inline int make_spline64(const tfep_spline_desc_f64* d, Spline64* a) {
    TFEP_REQUIRE(d != nullptr, "spline descriptor is NULL");
    TFEP_REQUIRE(d->x0 && d->xf && d->y0 && d->yf, "spline descriptor: x0/xf/y0/yf must be non-NULL");
    TFEP_REQUIRE(d->n_bins >= 1 && d->n_bins <= 32, "spline: n_bins=%d unsupported (1..32)", d->n_bins);
    TFEP_REQUIRE(!(d->circular && (d->learn_lower_bound || d->learn_upper_bound)),
                 "Cannot instantiate a circular spline with learnable limits.");
    TFEP_REQUIRE(d->min_bin_size > 0.0, "The minimum bin size should be positive.");
    TFEP_REQUIRE(d->min_slope > 0.0 && d->min_slope < 1.0, "The minimum slope should be between 0 and 1.");
    a->x0 = d->x0;
    a->xf = d->xf;
    a->y0 = d->y0;
    a->yf = d->yf;
    a->K = d->n_bins;
    a->circular = d->circular != 0;
    a->identity = d->identity_boundary_slopes != 0;
    a->learn_lower = d->learn_lower_bound != 0;
    a->learn_upper = d->learn_upper_bound != 0;
    a->min_bin = d->min_bin_size;
    a->min_slope = d->min_slope;
    a->slope_offset = log(exp(1.0 - d->min_slope) - 1.0);
    a->P = n_params64(a->K, a->circular, a->identity, a->learn_lower, a->learn_upper);
    return TFEP_OK;
}

}  // namespace tfep
