// Standalone (unfused) transformer kernels: affine, volume-preserving shift, RQ spline,
// Moebius, periodic embedding, column gather/scatter.  HBM-bound elementwise work with a
// per-sample log|det J| reduction: one wavefront owns one sample (row), its 64 lanes walk the
// features with unit stride (coalesced 256-B segments per parameter row) and the log-derivative
// is summed in fp64 with a wave butterfly -- no atomics, bit-reproducible.
// Affine, volume-preserving shift, SOS, Moebius, symmetrized Moebius, quaternion product, periodic embedding and column gather / scatter are templates on the element
// type: the float instantiation serves the float32 entry points, the double one their _f64 twins.  (The float64 RQ spline
// has numerics of its own: spline_f64.hip.)
#include "common.h"
#include "spline.h"
#include "moebius.h"
#include "symmoebius.h"
#include "quatprod.h"
#include "sos.h"
#include "embedding.h"

#include <stdarg.h>

#include <type_traits>

namespace tfep {

std::string& last_error() {
    static thread_local std::string s;
    return s;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}

constexpr int ROWS_PER_BLOCK = 4;   // 4 waves = 256 threads

template <typename T>
__device__ inline void store_ldj(T* ldj, int b, double total, int accumulate) {
    if ((threadIdx.x & 63) == 0) {
        if (accumulate)
            ldj[b] = (T)((double)ldj[b] + total);
        else
            ldj[b] = (T)total;
    }
}

// ---------------------------------------------------------------- affine (affine.py:321-323, :361-363)
template <typename T, bool INVERSE>
__global__ void __launch_bounds__(256) affine_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ params,
                                                     tfep_param_layout L, T* __restrict__ y, int64_t ldy,
                                                     T* __restrict__ ldj, int accumulate, int B, int D) {
    const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const T* xr = x + (int64_t)b * ldx;
    const T* pr = params + (int64_t)b * L.ld;
    T* yr = y + (int64_t)b * ldy;
    double acc = 0.0;
    for (int f = lane; f < D; f += 64) {
        const T shift = pr[f * L.stride_f];
        const T ls = pr[L.stride_p + f * L.stride_f];
        const T v = xr[f];
        if (INVERSE)
            yr[f] = (v - shift) * exp(-ls);
        else
            yr[f] = v * exp(ls) + shift;
        acc += (double)ls;
    }
    acc = wave_sum(acc);
    if (ldj) store_ldj(ldj, b, INVERSE ? -acc : acc, accumulate);
}

// ---------------------------------------------------------------- volume preserving shift (affine.py:366-456)
// (py_mod: fmodf + sign fix-up in float32, floor + fma in float64; common.h)
template <typename T>
__global__ void __launch_bounds__(256) volpres_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ shift,
                                                      int64_t ldp, const int32_t* __restrict__ periodic, T lower, T upper,
                                                      T sign, T* __restrict__ y, int64_t ldy, int B, int D) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * D) return;
    const int b = (int)(i / D), f = (int)(i % D);
    T v = x[(int64_t)b * ldx + f] + sign * shift[(int64_t)b * ldp + f];
    if (periodic && periodic[f]) v = py_mod(v, upper - lower) + lower;      // Python `%`, then + lower (affine.py:409, :454)
    y[(int64_t)b * ldy + f] = v;
}

// ---------------------------------------------------------------- RQ spline (spline.py)
template <int KMAX, bool INVERSE>
__global__ void __launch_bounds__(256) spline_kernel(const float* __restrict__ x, int64_t ldx,
                                                     const float* __restrict__ params, tfep_param_layout L,
                                                     SplineArgs a, float* __restrict__ y, int64_t ldy,
                                                     float* __restrict__ ldj, int accumulate, int B, int D) {
    const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + (int64_t)b * ldx;
    const float* pr = params + (int64_t)b * L.ld;
    float* yr = y + (int64_t)b * ldy;
    const int K = a.f.K;
    double acc = 0.0;
    for (int f = lane; f < D; f += 64) {
        const float* pf = pr + f * L.stride_f;
        float w[KMAX], h[KMAX], sraw[KMAX + 1];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            w[k] = 0.f;
            h[k] = 0.f;
            if (k < K) {
                w[k] = pf[k * L.stride_p];
                h[k] = pf[(K + k) * L.stride_p];
            }
        }
#pragma unroll
        for (int j = 0; j <= KMAX; ++j) {
            sraw[j] = 0.f;
            if (j <= K) {
                const int pi = spline_slope_param(j, K, a.f.circular, a.f.identity);
                if (pi >= 0) sraw[j] = pf[pi * L.stride_p];
            }
        }
        float last = 0.f, last2 = 0.f;
        if (a.f.circular || a.f.learn_lower || a.f.learn_upper) last = pf[(a.P - 1) * L.stride_p];
        if (a.f.learn_lower && a.f.learn_upper) last2 = pf[(a.P - 2) * L.stride_p];
        double ld;
        const double out = rq_spline_element<KMAX, INVERSE>(w, h, sraw, last, last2, a.f, a.x0[f], a.xf[f],
                                                            a.y0[f], a.yf[f], xr[f], &ld);
        yr[f] = (float)out;
        acc += ld;
    }
    acc = wave_sum(acc);
    if (ldj) store_ldj(ldj, b, INVERSE ? -acc : acc, accumulate);
}

// ---------------------------------------------------------------- Moebius (moebius.py:374-478)
// One lane per d-vector; the map and its closed-form log|det J| are in moebius.h.  DIM > 0: the dimension is a compile-time
// constant (d = 2, 3: the loops of moebius_vector unroll to d steps instead of MOEBIUS_MAX_DIM predicated ones; the
// d = 2 vector is one 8-byte (float) or 16-byte (double) load / store) -- the same arithmetic in the same order, bit for
// bit; DIM = 0: any d.  T = double: float64 I/O and the IEEE arithmetic of SymMath<double>; the split-f16 copy of y
// (y_split) is a float kernel's only.
template <typename T, int DIM>
__global__ void __launch_bounds__(256) moebius_kernel(const T* __restrict__ x, int64_t ldx,
                                                      const T* __restrict__ params, int64_t ldp, int dim_rt,
                                                      double max_radius, int unit_sphere, T sign,
                                                      T* __restrict__ y, int64_t ldy, T* __restrict__ ldj,
                                                      int accumulate, int B, int D, uint32_t* __restrict__ y_split = nullptr,
                                                      int64_t ld_split = 0, float* __restrict__ y_inv_scale = nullptr) {
    using T2 = std::conditional_t<std::is_same_v<T, float>, float2, double2>;
    const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const int dim = DIM > 0 ? DIM : dim_rt;
    const int nvec = D / dim;
    const T* xr = x + (int64_t)b * ldx;
    const T* pr = params + (int64_t)b * ldp;
    T* yr = y + (int64_t)b * ldy;
    // (one access per vector for d = 2 when the three rows start on boundaries of a whole vector: wave uniform)
    const bool vec2 = DIM == 2 && (((uintptr_t)xr | (uintptr_t)pr | (uintptr_t)yr) & (uintptr_t)(sizeof(T2) - 1)) == 0;
    double acc = 0.0;
    for (int v = lane; v < nvec; v += 64) {
        double xv[MOEBIUS_MAX_DIM], wv[MOEBIUS_MAX_DIM], yv[MOEBIUS_MAX_DIM];
        if (vec2) {
            const T2 xx = reinterpret_cast<const T2*>(xr)[v], pp = reinterpret_cast<const T2*>(pr)[v];
            xv[0] = (double)xx.x; xv[1] = (double)xx.y;
            wv[0] = (double)(sign * pp.x); wv[1] = (double)(sign * pp.y);
        } else {
#pragma unroll
            for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
                if (i < dim) {
                    xv[i] = (double)xr[v * dim + i];
                    wv[i] = (double)(sign * pr[v * dim + i]);
                }
        }
        acc += moebius_vector<T>(xv, wv, dim, max_radius, unit_sphere, yv);
        if (vec2) {
            reinterpret_cast<T2*>(yr)[v] = T2{(T)yv[0], (T)yv[1]};
            if constexpr (std::is_same_v<T, float>) {
                if (y_split) {
                    // the same row as split-f16 halves for the next layer's GEMM (tfep_split_rows' format: per 8 features 8 hi
                    // then 8 lo halves), with the scale of the bound |y| <= 1 of a unit-sphere map: 2^14
                    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
                    const float t0 = (float)yv[0] * 16384.0f, t1 = (float)yv[1] * 16384.0f;
                    const _Float16 h0 = (_Float16)t0, h1 = (_Float16)t1;
                    const h2 hi = {h0, h1}, lo = {(_Float16)(t0 - (float)h0), (_Float16)(t1 - (float)h1)};
                    uint32_t* grp = y_split + (int64_t)b * ld_split + (v >> 2) * 8;        // 8 words = 32 bytes per group of 8 features
                    grp[v & 3] = __builtin_bit_cast(uint32_t, hi);
                    grp[4 + (v & 3)] = __builtin_bit_cast(uint32_t, lo);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
                if (i < dim) yr[v * dim + i] = (T)yv[i];
        }
    }
    if constexpr (std::is_same_v<T, float>) {
        if (y_split) {
            // padding groups up to the row's k-tile stay zero (the caller clears the buffer once); the row's 1/scale
            if (lane == 0) y_inv_scale[b] = 1.0f / 16384.0f;
        }
    }
    acc = wave_sum(acc);
    if (ldj) store_ldj(ldj, b, acc, accumulate);
}

// ---------------------------------------------------------------- symmetrized Moebius (moebius.py:481-629; symmoebius.h)
// One lane per d-vector like moebius_kernel; DIM = 2, 3, 4 at compile time (4: quaternions), DIM = 0: any d.  A vector of
// 8 or 16 bytes is one load / store when the three rows start on such a boundary (wave uniform).
template <typename T, int DIM, bool INVERSE>
__global__ void __launch_bounds__(256) symmoebius_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ params,
                                                         int64_t ldp, int dim_rt, double max_radius, T* __restrict__ y,
                                                         int64_t ldy, T* __restrict__ ldj, int accumulate, int B, int D) {
    const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const int dim = DIM > 0 ? DIM : dim_rt;
    const int nvec = D / dim;
    const T* xr = x + (int64_t)b * ldx;
    const T* pr = params + (int64_t)b * ldp;
    T* yr = y + (int64_t)b * ldy;
    constexpr int VB = DIM * (int)sizeof(T);                    // bytes of one vector
    constexpr bool CAN_PACK = VB == 8 || VB == 16;
    struct alignas(CAN_PACK ? VB : (int)sizeof(T)) Pack { T v[DIM > 0 ? DIM : 1]; };
    const bool packed = CAN_PACK && (((uintptr_t)xr | (uintptr_t)pr | (uintptr_t)yr) & (uintptr_t)(VB - 1)) == 0;
    double acc = 0.0;
    for (int v = lane; v < nvec; v += 64) {
        double xv[MOEBIUS_MAX_DIM], wv[MOEBIUS_MAX_DIM], yv[MOEBIUS_MAX_DIM];
        if (packed) {
            const Pack xx = reinterpret_cast<const Pack*>(xr)[v], pp = reinterpret_cast<const Pack*>(pr)[v];
#pragma unroll
            for (int i = 0; i < DIM; ++i) {
                xv[i] = (double)xx.v[i];
                wv[i] = (double)pp.v[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
                if (i < dim) {
                    xv[i] = (double)xr[v * dim + i];
                    wv[i] = (double)pr[v * dim + i];
                }
        }
        acc += symmoebius_vector<T, INVERSE>(xv, wv, dim, max_radius, yv);
        if (packed) {
            Pack yy;
#pragma unroll
            for (int i = 0; i < DIM; ++i) yy.v[i] = (T)yv[i];
            reinterpret_cast<Pack*>(yr)[v] = yy;
        } else {
#pragma unroll
            for (int i = 0; i < MOEBIUS_MAX_DIM; ++i)
                if (i < dim) yr[v * dim + i] = (T)yv[i];
        }
    }
    acc = wave_sum(acc);
    if (ldj) store_ldj(ldj, b, acc, accumulate);
}

// ---------------------------------------------------------------- quaternion product (quatprod.py; quatprod.h)
// One lane per quaternion, one wave per row like the others.  The map preserves volume: the log-det written is zero, and
// an accumulated log-det is left as it is.
template <typename T, bool INVERSE>
__global__ void __launch_bounds__(256) quatprod_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ params,
                                                       int64_t ldp, T* __restrict__ y, int64_t ldy, T* __restrict__ ldj,
                                                       int accumulate, int B, int D) {
    const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const int nq = D / 4;
    const T* xr = x + (int64_t)b * ldx;
    const T* pr = params + (int64_t)b * ldp;
    T* yr = y + (int64_t)b * ldy;
    const bool px = quat_aligned<T>(xr), pp = quat_aligned<T>(pr), py = quat_aligned<T>(yr);      // wave uniform
    for (int q = lane; q < nq; q += 64) {
        double xv[4], pv[4], yv[4];
        quat_load(xr, q, px, xv);
        quat_load(pr, q, pp, pv);
        quatprod_element<T, INVERSE>(xv, pv, yv);
        quat_store(yr, q, py, yv);
    }
    if (ldj && !accumulate && lane == 0) ldj[b] = (T)0;
}

// ---------------------------------------------------------------- SOS polynomial (sos.py:198-265; sos.h)
// K runtime; the log of the sum-of-squares derivative per element, summed in fp64 with the wave butterfly like the others.
template <typename T>
__global__ void __launch_bounds__(256) sos_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ params,
                                                  tfep_param_layout L, int K, T* __restrict__ y, int64_t ldy,
                                                  T* __restrict__ ldj, int accumulate, int B, int D) {
    const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const T* xr = x + (int64_t)b * ldx;
    const T* pr = params + (int64_t)b * L.ld;
    T* yr = y + (int64_t)b * ldy;
    double acc = 0.0;
    for (int f = lane; f < D; f += 64) {
        const T* pf = pr + f * L.stride_f;
        T d;
        yr[f] = sos_element<0, T>(K, [&](int p) { return pf[p * L.stride_p]; }, xr[f], &d);
        acc += (double)log(d);
    }
    acc = wave_sum(acc);
    if (ldj) store_ldj(ldj, b, acc, accumulate);
}

// VJP: every parameter of every feature and the direct g_x; no log-det cotangent (non-differentiable in the reference).
template <typename T>
__global__ void __launch_bounds__(256) sos_backward_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ params,
                                                           tfep_param_layout L, int K, const T* __restrict__ gy, int64_t ldgy,
                                                           T* __restrict__ gparams, tfep_param_layout GL,
                                                           T* __restrict__ gx, int64_t ldgx, int B, int D) {
    const int b = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (b >= B) return;
    const int lane = threadIdx.x & 63;
    const T* pr = params + (int64_t)b * L.ld;
    T* gpr = gparams + (int64_t)b * GL.ld;
    for (int f = lane; f < D; f += 64) {
        const T* pf = pr + f * L.stride_f;
        T* gpf = gpr + f * GL.stride_f;
        gx[(int64_t)b * ldgx + f] = sos_vjp_element<T>(
            K, [&](int p) { return pf[p * L.stride_p]; }, [&](int p, T v) { gpf[p * GL.stride_p] = v; },
            x[(int64_t)b * ldx + f], gy[(int64_t)b * ldgy + f]);
    }
}

// ---------------------------------------------------------------- column gather / scatter
template <typename T, bool SCATTER>
__global__ void __launch_bounds__(256) columns_kernel(const T* __restrict__ src, int64_t lds, const int32_t* __restrict__ idx,
                                                      int n_idx, T* __restrict__ dst, int64_t ldd, int B) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * n_idx) return;
    const int b = (int)(i / n_idx), j = (int)(i % n_idx);
    if (SCATTER)
        dst[(int64_t)b * ldd + idx[j]] = src[(int64_t)b * lds + j];
    else
        dst[(int64_t)b * ldd + j] = src[(int64_t)b * lds + idx[j]];
}

static inline unsigned row_blocks(int B) { return (unsigned)((B + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK); }

template <bool INVERSE>
static int launch_spline(const float* x, int64_t ldx, const float* params, tfep_param_layout L,
                         const tfep_spline_desc* desc, float* y, int64_t ldy, float* ldj, int accumulate,
                         int B, int D, void* stream) {
    SplineArgs a;
    int rc = make_spline_args(desc, &a);
    if (rc) return rc;
    TFEP_REQUIRE(B >= 0 && D >= 0, "spline: negative size");
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(x && params && y, "spline: x/params/y must be non-NULL");
    hipStream_t s = (hipStream_t)stream;
    if (a.f.K <= 8)
        spline_kernel<8, INVERSE><<<row_blocks(B), 256, 0, s>>>(x, ldx, params, L, a, y, ldy, ldj, accumulate, B, D);
    else if (a.f.K <= 16)
        spline_kernel<16, INVERSE><<<row_blocks(B), 256, 0, s>>>(x, ldx, params, L, a, y, ldy, ldj, accumulate, B, D);
    else
        spline_kernel<32, INVERSE><<<row_blocks(B), 256, 0, s>>>(x, ldx, params, L, a, y, ldy, ldj, accumulate, B, D);
    return check_launch("spline_kernel");
}

// Launchers shared by the float32 entry points and their _f64 twins; `who` prefixes the error messages.
template <typename T, bool INVERSE>
static int launch_affine(const char* who, const T* x, int64_t ldx, const T* params, tfep_param_layout L, T* y, int64_t ldy,
                         T* ldj, int accumulate, int B, int D, void* stream) {
    TFEP_REQUIRE(B >= 0 && D >= 0, "%s: negative size", who);
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(x && params && y, "%s: x/params/y must be non-NULL", who);
    affine_kernel<T, INVERSE><<<row_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, params, L, y, ldy, ldj, accumulate, B, D);
    return check_launch("affine_kernel");
}

template <typename T>
static int launch_sos(const char* who, const T* x, int64_t ldx, const T* params, tfep_param_layout L, int K, T* y,
                      int64_t ldy, T* ldj, int accumulate, int B, int D, void* stream) {
    TFEP_REQUIRE(B >= 0 && D >= 0, "%s: negative size", who);
    TFEP_REQUIRE(K >= 1, "%s: n_polynomials=%d must be positive", who, K);
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(x && params && y, "%s: x/params/y must be non-NULL", who);
    sos_kernel<T><<<row_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, params, L, K, y, ldy, ldj, accumulate, B, D);
    return check_launch("sos_kernel");
}

template <typename T>
static int launch_moebius(const char* who, const T* x, int64_t ldx, const T* params, int64_t ldp, int dimension, double max_radius,
                          int unit_sphere, int sign, T* y, int64_t ldy, T* ldj, int accumulate, int B, int D, void* stream) {
    TFEP_REQUIRE(B == 0 || (x && params && y), "%s: x/params/y must be non-NULL", who);
    TFEP_REQUIRE(dimension >= 1 && dimension <= MOEBIUS_MAX_DIM, "%s: dimension=%d unsupported (1..%d)", who, dimension,
                 MOEBIUS_MAX_DIM);
    TFEP_REQUIRE(D % dimension == 0, "%s: n_features=%d is not a multiple of dimension=%d", who, D, dimension);
    TFEP_REQUIRE(sign == 1 || sign == -1, "%s: sign must be +1 or -1", who);
    if (B == 0) return TFEP_OK;
    auto kernel = dimension == 2 ? moebius_kernel<T, 2> : dimension == 3 ? moebius_kernel<T, 3> : moebius_kernel<T, 0>;
    kernel<<<row_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, params, ldp, dimension, max_radius, unit_sphere, (T)sign, y,
                                                           ldy, ldj, accumulate, B, D, nullptr, 0, nullptr);
    return check_launch("moebius_kernel");
}

template <typename T, bool INVERSE>
static int launch_symmoebius_dir(const T* x, int64_t ldx, const T* params, int64_t ldp, int dim, double max_radius, T* y,
                                 int64_t ldy, T* ldj, int accumulate, int B, int D, hipStream_t s) {
    auto kernel = dim == 2 ? symmoebius_kernel<T, 2, INVERSE> : dim == 3 ? symmoebius_kernel<T, 3, INVERSE>
                : dim == 4 ? symmoebius_kernel<T, 4, INVERSE> : symmoebius_kernel<T, 0, INVERSE>;
    kernel<<<row_blocks(B), 256, 0, s>>>(x, ldx, params, ldp, dim, max_radius, y, ldy, ldj, accumulate, B, D);
    return check_launch("symmoebius_kernel");
}

template <typename T>
static int launch_symmoebius(const char* who, const T* x, int64_t ldx, const T* params, int64_t ldp, int dimension,
                             double max_radius, int inverse, T* y, int64_t ldy, T* ldj, int accumulate, int B, int D,
                             void* stream) {
    TFEP_REQUIRE(B >= 0 && D >= 0, "%s: negative size", who);
    TFEP_REQUIRE(dimension >= 2 && dimension <= MOEBIUS_MAX_DIM, "%s: dimension=%d unsupported (2..%d)", who, dimension,
                 MOEBIUS_MAX_DIM);
    TFEP_REQUIRE(D % dimension == 0, "%s: n_features=%d is not a multiple of dimension=%d", who, D, dimension);
    TFEP_REQUIRE(max_radius > 0.0 && max_radius < 1.0, "%s: max_radius=%g must lie in (0, 1)", who, max_radius);
    TFEP_REQUIRE(inverse == 0 || inverse == 1, "%s: inverse must be 0 or 1", who);
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(D == 0 || (x && params && y), "%s: x/params/y must be non-NULL", who);
    TFEP_REQUIRE(ldx >= D && ldp >= D && ldy >= D, "%s: a row stride is shorter than n_features=%d", who, D);
    return inverse ? launch_symmoebius_dir<T, true>(x, ldx, params, ldp, dimension, max_radius, y, ldy, ldj, accumulate, B, D,
                                                    (hipStream_t)stream)
                   : launch_symmoebius_dir<T, false>(x, ldx, params, ldp, dimension, max_radius, y, ldy, ldj, accumulate, B, D,
                                                     (hipStream_t)stream);
}

template <typename T>
static int launch_quatprod(const char* who, const T* x, int64_t ldx, const T* params, int64_t ldp, int inverse, T* y,
                           int64_t ldy, T* ldj, int accumulate, int B, int D, void* stream) {
    TFEP_REQUIRE(B >= 0 && D >= 0, "%s: negative size", who);
    TFEP_REQUIRE(D % 4 == 0, "%s: n_features=%d is not a multiple of 4 (quaternions)", who, D);
    TFEP_REQUIRE(inverse == 0 || inverse == 1, "%s: inverse must be 0 or 1", who);
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(D == 0 || (x && params && y), "%s: x/params/y must be non-NULL", who);
    TFEP_REQUIRE(ldx >= D && ldp >= D && ldy >= D, "%s: a row stride is shorter than n_features=%d", who, D);
    auto kernel = inverse ? quatprod_kernel<T, true> : quatprod_kernel<T, false>;
    kernel<<<row_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, params, ldp, y, ldy, ldj, accumulate, B, D);
    return check_launch("quatprod_kernel");
}

template <typename T>
static int launch_sos_backward(const char* who, const T* x, int64_t ldx, const T* params, tfep_param_layout L, int K,
                               const T* gy, int64_t ldgy, T* gparams, tfep_param_layout GL, T* gx, int64_t ldgx, int B, int D,
                               void* stream) {
    TFEP_REQUIRE(B >= 0 && D >= 0, "%s: negative size", who);
    TFEP_REQUIRE(K >= 1, "%s: n_polynomials=%d must be positive", who, K);
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(x && params && gy && gparams && gx, "%s: NULL pointer", who);
    sos_backward_kernel<T><<<row_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, params, L, K, gy, ldgy, gparams, GL, gx,
                                                                            ldgx, B, D);
    return check_launch("sos_backward_kernel");
}

template <typename T>
static int launch_volpres(const char* who, const T* x, int64_t ldx, const T* shift, int64_t ldp, const int32_t* periodic_mask,
                          T lower, T upper, int sign, T* y, int64_t ldy, int B, int D, void* stream) {
    TFEP_REQUIRE(sign == 1 || sign == -1, "%s: sign must be +1 or -1", who);
    TFEP_REQUIRE(B >= 0 && D >= 0, "%s: negative size", who);
    const int64_t n = (int64_t)B * D;
    if (n == 0) return TFEP_OK;
    TFEP_REQUIRE(x && shift && y, "%s: x/shift/y must be non-NULL", who);
    volpres_kernel<T><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, ldx, shift, ldp, periodic_mask, lower,
                                                                                     upper, (T)sign, y, ldy, B, D);
    return check_launch("volpres_kernel");
}

template <typename T>
static int launch_periodic_embedding(const char* who, const T* x, int64_t ldx, const int32_t* pidx, int n_per,
                                     const int32_t* nidx, int n_non, T lower, T upper, T* out, int64_t ldo, int B,
                                     void* stream) {
    TFEP_REQUIRE(B >= 0 && n_per >= 0 && n_non >= 0, "%s: negative size", who);
    TFEP_REQUIRE(B == 0 || (x && out), "%s: x/out must be non-NULL", who);
    TFEP_REQUIRE(n_per == 0 || pidx, "%s: periodic_indices is NULL", who);
    TFEP_REQUIRE(n_non == 0 || nidx, "%s: nonperiodic_indices is NULL", who);
    TFEP_REQUIRE(upper != lower, "%s: empty period", who);
    const int64_t n = (int64_t)B * (n_per + n_non);
    if (n == 0) return TFEP_OK;
    periodic_embedding_kernel<T, false><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        x, ldx, pidx, n_per, nidx, n_non, lower, embedding_scale(lower, upper), nullptr, 0, out, ldo, B);
    return check_launch("periodic_embedding_kernel");
}

template <typename T, bool SCATTER>
static int launch_columns(const char* who, const T* src, int64_t lds, const int32_t* idx, int n_idx, T* dst, int64_t ldd,
                          int B, void* stream) {
    TFEP_REQUIRE(B >= 0 && n_idx >= 0, "%s: negative size", who);
    const int64_t n = (int64_t)B * n_idx;
    if (n == 0) return TFEP_OK;
    TFEP_REQUIRE(src && dst && idx, "%s: NULL pointer", who);
    columns_kernel<T, SCATTER><<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(src, lds, idx, n_idx, dst, ldd, B);
    return check_launch(who);
}

}  // namespace tfep

using namespace tfep;

extern "C" {

int tfep_hip_abi_version(void) { return TFEP_HIP_ABI_VERSION; }
const char* tfep_last_error(void) { return last_error().c_str(); }

int tfep_affine_forward(const float* x, int64_t ldx, const float* params, tfep_param_layout layout, float* y,
                        int64_t ldy, float* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_affine<float, false>("affine", x, ldx, params, layout, y, ldy, log_det_J, accumulate, B, D, stream);
}

int tfep_affine_inverse(const float* y, int64_t ldy, const float* params, tfep_param_layout layout, float* x,
                        int64_t ldx, float* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_affine<float, true>("affine", y, ldy, params, layout, x, ldx, log_det_J, accumulate, B, D, stream);
}

int tfep_affine_forward_f64(const double* x, int64_t ldx, const double* params, tfep_param_layout layout, double* y,
                            int64_t ldy, double* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_affine<double, false>("affine_f64", x, ldx, params, layout, y, ldy, log_det_J, accumulate, B, D, stream);
}

int tfep_affine_inverse_f64(const double* y, int64_t ldy, const double* params, tfep_param_layout layout, double* x,
                            int64_t ldx, double* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_affine<double, true>("affine_f64", y, ldy, params, layout, x, ldx, log_det_J, accumulate, B, D, stream);
}

int tfep_sos_forward(const float* x, int64_t ldx, const float* params, tfep_param_layout layout, int n_polynomials,
                     float* y, int64_t ldy, float* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_sos("sos", x, ldx, params, layout, n_polynomials, y, ldy, log_det_J, accumulate, B, D, stream);
}

int tfep_sos_forward_f64(const double* x, int64_t ldx, const double* params, tfep_param_layout layout, int n_polynomials,
                         double* y, int64_t ldy, double* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_sos("sos_f64", x, ldx, params, layout, n_polynomials, y, ldy, log_det_J, accumulate, B, D, stream);
}

int tfep_sos_backward(const float* x, int64_t ldx, const float* params, tfep_param_layout layout, int n_polynomials,
                      const float* gy, int64_t ldgy, float* gparams, tfep_param_layout glayout, float* gx, int64_t ldgx,
                      int B, int D, void* stream) {
    return launch_sos_backward("sos_backward", x, ldx, params, layout, n_polynomials, gy, ldgy, gparams, glayout, gx, ldgx,
                               B, D, stream);
}

int tfep_sos_backward_f64(const double* x, int64_t ldx, const double* params, tfep_param_layout layout, int n_polynomials,
                          const double* gy, int64_t ldgy, double* gparams, tfep_param_layout glayout, double* gx,
                          int64_t ldgx, int B, int D, void* stream) {
    return launch_sos_backward("sos_backward_f64", x, ldx, params, layout, n_polynomials, gy, ldgy, gparams, glayout, gx,
                               ldgx, B, D, stream);
}

int tfep_volume_preserving_shift(const float* x, int64_t ldx, const float* shift, int64_t ldp,
                                 const int32_t* periodic_mask, float lower, float upper, int sign, float* y,
                                 int64_t ldy, int B, int D, void* stream) {
    return launch_volpres("volume_preserving_shift", x, ldx, shift, ldp, periodic_mask, lower, upper, sign, y, ldy, B, D,
                          stream);
}

int tfep_volume_preserving_shift_f64(const double* x, int64_t ldx, const double* shift, int64_t ldp,
                                     const int32_t* periodic_mask, double lower, double upper, int sign, double* y,
                                     int64_t ldy, int B, int D, void* stream) {
    return launch_volpres("volume_preserving_shift_f64", x, ldx, shift, ldp, periodic_mask, lower, upper, sign, y, ldy, B, D,
                          stream);
}

int tfep_spline_n_parameters_per_feature(const tfep_spline_desc* d) {
    if (!d) return fail(TFEP_ERR_INVALID_ARGUMENT, "spline descriptor is NULL");
    return spline_n_params(d->n_bins, d->circular != 0, d->identity_boundary_slopes != 0, d->learn_lower_bound != 0,
                           d->learn_upper_bound != 0);
}

int tfep_spline_forward(const float* x, int64_t ldx, const float* params, tfep_param_layout layout,
                        const tfep_spline_desc* desc, float* y, int64_t ldy, float* log_det_J, int accumulate, int B,
                        int D, void* stream) {
    return launch_spline<false>(x, ldx, params, layout, desc, y, ldy, log_det_J, accumulate, B, D, stream);
}

int tfep_spline_inverse(const float* y, int64_t ldy, const float* params, tfep_param_layout layout,
                        const tfep_spline_desc* desc, float* x, int64_t ldx, float* log_det_J, int accumulate, int B,
                        int D, void* stream) {
    return launch_spline<true>(y, ldy, params, layout, desc, x, ldx, log_det_J, accumulate, B, D, stream);
}

int tfep_moebius_forward(const float* x, int64_t ldx, const float* params, int64_t ldp, int dimension,
                         double max_radius, int unit_sphere, int sign, float* y, int64_t ldy, float* log_det_J,
                         int accumulate, int B, int D, void* stream) {
    return launch_moebius("moebius", x, ldx, params, ldp, dimension, max_radius, unit_sphere, sign, y, ldy, log_det_J,
                          accumulate, B, D, stream);
}

int tfep_moebius_forward_f64(const double* x, int64_t ldx, const double* params, int64_t ldp, int dimension,
                             double max_radius, int unit_sphere, int sign, double* y, int64_t ldy, double* log_det_J,
                             int accumulate, int B, int D, void* stream) {
    return launch_moebius("moebius_f64", x, ldx, params, ldp, dimension, max_radius, unit_sphere, sign, y, ldy, log_det_J,
                          accumulate, B, D, stream);
}

int tfep_symmetrized_moebius(const float* x, int64_t ldx, const float* params, int64_t ldp, int dimension, double max_radius,
                             int inverse, float* y, int64_t ldy, float* log_det_J, int accumulate, int B, int D,
                             void* stream) {
    return launch_symmoebius("symmetrized_moebius", x, ldx, params, ldp, dimension, max_radius, inverse, y, ldy, log_det_J,
                             accumulate, B, D, stream);
}

int tfep_symmetrized_moebius_f64(const double* x, int64_t ldx, const double* params, int64_t ldp, int dimension,
                                 double max_radius, int inverse, double* y, int64_t ldy, double* log_det_J, int accumulate,
                                 int B, int D, void* stream) {
    return launch_symmoebius("symmetrized_moebius_f64", x, ldx, params, ldp, dimension, max_radius, inverse, y, ldy,
                             log_det_J, accumulate, B, D, stream);
}

int tfep_quaternion_product(const float* x, int64_t ldx, const float* params, int64_t ldp, int inverse, float* y,
                            int64_t ldy, float* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_quatprod("quaternion_product", x, ldx, params, ldp, inverse, y, ldy, log_det_J, accumulate, B, D, stream);
}

int tfep_quaternion_product_f64(const double* x, int64_t ldx, const double* params, int64_t ldp, int inverse, double* y,
                                int64_t ldy, double* log_det_J, int accumulate, int B, int D, void* stream) {
    return launch_quatprod("quaternion_product_f64", x, ldx, params, ldp, inverse, y, ldy, log_det_J, accumulate, B, D,
                           stream);
}

int tfep_moebius_forward_split_out(const float* x, int64_t ldx, const float* params, int64_t ldp, double max_radius, float* y, int64_t ldy,
                                   float* log_det_J, int accumulate, void* y_split, int64_t ld_split, float* y_inv_scale, int B, int D,
                                   void* stream) {
    TFEP_REQUIRE(B == 0 || (x && params && y && y_split && y_inv_scale), "moebius_split_out: NULL pointer");
    TFEP_REQUIRE(D % 2 == 0 && D % 8 == 0, "moebius_split_out: n_features=%d must be a multiple of 8 (whole split groups of 2-vectors)", D);
    TFEP_REQUIRE(ld_split >= D && ld_split % 8 == 0 && ((uintptr_t)y_split & 15) == 0, "moebius_split_out: split rows too short / not aligned");
    TFEP_REQUIRE(((uintptr_t)x & 7) == 0 && ((uintptr_t)params & 7) == 0 && ((uintptr_t)y & 7) == 0 && ldx % 2 == 0 && ldp % 2 == 0 && ldy % 2 == 0,
                 "moebius_split_out: x, params and y rows must start on 8-byte boundaries");
    if (B == 0) return TFEP_OK;
    moebius_kernel<float, 2><<<row_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, params, ldp, 2, max_radius, 1, 1.0f, y, ldy, log_det_J, accumulate, B,
                                                                      D, (uint32_t*)y_split, ld_split, y_inv_scale);
    return check_launch("moebius_kernel");
}

int tfep_periodic_embedding(const float* x, int64_t ldx, const int32_t* periodic_indices, int n_periodic,
                            const int32_t* nonperiodic_indices, int n_nonperiodic, float lower, float upper,
                            float* out, int64_t ldo, int B, void* stream) {
    return launch_periodic_embedding("periodic_embedding", x, ldx, periodic_indices, n_periodic, nonperiodic_indices,
                                     n_nonperiodic, lower, upper, out, ldo, B, stream);
}

int tfep_periodic_embedding_f64(const double* x, int64_t ldx, const int32_t* periodic_indices, int n_periodic,
                                const int32_t* nonperiodic_indices, int n_nonperiodic, double lower, double upper,
                                double* out, int64_t ldo, int B, void* stream) {
    return launch_periodic_embedding("periodic_embedding_f64", x, ldx, periodic_indices, n_periodic, nonperiodic_indices,
                                     n_nonperiodic, lower, upper, out, ldo, B, stream);
}

int tfep_gather_columns(const float* src, int64_t lds, const int32_t* idx, int n_idx, float* dst, int64_t ldd, int B,
                        void* stream) {
    return launch_columns<float, false>("gather_columns", src, lds, idx, n_idx, dst, ldd, B, stream);
}

int tfep_scatter_columns(const float* src, int64_t lds, const int32_t* idx, int n_idx, float* dst, int64_t ldd, int B,
                         void* stream) {
    return launch_columns<float, true>("scatter_columns", src, lds, idx, n_idx, dst, ldd, B, stream);
}

int tfep_gather_columns_f64(const double* src, int64_t lds, const int32_t* idx, int n_idx, double* dst, int64_t ldd, int B,
                            void* stream) {
    return launch_columns<double, false>("gather_columns_f64", src, lds, idx, n_idx, dst, ldd, B, stream);
}

int tfep_scatter_columns_f64(const double* src, int64_t lds, const int32_t* idx, int n_idx, double* dst, int64_t ldd, int B,
                             void* stream) {
    return launch_columns<double, true>("scatter_columns_f64", src, lds, idx, n_idx, dst, ldd, B, stream);
}

}  // extern "C"
