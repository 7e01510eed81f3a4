// Device helpers shared by the EGNN translation units (egnn.hip, egnn_param_grad.hip): the packed-layer layout, the
// transposed MFMA chain products (exact fp32 and split-f16), the fast transcendental forms and the SiLU tiles.
#pragma once
#include "common.h"
#include <type_traits>

namespace tfep {
namespace {

using f4 = __attribute__((ext_vector_type(4))) float;

#ifndef TFEP_EGNN_FAST_GEOM
#define TFEP_EGNN_FAST_GEOM 1
#endif
constexpr int EDGE_WAVES = 8;            // waves per workgroup of the edge kernel (2 per SIMD)
constexpr int NODE_WAVES = 4;

__host__ __device__ inline int64_t img_floats(int nt) { return (int64_t)nt * nt * 256; }       // (16 nt)^2
// layout of a packed layer (floats)
struct PackedLayout {
    int64_t w1c, w2, x1, b2, d1, wa, x2, mu, gamma, scal, u1a, u1b, u2, c1, c2, w1a, w1b, b1;
    int64_t w1cT, w2T, x1T, w1aT, w1bT, u2T, u1aT, u1bT;        // transposed fp32 images (reverse pass)
    int64_t s_w1c, s_w2, s_x1, s_w1cT, s_w2T, s_x1T, total;     // split-f16 images, forward and transposed
};
// A split-f16 operand image: per (row tile tp, pair of k tiles T) 64 lanes x 8 halves -- the "hi" image (fp16 of the
// scaled weight) followed by the "lo" image (fp16 of the residual); in floats of the packed buffer.
__host__ __device__ inline int64_t split_img_floats(int nt) { return (int64_t)nt * ((nt + 1) / 2) * 64 * 8; }
__host__ __device__ inline PackedLayout packed_layout(int nt) {
    PackedLayout L;
    const int64_t I = img_floats(nt), V = 16 * nt;
    int64_t o = 0;
    L.w1c = o; o += I; L.w2 = o; o += I; L.x1 = o; o += I;
    L.b2 = o; o += V; L.d1 = o; o += V; L.wa = o; o += V; L.x2 = o; o += V; L.mu = o; o += V; L.gamma = o; o += V;
    L.scal = o; o += 4;
    L.u1a = o; o += I; L.u1b = o; o += I; L.u2 = o; o += I; L.c1 = o; o += V; L.c2 = o; o += V;
    L.w1a = o; o += I; L.w1b = o; o += I; L.b1 = o; o += V;
    L.w1cT = o; o += I; L.w2T = o; o += I; L.x1T = o; o += I;
    L.w1aT = o; o += I; L.w1bT = o; o += I; L.u2T = o; o += I; L.u1aT = o; o += I; L.u1bT = o; o += I;
    const int64_t SI = split_img_floats(nt);
    L.s_w1c = o; o += SI; L.s_w2 = o; o += SI; L.s_x1 = o; o += SI;
    L.s_w1cT = o; o += SI; L.s_w2T = o; o += SI; L.s_x1T = o; o += SI;
    L.total = o;
    return L;
}
constexpr int EDGE_CONST_VECS = 6;       // b2, d1, wa, x2, mu, gamma follow the three edge images contiguously

__device__ inline f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// acc[tp] += W[tp][:] x  (and the same for the tangent dx with the SAME weight fragment), W as a lane-linear LDS image
template <int NT, bool TAN>
__device__ inline void chain_gemm(const f4* __restrict__ img, const f4 (&x)[NT], const f4 (&dx)[NT], f4 (&acc)[NT],
                                  f4 (&dacc)[NT], int lane) {
#pragma unroll
    for (int tp = 0; tp < NT; ++tp) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const f4 a = img[(tp * NT + t) * 64 + lane];
            acc[tp] = mfma4(a.x, x[t].x, acc[tp]);
            if (TAN) dacc[tp] = mfma4(a.x, dx[t].x, dacc[tp]);
            acc[tp] = mfma4(a.y, x[t].y, acc[tp]);
            if (TAN) dacc[tp] = mfma4(a.y, dx[t].y, dacc[tp]);
            acc[tp] = mfma4(a.z, x[t].z, acc[tp]);
            if (TAN) dacc[tp] = mfma4(a.z, dx[t].z, dacc[tp]);
            acc[tp] = mfma4(a.w, x[t].w, acc[tp]);
            if (TAN) dacc[tp] = mfma4(a.w, dx[t].w, dacc[tp]);
        }
    }
}

using h8 = __attribute__((ext_vector_type(8))) _Float16;
constexpr float SPLIT_X_SCALE = 16.0f;       // activations enter the split products as x * 16: |x| < 4094 fits fp16

// Inline-asm MFMAs on purpose: with the builtin, hipcc (ROCm 7.2) gave destination and SrcC different registers and re-used the
// SrcC registers of the last products two wait states later while those MFMAs were still in flight -- the tangent of the
// split chain came out different from run to run (caught by the bitwise row-independence check of
// tests/test_gpu_continuous.py::test_cfg5_full_size_properties; the value tests against the goldens at 1e-5 passed).
// Accumulating in place there is no separate SrcC to clobber; A / B are read when the instruction issues.  hipcc pads nothing
// around an asm statement: the chain puts the wait states before the first product and after the last itself.

// ---- the forward edge kernel's version of the split product: operands arrive PRE-SCALED (the producers fold the x 16 into
// arithmetic they do anyway), every fp32 -> (hi, lo) pair costs three vector instructions, and the first product of an
// accumulator takes the inline constant 0 as SrcC (no zero fill of 2 x 16 NT registers per product).
using u4 = __attribute__((ext_vector_type(4))) uint32_t;

// (a, b) -> hi = (fp16(a), fp16(b)), lo = (fp16(a - hi_a), fp16(b - hi_b)); v_fma_mix reads the fp16 high half directly
// (op_sel_hi marks src2 as fp16, op_sel picks its upper half), so there is no conversion back and no subtraction.
__device__ inline void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
    asm("v_cvt_pk_f16_f32 %0, %2, %3\n\t"
        "v_fma_mixlo_f16 %1, %2, 1.0, -%0 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %1, %3, 1.0, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(hi), "=&v"(lo) : "v"(a), "v"(b));
}
__device__ inline void mfma16_first(f4& acc, const u4& a, const u4& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "v"(b));
}
__device__ inline void mfma16_next(f4& acc, const u4& a, const u4& b) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
template <int NT>
__device__ inline void split_tiles(const f4 (&x)[NT], u4 (&xh)[(NT + 1) / 2], u4 (&xl)[(NT + 1) / 2]) {
#pragma unroll
    for (int T = 0; T < (NT + 1) / 2; ++T) {
        uint32_t h0, l0, h1, l1, h2 = 0u, l2 = 0u, h3 = 0u, l3 = 0u;
        split_pair(x[2 * T].x, x[2 * T].y, h0, l0);
        split_pair(x[2 * T].z, x[2 * T].w, h1, l1);
        if (2 * T + 1 < NT) {
            const f4& b = x[(2 * T + 1 < NT) ? 2 * T + 1 : 0];
            split_pair(b.x, b.y, h2, l2);
            split_pair(b.z, b.w, h3, l3);
        }
        xh[T] = u4{h0, h1, h2, h3};
        xl[T] = u4{l0, l1, l2, l3};
    }
}
// LDS byte address of a pointer into shared memory (the low 32 bits of a flat address in the LDS aperture are the offset)
__device__ inline uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)p; }
// the hi / lo weight fragments of one (row tile, k-tile pair) group, issued without waiting: the compiler does not know
// these loads (nor count them), lds_wait_pair before the first use is what orders them
template <int OFF_H, int OFF_L>
__device__ inline void lds_read_pair(u4& wh, u4& wl, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %2 offset:%3\n\tds_read_b128 %1, %2 offset:%4"
                 : "=&v"(wh), "=&v"(wl) : "v"(addr), "i"(OFF_H), "i"(OFF_L));
}
template <int N>
__device__ inline void lds_wait_pair(u4& wh, u4& wl) {
    asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(wh), "+v"(wl) : "i"(N));
}
template <int I, int N, class F>
__device__ inline void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// acc = W x, dacc = W dx for pre-scaled x, dx (acc / dacc need no initialisation).  The weight fragments are read one
// group AHEAD of the products that use them (two register sets, counted lgkmcnt): left to the compiler every group was
// "two ds_read_b128, wait, six MFMAs" -- 24 exposed LDS round trips per source with the matrix pipe idle behind each.
template <int NT, bool TAN>
__device__ inline void chain_gemm_split_pre(const u4* __restrict__ img, const f4 (&x)[NT], const f4 (&dx)[NT],
                                            f4 (&acc)[NT], f4 (&dacc)[NT], int lane) {
    constexpr int NT2 = (NT + 1) / 2, G = NT * NT2, LO = NT * NT2 * 64 * 16;
    static_assert(LO + G * 1024 < 65536, "ds_read offset field");
    u4 xh[NT2], xl[NT2], dxh[NT2], dxl[NT2];
    split_tiles<NT>(x, xh, xl);
    if (TAN) split_tiles<NT>(dx, dxh, dxl);
    const uint32_t base = lds_addr(img) + (uint32_t)lane * 16u;
    // the halves come from VALU instructions inside asm statements: keep them ahead of the first product and give the
    // VALU -> MFMA operand hazard its wait states by hand (hipcc pads nothing around asm)
#pragma unroll
    for (int T = 0; T < NT2; ++T) {
        asm volatile("" : "+v"(xh[T]), "+v"(xl[T]));
        if (TAN) asm volatile("" : "+v"(dxh[T]), "+v"(dxl[T]));
    }
    __builtin_amdgcn_sched_barrier(0);
    u4 wh[2], wl[2];
    lds_read_pair<0, LO>(wh[0], wl[0], base);
    static_for<0, G>([&](auto gc) {
        constexpr int g = decltype(gc)::value, tp = g / NT2, T = g % NT2, cur = g & 1;
        if constexpr (g + 1 < G) lds_read_pair<(g + 1) * 1024, LO + (g + 1) * 1024>(wh[cur ^ 1], wl[cur ^ 1], base);
        lds_wait_pair<(g + 1 < G) ? 2 : 0>(wh[cur], wl[cur]);
        if (T == 0) {
            mfma16_first(acc[tp], wh[cur], xh[T]);
            if (TAN) mfma16_first(dacc[tp], wh[cur], dxh[T]);
        } else {
            mfma16_next(acc[tp], wh[cur], xh[T]);
            if (TAN) mfma16_next(dacc[tp], wh[cur], dxh[T]);
        }
        mfma16_next(acc[tp], wl[cur], xh[T]);
        if (TAN) mfma16_next(dacc[tp], wl[cur], dxh[T]);
        mfma16_next(acc[tp], wh[cur], xl[T]);
        if (TAN) mfma16_next(dacc[tp], wh[cur], dxl[T]);
    });
    // leave the matrix pipe's result latency behind before anything reads the accumulators
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// The same product for UNSCALED operands (the reverse-pass kernel: cotangents have no producer to fold the factor into):
// one multiply per element in front of the pre-scaled chain.  acc / dacc need no initialisation; the caller un-scales
// (weights carry a per-matrix power of two, activations SPLIT_X_SCALE).
template <int NT, bool TAN>
__device__ inline void chain_gemm_split(const h8* __restrict__ img, const f4 (&x)[NT], const f4 (&dx)[NT], f4 (&acc)[NT],
                                        f4 (&dacc)[NT], int lane) {
    f4 xs[NT], dxs[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xs[t][r] = x[t][r] * SPLIT_X_SCALE;
            if (TAN) dxs[t][r] = dx[t][r] * SPLIT_X_SCALE;
        }
    }
    chain_gemm_split_pre<NT, TAN>(reinterpret_cast<const u4*>(img), xs, dxs, acc, dacc, lane);
}

// exp and 1/x on the transcendental unit (v_exp_f32 / v_rcp_f32, 1 ulp each; the argument scaling x * log2(e) adds
// |x| 6e-8 of relative error): the library expf / IEEE division cost ~10 instructions each, and the edge kernel evaluates
// 64 of each per 16 edges and layer.  Measured against the float64 goldens the velocities keep their 6e-7 relative error.
__device__ inline float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ inline float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
// tanh on the same two instructions: 1 - 2 / (1 + e^{2x}) (absolute error ~2e-7: an exp and a reciprocal of 1 ulp each), and the odd
// series to x^5 below |x| = 0.1, where that form cancels (its remainder there: 17 x^7 / 315 < 6e-9).  The library tanhf() is ~40
// instructions, once per edge and layer, on a kernel bound by its vector instructions (tanh'(x) = 1 - tanh^2 stays as it is).
__device__ inline float fast_tanh(float x) {
    const float ax = fminf(fabsf(x), 15.0f);
    const float big = 1.0f - 2.0f * fast_rcp(1.0f + fast_exp(2.0f * ax));
    const float x2 = ax * ax;
    const float small = ax * fmaf(x2, fmaf(x2, 2.0f / 15.0f, -1.0f / 3.0f), 1.0f);
    return copysignf(ax < 0.1f ? small : big, x);
}

// SiLU and its derivative (torch.nn.SiLU: x * sigmoid(x)), elementwise on a tile; dz <- silu'(z) dz, z <- silu(z)
template <int NT, bool TAN>
__device__ inline void silu_tile(f4 (&z)[NT], f4 (&dz)[NT]) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = z[t][r];
            const float sig = fast_rcp(1.0f + fast_exp(-v));
            const float sv = v * sig;
            z[t][r] = sv;
            if (TAN) dz[t][r] *= fmaf(sv, 1.0f - sig, sig);       // silu' = sig + silu (1 - sig)
        }
    }
}

// The same with the result scaled by XS = 2^LOG2S (the split products take their operands pre-scaled; XS = 1 is the plain
// SiLU at the same instruction count): z <- XS silu(z), dz <- XS silu'(z) dz.  XS sigma = 1 / (1/XS + exp(-z) / XS), the
// 1 / XS inside the exponent is an exact shift of the exp2 argument.
template <int NT, bool TAN, int LOG2S>
__device__ inline void silu_tile_scaled(f4 (&z)[NT], f4 (&dz)[NT]) {
    constexpr float IS = 1.0f / (float)(1 << LOG2S);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = z[t][r];
            const float e = __builtin_amdgcn_exp2f(fmaf(v, -1.44269504088896340736f, -(float)LOG2S));
            const float sig = fast_rcp(e + IS);                  // XS sigma(v)
            const float sv = v * sig;                            // XS silu(v)
            z[t][r] = sv;
            if (TAN) dz[t][r] *= fmaf(sv, fmaf(sig, -IS, 1.0f), sig);       // XS (sigma + silu (1 - sigma))
        }
    }
}

// sum over the four 16-lane groups of a wave (the lanes that hold the same edge column)
__device__ inline float sum_over_q(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

template <int NT>
__device__ inline void silu_keep(f4 (&z)[NT], f4 (&ds)[NT]) {          // z <- silu(z), ds <- silu'(z)
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = z[t][r];
            const float sig = fast_rcp(1.0f + fast_exp(-v));
            const float sv = v * sig;
            z[t][r] = sv;
            ds[t][r] = fmaf(sv, 1.0f - sig, sig);
        }
    }
}

}  // namespace
}  // namespace tfep
