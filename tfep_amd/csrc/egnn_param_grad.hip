// Parameter gradients of <g, velocity(t, x; theta)> of the EGNN dynamics: separate passes beside the reverse pass of
// egnn.hip (no existing kernel is touched), fed with the layer inputs the forward pass saved and the cotangents the
// reverse pass produced.  Notation: the reverse-pass comment of egnn.hip.
//
//   edge pass   recomputes the edge chain as the destination-owned reverse pass does (lanes = 16 destinations, the waves
//               of a workgroup walk the sources) and sums, over the live edges,
//                 g_z3 (x) m, g_z2 (x) silu(z1), g_z1 (x) rbf     the three F x F-sized sums: GEMMs whose K is the edges
//                 g_z3, g_s silu(z3), g_e a2, g_e, g_z2, g_rbf d rbf / d log gamma            the vector-sized sums
//   node pass   part 0: g_P (x) h', g_Q (x) h', sum g_Q (first linear of the next layer's message MLP, node columns);
//               part 1: update_h_mlp of this layer, its hidden activation recomputed (as egnn_node_bwd_kernel does)
//   reduce      adds the workgroups' partial sets in workgroup order in fp64, rounds once, un-pads into the parameter shapes
//
// The outer-product sums run on v_mfma_f32_16x16x4_f32 with exact fp32 operands.  The chain holds a tile as "lane = edge
// column, registers = 4 consecutive features"; a product over the edges needs "lane = (feature row, 4 consecutive
// edges)".  Each wave transposes through a private LDS tile [feature][TR_LD]: the k index of an MFMA is then the edge
// 4 (lane >> 4) + step for both operands (any order of k is the same sum up to fp32 grouping).
//
// Two summation levels.  One fp32 running sum over a workgroup's whole item list grows its rounding error with the list
// (measured: 35 000 terms per wave put a tensor 1.3e-6 from the sum of 34 short lists), so the fp32 register
// accumulators of the edge pass cover ONE item (a wave's share of the n sources of 16 destinations) and are then added,
// as doubles, into the workgroup's partial set in global memory: one wave after the other, a barrier between them --
// every entry receives the waves in a fixed order.  The item sums do not depend on the grid, the level above them is fp64 throughout (the reduce kernel adds
// the sets in workgroup order): grids of any size agree to fp64 rounding.  The node pass, whose lists are short (16 nodes
// per step), folds once at the end through LDS.  No atomics anywhere: results are bit-reproducible.
//
// Launch bounds: 256 threads (4 waves, one per SIMD, up to 512 registers each: the edge pass at the 64-wide tile keeps
// 3 x 64 accumulator registers beside the chain, the node pass 2 x 64 or 3 x 64).  LDS: the six operand images of the
// reverse pass (96 KiB at the 64-wide tile) + per-sample positions + 4 transposition tiles of 5 KiB; checked against
// gfx950's 160 KiB per workgroup before the launch.
#include "egnn_common.h"
#include <algorithm>

namespace tfep {
namespace {

constexpr int PG_WAVES = 4;
constexpr int TR_LD = 20;       // row stride (floats) of a transposition tile: 16-byte aligned rows, writes of a wave hit 64 banks

__host__ __device__ inline int64_t pg_partial_entries(int nt, int kind) {
    const int64_t fp = 16 * nt;
    return kind == 0 ? 3 * fp * fp + 6 * fp : (kind == 1 ? 2 * fp * fp + fp : 3 * fp * fp + 2 * fp);
}

// chain layout (lane (q, c): features 16 t + 4 q + r of column c) -> operand layout of a product over the columns:
// lane l gets [feature 16 t + (l & 15)][columns 4 (l >> 4) .. + 3].  One wave, its own tile; LDS operations of a wave
// complete in order, the fences keep the compiler from moving them across each other.
template <int NT>
__device__ inline void transpose_tile(float* __restrict__ tile, const f4 (&x)[NT], f4 (&out)[NT], int lane) {
    const int q = lane >> 4, c = lane & 15;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(16 * t + 4 * q + r) * TR_LD + c] = x[t][r];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int t = 0; t < NT; ++t) out[t] = *reinterpret_cast<const f4*>(tile + (16 * t + c) * TR_LD + 4 * q);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// acc[tf][tk] += sum over the 16 columns of  A[16 tf + .][column] B[16 tk + .][column]   (operands already transposed)
template <int NT>
__device__ inline void outer_acc(f4 (&acc)[NT][NT], const f4 (&A)[NT], const f4 (&B)[NT]) {
#pragma unroll
    for (int tf = 0; tf < NT; ++tf)
#pragma unroll
        for (int tk = 0; tk < NT; ++tk) {
            acc[tf][tk] = mfma4(A[tf].x, B[tk].x, acc[tf][tk]);
            acc[tf][tk] = mfma4(A[tf].y, B[tk].y, acc[tf][tk]);
            acc[tf][tk] = mfma4(A[tf].z, B[tk].z, acc[tf][tk]);
            acc[tf][tk] = mfma4(A[tf].w, B[tk].w, acc[tf][tk]);
        }
}
template <int NT>
__device__ inline void outer_product(float* tile, f4 (&acc)[NT][NT], const f4 (&a)[NT], const f4 (&b)[NT], int lane) {
    f4 A[NT], B[NT];
    transpose_tile<NT>(tile, a, A, lane);
    transpose_tile<NT>(tile, b, B, lane);
    outer_acc<NT>(acc, A, B);
}

// this wave's matrix accumulator (lane l, register r: row 16 tf + 4 (l >> 4) + r, column 16 tk + (l & 15)) into the
// workgroup's LDS image; `first`: store, else add
template <int NT>
__device__ inline void fold_matrix(float* __restrict__ red, const f4 (&acc)[NT][NT], int lane, bool first) {
    constexpr int FP = 16 * NT;
#pragma unroll
    for (int tf = 0; tf < NT; ++tf)
#pragma unroll
        for (int tk = 0; tk < NT; ++tk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* p = red + (16 * tf + 4 * (lane >> 4) + r) * FP + 16 * tk + (lane & 15);
                *p = first ? acc[tf][tk][r] : *p + acc[tf][tk][r];
            }
}
// a per-lane vector accumulator in the chain layout: summed over the 16 columns (fixed butterfly), then folded
template <int NT>
__device__ inline void fold_vector(float* __restrict__ red, const f4 (&acc)[NT], int lane, bool first) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[t][r];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            if ((lane & 15) == 0) {
                float* p = red + 16 * t + 4 * (lane >> 4) + r;
                *p = first ? v : *p + v;
            }
        }
}

// the same two folds into a partial set of doubles in global memory (the edge pass, once per item)
template <int NT>
__device__ inline void fold_matrix_f64(double* __restrict__ red, const f4 (&acc)[NT][NT], int lane, bool first) {
    constexpr int FP = 16 * NT;
#pragma unroll
    for (int tf = 0; tf < NT; ++tf) {
#pragma unroll
        for (int tk = 0; tk < NT; ++tk)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double* p = red + (16 * tf + 4 * (lane >> 4) + r) * FP + 16 * tk + (lane & 15);
                *p = first ? (double)acc[tf][tk][r] : *p + (double)acc[tf][tk][r];
            }
        // one row of tiles in flight at a time: the loads of a whole 64-wide matrix hoisted together (128 registers of
        // doubles beside the 272 accumulator registers) spilled
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int NT>
__device__ inline void fold_vector_f64(double* __restrict__ red, const f4 (&acc)[NT], int lane, bool first) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = acc[t][r];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            if ((lane & 15) == 0) {
                double* p = red + 16 * t + 4 * (lane >> 4) + r;
                *p = first ? (double)v : *p + (double)v;
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------
// edge pass
// ---------------------------------------------------------------------------------------------------------------
template <int NT, bool SPLIT>
__global__ __launch_bounds__(PG_WAVES * 64) void egnn_edge_param_grad_kernel(tfep_egnn_edge_param_grad_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int FP = 16 * NT;
    constexpr int IMG4 = SPLIT ? NT * ((NT + 1) / 2) * 64 * 2 : NT * NT * 64;
    constexpr int MAT = FP * FP;
    const PackedLayout L = packed_layout(NT);
    const int n = a.n_nodes;
    const int n_blk = (n + 15) / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, c = lane & 15;

    // ---- LDS: [3 forward images][3 transposed images][6 vectors][pos][gpos][lane Q][lane g_nm][transposition tiles]
    f4* const w_img = reinterpret_cast<f4*>(smem);
    float* const vecs = smem + 6 * IMG4 * 4;
    float* const s_pos = vecs + EDGE_CONST_VECS * FP;
    float* const s_gpos = s_pos + ((3 * n + 3) & ~3);
    f4* const s_lane = reinterpret_cast<f4*>(s_gpos + ((3 * n + 3) & ~3));
    f4* const s_gnm = s_lane + NT * 64;
    float* const tile = reinterpret_cast<float*>(s_gnm + NT * 64) + wave * FP * TR_LD;
    {
        const f4* src = reinterpret_cast<const f4*>(a.packed + (SPLIT ? L.s_w1c : L.w1c));
        for (int i = tid; i < 3 * IMG4; i += PG_WAVES * 64) w_img[i] = src[i];
        const f4* srcT = reinterpret_cast<const f4*>(a.packed + (SPLIT ? L.s_w1cT : L.w1cT));
        for (int i = tid; i < 3 * IMG4; i += PG_WAVES * 64) w_img[3 * IMG4 + i] = srcT[i];
        const f4* vsrc = reinterpret_cast<const f4*>(a.packed + L.b2);
        for (int i = tid; i < EDGE_CONST_VECS * FP / 4; i += PG_WAVES * 64) w_img[6 * IMG4 + i] = vsrc[i];
    }
    const float att_b = a.packed[L.scal];
    const float inv1 = SPLIT ? 1.0f / (a.packed[L.scal + 1] * SPLIT_X_SCALE) : 1.0f;
    const float inv2 = SPLIT ? 1.0f / (a.packed[L.scal + 2] * SPLIT_X_SCALE) : 1.0f;
    const float inv3 = SPLIT ? 1.0f / (a.packed[L.scal + 3] * SPLIT_X_SCALE) : 1.0f;
    const f4* const img_w1c = w_img;
    const f4* const img_w2 = w_img + IMG4;
    const f4* const img_x1 = w_img + 2 * IMG4;
    const f4* const img_w1cT = w_img + 3 * IMG4;
    const f4* const img_w2T = w_img + 4 * IMG4;
    const f4* const img_x1T = w_img + 5 * IMG4;
    const f4* const v_b2 = reinterpret_cast<const f4*>(vecs);
    const f4* const v_d1 = v_b2 + FP / 4;
    const f4* const v_wa = v_d1 + FP / 4;
    const f4* const v_x2 = v_wa + FP / 4;
    const f4* const v_mu = v_x2 + FP / 4;
    const f4* const v_ga = v_mu + FP / 4;
    const f4 zero4 = f4{0.f, 0.f, 0.f, 0.f};
    // out = init + W x  (the recompute follows the module's arithmetic, like the reverse pass)
    auto product = [&](const f4* img, const f4 (&x)[NT], f4 (&out)[NT], float inv, auto init) {
        f4 dummy[NT];
        if constexpr (SPLIT) {
#pragma unroll
            for (int t = 0; t < NT; ++t) out[t] = zero4;
            chain_gemm_split<NT, false>(reinterpret_cast<const h8*>(img), x, x, out, dummy, lane);
#pragma unroll
            for (int t = 0; t < NT; ++t) out[t] = out[t] * inv + init(t);
        } else {
#pragma unroll
            for (int t = 0; t < NT; ++t) out[t] = init(t);
            chain_gemm<NT, false>(img, x, x, out, dummy, lane);
        }
    };
    auto zero_init = [&](int) { return zero4; };

    f4 acc_x1[NT][NT], acc_w2[NT][NT], acc_w1c[NT][NT];
    f4 acc_d1[NT], acc_x2[NT], acc_wa[NT], acc_b2[NT], acc_lg[NT];
    float acc_ab;
    const float rc = a.r_cutoff, pi_rc = 3.14159265358979323846f / rc;
    double* const out = a.partials + (int64_t)blockIdx.x * (3 * MAT + 6 * FP);

    const int64_t items = (int64_t)a.B * n_blk;
    const int64_t first = (int64_t)blockIdx.x * items / gridDim.x, last = ((int64_t)blockIdx.x + 1) * items / gridDim.x;
    for (int64_t item = first; item < last; ++item) {
        const int b = (int)(item / n_blk), ab = (int)(item % n_blk);
        acc_ab = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            acc_d1[t] = acc_x2[t] = acc_wa[t] = acc_b2[t] = acc_lg[t] = zero4;
#pragma unroll
            for (int u = 0; u < NT; ++u) acc_x1[t][u] = acc_w2[t][u] = acc_w1c[t][u] = zero4;
        }
        const int64_t pq_b = (int64_t)b * a.pq_bstride;
        __syncthreads();                                 // the previous item's readers (and the image load) are done
        {
            const float* px = a.pos + (int64_t)b * 3 * n;
            const float* pg = a.g_pos_out + (int64_t)b * 3 * n;
            for (int i = tid; i < 3 * n; i += PG_WAVES * 64) { s_pos[i] = px[i]; s_gpos[i] = pg[i]; }
            for (int e = tid; e < NT * 64 * 2; e += PG_WAVES * 64) {
                const bool second = e >= NT * 64;
                const int ee = second ? e - NT * 64 : e;
                const int cc = ee & 15, tq = ee >> 4;
                const int node = ab * 16 + cc;
                f4 v = zero4;
                if (node < n) {
                    if (!second) v = reinterpret_cast<const f4*>(a.Q + (pq_b + node) * FP)[tq];
                    else if (a.g_nm != nullptr) v = reinterpret_cast<const f4*>(a.g_nm + ((int64_t)b * n + node) * FP)[tq];
                }
                (second ? s_gnm : s_lane)[ee] = v;
            }
        }
        __syncthreads();
        const int an = ab * 16 + c;                          // the lane's destination
        const bool a_ok = an < n;
        const int ac = a_ok ? an : 0;
        const float xa0 = s_pos[3 * ac], xa1 = s_pos[3 * ac + 1], xa2 = s_pos[3 * ac + 2];
        const float gp0 = s_gpos[3 * ac], gp1 = s_gpos[3 * ac + 1], gp2 = s_gpos[3 * ac + 2];
        const float* const P_base = a.P + pq_b * FP;
        for (int i = wave; i < n; i += PG_WAVES) {
            const float v0 = xa0 - s_pos[3 * i], v1 = xa1 - s_pos[3 * i + 1], v2 = xa2 - s_pos[3 * i + 2];
#if TFEP_EGNN_FAST_GEOM
            const float d = __builtin_amdgcn_sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
#else
            const float d = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
#endif
            const bool keep = a_ok && (an != i) && (d <= rc);
            if (__ballot(keep) == 0ull) continue;
#if TFEP_EGNN_FAST_GEOM
            const float inv_d = keep ? fast_rcp(d) : 0.0f;
#else
            const float inv_d = keep ? 1.0f / d : 0.0f;
#endif
            const float u0 = v0 * inv_d, u1 = v1 * inv_d, u2 = v2 * inv_d;
            float cs;
#if TFEP_EGNN_FAST_GEOM
            cs = __builtin_amdgcn_cosf(fminf(d, rc) * (0.5f / rc));
#else
            cs = cosf(pi_rc * d);
#endif
            (void)pi_rc;
            const float sw = 0.5f * cs + 0.5f;
            // ---- forward chain, every activation the sums need kept
            f4 rbf[NT], s1[NT], ds1[NT], a2[NT], ds2[NT], s3[NT], ds3[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f4 mu = v_mu[4 * t + q], ga = v_ga[4 * t + q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float dm = d - mu[r];
                    rbf[t][r] = fast_exp(-ga[r] * dm * dm) * sw;
                }
            }
            {
                const f4* p = reinterpret_cast<const f4*>(P_base + (int64_t)i * FP);
                f4 Pn[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) Pn[t] = p[4 * t + q];
                product(img_w1c, rbf, s1, inv1, [&](int t) { return Pn[t] + s_lane[(4 * t + q) * 16 + c]; });
            }
            silu_keep<NT>(s1, ds1);
            product(img_w2, s1, a2, inv2, [&](int t) { return v_b2[4 * t + q]; });
            silu_keep<NT>(a2, ds2);
            float e = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f4 wa = v_wa[4 * t + q];
#pragma unroll
                for (int r = 0; r < 4; ++r) e += wa[r] * a2[t][r];
            }
            e = sum_over_q(e) + att_b;
#if TFEP_EGNN_FAST_GEOM
            const float sig_e = fast_rcp(1.0f + fast_exp(-e));
#else
            const float sig_e = 1.0f / (1.0f + expf(-e));
#endif
            const float att = keep ? sig_e : 0.0f;
            f4 m[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) m[t] = a2[t] * att;
            product(img_x1, m, s3, inv3, [&](int t) { return v_d1[4 * t + q]; });
            silu_keep<NT>(s3, ds3);
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f4 x2 = v_x2[4 * t + q];
#pragma unroll
                for (int r = 0; r < 4; ++r) s += x2[r] * s3[t][r];
            }
#if TFEP_EGNN_FAST_GEOM
            const float mag = fast_tanh(sum_over_q(s));
#else
            const float mag = tanhf(sum_over_q(s));
#endif
            // ---- reverse chain; a dead edge of a live column group has g_mag = 0 and att = 0: every cotangent below is an
            // exact zero for it
            const float cs_k = keep ? a.speed_factor : 0.0f;
            const float g_mag = cs_k * (u0 * gp0 + u1 * gp1 + u2 * gp2);
            const float g_s = (1.0f - mag * mag) * g_mag;
            f4 gz[NT], gm[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f4 x2 = v_x2[4 * t + q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gz[t][r] = ds3[t][r] * x2[r] * g_s;                       // g_z3
                    acc_x2[t][r] = fmaf(g_s, s3[t][r], acc_x2[t][r]);
                }
                acc_d1[t] += gz[t];
            }
            outer_product<NT>(tile, acc_x1, gz, m, lane);                       // g_z3 (x) m
            product(img_x1T, gz, gm, inv3, [&](int t) { return s_gnm[(4 * t + q) * 16 + c]; });      // g_m
            float g_att = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) g_att += gm[t][r] * a2[t][r];
            const float ce = sum_over_q(g_att) * att * (1.0f - sig_e);          // g_e
            if (q == 0) acc_ab += ce;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f4 wa = v_wa[4 * t + q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gz[t][r] = ds2[t][r] * (att * gm[t][r] + wa[r] * ce);     // g_z2
                    acc_wa[t][r] = fmaf(ce, a2[t][r], acc_wa[t][r]);
                }
                acc_b2[t] += gz[t];
            }
            outer_product<NT>(tile, acc_w2, gz, s1, lane);                      // g_z2 (x) silu(z1)
            product(img_w2T, gz, gm, inv2, zero_init);
#pragma unroll
            for (int t = 0; t < NT; ++t) gz[t] = ds1[t] * gm[t];                // g_z1
            outer_product<NT>(tile, acc_w1c, gz, rbf, lane);                    // g_z1 (x) rbf
            product(img_w1cT, gz, gm, inv1, zero_init);                         // g_rbf
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const f4 mu = v_mu[4 * t + q], ga = v_ga[4 * t + q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {                                   // d rbf_k / d log gamma_k = -gamma_k (d - mu_k)^2 rbf_k
                    const float dm = d - mu[r];
                    acc_lg[t][r] = fmaf(gm[t][r] * rbf[t][r], -ga[r] * dm * dm, acc_lg[t][r]);
                }
            }
        }

        // ---- second level: this item's sums into the workgroup's partial set (doubles, global memory).  Round w: wave w
        // adds its sums, the barrier between rounds orders the waves on every entry (straight-line code per wave: a round
        // that picks one of the three matrices by wave made the compiler merge the folds and spill at the 64-wide tile).
        acc_ab += __shfl_xor(acc_ab, 1, 64);
        acc_ab += __shfl_xor(acc_ab, 2, 64);
        acc_ab += __shfl_xor(acc_ab, 4, 64);
        acc_ab += __shfl_xor(acc_ab, 8, 64);
#pragma unroll 1
        for (int w = 0; w < PG_WAVES; ++w) {
            if (wave == w) {
                const bool f = item == first && w == 0;      // the first addition to an entry stores
                fold_matrix_f64<NT>(out, acc_x1, lane, f);
                fold_matrix_f64<NT>(out + MAT, acc_w2, lane, f);
                fold_matrix_f64<NT>(out + 2 * MAT, acc_w1c, lane, f);
                fold_vector_f64<NT>(out + 3 * MAT, acc_d1, lane, f);
                fold_vector_f64<NT>(out + 3 * MAT + FP, acc_x2, lane, f);
                fold_vector_f64<NT>(out + 3 * MAT + 2 * FP, acc_wa, lane, f);
                fold_vector_f64<NT>(out + 3 * MAT + 3 * FP, acc_b2, lane, f);
                fold_vector_f64<NT>(out + 3 * MAT + 4 * FP, acc_lg, lane, f);
                if (lane == 0) {                             // (the other entries of this vector slot are never read)
                    double* p = out + 3 * MAT + 5 * FP;
                    *p = f ? (double)acc_ab : *p + (double)acc_ab;
                }
            }
            __syncthreads();
        }
    }
}

template <int NT, bool SPLIT>
size_t edge_pg_lds_bytes(int n) {
    const size_t fp = 16 * NT, img4 = SPLIT ? (size_t)NT * ((NT + 1) / 2) * 64 * 2 : (size_t)NT * NT * 64;
    size_t fl = 6 * img4 * 4 + EDGE_CONST_VECS * fp + 2 * (size_t)((3 * n + 3) & ~3) + 2 * (size_t)NT * 64 * 4;
    fl += (size_t)PG_WAVES * fp * TR_LD;                             // the transposition tiles
    return fl * sizeof(float);
}

// ---------------------------------------------------------------------------------------------------------------
// node pass
// ---------------------------------------------------------------------------------------------------------------
template <int NT, int PART>
__global__ __launch_bounds__(PG_WAVES * 64) void egnn_node_param_grad_kernel(tfep_egnn_node_param_grad_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int FP = 16 * NT;
    constexpr int IMG4 = NT * NT * 64;
    constexpr int MAT = FP * FP;
    constexpr int NMAT = PART == 0 ? 2 : 3, NVEC = PART == 0 ? 1 : 2;
    constexpr int SET = NMAT * MAT + NVEC * FP;
    // LDS: part 1 [U1a, U1b][U2^T][W1a^T, W1b^T of the next layer][c1] (the partial set is folded over them); then the tiles
    constexpr int HEAD = PART == 0 ? SET : 5 * IMG4 * 4 + FP;
    static_assert(SET <= HEAD, "the partial set is folded in the image area");
    const PackedLayout L = packed_layout(NT);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = lane >> 4, c = lane & 15;
    f4* const imgs = reinterpret_cast<f4*>(smem);
    float* const tile = smem + HEAD + wave * FP * TR_LD;
    if (PART == 1) {
        const f4* s0 = reinterpret_cast<const f4*>(a.packed + L.u1a);
        for (int i = tid; i < 2 * IMG4; i += PG_WAVES * 64) imgs[i] = s0[i];
        const f4* s1 = reinterpret_cast<const f4*>(a.packed + L.u2T);
        for (int i = tid; i < IMG4; i += PG_WAVES * 64) imgs[2 * IMG4 + i] = s1[i];
        const f4* s2 = reinterpret_cast<const f4*>(a.packed_next + L.w1aT);
        for (int i = tid; i < 2 * IMG4; i += PG_WAVES * 64) imgs[3 * IMG4 + i] = s2[i];
        const f4* s3 = reinterpret_cast<const f4*>(a.packed + L.c1);
        for (int i = tid; i < FP / 4; i += PG_WAVES * 64) imgs[5 * IMG4 + i] = s3[i];
    }
    __syncthreads();
    const f4 *img_u1a = imgs, *img_u1b = imgs + IMG4, *img_u2T = imgs + 2 * IMG4, *img_w1aT = imgs + 3 * IMG4,
             *img_w1bT = imgs + 4 * IMG4, *vc1 = imgs + 5 * IMG4;
    const int64_t n_total = (int64_t)a.B * a.n_nodes;
    const int64_t n_groups = (n_total + 15) / 16;
    const int64_t first = (int64_t)blockIdx.x * n_groups / gridDim.x, last = ((int64_t)blockIdx.x + 1) * n_groups / gridDim.x;
    const f4 zero4 = f4{0.f, 0.f, 0.f, 0.f};
    f4 acc[NMAT][NT][NT], vacc[NVEC][NT];
#pragma unroll
    for (int m = 0; m < NMAT; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int u = 0; u < NT; ++u) acc[m][t][u] = zero4;
#pragma unroll
    for (int m = 0; m < NVEC; ++m)
#pragma unroll
        for (int t = 0; t < NT; ++t) vacc[m][t] = zero4;

    for (int64_t g = first + wave; g < last; g += PG_WAVES) {
        const int64_t node = g * 16 + c;
        const bool ok = node < n_total;                  // a column past the end carries zero cotangents: exact zeros in every sum
        const int64_t nd = ok ? node : 0;
        f4 gP[NT], gQ[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            gP[t] = ok ? reinterpret_cast<const f4*>(a.g_P + nd * FP)[4 * t + q] : zero4;
            gQ[t] = ok ? reinterpret_cast<const f4*>(a.g_Q + nd * FP)[4 * t + q] : zero4;
        }
        if constexpr (PART == 0) {
            f4 y[NT], A[NT], B[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                y[t] = reinterpret_cast<const f4*>(a.h_next + nd * FP)[4 * t + q];
                vacc[0][t] += gQ[t];
            }
            transpose_tile<NT>(tile, y, B, lane);
            transpose_tile<NT>(tile, gP, A, lane);
            outer_acc<NT>(acc[0], A, B);
            transpose_tile<NT>(tile, gQ, A, lane);
            outer_acc<NT>(acc[1], A, B);
        } else {
            const int64_t hb = (nd / a.n_nodes) * a.h_bstride + (nd % a.n_nodes);
            f4 h[NT], m[NT], G[NT], dummy[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                h[t] = reinterpret_cast<const f4*>(a.h + hb * FP)[4 * t + q];
                m[t] = reinterpret_cast<const f4*>(a.nm + nd * FP)[4 * t + q];
                G[t] = (ok && a.g_h_next != nullptr) ? reinterpret_cast<const f4*>(a.g_h_next + nd * FP)[4 * t + q] : zero4;
            }
            chain_gemm<NT, false>(img_w1aT, gP, gP, G, dummy, lane);
            chain_gemm<NT, false>(img_w1bT, gQ, gQ, G, dummy, lane);            // G: cotangent of h'
            f4 z[NT], ds[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) z[t] = vc1[4 * t + q];
            chain_gemm<NT, false>(img_u1a, h, h, z, dummy, lane);
            chain_gemm<NT, false>(img_u1b, m, m, z, dummy, lane);
            silu_keep<NT>(z, ds);
            f4 tt[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) tt[t] = zero4;
            chain_gemm<NT, false>(img_u2T, G, G, tt, dummy, lane);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                tt[t] = tt[t] * ds[t];                                          // cotangent of the hidden pre-activation
                vacc[0][t] += tt[t];
                vacc[1][t] += G[t];
            }
            f4 A[NT], B[NT];
            transpose_tile<NT>(tile, tt, A, lane);
            transpose_tile<NT>(tile, h, B, lane);
            outer_acc<NT>(acc[0], A, B);                                        // U1a
            transpose_tile<NT>(tile, m, B, lane);
            outer_acc<NT>(acc[1], A, B);                                        // U1b
            transpose_tile<NT>(tile, G, A, lane);
            transpose_tile<NT>(tile, z, B, lane);
            outer_acc<NT>(acc[2], A, B);                                        // U2
        }
    }
    (void)img_u1a; (void)img_u1b; (void)img_u2T; (void)img_w1aT; (void)img_w1bT; (void)vc1;

    float* const red = smem;
    __syncthreads();
    for (int w = 0; w < PG_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int m = 0; m < NMAT; ++m) fold_matrix<NT>(red + m * MAT, acc[m], lane, w == 0);
#pragma unroll
            for (int m = 0; m < NVEC; ++m) fold_vector<NT>(red + NMAT * MAT + m * FP, vacc[m], lane, w == 0);
        }
        __syncthreads();
    }
    double* const out = a.partials + (int64_t)blockIdx.x * SET;
    for (int i = tid; i < SET; i += PG_WAVES * 64) out[i] = (double)red[i];
}

// ---------------------------------------------------------------------------------------------------------------
// reduce: one thread per entry of the partial set
// ---------------------------------------------------------------------------------------------------------------
__global__ void egnn_param_grad_reduce_kernel(tfep_egnn_param_grad_reduce_args a) {
    const int FP = 16 * a.nt, MAT = FP * FP;
    const int64_t set = pg_partial_entries(a.nt, a.kind);
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= set) return;
    const int F = a.grads.F, G = a.grads.G, ld0 = 2 * F + G;
    const int n_mat = a.kind == 1 ? 2 : 3;
    float* dst = nullptr;
    if (idx < (int64_t)n_mat * MAT) {
        const int m = (int)(idx / MAT), row = (int)(idx % MAT) / FP, col = (int)(idx % MAT) % FP;
        if (a.kind == 0) {
            if (m == 0 && row < F && col < F && a.grads.ux0_w) dst = a.grads.ux0_w + row * F + col;
            if (m == 1 && row < F && col < F && a.grads.msg2_w) dst = a.grads.msg2_w + row * F + col;
            if (m == 2 && row < F && col < G && a.grads.msg0_w) dst = a.grads.msg0_w + row * ld0 + 2 * F + col;
        } else if (a.kind == 1) {
            if (row < F && col < F && a.grads.msg0_w) dst = a.grads.msg0_w + row * ld0 + m * F + col;
        } else {
            if (m < 2 && row < F && col < F && a.grads.uh0_w) dst = a.grads.uh0_w + row * 2 * F + m * F + col;
            if (m == 2 && row < F && col < F && a.grads.uh2_w) dst = a.grads.uh2_w + row * F + col;
        }
    } else {
        const int v = (int)((idx - (int64_t)n_mat * MAT) / FP), i = (int)((idx - (int64_t)n_mat * MAT) % FP);
        if (a.kind == 0) {
            float* const vec[5] = {a.grads.ux0_b, a.grads.ux2_w, a.grads.att_w, a.grads.msg2_b, a.grads.dist_log_gammas};
            if (v < 5 && i < (v == 4 ? G : F) && vec[v]) dst = vec[v] + i;
            if (v == 5 && i == 0 && a.grads.att_b) dst = a.grads.att_b;
        } else if (a.kind == 1) {
            if (i < F && a.grads.msg0_b) dst = a.grads.msg0_b + i;
        } else {
            float* const p = v == 0 ? a.grads.uh0_b : a.grads.uh2_b;
            if (i < F && p) dst = p + i;
        }
    }
    if (dst == nullptr) return;
    double s = 0.0;
    for (int p = 0; p < a.n_partials; ++p) s += a.partials[(int64_t)p * set + idx];
    *dst = (float)s;
}

template <typename K>
int allow_lds(K kernel, size_t bytes, const char* what) {
    if (bytes > 160 * 1024) return fail(TFEP_ERR_UNSUPPORTED, "%s needs %zu bytes of LDS (> 160 KiB)", what, bytes);
    if (bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return fail(TFEP_ERR_LAUNCH, "%s: hipFuncSetAttribute: %s", what, hipGetErrorString(e));
    }
    return TFEP_OK;
}

int workgroups_for(int64_t items, int max_workgroups) {
    int cap = max_workgroups;
    if (cap <= 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            cus <= 0)
            cus = 256;
        cap = 2 * cus;
    }
    return (int)std::max<int64_t>(1, std::min<int64_t>(items, cap));
}

template <int NT, bool SPLIT>
int launch_edge_pg(const tfep_egnn_edge_param_grad_args& a, hipStream_t st) {
    const size_t lds = edge_pg_lds_bytes<NT, SPLIT>(a.n_nodes);
    int rc = allow_lds(egnn_edge_param_grad_kernel<NT, SPLIT>, lds, "tfep_egnn_edge_param_grad");
    if (rc != TFEP_OK) return rc;
    const int wgs = workgroups_for((int64_t)a.B * ((a.n_nodes + 15) / 16), a.max_workgroups);
    hipLaunchKernelGGL((egnn_edge_param_grad_kernel<NT, SPLIT>), dim3(wgs), dim3(PG_WAVES * 64), lds, st, a);
    return check_launch("tfep_egnn_edge_param_grad");
}

template <int NT, int PART>
int launch_node_pg(const tfep_egnn_node_param_grad_args& a, hipStream_t st) {
    const size_t fp = 16 * NT, set = (size_t)pg_partial_entries(NT, 1 + PART);
    const size_t head = PART == 0 ? set : (size_t)5 * NT * NT * 64 * 4 + fp;
    const size_t lds = (head + PG_WAVES * fp * TR_LD) * sizeof(float);
    int rc = allow_lds(egnn_node_param_grad_kernel<NT, PART>, lds, "tfep_egnn_node_param_grad");
    if (rc != TFEP_OK) return rc;
    const int wgs = workgroups_for(((int64_t)a.B * a.n_nodes + 15) / 16, a.max_workgroups);
    hipLaunchKernelGGL((egnn_node_param_grad_kernel<NT, PART>), dim3(wgs), dim3(PG_WAVES * 64), lds, st, a);
    return check_launch("tfep_egnn_node_param_grad");
}

static_assert(sizeof(tfep_egnn_edge_param_grad_args) == 96, "tfep_egnn_edge_param_grad_args: the ctypes mirror assumes this");
static_assert(sizeof(tfep_egnn_node_param_grad_args) == 104, "tfep_egnn_node_param_grad_args: the ctypes mirror assumes this");
static_assert(sizeof(tfep_egnn_param_grad_reduce_args) == 144, "tfep_egnn_param_grad_reduce_args: the ctypes mirror assumes this");

}  // namespace
}  // namespace tfep

using namespace tfep;

extern "C" {

int tfep_egnn_param_grad_workgroups(int64_t items, int max_workgroups) { return workgroups_for(items, max_workgroups); }

int64_t tfep_egnn_param_grad_partial_entries(int nt, int kind) {
    if ((nt != 1 && nt != 2 && nt != 4) || kind < 0 || kind > 2) return -1;
    return pg_partial_entries(nt, kind);
}

int64_t tfep_egnn_param_grad_struct_bytes(int which) {
    switch (which) {
        case 0: return (int64_t)sizeof(tfep_egnn_edge_param_grad_args);
        case 1: return (int64_t)sizeof(tfep_egnn_node_param_grad_args);
        case 2: return (int64_t)sizeof(tfep_egnn_param_grad_reduce_args);
    }
    return -1;
}

int tfep_egnn_edge_param_grad(const tfep_egnn_edge_param_grad_args* a, void* stream) {
    TFEP_REQUIRE(a != nullptr, "tfep_egnn_edge_param_grad: null argument");
    TFEP_REQUIRE(a->B >= 1 && a->n_nodes >= 1 && a->n_nodes <= 4096, "tfep_egnn_edge_param_grad: bad sizes (B=%d, n_nodes=%d)",
                 a->B, a->n_nodes);
    TFEP_REQUIRE(a->packed && a->pos && a->P && a->Q && a->g_pos_out && a->partials, "tfep_egnn_edge_param_grad: null tensor");
    TFEP_REQUIRE(a->r_cutoff > 0.0f, "tfep_egnn_edge_param_grad: r_cutoff must be positive");
    TFEP_REQUIRE(a->pq_bstride == 0 || a->pq_bstride == a->n_nodes, "tfep_egnn_edge_param_grad: pq_bstride must be 0 or n_nodes");
    TFEP_REQUIRE(a->max_workgroups >= 0, "tfep_egnn_edge_param_grad: max_workgroups must not be negative");
    hipStream_t st = (hipStream_t)stream;
    switch (a->nt * 2 + (a->split ? 1 : 0)) {
        case 2: return launch_edge_pg<1, false>(*a, st);
        case 3: return launch_edge_pg<1, true>(*a, st);
        case 4: return launch_edge_pg<2, false>(*a, st);
        case 5: return launch_edge_pg<2, true>(*a, st);
        case 8: return launch_edge_pg<4, false>(*a, st);
        case 9: return launch_edge_pg<4, true>(*a, st);
    }
    return fail(TFEP_ERR_INVALID_ARGUMENT, "tfep_egnn_edge_param_grad: nt must be 1, 2 or 4 (got %d)", a->nt);
}

int tfep_egnn_node_param_grad(const tfep_egnn_node_param_grad_args* a, void* stream) {
    TFEP_REQUIRE(a != nullptr, "tfep_egnn_node_param_grad: null argument");
    TFEP_REQUIRE(a->B >= 1 && a->n_nodes >= 1, "tfep_egnn_node_param_grad: bad sizes");
    TFEP_REQUIRE(a->part == 0 || a->part == 1, "tfep_egnn_node_param_grad: part must be 0 or 1");
    TFEP_REQUIRE(a->g_P && a->g_Q && a->partials, "tfep_egnn_node_param_grad: null tensor");
    if (a->part == 0) TFEP_REQUIRE(a->h_next != nullptr, "tfep_egnn_node_param_grad: h_next missing");
    else TFEP_REQUIRE(a->packed && a->packed_next && a->h && a->nm, "tfep_egnn_node_param_grad: null tensor");
    TFEP_REQUIRE(a->h_bstride == 0 || a->h_bstride == a->n_nodes, "tfep_egnn_node_param_grad: h_bstride must be 0 or n_nodes");
    TFEP_REQUIRE(a->max_workgroups >= 0, "tfep_egnn_node_param_grad: max_workgroups must not be negative");
    hipStream_t st = (hipStream_t)stream;
    switch (a->nt * 2 + a->part) {
        case 2: return launch_node_pg<1, 0>(*a, st);
        case 3: return launch_node_pg<1, 1>(*a, st);
        case 4: return launch_node_pg<2, 0>(*a, st);
        case 5: return launch_node_pg<2, 1>(*a, st);
        case 8: return launch_node_pg<4, 0>(*a, st);
        case 9: return launch_node_pg<4, 1>(*a, st);
    }
    return fail(TFEP_ERR_INVALID_ARGUMENT, "tfep_egnn_node_param_grad: nt must be 1, 2 or 4 (got %d)", a->nt);
}

int tfep_egnn_param_grad_reduce(const tfep_egnn_param_grad_reduce_args* a, void* stream) {
    TFEP_REQUIRE(a != nullptr && a->partials != nullptr, "tfep_egnn_param_grad_reduce: null argument");
    TFEP_REQUIRE(a->n_partials >= 1, "tfep_egnn_param_grad_reduce: n_partials must be positive");
    const int64_t set = tfep_egnn_param_grad_partial_entries(a->nt, a->kind);
    TFEP_REQUIRE(set > 0, "tfep_egnn_param_grad_reduce: bad nt / kind (%d, %d)", a->nt, a->kind);
    TFEP_REQUIRE(a->grads.F >= 1 && a->grads.G >= 1 && a->grads.F <= 16 * a->nt && a->grads.G <= 16 * a->nt,
                 "tfep_egnn_param_grad_reduce: feature sizes (%d, %d) do not fit a tile of %d", a->grads.F, a->grads.G, 16 * a->nt);
    hipLaunchKernelGGL(egnn_param_grad_reduce_kernel, dim3((unsigned)((set + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a);
    return check_launch("tfep_egnn_param_grad_reduce");
}

}  // extern "C"
