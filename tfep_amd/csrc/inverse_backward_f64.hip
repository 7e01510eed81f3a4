// float64 blocked backward through the inverse of a MAF layer: the in-block chain (tfep_inverse_backward_chain_f64, and
// tfep_inverse_backward_chain_vec_f64 for layers with vector-valued members).
//
// With y = f(x), the inverse returns (x, -ldj_f(x)); for cotangents (gx, gl) of the two, the gradient with respect to y is
// the u that solves J^T u + gl grad_x ldj_f = gx, J = df/dx triangular in degree order.  The solve walks the
// degrees DOWNWARDS: the cotangent of a unit of degree d collects, through the transposed masked linears, the cotangents
// of the rows that read it -- rows of degree >= d of a hidden linear, parameter rows of features of degree > d of the
// output linear -- a SUFFIX [start, n) of the degree-sorted packed rows.  The host walks the degrees in blocks
// (flows/_blocked_f64_backward.py).  At the head of a block the fp64-MFMA GEMM (masked_linear_f64.hip) forms, for every
// linear, what the rows [R, n_pad) add to the block's columns ("panel": R = the first row that earlier blocks made
// final, rounded UP to 16).  This kernel walks the degrees of the block in descending order and adds rows [start, R) of
// each column: the few final rows below R and everything the block itself has produced.  Every product is counted
// exactly once.
//
// Per degree: the hidden linears from l = L down to 1 (G_l = panel + W_l^T ga_l on the mask; ga_{l-1} = ELU'(h_l) G_l with
// ELU' = h > 0 ? 1 : h + 1 from the stored activation), then the features of the degree: G_0 at their conditioner inputs,
// s = E^T G_0 (E the embedding Jacobian: identity, or scale (-sin t, cos t) for a periodic feature), u = (r - s) / tau_x,
// q = A u + c -- the parameter cotangents, the rows of ga_L.  r, tau_x, A, c come from the transformer's own VJP kernel
// (two calls on the host side), so no transformer code lives here.
//
// Layout as inverse_block_f64.hip: one workgroup = 4 waves owns 64 sample rows, lane = row; the rows [row0_l, R_l) of every
// ga_l live in LDS as [row][sample] (conflict-free 8-byte accesses); the transposed packs are read through wave-uniform
// addresses, contiguous along the dot; within a stage the four waves split the independent columns and meet at a barrier.
// Summation order of a column: the panel value, then the chain's rows in ascending order on two interleaved accumulators
// -- fixed per sample row, no atomics, independent of the batch.  Everything is fp64 IEEE fma.
//
// Vector members (tfep_inverse_backward_chain_vec_f64, chain_kernel<true>): a symmetrized Moebius d-vector or a quaternion
// is one unit of work of a degree.  The wave that owns it follows the links of its feature records (feats[s][6]: 1 +
// component index, feats[s][7]: the slot of the next component), forms g_i = gx_i - s_i per component (the same chain sum
// as a scalar feature), and calls the member's INVERSE VJP of symmoebius.h / quatprod.h at (y_v, theta_v) with the
// cotangents (g, gl): that returns (u_v, -q_v) = (T^-T (g - gl l_x), -(Theta^T u_v + gl l_theta)) -- no k x k solve
// (include/tfep_hip.h).  It writes u and q at every component.  A feature of a scalar member runs the code below unchanged;
// the scalar instantiation chain_kernel<false> compiles none of the vector code.
#include <type_traits>

#include "common.h"
#include "quatprod.h"
#include "symmoebius.h"

namespace tfep {
namespace invb64 {

constexpr int ROWS = 64, WAVES = 4, THREADS = ROWS * WAVES;
constexpr int MAXL = TFEP_INVERSE_F64_MAX_LINEARS, MAXM = TFEP_INVERSE_F64_MAX_MEMBERS;
constexpr int STEP_INTS = 20, FEAT_INTS = 8;
constexpr int64_t LDS_LIMIT = 160 * 1024;

// acc + sum_j w[j] * s[j][lane], j ascending, even / odd j on two accumulators
__device__ inline double chain_dot(double acc, const double* __restrict__ w, const double* s, int n, int lane) {
    double acc1 = 0.0;
    int j = 0;
    for (; j + 1 < n; j += 2) {
        acc = fma(w[j], s[j * ROWS + lane], acc);
        acc1 = fma(w[j + 1], s[(j + 1) * ROWS + lane], acc1);
    }
    if (j < n) acc = fma(w[j], s[j * ROWS + lane], acc);
    return acc + acc1;
}

using ScalarDesc = tfep_inverse_backward_chain_f64_desc;
using VecDesc = tfep_inverse_backward_chain_vec_f64_desc;

__device__ __host__ inline const ScalarDesc& chain_of(const ScalarDesc& g) { return g; }
__device__ __host__ inline const ScalarDesc& chain_of(const VecDesc& g) { return g.chain; }

// One vector of a vector-valued member, head in slot f of the step's [f0, f1): u at its slots, q at its parameter rows.
__device__ inline void vector_step(const VecDesc& g, int f, int f0, int f1, int start, int n, const double* S, double* Q,
                                   int lane, int b, int64_t bc, bool live) {
    const ScalarDesc& d = g.chain;
    const int L = d.n_linears - 1;
    const int member = d.feats[(int64_t)f * FEAT_INTS + 1];
    const int kind = member >= 0 && member < g.n_members && member < MAXM ? g.member_kind[member] : -1;
    if (kind != 2 && kind != 3) return;                              // (the host checks the kinds; the tables are the caller's)
    const int dim = kind == 3 ? 4 : g.member_dim[member];
    double yv[MOEBIUS_MAX_DIM], wv[MOEBIUS_MAX_DIM], gv[MOEBIUS_MAX_DIM], gyv[MOEBIUS_MAX_DIM], gwv[MOEBIUS_MAX_DIM];
    int slot[MOEBIUS_MAX_DIM];
    int s_ = f;
#pragma unroll
    for (int i = 0; i < MOEBIUS_MAX_DIM; ++i) {
        slot[i] = -1;
        yv[i] = wv[i] = gv[i] = gyv[i] = gwv[i] = 0.0;
        if (i < dim && s_ >= f0 && s_ < f1) {                        // (a link that leaves the degree ends the chain)
            const int32_t* fc = d.feats + (int64_t)s_ * FEAT_INTS;
            const int pos = fc[4];
            slot[i] = s_;
            double g0 = d.has_panel[0] ? d.G[0][bc * d.ldG[0] + pos] : 0.0;
            g0 = chain_dot(g0, d.wt[0] + (int64_t)pos * d.ldwt[0] + start, S, n, lane);
            gv[i] = d.r[bc * d.ldr + s_] - g0;                       // gx - s
            yv[i] = g.y[bc * g.ldy + fc[0]];
            wv[i] = g.theta[bc * g.ldtheta + fc[3]];
            s_ = fc[7];
        }
    }
    if (kind == 3) {                                                 // quaternion product: log-det 0, gl takes no part
        const double y4[4] = {yv[0], yv[1], yv[2], yv[3]}, w4[4] = {wv[0], wv[1], wv[2], wv[3]};
        const double g4[4] = {gv[0], gv[1], gv[2], gv[3]};
        double gy4[4], gw4[4];
        quatprod_vjp_element<double, true>(y4, w4, g4, gy4, gw4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            gyv[i] = gy4[i];
            gwv[i] = gw4[i];
        }
    } else {
        symmoebius_vjp_vector<double, true>(yv, wv, dim, g.member_max_radius[member], gv, g.gl[bc], gyv, gwv);
    }
#pragma unroll
    for (int i = 0; i < MOEBIUS_MAX_DIM; ++i) {
        if (slot[i] < 0) continue;
        const int row = d.feats[(int64_t)slot[i] * FEAT_INTS + 3];
        const double u = gyv[i], q = -gwv[i];
        if (live) d.u[(int64_t)b * d.ldu + slot[i]] = u;
        Q[(row - d.row0[L]) * ROWS + lane] = q;
        if (live) d.ga[L][(int64_t)b * d.ldga[L] + row] = q;
    }
}

template <bool VEC>
__global__ void __launch_bounds__(THREADS) chain_kernel(std::conditional_t<VEC, VecDesc, ScalarDesc> g) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const ScalarDesc& d = chain_of(g);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * ROWS + lane;
    const bool live = b < d.B;
    const int64_t bc = live ? b : d.B - 1;         // rows past the batch repeat the last one and store nothing
    const int L = d.n_linears - 1;                  // index of the output linear

    // the final rows of earlier (higher) blocks that lie below R: from the global workspaces
    for (int l = 0; l <= L; ++l) {
        double* S = lds + (int64_t)d.lds_row0[l] * ROWS;
        const int r0 = d.R[l] - d.n_old[l];
        for (int j = wave; j < d.n_old[l]; j += WAVES) S[(r0 + j - d.row0[l]) * ROWS + lane] = d.ga[l][bc * d.ldga[l] + r0 + j];
    }
    __syncthreads();

    for (int s = 0; s < d.n_steps; ++s) {
        const int32_t* st = d.steps + (int64_t)s * STEP_INTS;
        // 1. the hidden units of this degree, from the last hidden layer down: columns of linear l = rows of linear l - 1
        for (int l = L; l >= 1; --l) {
            const int c0 = st[2 + 3 * l], c1 = st[3 + 3 * l], start = st[4 + 3 * l], n = d.R[l] - start;
            const double* S = lds + (int64_t)(d.lds_row0[l] + start - d.row0[l]) * ROWS;
            double* T = lds + (int64_t)d.lds_row0[l - 1] * ROWS;
            for (int j = c0 + wave; j < c1; j += WAVES) {
                double acc = d.has_panel[l] ? d.G[l][bc * d.ldG[l] + j] : 0.0;
                acc = chain_dot(acc, d.wt[l] + (int64_t)j * d.ldwt[l] + start, S, n, lane);
                const double hv = d.h[l][bc * d.ldh[l] + j];
                const double v = acc * (hv > 0.0 ? 1.0 : hv + 1.0);
                T[(j - d.row0[l - 1]) * ROWS + lane] = v;
                if (live) d.ga[l - 1][(int64_t)b * d.ldga[l - 1] + j] = v;
            }
            __syncthreads();
        }
        // 2. the features of this degree: G_0 at their inputs, the embedding's VJP, u, the parameter cotangents
        const int f0 = st[0], f1 = st[1], start = st[4], n = d.R[0] - start;
        const double* S = lds + (int64_t)(d.lds_row0[0] + start - d.row0[0]) * ROWS;
        double* Q = lds + (int64_t)d.lds_row0[L] * ROWS;
        [[maybe_unused]] int unit = 0;                                   // VEC: scalar features and heads of vectors
        for (int f = VEC ? f0 : f0 + wave; f < f1; f += VEC ? 1 : WAVES) {
            const int32_t* ft = d.feats + (int64_t)f * FEAT_INTS;
            if constexpr (VEC) {
                const int comp = ft[6];
                if (comp > 1) continue;                                 // written with the head of its vector
                if ((unit++ & (WAVES - 1)) != wave) continue;
                if (comp == 1) {
                    vector_step(g, f, f0, f1, start, n, S, Q, lane, b, bc, live);
                    continue;
                }
            }
            const int P = ft[2], prow0 = ft[3], pos = ft[4], periodic = ft[5];
            double g0 = d.has_panel[0] ? d.G[0][bc * d.ldG[0] + pos] : 0.0;
            g0 = chain_dot(g0, d.wt[0] + (int64_t)pos * d.ldwt[0] + start, S, n, lane);
            double sv = g0;
            if (periodic) {                                             // inputs (cos t, sin t), t = (x - lower) scale
                double g1 = d.has_panel[0] ? d.G[0][bc * d.ldG[0] + pos + 1] : 0.0;
                g1 = chain_dot(g1, d.wt[0] + (int64_t)(pos + 1) * d.ldwt[0] + start, S, n, lane);
                const double ct = d.h[0][bc * d.ldh[0] + pos], sn = d.h[0][bc * d.ldh[0] + pos + 1];
                sv = d.emb_scale * fma(-sn, g0, ct * g1);
            }
            const double u = (d.r[bc * d.ldr + f] - sv) / d.tau_x[bc * d.ldr + f];
            if (live) d.u[(int64_t)b * d.ldu + f] = u;
            for (int p = 0; p < P; ++p) {
                const int row = prow0 + p;
                const double q = fma(d.A[bc * d.ldA + row], u, d.c[bc * d.ldA + row]);
                Q[(row - d.row0[L]) * ROWS + lane] = q;
                if (live) d.ga[L][(int64_t)b * d.ldga[L] + row] = q;
            }
        }
        __syncthreads();
    }
}

inline int64_t lds_bytes(int64_t n_rows_total) { return n_rows_total * ROWS * (int64_t)sizeof(double); }

// The argument checks and the launch of both entry points; `who` prefixes the error messages.  VEC: member kinds 0 .. 3 with
// member_dim / member_max_radius, and y / theta / gl.
template <bool VEC>
int run(const char* who, const std::conditional_t<VEC, VecDesc, ScalarDesc>* g, void* stream) {
    const ScalarDesc* d = &chain_of(*g);
    TFEP_REQUIRE(d->B >= 0, "%s: negative batch", who);
    TFEP_REQUIRE(d->n_linears >= 2 && d->n_linears <= MAXL, "%s: n_linears=%d unsupported (2..%d)", who, d->n_linears, MAXL);
    TFEP_REQUIRE(d->n_steps >= 0, "%s: negative step count", who);
    if (d->B == 0 || d->n_steps == 0) return TFEP_OK;         // (an empty batch has no storage: its pointers are NULL)
    bool scalar_members = true;                                 // is tau_x / A / c read at all
    if constexpr (VEC) {
        TFEP_REQUIRE(g->n_members >= 1 && g->n_members <= MAXM, "%s: n_members=%d unsupported (1..%d)", who, g->n_members, MAXM);
        scalar_members = false;
        for (int m = 0; m < g->n_members; ++m) {
            const int kind = g->member_kind[m];
            TFEP_REQUIRE(kind >= 0 && kind <= 3, "%s: member %d: kind must be 0 (affine), 1 (RQ spline), 2 (symmetrized Moebius) "
                         "or 3 (quaternion product)", who, m);
            if (kind == 2) {
                TFEP_REQUIRE(g->member_dim[m] >= 2 && g->member_dim[m] <= MOEBIUS_MAX_DIM, "%s: member %d: member_dim=%d of a "
                             "symmetrized Moebius member must be in 2..%d", who, m, g->member_dim[m], MOEBIUS_MAX_DIM);
                TFEP_REQUIRE(g->member_max_radius[m] > 0.0 && g->member_max_radius[m] < 1.0, "%s: member %d: max_radius=%g must be "
                             "in (0, 1)", who, m, g->member_max_radius[m]);
            } else if (kind == 3) {
                TFEP_REQUIRE(g->member_dim[m] == 4, "%s: member %d: member_dim=%d of a quaternion member must be 4", who, m,
                             g->member_dim[m]);
            } else {
                scalar_members = true;
            }
        }
        TFEP_REQUIRE(g->y && g->theta && g->gl, "%s: NULL pointer (y / theta / gl)", who);
        TFEP_REQUIRE((uintptr_t)g->y % 8 == 0 && (uintptr_t)g->theta % 8 == 0 && (uintptr_t)g->gl % 8 == 0,
                     "%s: y / theta / gl are not 8-byte aligned", who);
        TFEP_REQUIRE(g->ldy >= 1 && g->ldtheta >= 1, "%s: row strides of y / theta must be positive", who);
    }
    TFEP_REQUIRE(d->r && d->u && d->steps && d->feats && (!scalar_members || (d->tau_x && d->A && d->c)),
                 "%s: NULL pointer (r / tau_x / A / c / u / tables)", who);
    TFEP_REQUIRE((uintptr_t)d->r % 8 == 0 && (uintptr_t)d->tau_x % 8 == 0 && (uintptr_t)d->A % 8 == 0 && (uintptr_t)d->c % 8 == 0 &&
                 (uintptr_t)d->u % 8 == 0, "%s: r / tau_x / A / c / u are not 8-byte aligned", who);
    TFEP_REQUIRE(d->ldr >= 1 && d->ldu >= 1 && (!scalar_members || d->ldA >= 1), "%s: row strides of r / A / u must be positive", who);
    const int L = d->n_linears - 1;
    int64_t n_rows_total = 0;
    for (int l = 0; l <= L; ++l) {
        TFEP_REQUIRE(d->ga[l] && d->wt[l] && d->h[l], "%s: NULL operand of linear %d", who, l);
        TFEP_REQUIRE((uintptr_t)d->ga[l] % 8 == 0 && (uintptr_t)d->wt[l] % 8 == 0 && (uintptr_t)d->h[l] % 8 == 0 &&
                     (uintptr_t)d->G[l] % 8 == 0, "%s: operands of linear %d are not 8-byte aligned", who, l);
        TFEP_REQUIRE(d->R[l] >= 0 && d->R[l] % 16 == 0, "%s: R[%d]=%d must be a non-negative multiple of 16 "
                     "(where the panel product starts)", who, l, d->R[l]);
        TFEP_REQUIRE(d->row0[l] >= 0 && d->row0[l] <= d->R[l], "%s: linear %d: row0=%d must be in [0, R=%d]", who, l, d->row0[l],
                     d->R[l]);
        TFEP_REQUIRE(d->n_old[l] >= 0 && d->n_old[l] < 16 && d->n_old[l] <= d->R[l] - d->row0[l],
                     "%s: linear %d: n_old=%d must be in [0, 16) and at most R - row0 = %d", who, l, d->n_old[l],
                     d->R[l] - d->row0[l]);
        TFEP_REQUIRE(d->ldga[l] >= d->R[l] && d->ldwt[l] >= d->R[l] && d->ldh[l] >= 1,
                     "%s: row strides of linear %d too small for rows [0, %d)", who, l, d->R[l]);
        TFEP_REQUIRE(!d->has_panel[l] || (d->G[l] && d->ldG[l] >= 1), "%s: the panel of linear %d needs G and a positive row "
                     "stride", who, l);
        TFEP_REQUIRE(d->lds_row0[l] == n_rows_total, "%s: lds_row0[%d]=%d, expected the running sum of R - row0 (%lld)", who, l,
                     d->lds_row0[l], (long long)n_rows_total);
        n_rows_total += d->R[l] - d->row0[l];
    }
    const int64_t lds = lds_bytes(n_rows_total);
    TFEP_REQUIRE(lds <= LDS_LIMIT, "%s: the block's state needs %lld bytes of LDS (limit %lld): fewer degrees per block", who,
                 (long long)lds, (long long)LDS_LIMIT);
    static bool attr_done[TFEP_MAX_DEVICES] = {};
    const int slot = current_device_slot();
    if (!attr_done[slot]) {
        hipError_t e = hipFuncSetAttribute((const void*)chain_kernel<VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_LIMIT);
        if (e != hipSuccess) return fail(TFEP_ERR_LAUNCH, "hipFuncSetAttribute(LDS=%d): %s", (int)LDS_LIMIT, hipGetErrorString(e));
        attr_done[slot] = true;
    }
    chain_kernel<VEC><<<(unsigned)((d->B + ROWS - 1) / ROWS), THREADS, (size_t)lds, (hipStream_t)stream>>>(*g);
    return check_launch(VEC ? "inverse_backward_chain_vec_f64_kernel" : "inverse_backward_chain_f64_kernel");
}

}  // namespace invb64
}  // namespace tfep

using namespace tfep;

extern "C" {

int64_t tfep_inverse_backward_chain_f64_lds_bytes(int n_rows_total) {
    if (n_rows_total < 0) return -1;
    return invb64::lds_bytes(n_rows_total);
}

int tfep_inverse_backward_chain_f64(const tfep_inverse_backward_chain_f64_desc* d, void* stream) {
    TFEP_REQUIRE(d != nullptr, "inverse_backward_chain_f64: descriptor is NULL");
    return invb64::run<false>("inverse_backward_chain_f64", d, stream);
}

int tfep_inverse_backward_chain_vec_f64(const tfep_inverse_backward_chain_vec_f64_desc* d, void* stream) {
    TFEP_REQUIRE(d != nullptr, "inverse_backward_chain_vec_f64: descriptor is NULL");
    return invb64::run<true>("inverse_backward_chain_vec_f64", d, stream);
}

}  // extern "C"
