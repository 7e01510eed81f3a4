// float64 blocked inverse of a MAF layer: the in-block chain (tfep_inverse_chain_f64).
//
// The inverse of an autoregressive layer is a forward substitution over the degrees: the inputs of degree <= k fix every
// hidden unit of degree <= k ('>=' masks) and the transformer parameters of degree k + 1 (strict '>').  The host walks the
// degrees in blocks (flows/_blocked_f64.py).  At the head of a block the fp64-MFMA GEMM (masked_linear_f64.hip) forms,
// for every masked linear, what the columns of all EARLIER blocks add to the block's rows ("panel": columns [0, k0) of the
// degree-sorted packed weights, k0 a multiple of 16).  This kernel then walks the degrees of the block in order and adds
// what is left: columns [k0, cut) of each row, cut = the row's mask prefix -- the few columns of earlier blocks past the
// last aligned one and everything the block itself has produced.  Every product is counted exactly once: the panel stops
// at k0, the chain starts there and stops at the mask's cut (the packed weights are zero past it anyway).
//
// Layout: one workgroup = 4 waves owns 64 sample rows, lane = row.  fp64 state costs two VGPRs per value, so the block's
// state lives in LDS, transposed ([column][row]: conflict-free 8-byte reads): for every linear l the columns
// [k0_l, end of block) of its input a_l, then the parameters of the features of the current degree.  Weights are read
// through wave-uniform addresses (scalar loads, broadcast to the 64 rows).  Within a degree the four waves split the
// independent dot products (parameter rows, then the hidden units layer by layer) and meet at a barrier per layer.
//
// Summation order of a row's pre-activation: panel + bias, then the chain's columns in ascending order on two
// interleaved accumulators -- fixed per sample row and independent of the batch (no atomics, no split by batch size), so
// a row has the same bits alone and inside any batch.  Everything is fp64: IEEE fma, library expm1 / exp / log / sincos.
//
// Vector members (tfep_inverse_chain_vec_f64, chain_kernel<KMAX, true>): a symmetrized Moebius d-vector or a quaternion
// is one unit of work of a degree.  The wave that owns it follows the links of its feature records (feats[s][6]: 1 +
// component index, feats[s][7]: the slot of the next component), reads the d parameters from `par` (P = 1 per feature)
// and the d values of y, evaluates the map of symmoebius.h / quatprod.h once and writes every component; the log-det
// goes to the slot of component 0, 0.0 to the others, so the row's sum stays "in slot order, wave 0".  The plain Moebius
// map (kinds 5: general, 6: on the unit sphere; 4 is not assigned) is a vector member of the same shape: its inverse is moebius.h's
// moebius_vector<double> on the negated parameters (moebius.py:142-147), whose log-det is that of the inverse itself.
// The scalar instantiation chain_kernel<KMAX, false> compiles none of this.
#include <type_traits>

#include "common.h"
#include "quatprod.h"
#include "spline_f64.h"
#include "symmoebius.h"

namespace tfep {
namespace inv64 {

constexpr int ROWS = 64, WAVES = 4, THREADS = ROWS * WAVES;
constexpr int MAXL = TFEP_INVERSE_F64_MAX_LINEARS, MAXM = TFEP_INVERSE_F64_MAX_MEMBERS;
constexpr int STEP_INTS = 16, FEAT_INTS = 8;
constexpr int64_t LDS_LIMIT = 160 * 1024;

struct ChainArgs {
    tfep_inverse_chain_f64_desc d;
    Spline64 spl[MAXM];
};

struct ChainVecArgs : ChainArgs {
    int32_t dim[MAXM];
    double max_radius[MAXM];
};

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

template <int KMAX, bool VEC>
__global__ void __launch_bounds__(THREADS) chain_kernel(std::conditional_t<VEC, ChainVecArgs, ChainArgs> g) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const tfep_inverse_chain_f64_desc& d = g.d;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int b = blockIdx.x * ROWS + lane;
    const bool live = b < d.B;
    const int64_t bc = live ? b : d.B - 1;         // rows past the batch repeat the last one and store nothing
    const int L = d.n_linears - 1;                  // index of the output linear

    int total_cols = 0;
    for (int l = 0; l <= L; ++l) total_cols += d.n_cols[l];
    double* par = lds + (int64_t)total_cols * ROWS;                       // [feature of the degree][parameter][row]
    double* ldjc = par + (int64_t)d.par_cols * d.max_feats * ROWS;        // [feature of the degree][row]

    // the columns of earlier blocks past the last aligned one: final values, from the global workspaces
    for (int l = 0; l <= L; ++l)
        for (int j = wave; j < d.n_old[l]; j += WAVES) (lds + (int64_t)d.lds_col0[l] * ROWS)[j * ROWS + lane] = d.a[l][bc * d.lda[l] + d.k0[l] + j];
    __syncthreads();

    double* S0 = lds + (int64_t)d.lds_col0[0] * ROWS;
    double ldj = 0.0;
    for (int s = 0; s < d.n_steps; ++s) {
        const int32_t* st = d.steps + (int64_t)s * STEP_INTS;
        const int f0 = st[0], f1 = st[1];
        if (f1 > f0) {
            // 1. transformer parameters of the features of this degree: rows of the output linear
            const int n = st[2] - d.k0[L];
            int item = 0;
            for (int f = f0; f < f1; ++f) {
                const int32_t* ft = d.feats + (int64_t)f * FEAT_INTS;
                const int P = ft[2], prow0 = ft[3];
                for (int p = 0; p < P; ++p, ++item) {
                    if ((item & (WAVES - 1)) != wave) continue;
                    const int row = prow0 + p;
                    double acc = d.bias[L][row];
                    if (d.has_panel[L]) acc += d.zout[bc * d.ldzout + (row - d.zout_row0)];
                    acc = chain_dot(acc, d.w[L] + (int64_t)row * d.ldw[L] + d.k0[L], lds + (int64_t)d.lds_col0[L] * ROWS, n, lane);
                    par[((int64_t)(f - f0) * d.par_cols + p) * ROWS + lane] = acc;
                }
            }
            __syncthreads();
            // 2. the inverse transformer element, x, the conditioner inputs it feeds
            [[maybe_unused]] int unit = 0;                              // VEC: scalar features and heads of vectors
            for (int f = VEC ? f0 : f0 + wave; f < f1; f += VEC ? 1 : WAVES) {
                const int32_t* ft = d.feats + (int64_t)f * FEAT_INTS;
                const int col_x = ft[0], member = ft[1], pos = ft[4], periodic = ft[5];
                if constexpr (VEC) {
                    const int comp = ft[6];
                    if (comp > 1) continue;                                 // written with the head of its vector
                    if ((unit++ & (WAVES - 1)) != wave) continue;
                    if (comp == 1) {
                        const int kind = d.member_kind[member], dim = kind == 3 ? 4 : g.dim[member];
                        double yv[MOEBIUS_MAX_DIM], wv[MOEBIUS_MAX_DIM], xv[MOEBIUS_MAX_DIM];
                        int slot[MOEBIUS_MAX_DIM];
                        int s_ = f;
#pragma unroll
                        for (int i = 0; i < MOEBIUS_MAX_DIM; ++i) {
                            slot[i] = -1;
                            yv[i] = wv[i] = xv[i] = 0.0;
                            if (i < dim && s_ >= f0 && s_ < f1) {                // (a link never leaves the degree: host plan)
                                const int32_t* fc = d.feats + (int64_t)s_ * FEAT_INTS;
                                slot[i] = s_;
                                wv[i] = par[(int64_t)(s_ - f0) * d.par_cols * ROWS + lane];
                                yv[i] = d.y[bc * d.ldy + fc[0]];
                                s_ = fc[7];
                            }
                        }
                        double ld = 0.0;
                        if (kind == 3) {                                    // quaternion product: volume preserving
                            const double y4[4] = {yv[0], yv[1], yv[2], yv[3]}, w4[4] = {wv[0], wv[1], wv[2], wv[3]};
                            double x4[4];
                            quatprod_element<double, true>(y4, w4, x4);
#pragma unroll
                            for (int i = 0; i < 4; ++i) xv[i] = x4[i];
                        } else if (kind >= 5) {                             // Moebius: the map with -w (moebius.py:142-147)
#pragma unroll
                            for (int i = 0; i < MOEBIUS_MAX_DIM; ++i) wv[i] = -wv[i];
                            ld = moebius_vector<double>(yv, wv, dim, g.max_radius[member], kind == 6 ? 1 : 0, xv);
                        } else {                                            // log|det J| of the inverse itself (symmoebius.h)
                            ld = symmoebius_vector<double, true>(yv, wv, dim, g.max_radius[member], xv);
                        }
#pragma unroll
                        for (int i = 0; i < MOEBIUS_MAX_DIM; ++i) {
                            if (slot[i] < 0) continue;
                            const int32_t* fc = d.feats + (int64_t)slot[i] * FEAT_INTS;
                            const int cx = fc[0], ps = fc[4];
                            ldjc[(slot[i] - f0) * ROWS + lane] = i == 0 ? ld : 0.0;
                            S0[(ps - d.k0[0]) * ROWS + lane] = xv[i];
                            if (live) {
                                d.x[(int64_t)b * d.ldx + cx] = xv[i];
                                d.a[0][(int64_t)b * d.lda[0] + ps] = xv[i];
                            }
                        }
                        continue;
                    }
                }
                const double* pf = par + (int64_t)(f - f0) * d.par_cols * ROWS + lane;
                const double yv = d.y[bc * d.ldy + col_x];
                double xv, contrib;
                if (d.member_kind[member] == 0) {                       // affine (affine.py:361-363)
                    const double shift = pf[0], ls = pf[ROWS];
                    xv = (yv - shift) * exp(-ls);
                    contrib = -ls;
                } else {
                    const Spline64 a = g.spl[member];
                    double w[KMAX], h[KMAX], sraw[KMAX + 1], last, last2, ld;
                    load_element64<KMAX>(pf, ROWS, a, w, h, sraw, last, last2);
                    xv = rq_spline_element_f64<KMAX, true>(w, h, sraw, last, last2, a, a.x0[f], a.xf[f], a.y0[f], a.yf[f],
                                                           yv, &ld);
                    contrib = -ld;
                }
                ldjc[(f - f0) * ROWS + lane] = contrib;
                if (live) d.x[(int64_t)b * d.ldx + col_x] = xv;
                double v0 = xv, v1 = 0.0;
                if (periodic) {                                         // (cos, sin) pair (mafembed.py:137-145)
                    const double t = (xv - d.emb_lower) * d.emb_scale;
                    sincos(t, &v1, &v0);
                }
                S0[(pos - d.k0[0]) * ROWS + lane] = v0;
                if (live) d.a[0][(int64_t)b * d.lda[0] + pos] = v0;
                if (periodic) {
                    S0[(pos + 1 - d.k0[0]) * ROWS + lane] = v1;
                    if (live) d.a[0][(int64_t)b * d.lda[0] + pos + 1] = v1;
                }
            }
            __syncthreads();
        }
        // 3. the hidden units of this degree, layer by layer
        for (int l = 0; l < L; ++l) {
            if (l == 0 && wave == 0)
                for (int f = f0; f < f1; ++f) ldj += ldjc[(f - f0) * ROWS + lane];      // in feature order
            const int r0 = st[3 + 3 * l], r1 = st[4 + 3 * l], n = st[5 + 3 * l] - d.k0[l];
            for (int r = r0 + wave; r < r1; r += WAVES) {
                double acc = d.bias[l][r];
                if (d.has_panel[l]) acc += d.a[l + 1][bc * d.lda[l + 1] + r];
                acc = chain_dot(acc, d.w[l] + (int64_t)r * d.ldw[l] + d.k0[l], lds + (int64_t)d.lds_col0[l] * ROWS, n, lane);
                const double v = acc > 0.0 ? acc : expm1(acc);
                (lds + (int64_t)d.lds_col0[l + 1] * ROWS)[(r - d.k0[l + 1]) * ROWS + lane] = v;
                if (live) d.a[l + 1][(int64_t)b * d.lda[l + 1] + r] = v;
            }
            __syncthreads();
        }
    }
    if (wave == 0 && live) d.log_det_J[b] += ldj;
}

inline int64_t lds_bytes(int64_t n_cols_total, int64_t par_cols, int64_t max_feats) {
    return (n_cols_total + par_cols * max_feats + max_feats) * ROWS * (int64_t)sizeof(double);
}

template <int KMAX, bool VEC>
int launch(const std::conditional_t<VEC, ChainVecArgs, ChainArgs>& g, size_t lds, hipStream_t stream) {
    static bool attr_done[TFEP_MAX_DEVICES] = {};
    const int slot = current_device_slot();
    if (!attr_done[slot]) {
        hipError_t e = hipFuncSetAttribute((const void*)chain_kernel<KMAX, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)LDS_LIMIT);
        if (e != hipSuccess) return fail(TFEP_ERR_LAUNCH, "hipFuncSetAttribute(LDS=%d): %s", (int)LDS_LIMIT, hipGetErrorString(e));
        attr_done[slot] = true;
    }
    chain_kernel<KMAX, VEC><<<(unsigned)((g.d.B + ROWS - 1) / ROWS), THREADS, lds, stream>>>(g);
    return check_launch(VEC ? "inverse_chain_vec_f64_kernel" : "inverse_chain_f64_kernel");
}

// The argument checks and the launch of both entry points; `who` prefixes the error messages.  VEC: member kinds 2, 3, 5 and 6
// with member_dim / member_max_radius.
template <bool VEC>
int run(const char* who, const tfep_inverse_chain_f64_desc* d, const int32_t* member_dim, const double* member_max_radius,
        void* stream) {
    TFEP_REQUIRE(d->B >= 0, "%s: negative batch", who);
    TFEP_REQUIRE(d->n_linears >= 2 && d->n_linears <= MAXL, "%s: n_linears=%d unsupported (2..%d)", who, d->n_linears, MAXL);
    TFEP_REQUIRE(d->n_members >= 1 && d->n_members <= MAXM, "%s: n_members=%d unsupported (1..%d)", who, d->n_members, MAXM);
    TFEP_REQUIRE(d->n_steps >= 0 && d->par_cols >= 1 && d->max_feats >= 1, "%s: bad step / parameter counts", who);
    if (d->B == 0 || d->n_steps == 0) return TFEP_OK;         // (an empty batch has no storage: its pointers are NULL)
    TFEP_REQUIRE(d->y && d->x && d->log_det_J && d->steps && d->feats, "%s: NULL pointer (y / x / log_det_J / tables)", who);
    TFEP_REQUIRE(d->ldy >= 1 && d->ldx >= 1, "%s: row strides of x / y must be positive", who);
    const int L = d->n_linears - 1;
    int64_t n_cols_total = 0;
    for (int l = 0; l <= L; ++l) {
        TFEP_REQUIRE(d->a[l] && d->w[l] && d->bias[l], "%s: NULL operand of linear %d", who, l);
        TFEP_REQUIRE((uintptr_t)d->a[l] % 8 == 0 && (uintptr_t)d->w[l] % 8 == 0 && (uintptr_t)d->bias[l] % 8 == 0,
                     "%s: operands of linear %d are not 8-byte aligned", who, l);
        TFEP_REQUIRE(d->k0[l] >= 0 && d->k0[l] % 16 == 0, "%s: k0[%d]=%d must be a non-negative multiple of 16 "
                     "(where the panel product stops)", who, l, d->k0[l]);
        TFEP_REQUIRE(d->n_old[l] >= 0 && d->n_old[l] < 16 && d->n_cols[l] >= d->n_old[l],
                     "%s: linear %d: n_old=%d must be in [0, 16) and at most n_cols=%d", who, l, d->n_old[l], d->n_cols[l]);
        TFEP_REQUIRE(d->lda[l] >= (int64_t)d->k0[l] + d->n_cols[l] && d->ldw[l] >= (int64_t)d->k0[l] + d->n_cols[l],
                     "%s: row strides of linear %d too small for columns [%d, %d)", who, l, d->k0[l], d->k0[l] + d->n_cols[l]);
        TFEP_REQUIRE(d->lds_col0[l] == n_cols_total, "%s: lds_col0[%d]=%d, expected the running sum of n_cols (%lld)", who, l,
                     d->lds_col0[l], (long long)n_cols_total);
        n_cols_total += d->n_cols[l];
    }
    TFEP_REQUIRE(!d->has_panel[L] || (d->zout && d->ldzout >= 1 && (uintptr_t)d->zout % 8 == 0),
                 "%s: the output panel needs zout and a positive row stride", who);
    const int64_t lds = lds_bytes(n_cols_total, d->par_cols, d->max_feats);
    TFEP_REQUIRE(lds <= LDS_LIMIT, "%s: the block's state needs %lld bytes of LDS (limit %lld): fewer degrees per block", who,
                 (long long)lds, (long long)LDS_LIMIT);
    std::conditional_t<VEC, ChainVecArgs, ChainArgs> g = {};
    g.d = *d;
    int kmax = 0;
    for (int m = 0; m < d->n_members; ++m) {
        const int kind = d->member_kind[m];
        if constexpr (VEC) {
            TFEP_REQUIRE(kind >= 0 && kind <= 6 && kind != 4, "%s: member %d: kind must be 0 (affine), 1 (RQ spline), "
                         "2 (symmetrized Moebius), 3 (quaternion product), 5 (Moebius) or 6 (Moebius on the unit sphere)", who, m);
            if (kind >= 5) {
                TFEP_REQUIRE(member_dim[m] >= 1 && member_dim[m] <= MOEBIUS_MAX_DIM, "%s: member %d: member_dim=%d of a "
                             "Moebius member must be in 1..%d", who, m, member_dim[m], MOEBIUS_MAX_DIM);
                TFEP_REQUIRE(member_max_radius[m] > 0.0 && member_max_radius[m] < 1.0, "%s: member %d: max_radius=%g must be "
                             "in (0, 1)", who, m, member_max_radius[m]);
            } else if (kind == 2) {
                TFEP_REQUIRE(member_dim[m] >= 2 && member_dim[m] <= MOEBIUS_MAX_DIM, "%s: member %d: member_dim=%d of a "
                             "symmetrized Moebius member must be in 2..%d", who, m, member_dim[m], MOEBIUS_MAX_DIM);
                TFEP_REQUIRE(member_max_radius[m] > 0.0 && member_max_radius[m] < 1.0, "%s: member %d: max_radius=%g must be "
                             "in (0, 1)", who, m, member_max_radius[m]);
            } else if (kind == 3) {
                TFEP_REQUIRE(member_dim[m] == 4, "%s: member %d: member_dim=%d of a quaternion member must be 4", who, m,
                             member_dim[m]);
            }
            g.dim[m] = kind >= 2 ? member_dim[m] : 0;
            g.max_radius[m] = kind == 2 || kind >= 5 ? member_max_radius[m] : 0.0;
        } else {
            TFEP_REQUIRE(kind == 0 || kind == 1, "%s: member %d: kind must be 0 (affine) or 1 (RQ spline)", who, m);
        }
        if (kind == 1) {
            int rc = make_spline64(&d->spline[m], &g.spl[m]);
            if (rc) return rc;
            TFEP_REQUIRE(g.spl[m].P <= d->par_cols, "%s: member %d has %d parameters per feature, par_cols=%d", who, m,
                         g.spl[m].P, d->par_cols);
            kmax = g.spl[m].K > kmax ? g.spl[m].K : kmax;
        } else if (kind == 0) {
            TFEP_REQUIRE(d->par_cols >= 2, "%s: an affine member needs par_cols >= 2", who);
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (kmax <= 8) return launch<8, VEC>(g, (size_t)lds, s);
    if (kmax <= 16) return launch<16, VEC>(g, (size_t)lds, s);
    return launch<32, VEC>(g, (size_t)lds, s);
}

}  // namespace inv64
}  // namespace tfep

using namespace tfep;

extern "C" {

int64_t tfep_inverse_chain_f64_lds_bytes(int n_cols_total, int par_cols, int max_feats) {
    if (n_cols_total < 0 || par_cols < 1 || max_feats < 1) return -1;
    return inv64::lds_bytes(n_cols_total, par_cols, max_feats);
}

int tfep_inverse_chain_f64(const tfep_inverse_chain_f64_desc* d, void* stream) {
    TFEP_REQUIRE(d != nullptr, "inverse_chain_f64: descriptor is NULL");
    return inv64::run<false>("inverse_chain_f64", d, nullptr, nullptr, stream);
}

int tfep_inverse_chain_vec_f64(const tfep_inverse_chain_vec_f64_desc* d, void* stream) {
    TFEP_REQUIRE(d != nullptr, "inverse_chain_vec_f64: descriptor is NULL");
    return inv64::run<true>("inverse_chain_vec_f64", &d->chain, d->member_dim, d->member_max_radius, stream);
}

}  // extern "C"
