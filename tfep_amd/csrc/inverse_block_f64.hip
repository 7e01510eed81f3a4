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
#include "common.h"
#include "spline_f64.h"

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

template <int KMAX>
__global__ void __launch_bounds__(THREADS) chain_kernel(ChainArgs g) {
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
            for (int f = f0 + wave; f < f1; f += WAVES) {
                const int32_t* ft = d.feats + (int64_t)f * FEAT_INTS;
                const int col_x = ft[0], member = ft[1], pos = ft[4], periodic = ft[5];
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

template <int KMAX>
int launch(const ChainArgs& g, size_t lds, hipStream_t stream) {
    static bool attr_done[TFEP_MAX_DEVICES] = {};
    const int slot = current_device_slot();
    if (!attr_done[slot]) {
        hipError_t e = hipFuncSetAttribute((const void*)chain_kernel<KMAX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)LDS_LIMIT);
        if (e != hipSuccess) return fail(TFEP_ERR_LAUNCH, "hipFuncSetAttribute(LDS=%d): %s", (int)LDS_LIMIT, hipGetErrorString(e));
        attr_done[slot] = true;
    }
    chain_kernel<KMAX><<<(unsigned)((g.d.B + ROWS - 1) / ROWS), THREADS, lds, stream>>>(g);
    return check_launch("inverse_chain_f64_kernel");
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
    TFEP_REQUIRE(d->B >= 0, "inverse_chain_f64: negative batch");
    TFEP_REQUIRE(d->n_linears >= 2 && d->n_linears <= inv64::MAXL, "inverse_chain_f64: n_linears=%d unsupported (2..%d)",
                 d->n_linears, inv64::MAXL);
    TFEP_REQUIRE(d->n_members >= 1 && d->n_members <= inv64::MAXM, "inverse_chain_f64: n_members=%d unsupported (1..%d)",
                 d->n_members, inv64::MAXM);
    TFEP_REQUIRE(d->n_steps >= 0 && d->par_cols >= 1 && d->max_feats >= 1, "inverse_chain_f64: bad step / parameter counts");
    if (d->B == 0 || d->n_steps == 0) return TFEP_OK;         // (an empty batch has no storage: its pointers are NULL)
    TFEP_REQUIRE(d->y && d->x && d->log_det_J && d->steps && d->feats, "inverse_chain_f64: NULL pointer (y / x / log_det_J / tables)");
    TFEP_REQUIRE(d->ldy >= 1 && d->ldx >= 1, "inverse_chain_f64: row strides of x / y must be positive");
    const int L = d->n_linears - 1;
    int64_t n_cols_total = 0;
    for (int l = 0; l <= L; ++l) {
        TFEP_REQUIRE(d->a[l] && d->w[l] && d->bias[l], "inverse_chain_f64: NULL operand of linear %d", l);
        TFEP_REQUIRE((uintptr_t)d->a[l] % 8 == 0 && (uintptr_t)d->w[l] % 8 == 0 && (uintptr_t)d->bias[l] % 8 == 0,
                     "inverse_chain_f64: operands of linear %d are not 8-byte aligned", l);
        TFEP_REQUIRE(d->k0[l] >= 0 && d->k0[l] % 16 == 0, "inverse_chain_f64: k0[%d]=%d must be a non-negative multiple of 16 "
                     "(where the panel product stops)", l, d->k0[l]);
        TFEP_REQUIRE(d->n_old[l] >= 0 && d->n_old[l] < 16 && d->n_cols[l] >= d->n_old[l],
                     "inverse_chain_f64: linear %d: n_old=%d must be in [0, 16) and at most n_cols=%d", l, d->n_old[l], d->n_cols[l]);
        TFEP_REQUIRE(d->lda[l] >= (int64_t)d->k0[l] + d->n_cols[l] && d->ldw[l] >= (int64_t)d->k0[l] + d->n_cols[l],
                     "inverse_chain_f64: row strides of linear %d too small for columns [%d, %d)", l, d->k0[l],
                     d->k0[l] + d->n_cols[l]);
        TFEP_REQUIRE(d->lds_col0[l] == n_cols_total, "inverse_chain_f64: lds_col0[%d]=%d, expected the running sum of n_cols (%lld)",
                     l, d->lds_col0[l], (long long)n_cols_total);
        n_cols_total += d->n_cols[l];
    }
    TFEP_REQUIRE(!d->has_panel[L] || (d->zout && d->ldzout >= 1 && (uintptr_t)d->zout % 8 == 0),
                 "inverse_chain_f64: the output panel needs zout and a positive row stride");
    const int64_t lds = inv64::lds_bytes(n_cols_total, d->par_cols, d->max_feats);
    TFEP_REQUIRE(lds <= inv64::LDS_LIMIT, "inverse_chain_f64: the block's state needs %lld bytes of LDS (limit %lld): fewer "
                 "degrees per block", (long long)lds, (long long)inv64::LDS_LIMIT);
    inv64::ChainArgs g = {};
    g.d = *d;
    int kmax = 0;
    for (int m = 0; m < d->n_members; ++m) {
        TFEP_REQUIRE(d->member_kind[m] == 0 || d->member_kind[m] == 1, "inverse_chain_f64: member %d: kind must be 0 (affine) or "
                     "1 (RQ spline)", m);
        if (d->member_kind[m] == 1) {
            int rc = make_spline64(&d->spline[m], &g.spl[m]);
            if (rc) return rc;
            TFEP_REQUIRE(g.spl[m].P <= d->par_cols, "inverse_chain_f64: member %d has %d parameters per feature, par_cols=%d",
                         m, g.spl[m].P, d->par_cols);
            kmax = g.spl[m].K > kmax ? g.spl[m].K : kmax;
        } else {
            TFEP_REQUIRE(d->par_cols >= 2, "inverse_chain_f64: an affine member needs par_cols >= 2");
        }
    }
    hipStream_t s = (hipStream_t)stream;
    if (kmax <= 8) return inv64::launch<8>(g, (size_t)lds, s);
    if (kmax <= 16) return inv64::launch<16>(g, (size_t)lds, s);
    return inv64::launch<32>(g, (size_t)lds, s);
}

}  // extern "C"
