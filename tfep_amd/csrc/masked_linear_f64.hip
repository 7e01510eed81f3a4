// float64 masked linear layers for gfx950: the fp64-MFMA masked GEMM, its peak probe and the column sums of its backward.
// These differ from the float32 kernels by design.  The float64 weight preparation, mask k-ranges, transpose and
// weight-norm backward are the float32 kernels' double instantiations (masked_linear.hip, backward.hip).
//
// GEMM shape:  Y[b, n] = sum_k X[b, k] * W[n, k]      (both operands K-contiguous, "NT"), fp64 products and fp64 sums.
//
// Tiling (one workgroup = 4 wavefronts = 256 threads):
//   workgroup tile  BM x BN = 128 x 128,  BK = 16;  wave w owns the 64 x 64 quadrant (w & 1, w >> 1) as 4 x 4 tiles of
//   v_mfma_f64_16x16x4_f64 (4 doubles = 8 accumulator VGPRs each).  The f64 MFMA takes 64 cycles, 16 of them per
//   4-deep k-step per wave, so the operand traffic is small beside the matrix pipe: the next k-tile is loaded into
//   registers (16-byte loads, rows past B / past the weight's rows read as zero) while the current one is multiplied
//   out of LDS, then stored to the single LDS stage between two barriers.
//   Each lane reads its fragments as 4 consecutive doubles: lane l takes k = [4q, 4q + 4) (q = l >> 4) of row (l & 15)
//   and uses element s in MFMA step s; A and B use the same k permutation, so the dot product is unchanged.
//
// Fragment layout of v_mfma_f64_16x16x4_f64 (NOT the f32 16x16x4 map for C/D):
//   A: lane l holds A[row l & 15][k l >> 4];  B: lane l holds B[k l >> 4][col l & 15]   (as the f32 16x16x4 form)
//   C/D: acc[r] of lane l is D[row (l >> 4) + 4 r][col l & 15]
//
// Mask sparsity: per tile of kr_tile_n packed rows (a multiple of 128; the float32 GEMM's tables have 256), a
// [k_begin, k_end) range bounds the non-zeros; a 128-column tile uses the range of the table tile it lies in.
#include "common.h"

#include <math.h>

namespace tfep {
namespace f64 {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int BK = 16, BM = 128, BN = 128, THREADS = 256;
constexpr int LOADS = BM * BK / 2 / THREADS;   // 16-byte loads per thread and operand per k-tile (4)
// LDS row pitch in doubles: BK + 2 (144 bytes) puts the 16-byte fragment reads of 8 consecutive rows into distinct banks;
// at a 128-byte pitch they would fall into the same bank set.  (-DTFEP_F64_LDS_PAD=0: the unpadded layout, for A/B.)
#ifndef TFEP_F64_LDS_PAD
#define TFEP_F64_LDS_PAD 2
#endif
constexpr int LDR = BK + TFEP_F64_LDS_PAD;

struct GemmArgs {
    const double* a;           // (B, lda), zero padded up to k_padded columns
    int64_t lda;
    const double* w;           // (n_rows_w, ldw) packed masked weights
    int64_t ldw;
    const double* bias;        // (N) or NULL
    const int32_t* k_ranges;   // per tile of kr_tile_n columns [begin, end) or NULL
    int kr_tile_n;             //   (a multiple of BN)
    double* y;
    int64_t ldy;
    const double* aux;         // if set: y = value * elu'(aux), elu'(h) = h > 0 ? 1 : h + 1 (same indexing as y)
    int64_t ldaux;
    int B, N, n_rows_w, k_padded, m_tiles, accumulate;
};

__device__ inline void load_tile(const GemmArgs& g, int m0, int n0, int k0, int tid, f64x2 (&ra)[LOADS], f64x2 (&rb)[LOADS]) {
#pragma unroll
    for (int i = 0; i < LOADS; ++i) {
        const int c = tid + i * THREADS, r = c >> 3, q = c & 7;   // row r of the tile, doubles [2q, 2q + 2) of the k-tile
        const int ra_row = m0 + r, rb_row = n0 + r;
        ra[i] = ra_row < g.B ? *(const f64x2*)(g.a + (int64_t)ra_row * g.lda + k0 + 2 * q) : (f64x2){0.0, 0.0};
        rb[i] = rb_row < g.n_rows_w ? *(const f64x2*)(g.w + (int64_t)rb_row * g.ldw + k0 + 2 * q) : (f64x2){0.0, 0.0};
    }
}

template <int ACT>
__global__ void __launch_bounds__(THREADS, 2) gemm_f64_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) double lds[(BM + BN) * LDR];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int mt = blockIdx.x % g.m_tiles, nt = blockIdx.x / g.m_tiles;
    const int m0 = mt * BM, n0 = nt * BN;
    int kb = 0, ke = g.k_padded;
    if (g.k_ranges) {
        const int t = n0 / g.kr_tile_n;
        kb = g.k_ranges[2 * t];
        ke = g.k_ranges[2 * t + 1];
    }
    const int nk = ke > kb ? (ke - kb) / BK : 0;

    f64x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = (f64x4){0.0, 0.0, 0.0, 0.0};

    const int wm = wave & 1, wn = wave >> 1;
    const int frag = (lane & 15) * LDR + (lane >> 4) * 4;
    const double* As = lds + (wm * 64) * LDR + frag;
    const double* Bs = lds + BM * LDR + (wn * 64) * LDR + frag;
    f64x2 ra[LOADS], rb[LOADS];
    if (nk > 0) load_tile(g, m0, n0, kb, tid, ra, rb);
    for (int t = 0; t < nk; ++t) {
        __syncthreads();                                // every wave is done reading the previous k-tile
#pragma unroll
        for (int i = 0; i < LOADS; ++i) {
            const int c = tid + i * THREADS;
            *(f64x2*)(lds + (c >> 3) * LDR + 2 * (c & 7)) = ra[i];
            *(f64x2*)(lds + BM * LDR + (c >> 3) * LDR + 2 * (c & 7)) = rb[i];
        }
        __syncthreads();
        if (t + 1 < nk) load_tile(g, m0, n0, kb + (t + 1) * BK, tid, ra, rb);   // in flight under the MFMAs below
        f64x4 af[4], bf[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const f64x2 lo = *(const f64x2*)(As + m * 16 * LDR), hi = *(const f64x2*)(As + m * 16 * LDR + 2);
            af[m] = (f64x4){lo[0], lo[1], hi[0], hi[1]};
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const f64x2 lo = *(const f64x2*)(Bs + n * 16 * LDR), hi = *(const f64x2*)(Bs + n * 16 * LDR + 2);
            bf[n] = (f64x4){lo[0], lo[1], hi[0], hi[1]};
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m][s], bf[n][s], acc[m][n], 0, 0, 0);
    }

    // epilogue: acc[m][n][r] is row (lane >> 4) + 4 r, column lane & 15 of tile (m, n)
    const int cj = lane & 15, rq = lane >> 4;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int col = n0 + wn * 64 + n * 16 + cj;
        if (col >= g.N) continue;
        const double bv = g.bias ? g.bias[col] : 0.0;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wm * 64 + m * 16 + rq + 4 * r;
                if (row >= g.B) continue;
                double v = acc[m][n][r] + bv;
                if (ACT == 1) v = v > 0.0 ? v : expm1(v);
                if (g.aux) {
                    const double h = g.aux[(int64_t)row * g.ldaux + col];
                    v *= h > 0.0 ? 1.0 : h + 1.0;
                }
                double* dst = g.y + (int64_t)row * g.ldy + col;
                *dst = g.accumulate ? *dst + v : v;
            }
    }
}

// Diagnostic: the f64 matrix-pipe rate of this device -- the GEMM's 4 x 4 accumulator tiles per wave, operands in
// registers, no memory.
__global__ void __launch_bounds__(THREADS, 2) mfma_f64_peak_kernel(double* out, int iters) {
    f64x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = (f64x4){0.0, 0.0, 0.0, 0.0};
    f64x4 af[4], bf[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        af[m] = (f64x4){1.0 + threadIdx.x, 0.5 * m, 0.25, 2.0};
        bf[m] = (f64x4){1e-3 * threadIdx.x, 1e-3, 2e-3 * m, 3e-3};
    }
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[m][s], bf[n][s], acc[m][n], 0, 0, 0);
    }
    double sum = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) sum += acc[m][n][0] + acc[m][n][1] + acc[m][n][2] + acc[m][n][3];
    out[(int64_t)blockIdx.x * THREADS + threadIdx.x] = sum;
}

// ------------------------------------------------------------------------------------------ column sums
// out[c] (+)= sum_r in[r, c]: 64 columns per workgroup, 16 contiguous row slices summed in a fixed pairwise order.  Each
// slice is one summation chain; the float32 colsum_kernel (backward.hip) keeps eight partial sums per slice, an order
// that would change the float64 results.
constexpr int CS_COLS = 64, CS_SLICES = 16;
__global__ void __launch_bounds__(CS_COLS * CS_SLICES) colsum_kernel(const double* __restrict__ in, int64_t ld, int R, int C,
                                                                    double* __restrict__ out, int accumulate) {
    __shared__ double part[CS_SLICES][CS_COLS];
    const int cx = threadIdx.x & (CS_COLS - 1), sl = threadIdx.x / CS_COLS;
    const int c = blockIdx.x * CS_COLS + cx;
    const int per = (R + CS_SLICES - 1) / CS_SLICES;
    const int r0 = sl * per, r1 = min(R, r0 + per);
    double s = 0.0;
    if (c < C)
        for (int r = r0; r < r1; ++r) s += in[(int64_t)r * ld + c];
    part[sl][cx] = s;
    __syncthreads();
    if (sl == 0 && c < C) {
        double t[CS_SLICES];
#pragma unroll
        for (int q = 0; q < CS_SLICES; ++q) t[q] = part[q][cx];
#pragma unroll
        for (int w = 1; w < CS_SLICES; w *= 2)
#pragma unroll
            for (int q = 0; q + w < CS_SLICES; q += 2 * w) t[q] += t[q + w];
        out[c] = accumulate ? out[c] + t[0] : t[0];
    }
}

}  // namespace f64
}  // namespace tfep

using namespace tfep;

extern "C" {

int tfep_masked_linear_gemm_f64(const double* x, int64_t ldx, const double* w, int64_t ldw, const double* bias,
                                const int32_t* k_ranges, int kr_tile_n, double* y, int64_t ldy, int B, int N, int n_rows_w,
                                int k_padded, int act, int accumulate, const double* elu_grad_of, int64_t ld_elu_grad_of,
                                void* stream) {
    TFEP_REQUIRE(B >= 0 && N >= 0 && n_rows_w >= N, "masked_linear_gemm_f64: bad sizes B=%d N=%d rows=%d", B, N, n_rows_w);
    TFEP_REQUIRE(act == 0 || act == 1, "masked_linear_gemm_f64: act must be 0 (identity) or 1 (ELU)");
    if (B == 0 || N == 0) return TFEP_OK;                  // (an empty batch has no storage: its pointers are NULL)
    TFEP_REQUIRE(x && w && y, "masked_linear_gemm_f64: NULL operand");
    TFEP_REQUIRE(k_padded > 0 && k_padded % f64::BK == 0, "masked_linear_gemm_f64: k_padded=%d must be a positive multiple of %d",
                 k_padded, f64::BK);
    TFEP_REQUIRE(ldx >= k_padded && ldw >= k_padded && ldy >= N, "masked_linear_gemm_f64: row strides too small");
    TFEP_REQUIRE(ldx % 2 == 0 && ldw % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)w % 16 == 0,
                 "masked_linear_gemm_f64: operands need 16-byte aligned rows (even row strides)");
    TFEP_REQUIRE(!elu_grad_of || ld_elu_grad_of >= N, "masked_linear_gemm_f64: ld_elu_grad_of too small");
    TFEP_REQUIRE(!k_ranges || (kr_tile_n > 0 && kr_tile_n % f64::BN == 0),
                 "masked_linear_gemm_f64: kr_tile_n=%d must be a positive multiple of %d (the kernel's column tile)", kr_tile_n,
                 f64::BN);
    f64::GemmArgs g = {};
    g.a = x; g.lda = ldx; g.w = w; g.ldw = ldw; g.bias = bias; g.k_ranges = k_ranges; g.kr_tile_n = kr_tile_n; g.y = y; g.ldy = ldy;
    g.aux = elu_grad_of; g.ldaux = ld_elu_grad_of; g.B = B; g.N = N; g.n_rows_w = n_rows_w; g.k_padded = k_padded;
    g.accumulate = accumulate;
    g.m_tiles = (B + f64::BM - 1) / f64::BM;
    const long long blocks = (long long)g.m_tiles * ((N + f64::BN - 1) / f64::BN);
    TFEP_REQUIRE(blocks <= 0x7fffffffLL, "masked_linear_gemm_f64: grid too large");
    if (act == 1)
        f64::gemm_f64_kernel<1><<<(unsigned)blocks, f64::THREADS, 0, (hipStream_t)stream>>>(g);
    else
        f64::gemm_f64_kernel<0><<<(unsigned)blocks, f64::THREADS, 0, (hipStream_t)stream>>>(g);
    return check_launch("gemm_f64_kernel");
}

int tfep_column_sums_f64(const double* in, int64_t ld, int R, int C, double* out, int accumulate, void* stream) {
    TFEP_REQUIRE(R >= 0 && C >= 0, "column_sums_f64: bad sizes");
    if (C == 0) return TFEP_OK;
    TFEP_REQUIRE(out && (in || R == 0), "column_sums_f64: NULL pointer");
    f64::colsum_kernel<<<(unsigned)((C + f64::CS_COLS - 1) / f64::CS_COLS), f64::CS_COLS * f64::CS_SLICES, 0, (hipStream_t)stream>>>(
        in, ld, R, C, out, accumulate);
    return check_launch("colsum_kernel_f64");
}

int tfep_diag_mfma_f64_peak(double* scratch, int blocks, int iters, void* stream) {
    TFEP_REQUIRE(scratch && blocks > 0 && iters > 0, "diag_mfma_f64_peak: bad arguments");
    f64::mfma_f64_peak_kernel<<<blocks, f64::THREADS, 0, (hipStream_t)stream>>>(scratch, iters);
    return check_launch("mfma_f64_peak_kernel");
}

}  // extern "C"
