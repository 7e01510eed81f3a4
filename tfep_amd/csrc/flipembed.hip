// FlipInvariantEmbedding (reference embeddings/mafembed.py:174-348) forward and VJP, float32 and float64.  The per-vector
// arithmetic and the LDS image of the two networks are in flipembed.h.
//
// Forward: one lane per (row, vector); the same launch copies the non-embedded columns, so it writes the whole output
// row [x[:, nonembedded]..., E values per vector...].
//
// Backward: the forward is recomputed from x.  A lane holds ITEMS (row, vector) items; for every hidden unit it sums the
// parameter-gradient contributions of its items in fp64, the wave sums them (butterfly), the four waves of the workgroup
// are added in wave order, and the workgroup adds the result to its own row of the workspace.  A second launch adds the
// rows in row order and writes (or accumulates into) the eight gradient tensors.  No atomics: for a given launch shape
// the sums are formed in one fixed order, so two runs give the same bits.
#include "common.h"
#include "flipembed.h"

namespace tfep {

constexpr int FLIP_MAX_BLOCKS = 2048;       // workgroups (= workspace rows) of the backward

// compile-time bound of the embedding dimension, and items per lane of the backward, of the instance that serves E
static inline int flip_ep(int E) { return E <= 4 ? 4 : E <= 8 ? 8 : E <= 16 ? 16 : 32; }
static inline int flip_items(int EP) { return EP <= 8 ? 4 : EP == 16 ? 2 : 1; }

static inline int flip_backward_blocks(int64_t n_items, int EP) {
    const int64_t per = 256 * (int64_t)flip_items(EP);
    const int64_t blocks = (n_items + per - 1) / per;
    return (int)(blocks < 1 ? 1 : blocks > FLIP_MAX_BLOCKS ? FLIP_MAX_BLOCKS : blocks);
}

template <typename T, int EP>
__global__ void __launch_bounds__(256) flipembed_forward_kernel(const T* __restrict__ x, int64_t ldx,
                                                                const int32_t* __restrict__ eidx, int n_vec,
                                                                const int32_t* __restrict__ nidx, int n_non, int d, int H,
                                                                int E, FlipNets<const T> nets, T* __restrict__ out,
                                                                int64_t ldo, int B) {
    __shared__ T sW[flip_staged(FLIP_MAX_DIM, FLIP_MAX_HIDDEN, EP)];
    flip_stage<T, EP>(sW, nets, d, H, E);
    __syncthreads();
    const int lanes = n_vec > 0 ? n_vec : 1;                 // lanes of one row (a row without vectors is copied by one)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * lanes) return;
    const int b = (int)(i / lanes), k = (int)(i % lanes);
    const T* xr = x + (int64_t)b * ldx;
    T* orow = out + (int64_t)b * ldo;
    for (int j = k; j < n_non; j += lanes) orow[j] = xr[nidx[j]];
    if (k >= n_vec) return;
    T v[FLIP_MAX_DIM];
#pragma unroll
    for (int c = 0; c < FLIP_MAX_DIM; ++c) v[c] = c < d ? xr[eidx[k * d + c]] : (T)0;
    T ep[EP], em[EP], ap, am, wp, wm;
    flip_networks<T, EP>(sW, d, H, v, ep, em, ap, am);
    flip_softmax(ap, am, wp, wm);
    T* o = orow + n_non + (int64_t)k * E;
#pragma unroll
    for (int e = 0; e < EP; ++e)
        if (e < E) o[e] = flip_mix(wp, ep[e], wm, em[e]);
}

// Sum of one fp64 value over the workgroup's lanes into slot j of the wave's row of sRed (lane 0 of every wave writes).
__device__ __forceinline__ void flip_wave_store(double v, double* __restrict__ row, int j) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) row[j] = v;
}

// The n values the four waves left in sRed, added in wave order into the workgroup's workspace row.
template <int RMAX>
__device__ __forceinline__ void flip_block_store(const double (&sRed)[4][RMAX], int n, double* __restrict__ dst, bool first) {
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const int j = threadIdx.x;
        const double s = ((sRed[0][j] + sRed[1][j]) + sRed[2][j]) + sRed[3][j];
        dst[j] = first ? s : dst[j] + s;
    }
    __syncthreads();
}

template <typename T, int EP, int ITEMS>
__global__ void __launch_bounds__(256) flipembed_backward_kernel(const T* __restrict__ x, int64_t ldx,
                                                                 const int32_t* __restrict__ eidx, int n_vec,
                                                                 const int32_t* __restrict__ nidx, int n_non, int d, int H,
                                                                 int E, FlipNets<const T> nets, const T* __restrict__ gout,
                                                                 int64_t ldg, T* __restrict__ gx, int64_t ldgx,
                                                                 double* __restrict__ partial, int B) {
    constexpr int RMAX = flip_record(FLIP_MAX_DIM, EP);
    __shared__ T sW[flip_staged(FLIP_MAX_DIM, FLIP_MAX_HIDDEN, EP)];
    __shared__ double sRed[4][RMAX];
    flip_stage<T, EP>(sW, nets, d, H, E);
    __syncthreads();
    const int R = flip_record(d, EP);
    double* mine = partial + (int64_t)blockIdx.x * flip_staged(d, H, EP);
    double* red = sRed[threadIdx.x >> 6];
    const int lanes = n_vec > 0 ? n_vec : 1;
    const int64_t n_items = (int64_t)B * lanes, per_batch = 256 * (int64_t)ITEMS;
    bool first = true;
    // (every workgroup of the launch has at least one batch: flip_backward_blocks)
    for (int64_t base = (int64_t)blockIdx.x * per_batch; base < n_items; base += (int64_t)gridDim.x * per_batch, first = false) {
        T v[ITEMS][FLIP_MAX_DIM], dv[ITEMS][FLIP_MAX_DIM], g[ITEMS][EP], wp[ITEMS], wm[ITEMS], dap[ITEMS];
        double acc_b2e[EP], acc_b2w = 0.0;
#pragma unroll
        for (int e = 0; e < EP; ++e) acc_b2e[e] = 0.0;

        // ---- per item: pass-through columns, forward, and the cotangents of the softmax weights
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int64_t i = base + (int64_t)it * 256 + threadIdx.x;
            const bool valid = i < n_items;
            const int b = valid ? (int)(i / lanes) : 0, k = valid ? (int)(i % lanes) : 0;
            const bool live = valid && k < n_vec;
            const T* xr = x + (int64_t)b * ldx;
            const T* gr = gout + (int64_t)b * ldg;
            if (valid)
                for (int j = k; j < n_non; j += lanes) gx[(int64_t)b * ldgx + nidx[j]] = gr[j];
            // (an item past the end is a zero vector with a zero cotangent: it adds exact zeros to every sum)
#pragma unroll
            for (int c = 0; c < FLIP_MAX_DIM; ++c) {
                v[it][c] = (live && c < d) ? xr[eidx[k * d + c]] : (T)0;
                dv[it][c] = (T)0;
            }
#pragma unroll
            for (int e = 0; e < EP; ++e) g[it][e] = (live && e < E) ? gr[n_non + (int64_t)k * E + e] : (T)0;
            T ep[EP], em[EP], ap, am;
            flip_networks<T, EP>(sW, d, H, v[it], ep, em, ap, am);
            flip_softmax(ap, am, wp[it], wm[it]);
            T dwp = (T)0, dwm = (T)0;
#pragma unroll
            for (int e = 0; e < EP; ++e) {
                dwp = flip_fma(g[it][e], ep[e], dwp);
                dwm = flip_fma(g[it][e], em[e], dwm);
                acc_b2e[e] += (double)(wp[it] * g[it][e]) + (double)(wm[it] * g[it][e]);
            }
            // softmax over a pair: da+ = w+ w- (dw+ - dw-) and da- = -da+ (the weights sum to one)
            dap[it] = wp[it] * wm[it] * (dwp - dwm);
            acc_b2w += (double)dap[it] + (double)(-dap[it]);
        }

        // ---- per hidden unit: recompute its activations, sum the gradients of its record
        for (int h = 0; h < H; ++h) {
            const T* rec = sW + h * R;
            const T b1e = rec[d], b1w = rec[2 * d + 1], w2w = rec[2 * d + 2];
            const T* w2e = rec + 2 * d + 3;
            double acc_w1e[FLIP_MAX_DIM], acc_w1w[FLIP_MAX_DIM], acc_w2e[EP], acc_b1e = 0.0, acc_b1w = 0.0, acc_w2w = 0.0;
#pragma unroll
            for (int c = 0; c < FLIP_MAX_DIM; ++c) acc_w1e[c] = acc_w1w[c] = 0.0;
#pragma unroll
            for (int e = 0; e < EP; ++e) acc_w2e[e] = 0.0;
#pragma unroll
            for (int it = 0; it < ITEMS; ++it) {
                const T u = flip_dot(rec, v[it], d), q = flip_dot(rec + d + 1, v[it], d);
                const T zp = b1e + u, zm = b1e - u, yp = b1w + q, ym = b1w - q;
                const T hp = flip_elu(zp), hm = flip_elu(zm), hpw = flip_elu(yp), hmw = flip_elu(ym);
                T G = (T)0;                                    // cotangent of e+ / w+ (= of e- / w-) at this hidden unit
#pragma unroll
                for (int e = 0; e < EP; ++e) G = flip_fma(g[it][e], w2e[e], G);
                const T dzp = wp[it] * G * flip_elu_grad(zp, hp), dzm = wm[it] * G * flip_elu_grad(zm, hm);
                const T dyp = dap[it] * w2w * flip_elu_grad(yp, hpw), dym = -dap[it] * w2w * flip_elu_grad(ym, hmw);
                const T du = dzp - dzm, dq = dyp - dym;
                acc_b1e += (double)dzp + (double)dzm;
                acc_b1w += (double)dyp + (double)dym;
                acc_w2w += (double)(dap[it] * hpw) + (double)(-dap[it] * hmw);
                const T mixed_h = flip_fma(wp[it], hp, wm[it] * hm);
#pragma unroll
                for (int e = 0; e < EP; ++e) acc_w2e[e] += (double)(g[it][e] * mixed_h);
#pragma unroll
                for (int c = 0; c < FLIP_MAX_DIM; ++c)
                    if (c < d) {
                        acc_w1e[c] += (double)(du * v[it][c]);
                        acc_w1w[c] += (double)(dq * v[it][c]);
                        dv[it][c] = flip_fma(du, rec[c], flip_fma(dq, rec[d + 1 + c], dv[it][c]));
                    }
            }
#pragma unroll
            for (int c = 0; c < FLIP_MAX_DIM; ++c)
                if (c < d) {
                    flip_wave_store(acc_w1e[c], red, c);
                    flip_wave_store(acc_w1w[c], red, d + 1 + c);
                }
            flip_wave_store(acc_b1e, red, d);
            flip_wave_store(acc_b1w, red, 2 * d + 1);
            flip_wave_store(acc_w2w, red, 2 * d + 2);
#pragma unroll
            for (int e = 0; e < EP; ++e) flip_wave_store(acc_w2e[e], red, 2 * d + 3 + e);
            flip_block_store<RMAX>(sRed, R, mine + h * R, first);
        }
#pragma unroll
        for (int e = 0; e < EP; ++e) flip_wave_store(acc_b2e[e], red, e);
        flip_wave_store(acc_b2w, red, EP);
        flip_block_store<RMAX>(sRed, EP + 1, mine + H * R, first);

        // ---- cotangent of the embedded columns
#pragma unroll
        for (int it = 0; it < ITEMS; ++it) {
            const int64_t i = base + (int64_t)it * 256 + threadIdx.x;
            if (i < n_items && (int)(i % lanes) < n_vec) {
                const int b = (int)(i / lanes), k = (int)(i % lanes);
#pragma unroll
                for (int c = 0; c < FLIP_MAX_DIM; ++c)
                    if (c < d) gx[(int64_t)b * ldgx + eidx[k * d + c]] = dv[it][c];
            }
        }
    }
}

// Workspace rows added in row order; one thread per parameter.
template <typename T>
__global__ void __launch_bounds__(256) flipembed_reduce_kernel(const double* __restrict__ partial, int n_rows, int d, int H,
                                                               int E, int EP, FlipNets<T> grads, int accumulate) {
    const int n = flip_staged(d, H, EP);
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    T* dst = flip_locate<T>(grads, p, d, H, E, EP);
    if (!dst) return;
    double s = 0.0;
    for (int r = 0; r < n_rows; ++r) s += partial[(int64_t)r * n + p];
    *dst = accumulate ? (T)((double)*dst + s) : (T)s;
}

static int flip_check_sizes(const char* who, int n_emb, int n_non, int d, int H, int E, int B) {
    TFEP_REQUIRE(B >= 0 && n_emb >= 0 && n_non >= 0, "%s: negative size", who);
    TFEP_REQUIRE(d >= 1 && d <= FLIP_MAX_DIM, "%s: vector_dim=%d unsupported (1..%d)", who, d, FLIP_MAX_DIM);
    TFEP_REQUIRE(H >= 1 && H <= FLIP_MAX_HIDDEN, "%s: hidden=%d unsupported (1..%d)", who, H, FLIP_MAX_HIDDEN);
    TFEP_REQUIRE(E >= 1 && E <= FLIP_MAX_EMB, "%s: emb_dim=%d unsupported (1..%d)", who, E, FLIP_MAX_EMB);
    TFEP_REQUIRE(n_emb % d == 0, "%s: n_embedded=%d is not a multiple of vector_dim=%d", who, n_emb, d);
    return TFEP_OK;
}

template <typename T>
static bool flip_nets_complete(const FlipNets<T>& n) {
    return n.emb_w1 && n.emb_b1 && n.emb_w2 && n.emb_b2 && n.wgt_w1 && n.wgt_b1 && n.wgt_w2 && n.wgt_b2;
}

template <typename T>
static int launch_flipembed(const char* who, const T* x, int64_t ldx, const int32_t* eidx, int n_emb, const int32_t* nidx,
                            int n_non, int d, int H, int E, FlipNets<const T> nets, T* out, int64_t ldo, int B, void* stream) {
    if (int rc = flip_check_sizes(who, n_emb, n_non, d, H, E, B)) return rc;
    if (B == 0 || n_emb + n_non == 0) return TFEP_OK;
    TFEP_REQUIRE(x && out, "%s: x/out must be non-NULL", who);
    TFEP_REQUIRE(n_emb == 0 || eidx, "%s: embedded_indices is NULL", who);
    TFEP_REQUIRE(n_non == 0 || nidx, "%s: nonembedded_indices is NULL", who);
    TFEP_REQUIRE(flip_nets_complete(nets), "%s: a parameter pointer is NULL", who);
    const int n_vec = n_emb / d;
    const int64_t n = (int64_t)B * (n_vec > 0 ? n_vec : 1);
    const int64_t blocks = (n + 255) / 256;
    TFEP_REQUIRE(blocks <= 0x7fffffffLL, "%s: batch too large", who);
    const int EP = flip_ep(E);
    auto kernel = EP == 4 ? flipembed_forward_kernel<T, 4> : EP == 8 ? flipembed_forward_kernel<T, 8>
                : EP == 16 ? flipembed_forward_kernel<T, 16> : flipembed_forward_kernel<T, 32>;
    kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, ldx, eidx, n_vec, nidx, n_non, d, H, E, nets, out, ldo, B);
    return check_launch("flipembed_forward_kernel");
}

template <typename T>
static int launch_flipembed_backward(const char* who, const T* x, int64_t ldx, const int32_t* eidx, int n_emb,
                                     const int32_t* nidx, int n_non, int d, int H, int E, FlipNets<const T> nets,
                                     const T* gout, int64_t ldg, T* gx, int64_t ldgx, FlipNets<T> grads, int accumulate,
                                     double* workspace, int B, void* stream) {
    if (int rc = flip_check_sizes(who, n_emb, n_non, d, H, E, B)) return rc;
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(x && gout && gx, "%s: x/gout/gx must be non-NULL", who);
    TFEP_REQUIRE(n_emb == 0 || eidx, "%s: embedded_indices is NULL", who);
    TFEP_REQUIRE(n_non == 0 || nidx, "%s: nonembedded_indices is NULL", who);
    TFEP_REQUIRE(flip_nets_complete(nets), "%s: a parameter pointer is NULL", who);
    TFEP_REQUIRE(flip_nets_complete(grads), "%s: a gradient pointer is NULL", who);
    TFEP_REQUIRE(workspace, "%s: workspace is NULL", who);
    const int n_vec = n_emb / d;
    const int EP = flip_ep(E);
    const int blocks = flip_backward_blocks((int64_t)B * (n_vec > 0 ? n_vec : 1), EP);
    hipStream_t s = (hipStream_t)stream;
    auto kernel = EP == 4 ? flipembed_backward_kernel<T, 4, 4> : EP == 8 ? flipembed_backward_kernel<T, 8, 4>
                : EP == 16 ? flipembed_backward_kernel<T, 16, 2> : flipembed_backward_kernel<T, 32, 1>;
    kernel<<<blocks, 256, 0, s>>>(x, ldx, eidx, n_vec, nidx, n_non, d, H, E, nets, gout, ldg, gx, ldgx, workspace, B);
    if (int rc = check_launch("flipembed_backward_kernel")) return rc;
    const int n = flip_staged(d, H, EP);
    flipembed_reduce_kernel<T><<<(n + 255) / 256, 256, 0, s>>>(workspace, blocks, d, H, E, EP, grads, accumulate);
    return check_launch("flipembed_reduce_kernel");
}

}  // namespace tfep

using namespace tfep;

#define FLIP_NETS(T, p) FlipNets<T>{p##emb_w1, p##emb_b1, p##emb_w2, p##emb_b2, p##wgt_w1, p##wgt_b1, p##wgt_w2, p##wgt_b2}

extern "C" {

int64_t tfep_flip_invariant_embedding_backward_workspace_bytes(int B, int n_embedded, int vector_dim, int hidden, int emb_dim) {
    if (B < 0 || n_embedded < 0 || vector_dim < 1 || vector_dim > FLIP_MAX_DIM || hidden < 1 || hidden > FLIP_MAX_HIDDEN ||
        emb_dim < 1 || emb_dim > FLIP_MAX_EMB || n_embedded % vector_dim != 0)
        return fail(TFEP_ERR_INVALID_ARGUMENT, "flip_invariant_embedding_backward_workspace_bytes: unsupported sizes");
    const int EP = flip_ep(emb_dim), n_vec = n_embedded / vector_dim;
    const int blocks = flip_backward_blocks((int64_t)B * (n_vec > 0 ? n_vec : 1), EP);
    return (int64_t)blocks * flip_staged(vector_dim, hidden, EP) * (int64_t)sizeof(double);
}

int tfep_flip_invariant_embedding(const float* x, int64_t ldx, const int32_t* embedded_indices, int n_embedded,
                                  const int32_t* nonembedded_indices, int n_nonembedded, int vector_dim, int hidden,
                                  int emb_dim, const float* emb_w1, const float* emb_b1, const float* emb_w2,
                                  const float* emb_b2, const float* wgt_w1, const float* wgt_b1, const float* wgt_w2,
                                  const float* wgt_b2, float* out, int64_t ldo, int B, void* stream) {
    return launch_flipembed<float>("flip_invariant_embedding", x, ldx, embedded_indices, n_embedded, nonembedded_indices,
                                   n_nonembedded, vector_dim, hidden, emb_dim, FLIP_NETS(const float, ), out, ldo, B, stream);
}

int tfep_flip_invariant_embedding_f64(const double* x, int64_t ldx, const int32_t* embedded_indices, int n_embedded,
                                      const int32_t* nonembedded_indices, int n_nonembedded, int vector_dim, int hidden,
                                      int emb_dim, const double* emb_w1, const double* emb_b1, const double* emb_w2,
                                      const double* emb_b2, const double* wgt_w1, const double* wgt_b1, const double* wgt_w2,
                                      const double* wgt_b2, double* out, int64_t ldo, int B, void* stream) {
    return launch_flipembed<double>("flip_invariant_embedding_f64", x, ldx, embedded_indices, n_embedded, nonembedded_indices,
                                    n_nonembedded, vector_dim, hidden, emb_dim, FLIP_NETS(const double, ), out, ldo, B,
                                    stream);
}

int tfep_flip_invariant_embedding_backward(const float* x, int64_t ldx, const int32_t* embedded_indices, int n_embedded,
                                           const int32_t* nonembedded_indices, int n_nonembedded, int vector_dim,
                                           int hidden, int emb_dim, const float* emb_w1, const float* emb_b1,
                                           const float* emb_w2, const float* emb_b2, const float* wgt_w1,
                                           const float* wgt_b1, const float* wgt_w2, const float* wgt_b2, const float* gout,
                                           int64_t ldg, float* gx, int64_t ldgx, float* g_emb_w1, float* g_emb_b1,
                                           float* g_emb_w2, float* g_emb_b2, float* g_wgt_w1, float* g_wgt_b1,
                                           float* g_wgt_w2, float* g_wgt_b2, int accumulate, double* workspace, int B,
                                           void* stream) {
    return launch_flipembed_backward<float>("flip_invariant_embedding_backward", x, ldx, embedded_indices, n_embedded,
                                            nonembedded_indices, n_nonembedded, vector_dim, hidden, emb_dim,
                                            FLIP_NETS(const float, ), gout, ldg, gx, ldgx, FLIP_NETS(float, g_), accumulate,
                                            workspace, B, stream);
}

int tfep_flip_invariant_embedding_backward_f64(const double* x, int64_t ldx, const int32_t* embedded_indices, int n_embedded,
                                               const int32_t* nonembedded_indices, int n_nonembedded, int vector_dim,
                                               int hidden, int emb_dim, const double* emb_w1, const double* emb_b1,
                                               const double* emb_w2, const double* emb_b2, const double* wgt_w1,
                                               const double* wgt_b1, const double* wgt_w2, const double* wgt_b2,
                                               const double* gout, int64_t ldg, double* gx, int64_t ldgx, double* g_emb_w1,
                                               double* g_emb_b1, double* g_emb_w2, double* g_emb_b2, double* g_wgt_w1,
                                               double* g_wgt_b1, double* g_wgt_w2, double* g_wgt_b2, int accumulate,
                                               double* workspace, int B, void* stream) {
    return launch_flipembed_backward<double>("flip_invariant_embedding_backward_f64", x, ldx, embedded_indices, n_embedded,
                                             nonembedded_indices, n_nonembedded, vector_dim, hidden, emb_dim,
                                             FLIP_NETS(const double, ), gout, ldg, gx, ldgx, FLIP_NETS(double, g_),
                                             accumulate, workspace, B, stream);
}

}  // extern "C"
