// Flip-invariant embedding of one vector (reference embeddings/mafembed.py:174-348; Koehler et al. 2023, SI eq. 46), shared
// by the forward and the backward kernel of flipembed.hip.
//
// For a vector v of d components and two perceptrons d -> H -> E ("embedding") and d -> H -> 1 ("weight"), ELU between:
//   u = W1e v,   e+- = W2e ELU(b1e +- u) + b2e        (the first-layer product is shared between v and -v)
//   q = W1w v,   a+- = W2w ELU(b1w +- q) + b2w
//   w+- = softmax(a+, a-),   out = w+ e+ + w- e-
//
// Bitwise flip invariance.  Negating v negates u and q exactly (a chain of fmas on negated operands), so the "+" and "-"
// branches swap their inputs, and every step below applies the SAME instruction sequence to both branches: they swap their
// results bit for bit.  The two steps that combine the branches are symmetric under the swap: the softmax normaliser is one
// commutative add, and the output is two separately rounded products and one add (flip_mix, contraction off -- an fma of
// one product into the other is not symmetric).
//
// Parameters in LDS.  A workgroup stages both networks once, one record of R = 2 d + 3 + EP values per hidden unit h:
//   [W1e[h][0..d) | b1e[h] | W1w[h][0..d) | b1w[h] | W2w[h] | W2e[0..EP)[h]]      then  [b2e[0..EP) | b2w]
// EP >= E is the compile-time bound of the kernel instance; the entries e >= E are zero.  Every lane of a wave reads the
// same address (a broadcast, no bank conflict), and a hidden unit's values are contiguous.  The loops run over the hidden
// units and accumulate the E outputs: the hidden vectors never exist as a whole.
//
// T is the element type AND the arithmetic: float kernels compute in fp32 (fmaf, expm1f, expf), double kernels in IEEE
// fp64 with the library expm1 / exp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tfep {

constexpr int FLIP_MAX_DIM = 8;         // vector_dimension
constexpr int FLIP_MAX_HIDDEN = 64;     // hidden_layer_width
constexpr int FLIP_MAX_EMB = 32;        // embedding_dimension

// The eight parameter tensors in torch.nn.Linear layout (weight: out x in, row-major), or their gradients.
template <typename T>
struct FlipNets {
    T* emb_w1;   // (H, d)   embedding_layer.0.weight
    T* emb_b1;   // (H)      embedding_layer.0.bias
    T* emb_w2;   // (E, H)   embedding_layer.2.weight
    T* emb_b2;   // (E)      embedding_layer.2.bias
    T* wgt_w1;   // (H, d)   weight_layer.0.weight
    T* wgt_b1;   // (H)      weight_layer.0.bias
    T* wgt_w2;   // (1, H)   weight_layer.2.weight
    T* wgt_b2;   // (1)      weight_layer.2.bias
};

__host__ __device__ constexpr int flip_record(int d, int EP) { return 2 * d + 3 + EP; }
__host__ __device__ constexpr int flip_staged(int d, int H, int EP) { return H * flip_record(d, EP) + EP + 1; }

// The element of the staged image at position p, as a pointer into the parameter (or gradient) tensors; nullptr for the
// zero padding e >= E.
template <typename T>
__device__ __forceinline__ T* flip_locate(const FlipNets<T>& n, int p, int d, int H, int E, int EP) {
    const int R = flip_record(d, EP);
    if (p < H * R) {
        const int h = p / R, j = p % R;
        if (j < d) return n.emb_w1 + h * d + j;
        if (j == d) return n.emb_b1 + h;
        if (j < 2 * d + 1) return n.wgt_w1 + h * d + (j - d - 1);
        if (j == 2 * d + 1) return n.wgt_b1 + h;
        if (j == 2 * d + 2) return n.wgt_w2 + h;
        const int e = j - (2 * d + 3);
        return e < E ? n.emb_w2 + e * H + h : nullptr;
    }
    const int e = p - H * R;
    if (e < EP) return e < E ? n.emb_b2 + e : nullptr;
    return n.wgt_b2;
}

// Stage both networks (every thread of the workgroup takes part; the caller synchronises).
template <typename T, int EP>
__device__ __forceinline__ void flip_stage(T* __restrict__ sW, const FlipNets<const T>& nets, int d, int H, int E) {
    const int n = flip_staged(d, H, EP);
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        const T* src = flip_locate<const T>(nets, p, d, H, E, EP);
        sW[p] = src ? *src : (T)0;
    }
}

__device__ __forceinline__ float flip_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double flip_fma(double a, double b, double c) { return ::fma(a, b, c); }
__device__ __forceinline__ float flip_expm1(float a) { return expm1f(a); }
__device__ __forceinline__ double flip_expm1(double a) { return ::expm1(a); }
__device__ __forceinline__ float flip_exp(float a) { return expf(a); }
__device__ __forceinline__ double flip_exp(double a) { return ::exp(a); }
__device__ __forceinline__ float flip_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double flip_max(double a, double b) { return ::fmax(a, b); }

template <typename T> __device__ __forceinline__ T flip_elu(T z) { return z > (T)0 ? z : flip_expm1(z); }
// ELU'(z) from z and ELU(z): 1, or exp(z) = ELU(z) + 1
template <typename T> __device__ __forceinline__ T flip_elu_grad(T z, T elu) { return z > (T)0 ? (T)1 : elu + (T)1; }

// W1 v over the first d components (fmas in a fixed order: W1 (-v) = -(W1 v) bit for bit)
template <typename T>
__device__ __forceinline__ T flip_dot(const T* __restrict__ w, const T (&v)[FLIP_MAX_DIM], int d) {
    T u = w[0] * v[0];
#pragma unroll
    for (int i = 1; i < FLIP_MAX_DIM; ++i)
        if (i < d) u = flip_fma(w[i], v[i], u);
    return u;
}

// First pass over the hidden units: the candidate embeddings e+ (ep), e- (em) and the pre-softmax weights a+, a-.
template <typename T, int EP>
__device__ __forceinline__ void flip_networks(const T* __restrict__ sW, int d, int H, const T (&v)[FLIP_MAX_DIM], T (&ep)[EP],
                                              T (&em)[EP], T& ap, T& am) {
    const int R = flip_record(d, EP);
    const T* tail = sW + H * R;
#pragma unroll
    for (int e = 0; e < EP; ++e) ep[e] = em[e] = tail[e];
    ap = am = tail[EP];
    for (int h = 0; h < H; ++h) {
        const T* rec = sW + h * R;
        const T u = flip_dot(rec, v, d), b1e = rec[d];
        const T q = flip_dot(rec + d + 1, v, d), b1w = rec[2 * d + 1], w2w = rec[2 * d + 2];
        const T hp = flip_elu(b1e + u), hm = flip_elu(b1e - u);
        ap = flip_fma(w2w, flip_elu(b1w + q), ap);
        am = flip_fma(w2w, flip_elu(b1w - q), am);
        const T* w2e = rec + 2 * d + 3;
#pragma unroll
        for (int e = 0; e < EP; ++e) {
            ep[e] = flip_fma(w2e[e], hp, ep[e]);
            em[e] = flip_fma(w2e[e], hm, em[e]);
        }
    }
}

// softmax over the pair, symmetric under the swap of the branches
template <typename T>
__device__ __forceinline__ void flip_softmax(T ap, T am, T& wp, T& wm) {
    const T mx = flip_max(ap, am);
    const T xp = flip_exp(ap - mx), xm = flip_exp(am - mx);
    const T s = xp + xm;
    wp = xp / s;
    wm = xm / s;
}

// w+ e+ + w- e-: two rounded products, one add (never contracted into an fma)
template <typename T>
__device__ __forceinline__ T flip_mix(T wp, T ep, T wm, T em) {
#pragma clang fp contract(off)
    const T a = wp * ep;
    const T b = wm * em;
    return a + b;
}

}  // namespace tfep
