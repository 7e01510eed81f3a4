// The counter-based resampling stream of the bootstrap kernels (csrc/reduce.hip).  Device
// functions only.
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) with
//   key     = (seed & 0xffffffff, seed >> 32)                       seed in [0, 2^63)
//   counter = (q & 0xffffffff, q >> 32, r, stream)                  r = global resample number < 2^31, q = group number
//   stream  = 0: indices, word k of group q is draw j = 4q + k, i_j = (uint64(word) * high) >> 32
//   stream  = 1: Bayesian weights, draw j takes words (a, b) = (2 (j % 2), 2 (j % 2) + 1) of group q = j / 2,
//                u_j = (((a >> 5) * 2^26 + (b >> 6)) + 0.5) * 2^-53 in fp64,  E_j = -log(u_j)
// A draw depends on (seed, r, j) alone: not on the batch, the grid or the lane that makes it.
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

namespace tfep {

constexpr uint32_t BOOTSTRAP_STREAM_INDICES = 0, BOOTSTRAP_STREAM_WEIGHTS = 1;

struct BootstrapStream {
    uint32_t key0, key1, r, stream;
};

__device__ inline BootstrapStream bootstrap_stream(int64_t seed, int64_t r, uint32_t stream) {
    return {(uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32), (uint32_t)r, stream};
}

__device__ inline void philox4x32_10(const uint32_t counter[4], uint32_t k0, uint32_t k1, uint32_t out[4]) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3];
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// the four words of group q
__device__ inline void bootstrap_words(const BootstrapStream& s, int64_t q, uint32_t out[4]) {
    const uint32_t counter[4] = {(uint32_t)((uint64_t)q & 0xffffffffu), (uint32_t)((uint64_t)q >> 32), s.r, s.stream};
    philox4x32_10(counter, s.key0, s.key1, out);
}

// multiply-high: in [0, high) for 1 <= high < 2^31, bias at most high / 2^32
__device__ inline int64_t bootstrap_index(uint32_t word, uint32_t high) { return (int64_t)__umulhi(word, high); }

// E = -log(u) of the pair of words (a, b): a standard exponential variate
__device__ inline double bootstrap_exponential(uint32_t a, uint32_t b) {
    const uint64_t bits = ((uint64_t)(a >> 5) << 26) + (uint64_t)(b >> 6);
    return -log(((double)bits + 0.5) * 0x1p-53);
}

// index draw j on its own (the replay of a single draw: the whole group is generated for it)
__device__ inline int64_t bootstrap_index_at(const BootstrapStream& s, int64_t j, uint32_t high) {
    uint32_t w[4];
    bootstrap_words(s, j >> 2, w);
    const int k = (int)(j & 3);                                  // selects, not a dynamic index into registers
    return bootstrap_index(k == 0 ? w[0] : k == 1 ? w[1] : k == 2 ? w[2] : w[3], high);
}

__device__ inline double bootstrap_exponential_at(const BootstrapStream& s, int64_t j) {
    uint32_t w[4];
    bootstrap_words(s, j >> 1, w);
    return (j & 1) ? bootstrap_exponential(w[2], w[3]) : bootstrap_exponential(w[0], w[1]);
}

}  // namespace tfep
