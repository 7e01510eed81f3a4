// Periodic embedding (mafembed.py:112-145) and its VJP, float32 and float64: the forward is launched from transformers.hip,
// the VJP from backward.hip.
#pragma once

#include "common.h"

namespace tfep {

// out = [x_non..., cos t, sin t, ...], t = (x - lower) * scale; backward: gx[p] = (-sin t g_cos + cos t g_sin) * scale.
// One thread per (row, source feature).
template <typename T, bool BACKWARD>
__global__ void __launch_bounds__(256) periodic_embedding_kernel(const T* __restrict__ x, int64_t ldx,
                                                                 const int32_t* __restrict__ pidx, int n_per,
                                                                 const int32_t* __restrict__ nidx, int n_non, T lower,
                                                                 T scale, const T* __restrict__ gout, int64_t ldg,
                                                                 T* __restrict__ out, int64_t ldo, int B) {
    const int n_src = n_non + n_per;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * n_src) return;
    const int b = (int)(i / n_src), j = (int)(i % n_src);
    if (j < n_non) {
        if (BACKWARD)
            out[(int64_t)b * ldo + nidx[j]] = gout[(int64_t)b * ldg + j];
        else
            out[(int64_t)b * ldo + j] = x[(int64_t)b * ldx + nidx[j]];
    } else {
        const int q = j - n_non;
        const T t = (x[(int64_t)b * ldx + pidx[q]] - lower) * scale;
        T s, c;
        sincos(t, &s, &c);
        if (BACKWARD) {
            const T gc = gout[(int64_t)b * ldg + n_non + 2 * q], gs = gout[(int64_t)b * ldg + n_non + 2 * q + 1];
            out[(int64_t)b * ldo + pidx[q]] = (-s * gc + c * gs) * scale;
        } else {
            out[(int64_t)b * ldo + n_non + 2 * q] = c;
            out[(int64_t)b * ldo + n_non + 2 * q + 1] = s;
        }
    }
}

// 2 pi / (upper - lower), formed in double
template <typename T>
inline T embedding_scale(T lower, T upper) {
    return (T)(2.0 * 3.14159265358979323846 / ((double)upper - (double)lower));
}

}  // namespace tfep
