// Sum-of-squares polynomial transformer (reference transformers/sos.py): the element functions shared by the standalone
// kernels (transformers.hip, float and double) and the fused epilogue of the MADE output GEMM (gemm_common.h).
//
// K squared linear polynomials per feature, P = 2 K + 1 parameters: prm(0) = a0, prm(1 + 2k) = a_k0, prm(2 + 2k) = a_k1.
//   y     = a0 + x (s0 + s1 x + s2 x^2),   s0 = sum a_k0^2, s1 = sum a_k0 a_k1, s2 = sum a_k1^2 / 3    (sos.py:198-219, :261-265)
//   dy/dx = sum_k (a_k0 + a_k1 x)^2
// dy/dx is evaluated as the sum of squares, not as the expanded s0 + 2 s1 x + 3 s2 x^2 of the reference: in float32 the
// expanded form can round below zero where the polynomials nearly cancel, and its log is then NaN.
#pragma once

namespace tfep {

// KC > 0: K is the compile-time constant KC (the fused epilogue: prm indexes accumulator registers, every index must fold
// to a constant); KC = 0: K = K_rt at run time (the standalone kernels read the parameters from memory).
template <int KC, typename T, class F>
__device__ __forceinline__ T sos_element(int K_rt, F&& prm, T x, T* dydx) {
    const int K = KC > 0 ? KC : K_rt;
    T s0 = T(0), s1 = T(0), s2 = T(0), d = T(0);
#pragma unroll
    for (int k = 0; k < (KC > 0 ? KC : K); ++k) {
        const T a = prm(1 + 2 * k), b = prm(2 + 2 * k);
        s0 += a * a;
        s1 += a * b;
        s2 += b * b;
        const T q = a + b * x;
        d += q * q;
    }
    *dydx = d;
    // the reference's order: (c1 + c2 x + c3 x^2) x + c0 with c3 = s2 / 3
    return (s0 + s1 * x + (s2 / T(3)) * (x * x)) * x + prm(0);
}

// VJP of one element (SOSPolynomialTransformerFunc.backward, sos.py:226-257): put(p, g_p) receives the gradient of every
// parameter, the return value is g_x = gy dy/dx.  The log-det is non-differentiable in the reference (mark_non_differentiable):
// it contributes nothing here.
template <typename T, class F, class G>
__device__ __forceinline__ T sos_vjp_element(int K, F&& prm, G&& put, T x, T gy) {
    const T x2 = x * x, x3 = x2 * x;
    T d = T(0);
    put(0, gy);                                                       // d y / d a0 = 1
    for (int k = 0; k < K; ++k) {
        const T a = prm(1 + 2 * k), b = prm(2 + 2 * k);
        const T q = a + b * x;
        d += q * q;
        put(1 + 2 * k, (b * x2 + T(2) * a * x) * gy);                 // 2 a_k0 x + a_k1 x^2
        put(2 + 2 * k, (T(2.0 / 3.0) * b * x3 + a * x2) * gy);       // a_k0 x^2 + 2/3 a_k1 x^3
    }
    return d * gy;
}

}  // namespace tfep
