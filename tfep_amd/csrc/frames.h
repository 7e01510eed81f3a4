// Rigid-frame arithmetic of the Cartesian flow wrappers (reference utils/geometry.py:296-411, flows/centroid.py,
// flows/oriented.py), shared by the kernels of frames.hip.  Everything here is per sample row and in fp64, whatever the
// element type of the tensors (as symmoebius.h / quatprod.h): a float32 row is widened on load and rounded once on store.
//
// The frame rotation R = R2 R1 of a row is a function of two of its points, the axis point a and the plane point p:
//   u  = +-a / |a|, the sign that makes c = u . e_axis >= 0 (the nearer half-axis, project_on_positive_axis=False)
//   R1 = I + [w]x + [w]x^2 / (1 + c),  w = u x e_axis            (Rodrigues with sin = |w|, cos = c; 1 + c >= 1)
//   q  = R1 p,  q_p = q . e_plane,  q_n = q . n                   (n: the signed unit normal of the plane)
//   R2 = cos I + sin [e_axis]x + (1 - cos) e_axis e_axis^T,  cos = |q_p| / |(q_p, q_n)|,  sin = -sign(q_p) q_n / |(q_p, q_n)|
//        and R2 = I when q_p == 0 exactly (the sign(q_p) == 0 branch of the torch code)
// Degenerate geometry is not special-cased: a zero-length axis point divides 0 by 0 and every entry of R is NaN, as the
// torch code gives; so does a plane point on the axis with q_p != 0 rounded to it (|(q_p, q_n)| = 0 is reached only with
// q_p == 0, which is the identity branch).
//
// frame_rotation<false> is the project_on_positive_axis=True variant (relframe.h): u = a / |a| with no flip, c in [-1, 1],
// and when 1 + c <= 1e-12 (a antiparallel to e_axis) R1 is the rotation by pi about e_plane x e_axis, 2 n n^T - I -- a
// constant, so that branch has zero derivative with respect to a, as torch.where gives it.  The default, <true>, is the
// arithmetic above, unchanged.
//
// frame_rotation_vjp is the reverse-mode derivative of frame_rotation, written out by hand: the cotangent of R (row-major
// 3 x 3) gives the cotangents of a and p.  The q_p == 0 branch has zero derivative with respect to q, as torch.where
// gives it.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace tfep {

constexpr int FRAME_ROWS = 4;               // rows (waves) per workgroup of the kernels of frames.hip and relframe.hip

// The frame in small integers: `axis` and `plane_axis` in 0..2 (x, y, z), `normal` = +-(1 + index of the third axis), the
// sign that of the plane normal (for OrientedFlow: e_axis x e_plane).
struct FrameAxes {
    int axis, plane_axis, normal;
};

__host__ __device__ inline bool frame_axes_valid(const FrameAxes& f) {
    const int n = (f.normal < 0 ? -f.normal : f.normal) - 1;
    return f.axis >= 0 && f.axis < 3 && f.plane_axis >= 0 && f.plane_axis < 3 && n >= 0 && n < 3 && f.axis != f.plane_axis &&
           n != f.axis && n != f.plane_axis;
}

// What frame_rotation_vjp needs of the forward.
struct FrameState {
    double na, flip, u0[3], K[3][3], s, r1[3][3], r2[3][3], qp, qn, qnorm, sgn;
    bool antiparallel;          // (frame_rotation<false> only: R1 is the constant rotation by pi)
};

// v[i] for a run-time i, without indexing a register array dynamically
__host__ __device__ inline double sel3(const double (&v)[3], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : v[2]; }
__host__ __device__ inline void unit3(int i, double (&e)[3]) { e[0] = i == 0, e[1] = i == 1, e[2] = i == 2; }

__host__ __device__ inline void mat3_mul(const double (&a)[3][3], const double (&b)[3][3], double (&c)[3][3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[i][j] = a[i][0] * b[0][j] + a[i][1] * b[1][j] + a[i][2] * b[2][j];
}

__host__ __device__ inline void skew3(const double (&w)[3], double (&K)[3][3]) {
    K[0][0] = 0.0, K[0][1] = -w[2], K[0][2] = w[1];
    K[1][0] = w[2], K[1][1] = 0.0, K[1][2] = -w[0];
    K[2][0] = -w[1], K[2][1] = w[0], K[2][2] = 0.0;
}

template <bool FLIP = true>
__host__ __device__ inline void frame_rotation(const double (&a)[3], const double (&p)[3], const FrameAxes& f,
                                               double (&R)[3][3], FrameState& st) {
    const int ax = f.axis, pl = f.plane_axis, nn = (f.normal < 0 ? -f.normal : f.normal) - 1;
    const double sn = f.normal < 0 ? -1.0 : 1.0;
    st.na = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    double u[3], e[3];
    unit3(ax, e);
#pragma unroll
    for (int i = 0; i < 3; ++i) st.u0[i] = a[i] / st.na;
    st.flip = (FLIP && sel3(st.u0, ax) < 0.0) ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = st.u0[i] * st.flip;
    const double c = sel3(u, ax);
    const double w[3] = {u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]};
    skew3(w, st.K);
    double KK[3][3];
    mat3_mul(st.K, st.K, KK);
    const double denom = 1.0 + c;
    st.s = 1.0 / (denom > 1e-12 ? denom : 1.0);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) st.r1[i][j] = (i == j ? 1.0 : 0.0) + st.K[i][j] + KK[i][j] * st.s;
    st.antiparallel = !FLIP && !(denom > 1e-12);
    if (st.antiparallel) {                        // n = e_plane x e_axis = -sn e_normal: 2 n n^T - I
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) st.r1[i][j] = (i == j ? (i == nn ? 1.0 : -1.0) : 0.0);
    }
    double q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = st.r1[i][0] * p[0] + st.r1[i][1] * p[1] + st.r1[i][2] * p[2];
    st.qp = sel3(q, pl);
    st.qn = sn * sel3(q, nn);
    st.qnorm = sqrt(st.qp * st.qp + st.qn * st.qn);
    double cos2 = 1.0, sin2 = 0.0;
    st.sgn = 0.0;
    if (st.qp != 0.0) {                           // (a NaN q_p takes this branch and stays NaN)
        st.sgn = st.qp < 0.0 ? -1.0 : 1.0;
        cos2 = fabs(st.qp) / st.qnorm;
        sin2 = -st.sgn * st.qn / st.qnorm;
    }
    double Kx[3][3];
    skew3(e, Kx);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            st.r2[i][j] = (i == j ? cos2 : 0.0) + sin2 * Kx[i][j] + ((i == ax && j == ax) ? 1.0 - cos2 : 0.0);
    mat3_mul(st.r2, st.r1, R);
}

// Cotangents of the axis point (ga) and the plane point (gp) from the cotangent G of R.
template <bool FLIP = true>
__host__ __device__ inline void frame_rotation_vjp(const double (&p)[3], const FrameAxes& f, const FrameState& st,
                                                   const double (&G)[3][3], double (&ga)[3], double (&gp)[3]) {
    const int ax = f.axis, pl = f.plane_axis, nn = (f.normal < 0 ? -f.normal : f.normal) - 1;
    const double sn = f.normal < 0 ? -1.0 : 1.0;
    double e[3];
    unit3(ax, e);
    // R = r2 r1
    double G2[3][3], G1[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            G2[i][j] = G[i][0] * st.r1[j][0] + G[i][1] * st.r1[j][1] + G[i][2] * st.r1[j][2];       // G r1^T
            G1[i][j] = st.r2[0][i] * G[0][j] + st.r2[1][i] * G[1][j] + st.r2[2][i] * G[2][j];       // r2^T G
        }
    // r2 = cos I + sin [e]x + (1 - cos) e e^T
    double Kx[3][3];
    skew3(e, Kx);
    const double g_cos = (ax == 0 ? 0.0 : G2[0][0]) + (ax == 1 ? 0.0 : G2[1][1]) + (ax == 2 ? 0.0 : G2[2][2]);
    double g_sin = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) g_sin += G2[i][j] * Kx[i][j];
    double g_qp = 0.0, g_qn = 0.0;
    if (st.qp != 0.0) {
        const double n3 = st.qnorm * st.qnorm * st.qnorm;
        g_qp = st.sgn * st.qn * (g_cos * st.qn + g_sin * st.qp) / n3;
        g_qn = -st.sgn * st.qp * (g_cos * st.qn + g_sin * st.qp) / n3;
    }
    double gq[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) gq[i] = (i == pl ? g_qp : 0.0) + (i == nn ? sn * g_qn : 0.0);
    // q = r1 p
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gp[i] = st.r1[0][i] * gq[0] + st.r1[1][i] * gq[1] + st.r1[2][i] * gq[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) G1[i][j] += gq[i] * p[j];
    }
    if (!FLIP && st.antiparallel) {               // r1 is a constant
        ga[0] = ga[1] = ga[2] = 0.0;
        return;
    }
    // r1 = I + K + s K K
    double KK[3][3], GK[3][3];
    mat3_mul(st.K, st.K, KK);
    double g_s = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g_s += G1[i][j] * KK[i][j];
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) t += G1[i][k] * st.K[j][k] + st.K[k][i] * G1[k][j];       // G K^T + K^T G
            GK[i][j] = G1[i][j] + st.s * t;
        }
    const double g_c = -g_s * st.s * st.s;
    // K = [w]x, w = u x e, c = u . e, u = flip u0, u0 = a / |a|
    const double gw[3] = {GK[2][1] - GK[1][2], GK[0][2] - GK[2][0], GK[1][0] - GK[0][1]};
    double gu0[3] = {e[1] * gw[2] - e[2] * gw[1], e[2] * gw[0] - e[0] * gw[2], e[0] * gw[1] - e[1] * gw[0]};
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        gu0[i] = st.flip * (gu0[i] + g_c * e[i]);
        dot += st.u0[i] * gu0[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) ga[i] = (gu0[i] - st.u0[i] * dot) / st.na;
}

}  // namespace tfep
