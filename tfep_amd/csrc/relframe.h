// The relative frame of the mixed (internal + Cartesian) coordinates (reference app/mixedmaf.py:1216-1271, 1321-1375): the
// Cartesian atoms of a row expressed in the frame of three of them, and back.  Per sample row and in fp64 whatever the
// element type, as frames.h; shared by the kernels of relframe.hip and by tools/relframe_host_check.cpp, which runs the
// same functions on the CPU (lane 0 of a stride of 1 is the whole row).
//
// A row x holds n_c >= 3 atoms; the LAST THREE are the origin atom o, the axis atom a and the plane atom p, in that order,
// the n_o = n_c - 3 before them are the other atoms.  `remove` says which rototranslational degrees of freedom (DOFs) of
// the three reference atoms are dropped from the coordinates: those of the origin (3), the axis atom (2), the plane atom (1).
//
// Encode: x -> (coords, origin, R, log_det_J)
//   origin = o,  R = R2 R1 = frame_rotation<false>(a - o, p - o) with e_axis = e_x, e_plane = e_y, normal +e_z (frames.h):
//       u = (a - o) / |a - o| with no flip, c = u . e_x in [-1, 1], R1 = I + [w]x + [w]x^2 / (1 + c), w = u x e_x;
//       when 1 + c <= 1e-12, R1 = 2 n n^T - I with n = e_y x e_x = -e_z (the rotation by pi); R2 as in frames.h
//   v_i = R (x_i - o) for every atom
//   d01 = (v_a)_x,  d02 = hypot((v_p)_x, (v_p)_y),  a102 = atan2((v_p)_y, (v_p)_x),  a102n = (a102 + pi) / (2 pi)
//   coords = [d01, d02, a102n | v_i of the other atoms, 3 each, in input order | kept reference DOFs]
//       kept reference DOFs, in this order: v_o (3; R (o - o), exact zeros) unless remove.origin, (v_a)_y and (v_a)_z
//       unless remove.axis, (v_p)_z unless remove.plane.  (v_a)_x, (v_p)_x and (v_p)_y never appear.
//       width = 3 + 3 n_o + kept
//   log_det_J = -log d02 - log 2 pi
// Decode: (coords, origin, R) -> (x, log_det_J)
//   a102 = 2 pi a102n - pi,  v_a = (d01, y, z),  v_p = (d02 cos a102, d02 sin a102, z),  v_o; a removed DOF is exactly 0, a
//   kept one is read from coords.  x_i = R^T v_i + o for every atom,  log_det_J = log 2 pi + log d02.
//
// The VJPs are written out by hand.  Encode: origin and R are outputs with cotangents of their own; the cotangent of R also
// collects sum_i g_{v_i} (x_i - o)^T and goes through frame_rotation_vjp<false> to the axis and plane atoms; the origin
// atom receives g_origin minus everything the other atoms receive through (x_i - o).  The kept DOFs of the origin are
// R (o - o): they have no derivative.  Decode: origin and R are inputs, g_origin = sum_i g_{x_i}, g_R = sum_i v_i g_{x_i}^T.
// A sum over the atoms is accumulated by each lane in atom order into acc[12]; the caller adds the lanes up (wave_sum in
// the kernels, nothing on the host) before the reference atoms are handled by lane 0.
//
// Degenerate geometry is not special-cased beyond the above: a zero-length axis vector gives NaN, as in frames.h; d02 = 0
// gives an infinite log-det; the antiparallel branch has the derivative torch.where gives it (R1 constant: nothing reaches
// the axis atom through R1).
#pragma once
#include "frames.h"

namespace tfep {

constexpr double RELFRAME_PI = 3.14159265358979323846;
constexpr double RELFRAME_TWO_PI = 6.28318530717958647692;
constexpr double RELFRAME_LOG_TWO_PI = 1.83787706640934548356;

// Which reference DOFs are dropped (non-zero: dropped).
struct RelRemove {
    int origin, axis, plane;
};

__host__ __device__ inline int relframe_kept(const RelRemove& rm) {
    return (rm.origin ? 0 : 3) + (rm.axis ? 0 : 2) + (rm.plane ? 0 : 1);
}
__host__ __device__ inline int64_t relframe_width(int n_c, const RelRemove& rm) {
    return 3 + 3 * (int64_t)(n_c - 3) + relframe_kept(rm);
}

// The frame of a row: the origin, the axis and plane vectors from it, the rotation and what its VJP needs.
struct RelFrameRow {
    double o[3], da[3], dp[3], R[3][3];
    FrameState st;
};

__host__ __device__ inline FrameAxes relframe_axes() { return FrameAxes{0, 1, 3}; }

// M v and M^T v
__host__ __device__ inline void mat3_vec(const double (&M)[3][3], const double (&v)[3], double (&o)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = M[r][0] * v[0] + M[r][1] * v[1] + M[r][2] * v[2];
}
__host__ __device__ inline void mat3t_vec(const double (&M)[3][3], const double (&v)[3], double (&o)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = M[0][c] * v[0] + M[1][c] * v[1] + M[2][c] * v[2];
}

template <typename T>
__host__ __device__ inline void relframe_load(const T* xr, int n_c, RelFrameRow& f) {
    const T *xo = xr + 3 * (n_c - 3), *xa = xo + 3, *xp = xo + 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        f.o[c] = (double)xo[c];
        f.da[c] = (double)xa[c] - f.o[c];
        f.dp[c] = (double)xp[c] - f.o[c];
    }
    frame_rotation<false>(f.da, f.dp, relframe_axes(), f.R, f.st);
}

template <typename T>
__host__ __device__ inline void relframe_encode_row(const T* xr, int n_c, const RelRemove& rm, int lane, int stride, T* cr,
                                                    T* origin, T* rot, T* ldj) {
    RelFrameRow f;
    relframe_load(xr, n_c, f);
    const int n_o = n_c - 3;
    for (int i = lane; i < n_o; i += stride) {
        const double d[3] = {(double)xr[3 * i] - f.o[0], (double)xr[3 * i + 1] - f.o[1], (double)xr[3 * i + 2] - f.o[2]};
        double v[3];
        mat3_vec(f.R, d, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) cr[3 + 3 * i + c] = (T)v[c];
    }
    if (lane != 0) return;
    double va[3], vp[3];
    mat3_vec(f.R, f.da, va);
    mat3_vec(f.R, f.dp, vp);
    const double d02 = hypot(vp[0], vp[1]);
    cr[0] = (T)va[0];
    cr[1] = (T)d02;
    cr[2] = (T)((atan2(vp[1], vp[0]) + RELFRAME_PI) / RELFRAME_TWO_PI);
    int k = 3 + 3 * n_o;
    if (!rm.origin) {
        cr[k] = cr[k + 1] = cr[k + 2] = (T)0;
        k += 3;
    }
    if (!rm.axis) {
        cr[k] = (T)va[1], cr[k + 1] = (T)va[2];
        k += 2;
    }
    if (!rm.plane) cr[k] = (T)vp[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        origin[r] = (T)f.o[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) rot[3 * r + c] = (T)f.R[r][c];
    }
    *ldj = (T)(-log(d02) - RELFRAME_LOG_TWO_PI);
}

// VJP of encode, the other atoms: gx_i = R^T g_{v_i}, and this lane's part of acc[3 r + c] = sum_i (g_{v_i})_r (x_i - o)_c
// and acc[9 + c] = sum_i (gx_i)_c.
template <typename T>
__host__ __device__ inline void relframe_encode_vjp_atoms(const T* xr, int n_c, const RelFrameRow& f, const T* gcr, int lane,
                                                          int stride, T* gxr, double (&acc)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (int i = lane; i < n_c - 3; i += stride) {
        const double d[3] = {(double)xr[3 * i] - f.o[0], (double)xr[3 * i + 1] - f.o[1], (double)xr[3 * i + 2] - f.o[2]};
        const double g[3] = {(double)gcr[3 + 3 * i], (double)gcr[3 + 3 * i + 1], (double)gcr[3 + 3 * i + 2]};
        double gx[3];
        mat3t_vec(f.R, g, gx);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gxr[3 * i + c] = (T)gx[c];
            acc[9 + c] += gx[c];
#pragma unroll
            for (int r = 0; r < 3; ++r) acc[3 * r + c] += g[r] * d[c];
        }
    }
}

// VJP of encode, the three reference atoms (one lane, with acc summed over the lanes).  g_origin, g_rot and g_ldj may be
// NULL (no cotangent).
template <typename T>
__host__ __device__ inline void relframe_encode_vjp_refs(int n_c, const RelRemove& rm, const RelFrameRow& f, const T* gcr,
                                                         const T* g_origin, const T* g_rot, const T* g_ldj,
                                                         const double (&acc)[12], T* gxr) {
    double va[3], vp[3];
    mat3_vec(f.R, f.da, va);
    mat3_vec(f.R, f.dp, vp);
    const double d02sq = vp[0] * vp[0] + vp[1] * vp[1], d02 = hypot(vp[0], vp[1]);
    int k = 3 + 3 * (n_c - 3) + (rm.origin ? 0 : 3);              // (the kept DOFs of the origin have no derivative)
    double gva[3] = {(double)gcr[0], 0.0, 0.0}, gvp[3] = {0.0, 0.0, 0.0};
    if (!rm.axis) {
        gva[1] = (double)gcr[k], gva[2] = (double)gcr[k + 1];
        k += 2;
    }
    if (!rm.plane) gvp[2] = (double)gcr[k];
    const double g_d02 = (double)gcr[1] - (g_ldj ? (double)*g_ldj : 0.0) / d02, g_a = (double)gcr[2] / RELFRAME_TWO_PI;
    gvp[0] = g_d02 * vp[0] / d02 - g_a * vp[1] / d02sq;
    gvp[1] = g_d02 * vp[1] / d02 + g_a * vp[0] / d02sq;
    double GR[3][3], ga[3], gp[3], gxa[3], gxp[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            GR[r][c] = acc[3 * r + c] + gva[r] * f.da[c] + gvp[r] * f.dp[c] + (g_rot ? (double)g_rot[3 * r + c] : 0.0);
    frame_rotation_vjp<false>(f.dp, relframe_axes(), f.st, GR, ga, gp);
    mat3t_vec(f.R, gva, gxa);
    mat3t_vec(f.R, gvp, gxp);
    T *go = gxr + 3 * (n_c - 3), *gxa_out = go + 3, *gxp_out = go + 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gxa[c] += ga[c];
        gxp[c] += gp[c];
        gxa_out[c] = (T)gxa[c];
        gxp_out[c] = (T)gxp[c];
        go[c] = (T)((g_origin ? (double)g_origin[c] : 0.0) - acc[9 + c] - gxa[c] - gxp[c]);
    }
}

// What decode reads of a row besides the other atoms: the frame and the three reference atoms in it.
struct RelDecodeRow {
    double o[3], R[3][3], vo[3], va[3], vp[3], d02, sin_a, cos_a;
};

template <typename T>
__host__ __device__ inline void relframe_decode_load(const T* cr, const T* origin, const T* rot, int n_c, const RelRemove& rm,
                                                     RelDecodeRow& f) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        f.o[r] = (double)origin[r];
        f.vo[r] = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) f.R[r][c] = (double)rot[3 * r + c];
    }
    const double a102 = RELFRAME_TWO_PI * (double)cr[2] - RELFRAME_PI;
    f.d02 = (double)cr[1];
    f.sin_a = sin(a102), f.cos_a = cos(a102);
    f.va[0] = (double)cr[0], f.va[1] = f.va[2] = 0.0;
    f.vp[0] = f.d02 * f.cos_a, f.vp[1] = f.d02 * f.sin_a, f.vp[2] = 0.0;
    int k = 3 + 3 * (n_c - 3);
    if (!rm.origin) {
        f.vo[0] = (double)cr[k], f.vo[1] = (double)cr[k + 1], f.vo[2] = (double)cr[k + 2];
        k += 3;
    }
    if (!rm.axis) {
        f.va[1] = (double)cr[k], f.va[2] = (double)cr[k + 1];
        k += 2;
    }
    if (!rm.plane) f.vp[2] = (double)cr[k];
}

template <typename T>
__host__ __device__ inline void relframe_decode_row(const T* cr, const T* origin, const T* rot, int n_c, const RelRemove& rm,
                                                    int lane, int stride, T* xr, T* ldj) {
    RelDecodeRow f;
    relframe_decode_load(cr, origin, rot, n_c, rm, f);
    const int n_o = n_c - 3;
    for (int i = lane; i < n_o; i += stride) {
        const double v[3] = {(double)cr[3 + 3 * i], (double)cr[3 + 3 * i + 1], (double)cr[3 + 3 * i + 2]};
        double x[3];
        mat3t_vec(f.R, v, x);
#pragma unroll
        for (int c = 0; c < 3; ++c) xr[3 * i + c] = (T)(x[c] + f.o[c]);
    }
    if (lane != 0) return;
    double xo[3], xa[3], xp[3];
    mat3t_vec(f.R, f.vo, xo);
    mat3t_vec(f.R, f.va, xa);
    mat3t_vec(f.R, f.vp, xp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        xr[3 * n_o + c] = (T)(xo[c] + f.o[c]);
        xr[3 * n_o + 3 + c] = (T)(xa[c] + f.o[c]);
        xr[3 * n_o + 6 + c] = (T)(xp[c] + f.o[c]);
    }
    *ldj = (T)(RELFRAME_LOG_TWO_PI + log(f.d02));
}

// One atom of decode's VJP: x = R^T v + o gives g_v = R g_x, and adds v g_x^T to acc[0..9) and g_x to acc[9..12).
__host__ __device__ inline void relframe_decode_vjp_atom(const double (&R)[3][3], const double (&v)[3], const double (&g)[3],
                                                         double (&gv)[3], double (&acc)[12]) {
    mat3_vec(R, g, gv);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        acc[9 + c] += g[c];
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[3 * r + c] += v[r] * g[c];
    }
}

// VJP of decode, the other atoms: their columns of g_coords, and this lane's part of acc.
template <typename T>
__host__ __device__ inline void relframe_decode_vjp_atoms(const T* cr, int n_c, const RelDecodeRow& f, const T* gxr, int lane,
                                                          int stride, T* gcr, double (&acc)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = 0.0;
    for (int i = lane; i < n_c - 3; i += stride) {
        const double v[3] = {(double)cr[3 + 3 * i], (double)cr[3 + 3 * i + 1], (double)cr[3 + 3 * i + 2]};
        const double g[3] = {(double)gxr[3 * i], (double)gxr[3 * i + 1], (double)gxr[3 * i + 2]};
        double gv[3];
        relframe_decode_vjp_atom(f.R, v, g, gv, acc);
#pragma unroll
        for (int c = 0; c < 3; ++c) gcr[3 + 3 * i + c] = (T)gv[c];
    }
}

// VJP of decode, the three reference atoms (one lane, with acc summed over the lanes): the remaining columns of g_coords,
// g_origin and g_R.  g_ldj may be NULL.
template <typename T>
__host__ __device__ inline void relframe_decode_vjp_refs(int n_c, const RelRemove& rm, const RelDecodeRow& f, const T* gxr,
                                                         const T* g_ldj, double (&acc)[12], T* gcr, T* g_origin, T* g_rot) {
    const T* gref = gxr + 3 * (n_c - 3);
    double g[3], gvo[3], gva[3], gvp[3];
    g[0] = (double)gref[0], g[1] = (double)gref[1], g[2] = (double)gref[2];
    relframe_decode_vjp_atom(f.R, f.vo, g, gvo, acc);
    g[0] = (double)gref[3], g[1] = (double)gref[4], g[2] = (double)gref[5];
    relframe_decode_vjp_atom(f.R, f.va, g, gva, acc);
    g[0] = (double)gref[6], g[1] = (double)gref[7], g[2] = (double)gref[8];
    relframe_decode_vjp_atom(f.R, f.vp, g, gvp, acc);
    gcr[0] = (T)gva[0];
    gcr[1] = (T)(gvp[0] * f.cos_a + gvp[1] * f.sin_a + (g_ldj ? (double)*g_ldj : 0.0) / f.d02);
    gcr[2] = (T)(RELFRAME_TWO_PI * f.d02 * (gvp[1] * f.cos_a - gvp[0] * f.sin_a));
    int k = 3 + 3 * (n_c - 3);
    if (!rm.origin) {
        gcr[k] = (T)gvo[0], gcr[k + 1] = (T)gvo[1], gcr[k + 2] = (T)gvo[2];
        k += 3;
    }
    if (!rm.axis) {
        gcr[k] = (T)gva[1], gcr[k + 1] = (T)gva[2];
        k += 2;
    }
    if (!rm.plane) gcr[k] = (T)gvp[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) g_origin[c] = (T)acc[9 + c];
#pragma unroll
    for (int k9 = 0; k9 < 9; ++k9) g_rot[k9] = (T)acc[k9];
}

}  // namespace tfep
