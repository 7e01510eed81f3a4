// The frame arithmetic of CenteredCentroidFlow and OrientedFlow (reference flows/centroid.py, flows/oriented.py,
// utils/geometry.py:239-411), forward and VJP, float32 and float64.  The per-row rotation and its derivative are in
// frames.h.
//
// Layout: one wave per sample row (four rows per workgroup), lanes stride over the points of the row.  A per-row sum is
// each lane's partial in fp64, in point order, then the wave butterfly (wave_sum): no atomics, one fixed order, and nothing
// of another row enters -- the bits of a row do not depend on the batch it is in.  Arithmetic is fp64 for both element
// types.  Row strides are arguments, so a column slice of a wider tensor is read or written in place.
//
// The kernels move two or three values per feature and do a few fp64 operations on each: they are expected to be bound by
// HBM traffic.  That has not been measured (tools/measure_frames.py).
//
// Centroid subsets: `subset` lists DISTINCT point indices (the backward kernels write the cotangent of a listed point
// once).  An entry outside [0, n_points) is never dereferenced; it makes the row's centroid NaN.
#include "common.h"
#include "frames.h"

namespace tfep {

constexpr int FRAME_MAX_DIM = 3;

__device__ __forceinline__ int frame_row() { return blockIdx.x * FRAME_ROWS + (threadIdx.x >> 6); }
__device__ __forceinline__ int frame_lane() { return threadIdx.x & 63; }

// Point index and weight of entry k of the centroid's selection (all points when there is no subset; equal weights when
// there are none).  An index out of range gives point 0 with a NaN weight.
template <typename T>
__device__ __forceinline__ int centroid_entry(const int32_t* __restrict__ subset, const T* __restrict__ weights, int k,
                                              int n_sel, int n_points, double& w) {
    int i = subset ? subset[k] : k;
    w = weights ? (double)weights[k] : 1.0 / (double)n_sel;
    if ((unsigned)i >= (unsigned)n_points) {
        i = 0;
        w = __builtin_nan("");
    }
    return i;
}

template <typename T>
__global__ void __launch_bounds__(256) centroid_shift_kernel(const T* __restrict__ x, int64_t ldx,
                                                             const int32_t* __restrict__ subset, int n_sel,
                                                             const T* __restrict__ weights, const T* __restrict__ origin,
                                                             int dim, int n_points, T* __restrict__ shift,
                                                             T* __restrict__ y, int64_t ldy, int B) {
    const int row = frame_row(), lane = frame_lane();
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    T* yr = y + (int64_t)row * ldy;
    double acc[FRAME_MAX_DIM] = {0.0, 0.0, 0.0}, sh[FRAME_MAX_DIM];
    for (int k = lane; k < n_sel; k += WAVE) {
        double w;
        const int i = centroid_entry(subset, weights, k, n_sel, n_points, w);
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) acc[c] += w * (double)xr[i * dim + c];
    }
#pragma unroll
    for (int c = 0; c < FRAME_MAX_DIM; ++c) {
        sh[c] = c < dim ? (double)origin[c] - wave_sum(acc[c]) : 0.0;
        if (c < dim && lane == 0) shift[(int64_t)row * dim + c] = (T)sh[c];
    }
    for (int i = lane; i < n_points; i += WAVE)
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) yr[i * dim + c] = (T)((double)xr[i * dim + c] + sh[c]);
}

template <typename T>
__global__ void __launch_bounds__(256) centroid_restore_kernel(const T* __restrict__ y, int64_t ldy,
                                                               const T* __restrict__ shift,
                                                               const int32_t* __restrict__ subset, int n_sel,
                                                               const T* __restrict__ weights, const T* __restrict__ origin,
                                                               int fixed_point, int fixed_entry, int restore, int dim,
                                                               int n_points, int translate_back, T* __restrict__ out,
                                                               int64_t ldo, int B) {
    const int row = frame_row(), lane = frame_lane();
    if (row >= B) return;
    const T* yr = y + (int64_t)row * ldy;
    T* orow = out + (int64_t)row * ldo;
    double fixed[FRAME_MAX_DIM] = {0.0, 0.0, 0.0}, sh[FRAME_MAX_DIM];
    if (restore) {
        double rest[FRAME_MAX_DIM] = {0.0, 0.0, 0.0}, w_fixed;
        centroid_entry(subset, weights, fixed_entry, n_sel, n_points, w_fixed);
        for (int k = lane; k < n_sel; k += WAVE) {
            double w;
            const int i = centroid_entry(subset, weights, k, n_sel, n_points, w);
            if (k == fixed_entry) continue;
#pragma unroll
            for (int c = 0; c < FRAME_MAX_DIM; ++c)
                if (c < dim) rest[c] += w * (double)yr[i * dim + c];
        }
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) fixed[c] = ((double)origin[c] - wave_sum(rest[c])) / w_fixed;
    }
#pragma unroll
    for (int c = 0; c < FRAME_MAX_DIM; ++c) sh[c] = (translate_back && c < dim) ? (double)shift[(int64_t)row * dim + c] : 0.0;
    for (int i = lane; i < n_points; i += WAVE) {
        const bool is_fixed = restore && i == fixed_point;
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) orow[i * dim + c] = (T)((is_fixed ? fixed[c] : (double)yr[i * dim + c]) - sh[c]);
    }
}

// VJP of centroid_shift: outputs shift = origin - sum_k w_k x_{s_k} and y_i = x_i + shift.  With G = gshift + sum_i gy_i the
// cotangent of x_i is gy_i, minus w_k G for a point of the selection.  Every point is written first, the workgroup
// synchronises, then the points of the selection are written again (distinct indices: once each).
template <typename T>
__global__ void __launch_bounds__(256) centroid_shift_backward_kernel(const int32_t* __restrict__ subset, int n_sel,
                                                                      const T* __restrict__ weights, int dim, int n_points,
                                                                      const T* __restrict__ gy, int64_t ldgy,
                                                                      const T* __restrict__ gshift, T* __restrict__ gx,
                                                                      int64_t ldgx, int B) {
    const int row = frame_row(), lane = frame_lane();
    const bool live = row < B;                   // (no early return: every thread reaches the barrier)
    const T* gr = gy + (int64_t)row * ldgy;
    T* gxr = gx + (int64_t)row * ldgx;
    double G[FRAME_MAX_DIM] = {0.0, 0.0, 0.0};
    if (live) {
        for (int i = lane; i < n_points; i += WAVE)
#pragma unroll
            for (int c = 0; c < FRAME_MAX_DIM; ++c)
                if (c < dim) {
                    const T g = gr[i * dim + c];
                    gxr[i * dim + c] = g;
                    G[c] += (double)g;
                }
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) G[c] = wave_sum(G[c]) + (gshift ? (double)gshift[(int64_t)row * dim + c] : 0.0);
    }
    __syncthreads();
    if (!live) return;
    for (int k = lane; k < n_sel; k += WAVE) {
        double w;
        const int i = centroid_entry(subset, weights, k, n_sel, n_points, w);
        if (w != w) continue;                    // (index out of range: the forward was NaN already)
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) gxr[i * dim + c] = (T)((double)gr[i * dim + c] - w * G[c]);
    }
}

// VJP of centroid_restore: out_i = y_i - shift except at the fixed point f, where out_f = (origin - sum_{k != f} w_k y_{s_k})
// / w_f - shift (`restore`); the shift is subtracted only with `translate_back`.
template <typename T>
__global__ void __launch_bounds__(256) centroid_restore_backward_kernel(const int32_t* __restrict__ subset, int n_sel,
                                                                        const T* __restrict__ weights, int fixed_point,
                                                                        int fixed_entry, int restore, int dim, int n_points,
                                                                        int translate_back, const T* __restrict__ g,
                                                                        int64_t ldg, T* __restrict__ gy, int64_t ldgy,
                                                                        T* __restrict__ gshift, int B) {
    const int row = frame_row(), lane = frame_lane();
    const bool live = row < B;
    const T* gr = g + (int64_t)row * ldg;
    T* gyr = gy + (int64_t)row * ldgy;
    if (live) {
        double acc[FRAME_MAX_DIM] = {0.0, 0.0, 0.0};
        for (int i = lane; i < n_points; i += WAVE) {
            const bool is_fixed = restore && i == fixed_point;
#pragma unroll
            for (int c = 0; c < FRAME_MAX_DIM; ++c)
                if (c < dim) {
                    const T v = gr[i * dim + c];
                    gyr[i * dim + c] = is_fixed ? (T)0 : v;
                    acc[c] += (double)v;
                }
        }
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) {
                const double s = wave_sum(acc[c]);
                if (lane == 0) gshift[(int64_t)row * dim + c] = translate_back ? (T)(-s) : (T)0;
            }
    }
    __syncthreads();
    if (!live || !restore) return;
    double w_fixed, gf[FRAME_MAX_DIM];
    centroid_entry(subset, weights, fixed_entry, n_sel, n_points, w_fixed);
#pragma unroll
    for (int c = 0; c < FRAME_MAX_DIM; ++c) gf[c] = c < dim ? (double)gr[fixed_point * dim + c] / w_fixed : 0.0;
    for (int k = lane; k < n_sel; k += WAVE) {
        double w;
        const int i = centroid_entry(subset, weights, k, n_sel, n_points, w);
        if (k == fixed_entry || w != w) continue;
#pragma unroll
        for (int c = 0; c < FRAME_MAX_DIM; ++c)
            if (c < dim) gyr[i * dim + c] = (T)((double)gr[i * dim + c] - w * gf[c]);
    }
}

// Description of a frame: the two defining points and the axes.
struct FrameSpec {
    int axis_point, plane_point, round_off;
    FrameAxes axes;
};

template <typename T>
__device__ __forceinline__ void load3(const T* __restrict__ p, double (&v)[3]) {
    v[0] = (double)p[0], v[1] = (double)p[1], v[2] = (double)p[2];
}

// The cotangent of a framed point as the forward's round_off leaves it: the constrained coordinates carry none.
__device__ __forceinline__ void frame_mask(const FrameSpec& f, int i, double (&g)[3]) {
    if (!f.round_off) return;
    const int nn = (f.axes.normal < 0 ? -f.axes.normal : f.axes.normal) - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if ((i == f.axis_point && c != f.axes.axis) || (i == f.plane_point && c == nn)) g[c] = 0.0;
}

template <typename T>
__global__ void __launch_bounds__(256) frame_orient_kernel(const T* __restrict__ x, int64_t ldx, FrameSpec f,
                                                           T* __restrict__ y, int64_t ldy, T* __restrict__ rot,
                                                           int n_points, int B) {
    const int row = frame_row(), lane = frame_lane();
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    T* yr = y + (int64_t)row * ldy;
    double a[3], p[3], R[3][3];
    load3(xr + 3 * f.axis_point, a);
    load3(xr + 3 * f.plane_point, p);
    FrameState st;
    frame_rotation(a, p, f.axes, R, st);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) rot[(int64_t)row * 9 + 3 * r + c] = (T)R[r][c];
    }
    for (int i = lane; i < n_points; i += WAVE) {
        double v[3], o[3];
        load3(xr + 3 * i, v);
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2];
        frame_mask(f, i, o);                      // (the same coordinates, set to exact zeros)
#pragma unroll
        for (int r = 0; r < 3; ++r) yr[3 * i + r] = (T)o[r];
    }
}

// y_i = x_i M with M = R, or R^T when `transposed` (row vectors: y[c] = sum_r x[r] M[r][c]).
template <typename T>
__device__ __forceinline__ void load_rotation(const T* __restrict__ rot, int transposed, double (&M)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = (double)(transposed ? rot[3 * c + r] : rot[3 * r + c]);
}

template <typename T>
__global__ void __launch_bounds__(256) frame_rotate_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ rot,
                                                           int transposed, T* __restrict__ y, int64_t ldy, int n_points,
                                                           int B) {
    const int row = frame_row(), lane = frame_lane();
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    T* yr = y + (int64_t)row * ldy;
    double M[3][3];
    load_rotation(rot + (int64_t)row * 9, transposed, M);
    for (int i = lane; i < n_points; i += WAVE) {
        double v[3];
        load3(xr + 3 * i, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) yr[3 * i + c] = (T)(v[0] * M[0][c] + v[1] * M[1][c] + v[2] * M[2][c]);
    }
}

// VJP of frame_rotate: gx_i = gy_i M^T and gM = sum_i x_i^T gy_i (nine wave sums), returned as the cotangent of R.
template <typename T>
__global__ void __launch_bounds__(256) frame_rotate_backward_kernel(const T* __restrict__ x, int64_t ldx,
                                                                    const T* __restrict__ rot, int transposed,
                                                                    const T* __restrict__ gy, int64_t ldgy,
                                                                    T* __restrict__ gx, int64_t ldgx, T* __restrict__ grot,
                                                                    int n_points, int B) {
    const int row = frame_row(), lane = frame_lane();
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    const T* gr = gy + (int64_t)row * ldgy;
    T* gxr = gx + (int64_t)row * ldgx;
    double M[3][3], GM[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    load_rotation(rot + (int64_t)row * 9, transposed, M);
    for (int i = lane; i < n_points; i += WAVE) {
        double v[3], g[3];
        load3(xr + 3 * i, v);
        load3(gr + 3 * i, g);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            gxr[3 * i + r] = (T)(g[0] * M[r][0] + g[1] * M[r][1] + g[2] * M[r][2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) GM[r][c] += v[r] * g[c];
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double s = wave_sum(GM[r][c]);
            if (lane == 0) grot[(int64_t)row * 9 + (transposed ? 3 * c + r : 3 * r + c)] = (T)s;
        }
}

// VJP of frame_orient: y_i = R x_i (then the round-off), R = R(x_a, x_p).  The cotangent of R is grot (the rotate-back's,
// may be NULL) plus sum_i gy_i x_i^T; frame_rotation_vjp turns it into the cotangents of the two defining points, which the
// lanes that own those points add to gx_i = R^T gy_i (each lane rewrites only what it wrote itself).
template <typename T>
__global__ void __launch_bounds__(256) frame_orient_backward_kernel(const T* __restrict__ x, int64_t ldx, FrameSpec f,
                                                                    const T* __restrict__ gy, int64_t ldgy,
                                                                    const T* __restrict__ grot, T* __restrict__ gx,
                                                                    int64_t ldgx, int n_points, int B) {
    const int row = frame_row(), lane = frame_lane();
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    const T* gr = gy + (int64_t)row * ldgy;
    T* gxr = gx + (int64_t)row * ldgx;
    double a[3], p[3], R[3][3], GR[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    load3(xr + 3 * f.axis_point, a);
    load3(xr + 3 * f.plane_point, p);
    FrameState st;
    frame_rotation(a, p, f.axes, R, st);
    for (int i = lane; i < n_points; i += WAVE) {
        double v[3], g[3];
        load3(xr + 3 * i, v);
        load3(gr + 3 * i, g);
        frame_mask(f, i, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gxr[3 * i + c] = (T)(R[0][c] * g[0] + R[1][c] * g[1] + R[2][c] * g[2]);
#pragma unroll
            for (int r = 0; r < 3; ++r) GR[r][c] += g[r] * v[c];
        }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            GR[r][c] = wave_sum(GR[r][c]) + (grot ? (double)grot[(int64_t)row * 9 + 3 * r + c] : 0.0);
    double ga[3], gp[3];
    frame_rotation_vjp(p, f.axes, st, GR, ga, gp);
    const bool owns_a = lane == (f.axis_point & 63), owns_p = lane == (f.plane_point & 63);
    if (owns_a || owns_p) {
        const int i = owns_a ? f.axis_point : f.plane_point;
        double g[3];
        load3(gr + 3 * i, g);
        frame_mask(f, i, g);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            gxr[3 * i + c] = (T)(R[0][c] * g[0] + R[1][c] * g[1] + R[2][c] * g[2] + (owns_a ? ga[c] : gp[c]));
    }
    // (one lane can own both points when they are a multiple of 64 apart)
    if (owns_a && owns_p) {
        double g[3];
        load3(gr + 3 * f.plane_point, g);
        frame_mask(f, f.plane_point, g);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            gxr[3 * f.plane_point + c] = (T)(R[0][c] * g[0] + R[1][c] * g[1] + R[2][c] * g[2] + gp[c]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

static inline unsigned frame_blocks(int B) { return (unsigned)((B + FRAME_ROWS - 1) / FRAME_ROWS); }

// Sizes every entry point shares: `width` = features per point.
static int frames_check_rows(const char* who, int n_points, int width, int B, int64_t ld_in, int64_t ld_out) {
    TFEP_REQUIRE(B >= 0 && n_points >= 0, "%s: negative size", who);
    TFEP_REQUIRE(n_points <= 0x7fffffff / 4, "%s: n_points=%d too large", who, n_points);
    TFEP_REQUIRE(ld_in >= (int64_t)n_points * width && ld_out >= (int64_t)n_points * width,
                 "%s: a row stride is shorter than the row (%d points of %d)", who, n_points, width);
    return TFEP_OK;
}

static int centroid_check(const char* who, const void* subset, int n_subset, int fixed_point, int fixed_entry, int dim,
                          int n_points, bool has_fixed) {
    TFEP_REQUIRE(dim >= 1 && dim <= FRAME_MAX_DIM, "%s: dim=%d unsupported (1..%d)", who, dim, FRAME_MAX_DIM);
    TFEP_REQUIRE(n_subset >= 0 && (subset || n_subset == 0), "%s: n_subset=%d without a subset", who, n_subset);
    TFEP_REQUIRE(!subset || n_subset >= 1, "%s: an empty subset has no centroid", who);
    TFEP_REQUIRE(subset || n_points >= 1, "%s: no points, no centroid", who);
    if (has_fixed) {
        const int n_sel = subset ? n_subset : n_points;
        TFEP_REQUIRE(fixed_point >= 0 && fixed_point < n_points, "%s: fixed_point=%d out of range (%d points)", who,
                     fixed_point, n_points);
        TFEP_REQUIRE(fixed_entry >= 0 && fixed_entry < n_sel, "%s: fixed_entry=%d out of range (%d entries)", who,
                     fixed_entry, n_sel);
        TFEP_REQUIRE(subset || fixed_entry == fixed_point, "%s: without a subset fixed_entry must equal fixed_point", who);
    }
    return TFEP_OK;
}

static int frame_spec_check(const char* who, const FrameSpec& f, int n_points) {
    TFEP_REQUIRE(n_points >= 2, "%s: n_points=%d, a frame needs an axis point and a plane point", who, n_points);
    TFEP_REQUIRE(f.axis_point >= 0 && f.axis_point < n_points, "%s: axis_point=%d out of range (%d points)", who,
                 f.axis_point, n_points);
    TFEP_REQUIRE(f.plane_point >= 0 && f.plane_point < n_points, "%s: plane_point=%d out of range (%d points)", who,
                 f.plane_point, n_points);
    TFEP_REQUIRE(f.axis_point != f.plane_point, "%s: axis_point and plane_point must differ", who);
    TFEP_REQUIRE(frame_axes_valid(f.axes), "%s: axis=%d, plane_axis=%d, normal=%d is not a frame (axes 0..2, all different, "
                 "normal = +-(1 + third axis))", who, f.axes.axis, f.axes.plane_axis, f.axes.normal);
    return TFEP_OK;
}

template <typename T>
static int launch_centroid_shift(const char* who, const T* x, int64_t ldx, const int32_t* subset, int n_subset,
                                 const T* weights, const T* origin, int dim, int n_points, T* shift, T* y, int64_t ldy,
                                 int B, void* stream) {
    if (int rc = centroid_check(who, subset, n_subset, 0, 0, dim, n_points, false)) return rc;
    if (int rc = frames_check_rows(who, n_points, dim, B, ldx, ldy)) return rc;
    TFEP_REQUIRE(x && origin && shift && y, "%s: x/origin/shift/y must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    centroid_shift_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(
        x, ldx, subset, subset ? n_subset : n_points, weights, origin, dim, n_points, shift, y, ldy, B);
    return check_launch("centroid_shift_kernel");
}

template <typename T>
static int launch_centroid_restore(const char* who, const T* y, int64_t ldy, const T* shift, const int32_t* subset,
                                   int n_subset, const T* weights, const T* origin, int fixed_point, int fixed_entry, int dim,
                                   int n_points, int translate_back, T* out, int64_t ldo, int B, void* stream) {
    if (int rc = centroid_check(who, subset, n_subset, fixed_point, fixed_entry, dim, n_points, true)) return rc;
    if (int rc = frames_check_rows(who, n_points, dim, B, ldy, ldo)) return rc;
    TFEP_REQUIRE(y && origin && out, "%s: y/origin/out must be non-NULL", who);
    TFEP_REQUIRE(shift || !translate_back, "%s: translate_back needs the shift", who);
    if (B == 0) return TFEP_OK;
    const int restore = !(subset && n_subset <= 1);      // (a one-point centroid IS the fixed point: nothing to place)
    centroid_restore_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(
        y, ldy, shift, subset, subset ? n_subset : n_points, weights, origin, fixed_point, fixed_entry, restore, dim,
        n_points, translate_back != 0, out, ldo, B);
    return check_launch("centroid_restore_kernel");
}

template <typename T>
static int launch_centroid_shift_backward(const char* who, const int32_t* subset, int n_subset, const T* weights, int dim,
                                          int n_points, const T* gy, int64_t ldgy, const T* gshift, T* gx, int64_t ldgx,
                                          int B, void* stream) {
    if (int rc = centroid_check(who, subset, n_subset, 0, 0, dim, n_points, false)) return rc;
    if (int rc = frames_check_rows(who, n_points, dim, B, ldgy, ldgx)) return rc;
    TFEP_REQUIRE(gy && gx, "%s: gy/gx must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    centroid_shift_backward_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(
        subset, subset ? n_subset : n_points, weights, dim, n_points, gy, ldgy, gshift, gx, ldgx, B);
    return check_launch("centroid_shift_backward_kernel");
}

template <typename T>
static int launch_centroid_restore_backward(const char* who, const int32_t* subset, int n_subset, const T* weights,
                                            int fixed_point, int fixed_entry, int dim, int n_points, int translate_back,
                                            const T* g, int64_t ldg, T* gy, int64_t ldgy, T* gshift, int B, void* stream) {
    if (int rc = centroid_check(who, subset, n_subset, fixed_point, fixed_entry, dim, n_points, true)) return rc;
    if (int rc = frames_check_rows(who, n_points, dim, B, ldg, ldgy)) return rc;
    TFEP_REQUIRE(g && gy && gshift, "%s: g/gy/gshift must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    const int restore = !(subset && n_subset <= 1);
    centroid_restore_backward_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(
        subset, subset ? n_subset : n_points, weights, fixed_point, fixed_entry, restore, dim, n_points, translate_back != 0,
        g, ldg, gy, ldgy, gshift, B);
    return check_launch("centroid_restore_backward_kernel");
}

template <typename T>
static int launch_frame_orient(const char* who, const T* x, int64_t ldx, FrameSpec f, T* y, int64_t ldy, T* rot,
                               int n_points, int B, void* stream) {
    if (int rc = frame_spec_check(who, f, n_points)) return rc;
    if (int rc = frames_check_rows(who, n_points, 3, B, ldx, ldy)) return rc;
    TFEP_REQUIRE(x && y && rot, "%s: x/y/R must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    frame_orient_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, f, y, ldy, rot, n_points, B);
    return check_launch("frame_orient_kernel");
}

template <typename T>
static int launch_frame_orient_backward(const char* who, const T* x, int64_t ldx, FrameSpec f, const T* gy, int64_t ldgy,
                                        const T* grot, T* gx, int64_t ldgx, int n_points, int B, void* stream) {
    if (int rc = frame_spec_check(who, f, n_points)) return rc;
    if (int rc = frames_check_rows(who, n_points, 3, B, ldx < ldgy ? ldx : ldgy, ldgx)) return rc;
    TFEP_REQUIRE(x && gy && gx, "%s: x/gy/gx must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    frame_orient_backward_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, f, gy, ldgy, grot, gx, ldgx,
                                                                                      n_points, B);
    return check_launch("frame_orient_backward_kernel");
}

template <typename T>
static int launch_frame_rotate(const char* who, const T* x, int64_t ldx, const T* rot, int transposed, T* y, int64_t ldy,
                               int n_points, int B, void* stream) {
    if (int rc = frames_check_rows(who, n_points, 3, B, ldx, ldy)) return rc;
    TFEP_REQUIRE(x && rot && y, "%s: x/R/y must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    frame_rotate_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, rot, transposed != 0, y, ldy, n_points, B);
    return check_launch("frame_rotate_kernel");
}

template <typename T>
static int launch_frame_rotate_backward(const char* who, const T* x, int64_t ldx, const T* rot, int transposed, const T* gy,
                                        int64_t ldgy, T* gx, int64_t ldgx, T* grot, int n_points, int B, void* stream) {
    if (int rc = frames_check_rows(who, n_points, 3, B, ldx < ldgy ? ldx : ldgy, ldgx)) return rc;
    TFEP_REQUIRE(x && rot && gy && gx && grot, "%s: x/R/gy/gx/gR must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    frame_rotate_backward_kernel<T><<<frame_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, rot, transposed != 0, gy, ldgy,
                                                                                      gx, ldgx, grot, n_points, B);
    return check_launch("frame_rotate_backward_kernel");
}

}  // namespace tfep

using namespace tfep;

// The float and the double entry point of each launcher, from one argument list.
#define TFEP_FRAME_ENTRY(T, sfx)                                                                                             \
    int tfep_centroid_shift##sfx(const T* x, int64_t ldx, const int32_t* subset, int n_subset, const T* weights,             \
                                 const T* origin, int dim, int n_points, T* shift, T* y, int64_t ldy, int B, void* stream) { \
        return launch_centroid_shift<T>("centroid_shift" #sfx, x, ldx, subset, n_subset, weights, origin, dim, n_points,     \
                                        shift, y, ldy, B, stream);                                                          \
    }                                                                                                                        \
    int tfep_centroid_restore##sfx(const T* y, int64_t ldy, const T* shift, const int32_t* subset, int n_subset,             \
                                   const T* weights, const T* origin, int fixed_point, int fixed_entry, int dim,             \
                                   int n_points, int translate_back, T* out, int64_t ldo, int B, void* stream) {             \
        return launch_centroid_restore<T>("centroid_restore" #sfx, y, ldy, shift, subset, n_subset, weights, origin,         \
                                          fixed_point, fixed_entry, dim, n_points, translate_back, out, ldo, B, stream);     \
    }                                                                                                                        \
    int tfep_centroid_shift_backward##sfx(const int32_t* subset, int n_subset, const T* weights, int dim, int n_points,      \
                                          const T* gy, int64_t ldgy, const T* gshift, T* gx, int64_t ldgx, int B,            \
                                          void* stream) {                                                                    \
        return launch_centroid_shift_backward<T>("centroid_shift_backward" #sfx, subset, n_subset, weights, dim, n_points,   \
                                                 gy, ldgy, gshift, gx, ldgx, B, stream);                                    \
    }                                                                                                                        \
    int tfep_centroid_restore_backward##sfx(const int32_t* subset, int n_subset, const T* weights, int fixed_point,          \
                                            int fixed_entry, int dim, int n_points, int translate_back, const T* g,          \
                                            int64_t ldg, T* gy, int64_t ldgy, T* gshift, int B, void* stream) {              \
        return launch_centroid_restore_backward<T>("centroid_restore_backward" #sfx, subset, n_subset, weights, fixed_point, \
                                                   fixed_entry, dim, n_points, translate_back, g, ldg, gy, ldgy, gshift, B,  \
                                                   stream);                                                                  \
    }                                                                                                                        \
    int tfep_frame_orient##sfx(const T* x, int64_t ldx, int axis_point, int plane_point, int axis, int plane_axis,           \
                               int normal, int round_off, T* y, int64_t ldy, T* R, int n_points, int B, void* stream) {      \
        return launch_frame_orient<T>("frame_orient" #sfx, x, ldx,                                                           \
                                      FrameSpec{axis_point, plane_point, round_off != 0, {axis, plane_axis, normal}}, y,     \
                                      ldy, R, n_points, B, stream);                                                          \
    }                                                                                                                        \
    int tfep_frame_orient_backward##sfx(const T* x, int64_t ldx, int axis_point, int plane_point, int axis, int plane_axis,  \
                                        int normal, int round_off, const T* gy, int64_t ldgy, const T* gR, T* gx,            \
                                        int64_t ldgx, int n_points, int B, void* stream) {                                   \
        return launch_frame_orient_backward<T>("frame_orient_backward" #sfx, x, ldx,                                         \
                                               FrameSpec{axis_point, plane_point, round_off != 0,                            \
                                                         {axis, plane_axis, normal}},                                        \
                                               gy, ldgy, gR, gx, ldgx, n_points, B, stream);                                 \
    }                                                                                                                        \
    int tfep_frame_rotate##sfx(const T* x, int64_t ldx, const T* R, int transposed, T* y, int64_t ldy, int n_points, int B,  \
                               void* stream) {                                                                               \
        return launch_frame_rotate<T>("frame_rotate" #sfx, x, ldx, R, transposed, y, ldy, n_points, B, stream);              \
    }                                                                                                                        \
    int tfep_frame_rotate_backward##sfx(const T* x, int64_t ldx, const T* R, int transposed, const T* gy, int64_t ldgy,      \
                                        T* gx, int64_t ldgx, T* gR, int n_points, int B, void* stream) {                     \
        return launch_frame_rotate_backward<T>("frame_rotate_backward" #sfx, x, ldx, R, transposed, gy, ldgy, gx, ldgx, gR,  \
                                               n_points, B, stream);                                                         \
    }

extern "C" {
TFEP_FRAME_ENTRY(float, )
TFEP_FRAME_ENTRY(double, _f64)
}  // extern "C"
