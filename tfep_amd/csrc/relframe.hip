// The relative frame of the mixed coordinates (reference app/mixedmaf.py:1216-1271, 1321-1375), forward and VJP, both
// directions, float32 and float64: one launch each.  The per-row arithmetic is in relframe.h.
//
// Layout, that of frames.hip: one wave per sample row (FRAME_ROWS rows per workgroup), lanes stride over the atoms of the
// row that are no reference atoms; lane 0 handles the three reference atoms.  A per-row sum is each lane's partial in fp64,
// in atom order, then the wave butterfly (wave_sum): no atomics, one fixed order, and nothing of another row enters -- the
// bits of a row do not depend on the batch it is in.  Arithmetic is fp64 for both element types, one rounding on store.
// Row strides are arguments, so a column slice of a wider tensor is read or written in place.  Every element of every
// output is written once, by one lane.
//
// The kernels move about two values per coordinate and do a few fp64 operations on each: they are expected to be bound
// by HBM traffic (tools/measure_relframe.py).
#include "common.h"
#include "relframe.h"

namespace tfep {

__device__ __forceinline__ int relframe_row() { return blockIdx.x * FRAME_ROWS + (threadIdx.x >> 6); }
__device__ __forceinline__ int relframe_lane() { return threadIdx.x & 63; }

template <typename T>
__global__ void __launch_bounds__(256) relframe_encode_kernel(const T* __restrict__ x, int64_t ldx, int n_c, RelRemove rm,
                                                              T* __restrict__ coords, int64_t ldc, T* __restrict__ origin,
                                                              T* __restrict__ rot, T* __restrict__ ldj, int B) {
    const int row = relframe_row();
    if (row >= B) return;
    relframe_encode_row(x + (int64_t)row * ldx, n_c, rm, relframe_lane(), WAVE, coords + (int64_t)row * ldc,
                        origin + (int64_t)row * 3, rot + (int64_t)row * 9, ldj + row);
}

template <typename T>
__global__ void __launch_bounds__(256) relframe_encode_backward_kernel(const T* __restrict__ x, int64_t ldx, int n_c,
                                                                       RelRemove rm, const T* __restrict__ gc, int64_t ldgc,
                                                                       const T* __restrict__ g_origin,
                                                                       const T* __restrict__ g_rot,
                                                                       const T* __restrict__ g_ldj, T* __restrict__ gx,
                                                                       int64_t ldgx, int B) {
    const int row = relframe_row(), lane = relframe_lane();
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    const T* gcr = gc + (int64_t)row * ldgc;
    T* gxr = gx + (int64_t)row * ldgx;
    RelFrameRow f;
    relframe_load(xr, n_c, f);
    double acc[12];
    relframe_encode_vjp_atoms(xr, n_c, f, gcr, lane, WAVE, gxr, acc);
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0)
        relframe_encode_vjp_refs(n_c, rm, f, gcr, g_origin ? g_origin + (int64_t)row * 3 : nullptr,
                                 g_rot ? g_rot + (int64_t)row * 9 : nullptr, g_ldj ? g_ldj + row : nullptr, acc, gxr);
}

template <typename T>
__global__ void __launch_bounds__(256) relframe_decode_kernel(const T* __restrict__ coords, int64_t ldc,
                                                              const T* __restrict__ origin, const T* __restrict__ rot,
                                                              int n_c, RelRemove rm, T* __restrict__ x, int64_t ldx,
                                                              T* __restrict__ ldj, int B) {
    const int row = relframe_row();
    if (row >= B) return;
    relframe_decode_row(coords + (int64_t)row * ldc, origin + (int64_t)row * 3, rot + (int64_t)row * 9, n_c, rm,
                        relframe_lane(), WAVE, x + (int64_t)row * ldx, ldj + row);
}

template <typename T>
__global__ void __launch_bounds__(256) relframe_decode_backward_kernel(const T* __restrict__ coords, int64_t ldc,
                                                                       const T* __restrict__ origin,
                                                                       const T* __restrict__ rot, int n_c, RelRemove rm,
                                                                       const T* __restrict__ gx, int64_t ldgx,
                                                                       const T* __restrict__ g_ldj, T* __restrict__ gc,
                                                                       int64_t ldgc, T* __restrict__ g_origin,
                                                                       T* __restrict__ g_rot, int B) {
    const int row = relframe_row(), lane = relframe_lane();
    if (row >= B) return;
    const T* cr = coords + (int64_t)row * ldc;
    const T* gxr = gx + (int64_t)row * ldgx;
    T* gcr = gc + (int64_t)row * ldgc;
    RelDecodeRow f;
    relframe_decode_load(cr, origin + (int64_t)row * 3, rot + (int64_t)row * 9, n_c, rm, f);
    double acc[12];
    relframe_decode_vjp_atoms(cr, n_c, f, gxr, lane, WAVE, gcr, acc);
#pragma unroll
    for (int k = 0; k < 12; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0)
        relframe_decode_vjp_refs(n_c, rm, f, gxr, g_ldj ? g_ldj + row : nullptr, acc, gcr, g_origin + (int64_t)row * 3,
                                 g_rot + (int64_t)row * 9);
}

// ---------------------------------------------------------------------------------------------------------------- host

static inline unsigned relframe_blocks(int B) { return (unsigned)((B + FRAME_ROWS - 1) / FRAME_ROWS); }

// Sizes every entry point shares: ldx / ldc are the strides of the rows of atoms and of the rows of coordinates.
static int relframe_check(const char* who, int n_c, const RelRemove& rm, int B, int64_t ldx, int64_t ldc) {
    TFEP_REQUIRE(B >= 0, "%s: negative size", who);
    TFEP_REQUIRE(n_c >= 3, "%s: n_c=%d, the relative frame needs the origin, axis and plane atoms", who, n_c);
    TFEP_REQUIRE(n_c <= 0x7fffffff / 4, "%s: n_c=%d too large", who, n_c);
    TFEP_REQUIRE(ldx >= 3 * (int64_t)n_c, "%s: a row stride is shorter than the row (%d atoms)", who, n_c);
    TFEP_REQUIRE(ldc >= relframe_width(n_c, rm), "%s: a row stride is shorter than the row (%lld coordinates)", who,
                 (long long)relframe_width(n_c, rm));
    return TFEP_OK;
}

template <typename T>
static int launch_relframe_encode(const char* who, const T* x, int64_t ldx, int n_c, RelRemove rm, T* coords, int64_t ldc,
                                  T* origin, T* rot, T* ldj, int B, void* stream) {
    if (int rc = relframe_check(who, n_c, rm, B, ldx, ldc)) return rc;
    TFEP_REQUIRE(x && coords && origin && rot && ldj, "%s: x/coords/origin/R/log_det_J must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    relframe_encode_kernel<T><<<relframe_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, n_c, rm, coords, ldc, origin, rot,
                                                                                   ldj, B);
    return check_launch("relframe_encode_kernel");
}

template <typename T>
static int launch_relframe_encode_backward(const char* who, const T* x, int64_t ldx, int n_c, RelRemove rm, const T* gc,
                                           int64_t ldgc, const T* g_origin, const T* g_rot, const T* g_ldj, T* gx,
                                           int64_t ldgx, int B, void* stream) {
    if (int rc = relframe_check(who, n_c, rm, B, ldx < ldgx ? ldx : ldgx, ldgc)) return rc;
    TFEP_REQUIRE(x && gc && gx, "%s: x/g_coords/gx must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    relframe_encode_backward_kernel<T><<<relframe_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, n_c, rm, gc, ldgc, g_origin,
                                                                                            g_rot, g_ldj, gx, ldgx, B);
    return check_launch("relframe_encode_backward_kernel");
}

template <typename T>
static int launch_relframe_decode(const char* who, const T* coords, int64_t ldc, const T* origin, const T* rot, int n_c,
                                  RelRemove rm, T* x, int64_t ldx, T* ldj, int B, void* stream) {
    if (int rc = relframe_check(who, n_c, rm, B, ldx, ldc)) return rc;
    TFEP_REQUIRE(coords && origin && rot && x && ldj, "%s: coords/origin/R/x/log_det_J must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    relframe_decode_kernel<T><<<relframe_blocks(B), 256, 0, (hipStream_t)stream>>>(coords, ldc, origin, rot, n_c, rm, x, ldx,
                                                                                   ldj, B);
    return check_launch("relframe_decode_kernel");
}

template <typename T>
static int launch_relframe_decode_backward(const char* who, const T* coords, int64_t ldc, const T* origin, const T* rot,
                                           int n_c, RelRemove rm, const T* gx, int64_t ldgx, const T* g_ldj, T* gc,
                                           int64_t ldgc, T* g_origin, T* g_rot, int B, void* stream) {
    if (int rc = relframe_check(who, n_c, rm, B, ldgx, ldc < ldgc ? ldc : ldgc)) return rc;
    TFEP_REQUIRE(coords && origin && rot && gx && gc && g_origin && g_rot,
                 "%s: coords/origin/R/gx/g_coords/g_origin/g_R must be non-NULL", who);
    if (B == 0) return TFEP_OK;
    relframe_decode_backward_kernel<T><<<relframe_blocks(B), 256, 0, (hipStream_t)stream>>>(
        coords, ldc, origin, rot, n_c, rm, gx, ldgx, g_ldj, gc, ldgc, g_origin, g_rot, B);
    return check_launch("relframe_decode_backward_kernel");
}

}  // namespace tfep

using namespace tfep;

// The float and the double entry point of each launcher, from one argument list.
#define TFEP_RELFRAME_ENTRY(T, sfx)                                                                                          \
    int tfep_relative_frame_encode##sfx(const T* x, int64_t ldx, int n_c, int remove_origin, int remove_axis,                \
                                        int remove_plane, T* coords, int64_t ldc, T* origin, T* R, T* log_det_J, int B,      \
                                        void* stream) {                                                                      \
        return launch_relframe_encode<T>("relative_frame_encode" #sfx, x, ldx, n_c,                                          \
                                         RelRemove{remove_origin, remove_axis, remove_plane}, coords, ldc, origin, R,        \
                                         log_det_J, B, stream);                                                              \
    }                                                                                                                        \
    int tfep_relative_frame_encode_backward##sfx(const T* x, int64_t ldx, int n_c, int remove_origin, int remove_axis,       \
                                                 int remove_plane, const T* g_coords, int64_t ldgc, const T* g_origin,       \
                                                 const T* g_R, const T* g_log_det_J, T* gx, int64_t ldgx, int B,             \
                                                 void* stream) {                                                             \
        return launch_relframe_encode_backward<T>("relative_frame_encode_backward" #sfx, x, ldx, n_c,                        \
                                                  RelRemove{remove_origin, remove_axis, remove_plane}, g_coords, ldgc,       \
                                                  g_origin, g_R, g_log_det_J, gx, ldgx, B, stream);                          \
    }                                                                                                                        \
    int tfep_relative_frame_decode##sfx(const T* coords, int64_t ldc, const T* origin, const T* R, int n_c,                  \
                                        int remove_origin, int remove_axis, int remove_plane, T* x, int64_t ldx,             \
                                        T* log_det_J, int B, void* stream) {                                                 \
        return launch_relframe_decode<T>("relative_frame_decode" #sfx, coords, ldc, origin, R, n_c,                          \
                                         RelRemove{remove_origin, remove_axis, remove_plane}, x, ldx, log_det_J, B, stream); \
    }                                                                                                                        \
    int tfep_relative_frame_decode_backward##sfx(const T* coords, int64_t ldc, const T* origin, const T* R, int n_c,         \
                                                 int remove_origin, int remove_axis, int remove_plane, const T* gx,          \
                                                 int64_t ldgx, const T* g_log_det_J, T* g_coords, int64_t ldgc,              \
                                                 T* g_origin, T* g_R, int B, void* stream) {                                 \
        return launch_relframe_decode_backward<T>("relative_frame_decode_backward" #sfx, coords, ldc, origin, R, n_c,        \
                                                  RelRemove{remove_origin, remove_axis, remove_plane}, gx, ldgx,             \
                                                  g_log_det_J, g_coords, ldgc, g_origin, g_R, B, stream);                    \
    }

extern "C" {
TFEP_RELFRAME_ENTRY(float, )
TFEP_RELFRAME_ENTRY(double, _f64)
}  // extern "C"
