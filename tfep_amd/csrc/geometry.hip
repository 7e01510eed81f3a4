// Internal coordinates of a batch of point rows (distances, angles, proper dihedrals over index tables) with their VJP,
// and the element-wise polar map with its VJP (reference utils/geometry.py:28-178, 414-471), float32 and float64.  The
// per-entry arithmetic is in geometry.h.
//
// Layout of the internal-coordinate kernels, as frames.hip: one wave per sample row (four rows per workgroup), fp64
// arithmetic for both element types, row strides of x and gx as arguments, no atomics.
//   forward   the lanes stride over the P + A + T entries of the three tables; an entry reads its two to four points and
//             writes one value.  One launch for all three kinds.
//   backward  the lanes stride over the ATOMS of the row.  An atom's cotangent is the sum over the entries it appears in,
//             taken in table order (pairs, then triples, then quads; within a table by entry) from the atom's incidence
//             list: atom_start (n_atoms + 1 offsets) and atom_items (4 * entry + slot, `entry` counted through the three
//             tables, `slot` the atom's place in the entry).  The lane recomputes each entry's derivative and keeps its
//             own slot, accumulates in a register and writes every coordinate of gx once.  Nothing of another lane or
//             another row enters a sum: the bits of a row do not depend on the batch it is in.
// The tables hold int32 point indices, validated by the caller on the host.  The kernels never reject: an index outside
// [0, n_atoms) is not dereferenced and makes its entry NaN, an item that names no entry is skipped, an offset outside
// the item list is clipped to it.
//
// The polar kernels are element-wise over contiguous arrays, with 16-byte accesses when every pointer is 16-byte aligned.
//
// Both families move a few values per entry and do tens of fp64 operations on each; whether HBM traffic or fp64 issue
// bounds them has not been measured (tools/measure_geometry.py).
#include <initializer_list>

#include "common.h"
#include "geometry.h"

namespace tfep {

constexpr int GEOM_ROWS = 4;                // rows (waves) per workgroup

struct IndexTables {
    const int32_t *pairs, *triples, *quads;      // (2, P), (3, A), (4, T), row-major
    int P, A, T;
};

// Point i of a row, NaN when the index is out of range.
template <typename T>
__device__ __forceinline__ void load_point(const T* __restrict__ xr, int i, int n_atoms, double (&v)[3]) {
    if ((unsigned)i < (unsigned)n_atoms) {
        v[0] = (double)xr[3 * i], v[1] = (double)xr[3 * i + 1], v[2] = (double)xr[3 * i + 2];
    } else {
        v[0] = v[1] = v[2] = __builtin_nan("");
    }
}

template <typename T>
__global__ void __launch_bounds__(256) internal_coordinates_kernel(const T* __restrict__ x, int64_t ldx, IndexTables tb,
                                                                   T* __restrict__ d, T* __restrict__ a, T* __restrict__ t,
                                                                   int n_atoms, int B) {
    const int row = blockIdx.x * GEOM_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    for (int e = lane; e < tb.P + tb.A + tb.T; e += WAVE) {
        double p0[3], p1[3], p2[3], p3[3];
        if (e < tb.P) {
            load_point(xr, tb.pairs[e], n_atoms, p0);
            load_point(xr, tb.pairs[tb.P + e], n_atoms, p1);
            d[(int64_t)row * tb.P + e] = (T)ic_distance(p0, p1);
        } else if (e < tb.P + tb.A) {
            const int k = e - tb.P;
            load_point(xr, tb.triples[k], n_atoms, p0);
            load_point(xr, tb.triples[tb.A + k], n_atoms, p1);
            load_point(xr, tb.triples[2 * tb.A + k], n_atoms, p2);
            a[(int64_t)row * tb.A + k] = (T)ic_angle(p0, p1, p2);
        } else {
            const int k = e - tb.P - tb.A;
            load_point(xr, tb.quads[k], n_atoms, p0);
            load_point(xr, tb.quads[tb.T + k], n_atoms, p1);
            load_point(xr, tb.quads[2 * tb.T + k], n_atoms, p2);
            load_point(xr, tb.quads[3 * tb.T + k], n_atoms, p3);
            DihedralState st;
            t[(int64_t)row * tb.T + k] = (T)ic_dihedral(p0, p1, p2, p3, st);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) internal_coordinates_backward_kernel(
    const T* __restrict__ x, int64_t ldx, IndexTables tb, const int32_t* __restrict__ atom_start,
    const int32_t* __restrict__ atom_items, int n_items, const T* __restrict__ gd, const T* __restrict__ ga, const T* __restrict__ gt,
    T* __restrict__ gx, int64_t ldgx, int n_atoms, int B) {
    const int row = blockIdx.x * GEOM_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const T* xr = x + (int64_t)row * ldx;
    T* gxr = gx + (int64_t)row * ldgx;
    for (int i = lane; i < n_atoms; i += WAVE) {
        double acc[3] = {0.0, 0.0, 0.0};
        const int j0 = atom_start[i], j1 = atom_start[i + 1];
        for (int j = j0 < 0 ? 0 : j0; j < (j1 < n_items ? j1 : n_items); ++j) {
            const int item = atom_items[j], e = item >> 2, slot = item & 3;
            double p0[3], p1[3], p2[3], p3[3], g[4][3];
            if (e < 0 || e >= tb.P + tb.A + tb.T) continue;
            if (e < tb.P) {
                load_point(xr, tb.pairs[e], n_atoms, p0);
                load_point(xr, tb.pairs[tb.P + e], n_atoms, p1);
                ic_distance_vjp(p0, p1, (double)gd[(int64_t)row * tb.P + e], g[0], g[1]);
            } else if (e < tb.P + tb.A) {
                const int k = e - tb.P;
                load_point(xr, tb.triples[k], n_atoms, p0);
                load_point(xr, tb.triples[tb.A + k], n_atoms, p1);
                load_point(xr, tb.triples[2 * tb.A + k], n_atoms, p2);
                ic_angle_vjp(p0, p1, p2, (double)ga[(int64_t)row * tb.A + k], g[0], g[1], g[2]);
            } else {
                const int k = e - tb.P - tb.A;
                load_point(xr, tb.quads[k], n_atoms, p0);
                load_point(xr, tb.quads[tb.T + k], n_atoms, p1);
                load_point(xr, tb.quads[2 * tb.T + k], n_atoms, p2);
                load_point(xr, tb.quads[3 * tb.T + k], n_atoms, p3);
                ic_dihedral_vjp(p0, p1, p2, p3, (double)gt[(int64_t)row * tb.T + k], g[0], g[1], g[2], g[3]);
            }
            // (selected by comparison: a run-time index into g would put it in scratch memory; the slots an entry
            // does not have are never named by a valid item)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += slot == 0 ? g[0][c] : slot == 1 ? g[1][c] : slot == 2 ? g[2][c] : g[3][c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gxr[3 * i + c] = (T)acc[c];
    }
}

// elements of a 16-byte access
template <typename T>
constexpr int POLAR_VEC = 16 / sizeof(T);

// Element-wise: each thread takes the VEC consecutive elements from `i`; VEC = 1 is the unaligned and the tail path.
template <typename T, int VEC>
__device__ __forceinline__ void polar_elements(const T* __restrict__ a, const T* __restrict__ b, int to_cartesian,
                                               T* __restrict__ o0, T* __restrict__ o1, T* __restrict__ ldj, int64_t i) {
    struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
    const Pack pa = *reinterpret_cast<const Pack*>(a + i), pb = *reinterpret_cast<const Pack*>(b + i);
    Pack r0, r1, rl;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        double v0, v1, vl;
        polar_map(to_cartesian, (double)pa.v[k], (double)pb.v[k], v0, v1, vl);
        r0.v[k] = (T)v0, r1.v[k] = (T)v1, rl.v[k] = (T)vl;
    }
    *reinterpret_cast<Pack*>(o0 + i) = r0;
    *reinterpret_cast<Pack*>(o1 + i) = r1;
    if (ldj) *reinterpret_cast<Pack*>(ldj + i) = rl;
}

template <typename T, int VEC>
__device__ __forceinline__ void polar_backward_elements(const T* __restrict__ a, const T* __restrict__ b, int to_cartesian,
                                                        const T* __restrict__ g0, const T* __restrict__ g1,
                                                        const T* __restrict__ gl, T* __restrict__ ga, T* __restrict__ gb,
                                                        int64_t i) {
    struct alignas(sizeof(T) * VEC) Pack { T v[VEC]; };
    const Pack pa = *reinterpret_cast<const Pack*>(a + i), pb = *reinterpret_cast<const Pack*>(b + i);
    const Pack p0 = *reinterpret_cast<const Pack*>(g0 + i), p1 = *reinterpret_cast<const Pack*>(g1 + i);
    Pack pl, ra, rb;
    if (gl) pl = *reinterpret_cast<const Pack*>(gl + i);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        double va, vb;
        polar_map_vjp(to_cartesian, (double)pa.v[k], (double)pb.v[k], (double)p0.v[k], (double)p1.v[k],
                      gl ? (double)pl.v[k] : 0.0, va, vb);
        ra.v[k] = (T)va, rb.v[k] = (T)vb;
    }
    *reinterpret_cast<Pack*>(ga + i) = ra;
    *reinterpret_cast<Pack*>(gb + i) = rb;
}

// `n_vec` elements from the front in packs of VEC per thread, the rest one per thread (n_vec = 0: all of them).
template <typename T>
__global__ void __launch_bounds__(256) polar_kernel(const T* __restrict__ a, const T* __restrict__ b, int to_cartesian,
                                                    T* __restrict__ o0, T* __restrict__ o1, T* __restrict__ ldj,
                                                    int64_t n_vec, int64_t n) {
    constexpr int VEC = POLAR_VEC<T>;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < n_vec / VEC) polar_elements<T, VEC>(a, b, to_cartesian, o0, o1, ldj, tid * VEC);
    else if (tid - n_vec / VEC < n - n_vec) polar_elements<T, 1>(a, b, to_cartesian, o0, o1, ldj, n_vec + tid - n_vec / VEC);
}

template <typename T>
__global__ void __launch_bounds__(256) polar_backward_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                             int to_cartesian, const T* __restrict__ g0,
                                                             const T* __restrict__ g1, const T* __restrict__ gl,
                                                             T* __restrict__ ga, T* __restrict__ gb, int64_t n_vec,
                                                             int64_t n) {
    constexpr int VEC = POLAR_VEC<T>;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < n_vec / VEC) polar_backward_elements<T, VEC>(a, b, to_cartesian, g0, g1, gl, ga, gb, tid * VEC);
    else if (tid - n_vec / VEC < n - n_vec)
        polar_backward_elements<T, 1>(a, b, to_cartesian, g0, g1, gl, ga, gb, n_vec + tid - n_vec / VEC);
}

// ---------------------------------------------------------------------------------------------------------------- host

static int tables_check(const char* who, const IndexTables& tb, int n_atoms, int B, int64_t ldx) {
    TFEP_REQUIRE(B >= 0 && n_atoms >= 0 && tb.P >= 0 && tb.A >= 0 && tb.T >= 0, "%s: negative size", who);
    TFEP_REQUIRE(n_atoms <= 0x7fffffff / 4, "%s: n_atoms=%d too large", who, n_atoms);
    TFEP_REQUIRE((int64_t)tb.P + tb.A + tb.T <= 0x7fffffff / 4, "%s: %d + %d + %d table entries are too many", who, tb.P,
                 tb.A, tb.T);
    TFEP_REQUIRE((tb.pairs || !tb.P) && (tb.triples || !tb.A) && (tb.quads || !tb.T), "%s: a non-empty table is NULL", who);
    TFEP_REQUIRE(ldx >= (int64_t)3 * n_atoms, "%s: a row stride is shorter than the row (%d points of 3)", who, n_atoms);
    return TFEP_OK;
}

static inline unsigned geom_blocks(int B) { return (unsigned)((B + GEOM_ROWS - 1) / GEOM_ROWS); }

template <typename T>
static int launch_internal_coordinates(const char* who, const T* x, int64_t ldx, IndexTables tb, T* d, T* a, T* t,
                                       int n_atoms, int B, void* stream) {
    if (int rc = tables_check(who, tb, n_atoms, B, ldx)) return rc;
    TFEP_REQUIRE((d || !tb.P) && (a || !tb.A) && (t || !tb.T), "%s: the output of a non-empty table is NULL", who);
    if (B == 0 || tb.P + tb.A + tb.T == 0) return TFEP_OK;
    TFEP_REQUIRE(x, "%s: x must be non-NULL", who);
    internal_coordinates_kernel<T><<<geom_blocks(B), 256, 0, (hipStream_t)stream>>>(x, ldx, tb, d, a, t, n_atoms, B);
    return check_launch("internal_coordinates_kernel");
}

template <typename T>
static int launch_internal_coordinates_backward(const char* who, const T* x, int64_t ldx, IndexTables tb,
                                                const int32_t* atom_start, const int32_t* atom_items, int n_items,
                                                const T* gd, const T* ga, const T* gt, T* gx, int64_t ldgx, int n_atoms,
                                                int B, void* stream) {
    if (int rc = tables_check(who, tb, n_atoms, B, ldx < ldgx ? ldx : ldgx)) return rc;
    TFEP_REQUIRE((gd || !tb.P) && (ga || !tb.A) && (gt || !tb.T), "%s: the cotangent of a non-empty table is NULL", who);
    if (B == 0 || n_atoms == 0) return TFEP_OK;
    TFEP_REQUIRE(n_items >= 0 && (atom_items || n_items == 0), "%s: n_items=%d without the items", who, n_items);
    TFEP_REQUIRE(x && gx && atom_start, "%s: x/gx/atom_start must be non-NULL", who);
    internal_coordinates_backward_kernel<T><<<geom_blocks(B), 256, 0, (hipStream_t)stream>>>(
        x, ldx, tb, atom_start, atom_items, n_items, gd, ga, gt, gx, ldgx, n_atoms, B);
    return check_launch("internal_coordinates_backward_kernel");
}

// The elements the 16-byte path takes: all whole packs when every pointer is 16-byte aligned, else none.
template <typename T>
static int64_t polar_n_vec(int64_t n, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p % 16 != 0) return 0;
    return n - n % POLAR_VEC<T>;
}

static inline unsigned polar_blocks(int64_t n_threads) { return (unsigned)((n_threads + 255) / 256); }

template <typename T>
static int launch_polar(const char* who, const T* a, const T* b, int to_cartesian, T* o0, T* o1, T* ldj, int64_t n,
                        void* stream) {
    TFEP_REQUIRE(n >= 0 && n <= ((int64_t)1 << 38), "%s: n=%lld out of range", who, (long long)n);
    if (n == 0) return TFEP_OK;
    TFEP_REQUIRE(a && b && o0 && o1, "%s: the inputs and the two outputs must be non-NULL", who);
    const int64_t n_vec = polar_n_vec<T>(n, {a, b, o0, o1, ldj});
    polar_kernel<T><<<polar_blocks(n_vec / POLAR_VEC<T> + (n - n_vec)), 256, 0, (hipStream_t)stream>>>(
        a, b, to_cartesian != 0, o0, o1, ldj, n_vec, n);
    return check_launch("polar_kernel");
}

template <typename T>
static int launch_polar_backward(const char* who, const T* a, const T* b, int to_cartesian, const T* g0, const T* g1,
                                 const T* gl, T* ga, T* gb, int64_t n, void* stream) {
    TFEP_REQUIRE(n >= 0 && n <= ((int64_t)1 << 38), "%s: n=%lld out of range", who, (long long)n);
    if (n == 0) return TFEP_OK;
    TFEP_REQUIRE(a && b && g0 && g1 && ga && gb, "%s: the inputs, the two cotangents and the two outputs must be non-NULL",
                 who);
    const int64_t n_vec = polar_n_vec<T>(n, {a, b, g0, g1, gl, ga, gb});
    polar_backward_kernel<T><<<polar_blocks(n_vec / POLAR_VEC<T> + (n - n_vec)), 256, 0, (hipStream_t)stream>>>(
        a, b, to_cartesian != 0, g0, g1, gl, ga, gb, n_vec, n);
    return check_launch("polar_backward_kernel");
}

}  // namespace tfep

using namespace tfep;

// The float and the double entry point of each launcher, from one argument list.
#define TFEP_GEOMETRY_ENTRY(T, sfx)                                                                                          \
    int tfep_internal_coordinates##sfx(const T* x, int64_t ldx, const int32_t* pairs, int n_pairs, const int32_t* triples,   \
                                       int n_triples, const int32_t* quads, int n_quads, T* d, T* a, T* t, int n_atoms,      \
                                       int B, void* stream) {                                                                \
        return launch_internal_coordinates<T>("internal_coordinates" #sfx, x, ldx,                                          \
                                              IndexTables{pairs, triples, quads, n_pairs, n_triples, n_quads}, d, a, t,      \
                                              n_atoms, B, stream);                                                           \
    }                                                                                                                        \
    int tfep_internal_coordinates_backward##sfx(const T* x, int64_t ldx, const int32_t* pairs, int n_pairs,                  \
                                                const int32_t* triples, int n_triples, const int32_t* quads, int n_quads,    \
                                                const int32_t* atom_start, const int32_t* atom_items, int n_items,           \
                                                const T* gd, const T* ga, const T* gt, T* gx, int64_t ldgx, int n_atoms,     \
                                                int B, void* stream) {                                                       \
        return launch_internal_coordinates_backward<T>("internal_coordinates_backward" #sfx, x, ldx,                        \
                                                       IndexTables{pairs, triples, quads, n_pairs, n_triples, n_quads},      \
                                                       atom_start, atom_items, n_items, gd, ga, gt, gx, ldgx, n_atoms, B,    \
                                                       stream);                                                              \
    }                                                                                                                        \
    int tfep_polar##sfx(const T* a, const T* b, int to_cartesian, T* out0, T* out1, T* log_det_J, int64_t n,                 \
                        void* stream) {                                                                                      \
        return launch_polar<T>("polar" #sfx, a, b, to_cartesian, out0, out1, log_det_J, n, stream);                          \
    }                                                                                                                        \
    int tfep_polar_backward##sfx(const T* a, const T* b, int to_cartesian, const T* g0, const T* g1, const T* gl, T* ga,     \
                                 T* gb, int64_t n, void* stream) {                                                           \
        return launch_polar_backward<T>("polar_backward" #sfx, a, b, to_cartesian, g0, g1, gl, ga, gb, n, stream);           \
    }

extern "C" {
TFEP_GEOMETRY_ENTRY(float, )
TFEP_GEOMETRY_ENTRY(double, _f64)
}  // extern "C"
