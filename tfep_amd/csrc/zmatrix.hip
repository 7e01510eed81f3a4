// Placement of the atoms of a batch of rows from a Z-matrix -- (d, a, t) and the fixed atoms to Cartesian positions, with
// the log-det -- and its VJP, float32 and float64.  The per-atom arithmetic is in zmatrix.h.  This is the inverse of the
// internal-coordinate kernel of geometry.hip on the tables of one Z-matrix.
//
// An atom is placed from three atoms that are in place already, so the rows of a Z-matrix form a dependency graph.  The
// host (ops.zmatrix_tables) sorts them into LEVELS: the fixed atoms are level 0, an atom is one level above the highest of
// its three references, and the atoms of one level do not depend on each other.  The kernels take
//   rows         (5, n_ic) int32, row-major, level-sorted: the atom placed, its references j, k, l, and the column of
//                (d, a, t) that holds its values (the caller's row order)
//   level_start  n_levels + 1 offsets into the sorted rows
//   fixed        the n_fixed atoms whose positions are given
// Layout, as geometry.hip: one wave per sample row, fp64 arithmetic for both element types, one rounding on store, row
// strides as arguments, no atomics.  Nothing of another wave or another row enters a value: the bits of a row do not
// depend on the batch it is in, nor on the number of rows a workgroup holds.
//   forward   the wave copies the fixed atoms into its output row, then walks the levels in order, the lanes striding
//             over the atoms of a level.  Every position is kept in fp64 in LDS (3 n_atoms doubles per row) and later
//             levels read it from there: a float32 row is rounded once, on store, and never read back.  A lane adds the
//             log-det contributions of its atoms level by level; the 64 lane sums are reduced by the butterfly of wave_sum.
//   backward  the wave walks the levels in reverse, a lane owning one atom at a time.  The atom's cotangent is its incoming
//             one plus what the atoms placed from it (its children, all in higher levels) sent, gathered in table order
//             from the atom's incidence list: atom_start (n_atoms + 1 offsets) and atom_items (4 * sorted row + slot, slot
//             0, 1, 2 for a child that names the atom as j, k, l).  The lane computes (g_d, g_a, g_t), writes them, and
//             leaves its three contributions in LDS (9 doubles per sorted row) for lower levels.  The fixed atoms gather
//             last and write g_x_fixed.  Every output element is written once.  The positions are read from the forward's
//             output.
// Between two levels the wave's LDS writes must be visible to its own later reads from other lanes: wave_lds_sync() is a
// wavefront-scope release fence, a wave barrier and an acquire fence -- the memory model's statement of that ordering,
// which neither assumes that the lanes run in lock step nor waits for the other waves of the workgroup (they work on
// other rows, and a row past the batch has left).
//
// The workgroup holds as many rows as fit 64 KiB of LDS, four at the most; one row may take up to the CU's 160 KiB
// (ZMATRIX_LDS_LIMIT), and a row that needs more is an invalid argument before anything is launched.
//
// The tables are validated by the caller on the host.  The kernels never reject: an index outside its range is not
// dereferenced and makes its atom NaN (or is not written), an item that names no row is skipped, an offset outside a
// list is clipped to it.
#include "common.h"
#include "zmatrix.h"

namespace tfep {

constexpr int ZMATRIX_MAX_ROWS = 4;                       // rows (waves) per workgroup, at the most
constexpr int64_t ZMATRIX_LDS_SHARED = 64 * 1024;         // what a workgroup of several rows may take
constexpr int64_t ZMATRIX_LDS_LIMIT = 160 * 1024;         // the LDS of a CU: one row may take it all

struct ZTables {
    const int32_t *rows, *level_start, *fixed;            // (5, n_ic), (n_levels + 1), (n_fixed)
    int n_ic, n_levels, n_fixed, n_atoms;
};

// Orders this wave's LDS writes before its later LDS reads, across lanes.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int clip(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// Point i of an fp64 LDS row, NaN when the index is out of range.
__device__ __forceinline__ void lds_point(const double* pos, int i, int n_atoms, double (&v)[3]) {
    if ((unsigned)i < (unsigned)n_atoms) {
        v[0] = pos[3 * i], v[1] = pos[3 * i + 1], v[2] = pos[3 * i + 2];
    } else {
        v[0] = v[1] = v[2] = __builtin_nan("");
    }
}

template <typename T>
__device__ __forceinline__ void global_point(const T* __restrict__ xr, int i, int n_atoms, double (&v)[3]) {
    if ((unsigned)i < (unsigned)n_atoms) {
        v[0] = (double)xr[3 * i], v[1] = (double)xr[3 * i + 1], v[2] = (double)xr[3 * i + 2];
    } else {
        v[0] = v[1] = v[2] = __builtin_nan("");
    }
}

template <typename T>
__global__ void __launch_bounds__(256) zmatrix_place_kernel(const T* __restrict__ d, int64_t ldd, const T* __restrict__ a,
                                                            int64_t lda, const T* __restrict__ t, int64_t ldt,
                                                            const T* __restrict__ x_fixed, int64_t ldf, ZTables tb,
                                                            T* __restrict__ x, int64_t ldx, T* __restrict__ log_det_J,
                                                            int rows_per_block, int B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * rows_per_block + wave;
    if (row >= B) return;                                  // (nothing below waits for another wave)
    double* pos = reinterpret_cast<double*>(smem) + (int64_t)wave * 3 * tb.n_atoms;
    const int n = tb.n_atoms, n_ic = tb.n_ic;
    T* xr = x + (int64_t)row * ldx;

    for (int f = lane; f < tb.n_fixed; f += WAVE) {
        const int i = tb.fixed[f];
        if ((unsigned)i >= (unsigned)n) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const T v = x_fixed[(int64_t)row * ldf + 3 * f + c];
            pos[3 * i + c] = (double)v;
            xr[3 * i + c] = v;
        }
    }
    wave_lds_sync();

    double ldj = 0.0;
    for (int level = 0; level < tb.n_levels; ++level) {
        const int s0 = clip(tb.level_start[level], n_ic), s1 = clip(tb.level_start[level + 1], n_ic);
        for (int s = s0 + lane; s < s1; s += WAVE) {
            const int i = tb.rows[s], col = tb.rows[4 * n_ic + s];
            double xj[3], xk[3], xl[3], xi[3];
            lds_point(pos, tb.rows[n_ic + s], n, xj);
            lds_point(pos, tb.rows[2 * n_ic + s], n, xk);
            lds_point(pos, tb.rows[3 * n_ic + s], n, xl);
            const bool has = (unsigned)col < (unsigned)n_ic;
            const double nan = __builtin_nan("");
            PlaceState ps;
            ldj += place_atom(xj, xk, xl, has ? (double)d[(int64_t)row * ldd + col] : nan,
                              has ? (double)a[(int64_t)row * lda + col] : nan,
                              has ? (double)t[(int64_t)row * ldt + col] : nan, xi, ps);
            if ((unsigned)i < (unsigned)n) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    pos[3 * i + c] = xi[c];
                    xr[3 * i + c] = (T)xi[c];
                }
            }
        }
        wave_lds_sync();
    }
    ldj = wave_sum(ldj);
    if (lane == 0) log_det_J[row] = (T)ldj;
}

struct ZIncidence {
    const int32_t *atom_start, *atom_items;               // (n_atoms + 1), (n_items): 4 * sorted row + slot
    int n_items;
};

// The cotangent of atom i: its incoming one, then its children's contributions in the order of its incidence list.
template <typename T>
__device__ __forceinline__ void gather_cotangent(const T* __restrict__ gxr, const double* contrib, int i, const ZTables& tb,
                                                 const ZIncidence& inc, double (&g)[3]) {
    if ((unsigned)i >= (unsigned)tb.n_atoms) {
        g[0] = g[1] = g[2] = __builtin_nan("");
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) g[c] = (double)gxr[3 * i + c];
    const int j0 = clip(inc.atom_start[i], inc.n_items), j1 = clip(inc.atom_start[i + 1], inc.n_items);
    for (int j = j0; j < j1; ++j) {
        const int item = inc.atom_items[j], s = item >> 2, slot = item & 3;
        if (item < 0 || s >= tb.n_ic || slot == 3) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] += contrib[9 * s + 3 * slot + c];
    }
}

template <typename T>
__global__ void __launch_bounds__(256) zmatrix_place_backward_kernel(
    const T* __restrict__ x, int64_t ldx, const T* __restrict__ d, int64_t ldd, const T* __restrict__ a, int64_t lda,
    const T* __restrict__ t, int64_t ldt, ZTables tb, ZIncidence inc, const T* __restrict__ gx, int64_t ldgx,
    const T* __restrict__ gl, T* __restrict__ gd, T* __restrict__ ga, T* __restrict__ gt, T* __restrict__ g_fixed,
    int rows_per_block, int B) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * rows_per_block + wave;
    if (row >= B) return;                                  // (nothing below waits for another wave)
    double* contrib = reinterpret_cast<double*>(smem) + (int64_t)wave * 9 * tb.n_ic;
    const int n = tb.n_atoms, n_ic = tb.n_ic;
    const T* xr = x + (int64_t)row * ldx;
    const T* gxr = gx + (int64_t)row * ldgx;
    const double g_ldj = (double)gl[row];

    for (int level = tb.n_levels - 1; level >= 0; --level) {
        const int s0 = clip(tb.level_start[level], n_ic), s1 = clip(tb.level_start[level + 1], n_ic);
        for (int s = s0 + lane; s < s1; s += WAVE) {
            const int col = tb.rows[4 * n_ic + s];
            double g[3], xj[3], xk[3], xl[3], gj[3], gk[3], gl3[3], vd, va, vt;
            gather_cotangent(gxr, contrib, tb.rows[s], tb, inc, g);
            global_point(xr, tb.rows[n_ic + s], n, xj);
            global_point(xr, tb.rows[2 * n_ic + s], n, xk);
            global_point(xr, tb.rows[3 * n_ic + s], n, xl);
            const bool has = (unsigned)col < (unsigned)n_ic;
            const double nan = __builtin_nan("");
            place_atom_vjp(xj, xk, xl, has ? (double)d[(int64_t)row * ldd + col] : nan,
                           has ? (double)a[(int64_t)row * lda + col] : nan, has ? (double)t[(int64_t)row * ldt + col] : nan,
                           g, g_ldj, vd, va, vt, gj, gk, gl3);
            if (has) {
                gd[(int64_t)row * n_ic + col] = (T)vd;
                ga[(int64_t)row * n_ic + col] = (T)va;
                gt[(int64_t)row * n_ic + col] = (T)vt;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                contrib[9 * s + c] = gj[c];
                contrib[9 * s + 3 + c] = gk[c];
                contrib[9 * s + 6 + c] = gl3[c];
            }
        }
        wave_lds_sync();
    }
    for (int f = lane; f < tb.n_fixed; f += WAVE) {
        double g[3];
        gather_cotangent(gxr, contrib, tb.fixed[f], tb, inc, g);
#pragma unroll
        for (int c = 0; c < 3; ++c) g_fixed[(int64_t)row * 3 * tb.n_fixed + 3 * f + c] = (T)g[c];
    }
}

// ---------------------------------------------------------------------------------------------------------------- host

// The launch shape of a kernel (the forward keeps 3 doubles per atom, the backward 9 per placed atom): rows per workgroup
// and the workgroup's LDS; an invalid argument when one row does not fit.  The launchers and the exported query
// tfep_zmatrix_launch_shape both come through here.
static int zmatrix_launch_shape(const char* who, int n_atoms, int n_ic, bool backward, int* rows, int64_t* lds) {
    TFEP_REQUIRE(n_atoms >= 0 && n_ic >= 0, "%s: negative size", who);
    const int64_t row_bytes = (backward ? (int64_t)9 * n_ic : (int64_t)3 * n_atoms) * (int64_t)sizeof(double);
    TFEP_REQUIRE(row_bytes <= ZMATRIX_LDS_LIMIT,
                 "%s: a row needs %lld bytes of LDS, the limit is %lld (6826 atoms forward, 2275 placed atoms backward)", who,
                 (long long)row_bytes, (long long)ZMATRIX_LDS_LIMIT);
    const int64_t fit = row_bytes > 0 ? ZMATRIX_LDS_SHARED / row_bytes : ZMATRIX_MAX_ROWS;
    *rows = fit < 1 ? 1 : fit > ZMATRIX_MAX_ROWS ? ZMATRIX_MAX_ROWS : (int)fit;
    *lds = *rows * row_bytes;
    return TFEP_OK;
}

// A workgroup that takes more dynamic LDS than a kernel gets by default (48 KiB is the lowest default of the runtimes in
// use) needs the attribute; set once per kernel and device, to the whole limit.
template <typename K>
static int allow_lds(K kernel, int64_t lds, bool (&done)[TFEP_MAX_DEVICES], const char* who) {
    bool& set = done[current_device_slot()];
    if (lds > 48 * 1024 && !set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)ZMATRIX_LDS_LIMIT);
        if (e != hipSuccess) return fail(TFEP_ERR_LAUNCH, "%s: hipFuncSetAttribute(LDS=%d): %s", who, (int)ZMATRIX_LDS_LIMIT,
                                         hipGetErrorString(e));
        set = true;
    }
    return TFEP_OK;
}

static int ztables_check(const char* who, const ZTables& tb, int B) {
    TFEP_REQUIRE(B >= 0 && tb.n_atoms >= 0 && tb.n_ic >= 0 && tb.n_levels >= 0 && tb.n_fixed >= 0, "%s: negative size", who);
    TFEP_REQUIRE(tb.n_atoms <= 0x7fffffff / 16 && tb.n_ic <= 0x7fffffff / 16, "%s: n_atoms=%d / n_ic=%d too large", who,
                 tb.n_atoms, tb.n_ic);
    TFEP_REQUIRE((int64_t)tb.n_fixed + tb.n_ic == tb.n_atoms, "%s: %d fixed and %d placed atoms are not the %d atoms", who,
                 tb.n_fixed, tb.n_ic, tb.n_atoms);
    TFEP_REQUIRE((tb.rows || !tb.n_ic) && (tb.fixed || !tb.n_fixed) && (tb.level_start || !tb.n_levels),
                 "%s: a non-empty table is NULL", who);
    return TFEP_OK;
}

template <typename T>
static int launch_zmatrix_place(const char* who, const T* d, int64_t ldd, const T* a, int64_t lda, const T* t, int64_t ldt,
                                const T* x_fixed, int64_t ldf, ZTables tb, T* x, int64_t ldx, T* log_det_J, int B,
                                void* stream) {
    if (int rc = ztables_check(who, tb, B)) return rc;
    TFEP_REQUIRE(ldd >= tb.n_ic && lda >= tb.n_ic && ldt >= tb.n_ic && ldf >= (int64_t)3 * tb.n_fixed &&
                     ldx >= (int64_t)3 * tb.n_atoms, "%s: a row stride is shorter than the row", who);
    int rows;
    int64_t lds;
    if (int rc = zmatrix_launch_shape(who, tb.n_atoms, tb.n_ic, false, &rows, &lds)) return rc;
    if (B == 0) return TFEP_OK;
    TFEP_REQUIRE(log_det_J && (x || !tb.n_atoms) && (x_fixed || !tb.n_fixed) && ((d && a && t) || !tb.n_ic),
                 "%s: d/a/t/x_fixed/x/log_det_J must be non-NULL", who);
    static bool attr_done[TFEP_MAX_DEVICES] = {};
    if (int rc = allow_lds(zmatrix_place_kernel<T>, lds, attr_done, who)) return rc;
    zmatrix_place_kernel<T><<<(unsigned)((B + rows - 1) / rows), rows * WAVE, (size_t)lds, (hipStream_t)stream>>>(
        d, ldd, a, lda, t, ldt, x_fixed, ldf, tb, x, ldx, log_det_J, rows, B);
    return check_launch("zmatrix_place_kernel");
}

template <typename T>
static int launch_zmatrix_place_backward(const char* who, const T* x, int64_t ldx, const T* d, int64_t ldd, const T* a,
                                         int64_t lda, const T* t, int64_t ldt, ZTables tb, ZIncidence inc, const T* gx,
                                         int64_t ldgx, const T* gl, T* gd, T* ga, T* gt, T* g_fixed, int B, void* stream) {
    if (int rc = ztables_check(who, tb, B)) return rc;
    TFEP_REQUIRE(ldd >= tb.n_ic && lda >= tb.n_ic && ldt >= tb.n_ic && ldx >= (int64_t)3 * tb.n_atoms &&
                     ldgx >= (int64_t)3 * tb.n_atoms, "%s: a row stride is shorter than the row", who);
    TFEP_REQUIRE(inc.n_items >= 0 && (inc.atom_items || inc.n_items == 0), "%s: n_items=%d without the items", who,
                 inc.n_items);
    int rows;
    int64_t lds;
    if (int rc = zmatrix_launch_shape(who, tb.n_atoms, tb.n_ic, true, &rows, &lds)) return rc;
    if (B == 0 || tb.n_atoms == 0) return TFEP_OK;
    TFEP_REQUIRE(x && gx && gl && inc.atom_start && (g_fixed || !tb.n_fixed) && ((d && a && t && gd && ga && gt) || !tb.n_ic),
                 "%s: x/d/a/t, the cotangents, the outputs and atom_start must be non-NULL", who);
    static bool attr_done[TFEP_MAX_DEVICES] = {};
    if (int rc = allow_lds(zmatrix_place_backward_kernel<T>, lds, attr_done, who)) return rc;
    zmatrix_place_backward_kernel<T><<<(unsigned)((B + rows - 1) / rows), rows * WAVE, (size_t)lds, (hipStream_t)stream>>>(
        x, ldx, d, ldd, a, lda, t, ldt, tb, inc, gx, ldgx, gl, gd, ga, gt, g_fixed, rows, B);
    return check_launch("zmatrix_place_backward_kernel");
}

}  // namespace tfep

using namespace tfep;

// The float and the double entry point of each launcher, from one argument list.
#define TFEP_ZMATRIX_ENTRY(T, sfx)                                                                                           \
    int tfep_zmatrix_place##sfx(const T* d, int64_t ldd, const T* a, int64_t lda, const T* t, int64_t ldt, const T* x_fixed, \
                                int64_t ldf, const int32_t* rows, int n_ic, const int32_t* level_start, int n_levels,        \
                                const int32_t* fixed, int n_fixed, T* x, int64_t ldx, T* log_det_J, int n_atoms, int B,      \
                                void* stream) {                                                                              \
        return launch_zmatrix_place<T>("zmatrix_place" #sfx, d, ldd, a, lda, t, ldt, x_fixed, ldf,                           \
                                       ZTables{rows, level_start, fixed, n_ic, n_levels, n_fixed, n_atoms}, x, ldx,          \
                                       log_det_J, B, stream);                                                                \
    }                                                                                                                        \
    int tfep_zmatrix_place_backward##sfx(const T* x, int64_t ldx, const T* d, int64_t ldd, const T* a, int64_t lda,          \
                                         const T* t, int64_t ldt, const int32_t* rows, int n_ic,                             \
                                         const int32_t* level_start, int n_levels, const int32_t* fixed, int n_fixed,        \
                                         const int32_t* atom_start, const int32_t* atom_items, int n_items, const T* gx,     \
                                         int64_t ldgx, const T* gl, T* gd, T* ga, T* gt, T* g_fixed, int n_atoms, int B,     \
                                         void* stream) {                                                                     \
        return launch_zmatrix_place_backward<T>("zmatrix_place_backward" #sfx, x, ldx, d, ldd, a, lda, t, ldt,               \
                                                ZTables{rows, level_start, fixed, n_ic, n_levels, n_fixed, n_atoms},         \
                                                ZIncidence{atom_start, atom_items, n_items}, gx, ldgx, gl, gd, ga, gt,       \
                                                g_fixed, B, stream);                                                         \
    }

extern "C" {
TFEP_ZMATRIX_ENTRY(float, )
TFEP_ZMATRIX_ENTRY(double, _f64)

int tfep_zmatrix_launch_shape(int n_atoms, int n_ic, int backward, int* rows_per_block, int64_t* lds_bytes) {
    TFEP_REQUIRE(rows_per_block && lds_bytes, "zmatrix_launch_shape: rows_per_block and lds_bytes must be non-NULL");
    return zmatrix_launch_shape("zmatrix_launch_shape", n_atoms, n_ic, backward != 0, rows_per_block, lds_bytes);
}
}  // extern "C"
