// The differentiable building blocks of tfep.nn.embeddings.radial and tfep.nn.graph for callers that assemble their own
// graph networks (reference radial.py:110-130, 161-176, 269-291; graph.py:304-316), float32 and float64:
//
//   radial expansion   f[i, k] = s(r_i) exp(-gamma_k (r_i - mu_k)^2),  gamma_k = exp(lg_k); s = 0.5 cos(pi r / r_c) + 0.5 with
//                      `switching` (zero beyond r_c when forced), else 1.  Forward in float64 here (the float32 forward is
//                      egnn.hip's radial_kernel, untouched) and the VJP in both types.
//   segment sum        forward in float64 (the float32 one is egnn.hip's), and its VJP, a row gather, in both types.
//
// Layout of the expansion kernels.  A wave owns GROUPS of 64 consecutive rows: lane l loads r of row l of the group and
// forms that row's switch and its derivative once; the wave then walks the 64 rows, every row's scalars broadcast from its
// lane, with the lanes over the basis functions k = 64 c + lane (coalesced rows of f and g).
//
// VJP.  Arithmetic in fp64 for both element types, one rounding on store.
//   g_r[i]    = sum_k g[i, k] (f_ik (-2 gamma_k (r_i - mu_k)) + e_ik s'(r_i)),  s' = -(pi / 2 r_c) sin(pi r / r_c):
//               the wave sums the 64 terms of a pass over k (butterfly), the passes are added in ascending k -- one fixed
//               order that does not depend on which other rows are in the batch.
//   g_mu[k]   = sum_i g[i, k] f_ik 2 gamma_k (r_i - mu_k),   g_lg[k] = -sum_i g[i, k] f_ik gamma_k (r_i - mu_k)^2:
//               lane-private running sums over the wave's rows, kept in the wave's own row of an fp64 workspace (read and
//               written once per group and 64 columns, by the lane that owns the column).  A second launch adds the workspace
//               rows: 16 interleaved slices in row order, then the 16 slices in order.  No atomics; the number of waves is a
//               function of n alone, so the order of every sum is one function of (n, K) and two calls agree bit for bit.
#include "common.h"

namespace tfep {

constexpr int RADIAL_WAVES = 4;                // waves per workgroup of the expansion kernels
constexpr int RADIAL_MAX_BLOCKS = 1024;        // workgroups of the expansion kernels (4096 workspace rows at most)
constexpr int RADIAL_SLICES = 16;              // waves per workgroup of the workspace reduction
constexpr double RADIAL_PI = 3.14159265358979323846;

static inline int64_t radial_groups(int64_t n) { return (n + WAVE - 1) / WAVE; }

static inline int radial_blocks(int64_t n) {
    const int64_t blocks = (radial_groups(n) + RADIAL_WAVES - 1) / RADIAL_WAVES;
    return (int)(blocks < 1 ? 1 : blocks > RADIAL_MAX_BLOCKS ? RADIAL_MAX_BLOCKS : blocks);
}

// workspace rows that are written: one per wave that owns at least one group
static inline int radial_partials(int64_t n) {
    const int64_t waves = (int64_t)radial_blocks(n) * RADIAL_WAVES, groups = radial_groups(n);
    return (int)(groups < waves ? groups : waves);
}

// The value lane j holds (j wave-uniform): a scalar read, whatever lanes are active.
__device__ inline float lane_value(float v, int j) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j));
}
__device__ inline double lane_value(double v, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

// The switch of one row and its derivative (1 and 0 without switching).
__device__ inline void radial_switch(double r, double r_cutoff, int switching, int force_zero, double* s, double* ds) {
    *s = 1.0;
    *ds = 0.0;
    if (!switching) return;
    double sn, cs;
    sincos(RADIAL_PI / r_cutoff * r, &sn, &cs);
    *s = 0.5 * cs + 0.5;
    *ds = -0.5 * (RADIAL_PI / r_cutoff) * sn;
    if (force_zero && r > r_cutoff) *s = *ds = 0.0;
}

template <typename T>
__global__ void __launch_bounds__(RADIAL_WAVES * WAVE) radial_forward_kernel(
    const T* __restrict__ r, int64_t n, const T* __restrict__ means, const T* __restrict__ log_gammas, int K, T r_cutoff,
    int switching, int force_zero, T* __restrict__ out) {
    const int lane = threadIdx.x % WAVE;
    const int64_t wave = (int64_t)blockIdx.x * RADIAL_WAVES + threadIdx.x / WAVE, n_waves = (int64_t)gridDim.x * RADIAL_WAVES;
    for (int64_t grp = wave; grp * WAVE < n; grp += n_waves) {
        const int64_t row0 = grp * WAVE;
        const int n_rows = (int)(n - row0 < WAVE ? n - row0 : WAVE);
        const T r_mine = lane < n_rows ? r[row0 + lane] : (T)0;
        T s_mine = (T)1;
        if (switching) {
            s_mine = (T)0.5 * cos((T)RADIAL_PI / r_cutoff * r_mine) + (T)0.5;
            if (force_zero && r_mine > r_cutoff) s_mine = (T)0;
        }
        for (int k0 = 0; k0 < K; k0 += WAVE) {
            const int k = k0 + lane;
            const bool live = k < K;
            const T mu = live ? means[k] : (T)0, gamma = live ? exp(log_gammas[k]) : (T)0;
            T* o = out + row0 * K + k;
            for (int j = 0; j < n_rows; ++j) {
                const T d = lane_value(r_mine, j) - mu;
                const T v = exp(-gamma * d * d) * lane_value(s_mine, j);
                if (live) o[(int64_t)j * K] = v;
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(RADIAL_WAVES * WAVE) radial_backward_kernel(
    const T* __restrict__ r, int64_t n, const T* __restrict__ means, const T* __restrict__ log_gammas, int K, double r_cutoff,
    int switching, int force_zero, const T* __restrict__ g, T* __restrict__ g_r, double* __restrict__ partial) {
    const int lane = threadIdx.x % WAVE;
    const int64_t wave = (int64_t)blockIdx.x * RADIAL_WAVES + threadIdx.x / WAVE, n_waves = (int64_t)gridDim.x * RADIAL_WAVES;
    double* mine = partial ? partial + wave * 2 * K : nullptr;      // [g_mu (K) | g_lg (K)] of this wave's rows
    bool first = true;
    for (int64_t grp = wave; grp * WAVE < n; grp += n_waves, first = false) {
        const int64_t row0 = grp * WAVE;
        const int n_rows = (int)(n - row0 < WAVE ? n - row0 : WAVE);
        const double r_mine = lane < n_rows ? (double)r[row0 + lane] : 0.0;
        double s_mine, ds_mine, gr_mine = 0.0;
        radial_switch(r_mine, r_cutoff, switching, force_zero, &s_mine, &ds_mine);
        for (int k0 = 0; k0 < K; k0 += WAVE) {                      // (wave-uniform trip count: wave_sum needs every lane)
            const int k = k0 + lane;
            const bool live = k < K;
            const double mu = live ? (double)means[k] : 0.0, gamma = live ? exp((double)log_gammas[k]) : 0.0;
            const T* gk = g + row0 * K + (live ? k : 0);
            double a_mu = 0.0, a_lg = 0.0;
            for (int j = 0; j < n_rows; ++j) {
                const double d = lane_value(r_mine, j) - mu, s = lane_value(s_mine, j), ds = lane_value(ds_mine, j);
                double t_r = 0.0;
                if (live) {
                    const double gv = (double)gk[(int64_t)j * K];
                    const double e = exp(-gamma * d * d), gf = gv * (s * e), gd = gamma * d;
                    t_r = gf * (-2.0 * gd) + gv * (e * ds);
                    a_mu += gf * (2.0 * gd);
                    a_lg -= gf * (gd * d);
                }
                if (g_r) {
                    // row j's terms of this pass, lanes in one order; lane j keeps the row's running sum over the passes
                    const double t = wave_sum(t_r);
                    if (lane == j) gr_mine += t;
                }
            }
            if (mine && live) {
                mine[k] = first ? a_mu : mine[k] + a_mu;
                mine[K + k] = first ? a_lg : mine[K + k] + a_lg;
            }
        }
        if (g_r && lane < n_rows) g_r[row0 + lane] = (T)gr_mine;
    }
}

// Workspace rows added per column: slice w adds the rows w, w + 16, ... in that order, then the 16 slices are added in
// order.  Writes zeros when there is no row (an empty batch).
template <typename T>
__global__ void __launch_bounds__(RADIAL_SLICES * WAVE) radial_reduce_kernel(const double* __restrict__ partial, int n_rows,
                                                                             int K, T* __restrict__ g_means,
                                                                             T* __restrict__ g_log_gammas) {
    __shared__ double sums[RADIAL_SLICES][WAVE];
    const int lane = threadIdx.x % WAVE, slice = threadIdx.x / WAVE;
    const int p = blockIdx.x * WAVE + lane;                         // column of [g_mu | g_lg]
    double s = 0.0;
    if (p < 2 * K)
        for (int row = slice; row < n_rows; row += RADIAL_SLICES) s += partial[(int64_t)row * 2 * K + p];
    sums[slice][lane] = s;
    __syncthreads();
    if (slice != 0 || p >= 2 * K) return;
    double total = 0.0;
    for (int w = 0; w < RADIAL_SLICES; ++w) total += sums[w][lane];
    if (p < K) {
        if (g_means) g_means[p] = (T)total;
    } else if (g_log_gammas) {
        g_log_gammas[p - K] = (T)total;
    }
}

// scatter-add of rows into segments (graph.py:304-316) on fp64 atomics: as the float32 kernel of egnn.hip, the order of the
// additions is not fixed
__global__ void segment_sum_f64_kernel(const double* __restrict__ data, const int64_t* __restrict__ ids, int64_t n_rows,
                                       int n_cols, int64_t n_segments, double* __restrict__ out) {
    const int64_t total = n_rows * n_cols;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / n_cols, seg = ids[row];
        if (seg >= 0 && seg < n_segments) unsafeAtomicAdd(out + seg * n_cols + (i % n_cols), data[i]);
    }
}

template <typename T>
__global__ void fill_zero_kernel(T* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = (T)0;
}

// VJP of the segment sum: row i of g_data is row ids[i] of g_out, zeros when the id names no segment.  V is the unit of
// one access: the element type, or 16 bytes when the row length and both pointers allow (then n_units counts 16-byte units).
template <typename V>
__global__ void segment_gather_kernel(const V* __restrict__ g_out, const int64_t* __restrict__ ids, int64_t n_rows,
                                      int n_units, int64_t n_segments, V* __restrict__ g_data) {
    const int64_t total = n_rows * n_units;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / n_units, seg = ids[row];
        V v = {};
        if (seg >= 0 && seg < n_segments) v = g_out[seg * n_units + (i % n_units)];
        g_data[i] = v;
    }
}

static inline unsigned graph_grid(int64_t n, int block) {
    const int64_t b = (n + block - 1) / block;
    return (unsigned)(b < 1 ? 1 : b > 2048 ? 2048 : b);            // the kernels stride over the rest
}

static int radial_check(const char* who, int64_t n, int K, int switching, double r_cutoff) {
    TFEP_REQUIRE(n >= 0 && K >= 1, "%s: bad sizes", who);
    TFEP_REQUIRE(n <= 0x7fffffffffffLL / K, "%s: n * n_basis too large", who);
    TFEP_REQUIRE(!switching || r_cutoff > 0.0, "%s: r_cutoff must be positive", who);
    return TFEP_OK;
}

template <typename T>
static int launch_radial_backward(const char* who, const T* r, int64_t n, const T* means, const T* log_gammas, int K,
                                  double r_cutoff, int switching, int force_zero, const T* g, T* g_r, T* g_means,
                                  T* g_log_gammas, double* workspace, void* stream) {
    if (int rc = radial_check(who, n, K, switching, r_cutoff)) return rc;
    const bool params = g_means || g_log_gammas;
    if (!params && (!g_r || n == 0)) return TFEP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        TFEP_REQUIRE(r && means && log_gammas && g, "%s: null tensor", who);
        TFEP_REQUIRE(!params || workspace, "%s: workspace is NULL", who);
        radial_backward_kernel<T><<<radial_blocks(n), RADIAL_WAVES * WAVE, 0, s>>>(
            r, n, means, log_gammas, K, r_cutoff, switching, force_zero, g, g_r, params ? workspace : nullptr);
        if (int rc = check_launch("radial_backward_kernel")) return rc;
    }
    if (!params) return TFEP_OK;
    radial_reduce_kernel<T><<<(2 * K + WAVE - 1) / WAVE, RADIAL_SLICES * WAVE, 0, s>>>(workspace, n > 0 ? radial_partials(n) : 0,
                                                                                      K, g_means, g_log_gammas);
    return check_launch("radial_reduce_kernel");
}

template <typename T>
static int launch_segment_gather(const char* who, const T* g_out, const int64_t* ids, int64_t n_rows, int n_cols,
                                 int64_t n_segments, T* g_data, void* stream) {
    TFEP_REQUIRE(n_rows >= 0 && n_cols >= 1 && n_segments >= 0, "%s: bad sizes", who);
    TFEP_REQUIRE(n_rows <= 0x7fffffffffffLL / n_cols, "%s: n_rows * n_cols too large", who);
    if (n_rows == 0) return TFEP_OK;
    TFEP_REQUIRE(ids && g_data && (g_out || n_segments == 0), "%s: null tensor", who);
    hipStream_t s = (hipStream_t)stream;
    constexpr int per = 16 / (int)sizeof(T);
    const bool wide = n_cols % per == 0 && (((uintptr_t)g_out | (uintptr_t)g_data) & 15) == 0;
    if (wide)
        segment_gather_kernel<float4><<<graph_grid(n_rows * (n_cols / per), 256), 256, 0, s>>>(
            (const float4*)g_out, ids, n_rows, n_cols / per, n_segments, (float4*)g_data);
    else
        segment_gather_kernel<T><<<graph_grid(n_rows * n_cols, 256), 256, 0, s>>>(g_out, ids, n_rows, n_cols, n_segments,
                                                                                 g_data);
    return check_launch("segment_gather_kernel");
}

}  // namespace tfep

using namespace tfep;

extern "C" {

int tfep_radial_expansion_f64(const double* r, int64_t n, const double* means, const double* log_gammas, int n_basis,
                              double r_cutoff, int switching, int force_zero_after_cutoff, double* out, void* stream) {
    if (int rc = radial_check("tfep_radial_expansion_f64", n, n_basis, switching, r_cutoff)) return rc;
    if (n == 0) return TFEP_OK;
    TFEP_REQUIRE(r && means && log_gammas && out, "tfep_radial_expansion_f64: null tensor");
    radial_forward_kernel<double><<<radial_blocks(n), RADIAL_WAVES * WAVE, 0, (hipStream_t)stream>>>(
        r, n, means, log_gammas, n_basis, r_cutoff, switching, force_zero_after_cutoff, out);
    return check_launch("tfep_radial_expansion_f64");
}

int64_t tfep_radial_expansion_backward_workspace_doubles(int64_t n, int n_basis) {
    if (n < 0 || n_basis < 1) return fail(TFEP_ERR_INVALID_ARGUMENT, "radial_expansion_backward_workspace_doubles: bad sizes");
    return (int64_t)radial_blocks(n) * RADIAL_WAVES * 2 * n_basis;
}

int tfep_radial_expansion_backward(const float* r, int64_t n, const float* means, const float* log_gammas, int n_basis,
                                   float r_cutoff, int switching, int force_zero_after_cutoff, const float* g, float* g_r,
                                   float* g_means, float* g_log_gammas, double* workspace, void* stream) {
    return launch_radial_backward<float>("tfep_radial_expansion_backward", r, n, means, log_gammas, n_basis, (double)r_cutoff,
                                         switching, force_zero_after_cutoff, g, g_r, g_means, g_log_gammas, workspace, stream);
}

int tfep_radial_expansion_backward_f64(const double* r, int64_t n, const double* means, const double* log_gammas, int n_basis,
                                       double r_cutoff, int switching, int force_zero_after_cutoff, const double* g,
                                       double* g_r, double* g_means, double* g_log_gammas, double* workspace, void* stream) {
    return launch_radial_backward<double>("tfep_radial_expansion_backward_f64", r, n, means, log_gammas, n_basis, r_cutoff,
                                          switching, force_zero_after_cutoff, g, g_r, g_means, g_log_gammas, workspace, stream);
}

int tfep_segment_sum_f64(const double* data, const int64_t* segment_ids, int64_t n_rows, int n_cols, int64_t n_segments,
                         double* out, void* stream) {
    TFEP_REQUIRE(n_rows >= 0 && n_cols >= 1 && n_segments >= 0, "tfep_segment_sum_f64: bad sizes");
    TFEP_REQUIRE(n_rows <= 0x7fffffffffffLL / n_cols && n_segments <= 0x7fffffffffffLL / n_cols,
                 "tfep_segment_sum_f64: sizes too large");
    if (n_segments == 0) return TFEP_OK;
    TFEP_REQUIRE(out != nullptr, "tfep_segment_sum_f64: null output");
    hipStream_t s = (hipStream_t)stream;
    fill_zero_kernel<double><<<graph_grid(n_segments * n_cols, 256), 256, 0, s>>>(out, n_segments * n_cols);
    if (n_rows == 0) return check_launch("tfep_segment_sum_f64");
    TFEP_REQUIRE(data && segment_ids, "tfep_segment_sum_f64: null tensor");
    segment_sum_f64_kernel<<<graph_grid(n_rows * n_cols, 256), 256, 0, s>>>(data, segment_ids, n_rows, n_cols, n_segments, out);
    return check_launch("tfep_segment_sum_f64");
}

int tfep_segment_gather(const float* g_out, const int64_t* segment_ids, int64_t n_rows, int n_cols, int64_t n_segments,
                        float* g_data, void* stream) {
    return launch_segment_gather<float>("tfep_segment_gather", g_out, segment_ids, n_rows, n_cols, n_segments, g_data, stream);
}

int tfep_segment_gather_f64(const double* g_out, const int64_t* segment_ids, int64_t n_rows, int n_cols, int64_t n_segments,
                            double* g_data, void* stream) {
    return launch_segment_gather<double>("tfep_segment_gather_f64", g_out, segment_ids, n_rows, n_cols, n_segments, g_data,
                                         stream);
}

}  // extern "C"
