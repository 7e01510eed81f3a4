// The head of a message-passing layer for callers that assemble their own graph networks on tfep.nn.graph (reference
// graph.py:222-301), float32 and float64 from one template:
//
//   edge geometry   v_e = x[edges[1][e]] - x[edges[0][e]] (the other way round with `inverse`), r_e = |v_e|; with `normalize`
//                   the directions are v_e / r_e.  One lane per edge, one launch.
//   its VJP         one lane per NODE over the node's incidence list (node_ptr, incident): the lane recomputes the forward
//                   of every incident edge and adds the contributions in list order.  No atomics.
//   pruning         ordered stream compaction of the edges with r_e <= r_cutoff: a count per tile of 256 edges, an
//                   exclusive scan of the counts, then a second pass that writes the kept edge ids in ascending order.
//
// Arithmetic is fp64 for both element types, one rounding on store; IEEE sqrt and division (the ops are bound by memory).
//
// Incidence list.  incident[node_ptr[n] .. node_ptr[n + 1]) holds the items 2 e + role of node n in ascending order: role 0
// when n is edges[0][e] (the source), role 1 when it is edges[1][e] (the destination).  Ascending items are ascending edges
// with the source entry first on a tie (a self-loop).  The order of a node's sum is therefore a function of its own edges
// alone: the gradient of a node has the same bits whatever else is in the batch.
//
// VJP of one edge.  With u = v / r, the cotangents g_r (of the distance) and g_d (of the direction):
//   plain        g_v = g_d + g_r u
//   normalized   g_v = (g_d - u (u . g_d)) / r + g_r u            -- (I - u u^T) / r applied to g_d
// and g_x[head] += g_v, g_x[tail] -= g_v, where v = x[head] - x[tail].  A NULL cotangent is a zero and goes through the same
// arithmetic.  r = 0 makes u = 0 / 0: NaN in g_x of the edge's two nodes, as autograd of sqrt at 0 gives.
//
// Indices are validated on the host (tfep_amd.ops.check_edges); the kernels still skip what is out of range instead of
// reading there (a forward edge with a bad index gets NaN).
#include "common.h"

namespace tfep {

constexpr int EDGE_BLOCK = 256;                // lanes per workgroup of the geometry kernels: one edge / one node each
constexpr int EDGE_MAX_BLOCKS = 2048;          // the kernels stride over the rest
constexpr int PRUNE_TILE = 256;                // edges per tile of the compaction = lanes per workgroup
constexpr int PRUNE_WAVES = PRUNE_TILE / WAVE;
constexpr int PRUNE_SCAN_LANES = 1024;         // the one workgroup that scans the tile counts
constexpr int64_t EDGE_MAX_EDGES = 0x1fffffffffffffffLL;      // 2 E + 1 items and 3 E direction elements fit in int64

static inline unsigned edge_grid(int64_t n, int block) {
    const int64_t b = (n + block - 1) / block;
    return (unsigned)(b < 1 ? 1 : b > EDGE_MAX_BLOCKS ? EDGE_MAX_BLOCKS : b);
}

static inline int64_t prune_tiles(int64_t E) { return (E + PRUNE_TILE - 1) / PRUNE_TILE; }

// v = x[head] - x[tail] and r = |v| in fp64
template <typename T>
__device__ inline void edge_vector(const T* __restrict__ x, int64_t ldx, int64_t head, int64_t tail, double v[3], double* r) {
    const T *h = x + head * ldx, *t = x + tail * ldx;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (double)h[c] - (double)t[c];
    *r = sqrt(fma(v[2], v[2], fma(v[1], v[1], v[0] * v[0])));
}

template <typename T>
__global__ void __launch_bounds__(EDGE_BLOCK) edge_geometry_kernel(const T* __restrict__ x, int64_t ldx,
                                                                   const int64_t* __restrict__ edges, int64_t N, int64_t E,
                                                                   int normalize, int inverse, T* __restrict__ distances,
                                                                   T* __restrict__ directions) {
    for (int64_t e = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x; e < E; e += (int64_t)gridDim.x * EDGE_BLOCK) {
        const int64_t src = edges[e], dst = edges[E + e];
        double v[3] = {NAN, NAN, NAN}, r = NAN;
        if (src >= 0 && src < N && dst >= 0 && dst < N) {
            edge_vector(x, ldx, inverse ? src : dst, inverse ? dst : src, v, &r);
            if (normalize) {
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] /= r;
            }
        }
        distances[e] = (T)r;
#pragma unroll
        for (int c = 0; c < 3; ++c) directions[3 * e + c] = (T)v[c];
    }
}

template <typename T>
__global__ void __launch_bounds__(EDGE_BLOCK) edge_geometry_backward_kernel(
    const T* __restrict__ x, int64_t ldx, const int64_t* __restrict__ edges, int64_t N, int64_t E,
    const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ incident, int normalize, int inverse,
    const T* __restrict__ g_distances, const T* __restrict__ g_directions, T* __restrict__ gx, int64_t ldgx) {
    for (int64_t n = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x; n < N; n += (int64_t)gridDim.x * EDGE_BLOCK) {
        int64_t p = node_ptr[n], p_end = node_ptr[n + 1];
        if (p < 0) p = 0;
        if (p_end > 2 * E) p_end = 2 * E;
        double acc[3] = {0.0, 0.0, 0.0};
        for (; p < p_end; ++p) {
            const int64_t item = incident[p], e = item >> 1;
            if (e < 0 || e >= E) continue;
            const int64_t src = edges[e], dst = edges[E + e];
            if (src < 0 || src >= N || dst < 0 || dst >= N) continue;
            const int64_t head = inverse ? src : dst, tail = inverse ? dst : src;
            double v[3], r, g_d[3], g_v[3];
            edge_vector(x, ldx, head, tail, v, &r);
            const double g_r = g_distances ? (double)g_distances[e] : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                g_d[c] = g_directions ? (double)g_directions[3 * e + c] : 0.0;
                v[c] /= r;                                          // u
            }
            if (normalize) {
                const double dot = fma(v[2], g_d[2], fma(v[1], g_d[1], v[0] * g_d[0]));
#pragma unroll
                for (int c = 0; c < 3; ++c) g_v[c] = (g_d[c] - v[c] * dot) / r + g_r * v[c];
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) g_v[c] = g_d[c] + g_r * v[c];
            }
            // role 1: this node is the edge's destination, which is the head unless the directions are inverted
            const bool is_head = ((item & 1) != 0) != (inverse != 0);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += is_head ? g_v[c] : -g_v[c];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) gx[n * ldgx + c] = (T)acc[c];
    }
}

template <typename T>
__global__ void __launch_bounds__(EDGE_BLOCK) edge_zero_rows_kernel(T* __restrict__ gx, int64_t ldgx, int64_t N) {
    for (int64_t i = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x; i < 3 * N; i += (int64_t)gridDim.x * EDGE_BLOCK)
        gx[(i / 3) * ldgx + i % 3] = (T)0;
}

// The position of this lane among the kept lanes of its workgroup, and the number of kept lanes (the same in every lane).
// Every lane of the workgroup calls it.  NaN <= r_cutoff is false: such an edge is dropped.
__device__ inline int prune_rank(bool keep, int* wave_counts, int* total) {
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) wave_counts[wave] = __popcll(kept);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < PRUNE_WAVES; ++w) {
        const int c = wave_counts[w];
        before += w < wave ? c : 0;
        all += c;
    }
    __syncthreads();                                                // (the next tile writes wave_counts again)
    *total = all;
    return before + __popcll(kept & ((1ull << lane) - 1ull));
}

// counts[t] = kept edges of tile t (the trip count of the loop is one per workgroup: the barriers are safe)
template <typename T>
__global__ void __launch_bounds__(PRUNE_TILE) edge_prune_count_kernel(const T* __restrict__ distances, int64_t E, T r_cutoff,
                                                                      int64_t* __restrict__ counts) {
    __shared__ int wave_counts[PRUNE_WAVES];
    const int64_t n_tiles = (E + PRUNE_TILE - 1) / PRUNE_TILE;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t e = t * PRUNE_TILE + threadIdx.x;
        int total;
        prune_rank(e < E && distances[e] <= r_cutoff, wave_counts, &total);
        if (threadIdx.x == 0) counts[t] = total;
    }
}

// In place: counts[0 .. n) become their exclusive prefix sums and counts[n] the total.  One workgroup; lane l owns the
// entries [l chunk, (l + 1) chunk).
__global__ void __launch_bounds__(PRUNE_SCAN_LANES) edge_prune_scan_kernel(int64_t* __restrict__ counts, int64_t n) {
    __shared__ int64_t wave_totals[PRUNE_SCAN_LANES / WAVE];
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    const int64_t chunk = (n + PRUNE_SCAN_LANES - 1) / PRUNE_SCAN_LANES;
    const int64_t first = threadIdx.x * chunk, last = first + chunk < n ? first + chunk : n;
    int64_t mine = 0;
    for (int64_t i = first; i < last; ++i) mine += counts[i];
    int64_t upto = mine;                                            // inclusive scan over the lanes of the wave
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int64_t o = __shfl_up(upto, off, WAVE);
        if (lane >= off) upto += o;
    }
    if (lane == WAVE - 1) wave_totals[wave] = upto;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int w = 0; w < PRUNE_SCAN_LANES / WAVE; ++w) {
        const int64_t c = wave_totals[w];
        before += w < wave ? c : 0;
        all += c;
    }
    int64_t running = before + upto - mine;
    for (int64_t i = first; i < last; ++i) {
        const int64_t c = counts[i];
        counts[i] = running;
        running += c;
    }
    if (threadIdx.x == 0) counts[n] = all;
}

template <typename T>
__global__ void __launch_bounds__(PRUNE_TILE) edge_prune_compact_kernel(const T* __restrict__ distances, int64_t E, T r_cutoff,
                                                                        const int64_t* __restrict__ offsets,
                                                                        int64_t* __restrict__ keep_index, int64_t n_kept) {
    __shared__ int wave_counts[PRUNE_WAVES];
    const int64_t n_tiles = (E + PRUNE_TILE - 1) / PRUNE_TILE;
    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const int64_t e = t * PRUNE_TILE + threadIdx.x;
        const bool keep = e < E && distances[e] <= r_cutoff;
        int total;
        const int64_t at = offsets[t] + prune_rank(keep, wave_counts, &total);
        if (keep && at >= 0 && at < n_kept) keep_index[at] = e;
    }
}

// out[row, i] = edges[row, keep_index[i]], row = 0, 1 (-1 where keep_index names no edge)
__global__ void __launch_bounds__(EDGE_BLOCK) edge_select_edges_kernel(const int64_t* __restrict__ edges, int64_t E,
                                                                       const int64_t* __restrict__ keep_index, int64_t n_kept,
                                                                       int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * EDGE_BLOCK + threadIdx.x; i < 2 * n_kept; i += (int64_t)gridDim.x * EDGE_BLOCK) {
        const int64_t row = i / n_kept, k = keep_index[i - row * n_kept];
        out[i] = k >= 0 && k < E ? edges[row * E + k] : -1;
    }
}

static int edge_sizes_check(const char* who, int64_t N, int64_t E) {
    TFEP_REQUIRE(N >= 0 && E >= 0, "%s: negative size", who);
    TFEP_REQUIRE(E <= EDGE_MAX_EDGES && N <= EDGE_MAX_EDGES, "%s: too many edges or nodes", who);
    return TFEP_OK;
}

template <typename T>
static int launch_edge_geometry(const char* who, const T* x, int64_t ldx, const int64_t* edges, int64_t N, int64_t E,
                                int normalize, int inverse, T* distances, T* directions, void* stream) {
    if (int rc = edge_sizes_check(who, N, E)) return rc;
    if (E == 0) return TFEP_OK;
    TFEP_REQUIRE(N > 0, "%s: edges without nodes", who);
    TFEP_REQUIRE(x && edges && distances && directions, "%s: null tensor", who);
    TFEP_REQUIRE(ldx >= 3, "%s: a row of x holds 3 coordinates, the row stride is %lld", who, (long long)ldx);
    edge_geometry_kernel<T><<<edge_grid(E, EDGE_BLOCK), EDGE_BLOCK, 0, (hipStream_t)stream>>>(x, ldx, edges, N, E, normalize,
                                                                                             inverse, distances, directions);
    return check_launch(who);
}

template <typename T>
static int launch_edge_geometry_backward(const char* who, const T* x, int64_t ldx, const int64_t* edges, int64_t N, int64_t E,
                                         const int64_t* node_ptr, const int64_t* incident, int normalize, int inverse,
                                         const T* g_distances, const T* g_directions, T* gx, int64_t ldgx, void* stream) {
    if (int rc = edge_sizes_check(who, N, E)) return rc;
    if (N == 0) return TFEP_OK;
    TFEP_REQUIRE(gx != nullptr, "%s: null output", who);
    TFEP_REQUIRE(ldgx >= 3, "%s: a row of gx holds 3 coordinates, the row stride is %lld", who, (long long)ldgx);
    hipStream_t s = (hipStream_t)stream;
    if (E == 0) {                                                   // no edge: every node's gradient is zero
        edge_zero_rows_kernel<T><<<edge_grid(3 * N, EDGE_BLOCK), EDGE_BLOCK, 0, s>>>(gx, ldgx, N);
        return check_launch(who);
    }
    TFEP_REQUIRE(x && edges && node_ptr && incident, "%s: null tensor", who);
    TFEP_REQUIRE(ldx >= 3, "%s: a row of x holds 3 coordinates, the row stride is %lld", who, (long long)ldx);
    edge_geometry_backward_kernel<T><<<edge_grid(N, EDGE_BLOCK), EDGE_BLOCK, 0, s>>>(
        x, ldx, edges, N, E, node_ptr, incident, normalize, inverse, g_distances, g_directions, gx, ldgx);
    return check_launch(who);
}

template <typename T>
static int launch_edge_prune_count(const char* who, const T* distances, int64_t E, T r_cutoff, int64_t* workspace,
                                   void* stream) {
    if (int rc = edge_sizes_check(who, 0, E)) return rc;
    TFEP_REQUIRE(workspace != nullptr, "%s: workspace is NULL", who);
    hipStream_t s = (hipStream_t)stream;
    const int64_t n_tiles = prune_tiles(E);
    if (E > 0) {
        TFEP_REQUIRE(distances != nullptr, "%s: null tensor", who);
        edge_prune_count_kernel<T><<<edge_grid(E, PRUNE_TILE), PRUNE_TILE, 0, s>>>(distances, E, r_cutoff, workspace);
        if (int rc = check_launch(who)) return rc;
    }
    edge_prune_scan_kernel<<<1, PRUNE_SCAN_LANES, 0, s>>>(workspace, n_tiles);      // (E = 0: writes the total, 0)
    return check_launch(who);
}

template <typename T>
static int launch_edge_prune_compact(const char* who, const T* distances, int64_t E, T r_cutoff, const int64_t* workspace,
                                     int64_t* keep_index, int64_t n_kept, void* stream) {
    if (int rc = edge_sizes_check(who, 0, E)) return rc;
    TFEP_REQUIRE(n_kept >= 0 && n_kept <= E, "%s: n_kept must be in [0, n_edges]", who);
    if (E == 0 || n_kept == 0) return TFEP_OK;
    TFEP_REQUIRE(distances && workspace && keep_index, "%s: null tensor", who);
    edge_prune_compact_kernel<T><<<edge_grid(E, PRUNE_TILE), PRUNE_TILE, 0, (hipStream_t)stream>>>(distances, E, r_cutoff,
                                                                                                  workspace, keep_index, n_kept);
    return check_launch(who);
}

}  // namespace tfep

using namespace tfep;

extern "C" {

int tfep_edge_geometry(const float* x, int64_t ldx, const int64_t* edges, int64_t n_nodes, int64_t n_edges, int normalize,
                       int inverse, float* distances, float* directions, void* stream) {
    return launch_edge_geometry<float>("tfep_edge_geometry", x, ldx, edges, n_nodes, n_edges, normalize, inverse, distances,
                                       directions, stream);
}

int tfep_edge_geometry_f64(const double* x, int64_t ldx, const int64_t* edges, int64_t n_nodes, int64_t n_edges, int normalize,
                           int inverse, double* distances, double* directions, void* stream) {
    return launch_edge_geometry<double>("tfep_edge_geometry_f64", x, ldx, edges, n_nodes, n_edges, normalize, inverse, distances,
                                        directions, stream);
}

int tfep_edge_geometry_backward(const float* x, int64_t ldx, const int64_t* edges, int64_t n_nodes, int64_t n_edges,
                                const int64_t* node_ptr, const int64_t* incident, int normalize, int inverse,
                                const float* g_distances, const float* g_directions, float* gx, int64_t ldgx, void* stream) {
    return launch_edge_geometry_backward<float>("tfep_edge_geometry_backward", x, ldx, edges, n_nodes, n_edges, node_ptr, incident,
                                                normalize, inverse, g_distances, g_directions, gx, ldgx, stream);
}

int tfep_edge_geometry_backward_f64(const double* x, int64_t ldx, const int64_t* edges, int64_t n_nodes, int64_t n_edges,
                                    const int64_t* node_ptr, const int64_t* incident, int normalize, int inverse,
                                    const double* g_distances, const double* g_directions, double* gx, int64_t ldgx,
                                    void* stream) {
    return launch_edge_geometry_backward<double>("tfep_edge_geometry_backward_f64", x, ldx, edges, n_nodes, n_edges, node_ptr,
                                                 incident, normalize, inverse, g_distances, g_directions, gx, ldgx, stream);
}

int64_t tfep_edge_prune_workspace_int64s(int64_t n_edges) {
    if (n_edges < 0 || n_edges > EDGE_MAX_EDGES) return fail(TFEP_ERR_INVALID_ARGUMENT, "edge_prune_workspace_int64s: bad size");
    return prune_tiles(n_edges) + 1;
}

int tfep_edge_prune_count(const float* distances, int64_t n_edges, float r_cutoff, int64_t* workspace, void* stream) {
    return launch_edge_prune_count<float>("tfep_edge_prune_count", distances, n_edges, r_cutoff, workspace, stream);
}

int tfep_edge_prune_count_f64(const double* distances, int64_t n_edges, double r_cutoff, int64_t* workspace, void* stream) {
    return launch_edge_prune_count<double>("tfep_edge_prune_count_f64", distances, n_edges, r_cutoff, workspace, stream);
}

int tfep_edge_prune_compact(const float* distances, int64_t n_edges, float r_cutoff, const int64_t* workspace,
                            int64_t* keep_index, int64_t n_kept, void* stream) {
    return launch_edge_prune_compact<float>("tfep_edge_prune_compact", distances, n_edges, r_cutoff, workspace, keep_index, n_kept,
                                            stream);
}

int tfep_edge_prune_compact_f64(const double* distances, int64_t n_edges, double r_cutoff, const int64_t* workspace,
                                int64_t* keep_index, int64_t n_kept, void* stream) {
    return launch_edge_prune_compact<double>("tfep_edge_prune_compact_f64", distances, n_edges, r_cutoff, workspace, keep_index,
                                             n_kept, stream);
}

int tfep_edge_select_edges(const int64_t* edges, int64_t n_edges, const int64_t* keep_index, int64_t n_kept, int64_t* out,
                           void* stream) {
    if (int rc = edge_sizes_check("tfep_edge_select_edges", 0, n_edges)) return rc;
    TFEP_REQUIRE(n_kept >= 0 && n_kept <= EDGE_MAX_EDGES, "tfep_edge_select_edges: bad n_kept");
    if (n_kept == 0) return TFEP_OK;
    TFEP_REQUIRE(keep_index && out && (edges || n_edges == 0), "tfep_edge_select_edges: null tensor");
    edge_select_edges_kernel<<<edge_grid(2 * n_kept, EDGE_BLOCK), EDGE_BLOCK, 0, (hipStream_t)stream>>>(edges, n_edges, keep_index,
                                                                                                     n_kept, out);
    return check_launch("tfep_edge_select_edges");
}

}  // extern "C"
