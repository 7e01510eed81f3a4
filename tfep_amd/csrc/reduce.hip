// TFEP loss / free-energy estimator sufficient statistics (reference loss.py:125-140,
// analysis/estimator.py:73-86).  One pass over the local shard; the 9 fp64 statistics are what
// the multi-GPU path all-reduces (max + rescaled sums) -- see tfep_hip.h.
//
// Two kernels: per-block partials (online max / rescaled-sum, fp64) then a single-block
// combine.  No atomics -> bit-reproducible for a fixed N.
#include "common.h"
#include "bootstrap_rng.h"

namespace tfep {

struct Stats {
    double count, sum_r;
    double m_w, s_w, s_wr;
    double m_e, s_e;
    double m_b, s_b;
};

// exp(a - b) for a <= b, with 1 where the two are equal: two +inf count one each, as in torch.logsumexp, where
// exp(inf - inf) would be NaN.  For finite a == b this is exp(0) = 1 either way.
__device__ inline double rescale(double a, double b) { return a == b ? 1.0 : exp(a - b); }

__device__ inline void online_add(double& m, double& s, double v) {
    // s = sum exp(v_i - m), m = running max.  -inf values contribute nothing.
    if (v == -INFINITY) return;
    if (v > m) {
        s = s * exp(m - v) + 1.0;
        m = v;
    } else {
        s += rescale(v, m);
    }
}

// The weight pair keeps exp(m - m): a +inf log-weight makes the sums NaN, as torch.softmax does (its own term too,
// so that a thread or a batch that holds nothing else says the same).
__device__ inline void online_add2(double& m, double& s, double& sr, double v, double r) {
    if (v == -INFINITY) return;
    if (v > m) {
        const double c = exp(m - v);
        s = s * c + 1.0;
        sr = sr * c + r;
        m = v;
        if (v == INFINITY) s = sr = NAN;
    } else {
        const double e = exp(v - m);
        s += e;
        sr += e * r;
    }
}

__device__ inline void combine(double& m, double& s, double m2, double s2) {
    if (m2 == -INFINITY) return;
    if (m == -INFINITY) {
        m = m2;
        s = s2;
        return;
    }
    const double mm = fmax(m, m2);
    s = s * rescale(m, mm) + s2 * rescale(m2, mm);
    m = mm;
}

__device__ inline void combine2(double& m, double& s, double& sr, double m2, double s2, double sr2) {
    if (m2 == -INFINITY) return;
    if (m == -INFINITY) {
        m = m2;
        s = s2;
        sr = sr2;
        return;
    }
    const double mm = fmax(m, m2);
    const double c1 = exp(m - mm), c2 = exp(m2 - mm);
    s = s * c1 + s2 * c2;
    sr = sr * c1 + sr2 * c2;
    m = mm;
}

__device__ inline Stats stats_identity() {
    Stats s;
    s.count = 0.0;
    s.sum_r = 0.0;
    s.m_w = -INFINITY;
    s.s_w = 0.0;
    s.s_wr = 0.0;
    s.m_e = -INFINITY;
    s.s_e = 0.0;
    s.m_b = -INFINITY;
    s.s_b = 0.0;
    return s;
}

__device__ inline void stats_merge(Stats& a, const Stats& b) {
    a.count += b.count;
    a.sum_r += b.sum_r;
    combine2(a.m_w, a.s_w, a.s_wr, b.m_w, b.s_w, b.s_wr);
    combine(a.m_e, a.s_e, b.m_e, b.s_e);
    combine(a.m_b, a.s_b, b.m_b, b.s_b);
}

__device__ inline Stats stats_shfl_xor(const Stats& s, int off) {
    Stats o;
    o.count = __shfl_xor(s.count, off, 64);
    o.sum_r = __shfl_xor(s.sum_r, off, 64);
    o.m_w = __shfl_xor(s.m_w, off, 64);
    o.s_w = __shfl_xor(s.s_w, off, 64);
    o.s_wr = __shfl_xor(s.s_wr, off, 64);
    o.m_e = __shfl_xor(s.m_e, off, 64);
    o.s_e = __shfl_xor(s.s_e, off, 64);
    o.m_b = __shfl_xor(s.m_b, off, 64);
    o.s_b = __shfl_xor(s.s_b, off, 64);
    return o;
}

__device__ inline void block_reduce_and_store(Stats st, double* out) {
    __shared__ Stats sh[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        Stats o = stats_shfl_xor(st, off);
        stats_merge(st, o);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) sh[wave] = st;
    __syncthreads();
    if (threadIdx.x == 0) {
        Stats t = sh[0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) stats_merge(t, sh[w]);
        out[0] = t.count;
        out[1] = t.sum_r;
        out[2] = t.m_w;
        out[3] = t.s_w;
        out[4] = t.s_wr;
        out[5] = t.m_e;
        out[6] = t.s_e;
        out[7] = t.m_b;
        out[8] = t.s_b;
    }
}

// T = float: r in float32 arithmetic, like the reference's float32 tensors; T = double: float64 flows (r in fp64).
template <typename T>
__global__ void __launch_bounds__(256) tfep_reduce_partial_kernel(const T* __restrict__ uB,
                                                                  const T* __restrict__ ldj,
                                                                  const T* __restrict__ uA,
                                                                  const T* __restrict__ lw,
                                                                  const T* __restrict__ bias, double inv_kT,
                                                                  int ignore_nan, int N, double* __restrict__ partial) {
    Stats st = stats_identity();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        // arithmetic for r in the type of the inputs, like the reference tensors (loss.py:125-129)
        T rf = uB[i];
        if (ldj) rf = rf - ldj[i];
        if (uA) rf = rf - uA[i];
        const double r = (double)rf;
        const bool isn = isnan(rf);
        if (!(ignore_nan && isn)) {
            st.count += 1.0;
            st.sum_r += r;
        }
        if (lw) {
            // softmax over the whole batch (loss.py:133); NaN r skipped by nansum when ignore_nan
            // an ignored sample adds 0 to s_wr through the same pair: a new maximum has to rescale s_wr as well
            const double v = (double)lw[i];
            online_add2(st.m_w, st.s_w, st.s_wr, v, (ignore_nan && isn) ? 0.0 : r);
        }
        double e = -r * inv_kT;
        if (bias) {
            const double bb = (double)bias[i] * inv_kT;
            online_add(st.m_b, st.s_b, bb);
            e += bb;
        }
        if (isn) {
            st.m_e = NAN;      // logsumexp propagates NaN (estimator.py:86)
        } else if (!isnan(st.m_e)) {
            online_add(st.m_e, st.s_e, e);
        }
    }
    block_reduce_and_store(st, partial + (int64_t)blockIdx.x * 9);
}

__global__ void __launch_bounds__(256) tfep_reduce_final_kernel(const double* __restrict__ partial, int n_partial,
                                                                double* __restrict__ out) {
    Stats st = stats_identity();
    for (int i = threadIdx.x; i < n_partial; i += blockDim.x) {
        Stats o;
        const double* p = partial + (int64_t)i * 9;
        o.count = p[0];
        o.sum_r = p[1];
        o.m_w = p[2];
        o.s_w = p[3];
        o.s_wr = p[4];
        o.m_e = p[5];
        o.s_e = p[6];
        o.m_b = p[7];
        o.s_b = p[8];
        stats_merge(st, o);
    }
    block_reduce_and_store(st, out);
}


// ------------------------------------------------------------------------------------------
// Bootstrap of the FEP estimator (reference analysis/bootstrap.py:185-262 with statistic = fep_estimator):
// one workgroup per resample; the resampled data are never materialised.
//   standard:  a_j = -work[idx[r][j]] / kT (+ bias[idx[r][j]] / kT),
//              dF_r = -kT (logsumexp_j a_j - log S)                     (no bias)
//              dF_r = -kT (logsumexp_j a_j - logsumexp_j bias_j / kT)   (bias: log_softmax of the resampled biases)
//   Bayesian:  idx == NULL, weights (R, S) >= 0 summing to 1:  dF_r = -kT logsumexp_j (-work[j]/kT + log weights[r][j])
// Online (max, rescaled sum) in fp64 per thread, merged across the workgroup.
// ------------------------------------------------------------------------------------------
struct MaxSum {
    double m, s;
};
__device__ inline void ms_add(MaxSum& a, double v) {
    if (v == -INFINITY) return;
    if (v <= a.m) {
        a.s += rescale(v, a.m);
    } else {
        a.s = a.s * exp(a.m - v) + 1.0;
        a.m = v;
    }
}
__device__ inline MaxSum ms_merge(MaxSum a, MaxSum b) {
    if (b.s == 0.0) return a;
    if (a.s == 0.0) return b;
    MaxSum r;
    r.m = fmax(a.m, b.m);
    r.s = a.s * rescale(a.m, r.m) + b.s * rescale(b.m, r.m);
    return r;
}
__device__ inline MaxSum ms_block_reduce(MaxSum v, MaxSum* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        MaxSum o;
        o.m = __shfl_xor(v.m, off, 64);
        o.s = __shfl_xor(v.s, off, 64);
        v = ms_merge(v, o);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    MaxSum r = sh[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r = ms_merge(r, sh[w]);
    __syncthreads();
    return r;
}

// T = float: the float32 data of the reference's default dtype; T = double: float64 work values, biases and weights.
template <typename T>
__global__ void __launch_bounds__(256) bootstrap_fep_kernel(const T* __restrict__ work, const T* __restrict__ bias,
                                                            const int64_t* __restrict__ idx, const T* __restrict__ weights,
                                                            int64_t n_data, int64_t S, double inv_kT, double kT,
                                                            double* __restrict__ out) {
    __shared__ MaxSum sh[4];
    const int64_t r = blockIdx.x;
    MaxSum a = {-INFINITY, 0.0}, b = {-INFINITY, 0.0};
    for (int64_t j = threadIdx.x; j < S; j += blockDim.x) {
        const int64_t i = idx ? idx[r * S + j] : j;
        if (i < 0 || i >= n_data) continue;                       // never for torch.randint(0, n_data) indices
        double v = -(double)work[i] * inv_kT;
        if (weights) v += log((double)weights[r * S + j]);
        if (bias) {
            const double bb = (double)bias[i] * inv_kT;
            v += bb;
            ms_add(b, bb);
        }
        ms_add(a, v);
    }
    a = ms_block_reduce(a, sh);
    if (bias) b = ms_block_reduce(b, sh);
    if (threadIdx.x == 0) {
        double lse = a.m + log(a.s);
        if (bias)
            lse -= b.m + log(b.s);
        else if (!weights)
            lse -= log((double)S);
        out[r] = -kT * lse;
    }
}

// The loop of bootstrap_fep_kernel with the item of draw j named by item(j, i, lw) instead of read from memory: i is the
// data item and, where item returns true, lw the log-weight of the draw.  The resampling kernel below replays a resample
// through it, item j on thread j % 256 as above, so that a replayed resample is what the explicit kernel gives on the same
// draws.  (The explicit kernel keeps its own loop: its float32 code stays what it was, instruction for instruction.)
template <typename T, typename Item>
__device__ inline void replay_online(const T* __restrict__ work, const T* __restrict__ bias, int64_t n_data, int64_t S,
                                     double inv_kT, Item item, MaxSum& a, MaxSum& b) {
    for (int64_t j = threadIdx.x; j < S; j += blockDim.x) {
        int64_t i;
        double lw = 0.0;
        const bool weighted = item(j, i, lw);
        if (i < 0 || i >= n_data) continue;
        double v = -(double)work[i] * inv_kT;
        if (weighted) v += lw;
        if (bias) {
            const double bb = (double)bias[i] * inv_kT;
            v += bb;
            ms_add(b, bb);
        }
        ms_add(a, v);
    }
}

// ------------------------------------------------------------------------------------------
// The same bootstrap with the resamples drawn in the kernel (bootstrap_rng.h) from a table of exponentials:
//   t_i = exp(a_i - M),  a_i = -work_i / kT (+ bias_i / kT),  M = max_i a_i;   u_i = exp(b_i - M_b),  b_i = bias_i / kT
// so that a resample is a gather and a sum, sum_j exp(a_{i_j}) = exp(M) sum_j t_{i_j}.  Only n distinct exponentials
// exist, whatever the number of resamples.  The table is built by two launches: per-workgroup maxima (and a flag for a NaN
// or +inf item, for which no table exists), then the table itself, each workgroup taking the maximum of the partial
// maxima on its own -- a maximum does not depend on the order, so no atomics and no third launch.
// ------------------------------------------------------------------------------------------
constexpr int TABLE_MAX_BLOCKS = 1024;

// maxima of three values over the workgroup, on every thread
__device__ inline void block_max3(double& x, double& y, double& z, double (*sh)[4]) {
    x = wave_max(x);
    y = wave_max(y);
    z = wave_max(z);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        sh[0][wave] = x;
        sh[1][wave] = y;
        sh[2][wave] = z;
    }
    __syncthreads();
    x = fmax(fmax(sh[0][0], sh[0][1]), fmax(sh[0][2], sh[0][3]));
    y = fmax(fmax(sh[1][0], sh[1][1]), fmax(sh[1][2], sh[1][3]));
    z = fmax(fmax(sh[2][0], sh[2][1]), fmax(sh[2][2], sh[2][3]));
    __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(256) bootstrap_table_max_kernel(const T* __restrict__ work, const T* __restrict__ bias,
                                                                  int64_t n, double inv_kT, double* __restrict__ partial) {
    __shared__ double sh[3][4];
    double ma = -INFINITY, mb = -INFINITY, bad = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double a = -(double)work[i] * inv_kT;
        if (bias) {
            const double bb = (double)bias[i] * inv_kT;
            a += bb;
            if (!(bb < INFINITY)) bad = 1.0;                     // NaN or +inf
            mb = fmax(mb, bb);
        }
        if (!(a < INFINITY)) bad = 1.0;
        ma = fmax(ma, a);
    }
    block_max3(ma, mb, bad, sh);
    if (threadIdx.x == 0) {
        partial[3 * blockIdx.x + 0] = ma;
        partial[3 * blockIdx.x + 1] = mb;
        partial[3 * blockIdx.x + 2] = bad;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) bootstrap_table_fill_kernel(const T* __restrict__ work, const T* __restrict__ bias,
                                                                   int64_t n, double inv_kT,
                                                                   const double* __restrict__ partial, int n_partial,
                                                                   double* __restrict__ table, double* __restrict__ stats,
                                                                   int* __restrict__ flag) {
    __shared__ double sh[3][4];
    double ma = -INFINITY, mb = -INFINITY, bad = 0.0;
    for (int p = threadIdx.x; p < n_partial; p += blockDim.x) {
        ma = fmax(ma, partial[3 * p + 0]);
        mb = fmax(mb, partial[3 * p + 1]);
        bad = fmax(bad, partial[3 * p + 2]);
    }
    block_max3(ma, mb, bad, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[0] = ma;
        stats[1] = mb;
        *flag = bad != 0.0;
    }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double a = -(double)work[i] * inv_kT;
        if (bias) {
            const double bb = (double)bias[i] * inv_kT;
            a += bb;
            table[n + i] = exp(bb - mb);
        }
        table[i] = exp(a - ma);                                  // NaN where every item is -inf: the resample is replayed
    }
}

// sum over the workgroup in a fixed order, on every thread
__device__ inline double block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    const double total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return total;
}

// visit(j, E_j) for every draw of the Bayesian stream: thread q % 256 takes group q, that is draws 2q and 2q + 1
template <typename Visit>
__device__ inline void for_each_exponential(const BootstrapStream& stream, int64_t S, Visit visit) {
    for (int64_t q = threadIdx.x; 2 * q < S; q += blockDim.x) {
        uint32_t w[4];
        bootstrap_words(stream, q, w);
        visit(2 * q, bootstrap_exponential(w[0], w[1]));
        if (2 * q + 1 < S) visit(2 * q + 1, bootstrap_exponential(w[2], w[3]));
    }
}

// One workgroup per resample r = offset + blockIdx.x.
//   standard:  dF_r = -kT (M + log sum_j t[i_j] - log S)          or, with a bias,
//              dF_r = -kT ((M + log sum_j t[i_j]) - (M_b + log sum_j u[i_j]))
//   Bayesian:  dF_r = -kT (M + log sum_j E_j t[j] - log sum_j E_j)           (S == high == n_data, no bias)
// A sum below 2^-1000 (or NaN), or a set flag, sends the whole workgroup to the replay: the same draws through
// replay_online on the data themselves.  Above 2^-1000 a term that left the normal range is off by at most 2^-1075, all S
// < 2^31 of them by 2^-1044 together: 2^-44 of the sum.
template <typename T>
__global__ void __launch_bounds__(256) bootstrap_fep_resampled_kernel(
        const T* __restrict__ work, const T* __restrict__ bias, const double* __restrict__ table,
        const double* __restrict__ stats, const int* __restrict__ flag, int64_t n_data, int64_t S, uint32_t high,
        int64_t seed, int64_t offset, int bayesian, double inv_kT, double kT, double* __restrict__ out) {
    __shared__ MaxSum sh[4];
    __shared__ double sh_sum[4];
    const int64_t r = offset + blockIdx.x;
    const BootstrapStream stream = bootstrap_stream(seed, r, bayesian ? BOOTSTRAP_STREAM_WEIGHTS : BOOTSTRAP_STREAM_INDICES);
    const double* __restrict__ u = table + n_data;
    double sa = 0.0, sb = 0.0;                                    // sum of t (times E); sum of u, or of E
    if (bayesian) {
        for_each_exponential(stream, S, [&](int64_t j, double e) {
            sa += e * table[j];
            sb += e;
        });
    } else {
        for (int64_t q = threadIdx.x; 4 * q < S; q += blockDim.x) {
            uint32_t w[4];
            bootstrap_words(stream, q, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (4 * q + k < S) {
                    const int64_t i = bootstrap_index(w[k], high);
                    sa += table[i];
                    if (bias) sb += u[i];
                }
            }
        }
    }
    sa = block_sum(sa, sh_sum);
    if (bias || bayesian) sb = block_sum(sb, sh_sum);
    constexpr double TINY = 0x1p-1000;
    const bool replay = *flag != 0 || !(sa >= TINY) || (bias && !(sb >= TINY));      // the same on every thread
    double lse;
    if (!replay) {
        lse = stats[0] + log(sa);
        if (bias) lse -= stats[1] + log(sb);
    } else {
        MaxSum a = {-INFINITY, 0.0}, b = {-INFINITY, 0.0};
        if (bayesian)
            replay_online(work, bias, n_data, S, inv_kT, [&](int64_t j, int64_t& i, double& lw) {
                i = j;
                lw = log(bootstrap_exponential_at(stream, j));
                return true;
            }, a, b);
        else
            replay_online(work, bias, n_data, S, inv_kT, [&](int64_t j, int64_t& i, double&) {
                i = bootstrap_index_at(stream, j, high);
                return false;
            }, a, b);
        a = ms_block_reduce(a, sh);
        lse = a.m + log(a.s);
        if (bias) {
            b = ms_block_reduce(b, sh);
            lse -= b.m + log(b.s);
        }
    }
    if (threadIdx.x == 0) {
        if (!bias) lse -= log(bayesian ? sb : (double)S);
        out[blockIdx.x] = -kT * lse;
    }
}

// The resamples themselves, for the explicit kernel and for users: one workgroup per row.
__global__ void __launch_bounds__(256) bootstrap_resample_indices_kernel(int64_t S, uint32_t high, int64_t seed,
                                                                        int64_t offset, int64_t* __restrict__ out) {
    const BootstrapStream stream = bootstrap_stream(seed, offset + blockIdx.x, BOOTSTRAP_STREAM_INDICES);
    int64_t* __restrict__ row = out + (int64_t)blockIdx.x * S;
    for (int64_t q = threadIdx.x; 4 * q < S; q += blockDim.x) {
        uint32_t w[4];
        bootstrap_words(stream, q, w);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * q + k < S) row[4 * q + k] = bootstrap_index(w[k], high);
    }
}

__global__ void __launch_bounds__(256) bootstrap_resample_weights_kernel(int64_t S, int64_t seed, int64_t offset,
                                                                        double* __restrict__ out) {
    __shared__ double sh_sum[4];
    const BootstrapStream stream = bootstrap_stream(seed, offset + blockIdx.x, BOOTSTRAP_STREAM_WEIGHTS);
    double* __restrict__ row = out + (int64_t)blockIdx.x * S;
    double total = 0.0;
    for_each_exponential(stream, S, [&](int64_t, double e) { total += e; });
    total = block_sum(total, sh_sum);
    for_each_exponential(stream, S, [&](int64_t j, double e) { row[j] = e / total; });
}

inline int table_blocks(int64_t n) {
    const int64_t blocks = (n + 255) / 256;
    return blocks > TABLE_MAX_BLOCKS ? TABLE_MAX_BLOCKS : (int)blocks;
}

template <typename T>
int bootstrap_fep_launch(const T* work, const T* bias, const int64_t* indices, const T* weights, int64_t n_data,
                         int64_t n_resamples, int64_t sample_size, T kT, double* out, void* stream) {
    TFEP_REQUIRE(n_resamples >= 0 && sample_size >= 0 && n_data >= 0, "bootstrap_fep: negative size");
    if (n_resamples == 0) return TFEP_OK;
    TFEP_REQUIRE(work && out, "bootstrap_fep: NULL pointer");
    TFEP_REQUIRE(kT > (T)0, "bootstrap_fep: kT must be positive");
    TFEP_REQUIRE(indices || sample_size <= n_data, "bootstrap_fep: without indices sample_size must be <= n_data");
    TFEP_REQUIRE(!(bias && weights), "bootstrap_fep: Bayesian weights are not supported with biased data");
    TFEP_REQUIRE(n_resamples <= 0x7fffffffLL, "bootstrap_fep: too many resamples");
    bootstrap_fep_kernel<T><<<(unsigned)n_resamples, 256, 0, (hipStream_t)stream>>>(
        work, bias, indices, weights, n_data, sample_size, 1.0 / (double)kT, (double)kT, out);
    return check_launch("bootstrap_fep_kernel");
}

template <typename T>
int bootstrap_table_launch(const T* work, const T* bias, int64_t n, T kT, double* table, double* stats, int* flag,
                           double* workspace, void* stream) {
    TFEP_REQUIRE(n >= 1, "bootstrap_table: needs at least one item");
    TFEP_REQUIRE(work && table && stats && flag && workspace, "bootstrap_table: NULL pointer");
    TFEP_REQUIRE(kT > (T)0, "bootstrap_table: kT must be positive");
    const int blocks = table_blocks(n);
    hipStream_t s = (hipStream_t)stream;
    bootstrap_table_max_kernel<T><<<blocks, 256, 0, s>>>(work, bias, n, 1.0 / (double)kT, workspace);
    bootstrap_table_fill_kernel<T><<<blocks, 256, 0, s>>>(work, bias, n, 1.0 / (double)kT, workspace, blocks, table, stats,
                                                          flag);
    return check_launch("bootstrap_table");
}

// the checks that the stream definition needs, shared by the three entry points that draw from it
inline int bootstrap_stream_check(int64_t n_resamples, int64_t sample_size, int64_t seed, int64_t offset) {
    TFEP_REQUIRE(n_resamples >= 0 && sample_size >= 1, "bootstrap stream: n_resamples >= 0 and sample_size >= 1");
    TFEP_REQUIRE(seed >= 0, "bootstrap stream: the seed must be in [0, 2^63)");
    TFEP_REQUIRE(offset >= 0 && offset <= 0x80000000LL && n_resamples <= 0x80000000LL - offset,
                 "bootstrap stream: offset + n_resamples must be <= 2^31");
    TFEP_REQUIRE(n_resamples <= 0x7fffffffLL, "bootstrap stream: too many resamples in one launch");
    return TFEP_OK;
}

template <typename T>
int bootstrap_fep_resampled_launch(const T* work, const T* bias, const double* table, const double* stats, const int* flag,
                                   int64_t n_data, int64_t n_resamples, int64_t sample_size, int64_t high, int64_t seed,
                                   int64_t offset, int bayesian, T kT, double* out, void* stream) {
    if (int rc = bootstrap_stream_check(n_resamples, sample_size, seed, offset)) return rc;
    TFEP_REQUIRE(high >= 1 && high <= 0x7fffffffLL, "bootstrap_fep_resampled: high must be in [1, 2^31)");
    TFEP_REQUIRE(high <= n_data, "bootstrap_fep_resampled: high must be <= n_data");
    TFEP_REQUIRE(!bayesian || (sample_size == high && !bias),
                 "bootstrap_fep_resampled: the Bayesian mode needs sample_size == high and no bias");
    TFEP_REQUIRE(kT > (T)0, "bootstrap_fep_resampled: kT must be positive");
    if (n_resamples == 0) return TFEP_OK;
    TFEP_REQUIRE(work && table && stats && flag && out, "bootstrap_fep_resampled: NULL pointer");
    bootstrap_fep_resampled_kernel<T><<<(unsigned)n_resamples, 256, 0, (hipStream_t)stream>>>(
        work, bias, table, stats, flag, n_data, sample_size, (uint32_t)high, seed, offset, bayesian, 1.0 / (double)kT,
        (double)kT, out);
    return check_launch("bootstrap_fep_resampled_kernel");
}

}  // namespace tfep

using namespace tfep;

extern "C" {

int tfep_tfep_reduce_workspace_doubles(int N) {
    int blocks = (N + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    return blocks * 9;
}

int tfep_tfep_reduce(const float* target_potentials, const float* log_det_J, const float* ref_potentials,
                     const float* log_weights, const float* bias, float kT, int ignore_nan, int N,
                     double* workspace, double* out, void* stream) {
    // an empty batch (its tensor has no storage) gives the identity: nothing is read
    TFEP_REQUIRE((target_potentials || N == 0) && out && workspace, "tfep_reduce: NULL pointer");
    TFEP_REQUIRE(N >= 0, "tfep_reduce: negative N");
    TFEP_REQUIRE(kT > 0.f, "tfep_reduce: kT must be positive");
    int blocks = (N + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipStream_t s = (hipStream_t)stream;
    tfep_reduce_partial_kernel<float><<<blocks, 256, 0, s>>>(target_potentials, log_det_J, ref_potentials, log_weights, bias,
                                                             1.0 / (double)kT, ignore_nan, N, workspace);
    tfep_reduce_final_kernel<<<1, 256, 0, s>>>(workspace, blocks, out);
    return check_launch("tfep_reduce");
}

int tfep_tfep_reduce_f64(const double* target_potentials, const double* log_det_J, const double* ref_potentials,
                         const double* log_weights, const double* bias, double kT, int ignore_nan, int N,
                         double* workspace, double* out, void* stream) {
    TFEP_REQUIRE((target_potentials || N == 0) && out && workspace, "tfep_reduce_f64: NULL pointer");
    TFEP_REQUIRE(N >= 0, "tfep_reduce_f64: negative N");
    TFEP_REQUIRE(kT > 0.0, "tfep_reduce_f64: kT must be positive");
    int blocks = (N + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    hipStream_t s = (hipStream_t)stream;
    tfep_reduce_partial_kernel<double><<<blocks, 256, 0, s>>>(target_potentials, log_det_J, ref_potentials, log_weights,
                                                              bias, 1.0 / kT, ignore_nan, N, workspace);
    tfep_reduce_final_kernel<<<1, 256, 0, s>>>(workspace, blocks, out);
    return check_launch("tfep_reduce_f64");
}

int tfep_bootstrap_fep(const float* work, const float* bias, const int64_t* indices, const float* weights,
                       int64_t n_data, int64_t n_resamples, int64_t sample_size, float kT, double* out, void* stream) {
    return bootstrap_fep_launch<float>(work, bias, indices, weights, n_data, n_resamples, sample_size, kT, out, stream);
}

int tfep_bootstrap_fep_f64(const double* work, const double* bias, const int64_t* indices, const double* weights,
                           int64_t n_data, int64_t n_resamples, int64_t sample_size, double kT, double* out, void* stream) {
    return bootstrap_fep_launch<double>(work, bias, indices, weights, n_data, n_resamples, sample_size, kT, out, stream);
}

int64_t tfep_bootstrap_table_workspace_doubles(int64_t n) { return 3 * (int64_t)table_blocks(n < 1 ? 1 : n); }

int tfep_bootstrap_table(const float* work, const float* bias, int64_t n, float kT, double* table, double* stats, int* flag,
                         double* workspace, void* stream) {
    return bootstrap_table_launch<float>(work, bias, n, kT, table, stats, flag, workspace, stream);
}

int tfep_bootstrap_table_f64(const double* work, const double* bias, int64_t n, double kT, double* table, double* stats,
                             int* flag, double* workspace, void* stream) {
    return bootstrap_table_launch<double>(work, bias, n, kT, table, stats, flag, workspace, stream);
}

int tfep_bootstrap_fep_resampled(const float* work, const float* bias, const double* table, const double* stats,
                                 const int* flag, int64_t n_data, int64_t n_resamples, int64_t sample_size, int64_t high,
                                 int64_t seed, int64_t offset, int bayesian, float kT, double* out, void* stream) {
    return bootstrap_fep_resampled_launch<float>(work, bias, table, stats, flag, n_data, n_resamples, sample_size, high, seed,
                                                 offset, bayesian, kT, out, stream);
}

int tfep_bootstrap_fep_resampled_f64(const double* work, const double* bias, const double* table, const double* stats,
                                     const int* flag, int64_t n_data, int64_t n_resamples, int64_t sample_size, int64_t high,
                                     int64_t seed, int64_t offset, int bayesian, double kT, double* out, void* stream) {
    return bootstrap_fep_resampled_launch<double>(work, bias, table, stats, flag, n_data, n_resamples, sample_size, high, seed,
                                                  offset, bayesian, kT, out, stream);
}

int tfep_bootstrap_resample_indices(int64_t n_resamples, int64_t sample_size, int64_t high, int64_t seed, int64_t offset,
                                    int64_t* out, void* stream) {
    if (int rc = bootstrap_stream_check(n_resamples, sample_size, seed, offset)) return rc;
    TFEP_REQUIRE(high >= 1 && high <= 0x7fffffffLL, "bootstrap_resample_indices: high must be in [1, 2^31)");
    if (n_resamples == 0) return TFEP_OK;
    TFEP_REQUIRE(out, "bootstrap_resample_indices: NULL pointer");
    bootstrap_resample_indices_kernel<<<(unsigned)n_resamples, 256, 0, (hipStream_t)stream>>>(sample_size, (uint32_t)high, seed,
                                                                                           offset, out);
    return check_launch("bootstrap_resample_indices_kernel");
}

int tfep_bootstrap_resample_weights(int64_t n_resamples, int64_t sample_size, int64_t seed, int64_t offset, double* out,
                                    void* stream) {
    if (int rc = bootstrap_stream_check(n_resamples, sample_size, seed, offset)) return rc;
    if (n_resamples == 0) return TFEP_OK;
    TFEP_REQUIRE(out, "bootstrap_resample_weights: NULL pointer");
    bootstrap_resample_weights_kernel<<<(unsigned)n_resamples, 256, 0, (hipStream_t)stream>>>(sample_size, seed, offset, out);
    return check_launch("bootstrap_resample_weights_kernel");
}

}  // extern "C"
