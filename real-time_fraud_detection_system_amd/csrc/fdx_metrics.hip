// fdx_metrics.hip -- f-5: the score ranking metrics of shared_functions.py:442-460
// (performance_assessment: sklearn's roc_auc_score and average_precision_score) and :538-581
// (threshold_based_metrics: the confusion counts per threshold), on device-resident scores.
//
// fdx_ranking_metrics: score -> order-preserving u64 key (descending) -> the 64-bit stable radix
// sort of fdx_rekey.hip with the label as the value stream's flag bit -> one u64 scan of the
// packed pair (group starts << 32 | positives) whose group ends are compacted into (K_g, TP_g)
// -> a fixed-grid reduction over the groups.  Every sum is either an integer one or a float64 one
// in a fixed order, so the result does not depend on the order of the input rows.
//
// fdx_threshold_counts: one pass, no sort: each row is binned against the ascending thresholds
// (LDS) into wave-private LDS counters per class; a suffix sum over the bins gives TN, FP, FN, TP.
#include <algorithm>
#include <cmath>

#include "fdx_internal.h"

namespace fdx {
namespace {

constexpr int kMBlock = 256;
constexpr int kMItems = 16;
constexpr int kMChunk = kMBlock * kMItems;  // rows per block of the scan kernels
constexpr int kMWaves = kMBlock / kWave;
constexpr int kRedGridMax = 1024;           // blocks of the group reduction
constexpr int kMaxThr = 1024;

// Ascending u64 order of the key = descending order of the score; -0.0 and +0.0 share a key
// (the group of zeros reports +0.0 as its threshold), denormals keep their own.
__device__ __forceinline__ uint64_t score_key(double s) {
    uint64_t b = (uint64_t)__double_as_longlong(s);
    if (s == 0.0) b = 0;
    const uint64_t asc = (b >> 63) ? ~b : (b | (1ull << 63));
    return ~asc;
}
__device__ __forceinline__ double key_score(uint64_t key) {
    const uint64_t asc = ~key;
    const uint64_t b = (asc >> 63) ? (asc & ~(1ull << 63)) : ~asc;
    return __longlong_as_double((long long)b);
}

__global__ void __launch_bounds__(kMBlock) k_score_keys(const double *__restrict__ score, int64_t n,
                                                        uint64_t *__restrict__ keys,
                                                        fdx_ranking_result *__restrict__ res) {
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kMBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kMBlock) {
        const double s = score[i];
        keys[i] = score_key(s);
        bad += !(fabs(s) < INFINITY);  // NaN, +-inf
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) bad += __shfl_down(bad, d, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && bad)
        atomicAdd(reinterpret_cast<unsigned long long *>(&res->n_nonfinite), (unsigned long long)bad);
}

// The scanned element of sorted position i: (i starts a group) << 32 | (label of the row).
__device__ __forceinline__ uint64_t pair_of(bool starts, uint32_t val) {
    return ((uint64_t)(starts ? 1u : 0u) << 32) | (val >> 31);
}

// part[b] = sum of the pairs of chunk b
__global__ void __launch_bounds__(kMBlock) k_group_partials(const uint64_t *__restrict__ sk,
                                                            const uint32_t *__restrict__ vals, int64_t n,
                                                            uint64_t *__restrict__ part) {
    const int64_t base = (int64_t)blockIdx.x * kMChunk;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kMItems; ++k) {
        const int64_t i = base + (int64_t)k * kMBlock + threadIdx.x;
        if (i < n) s += pair_of(i == 0 || sk[i] != sk[i - 1], vals[i]);
    }
    uint64_t tot;
    block_excl_scan<kMWaves>(s, &tot);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// single block: exclusive scan of part[0..P) in place
__global__ void __launch_bounds__(kMBlock) k_part_scan(uint64_t *__restrict__ part, int64_t P) {
    uint64_t carry = 0;
    for (int64_t c = 0; c < P; c += kMBlock) {
        const int64_t i = c + threadIdx.x;
        const uint64_t v = i < P ? part[i] : 0ull;
        uint64_t tot;
        const uint64_t ex = block_excl_scan<kMWaves>(v, &tot);
        if (i < P) part[i] = ex + carry;
        carry += tot;
    }
}

// The inclusive scan of the pairs, kept in registers: at the last row of group g (0-based) it
// holds g + 1 and TP_g, and that row writes gk[g] = K_g | TP_g << 32 (K_g = i + 1 < 2^31) and
// the curve point; the last row of all writes the totals.  g <= i < n: inside every array.
__global__ void __launch_bounds__(kMBlock) k_group_ends(const uint64_t *__restrict__ sk,
                                                        const uint32_t *__restrict__ vals, int64_t n,
                                                        const uint64_t *__restrict__ part, uint64_t *__restrict__ gk,
                                                        double *__restrict__ thr, int64_t *__restrict__ tps,
                                                        int64_t *__restrict__ fps, fdx_ranking_result *__restrict__ res) {
    const int64_t i0 = (int64_t)blockIdx.x * kMChunk + (int64_t)threadIdx.x * kMItems;
    uint64_t key[kMItems + 2];  // [0] = the row before, [kMItems + 1] = the row after
    uint32_t val[kMItems];
#pragma unroll
    for (int k = 0; k < kMItems + 2; ++k) {
        const int64_t i = i0 + k - 1;
        key[k] = i >= 0 && i < n ? sk[i] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < kMItems; ++k) val[k] = i0 + k < n ? vals[i0 + k] : 0u;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < kMItems; ++k) {
        const int64_t i = i0 + k;
        if (i < n) s += pair_of(i == 0 || key[k + 1] != key[k], val[k]);
    }
    uint64_t tot;
    uint64_t run = block_excl_scan<kMWaves>(s, &tot) + part[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kMItems; ++k) {
        const int64_t i = i0 + k;
        if (i < n) {
            run += pair_of(i == 0 || key[k + 1] != key[k], val[k]);
            if (i == n - 1 || key[k + 2] != key[k + 1]) {
                const int64_t g = (int64_t)(run >> 32) - 1, tp = (int64_t)(run & 0xFFFFFFFFull);
                gk[g] = (uint64_t)(i + 1) | ((uint64_t)tp << 32);
                if (thr) {
                    thr[g] = key_score(key[k + 1]);
                    tps[g] = tp;
                    fps[g] = i + 1 - tp;
                }
                if (i == n - 1) {
                    res->n_groups = g + 1;
                    res->n_pos = tp;
                    res->n_neg = n - tp;
                }
            }
        }
    }
}

// Per block: the partial sums over its share of the groups of
//   num = (FP_g - FP_{g-1}) * (TP_g + TP_{g-1})        (u64, exact)
//   ap  = (TP_g - TP_{g-1}) * (TP_g / K_g)             (float64: one division, one product)
// in a fixed order, so the bits depend only on (n, the groups).  Additions behind one float64
// term, longest chain: ceil(m / (grid * 256)) in the thread's loop + 8 in this block's tree
// + ceil(grid / 256) + 8 in k_ranking_final's; grid = min(ceil(n / 4096), 1024) and m <= n, so
// at most 16 + 8 + 4 + 8 = 36 for n <= 2^22, and ceil(n / 2^18) + 20 <= 8212 beyond.
// All terms are >= 0: relative error of ap <= (chain + 3) * 2^-53 (division, product, sums, / P).
__device__ __forceinline__ void block_tree_sum(uint64_t &num, double &ap) {
    __shared__ uint64_t s_n[kMBlock];
    __shared__ double s_a[kMBlock];
    const int t = threadIdx.x;
    s_n[t] = num;
    s_a[t] = ap;
    __syncthreads();
#pragma unroll
    for (int off = kMBlock / 2; off > 0; off >>= 1) {
        if (t < off) {
            s_n[t] += s_n[t + off];
            s_a[t] = s_a[t] + s_a[t + off];
        }
        __syncthreads();
    }
    num = s_n[0];
    ap = s_a[0];
}

__global__ void __launch_bounds__(kMBlock) k_group_reduce(const uint64_t *__restrict__ gk,
                                                          const fdx_ranking_result *__restrict__ res,
                                                          uint64_t *__restrict__ pnum, double *__restrict__ pap) {
    const int64_t m = res->n_groups;
    uint64_t num = 0;
    double ap = 0.0;
    for (int64_t g = (int64_t)blockIdx.x * kMBlock + threadIdx.x; g < m; g += (int64_t)gridDim.x * kMBlock) {
        const uint64_t cur = gk[g], prev = g > 0 ? gk[g - 1] : 0ull;
        const uint64_t K = cur & 0xFFFFFFFFull, TP = cur >> 32, K0 = prev & 0xFFFFFFFFull, TP0 = prev >> 32;
        num += ((K - TP) - (K0 - TP0)) * (TP + TP0);
        ap = ap + (double)(TP - TP0) * ((double)TP / (double)K);
    }
    block_tree_sum(num, ap);
    if (threadIdx.x == 0) {
        pnum[blockIdx.x] = num;
        pap[blockIdx.x] = ap;
    }
}

// one block: the block partials in index order, then the result's derived fields
__global__ void __launch_bounds__(kMBlock) k_ranking_final(const uint64_t *__restrict__ pnum,
                                                           const double *__restrict__ pap, int parts,
                                                           fdx_ranking_result *__restrict__ res) {
    uint64_t num = 0;
    double ap = 0.0;
    for (int b = threadIdx.x; b < parts; b += kMBlock) {
        num += pnum[b];
        ap = ap + pap[b];
    }
    block_tree_sum(num, ap);
    if (threadIdx.x == 0) {
        const uint64_t P = (uint64_t)res->n_pos, N = (uint64_t)res->n_neg;
        res->auc_num = num;
        res->auc = P && N ? (double)num / (double)(2 * P * N) : (double)NAN;
        res->ap = P ? ap / (double)P : 0.0;
    }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct RankWs {
    uint64_t *keys;  // the sort's input; its first pass consumes it, and the (K_g, TP_g) pairs follow
    uint64_t *pnum;
    double *pap;
    uint64_t *part;
    void *sort;
};

size_t rank_ws(int64_t n, RankWs *w, char *base) {
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *p = base ? base + off : nullptr;
        off += align256(bytes);
        return p;
    };
    RankWs t;
    t.keys = reinterpret_cast<uint64_t *>(take(sizeof(uint64_t) * (size_t)n));
    t.pnum = reinterpret_cast<uint64_t *>(take(sizeof(uint64_t) * kRedGridMax));
    t.pap = reinterpret_cast<double *>(take(sizeof(double) * kRedGridMax));
    t.part = reinterpret_cast<uint64_t *>(take(sizeof(uint64_t) * (size_t)(ceil_div(n, kMChunk) + 1)));
    t.sort = take(sort_u64_flag_workspace_size(n));
    if (w) *w = t;
    return off;
}

// ---- threshold counts
// bins[c][b], b = #{j : t_j <= p} (NaN score: n_thr), c = label != 0
__global__ void __launch_bounds__(kMBlock) k_thr_bins(const double *__restrict__ score,
                                                      const uint8_t *__restrict__ label, int64_t n,
                                                      const double *__restrict__ thr, int n_thr,
                                                      unsigned long long *__restrict__ bins) {
    __shared__ double s_t[kMaxThr];
    __shared__ uint32_t s_c[kMWaves][2][kMaxThr + 1];
    const int tid = threadIdx.x, wv = tid / kWave, nb = n_thr + 1;
    for (int j = tid; j < n_thr; j += kMBlock) s_t[j] = thr[j];
    for (int d = tid; d < kMWaves * 2 * (kMaxThr + 1); d += kMBlock) (&s_c[0][0][0])[d] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kMBlock + tid; i < n; i += (int64_t)gridDim.x * kMBlock) {
        const double p = score[i];
        int lo = 0, hi = n_thr;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_t[mid] <= p) lo = mid + 1; else hi = mid;
        }
        if (p != p) lo = n_thr;  // not (NaN < t) at every threshold
        atomicAdd(&s_c[wv][label[i] != 0][lo], 1u);
    }
    __syncthreads();
    for (int d = tid; d < 2 * nb; d += kMBlock) {
        const int c = d / nb, b = d - c * nb;
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kMWaves; ++w) s += s_c[w][c][b];
        if (s) atomicAdd(&bins[d], (unsigned long long)s);
    }
}

// counts[j] = TN, FP, FN, TP with "predicted 1" = the bins above j (t_j <= p, or p NaN)
__global__ void __launch_bounds__(kMBlock) k_thr_counts(const unsigned long long *__restrict__ bins, int n_thr,
                                                        int64_t *__restrict__ counts) {
    __shared__ unsigned long long s_b[2][kMaxThr + 1];
    const int nb = n_thr + 1;
    for (int d = threadIdx.x; d < 2 * nb; d += kMBlock) s_b[d / nb][d % nb] = bins[d];
    __syncthreads();
    for (int j = threadIdx.x; j < n_thr; j += kMBlock) {
        unsigned long long neg = 0, pos = 0, fp = 0, tp = 0;
        for (int b = 0; b < nb; ++b) {
            neg += s_b[0][b];
            pos += s_b[1][b];
            if (b > j) {
                fp += s_b[0][b];
                tp += s_b[1][b];
            }
        }
        counts[4 * j + 0] = (int64_t)(neg - fp);
        counts[4 * j + 1] = (int64_t)fp;
        counts[4 * j + 2] = (int64_t)(pos - tp);
        counts[4 * j + 3] = (int64_t)tp;
    }
}

}  // namespace
}  // namespace fdx

using namespace fdx;

extern "C" size_t fdx_ranking_metrics_workspace_size(int64_t n) {
    return rank_ws(n < 0 ? 0 : n, nullptr, nullptr);
}

extern "C" int fdx_ranking_metrics(const double *score_d, const uint8_t *label_d, int64_t n,
                                   fdx_ranking_result *result_d, double *thr_d, int64_t *tps_d, int64_t *fps_d,
                                   void *workspace_d, size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "n out of range");
    FDX_REQUIRE(result_d, "null result_d");
    FDX_REQUIRE((thr_d != nullptr) == (tps_d != nullptr) && (thr_d != nullptr) == (fps_d != nullptr),
                "thr_d, tps_d and fps_d: all three or none");
    FDX_REQUIRE(n == 0 || (score_d && label_d), "null score_d / label_d");
    RankWs w;
    const size_t need = rank_ws(n, &w, reinterpret_cast<char *>(workspace_d));
    if (!workspace_d || workspace_bytes < need) {
        set_error("ranking metrics workspace too small: %zu < %zu", workspace_bytes, need);
        return FDX_E_WORKSPACE;
    }
    FDX_REQUIRE(((uintptr_t)workspace_d & 255) == 0, "workspace_d must be 256-byte aligned");
    hipStream_t st = as_stream(stream);
    FDX_HIP(hipMemsetAsync(result_d, 0, sizeof(fdx_ranking_result), st));
    int parts = 0;
    if (n > 0) {
        hipLaunchKernelGGL(k_score_keys, dim3(stream_grid(n, kMBlock)), dim3(kMBlock), 0, st, score_d, n, w.keys,
                           result_d);
        FDX_LAUNCHED("k_score_keys");
        const uint64_t *sk = nullptr;
        const uint32_t *vals = nullptr;
        int rc = sort_u64_flag(w.keys, label_d, n, w.sort, st, &sk, &vals);
        if (rc) return rc;
        const int64_t chunks = ceil_div(n, kMChunk);
        hipLaunchKernelGGL(k_group_partials, dim3((unsigned)chunks), dim3(kMBlock), 0, st, sk, vals, n, w.part);
        FDX_LAUNCHED("k_group_partials");
        hipLaunchKernelGGL(k_part_scan, dim3(1), dim3(kMBlock), 0, st, w.part, chunks);
        FDX_LAUNCHED("k_part_scan");
        uint64_t *gk = w.keys;
        hipLaunchKernelGGL(k_group_ends, dim3((unsigned)chunks), dim3(kMBlock), 0, st, sk, vals, n, w.part, gk, thr_d,
                           tps_d, fps_d, result_d);
        FDX_LAUNCHED("k_group_ends");
        parts = (int)std::min<int64_t>(chunks, kRedGridMax);
        hipLaunchKernelGGL(k_group_reduce, dim3((unsigned)parts), dim3(kMBlock), 0, st, gk, result_d, w.pnum, w.pap);
        FDX_LAUNCHED("k_group_reduce");
    }
    hipLaunchKernelGGL(k_ranking_final, dim3(1), dim3(kMBlock), 0, st, w.pnum, w.pap, parts, result_d);
    FDX_LAUNCHED("k_ranking_final");
    return FDX_OK;
}

extern "C" size_t fdx_threshold_counts_workspace_size(int32_t n_thr) {
    if (n_thr < 0) n_thr = 0;
    if (n_thr > kMaxThr) n_thr = kMaxThr;
    return sizeof(unsigned long long) * 2 * (size_t)(n_thr + 1);
}

extern "C" int fdx_threshold_counts(const double *score_d, const uint8_t *label_d, int64_t n,
                                    const double *thr_sorted_d, int32_t n_thr, int64_t *counts_d, void *workspace_d,
                                    size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(n >= 0 && n < (int64_t)INT32_MAX, "n out of range");
    FDX_REQUIRE(n_thr >= 0 && n_thr <= kMaxThr, "n_thr must be in [0, %d]", kMaxThr);
    if (n_thr == 0) return FDX_OK;
    FDX_REQUIRE(thr_sorted_d && counts_d, "null thr_sorted_d / counts_d");
    FDX_REQUIRE(n == 0 || (score_d && label_d), "null score_d / label_d");
    const size_t need = fdx_threshold_counts_workspace_size(n_thr);
    if (!workspace_d || workspace_bytes < need) {
        set_error("threshold counts workspace too small: %zu < %zu", workspace_bytes, need);
        return FDX_E_WORKSPACE;
    }
    FDX_REQUIRE(((uintptr_t)workspace_d & 7) == 0, "workspace_d must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    // the thresholds are read back (n_thr * 8 bytes, the call's one host sync): a NaN or an
    // unsorted list would bin the rows wrongly without a trace
    double thr_h[kMaxThr];
    FDX_HIP(hipMemcpyAsync(thr_h, thr_sorted_d, sizeof(double) * n_thr, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < n_thr; ++j) {
        FDX_REQUIRE(!std::isnan(thr_h[j]), "thr_sorted_d[%d] is NaN", j);
        FDX_REQUIRE(j == 0 || thr_h[j - 1] <= thr_h[j], "thr_sorted_d is not ascending at [%d]", j);
    }
    unsigned long long *bins = reinterpret_cast<unsigned long long *>(workspace_d);
    FDX_HIP(hipMemsetAsync(bins, 0, need, st));
    if (n > 0) {
        hipLaunchKernelGGL(k_thr_bins, dim3(stream_grid(n, kMBlock)), dim3(kMBlock), 0, st, score_d, label_d, n,
                           thr_sorted_d, (int)n_thr, bins);
        FDX_LAUNCHED("k_thr_bins");
    }
    hipLaunchKernelGGL(k_thr_counts, dim3(1), dim3(kMBlock), 0, st, bins, (int)n_thr, counts_d);
    FDX_LAUNCHED("k_thr_counts");
    return FDX_OK;
}
