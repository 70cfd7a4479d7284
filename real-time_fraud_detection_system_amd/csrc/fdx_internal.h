// Internal helpers shared by the fdx HIP translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "fdx.h"

namespace fdx {

constexpr int kWave = 64;  // CDNA wavefront width

void set_error(const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

#define FDX_REQUIRE(cond, ...)                     \
    do {                                           \
        if (!(cond)) {                             \
            ::fdx::set_error(__VA_ARGS__);         \
            return FDX_E_INVALID;                  \
        }                                          \
    } while (0)

#define FDX_HIP(call)                                                                     \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            ::fdx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),       \
                             __FILE__, __LINE__);                                         \
            return FDX_E_HIP;                                                             \
        }                                                                                 \
    } while (0)

// Checks the launch that was just enqueued.
#define FDX_LAUNCHED(name)                                                                \
    do {                                                                                  \
        hipError_t e_ = hipGetLastError();                                                \
        if (e_ != hipSuccess) {                                                           \
            ::fdx::set_error("launch of %s failed: %s", name, hipGetErrorString(e_));      \
            return FDX_E_HIP;                                                             \
        }                                                                                 \
    } while (0)

// Integer min / max for device code.  HIP's min<int64_t>(a, b) with either argument not already
// int64_t converts both to double (v_cvt + v_ldexp + v_min_f64 + v_cvt back): slow, and a VGPR
// result where the operands were wave-uniform -- a buffer descriptor built from one made every
// buffer store of k_customer_walk a readfirstlane loop.
__device__ __forceinline__ int64_t imin64(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t imax64(int64_t a, int64_t b) { return a > b ? a : b; }

// Terminal count record word (fdx_terminal_windows_packed): NB | FRAUD << 32.
__device__ __forceinline__ int64_t term_word(int32_t nb, int32_t fraud) {
    return (int64_t)(((uint64_t)(uint32_t)fraud << 32) | (uint32_t)nb);
}
__device__ __forceinline__ int32_t term_nb(int64_t w) { return (int32_t)(uint32_t)((uint64_t)w & 0xFFFFFFFFu); }
// RISK = FRAUD / NB with fillna(0) of 0/0 (feature_transformation.ipynb:1512-1517)
__device__ __forceinline__ double term_risk(int64_t w) {
    const uint32_t nb = (uint32_t)((uint64_t)w & 0xFFFFFFFFu), fr = (uint32_t)((uint64_t)w >> 32);
    return nb > 0 ? (double)fr / (double)nb : 0.0;
}

// COMPACT count records (fdx_terminal_windows_grouped + FDX_TERM_COMPACT, W = 3): 16 bytes per row,
// lo = NB_0 | NB_1 << 21 | NB_2 << 42, hi = FRAUD_0 | FRAUD_1 << 21 | FRAUD_2 << 42 (one
// aligned 16-byte access instead of a 24-byte record over two).  A row whose window count
// does not fit 21 bits has bit 63 of lo set and the low 63 bits = the word offset, from the
// start of the record array, of its full 3-word record (the array's overflow area).
constexpr int kCompactBits = 21;
constexpr int64_t kCompactMax = (1LL << kCompactBits) - 1;
__device__ __forceinline__ void compact_load(const int64_t *rec, int64_t q, int64_t (&tw)[3]) {
    const longlong2 p = *reinterpret_cast<const longlong2 *>(rec + 2 * q);
    if (p.x < 0) {
        const int64_t *wide = rec + (p.x & INT64_MAX);
        tw[0] = wide[0];
        tw[1] = wide[1];
        tw[2] = wide[2];
    } else {
#pragma unroll
        for (int w = 0; w < 3; ++w)
            tw[w] = term_word((int32_t)((p.x >> (kCompactBits * w)) & kCompactMax),
                              (int32_t)((p.y >> (kCompactBits * w)) & kCompactMax));
    }
}

// pandas roll_sum state (aggregations.pyx add_sum/remove_sum/calc_sum), emulated exactly: the
// batch windows (fdx_windows.hip) and the streaming state (fdx_stream.hip) run this one copy.
struct RollSum {
    double sum, c_add, c_rem, prev;
    int32_t nobs, nsame;

    __device__ __forceinline__ void reset(double first) {
        sum = 0.0; c_add = 0.0; c_rem = 0.0; prev = first; nobs = 0; nsame = 0;
    }
    __device__ __forceinline__ void add(double v) {
        if (v == v) {
            nobs += 1;
            double y = v - c_add;
            double t = sum + y;
            c_add = (t - sum) - y;
            sum = t;
            nsame = (v == prev) ? nsame + 1 : 1;
            prev = v;
        }
    }
    __device__ __forceinline__ void remove(double v) {
        if (v == v) {
            nobs -= 1;
            double y = -v - c_rem;
            double t = sum + y;
            c_rem = (t - sum) - y;
            sum = t;
        }
    }
    // calc_sum with min_periods = 1 (offset windows)
    __device__ __forceinline__ double value() const {
        if (nobs >= 1) return (nsame >= nobs) ? prev * (double)nobs : sum;
        return __builtin_nan("");
    }
};

// A rolling sum over its count (the count as a double; the average of every customer window),
// correctly rounded also where the quotient is denormal.  Observed on an MI355X: with plain
// `s / n`, denormal averages of denormal amounts (tests/amount_classes.py, class "tiny") came out
// 1 unit off the IEEE quotient (x86, pandas) in 4 of 61,881 cells of k_customer_exact, the strided
// walk and the stream alike, every normal quotient being right.  The supposed cause, not measured
// further: the division's last step rounds to 53 bits in a scaled domain and the result is
// rounded again when it is scaled back into the denormal range.  Whatever the cause, where the
// quotient is at most DBL_MIN (the double rounding can also land on DBL_MIN itself) the residual
// s - q * n is a small multiple of the denormal unit u, so one fma gives it exactly, and q moves
// by one unit when it is not the nearest (ties to even); this assumes the device's q is within
// one unit, which is all that was ever seen.  A larger, zero-from-zero, infinite or NaN quotient
// skips all of it.
__device__ __forceinline__ double div_count(double s, double n) {
    double q = s / n;
    if (__builtin_fabs(q) <= 2.2250738585072014e-308 && s != 0.0) {
        const double u = 4.9406564584124654e-324;
        const double r = __builtin_fma(-q, n, s);
        const double d = 2.0 * __builtin_fabs(r), nu = n * u;
        if (d > nu || (d == nu && (__double_as_longlong(q) & 1))) q += __builtin_copysign(u, r);
        if (q == 0.0) q = __builtin_copysign(0.0, s);  // n > 0: an underflow to zero keeps the sum's sign
    }
    return q;
}

// The 64-bit finaliser the open-addressing tables hash their keys with (the dedup table of
// fdx_aux.hip, the key directory of fdx_keydir.hip): every input bit reaches every output bit.
__device__ __forceinline__ unsigned long long mix64(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

constexpr int64_t kNsPerSec = 1000000000LL;
constexpr int32_t kSecPerDay = 86400, kSecPerHour = 3600;

// The weekend / night flags of a nanosecond timestamp, with the floor divisions of pandas'
// dt accessors (feature_transformation.ipynb's is_weekend / is_night; fraud_detection.py's
// dayofweek / hour for FDX_FLAGS_SPARK).  floor(t / 1 day) = floor(floor(t / 1 s) / 86,400 s) and
// the hour likewise, so one 64-bit division to whole seconds, then 32-bit day / hour / weekday
// arithmetic while the seconds fit (1901-2038), the 64-bit form otherwise: the same values.
__device__ __forceinline__ void day_flags(int64_t t, int32_t flags_mode, bool &we, bool &ni) {
    int64_t sec = t / kNsPerSec;
    if (sec * kNsPerSec != t && t < 0) --sec;
    int32_t hour, wd;
    if (sec >= INT32_MIN && sec <= INT32_MAX) {
        const int32_t s32 = (int32_t)sec;
        int32_t day = s32 / kSecPerDay;
        if (day * kSecPerDay != s32 && s32 < 0) --day;
        hour = (s32 - day * kSecPerDay) / kSecPerHour;
        wd = (day + 3) % 7;  // Monday = 0 (1970-01-01 was a Thursday); day may be < 0
    } else {
        int64_t day = sec / kSecPerDay;
        if (day * kSecPerDay != sec && sec < 0) --day;
        hour = (int32_t)((sec - day * kSecPerDay) / kSecPerHour);
        wd = (int32_t)((day + 3) % 7);
    }
    if (wd < 0) wd += 7;
    // Spark dayofweek: Sunday = 1 .. Saturday = 7
    we = flags_mode == FDX_FLAGS_NOTEBOOK ? wd >= 5 : (((wd + 1) % 7) + 1) >= 5;
    ni = flags_mode == FDX_FLAGS_NOTEBOOK ? hour <= 6 : hour >= 20;
}

// Inclusive scan (sum) across the wave; lane = the thread's lane.
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
    // __shfl_up has no uint64_t overload: 8-byte integers travel as unsigned long long
    using S = std::conditional_t<std::is_integral<T>::value && sizeof(T) == 8, unsigned long long, T>;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const T u = (T)__shfl_up((S)v, d, kWave);
        if (lane >= d) v += u;
    }
    return v;
}

// Exclusive scan of one value per thread over a block of WAVES waves; *total = the block's sum.
// Its own barriers on both sides of the LDS use, so calls may follow each other.
template <int WAVES, class T>
__device__ __forceinline__ T block_excl_scan(T v, T *total) {
    __shared__ T s_w[WAVES];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const T inc = wave_incl_scan(v, lane);
    if (lane == kWave - 1) s_w[wv] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const T x = s_w[w];
        if (w < wv) base += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline size_t round_up(size_t a, size_t m) { return (a + m - 1) / m * m; }
inline size_t al256(size_t x) { return round_up(x, 256); }  // workspace carve-outs: 256-byte aligned

// Grid for a grid-stride streaming kernel: enough blocks to fill 256 CUs several times,
// capped so launch overhead and tail stay small (cdna_hip_programming.md Guideline 11).
inline unsigned stream_grid(int64_t n, int block, int64_t cap = 256 * 8) {
    int64_t g = ceil_div(n, block);
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

// f-10: the device check of a retirement id map (fdx_stream.hip; fdx_stream_retire_apply and
// fdx_keydir_remap run this one copy).  A valid map over n ids is -1 for a retired id and, for
// the survivors, their rank among the survivors: 0 .. kept-1 in increasing id order.  Enqueues
// three phases on st (flags, exclusive scan, check) and reads nothing back; afterwards, on the
// device, res_d->bad != 0: malformed; kept: the survivors; first: the first id with map[id] != id
// (n when there is none), so ids below it stay where they are.  flag_d: n + 1 words; scan_ws_d:
// fdx_exclusive_scan_u32_workspace_size(n + 1) bytes.
struct MapRes {
    unsigned long long kept, first;
    uint32_t bad, pad;
};
int map_validate(const int32_t *map_d, int64_t n, MapRes *res_d, uint32_t *flag_d, void *scan_ws_d, hipStream_t st);

// The stable 64-bit LSD radix sort of fdx_rekey.hip (the one behind fdx_argsort_i64), for the
// other translation units: ascending over all 64 bits of keys_d, n in [1, INT32_MAX).
// *sorted_d = the sorted keys and *vals_d = per sorted position the input row index with
// bit 31 = flag_d[row] != 0; both lie inside workspace_d (sort_u64_flag_workspace_size(n) bytes,
// 256-byte aligned).
size_t sort_u64_flag_workspace_size(int64_t n);
int sort_u64_flag(const uint64_t *keys_d, const uint8_t *flag_d, int64_t n, void *workspace_d, hipStream_t st,
                  const uint64_t **sorted_d, const uint32_t **vals_d);

}  // namespace fdx
