// fdx_stream.hip -- config 5 (BASELINE.json): streaming micro-batches of CDC transactions with
// INCREMENTAL window state, so that a batch costs O(batch) instead of a re-scan of history.
//
// The state carried between batches is exactly what the batch kernels' recurrences hold at
// the last row of a key, so a stream of batches gives bit-identical features to one batch
// call over the concatenated history (tests/test_gpu_stream.py):
//   customer (feature_transformation.ipynb:601-628): per window the pandas roll_sum state
//     (sum, Kahan add/remove compensations, nobs, n-same run, prev -- aggregations.pyx
//     add_sum/remove_sum/calc_sum, see RollSum in fdx_internal.h) and the window's tail
//     (pandas' variable-window start), plus a ring of the customer's recent (ts, amount) rows
//     from which the tails remove;
//   terminal (:1495-1522): per window boundary (delay, delay + w) the count of the terminal's
//     rows with ts <= t - boundary and their fraud count, plus a ring of recent (ts, fraud).
//
// HBM layout (one record per key, 8-byte words, so a key's state is 2-3 cache lines):
//   customer record  [n, last_ts, (tail, sum, c_add, c_rem, prev, nobs | nsame << 32) x W]
//   customer ring    C entries of {ts, amount} per customer (C a power of two)
//   terminal record  [n, last_ts, (p_k, F_k) x (W + 1)]     k = 0: delay, k = w+1: delay + w
//   terminal ring    T entries of (ts << 1 | fraud) per terminal
// Row r of a key's history sits in ring slot r & (C-1); a ring slot is overwritten only once
// every window has passed the row in it (else status bit 1/2: ring too small).
//
// One update = two launches over the batch:
//   k_stream_link    per row: push the row on its customer's and terminal's chain (one
//                    atomic exchange each on a head array), write amount + flags;
//   k_stream_process per row: the thread whose row ended up at the head of a chain owns the
//                    key: it walks the chain in (ts, row) order, advances the key's state
//                    row by row, writes that row's features, stores the state back and clears
//                    the head.  Rows of one key in one batch are few (64k rows over 1M
//                    customers: mostly one), so the chain selection (quadratic in the rows of
//                    one key in one batch) is short; big bootstrap batches pay it per key.
// Delayed fraud reports (a row's label is rarely known when the row is scored) = two launches
// over the reports: k_stream_link (terminal chains only) and k_stream_labels, which sets the
// row's ring bit and corrects the fraud counts as if the label had been there all along.
// Latency-bound (a handful of dependent HBM reads per key), no MFMA, no LDS.
#include <climits>
#include <cstdlib>
#include <cstring>

#include "fdx_internal.h"

namespace fdx {
namespace {

constexpr int kMaxW = FDX_MAX_WINDOWS;

enum : int32_t {
    kStCustRing = 1,    // a customer ring slot still inside a window was overwritten
    kStTermRing = 2,    // same for a terminal ring
    kStKey = 4,         // customer / terminal id outside [0, capacity)
    kStOrder = 8,       // a key's rows went back in time across batches
    kStLateRing = 16,   // a late terminal row's farthest window reaches past the ring's live rows
};

// k_stream_process<W, LATE>'s extra arguments; none when LATE is false
template <bool LATE>
struct LateArgs {};
template <>
struct LateArgs<true> {
    int64_t max_late;             // a terminal row may be this far (ns) behind the terminal's last row
    int32_t strict;               // the state was restored: n <= T no longer proves the ring is whole
    unsigned long long *counts;   // {late_rows, late_past_delay}
};

struct StreamWin {
    int64_t win[kMaxW];         // customer windows (ns)
    int64_t tb[kMaxW + 1];      // terminal boundaries: delay, delay + win[w] (ns)
};

struct alignas(16) CEnt {
    int64_t ts;
    double amt;
};

__global__ void __launch_bounds__(256) k_stream_link(
    const int64_t *__restrict__ ts, const int32_t *__restrict__ cust, const double *__restrict__ amount,
    const int32_t *__restrict__ term, int64_t n, int64_t n_cust, int64_t n_term, int32_t *__restrict__ chead,
    int32_t *__restrict__ cnext, int32_t *__restrict__ thead, int32_t *__restrict__ tnext, int32_t mode,
    double *__restrict__ X, int64_t ld, int32_t *__restrict__ status) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (cust) {
            const int32_t c = cust[i];
            if (c < 0 || c >= n_cust) {
                atomicOr(status, kStKey);
            } else {
                cnext[i] = atomicExch(&chead[c], (int32_t)i);
            }
            if (X) {
                bool we, ni;
                day_flags(ts[i], mode, we, ni);
                double *x = X + i * ld;
                x[0] = amount[i]; x[1] = we; x[2] = ni;
            }
        }
        if (term) {
            const int32_t t = term[i];
            if (t < 0 || t >= n_term) {
                atomicOr(status, kStKey);
            } else {
                tnext[i] = atomicExch(&thead[t], (int32_t)i);
            }
        }
    }
}

// Visit the rows of the chain at `head` in (ts, row) order.
template <class F>
__device__ __forceinline__ void chain_in_order(int32_t head, const int32_t *__restrict__ next,
                                               const int64_t *__restrict__ ts, F &&visit) {
    int cnt = 0;
    int64_t bt = INT64_MAX;
    int32_t br = INT32_MAX;
    for (int32_t j = head; j >= 0; j = next[j]) {
        ++cnt;
        const int64_t t = ts[j];
        if (t < bt || (t == bt && j < br)) { bt = t; br = j; }
    }
    visit(br, bt);
    for (int k = 1; k < cnt; ++k) {
        int64_t nt = INT64_MAX;
        int32_t nr = INT32_MAX;
        for (int32_t j = head; j >= 0; j = next[j]) {
            const int64_t t = ts[j];
            const bool after = t > bt || (t == bt && j > br);
            const bool before = t < nt || (t == nt && j < nr);
            if (after && before) { nt = t; nr = j; }
        }
        bt = nt; br = nr;
        visit(br, bt);
    }
}

template <int W>
__device__ void customer_key(int32_t c, int32_t head, const int32_t *__restrict__ cnext,
                             const int64_t *__restrict__ ts, const double *__restrict__ amount,
                             const StreamWin &sw, int64_t *__restrict__ cstate, CEnt *__restrict__ cring,
                             int32_t C, double *__restrict__ X, int64_t ld, int32_t *__restrict__ cnb_out,
                             double *__restrict__ csum_out, int64_t n_rows, int32_t *__restrict__ status) {
    int64_t *rec = cstate + (int64_t)c * (2 + 6 * W);
    CEnt *ring = cring + (int64_t)c * C;
    const int64_t mask = C - 1;
    int64_t n = rec[0], last = rec[1];
    int64_t tail[W];
    RollSum s[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const int64_t *r = rec + 2 + 6 * w;
        tail[w] = r[0];
        s[w].sum = __longlong_as_double(r[1]);
        s[w].c_add = __longlong_as_double(r[2]);
        s[w].c_rem = __longlong_as_double(r[3]);
        s[w].prev = __longlong_as_double(r[4]);
        s[w].nobs = (int32_t)(uint32_t)((uint64_t)r[5] & 0xFFFFFFFFu);
        s[w].nsame = (int32_t)(uint32_t)((uint64_t)r[5] >> 32);
    }
    int32_t bad = 0;
    chain_in_order(head, cnext, ts, [&](int32_t row, int64_t t) {
        const double v = amount[row];
        if (n > 0 && t < last) bad |= kStOrder;
        // the first ring entry each window's tail looks at, loaded together
        CEnt e[W];
#pragma unroll
        for (int w = 0; w < W; ++w) e[w] = tail[w] < n ? ring[tail[w] & mask] : CEnt{INT64_MAX, 0.0};
        int64_t tmin = n;
        double *x = cnb_out ? nullptr : X + (int64_t)row * ld + 3;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int64_t bound = t - sw.win[w];
            int64_t nt = tail[w];
            // pandas removes rows start[i-1] .. start[i]-1 (Kahan, c_rem) then adds row i;
            // when the window restarts (start[i] >= end[i-1]) it re-initialises instead, which
            // discards whatever the removals did -- so removing while advancing is exact.
            while (e[w].ts <= bound) {
                s[w].remove(e[w].amt);
                ++nt;
                e[w] = nt < n ? ring[nt & mask] : CEnt{INT64_MAX, 0.0};
            }
            if (nt >= n) s[w].reset(v);
            s[w].add(v);
            tail[w] = nt;
            tmin = nt < tmin ? nt : tmin;
            if (cnb_out) {  // scoring planes: NB and the rolling SUM (the consumer divides)
                cnb_out[(int64_t)w * n_rows + row] = s[w].nobs;
                csum_out[(int64_t)w * n_rows + row] = s[w].value();
            } else {
                x[2 * w] = (double)s[w].nobs;
                x[2 * w + 1] = div_count(s[w].value(), (double)s[w].nobs);
            }
        }
        if (n >= C && n - C >= tmin) bad |= kStCustRing;
        ring[n & mask] = CEnt{t, v};
        ++n;
        last = t;
    });
    rec[0] = n;
    rec[1] = last;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        int64_t *r = rec + 2 + 6 * w;
        r[0] = tail[w];
        r[1] = __double_as_longlong(s[w].sum);
        r[2] = __double_as_longlong(s[w].c_add);
        r[3] = __double_as_longlong(s[w].c_rem);
        r[4] = __double_as_longlong(s[w].prev);
        r[5] = (int64_t)(((uint64_t)(uint32_t)s[w].nsame << 32) | (uint32_t)s[w].nobs);
    }
    if (bad) atomicOr(status, bad);
}

// Late terminal rows (f-8, LATE only).  chain_in_order visits a batch's rows in (ts, row) order,
// so the rows older than the terminal's last row come first; each is handled on its own and
// the in-order rows that follow take the unchanged path.
//
// Invariant: after a late row landed, the terminal's record and its live ring equal those of a
// stream that had received the same rows in (ts, arrival) order.  The ring stays sorted: the
// row is inserted after the rows with ts <= t (positions [q, n) move up by one), and a boundary
// pointer p[k] counts the rows with ts <= last - tb[k], so it gains the row (and F[k] its fraud
// bit) exactly when t <= last - tb[k].  The row's own features are counted over what had
// arrived: pos_k = the live rows with ts <= t - tb[k] (binary search; pos_k <= p[k] because
// t < last) and the fraud bits of [pos_k, p[k]) taken back out of F[k].  The windows end tb[0]
// before a row, so a row late by no more than that delay changes no feature of any row.
// Refused (status bit, zero counts, nothing inserted): a row more than max_late behind, and a
// row whose farthest window starts before the ring's oldest live row -- unless the ring never
// wrapped (n <= T) on a state that was never restored (a snapshot drops the rows before
// min p[k], so after a restore only the oldest live row's ts proves coverage).
template <int W, bool LATE>
__device__ void terminal_key(int32_t tk, int32_t head, const int32_t *__restrict__ tnext,
                             const int64_t *__restrict__ ts, const uint8_t *__restrict__ fraud,
                             const StreamWin &sw, int64_t *__restrict__ tstate, int64_t *__restrict__ tring,
                             int32_t T, double *__restrict__ X, int64_t ld, int32_t tcol0, int64_t *__restrict__ rec_out,
                             int32_t *__restrict__ status, const LateArgs<LATE> &la) {
    constexpr int K = W + 1;
    int64_t *rec = tstate + (int64_t)tk * (2 + 2 * K);
    int64_t *ring = tring + (int64_t)tk * T;
    const int64_t mask = T - 1;
    int64_t n = rec[0], last = rec[1];
    int64_t p[K], F[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] = rec[2 + 2 * k]; F[k] = rec[3 + 2 * k]; }
    int32_t bad = 0;
    [[maybe_unused]] int32_t late_rows = 0, late_past = 0;
    chain_in_order(head, tnext, ts, [&](int32_t row, int64_t t) {
        if constexpr (LATE) {
            if (n > 0 && t < last) {
                const int64_t lo = n > T ? n - T : 0;  // live ring positions [lo, n), sorted by ts
                auto upper = [&](int64_t bound) {      // the first live position with ts > bound
                    int64_t a = lo, b = n;
                    while (a < b) {
                        const int64_t mid = (a + b) >> 1;
                        if ((ring[mid & mask] >> 1) <= bound) a = mid + 1; else b = mid;
                    }
                    return a;
                };
                int32_t refused = 0;
                if (last - t > la.max_late) {
                    refused = kStOrder;
                } else if (!((n <= T && !la.strict) || (ring[lo & mask] >> 1) <= t - sw.tb[W])) {
                    refused = kStLateRing;
                }
                bad |= refused;
                // the row's own counts, from what had arrived
                int64_t pos[K], Fat[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    pos[k] = 0; Fat[k] = 0;
                    if (!refused) {
                        pos[k] = upper(t - sw.tb[k]);
                        Fat[k] = F[k];
                        const int64_t pe = imin64(p[k], n);
                        for (int64_t j = pos[k]; j < pe; ++j) Fat[k] -= ring[j & mask] & 1;
                    }
                }
                // (the output forms of the in-order path, written out again: behind one shared helper
                // the LATE = false kernel compiles to another register assignment, and it is to stay
                // instruction for instruction the kernel it was before LATE existed)
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const int32_t nb = (int32_t)(pos[0] - pos[w + 1]), fr = (int32_t)(Fat[0] - Fat[w + 1]);
                    if (rec_out) {
                        rec_out[(int64_t)row * W + w] = term_word(nb, fr);
                    } else {
                        double *x = X + (int64_t)row * ld + tcol0 + 2 * w;
                        x[0] = (double)nb;
                        x[1] = nb > 0 ? (double)fr / (double)nb : 0.0;
                    }
                }
                if (refused) return;
                // insertion after the rows with ts <= t: every later row moves up one position (a
                // carry from the lowest, so a full ring drops its oldest row, as a push does)
                const int64_t fbit = fraud[row] ? 1 : 0;
                int64_t carry = (int64_t)(((uint64_t)t << 1) | (uint64_t)fbit);
                for (int64_t j = upper(t); j < n; ++j) {
                    const int64_t moved = ring[j & mask];
                    ring[j & mask] = carry;
                    carry = moved;
                }
                ring[n & mask] = carry;
                int64_t pmin = n + 1;
#pragma unroll
                for (int k = 0; k < K; ++k) {   // by the timestamps: q == p[k] happens either way
                    if (t <= last - sw.tb[k]) { ++p[k]; F[k] += fbit; }
                    pmin = p[k] < pmin ? p[k] : pmin;
                }
                if (n >= T && n - T >= pmin) bad |= kStTermRing;  // position n - T lost its slot
                ++n;
                ++late_rows;
                late_past += t <= last - sw.tb[0];  // a feature already emitted lacked the row
                return;
            }
        } else {
            if (n > 0 && t < last) bad |= kStOrder;
        }
        int64_t e[K];
#pragma unroll
        for (int k = 0; k < K; ++k) e[k] = p[k] < n ? ring[p[k] & mask] : INT64_MAX;
        int64_t pmin = n;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t bound = t - sw.tb[k];
            while ((e[k] >> 1) <= bound) {   // rows with ts <= t - boundary
                F[k] += e[k] & 1;
                ++p[k];
                e[k] = p[k] < n ? ring[p[k] & mask] : INT64_MAX;
            }
            pmin = p[k] < pmin ? p[k] : pmin;
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int32_t nb = (int32_t)(p[0] - p[w + 1]), fr = (int32_t)(F[0] - F[w + 1]);
            if (rec_out) {
                rec_out[(int64_t)row * W + w] = term_word(nb, fr);
            } else {
                double *x = X + (int64_t)row * ld + tcol0 + 2 * w;
                x[0] = (double)nb;
                x[1] = nb > 0 ? (double)fr / (double)nb : 0.0;  // fillna(0) of 0/0
            }
        }
        if (n >= T && n - T >= pmin) bad |= kStTermRing;
        ring[n & mask] = (int64_t)(((uint64_t)t << 1) | (fraud[row] ? 1u : 0u));
        ++n;
        last = t;
    });
    rec[0] = n;
    rec[1] = last;
#pragma unroll
    for (int k = 0; k < K; ++k) { rec[2 + 2 * k] = p[k]; rec[3 + 2 * k] = F[k]; }
    if (bad) atomicOr(status, bad);
    if constexpr (LATE) {
        if (late_rows) atomicAdd(la.counts, (unsigned long long)late_rows);
        if (late_past) atomicAdd(la.counts + 1, (unsigned long long)late_past);
    }
}

// LATE = false is the kernel of every state whose terminal lateness is 0 (the default): rows of
// a key that go back in time raise kStOrder.  LATE = true is launched only with a lateness > 0.
template <int W, bool LATE>
__global__ void __launch_bounds__(256) k_stream_process(
    const int64_t *__restrict__ ts, const int32_t *__restrict__ cust, const double *__restrict__ amount,
    const int32_t *__restrict__ term, const uint8_t *__restrict__ fraud, int64_t n, int64_t n_cust, int64_t n_term,
    StreamWin sw, int32_t *__restrict__ chead, const int32_t *__restrict__ cnext, int32_t *__restrict__ thead,
    const int32_t *__restrict__ tnext, int64_t *__restrict__ cstate, CEnt *__restrict__ cring, int32_t C,
    int64_t *__restrict__ tstate, int64_t *__restrict__ tring, int32_t T, double *__restrict__ X, int64_t ld,
    int32_t tcol0, int32_t *__restrict__ cnb_out, double *__restrict__ csum_out, int64_t *__restrict__ rec_out,
    int32_t *__restrict__ status, LateArgs<LATE> la) {
    // grid.y = 2 when both halves run: the customer and terminal keys of a row are walked by
    // different threads, so their dependent-load chains overlap instead of adding up
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool do_c = cust && (gridDim.y == 1 || blockIdx.y == 0);
    const bool do_t = term && (gridDim.y == 1 || blockIdx.y == 1);
    if (do_c) {
        const int32_t c = cust[i];
        if (c >= 0 && c < n_cust && chead[c] == (int32_t)i) {
            customer_key<W>(c, (int32_t)i, cnext, ts, amount, sw, cstate, cring, C, X, ld, cnb_out, csum_out, n,
                            status);
            chead[c] = -1;
        }
    }
    if (do_t) {
        const int32_t t = term[i];
        if (t >= 0 && t < n_term && thead[t] == (int32_t)i) {
            terminal_key<W, LATE>(t, (int32_t)i, tnext, ts, fraud, sw, tstate, tring, T, X, ld, tcol0, rec_out, status,
                                  la);
            thead[t] = -1;
        }
    }
}

// Delayed fraud reports (fdx_stream_report_frauds): "the transaction of this terminal at this
// ts was fraud", arriving after the row was pushed with its bit clear.  Chains built by
// k_stream_link (customer half null); the thread at a chain's head owns the terminal and
// visits its reports in (ts, row) order.
//
// Invariant: after a report the terminal's record and ring equal those of a stream that had
// the label on the row from the start.  F[k] counts the fraud bits of ring rows [0, p[k]); a
// row's bit is read only when p[k] steps over it, so setting the bit of row r and adding 1 to
// every F[k] with r < p[k] is exactly what those steps would have added.  A report that lands
// before p[0] (the delay boundary, the first pointer to move) passes the row changes no
// feature already emitted; one that lands after it is counted late.
// Only positive reports exist: a row starts as "not fraud" and there is no un-report.
enum : int { kLabOnTime = 0, kLabLate, kLabDuplicate, kLabExpired, kLabUnmatched, kLabCounters };

template <int W>
__global__ void __launch_bounds__(256) k_stream_labels(
    const int64_t *__restrict__ ts, const int32_t *__restrict__ term, int64_t n, int64_t n_term,
    int32_t *__restrict__ thead, const int32_t *__restrict__ tnext, int64_t *__restrict__ tstate,
    int64_t *__restrict__ tring, int32_t T, unsigned long long *__restrict__ counts) {
    constexpr int K = W + 1;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t tk = term[i];
    if (tk < 0 || tk >= n_term || thead[tk] != (int32_t)i) return;
    int64_t *rec = tstate + (int64_t)tk * (2 + 2 * K);
    int64_t *ring = tring + (int64_t)tk * T;
    const int64_t mask = T - 1;
    const int64_t nrows = rec[0];
    int64_t p[K], F[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] = rec[2 + 2 * k]; F[k] = rec[3 + 2 * k]; }
    // live ring positions [lo, nrows); non-decreasing in ts unless kStOrder was raised (then a
    // search may miss its row: unmatched, never out of bounds)
    int64_t lo = nrows > T ? nrows - T : 0;
    const int64_t oldest = lo < nrows ? ring[lo & mask] >> 1 : INT64_MAX;
    const bool evicted = nrows > T;
    int32_t on_time = 0, late = 0, dup = 0, expired = 0, unmatched = 0;
    chain_in_order((int32_t)i, tnext, ts, [&](int32_t, int64_t t) {
        int64_t a = lo, b = nrows;
        while (a < b) {  // first live row with ts >= t
            const int64_t mid = (a + b) >> 1;
            if ((ring[mid & mask] >> 1) < t) a = mid + 1; else b = mid;
        }
        lo = a;  // reports come in time order: the next search starts here
        bool tied = false, found = false;
        int64_t r = a, e = 0;
        for (; r < nrows; ++r) {  // among the rows tied on t, the first whose bit is clear
            e = ring[r & mask];
            if ((e >> 1) != t) break;
            tied = true;
            if (!(e & 1)) { found = true; break; }
        }
        if (found) {
            ring[r & mask] = e | 1;
#pragma unroll
            for (int k = 0; k < K; ++k) F[k] += r < p[k] ? 1 : 0;
        }
        // expired: the row left the ring; without ring overflow every pointer had passed it, so
        // no difference F[0] - F[w + 1] a later row sees would change: nothing is written
        const bool in_time = found && r >= p[0], gone = !tied && evicted && t < oldest;
        on_time += in_time;
        late += found && !in_time;
        dup += tied && !found;
        expired += gone;
        unmatched += !tied && !gone;
    });
#pragma unroll
    for (int k = 0; k < K; ++k) rec[3 + 2 * k] = F[k];
    thead[tk] = -1;
    if (on_time) atomicAdd(counts + kLabOnTime, (unsigned long long)on_time);
    if (late) atomicAdd(counts + kLabLate, (unsigned long long)late);
    if (dup) atomicAdd(counts + kLabDuplicate, (unsigned long long)dup);
    if (expired) atomicAdd(counts + kLabExpired, (unsigned long long)expired);
    if (unmatched) atomicAdd(counts + kLabUnmatched, (unsigned long long)unmatched);
}

bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

}  // namespace
}  // namespace fdx

using namespace fdx;

struct fdx_stream_s {
    int64_t n_cust = 0, n_term = 0, max_batch = 0;
    int32_t C = 0, T = 0, W = 0, mode = 0;
    StreamWin sw{};
    CEnt *cring_d = nullptr;
    int64_t *cstate_d = nullptr, *tring_d = nullptr, *tstate_d = nullptr;
    int32_t *chead_d = nullptr, *thead_d = nullptr, *cnext_d = nullptr, *tnext_d = nullptr, *status_d = nullptr;
    unsigned long long *labels_d = nullptr;  // kLabCounters report outcomes since create / reset
    unsigned long long *late_d = nullptr;    // {late_rows, late_past_delay} since create / reset
    int64_t max_late = 0;                    // terminal lateness (ns); 0: rows must not go back in time
    bool restored = false;                   // a restore wrote keys since create / reset (LateArgs::strict)
    size_t bytes = 0;
};

namespace {
size_t cust_rec_bytes(int W) { return (size_t)(2 + 6 * W) * 8; }
size_t term_rec_bytes(int W) { return (size_t)(2 + 2 * (W + 1)) * 8; }
}  // namespace

extern "C" int fdx_stream_destroy(fdx_stream s) {
    if (!s) return FDX_OK;
    (void)hipFree(s->cring_d);
    (void)hipFree(s->cstate_d);
    (void)hipFree(s->tring_d);
    (void)hipFree(s->tstate_d);
    (void)hipFree(s->chead_d);
    (void)hipFree(s->thead_d);
    (void)hipFree(s->cnext_d);
    (void)hipFree(s->tnext_d);
    (void)hipFree(s->status_d);
    (void)hipFree(s->labels_d);
    (void)hipFree(s->late_d);
    delete s;
    return FDX_OK;
}

extern "C" int fdx_stream_reset(fdx_stream s, void *stream) {
    FDX_REQUIRE(s, "null stream state");
    hipStream_t st = as_stream(stream);
    if (s->n_cust) {
        FDX_HIP(hipMemsetAsync(s->cstate_d, 0, (size_t)s->n_cust * cust_rec_bytes(s->W), st));
        FDX_HIP(hipMemsetAsync(s->chead_d, 0xFF, (size_t)s->n_cust * 4, st));
    }
    if (s->n_term) {
        FDX_HIP(hipMemsetAsync(s->tstate_d, 0, (size_t)s->n_term * term_rec_bytes(s->W), st));
        FDX_HIP(hipMemsetAsync(s->thead_d, 0xFF, (size_t)s->n_term * 4, st));
    }
    FDX_HIP(hipMemsetAsync(s->status_d, 0, 4, st));
    FDX_HIP(hipMemsetAsync(s->labels_d, 0, kLabCounters * 8, st));
    FDX_HIP(hipMemsetAsync(s->late_d, 0, 2 * 8, st));
    s->restored = false;
    return FDX_OK;
}

extern "C" int fdx_stream_create(int64_t n_customers, int64_t n_terminals, int32_t customer_ring,
                                 int32_t terminal_ring, int32_t n_windows, const int64_t *window_ns,
                                 int64_t delay_ns, int32_t flags_mode, int64_t max_batch, fdx_stream *out,
                                 void *stream) {
    FDX_REQUIRE(out, "null pointer");
    *out = nullptr;
    FDX_REQUIRE(n_customers >= 0 && n_customers <= INT32_MAX && n_terminals >= 0 && n_terminals <= INT32_MAX,
                "key capacity out of range");
    FDX_REQUIRE(n_windows >= 1 && n_windows <= kMaxW && window_ns, "n_windows must be in [1, %d]", kMaxW);
    FDX_REQUIRE(!n_customers || pow2(customer_ring), "customer_ring must be a power of two");
    FDX_REQUIRE(!n_terminals || pow2(terminal_ring), "terminal_ring must be a power of two");
    FDX_REQUIRE(max_batch >= 1 && max_batch <= INT32_MAX, "max_batch out of range");
    FDX_REQUIRE(delay_ns >= 0, "negative delay");
    FDX_REQUIRE(flags_mode == FDX_FLAGS_NOTEBOOK || flags_mode == FDX_FLAGS_SPARK, "bad flags mode");
    fdx_stream s = new fdx_stream_s;
    s->n_cust = n_customers; s->n_term = n_terminals; s->max_batch = max_batch;
    s->C = n_customers ? customer_ring : 0; s->T = n_terminals ? terminal_ring : 0;
    s->W = n_windows; s->mode = flags_mode;
    s->sw.tb[0] = delay_ns;
    for (int w = 0; w < n_windows; ++w) {
        if (window_ns[w] <= 0) {
            delete s;
            FDX_REQUIRE(false, "window lengths must be positive");
        }
        s->sw.win[w] = window_ns[w];
        s->sw.tb[w + 1] = delay_ns + window_ns[w];
    }
    auto alloc = [&](void **p, size_t b) -> hipError_t {
        s->bytes += b;
        return b ? hipMalloc(p, b) : hipSuccess;
    };
    hipError_t e = hipSuccess;
    const size_t nc = (size_t)n_customers, nt = (size_t)n_terminals;
    if ((e = alloc((void **)&s->cring_d, nc * s->C * sizeof(CEnt))) ||
        (e = alloc((void **)&s->cstate_d, nc * cust_rec_bytes(n_windows))) ||
        (e = alloc((void **)&s->chead_d, nc * 4)) ||
        (e = alloc((void **)&s->tring_d, nt * s->T * 8)) ||
        (e = alloc((void **)&s->tstate_d, nt * term_rec_bytes(n_windows))) ||
        (e = alloc((void **)&s->thead_d, nt * 4)) ||
        (e = alloc((void **)&s->cnext_d, (size_t)max_batch * 4)) ||
        (e = alloc((void **)&s->tnext_d, (size_t)max_batch * 4)) || (e = alloc((void **)&s->status_d, 4)) ||
        (e = alloc((void **)&s->labels_d, kLabCounters * 8)) || (e = alloc((void **)&s->late_d, 2 * 8))) {
        set_error("hipMalloc of the stream state (%zu bytes so far) failed: %s", s->bytes, hipGetErrorString(e));
        fdx_stream_destroy(s);
        return FDX_E_HIP;
    }
    const int rc = fdx_stream_reset(s, stream);
    if (rc) {
        fdx_stream_destroy(s);
        return rc;
    }
    *out = s;
    return FDX_OK;
}

extern "C" int fdx_stream_memory(fdx_stream s, size_t *bytes) {
    FDX_REQUIRE(s && bytes, "null pointer");
    *bytes = s->bytes;
    return FDX_OK;
}

#define FDX_STREAM_LAUNCH(WW, LATE, LA)                                                                          \
    hipLaunchKernelGGL((k_stream_process<WW, LATE>), grid, dim3(256), 0, st, ts_d, cust_d, amount_d, term_d,     \
                       fraud_d, n, s->n_cust, s->n_term, s->sw, s->chead_d, s->cnext_d, s->thead_d, s->tnext_d,  \
                       s->cstate_d, s->cring_d, s->C, s->tstate_d, s->tring_d, s->T, X_d, ld, tcol, cust_nb_d,   \
                       cust_sum_d, term_rec_d, s->status_d, LA)
#define FDX_STREAM_PROCESS(WW)                                                                                   \
    case WW:                                                                                                     \
        if (late) {                                                                                              \
            FDX_STREAM_LAUNCH(WW, true, la);                                                                     \
        } else {                                                                                                 \
            FDX_STREAM_LAUNCH(WW, false, LateArgs<false>{});                                                     \
        }                                                                                                        \
        break;

extern "C" int fdx_stream_update(fdx_stream s, const int64_t *ts_d, const int32_t *cust_d, const double *amount_d,
                                 const int32_t *term_d, const uint8_t *fraud_d, int64_t n, double *X_d, int64_t ld,
                                 int32_t term_col0, int32_t *cust_nb_d, double *cust_sum_d, int64_t *term_rec_d,
                                 void *stream) {
    FDX_REQUIRE(s, "null stream state");
    FDX_REQUIRE(n >= 0 && n <= s->max_batch, "batch of %lld rows exceeds max_batch %lld", (long long)n,
                (long long)s->max_batch);
    if (n == 0) return FDX_OK;
    FDX_REQUIRE(ts_d, "null ts");
    FDX_REQUIRE(!cust_d || (amount_d && s->n_cust), "customer half needs amounts and customer state");
    FDX_REQUIRE(!term_d || (fraud_d && s->n_term), "terminal half needs fraud labels and terminal state");
    const int W = s->W;
    const int32_t tcol = term_col0 < 0 ? 3 + 2 * W : term_col0;
    FDX_REQUIRE(!cust_nb_d == !cust_sum_d, "cust_nb_d and cust_sum_d go together");
    FDX_REQUIRE(!cust_d || cust_nb_d || (X_d && ld >= 3 + 2 * W), "X needs ld >= 3 + 2 * n_windows");
    FDX_REQUIRE(!X_d || ld >= 3, "X needs ld >= 3");
    FDX_REQUIRE(!term_d || term_rec_d || (X_d && ld >= tcol + 2 * W), "terminal columns do not fit ld");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_stream_link, dim3(stream_grid(n, 256)), dim3(256), 0, st, ts_d, cust_d, amount_d, term_d, n,
                       s->n_cust, s->n_term, s->chead_d, s->cnext_d, s->thead_d, s->tnext_d, s->mode, X_d, ld,
                       s->status_d);
    FDX_LAUNCHED("k_stream_link");
    const dim3 grid((unsigned)ceil_div(n, 256), cust_d && term_d ? 2u : 1u);
    const bool late = term_d && s->max_late > 0;
    const LateArgs<true> la{s->max_late, s->restored ? 1 : 0, s->late_d};
    switch (W) {
        FDX_STREAM_PROCESS(1)
        FDX_STREAM_PROCESS(2)
        FDX_STREAM_PROCESS(3)
        FDX_STREAM_PROCESS(4)
        FDX_STREAM_PROCESS(5)
        FDX_STREAM_PROCESS(6)
        FDX_STREAM_PROCESS(7)
        FDX_STREAM_PROCESS(8)
    }
    FDX_LAUNCHED("k_stream_process");
    return FDX_OK;
}

#define FDX_STREAM_LABELS(WW)                                                                                    \
    case WW:                                                                                                     \
        hipLaunchKernelGGL(k_stream_labels<WW>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, ts_d, term_d, \
                           n, s->n_term, s->thead_d, s->tnext_d, s->tstate_d, s->tring_d, s->T, s->labels_d);     \
        break;

extern "C" int fdx_stream_report_frauds(fdx_stream s, const int64_t *ts_d, const int32_t *term_d, int64_t n,
                                        void *stream) {
    FDX_REQUIRE(s, "null stream state");
    FDX_REQUIRE(n >= 0 && n <= s->max_batch, "batch of %lld reports exceeds max_batch %lld", (long long)n,
                (long long)s->max_batch);
    if (n == 0) return FDX_OK;
    FDX_REQUIRE(ts_d && term_d, "null ts or terminal");
    FDX_REQUIRE(s->n_term, "fraud reports need terminal state");
    hipStream_t st = as_stream(stream);
    // terminal chains only (customer half null): flags an id out of range, writes no X
    hipLaunchKernelGGL(k_stream_link, dim3(stream_grid(n, 256)), dim3(256), 0, st, ts_d, (const int32_t *)nullptr,
                       (const double *)nullptr, term_d, n, s->n_cust, s->n_term, s->chead_d, s->cnext_d, s->thead_d,
                       s->tnext_d, s->mode, (double *)nullptr, (int64_t)0, s->status_d);
    FDX_LAUNCHED("k_stream_link");
    switch (s->W) {
        FDX_STREAM_LABELS(1)
        FDX_STREAM_LABELS(2)
        FDX_STREAM_LABELS(3)
        FDX_STREAM_LABELS(4)
        FDX_STREAM_LABELS(5)
        FDX_STREAM_LABELS(6)
        FDX_STREAM_LABELS(7)
        FDX_STREAM_LABELS(8)
    }
    FDX_LAUNCHED("k_stream_labels");
    return FDX_OK;
}

extern "C" int fdx_stream_label_counts(fdx_stream s, int64_t counts_h[5], void *stream) {
    FDX_REQUIRE(s && counts_h, "null pointer");
    static_assert(kLabCounters == 5, "fdx.h documents five counters");
    hipStream_t st = as_stream(stream);
    FDX_HIP(hipMemcpyAsync(counts_h, s->labels_d, kLabCounters * 8, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    return FDX_OK;
}

extern "C" int fdx_stream_set_terminal_lateness(fdx_stream s, int64_t max_late_ns) {
    FDX_REQUIRE(s, "null stream state");
    FDX_REQUIRE(max_late_ns >= 0, "negative terminal lateness");
    s->max_late = max_late_ns;
    return FDX_OK;
}

extern "C" int fdx_stream_late_counts(fdx_stream s, int64_t counts_h[2], void *stream) {
    FDX_REQUIRE(s && counts_h, "null pointer");
    hipStream_t st = as_stream(stream);
    FDX_HIP(hipMemcpyAsync(counts_h, s->late_d, 2 * 8, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    return FDX_OK;
}

extern "C" int fdx_stream_status(fdx_stream s, int32_t *flags_h, void *stream) {
    FDX_REQUIRE(s && flags_h, "null pointer");
    hipStream_t st = as_stream(stream);
    FDX_HIP(hipMemcpyAsync(flags_h, s->status_d, 4, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    if (*flags_h) FDX_HIP(hipMemsetAsync(s->status_d, 0, 4, st));
    return FDX_OK;
}

extern "C" int fdx_stream_status_async(fdx_stream s, int32_t *flags_pinned_h, void *stream) {
    FDX_REQUIRE(s && flags_pinned_h, "null pointer");
    FDX_HIP(hipMemcpyAsync(flags_pinned_h, s->status_d, 4, hipMemcpyDeviceToHost, as_stream(stream)));
    return FDX_OK;
}


// ---------------------------------------------------------------- snapshot / restore (f-7)
// The live state as one flat, self-describing buffer of little-endian 8-byte words (format:
// include/fdx.h).  Per key only the LIVE rows travel: ring positions [min pointer, n), where
// the pointers are the customer's tail[w] resp. the terminal's p[k].  A row before every
// pointer has left every window and cannot re-enter one (a key's time does not go back), so
// the update kernels never read it again; n and the pointers are rebased to the first carried
// row, every other word (last_ts, the Kahan words, nobs | nsame << 32, F[k] -- only differences
// of F are used) keeps its value.  The bytes do not depend on the source's ring size, so a
// snapshot restores into any ring that holds the longest live run and any key capacity.
//
//   k_snap_count     8 lanes per selected key: live count -> u32 array (then the exclusive
//                    scan of fdx_rekey.hip gives the entry offsets), max and 64-bit sum
//   k_snap_pack      a group of 2^gshift lanes per key: record words (rebased) and the live
//                    rows, consecutive lanes on consecutive ring entries -- a key's rows are
//                    one or two contiguous runs of its ring, and rings sit ring * 16 B apart,
//                    so one thread per key would touch 64 different rows per wave
//   k_snap_header    the 64 header words, the closing offset of both halves, zero padding
//   k_snap_validate  restore, pass 1: one thread per key checks offsets and pointers and that
//                    the live count fits the destination ring; reads only inside the sections
//                    whose sizes the host checked against the byte count
//   k_snap_unpack    restore, pass 2 (only after pass 1 came back clean): group per key
// Bandwidth-bound copies through vector loads / stores; no LDS.
namespace fdx {
namespace {

constexpr uint64_t kSnapMagic = 0x3150414E53584446ull;  // the bytes "FDXSNAP1"
constexpr int kSnapVersion = 1;
enum : int {  // header word indices (include/fdx.h)
    kHMagic = 0, kHVersion, kHBytes, kHWindows, kHWin0,
    kHDelay = kHWin0 + kMaxW, kHMode, kHCRing, kHTRing,
    kHCKeys, kHCEntries, kHCMaxLive, kHTKeys, kHTEntries, kHTMaxLive,
    kHLabels, kHOff = kHLabels + kLabCounters, kHUsed = kHOff + 6, kHWords = 64
};
static_assert(kHWords * 8 == FDX_SNAPSHOT_HEADER_BYTES && kHUsed <= kHWords && kHDelay == 12 && kHOff == 27,
              "fdx.h documents the header words");

struct SnapHeader { int64_t w[kHWords]; };

// device-side results of the count / validate passes (zeroed, resp. preset, before each pass)
struct SnapRes {
    unsigned long long total[2], max_live[2];  // [0] customers, [1] terminals
    unsigned long long small[2];               // validate: min over keys of (key << 32 | live) that do not fit
    uint32_t bad, pad;                         // count: bit h = half h inconsistent; validate: malformed
};

struct Sel { int64_t first, count, step; };

struct Half {  // what the generic kernels need to know about one half
    int64_t *state;
    void *ring;
    int64_t n_keys;
    int32_t R, pstride, np, ring_len;  // record words; pointers at words 2 + k * pstride, k < np
};

uint64_t round16(uint64_t b) { return (b + 15) & ~(uint64_t)15; }

// Section offsets of the canonical layout; counts already range-checked (keys <= INT32_MAX,
// entries < 2^32), so nothing overflows 64 bits.
void snap_layout(int W, uint64_t ck, uint64_t ce, uint64_t tk, uint64_t te, uint64_t off[6], uint64_t *total) {
    uint64_t o = (uint64_t)kHWords * 8;
    off[0] = o; o += ck * cust_rec_bytes(W);
    off[1] = o; o += round16((ck + 1) * 8);
    off[2] = o; o += ce * sizeof(CEnt);
    off[3] = o; o += tk * term_rec_bytes(W);
    off[4] = o; o += round16((tk + 1) * 8);
    off[5] = o; o += round16(te * 8);
    *total = o;
}

// n and lo = min(n, pointers) of one record, read by a group of G = 2^k lanes with consecutive
// lanes on consecutive words (one thread per record would put 64 lanes on 64 records 80-160 B
// apart and wait for its pointer loads one after the other: 570 us per launch at config 5).
// Every lane of the group gets both.  Pointers sit at words 2 + k * pstride, all of them below R.
__device__ __forceinline__ bool snap_rebased(int32_t i, int32_t pstride) {
    return i == 0 || (i >= 2 && (i - 2) % pstride == 0);
}
__device__ __forceinline__ void group_live_range(const int64_t *__restrict__ rec, int32_t R, int32_t pstride,
                                                 int32_t lane, int32_t G, int64_t &n, int64_t &lo) {
    int64_t m = INT64_MAX, n0 = 0;
    for (int32_t i = lane; i < R; i += G) {
        const int64_t v = rec[i];
        if (i == 0) n0 = v;
        if (snap_rebased(i, pstride)) m = imin64(m, v);
    }
    for (int32_t d = G >> 1; d >= 1; d >>= 1) m = imin64(m, __shfl_xor(m, d, G));
    n = __shfl(n0, 0, G);
    lo = m;
}

constexpr int kCountShift = 3;  // k_snap_count: 8 lanes per key

__global__ void __launch_bounds__(256) k_snap_count(const int64_t *__restrict__ state, int32_t R, int32_t pstride,
                                                    int64_t ring, Sel sel, uint32_t *__restrict__ cnt,
                                                    SnapRes *__restrict__ res, int32_t half) {
    constexpr int32_t G = 1 << kCountShift;
    const int32_t lane = (int32_t)threadIdx.x & (G - 1);
    const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> kCountShift;
    // Grid-stride over the keys, so that a wave ends in ONE set of atomics on the result words:
    // with a wave per 64 keys (47k waves at config 5) the launch took 570 us, with a wave per 8
    // keys 4.4 ms -- the same-address atomics, not the loads, were its time.
    unsigned long long sum = 0, mx = 0;
    uint32_t bad = 0;
    for (int64_t j = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> kCountShift; j <= sel.count; j += groups) {
        unsigned long long live = 0;
        if (j < sel.count) {  // the whole group or none of it
            int64_t n, lo;
            group_live_range(state + (sel.first + j * sel.step) * R, R, pstride, lane, G, n, lo);
            int64_t l = n - lo;
            // a consistent state has 0 <= lo, one live row when n >= 1, and the live rows in the ring
            if (lo < 0 || l > ring || (n > 0 && l < 1)) {
                bad = 1u << half;
                l = 0;
            }
            live = (unsigned long long)l;
        }
        if (lane == 0) {  // j == count: cnt[count] = 0 closes the scan
            cnt[j] = (uint32_t)live;
            sum += live;
            mx = live > mx ? live : mx;
        }
    }
#pragma unroll
    for (int d = kWave / 2; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d, kWave);
        const unsigned long long o = __shfl_xor(mx, d, kWave);
        mx = o > mx ? o : mx;
        bad |= __shfl_xor(bad, d, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (sum) atomicAdd(&res->total[half], sum);
        if (mx) atomicMax(&res->max_live[half], mx);
        if (bad) atomicOr(&res->bad, bad);
    }
}

template <class E>
__global__ void __launch_bounds__(256) k_snap_pack(const int64_t *__restrict__ state, const E *__restrict__ rings,
                                                   int32_t R, int32_t pstride, int64_t ring, Sel sel,
                                                   const uint32_t *__restrict__ off, int64_t *__restrict__ out_rec,
                                                   int64_t *__restrict__ out_off, E *__restrict__ out_ent,
                                                   int32_t gshift) {
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> gshift;
    if (g >= sel.count) return;  // the whole group or none of it
    const int32_t G = 1 << gshift, lane = (int32_t)threadIdx.x & (G - 1);
    const int64_t key = sel.first + g * sel.step;
    const int64_t *rec = state + key * R;
    // the entry range comes from the count pass, so the writes stay inside what the host sized
    const int64_t o = off[g], live = (int64_t)off[g + 1] - o;
    int64_t n, lo;
    group_live_range(rec, R, pstride, lane, G, n, lo);
    for (int32_t i = lane; i < R; i += G)  // (the words again, from cache) n and the pointers: rebased
        out_rec[g * R + i] = rec[i] - (snap_rebased(i, pstride) ? lo : 0);
    if (lane == 0) out_off[g] = o;
    const E *rg = rings + key * ring;
    const int64_t mask = ring - 1;
#pragma unroll 4
    for (int64_t i = lane; i < live; i += G) out_ent[o + i] = rg[(lo + i) & mask];
}

struct SnapTail {  // words k_snap_header writes besides the header: closing offsets, zero padding
    int64_t word[5], value[5];
    int32_t n;
};

__global__ void __launch_bounds__(64) k_snap_header(int64_t *__restrict__ dst, SnapHeader h, SnapTail t,
                                                   const unsigned long long *__restrict__ labels) {
    const int i = threadIdx.x;
    int64_t v = h.w[i];
    if (i >= kHLabels && i < kHLabels + kLabCounters) v = (int64_t)labels[i - kHLabels];
    dst[i] = v;
    if (i < t.n) dst[t.word[i]] = t.value[i];
}

__global__ void __launch_bounds__(256) k_snap_validate(const int64_t *__restrict__ rec_d, const int64_t *__restrict__ off,
                                                       int32_t R, int32_t pstride, int32_t np, int64_t keys,
                                                       int64_t entries, int64_t ring, SnapRes *__restrict__ res,
                                                       int32_t half) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= keys) return;
    const int64_t o0 = off[j], o1 = off[j + 1];
    const int64_t *rec = rec_d + j * R;
    const int64_t n = rec[0];
    bool bad = o0 < 0 || o1 < o0 || o1 > entries || (j == 0 && o0 != 0) || (j == keys - 1 && o1 != entries) ||
               n != o1 - o0;
    for (int k = 0; k < np; ++k) {
        const int64_t p = rec[2 + k * pstride];
        bad |= p < 0 || p > n;
    }
    if (bad) {
        atomicOr(&res->bad, 1u << half);
    } else if (n > ring) {
        const unsigned long long c = n > 0xFFFFFFFFll ? 0xFFFFFFFFull : (unsigned long long)n;
        atomicMin(&res->small[half], ((unsigned long long)j << 32) | c);
    }
}

template <class E>
__global__ void __launch_bounds__(256) k_snap_unpack(const int64_t *__restrict__ rec_d, const int64_t *__restrict__ off,
                                                     const E *__restrict__ ent, int32_t R, int64_t keys, int64_t first,
                                                     int64_t step, int64_t ring, int64_t *__restrict__ state,
                                                     E *__restrict__ rings, int32_t gshift) {
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> gshift;
    if (g >= keys) return;
    const int32_t G = 1 << gshift, lane = (int32_t)threadIdx.x & (G - 1);
    const int64_t key = first + g * step;
    for (int32_t i = lane; i < R; i += G) state[key * R + i] = rec_d[g * R + i];
    // validated: 0 <= off[g] <= off[g + 1] <= entries and off[g + 1] - off[g] <= ring
    const int64_t o = off[g], live = off[g + 1] - o;
    E *rg = rings + key * ring;
#pragma unroll 4
    for (int64_t i = lane; i < live; i += G) rg[i] = ent[o + i];
}

__global__ void __launch_bounds__(64) k_snap_add_labels(unsigned long long *__restrict__ labels, SnapHeader h) {
    if (threadIdx.x < kLabCounters) labels[threadIdx.x] += (unsigned long long)h.w[kHLabels + threadIdx.x];
}


// Lanes per key: 16, the fastest of 4 .. 64 at config 5 (58 live rows per customer on average,
// 160 at most: profiles/stream_snapshot.json; a group covering the longest run, 64, was the
// slowest); narrower, down to 4, when no key has that many live rows.  FDX_SNAP_GROUP overrides
// it for that measurement.
int32_t snap_gshift(int64_t max_live) {
    if (const char *e = getenv("FDX_SNAP_GROUP")) {
        const int g = atoi(e);
        for (int sh = 0; sh <= 6; ++sh)
            if (g == (1 << sh)) return sh;
    }
    int32_t sh = 2;
    while (sh < 4 && (1ll << sh) < max_live) ++sh;
    return sh;
}

unsigned group_grid(int64_t keys, int32_t gshift) { return (unsigned)ceil_div(keys << gshift, 256); }

Half cust_half(fdx_stream s) {
    return Half{s->cstate_d, s->cring_d, s->n_cust, 2 + 6 * s->W, 6, s->W, s->C};
}
Half term_half(fdx_stream s) {
    return Half{s->tstate_d, s->tring_d, s->n_term, 4 + 2 * s->W, 2, s->W + 1, s->T};
}

struct SnapWs {
    SnapRes *res;
    uint32_t *cnt[2];
    void *scan;
};

SnapWs snap_ws(fdx_stream s, void *ws) {
    char *p = reinterpret_cast<char *>(ws);
    SnapWs w;
    w.res = reinterpret_cast<SnapRes *>(p);
    p += 256;
    w.cnt[0] = reinterpret_cast<uint32_t *>(p);
    p += al256((size_t)(s->n_cust + 1) * 4);
    w.cnt[1] = reinterpret_cast<uint32_t *>(p);
    p += al256((size_t)(s->n_term + 1) * 4);
    w.scan = p;
    return w;
}

int resolve_sel(const fdx_key_selection *in, int64_t n_keys, const char *what, Sel *out) {
    if (!in) {
        *out = Sel{0, n_keys, 1};
        return FDX_OK;
    }
    FDX_REQUIRE(in->first >= 0 && in->count >= 0 && in->step >= 1, "%s selection: first >= 0, count >= 0, step >= 1",
                what);
    FDX_REQUIRE(in->count == 0 || (in->first < n_keys && (in->count - 1) <= (n_keys - 1 - in->first) / in->step),
                "%s selection (%lld, %lld, %lld) leaves the state's %lld keys", what, (long long)in->first,
                (long long)in->count, (long long)in->step, (long long)n_keys);
    *out = Sel{in->first, in->count, in->step};
    return FDX_OK;
}

// The count pass of both halves; synchronises.  -> selections, totals and max_live on the host.
int snap_count(fdx_stream s, const fdx_key_selection *csel, const fdx_key_selection *tsel, void *ws_d, size_t ws_bytes,
               hipStream_t st, Sel sel[2], SnapRes *res_h) {
    FDX_REQUIRE(s, "null stream state");
    FDX_REQUIRE(ws_d && ws_bytes >= fdx_stream_snapshot_workspace_size(s), "workspace too small");
    int rc;
    if ((rc = resolve_sel(csel, s->n_cust, "customer", &sel[0]))) return rc;
    if ((rc = resolve_sel(tsel, s->n_term, "terminal", &sel[1]))) return rc;
    int32_t flags = 0;
    FDX_HIP(hipMemcpyAsync(&flags, s->status_d, 4, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    if (flags) {  // left set: the caller's fdx_stream_status still reports it
        set_error("the stream state carries status bits %d (fdx_stream_status): not worth saving", flags);
        return FDX_E_UNSUPPORTED;
    }
    const SnapWs w = snap_ws(s, ws_d);
    FDX_HIP(hipMemsetAsync(w.res, 0, sizeof(SnapRes), st));
    const Half h[2] = {cust_half(s), term_half(s)};
    for (int i = 0; i < 2; ++i) {
        hipLaunchKernelGGL(k_snap_count, dim3(stream_grid((sel[i].count + 1) << kCountShift, 256, 1024)), dim3(256), 0, st, h[i].state,
                           h[i].R, h[i].pstride, (int64_t)h[i].ring_len, sel[i], w.cnt[i], w.res, i);
        FDX_LAUNCHED("k_snap_count");
        if ((rc = fdx_exclusive_scan_u32(w.cnt[i], sel[i].count + 1, w.scan, st))) return rc;
    }
    FDX_HIP(hipMemcpyAsync(res_h, w.res, sizeof(SnapRes), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    if (res_h->bad) {
        set_error("the %s state is inconsistent (a ring overflowed earlier?): not worth saving",
                  res_h->bad & 1 ? "customer" : "terminal");
        return FDX_E_UNSUPPORTED;
    }
    FDX_REQUIRE(res_h->total[0] < (1ull << 32) && res_h->total[1] < (1ull << 32),
                "a half carries 2^32 or more ring entries: snapshot it in several key selections");
    return FDX_OK;
}

}  // namespace
}  // namespace fdx

extern "C" size_t fdx_stream_snapshot_workspace_size(fdx_stream s) {
    if (!s) return 0;
    const int64_t m = (s->n_cust > s->n_term ? s->n_cust : s->n_term) + 1;
    return 256 + al256((size_t)(s->n_cust + 1) * 4) + al256((size_t)(s->n_term + 1) * 4) +
           fdx_exclusive_scan_u32_workspace_size(m) + 256;
}

extern "C" int fdx_stream_snapshot_size(fdx_stream s, const fdx_key_selection *customers,
                                        const fdx_key_selection *terminals, size_t *bytes_h, void *workspace_d,
                                        size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(bytes_h, "null pointer");
    Sel sel[2];
    SnapRes r;
    const int rc = snap_count(s, customers, terminals, workspace_d, workspace_bytes, as_stream(stream), sel, &r);
    if (rc) return rc;
    uint64_t off[6], total;
    snap_layout(s->W, (uint64_t)sel[0].count, r.total[0], (uint64_t)sel[1].count, r.total[1], off, &total);
    *bytes_h = (size_t)total;
    return FDX_OK;
}

extern "C" int fdx_stream_snapshot(fdx_stream s, const fdx_key_selection *customers,
                                   const fdx_key_selection *terminals, void *snap_d, size_t snap_bytes,
                                   size_t *written_h, void *workspace_d, size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(snap_d && ((uintptr_t)snap_d & 15) == 0, "snap_d must be a 16-byte aligned device pointer");
    hipStream_t st = as_stream(stream);
    Sel sel[2];
    SnapRes r;
    const int rc = snap_count(s, customers, terminals, workspace_d, workspace_bytes, st, sel, &r);
    if (rc) return rc;
    uint64_t off[6], total;
    snap_layout(s->W, (uint64_t)sel[0].count, r.total[0], (uint64_t)sel[1].count, r.total[1], off, &total);
    FDX_REQUIRE(snap_bytes >= total, "snapshot buffer of %zu bytes, the snapshot needs %llu", snap_bytes,
                (unsigned long long)total);
    const SnapWs w = snap_ws(s, workspace_d);
    char *base = reinterpret_cast<char *>(snap_d);
    auto words = [&](int sec) { return reinterpret_cast<int64_t *>(base + off[sec]); };
    const Half hc = cust_half(s), ht = term_half(s);
    if (sel[0].count) {
        const int32_t sh = snap_gshift((int64_t)r.max_live[0]);
        hipLaunchKernelGGL(k_snap_pack<CEnt>, dim3(group_grid(sel[0].count, sh)), dim3(256), 0, st, hc.state,
                           s->cring_d, hc.R, hc.pstride, (int64_t)hc.ring_len, sel[0], w.cnt[0], words(0),
                           words(1), reinterpret_cast<CEnt *>(base + off[2]), sh);
        FDX_LAUNCHED("k_snap_pack");
    }
    if (sel[1].count) {
        const int32_t sh = snap_gshift((int64_t)r.max_live[1]);
        hipLaunchKernelGGL(k_snap_pack<int64_t>, dim3(group_grid(sel[1].count, sh)), dim3(256), 0, st, ht.state,
                           s->tring_d, ht.R, ht.pstride, (int64_t)ht.ring_len, sel[1], w.cnt[1], words(3),
                           words(4), words(5), sh);
        FDX_LAUNCHED("k_snap_pack");
    }
    SnapHeader h{};
    h.w[kHMagic] = (int64_t)kSnapMagic;
    h.w[kHVersion] = kSnapVersion;
    h.w[kHBytes] = (int64_t)total;
    h.w[kHWindows] = s->W;
    for (int i = 0; i < s->W; ++i) h.w[kHWin0 + i] = s->sw.win[i];
    h.w[kHDelay] = s->sw.tb[0];
    h.w[kHMode] = s->mode;
    h.w[kHCRing] = s->C;
    h.w[kHTRing] = s->T;
    h.w[kHCKeys] = sel[0].count; h.w[kHCEntries] = (int64_t)r.total[0]; h.w[kHCMaxLive] = (int64_t)r.max_live[0];
    h.w[kHTKeys] = sel[1].count; h.w[kHTEntries] = (int64_t)r.total[1]; h.w[kHTMaxLive] = (int64_t)r.max_live[1];
    for (int i = 0; i < 6; ++i) h.w[kHOff + i] = (int64_t)off[i];
    SnapTail t{};
    auto put = [&](uint64_t byte, int64_t v) { t.word[t.n] = (int64_t)(byte / 8); t.value[t.n++] = v; };
    put(off[1] + (uint64_t)sel[0].count * 8, (int64_t)r.total[0]);  // offsets[keys] = entries
    if (!(sel[0].count & 1)) put(off[1] + (uint64_t)(sel[0].count + 1) * 8, 0);
    put(off[4] + (uint64_t)sel[1].count * 8, (int64_t)r.total[1]);
    if (!(sel[1].count & 1)) put(off[4] + (uint64_t)(sel[1].count + 1) * 8, 0);
    if (r.total[1] & 1) put(off[5] + r.total[1] * 8, 0);
    hipLaunchKernelGGL(k_snap_header, dim3(1), dim3(kHWords), 0, st, reinterpret_cast<int64_t *>(base), h, t,
                       s->labels_d);
    FDX_LAUNCHED("k_snap_header");
    if (written_h) *written_h = (size_t)total;
    return FDX_OK;
}

extern "C" int fdx_stream_snapshot_info(const void *header_h, size_t bytes, fdx_snapshot_info *out) {
    FDX_REQUIRE(header_h && out, "null pointer");
    FDX_REQUIRE(bytes >= (size_t)kHWords * 8, "%zu bytes are less than a snapshot header", bytes);
    int64_t w[kHWords];
    memcpy(w, header_h, sizeof(w));
    FDX_REQUIRE((uint64_t)w[kHMagic] == kSnapMagic, "not a stream snapshot (magic)");
    FDX_REQUIRE(w[kHVersion] == kSnapVersion, "snapshot format version %lld, this library reads %d",
                (long long)w[kHVersion], kSnapVersion);
    FDX_REQUIRE(w[kHBytes] >= 0 && (uint64_t)w[kHBytes] <= bytes, "the snapshot says %lld bytes, %zu are here",
                (long long)w[kHBytes], bytes);
    FDX_REQUIRE(w[kHWindows] >= 1 && w[kHWindows] <= kMaxW, "snapshot n_windows %lld outside [1, %d]",
                (long long)w[kHWindows], kMaxW);
    FDX_REQUIRE(w[kHCKeys] >= 0 && w[kHCKeys] <= INT32_MAX && w[kHTKeys] >= 0 && w[kHTKeys] <= INT32_MAX &&
                    w[kHCEntries] >= 0 && w[kHCEntries] < (1ll << 32) && w[kHTEntries] >= 0 &&
                    w[kHTEntries] < (1ll << 32),
                "snapshot key or entry counts out of range");
    FDX_REQUIRE((w[kHCKeys] || !w[kHCEntries]) && (w[kHTKeys] || !w[kHTEntries]), "snapshot entries without keys");
    uint64_t off[6], total;
    snap_layout((int)w[kHWindows], (uint64_t)w[kHCKeys], (uint64_t)w[kHCEntries], (uint64_t)w[kHTKeys],
                (uint64_t)w[kHTEntries], off, &total);
    for (int i = 0; i < 6; ++i)
        FDX_REQUIRE((uint64_t)w[kHOff + i] == off[i], "snapshot section %d at byte %lld, the layout puts it at %llu", i,
                    (long long)w[kHOff + i], (unsigned long long)off[i]);
    FDX_REQUIRE((uint64_t)w[kHBytes] == total, "snapshot sections end at byte %llu, the header says %lld",
                (unsigned long long)total, (long long)w[kHBytes]);
    out->version = w[kHVersion];
    out->total_bytes = w[kHBytes];
    out->n_windows = w[kHWindows];
    for (int i = 0; i < kMaxW; ++i) out->window_ns[i] = w[kHWin0 + i];
    out->delay_ns = w[kHDelay];
    out->flags_mode = w[kHMode];
    out->customer_ring = w[kHCRing];
    out->terminal_ring = w[kHTRing];
    out->customer_keys = w[kHCKeys]; out->customer_entries = w[kHCEntries]; out->customer_max_live = w[kHCMaxLive];
    out->terminal_keys = w[kHTKeys]; out->terminal_entries = w[kHTEntries]; out->terminal_max_live = w[kHTMaxLive];
    for (int i = 0; i < kLabCounters; ++i) out->label_counts[i] = w[kHLabels + i];
    for (int i = 0; i < 6; ++i) out->section_offset[i] = w[kHOff + i];
    return FDX_OK;
}

extern "C" int fdx_stream_restore(fdx_stream s, const void *snap_d, size_t snap_bytes, int64_t customer_first,
                                  int64_t customer_step, int64_t terminal_first, int64_t terminal_step, int32_t flags,
                                  void *workspace_d, size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(s, "null stream state");
    FDX_REQUIRE(snap_d && ((uintptr_t)snap_d & 15) == 0, "snap_d must be a 16-byte aligned device pointer");
    FDX_REQUIRE((flags & ~FDX_RESTORE_COUNTERS) == 0, "unknown restore flags %d", flags);
    FDX_REQUIRE(workspace_d && workspace_bytes >= 256, "workspace too small");
    FDX_REQUIRE(snap_bytes >= (size_t)kHWords * 8, "%zu bytes are less than a snapshot header", snap_bytes);
    hipStream_t st = as_stream(stream);
    SnapHeader h;
    FDX_HIP(hipMemcpyAsync(h.w, snap_d, sizeof(h.w), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    fdx_snapshot_info f;
    const int rc = fdx_stream_snapshot_info(h.w, snap_bytes, &f);
    if (rc) return rc;
    FDX_REQUIRE(f.n_windows == s->W, "the snapshot has %lld windows, the state %d", (long long)f.n_windows, s->W);
    for (int i = 0; i < s->W; ++i)
        FDX_REQUIRE(f.window_ns[i] == s->sw.win[i], "window %d: the snapshot has %lld ns, the state %lld", i,
                    (long long)f.window_ns[i], (long long)s->sw.win[i]);
    FDX_REQUIRE(f.delay_ns == s->sw.tb[0], "delay: the snapshot has %lld ns, the state %lld", (long long)f.delay_ns,
                (long long)s->sw.tb[0]);
    const Half half[2] = {cust_half(s), term_half(s)};
    const int64_t keys[2] = {f.customer_keys, f.terminal_keys}, entries[2] = {f.customer_entries, f.terminal_entries};
    const int64_t first[2] = {customer_first, terminal_first}, step[2] = {customer_step, terminal_step};
    const int64_t max_live[2] = {f.customer_max_live, f.terminal_max_live};
    const char *name[2] = {"customer", "terminal"};
    for (int i = 0; i < 2; ++i) {
        if (!keys[i]) continue;
        FDX_REQUIRE(half[i].n_keys > 0, "the snapshot carries %s keys, the state has no %s half", name[i], name[i]);
        FDX_REQUIRE(first[i] >= 0 && step[i] >= 1, "%s placement: first >= 0, step >= 1", name[i]);
        FDX_REQUIRE(first[i] < half[i].n_keys && keys[i] - 1 <= (half[i].n_keys - 1 - first[i]) / step[i],
                    "%s key %lld + %lld * %lld is beyond the state's capacity %lld", name[i], (long long)first[i],
                    (long long)(keys[i] - 1), (long long)step[i], (long long)half[i].n_keys);
    }
    const char *base = reinterpret_cast<const char *>(snap_d);
    auto words = [&](int sec) { return reinterpret_cast<const int64_t *>(base + f.section_offset[sec]); };
    // pass 1, to completion before anything is written
    SnapRes *res_d = reinterpret_cast<SnapRes *>(workspace_d), r;
    memset(&r, 0, sizeof(r));
    r.small[0] = r.small[1] = ~0ull;
    FDX_HIP(hipMemcpyAsync(res_d, &r, sizeof(r), hipMemcpyHostToDevice, st));
    for (int i = 0; i < 2; ++i) {
        if (!keys[i]) continue;
        hipLaunchKernelGGL(k_snap_validate, dim3((unsigned)ceil_div(keys[i], 256)), dim3(256), 0, st, words(3 * i),
                           words(3 * i + 1), half[i].R, half[i].pstride, half[i].np, keys[i], entries[i],
                           (int64_t)half[i].ring_len, res_d, i);
        FDX_LAUNCHED("k_snap_validate");
    }
    FDX_HIP(hipMemcpyAsync(&r, res_d, sizeof(r), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    FDX_REQUIRE(!r.bad, "the snapshot's %s offsets or pointers are malformed", r.bad & 1 ? "customer" : "terminal");
    for (int i = 0; i < 2; ++i)
        FDX_REQUIRE(r.small[i] == ~0ull, "%s key %lld has %llu live rows, the state's %s ring holds %d", name[i],
                    (long long)(first[i] + (int64_t)(r.small[i] >> 32) * step[i]),
                    (unsigned long long)(r.small[i] & 0xFFFFFFFFull), name[i], half[i].ring_len);
    // pass 2
    s->restored = true;  // the carried rings start at min p[k]: late terminal rows take the strict rule
    if (keys[0]) {
        const int32_t sh = snap_gshift(max_live[0]);
        hipLaunchKernelGGL(k_snap_unpack<CEnt>, dim3(group_grid(keys[0], sh)), dim3(256), 0, st, words(0), words(1),
                           reinterpret_cast<const CEnt *>(base + f.section_offset[2]), half[0].R, keys[0], first[0],
                           step[0], (int64_t)s->C, s->cstate_d, s->cring_d, sh);
        FDX_LAUNCHED("k_snap_unpack");
    }
    if (keys[1]) {
        const int32_t sh = snap_gshift(max_live[1]);
        hipLaunchKernelGGL(k_snap_unpack<int64_t>, dim3(group_grid(keys[1], sh)), dim3(256), 0, st, words(3), words(4),
                           words(5), half[1].R, keys[1], first[1], step[1], (int64_t)s->T, s->tstate_d, s->tring_d, sh);
        FDX_LAUNCHED("k_snap_unpack");
    }
    if (flags & FDX_RESTORE_COUNTERS) {
        hipLaunchKernelGGL(k_snap_add_labels, dim3(1), dim3(64), 0, st, s->labels_d, h);
        FDX_LAUNCHED("k_snap_add_labels");
    }
    return FDX_OK;
}


// ---------------------------------------------------------------- retiring idle keys (f-10)
// A key whose last row lies a whole horizon (customers: the longest window; terminals: delay +
// the longest window) before every row still to come behaves exactly like a key never seen: the
// customer's windows all drain and RollSum::reset runs before the add, the terminal's pointers
// all reach n and every count difference is 0.  Such keys are dropped, the survivors renumbered
// by their rank (order kept), and the freed ids go back to the key directory (fdx_keydir_remap).
//
//   k_retire_mark     plan: one thread per key reads {n, last_ts} (one 16-byte load): alive flag
//                     -> u32 array, retired keys with rows counted; then the exclusive scan
//   k_retire_map      plan: map[id] = alive ? rank : -1; the survivor count
//   k_map_flag/check  apply (and fdx_keydir_remap): a caller's map is checked on the device --
//                     flags, scan, map[id] == -1 or == its rank -- before anything is written
//   k_retire_gather   apply: the records and whole rings of one chunk of ids -> workspace
//   k_retire_scatter  apply: workspace -> the new ids.  new(id) <= id and the map is monotone, so
//                     a chunk's destinations never lie above its own sources, but they may
//                     overlap sources of the SAME chunk: hence the staging, and chunk c's scatter
//                     is a launch before chunk c + 1's gather.  The ids below the first one that
//                     moves are skipped.
// Rings travel whole and verbatim: positions are r & mask of the absolute n, so the unchanged
// record with the unchanged ring is exact.  16 lanes per key on consecutive words / entries, as
// k_snap_pack.  Nothing a launch reads by plain loads was written in that launch; no LDS but the
// block scan that sums k_retire_mark's count.  Records and heads of [kept, capacity) are cleared
// as fdx_stream_reset clears them; their rings are unreachable while n == 0.
namespace fdx {
namespace {

constexpr int64_t kRetireChunk = 8192;  // keys staged per gather / scatter pair by default
constexpr int kMoveShift = 4;           // 16 lanes per key

struct RetRes {
    MapRes map[2];
    unsigned long long retired[2];  // plan: keys with n >= 1 that are retired
};
static_assert(sizeof(RetRes) <= 256, "the workspace's first 256 bytes");

__global__ void __launch_bounds__(256) k_retire_mark(const int64_t *__restrict__ state, int32_t R, int64_t n_keys,
                                                     int64_t cut, uint32_t *__restrict__ flag,
                                                     RetRes *__restrict__ res, int32_t half) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t alive = 0, dead = 0;
    if (i < n_keys) {
        const longlong2 w = *reinterpret_cast<const longlong2 *>(state + i * R);  // {n, last_ts}
        alive = w.x > 0 && w.y > cut;
        dead = w.x > 0 && !alive;
    }
    if (i <= n_keys) flag[i] = alive;  // flag[n_keys] = 0 closes the scan
    // one atomic per block: with one per wave the same-address atomics were the launch's time
    uint32_t tot;
    block_excl_scan<256 / kWave>(dead, &tot);
    if (threadIdx.x == 0 && tot) atomicAdd(&res->retired[half], (unsigned long long)tot);
}

__global__ void __launch_bounds__(256) k_retire_map(const uint32_t *__restrict__ rank, int64_t n_keys,
                                                    int32_t *__restrict__ map, RetRes *__restrict__ res,
                                                    int32_t half) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_keys) {
        const uint32_t r = rank[i];
        map[i] = rank[i + 1] != r ? (int32_t)r : -1;
    }
    if (i == 0) res->map[half].kept = rank[n_keys];
}

__global__ void __launch_bounds__(256) k_map_flag(const int32_t *__restrict__ map, int64_t n,
                                                  uint32_t *__restrict__ flag, MapRes *__restrict__ res) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flag[i] = i < n && map[i] >= 0;
    if (i == 0) *res = MapRes{0, (unsigned long long)n, 0, 0};
}

__global__ void __launch_bounds__(256) k_map_check(const int32_t *__restrict__ map, int64_t n,
                                                   const uint32_t *__restrict__ rank, MapRes *__restrict__ res) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int32_t v = map[i];
        if (v < 0 ? v != -1 : (uint32_t)v != rank[i]) atomicOr(&res->bad, 1u);
        // In a valid map every id from the first one that moves on differs from its entry (a
        // survivor's rank is below its id), so exactly one id differs while its predecessor does
        // not: a plain store by that thread, where an atomicMin by every moved id took 270 us per
        // launch over 2M ids.  (A malformed map may store several times: it is refused anyway.)
        if ((int64_t)v != i && (i == 0 || (int64_t)map[i - 1] == i - 1)) res->first = (unsigned long long)i;
    }
    if (i == 0) res->kept = rank[n];  // (no other thread of this launch touches the word)
}

template <class E>
__global__ void __launch_bounds__(256) k_retire_gather(const int64_t *__restrict__ state, const E *__restrict__ rings,
                                                       int32_t R, int64_t ring, const int32_t *__restrict__ map,
                                                       int64_t id0, int64_t m, int64_t *__restrict__ st_rec,
                                                       E *__restrict__ st_ent) {
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> kMoveShift;
    if (g >= m) return;  // the whole group or none of it
    constexpr int32_t G = 1 << kMoveShift;
    const int32_t lane = (int32_t)threadIdx.x & (G - 1);
    const int64_t id = id0 + g;
    if (map[id] < 0) return;
    for (int32_t i = lane; i < R; i += G) st_rec[g * R + i] = state[id * R + i];
    const E *src = rings + id * ring;
    E *dst = st_ent + g * ring;
#pragma unroll 4
    for (int64_t i = lane; i < ring; i += G) dst[i] = src[i];
}

template <class E>
__global__ void __launch_bounds__(256) k_retire_scatter(const int64_t *__restrict__ st_rec, const E *__restrict__ st_ent,
                                                        int32_t R, int64_t ring, const int32_t *__restrict__ map,
                                                        int64_t id0, int64_t m, int64_t *__restrict__ state,
                                                        E *__restrict__ rings) {
    const int64_t g = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> kMoveShift;
    if (g >= m) return;
    constexpr int32_t G = 1 << kMoveShift;
    const int32_t lane = (int32_t)threadIdx.x & (G - 1);
    const int64_t to = map[id0 + g];  // validated: -1 or a rank <= id0 + g
    if (to < 0) return;
    for (int32_t i = lane; i < R; i += G) state[to * R + i] = st_rec[g * R + i];
    const E *src = st_ent + g * ring;
    E *dst = rings + to * ring;
#pragma unroll 4
    for (int64_t i = lane; i < ring; i += G) dst[i] = src[i];
}

size_t half_key_bytes(const Half &h, size_t ent_bytes) { return (size_t)h.R * 8 + (size_t)h.ring_len * ent_bytes; }

struct RetWs {
    RetRes *res;
    uint32_t *flag;
    void *scan;
    char *stage;
    size_t fixed;  // bytes before the staging area
};

RetWs ret_ws(fdx_stream s, void *ws) {
    const int64_t m = (s->n_cust > s->n_term ? s->n_cust : s->n_term) + 1;
    char *p = reinterpret_cast<char *>(ws);
    RetWs w{};
    const size_t o_flag = 256, o_scan = o_flag + al256((size_t)m * 4);
    w.fixed = o_scan + al256(fdx_exclusive_scan_u32_workspace_size(m));
    w.res = reinterpret_cast<RetRes *>(p);
    if (!p) return w;  // the size query: only `fixed`
    w.flag = reinterpret_cast<uint32_t *>(p + o_flag);
    w.scan = p + o_scan;
    w.stage = p + w.fixed;
    return w;
}

size_t max_key_bytes(fdx_stream s) {
    const size_t c = s->n_cust ? half_key_bytes(cust_half(s), sizeof(CEnt)) : 0;
    const size_t t = s->n_term ? half_key_bytes(term_half(s), 8) : 0;
    return c > t ? c : t;
}

// t - h without signed overflow (h >= 0): saturates at INT64_MIN, where `last_ts <= cut` holds
// for no timestamp but INT64_MIN itself
int64_t sat_sub(int64_t t, int64_t h) { return t < INT64_MIN + h ? INT64_MIN : t - h; }

// the status word, read first (as the snapshot does): a set bit refuses and stays set
int retire_status(fdx_stream s, hipStream_t st) {
    int32_t flags = 0;
    FDX_HIP(hipMemcpyAsync(&flags, s->status_d, 4, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    if (flags) {
        set_error("the stream state carries status bits %d (fdx_stream_status): nothing retired", flags);
        return FDX_E_UNSUPPORTED;
    }
    return FDX_OK;
}

template <class E>
int retire_move(const Half &h, E *rings, const int32_t *map_d, int64_t first, int64_t kept, int32_t *head_d,
                char *stage, int64_t chunk, hipStream_t st) {
    int64_t *st_rec = reinterpret_cast<int64_t *>(stage);
    E *st_ent = reinterpret_cast<E *>(stage + (size_t)chunk * h.R * 8);  // R is even: 16-byte aligned
    for (int64_t id0 = first; id0 < h.n_keys; id0 += chunk) {
        const int64_t m = h.n_keys - id0 < chunk ? h.n_keys - id0 : chunk;
        const dim3 grid((unsigned)ceil_div(m << kMoveShift, 256));
        hipLaunchKernelGGL(k_retire_gather<E>, grid, dim3(256), 0, st, h.state, rings, h.R, (int64_t)h.ring_len,
                           map_d, id0, m, st_rec, st_ent);
        FDX_LAUNCHED("k_retire_gather");
        hipLaunchKernelGGL(k_retire_scatter<E>, grid, dim3(256), 0, st, st_rec, st_ent, h.R, (int64_t)h.ring_len,
                           map_d, id0, m, h.state, rings);
        FDX_LAUNCHED("k_retire_scatter");
    }
    if (kept < h.n_keys) {
        FDX_HIP(hipMemsetAsync(h.state + kept * h.R, 0, (size_t)(h.n_keys - kept) * h.R * 8, st));
        FDX_HIP(hipMemsetAsync(head_d + kept, 0xFF, (size_t)(h.n_keys - kept) * 4, st));
    }
    return FDX_OK;
}

}  // namespace

int map_validate(const int32_t *map_d, int64_t n, MapRes *res_d, uint32_t *flag_d, void *scan_ws_d, hipStream_t st) {
    const dim3 grid((unsigned)ceil_div(n + 1, 256));
    hipLaunchKernelGGL(k_map_flag, grid, dim3(256), 0, st, map_d, n, flag_d, res_d);
    FDX_LAUNCHED("k_map_flag");
    const int rc = fdx_exclusive_scan_u32(flag_d, n + 1, scan_ws_d, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_map_check, grid, dim3(256), 0, st, map_d, n, flag_d, res_d);
    FDX_LAUNCHED("k_map_check");
    return FDX_OK;
}

}  // namespace fdx

extern "C" size_t fdx_stream_retire_workspace_size(fdx_stream s, int64_t chunk_keys) {
    if (!s) return 0;
    const int64_t m = s->n_cust > s->n_term ? s->n_cust : s->n_term;
    int64_t chunk = chunk_keys > 0 ? chunk_keys : kRetireChunk;
    if (chunk > m) chunk = m;
    if (chunk < 1) chunk = 1;
    return ret_ws(s, nullptr).fixed + al256((size_t)chunk * max_key_bytes(s));
}

extern "C" int fdx_stream_retire_plan(fdx_stream s, int64_t watermark_ns, int32_t *cust_map_d, int32_t *term_map_d,
                                      int64_t counts_h[4], void *workspace_d, size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(s && counts_h, "null pointer");
    FDX_REQUIRE(workspace_d && workspace_bytes >= fdx_stream_retire_workspace_size(s, 1), "workspace too small");
    hipStream_t st = as_stream(stream);
    int rc;
    if ((rc = retire_status(s, st))) return rc;
    const RetWs w = ret_ws(s, workspace_d);
    FDX_HIP(hipMemsetAsync(w.res, 0, sizeof(RetRes), st));
    const Half h[2] = {cust_half(s), term_half(s)};
    int32_t *map[2] = {cust_map_d, term_map_d};
    int64_t cmax = 0;
    for (int i = 0; i < s->W; ++i) cmax = s->sw.win[i] > cmax ? s->sw.win[i] : cmax;
    // delay + the longest window, saturating (both are >= 0)
    const int64_t tmax = cmax > INT64_MAX - s->sw.tb[0] ? INT64_MAX : s->sw.tb[0] + cmax;
    const int64_t cut[2] = {sat_sub(watermark_ns, cmax), sat_sub(watermark_ns, tmax)};
    for (int i = 0; i < 2; ++i) {
        if (!map[i] || !h[i].n_keys) continue;
        const dim3 grid((unsigned)ceil_div(h[i].n_keys + 1, 256));
        hipLaunchKernelGGL(k_retire_mark, grid, dim3(256), 0, st, h[i].state, h[i].R, h[i].n_keys, cut[i], w.flag,
                           w.res, i);
        FDX_LAUNCHED("k_retire_mark");
        if ((rc = fdx_exclusive_scan_u32(w.flag, h[i].n_keys + 1, w.scan, st))) return rc;
        hipLaunchKernelGGL(k_retire_map, grid, dim3(256), 0, st, w.flag, h[i].n_keys, map[i], w.res, i);
        FDX_LAUNCHED("k_retire_map");
    }
    RetRes r;
    FDX_HIP(hipMemcpyAsync(&r, w.res, sizeof(r), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 2; ++i) {
        counts_h[2 * i] = (int64_t)r.map[i].kept;
        counts_h[2 * i + 1] = (int64_t)r.retired[i];
    }
    return FDX_OK;
}

extern "C" int fdx_stream_retire_apply(fdx_stream s, const int32_t *cust_map_d, int64_t cust_kept,
                                       const int32_t *term_map_d, int64_t term_kept, void *workspace_d,
                                       size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(s, "null stream state");
    FDX_REQUIRE(workspace_d && workspace_bytes >= fdx_stream_retire_workspace_size(s, 1), "workspace too small");
    const Half h[2] = {cust_half(s), term_half(s)};
    const int32_t *map[2] = {cust_map_d, term_map_d};
    const int64_t kept[2] = {cust_kept, term_kept};
    const char *name[2] = {"customer", "terminal"};
    for (int i = 0; i < 2; ++i) {
        if (!map[i]) continue;
        FDX_REQUIRE(h[i].n_keys > 0, "a %s map for a state without a %s half", name[i], name[i]);
        FDX_REQUIRE(kept[i] >= 0 && kept[i] <= h[i].n_keys, "%s kept %lld outside [0, %lld]", name[i],
                    (long long)kept[i], (long long)h[i].n_keys);
    }
    hipStream_t st = as_stream(stream);
    int rc;
    if ((rc = retire_status(s, st))) return rc;
    const RetWs w = ret_ws(s, workspace_d);
    // pass 1, to completion before anything is written
    for (int i = 0; i < 2; ++i)
        if (map[i] && (rc = map_validate(map[i], h[i].n_keys, &w.res->map[i], w.flag, w.scan, st))) return rc;
    RetRes r;
    FDX_HIP(hipMemcpyAsync(&r, w.res, sizeof(r), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < 2; ++i) {
        if (!map[i]) continue;
        FDX_REQUIRE(!r.map[i].bad, "the %s map is malformed: -1 or the rank among the survivors, in id order", name[i]);
        FDX_REQUIRE((int64_t)r.map[i].kept == kept[i], "the %s map keeps %lld keys, the call says %lld", name[i],
                    (long long)r.map[i].kept, (long long)kept[i]);
    }
    // pass 2
    const size_t avail = workspace_bytes - w.fixed;
    if (map[0]) {
        int64_t chunk = (int64_t)(avail / half_key_bytes(h[0], sizeof(CEnt)));
        chunk = chunk > h[0].n_keys ? h[0].n_keys : chunk;
        if ((rc = retire_move<CEnt>(h[0], s->cring_d, map[0], (int64_t)r.map[0].first, kept[0], s->chead_d, w.stage,
                                    chunk, st)))
            return rc;
    }
    if (map[1]) {
        int64_t chunk = (int64_t)(avail / half_key_bytes(h[1], 8));
        chunk = chunk > h[1].n_keys ? h[1].n_keys : chunk;
        if ((rc = retire_move<int64_t>(h[1], s->tring_d, map[1], (int64_t)r.map[1].first, kept[1], s->thead_d,
                                       w.stage, chunk, st)))
            return rc;
    }
    return FDX_OK;
}
