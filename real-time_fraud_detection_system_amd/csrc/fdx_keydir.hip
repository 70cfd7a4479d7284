// f-9: the device key directory -- raw int64 ids -> dense int32 state rows, in front of
// fdx_stream_update / fdx_stream_report_frauds (contract: include/fdx.h).
//
// An open-addressing table of 16-byte slots {key, id, first} (one aligned 16-byte load per
// probe step) plus the reverse map key_of[id].  A batch is mapped in PHASES THAT ARE KERNEL
// LAUNCHES, so no lane ever waits for another lane's store and there is no spin loop:
//   find    each row probes linearly.  A slot's key word changes only by atomicCAS(empty -> key);
//           a row that ends on a slot without an id leaves its row index there by atomicMin into
//           `first` and remembers the slot (slot_of).  Rows of keys that had an id before this
//           launch are finished here (plain loads only).
//   mark    flag[r] = the slot has no id and first == r: the first occurrence of a new key.
//   assign  id = held + (exclusive scan of the flags): first-occurrence order, whatever the
//           scheduling or the hash.  id < capacity: written to the slot, key_of[id] = key; else
//           the key is refused and `first` is reset.
//   read    ids[r] = the slot's id (-1 = refused), refused rows counted, the held count advanced
//           by one thread.
// Visibility: the XCD L2s are not coherent inside a launch, so words written in the same launch
// are read through atomics only (the CAS's return value, the atomicMin); everything else a phase
// reads was written by an EARLIER launch.  The find kernel's plain slot load may see a stale
// "empty" -- the CAS that follows tells the truth -- but a non-empty key it sees is final, because
// a key word never changes once set.  A batch of at most kTailRows rows runs mark + assign + read
// as ONE block (barriers between the phases; a block's own stores are visible to it).
//
// Probe bound: at most `slots` steps, by the loop's own counter; garbage keys cannot extend it.
// Once every id is taken the find kernel stops inserting (an unknown key is refused without a
// CAS), so refused keys enter the table only in the call that crosses the capacity, and a call
// is cut into chunks of at most min(capacity, kChunkRows) rows: a chunk claims at most
// held + chunk <= 2 * capacity <= slots slots, so a key that is due an id always finds a slot.
#include <algorithm>

#include "fdx_internal.h"

namespace fdx {
namespace {

struct alignas(16) KSlot {
    unsigned long long key;
    int32_t id;     // -1: none (claimed in this call, or refused)
    int32_t first;  // the smallest batch row waiting for this slot's id; kNoRow: none
};
static_assert(sizeof(KSlot) == 16, "one probe step = one 16-byte load");

constexpr unsigned long long kKeyEmpty = 0x8000000000000000ull;  // INT64_MIN: the reserved key
constexpr int32_t kNoRow = INT32_MAX;
constexpr int kBlock = 256, kTail = 1024;
constexpr int64_t kTailRows = kTail;       // <= this: mark + assign + read in one block
constexpr int64_t kChunkRows = 65536;      // <= 256 blocks per phase: the block counts are summed per block
enum { kHeld = 0, kFull = 1, kReserved = 2, kMiss = 3, kPending = 4, kCounters = 8 };

__global__ void __launch_bounds__(kBlock) k_keydir_clear(KSlot *__restrict__ slots, int64_t n_slots) {
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < n_slots; h += (int64_t)gridDim.x * blockDim.x)
        slots[h] = KSlot{kKeyEmpty, -1, kNoRow};
}

// find (and, with insert, claim) the slot of each row's key
__global__ void __launch_bounds__(kBlock) k_keydir_find(const int64_t *__restrict__ keys, int64_t r0, int64_t n,
                                                        KSlot *slots, uint32_t mask, int64_t cap,
                                                        unsigned long long *cnt, int32_t insert,
                                                        int32_t *__restrict__ slot_of, int32_t *__restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t r = r0 + i;
    const unsigned long long k = (unsigned long long)keys[r];
    slot_of[r] = -1;
    if (k == kKeyEmpty) {
        ids[r] = -1;
        atomicAdd(cnt + kReserved, 1ull);
        return;
    }
    // the held count is written by the read phase only: stable during this launch
    const bool ins = insert && (int64_t)cnt[kHeld] < cap;
    uint32_t h = (uint32_t)mix64(k) & mask;
    int32_t id = -1;
    bool hit = false;
    for (uint64_t step = 0; step <= (uint64_t)mask; ++step, h = (h + 1) & mask) {
        const longlong2 w = *reinterpret_cast<const longlong2 *>(slots + h);
        unsigned long long sk = (unsigned long long)w.x;
        if (sk == k) {  // held since an earlier launch (or claimed in this one: then id is -1)
            hit = true;
            id = (int32_t)(uint32_t)((unsigned long long)w.y & 0xFFFFFFFFull);
            break;
        }
        if (sk != kKeyEmpty) continue;
        if (!ins) break;  // lookup: an empty slot ends the chain
        sk = atomicCAS(&slots[h].key, kKeyEmpty, k);
        if (sk == kKeyEmpty || sk == k) {  // claimed here, or by another row of this launch
            hit = true;
            break;
        }
    }
    if (hit && id >= 0) {
        ids[r] = id;
    } else if (hit && ins) {
        atomicMin(&slots[h].first, (int32_t)r);
        slot_of[r] = (int32_t)h;
    } else {  // not held (a refused key left in the table has no id either)
        ids[r] = -1;
        atomicAdd(cnt + (insert ? kFull : kMiss), 1ull);
    }
}

__device__ __forceinline__ int32_t kd_mark(const int32_t *slot_of, const KSlot *slots, int64_t r, bool live) {
    if (!live) return 0;
    const int32_t h = slot_of[r];
    if (h < 0) return 0;
    const longlong2 w = *reinterpret_cast<const longlong2 *>(slots + (uint32_t)h);
    const int32_t id = (int32_t)(uint32_t)((unsigned long long)w.y & 0xFFFFFFFFull);
    const int32_t first = (int32_t)(uint32_t)((unsigned long long)w.y >> 32);
    return (id < 0 && first == (int32_t)r) ? 1 : 0;
}

__device__ __forceinline__ void kd_assign(const int64_t *keys, const int32_t *slot_of, KSlot *slots, int64_t *key_of,
                                          int64_t r, int64_t id, int64_t cap) {
    KSlot *s = slots + (uint32_t)slot_of[r];
    if (id < cap) {
        s->id = (int32_t)id;
        key_of[id] = keys[r];
    } else {
        s->first = kNoRow;  // refused: the key stays as garbage, ready to be refused again
    }
}

// -> 1 when row r waited for an id and got none
__device__ __forceinline__ int32_t kd_read(const int32_t *slot_of, const KSlot *slots, int32_t *ids, int64_t r,
                                           bool live) {
    if (!live) return 0;
    const int32_t h = slot_of[r];
    if (h < 0) return 0;
    const int32_t id = slots[(uint32_t)h].id;
    ids[r] = id;
    return id < 0 ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock) k_keydir_mark(int64_t r0, int64_t n, const KSlot *__restrict__ slots,
                                                        const int32_t *__restrict__ slot_of,
                                                        uint8_t *__restrict__ flag, int32_t *__restrict__ bcount) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int32_t f = kd_mark(slot_of, slots, r0 + i, i < n);
    if (i < n) flag[r0 + i] = (uint8_t)f;
    int32_t tot;
    block_excl_scan<kBlock / kWave>(f, &tot);
    if (threadIdx.x == 0) bcount[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kBlock) k_keydir_assign(const int64_t *__restrict__ keys, int64_t r0, int64_t n,
                                                          KSlot *__restrict__ slots, int64_t *__restrict__ key_of,
                                                          int64_t cap, unsigned long long *__restrict__ cnt,
                                                          const int32_t *__restrict__ slot_of,
                                                          const uint8_t *__restrict__ flag,
                                                          const int32_t *__restrict__ bcount) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    // new keys in the blocks before this one (gridDim.x <= kChunkRows / kBlock = kBlock: one per thread)
    int32_t base;
    block_excl_scan<kBlock / kWave>((int32_t)(threadIdx.x < blockIdx.x ? bcount[threadIdx.x] : 0), &base);
    const int32_t f = i < n ? flag[r0 + i] : 0;
    int32_t tot;
    const int32_t ex = block_excl_scan<kBlock / kWave>(f, &tot);
    if (f) kd_assign(keys, slot_of, slots, key_of, r0 + i, (int64_t)cnt[kHeld] + base + ex, cap);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) cnt[kPending] = (unsigned long long)(base + tot);
}

__global__ void __launch_bounds__(kBlock) k_keydir_read(int64_t r0, int64_t n, const KSlot *__restrict__ slots,
                                                        int64_t cap, unsigned long long *__restrict__ cnt,
                                                        const int32_t *__restrict__ slot_of,
                                                        int32_t *__restrict__ ids) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int32_t tot;
    block_excl_scan<kBlock / kWave>(kd_read(slot_of, slots, ids, r0 + i, i < n), &tot);
    if (threadIdx.x == 0) {
        if (tot) atomicAdd(cnt + kFull, (unsigned long long)tot);
        if (blockIdx.x == 0) cnt[kHeld] = (unsigned long long)imin64((int64_t)(cnt[kHeld] + cnt[kPending]), cap);
    }
}

// mark + assign + read of a batch of at most kTailRows rows, one block
__global__ void __launch_bounds__(kTail) k_keydir_tail(const int64_t *__restrict__ keys, int64_t r0, int64_t n,
                                                       KSlot *slots, int64_t *__restrict__ key_of, int64_t cap,
                                                       unsigned long long *cnt, const int32_t *__restrict__ slot_of,
                                                       int32_t *__restrict__ ids) {
    const int64_t i = threadIdx.x, r = r0 + i;
    const int32_t f = kd_mark(slot_of, slots, r, i < n);
    int32_t tot;
    const int32_t ex = block_excl_scan<kTail / kWave>(f, &tot);
    const int64_t held = (int64_t)cnt[kHeld];
    if (f) kd_assign(keys, slot_of, slots, key_of, r, held + ex, cap);
    __syncthreads();  // the block's id stores, before the block's loads of them
    int32_t refused;
    block_excl_scan<kTail / kWave>(kd_read(slot_of, slots, ids, r, i < n), &refused);
    if (threadIdx.x == 0) {
        if (refused) atomicAdd(cnt + kFull, (unsigned long long)refused);
        cnt[kHeld] = (unsigned long long)imin64(held + tot, cap);
    }
}

// load: key i gets id i (an empty directory); *err: a duplicate or the reserved key
__global__ void __launch_bounds__(kBlock) k_keydir_load(const int64_t *__restrict__ keys, int64_t n, KSlot *slots,
                                                        uint32_t mask, int64_t *__restrict__ key_of,
                                                        int32_t *__restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const unsigned long long k = (unsigned long long)keys[i];
    if (k == kKeyEmpty) {
        *err = 1;
        return;
    }
    uint32_t h = (uint32_t)mix64(k) & mask;
    for (uint64_t step = 0; step <= (uint64_t)mask; ++step, h = (h + 1) & mask) {
        const unsigned long long sk = atomicCAS(&slots[h].key, kKeyEmpty, k);
        if (sk == kKeyEmpty) {  // this row owns the slot
            slots[h].id = (int32_t)i;
            key_of[i] = (int64_t)k;
            return;
        }
        if (sk == k) break;  // a duplicate
    }
    *err = 1;  // (n <= capacity <= slots / 2: the probe cannot run out of slots)
}

// remap (f-10), phase 1: the surviving keys in their new order, staged outside key_of (new id <=
// old id, so a compaction in place would overwrite keys other lanes still have to read)
__global__ void __launch_bounds__(kBlock) k_keydir_compact(const int64_t *__restrict__ key_of,
                                                           const int32_t *__restrict__ map, int64_t held,
                                                           int64_t *__restrict__ staged) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= held) return;
    const int32_t to = map[i];  // validated: -1 or the rank among the survivors
    if (to >= 0) staged[to] = key_of[i];
}

// remap, last phase: the held count (read by the next find) and the pending count
__global__ void __launch_bounds__(kWave) k_keydir_set_held(unsigned long long *__restrict__ cnt, int64_t kept) {
    if (threadIdx.x == 0) {
        cnt[kHeld] = (unsigned long long)kept;
        cnt[kPending] = 0;
    }
}

}  // namespace
}  // namespace fdx

using namespace fdx;

struct fdx_keydir_s {
    int64_t cap = 0, max_batch = 0, n_slots = 0;
    KSlot *slots_d = nullptr;
    int64_t *key_of_d = nullptr;
    unsigned long long *cnt_d = nullptr;  // kCounters words; [kCounters] as int32: load's error flag
    int32_t *slot_of_d = nullptr, *bcount_d = nullptr;
    uint8_t *flag_d = nullptr;
    size_t bytes = 0;
};

extern "C" int fdx_keydir_destroy(fdx_keydir d) {
    if (!d) return FDX_OK;
    (void)hipFree(d->slots_d);
    (void)hipFree(d->key_of_d);
    (void)hipFree(d->cnt_d);
    (void)hipFree(d->slot_of_d);
    (void)hipFree(d->bcount_d);
    (void)hipFree(d->flag_d);
    delete d;
    return FDX_OK;
}

extern "C" int fdx_keydir_reset(fdx_keydir d, void *stream) {
    FDX_REQUIRE(d, "null key directory");
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_keydir_clear, dim3(stream_grid(d->n_slots, kBlock)), dim3(kBlock), 0, st, d->slots_d,
                       d->n_slots);
    FDX_LAUNCHED("k_keydir_clear");
    FDX_HIP(hipMemsetAsync(d->cnt_d, 0, (kCounters + 2) * 8, st));
    return FDX_OK;
}

extern "C" int fdx_keydir_create(int64_t capacity, int64_t max_batch, fdx_keydir *out, void *stream) {
    FDX_REQUIRE(out, "null pointer");
    *out = nullptr;
    FDX_REQUIRE(capacity >= 1 && capacity <= (1LL << 30), "capacity must be in [1, 2^30]");
    FDX_REQUIRE(max_batch >= 1 && max_batch < INT32_MAX, "max_batch out of range");
    fdx_keydir d = new fdx_keydir_s;
    d->cap = capacity;
    d->max_batch = max_batch;
    d->n_slots = 2;
    while (d->n_slots < 2 * capacity) d->n_slots <<= 1;
    auto alloc = [&](void **p, size_t b) -> hipError_t {
        d->bytes += b;
        return hipMalloc(p, b);
    };
    hipError_t e = hipSuccess;
    if ((e = alloc((void **)&d->slots_d, (size_t)d->n_slots * sizeof(KSlot))) ||
        (e = alloc((void **)&d->key_of_d, (size_t)capacity * 8)) ||
        (e = alloc((void **)&d->cnt_d, (kCounters + 2) * 8)) ||
        (e = alloc((void **)&d->slot_of_d, (size_t)max_batch * 4)) ||
        (e = alloc((void **)&d->bcount_d, (size_t)(kChunkRows / kBlock) * 4)) ||
        (e = alloc((void **)&d->flag_d, (size_t)max_batch))) {
        set_error("hipMalloc of the key directory (%zu bytes so far) failed: %s", d->bytes, hipGetErrorString(e));
        fdx_keydir_destroy(d);
        return FDX_E_HIP;
    }
    const int rc = fdx_keydir_reset(d, stream);
    if (rc) {
        fdx_keydir_destroy(d);
        return rc;
    }
    *out = d;
    return FDX_OK;
}

extern "C" int fdx_keydir_memory(fdx_keydir d, size_t *bytes) {
    FDX_REQUIRE(d && bytes, "null pointer");
    *bytes = d->bytes;
    return FDX_OK;
}

extern "C" int fdx_keydir_map(fdx_keydir d, const int64_t *keys_d, int64_t n, int32_t opts, int32_t *ids_d,
                              void *stream) {
    FDX_REQUIRE(d, "null key directory");
    FDX_REQUIRE(n >= 0 && n <= d->max_batch, "batch of %lld rows exceeds max_batch %lld", (long long)n,
                (long long)d->max_batch);
    FDX_REQUIRE((opts & ~FDX_KEYDIR_INSERT) == 0, "unknown option bits");
    if (n == 0) return FDX_OK;
    FDX_REQUIRE(keys_d && ids_d, "null keys or ids");
    hipStream_t st = as_stream(stream);
    const uint32_t mask = (uint32_t)(d->n_slots - 1);
    const int32_t insert = opts & FDX_KEYDIR_INSERT;
    // lookup writes nothing to the table: one launch over the whole batch
    const int64_t chunk = insert ? std::min(std::min(d->cap, kChunkRows), n) : n;
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t m = n - r0 < chunk ? n - r0 : chunk;
        const dim3 grid((unsigned)ceil_div(m, kBlock));
        hipLaunchKernelGGL(k_keydir_find, grid, dim3(kBlock), 0, st, keys_d, r0, m, d->slots_d, mask, d->cap,
                           d->cnt_d, insert, d->slot_of_d, ids_d);
        FDX_LAUNCHED("k_keydir_find");
        if (!insert) continue;
        if (m <= kTailRows) {
            hipLaunchKernelGGL(k_keydir_tail, dim3(1), dim3(kTail), 0, st, keys_d, r0, m, d->slots_d, d->key_of_d,
                               d->cap, d->cnt_d, d->slot_of_d, ids_d);
            FDX_LAUNCHED("k_keydir_tail");
            continue;
        }
        hipLaunchKernelGGL(k_keydir_mark, grid, dim3(kBlock), 0, st, r0, m, d->slots_d, d->slot_of_d, d->flag_d,
                           d->bcount_d);
        FDX_LAUNCHED("k_keydir_mark");
        hipLaunchKernelGGL(k_keydir_assign, grid, dim3(kBlock), 0, st, keys_d, r0, m, d->slots_d, d->key_of_d, d->cap,
                           d->cnt_d, d->slot_of_d, d->flag_d, d->bcount_d);
        FDX_LAUNCHED("k_keydir_assign");
        hipLaunchKernelGGL(k_keydir_read, grid, dim3(kBlock), 0, st, r0, m, d->slots_d, d->cap, d->cnt_d,
                           d->slot_of_d, ids_d);
        FDX_LAUNCHED("k_keydir_read");
    }
    return FDX_OK;
}

extern "C" int fdx_keydir_counts(fdx_keydir d, int64_t counts_h[4], void *stream) {
    FDX_REQUIRE(d && counts_h, "null pointer");
    hipStream_t st = as_stream(stream);
    FDX_HIP(hipMemcpyAsync(counts_h, d->cnt_d, 4 * 8, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    return FDX_OK;
}

extern "C" int fdx_keydir_keys(fdx_keydir d, int64_t *keys_out_d, int64_t cap, int64_t *n_h, void *stream) {
    FDX_REQUIRE(d && n_h, "null pointer");
    FDX_REQUIRE(cap >= 0 && (keys_out_d || cap == 0), "null keys_out_d");
    hipStream_t st = as_stream(stream);
    int64_t held = 0;
    FDX_HIP(hipMemcpyAsync(&held, d->cnt_d, 8, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    *n_h = held;
    FDX_REQUIRE(cap >= held, "keys_out_d holds %lld keys, the directory %lld", (long long)cap, (long long)held);
    if (held) FDX_HIP(hipMemcpyAsync(keys_out_d, d->key_of_d, (size_t)held * 8, hipMemcpyDeviceToDevice, st));
    return FDX_OK;
}

extern "C" int fdx_keydir_load(fdx_keydir d, const int64_t *keys_d, int64_t n, void *stream) {
    FDX_REQUIRE(d, "null key directory");
    FDX_REQUIRE(n >= 0 && n <= d->cap, "%lld keys do not fit the capacity %lld", (long long)n, (long long)d->cap);
    FDX_REQUIRE(keys_d || n == 0, "null keys");
    hipStream_t st = as_stream(stream);
    int64_t held = 0;
    FDX_HIP(hipMemcpyAsync(&held, d->cnt_d, 8, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    FDX_REQUIRE(held == 0, "load needs an empty directory (it holds %lld keys)", (long long)held);
    if (n == 0) return FDX_OK;
    int32_t *err_d = reinterpret_cast<int32_t *>(d->cnt_d + kCounters);
    hipLaunchKernelGGL(k_keydir_load, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, st, keys_d, n, d->slots_d,
                       (uint32_t)(d->n_slots - 1), d->key_of_d, err_d);
    FDX_LAUNCHED("k_keydir_load");
    int32_t err = 0;
    FDX_HIP(hipMemcpyAsync(&err, err_d, 4, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    if (err) {
        const int rc = fdx_keydir_reset(d, stream);
        if (rc) return rc;
        FDX_REQUIRE(false, "load: a duplicate or the reserved key (INT64_MIN); the directory stays empty");
    }
    const unsigned long long held_new = (unsigned long long)n;
    FDX_HIP(hipMemcpyAsync(d->cnt_d, &held_new, 8, hipMemcpyHostToDevice, st));
    FDX_HIP(hipStreamSynchronize(st));  // held_new lives on this frame
    return FDX_OK;
}

// ---- f-10: the directory after a retirement.  key_of is compacted by the id map (through the
// workspace), the table is cleared and refilled from it (key_of[i] -> id i, as fdx_keydir_load), so
// the retired keys' ids and slots -- and refused keys left in the table -- are free again.
namespace {
struct RemapWs {
    MapRes *res;
    uint32_t *flag;
    void *scan;
    int64_t *staged;
    size_t total;
};

RemapWs remap_ws(fdx_keydir d, void *ws) {
    char *p = reinterpret_cast<char *>(ws);
    RemapWs w{};
    const size_t o_flag = 256, o_scan = o_flag + al256((size_t)(d->cap + 1) * 4);
    const size_t o_staged = o_scan + al256(fdx_exclusive_scan_u32_workspace_size(d->cap + 1));
    w.total = o_staged + al256((size_t)d->cap * 8);
    if (!p) return w;  // the size query
    w.res = reinterpret_cast<MapRes *>(p);
    w.flag = reinterpret_cast<uint32_t *>(p + o_flag);
    w.scan = p + o_scan;
    w.staged = reinterpret_cast<int64_t *>(p + o_staged);
    return w;
}
}  // namespace

extern "C" size_t fdx_keydir_remap_workspace_size(fdx_keydir d) { return d ? remap_ws(d, nullptr).total : 0; }

extern "C" int fdx_keydir_remap(fdx_keydir d, const int32_t *map_d, int64_t n_map, int64_t kept, void *workspace_d,
                                size_t workspace_bytes, void *stream) {
    FDX_REQUIRE(d, "null key directory");
    FDX_REQUIRE(workspace_d && workspace_bytes >= fdx_keydir_remap_workspace_size(d), "workspace too small");
    FDX_REQUIRE(n_map >= 0 && n_map <= d->cap && (map_d || n_map == 0), "the map has %lld entries, the capacity is %lld",
                (long long)n_map, (long long)d->cap);
    hipStream_t st = as_stream(stream);
    int64_t held = 0;
    FDX_HIP(hipMemcpyAsync(&held, d->cnt_d, 8, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    FDX_REQUIRE(n_map >= held, "the map has %lld entries, the directory holds %lld keys", (long long)n_map,
                (long long)held);
    FDX_REQUIRE(kept >= 0 && kept <= held, "kept %lld outside [0, %lld keys held]", (long long)kept, (long long)held);
    const RemapWs w = remap_ws(d, workspace_d);
    // pass 1, to completion before anything is written: the map over the ids held (entries beyond are unused)
    int rc = map_validate(map_d, held, w.res, w.flag, w.scan, st);
    if (rc) return rc;
    MapRes r;
    FDX_HIP(hipMemcpyAsync(&r, w.res, sizeof(r), hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    FDX_REQUIRE(!r.bad, "the map is malformed: -1 or the rank among the survivors, in id order");
    FDX_REQUIRE((int64_t)r.kept == kept, "the map keeps %lld of the keys held, the call says %lld", (long long)r.kept,
                (long long)kept);
    // pass 2
    if (held) {
        hipLaunchKernelGGL(k_keydir_compact, dim3((unsigned)ceil_div(held, kBlock)), dim3(kBlock), 0, st, d->key_of_d,
                           map_d, held, w.staged);
        FDX_LAUNCHED("k_keydir_compact");
    }
    hipLaunchKernelGGL(k_keydir_clear, dim3(stream_grid(d->n_slots, kBlock)), dim3(kBlock), 0, st, d->slots_d,
                       d->n_slots);
    FDX_LAUNCHED("k_keydir_clear");
    int32_t *err_d = reinterpret_cast<int32_t *>(d->cnt_d + kCounters);
    FDX_HIP(hipMemsetAsync(err_d, 0, 4, st));
    if (kept) {
        hipLaunchKernelGGL(k_keydir_load, dim3((unsigned)ceil_div(kept, kBlock)), dim3(kBlock), 0, st, w.staged, kept,
                           d->slots_d, (uint32_t)(d->n_slots - 1), d->key_of_d, err_d);
        FDX_LAUNCHED("k_keydir_load");
    }
    hipLaunchKernelGGL(k_keydir_set_held, dim3(1), dim3(kWave), 0, st, d->cnt_d, kept);
    FDX_LAUNCHED("k_keydir_set_held");
    int32_t err = 0;
    FDX_HIP(hipMemcpyAsync(&err, err_d, 4, hipMemcpyDeviceToHost, st));
    FDX_HIP(hipStreamSynchronize(st));
    if (err) {  // cannot happen with a consistent directory; its keys are gone if it does
        hipLaunchKernelGGL(k_keydir_clear, dim3(stream_grid(d->n_slots, kBlock)), dim3(kBlock), 0, st, d->slots_d,
                           d->n_slots);
        FDX_LAUNCHED("k_keydir_clear");
        hipLaunchKernelGGL(k_keydir_set_held, dim3(1), dim3(kWave), 0, st, d->cnt_d, (int64_t)0);
        FDX_LAUNCHED("k_keydir_set_held");
        FDX_HIP(hipMemsetAsync(err_d, 0, 4, st));
        FDX_REQUIRE(false, "remap: the directory held a duplicate or the reserved key; it is empty now");
    }
    return FDX_OK;
}
