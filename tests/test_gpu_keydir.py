"""The device key directory (fdx_keydir_*, csrc/fdx_keydir.hip; fdx.streaming.KeyDirectory)
against the dict model of tests/keydir_ref.py: ids, keys() and counts() after every batch.

Batch sizes are the kernels' edges: the wave (64), the block (256), the single-block tail
(1,024 rows: up to there mark + assign + read run as one block, above it as three grids whose
block counts are summed), and the chunk (a call is cut into chunks of min(capacity, 65,536)
rows: 4,097 rows at capacity 4,096 are two chunks, 8,192 at capacity 8,192 one grid of 32
blocks).  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest
import torch

from fdx import _lib
from fdx.streaming import KeyDirectory
from keydir_ref import RESERVED, KeyDirModel

pytestmark = pytest.mark.gpu

I64_MAX = 2 ** 63 - 1
SPECIAL = [0, -1, I64_MAX, RESERVED + 1, 1 << 32, 2 << 32, 3 << 32, -(1 << 32), 5, 5 - 2 ** 63, 77, 77 - 2 ** 63,
           1000, 1001, 1002, 1003, 1004]  # ... multiples of 2^32, pairs differing only in bit 63, consecutive
SIZES = [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 4097]


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.int64))).to(dev)


def same(d, m, got, want):
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert d.counts() == m.counts()
    np.testing.assert_array_equal(d.keys().cpu().numpy(), m.keys())


def batches(seed=3):
    """~30 % of a batch's rows are keys not seen before (while the pool lasts), the rest repeats
    of earlier keys and of the batch's own; plus one batch that is a single key repeated."""
    rng = np.random.default_rng(seed)
    pool = np.r_[np.array(SPECIAL, np.int64), np.arange(10 ** 12, 10 ** 12 + 600),           # consecutive integers
                 rng.integers(-2 ** 63 + 1, 2 ** 63 - 1, 3500, dtype=np.int64)]
    pool = pool[np.r_[np.arange(len(SPECIAL)), len(SPECIAL) + rng.permutation(len(pool) - len(SPECIAL))]]
    seen, out = 0, []
    for n in SIZES:
        fresh = min(max(1, int(0.3 * n)), len(pool) - seen)
        new = pool[seen:seen + fresh]
        old = pool[rng.integers(0, max(seen, 1), n)] if seen else np.repeat(new[:1], n)
        pick = rng.random(n) < 0.45                      # each fresh key several times, in shuffled rows
        b = np.where(pick, new[rng.integers(0, fresh, n)], old)
        b[rng.permutation(n)[:fresh]] = new[rng.permutation(fresh)][:n]
        out.append(b.astype(np.int64))
        seen += fresh
    out.insert(4, np.full(300, 424242, np.int64))        # one key repeated
    return out


def test_numbering_equals_the_model_batch_by_batch_and_run_to_run(dev):
    bs = batches()
    assert sum(len(np.unique(b)) for b in bs) > 1200
    d, m = KeyDirectory(4096, max_batch=4097), KeyDirModel(4096)
    runs = []
    for _ in range(2):
        d.reset()
        m.reset()
        got = []
        for b in bs:
            ids = d.map(T(b, dev))
            same(d, m, ids, m.map(b))
            got.append(ids.cpu().numpy())
        runs.append((np.concatenate(got), d.keys().cpu().numpy()))
    assert m.counts()["held"] <= 4096 and m.counts()["refused_full"] == 0
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    import pandas as pd

    np.testing.assert_array_equal(runs[0][0], pd.factorize(np.concatenate(bs))[0])


def test_one_grid_of_many_blocks_and_the_first_occurrence_across_blocks(dev):
    """8,192 rows in one chunk (32 blocks): every key's first occurrence and its repeats lie in
    different blocks; 6,000 new keys numbered across the block sums."""
    rng = np.random.default_rng(8)
    keys = rng.integers(-2 ** 63 + 1, 2 ** 63 - 1, 6000, dtype=np.int64)
    b = keys[rng.integers(0, 6000, 8192)]
    b[rng.permutation(8192)[:6000]] = keys
    d, m = KeyDirectory(8192, max_batch=8192), KeyDirModel(8192)
    same(d, m, d.map(T(b, dev)), m.map(b))
    same(d, m, d.map(T(b[::-1].copy(), dev)), m.map(b[::-1]))
    assert m.counts()["held"] == 6000


def test_exactly_full_then_over(dev):
    d, m = KeyDirectory(8, max_batch=64), KeyDirModel(8)
    first = np.array([11, -1, I64_MAX, 0, 1 << 40, 7, 8, 9], np.int64)
    same(d, m, d.map(T(first, dev)), m.map(first))                 # filled to 8: table load 0.5
    same(d, m, d.map(T(first[::-1].copy(), dev)), m.map(first[::-1]))
    assert m.counts()["held"] == 8
    over = np.r_[first[:3], np.arange(100, 112), first[3:], np.arange(100, 112)].astype(np.int64)  # 12 new keys
    ids = d.map(T(over, dev))
    same(d, m, ids, m.map(over))
    assert (ids.cpu().numpy() >= 0).sum() == 8 and m.counts()["refused_full"] == 24
    for j in range(4):  # 64 unseen keys > 16 slots: every probe ends, every row is refused
        unseen = np.arange(1000 + 16 * j, 1016 + 16 * j, dtype=np.int64) * 7919
        ids = d.map(T(unseen, dev))
        assert ids.cpu().tolist() == [-1] * 16
        same(d, m, ids, m.map(unseen))
        same(d, m, d.map(T(first, dev)), m.map(first))             # known keys still map
    same(d, m, d.map(T(over, dev), insert=False), m.map(over, insert=False))


def test_partial_fit_is_by_first_occurrence(dev):
    d, m = KeyDirectory(8, max_batch=64), KeyDirModel(8)
    held = np.array([10, 11, 12, 13, 14], np.int64)
    same(d, m, d.map(T(held, dev)), m.map(held))
    b = np.array([25, 20, 11, 25, 21, 22, 20, 23, 24, 21, 23, 14], np.int64)     # 6 new keys: 25 20 21 22 23 24
    ids = d.map(T(b, dev))
    assert ids.cpu().tolist() == [5, 6, 1, 5, 7, -1, 6, -1, -1, 7, -1, 4]
    same(d, m, ids, m.map(b))
    assert d.keys().cpu().tolist() == [10, 11, 12, 13, 14, 25, 20, 21]
    # 12 rows at capacity 8 were two chunks; the same through a directory that takes them as one
    d2, m2 = KeyDirectory(16, max_batch=64), KeyDirModel(16)
    same(d2, m2, d2.map(T(np.r_[held, np.arange(50, 58)], dev)), m2.map(np.r_[held, np.arange(50, 58)]))
    assert m2.counts()["held"] == 13
    ids = d2.map(T(b, dev))
    assert ids.cpu().tolist() == [13, 14, 1, 13, 15, -1, 14, -1, -1, 15, -1, 4]
    same(d2, m2, ids, m2.map(b))


def test_lookup_mode(dev):
    d, m = KeyDirectory(64, max_batch=2048), KeyDirModel(64)
    a = np.arange(40, dtype=np.int64) * (1 << 33) - 5
    same(d, m, d.map(T(a, dev)), m.map(a))
    q = np.r_[a[::3], np.arange(7, dtype=np.int64) + 1, a[:5], RESERVED].astype(np.int64)
    q = np.tile(q, 50)[:1500]                                       # above the single-block tail's size as well
    for part in (q[:30], q):
        ids = d.map(T(part, dev), insert=False)
        same(d, m, ids, m.map(part, insert=False))
    assert m.counts()["misses"] > 0 and m.counts()["held"] == 40 and m.counts()["refused_reserved"] > 0
    same(d, m, d.map(T(q[:30], dev)), m.map(q[:30]))               # the missed keys were not left behind
    out = torch.full((30,), 99, dtype=torch.int32, device=dev)
    assert d.map(T(q[:30], dev), insert=False, out=out) is out and out.cpu().tolist() == m.map(q[:30], False).tolist()


def test_reserved_key_leaves_the_other_rows_alone(dev):
    d, m = KeyDirectory(16, max_batch=64), KeyDirModel(16)
    b = np.array([RESERVED, 3, RESERVED, RESERVED + 1, I64_MAX, 3, RESERVED, -1], np.int64)
    ids = d.map(T(b, dev))
    assert ids.cpu().tolist() == [-1, 0, -1, 1, 2, 0, -1, 3]
    same(d, m, ids, m.map(b))
    assert d.counts()["refused_reserved"] == 3


def test_load_keys_resized(dev):
    d, m = KeyDirectory(8, max_batch=64), KeyDirModel(8)
    keys = np.array([5, -9, I64_MAX, 1 << 50, 0, 6, 7, 8], np.int64)
    d.load(T(keys, dev))
    m.load(keys)
    q = np.r_[keys[::-1], 99].astype(np.int64)
    same(d, m, d.map(T(q, dev), insert=False), m.map(q, insert=False))
    with pytest.raises(_lib.FdxError, match="empty"):
        d.load(T(keys[:2], dev))                                   # not empty
    for bad in ([1, 2, 3, 2], [1, RESERVED, 2], list(range(9))):
        e = KeyDirectory(8, max_batch=64)
        with pytest.raises(_lib.FdxError):
            e.load(T(bad, dev))
        assert e.counts() == {"held": 0, "refused_full": 0, "refused_reserved": 0, "misses": 0}
        assert e.keys().numel() == 0
        assert e.map(T([2, 1, 7], dev)).cpu().tolist() == [0, 1, 2]     # still a working, empty directory
    # the full directory refuses, its resized(16) numbers the same keys 8, 9, ... in order
    new = np.array([300, 5, 301, 300, 302], np.int64)
    same(d, m, d.map(T(new, dev)), m.map(new))
    assert m.counts()["refused_full"] == 4
    d16, m16 = d.resized(16), m.resized(16)
    assert d16.capacity == 16 and d16.memory_bytes > d.memory_bytes
    ids = d16.map(T(new, dev))
    assert ids.cpu().tolist() == [8, 0, 9, 8, 10]
    same(d16, m16, ids, m16.map(new))
    same(d, m, d.map(T(keys, dev)), m.map(keys))                   # the old one is untouched


def test_entry_points_through_ctypes(dev):
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.fdx_keydir_create(4, 8, ctypes.byref(h), None) == 0
    keys = T([7, 8, 7, 9], dev)
    ids = torch.empty(4, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.fdx_keydir_map(h, P(keys), 9, 1, P(ids), None) == -1 and b"max_batch" in L.fdx_last_error()
    assert L.fdx_keydir_map(h, P(keys), -1, 1, P(ids), None) == -1
    assert L.fdx_keydir_map(h, None, 4, 1, P(ids), None) == -1
    assert L.fdx_keydir_map(h, P(keys), 4, 2, P(ids), None) == -1
    assert L.fdx_keydir_map(h, None, 0, 1, None, None) == 0          # n == 0: a no-op
    assert L.fdx_keydir_map(h, P(keys), 4, _lib.FDX_KEYDIR_INSERT, P(ids), None) == 0
    c = (ctypes.c_int64 * 4)()
    assert L.fdx_keydir_counts(h, c, None) == 0 and list(c) == [3, 0, 0, 0]
    assert ids.cpu().tolist() == [0, 1, 0, 2]
    out = torch.zeros(4, dtype=torch.int64, device=dev)
    n = ctypes.c_int64()
    assert L.fdx_keydir_keys(h, P(out), 2, ctypes.byref(n), None) == -1 and n.value == 3      # cap < held
    assert out.cpu().tolist() == [0, 0, 0, 0]
    assert L.fdx_keydir_keys(h, P(out), 4, ctypes.byref(n), None) == 0 and out.cpu().tolist() == [7, 8, 9, 0]
    assert L.fdx_keydir_load(h, P(keys), 5, None) == -1              # n > capacity
    b = ctypes.c_size_t()
    assert L.fdx_keydir_memory(h, ctypes.byref(b)) == 0 and b.value >= 8 * 16 + 4 * 8
    assert L.fdx_keydir_reset(h, None) == 0
    assert L.fdx_keydir_counts(h, c, None) == 0 and list(c) == [0, 0, 0, 0]
    assert L.fdx_keydir_destroy(h) == 0
