"""The key directory's model (tests/keydir_ref.py, no GPU): numbering == pandas.factorize over
the concatenated stream, the partial fit at the capacity edge, lookup mode, the reserved key,
load / resized -- the contract of include/fdx.h (f-9) that the GPU tests hold the kernels to."""
import numpy as np
import pandas as pd
import pytest

import bench_stream
from keydir_ref import RESERVED, KeyDirModel


def test_ids_over_a_stream_are_pandas_factorize():
    rng = np.random.default_rng(0)
    pool = np.r_[rng.integers(-2 ** 62, 2 ** 62, 300), 0, -1, 2 ** 63 - 1, RESERVED + 1]
    batches = [pool[rng.integers(0, min(len(pool), 40 * (j + 1)), n)] for j, n in enumerate([1, 63, 64, 65, 257, 1025])]
    m = KeyDirModel(1 << 12)
    got = np.concatenate([m.map(b) for b in batches])
    codes, uniques = pd.factorize(np.concatenate(batches))
    np.testing.assert_array_equal(got, codes)
    np.testing.assert_array_equal(m.keys(), uniques)
    assert m.counts() == {"held": len(uniques), "refused_full": 0, "refused_reserved": 0, "misses": 0}


def test_partial_fit_at_the_capacity_edge():
    m = KeyDirModel(8)
    assert m.map([10, 11, 12, 13, 14]).tolist() == [0, 1, 2, 3, 4]
    #            new  held new  new  dup  new  new  new  dup-of-refused
    got = m.map([20, 11, 21, 22, 20, 23, 24, 25, 23])
    assert got.tolist() == [5, 1, 6, 7, 5, -1, -1, -1, -1]
    assert m.counts() == {"held": 8, "refused_full": 4, "refused_reserved": 0, "misses": 0}
    assert m.keys().tolist() == [10, 11, 12, 13, 14, 20, 21, 22]
    assert m.map([23, 10, 22]).tolist() == [-1, 0, 7]           # refused keys stay refused, held keys map
    big = m.resized(16)
    assert big.map([23, 24, 10, 25]).tolist() == [8, 9, 0, 10]  # ... and are new to a larger directory


def test_lookup_mode_writes_nothing():
    m = KeyDirModel(8)
    m.map([5, 6])
    assert m.map([6, 7, 5, 7], insert=False).tolist() == [1, -1, 0, -1]
    assert m.counts() == {"held": 2, "refused_full": 0, "refused_reserved": 0, "misses": 2}
    assert m.keys().tolist() == [5, 6]
    assert m.map([7]).tolist() == [2]


def test_reserved_key_is_refused_and_counted():
    m = KeyDirModel(4)
    assert m.map([RESERVED, 1, RESERVED, -1, 2 ** 63 - 1, RESERVED + 1]).tolist() == [-1, 0, -1, 1, 2, 3]
    assert m.map([RESERVED], insert=False).tolist() == [-1]
    assert m.counts() == {"held": 4, "refused_full": 0, "refused_reserved": 3, "misses": 0}


def test_load_refuses_duplicates_the_reserved_key_and_overflow():
    for bad in ([1, 2, 1], [1, RESERVED], [1, 2, 3, 4, 5]):
        m = KeyDirModel(4)
        with pytest.raises(ValueError):
            m.load(bad)
        assert m.counts()["held"] == 0
    m = KeyDirModel(4)
    m.load([9, 8, 7])
    assert m.map([7, 9, 6]).tolist() == [2, 0, 3]
    with pytest.raises(ValueError):
        m.load([1])  # not empty


def test_bench_scramble_is_injective_and_above_2_40():
    """bench_stream.raw_id_scramble (--raw-ids): id * odd constant + offset, no wrap-around."""
    ids = np.r_[0, 1, 2, 999_999, 1_999_999, 2 ** 31 - 1, np.random.default_rng(1).integers(0, 2 ** 31, 5000)]
    for mult, off in bench_stream.RAW_ID_SCRAMBLE.values():
        raw = bench_stream.raw_id_scramble(ids, mult, off)
        assert raw.dtype == np.int64 and raw.min() > 2 ** 40
        assert [int(r) for r in raw[:6]] == [int(i) * mult + off for i in ids[:6]]   # exact in Python ints
        assert len(np.unique(raw)) == len(np.unique(ids))
    a, b = (bench_stream.raw_id_scramble(np.arange(1000), *bench_stream.RAW_ID_SCRAMBLE[k])
            for k in ("customer", "terminal"))
    assert not np.intersect1d(a, b).size and np.all(np.diff(a) > 2 ** 31)         # not dense, not int32
    for bad in ((2, 1 << 41), (3, 5), (1 << 33 | 1, 1 << 41)):
        with pytest.raises(ValueError):
            bench_stream.raw_id_scramble(ids, *bad)
    with pytest.raises(ValueError):
        bench_stream.raw_id_scramble(np.array([-1]), 3, 1 << 41)
