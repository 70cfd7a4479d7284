"""Retiring idle keys (f-10), without a GPU: the exactness claim itself -- a key idle for a whole
horizon that comes back has the features of a key never seen -- checked with the oracle over the
tables the GPU tests stream, the inclusive boundary on hand-built keys, and the model's own
parts (tests/retire_ref.py) against pandas.factorize."""
import numpy as np
import pandas as pd
import pytest

import oracle
import retire_ref as M
import stream_label_ref as R

DAY = M.DAY


def _features(cols, customer, terminal, windows=(1, 7, 30), delay=7):
    f = oracle.featurize_arrays(cols["ts"], customer, terminal, cols["amount"], cols["fraud"], windows, delay)
    return {k: v for k, v in f.items() if k.startswith(("CUSTOMER_ID", "TERMINAL_ID"))}


@pytest.mark.parametrize("name", ["era", "gap"])
def test_a_returning_key_is_a_new_key_to_the_oracle(name):
    """The oracle over the full history == the oracle over a table in which every incarnation of
    a key is a key of its own (so each row sees only its key's rows since the last retirement)."""
    cols = M.raw(M.era_table() if name == "era" else M.gap_table())
    c = M.cuts(len(cols["ts"]))
    when = (lambda j: j % 2 == 0) if name == "era" else (lambda j: True)
    caps = (80, 50) if name == "era" else (40, 25)
    cs, ts, _ = M.simulate(cols, c, when, caps)
    assert cs.dir.refused_full == 0 and ts.dir.refused_full == 0
    if name == "era":
        assert len(np.unique(cols["customer"])) == 160 and len(np.unique(cols["terminal"])) == 100
        assert (cs.peak, ts.peak) == (80, 50) and (cs.retired, ts.retired) == (120, 75)
    else:
        assert len(cols["ts"]) == 2414 and (cs.retired, ts.retired) == (12, 8)
        assert all(k in cs.last for k in cs.inc) and all(k in ts.last for k in ts.inc)   # all of them returned
    full = _features(cols, cols["customer"], cols["terminal"])
    split = _features(cols, cs.incarnation_ids(), ts.incarnation_ids())
    assert len(np.unique(cs.incarnation_ids())) == len(np.unique(cols["customer"])) + (12 if name == "gap" else 0)
    for k in full:
        np.testing.assert_array_equal(split[k], full[k], err_msg=k)


@pytest.mark.parametrize("windows,delay", [((1, 7, 30), 7), ((2, 5), 3)])
def test_the_boundary_is_inclusive(windows, delay):
    """last_ts == watermark - horizon: retired, and the next row at ts == watermark is exact.  One
    ns later the key is kept -- and would not be exact as a new key: the boundary is tight."""
    hc, ht = M.horizons(windows, delay)
    t0 = R.BASE + 5 * DAY
    for horizon, half in ((hc, "CUSTOMER_ID"), (ht, "TERMINAL_ID")):
        wm = t0 + horizon
        for last, retired in ((t0, True), (t0 + 1, False)):
            assert bool(M.idle([3], [last], wm, horizon)[0]) is retired
            ts = np.array([last - DAY // 2, last - 7, last, wm], np.int64)
            cols = {"ts": ts, "amount": np.array([10.5, 3.25, 8.0, 2.75]), "fraud": np.array([1, 0, 1, 0], np.uint8)}
            one, two = np.zeros(4, np.int64), np.array([0, 0, 0, 1])
            other = np.arange(4)          # the other half: every row its own key
            a = _features(cols, one if half == "CUSTOMER_ID" else other, one if half == "TERMINAL_ID" else other,
                          windows, delay)
            b = _features(cols, two if half == "CUSTOMER_ID" else other, two if half == "TERMINAL_ID" else other,
                          windows, delay)
            same = all(np.array_equal(a[k][3:], b[k][3:]) for k in a if k.startswith(half))
            assert same is retired, (half, last - t0)
    assert M.idle([0, 1, 1], [0, M.I64_MIN, M.I64_MIN + 1], M.I64_MIN + 5, hc).tolist() == [True, True, False]


def test_id_map_and_directory_model():
    m, kept = M.id_map([False, True, True, False, False, True])
    assert m.tolist() == [0, -1, -1, 1, 2, -1] and kept == 3
    rng = np.random.default_rng(4)
    keys = rng.integers(-2 ** 62, 2 ** 62, 300)
    col = keys[rng.integers(0, 300, 4000)]
    d = M.DirModel(400)
    d.map(col[:3000])
    held = d.keys()
    dead = rng.random(len(held)) < 0.4
    m, kept = M.id_map(dead)
    before = d.counts()
    d.remap(m, kept)
    gone = set(held[dead].tolist())
    np.testing.assert_array_equal(d.keys(), pd.factorize(np.array([k for k in col[:3000] if k not in gone]))[1])
    assert d.counts() == {**before, "held": kept}
    assert d.map(held[dead][:5], insert=False).tolist() == [-1] * 5
    # a retired key that comes back is a new key: the next free ids, in first-occurrence order
    ids = d.map(col[3000:])
    filtered = np.array([k for k in col[:3000] if k not in gone] + col[3000:].tolist())
    np.testing.assert_array_equal(ids, pd.factorize(filtered)[0][-1000:])
    for bad, k in (([1, 0], 2), ([0, 2], 2), ([0, -2], 1), ([0, 1], 1), ([0], 1)):
        e = M.DirModel(4)
        e.map(np.array([7, 8]))
        with pytest.raises(ValueError):
            e.remap(bad, k)
