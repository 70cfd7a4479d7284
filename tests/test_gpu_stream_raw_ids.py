"""StreamScorer(raw_ids=True): raw 64-bit customer / terminal ids mapped by the device key
directories in front of the stream state (fdx_keydir_map inside score, score_graph,
report_frauds and score_cdc; snapshot_keys / restore_keys; grow).

The reference of every test is the dense scorer on the original ids of the same table
(stream_label_ref.table: ~3,000 rows, 40 customers, 25 terminals, 60 days, batches of 257);
features do not depend on how the keys are numbered, so every comparison is an equality of
arrays or of bytes."""
import numpy as np
import pytest
import torch

import stream_label_ref as R
from bench_stream import RAW_ID_SCRAMBLE, cdc_encode, raw_id_scramble
from fdx import _lib, ops
from fdx.streaming import (StreamScorer, StreamState, load_keys, load_snapshot, save_keys, save_snapshot)

pytestmark = pytest.mark.gpu

N, N_C, N_T, B = 3000, 40, 25, 257
KEYS = (("ts", torch.int64), ("customer", torch.int32), ("amount", torch.float64), ("terminal", torch.int32))
RAW_KEYS = tuple((k, torch.int64 if k in ("customer", "terminal") else dt) for k, dt in KEYS)
CUTS = np.r_[np.arange(0, N, B), N]


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def table():
    return R.table(n=N, n_c=N_C, n_t=N_T, days=60)


def raw_table(cols=None):
    c = dict(cols or table())
    for k in ("customer", "terminal"):
        c[k] = raw_id_scramble(c[k], *RAW_ID_SCRAMBLE[k])
        assert c[k].min() > 2 ** 40
    return c


def forest(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def args(cols, keys, a, b, dev, fraud=True):
    out = [T(cols[k][a:b], dt, dev) for k, dt in keys]
    return out + [T(cols["fraud"][a:b], torch.uint8, dev)] if fraud else out


_dense = {}


def dense_run(dev, golden, cols_key="table"):
    """The dense scorers over the original ids, once: per batch the unfused path's X and
    probabilities and the fused path's probabilities (labels inline)."""
    if cols_key not in _dense:
        cols = table()
        f = forest(golden)
        un, fu = StreamScorer(f, N_C, N_T, max_batch=B, fused=False), StreamScorer(f, N_C, N_T, max_batch=B)
        X, pu, pf = [], [], []
        for a, b in zip(CUTS[:-1], CUTS[1:]):
            pu.append(un.score(*args(cols, KEYS, a, b, dev)).cpu().numpy().copy())
            X.append(un.X[:b - a].cpu().numpy().copy())
            pf.append(fu.score(*args(cols, KEYS, a, b, dev)).cpu().numpy().copy())
        un.finish()
        fu.finish()
        _dense[cols_key] = dict(X=X, pu=pu, pf=pf, snap=bytes(fu.snapshot().cpu().numpy()))
    return _dense[cols_key]


def first_seen(col):
    """per batch: does it bring a key no earlier batch had"""
    seen, out = set(), []
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        new = set(col[a:b].tolist()) - seen
        out.append(bool(new))
        seen |= new
    return out


def test_stream_parity_eager_and_graph(dev, golden):
    want = dense_run(dev, golden)
    raw = raw_table()
    f = forest(golden)
    un = StreamScorer(f, N_C, N_T, max_batch=B, fused=False, raw_ids=True)
    fu = StreamScorer(f, N_C, N_T, max_batch=B, raw_ids=True)
    gr = StreamScorer(f, N_C, N_T, max_batch=B, raw_ids=True)
    keys5 = RAW_KEYS + (("fraud", torch.uint8),)
    stage = {k: torch.empty(B, dtype=dt, device=dev) for k, dt in keys5}
    brings = [c or t for c, t in zip(first_seen(raw["customer"]), first_seen(raw["terminal"]))]
    assert brings[0] and not all(brings[1:]) and not brings[-2]
    first_graph = None
    for j, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        np.testing.assert_array_equal(un.score(*args(raw, RAW_KEYS, a, b, dev)).cpu().numpy(), want["pu"][j])
        np.testing.assert_array_equal(un.X[:b - a].cpu().numpy(), want["X"][j])
        np.testing.assert_array_equal(fu.score(*args(raw, RAW_KEYS, a, b, dev)).cpu().numpy(), want["pf"][j])
        for (k, _), t in zip(keys5, args(raw, RAW_KEYS, a, b, dev)):
            stage[k][:b - a].copy_(t)
        p = gr.score_graph(*(stage[k][:b - a] for k, _ in keys5))
        np.testing.assert_array_equal(p.cpu().numpy(), want["pf"][j])
        if first_graph is None:
            first_graph = next(iter(gr._graphs.values()))
    # one graph for the 257-row batches with and without new keys, one for the ragged last batch
    assert len(gr._graphs) == 2 and next(iter(gr._graphs.values())) is first_graph
    for s in (un, fu, gr):
        s.finish()
        kc = s.key_counts()
        assert kc["customers"] == {"held": N_C, "refused_full": 0, "refused_reserved": 0, "misses": 0}
        assert kc["terminals"] == {"held": N_T, "refused_full": 0, "refused_reserved": 0, "misses": 0}
    # the numbering is first-occurrence order: pandas.factorize of the raw columns
    import pandas as pd

    for s in (fu, gr):
        k = s.snapshot_keys()
        np.testing.assert_array_equal(k["customers"].cpu().numpy(), pd.factorize(raw["customer"])[1])
        np.testing.assert_array_equal(k["terminals"].cpu().numpy(), pd.factorize(raw["terminal"])[1])
    assert bytes(fu.snapshot().cpu().numpy()) == bytes(gr.snapshot().cpu().numpy())


def test_reports_with_raw_terminal_ids(dev, golden):
    cols, raw = table(), raw_table()
    ts = cols["ts"]
    due = R.schedule(ts, cols["fraud"], np.full(N, 3 * R.DAY), CUTS, "after")
    assert sum(len(d) for d in due[:-1]) > 20
    f = forest(golden)
    dn, rw = StreamScorer(f, N_C, N_T, max_batch=B), StreamScorer(f, N_C, N_T, max_batch=B, raw_ids=True)
    for j, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        for o in range(0, len(due[j]), B):
            d = due[j][o:o + B]
            dn.report_frauds(T(ts[d], torch.int64, dev), T(cols["terminal"][d], torch.int32, dev))
            rw.report_frauds(T(ts[d], torch.int64, dev), T(raw["terminal"][d], torch.int64, dev))
        want = dn.score(*args(cols, KEYS, a, b, dev, fraud=False)).cpu().numpy()
        np.testing.assert_array_equal(rw.score(*args(raw, RAW_KEYS, a, b, dev, fraud=False)).cpu().numpy(), want)
    dn.finish()
    rw.finish()
    assert rw.state.label_counts() == dn.state.label_counts() and dn.state.label_counts()["on_time"] > 0
    assert rw.key_counts()["terminals"]["misses"] == 0
    # a report for a terminal the stream never saw: lookup only, -1, raises as an id out of range does
    unseen = raw_id_scramble(np.array([N_T + 5]), *RAW_ID_SCRAMBLE["terminal"])
    rw.report_frauds(T(ts[:1], torch.int64, dev), T(unseen, torch.int64, dev))
    with pytest.raises(_lib.FdxUnsupported, match="outside the state's capacity"):
        rw.finish()
    dn.report_frauds(T(ts[:1], torch.int64, dev), T(np.array([N_T + 5]), torch.int32, dev))
    with pytest.raises(_lib.FdxUnsupported, match="outside the state's capacity"):
        dn.finish()
    kc = rw.key_counts()["terminals"]
    assert kc["misses"] == 1 and kc["held"] == N_T


def _dev_cdc(r, dev):
    return (T(r["tx_id"], torch.int64, dev), T(r["customer"], torch.int64, dev), T(r["terminal"], torch.int64, dev),
            T(r["blob"], torch.uint8, dev), T(r["offsets"], torch.int64, dev), T(r["us"], torch.int64, dev),
            T(r["kts"], torch.int64, dev))


def test_score_cdc_with_raw_ids(dev, golden):
    cols, raw = table(), raw_table()
    f = forest(golden)
    cap = 2 * B
    dn, rw = StreamScorer(f, N_C, N_T, max_batch=cap), StreamScorer(f, N_C + 8, N_T, max_batch=cap, raw_ids=True)
    kts = np.arange(N, dtype=np.int64) * 10 + 1_739_000_000_000
    ghost = int(raw_id_scramble(np.array([N_C + 3]), *RAW_ID_SCRAMBLE["customer"])[0])   # no true record has it
    assert raw["customer"].min() > 2 ** 31 and raw["terminal"].min() > 2 ** 31
    ghosts = 0
    for k, (a, b) in enumerate(zip(CUTS[:4], CUTS[1:5])):
        r = cdc_encode(np.arange(a, b), raw["customer"][a:b], raw["terminal"][a:b], cols["amount"][a:b],
                       cols["ts"][a:b], kts[a:b], dup_frac=0.05, seed=k)
        # the stale updates (the older of two records of a tx_id) carry another customer id
        order = np.lexsort((r["kts"], r["tx_id"]))
        stale = order[:-1][r["tx_id"][order][:-1] == r["tx_id"][order][1:]]
        assert len(stale) >= 5
        r["customer"][stale] = ghost
        ghosts += len(stale)
        p, rows = rw.score_cdc(*_dev_cdc(r, dev))
        np.testing.assert_array_equal(r["tx_id"][rows.cpu().numpy()], np.arange(a, b))
        want = dn.score(*args(cols, KEYS, a, b, dev, fraud=False)).cpu().numpy()
        np.testing.assert_array_equal(p.cpu().numpy(), want)
    dn.finish()
    rw.finish()
    kc = rw.key_counts()
    fed = slice(0, CUTS[4])
    assert ghosts > 0 and kc["customers"]["held"] == len(np.unique(raw["customer"][fed]))
    assert kc["terminals"]["held"] == len(np.unique(raw["terminal"][fed]))
    assert ghost not in rw.snapshot_keys()["customers"].cpu().tolist()


def test_restart_through_files(dev, golden, tmp_path):
    want = dense_run(dev, golden)
    raw = raw_table()
    f = forest(golden)
    a_sc = StreamScorer(f, N_C, N_T, max_batch=B, raw_ids=True)
    half = 5
    for j in range(half):
        a, b = CUTS[j], CUTS[j + 1]
        np.testing.assert_array_equal(a_sc.score(*args(raw, RAW_KEYS, a, b, dev)).cpu().numpy(), want["pf"][j])
    save_snapshot(tmp_path / "state.bin", a_sc.snapshot())
    save_keys(tmp_path / "keys.npz", a_sc.snapshot_keys())
    del a_sc
    with np.load(tmp_path / "keys.npz", allow_pickle=False) as z:     # plain little-endian int64 arrays
        assert sorted(z.files) == ["customers", "terminals"] and all(z[k].dtype == np.dtype("<i8") for k in z.files)
    b_sc = StreamScorer(f, N_C, N_T, max_batch=B, raw_ids=True)
    b_sc.restore(load_snapshot(tmp_path / "state.bin"))
    b_sc.restore_keys(load_keys(tmp_path / "keys.npz"))
    for j in range(half, len(CUTS) - 1):
        a, b = CUTS[j], CUTS[j + 1]
        np.testing.assert_array_equal(b_sc.score(*args(raw, RAW_KEYS, a, b, dev)).cpu().numpy(), want["pf"][j])
    b_sc.finish()
    # raw ids, same arrival order -> the dense run's numbering is NOT what the raw run has, its bytes are its own;
    # an uninterrupted raw run ends in the same bytes and keys as the restarted one
    c_sc = StreamScorer(f, N_C, N_T, max_batch=B, raw_ids=True)
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        c_sc.score(*args(raw, RAW_KEYS, a, b, dev))
    assert bytes(b_sc.snapshot().cpu().numpy()) == bytes(c_sc.snapshot().cpu().numpy())
    for k in ("customers", "terminals"):
        assert torch.equal(b_sc.snapshot_keys()[k], c_sc.snapshot_keys()[k])
    with pytest.raises(_lib.FdxError, match="empty"):
        b_sc.restore_keys(load_keys(tmp_path / "keys.npz"))             # the directories hold keys


def test_grow_mid_stream(dev, golden):
    """Capacity 8 / 8, two batches over 8 customers and 8 terminals, grow(64, 64), the rest of
    the table (40 / 25 keys) == an uninterrupted capacity-64 scorer."""
    cols = dict(table())
    early = np.arange(N) < 2 * B
    for k in ("customer", "terminal"):
        cols[k] = np.where(early, cols[k] % 8, cols[k]).astype(np.int32)
    raw = raw_table(cols)
    assert len(np.unique(raw["customer"][:2 * B])) == 8 and len(np.unique(raw["customer"][:3 * B])) > 8
    f = forest(golden)
    small = StreamScorer(f, 8, 8, max_batch=B, raw_ids=True)
    stuck = StreamScorer(f, 8, 8, max_batch=B, raw_ids=True)
    big = StreamScorer(f, 64, 64, max_batch=B, raw_ids=True)
    keys5 = RAW_KEYS + (("fraud", torch.uint8),)
    stage = {k: torch.empty(B, dtype=dt, device=dev) for k, dt in keys5}
    for j, (a, b) in enumerate(zip(CUTS[:-1], CUTS[1:])):
        if j == 2:
            assert small.key_counts()["customers"]["held"] == 8
            small.grow(n_customers=64, n_terminals=64)
            assert small.state.n_customers == 64 and small.customers.capacity == 64 and not small.__dict__.get("_graphs")
        want = big.score(*args(raw, RAW_KEYS, a, b, dev)).cpu().numpy()
        for (k, _), t in zip(keys5, args(raw, RAW_KEYS, a, b, dev)):
            stage[k][:b - a].copy_(t)
        p = small.score_graph(*(stage[k][:b - a] for k, _ in keys5))   # graphs captured before grow are dropped
        np.testing.assert_array_equal(p.cpu().numpy(), want)
        if j < 2:
            stuck.score(*args(raw, RAW_KEYS, a, b, dev))
    small.finish()
    big.finish()
    assert bytes(small.snapshot().cpu().numpy()) == bytes(big.snapshot().cpu().numpy())
    for k in ("customers", "terminals"):
        assert torch.equal(small.snapshot_keys()[k], big.snapshot_keys()[k])
    assert small.key_counts() == big.key_counts()
    # without grow: the ninth customer is refused (-1) and the next score raises
    stuck.finish()
    stuck.score(*args(raw, RAW_KEYS, CUTS[2], CUTS[3], dev))
    torch.cuda.synchronize()
    with pytest.raises(_lib.FdxUnsupported, match="outside the state's capacity"):
        stuck.score(*args(raw, RAW_KEYS, CUTS[3], CUTS[4], dev))
    kc = stuck.key_counts()
    assert kc["customers"]["held"] == 8 and kc["customers"]["refused_full"] > 0


def test_default_scorer_is_unchanged(dev, golden):
    """raw_ids=False: no directory, dense int32 ids, the probabilities of the state update +
    forest.predict; raw int64 ids are refused by the dtype check."""
    cols = table()
    f = forest(golden)
    sc = StreamScorer(f, N_C, N_T, max_batch=B)
    assert not sc.raw_ids and not hasattr(sc, "customers") and not hasattr(sc, "_cid")
    a5 = args(cols, KEYS, 0, B, dev)
    p = sc.score(*a5).cpu().numpy()
    st = StreamState(N_C, N_T, max_batch=B)
    np.testing.assert_array_equal(p, f.predict(st.update(*a5)).cpu().numpy())
    np.testing.assert_array_equal(p, dense_run(dev, golden)["pf"][0])
    with pytest.raises(_lib.FdxError, match="raw_ids=True"):
        sc.key_counts()
    with pytest.raises(_lib.FdxError, match="int32"):
        sc.score(*args(raw_table(), RAW_KEYS, B, 2 * B, dev))
