"""StreamScorer.retire_idle (f-10): idle keys are retired, their ids, state rows and hash slots
are reused, and nothing about the features changes.

The streams are tests/retire_ref.py's tables (era_table: the ids change every 50 days; gap_table:
12 customers and 8 terminals pause for longer than their horizon and return) under scrambled
64-bit ids, in batches of 257, with the forest_rf5d8 golden.  The reference of every feature and
probability is the dense scorer over the factorized full table, which in turn equals the oracle
over the whole history (tests/test_gpu_stream.py); states are compared as snapshot bytes.  Every
comparison is an equality."""
import numpy as np
import pandas as pd
import pytest
import torch

import retire_ref as M
from fdx import _lib, ops
from fdx.streaming import StreamScorer, load_keys, load_snapshot, save_keys, save_snapshot

pytestmark = pytest.mark.gpu

B = M.B
DAY = M.DAY
KEYS = (("ts", torch.int64), ("customer", torch.int32), ("amount", torch.float64), ("terminal", torch.int32))
RAW_KEYS = tuple((k, torch.int64 if k in ("customer", "terminal") else dt) for k, dt in KEYS)


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def forest(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def args(cols, keys, rows, dev, fraud=True):
    out = [T(cols[k][rows], dt, dev) for k, dt in keys]
    return out + [T(cols["fraud"][rows], torch.uint8, dev)] if fraud else out


def tables(name):
    """-> (raw columns, the same with pandas.factorize ids, batch cuts)"""
    raw = M.raw(M.era_table() if name == "era" else M.gap_table())
    dense = dict(raw)
    for k in ("customer", "terminal"):
        dense[k] = pd.factorize(raw[k])[0].astype(np.int32)
    return raw, dense, M.cuts(len(raw["ts"]))


_ref = {}


def reference(name, dev, golden):
    """The dense scorers over the factorized full table, once per table: per batch the unfused
    path's X and probabilities and the fused path's probabilities."""
    if name not in _ref:
        _, dense, c = tables(name)
        n_c, n_t = int(dense["customer"].max()) + 1, int(dense["terminal"].max()) + 1
        f = forest(golden)
        un, fu = StreamScorer(f, n_c, n_t, max_batch=B, fused=False), StreamScorer(f, n_c, n_t, max_batch=B)
        X, pu, pf = [], [], []
        for a, b in zip(c[:-1], c[1:]):
            pu.append(un.score(*args(dense, KEYS, slice(a, b), dev)).cpu().numpy().copy())
            X.append(un.X[:b - a].cpu().numpy().copy())
            pf.append(fu.score(*args(dense, KEYS, slice(a, b), dev)).cpu().numpy().copy())
        un.finish()
        fu.finish()
        _ref[name] = dict(X=X, pu=pu, pf=pf)
    return _ref[name]


def snap(sc):
    return bytes(sc.snapshot().cpu().numpy())


def add(tot, r):
    tot[0] += r["customers"]["retired"]
    tot[1] += r["terminals"]["retired"]


@pytest.mark.parametrize("fused", [False, True])
def test_capacity_is_reused(dev, golden, fused):
    """160 customers and 100 terminals pass through directories and a state of 80 / 50."""
    raw, _, c = tables("era")
    want = reference("era", dev, golden)
    f = forest(golden)
    sc = StreamScorer(f, 80, 50, max_batch=B, fused=fused, raw_ids=True)
    tot, peak = [0, 0], [0, 0]
    for j, (a, b) in enumerate(zip(c[:-1], c[1:])):
        if j % 2 == 0:
            wm = int(raw["ts"][a])
            add(tot, sc.retire_idle(np.datetime64(wm, "ns") if j % 4 == 0 else wm))
        p = sc.score(*args(raw, RAW_KEYS, slice(a, b), dev)).cpu().numpy()
        np.testing.assert_array_equal(p, want["pf" if fused else "pu"][j], err_msg=f"batch {j}")
        if not fused:
            np.testing.assert_array_equal(sc.X[:b - a].cpu().numpy(), want["X"][j], err_msg=f"batch {j}")
        kc = sc.key_counts()
        peak = [max(peak[0], kc["customers"]["held"]), max(peak[1], kc["terminals"]["held"])]
    sc.finish()
    kc = sc.key_counts()
    assert kc["customers"]["refused_full"] == 0 and kc["terminals"]["refused_full"] == 0
    assert peak == [80, 50] and tot == [120, 75]
    # the same stream without retire_idle: the directories fill up and the scorer raises
    stuck = StreamScorer(f, 80, 50, max_batch=B, fused=fused, raw_ids=True)
    with pytest.raises(_lib.FdxError, match="outside the state's capacity"):
        for a, b in zip(c[:-1], c[1:]):
            stuck.score(*args(raw, RAW_KEYS, slice(a, b), dev))
        stuck.finish()
    assert stuck.key_counts()["customers"]["refused_full"] > 0


def twin(f, raw, alive_c, alive_t, dev):
    """A second raw-id scorer fed the filtered history: per half, the rows of the keys still held."""
    tw = StreamScorer(f, 40, 25, max_batch=B, fused=False, raw_ids=True)
    st = tw.state
    for o in range(0, len(alive_c), B):
        r = alive_c[o:o + B]
        st.update(T(raw["ts"][r], torch.int64, dev), customer=tw.customers.map(T(raw["customer"][r], torch.int64, dev)),
                  amount=T(raw["amount"][r], torch.float64, dev), X=tw.X[:len(r)])
    for o in range(0, len(alive_t), B):
        r = alive_t[o:o + B]
        st.update(T(raw["ts"][r], torch.int64, dev), terminal=tw.terminals.map(T(raw["terminal"][r], torch.int64, dev)),
                  fraud=T(raw["fraud"][r], torch.uint8, dev),
                  term_records=torch.empty((len(r), 3), dtype=torch.int64, device=dev))
    st.check()
    return tw


def same_state(sc, tw):
    assert snap(sc) == snap(tw)
    ka, kb = sc.snapshot_keys(), tw.snapshot_keys()
    for k in ("customers", "terminals"):
        assert torch.equal(ka[k], kb[k]), k
    assert sc.key_counts() == tw.key_counts()


def test_keys_that_return(dev, golden):
    raw, _, c = tables("gap")
    want = reference("gap", dev, golden)
    cs, ts, log = M.simulate(raw, c, lambda j: True, (40, 25))
    assert (cs.retired, ts.retired) == (12, 8)
    f = forest(golden)
    sc = StreamScorer(f, 40, 25, max_batch=B, fused=False, raw_ids=True)
    tot = [0, 0]
    for j, (a, b) in enumerate(zip(c[:-1], c[1:])):
        r = sc.retire_idle(int(raw["ts"][a]))
        add(tot, r)
        alive_c, alive_t, keys_c, keys_t = log[j]
        assert (r["customers"]["kept"], r["terminals"]["kept"]) == (len(keys_c), len(keys_t))
        same_state(sc, twin(f, raw, alive_c, alive_t, dev))
        k = sc.snapshot_keys()
        np.testing.assert_array_equal(k["customers"].cpu().numpy(), keys_c)
        np.testing.assert_array_equal(k["customers"].cpu().numpy(), pd.factorize(raw["customer"][alive_c])[1])
        np.testing.assert_array_equal(k["terminals"].cpu().numpy(), pd.factorize(raw["terminal"][alive_t])[1])
        p = sc.score(*args(raw, RAW_KEYS, slice(a, b), dev)).cpu().numpy()
        np.testing.assert_array_equal(sc.X[:b - a].cpu().numpy(), want["X"][j], err_msg=f"batch {j}")
        np.testing.assert_array_equal(p, want["pu"][j], err_msg=f"batch {j}")
    sc.finish()
    assert tot == [12, 8]
    same_state(sc, twin(f, raw, cs.alive_rows(), ts.alive_rows(), dev))


def test_score_graph_across_retirements(dev, golden):
    raw, _, c = tables("gap")
    want = reference("gap", dev, golden)
    f = forest(golden)
    eager, gr = (StreamScorer(f, 40, 25, max_batch=B, raw_ids=True) for _ in range(2))
    keys5 = RAW_KEYS + (("fraud", torch.uint8),)
    stage = {k: torch.empty(B, dtype=dt, device=dev) for k, dt in keys5}
    tot, graphs, first = [0, 0], None, None
    for j, (a, b) in enumerate(zip(c[:-1], c[1:])):
        r = gr.retire_idle(int(raw["ts"][a]))
        assert eager.retire_idle(int(raw["ts"][a])) == r
        add(tot, r)
        if graphs is not None:       # the retirement dropped nothing: same dict, same graph for 257 rows
            assert gr._graphs is graphs and next(iter(gr._graphs.values())) is first
        batch = args(raw, RAW_KEYS, slice(a, b), dev)
        pe = eager.score(*batch).cpu().numpy()
        for (k, _), t in zip(keys5, batch):
            stage[k][:b - a].copy_(t)
        pg = gr.score_graph(*(stage[k][:b - a] for k, _ in keys5)).cpu().numpy()
        np.testing.assert_array_equal(pg, pe, err_msg=f"batch {j}")
        np.testing.assert_array_equal(pg, want["pf"][j], err_msg=f"batch {j}")
        if graphs is None:
            graphs, first = gr._graphs, next(iter(gr._graphs.values()))
    eager.finish()
    gr.finish()
    assert tot == [12, 8] and gr._graphs is graphs and len(graphs) == 2      # 257 rows, and the ragged last batch
    assert gr.key_counts() == eager.key_counts() and snap(gr) == snap(eager)


def test_with_late_terminal_rows(dev, golden):
    """The customers with id % 3 == 0 deliver the rows of a batch's last 0.9 days one batch later:
    the terminals see rows out of order, inside a lateness of 1 day.  The watermark is the latest
    ts delivered so far lowered by that lateness; the result equals the run without retirement."""
    raw, dense, c = tables("gap")
    ts = raw["ts"]
    slow = M.gap_table()["customer"] % 3 == 0
    batches, carry = [], np.zeros(0, np.int64)
    for a, b in zip(c[:-1], c[1:]):
        rows = np.arange(a, b)
        late = slow[rows] & (ts[rows] > ts[b - 1] - 9 * DAY // 10)
        batches.append((np.r_[carry, rows[~late]], int(ts[max(a - 1, 0)]) - DAY))   # the latest ts seen - the lateness
        carry = rows[late]
    batches.append((carry, int(ts[-1]) - DAY))
    assert all(len(r) and len(r) <= 2 * B and wm <= ts[r].min() for r, wm in batches)
    f = forest(golden)
    ret, plain = (StreamScorer(f, 40, 25, max_batch=2 * B, raw_ids=True, terminal_lateness_days=1) for _ in range(2))
    tot = [0, 0]
    for j, (rows, wm) in enumerate(batches):
        add(tot, ret.retire_idle(wm))
        got = ret.score(*args(raw, RAW_KEYS, rows, dev)).cpu().numpy()
        want = plain.score(*args(raw, RAW_KEYS, rows, dev)).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"batch {j}")
    ret.finish()
    plain.finish()
    assert tot == [12, 8]
    late = ret.state.late_counts()
    assert late == plain.state.late_counts() and late["late_rows"] > 0


def test_reports_restart_and_grow(dev, golden, tmp_path):
    raw, dense, c = tables("gap")
    ts = raw["ts"]
    f = forest(golden)
    mk = lambda: StreamScorer(f, 40, 25, max_batch=B, raw_ids=True)   # noqa: E731
    ret, plain = mk(), mk()
    sim = M.HalfSim(25, M.horizons()[1])       # which terminals are retired and not back yet
    j_report = None
    tot, twin_sc = [0, 0], None
    for j, (a, b) in enumerate(zip(c[:-1], c[1:])):
        if j_report is not None and j == j_report + 2:   # through files into a new scorer; the old one goes on beside it
            save_snapshot(tmp_path / "state.bin", ret.snapshot())
            save_keys(tmp_path / "keys.npz", ret.snapshot_keys())
            twin_sc, ret = ret, mk()
            ret.restore(load_snapshot(tmp_path / "state.bin"))
            ret.restore_keys(load_keys(tmp_path / "keys.npz"))
        if j_report is not None and j == j_report + 3:
            ret.grow(n_customers=48, n_terminals=32)
            assert ret.state.n_customers == 48 and ret.terminals.capacity == 32
        add(tot, ret.retire_idle(int(ts[a])))
        sim.retire(int(ts[a]))
        sim.feed(raw["terminal"][a:b], ts[a:b])
        away = [k for k in sim.inc if k not in sim.last]
        if twin_sc is not None:
            twin_sc.retire_idle(int(ts[a]))
            twin_sc.score(*args(raw, RAW_KEYS, slice(a, b), dev, fraud=False))
        got = ret.score(*args(raw, RAW_KEYS, slice(a, b), dev, fraud=False)).cpu().numpy()
        want = plain.score(*args(raw, RAW_KEYS, slice(a, b), dev, fraud=False)).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=f"batch {j}")
        if j_report is None and away:
            j_report = j
            assert tot[1] == 8 and j + 4 < len(c)
            # a report for a live row (this batch's last): on time, with and without retirements
            r = np.array([b - 1])
            for s in (ret, plain):
                s.report_frauds(T(ts[r], torch.int64, dev), T(raw["terminal"][r], torch.int64, dev))
                s.finish()
            assert ret.state.label_counts() == plain.state.label_counts()
            assert ret.state.label_counts() == dict(on_time=1, late=0, duplicate=0, expired=0, unmatched=0)
            # a report for a retired terminal: a lookup miss, as for a terminal never seen
            old = np.flatnonzero(raw["terminal"][:a] == away[0])[-1:]
            assert ret.key_counts()["terminals"]["misses"] == 0
            ret.report_frauds(T(ts[old], torch.int64, dev), T(raw["terminal"][old], torch.int64, dev))
            with pytest.raises(_lib.FdxError, match="outside the state's capacity"):
                ret.finish()
            assert ret.key_counts()["terminals"]["misses"] == 1
            assert ret.state.label_counts() == plain.state.label_counts()
    for s in (ret, plain, twin_sc):
        s.finish()
    assert tot == [12, 8]
    # restarted and grown == uninterrupted: the same keys under the same ids, the same bytes for them
    ka, kb = ret.snapshot_keys(), twin_sc.snapshot_keys()
    assert all(torch.equal(ka[k], kb[k]) for k in ka)
    held = (0, ka["customers"].numel(), 1), (0, ka["terminals"].numel(), 1)
    assert bytes(ret.snapshot(*held).cpu().numpy()) == bytes(twin_sc.snapshot(*held).cpu().numpy())


def test_no_op_and_dense_scorers(dev, golden):
    raw, dense, c = tables("gap")
    f = forest(golden)
    sc = StreamScorer(f, 40, 25, max_batch=B, raw_ids=True)
    for a, b in zip(c[:3], c[1:4]):
        sc.score(*args(raw, RAW_KEYS, slice(a, b), dev))
    before, keys = snap(sc), sc.snapshot_keys()
    r = sc.retire_idle(int(raw["ts"][0]) - 1)          # a watermark before the first row
    held = sc.key_counts()
    assert r == {"customers": {"kept": held["customers"]["held"], "retired": 0},
                 "terminals": {"kept": held["terminals"]["held"], "retired": 0}}
    assert snap(sc) == before and all(torch.equal(keys[k], sc.snapshot_keys()[k]) for k in keys)
    with pytest.raises(_lib.FdxError, match="raw_ids=True"):
        StreamScorer(f, 40, 25, max_batch=B).retire_idle(0)
