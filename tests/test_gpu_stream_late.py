"""Late terminal rows on the GPU (f-8): k_stream_process<W, true> in csrc/fdx_stream.hip,
fdx_stream_set_terminal_lateness / fdx_stream_late_counts, StreamState(terminal_lateness_days=...)
and StreamScorer.score_graph with a lateness.

Inputs, model, scripts and hand-worked expectations are those of tests/stream_late_ref.py, which
tests/test_stream_late_ref.py checks against the C oracle without a GPU.  Every batch goes
through both output forms (count records and X columns) and every comparison is an equality.
Every refusal here is a status bit; all accesses stay inside the ring."""
import ctypes

import numpy as np
import pytest
import torch

import stream_late_ref as R
from fdx import _lib, ops
from fdx.streaming import StreamScorer, StreamState

pytestmark = pytest.mark.gpu


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


class GpuBackend:
    """The backend of stream_late_ref's drivers over TWO StreamStates (terminal half only) fed the
    same batches: one writes count records, the other X columns; update() checks that the two
    forms agree and returns (NB, FRAUD) decoded from the records."""

    def __init__(self, dev, ring=64, lateness_days=0.0, max_batch=64, states=None):
        self.dev = dev
        self.rec, self.x = states or [StreamState(0, R.N_TERM, R.WINDOWS, R.DELAY, terminal_ring=ring,
                                                  max_batch=max_batch, terminal_lateness_days=lateness_days)
                                      for _ in range(2)]

    def update(self, ts, term, fraud):
        n, W = len(ts), len(R.WINDOWS)
        a = (T(np.asarray(ts, np.int64), torch.int64, self.dev), None, None,
             T(np.asarray(term, np.int32), torch.int32, self.dev), T(np.asarray(fraud, np.uint8), torch.uint8, self.dev))
        words = torch.full((n, W), -1, dtype=torch.int64, device=self.dev)
        self.rec.update(*a, term_records=words)
        X = torch.full((n, 3 + 4 * W), -1.0, dtype=torch.float64, device=self.dev)
        self.x.update(*a, X=X)
        w = words.cpu().numpy()
        nb, fr = w & 0xFFFFFFFF, w >> 32
        np.testing.assert_array_equal(X.cpu().numpy()[:, 3 + 2 * W:], R.columns(nb, fr))
        return nb, fr

    def take_status(self):
        f = [ctypes.c_int32(), ctypes.c_int32()]
        for st, v in zip((self.rec, self.x), f):
            _lib.check(_lib.load().fdx_stream_status(st._h, ctypes.byref(v), None), "fdx_stream_status")
        assert f[0].value == f[1].value
        return f[0].value

    def late_counts(self):
        c = self.rec.late_counts()
        assert c == self.x.late_counts()
        return c

    def reset(self):
        self.rec.reset()
        self.x.reset()

    def restore(self):
        late = self.rec.terminal_lateness_ns / R.DAY
        self.rec, self.x = [StreamState.from_snapshot(s.snapshot(), max_batch=s.max_batch, terminal_lateness_days=late)
                            for s in (self.rec, self.x)]
        assert self.rec.restored and self.rec.terminal_ring == 64 and self.rec.n_terminals == R.N_TERM


def test_lateness_within_delay_is_the_batch_path_over_the_sorted_history(dev):
    h, k = R.history(), R.disordered(6.0)
    assert k["n_late"] > 40 and k["worst"] <= 6 * R.DAY      # the preconditions (checked in full on the CPU)
    want = R.oracle_columns(h["ts"], h["terminal"], h["fraud"])
    be = GpuBackend(dev, lateness_days=7.0)
    nb, fr = R.drive(be, h, k["order"], k["cuts"])
    assert be.take_status() == 0
    np.testing.assert_array_equal(R.columns(nb, fr), want)
    assert be.late_counts() == {"late_rows": k["n_late"], "late_past_delay": 0}
    # the state is that of the in-order stream, byte for byte
    n = len(h["ts"])
    ino = GpuBackend(dev)
    nb0, fr0 = R.drive(ino, h, np.arange(n), R.in_order_cuts(n))
    np.testing.assert_array_equal(R.columns(nb0, fr0), want)
    assert ino.late_counts() == {"late_rows": 0, "late_past_delay": 0}
    for a, b in ((be.rec, ino.rec), (be.x, ino.x)):
        assert torch.equal(a.snapshot(), b.snapshot())
    # the same input with the default lateness is refused
    off = GpuBackend(dev)
    R.drive(off, h, k["order"], k["cuts"])
    with pytest.raises(_lib.FdxUnsupported, match="went back in time") as e:
        off.rec.check()
    assert "ring" not in str(e.value)


def test_lateness_past_delay_equals_the_model(dev):
    h, k = R.history(), R.disordered(10.0, lag_until_day=30)
    assert k["n_late"] > 40 and 7 * R.DAY < k["worst"] <= 10 * R.DAY
    model = R.StreamLateModel(lateness_days=12.0)
    mnb, mfr = R.drive(model, h, k["order"], k["cuts"])
    be = GpuBackend(dev, lateness_days=12.0)
    nb, fr = R.drive(be, h, k["order"], k["cuts"])
    assert be.take_status() == 0 == model.take_status()
    np.testing.assert_array_equal(nb, mnb)
    np.testing.assert_array_equal(fr, mfr)
    after = k["order"][k["cuts"][k["last_late"] + 1]:]
    want = R.oracle_columns(h["ts"], h["terminal"], h["fraud"])
    assert len(after) > 100
    np.testing.assert_array_equal(R.columns(nb, fr)[after], want[after])
    c = be.late_counts()
    assert c == model.late_counts() and 0 < c["late_past_delay"] < c["late_rows"] == k["n_late"]


def test_ring_of_8(dev):
    be = GpuBackend(dev, ring=8, lateness_days=40.0)
    assert R.ring8_script(be) == R.RING8_EXPECTED
    assert be.late_counts() == {"late_rows": 4, "late_past_delay": 4}   # days 65, 40, 30 and 39; not day 75
    # the refused row (terminal 0, day 75) left no trace: terminal 0's record and live ring are
    # those of a state that never saw it (n included: the snapshot carries n - min p[k])
    twin = GpuBackend(dev, ring=8, lateness_days=40.0)
    for k in range(10):
        R.feed(twin, [(10 * k, 0, k % 2)])
    for day in (65, 100, 110):
        R.feed(twin, [(day, 0, int(day == 65))])
    assert twin.take_status() == 0
    a, b = be.rec.snapshot(terminals=(0, 1, 1)), twin.rec.snapshot(terminals=(0, 1, 1))
    assert torch.equal(a, b)


def test_ties(dev):
    be, model = GpuBackend(dev, lateness_days=40.0), R.StreamLateModel(lateness_days=40.0)
    rows, nb, fr = R.ties_script(be)
    _, mnb, mfr = R.ties_script(model)
    np.testing.assert_array_equal(nb, mnb)
    np.testing.assert_array_equal(fr, mfr)
    assert be.take_status() == 0 and be.late_counts() == model.late_counts() == {"late_rows": 6, "late_past_delay": 6}


def test_too_late_row_is_refused_and_reset_clears(dev):
    be = GpuBackend(dev, lateness_days=12.0)
    assert R.too_late_script(be) == R.TOO_LATE_EXPECTED
    with pytest.raises(_lib.FdxError, match="negative"):
        be.rec.set_terminal_lateness(-1)
    assert be.rec.terminal_lateness_ns == 12 * R.DAY


def test_reports_on_inserted_rows(dev):
    """A late row fed unlabelled and reported afterwards leaves the features, and a state, equal to
    those of the same stream with the label on the row.  Day 12 lands 18 days behind day 30: the
    delay boundary had passed it (late report); day 28 lands 2 days behind: on time."""
    def stream(be, label):
        out = []
        for b in ([(5, 4, 1)], [(10, 4, 0)], [(30, 4, 0)], [(28, 4, label)], [(12, 4, label)]):
            out.append(R.feed(be, b))
        return out

    rep, inl = GpuBackend(dev, lateness_days=20.0), GpuBackend(dev, lateness_days=20.0)
    assert stream(rep, 0) == stream(inl, 1)                   # a row's own label is no part of its features
    for st in (rep.rec, rep.x):
        st.report_frauds(T([R.d(12), R.d(28)], torch.int64, dev), T([4, 4], torch.int32, dev))
    assert rep.rec.label_counts() == rep.x.label_counts() == {"on_time": 1, "late": 1, "duplicate": 0, "expired": 0,
                                                              "unmatched": 0}
    assert inl.rec.label_counts() == dict.fromkeys(rep.rec.label_counts(), 0)
    # day 36: (28, 29] holds nothing, (22, 29] holds 28, (-1, 29] holds 5, 10, 12, 28 (fraud: 5, 12, 28)
    for be in (rep, inl):
        assert R.feed(be, [(36, 4, 0)]) == ([[0, 1, 4]], [[0, 1, 3]]) and be.take_status() == 0
    assert rep.late_counts() == inl.late_counts() == {"late_rows": 2, "late_past_delay": 1}
    assert torch.equal(rep.rec.snapshot()[512:], inl.rec.snapshot()[512:])   # all but the header's label counters


def test_after_a_restore(dev):
    be = GpuBackend(dev, lateness_days=12.0)
    assert R.restore_script(be) == R.RESTORE_EXPECTED
    be.reset()                                               # the reset state is a fresh one again
    assert not be.rec.restored
    R.feed(be, [(90, 2, 0)])
    R.feed(be, [(100, 2, 1)])
    assert R.feed(be, [(95, 2, 1)]) == R.ZERO and be.take_status() == 0
    assert be.late_counts() == {"late_rows": 1, "late_past_delay": 0}


def _forest(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def test_score_graph_with_late_rows(dev, golden):
    """The customers with id % 3 == 0 deliver one batch behind the others (a slow partition): every
    customer's rows stay in order, the terminals' do not.  score_graph equals score batch for
    batch, and changing the lateness drops the captured graphs."""
    z = golden("tiny_a.npz")
    o = np.argsort(z["TRANSACTION_ID"], kind="stable")[:1536]
    cols = {"ts": z["TX_DATETIME"][o], "customer": z["CUSTOMER_ID"][o], "terminal": z["TERMINAL_ID"][o],
            "amount": z["TX_AMOUNT"][o], "fraud": z["TX_FRAUD"][o].astype(np.uint8)}
    n, B = len(o), 256
    slow = cols["customer"] % 3 == 0
    batches = [np.flatnonzero((np.arange(n) // B == j) & ~slow).tolist() + np.flatnonzero((np.arange(n) // B == j - 1) & slow).tolist()
               for j in range(n // B + 1)]
    span = max(cols["ts"][min(n - 1, (j + 1) * B - 1)] - cols["ts"][max(0, (j - 1) * B)] for j in range(n // B + 1))
    assert span < 7 * R.DAY and slow.sum() > 100
    n_c, n_t = int(cols["customer"].max()) + 1, int(cols["terminal"].max()) + 1
    forest = _forest(golden)
    keys = (("ts", torch.int64), ("customer", torch.int32), ("amount", torch.float64), ("terminal", torch.int32),
            ("fraud", torch.uint8))
    assert max(len(b) for b in batches) <= 2 * B and len(z["TRANSACTION_ID"]) >= n
    sc, gr = (StreamScorer(forest, n_c, n_t, max_batch=2 * B, terminal_lateness_days=7) for _ in range(2))
    stage = {k: torch.empty(2 * B, dtype=dt, device=dev) for k, dt in keys}
    for j, rows in enumerate(batches):
        if j == 3:                                           # re-capture: the value is a kernel argument
            seen = dict(gr._graphs)
            gr.set_terminal_lateness(7)                      # unchanged: the graphs stay
            assert gr._graphs == seen
            gr.set_terminal_lateness(6.5)
            sc.set_terminal_lateness(6.5)
            assert "_graphs" not in gr.__dict__
        args = [T(cols[k][rows], dt, dev) for k, dt in keys]
        want = sc.score(*args).cpu().numpy()
        for (k, _), t in zip(keys, args):
            stage[k][:len(rows)].copy_(t)
        got = gr.score_graph(*(stage[k][:len(rows)] for k, _ in keys))
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        assert all(key[-3:] == ("late", gr.state.terminal_lateness_ns, False) for key in gr._graphs)
    sc.finish()
    gr.finish()
    c = sc.state.late_counts()
    assert c == gr.state.late_counts() and c["late_rows"] > 50 and c["late_past_delay"] == 0
    # the default scorer refuses the same stream
    off = StreamScorer(forest, n_c, n_t, max_batch=2 * B)
    with pytest.raises(_lib.FdxUnsupported, match="went back in time"):
        for rows in batches:
            off.score(*[T(cols[k][rows], dt, dev) for k, dt in keys])
        off.finish()
