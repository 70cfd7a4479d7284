"""Delayed fraud reports on the GPU (fdx_stream_report_frauds, k_stream_labels in
csrc/fdx_stream.hip; StreamState.report_frauds / label_counts, StreamScorer.report_frauds).

Rows are streamed unlabelled, the labels arrive later as reports.  Reports that arrive within
the delay give, on every row, the terminal features of the batch path over the true labels;
late ones give the features of the labels known before each batch and leave the state as if
the label had been there all along.  Inputs, driver, references and expected counters are
those of tests/stream_label_ref.py, which tests/test_stream_label_ref.py checks against the
oracle without a GPU.  Every comparison is an equality."""
import ctypes

import numpy as np
import pytest
import torch

import stream_label_ref as R
from fdx import _lib, ops
from fdx.streaming import StreamScorer, StreamState

pytestmark = pytest.mark.gpu


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


class GpuBackend:
    """stream_label_ref.drive's backend over a StreamState: rows fed unlabelled (or with their
    labels inline), both halves when the columns have customers; keeps the whole X."""

    def __init__(self, dev, n_cust, n_term, windows, delay, inline=False, **kw):
        self.dev, self.inline, self.W = dev, inline, len(windows)
        self.st = StreamState(n_cust, n_term, windows, delay, **kw)
        self.X = []

    def update(self, cols, a, b):
        ts, term = T(cols["ts"][a:b], torch.int64, self.dev), T(cols["terminal"][a:b], torch.int32, self.dev)
        fr = T(cols["fraud"][a:b], torch.uint8, self.dev) if self.inline else \
            torch.zeros(b - a, dtype=torch.uint8, device=self.dev)
        if "customer" in cols:
            x = self.st.update(ts, T(cols["customer"][a:b], torch.int32, self.dev),
                               T(cols["amount"][a:b], torch.float64, self.dev), term, fr)
        else:
            x = self.st.update(ts, terminal=term, fraud=fr)
        x = x.cpu().numpy()
        self.X.append(x)
        return x[:, 3 + 2 * self.W:]

    def report(self, ts, term):
        self.st.report_frauds(T(np.asarray(ts, np.int64), torch.int64, self.dev),
                              T(np.asarray(term, np.int32), torch.int32, self.dev))

    def label_counts(self):
        return self.st.label_counts()


def _backend(dev, k, windows, delay, **kw):
    return GpuBackend(dev, 25, 40, windows, delay, max_batch=int(np.diff(k["cuts"]).max()), **kw)


@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_on_time_reports_equal_batch_path_with_true_labels(dev, windows, delay):
    k = R.case("on_time", windows, delay)
    assert k["late"] == 0                                  # the precondition (checked in full on the CPU)
    be = _backend(dev, k, windows, delay)
    X = R.drive(be, k["cols"], k["cuts"], k["due"])
    be.st.check()
    np.testing.assert_array_equal(X, k["true"])
    assert be.label_counts() == {"on_time": int(k["cols"]["fraud"].sum()), "late": 0, "duplicate": 0, "expired": 0,
                                 "unmatched": 0}
    inline = _backend(dev, k, windows, delay, inline=True)   # today's path: labels with the rows
    R.drive(inline, k["cols"], k["cuts"], [d[:0] for d in k["due"]])
    inline.st.check()
    np.testing.assert_array_equal(np.concatenate(be.X), np.concatenate(inline.X))
    assert inline.label_counts() == dict.fromkeys(R.OUTCOMES, 0)


@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_late_reports_equal_labels_known_before_each_batch(dev, windows, delay):
    k = R.case("late", windows, delay)
    be = _backend(dev, k, windows, delay)
    X = R.drive(be, k["cols"], k["cuts"], k["due"])
    be.st.check()
    np.testing.assert_array_equal(X, k["known"])
    a = k["cuts"][-2]                                      # one batch after the last report: the invariant
    np.testing.assert_array_equal(X[a:], k["true"][a:])
    model = R.ModelBackend(40, windows, delay)
    R.drive(model, k["cols"], k["cuts"], k["due"])
    assert be.label_counts() == model.label_counts()
    assert be.label_counts()["late"] == k["late"] > 0


def test_outcomes_at_the_smallest_shapes(dev):
    be = GpuBackend(dev, 0, 2, (1,), 1, terminal_ring=8, max_batch=16)
    assert R.outcome_script(be) == R.OUTCOME_EXPECTED
    # the script reported terminal ids -1 and 2: the key bit, and nothing else, is up
    with pytest.raises(_lib.FdxUnsupported, match="outside the state's capacity") as e:
        be.st.check()
    assert "ring" not in str(e.value) and "back in time" not in str(e.value)
    be.st.check()                                          # cleared
    before = be.label_counts()
    with pytest.raises(_lib.FdxError, match="max_batch"):
        be.report(np.full(17, R.BASE), np.zeros(17))
    L = _lib.load()
    p = ctypes.c_void_p(0x1000)                            # refused before any launch
    assert L.fdx_stream_report_frauds(be.st._h, p, p, 17, None) == -1 and b"max_batch" in L.fdx_last_error()
    assert be.label_counts() == before
    be.st.reset()
    assert be.label_counts() == dict.fromkeys(R.OUTCOMES, 0)
    # a state without terminals takes no reports
    with pytest.raises(_lib.FdxError, match="terminal state"):
        StreamState(4, 0, max_batch=8).report_frauds(T([R.BASE], torch.int64, dev), T([0], torch.int32, dev))


def _forest(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def test_scorer_unlabelled_rows_plus_reports_equal_inline_labels(dev, golden):
    """StreamScorer fed fraud=None plus on-time reports (lag 3 days, 256-row batches, delay 7)
    scores every row as the scorer fed the true labels inline does: through score(), and through
    score_graph() replayed across reports -- the graph captured before the first report is the
    one replayed after it."""
    z = golden("tiny_a.npz")
    o = np.argsort(z["TRANSACTION_ID"], kind="stable")
    cols = {"ts": z["TX_DATETIME"][o], "customer": z["CUSTOMER_ID"][o], "terminal": z["TERMINAL_ID"][o],
            "amount": z["TX_AMOUNT"][o], "fraud": z["TX_FRAUD"][o].astype(np.uint8)}
    ts, n = cols["ts"], len(cols["ts"])
    assert np.all(np.diff(ts) >= 0) and cols["fraud"].sum() > 0
    B = 256                                                # fixed batch size: one graph
    cuts = np.r_[np.arange(0, n, B), n]
    assert R.max_span(ts, cuts) < 3 * R.DAY                # lag 3 d + a batch's span < delay 7 d
    due = R.schedule(ts, cols["fraud"], np.full(n, 3 * R.DAY), cuts, "after")
    assert R.fed_late(cols, cuts, due, 7) == 0 and sum(len(d) for d in due[:-1]) > 0
    forest = _forest(golden)
    n_c, n_t = int(cols["customer"].max()) + 1, int(cols["terminal"].max()) + 1
    keys = (("ts", torch.int64), ("customer", torch.int32), ("amount", torch.float64), ("terminal", torch.int32))
    ref_sc, sc, gr = (StreamScorer(forest, n_c, n_t, max_batch=B) for _ in range(3))
    stage = {k: torch.empty(B, dtype=dt, device=dev) for k, dt in keys}
    first_graph, reports_before_replay = None, 0
    for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        args = [T(cols[k][a:b], dt, dev) for k, dt in keys]
        want = ref_sc.score(*args, T(cols["fraud"][a:b], torch.uint8, dev)).cpu().numpy()
        if len(due[j]):
            rt, rk = T(ts[due[j]], torch.int64, dev), T(cols["terminal"][due[j]], torch.int32, dev)
            sc.report_frauds(rt, rk)
            gr.report_frauds(rt, rk)
            reports_before_replay += first_graph is not None
        np.testing.assert_array_equal(sc.score(*args, None).cpu().numpy(), want)
        for (kk, _), t in zip(keys, args):
            stage[kk][:b - a].copy_(t)
        p = gr.score_graph(*(stage[kk][:b - a] for kk, _ in keys))
        np.testing.assert_array_equal(p.cpu().numpy(), want)
        if first_graph is None:
            assert not len(due[j])                         # captured before the first report
            first_graph = next(iter(gr._graphs.values()))
    assert reports_before_replay > 0
    assert len(gr._graphs) == (1 if n % B == 0 else 2) and next(iter(gr._graphs.values())) is first_graph
    for s in (ref_sc, sc, gr):
        s.finish()
    applied = sum(len(d) for d in due[:-1])
    want_counts = {"on_time": applied, "late": 0, "duplicate": 0, "expired": 0, "unmatched": 0}
    assert sc.state.label_counts() == want_counts and gr.state.label_counts() == want_counts
    # the labels did matter: unlabelled rows without reports score differently somewhere
    none = StreamScorer(forest, n_c, n_t, max_batch=n)
    full = StreamScorer(forest, n_c, n_t, max_batch=n)
    args = [T(cols[k], dt, dev) for k, dt in keys]
    assert not torch.equal(none.score(*args), full.score(*args, T(cols["fraud"], torch.uint8, dev)))


def test_report_entry_points_through_ctypes(dev):
    """fdx_stream_report_frauds / fdx_stream_label_counts with raw pointers, as a C caller would."""
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.fdx_last_error.restype = ctypes.c_char_p
    i64, vp = ctypes.c_int64, ctypes.c_void_p
    L.fdx_stream_create.argtypes = [i64, i64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, vp, i64, ctypes.c_int32,
                                    i64, vp, vp]
    L.fdx_stream_update.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp, i64, ctypes.c_int32, vp, vp, vp, vp]
    L.fdx_stream_report_frauds.argtypes = [vp, vp, vp, i64, vp]
    L.fdx_stream_label_counts.argtypes = [vp, ctypes.POINTER(i64), vp]
    L.fdx_stream_destroy.argtypes = [vp]
    h = vp()
    win = (i64 * 1)(R.DAY)
    assert L.fdx_stream_create(0, 3, 0, 8, 1, win, R.DAY, 0, 8, ctypes.byref(h), None) == 0, L.fdx_last_error()
    try:
        ts = T(R.BASE + np.arange(4) * R.H12, torch.int64, dev)            # rows at 0, 0.5, 1, 1.5 d
        term = T(np.full(4, 2), torch.int32, dev)
        X = torch.zeros((4, 7), dtype=torch.float64, device=dev)
        fr = torch.zeros(4, dtype=torch.uint8, device=dev)
        P = lambda t: vp(t.data_ptr())  # noqa: E731
        assert L.fdx_stream_update(h, P(ts), None, None, P(term), P(fr), 4, P(X), 7, -1, None, None, None, None) == 0
        assert L.fdx_stream_report_frauds(h, P(ts[:1]), P(term[:1]), 1, None) == 0, L.fdx_last_error()
        assert L.fdx_stream_report_frauds(h, None, None, 0, None) == 0
        c = (i64 * 5)(*[-1] * 5)
        assert L.fdx_stream_label_counts(h, c, None) == 0, L.fdx_last_error()
        assert list(c) == [0, 1, 0, 0, 0]      # late: the row at 1 d had moved the delay boundary past row 0
        # the corrected state: at 2 d, (t - 2 d, t - 1 d] holds rows 0.5 d and 1 d; row 0 (the label) is out
        t2 = T([R.BASE + 2 * R.DAY], torch.int64, dev)
        assert L.fdx_stream_update(h, P(t2), None, None, P(term[:1]), P(fr), 1, P(X), 7, -1, None, None, None,
                                   None) == 0
        torch.cuda.synchronize()
        assert X[0, 5:].tolist() == [2.0, 0.0]
        assert X[2, 5:].tolist() == [1.0, 0.0] and X[3, 5:].tolist() == [2.0, 0.0]  # emitted before the report
    finally:
        L.fdx_stream_destroy(h)
