"""Snapshot and restore of the streaming state on the GPU (fdx_stream_snapshot / _restore,
k_snap_* in csrc/fdx_stream.hip; StreamState.snapshot / restore / from_snapshot).

A state that is snapshotted, restored into other ring sizes (or other key placements) and fed
the rest of the stream gives the features of the uninterrupted stream and of the oracle; its
bytes are those of the numpy model of tests/stream_snapshot_ref.py.  Inputs are those of
tests/stream_label_ref.py.  Every comparison is an equality of arrays or of bytes."""
import ctypes

import numpy as np
import pytest
import torch

import stream_label_ref as R
import stream_snapshot_ref as S
from fdx import _lib, ops
from fdx.streaming import StreamScorer, StreamState, load_snapshot, save_snapshot, snapshot_info

pytestmark = pytest.mark.gpu

N_C, N_T = 25, 40
RINGS_A, RINGS_B, RINGS_SMALL = (256, 256), (512, 1024), (64, 64)


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def B(snap):
    return bytes(snap.cpu().numpy())


def grid(delay, a, b):
    """The batches [lo, hi) of stream_label_ref.cuts() inside [a, b)"""
    c = R.cuts(R.table()["ts"], delay)
    g = np.unique(np.r_[a, c[(c > a) & (c < b)], b])
    return list(zip(g[:-1], g[1:]))


def stream(st, dev, delay, a, b):
    """Feed rows [a, b) of the table on the cuts() grid, labels inline -> [b - a, 4W]"""
    c = R.table()
    out = np.empty((b - a, 4 * st.W))
    for lo, hi in grid(delay, a, b):
        x = st.update(T(c["ts"][lo:hi], torch.int64, dev), T(c["customer"][lo:hi], torch.int32, dev),
                      T(c["amount"][lo:hi], torch.float64, dev), T(c["terminal"][lo:hi], torch.int32, dev),
                      T(c["fraud"][lo:hi], torch.uint8, dev))
        out[lo - a:hi - a] = x.cpu().numpy()[:, 3:]
    st.check()
    return out


def state(windows, delay, rings=RINGS_A, n_c=N_C, n_t=N_T):
    return StreamState(n_c, n_t, windows, delay, rings[0], rings[1], max_batch=6000)


_prefix, _whole = {}, {}


def prefix(dev, windows, delay, cut):
    """State A (rings 256 / 256) after rows [0, cut): -> (features, snapshot bytes), computed once"""
    k = (windows, delay, cut)
    if k not in _prefix:
        st = state(windows, delay)
        _prefix[k] = (stream(st, dev, delay, 0, cut), B(st.snapshot()))
    return _prefix[k]


def whole(dev, windows, delay):
    """The uninterrupted state A over the whole table: -> (features, final snapshot bytes)"""
    k = (windows, delay)
    if k not in _whole:
        st = state(windows, delay)
        _whole[k] = (stream(st, dev, delay, 0, len(R.table()["ts"])), B(st.snapshot()))
    return _whole[k]


# ------------------------------------------------------------ 1. continue equals uninterrupted
@pytest.mark.parametrize("cut", S.cut_rows())
@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_continue_equals_uninterrupted(dev, windows, delay, cut):
    n = len(R.table()["ts"])
    full, _ = whole(dev, windows, delay)
    want = S.oracle_columns(windows, delay)
    np.testing.assert_array_equal(full, want)
    head, snap = prefix(dev, windows, delay, cut)
    np.testing.assert_array_equal(head, want[:cut])
    st = StreamState.from_snapshot(snap, customer_ring=RINGS_B[0], terminal_ring=RINGS_B[1], max_batch=6000)
    assert (st.windows_days, st.delay_days, st.n_customers, st.n_terminals) == (windows, delay, N_C, N_T)
    tail = stream(st, dev, delay, cut, n)
    np.testing.assert_array_equal(tail, full[cut:])
    np.testing.assert_array_equal(tail, want[cut:])
    if (windows, delay) == R.PARAMS[1]:                    # shrink: the rings only have to hold the live rows
        f = snapshot_info(snap)
        assert f["customer_max_live"] < 32 and f["terminal_max_live"] < 32
        small = StreamState.from_snapshot(snap, customer_ring=RINGS_SMALL[0], terminal_ring=RINGS_SMALL[1],
                                          max_batch=6000)
        np.testing.assert_array_equal(stream(small, dev, delay, cut, n), want[cut:])


# ------------------------------------------------------------------------- 2. canonical bytes
def _without_source_rings(b):
    """The bytes with header words 14 / 15 (the source's ring sizes, include/fdx.h) zeroed"""
    return b[:14 * 8] + bytes(16) + b[16 * 8:]


@pytest.mark.parametrize("cut", S.cut_rows())
@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_bytes_are_canonical(dev, windows, delay, cut):
    _, snap = prefix(dev, windows, delay, cut)
    assert snap == S.model_prefix(windows, delay, cut)[1]
    again = StreamState.from_snapshot(snap, max_batch=64)  # the source's ring sizes: every byte equal
    assert B(again.snapshot()) == snap
    for rings in (RINGS_B, RINGS_SMALL):
        if rings == RINGS_SMALL and max(snapshot_info(snap)[k] for k in ("customer_max_live",
                                                                          "terminal_max_live")) > RINGS_SMALL[0]:
            with pytest.raises(_lib.FdxError, match="live rows"):  # does not fit: refused, not truncated
                StreamState.from_snapshot(snap, customer_ring=rings[0], terminal_ring=rings[1], max_batch=64)
            continue
        st = StreamState.from_snapshot(snap, customer_ring=rings[0], terminal_ring=rings[1], max_batch=64)
        b = B(st.snapshot())
        f = snapshot_info(b)
        assert (f["customer_ring"], f["terminal_ring"]) == rings
        # the header names the ring sizes of the state it came from; every other byte is equal
        assert _without_source_rings(b) == _without_source_rings(snap)


# --------------------------------------------------------------- 3. reports across a restore
class Backend:
    """stream_label_ref.drive's backend over a StreamState fed unlabelled rows; restart_at = a:
    before the batch that starts at row a the state goes through a file into a fresh state."""

    def __init__(self, dev, windows, delay, max_batch, restart_at=None, path=None):
        self.dev, self.W, self.max_batch, self.restart_at, self.path = dev, len(windows), max_batch, restart_at, path
        self.st = StreamState(N_C, N_T, windows, delay, max_batch=max_batch)
        self.X = []

    def update(self, cols, a, b):
        if a == self.restart_at:
            save_snapshot(self.path, self.st.snapshot())
            loaded = load_snapshot(self.path)
            assert loaded.device.type == "cpu" and loaded.is_pinned()
            self.st = StreamState.from_snapshot(loaded, customer_ring=RINGS_B[0], terminal_ring=RINGS_B[1],
                                                max_batch=self.max_batch)
            self.restarted = True
        x = self.st.update(T(cols["ts"][a:b], torch.int64, self.dev), T(cols["customer"][a:b], torch.int32, self.dev),
                           T(cols["amount"][a:b], torch.float64, self.dev),
                           T(cols["terminal"][a:b], torch.int32, self.dev),
                           torch.zeros(b - a, dtype=torch.uint8, device=self.dev)).cpu().numpy()
        self.X.append(x)
        return x[:, 3 + 2 * self.W:]

    def report(self, ts, term):
        self.st.report_frauds(T(np.asarray(ts, np.int64), torch.int64, self.dev),
                              T(np.asarray(term, np.int32), torch.int32, self.dev))


@pytest.mark.parametrize("kind,windows,delay", [("on_time",) + p for p in R.PARAMS] + [("late",) + R.PARAMS[0]])
def test_reports_across_a_restore(dev, tmp_path, kind, windows, delay):
    k = R.case(kind, windows, delay)
    c = k["cuts"]
    mb = int(np.diff(c).max())
    plain = Backend(dev, windows, delay, mb)
    R.drive(plain, k["cols"], c, k["due"])
    plain.st.check()
    mid = int(c[len(c) // 2])                              # in the middle of the drive
    assert sum(len(d) for d in k["due"][:len(c) // 2]) > 0 and sum(len(d) for d in k["due"][len(c) // 2:]) > 0
    be = Backend(dev, windows, delay, mb, restart_at=mid, path=str(tmp_path / "state.snap"))
    R.drive(be, k["cols"], c, k["due"])
    be.st.check()
    assert be.restarted
    np.testing.assert_array_equal(np.concatenate(be.X), np.concatenate(plain.X))
    assert be.st.label_counts() == plain.st.label_counts()
    if kind == "late":
        assert plain.st.label_counts()["late"] == k["late"] > 0


# ----------------------------------------------------------------- 4. rewind under a graph
def test_rewind_under_a_graph(dev, golden):
    z = golden("forest_rf3.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    sc = StreamScorer(ops.Forest(arrays, 15, z["mean"], z["scale"]), N_C, N_T, max_batch=256)
    c = R.table()
    keys = (("ts", torch.int64), ("customer", torch.int32), ("amount", torch.float64), ("terminal", torch.int32))
    bs, k, m = 256, 6, 14
    batch = lambda j: [T(c[name][j * bs:(j + 1) * bs], dt, dev) for name, dt in keys]  # noqa: E731
    for j in range(k):
        sc.score(*batch(j))
    snap = sc.snapshot()
    stage = [torch.empty(bs, dtype=dt, device=dev) for _, dt in keys]

    def replay():
        out = []
        for j in range(k, m):
            for s, t in zip(stage, batch(j)):
                s.copy_(t)
            out.append(sc.score_graph(*stage).cpu().numpy().copy())
        return np.concatenate(out)

    first = replay()
    graphs = dict(sc._graphs)
    assert len(graphs) == 1
    later = B(sc.snapshot())
    sc.restore(snap, counters=False)
    assert B(sc.snapshot()) == B(snap) != later
    again = replay()
    assert sc._graphs == graphs                            # the already captured graph, not a new one
    np.testing.assert_array_equal(again, first)
    assert B(sc.snapshot()) == later
    sc.finish()


# ----------------------------------------------------------------- 5. re-shard on one GPU
def test_reshard_split_and_merge(dev):
    windows, delay = R.PARAMS[0]
    W = len(windows)
    cut = S.cut_rows()[1]
    c = R.table()
    n = len(c["ts"])
    a = state(windows, delay)
    stream(a, dev, delay, 0, cut)
    shards = []
    for r, (base, cnt) in enumerate(((0, 13), (13, 12))):
        st = StreamState.from_snapshot(a.snapshot(customers=(base, cnt, 1), terminals=(r, 20, 2)), max_batch=6000)
        assert (st.n_customers, st.n_terminals) == (cnt, 20)
        shards.append((st, base, cnt, r))
    got = np.full((n - cut, 4 * W), np.nan)
    for lo, hi in grid(delay, cut, n):
        for st, base, cnt, r in shards:
            mine = np.flatnonzero((c["customer"][lo:hi] >= base) & (c["customer"][lo:hi] < base + cnt)) + lo
            if len(mine):                                  # the customer half alone, shard-local ids
                x = st.update(T(c["ts"][mine], torch.int64, dev), T(c["customer"][mine] - base, torch.int32, dev),
                              T(c["amount"][mine], torch.float64, dev))
                got[mine - cut, :2 * W] = x.cpu().numpy()[:, 3:3 + 2 * W]
            mine = np.flatnonzero(c["terminal"][lo:hi] % 2 == r) + lo
            if len(mine):                                  # the terminal half alone, owner-local ids
                x = st.update(T(c["ts"][mine], torch.int64, dev), terminal=T(c["terminal"][mine] // 2, torch.int32, dev),
                              fraud=T(c["fraud"][mine], torch.uint8, dev))
                got[mine - cut, 2 * W:] = x.cpu().numpy()[:, 3 + 2 * W:]
    for st, *_ in shards:
        st.check()
    np.testing.assert_array_equal(got, S.oracle_columns(windows, delay)[cut:])
    merged = state(windows, delay)
    for st, base, cnt, r in shards:                        # the inverse placement; disjoint keys merge
        merged.restore(st.snapshot(), customers_at=(base, 1), terminals_at=(r, 2))
    assert B(merged.snapshot()) == whole(dev, windows, delay)[1]


# ------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_target_unchanged(dev):
    windows, delay = R.PARAMS[0]
    cut = S.cut_rows()[0]
    _, snap = prefix(dev, windows, delay, cut)
    f = snapshot_info(snap)
    assert f["customer_max_live"] > 4

    def fed(win=windows, dly=delay, rings=RINGS_A, rows=300):
        st = state(win, dly, rings)
        stream(st, dev, dly, 0, rows)
        return st

    d_snap = T(np.frombuffer(snap, np.uint8).copy(), torch.uint8, dev)
    for what, target, kw, msg in [
            ("windows differ", fed(win=(1, 7, 29)), {}, "window 2"),
            ("delay differs", fed(dly=6), {}, "delay"),
            ("customer key beyond capacity", fed(), {"customers_at": (1, 1)}, "customer key .* capacity"),
            ("terminal key beyond capacity", fed(), {"terminals_at": (1, 2)}, "terminal key .* capacity"),
            ("ring of 4", fed(rings=(4, 256), rows=5), {}, r"customer key \d+ has \d+ live rows"),
            ("terminal ring of 4", fed(rings=(256, 4), rows=5), {}, r"terminal key \d+ has \d+ live rows"),
            ("one byte short", fed(), {"snap": d_snap[:-1]}, "bytes")]:
        before = B(target.snapshot())
        counts = target.label_counts()
        with pytest.raises(_lib.FdxError, match=msg):
            target.restore(kw.pop("snap", snap), **kw)
        assert B(target.snapshot()) == before, what
        assert target.label_counts() == counts
    # fdx_stream_snapshot itself: a buffer one byte short
    st = fed()
    L, ws = _lib.load(), st._snap_ws()
    need = len(B(st.snapshot()))
    buf = torch.zeros(need, dtype=torch.uint8, device=dev)
    rc = L.fdx_stream_snapshot(st._h, None, None, ops._ptr(buf), need - 1, None, ops._ptr(ws), ws.numel(), ops._s())
    assert rc == -1 and b"snapshot needs" in L.fdx_last_error()
    torch.cuda.synchronize()
    assert not buf.any()
    # a flagged source refuses, and the bit stays for the caller's check()
    base = 1_717_200_000_000_000_000
    bad = StreamState(4, 4, customer_ring=4, terminal_ring=4, max_batch=64)
    z = np.zeros(10, np.int32)
    bad.update(T(base + np.arange(10, dtype=np.int64) * 3_600 * 10**9, torch.int64, dev), T(z, torch.int32, dev),
               T(np.ones(10), torch.float64, dev), T(z, torch.int32, dev), T(np.zeros(10), torch.uint8, dev))
    with pytest.raises(_lib.FdxUnsupported, match="status bits"):
        bad.snapshot()
    with pytest.raises(_lib.FdxUnsupported, match="customer ring overflow"):
        bad.check()


# ---------------------------------------------------------------------- 7. ABI through ctypes
def test_snapshot_entry_points_through_ctypes(dev):
    """Workspace size, size, snapshot and restore with raw pointers, as a C caller would: keys
    with n == 0, a state with only one half, null selections."""
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.fdx_last_error.restype = ctypes.c_char_p
    i64, i32, vp, sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
    L.fdx_stream_create.argtypes = [i64, i64, i32, i32, i32, vp, i64, i32, i64, vp, vp]
    L.fdx_stream_update.argtypes = [vp, vp, vp, vp, vp, vp, i64, vp, i64, i32, vp, vp, vp, vp]
    L.fdx_stream_destroy.argtypes = [vp]
    L.fdx_stream_snapshot_workspace_size.restype = sz
    L.fdx_stream_snapshot_workspace_size.argtypes = [vp]
    L.fdx_stream_snapshot_size.argtypes = [vp, vp, vp, ctypes.POINTER(sz), vp, sz, vp]
    L.fdx_stream_snapshot.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz), vp, sz, vp]
    L.fdx_stream_restore.argtypes = [vp, vp, sz, i64, i64, i64, i64, i32, vp, sz, vp]
    P = lambda t: vp(t.data_ptr())  # noqa: E731
    win = (i64 * 1)(R.DAY)
    ts = T(R.BASE + np.arange(6) * R.H12, torch.int64, dev)
    key = T([1, 3, 1, 1, 3, 1], torch.int32, dev)          # keys 0 and 2 of 4 never see a row
    amt = T(np.arange(6) + 0.25, torch.float64, dev)
    fr = T([0, 1, 0, 0, 0, 1], torch.uint8, dev)
    for half in ("customer", "terminal"):
        nc, nt = (4, 0) if half == "customer" else (0, 4)
        h1, h2 = vp(), vp()
        assert L.fdx_stream_create(nc, nt, 8, 8, 1, win, R.DAY, 0, 8, ctypes.byref(h1), None) == 0, L.fdx_last_error()
        assert L.fdx_stream_create(nc, nt, 16, 16, 1, win, R.DAY, 0, 8, ctypes.byref(h2), None) == 0
        try:
            def feed(h, a, b):
                X = torch.zeros((b - a, 7), dtype=torch.float64, device=dev)
                c = (P(key[a:b]), P(amt[a:b]), None, None) if half == "customer" else (None, None, P(key[a:b]),
                                                                                       P(fr[a:b]))
                assert L.fdx_stream_update(h, P(ts[a:b]), *c, b - a, P(X), 7, -1, None, None, None, None) == 0
                torch.cuda.synchronize()
                return X.cpu().numpy()[:, 3:]

            whole_x = feed(h2, 0, 6)
            assert L.fdx_stream_reset(h2, None) == 0
            feed(h1, 0, 4)
            wsz = L.fdx_stream_snapshot_workspace_size(h1)
            assert wsz > 0
            ws = torch.empty(wsz, dtype=torch.uint8, device=dev)
            nb, wrote = sz(), sz()
            assert L.fdx_stream_snapshot_size(h1, None, None, ctypes.byref(nb), P(ws), wsz, None) == 0, \
                L.fdx_last_error()
            buf = torch.full((nb.value,), 0xAB, dtype=torch.uint8, device=dev)
            assert L.fdx_stream_snapshot(h1, None, None, P(buf), nb.value, ctypes.byref(wrote), P(ws), wsz,
                                         None) == 0, L.fdx_last_error()
            assert wrote.value == nb.value
            f = snapshot_info(buf)
            # rows at 0, 1, 1.5 d of key 1 and 0.5 d of key 3: the customer's 1-day window has dropped
            # the row at 0; the terminal's delay + window boundary (2 d) has passed none
            lives = [0, 2, 0, 1] if half == "customer" else [0, 3, 0, 1]
            assert (f[f"{half}_keys"], f[f"{half}_entries"], f[f"{half}_max_live"]) == (4, sum(lives), max(lives))
            other = "terminal" if half == "customer" else "customer"
            assert (f[f"{other}_keys"], f[f"{other}_entries"], f[f"{other}_ring"]) == (0, 0, 0)
            d = S.decode(B(buf))
            assert [len(e) for _, e in d[half + "s"]] == lives
            assert S.encode(d) == B(buf)                   # every byte, the zero padding included
            assert L.fdx_stream_restore(h2, P(buf), nb.value, 0, 1, 0, 1, 1, P(ws), wsz, None) == 0, L.fdx_last_error()
            np.testing.assert_array_equal(feed(h2, 4, 6), whole_x[4:])
            np.testing.assert_array_equal(feed(h1, 4, 6), whole_x[4:])
            # workspace too small, a selection that leaves the state, a placement beyond the capacity
            assert L.fdx_stream_snapshot_size(h1, None, None, ctypes.byref(nb), P(ws), wsz - 1, None) == -1
            sel = (i64 * 3)(2, 2, 2)
            assert L.fdx_stream_snapshot_size(h1, sel, sel, ctypes.byref(nb), P(ws), wsz, None) == -1
            assert b"selection" in L.fdx_last_error()
            assert L.fdx_stream_restore(h2, P(buf), wrote.value, 1, 1, 1, 1, 0, P(ws), wsz, None) == -1
            assert b"capacity" in L.fdx_last_error()
        finally:
            L.fdx_stream_destroy(h1)
            L.fdx_stream_destroy(h2)
