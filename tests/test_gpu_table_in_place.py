"""The customer half writing its feature-table columns in place (FraudPipeline.table_in_place):
the walk stores cust_nb and the averages straight into the slot-order table
(fdx_customer_windows_walk_strided), the layout fill the row index, and the row assembly reads them
there (FDX_PREP_CUST_IN_TABLE) instead of copying them out of scratch arrays.  Everything must stay
bit-equal to the scratch-array path: proba, every table column of a live slot, row -1 and zero
features in padding slots -- also in a reused table, at the two capacities a caller sizes a table
to, with NaN amounts (a window with nb = 0), and an undersized table must be refused before
anything is written into it.

The table: ~20 k rows of 300 customers / 500 terminals over 40 days, plus one customer of 1,100 rows
(window starts searched outside LDS, the 256-row ring's length class), one of 500 (the two-wave long
class) and two hand-made customers whose rows lie days apart, with a NaN and a -NaN amount among
them: their 1-day and 7-day windows hold no valid amount there."""

import numpy as np
import pytest
import torch

from fdx import _lib, ops, synth
from fdx.pipeline import FraudPipeline
from table_check import assert_same_features, table_as_X

pytestmark = pytest.mark.gpu
N_CUST, N_TERM = 302, 500
DAY = 86_400 * 10**9
NEG_NAN = np.array([0xFFF8000000000000], np.uint64).view(np.float64)[0]


def T(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def _cap(d):
    """Slots for the hand-made table: its 1,100-row customer pads its whole group to 1,100 rows."""
    return 2 * len(d["ts"]) + 4096


def _plain_table():
    d = synth.generate(300, N_TERM, 40, seed=3)
    return {k: d[k] for k in ("ts", "customer", "terminal", "amount", "fraud")}


def _make_table():
    d = _plain_table()
    n0 = len(d["ts"])
    assert 15_000 < n0 < 30_000
    rng = np.random.default_rng(5)
    cust = d["customer"].copy()
    hot = rng.choice(n0, 1_600, replace=False)
    cust[hot[:1_100]] = 5    # > 1,024 rows
    cust[hot[1_100:]] = 9    # >= 480 rows: the long class
    t0 = int(d["ts"].min())
    # customers 300 / 301: rows 8+ days apart; the NaN rows' 1- and 7-day windows hold only themselves
    days = np.array([2, 10, 19, 28, 37])
    ts_x = np.concatenate([t0 + days * DAY + 3_600 * 10**9, t0 + days * DAY + 7_200 * 10**9])
    cust_x = np.repeat(np.array([300, 301], np.int32), 5)
    amt_x = np.array([10.0, np.nan, 30.5, 7.25, 1.0, 4.0, 5.5, NEG_NAN, 8.0, 9.75])
    ts = np.concatenate([d["ts"], ts_x])
    o = np.argsort(ts, kind="stable")
    cat = lambda a, b: np.concatenate([a, b])[o]  # noqa: E731
    return dict(ts=ts[o], customer=cat(cust, cust_x), terminal=cat(d["terminal"], np.array([3] * 10, np.int32)),
                amount=cat(d["amount"], amt_x), fraud=cat(d["fraud"], np.zeros(10, np.uint8)))


@pytest.fixture(scope="module")
def table():
    return _make_table()


@pytest.fixture(scope="module")
def forest(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def _args(d, dev):
    return (T(d["ts"], torch.int64, dev), T(d["customer"], torch.int32, dev), T(d["terminal"], torch.int32, dev),
            T(d["amount"], torch.float64, dev), T(d["fraud"], torch.uint8, dev))


def _run(forest, d, dev, in_place, rows, overlap=True):
    """-> (proba, the table's columns over the step's slots as numpy, slot count)"""
    pipe = FraudPipeline(forest=forest)
    pipe.table_in_place = in_place
    proba = torch.empty(len(d["ts"]), dtype=torch.float64, device=dev)
    pipe.run_fused(*_args(d, dev), N_CUST, N_TERM, proba, rows_out=rows, overlap=overlap)
    torch.cuda.synchronize()
    cols = None
    if isinstance(rows, ops.FeatureTable):
        cols = {k: v.cpu().numpy().copy() for k, v in rows.columns(pipe.last_slots).items()}
    return proba.cpu().numpy(), cols, pipe.last_slots


def _table(cap, dev, fill=0xAB):
    rows = ops.FeatureTable(cap, dev)
    rows.buf.fill_(fill)
    return rows


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _assert_same_columns(got, want, what):
    for k in want:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg=f"{what}: column {k}")


def _assert_padding(rows, n_slots, what):
    """row -1 and zero features in every padding slot below round_up(n_slots, 64)"""
    end = (n_slots + 63) // 64 * 64
    col = {k: v.cpu().numpy() for k, v in rows.columns(end).items()}
    pad = np.ones(end, bool)
    pad[:n_slots] = col["row"][:n_slots] < 0
    assert pad[n_slots:].all() and (col["row"][pad] == -1).all(), what
    for k in ("cust_nb", "term_nb", "cust_avg", "term_risk"):
        assert not _bits(col[k][:, pad]).any(), f"{what}: {k} of a padding slot"
    assert not col["weekend"][pad].any() and not col["night"][pad].any(), what


@pytest.fixture(scope="module")
def scratch_path(dev, table, forest):
    """The reference of every step-level test: the scratch-array path (table_in_place = 0)."""
    rows = _table(_cap(table), dev)
    assert forest.in_table_ok(3, rows), "the test forest must take the in-place path"
    proba, cols, slots = _run(forest, table, dev, 0, rows)
    return proba, cols, slots, table_as_X(rows, slots, table["amount"])


# ---------------------------------------------------------------------------- 1. the walk
@pytest.fixture(scope="module")
def layout(dev, table):
    ts, cust, _, amt, _ = _args(table, dev)
    cperm, cseg, gts, gamt = ops.rekey_payload(cust, N_CUST, ts, amt)
    plan = ops.customer_layout_plan(cseg, 3)
    lay = ops.customer_layout_fill(plan, cseg, cperm, gts, gamt, (1, 7, 30))
    nb, sm = ops.customer_windows_walk(lay, cseg)
    torch.cuda.synchronize()
    seg_len = (cseg[1:] - cseg[:-1]).cpu().numpy()
    assert seg_len.max() > 1_024 and ((seg_len >= 480) & (seg_len <= 1_024)).any()
    return lay, cseg, nb, sm


@pytest.mark.parametrize("extra", [0, 64])
def test_walk_strided_equals_walk(dev, layout, extra):
    lay, cseg, nb, sm = layout
    m = lay.n_slots
    stride = m + extra
    live = lay.irow[:m] >= 0
    assert int(live.sum()) < m, "the layout has padding slots"
    L = _lib.load()
    for is_avg in (1, 0):
        nb2 = torch.full((3, stride), -77, dtype=torch.int32, device=dev)
        val2 = torch.full((3, stride), -1234.5, dtype=torch.float64, device=dev)
        rc = L.fdx_customer_windows_walk_strided(
            lay.iamt.data_ptr(), cseg.data_ptr(), lay.sorder.data_ptr(), lay.goff.data_ptr(), cseg.numel() - 1, m, 3,
            lay.starts.data_ptr(), nb2.data_ptr(), stride, val2.data_ptr(), stride, is_avg,
            torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "fdx_customer_windows_walk_strided")
        torch.cuda.synchronize()
        assert torch.equal(nb2[:, :m][:, live], nb[:, live])
        want = sm / nb.to(torch.float64) if is_avg else sm  # torch float64 on the device: IEEE division
        assert int((nb[:, live] == 0).sum()) > 0, "rows with nb == 0 (NaN / 0.0)"
        assert torch.equal(val2[:, :m][:, live].view(torch.int64), want[:, live].view(torch.int64))
        # padding slots and the columns between n_slots and the stride: untouched
        assert bool((nb2[:, :m][:, ~live] == -77).all()) and bool((val2[:, :m][:, ~live] == -1234.5).all())
        assert bool((nb2[:, m:] == -77).all()) and bool((val2[:, m:] == -1234.5).all())


def test_walk_strided_refuses_a_stride_below_the_slot_count(dev, layout):
    lay, cseg, nb, sm = layout
    rc = _lib.load().fdx_customer_windows_walk_strided(
        lay.iamt.data_ptr(), cseg.data_ptr(), lay.sorder.data_ptr(), lay.goff.data_ptr(), cseg.numel() - 1, lay.n_slots,
        3, lay.starts.data_ptr(), nb.data_ptr(), lay.n_slots - 1, sm.data_ptr(), lay.n_slots, 1, 0)
    assert rc == -1  # FDX_E_INVALID


# ---------------------------------------------------------------------------- 2. the step
@pytest.mark.parametrize("overlap", [True, False])
def test_step_in_place_equals_scratch_path(dev, table, forest, scratch_path, overlap):
    p0, c0, slots0, X0 = scratch_path
    n = len(table["ts"])
    rows = _table(_cap(table), dev)
    p1, c1, slots1 = _run(forest, table, dev, 1, rows, overlap=overlap)
    assert slots1 == slots0
    np.testing.assert_array_equal(_bits(p1), _bits(p0))
    _assert_same_columns(c1, c0, f"overlap={overlap}")
    _assert_padding(rows, slots1, f"overlap={overlap}")
    # the same rows, read through `row`, against the by-row records
    rec = ops.FeatureRecords(n, dev)
    p2, _, _ = _run(forest, table, dev, 1, rec, overlap=overlap)
    np.testing.assert_array_equal(_bits(p2), _bits(p0))
    rc = {k: v.cpu().numpy() for k, v in rec.columns().items()}
    assert (rc["row"] == np.arange(n)).all()
    X1 = table_as_X(rows, slots1, table["amount"])
    assert_same_features(X1, X0, "in place vs scratch arrays")
    for w in range(3):
        for j, k in ((3 + 2 * w, "cust_nb"), (4 + 2 * w, "cust_avg"), (9 + 2 * w, "term_nb"), (10 + 2 * w, "term_risk")):
            np.testing.assert_array_equal(_bits(X1[:, j]), _bits(rc[k][w].astype(np.float64)), err_msg=f"{k}[{w}]")
    np.testing.assert_array_equal(X1[:, 1], rc["weekend"])
    np.testing.assert_array_equal(X1[:, 2], rc["night"])


# ---------------------------------------------------------------------------- 3. padding, reuse
def test_reused_table_padding_and_live_slots(dev, table, forest):
    keep = table["customer"] % 3 != 1  # batch B: a smaller batch with another layout
    small = {k: v[keep] for k, v in table.items()}
    rows = _table(_cap(table), dev)
    _, _, slots_a = _run(forest, table, dev, 1, rows)
    p_b, c_b, slots_b = _run(forest, small, dev, 1, rows)
    assert slots_b < slots_a
    _assert_padding(rows, slots_b, "batch B in the table batch A used")
    fresh = _table(_cap(table), dev, fill=0x5C)
    p_f, c_f, slots_f = _run(forest, small, dev, 1, fresh)
    assert slots_f == slots_b
    np.testing.assert_array_equal(_bits(p_b), _bits(p_f))
    _assert_same_columns(c_b, c_f, "reused vs fresh table")
    ref = _table(_cap(table), dev)
    p_r, c_r, _ = _run(forest, small, dev, 0, ref)
    np.testing.assert_array_equal(_bits(p_b), _bits(p_r))
    _assert_same_columns(c_b, c_r, "reused table vs scratch arrays")


# ---------------------------------------------------------------------------- 4. strides
def test_table_of_exactly_the_slots(dev, table, forest, scratch_path):
    """cap == round_up(n_slots, 64): the last column element written is the buffer's last"""
    p0, c0, slots0, _ = scratch_path
    rows = _table((slots0 + 63) // 64 * 64, dev)
    assert rows.cap - slots0 < 64
    _check_against(forest, table, dev, rows, p0, c0, slots0, "exact")


def test_table_sized_as_the_bench_sizes_it(dev, forest):
    """cap = n * 11 // 10, on the generator's own table (customers of like lengths: the layout pads a
    few percent; the hand-made table's 1,100-row customer pads far more than a tenth)"""
    d = _plain_table()
    cap = len(d["ts"]) * 11 // 10
    p0, c0, slots0 = _run(forest, d, dev, 0, _table(cap, dev))
    assert len(d["ts"]) < slots0 <= cap
    _check_against(forest, d, dev, _table(cap, dev), p0, c0, slots0, "bench")


def _check_against(forest, d, dev, rows, p0, c0, slots0, sizing):
    p1, c1, slots1 = _run(forest, d, dev, 1, rows)
    assert slots1 == slots0
    np.testing.assert_array_equal(_bits(p1), _bits(p0))
    _assert_same_columns(c1, c0, sizing)
    _assert_padding(rows, slots1, sizing)


# ---------------------------------------------------------------------------- 5. NaN amounts
def test_nan_amount_windows(dev, table, forest, scratch_path):
    _, c0, slots0, _ = scratch_path
    rows = _table(_cap(table), dev)
    _, c1, _ = _run(forest, table, dev, 1, rows)
    nan_rows = np.flatnonzero(np.isnan(table["amount"]))
    assert len(nan_rows) == 2 and np.signbit(table["amount"][nan_rows]).sum() == 1
    slot_of = {int(r): s for s, r in enumerate(c0["row"]) if r >= 0}
    for r in nan_rows:
        s = slot_of[int(r)]
        assert c0["cust_nb"][0][s] == 0 and c0["cust_nb"][1][s] == 0 and c0["cust_nb"][2][s] > 0
        for w in range(3):
            assert c1["cust_nb"][w][s] == c0["cust_nb"][w][s]
            assert _bits(c1["cust_avg"][w][s:s + 1])[0] == _bits(c0["cust_avg"][w][s:s + 1])[0]
        assert np.isnan(c1["cust_avg"][0][s]) and np.isnan(c1["cust_avg"][1][s])


# ---------------------------------------------------------------------------- 6. undersized table
@pytest.mark.parametrize("in_place", [1, 0])
def test_undersized_table_is_refused_before_any_write(dev, table, forest, scratch_path, in_place):
    _, _, slots0, _ = scratch_path
    n = len(table["ts"])
    cap = (n + 63) // 64 * 64
    assert n <= cap < slots0, "a capacity that holds the rows but not the layout's slots"
    rows = _table(cap, dev, fill=0x3D)
    pipe = FraudPipeline(forest=forest)
    pipe.table_in_place = in_place
    proba = torch.empty(n, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match=f"the feature table holds {rows.cap} slots < {slots0}"):
        pipe.run_fused(*_args(table, dev), N_CUST, N_TERM, proba, rows_out=rows)
    torch.cuda.synchronize()
    assert bool((rows.buf == 0x3D).all()), "the table was written before its size was checked"


# ---------------------------------------------------------------------------- 7. option combinations
def test_invalid_option_combinations(dev, forest):
    L = _lib.load()
    n = 64
    tbl, rec = ops.FeatureTable(n, dev), ops.FeatureRecords(n, dev)
    z64 = torch.zeros(3 * n, dtype=torch.int64, device=dev)
    ws = ops.workspace(forest.workspace_size(n), dev)
    before = ws.clone()
    IN_TABLE, SUM, COMPACT = _lib.FDX_PREP_CUST_IN_TABLE, 1, 4

    def call(n_windows, opts, out, order):
        p = z64.data_ptr()
        return L.fdx_forest_prepare_grouped(forest._h, n, n_windows, 0, opts, p, p, p, p, p, None, p, out.buf.data_ptr(),
                                            out.cap, order, ws.data_ptr(), ws.numel(), 0)

    assert call(3, IN_TABLE | COMPACT, rec, _lib.FDX_ROWS_INPUT_ORDER) == -1   # by-row records
    assert call(3, IN_TABLE | COMPACT | SUM, tbl, _lib.FDX_ROWS_SLOT_ORDER) == -1  # sums, not averages
    assert call(2, IN_TABLE, tbl, _lib.FDX_ROWS_SLOT_ORDER) == -1              # n_windows != 3
    assert L.fdx_forest_prepare_grouped(forest._h, n, 3, 0, IN_TABLE, z64.data_ptr(), z64.data_ptr(), None, None, None,
                                        None, z64.data_ptr(), None, 0, 0, ws.data_ptr(), ws.numel(), 0) == -1  # no table
    assert L.fdx_forest_prepare_in_table_ok(forest._h, 2, tbl.cap) == 0
    assert L.fdx_forest_prepare_in_table_ok(forest._h, 3, tbl.cap) == 1
    assert L.fdx_forest_prepare_in_table_ok(forest._h, 3, 2**31 // 78 // 64 * 64 + 64) == 0  # past 2^31 bytes
    torch.cuda.synchronize()
    assert torch.equal(ws, before), "a refused call enqueued nothing"
