"""The row assembly's two forms of slot arithmetic (k_zfill_grouped_w3: the 32-bit scalar loop every
batch below 2^31 slots takes, and the 64-bit one, FDX_PREP_INDEX64) write the same rank rows, NaN
flag and featurized table, bit for bit."""
import os

import numpy as np
import pytest
import torch

from fdx import _lib, ops, synth
from fdx.pipeline import FraudPipeline

pytestmark = pytest.mark.gpu

DAY = 86_400 * 10**9


def T(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


@pytest.fixture(scope="module")
def forest():
    """the bench model: its four continuous features are ranked by S-trees, the kernel the step runs"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z = np.load(os.path.join(root, "bench_assets", "rf100_d20.npz"))
    arrays = {k: z[k].astype(np.int64) if k in ("left", "right", "feature") else z[k]
              for k in ("node_offsets", "left", "right", "feature", "threshold", "missing_left", "value1")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def _stage(dev, ts, cust, term, amt, fraud, n_cust, n_term):
    """run_fused's stages up to the assembly's inputs, on one stream"""
    a = (T(ts, torch.int64, dev), T(cust, torch.int32, dev), T(term, torch.int32, dev), T(amt, torch.float64, dev),
         T(fraud, torch.uint8, dev))
    cperm, cseg, gts, gamt = ops.rekey_payload(a[1], n_cust, a[0], a[3])
    lay = ops.customer_layout_fill(ops.customer_layout_plan(cseg, 3), cseg, cperm, gts, gamt, (1, 7, 30))
    inb, isum = ops.customer_windows_walk(lay, cseg)
    tperm, tseg, tgts, _ = ops.rekey_payload(a[2], n_term, a[0], flag=a[4])
    trec = ops.terminal_windows_compact(tgts, tseg, rows=tperm)
    return dict(lay=lay, inb=inb, isum=isum, trec=trec, n=len(ts), args=a)


def _assemble(forest, st, dev, rows_kind, index64):
    """the workspace (rank rows + NaN flag) and the featurized table's bytes after one assembly"""
    lay = st["lay"]
    ws = torch.zeros(forest.workspace_size(lay.n_slots), dtype=torch.uint8, device=dev)
    rows = None
    if rows_kind == "table":
        rows = ops.FeatureTable(lay.n_slots, dev)
    elif rows_kind == "records":
        rows = ops.FeatureRecords(st["n"], dev)
    if rows is not None:
        rows.buf.zero_()
    ops.forest_prepare_grouped(forest, _lib.FDX_FLAGS_NOTEBOOK, lay.its, lay.iamt, st["inb"], st["isum"], lay.irow, None,
                               st["trec"], ws, n=lay.n_slots, val_is_sum=True, term_compact=True, rows_out=rows,
                               index64=index64)
    torch.cuda.synchronize()
    return ws, (rows.buf if rows is not None else None)


def _case(name):
    if name == "hot_terminal":  # one terminal with > 2^21 rows in a window: the compact record's overflow branch
        n_hot, n_late = 2_200_000, 300
        rng = np.random.default_rng(44)
        ts = np.concatenate([np.sort(rng.integers(0, DAY // 2, n_hot)),
                             7 * DAY + 6 * DAY // 10 + np.arange(n_late) * 10**9]).astype(np.int64)
        term = np.zeros(len(ts), np.int32)
        term[rng.random(len(ts)) < 0.001] = 1
        return (ts, rng.integers(0, 100, len(ts)).astype(np.int32), term, np.round(rng.uniform(1, 300, len(ts)), 2),
                (rng.random(len(ts)) < 0.01).astype(np.uint8), 100, 2)
    # small: a few 1,024-slot tiles and a ragged last one; large: more tiles than the grid has blocks
    n_c, n_t, days = {"small": (40, 60, 40), "large": (1700, 3000, 90), "nan": (300, 400, 40)}[name]
    d = synth.generate(n_customers=n_c, n_terminals=n_t, nb_days=days, seed=23)
    amt = d["amount"].copy()
    if name == "nan":
        amt[np.random.default_rng(1).choice(len(amt), 25, replace=False)] = np.nan
    return d["ts"], d["customer"], d["terminal"], amt, d["fraud"], n_c, n_t


@pytest.mark.parametrize("case", ["small", "large", "nan", "hot_terminal"])
def test_assembly_index_forms_agree(dev, forest, case):
    data = _case(case)
    st = _stage(dev, *data)
    lay = st["lay"]
    if case == "small":
        assert 1024 < lay.n_slots < 8 * 1024 and lay.n_slots % 1024 != 0, lay.n_slots
    if case == "large":
        assert lay.n_slots > 262_144 + 1024, lay.n_slots
    if case == "hot_terminal":
        assert bool((st["trec"][: 2 * st["n"]].view(-1, 2)[:, 0] < 0).any())  # escaped records exist
    for kind in ("none", "table", "records"):
        ws0, buf0 = _assemble(forest, st, dev, kind, True)
        ws1, buf1 = _assemble(forest, st, dev, kind, False)
        assert bool(ws0.any())
        assert torch.equal(ws1, ws0), kind
        if buf0 is not None:
            assert bool(buf0.any()) and torch.equal(buf1, buf0), kind
    if case == "nan":  # the NaN flag is set and the traversal takes missing_go_to_left, as the float64 path
        p0 = torch.empty(st["n"], dtype=torch.float64, device=dev)
        ws1, _ = _assemble(forest, st, dev, "none", False)
        ops.forest_traverse_perm(forest, lay.n_slots, ws1, p0, lay.irow)
        _, p_ref = FraudPipeline(forest=forest).run(*st["args"], *data[5:])
        assert torch.equal(p0, p_ref)


def test_run_fused_index_forms_agree(dev, forest):
    """run_fused with assembly_index64 0 and 1: the same proba and featurized table."""
    g = synth.generate_device(3000, 6000, 60, seed=9, device=dev)
    n = g["ts"].numel()
    out = []
    for i64 in (0, 1):
        pipe = FraudPipeline(forest=forest)
        pipe.assembly_index64 = i64
        p = torch.full((n,), -1.0, dtype=torch.float64, device=dev)
        rows = ops.FeatureTable(n * 11 // 10, dev)
        pipe.run_fused(g["ts"], g["customer"], g["terminal"], g["amount"], g["fraud"], 3000, 6000, p, rows_out=rows)
        torch.cuda.synchronize()
        out.append((p, {k: v.clone() for k, v in rows.columns(pipe.last_slots).items()}))
    assert torch.equal(out[0][0], out[1][0]) and bool((out[0][0] >= 0).all())
    assert out[0][1].keys() == out[1][1].keys()
    for k in out[0][1]:
        assert torch.equal(out[0][1][k].view(torch.uint8), out[1][1][k].view(torch.uint8)), k
