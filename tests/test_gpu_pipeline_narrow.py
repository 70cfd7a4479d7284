"""run_fused with the narrow payload forms off, on for the timestamps (FraudPipeline.narrow_payloads,
the default) and on for the amounts too (narrow_amounts): proba and the featurized table must be
bit-equal by input row, and equal to the C oracle -- on exact data (both re-keys go narrow), with
one inexact amount (the customer re-key falls back when it tried the amounts, the terminal one
stays narrow) and with one sub-second timestamp (both fall back).  The table has a terminal
past the 1,024-row stage and one between the short pass's 256 rows and the stage, so the
terminal windows' long kernel runs in both of its memory spaces."""
import numpy as np
import pytest
import torch

import oracle
from fdx import ops, synth
from fdx.pipeline import FraudPipeline
from table_check import assert_same_features, table_as_X

pytestmark = pytest.mark.gpu
N_CUST, N_TERM = 300, 500


def T(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


@pytest.fixture(scope="module")
def table():
    d = synth.generate(N_CUST, N_TERM, 40, seed=3)
    n = len(d["ts"])
    assert 15_000 < n < 30_000
    rng = np.random.default_rng(4)
    term = d["terminal"].copy()
    hot = rng.choice(n, 1_900, replace=False)
    term[hot[:1_500]] = 7    # > 1,024 rows: the long kernel's global-memory searches
    term[hot[1_500:]] = 11   # 256 < rows <= 1,024: the long kernel's LDS stage
    # (the generator's scenario-3 frauds are a cents amount x 5 in float64, not cents: rounded here, so
    # that the exact case is exact)
    return dict(ts=d["ts"], customer=d["customer"], terminal=term, amount=np.rint(d["amount"] * 100.0) / 100.0,
                fraud=d["fraud"])


@pytest.fixture(scope="module")
def forest(golden):
    z = golden("forest_rf5d8.npz")
    arrays = {k: z[k] for k in ("left", "right", "feature", "threshold", "missing_left", "value1", "node_offsets")}
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


def _fused(forest, d, dev, narrow):
    n = len(d["ts"])
    args = (T(d["ts"], torch.int64, dev), T(d["customer"], torch.int32, dev), T(d["terminal"], torch.int32, dev),
            T(d["amount"], torch.float64, dev), T(d["fraud"], torch.uint8, dev))
    pipe = FraudPipeline(forest=forest)
    pipe.narrow_payloads, pipe.narrow_amounts = narrow
    proba = torch.empty(n, dtype=torch.float64, device=dev)
    rows = ops.FeatureTable(2 * n + 4096, dev)
    rows.buf.fill_(0xAB)
    pipe.run_fused(*args, N_CUST, N_TERM, proba, rows_out=rows)
    torch.cuda.synchronize()
    flags = [None if f is None else not f.holds() for f in pipe.narrow_flags]
    return proba.cpu().numpy(), table_as_X(rows, pipe.last_slots, d["amount"]), flags


def _inject(table, what):
    d = {k: v.copy() for k, v in table.items()}
    n = len(d["ts"])
    if what == "inexact_amount":
        d["amount"][n // 3] = 0.1 + 0.2
    elif what == "subsecond_ts":
        k = n - 5  # (+ 1 ns keeps the time order: every later row is at least as late)
        d["ts"][k:] += 1
    return d


# case -> [customer re-key fell back, terminal re-key fell back], timestamps alone / amounts too
@pytest.mark.parametrize("what,fallback_ts,fallback_amt",
                         [("exact", [False, False], [False, False]),
                          ("inexact_amount", [False, False], [True, False]),
                          ("subsecond_ts", [True, True], [True, True])])
def test_fused_narrow_equals_wide_and_oracle(dev, table, forest, what, fallback_ts, fallback_amt):
    d = _inject(table, what)
    p_w, X_w, f_w = _fused(forest, d, dev, (0, 0))
    p_n, X_n, f_n = _fused(forest, d, dev, (1, 0))
    p_a, X_a, f_a = _fused(forest, d, dev, (1, 1))
    assert f_w == [None, None]
    assert f_n == fallback_ts and f_a == fallback_amt  # the branch each re-key actually took
    np.testing.assert_array_equal(p_n.view(np.int64), p_w.view(np.int64))
    np.testing.assert_array_equal(p_a.view(np.int64), p_w.view(np.int64))
    assert_same_features(X_n, X_w, f"{what}: narrow ts vs wide")
    assert_same_features(X_a, X_w, f"{what}: narrow ts + amount vs wide")
    ref = oracle.featurize_arrays(d["ts"], d["customer"], d["terminal"], d["amount"], d["fraud"])
    for X, side in ((X_n, "narrow ts"), (X_a, "narrow ts + amount"), (X_w, "wide")):
        np.testing.assert_array_equal(X[:, 1], ref["TX_DURING_WEEKEND"], err_msg=side)
        np.testing.assert_array_equal(X[:, 2], ref["TX_DURING_NIGHT"], err_msg=side)
        for j, c in enumerate(oracle.CUSTOMER_COLS):
            np.testing.assert_array_equal(X[:, 3 + j], ref[c], err_msg=f"{side} {c}")
        for j, c in enumerate(oracle.TERMINAL_COLS):
            np.testing.assert_array_equal(X[:, 9 + j], ref[c], err_msg=f"{side} {c}")
