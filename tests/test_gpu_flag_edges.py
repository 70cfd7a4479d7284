"""The weekend / night flags at the edges of the device code that computes them (day_flags in
fdx_internal.h, and k_time_flags' own 64-bit form): day and hour boundaries on both sides of 1970
and the boundary between day_flags' int32-seconds arithmetic (1901-2038) and its 64-bit fallback,
through every entry point that computes flags, in both flag modes, equal to the oracle on every row."""
import os

import numpy as np
import pytest
import torch

import oracle
from fdx import _lib, ops
from fdx.pipeline import FraudPipeline
from fdx.streaming import StreamState

pytestmark = pytest.mark.gpu

SEC = 10**9
DAY, H, B = 86400 * SEC, 3600 * SEC, 2**31
MODES = {_lib.FDX_FLAGS_NOTEBOOK: (oracle.weekend_flag, oracle.night_flag),
         _lib.FDX_FLAGS_SPARK: (oracle.spark_weekend_flag, oracle.spark_night_flag)}


def _timestamps():
    s = {0, -1, DAY - 1, DAY, -DAY, -DAY - 1}
    for base in (19000, -26000, 25000):
        for k in range(7):
            d = (base + k) * DAY
            s |= {d, d + 7 * H - 1, d + 7 * H, d + 20 * H - 1, d + 20 * H}
    s |= {(B - 1) * SEC, (B - 1) * SEC + SEC - 1, B * SEC, B * SEC + 1, -B * SEC, -B * SEC - 1, -B * SEC + 1,
          (-B - 1) * SEC}
    return np.array(sorted(s), dtype=np.int64)


TS = _timestamps()
REF = {m: (we(TS).astype(np.uint8), ni(TS).astype(np.uint8)) for m, (we, ni) in MODES.items()}


def T(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def test_inputs_reach_both_regimes():
    """an edited list cannot quietly lose a regime, a flag value or the overflow margin"""
    assert len(TS) == 119 and len(TS) % 8 == 7  # 14 eight-row groups and a 7-row tail in k_time_flags
    sec = np.array([int(t) // SEC for t in TS])  # Python's floor division
    fits = (sec >= -B) & (sec <= B - 1)
    assert fits.sum() == 45 and (~fits).sum() == 74
    for m in MODES:
        for flags in REF[m]:
            for sel in (fits, ~fits):
                assert set(flags[sel]) == {0, 1}
    assert max(abs(int(t)) for t in TS) < 2.3e18  # t - (delay + longest window = 37 days) cannot overflow


@pytest.mark.parametrize("mode", list(MODES))
def test_time_flags(dev, mode):
    we, ni = ops.time_flags(T(TS, torch.int64, dev), mode)
    np.testing.assert_array_equal(we.cpu().numpy(), REF[mode][0])
    np.testing.assert_array_equal(ni.cpu().numpy(), REF[mode][1])


@pytest.mark.parametrize("mode", list(MODES))
def test_stream_update(dev, mode):
    """the customer half alone, one customer per row: X[:, 1:3] are the flags"""
    n = len(TS)
    st = StreamState(n, 1, flags_mode=mode, max_batch=128)
    X = st.update(T(TS, torch.int64, dev), customer=T(np.arange(n), torch.int32, dev),
                  amount=T(np.ones(n), torch.float64, dev))
    st.check()
    X = X.cpu().numpy()
    np.testing.assert_array_equal(X[:, 1], REF[mode][0].astype(np.float64))
    np.testing.assert_array_equal(X[:, 2], REF[mode][1].astype(np.float64))


@pytest.fixture(scope="module", params=["bench", "no_search_trees"])
def forest(request):
    """the bench model (k_zfill_grouped_w3 builds its rows), and test_gpu_config1's forest with too
    many thresholds for that kernel's S-trees (k_zfill_grouped + k_feature_rows)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    z = np.load(os.path.join(root, "bench_assets", "rf100_d20.npz"))
    if request.param == "bench":
        arrays = {k: z[k].astype(np.int64) if k in ("left", "right", "feature") else z[k]
                  for k in ("node_offsets", "left", "right", "feature", "threshold", "missing_left", "value1")}
    else:
        from test_gpu_config1 import _many_threshold_forest

        arrays = _many_threshold_forest()
    return ops.Forest(arrays, 15, z["mean"], z["scale"])


@pytest.mark.parametrize("kind", ["table", "records"])
@pytest.mark.parametrize("mode", list(MODES))
def test_run_fused_rows(dev, forest, mode, kind):
    """the row assembly's flags, by input row; a table's padding slots hold zeros"""
    n = len(TS)
    key = T(np.arange(n) % 2, torch.int32, dev)
    pipe = FraudPipeline(flags_mode=mode, forest=forest)
    rows = ops.FeatureTable(64 * n, dev) if kind == "table" else ops.FeatureRecords(n, dev)
    rows.buf.fill_(0xAB)
    p = torch.empty(n, dtype=torch.float64, device=dev)
    pipe.run_fused(T(TS, torch.int64, dev), key, key, T(np.ones(n), torch.float64, dev),
                   torch.zeros(n, dtype=torch.uint8, device=dev), 2, 2, p, rows_out=rows)
    torch.cuda.synchronize()
    if kind == "table":
        col = {k: v.cpu().numpy() for k, v in rows.columns(pipe.last_slots).items()}
        real = col["row"] >= 0
        assert real.sum() == n and (~real).any()
        assert not col["weekend"][~real].any() and not col["night"][~real].any()
        o = np.argsort(col["row"][real], kind="stable")
        col = {k: col[k][real][o] for k in ("row", "weekend", "night")}
    else:
        col = {k: v.cpu().numpy() for k, v in rows.columns().items()}
    np.testing.assert_array_equal(col["row"], np.arange(n, dtype=np.int32))
    np.testing.assert_array_equal(col["weekend"], REF[mode][0])
    np.testing.assert_array_equal(col["night"], REF[mode][1])
