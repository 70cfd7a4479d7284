"""tools/record_reuse_sim.py at a reduced size (no GPU): visiting the slot granules in time order
brings the uses of a record line closer together than the linear slot sweep does."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_time_order_shortens_the_reuse_distance():
    import record_reuse_sim as sim

    res, n_slots, n = sim.table(400, 800, 183, seed=1234, granules=(64, 1024), per_lines=(8, 16))
    assert n_slots >= n > 100_000
    i5 = sim.SHARES.index(0.05)
    for per_line in (8, 16):
        lin = res[(per_line, "linear", None)][i5]
        for G in (64, 1024):
            assert res[(per_line, "by tile time", G)][i5] > lin, (per_line, G)
        assert res[(per_line, "by tile time", 64)][i5] <= 1 - 1 / per_line


def test_layout_holds_every_row_once():
    import record_reuse_sim as sim

    cust = np.random.default_rng(0).integers(0, 50, 3000).astype(np.int32)
    irow = sim.layout(cust, 50)
    live = irow[irow >= 0]
    np.testing.assert_array_equal(np.sort(live), np.arange(3000))
    # slot (t, l) of a group holds customer l's t-th row: every lane's rows are in time order
    assert (np.diff(irow[: sim.S * 10].reshape(10, sim.S), axis=0) > 0).all()
