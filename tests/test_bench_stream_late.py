"""bench_stream.hold_back (--late-terminals, no GPU): the held customers' rows arrive one batch
late, every customer's rows stay in time order, no row is lost or doubled."""
import numpy as np

import bench_stream


def test_hold_back_keeps_customers_in_order_and_terminals_not():
    rng = np.random.default_rng(2)
    n, h = 5000, 1000
    cols = {"ts": np.sort(rng.integers(0, 10 ** 6, n)).astype(np.int64), "customer": rng.integers(0, 50, n).astype(np.int32),
            "terminal": rng.integers(0, 20, n).astype(np.int32)}
    before = {k: v.copy() for k, v in cols.items()}
    bounds = np.r_[np.arange(h, n, 500), n]
    new, held = bench_stream.hold_back(cols, h, bounds, 0.3)
    assert new[0] == h and new[-1] == n and len(new) == len(bounds) + 1 and np.all(np.diff(new) > 0)
    assert 0.1 * (n - h) < held < 0.5 * (n - h)
    for k in cols:                                           # the history is untouched, the day is a permutation
        np.testing.assert_array_equal(cols[k][:h], before[k][:h])
    key = lambda c: np.lexsort((c["terminal"][h:], c["customer"][h:], c["ts"][h:]))  # noqa: E731
    for k in cols:
        np.testing.assert_array_equal(cols[k][h:][key(cols)], before[k][h:][key(before)])
    for c in range(50):                                      # every customer in time order ...
        assert np.all(np.diff(cols["ts"][h:][cols["customer"][h:] == c]) >= 0)
    back = sum(np.any(np.diff(cols["ts"][h:][cols["terminal"][h:] == t]) < 0) for t in range(20))
    assert back == 20                                        # ... and every terminal not
    # a row moves by at most one batch: batch k's rows come from time slices k - 1 and k
    for j, (a, b) in enumerate(zip(new[:-1], new[1:])):
        lo = before["ts"][bounds[max(j - 1, 0)]]
        hi = before["ts"][bounds[min(j + 1, len(bounds) - 1)] - 1]
        assert lo <= cols["ts"][a:b].min() and cols["ts"][a:b].max() <= hi
