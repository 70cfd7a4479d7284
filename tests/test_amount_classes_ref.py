"""The C oracle against pandas itself on the amount classes of amount_classes.py, and proof that the
generated inputs are what they claim (asserted on the oracle's output), so that the GPU tests
that compare the kernels with the oracle on these inputs cannot pass vacuously.  No GPU.

Compared bit for bit with NaNs canonicalised and signed zeros distinct (amount_classes.same_bits).
The infinity class is the one where pandas and IEEE arithmetic part: pandas' rolling sum() turns
+-inf into NaN before its roll_sum loop while count() still counts it, so AVG = SUM / NB is the
finite sum over a count that includes the infinities."""
import numpy as np
import pytest

import oracle
from amount_classes import (DENORM_MIN, KINDS, PATTERNS, escape_segment, pandas_customer_windows, same_bits,
                            segments)

WINDOWS = (1, 7, 30)


@pytest.fixture(scope="module")
def oracle_out():
    """(kind, pattern, nan) -> (ts, amt, seg, nb, avg), computed once"""
    cache = {}

    def get(kind, pattern, nan):
        key = (kind, pattern, nan)
        if key not in cache:
            ts, amt, seg = segments(kind, pattern, nan)
            cache[key] = (ts, amt, seg) + tuple(oracle.customer_windows(ts, amt, seg, WINDOWS))
        return cache[key]

    return get


@pytest.mark.parametrize("nan", [False, True], ids=["", "nan"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", KINDS)
def test_oracle_equals_pandas(oracle_out, kind, pattern, nan):
    ts, amt, seg, nb, avg = oracle_out(kind, pattern, nan)
    with np.errstate(all="ignore"):
        pnb, pavg = pandas_customer_windows(ts, amt, seg, WINDOWS)
    same_bits(nb, pnb, f"{kind} {pattern} counts")
    same_bits(avg, pavg, f"{kind} {pattern} averages")


def test_oracle_equals_pandas_other_windows(oracle_out):
    for kind in ("signed", "huge", "inf"):
        ts, amt, seg = segments(kind, "sparse", True)
        nb, avg = oracle.customer_windows(ts, amt, seg, (2, 5))
        with np.errstate(all="ignore"):
            pnb, pavg = pandas_customer_windows(ts, amt, seg, (2, 5))
        same_bits(nb, pnb, kind)
        same_bits(avg, pavg, kind)


def _all(oracle_out, kind, nan=False):
    """the class's averages over both time patterns"""
    return np.concatenate([oracle_out(kind, p, nan)[4].ravel() for p in PATTERNS])


@pytest.mark.parametrize("nan", [False, True], ids=["", "nan"])
def test_signed_has_negative_zero_averages(oracle_out, nan):
    avg = _all(oracle_out, "signed", nan)
    neg_zero = (avg == 0.0) & np.signbit(avg)
    assert neg_zero.mean() >= 0.01, neg_zero.mean()
    for p in PATTERNS:  # and each pattern on its own has some, of either sign
        a = oracle_out("signed", p, nan)[4]
        assert ((a == 0.0) & np.signbit(a)).any() and ((a == 0.0) & ~np.signbit(a)).any()
        assert (a < 0).any() and (a > 0).any()


@pytest.mark.parametrize("nan", [False, True], ids=["", "nan"])
def test_huge_overflows_from_finite_inputs(oracle_out, nan):
    for p in PATTERNS:
        amt = oracle_out("huge", p, nan)[1]
        assert np.isfinite(amt[~np.isnan(amt)]).all() and np.isnan(amt).any() == nan
    avg = _all(oracle_out, "huge", nan)
    assert np.isnan(avg).mean() >= 0.05, np.isnan(avg).mean()
    assert np.isinf(avg).sum() >= 10, np.isinf(avg).sum()


def test_escape_segment_counts(oracle_out):
    ts, amt = escape_segment()
    assert len(ts) == 55
    nb, avg = oracle.customer_windows(ts, amt, np.array([0, 55], np.int64), WINDOWS)
    # (exactly 5.0, NaN, inf); the other two rows of each window are 7.0 and (7 + 1e308) / 2
    want = {0: (44, 8, 1), 1: (13, 39, 1), 2: (0, 52, 1)}
    for w, (n5, n_nan, n_inf) in want.items():
        assert ((avg[w] == 5.0).sum(), np.isnan(avg[w]).sum(), np.isinf(avg[w]).sum()) == (n5, n_nan, n_inf), w
    # it is the last segment of every class and pattern
    for kind in KINDS:
        _, a, seg, _, av = oracle_out(kind, "dense", False)
        same_bits(a[seg[-2]:], amt)
        same_bits(av[:, seg[-2]:], avg)


def test_tiny_has_denormal_averages(oracle_out):
    for p in PATTERNS:
        _, amt, _, _, avg = oracle_out("tiny", p, False)
        assert (np.abs(amt[: -55]) < 2.3e-308).all() and (amt[: -55] != 0).all()
        den = (avg != 0) & (np.abs(avg) < 2.2250738585072014e-308)
        assert den.any() and (avg[den] < 0).any() and (avg[den] > 0).any()
        assert (np.abs(avg[den]) >= DENORM_MIN).all()


@pytest.mark.parametrize("nan", [False, True], ids=["", "nan"])
def test_inf_windows_have_finite_pandas_averages(oracle_out, nan):
    """>= 1 % of the cells: the window holds an infinity and pandas' average is finite."""
    hit = total = 0
    for p in PATTERNS:
        ts, amt, seg, nb, avg = oracle_out("inf", p, nan)
        # rolling count of the infinities alone, through the same oracle (an exact integer)
        ninf, _ = oracle.customer_windows(ts, np.where(np.isinf(amt), 1.0, np.nan), seg, WINDOWS)
        hit += int(((ninf > 0) & np.isfinite(avg)).sum())
        total += avg.size
    assert hit >= 0.01 * total, (hit, total)


def test_dense_windows_outgrow_the_walk_rings(oracle_out):
    for kind in KINDS:
        nb = oracle_out(kind, "dense", False)[3]
        assert nb[2].max() > 256, kind
