"""An exact reference for the ranking metrics of include/fdx.h (fdx_ranking_metrics) and the
named inputs its tests share.

exact(): numpy stable sort, then Python integers for auc_num, fractions.Fraction for AP and
Python's correctly rounded int / int for auc -- no floating-point sum anywhere.  The named inputs
are the smallest that can break a kernel (the sort tile and the scan block hold 4,096 rows); each
comes from np.random.default_rng with a fixed seed and is read-only.
"""
import functools
from fractions import Fraction

import numpy as np

TILE = 4096


def exact(score, label):
    """-> dict: n_pos, n_neg, n_groups, auc_num (int), auc (float, NaN without both classes),
    ap (Fraction, 0 without positives), thr / tps / fps (the curve, thresholds decreasing)."""
    s = np.asarray(score, dtype=np.float64)
    y = (np.asarray(label) != 0).astype(np.int64)
    if len(s) == 0:
        e = np.zeros(0, np.int64)
        return dict(n_pos=0, n_neg=0, n_groups=0, auc_num=0, auc=float("nan"), ap=Fraction(0),
                    thr=np.zeros(0), tps=e, fps=e)
    o = np.argsort(-s, kind="stable")
    s, y = s[o], y[o]
    end = np.r_[np.nonzero(s[1:] != s[:-1])[0], len(s) - 1]  # last row of each group (== : +-0 merge)
    tp = np.cumsum(y)[end]
    k = end + 1
    fp = k - tp
    P, N = int(tp[-1]), int(fp[-1])
    tp0, fp0 = np.r_[0, tp[:-1]], np.r_[0, fp[:-1]]
    num = sum(int(a) * int(b) for a, b in zip(fp - fp0, tp + tp0))
    auc = num / (2 * P * N) if P and N else float("nan")
    ap = sum((Fraction(int(d) * int(t), int(kk)) for d, t, kk in zip(tp - tp0, tp, k) if d), Fraction(0))
    ap = ap / P if P else Fraction(0)
    return dict(n_pos=P, n_neg=N, n_groups=len(end), auc_num=num, auc=auc, ap=ap, thr=s[end], tps=tp, fps=fp)


@functools.lru_cache(maxsize=None)
def named_inputs():
    """name -> (score float64, label uint8), read-only."""
    c = {}
    rng = np.random.default_rng(0)  # one generator, in this draw order
    n = TILE + 3
    c["cont"] = (rng.random(n), (rng.random(n) < 0.02).astype(np.uint8))
    p = np.round(rng.beta(0.3, 3, n) * 100) / 100
    c["ties100"] = (p, (rng.random(n) < p * 0.5 + 0.005).astype(np.uint8))
    c["alltie"] = (np.full(n, 0.25), (rng.random(n) < 0.3).astype(np.uint8))
    s = rng.random(n)
    y = (s > 0.9).astype(np.uint8)
    c["perfect"] = (s, y)
    c["inverted"] = (-s, y)
    s = np.r_[rng.normal(size=n - 6), [0.0, -0.0, 5e-324, -5e-324, 1e308, -1e308]]
    c["signs"] = (s, (rng.random(n) < 0.4).astype(np.uint8))
    n2 = 300001
    p = np.round(rng.beta(0.3, 3, n2) * 1000) / 1000
    c["big"] = (p, (rng.random(n2) < p * 0.5 + 0.002).astype(np.uint8))
    # the rest: a generator each
    rng = np.random.default_rng(3)
    c["alltie3"] = (np.full(3 * TILE, 0.25), (rng.random(3 * TILE) < 0.3).astype(np.uint8))
    rng = np.random.default_rng(4)
    o = rng.permutation(140000)
    c["block"] = (np.r_[np.ones(70000), np.zeros(70000)][o], np.r_[np.ones(70000), np.zeros(70000)].astype(np.uint8)[o])
    for m in (1, 2, TILE - 1, TILE, TILE + 1):
        rng = np.random.default_rng(100 + m)
        p = np.round(rng.beta(0.3, 3, m) * 100) / 100
        c[f"n{m}"] = (p, (rng.random(m) < p * 0.5 + 0.005).astype(np.uint8))
    rng = np.random.default_rng(5)
    p = np.round(rng.beta(0.3, 3, n) * 100) / 100
    c["no_pos"] = (p, np.zeros(n, np.uint8))
    c["no_neg"] = (p, np.ones(n, np.uint8))
    c["empty"] = (np.zeros(0), np.zeros(0, np.uint8))
    for s, y in c.values():
        s.setflags(write=False)
        y.setflags(write=False)
    return c


NAMES = ["cont", "ties100", "alltie", "alltie3", "perfect", "inverted", "signs", "block", "big", "n1", "n2",
         f"n{TILE - 1}", f"n{TILE}", f"n{TILE + 1}", "no_pos", "no_neg", "empty"]


@functools.lru_cache(maxsize=None)
def exact_of(name):
    return exact(*named_inputs()[name])


def both_classes(name):
    e = exact_of(name)
    return e["n_pos"] > 0 and e["n_neg"] > 0


@functools.lru_cache(maxsize=None)
def sklearn_of(name):
    """(roc_auc_score, average_precision_score) of a named input with both classes."""
    from sklearn.metrics import average_precision_score, roc_auc_score

    s, y = named_inputs()[name]
    return float(roc_auc_score(y, s)), float(average_precision_score(y, s))
