"""Amount classes beyond positive cents, for the customer-window tests (no GPU needed).

Every other window test feeds positive amounts rounded to cents.  The pandas roll_sum recurrence
(Kahan add, Kahan remove, re-initialisation, "n equal values give prev * n") behaves differently
on the classes below: a sum that cancels to a signed zero, a sum that overflows and poisons the
window with NaN until only equal values are left in it, denormals, infinities (which pandas'
rolling sum leaves out while its rolling count keeps them).

  amounts(kind, L, rng)        one segment's amounts of a class
  with_nan(a, rng)             the 5 % NaN overlay
  escape_segment()             55 rows whose windows are poisoned by overflow and come back
  times(pattern, L, rng)       "sparse" / "dense" timestamps of one segment
  segments(kind, pattern, ..)  all segment lengths + the escape segment, grouped
  table(kind, ...)             the same segments as a time-sorted transaction table
  same_bits(got, want)         bit comparison, NaNs canonical, signed zeros distinct
  pandas_customer_windows(..)  the reference's own three lines per segment
"""
import numpy as np

DAY = 86_400 * 10**9
HOUR = 3_600 * 10**9
NS = 10**9

KINDS = ("cents", "signed", "wide", "huge", "tiny", "inf")
FINITE_KINDS = ("cents", "signed", "wide", "huge", "tiny")
PATTERNS = ("sparse", "dense")
# both sides of the walk's 16-row chunks, its 128- and 256-row rings and its 480-row length class
LENGTHS = [0, 1, 2, 15, 16, 17, 127, 128, 129, 255, 256, 257, 300, 479, 480, 481, 700, 1500]
N_TERMINALS = 50
DENORM_MIN = 5e-324


def _cents(L, rng):
    return np.round(rng.gamma(2.0, 40.0, size=L), 2)


def amounts(kind, L, rng):
    """float64 [L] of one class."""
    if kind == "cents":
        return _cents(L, rng)
    if kind == "signed":  # signed cents, 15 % 0.0 and 10 % -0.0
        a = np.round(rng.normal(0.0, 80.0, size=L), 2)
        u = rng.random(L)
        a[u < 0.15] = 0.0
        a[(u >= 0.15) & (u < 0.25)] = -0.0
        return a
    if kind == "wide":  # 27 decades, either sign: sums that cancel and absorb
        return rng.choice([-1.0, 1.0], size=L) * 10.0 ** rng.uniform(-12.0, 15.0, size=L)
    if kind == "huge":  # finite values whose sums overflow; runs of equal values the windows can come back on
        a = _cents(L, rng)
        for p in range(int(rng.integers(0, 12)), L, 45):
            a[p:p + 12] = a[p]
        u = rng.random(L)
        big = rng.choice([1e308, -1e308, 1.7e308], size=L)
        return np.where(u < 0.08, big, a)
    if kind == "tiny":  # denormals of either sign
        return rng.choice([-1.0, 1.0], size=L) * (rng.integers(1, 1 << 40, size=L).astype(np.float64) * DENORM_MIN)
    if kind == "inf":
        a = _cents(L, rng)
        u = rng.random(L)
        a[u < 0.03] = np.inf
        a[(u >= 0.03) & (u < 0.06)] = -np.inf
        return a
    raise ValueError(kind)


def with_nan(a, rng, p=0.05):
    """5 % NaN, half of them with the sign bit set (what x86 gives for inf - inf)."""
    a = a.copy()
    u = rng.random(len(a))
    a[u < p] = np.nan
    a[u < p / 2] = np.copysign(np.nan, -1.0)
    return a


def escape_segment(t0=45 * DAY):
    """(ts, amount) of 55 rows, one every 6 hours.  Rows 1-3 overflow the sum: inf, then inf - inf =
    NaN, which stays in the Kahan words until the window re-initialises -- or holds equal values
    only, when pandas returns prev * n whatever the sum holds.  1-day windows (4 rows) come back
    at row 7, 7-day windows (28 rows) between row 31 and the 6.0 of row 44, 30-day windows never."""
    amt = np.array([7.0, 1e308, 1e308, -1e308] + [5.0] * 40 + [6.0] + [5.0] * 10)
    ts = t0 + np.arange(len(amt), dtype=np.int64) * (6 * HOUR)
    return ts, amt


ESCAPE_POISONED_ROW = 5   # 1-day and 7-day windows both poisoned, the run of 5.0 under way
ESCAPE_RUN_ROW = 20       # inside the run of 5.0: the 1-day window is back, the 7-day one not yet


def times(pattern, L, rng):
    """int64 ns [L], non-decreasing."""
    if pattern == "sparse":  # ties, gaps of exactly 1, 7 and 30 days, gaps longer than every window
        t0 = int(rng.integers(0, 400)) * DAY
        steps = rng.choice([0, 1, HOUR, DAY, 7 * DAY, 8 * DAY, 14 * DAY, 30 * DAY, 37 * DAY,
                            int(rng.integers(1, 3 * DAY))], size=L,
                           p=[.1, .02, .1, .1, .05, .03, .03, .03, .04, .5])
        return (t0 + np.cumsum(steps)).astype(np.int64)
    if pattern == "dense":  # every row inside 20 days: a 30-day window holds the whole segment
        return np.sort(rng.integers(40 * 86_400, 60 * 86_400, size=L)).astype(np.int64) * NS
    raise ValueError(pattern)


def segments(kind, pattern, nan=False, seed=0, reps=1, escape=True):
    """-> (ts int64 [n], amount float64 [n], seg_off int64 [n_seg + 1]): reps segments per entry of
    LENGTHS, then the escape segment (always its own amounts).  reps = 4 gives the interleaved
    layout (21 segments a group at 3 windows) a group of the walk's long class (>= 480 rows) and
    one of its short class that outgrows the 128-row ring."""
    rng = np.random.default_rng([seed, KINDS.index(kind), PATTERNS.index(pattern), int(nan)])
    ts, amt, seg = [], [], [0]
    for L in LENGTHS * reps:
        a = amounts(kind, L, rng)
        ts.append(times(pattern, L, rng))
        amt.append(with_nan(a, rng) if nan else a)
        seg.append(seg[-1] + L)
    if escape:
        ets, eamt = escape_segment()
        ts.append(ets); amt.append(eamt); seg.append(seg[-1] + len(ets))
    return np.concatenate(ts), np.concatenate(amt), np.asarray(seg, np.int64)


def table(kind, pattern="dense", nan=False, seed=0, reps=1, escape=True):
    """The segments as customers of a time-sorted transaction table: dict of ts, customer (int32, the
    segment's index), terminal (int32 < N_TERMINALS), amount, fraud (uint8, 5 %) + n_customers,
    n_terminals, escape (the escape segment's customer id, the last one; None without it)."""
    ts, amt, seg = segments(kind, pattern, nan, seed, reps, escape)
    rng = np.random.default_rng([seed, 77, KINDS.index(kind)])
    cust = np.repeat(np.arange(len(seg) - 1, dtype=np.int32), np.diff(seg))
    o = np.argsort(ts, kind="stable")  # ties keep the segment order, a segment's rows their own
    n = len(o)
    return {"ts": ts[o], "customer": cust[o], "terminal": rng.integers(0, N_TERMINALS, n).astype(np.int32),
            "amount": amt[o], "fraud": (rng.random(n) < 0.05).astype(np.uint8),
            "n_customers": len(seg) - 1, "n_terminals": N_TERMINALS, "escape": len(seg) - 2 if escape else None}


CANON_NAN = np.array([np.nan]).view(np.int64)[0]


def bits(a):
    """float64 -> int64 bit patterns with every NaN replaced by one canonical NaN (x86 and the GPU
    give NaNs of different sign for inf - inf); integers -> their float64 value's bits."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind in "iub":
        a = a.astype(np.float64)
    assert a.dtype == np.float64, a.dtype
    b = a.view(np.int64).copy()
    b[np.isnan(a)] = CANON_NAN
    return b


def same_bits(got, want, what=""):
    """Bit for bit: +0.0 and -0.0 differ, all NaNs are one value, counts compare exactly."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = bits(got), bits(want)
    bad = np.argwhere(g != w)
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} cells differ, first at {i}: "
                             f"got {got[i]!r} ({g[i]:#018x}), want {want[i]!r} ({w[i]:#018x})")


def pandas_customer_windows(ts, amt, seg, windows=(1, 7, 30)):
    """get_customer_spending_behaviour_features' three lines per segment and window:
    rolling(f"{w}d").sum(), .count(), sum / count  ->  (nb [W, n], avg [W, n]) float64."""
    import pandas as pd

    n = len(ts)
    nb, avg = np.zeros((len(windows), n)), np.zeros((len(windows), n))
    for a, b in zip(seg[:-1], seg[1:]):
        if b == a:
            continue
        s = pd.Series(amt[a:b], index=pd.DatetimeIndex(ts[a:b].astype("datetime64[ns]")))
        for k, w in enumerate(windows):
            sm = s.rolling(f"{w}d").sum()
            ct = s.rolling(f"{w}d").count()
            nb[k, a:b] = ct.values
            avg[k, a:b] = (sm / ct).values
    return nb, avg
