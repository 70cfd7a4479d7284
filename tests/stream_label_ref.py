"""Delayed fraud reports on the streaming terminal state: a numpy model, the inputs and the
driver that tests/test_stream_label_ref.py (CPU) and tests/test_gpu_stream_labels.py share.

TerminalModel is one terminal's state as csrc/fdx_stream.hip keeps it (ring of (ts, fraud),
boundary pointers p[k], fraud counts F[k]; k = 0: delay, k = w + 1: delay + window w) with
push (a row: its NB / FRAUD counts, then the row enters the ring) and report (a fraud report:
one of the five outcomes of include/fdx.h).  It finds a report's row by a linear scan of the
live ring, not by the kernel's binary search.

The driver: rows are fed with fraud = 0 in batches [a, b); before a batch, every report that
is due is applied: report time ts_i + lag_i <= ts[a] (and i < a: the row was fed).  The
reference for a batch is oracle.featurize_arrays over rows [0, b) with the fraud vector as
known before that batch, restricted to [a, b)."""
import functools

import numpy as np

import oracle

NS = 1_000_000_000
DAY = 86_400 * NS
BASE = 1_717_200_000 * NS
OUTCOMES = ("on_time", "late", "duplicate", "expired", "unmatched")
PARAMS = [((1, 7, 30), 7), ((2, 5), 3), ((1, 2, 4, 8, 16, 32), 7)]


class TerminalModel:
    def __init__(self, ring, tb):
        self.T, self.tb = int(ring), [int(b) for b in tb]
        self.ts = np.zeros(self.T, np.int64)
        self.fr = np.zeros(self.T, bool)
        self.n = 0
        self.p = [0] * len(self.tb)
        self.F = [0] * len(self.tb)

    def push(self, t, fraud=0):
        """-> ([NB_w], [FRAUD_w]) of a row at t, then the row enters the ring"""
        for k, b in enumerate(self.tb):
            while self.p[k] < self.n and self.ts[self.p[k] % self.T] <= t - b:
                self.F[k] += int(self.fr[self.p[k] % self.T])
                self.p[k] += 1
        assert self.n < self.T or self.n - self.T < min(self.p), "ring overflow: not modelled"
        nb = [self.p[0] - self.p[k] for k in range(1, len(self.tb))]
        fr = [self.F[0] - self.F[k] for k in range(1, len(self.tb))]
        self.ts[self.n % self.T], self.fr[self.n % self.T] = t, bool(fraud)
        self.n += 1
        return nb, fr

    def report(self, t):
        lo = max(0, self.n - self.T)
        tied = [r for r in range(lo, self.n) if self.ts[r % self.T] == t]
        for r in tied:
            if not self.fr[r % self.T]:
                self.fr[r % self.T] = True
                for k in range(len(self.tb)):     # as if the label had been there when p[k] passed
                    self.F[k] += r < self.p[k]
                return "on_time" if r >= self.p[0] else "late"
        if tied:
            return "duplicate"
        if self.n > self.T and t < self.ts[lo % self.T]:
            return "expired"
        return "unmatched"


class StreamModel:
    """The terminal half of StreamState + report_frauds / label_counts over n_term terminals."""

    def __init__(self, n_term, windows_days=(1, 7, 30), delay_days=7, ring=256):
        self.tb = [delay_days * DAY] + [(delay_days + w) * DAY for w in windows_days]
        self.W, self.ring, self.n_term = len(windows_days), ring, n_term
        self.reset()

    def reset(self):
        self.terms = [TerminalModel(self.ring, self.tb) for _ in range(self.n_term)]
        self.counts = dict.fromkeys(OUTCOMES, 0)

    def update(self, ts, term, fraud=None):
        """-> [n, 2W]: (NB_w, RISK_w) per window, the terminal columns of X"""
        out = np.zeros((len(ts), 2 * self.W))
        for i in np.argsort(ts, kind="stable"):
            nb, fr = self.terms[term[i]].push(int(ts[i]), 0 if fraud is None else fraud[i])
            out[i, 0::2] = nb
            out[i, 1::2] = [f / n if n > 0 else 0.0 for f, n in zip(fr, nb)]
        return out

    def report(self, ts, term):
        for i in np.argsort(ts, kind="stable"):
            if 0 <= term[i] < self.n_term:       # the kernel flags the others and skips them
                self.counts[self.terms[term[i]].report(int(ts[i]))] += 1

    def label_counts(self):
        return dict(self.counts)


# ------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def table(seed=11, n=6000, n_c=25, n_t=40, days=90, rate=0.1):
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.integers(0, days * 86400, n)) * NS + BASE
    ts[1000:1100] = ts[1000]                      # a 100-row tie run (cuts() cuts it at 1050)
    cols = {"ts": ts, "customer": rng.integers(0, n_c, n).astype(np.int32),
            "terminal": rng.integers(0, n_t, n).astype(np.int32), "amount": np.round(rng.uniform(0, 100, n), 2),
            "fraud": (rng.random(n) < rate).astype(np.uint8)}
    cols["fraud"][1040:1060] = 1                  # reports for rows of the tie run, either side of the cut
    cols["terminal"][1044:1050] = 3               # ... several of them tied on (terminal, ts), across the cut
    cols["terminal"][1050:1054] = 3
    return cols


def cuts(ts, delay_days, seed=5):
    """Batch boundaries: a time grid of delay / 4 (so that every batch spans less than
    delay / 2), 12 random rows, and row 1050 inside the tie run."""
    rng = np.random.default_rng(seed)
    grid = np.searchsorted(ts, np.arange(ts[0], ts[-1] + 1, delay_days * DAY // 4))
    return np.unique(np.r_[0, grid, rng.integers(1, len(ts), 12), 1050, len(ts)])


def max_span(ts, c):
    return int(max(ts[b - 1] - ts[a] for a, b in zip(c[:-1], c[1:])))


def lags(kind, ts, c, delay_days, seed=9):
    """kind "on_time": uniform in [1 s, delay / 2 - the longest batch span];
    kind "late": uniform in [0, 3 x delay]."""
    rng = np.random.default_rng(seed)
    if kind == "on_time":
        hi = delay_days * DAY // 2 - max_span(ts, c)
        assert hi > NS
        return rng.integers(NS, hi + 1, len(ts))
    return rng.integers(0, 3 * delay_days * DAY + 1, len(ts))


def schedule(ts, fraud, lag, c, flush):
    """-> due[j], j = 0 .. J: the rows whose reports are applied before batch j (J batches);
    due[J] after the last batch.  flush "after": what is still outstanding goes to due[J];
    flush "before_last": the outstanding reports of rows already fed go before the last batch
    (the `one extra batch after the last report`), due[J] is empty."""
    J = len(c) - 1
    fr = np.flatnonzero(fraud)
    done = np.zeros(len(ts), bool)
    due = []
    for j in range(J):
        a = c[j]
        d = fr[(fr < a) & ~done[fr] & (ts[fr] + lag[fr] <= ts[a])]
        if j == J - 1 and flush == "before_last":
            d = fr[(fr < a) & ~done[fr]]
        done[d] = True
        due.append(d)
    due.append(fr[~done[fr]] if flush == "after" else fr[:0])
    return due


def fed_late(cols, c, due, delay_days):
    """Per applied report: was a row of its terminal with ts >= ts_i + delay fed in an earlier
    batch?  (Then the delay boundary has passed row i and the report is late.)  -> count"""
    ts, term = cols["ts"], cols["terminal"]
    late = 0
    for j, d in enumerate(due):
        a = c[j] if j < len(c) - 1 else len(ts)   # rows fed so far
        for i in d:
            late += bool(np.any((term[:a] == term[i]) & (ts[:a] >= ts[i] + delay_days * DAY)))
    return late


def term_cols(f, windows):
    return np.stack([f[f"TERMINAL_ID_{k}_{w}DAY_WINDOW"] for w in windows for k in ("NB_TX", "RISK")], axis=1)


def reference_true(cols, windows, delay_days):
    return term_cols(oracle.featurize_arrays(cols["ts"], cols["customer"], cols["terminal"], cols["amount"],
                                             cols["fraud"], windows, delay_days), windows)


def reference_known_before(cols, c, due, windows, delay_days):
    """[n, 2W]: batch j's rows from the oracle over rows [0, b_j) with the labels known before it"""
    n = len(cols["ts"])
    known = np.zeros(n, np.uint8)
    out = np.zeros((n, 2 * len(windows)))
    for j, (a, b) in enumerate(zip(c[:-1], c[1:])):
        known[due[j]] = 1
        f = oracle.featurize_arrays(cols["ts"][:b], cols["customer"][:b], cols["terminal"][:b], cols["amount"][:b],
                                    known[:b], windows, delay_days)
        out[a:b] = term_cols(f, windows)[a:b]
    return out


@functools.lru_cache(maxsize=None)
def case(kind, windows, delay_days):
    """The inputs and references of one parametrisation, computed once: kind "on_time" (test 1)
    or "late" (test 2).  Treat the arrays as read-only."""
    cols = table()
    c = cuts(cols["ts"], delay_days)
    lag = lags(kind, cols["ts"], c, delay_days)
    due = schedule(cols["ts"], cols["fraud"], lag, c, "after" if kind == "on_time" else "before_last")
    return {"cols": cols, "cuts": c, "lag": lag, "due": due, "true": reference_true(cols, windows, delay_days),
            "known": reference_known_before(cols, c, due, windows, delay_days),
            "late": fed_late(cols, c, due, delay_days)}


def drive(be, cols, c, due):
    """Feed the batches unlabelled through backend `be` (update(cols, a, b) -> [b - a, 2W]
    terminal columns; report(ts, terminal)), each preceded by its due reports.  -> [n, 2W]"""
    out = None
    for j, (a, b) in enumerate(zip(c[:-1], c[1:])):
        if len(due[j]):
            be.report(cols["ts"][due[j]], cols["terminal"][due[j]])
        x = be.update(cols, a, b)
        out = np.zeros((len(cols["ts"]), x.shape[1])) if out is None else out
        out[a:b] = x
    if len(due[-1]):
        be.report(cols["ts"][due[-1]], cols["terminal"][due[-1]])
    return out


class ModelBackend:
    def __init__(self, n_term, windows, delay_days, ring=256):
        self.m = StreamModel(n_term, windows, delay_days, ring)

    def update(self, cols, a, b):
        return self.m.update(cols["ts"][a:b], cols["terminal"][a:b])

    def report(self, ts, term):
        self.m.report(ts, term)

    def label_counts(self):
        return self.m.label_counts()


# ------------------------------------------------- outcomes at the smallest shapes (test 3)
H12 = DAY // 2


def outcome_script(be):
    """One terminal (id 0 of 2), terminal_ring 8, windows (1,), delay 1, rows 12 h apart: no ring
    overflow.  `be`: update(cols, a, b) / report(ts, terminal) / label_counts().  Runs the
    steps and -> the list of (step, observation) that OUTCOME_EXPECTED spells out."""
    obs = []
    z = lambda k: np.zeros(k, np.int32)  # noqa: E731
    feed = lambda t, term=None: be.update({"ts": np.asarray(t, np.int64),  # noqa: E731
                                           "terminal": z(len(t)) if term is None else np.asarray(term, np.int32)},
                                          0, len(t))
    rep = lambda t, term=None: be.report(np.asarray(t, np.int64),  # noqa: E731
                                         z(len(t)) if term is None else np.asarray(term, np.int32))
    cnt = lambda: tuple(be.label_counts()[k] for k in OUTCOMES)  # noqa: E731
    t = BASE + np.arange(12) * H12
    feed(t[:5])
    feed(t[5:])                                   # 12 rows in a ring of 8: rows 4 .. 11 live
    feed([BASE + 5 * DAY], [1])                   # a row of the other terminal
    rep([t[1]])                                   # 10 back from the last row: evicted
    obs.append(("expired", cnt()))
    rep([t[8] + H12 // 2, BASE + 100 * DAY])      # between two rows; after the last row
    obs.append(("unmatched", cnt()))
    rep([t[11], t[11]])                           # the same row twice in one call
    obs.append(("twice in one call", cnt()))
    rep([t[11]])                                  # and again in a later call
    obs.append(("again later", cnt()))
    tie = BASE + 6 * DAY
    feed([tie, tie, tie])                         # rows 12 .. 14 tied
    rep([tie, tie])                               # two of the three in ONE call (one chain)
    obs.append(("two of three tied", cnt()))
    # t = 7.5 d: delay boundary at 6.5 d (all 15 rows), window boundary at 5.5 d (rows 0 .. 11):
    # NB = 3 (the tied rows), FRAUD = (row 11 + two bits) - (row 11) = 2 -- exactly two bits set;
    # the expired / unmatched / duplicate reports left no trace
    obs.append(("feature after", feed([BASE + 7 * DAY + H12])[0].tolist()))
    rep([tie])                                    # the third tied row (a sibling, by now late)
    rep([tie])                                    # all three marked: duplicate
    obs.append(("third and fourth tied", cnt()))
    obs.append(("feature after late", feed([BASE + 7 * DAY + H12])[0].tolist()))
    rep([tie, tie], [-1, 2])                      # ids outside [0, 2): flagged, skipped
    rep([], [])                                   # n = 0
    obs.append(("bad ids, empty", cnt()))
    # the other terminal: its one row at 5 d is inside (t - 2 d, t - 1 d] at t = 6.5 d, unlabelled
    obs.append(("other terminal", feed([BASE + 6 * DAY + H12], [1])[0].tolist()))
    return obs


#                                              on_time late dup expired unmatched
OUTCOME_EXPECTED = [("expired", (0, 0, 0, 1, 0)),
                    ("unmatched", (0, 0, 0, 1, 2)),
                    ("twice in one call", (1, 0, 1, 1, 2)),
                    ("again later", (1, 0, 2, 1, 2)),
                    ("two of three tied", (3, 0, 2, 1, 2)),
                    ("feature after", [3.0, 2.0 / 3.0]),
                    ("third and fourth tied", (3, 1, 3, 1, 2)),
                    ("feature after late", [3.0, 1.0]),
                    ("bad ids, empty", (3, 1, 3, 1, 2)),
                    ("other terminal", [1.0, 0.0])]
