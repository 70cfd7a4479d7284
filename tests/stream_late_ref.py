"""Late terminal rows on the streaming terminal state (f-8): a plain numpy model, the inputs and
the scripts that tests/test_stream_late_ref.py (CPU) and tests/test_gpu_stream_late.py share.

The model keeps, per terminal, every row that arrived, sorted by (ts, arrival).  A row's counts
are taken over what had arrived before it -- arrival order is batch order, and inside a batch
(ts, row) order:
    NB_w    = #{arrived j : t - tb[w + 1] < ts_j <= t - tb[0]}
    FRAUD_w = the fraud rows among them            (tb[0] = delay, tb[w + 1] = delay + window w)
It counts by comparing timestamps, not with the kernel's pointers and ring.  Of the ring it
knows only what the refusal rules of include/fdx.h need: the live rows are the last
min(n, ring) of the sorted rows.  A row with t < the terminal's last ts is late:
  * more than max_late behind: status bit 8, zero counts, not inserted;
  * its farthest window (t - tb[W]) starts before the oldest live row -- unless n <= ring on a
    state that was never restored: status bit 16, zero counts, not inserted;
  * else inserted; late_rows += 1, late_past_delay += (t <= last - tb[0]).
A push onto a full ring drops the oldest live row; if some boundary has not passed that row yet
(its ts > last - tb[k] for some k), status bit 2 is raised and the model stops following that
terminal (as tests/stream_label_ref.py: an overflowed ring is not modelled).
restore() is what a snapshot + restore does to the rows: only those from the oldest boundary
on (ts > last - tb[W]) are carried, and from then on only the strict coverage rule holds."""
import functools

import numpy as np

import oracle

NS = 1_000_000_000
DAY = 86_400 * NS
BASE = 1_717_200_000 * NS
WINDOWS, DELAY, N_TERM = (1, 7, 30), 7, 16
ST_TERM_RING, ST_ORDER, ST_LATE_RING = 2, 8, 16


class Terminal:
    def __init__(self):
        self.ts, self.fr = [], []   # the rows that arrived and were inserted, sorted by (ts, arrival)
        self.last = None
        self.broken = False

    def count(self, lo, hi):
        """-> (rows, fraud rows) with lo < ts <= hi"""
        ts = np.asarray(self.ts, np.int64)
        m = (ts > lo) & (ts <= hi)
        return int(m.sum()), int(np.asarray(self.fr, np.int64)[m].sum())


class StreamLateModel:
    """The terminal half of StreamState with a terminal lateness, over n_term terminals."""

    def __init__(self, n_term=N_TERM, windows_days=WINDOWS, delay_days=DELAY, ring=64, lateness_days=0.0):
        self.tb = [delay_days * DAY] + [(delay_days + w) * DAY for w in windows_days]
        self.W, self.ring, self.n_term = len(windows_days), int(ring), n_term
        self.max_late = int(round(lateness_days * DAY))
        self.reset()

    def reset(self):
        self.terms = [Terminal() for _ in range(self.n_term)]
        self.counts = {"late_rows": 0, "late_past_delay": 0}
        self.status, self.restored = 0, False

    def take_status(self):
        s, self.status = self.status, 0
        return s

    def late_counts(self):
        return dict(self.counts)

    def restore(self):
        for k in self.terms:
            if k.last is not None:
                keep = [i for i, t in enumerate(k.ts) if t > k.last - self.tb[-1]]
                k.ts, k.fr = [k.ts[i] for i in keep], [k.fr[i] for i in keep]
        self.restored = True

    def _push(self, k, t, fraud):
        """-> ([NB_w], [FRAUD_w]) of one row of terminal k, then the row lands (or is refused)"""
        zero = [0] * self.W, [0] * self.W
        n, T = len(k.ts), self.ring
        late = k.last is not None and t < k.last
        if late:
            if k.last - t > self.max_late:
                self.status |= ST_ORDER
                return zero
            oldest = k.ts[max(0, n - T)]
            if not ((n <= T and not self.restored) or oldest <= t - self.tb[-1]):
                self.status |= ST_LATE_RING
                return zero
        ends = [k.count(t - b, t - self.tb[0]) for b in self.tb[1:]]
        at = int(np.searchsorted(np.asarray(k.ts, np.int64), t, side="right"))  # after its ties
        k.ts.insert(at, t)
        k.fr.insert(at, int(bool(fraud)))
        if late:
            self.counts["late_rows"] += 1
            self.counts["late_past_delay"] += t <= k.last - self.tb[0]
        else:
            k.last = t
        if n >= T and k.ts[n - T] > k.last - self.tb[-1]:   # the dropped row (position n - T) is still needed
            self.status |= ST_TERM_RING
            k.broken = True
        return [e[0] for e in ends], [e[1] for e in ends]

    def update(self, ts, term, fraud=None):
        """One batch -> (NB [n, W], FRAUD [n, W]) int64"""
        nb, fr = np.zeros((len(ts), self.W), np.int64), np.zeros((len(ts), self.W), np.int64)
        for i in np.argsort(np.asarray(ts, np.int64), kind="stable"):
            k = self.terms[term[i]]
            assert not k.broken, "a terminal whose ring overflowed is not modelled"
            nb[i], fr[i] = self._push(k, int(ts[i]), 0 if fraud is None else fraud[i])
        return nb, fr


def columns(nb, fr):
    """(NB, FRAUD) -> [n, 2W] float64: (NB_w, RISK_w) per window, the terminal columns of X"""
    nb, fr = np.asarray(nb, np.int64), np.asarray(fr, np.int64)
    out = np.zeros((nb.shape[0], 2 * nb.shape[1]))
    out[:, 0::2] = nb
    out[:, 1::2] = np.where(nb > 0, fr / np.maximum(nb, 1), 0.0)
    return out


def words(nb, fr):
    """(NB, FRAUD) -> [n, W] int64 count records NB | FRAUD << 32"""
    return np.asarray(nb, np.int64) | (np.asarray(fr, np.int64) << 32)


def oracle_columns(ts, term, fraud, windows=WINDOWS, delay=DELAY):
    """The C oracle's terminal columns [n, 2W] over a history in time order."""
    n = len(ts)
    f = oracle.featurize_arrays(np.asarray(ts, np.int64), np.zeros(n, np.int32), np.asarray(term, np.int32),
                                np.ones(n), np.asarray(fraud, np.uint8), windows, delay)
    return np.stack([f[f"TERMINAL_ID_{k}_{w}DAY_WINDOW"] for w in windows for k in ("NB_TX", "RISK")], axis=1)


# ------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def history(seed=3, n=400, days=60, rate=0.15):
    """n rows of N_TERM terminals over `days` days in time order, every ts distinct (no ties)."""
    rng = np.random.default_rng(seed)
    ts = np.sort(rng.choice(days * 86400, n, replace=False)).astype(np.int64) * NS + BASE
    return {"ts": ts, "terminal": rng.integers(0, N_TERM, n).astype(np.int32),
            "fraud": (rng.random(n) < rate).astype(np.uint8)}


@functools.lru_cache(maxsize=None)
def disordered(max_lag_days, frac=0.4, batch_days=1.5, lag_until_day=None, seed=8):
    """history() as it arrives when `frac` of the rows (only those before lag_until_day, if given)
    are held back by a lag uniform in (0, max_lag_days]: arrival = ts + lag, the stream is the
    rows in arrival order, cut into batches on a grid of batch_days of arrival time.  A row is
    behind its terminal's latest row by at most its lag.  -> dict: order (history rows in arrival
    order), cuts (batch bounds into order), lag (per history row), last_late (the batch index of
    the last row that arrives behind its terminal's latest row)."""
    h = history()
    rng = np.random.default_rng(seed)
    n = len(h["ts"])
    lag = np.where(rng.random(n) < frac, rng.integers(1, int(max_lag_days * DAY) + 1, n), 0)
    if lag_until_day is not None:
        lag[h["ts"] >= BASE + lag_until_day * DAY] = 0
    arrival = h["ts"] + lag
    order = np.argsort(arrival, kind="stable")
    grid = np.arange(arrival.min(), arrival.max() + 1, int(batch_days * DAY))
    cuts = np.unique(np.r_[0, np.searchsorted(arrival[order], grid), n])
    last, last_late, n_late, worst = {}, -1, 0, 0
    for j, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        rows = order[a:b]
        for i in rows[np.argsort(h["ts"][rows], kind="stable")]:
            k, t = int(h["terminal"][i]), int(h["ts"][i])
            if k in last and t < last[k]:
                last_late, n_late, worst = j, n_late + 1, max(worst, last[k] - t)
            else:
                last[k] = t
    return {"order": order, "cuts": cuts, "lag": lag, "last_late": last_late, "n_late": n_late, "worst": worst}


def drive(be, h, order, cuts):
    """Feed history rows `order` in batches `cuts` through backend `be`
    (update(ts, terminal, fraud) -> (NB, FRAUD) [b - a, W]).  -> (NB, FRAUD) in HISTORY row order"""
    nb = fr = None
    for a, b in zip(cuts[:-1], cuts[1:]):
        r = order[a:b]
        x, y = be.update(h["ts"][r], h["terminal"][r], h["fraud"][r])
        if nb is None:
            nb, fr = np.zeros((len(h["ts"]), x.shape[1]), np.int64), np.zeros((len(h["ts"]), x.shape[1]), np.int64)
        nb[r], fr[r] = x, y
    return nb, fr


def in_order_cuts(n, step=37):
    return np.unique(np.r_[np.arange(0, n, step), n])


# ----------------------------------------------------------- scripts at the smallest shapes
def d(days):
    return BASE + int(round(days * 86400)) * NS


def feed(be, rows):
    """rows: [(day, terminal, fraud)] as ONE batch -> (NB, FRAUD) lists per row"""
    ts = np.array([d(r[0]) for r in rows], np.int64)
    nb, fr = be.update(ts, np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.uint8))
    return np.asarray(nb).tolist(), np.asarray(fr).tolist()


def ring8_script(be):
    """Ring of 8, windows (1, 7, 30), delay 7 (tb = 7, 8, 14, 37 days), lateness 40 days.  `be`:
    update(ts, terminal, fraud) and take_status() -> the bits raised since the last call.
    -> [(step, observation)] as RING8_EXPECTED spells out."""
    obs = []
    # terminal 0: rows at days 0, 10, .. 90 (n = 10: positions 2 .. 9 live, 8 and 9 in slots 0 and 1)
    for k in range(10):
        feed(be, [(10 * k, 0, k % 2)])
    # day 65, 25 days late: the oldest live row (day 20) reaches 65 - 37; it lands at position 7,
    # rows 7 .. 9 move to 8 .. 10 = slots 0 .. 2: the shift crosses the wrap.  Its own 30-day window
    # (28, 58] holds days 30, 40, 50 (fraud: 30 and 50)
    obs.append(("shift across the wrap", feed(be, [(65, 0, 1)]), be.take_status()))
    # day 100 sees the inserted row: (63, 93] holds 65, 70, 80, 90 (fraud: 65, 70, 90)
    obs.append(("in order after it", feed(be, [(100, 0, 0)]), be.take_status()))
    # terminal 1, a young ring: day 40 after days 50 and 60 lands at position lo = 0
    feed(be, [(50, 1, 1)])
    feed(be, [(60, 1, 0)])
    obs.append(("insertion at lo", feed(be, [(40, 1, 1)]), be.take_status()))
    # day 70: (33, 63] holds 40, 50, 60 (fraud: 40, 50); (56, 63] holds 60
    obs.append(("in order after it", feed(be, [(70, 1, 0)]), be.take_status()))
    # terminal 3, a FULL ring (n = 8 = T): days 40, 44, .. 68; day 30 is 38 days late and older than
    # every row: it lands at lo = 0 and is the row the full ring drops -- every boundary of day 68
    # (the farthest: 68 - 37 = 31) has passed it, so nothing is lost
    for k in range(8):
        feed(be, [(40 + 4 * k, 3, 1)])
    obs.append(("insertion at lo, full ring", feed(be, [(30, 3, 0)]), be.take_status()))
    # day 80 (it drops day 40, which (43, 73] no longer holds): 44 .. 68 = 7 rows, all fraud;
    # (66, 73] holds 68
    obs.append(("in order after it", feed(be, [(80, 3, 0)]), be.take_status()))
    # terminal 0 again (n = 12: days 40 .. 100 live): day 75 is 25 days late, its farthest window
    # starts at day 38, before the oldest live row (day 40) of a wrapped ring: bit 16, zero counts
    obs.append(("past the ring", feed(be, [(75, 0, 1)]), be.take_status()))
    # nothing was inserted: day 110's (73, 103] holds 80, 90, 100 (fraud: 90) -- not 75
    obs.append(("n unchanged", feed(be, [(110, 0, 0)]), be.take_status()))
    # terminal 2, a full ring: days 40 .. 68; day 39 is 29 days late and lands at lo = 0, but the
    # 30-day boundary of day 68 (day 31) has NOT passed it: the dropped row is still needed -> bit 2
    for k in range(8):
        feed(be, [(40 + 4 * k, 2, 0)])
    obs.append(("before the overflow", [], be.take_status()))
    obs.append(("overwrites a needed row", feed(be, [(39, 2, 0)]), be.take_status()))
    return obs


RING8_EXPECTED = [
    ("shift across the wrap", ([[0, 0, 3]], [[0, 0, 2]]), 0),
    ("in order after it", ([[0, 1, 4]], [[0, 1, 3]]), 0),
    ("insertion at lo", ([[0, 0, 0]], [[0, 0, 0]]), 0),
    ("in order after it", ([[0, 1, 3]], [[0, 0, 2]]), 0),
    ("insertion at lo, full ring", ([[0, 0, 0]], [[0, 0, 0]]), 0),
    ("in order after it", ([[0, 1, 7]], [[0, 1, 7]]), 0),
    ("past the ring", ([[0, 0, 0]], [[0, 0, 0]]), ST_LATE_RING),
    ("n unchanged", ([[0, 1, 3]], [[0, 0, 1]]), 0),
    ("before the overflow", [], 0),
    ("overwrites a needed row", ([[0, 0, 0]], [[0, 0, 0]]), ST_TERM_RING),
]


def ties_script(be):
    """Ring of 64, lateness 40 days.  -> (rows fed [(day, terminal, fraud)] in arrival order,
    (NB, FRAUD) per row in that order).  The counts do not depend on the order among tied rows."""
    batches = [
        [(10, 5, 1)], [(20, 5, 0)], [(20, 5, 1)], [(30, 5, 0)],
        [(20, 5, 1)],                          # late, tied with two live rows: lands after them
        [(15, 5, 1), (15, 5, 0)],              # two late rows tied with each other in one batch
        [(12, 5, 1), (41, 5, 0), (22, 5, 0)],  # late and in-order rows of one terminal in one batch
        [(29, 5, 1), (29, 6, 1), (48, 5, 0)],  # ... and a first row of another terminal between them
        [(50, 5, 0), (52, 5, 1), (60, 5, 0)],  # in order: every landed row is seen
    ]
    rows, nb, fr = [], [], []
    for b in batches:
        x, y = feed(be, b)
        rows += b
        nb += x
        fr += y
    return rows, np.array(nb, np.int64), np.array(fr, np.int64)


def too_late_script(be):
    """Lateness 12 days.  `be` also has reset() and late_counts()."""
    obs = []
    feed(be, [(0, 0, 1)])
    feed(be, [(20, 0, 0)])
    obs.append(("13 days late", feed(be, [(7, 0, 1)]), be.take_status()))
    # 12 days late: (1 - w, 1] holds day 0 (fraud) for the 7- and 30-day windows, not for (0, 1]
    obs.append(("12 days late", feed(be, [(8, 0, 1)]), be.take_status()))
    obs.append(("counters", be.late_counts()))
    be.reset()
    obs.append(("after reset", feed(be, [(7, 0, 1)]), be.take_status(), be.late_counts()))
    obs.append(("usable", feed(be, [(15, 0, 0)]), be.take_status()))
    return obs


ZERO = ([[0, 0, 0]], [[0, 0, 0]])
TOO_LATE_EXPECTED = [
    ("13 days late", ZERO, ST_ORDER),
    ("12 days late", ([[0, 1, 1]], [[0, 1, 1]]), 0),
    ("counters", {"late_rows": 1, "late_past_delay": 1}),
    ("after reset", ZERO, 0, {"late_rows": 0, "late_past_delay": 0}),
    ("usable", ([[0, 1, 1]], [[0, 1, 1]]), 0),   # day 15: (1, 8] and (-22, 8] hold day 7, (7, 8] does not
]


def restore_script(be):
    """Lateness 12 days, ring of 64.  `be` also has restore(): snapshot the state and go on with a
    state restored from it.  Terminal 1 has rows every 5 days up to day 100, of which the snapshot
    carries days 65 .. 100 (ts > 100 - 37); terminal 2 is young (days 90 and 100)."""
    obs = []
    for day in range(0, 101, 5):
        feed(be, [(day, 1, day % 2)])
    feed(be, [(90, 2, 0)])
    feed(be, [(100, 2, 1)])
    be.restore()
    # n <= ring proves nothing now: the young terminal's late row is refused ...
    obs.append(("young terminal", feed(be, [(95, 2, 1)]), be.take_status()))
    # ... and so is terminal 1's while its oldest carried row (day 65) is younger than 97 - 37
    obs.append(("carried rows too young", feed(be, [(97, 1, 1)]), be.take_status()))
    feed(be, [(120, 1, 0)])
    # day 110, 10 days late: day 65 <= 110 - 37, accepted; (73, 103] holds 75 .. 100 (6 rows; fraud:
    # 75, 85, 95), (96, 103] holds day 100
    obs.append(("carried rows reach", feed(be, [(110, 1, 1)]), be.take_status()))
    obs.append(("counters", be.late_counts()))
    # day 125: (88, 118] holds 90, 95, 100, 110 (fraud: 95, 110); (111, 118] is empty
    obs.append(("in order after it", feed(be, [(125, 1, 0)]), be.take_status()))
    return obs


RESTORE_EXPECTED = [
    ("young terminal", ZERO, ST_LATE_RING),
    ("carried rows too young", ZERO, ST_LATE_RING),
    ("carried rows reach", ([[0, 1, 6]], [[0, 0, 3]]), 0),
    ("counters", {"late_rows": 1, "late_past_delay": 1}),
    ("in order after it", ([[0, 0, 4]], [[0, 0, 2]]), 0),
]
