"""Retiring idle keys (include/fdx.h, f-10): a plain numpy / dict model, the inputs and the
driver that tests/test_retire_ref.py (CPU), tests/test_gpu_retire.py and
tests/test_gpu_stream_retire.py share.

Three parts: the idle rule of each half (idle), the order-preserving id map (id_map) and the key
directory as tests/keydir_ref.py's dict model with a remap (DirModel).  HalfSim puts them together
for one key space of a stream: it numbers the keys of each batch, remembers every key's last ts,
retires at a watermark, and records for every row the incarnation of its key (a key that was
retired and comes back is a new key), from which the filtered histories follow."""
import numpy as np

import stream_label_ref as R
from bench_stream import RAW_ID_SCRAMBLE, raw_id_scramble
from keydir_ref import KeyDirModel

DAY = R.DAY
B = 257
I64_MIN = -2 ** 63


def horizons(windows_days=(1, 7, 30), delay_days=7):
    """-> (customer, terminal) horizon in ns: the longest window; delay + the longest window"""
    w = max(int(d) for d in windows_days) * DAY
    return w, int(delay_days) * DAY + w


def idle(n, last_ts, watermark, horizon):
    """The retired keys: no rows, or the last row a whole horizon before the watermark
    (inclusive, as the kernels compare; the cut-off saturates at INT64_MIN).  Python ints, so
    nothing overflows here."""
    cut = max(int(watermark) - int(horizon), I64_MIN)
    return np.array([int(c) == 0 or int(t) <= cut for c, t in zip(n, last_ts)], bool)


def id_map(retired):
    """-> (map, kept): map[id] = rank among the survivors, -1 when retired"""
    retired = np.asarray(retired, bool)
    m = np.where(retired, -1, np.cumsum(~retired) - 1).astype(np.int32)
    return m, int((~retired).sum())


class DirModel(KeyDirModel):
    def remap(self, m, kept):
        """fdx_keydir_remap: key_of compacted by the map, ids renumbered, held = kept; the
        refusal counters stay.  ValueError where the C call refuses."""
        m = [int(v) for v in m]
        held = len(self.key_of)
        if len(m) < held or len(m) > self.capacity:
            raise ValueError("map length")
        want, _ = id_map([v < 0 for v in m[:held]])
        if any(v < -1 for v in m[:held]) or m[:held] != want.tolist() or kept != sum(v >= 0 for v in m[:held]):
            raise ValueError("map")
        self.key_of = [k for k, v in zip(self.key_of, m) if v >= 0]
        self.ids = {k: i for i, k in enumerate(self.key_of)}


class HalfSim:
    """One key space of a stream with retirements."""

    def __init__(self, capacity, horizon):
        self.dir, self.horizon = DirModel(capacity), int(horizon)
        self.last, self.inc = {}, {}      # key -> last ts; key -> incarnations retired so far
        self.peak = self.retired = 0
        self.row_inc = []                 # per row fed: (key, incarnation)

    def feed(self, keys, ts):
        ids = self.dir.map(keys, True)
        for k, t in zip((int(k) for k in keys), (int(t) for t in ts)):
            self.last[k] = max(self.last.get(k, t), t)   # late terminal rows do not move last_ts back
            self.row_inc.append((k, self.inc.get(k, 0)))
        self.peak = max(self.peak, len(self.dir.key_of))
        return ids

    def retire(self, watermark):
        """-> (map over the capacity, kept, keys retired)"""
        held = list(self.dir.key_of)
        dead = idle([1] * len(held), [self.last[k] for k in held], watermark, self.horizon)
        m, kept = id_map(dead)
        gone = [k for k, d in zip(held, dead) if d]
        for k in gone:
            del self.last[k]
            self.inc[k] = self.inc.get(k, 0) + 1
        self.dir.remap(m, kept)
        self.retired += len(gone)
        full = np.full(self.dir.capacity, -1, np.int32)
        full[:len(m)] = m
        return full, kept, gone

    def alive_rows(self):
        """the rows fed so far whose key (this incarnation) is still held, in feed order"""
        return np.array([i for i, (k, c) in enumerate(self.row_inc) if self.inc.get(k, 0) == c and k in self.last],
                        np.int64)

    def incarnation_ids(self):
        """per row fed: a dense id of (key, incarnation) -- the key column of a table in which a
        key that came back after a retirement IS another key"""
        seen = {}
        return np.array([seen.setdefault(p, len(seen)) for p in self.row_inc], np.int64)


# ------------------------------------------------------------------------------- inputs
def era_table():
    """6,000 rows over 200 days; the ids change every 50 days: 160 customers, 100 terminals, of
    which at most 80 / 50 are live within a horizon when idle keys are retired every second batch."""
    c = dict(R.table(n=6000, n_c=40, n_t=25, days=200))
    era = (c["ts"] - R.BASE) // DAY // 50
    c["customer"] = (c["customer"] + 40 * era).astype(np.int32)
    c["terminal"] = (c["terminal"] + 25 * era).astype(np.int32)
    return c


def gap_table():
    """3,000 rows over 150 days minus those of customers < 12 on days [20, 70) and of terminals
    < 8 on days [20, 80): 2,414 rows; these 12 + 8 keys go idle past their horizon and return."""
    c = R.table(n=3000, n_c=40, n_t=25, days=150)
    day = (c["ts"] - R.BASE) // DAY
    drop = ((c["customer"] < 12) & (day >= 20) & (day < 70)) | ((c["terminal"] < 8) & (day >= 20) & (day < 80))
    return {k: v[~drop] for k, v in c.items()}


def raw(cols):
    c = dict(cols)
    for k in ("customer", "terminal"):
        c[k] = raw_id_scramble(c[k], *RAW_ID_SCRAMBLE[k])
    return c


def cuts(n, b=B):
    return np.r_[np.arange(0, n, b), n]


def simulate(cols, c, retire_before, caps, windows_days=(1, 7, 30), delay_days=7, lateness=0):
    """Feed cols in batches c with a retirement (watermark = the batch's first ts - lateness)
    before every batch j with retire_before(j).  -> (customer HalfSim, terminal HalfSim, log);
    log[j] = None or (customer alive rows, terminal alive rows, customer keys, terminal keys) just
    after the retirement before batch j."""
    hc, ht = horizons(windows_days, delay_days)
    cs, ts = HalfSim(caps[0], hc), HalfSim(caps[1], ht)
    log = []
    for j, (a, b) in enumerate(zip(c[:-1], c[1:])):
        if retire_before(j):
            wm = int(cols["ts"][a]) - lateness
            cs.retire(wm)
            ts.retire(wm)
            log.append((cs.alive_rows(), ts.alive_rows(), cs.dir.keys(), ts.dir.keys()))
        else:
            log.append(None)
        cs.feed(cols["customer"][a:b], cols["ts"][a:b])
        ts.feed(cols["terminal"][a:b], cols["ts"][a:b])
    return cs, ts, log
