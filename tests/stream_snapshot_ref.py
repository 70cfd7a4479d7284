"""The streaming state's snapshot (f-7): a numpy model of both halves of the state and of the
snapshot format, written from the text of include/fdx.h alone, shared by
tests/test_stream_snapshot_ref.py (CPU) and tests/test_gpu_stream_snapshot.py.

CustomerModel is one customer's state: the pandas roll_sum recurrence per window in Python
floats (IEEE doubles, no fused multiply-add), the window tails and a ring of (ts, amount).
The terminal half is stream_label_ref.TerminalModel plus the last_ts word.  StateModel holds
n_customers + n_terminals of them and can snapshot (any key selection) and restore (any
placement, any ring size that fits); encode / decode translate between bytes and a dict.
The models assert that no ring overflows."""
import functools
import struct

import numpy as np

import oracle
import stream_label_ref as R
from stream_label_ref import DAY, OUTCOMES, TerminalModel

HEADER_WORDS = 64
MAGIC = int.from_bytes(b"FDXSNAP1", "little")
(H_MAGIC, H_VERSION, H_BYTES, H_WINDOWS, H_WIN0, H_DELAY, H_MODE, H_CRING, H_TRING, H_CKEYS, H_CENT, H_CMAX, H_TKEYS,
 H_TENT, H_TMAX, H_LABELS, H_OFF) = (0, 1, 2, 3, 4, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 27)


def f2i(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def i2f(w):
    return struct.unpack("<d", struct.pack("<q", w))[0]


class CustomerModel:
    def __init__(self, ring, win):
        self.C, self.win, W = int(ring), [int(w) for w in win], len(win)
        self.ts, self.amt = np.zeros(self.C, np.int64), np.zeros(self.C)
        self.n = self.last = 0
        self.tail = [0] * W
        self.sum, self.c_add, self.c_rem, self.prev = ([0.0] * W for _ in range(4))
        self.nobs, self.nsame = [0] * W, [0] * W

    def push(self, t, v):
        """-> ([NB_w], [AVG_w]) of a row (t, v), then the row enters the ring"""
        v = float(v)
        nb, avg = [], []
        for w, win in enumerate(self.win):
            nt = self.tail[w]
            while nt < self.n and self.ts[nt % self.C] <= t - win:      # remove_sum
                x = float(self.amt[nt % self.C])
                self.nobs[w] -= 1
                y = -x - self.c_rem[w]
                s = self.sum[w] + y
                self.c_rem[w] = (s - self.sum[w]) - y
                self.sum[w] = s
                nt += 1
            if nt >= self.n:                                            # the window restarts
                self.sum[w] = self.c_add[w] = self.c_rem[w] = 0.0
                self.prev[w], self.nobs[w], self.nsame[w] = v, 0, 0
            self.nobs[w] += 1                                           # add_sum
            y = v - self.c_add[w]
            s = self.sum[w] + y
            self.c_add[w] = (s - self.sum[w]) - y
            self.sum[w] = s
            self.nsame[w] = self.nsame[w] + 1 if v == self.prev[w] else 1
            self.prev[w] = v
            self.tail[w] = nt
            val = self.prev[w] * self.nobs[w] if self.nsame[w] >= self.nobs[w] else self.sum[w]
            nb.append(self.nobs[w])
            avg.append(val / self.nobs[w])
        assert self.n < self.C or self.n - self.C < min(self.tail), "customer ring overflow: not modelled"
        self.ts[self.n % self.C], self.amt[self.n % self.C] = t, v
        self.n += 1
        self.last = t
        return nb, avg

    # record words [n, last_ts, (tail, sum, c_add, c_rem, prev, nobs | nsame << 32) x W], entries (ts, amount)
    def export(self):
        lo = min([self.n] + self.tail)
        rec = [self.n - lo, self.last]
        for w in range(len(self.win)):
            rec += [self.tail[w] - lo, f2i(self.sum[w]), f2i(self.c_add[w]), f2i(self.c_rem[w]), f2i(self.prev[w]),
                    (self.nobs[w] & 0xFFFFFFFF) | (self.nsame[w] & 0xFFFFFFFF) << 32]
        return rec, [(int(self.ts[r % self.C]), float(self.amt[r % self.C])) for r in range(lo, self.n)]

    def load(self, rec, ent):
        assert len(ent) == rec[0] <= self.C, "live rows exceed the ring"
        self.n, self.last = rec[0], rec[1]
        for w in range(len(self.win)):
            r = rec[2 + 6 * w:8 + 6 * w]
            self.tail[w] = r[0]
            self.sum[w], self.c_add[w], self.c_rem[w], self.prev[w] = (i2f(x) for x in r[1:5])
            self.nobs[w], self.nsame[w] = r[5] & 0xFFFFFFFF, (r[5] >> 32) & 0xFFFFFFFF
        for i, (t, a) in enumerate(ent):
            self.ts[i % self.C], self.amt[i % self.C] = t, a


class Terminal(TerminalModel):
    """TerminalModel + the record's last_ts word; record [n, last_ts, (p_k, F_k) x (W + 1)],
    entries ts << 1 | fraud"""
    last = 0

    def push(self, t, fraud=0):
        out = super().push(t, fraud)
        self.last = t
        return out

    def export(self):
        lo = min([self.n] + self.p)
        rec = [self.n - lo, self.last]
        for p, F in zip(self.p, self.F):
            rec += [p - lo, F]
        return rec, [int(self.ts[r % self.T]) << 1 | int(self.fr[r % self.T]) for r in range(lo, self.n)]

    def load(self, rec, ent):
        assert len(ent) == rec[0] <= self.T, "live rows exceed the ring"
        self.n, self.last = rec[0], rec[1]
        self.p, self.F = list(rec[2::2]), list(rec[3::2])
        for i, e in enumerate(ent):
            self.ts[i % self.T], self.fr[i % self.T] = e >> 1, bool(e & 1)


def _pad16(b):
    return b + bytes(-len(b) % 16)


def encode(d):
    """dict (decode's result) -> snapshot bytes"""
    W = len(d["window_ns"])
    parts, counts = [], []
    for half, ent_dt in (("customers", np.dtype([("ts", "<i8"), ("amt", "<f8")])), ("terminals", np.dtype("<i8"))):
        keys = d[half]
        off = np.cumsum([0] + [len(e) for _, e in keys]).astype("<i8")
        rec = np.array([r for r, _ in keys], dtype=np.int64).astype("<i8")
        ent = np.array([x for _, e in keys for x in e], dtype=ent_dt)
        parts += [_pad16(rec.tobytes()), _pad16(off.tobytes()), _pad16(ent.tobytes())]
        counts.append((len(keys), int(off[-1]), max([len(e) for _, e in keys], default=0)))
    h = np.zeros(HEADER_WORDS, "<i8")
    h[H_MAGIC], h[H_VERSION], h[H_WINDOWS] = MAGIC, 1, W
    h[H_WIN0:H_WIN0 + W] = d["window_ns"]
    h[H_DELAY], h[H_MODE], h[H_CRING], h[H_TRING] = d["delay_ns"], d["flags_mode"], d["customer_ring"], d["terminal_ring"]
    h[H_CKEYS:H_CKEYS + 3], h[H_TKEYS:H_TKEYS + 3] = counts
    h[H_LABELS:H_LABELS + 5] = [d["label_counts"][k] for k in OUTCOMES]
    o = HEADER_WORDS * 8
    for i, p in enumerate(parts):
        h[H_OFF + i] = o
        o += len(p)
    h[H_BYTES] = o
    return h.tobytes() + b"".join(parts)


def decode(b):
    """snapshot bytes -> dict; the inverse of encode"""
    b = bytes(b)
    h = np.frombuffer(b[:HEADER_WORDS * 8], "<i8")
    assert h[H_MAGIC] == MAGIC and h[H_VERSION] == 1 and h[H_BYTES] == len(b)
    W = int(h[H_WINDOWS])
    d = {"window_ns": [int(x) for x in h[H_WIN0:H_WIN0 + W]], "delay_ns": int(h[H_DELAY]), "flags_mode": int(h[H_MODE]),
         "customer_ring": int(h[H_CRING]), "terminal_ring": int(h[H_TRING]),
         "label_counts": dict(zip(OUTCOMES, (int(x) for x in h[H_LABELS:H_LABELS + 5]))),
         "max_live": (int(h[H_CMAX]), int(h[H_TMAX]))}
    for half, kw, sec, R in (("customers", H_CKEYS, 0, 2 + 6 * W), ("terminals", H_TKEYS, 3, 4 + 2 * W)):
        keys, n_ent = int(h[kw]), int(h[kw + 1])
        o_rec, o_off, o_ent = (int(x) for x in h[H_OFF + sec:H_OFF + sec + 3])
        rec = np.frombuffer(b, "<i8", keys * R, o_rec).reshape(keys, R)
        off = np.frombuffer(b, "<i8", keys + 1, o_off)
        assert off[0] == 0 and off[-1] == n_ent and np.all(np.diff(off) >= 0)
        if half == "customers":
            e = np.frombuffer(b, np.dtype([("ts", "<i8"), ("amt", "<f8")]), n_ent, o_ent)
            ent = [(int(t), float(a)) for t, a in zip(e["ts"], e["amt"])]
        else:
            ent = [int(x) for x in np.frombuffer(b, "<i8", n_ent, o_ent)]
        d[half] = [([int(x) for x in rec[j]], ent[off[j]:off[j + 1]]) for j in range(keys)]
    return d


class StateModel:
    """fdx.streaming.StreamState in numpy: update (labels inline), report, snapshot, restore."""

    def __init__(self, n_customers, n_terminals, windows_days=(1, 7, 30), delay_days=7, customer_ring=256,
                 terminal_ring=256, flags_mode=0):
        self.win = [w * DAY for w in windows_days]
        self.delay = delay_days * DAY
        self.C, self.T, self.flags_mode = (customer_ring if n_customers else 0), (terminal_ring if n_terminals else 0), \
            flags_mode
        self.cust = [CustomerModel(customer_ring, self.win) for _ in range(n_customers)]
        self.term = [Terminal(terminal_ring, [self.delay] + [self.delay + w for w in self.win])
                     for _ in range(n_terminals)]
        self.counts = dict.fromkeys(OUTCOMES, 0)

    def update(self, ts, customer=None, amount=None, terminal=None, fraud=None):
        """-> [n, 4W]: (NB_w, AVG_w) x W of the customer half, (NB_w, RISK_w) x W of the terminal
        half (zeros for a half not fed); rows in (ts, row) order"""
        W = len(self.win)
        out = np.zeros((len(ts), 4 * W))
        for i in np.argsort(ts, kind="stable"):
            if customer is not None:
                nb, avg = self.cust[customer[i]].push(int(ts[i]), amount[i])
                out[i, 0:2 * W:2], out[i, 1:2 * W:2] = nb, avg
            if terminal is not None:
                nb, fr = self.term[terminal[i]].push(int(ts[i]), 0 if fraud is None else fraud[i])
                out[i, 2 * W::2] = nb
                out[i, 2 * W + 1::2] = [f / n if n > 0 else 0.0 for f, n in zip(fr, nb)]
        return out

    def report(self, ts, terminal):
        for i in np.argsort(ts, kind="stable"):
            if 0 <= terminal[i] < len(self.term):
                self.counts[self.term[terminal[i]].report(int(ts[i]))] += 1

    def snapshot(self, customers=None, terminals=None):
        pick = lambda keys, sel: keys if sel is None else [keys[sel[0] + j * sel[2]] for j in range(sel[1])]  # noqa: E731
        return encode({"window_ns": self.win, "delay_ns": self.delay, "flags_mode": self.flags_mode,
                       "customer_ring": self.C, "terminal_ring": self.T, "label_counts": self.counts,
                       "customers": [k.export() for k in pick(self.cust, customers)],
                       "terminals": [k.export() for k in pick(self.term, terminals)]})

    def restore(self, snap, customers_at=(0, 1), terminals_at=(0, 1), counters=True):
        d = decode(snap)
        assert d["window_ns"] == self.win and d["delay_ns"] == self.delay, "windows or delay differ"
        for keys, carried, (first, step) in ((self.cust, d["customers"], customers_at),
                                             (self.term, d["terminals"], terminals_at)):
            assert not carried or first + (len(carried) - 1) * step < len(keys), "key beyond the capacity"
            assert all(len(e) <= (k.C if hasattr(k, "C") else k.T) for (_, e), k in
                       zip(carried, keys[first::step])), "live rows exceed the ring"
            for j, (rec, ent) in enumerate(carried):
                keys[first + j * step].load(rec, ent)
        if counters:
            for k in OUTCOMES:
                self.counts[k] += d["label_counts"][k]

    @classmethod
    def from_snapshot(cls, snap, n_customers=None, n_terminals=None, customer_ring=None, terminal_ring=None):
        d = decode(snap)
        st = cls(len(d["customers"]) if n_customers is None else n_customers,
                 len(d["terminals"]) if n_terminals is None else n_terminals,
                 [w // DAY for w in d["window_ns"]], d["delay_ns"] // DAY, customer_ring or d["customer_ring"],
                 terminal_ring or d["terminal_ring"], d["flags_mode"])
        st.restore(snap)
        return st


# ---------------------------------------------------------- inputs shared by both test files
def cut_rows():
    """Where the tests stop and snapshot: inside the tie run, and the first row after day 45"""
    return [1050, int(np.searchsorted(R.table()["ts"], R.BASE + 45 * DAY, side="right"))]


@functools.lru_cache(maxsize=None)
def oracle_columns(windows, delay):
    """[n, 4W] over stream_label_ref.table(): (NB, AVG) x W customer columns, (NB, RISK) x W
    terminal columns, labels inline.  Treat as read-only."""
    c = R.table()
    f = oracle.featurize_arrays(c["ts"], c["customer"], c["terminal"], c["amount"], c["fraud"], windows, delay)
    cust = [f[f"CUSTOMER_ID_{k}_{w}DAY_WINDOW"] for w in windows for k in ("NB_TX", "AVG_AMOUNT")]
    return np.column_stack(cust + [R.term_cols(f, windows)]).astype(np.float64)


def feed(model, a, b):
    c = R.table()
    return model.update(c["ts"][a:b], c["customer"][a:b], c["amount"][a:b], c["terminal"][a:b], c["fraud"][a:b])


@functools.lru_cache(maxsize=None)
def model_prefix(windows, delay, cut):
    """-> (the model's features of rows [0, cut), its snapshot bytes), rings 256 / 256"""
    m = StateModel(25, 40, windows, delay, 256, 256)
    x = feed(m, 0, cut)
    return x, m.snapshot()
