"""Plain references for the kernels of csrc/fdx_aux.hip:
the delay-aware train/test split, Card-Precision@k, the two segmented snapshot selections and
the Debezium decode / dedup / compact.  Host only: loops over numpy arrays, Python sets and
dicts, written from the documented behaviour (include/fdx.h), not from the kernels.

tests/test_aux_ref.py pins split_masks and card_precision to the reference project's own
functions through the fixtures oracle/gen_split_golden.py writes; the GPU tests then compare
the kernels with these functions on inputs the fixtures cannot hold (ties at the top-k cut,
where the reference's order is an accident of pandas' unstable sort and the project's rule is
"prediction descending, customer ascending").

edge_frame / edge_predictions are the seeded inputs the fixture split_cpk_edges.npz and the
GPU tests share.
"""
from decimal import Decimal

import numpy as np

NS_PER_DAY = 86_400 * 10 ** 9
INT32_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------ f-4: split, CP@k
def split_masks(ts_ns, day, cust, fraud, t_lo, delta_train, delta_delay, delta_test):
    """-> (train, test) bool masks.  train: t_lo <= ts < t_lo + delta_train days.  d0 = the
    smallest day among the train rows (none: both masks empty).  The known set starts as the
    customers with a fraud among the train rows; for d in range(delta_test) the customers with
    a fraud on day d0 + delta_train + d - 1 join it, then the rows of day
    d0 + delta_train + delta_delay + d whose customer is not known are test rows."""
    n = len(ts_ns)
    train = np.zeros(n, bool)
    test = np.zeros(n, bool)
    t_lo = int(t_lo)
    t_hi = t_lo + int(delta_train) * NS_PER_DAY
    for i in range(n):
        train[i] = t_lo <= int(ts_ns[i]) < t_hi
    if not train.any():
        return train, np.zeros(n, bool)
    d0 = min(int(day[i]) for i in range(n) if train[i])
    known = {int(cust[i]) for i in range(n) if train[i] and fraud[i]}
    rows_of_day = {}
    for i in range(n):
        rows_of_day.setdefault(int(day[i]), []).append(i)
    for d in range(int(delta_test)):
        for i in rows_of_day.get(d0 + delta_train + d - 1, ()):
            if fraud[i]:
                known.add(int(cust[i]))
        for i in rows_of_day.get(d0 + delta_train + delta_delay + d, ()):
            if int(cust[i]) not in known:
                test[i] = True
    return train, test


def _card_precision_days(day, cust, pred, fraud, top_k, remove):
    """One record per day, days ascending: (nb_compromised, hits, tied_at_cut, tie_sensitive)."""
    top_k = int(top_k)
    rows_of_day = {}
    for i in range(len(day)):
        rows_of_day.setdefault(int(day[i]), []).append(i)
    detected = set()
    out = []
    for d in sorted(rows_of_day):
        best, label = {}, {}
        for i in rows_of_day[d]:
            c = int(cust[i])
            if c in detected:
                continue
            p = float(pred[i]) + 0.0                     # -0.0 ranks as 0.0
            if c not in best or p > best[c]:
                best[c] = p
            label[c] = max(label.get(c, 0), int(fraud[i] != 0))
        order = sorted(best, key=lambda c: (-best[c], c))  # prediction desc, customer asc
        top = order[:top_k]
        hits = [c for c in top if label[c]]
        tied = len(order) > top_k and best[order[top_k - 1]] == best[order[top_k]]
        sensitive = False
        if tied:
            group = [label[c] for c in order if best[c] == best[order[top_k]]]
            sensitive = any(group) if remove else len(set(group)) > 1
        out.append((sum(label.values()), len(hits), tied, sensitive))
        if remove:
            detected.update(hits)
    return out


def card_precision(day, cust, pred, fraud, top_k, remove):
    """-> (nb_compromised_per_day, cp_per_day, mean, tie_sensitive_per_day), days ascending.
    Rows of already detected customers are dropped; per customer max(prediction), max(label);
    nb = customers with label 1; the first top_k in (prediction desc, customer asc) order, -0.0
    equal to 0.0, are taken: hits = those with label 1, cp = hits / top_k; with `remove` the
    hits join the detected set.  tie_sensitive[d]: the customers at ranks top_k - 1 and top_k
    have equal predictions and the group with that prediction holds two different labels
    (remove=False) or any label 1 (remove=True) -- an order among ties other than customer
    ascending could then change a result."""
    days = _card_precision_days(day, cust, pred, fraud, top_k, remove)
    nb = [r[0] for r in days]
    cp = [r[1] / int(top_k) for r in days]
    mean = float(np.array(cp).mean()) if cp else float("nan")
    return nb, cp, mean, [r[3] for r in days]


def tied_at_cut(day, cust, pred, fraud, top_k, remove):
    """Per day: the customers at ranks top_k - 1 and top_k have equal predictions (a tied group
    straddles the cut), whatever its labels."""
    return [r[2] for r in _card_precision_days(day, cust, pred, fraud, top_k, remove)]


# ------------------------------------------------------------------ f-1: segment selections
def segment_latest(ts, perm, seg_off):
    """Per segment [seg_off[k], seg_off[k + 1]): the first position holding the segment's
    maximum of ts[perm[pos]] (ts[pos] without a perm), returned as perm[pos] (pos without a
    perm); -1 for an empty segment."""
    out = []
    for k in range(len(seg_off) - 1):
        best, best_t = -1, None
        for p in range(int(seg_off[k]), int(seg_off[k + 1])):
            r = p if perm is None else int(perm[p])
            t = int(ts[r])
            if best_t is None or t > best_t:
                best, best_t = r, t
        out.append(best)
    return np.array(out, np.int32).reshape(-1)


def segment_first_in_range(ts, perm, seg_off, t_lo, t_hi):
    """Per segment: the first position with t_lo <= ts < t_hi, as perm[pos] (or pos); -1 if none."""
    out = []
    for k in range(len(seg_off) - 1):
        hit = -1
        for p in range(int(seg_off[k]), int(seg_off[k + 1])):
            r = p if perm is None else int(perm[p])
            if int(t_lo) <= int(ts[r]) < int(t_hi):
                hit = r
                break
        out.append(hit)
    return np.array(out, np.int32).reshape(-1)


# ------------------------------------------------------------------ f-2: CDC
def cdc_decode(list_of_bytes, us):
    """Debezium DECIMAL(10,2) bytes and microsecond timestamps of a batch.
    -> (unscaled int64, amount float64, ts_ns int64, bad bool); an entry is None where its
    input is None.  unscaled = int.from_bytes(b, "big", signed=True); amount =
    float(Decimal(unscaled) / 100); ts_ns = int(us / 1_000_000) * 10**9 with the division in
    double precision and truncation toward zero.  bad[i]: the field has 0 or more than 8
    bytes (its unscaled value and amount are then 0)."""
    uns = amt = bad = tsn = None
    if list_of_bytes is not None:
        uns, amt, bad = [], [], []
        for b in list_of_bytes:
            ok = 1 <= len(b) <= 8
            v = int.from_bytes(bytes(b), "big", signed=True) if ok else 0
            uns.append(v)
            amt.append(float(Decimal(v) / 100))
            bad.append(not ok)
        uns, amt, bad = np.array(uns, np.int64), np.array(amt, np.float64), np.array(bad, bool)
    if us is not None:
        tsn = np.array([int(float(int(u)) / 1_000_000.0) * 10 ** 9 for u in us], np.int64)
    return uns, amt, tsn, bad


def dedup_latest(key, kts):
    """Keep mask: per key the record with the largest kts; among equals the last in batch order."""
    last = {}
    for i in range(len(key)):
        j = last.get(int(key[i]))
        if j is None or int(kts[i]) >= int(kts[j]):
            last[int(key[i])] = i
    keep = np.zeros(len(key), bool)
    for i in last.values():
        keep[i] = True
    return keep


def cdc_compact(keep, cust, term, ts, amt, fraud):
    """The kept rows in batch order: -> dict(cust, term (int32; an id outside [0, 2^31) is -1),
    ts, amt, fraud (uint8 0/1; zeros without a fraud column), row_out (batch positions), count)."""
    rows = [i for i in range(len(keep)) if keep[i]]

    def narrow(v):
        return int(v) if 0 <= int(v) <= INT32_MAX else -1

    return dict(
        cust=np.array([narrow(cust[i]) for i in rows], np.int32).reshape(-1),
        term=np.array([narrow(term[i]) for i in rows], np.int32).reshape(-1),
        ts=np.array([int(ts[i]) for i in rows], np.int64).reshape(-1),
        amt=np.array([float(amt[i]) for i in rows], np.float64).reshape(-1),
        fraud=np.array([0 if fraud is None else int(fraud[i] != 0) for i in rows], np.uint8).reshape(-1),
        row_out=np.array(rows, np.int32).reshape(-1),
        count=len(rows))


# ------------------------------------------------------------------ shared seeded inputs
EDGE_SEED = 20240601
EDGE_BASE_NS = int(np.datetime64("2024-06-01T00:00:00", "ns").astype(np.int64))
EDGE_DAYS = 50
EDGE_DAY_OFFSET = 100            # TX_TIME_DAYS of the first calendar day: numbering not from 0
EDGE_REMOVED_DAYS = (16, 25, 33)  # calendar day indices without any row
EDGE_CUSTOMERS = 900
EDGE_HOT = 20
EDGE_TXID0 = 5000                # TRANSACTION_ID of the first row: ids are not positions
EDGE_GRID = 32                   # tie-heavy predictions: multiples of 1 / 32


def edge_frame(seed=EDGE_SEED):
    """-> dict of int64 columns TRANSACTION_ID, TX_DATETIME (ns), TX_TIME_DAYS, CUSTOMER_ID,
    TX_FRAUD, in time order.  50 calendar days from 2024-06-01 with three of them removed,
    TX_TIME_DAYS starting at 100, 900 customers with sparse ids (some negative), 20 hot
    customers with several rows and sometimes several frauds per customer-day, frauds about
    3 % of the rows and confined to a pool of customers (so that most customers are still
    present late in a Card-Precision run that removes the detected ones).  Rows sit exactly
    on the window edges the split cases use (00:00:00 and 10:30:00)."""
    rng = np.random.default_rng(seed)
    ids = np.cumsum(rng.integers(1, 6000, EDGE_CUSTOMERS)) - 40_000      # ascending, distinct
    order = rng.permutation(EDGE_CUSTOMERS)
    hot = order[:EDGE_HOT]
    pool = np.zeros(EDGE_CUSTOMERS, bool)
    pool[order[EDGE_HOT:EDGE_HOT + 120]] = True
    sec, cust, fraud = [], [], []
    for di in range(EDGE_DAYS):
        if di in EDGE_REMOVED_DAYS:
            continue
        m = 380 + int(rng.integers(-30, 31))
        s = rng.integers(0, 86_400, m)
        s[0], s[1] = 0, 37_800                       # rows exactly at 00:00:00 and 10:30:00
        c = rng.integers(0, EDGE_CUSTOMERS, m)
        f = (rng.random(m) < 0.15) & pool[c]
        sec.append(di * 86_400 + s)
        cust.append(c)
        fraud.append(f)
        for h in hot:
            if rng.random() < 0.5:
                continue
            r = int(rng.integers(3, 6))
            hf = np.zeros(r, bool)
            if rng.random() < 0.2:
                hf[rng.permutation(r)[:int(rng.integers(2, 4))]] = True
            sec.append(di * 86_400 + rng.integers(0, 86_400, r))
            cust.append(np.full(r, h))
            fraud.append(hf)
    sec, cust, fraud = np.concatenate(sec), np.concatenate(cust), np.concatenate(fraud)
    o = np.argsort(sec, kind="stable")
    sec, cust, fraud = sec[o].astype(np.int64), cust[o], fraud[o]
    return {
        "TRANSACTION_ID": np.arange(len(sec), dtype=np.int64) + EDGE_TXID0,
        "TX_DATETIME": EDGE_BASE_NS + sec * 10 ** 9,
        "TX_TIME_DAYS": sec // 86_400 + EDGE_DAY_OFFSET,
        "CUSTOMER_ID": ids[cust].astype(np.int64),
        "TX_FRAUD": fraud.astype(np.int64),
    }


def fixture_frame(g):
    """The columns edge_frame returned, and the float64 predictions, rebuilt from the narrow
    arrays of tests/golden/split_cpk_edges.npz."""
    sec = g["ts_s"].astype(np.int64)
    frame = {
        "TRANSACTION_ID": np.arange(len(sec), dtype=np.int64) + int(g["txid0"]),
        "TX_DATETIME": int(g["base_ns"]) + sec * 10 ** 9,
        "TX_TIME_DAYS": g["day"].astype(np.int64),
        "CUSTOMER_ID": g["cust_ids"].astype(np.int64)[g["cust_idx"]],
        "TX_FRAUD": g["fraud"].astype(np.int64),
    }
    return frame, g["pred"].astype(np.float64)


def edge_predictions(frame, seed=EDGE_SEED, tie_safe=True):
    """float64 predictions for edge_frame's rows on a grid of 32 values (0.0 included), so
    that nearly every customer is tied with others.  One row of each customer-day carries the
    customer's value, its other rows lower grid values.
    tie_safe=True: a customer-day holding a fraud takes a value between the grid points
      ((2 j + 1) / 16384, j distinct within the day), so every tied group has one label and no
      compromised customer is tied at all: no order among ties can change a result.
    tie_safe=False: every customer-day, with a fraud or not, draws from every fourth grid
      value, so a tied group holds some 40 customers and more than one compromised one on
      average: on most days the group at the cut mixes labels and only the rule (customer
      ascending) decides."""
    rng = np.random.default_rng(seed + (1 if tie_safe else 2))
    day, cust, fraud = frame["TX_TIME_DAYS"], frame["CUSTOMER_ID"], frame["TX_FRAUD"]
    groups = {}
    for i in range(len(day)):
        groups.setdefault((int(day[i]), int(cust[i])), []).append(i)
    pred = np.zeros(len(day), np.float64)
    used = {}
    for (d, _c), rows in sorted(groups.items()):
        has_fraud = any(fraud[i] for i in rows)
        if has_fraud and tie_safe:
            taken = used.setdefault(d, set())
            j = int(rng.integers(2048, 8192))
            while j in taken:
                j = int(rng.integers(2048, 8192))
            taken.add(j)
            v = (2 * j + 1) / 16384
        elif not tie_safe:
            v = 4 * int(rng.integers(0, EDGE_GRID // 4)) / EDGE_GRID
        else:
            v = int(rng.integers(0, EDGE_GRID)) / EDGE_GRID
        top = rows[int(rng.integers(0, len(rows)))]
        for i in rows:
            pred[i] = v if i == top else int(rng.integers(0, int(v * EDGE_GRID) + 1)) / EDGE_GRID
    return pred
