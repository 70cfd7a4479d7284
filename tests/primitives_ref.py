"""Plain numpy models and input builders for the sort / scan / key primitives of
csrc/fdx_rekey.hip and for the unfused scoring rows (host only, no GPU).

test_primitives_ref.py checks on the CPU that every builder reaches the regime it is named for;
test_gpu_primitives.py and test_gpu_unfused_rows.py run the kernels on these inputs and compare
with the references below.  Everything is exact: integers, or floats compared bit for bit.
Replaces the regrouping of pandas' groupby('CUSTOMER_ID') / sort_values / groupby('TERMINAL_ID')
(feature_transformation.ipynb:1092-1093, :2435-2436) and the feature matrix of input_features
(model_training.ipynb:457-463)."""
import numpy as np

from record_decode import unpack_term_records

TILE = 4096  # keys per radix tile, words per scan chunk
N_EDGE = [1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 7 * 4096 + 1, 8 * 4096, 8 * 4096 + 1, 17 * 4096 + 17]
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


# ------------------------------------------------------------------ the radix digit schedule
def digit_plan(bits):
    """(passes, leading 9-bit passes) of a `bits`-bit re-key: 8-bit digits, 9-bit ones only where
    they save a pass and then only as many as the key needs (csrc/fdx_rekey.hip:digit_plan)."""
    p8, p9 = -(-bits // 8), -(-bits // 9)
    passes = min(p8, p9)
    return passes, (max(0, bits - 8 * passes) if p9 < p8 else 0)


def digit_shifts(bits):
    """[(shift, digit bits)] of every pass: 9 * p for the 9-bit passes, then 9 * n9 + 8 * (p - n9)."""
    passes, n9 = digit_plan(bits)
    return [(9 * p, 9) if p < n9 else (9 * n9 + 8 * (p - n9), 8) for p in range(passes)]


# key widths test_gpu_parity.py reaches (n_keys 1, 256, 257, 50,000, 100,000, 2^18, 2^21, 2^25) and
# the ones test_gpu_primitives.py adds; together every plan of PLANS_1_TO_31
PARITY_KEY_BITS = [1, 8, 9, 16, 17, 18, 21, 25]
NEW_KEY_BITS = [10, 19, 24, 26, 27, 28, 31]
PLANS_1_TO_31 = {(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3), (4, 0)}


# ------------------------------------------------------------------ exclusive scan
SCAN_SIZES = N_EDGE + [TILE * 255 + 1, TILE * 256, TILE * 256 + 1, TILE * 513 + 7]
SCAN_KINDS = ["zero", "one", "u16", "u32"]


def scan_input(kind, m, rng):
    if kind == "zero":
        return np.zeros(m, np.uint32)
    if kind == "one":
        return np.ones(m, np.uint32)
    hi = 1 << 16 if kind == "u16" else 1 << 32
    return rng.integers(0, hi, m, dtype=np.uint64).astype(np.uint32)


def scan_ref(x):
    """Exclusive prefix sum modulo 2^32 (from a uint64 cumsum: exact below 2^32 words)."""
    c = np.cumsum(x.astype(np.uint64), dtype=np.uint64)
    return (np.concatenate([np.zeros(1, np.uint64), c[:-1]]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ------------------------------------------------------------------ 64-bit argsort / dense ids
ARGSORT_KINDS = (["full", "equal", "two", "sorted", "descending", "low32_equal", "high32_equal"] +
                 [f"byte{p}" for p in range(8)])


def argsort_keys(kind, n, rng):
    """int64 keys of one class.  byte<p>: d << 8p with d in 0..255 (many ties; p = 7 puts d's top
    bit on the sign), so pass p alone decides and the other seven must keep its order."""
    if kind == "full":
        k = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        sp = np.array([I64_MIN, I64_MAX, -1, 0, 1], np.int64)
        pos = rng.permutation(n)[:len(sp)]
        k[pos] = sp[:len(pos)]
        return k
    if kind == "equal":
        return np.full(n, 0x0123456789ABCDEF, np.int64)
    if kind == "two":
        return np.where(rng.random(n) < 0.5, np.int64(-3), np.int64(1 << 40))
    if kind == "sorted":
        return np.sort(rng.integers(-(1 << 62), 1 << 62, n, dtype=np.int64))
    if kind == "descending":
        return (np.int64(1) << 50) - np.arange(n, dtype=np.int64) * 1_000_003
    if kind == "low32_equal":
        return (rng.integers(-(1 << 31), 1 << 31, n, dtype=np.int64) << 32) | np.int64(0x9ABCDEF0)
    if kind == "high32_equal":
        return (np.int64(-0x12345678) << 32) | rng.integers(0, 1 << 32, n, dtype=np.int64)
    p = int(kind[4:])
    d = rng.integers(0, 256, n, dtype=np.uint64)
    return (d << np.uint64(8 * p)).view(np.int64)


DENSE_KINDS = ["equal", "distinct", "extremes", "tile_edge"]
DENSE_EDGE_POS = (4095, 4096, 4097)


def dense_keys(kind, n, rng):
    """int64 keys for fdx_dense_ids_i64.  tile_edge: in sorted order a new key first appears exactly
    at positions 4095, 4096 and 4097 (those below n), shuffled."""
    if kind == "equal":
        return np.full(n, -77, np.int64)
    if kind == "distinct":
        return rng.permutation(n).astype(np.int64) * 2_654_435_761 - (1 << 40)
    if kind == "extremes":
        return rng.choice(np.array([I64_MIN, I64_MAX, 0, 1, -1], np.int64), n)
    s = np.zeros(n, np.int64)
    for j, p in enumerate(DENSE_EDGE_POS):
        s[p:] = (j + 1) * 1_000_000_007
    return rng.permutation(s)


# ------------------------------------------------------------------ re-key
def rekey_keys(bits, n, rng):
    """Uniform int32 keys of [0, 2^bits), always with 0 and 2^bits - 1 (n = 1: the largest alone)."""
    k = rng.integers(0, 1 << bits, n, dtype=np.int64)
    k[-1] = (1 << bits) - 1
    if n > 1:
        k[n // 2] = 0
    return k.astype(np.int32)


def with_negative_ids(keys, rng, frac=0.1):
    """A copy of int32 keys with a tenth of them (at least one) negated to negative ids."""
    k = keys.copy()
    pos = rng.permutation(len(k))[:max(1, int(len(k) * frac))]
    k[pos] = -1 - k[pos]
    return k


# ------------------------------------------------------------------ segment offsets
SEG_SIZES = [1, 2, 3, 4, 5, 4099]
SEG_PATTERNS = ["first_gt0", "last_lt", "gap", "single", "one_key", "each_once"]
SEG_GAP = 10_000


def seg_pattern(name, n, rng):
    """(sorted int32 keys [n], n_keys) of one pattern of present / absent keys."""
    if name == "first_gt0":  # leading empty keys
        return np.sort(rng.integers(37, 300, n)).astype(np.int32), 300
    if name == "last_lt":    # trailing empty keys
        k = np.sort(rng.integers(0, 200, n))
        k[0] = 0
        return k.astype(np.int32), 5000
    if name == "gap":        # SEG_GAP absent keys in a row, inside when there are two rows
        k = np.sort(rng.integers(0, 50, n))
        k[(n + 1) // 2:] += 50 + SEG_GAP
        return k.astype(np.int32), 50 + SEG_GAP + 50 + 7
    if name == "single":
        return np.full(n, 123, np.int32), 1000
    if name == "one_key":
        return np.zeros(n, np.int32), 1
    return np.arange(n, dtype=np.int32), n


def seg_off_ref(sorted_keys, n_keys):
    """seg_off[q] = the first sorted position whose key is >= q, q in [0, n_keys]."""
    return np.searchsorted(np.asarray(sorted_keys, np.int64), np.arange(n_keys + 1), side="left").astype(np.int64)


def with_out_of_range_tail(sorted_keys, n_keys):
    """The keys followed by ids >= n_keys and then negative ids, where an unsigned sort puts them."""
    tail = np.array([n_keys, n_keys + 1, n_keys + 1, I32_MAX, I32_MIN, -5, -1, -1], np.int64).astype(np.int32)
    out = np.concatenate([sorted_keys, tail])
    assert (np.diff(out.view(np.uint32).astype(np.int64)) >= 0).all()
    return out


# ------------------------------------------------------------------ key histogram / range count
KEYSEG_N_KEYS = [1, 2, 4096, 4097, (1 << 20) + 1]
KEYSEG_N = 50_000


def keyseg_keys(n_keys, n, rng, bad=False):
    """int32 keys of [0, n_keys) with 0 and n_keys - 1; bad: INT32_MIN, -1, n_keys, INT32_MAX too."""
    k = rng.integers(0, n_keys, n).astype(np.int32)
    if n:
        k[0], k[-1] = n_keys - 1, 0
    if bad:
        pos = rng.permutation(np.arange(1, n - 1))[:40]
        k[pos] = np.resize(np.array([I32_MIN, -1, n_keys, I32_MAX], np.int64), 40).astype(np.int32)
    return k


OOR_SIZES = [0, 1, 63, 64, 65, 255, 257, 100_003]
OOR_N_KEYS = 1000
OOR_RANGES = [(0, OOR_N_KEYS), (-5, 5), (7, 7), (I32_MIN, I32_MAX), (1000, 2000)]
OOR_LAYOUTS = ["one_wave", "per_wave"]
WAVE = 64


def oor_keys(n, lo, hi, layout, rng):
    """(keys int32 [n], planted positions): keys inside [lo, hi) where that is not empty, with
    out-of-range ids planted in one wave (the last 64-aligned one) or one per wave of 64."""
    if hi > lo:
        k = rng.integers(lo, hi, n, dtype=np.int64)
    else:
        k = rng.integers(-50, 50, n, dtype=np.int64)
    outs = [v for v in (lo - 1, hi, I32_MIN, I32_MAX) if I32_MIN <= v <= I32_MAX and (v < lo or v >= hi)]
    if n == 0 or not outs:
        return k.astype(np.int32), np.zeros(0, np.int64)
    if layout == "one_wave":
        w0 = (n - 1) // WAVE * WAVE
        pos = np.arange(w0, n)[::2]
    else:
        w0 = np.arange(0, n, WAVE)
        pos = w0 + rng.integers(0, np.minimum(WAVE, n - w0))
    k[pos] = np.resize(np.array(outs, np.int64), len(pos))
    return k.astype(np.int32), pos


def oor_count(keys, lo, hi):
    k = keys.astype(np.int64)
    return int(np.count_nonzero((k < lo) | (k >= hi)))


# ------------------------------------------------------------------ the multi-GPU exchange records
def exchange_pack_ref(ts, term, fraud, perm):
    """rec [n, 2] int64: {ts[r], term[r] << 32 | (fraud[r] != 0) << 31 | r}, r = perm[j]."""
    r = perm.astype(np.int64)
    w = (term[r].astype(np.int64) << 32) | ((fraud[r] != 0).astype(np.int64) << 31) | r
    return np.stack([ts[r].astype(np.int64), w], axis=1)


def exchange_unpack_ref(rec, world):
    """(ts int64, owner-local terminal id int32 = term / world, fraud 0/1 uint8) of records [m, 2]."""
    w = rec[:, 1]
    return rec[:, 0].copy(), ((w >> 32) // world).astype(np.int32), ((w >> 31) & 1).astype(np.uint8)


def count_records(nb, fraud):
    """Count records [n, W] int64 (NB | FRAUD << 32) from counts [W, n]."""
    return (nb.astype(np.int64) | (fraud.astype(np.int64) << 32)).T.copy()


def reply_assemble_ref(X, rec, perm, col0):
    """X with X[perm[j], col0 + 2w] = NB_w and [.. + 1] = RISK_w of record j (the count-record decode
    of record_decode.unpack_term_records: IEEE FRAUD / NB, 0.0 where NB = 0)."""
    nb, risk = unpack_term_records(rec)
    out = X.copy()
    for w in range(rec.shape[1]):
        out[perm, col0 + 2 * w] = nb[w].astype(np.float64)
        out[perm, col0 + 2 * w + 1] = risk[w]
    return out


# ------------------------------------------------------------------ the unfused scoring rows
ROWS_N = 4099
NAN_FEATURES = (0, 4, 6, 8)  # amount and the customer averages: the columns that can hold NaN


def rows_case(W, rng, nan_variant=False, n=ROWS_N):
    """Grouped window outputs of n rows and W windows, and the feature matrix they assemble to.
    nb in 0..40; averages on a grid of cents, NaN where nb = 0; risk = k / nb (0.0 where nb = 0);
    amounts in cents.  nan_variant: a handful of NaN amounts and more NaN averages.  Terminal
    counts are drawn by row (tnb / tfr [W, n]) so that count records can be built in any order."""
    d = dict(n=n, W=W, nf=3 + 4 * W)
    d["amount"] = rng.integers(1, 40_000, n).astype(np.float64) / 100.0
    d["weekend"], d["night"] = (rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.4).astype(np.uint8)
    d["cust_perm"], d["term_perm"] = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    d["cust_nb"] = rng.integers(0, 41, (W, n)).astype(np.int32)
    avg = rng.integers(1, 40_000, (W, n)).astype(np.float64) / 100.0
    avg[d["cust_nb"] == 0] = np.nan
    if nan_variant:
        d["amount"][rng.permutation(n)[:9]] = np.nan
        avg[rng.random((W, n)) < 0.02] = np.nan
    d["cust_avg"] = avg
    d["tnb"] = rng.integers(0, 41, (W, n)).astype(np.int32)
    d["tnb"][:, rng.permutation(n)[:50]] = 0  # rows whose every window is empty
    d["tfr"] = (rng.random((W, n)) * (d["tnb"] + 1)).astype(np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        risk_row = np.where(d["tnb"] > 0, d["tfr"].astype(np.float64) / np.maximum(d["tnb"], 1), 0.0)
    d["term_nb"] = np.ascontiguousarray(d["tnb"][:, d["term_perm"]])
    d["term_risk"] = np.ascontiguousarray(risk_row[:, d["term_perm"]])
    X = np.empty((n, d["nf"]))
    X[:, 0], X[:, 1], X[:, 2] = d["amount"], d["weekend"], d["night"]
    for w in range(W):
        X[d["cust_perm"], 3 + 2 * w] = d["cust_nb"][w]
        X[d["cust_perm"], 4 + 2 * w] = d["cust_avg"][w]
        X[d["term_perm"], 3 + 2 * W + 2 * w] = d["term_nb"][w]
        X[d["term_perm"], 4 + 2 * W + 2 * w] = d["term_risk"][w]
    d["X"] = X
    return d


def rows_scaler(nf, rng):
    """(mean, scale): no power of two among the scales, so the division rounds."""
    return rng.uniform(-3.0, 30.0, nf), rng.uniform(0.3, 9.7, nf) * 1.1


def rows_forest(case, rng, mean=None, scale=None, n_trees=8, depth=6):
    """forest_gen.random_forest over the case's features with every threshold drawn from the values
    its column takes (scaled as the forest scales them), half of them rounded to float32 -- a row
    at the threshold then ties exactly -- and missing_go_to_left 0 and 1 mixed (random_forest draws
    it per node)."""
    from forest_gen import random_forest

    arr = random_forest(rng, n_trees, depth, n_feat=case["nf"])
    X = case["X"]
    for i in np.flatnonzero(arr["left"] >= 0):
        f = int(arr["feature"][i])
        col = X[:, f]
        v = float(rng.choice(col[np.isfinite(col)]))
        if mean is not None:
            v = (v - mean[f]) / scale[f]
        arr["threshold"][i] = float(np.float32(v)) if rng.random() < 0.5 else v
    return arr


def nan_split_nodes(arr, features=NAN_FEATURES):
    """Internal nodes that split on one of `features`, and their missing_go_to_left."""
    m = (arr["left"] >= 0) & np.isin(arr["feature"], features)
    return np.flatnonzero(m), arr["missing_left"][m]
