"""Sklearn-layout forests for the forest tests (host only, no GPU): random ones, and forests
with an exact number of distinct thresholds per feature with the rows that sit on the edges of
the rank search tables those counts shape (threshold_forest, edge_rows, RANK_CASES)."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
SEARCHED = (0, 4, 6, 8)  # the features the row assembly ranks through S-trees (one sample per 4 thresholds)
SLOT_SPAN = 32767        # thresholds per rank-layout-v2 slot; the most one feature holds in v1 / v3


def random_forest(rng, n_trees, depth, n_feat=15, p_leaf=0.15):
    """Random sklearn-layout trees (pre-order, -1 leaves) for chunking / global-path tests."""
    L, R, F, TH, ML, V, off = [], [], [], [], [], [], [0]
    for _ in range(n_trees):
        left, right, feat, thr, ml, val = [], [], [], [], [], []

        def build(d):
            i = len(left)
            left.append(-1); right.append(-1); feat.append(-2); thr.append(-2.0); ml.append(0)
            val.append(float(rng.integers(0, 1000)) / 999.0)
            if d < depth and (d < 2 or rng.random() > p_leaf):
                feat[i] = int(rng.integers(0, n_feat)); thr[i] = float(rng.normal()) * 1.3
                ml[i] = int(rng.random() < 0.5)
                left[i] = build(d + 1)
                right[i] = build(d + 1)
            return i

        build(0)
        L += left; R += right; F += feat; TH += thr; ML += ml; V += val
        off.append(off[-1] + len(left))
    return dict(left=np.array(L, np.int64), right=np.array(R, np.int64), feature=np.array(F, np.int64),
                threshold=np.array(TH), missing_left=np.array(ML, np.uint8), value1=np.array(V),
                node_offsets=np.array(off, np.int64))


# ------------------------------------------------------------------ exact threshold counts
def _complete_tree(depth):
    """Pre-order template of a complete tree with `depth` levels of internal nodes: the children
    (-1 at leaves) and every node's position among the internal nodes / among the leaves in
    left-to-right (in-order) order, -1 where it is not one."""
    n = 2 ** (depth + 1) - 1
    left, right = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    ipos, lpos = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    idx, lo, llo = np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64)
    for h in range(depth, 0, -1):  # nodes whose subtree has h levels of internal nodes
        half = 2 ** (h - 1)        # leaves (and internal nodes + 1) of either child's subtree
        left[idx], right[idx], ipos[idx] = idx + 1, idx + 2 * half, lo + half - 1
        idx = np.concatenate([idx + 1, idx + 2 * half])
        lo, llo = np.concatenate([lo, lo + half]), np.concatenate([llo, llo + half])
    lpos[idx] = llo
    return left, right, ipos, lpos


def _pool(rng, c, candidates=None):
    """Exactly c distinct float32 values, sorted.  Without candidates: N(0, 1.3) draws, with 0.0
    among them from 8 values on.  With candidates (a table column): their distinct finite float32
    values below the largest (a subset that keeps the smallest when there are more than c), topped
    up with uniform draws between the smallest and the largest -- so the column's smallest value
    has rank 0 and its largest lies above every threshold, in the last segment."""
    if candidates is None:
        have, draw = np.zeros(0, np.float32), lambda m: rng.normal(0.0, 1.3, m)
    else:
        have = np.unique(np.asarray(candidates, np.float64).astype(np.float32))
        have = have[np.isfinite(have)]
        lo, hi = float(have[0]), float(have[-1]) if have[-1] > have[0] else float(have[0]) + 1.0
        have = have[have < hi] if len(have) > 1 else have
        draw = lambda m: rng.uniform(lo, hi, m)  # noqa: E731
    while len(have) < c:
        have = np.unique(np.concatenate([have, draw(2 * (c - len(have)) + 8).astype(np.float32)]))
        if candidates is not None:
            have = have[have < hi]  # (a draw the float32 cast rounded up to the largest)
    if len(have) > c:  # (the ends stay)
        mid = np.sort(rng.choice(len(have) - 2, max(c - 2, 0), replace=False)) + 1
        have = have[np.concatenate([[0], mid, [len(have) - 1]]).astype(np.int64)][:c] if c > 1 else have[:1]
    if candidates is None and c >= 8 and not (have == 0).any():
        have[np.argmin(np.abs(have))] = 0.0
        have = np.unique(have)
    assert len(have) == c and (np.diff(have) > 0).all()
    return have


def threshold_forest(counts, depth, rng, pools=None, n_mixed=2, inexact=0.1):
    """Complete depth-`depth` trees (sklearn pre-order) whose thresholds are, per feature f, exactly
    counts[f] distinct float32 values U_f, each used at least once.  Returns (arrays, [U_f]).

    Feature f gets ceil(counts[f] / (2^depth - 1)) trees that test f alone: a random partition of
    U_f (topped up with repeats), each part laid out as a search tree.  Such a tree's leaf tells
    between which two of its thresholds x_f lies whatever the other features are, so the rows U_f[k]
    and the next float32 above it always end in different leaves of the tree that holds U_f[k] --
    an off-by-one rank at any k changes the score.  n_mixed more trees draw feature and threshold
    at random (every feature in one walk).  Leaf values are distinct within a tree, grow from its
    leftmost leaf to its rightmost (so the trees that split the two rows of such a pair all move the
    score the same way) and are multiples of 2^-(depth+3), so a forest's sum is exact;
    missing_left is random; a fraction `inexact` of the
    thresholds are float64 values a quarter of the way to the next float32 (the library rounds them
    down, sklearn compares in double: the same split).  pools: {f: candidate values} -- U_f is
    drawn from them (see _pool); other features draw N(0, 1.3)."""
    left, right, ipos, lpos = _complete_tree(depth)
    nn, n_int, n_leaf = len(left), 2 ** depth - 1, 2 ** depth
    internal = left >= 0
    U = [_pool(rng, c, (pools or {}).get(f)) if c > 0 else np.zeros(0, np.float32) for f, c in enumerate(counts)]
    live = [f for f, u in enumerate(U) if len(u)]
    assert live, "a forest needs a threshold"
    feats, keys = [], []
    for f in live:
        m = -(-len(U[f]) // n_int)
        k = np.concatenate([rng.permutation(U[f]), rng.choice(U[f], m * n_int - len(U[f]))]).reshape(m, n_int)
        keys.append(np.sort(k, axis=1))
        feats += [f] * m
    nb, nt = len(feats), len(feats) + n_mixed
    feature = np.full((nt, nn), -2, np.int64)
    thr32 = np.zeros((nt, n_int), np.float32)
    feature[:nb, internal] = np.array(feats, np.int64)[:, None]
    thr32[:nb] = np.concatenate(keys)[:, ipos[internal]]
    if n_mixed:
        lens = np.array([len(U[f]) for f in live])
        allthr, first = np.concatenate([U[f] for f in live]), np.concatenate([[0], np.cumsum(lens)[:-1]])
        fi = rng.integers(0, len(live), (n_mixed, n_int))
        feature[nb:, internal] = np.array(live, np.int64)[fi]
        thr32[nb:] = allthr[first[fi] + (rng.random((n_mixed, n_int)) * lens[fi]).astype(np.int64)]
    thr = thr32.astype(np.float64)
    gap = np.nextafter(thr32, np.float32(np.inf)).astype(np.float64) - thr
    between = (rng.random(thr.shape) < inexact) & np.isfinite(gap)
    thr[between] += 0.25 * gap[between]
    threshold = np.full((nt, nn), -2.0)
    threshold[:, internal] = thr
    value1 = np.full((nt, nn), 0.5)
    # (increasing from the leftmost leaf to the rightmost, by random steps: going right at any node
    # of any tree raises that tree's value, so no two trees' changes can cancel)
    value1[:, ~internal] = (np.cumsum(rng.integers(1, 8, (nt, n_leaf)), axis=1) / (8.0 * n_leaf))[:, lpos[~internal]]
    ml = rng.integers(0, 2, (nt, nn)).astype(np.uint8)
    ml[:, ~internal] = 0
    arrays = dict(left=np.tile(left, nt), right=np.tile(right, nt), feature=feature.ravel(),
                  threshold=threshold.ravel(), missing_left=ml.ravel(), value1=value1.ravel(),
                  node_offsets=np.arange(nt + 1, dtype=np.int64) * nn)
    return arrays, U


def edge_ranks(c, seg, searched, rng, n_bound=40):
    """The threshold indices k of a feature with c thresholds whose neighbourhood a rank search
    over `seg`-float segments can get wrong (see edge_rows), sorted."""
    ks = {0, 1, c - 2, c - 1}
    ns = -(-c // seg)
    for j in {1, ns - 1} | set(rng.integers(1, max(ns, 2), n_bound).tolist()):  # segment boundaries
        ks |= {j * seg - 1, j * seg}
    if searched:  # the S-tree's samples: every 4th threshold; its nodes hold 8, its subtrees 9^p - 1
        n4 = -(-c // 4)
        for j in {1, n4 - 1, 8, 9, 80, 81, 728, 729, 6560, 6561} | set(rng.integers(1, max(n4, 2), n_bound).tolist()):
            ks |= {4 * j - 1, 4 * j}
    ks |= {SLOT_SPAN - 1, SLOT_SPAN, SLOT_SPAN + 1}  # the last rank of v1 / v3; v2's slot bases
    for j in range(1, c // SLOT_SPAN + 1):
        ks |= {j * SLOT_SPAN - 1, j * SLOT_SPAN, j * SLOT_SPAN + 1}
    return sorted(k for k in ks if 0 <= k < c)


def edge_rows(thresholds, seg, rng, n_rows=4096, searched=SEARCHED):
    """Rows that put one feature at an edge of its threshold table and fill the others at random.
    For every feature and every k of edge_ranks: U[k], the float32 just below and the one just
    above (three rows that differ in that feature only).  Per feature also +-inf, NaN, a NaN with
    the sign bit set, +-FLT_MAX, and +-0.0 where 0 is a threshold.  Random rows (normal draws and
    thresholds mixed) top the table up to n_rows.  Returns dict(X float64 [n, n_feat], pairs
    [m, 2] = the rows (at U[k], just above), pair_feature [m], pair_k [m])."""
    nf = len(thresholds)
    live = [f for f in range(nf) if len(thresholds[f])]

    def random_rows(m):
        X = rng.normal(0.0, 1.3, (m, nf)).astype(np.float32)
        for f in live:  # half of the values at a threshold
            at = rng.random(m) < 0.5
            X[at, f] = rng.choice(thresholds[f], int(at.sum()))
        return X.astype(np.float64)

    rows, pairs, pf, pk = [], [], [], []
    n = 0
    up, down = np.float32(np.inf), np.float32(-np.inf)
    for f in live:
        u = thresholds[f]
        ks = np.array(edge_ranks(len(u), seg, f in searched, rng), np.int64)
        base = random_rows(len(ks))
        X = np.repeat(base, 3, axis=0)
        X[0::3, f], X[1::3, f], X[2::3, f] = u[ks], np.nextafter(u[ks], down), np.nextafter(u[ks], up)
        rows.append(X)
        pairs.append(np.stack([n + 3 * np.arange(len(ks)), n + 3 * np.arange(len(ks)) + 2], axis=1))
        pf.append(np.full(len(ks), f))
        pk.append(ks)
        n += len(X)
    for f in range(nf):
        sp = [np.inf, -np.inf, np.nan, np.copysign(np.nan, -1.0), FLT_MAX, -FLT_MAX]
        if len(thresholds[f]) and (thresholds[f] == 0).any():
            sp += [0.0, -0.0]
        X = random_rows(len(sp))
        X[:, f] = sp
        rows.append(X)
        n += len(X)
    if n < n_rows:
        rows.append(random_rows(n_rows - n))
    return dict(X=np.concatenate(rows), pairs=np.concatenate(pairs), pair_feature=np.concatenate(pf),
                pair_k=np.concatenate(pk))


# ------------------------------------------------------------------ the rank-table regimes
def expected_tables(counts, v2_rows=False):
    """The search-table shape a 15-feature forest with these threshold counts must get, from the
    formats' rules: the smallest segment of 16, 32, 64 floats whose samples (one per segment and
    feature) fit the LDS table of the kernels that stage them -- 8,192 floats for the v1 row format,
    20,480 for v2 rows -- and, for the v1 row format, the S-trees of features 0, 4, 6, 8: one sample
    per 4 thresholds in a complete 9-ary tree (9^levels - 1 samples), dropped (0 floats) when the
    four exceed 28,672 floats."""
    seg = 16
    while sum(-(-c // seg) for c in counts) > (20480 if v2_rows else 8192):
        seg *= 2
    levels, floats = [0, 0, 0, 0], 0
    if not v2_rows:
        for s, f in enumerate(SEARCHED):
            while 9 ** levels[s] - 1 < -(-counts[f] // 4):
                levels[s] += 1
            floats += 9 ** levels[s] - 1
    return dict(seg=seg, n_samples=sum(-(-c // seg) for c in counts), n_tree_floats=floats if floats <= 28672 else 0,
                tree_levels=levels)


def _counts(*groups, rest=0):
    c = [rest] * 15
    for feats, n in groups:
        for f, m in zip(feats, n if isinstance(n, (tuple, list)) else [n] * len(feats)):
            c[f] = m
    return c


# name -> (threshold counts of the 15 features, the shape fdx_forest_rank_tables must report for the
# default layout: seg, samples, S-tree floats, S-tree levels).  The shapes are written out, not
# computed: test_forest_gen checks them against expected_tables, the GPU tests against the library.
RANK_CASES = {
    # s_smp[8192] of the v1-row kernels filled to its last float; one threshold more halves it
    "v1_full": (_counts((range(8), 16384)), (16, 8192, 19680, [4, 4, 4, 0])),
    "v1_full_no_trees": (_counts(((1, 2, 3, 5, 7, 9, 10, 11), 16384)), (16, 8192, 0, [0, 0, 0, 0])),
    "v1_one_more": (_counts((range(1, 8), 16384), ((0,), 16385)), (32, 4097, 19680, [4, 4, 4, 0])),
    # 8,411 samples at 32 floats: 64-float segments, with 4-level S-trees (6,500 <= 6,560 samples) ...
    "seg64_trees": (_counts((SEARCHED, 26000), rest=15000), (64, 4213, 26240, [4, 4, 4, 4])),
    # ... and with trees of 5 levels (7,500 samples), which are dropped: the two-level search ranks all
    "seg64_no_trees": (_counts(((0, 1, 2, 3, 4, 5, 6, 7, 8), 30000), (range(9, 15), 100)), (64, 4233, 0, [5, 5, 5, 5])),
    # S-tree levels: none, 1 (<= 32 thresholds), 2 (<= 320), 3 (<= 2,912), 4 (<= 26,240), 5 = dropped
    "levels_0122": (_counts((SEARCHED, (0, 32, 33, 320)), rest=50), (16, 69, 168, [0, 1, 2, 2])),
    "levels_2344": (_counts((SEARCHED, (320, 2912, 2916, 26240)), rest=50), (16, 2069, 13928, [2, 3, 4, 4])),
    "levels_3444": (_counts((SEARCHED, (324, 2916, 2920, 26240)), rest=50), (16, 2071, 20408, [3, 4, 4, 4])),
    "levels_3445": (_counts((SEARCHED, (324, 2916, 2920, 26241)), rest=50), (16, 2072, 0, [3, 4, 4, 5])),
    "levels_none": (_counts((SEARCHED, 0), rest=50), (16, 44, 0, [0, 0, 0, 0])),
    # the most thresholds a v1 / v3 feature holds (rank 32,767 against the leaf word), the first v2 forest
    "v1_limit": (_counts(((0,), 32767)), (16, 2048, 0, [5, 0, 0, 0])),
    "v2_first": (_counts(((0,), 32768)), (16, 2048, 0, [0, 0, 0, 0])),
    # s_smp[20480] of k_prepare_v2 filled to its last float (five features of three slots); one more
    "v2_full": (_counts(((0, 4, 6, 8, 10), 65536)), (16, 20480, 0, [0, 0, 0, 0])),
    "v2_one_more": (_counts(((4, 6, 8, 10), 65536), ((0,), 65537)), (32, 10241, 0, [0, 0, 0, 0])),
}
FUSED_CUSTOMERS, FUSED_TERMINALS = 300, 400


def rank_case(name, depth=11):
    """The forest, edge rows and fused-step table of RANK_CASES[name] (host only), as a dict:
    arrays / thresholds (threshold_forest), v2 (a feature needs more than one slot), tables
    (expected_tables), edge (edge_rows), data (a synthetic transaction table whose amounts are
    feature 0's edge values and thresholds) and table (its 15 feature columns from the oracle).
    Every feature's thresholds are drawn from the values its column takes in that table."""
    import zlib

    import oracle
    from fdx import synth

    counts, _ = RANK_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    v2 = max(counts) > SLOT_SPAN
    tables = expected_tables(counts, v2)
    d = synth.generate(n_customers=FUSED_CUSTOMERS, n_terminals=FUSED_TERMINALS, nb_days=20, seed=51)
    n = len(d["ts"])
    amount = d["amount"].astype(np.float32)
    pools = {}
    if counts[0]:  # amounts: feature 0's thresholds at the edges and their float32 neighbours, or any threshold
        u0 = pools[0] = _pool(rng, counts[0], amount)
        ks = np.array(edge_ranks(counts[0], tables["seg"], True, rng), np.int64)
        edges = np.concatenate([u0[ks], np.nextafter(u0[ks], np.float32(np.inf)),
                                np.nextafter(u0[ks], np.float32(-np.inf))])
        amount = np.where(rng.random(n) < 0.5, rng.permutation(np.resize(edges, n)), rng.choice(u0, n))
    d = dict(d, amount=amount.astype(np.float64))
    ref = oracle.featurize_arrays(d["ts"], d["customer"], d["terminal"], d["amount"], d["fraud"])
    names = ["TX_DURING_WEEKEND", "TX_DURING_NIGHT"] + oracle.CUSTOMER_COLS + oracle.TERMINAL_COLS
    table = np.column_stack([d["amount"]] + [ref[k] for k in names]).astype(np.float64)
    for f in range(1, 15):
        pools[f] = table[:, f]
    arrays, U = threshold_forest(counts, depth, rng, pools)
    return dict(name=name, counts=counts, v2=v2, tables=tables, arrays=arrays, thresholds=U,
                edge=edge_rows(U, tables["seg"], rng), data=d, table=table)


def table_edge_report(x, u, seg):
    """What the values x of one table column reach in the search over thresholds u: (rank 0 or the
    first segment, the last segment, both sides of one segment boundary -- the full count j * seg of
    a segment and the first count j * seg + 1 of the next)."""
    r = np.searchsorted(u, x.astype(np.float32), side="left")
    cs = np.searchsorted(u[::seg], x.astype(np.float32), side="left")  # samples < x: the segment read is cs - 1
    ns = -(-len(u) // seg)
    j = np.arange(1, ns)
    return bool((cs <= 1).any()), bool((cs == ns).any()), bool((np.isin(j * seg, r) & np.isin(j * seg + 1, r)).any())
