"""Reuse distance of the row assembly's terminal-record gather, on the host (tools only; numpy and
fdx.synth.generate, no GPU).

The count records are written by input row (time order), 16 bytes each, so a 128-byte line holds 8
rows that are neighbours in time; the assembly reads them by customer slot (the interleaved layout
of DESIGN §3: customers by decreasing length in groups of 21, slot (t, l) of a group = its t-th row
of customer l).  For every gather this prints the share whose line was last touched fewer than d
slots earlier in the processing sequence, d as a share of all slots, for the linear slot sweep and
for granules of G slots visited in the order of the smallest timestamp they hold -- the order a
time-sorted assembly would take.  (DESIGN §8 has what the GPU made of it: the Infinity Cache did
not turn the shorter distances into time.)

    python tools/record_reuse_sim.py [--customers 5000 --terminals 10000 --days 183 --seed 1234]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time_fraud_detection_system_amd"))

S = 21  # customers per group (64 lanes // 3 windows)
SHARES = (0.015, 0.03, 0.05, 0.10)


def layout(customer, n_customers):
    """slot -> input row (-1: padding) of the interleaved layout; input rows are in time order"""
    order = np.argsort(customer, kind="stable")  # rows by customer, time order inside
    lens = np.bincount(customer, minlength=n_customers)
    seg = np.r_[0, np.cumsum(lens)]
    sorder = np.argsort(65535 - np.minimum(lens, 65535), kind="stable")
    parts = []
    for g0 in range(0, n_customers, S):
        cs = sorder[g0:g0 + S]
        Lg = int(lens[cs[0]])
        blk = np.full((Lg, S), -1, np.int64)
        for l, c in enumerate(cs):
            blk[:lens[c], l] = order[seg[c]:seg[c + 1]]
        parts.append(blk.reshape(-1))
    return np.concatenate(parts) if parts else np.zeros(0, np.int64)


def sequence(irow, ts, granule):
    """the slots in processing order: linear (granule None) or granules by their smallest live ts"""
    n = len(irow)
    if granule is None:
        return np.arange(n)
    ng = -(-n // granule)
    t = np.where(irow >= 0, ts[np.maximum(irow, 0)], np.iinfo(np.int64).max)
    t = np.r_[t, np.full(ng * granule - n, np.iinfo(np.int64).max)].reshape(ng, granule)
    gorder = np.argsort(t.min(axis=1), kind="stable")
    seq = (gorder[:, None] * granule + np.arange(granule)[None, :]).reshape(-1)
    return seq[seq < n]


def reuse_shares(irow, seq, per_line):
    """per gather (live slot): share with the line's previous touch < d slots back, d in SHARES of all slots"""
    n = len(irow)
    pos = np.empty(n, np.int64)
    pos[seq] = np.arange(n)
    live = irow >= 0
    line, p = irow[live] // per_line, pos[live]
    o = np.lexsort((p, line))
    line, p = line[o], p[o]
    d = np.full(len(p), np.iinfo(np.int64).max)
    same = line[1:] == line[:-1]
    d[1:][same] = (p[1:] - p[:-1])[same]
    return [float((d < s * n).mean()) for s in SHARES]


def table(customers, terminals, days, seed, granules=(64, 256, 1024), per_lines=(8, 16)):
    from fdx import synth

    g = synth.generate(customers, terminals, days, seed=seed)
    irow = layout(g["customer"], customers)
    out = {}
    for per_line in per_lines:
        out[(per_line, "linear", None)] = reuse_shares(irow, sequence(irow, g["ts"], None), per_line)
        for G in granules:
            out[(per_line, "by tile time", G)] = reuse_shares(irow, sequence(irow, g["ts"], G), per_line)
    return out, len(irow), len(g["ts"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--customers", type=int, default=5000)
    ap.add_argument("--terminals", type=int, default=10000)
    ap.add_argument("--days", type=int, default=183)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    res, n_slots, n = table(a.customers, a.terminals, a.days, a.seed)
    print(f"{n} rows in {n_slots} slots; share of gathers whose line was touched < d slots earlier")
    print("| records per line | tile order | granule | " + " | ".join(f"d < {100 * s:g} %" for s in SHARES) + " |")
    print("|---|---|---|" + "---|" * len(SHARES))
    for (per_line, name, G), v in res.items():
        print(f"| {per_line} | {name} | {G or '-'} | " + " | ".join(f"{x:.2f}" for x in v) + " |")
    print("(the most possible is 1 - 1 / records per line: a line's first touch always misses)")


if __name__ == "__main__":
    main()
