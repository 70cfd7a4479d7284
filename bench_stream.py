"""Config 5 benchmark (BASELINE.json configs[4]): streaming micro-batches of 64k CDC
transactions -- incremental customer / terminal window state update + StandardScaler +
RandomForest(100, depth 20) predict_proba -- p50 / p99 batch latency.

Workload: the tail of config 4 (1M customers / 2M terminals, handbook distributions,
fdx.synth).  History: --history-days days streamed into the state first (day-sized batches,
untimed), so every ring holds a realistic 30 / 37-day window; then the next day is cut into
micro-batches of --batch transactions (global) and each is timed end to end:
  host batch (pinned) -> HBM -> fdx_stream_update (2 launches) -> forest -> proba -> host.
Also reported: the device-only time of the update + scoring (HIP events) and the rate.

N GPUs, one process per GPU (torch.distributed.run, or `--gpus N` alone: the script starts
the N ranks itself, bench.spawn_ranks): customers sharded by contiguous id
range, each micro-batch split by customer owner, terminals owned by id % N, one RCCL
all-to-all there and back per batch (fdx.streaming.ShardedStreamScorer); the batch latency
is the max over ranks.  Rank 0 prints one JSON line.

--fraud-reports: the rows arrive unlabelled, as from the CDC topic, and the labels as delayed
fraud reports before each batch (StreamScorer.report_frauds); the line gains the report call's
device time and the five report outcomes.

--snapshot: after the streamed day, the state's snapshot (StreamState.snapshot's C call) and its
restore into a second state of the same geometry are timed with HIP events, alternated with a
device-to-device copy of a buffer of the snapshot's size (the yardstick); the line gains a
"snapshot" object.  The default line is unchanged.

--late-terminals FRAC: a slow partition.  The customers whose id hashes below FRAC deliver the
streamed day's rows one micro-batch late, so every customer's rows stay in time order while the
terminals' do not; the scorer runs with terminal_lateness_days=1 (the late path of
k_stream_process) and the line gains a "late_terminals" object with the two late-row counters.
The default line is unchanged.

usage: python bench_stream.py [--gpus N] [--batches K] [--warmup W] [--fraud-reports] [--snapshot]
                              [--late-terminals FRAC]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "real-time_fraud_detection_system_amd"))


def cdc_encode(tx_id, customer, terminal, amount, ts_ns, kafka_ts, dup_frac=0.0, seed=0):
    """The Debezium wire columns of a batch of transactions, as the reference's sink receives
    them (pyspark/scripts/kafka_s3_sink_transactions.py:77-126): tx_amount DECIMAL(10,2) as
    big-endian two's-complement bytes of the cents (minimal length, as Kafka Connect encodes
    it), tx_datetime in microseconds, ids int64, a Kafka timestamp per record.  dup_frac adds,
    for that fraction of the records, a STALE update of the same tx_id (older Kafka timestamp,
    another amount) placed earlier or later in the batch -- the dedup (:180) must drop it.
    -> dict of numpy arrays (blob uint8 + offsets int64 [n' + 1]) with n' >= n records."""
    import numpy as np

    n = len(tx_id)
    cents = np.rint(np.asarray(amount, np.float64) * 100.0).astype(np.int64)
    rec = {"tx_id": np.asarray(tx_id, np.int64), "customer": np.asarray(customer, np.int64),
           "terminal": np.asarray(terminal, np.int64), "cents": cents,
           "us": np.asarray(ts_ns, np.int64) // 1000, "kts": np.asarray(kafka_ts, np.int64)}
    if dup_frac > 0 and n:
        rng = np.random.default_rng(seed)
        d = rng.choice(n, max(1, int(n * dup_frac)), replace=False)
        stale = {k: v[d].copy() for k, v in rec.items()}
        stale["cents"] = stale["cents"] + rng.integers(1, 10_000, len(d))
        stale["kts"] = stale["kts"] - rng.integers(1, 1000, len(d))
        pos = rng.integers(0, n + 1, len(d))      # insertion points in the batch
        order = np.argsort(np.r_[np.arange(n) * 2 + 1, pos * 2], kind="stable")
        rec = {k: np.r_[rec[k], stale[k]][order] for k in rec}
    c = rec["cents"]
    nbytes = np.maximum(1, (_bit_length(c) + 8) // 8)
    offsets = np.r_[0, np.cumsum(nbytes)].astype(np.int64)
    blob = np.zeros(int(offsets[-1]), np.uint8)
    u = c.astype(np.uint64)  # two's complement bits
    for k in range(8):  # byte k from the END of each record: (u >> 8k) & 0xFF
        m = nbytes > k
        blob[offsets[1:][m] - 1 - k] = ((u[m] >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint8)
    return {"tx_id": rec["tx_id"], "customer": rec["customer"], "terminal": rec["terminal"], "blob": blob,
            "offsets": offsets, "us": rec["us"], "kts": rec["kts"], "cents": c}


def _bit_length(c):
    """int.bit_length of the two's-complement magnitude: v >= 0 -> bits of v, v < 0 -> bits of ~v."""
    import numpy as np

    m = np.where(c < 0, ~c, c).astype(np.uint64)
    bl = np.zeros(len(m), np.int64)
    for s in range(63, -1, -1):
        hit = (bl == 0) & ((m >> np.uint64(s)) != 0)
        bl[hit] = s + 1
    return bl


def hold_back(cols, h, bounds, frac):
    """Reorder rows [h, n) of the columns `cols` (dict of numpy arrays in time order, changed in
    place) as they arrive when the customers whose id hashes below `frac` deliver one batch late:
    batch k = the held customers' rows of time slice k - 1, then the other customers' rows of
    slice k (slices = `bounds`), plus one closing batch with the last slice's held rows.  Every
    customer's rows stay in time order.  -> (new bounds, number of held rows)"""
    import numpy as np

    cust = cols["customer"][h:].astype(np.uint64)
    slow = ((cust * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) < np.uint64(int(frac * 2 ** 32))
    nb = len(bounds) - 1
    batch = np.clip(np.searchsorted(bounds, np.arange(h, h + len(cust)), side="right") - 1, 0, nb - 1)
    arrive = batch + slow
    perm = np.argsort(arrive, kind="stable")
    for k in cols:
        cols[k][h:] = cols[k][h:][perm]
    new = h + np.searchsorted(arrive[perm], np.arange(nb + 2))
    if new[-1] == new[-2]:
        new = new[:-1]
    return new, int(slow.sum())


RAW_ID_SCRAMBLE = {"customer": (0x9E3779B1, 1 << 41), "terminal": (0x85EBCA6B, 1 << 42)}  # (odd multiplier, offset)


def raw_id_scramble(ids, mult, offset):
    """--raw-ids: dense ids -> raw 64-bit ids, id * mult + offset in int64.  Injective (no
    wrap-around: 0 <= id < 2^31 and mult < 2^32 keep the product under 2^63) and above 2^40
    (offset), so nothing about the values is dense, sorted by arrival or fits int32."""
    import numpy as np

    ids = np.asarray(ids)
    if mult % 2 == 0 or not 0 < mult < 2 ** 32 or not 2 ** 40 < offset < 2 ** 62:
        raise ValueError("the scramble needs an odd 32-bit multiplier and an offset in (2^40, 2^62)")
    if ids.size and (ids.min() < 0 or ids.max() >= 2 ** 31):
        raise ValueError("ids must lie in [0, 2^31)")
    return ids.astype(np.int64) * np.int64(mult) + np.int64(offset)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--rehearse-one-gpu", action="store_true",
                    help="as bench.py: every rank on cuda:0, gloo, host-staged exchange collectives (not a measurement)")
    ap.add_argument("--customers", type=int, default=1_000_000)
    ap.add_argument("--terminals", type=int, default=2_000_000)
    ap.add_argument("--history-days", type=int, default=38)
    ap.add_argument("--batch", type=int, default=65536, help="global transactions per micro-batch")
    ap.add_argument("--batches", type=int, default=0, help="timed batches (0 = the whole streamed day)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed micro-batches before the timed ones")
    ap.add_argument("--customer-ring", type=int, default=256)
    ap.add_argument("--terminal-ring", type=int, default=256)
    ap.add_argument("--model", default=os.path.join(ROOT, "bench_assets", "rf100_d20.npz"))
    ap.add_argument("--column-copies", action="store_true",
                    help="a batch's 5 columns copied to the device one by one (default: one packed pinned buffer)")
    ap.add_argument("--no-graph", action="store_true",
                    help="enqueue each batch's kernels one by one (default at world 1: one HIP graph per batch "
                         "size, StreamScorer.score_graph, the probabilities' copy to the host inside it)")
    ap.add_argument("--cdc", action="store_true",
                    help="timed batches arrive as Debezium wire columns (decimal bytes, us timestamps, Kafka "
                         "timestamps, 2%% stale duplicate updates): device decode + dedup + compact + score "
                         "(StreamScorer.score_cdc; world 1)")
    ap.add_argument("--fraud-reports", action="store_true",
                    help="rows are fed unlabelled (fraud=None); before each batch the fraud reports due by then "
                         "(the generator's labels, 3 days after the transaction) go in through "
                         "StreamScorer.report_frauds, timed on their own (world 1, not with --cdc)")
    ap.add_argument("--snapshot", action="store_true",
                    help="after the streamed day: time the state's snapshot and its restore into a second state "
                         "against a device-to-device copy of the same size (world 1)")
    ap.add_argument("--snapshot-repeats", type=int, default=10)
    ap.add_argument("--late-terminals", type=float, default=0.0, metavar="FRAC",
                    help="the customers whose id hashes below FRAC deliver the streamed day's rows one micro-batch "
                         "late; the scorer runs with terminal_lateness_days=1 (world 1, not with --cdc or "
                         "--fraud-reports)")
    ap.add_argument("--raw-ids", action="store_true",
                    help="the same table with customer / terminal ids scrambled to raw 64-bit values "
                         "(raw_id_scramble) into a StreamScorer(raw_ids=True): the key directories map them "
                         "inside the batch's graph.  A dense scorer runs beside it up to the first timed "
                         "batch, whose probabilities must be bit-identical (raw_ids_match_dense)")
    ap.add_argument("--retire", type=float, default=0.0, metavar="SHARE",
                    help="with --raw-ids, after the streamed day: time StreamScorer.retire_idle at a watermark that "
                         "leaves SHARE of the customers idle (0 < SHARE < 1), the state re-created from a snapshot "
                         "for every repeat, against a device-to-device copy of the bytes the move touches")
    ap.add_argument("--retire-repeats", type=int, default=10)
    return ap.parse_args(argv)


def measure_snapshot(state, repeats=10):
    """Time fdx_stream_snapshot and fdx_stream_restore (into a second state of the same geometry)
    of `state` with HIP events, each alternated with a device-to-device copy of a buffer of the
    snapshot's size; one warm-up round, then `repeats`.  The calls synchronise inside (status and
    counts come to the host), so the event times are those of the whole call.  -> dict."""
    import numpy as np
    import torch

    from fdx import _lib, ops
    from fdx.streaming import StreamState, snapshot_info

    L = _lib.load()
    snap = state.snapshot()
    f = snapshot_info(snap)
    nbytes = snap.numel()
    second = StreamState(state.n_customers, state.n_terminals, state.windows_days, state.delay_days,
                         state.customer_ring, state.terminal_ring, 1, state.flags_mode)
    second.restore(snap, counters=False)
    if not torch.equal(second.snapshot(), snap):
        raise SystemExit("--snapshot: the restored state's snapshot differs from the source's")
    copy_dst = torch.empty_like(snap)
    ws = state._snap_ws()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    ms = {"snapshot": [], "restore": [], "copy": []}
    for i in range(repeats + 1):
        pairs = {k: (ev(), ev()) for k in ("snapshot", "copy_a", "restore", "copy_b")}
        pairs["snapshot"][0].record()
        _lib.check(L.fdx_stream_snapshot(state._h, None, None, ops._ptr(snap), nbytes, None, ops._ptr(ws), ws.numel(),
                                         ops._s()), "fdx_stream_snapshot")
        pairs["snapshot"][1].record()
        pairs["copy_a"][0].record()
        copy_dst.copy_(snap)
        pairs["copy_a"][1].record()
        pairs["restore"][0].record()
        second.restore(snap, counters=False)
        pairs["restore"][1].record()
        pairs["copy_b"][0].record()
        copy_dst.copy_(snap)
        pairs["copy_b"][1].record()
        torch.cuda.synchronize()
        if i:  # round 0 warms up
            ms["snapshot"].append(pairs["snapshot"][0].elapsed_time(pairs["snapshot"][1]))
            ms["restore"].append(pairs["restore"][0].elapsed_time(pairs["restore"][1]))
            ms["copy"] += [pairs[k][0].elapsed_time(pairs[k][1]) for k in ("copy_a", "copy_b")]
    W = f["n_windows"]
    rec = f["customer_keys"] * (2 + 6 * W) * 8 + f["terminal_keys"] * (4 + 2 * W) * 8
    ent = f["customer_entries"] * 16 + f["terminal_entries"] * 8
    off = (f["customer_keys"] + f["terminal_keys"] + 2) * 8
    keys4 = (f["customer_keys"] + f["terminal_keys"] + 2) * 4
    # from the header's counts.  snapshot: the count pass reads the records and writes + scans the
    # u32 counts, the pack reads records + counts + entries and writes records + offsets + entries;
    # restore: the validation reads records + offsets, the unpack reads all and writes records + entries
    moved = {"snapshot": rec + 3 * keys4 + (rec + keys4 + ent) + (rec + off + ent),
             "restore": (rec + off) + (rec + off + ent) + (rec + ent), "copy": 2 * nbytes}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"snapshot_bytes": nbytes, "customer_max_live": f["customer_max_live"],
            "terminal_max_live": f["terminal_max_live"], "customer_entries": f["customer_entries"],
            "terminal_entries": f["terminal_entries"], "repeats": repeats,
            "snapshot_ms": round(med["snapshot"], 3), "restore_ms": round(med["restore"], 3),
            "copy_ms": round(med["copy"], 3),
            "snapshot_ms_all": [round(v, 3) for v in ms["snapshot"]],
            "restore_ms_all": [round(v, 3) for v in ms["restore"]],
            "copy_ms_all": [round(v, 3) for v in ms["copy"]],
            "bytes_moved": moved,
            "gb_per_s": {k: round(moved[k] / (med[k] * 1e-3) / 1e9, 1) for k in moved},
            "snapshot_over_copy": round(med["snapshot"] / med["copy"], 2),
            "restore_over_copy": round(med["restore"] / med["copy"], 2),
            "unit": "ms (median HIP-event time of the whole call, host synchronisations inside included); "
                    "copy = device-to-device copy of snapshot_bytes, alternated with the calls"}


def measure_retire(sc, share, repeats=10):
    """Time StreamScorer.retire_idle on the scorer's state at a watermark that leaves `share` of the
    customers idle (the terminals' share follows from it), with HIP events around the whole call,
    alternated with a device-to-device copy of the bytes the in-place move touches (the records
    and rings of the keys that move); one warm-up round, then `repeats`.  A retirement mutates the
    state, so every round first puts back the snapshot and the keys taken once.  Then three
    rounds with events between the phases (plan, apply, the two directory rebuilds).  -> dict."""
    import numpy as np
    import torch

    from fdx.streaming import snapshot_info

    st = sc.state
    snap, keys = sc.snapshot(), sc.snapshot_keys()
    f = snapshot_info(snap)
    W = st.W
    rec = snap[f["section_offset"][0]:f["section_offset"][1]].view(torch.int64).view(-1, 2 + 6 * W)
    last = rec[rec[:, 0] > 0, 1]
    horizon = max(st.windows_days) * 86400 * 10 ** 9
    watermark = int(torch.sort(last).values[int(share * (last.numel() - 1))].item()) + horizon

    def put_back():
        st.restore(snap, counters=False)
        for d, k in ((sc.customers, "customers"), (sc.terminals, "terminals")):
            d.reset()
            d.load(keys[k])

    cmap, tmap, counts = st.retire_plan(watermark)
    key_bytes = ((2 + 6 * W) * 8 + st.customer_ring * 16, (4 + 2 * W) * 8 + st.terminal_ring * 8)
    moved_keys = []
    for m in (cmap, tmap):
        moves = (m >= 0) & (m != torch.arange(m.numel(), dtype=torch.int32, device=m.device))
        moved_keys.append(int(moves.sum().item()))
    touched = moved_keys[0] * key_bytes[0] + moved_keys[1] * key_bytes[1]
    src = torch.empty(max(touched, 1), dtype=torch.uint8, device=st.device)
    dst = torch.empty_like(src)
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    ms = {"retire": [], "copy": []}
    result = None
    for i in range(repeats + 1):
        put_back()
        e = [ev() for _ in range(4)]
        e[0].record()
        r = sc.retire_idle(watermark)
        e[1].record()
        e[2].record()
        dst.copy_(src)
        e[3].record()
        torch.cuda.synchronize()
        if result is None:
            result = r
        elif r != result:
            raise SystemExit("--retire: two rounds retired different keys")
        if i:  # round 0 warms up
            ms["retire"].append(e[0].elapsed_time(e[1]))
            ms["copy"].append(e[2].elapsed_time(e[3]))
    after = bytes(sc.snapshot()[:512].cpu().numpy())
    phases = {"plan": [], "apply": [], "remap_customers": [], "remap_terminals": []}
    for _ in range(3):
        put_back()
        e = [ev() for _ in range(5)]
        e[0].record()
        cm, tm, c = st.retire_plan(watermark)
        e[1].record()
        st.retire_apply(cm, c["customers"]["kept"], tm, c["terminals"]["kept"])
        e[2].record()
        sc.customers.remap(cm, c["customers"]["kept"])
        e[3].record()
        sc.terminals.remap(tm, c["terminals"]["kept"])
        e[4].record()
        torch.cuda.synchronize()
        for j, k in enumerate(phases):
            phases[k].append(e[j].elapsed_time(e[j + 1]))
    if bytes(sc.snapshot()[:512].cpu().numpy()) != after:
        raise SystemExit("--retire: the phase-by-phase rounds end in another snapshot header")
    med = {k: float(np.median(v)) for k, v in ms.items()}
    n_keys = {"customers": int(last.numel()), "terminals": counts["terminals"]["kept"] + counts["terminals"]["retired"]}
    return {"watermark_ns": watermark, "result": result,
            "idle_share": {k: round(result[k]["retired"] / max(n_keys[k], 1), 4) for k in n_keys},
            "keys_with_rows": n_keys, "moved_keys": {"customers": moved_keys[0], "terminals": moved_keys[1]},
            "key_bytes": {"customers": key_bytes[0], "terminals": key_bytes[1]}, "touched_bytes": touched,
            "repeats": repeats, "retire_ms": round(med["retire"], 3), "copy_ms": round(med["copy"], 3),
            "retire_over_copy": round(med["retire"] / med["copy"], 2),
            "retire_ms_all": [round(v, 3) for v in ms["retire"]], "copy_ms_all": [round(v, 3) for v in ms["copy"]],
            "gb_per_s": {"retire": round(2 * touched / (med["retire"] * 1e-3) / 1e9, 1),
                         "copy": round(2 * touched / (med["copy"] * 1e-3) / 1e9, 1)},
            "phase_ms": {k: round(float(np.median(v)), 3) for k, v in phases.items()},
            "unit": "ms (median HIP-event time of the whole retire_idle call, host synchronisations inside "
                    "included); copy = device-to-device copy of touched_bytes (records + whole rings of the keys "
                    "that move), alternated with the calls; the move itself reads and writes them twice (staged); "
                    "phase_ms: events between plan, apply and the two fdx_keydir_remap calls, three rounds"}


def rank_shard(args, world: int, rank: int):
    """configs[4]'s key state over the ranks: rank r owns the contiguous customer ids
    [r * n_c, (r + 1) * n_c) (n_c = customers // world) and all terminals (terminal t is owned
    by t % world for the exchange).  Returns (n_c, customer_base, n_terminals)."""
    n_c = args.customers // world
    return n_c, rank * n_c, args.terminals


def main():
    args = parse()
    if args.retire and (not args.raw_ids or not 0 < args.retire < 1):
        raise SystemExit("--retire SHARE needs --raw-ids and 0 < SHARE < 1")
    from bench import load_model, rehearse_host_collectives, spawn_ranks, stdout_to_stderr

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))  # one process per GPU, before this one touches the GPU
    json_out = stdout_to_stderr()
    import numpy as np
    import torch
    import torch.distributed as dist

    from fdx import ops, synth
    from fdx.streaming import ShardedStreamScorer, StreamScorer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if args.rehearse_one_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    cdev = torch.device("cpu") if args.rehearse_one_gpu else dev  # this script's own collectives
    if world > 1 and args.rehearse_one_gpu:
        dist.init_process_group("gloo")
        rehearse_host_collectives()
    elif world > 1:
        dist.init_process_group("nccl", device_id=dev)

    n_c, base, _ = rank_shard(args, world, rank)
    t_gen = time.perf_counter()
    # generated on the GPU (csrc/fdx_synth.hip), then copied to host: the micro-batches arrive
    # from pinned host memory, as CDC batches would
    # one population for every N (draws keyed by the global customer id): the union of the ranks'
    # rows is the same stream at every world size
    g = synth.generate_device(n_c, args.terminals, args.history_days + 1, seed=4321, customer_offset=base,
                              n_customers_total=n_c * world, device=dev)
    d = {k: g[k].cpu().numpy() for k in ("ts", "customer", "terminal", "amount", "fraud")}
    del g
    t_gen = time.perf_counter() - t_gen
    split = synth.START_NS + args.history_days * 86400 * synth.NS
    h = int(np.searchsorted(d["ts"], split))
    day_ns = 86400 * synth.NS

    arrays, mean, scale, check_X, check_proba = load_model(args.model)
    forest = ops.Forest(arrays, 15, mean, scale)
    T = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(dev, t)  # noqa: E731
    if not np.array_equal(forest.predict(T(check_X, torch.float64)).cpu().numpy(), check_proba):
        raise SystemExit("forest parity check against sklearn failed")

    # history batches: one per day (untimed); the state's batch capacity covers them
    day_cuts = np.searchsorted(d["ts"][:h], synth.START_NS + np.arange(args.history_days + 1) * day_ns)
    max_day = int(np.diff(day_cuts).max()) if h else 0
    per_rank = args.batch // world
    # common micro-batch time cuts: every per_rank-th timestamp of rank 0's streamed day
    s_ts = d["ts"][h:]
    if rank == 0:
        cuts = s_ts[::per_rank].astype(np.int64)
        cuts = np.r_[cuts, s_ts[-1] + 1] if len(s_ts) else np.array([split, split + 1])
        hdr = torch.tensor([len(cuts)], dtype=torch.int64, device=cdev)
    else:
        hdr = torch.zeros(1, dtype=torch.int64, device=cdev)
    if world > 1:
        dist.broadcast(hdr, 0)
    cut_t = torch.zeros(int(hdr.item()), dtype=torch.int64, device=cdev)
    if rank == 0:
        cut_t.copy_(torch.from_numpy(cuts))
    if world > 1:
        dist.broadcast(cut_t, 0)
    cuts = cut_t.cpu().numpy()
    bounds = np.searchsorted(s_ts, cuts) + h
    bounds[0], bounds[-1] = h, len(d["ts"])
    held = 0
    if args.late_terminals > 0:
        if world > 1 or args.cdc or args.fraud_reports:
            raise SystemExit("--late-terminals runs at world 1 without --cdc and --fraud-reports")
        bounds, held = hold_back(d, h, bounds, args.late_terminals)
    max_mb = int(np.diff(bounds).max())
    cap = max(max_day, max_mb, 1)
    dense_ids = None
    if args.raw_ids:
        if world > 1 or args.cdc or args.fraud_reports or args.late_terminals > 0:
            raise SystemExit("--raw-ids runs at world 1 without --cdc, --fraud-reports and --late-terminals")
        dense_ids = {k: d[k] for k in ("customer", "terminal")}
        for k in dense_ids:
            d[k] = raw_id_scramble(d[k], *RAW_ID_SCRAMBLE[k])

    wire = None
    if args.cdc:
        if world > 1:
            raise SystemExit("--cdc runs at world 1 (StreamScorer.score_cdc)")
        # the streamed day as CDC micro-batches, encoded up front (untimed): pinned host
        # buffers per batch, as a Kafka consumer would hold them
        kts = np.arange(len(d["ts"]), dtype=np.int64) * 10 + 1_739_000_000_000
        wire = []
        for k in range(len(bounds) - 1):
            a, b = int(bounds[k]), int(bounds[k + 1])
            r = cdc_encode(np.arange(a, b), d["customer"][a:b], d["terminal"][a:b], d["amount"][a:b], d["ts"][a:b],
                           kts[a:b], dup_frac=0.02, seed=k)
            wire.append({key: torch.from_numpy(np.ascontiguousarray(r[key] if len(r[key]) else np.zeros(1, r[key].dtype)))
                         .pin_memory() for key in ("tx_id", "customer", "terminal", "blob", "offsets", "us", "kts")})
        cap_w = max(int(w["tx_id"].numel()) for w in wire)
        cap = max(cap, cap_w)
        wdev = {key: torch.empty(max(int(w[key].numel()) for w in wire), dtype=wire[0][key].dtype, device=dev)
                for key in wire[0]}

    if world > 1:
        sc = ShardedStreamScorer(forest, world, rank, n_c, base, args.terminals, customer_ring=args.customer_ring,
                                 terminal_ring=args.terminal_ring, max_batch=cap, max_recv=cap * world * 2)
    else:
        sc = StreamScorer(forest, n_c, args.terminals, customer_ring=args.customer_ring,
                          terminal_ring=args.terminal_ring, max_batch=cap,
                          terminal_lateness_days=1 if args.late_terminals > 0 else 0, raw_ids=args.raw_ids)
    id_t, id_b = (torch.int64, 8) if args.raw_ids else (torch.int32, 4)
    row_b = 17 + 2 * id_b  # bytes per row of a packed batch
    cols = [("ts", torch.int64), ("customer", id_t), ("amount", torch.float64), ("terminal", id_t),
            ("fraud", torch.uint8)]
    # --raw-ids: the dense scorer the raw one is checked against, fed the original ids
    dense = StreamScorer(forest, n_c, args.terminals, customer_ring=args.customer_ring,
                         terminal_ring=args.terminal_ring, max_batch=cap) if args.raw_ids else None

    def dense_step(a, b):
        """the dense scorer over rows [a, b) (after run / one staged them) -> probabilities on the host"""
        ids = [T(dense_ids[k][a:b], torch.int32) for k in ("customer", "terminal")]
        p = dense.score(T(d["ts"][a:b], torch.int64), ids[0], T(d["amount"][a:b], torch.float64), ids[1],
                        T(d["fraud"][a:b], torch.uint8))
        return p.cpu().numpy().copy()
    reports = None
    if args.fraud_reports:
        if world > 1 or args.cdc:
            raise SystemExit("--fraud-reports runs at world 1 without --cdc (StreamScorer.report_frauds)")
        # a chargeback feed: every fraud of the generator, reported 3 days after the transaction
        # (inside the 7-day delay, so no report may come late); on the device up front, untimed
        f_idx = np.flatnonzero(d["fraud"])
        reports = {"due": d["ts"][f_idx] + 3 * day_ns, "ts": T(d["ts"][f_idx], torch.int64),
                   "terminal": T(d["terminal"][f_idx], torch.int32), "next": 0}

    def report_due(a, ev=None):
        """the reports due before the batch that starts at row a -> how many"""
        if a >= len(d["ts"]):
            return 0
        lo, hi = reports["next"], int(np.searchsorted(reports["due"], d["ts"][a], side="right"))
        reports["next"] = hi
        if ev is not None:
            ev[0].record()
        for o in range(lo, hi, cap):
            sc.report_frauds(reports["ts"][o:min(o + cap, hi)], reports["terminal"][o:min(o + cap, hi)])
        if ev is not None:
            ev[1].record()
        return hi - lo

    def labels(views):  # --fraud-reports: the batch's fraud column is not passed on
        return views[:4] + [None] if reports is not None else views
    # pinned host copies of the whole input (the "arriving" micro-batches are slices)
    pin = {k: torch.from_numpy(np.ascontiguousarray(d[k])).pin_memory() for k, _ in cols}
    dcols = {k: torch.empty(cap, dtype=t, device=dev) for k, t in cols}
    out_h = torch.empty(cap, dtype=torch.float64).pin_memory()

    def run_cdc(k, ev=None):
        w = wire[k]
        n = int(w["tx_id"].numel())
        for key, t in w.items():
            wdev[key][:t.numel()].copy_(t, non_blocking=True)
        if ev is not None:
            ev[0].record()
        p, rows = sc.score_cdc(wdev["tx_id"][:n], wdev["customer"][:n], wdev["terminal"][:n],
                               wdev["blob"][:int(w["blob"].numel())], wdev["offsets"][:n + 1], wdev["us"][:n],
                               wdev["kts"][:n])
        if ev is not None:
            ev[1].record()
        m = p.numel()
        out_h[:m].copy_(p, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return m

    # a streamed micro-batch arrives as ONE pinned host buffer holding its 5 columns back to back
    # (ts 8n | amount 8n | customer 4n | terminal 4n | fraud n bytes: every column aligned), as a
    # consumer would fill it -- one host-to-device copy instead of five (each copy costs ~9 us of
    # enqueue gap: 100 -> ~35 us per 64k batch, profiles/r06e trace); packed up front, untimed
    packed_cols = [("ts", torch.int64, 8), ("amount", torch.float64, 8), ("customer", id_t, id_b),
                   ("terminal", id_t, id_b), ("fraud", torch.uint8, 1)]
    dstage = torch.empty(row_b * cap, dtype=torch.uint8, device=dev)

    def pack(a, b):
        buf = torch.empty(row_b * (b - a), dtype=torch.uint8).pin_memory()
        o = 0
        for k, _, w in packed_cols:
            buf[o:o + w * (b - a)].copy_(pin[k][a:b].view(torch.uint8))
            o += w * (b - a)
        return buf

    def stage_views(n):
        views, o = {}, 0
        for key, t, w in packed_cols:
            views[key] = dstage[o:o + w * n].view(t)
            o += w * n
        return labels([views[key] for key, _ in cols])

    # one HIP graph per batch size (world 1): the batch's ~10 launches + the probabilities' copy
    # to the host as one graph launch; every size of the streamed day is captured before the
    # first timed batch (a consumer of fixed-size batches captures once)
    graph = world == 1 and not args.no_graph

    def run_packed(k, ev=None):
        buf = packed[k]
        n = buf.numel() // row_b
        dstage[:row_b * n].copy_(buf, non_blocking=True)
        if ev is not None:
            ev[0].record()
        if graph:
            sc.score_graph(*stage_views(n), out_host=out_h)
            if ev is not None:
                ev[1].record()
        else:
            p = sc.score(*stage_views(n))
            if ev is not None:
                ev[1].record()
            out_h[:n].copy_(p, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return n

    def run(a, b, ev=None):
        n = b - a
        for k, _ in cols:
            dcols[k][:n].copy_(pin[k][a:b], non_blocking=True)
        if ev is not None:
            ev[0].record()
        p = sc.score(*labels([dcols[k][:n] for k, _ in cols]))
        if ev is not None:
            ev[1].record()
        out_h[:n].copy_(p, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return n

    t_hist = time.perf_counter()
    for k in range(args.history_days):
        if reports is not None and day_cuts[k] < day_cuts[k + 1]:
            report_due(int(day_cuts[k]))
        run(int(day_cuts[k]), int(day_cuts[k + 1]))
        if dense is not None and day_cuts[k] < day_cuts[k + 1]:
            dense_step(int(day_cuts[k]), int(day_cuts[k + 1]))
    sc.state.check()
    t_hist = time.perf_counter() - t_hist

    nb = len(bounds) - 1
    n_warm = min(args.warmup, max(nb - 1, 0))
    n_timed = nb - n_warm if args.batches <= 0 else min(args.batches, nb - n_warm)
    packed = None
    if wire is None and not args.column_copies:
        packed = [pack(int(bounds[k]), int(bounds[k + 1])) for k in range(n_warm + n_timed)]
        if graph:
            for n in sorted({b.numel() // row_b for b in packed}):
                sc.score_graph(*stage_views(n), out_host=out_h, replay=False)
    one = (lambda k, ev=None: run_packed(k, ev)) if packed is not None else \
        (lambda k, ev=None: run(int(bounds[k]), int(bounds[k + 1]), ev))
    for k in range(n_warm):
        if reports is not None:
            report_due(int(bounds[k]))
        if wire is not None:
            run_cdc(k)
        else:
            one(k)
        if dense is not None:
            dense_step(int(bounds[k]), int(bounds[k + 1]))
    if world > 1:
        dist.barrier()
    lat, dev_ms, rows = [], [], 0
    rep_ms, n_rep = [], 0
    p_dense = None
    if dense is not None and n_timed:  # the first timed batch through the dense scorer, before the clock starts
        p_dense = dense_step(int(bounds[n_warm]), int(bounds[n_warm + 1]))
        dense.state.check()
        dense = None  # its state is not needed any more
    for k in range(n_warm, n_warm + n_timed):
        if reports is not None:  # before the batch, outside its latency: device time of the report call alone
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            n_rep += report_due(int(bounds[k]), ev)
            torch.cuda.current_stream().synchronize()
            rep_ms.append(ev[0].elapsed_time(ev[1]))
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        t0 = time.perf_counter()
        rows += run_cdc(k, ev) if wire is not None else one(k, ev)
        lat.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(ev[0].elapsed_time(ev[1]))
        if p_dense is not None and k == n_warm:
            if not np.array_equal(out_h[:len(p_dense)].numpy(), p_dense) or rows != len(p_dense):
                raise SystemExit("--raw-ids: the first timed batch's probabilities differ from the dense run's")
    sc.state.check()
    lat, dev_ms = np.array(lat), np.array(dev_ms)
    total_rows = rows
    if world > 1:
        t = torch.tensor(np.stack([lat, dev_ms]), dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        lat, dev_ms = t[0].cpu().numpy(), t[1].cpu().numpy()
        r = torch.tensor([rows], dtype=torch.int64, device=cdev)
        dist.all_reduce(r)
        total_rows = int(r.item())
    out = {
        "metric": "config 5: micro-batch latency, incremental window-state update + RF(100, d20) scoring",
        "value": round(float(np.percentile(lat, 50)), 3),
        "unit": "ms (p50 per micro-batch, host batch in -> probabilities on host)"
                + ("; batches as Debezium wire columns (decode + dedup + compact on the device)" if args.cdc else ""),
        "p99_ms": round(float(np.percentile(lat, 99)), 3),
        "max_ms": round(float(lat.max()), 3),
        "device_p50_ms": round(float(np.percentile(dev_ms, 50)), 3),
        "device_p99_ms": round(float(np.percentile(dev_ms, 99)), 3),
        "tx_per_s": round(total_rows / (lat.sum() * 1e-3), 1),
        "higher_is_better": False,
        "n_gpus": world,
        "batches": int(n_timed),
        "warmup": int(n_warm),
        "mean_batch_tx": round(total_rows / max(n_timed, 1), 1),
        "dtype": "f64",
        **({"rehearsal": "--rehearse-one-gpu: every rank on one GPU, host-staged gloo collectives; not a "
                         "measurement"} if args.rehearse_one_gpu else {}),
        "data": "synthetic: handbook-distribution generator on the GPU (fdx.synth.generate_device, seed 4321, draws keyed by the global customer id)",
        "config": {"workload": f"configs[4]: tail of configs[3] ({args.customers} customers / {args.terminals} "
                               f"terminals), {args.history_days} days of history in the state, then day "
                               f"{args.history_days} as micro-batches of {args.batch} tx",
                   "parallelism": f"customer-sharded x{world}, terminal owner = id % {world}",
                   "state_bytes_per_gpu": sc.state.memory_bytes,
                   "rings": [args.customer_ring, args.terminal_ring]},
        "setup_s": {"generate": round(t_gen, 1), "history_stream": round(t_hist, 1)},
        "launch": ("one HIP graph per batch (state update, row assembly, forest, status and probabilities "
                   "copies; device_p50 includes the probabilities' copy to the host)"
                   if packed is not None and graph else "kernels enqueued one by one"),
        "host_input": ("Debezium wire columns, one pinned buffer per column" if args.cdc else
                       "five pinned columns, one copy each" if packed is None else
                       "one pinned buffer per batch, the five columns back to back (one host-to-device copy)"),
    }
    if reports is not None:
        counts = sc.state.label_counts()
        if counts["late"]:
            raise SystemExit(f"--fraud-reports: {counts['late']} reports came late (lag 3 days, delay 7)")
        out.update({"report_p50_ms": round(float(np.percentile(rep_ms, 50)), 3),
                    "report_unit": "ms (p50 device time of the report_frauds call before each timed batch; "
                                   "beside device_p50_ms)",
                    "mean_batch_reports": round(n_rep / max(n_timed, 1), 1), **counts})
    if args.late_terminals > 0:
        out["late_terminals"] = {"fraction": args.late_terminals, "held_rows": held, "terminal_lateness_days": 1,
                                 **sc.state.late_counts(),
                                 "what": "the held customers' rows arrive one micro-batch late; value / device_p50_ms "
                                         "above are this run's (k_stream_process<W, true>)"}
    if args.raw_ids:
        kc = sc.key_counts()
        out["raw_ids"] = {"raw_ids_match_dense": p_dense is not None, "key_counts": kc,
                          "keydir_bytes": {"customers": sc.customers.memory_bytes,
                                           "terminals": sc.terminals.memory_bytes},
                          "what": "ids scrambled to 64-bit values (id * odd constant + offset > 2^40), mapped by the "
                                  "two key directories inside the batch's graph; value / device_p50_ms above are "
                                  "this run's"}
        out["raw_ids_match_dense"] = p_dense is not None
        if any(c["refused_full"] or c["refused_reserved"] or c["misses"] for c in kc.values()):
            raise SystemExit(f"--raw-ids: the directories refused rows: {kc}")
    if args.retire:
        out["retire"] = measure_retire(sc, args.retire, args.retire_repeats)
    if args.snapshot:
        if world > 1:
            raise SystemExit("--snapshot runs at world 1")
        out["snapshot"] = measure_snapshot(sc.state, args.snapshot_repeats)
    if rank == 0:
        print(json.dumps(out), file=json_out, flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
