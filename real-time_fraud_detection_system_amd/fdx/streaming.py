"""BASELINE.json config 5: streaming micro-batches with incremental window state + scoring.

The reference's streaming job (pyspark/scripts/fraud_detection.py:88-201) reads Debezium
micro-batches from Kafka, LEFT JOINs them against feature snapshot tables written by the
batch notebooks, scales and scores them in a pandas UDF.  Config 5 asks for the real-time
version of that: each micro-batch updates the customer / terminal window state and is
scored on fresh features.  The state lives in HBM (csrc/fdx_stream.hip) and is exactly the
batch recurrences' state at each key's last row, so streaming a history batch by batch gives
the same 15 features, bit for bit, as the batch path over the whole history
(get_customer_spending_behaviour_features feature_transformation.ipynb:601-628,
get_count_risk_rolling_window :1495-1522, tests/test_gpu_stream.py).

That identity is over the TX_FRAUD labels, and no live caller has a row's label when it
scores the row: the reference's Postgres table and Debezium topic carry no TX_FRAUD, fraud
is confirmed days later (which is why the terminal windows are delayed, :1495-1522).  Rows
are therefore fed unlabelled (fraud=None; score_cdc feeds zeros) and the labels arrive through
report_frauds, which sets them in the terminal state as if known all along; reports that
arrive within the delay keep the stream bit-identical to the batch path over the true labels
(tests/test_gpu_stream_labels.py).

  StreamState          device state + fdx_stream_update (features of a batch) +
                       fdx_stream_report_frauds (delayed labels)
  KeyDirectory         device hash table raw int64 id -> dense state row (fdx_keydir_*), for
                       streams whose ids are not 0..n-1 (StreamScorer(raw_ids=True));
                       StreamScorer.retire_idle drops the keys idle for a whole horizon, so
                       their ids and state rows are reused (fdx_stream_retire_*, fdx_keydir_remap)
  StreamScorer         StreamState + the forest (scale + predict_proba) per batch
  ShardedStreamScorer  one process per GPU: customers sharded by id range, terminals owned
                       by id % world, one RCCL all-to-all there and back per batch (the
                       exchange of fdx.distributed, with the owner running its incremental
                       terminal state instead of the batch windows)
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ops
from ._lib import FdxError, FdxUnsupported, check

_STATUS = {1: "customer ring overflow (raise customer_ring)", 2: "terminal ring overflow (raise terminal_ring)",
           4: "customer or terminal id outside the state's capacity", 8: "a key's rows went back in time",
           16: "a late terminal row reaches past the ring (raise terminal_ring)"}
LABEL_OUTCOMES = ("on_time", "late", "duplicate", "expired", "unmatched")  # fdx_stream_label_counts
LATE_COUNTS = ("late_rows", "late_past_delay")  # fdx_stream_late_counts
KEY_COUNTS = ("held", "refused_full", "refused_reserved", "misses")  # fdx_keydir_counts


def _as_bytes_tensor(snap) -> torch.Tensor:
    """A snapshot given as a tensor, a numpy array or bytes -> a flat uint8 tensor (where it lives)."""
    if isinstance(snap, torch.Tensor):
        t = snap
    elif isinstance(snap, (bytes, bytearray, memoryview)):
        t = torch.frombuffer(bytearray(snap), dtype=torch.uint8)
    else:  # numpy
        import numpy as np

        t = torch.from_numpy(np.ascontiguousarray(snap).view(np.uint8).reshape(-1).copy())
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise FdxError("a snapshot is a contiguous uint8 buffer")
    return t.reshape(-1)


def _to_device_bytes(snap, device) -> torch.Tensor:
    t = _as_bytes_tensor(snap)
    return t if t.device.type == "cuda" else t.to(device)


def snapshot_info(snap) -> dict:
    """The checked header of a snapshot (device or host tensor, numpy array or bytes) as a dict:
    version, total_bytes, window_ns, delay_ns, flags_mode, the source's customer_ring /
    terminal_ring, per half keys / entries / max_live (the largest live row count of a key: a
    ring must hold at least that), label_counts, section_offset.  Raises FdxError on anything
    that is not a well-formed version-1 header."""
    t = _as_bytes_tensor(snap)
    head = bytes(t[:_lib.FDX_SNAPSHOT_HEADER_BYTES].cpu().numpy())
    f = _lib.SnapshotInfo()
    check(_lib.load().fdx_stream_snapshot_info(head, t.numel(), ctypes.byref(f)), "fdx_stream_snapshot_info")
    d = {k: int(getattr(f, k)) for k, _ in _lib.SnapshotInfo._fields_ if k not in ("window_ns", "label_counts",
                                                                                     "section_offset")}
    d["window_ns"] = [int(w) for w in f.window_ns[:d["n_windows"]]]
    d["label_counts"] = dict(zip(LABEL_OUTCOMES, (int(v) for v in f.label_counts)))
    d["section_offset"] = [int(v) for v in f.section_offset]
    return d


def save_snapshot(path, snap) -> None:
    """The snapshot's raw bytes to a file (no pickle)."""
    _as_bytes_tensor(snap).cpu().numpy().tofile(path)


def load_snapshot(path) -> torch.Tensor:
    """-> the file's bytes as a pinned host uint8 tensor (StreamState.restore / from_snapshot take it)."""
    import numpy as np

    a = np.fromfile(path, dtype=np.uint8)
    t = torch.empty(a.size, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    t.numpy()[:] = a
    return t


def save_keys(path, d) -> None:
    """StreamScorer.snapshot_keys()'s dict to a file: an .npz of plain little-endian int64 arrays
    (no pickle).  It travels beside the state snapshot (save_snapshot), whose format it leaves alone."""
    import numpy as np

    with open(path, "wb") as f:
        np.savez(f, **{k: v.cpu().numpy().astype("<i8", copy=False) for k, v in d.items()})


def load_keys(path) -> dict:
    """-> {"customers": int64 tensor, "terminals": int64 tensor} on the host (restore_keys takes it)."""
    import numpy as np

    with np.load(path, allow_pickle=False) as z:
        return {k: torch.from_numpy(z[k].astype(np.int64)) for k in z.files}


class KeyDirectory:
    """Raw int64 keys -> dense int32 ids on the current GPU (include/fdx.h, f-9): a new key gets
    the next free id, new keys of a batch in the order of their first occurrence, so over a
    stream the ids are pandas.factorize of the keys in arrival order.  INT64_MIN is reserved."""

    def __init__(self, capacity: int, max_batch: int = 65536, stream=None):
        self.device = ops.require_gpu()
        self.capacity, self.max_batch = int(capacity), int(max_batch)
        h = ctypes.c_void_p()
        check(_lib.load().fdx_keydir_create(self.capacity, self.max_batch, ctypes.byref(h), ops._s(stream)),
              "fdx_keydir_create")
        self._h = h
        b = ctypes.c_size_t()
        check(_lib.load().fdx_keydir_memory(h, ctypes.byref(b)), "fdx_keydir_memory")
        self.memory_bytes = b.value

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib._lib.fdx_keydir_destroy(h)
            self._h = None

    def reset(self, stream=None):
        check(_lib.load().fdx_keydir_reset(self._h, ops._s(stream)), "fdx_keydir_reset")

    def map(self, keys, insert: bool = True, out=None, stream=None) -> torch.Tensor:
        """-> int32 ids of the int64 device tensor `keys` (at most max_batch rows), stream-ordered,
        no host read.  insert: new keys get ids; else lookup only.  -1: the row was refused (the
        directory is full, the reserved key) or, without insert, not held; counts() tells which."""
        ops._dev(keys, torch.int64, "keys")
        n = keys.numel()
        if n > self.max_batch:
            raise FdxError(f"batch of {n} keys > max_batch {self.max_batch}")
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=keys.device)
        ops._dev(out, torch.int32, "out")
        if out.numel() != n:
            raise FdxError(f"out has {out.numel()} rows, keys has {n}")
        check(_lib.load().fdx_keydir_map(self._h, ops._ptr(keys), n, _lib.FDX_KEYDIR_INSERT if insert else 0,
                                         ops._ptr(out), ops._s(stream)), "fdx_keydir_map")
        return out

    def counts(self, stream=None) -> dict:
        """Synchronise; -> {held, refused_full, refused_reserved, misses}: keys held now, rows
        refused / missed since create / reset."""
        c = (ctypes.c_int64 * len(KEY_COUNTS))()
        check(_lib.load().fdx_keydir_counts(self._h, c, ops._s(stream)), "fdx_keydir_counts")
        return dict(zip(KEY_COUNTS, (int(v) for v in c)))

    def keys(self, stream=None) -> torch.Tensor:
        """Synchronise; -> the keys held as a device int64 tensor, keys()[id] = key."""
        out = torch.empty(self.counts(stream)["held"], dtype=torch.int64, device=self.device)
        n = ctypes.c_int64()
        check(_lib.load().fdx_keydir_keys(self._h, ops._ptr(out), out.numel(), ctypes.byref(n), ops._s(stream)),
              "fdx_keydir_keys")
        return out[:n.value]

    def load(self, keys, stream=None):
        """Into the EMPTY directory: keys[i] gets id i (int64 tensor, device or host).  More keys
        than the capacity, a duplicate or the reserved key raises and the directory stays empty."""
        k = keys.to(self.device).contiguous()
        ops._dev(k, torch.int64, "keys")
        check(_lib.load().fdx_keydir_load(self._h, ops._ptr(k), k.numel(), ops._s(stream)), "fdx_keydir_load")

    def remap(self, id_map, kept: int, stream=None):
        """After a retirement (f-10): id_map[id] = the key's new id or -1 (int32 device tensor over
        at least the keys held; StreamState.retire_plan makes it), kept = the survivors.  key_of
        is compacted, the table cleared and refilled, so the retired keys' ids and slots -- and
        refused keys left in the table -- are free again; the refusal counters keep their values.
        A malformed map or a wrong kept raises with nothing written.  Addresses do not move.
        Synchronises (a cold path)."""
        ops._dev(id_map, torch.int32, "id_map")
        L = _lib.load()
        ws = getattr(self, "_remap_ws", None)
        if ws is None:
            ws = self._remap_ws = ops.workspace(L.fdx_keydir_remap_workspace_size(self._h), self.device)
        check(L.fdx_keydir_remap(self._h, ops._ptr(id_map), id_map.numel(), int(kept), ops._ptr(ws), ws.numel(),
                                 ops._s(stream)), "fdx_keydir_remap")

    def resized(self, capacity: int) -> "KeyDirectory":
        """-> a new directory of `capacity` keys holding this one's keys under the same ids (a
        cold path; keys this one refused are new to it)."""
        d = KeyDirectory(capacity, self.max_batch)
        d.load(self.keys())
        return d


class StreamState:
    """Per-customer and per-terminal window state on the current GPU."""

    def __init__(self, n_customers: int, n_terminals: int, windows_days=(1, 7, 30), delay_days=7,
                 customer_ring=256, terminal_ring=256, max_batch=65536, flags_mode=_lib.FDX_FLAGS_NOTEBOOK,
                 stream=None, terminal_lateness_days=0):
        """terminal_lateness_days (fractions allowed; 0 = off): how far a terminal's row may lie
        behind the terminal's latest row (set_terminal_lateness)."""
        self.device = ops.require_gpu()
        self.windows_days = tuple(int(d) for d in windows_days)
        self.W = len(self.windows_days)
        self.max_batch = int(max_batch)
        h = ctypes.c_void_p()
        check(_lib.load().fdx_stream_create(int(n_customers), int(n_terminals), int(customer_ring), int(terminal_ring),
                                            self.W, ops._win_ns(self.windows_days), int(delay_days) * ops.NS_PER_DAY,
                                            int(flags_mode), self.max_batch, ctypes.byref(h), ops._s(stream)),
              "fdx_stream_create")
        self._h = h
        b = ctypes.c_size_t()
        check(_lib.load().fdx_stream_memory(h, ctypes.byref(b)), "fdx_stream_memory")
        self.memory_bytes = b.value
        self.n_customers, self.n_terminals = int(n_customers), int(n_terminals)
        self.customer_ring, self.terminal_ring = int(customer_ring), int(terminal_ring)
        self.delay_days, self.flags_mode = int(delay_days), int(flags_mode)
        self.terminal_lateness_ns, self.restored = 0, False
        if terminal_lateness_days:
            self.set_terminal_lateness(terminal_lateness_days)

    def set_terminal_lateness(self, days):
        """Accept terminal rows up to `days` (fractions allowed) behind their terminal's latest
        row: they get the counts of what had arrived and land in the state as if they had come
        in order (include/fdx.h: the refusals, status bits 8 and 16).  Rows late by no more than
        the delay change no feature of any row.  0 = off: any row that goes back in time raises.
        The customer half stays strict.  The value is a kernel argument: graphs captured by
        StreamScorer.score_graph are keyed by it."""
        ns = int(round(float(days) * ops.NS_PER_DAY))
        check(_lib.load().fdx_stream_set_terminal_lateness(self._h, ns), "fdx_stream_set_terminal_lateness")
        self.terminal_lateness_ns = ns

    def late_counts(self, stream=None) -> dict:
        """Synchronise; -> {late_rows: late terminal rows inserted, late_past_delay: those already
        behind the delay boundary (an earlier row's features lacked them)} since create / reset."""
        c = (ctypes.c_int64 * len(LATE_COUNTS))()
        check(_lib.load().fdx_stream_late_counts(self._h, c, ops._s(stream)), "fdx_stream_late_counts")
        return dict(zip(LATE_COUNTS, (int(v) for v in c)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and _lib._lib is not None:
            _lib._lib.fdx_stream_destroy(h)
            self._h = None

    def reset(self, stream=None):
        check(_lib.load().fdx_stream_reset(self._h, ops._s(stream)), "fdx_stream_reset")
        self.restored = False

    def update(self, ts, customer=None, amount=None, terminal=None, fraud=None, X=None, term_col0=-1,
               term_records=None, cust_nb=None, cust_sum=None, stream=None):
        """One micro-batch (device tensors; int64 ns, int32 ids, f64, int32 ids, u8).  Writes and
        returns X [n, >= 3 + 4W] float64 (columns in `input_features` order) unless the
        terminal half goes to term_records [n, W] int64 (count records) and the customer half
        to the planes cust_nb [W, n] int32 / cust_sum [W, n] float64 (rolling SUM; the scoring
        layout of ops.forest_prepare_grouped with val_is_sum) -- then X is None."""
        ops._dev(ts, torch.int64, "ts")
        n = ts.numel()
        if n > self.max_batch:
            raise FdxError(f"batch of {n} rows > max_batch {self.max_batch}")
        for t, dt, name in ((customer, torch.int32, "customer"), (amount, torch.float64, "amount"),
                            (terminal, torch.int32, "terminal"), (fraud, torch.uint8, "fraud")):
            if t is not None:
                ops._dev(t, dt, name)
                if t.numel() != n:
                    raise FdxError(f"{name} has {t.numel()} rows, ts has {n}")
        W = self.W
        if (cust_nb is None) != (cust_sum is None):
            raise FdxError("cust_nb and cust_sum go together")
        if cust_nb is not None:
            ops._dev(cust_nb, torch.int32, "cust_nb")
            ops._dev(cust_sum, torch.float64, "cust_sum")
            if cust_nb.numel() < W * n or cust_sum.numel() < W * n or not (cust_nb.is_contiguous()
                                                                           and cust_sum.is_contiguous()):
                raise FdxError(f"cust_nb / cust_sum need {W} x {n} contiguous elements")
        cust_planes = customer is not None and cust_nb is not None
        if X is None and ((customer is not None and not cust_planes) or (terminal is not None
                                                                         and term_records is None)):
            X = torch.empty((n, 3 + 4 * W), dtype=torch.float64, device=ts.device)
        if X is not None and (X.dtype != torch.float64 or X.stride(1) != 1):
            raise FdxError("X must be float64 with unit column stride")
        check(_lib.load().fdx_stream_update(self._h, ops._ptr(ts), ops._ptr(customer), ops._ptr(amount),
                                            ops._ptr(terminal), ops._ptr(fraud), n, ops._ptr(X),
                                            X.stride(0) if X is not None else 0, int(term_col0),
                                            ops._ptr(cust_nb), ops._ptr(cust_sum), ops._ptr(term_records),
                                            ops._s(stream)), "fdx_stream_update")
        return X

    def report_frauds(self, ts, terminal, stream=None):
        """Delayed fraud reports (device tensors; int64 ns, int32 ids): the transaction of
        terminal[i] at ts[i] was fraud.  Sets the row's label in the terminal state as if it had
        been known all along (include/fdx.h: the five outcomes, the limit on tied rows); a
        report that arrives within the delay changes no feature already emitted.  Positive
        reports only.  Stream-ordered with update(); state addresses do not move, so a captured
        score_graph stays valid."""
        ops._dev(ts, torch.int64, "ts")
        ops._dev(terminal, torch.int32, "terminal")
        n = ts.numel()
        if terminal.numel() != n:
            raise FdxError(f"terminal has {terminal.numel()} rows, ts has {n}")
        if n > self.max_batch:
            raise FdxError(f"batch of {n} reports > max_batch {self.max_batch}")
        check(_lib.load().fdx_stream_report_frauds(self._h, ops._ptr(ts), ops._ptr(terminal), n, ops._s(stream)),
              "fdx_stream_report_frauds")

    def label_counts(self, stream=None) -> dict:
        """Synchronise; -> the outcomes of the reports since create / reset."""
        c = (ctypes.c_int64 * len(LABEL_OUTCOMES))()
        check(_lib.load().fdx_stream_label_counts(self._h, c, ops._s(stream)), "fdx_stream_label_counts")
        return dict(zip(LABEL_OUTCOMES, (int(v) for v in c)))

    def _snap_ws(self):
        ws = getattr(self, "_snapshot_ws", None)
        if ws is None:
            ws = self._snapshot_ws = ops.workspace(_lib.load().fdx_stream_snapshot_workspace_size(self._h), self.device)
        return ws

    def snapshot(self, customers=None, terminals=None, stream=None) -> torch.Tensor:
        """-> the live state as a device uint8 tensor (format: include/fdx.h; canonical bytes that
        restore into any ring size and key capacity that fits).  customers / terminals: a key
        selection (first, count, step) = keys first + j * step, j < count; None = every key.
        Synchronises (a cold path); a state with a status bit up raises FdxUnsupported and the
        bit stays up."""
        L = _lib.load()
        sel = [ctypes.byref(_lib.KeySelection(*(int(v) for v in s))) if s is not None else None
               for s in (customers, terminals)]
        ws = self._snap_ws()
        nb = ctypes.c_size_t()
        check(L.fdx_stream_snapshot_size(self._h, sel[0], sel[1], ctypes.byref(nb), ops._ptr(ws), ws.numel(),
                                         ops._s(stream)), "fdx_stream_snapshot_size")
        out = torch.empty(nb.value, dtype=torch.uint8, device=self.device)
        check(L.fdx_stream_snapshot(self._h, sel[0], sel[1], ops._ptr(out), out.numel(), None, ops._ptr(ws),
                                    ws.numel(), ops._s(stream)), "fdx_stream_snapshot")
        return out

    def restore(self, snap, customers_at=(0, 1), terminals_at=(0, 1), counters=True, stream=None):
        """Write a snapshot's keys into this state: snapshot key j lands on key first + j * step
        (customers_at / terminals_at = (first, step)); all other keys are untouched, so restores
        into disjoint key sets merge.  snap: device or host uint8 tensor, numpy array or bytes.
        Refused (FdxError, nothing written) when the windows or the delay differ, a key falls
        outside the capacity or a key's live rows exceed this state's ring.  counters: add the
        snapshot's label counters to this state's.  State addresses do not move: a captured
        score_graph stays valid.  A snapshot carries a key's rows from its oldest boundary on, so
        from here until reset() a late terminal row is accepted only when the oldest row the ring
        holds reaches the row's farthest window (else status bit 16)."""
        d = _to_device_bytes(snap, self.device)
        ws = self._snap_ws()
        check(_lib.load().fdx_stream_restore(self._h, ops._ptr(d), d.numel(), int(customers_at[0]),
                                             int(customers_at[1]), int(terminals_at[0]), int(terminals_at[1]),
                                             _lib.FDX_RESTORE_COUNTERS if counters else 0, ops._ptr(ws), ws.numel(),
                                             ops._s(stream)), "fdx_stream_restore")
        self.restored = True

    @classmethod
    def from_snapshot(cls, snap, n_customers=None, n_terminals=None, customer_ring=None, terminal_ring=None,
                      max_batch=65536, terminal_lateness_days=0):
        """A new state holding the snapshot: windows, delay and flags mode from its header; key
        capacities default to its key counts, ring sizes to those of its source.  The terminal
        lateness is no part of a snapshot: pass it again."""
        f = snapshot_info(snap)
        if any(w % ops.NS_PER_DAY for w in f["window_ns"]) or f["delay_ns"] % ops.NS_PER_DAY:
            raise FdxUnsupported("the snapshot's windows or delay are not whole days")
        st = cls(f["customer_keys"] if n_customers is None else n_customers,
                 f["terminal_keys"] if n_terminals is None else n_terminals,
                 tuple(w // ops.NS_PER_DAY for w in f["window_ns"]), f["delay_ns"] // ops.NS_PER_DAY,
                 f["customer_ring"] if customer_ring is None else customer_ring,
                 f["terminal_ring"] if terminal_ring is None else terminal_ring, max_batch, f["flags_mode"],
                 terminal_lateness_days=terminal_lateness_days)
        st.restore(snap)
        return st

    def _retire_ws(self, chunk_keys=0):
        cache = self.__dict__.setdefault("_retire_wss", {})
        ws = cache.get(int(chunk_keys))
        if ws is None:
            nb = _lib.load().fdx_stream_retire_workspace_size(self._h, int(chunk_keys))
            ws = cache[int(chunk_keys)] = ops.workspace(nb, self.device)
        return ws

    def retire_plan(self, watermark_ns: int, stream=None):
        """Which keys can no longer influence a feature, given that no later row has
        ts < watermark_ns (include/fdx.h, f-10): -> (cust_map, term_map, counts).  A map is an
        int32 device tensor over the half's capacity, map[id] = the new id (the rank among the
        survivors) or -1 when retired; None for a half the state lacks.  counts = {"customers":
        {"kept", "retired"}, "terminals": {...}}, retired counting the keys that had rows.  Writes
        nothing to the state; synchronises; a state with a status bit up raises FdxUnsupported."""
        maps = [torch.empty(n, dtype=torch.int32, device=self.device) if n else None
                for n in (self.n_customers, self.n_terminals)]
        c = (ctypes.c_int64 * 4)()
        ws = self._retire_ws()
        check(_lib.load().fdx_stream_retire_plan(self._h, int(watermark_ns), ops._ptr(maps[0]), ops._ptr(maps[1]), c,
                                                 ops._ptr(ws), ws.numel(), ops._s(stream)), "fdx_stream_retire_plan")
        counts = {"customers": {"kept": int(c[0]), "retired": int(c[1])},
                  "terminals": {"kept": int(c[2]), "retired": int(c[3])}}
        return maps[0], maps[1], counts

    def retire_apply(self, cust_map, cust_kept, term_map, term_kept, chunk_keys=0, stream=None):
        """Move the surviving keys' records and rings to their new ids, in place, and clear the
        records of the ids from kept on (a map of None skips that half).  chunk_keys: keys staged
        per gather / scatter pair (0: the default).  A malformed map, a wrong kept or a status bit
        up raises with nothing written.  State addresses do not move: a captured score_graph
        stays valid."""
        for m, name in ((cust_map, "cust_map"), (term_map, "term_map")):
            if m is not None:
                ops._dev(m, torch.int32, name)
        if cust_map is not None and cust_map.numel() != self.n_customers:
            raise FdxError(f"cust_map has {cust_map.numel()} entries, the state {self.n_customers} customers")
        if term_map is not None and term_map.numel() != self.n_terminals:
            raise FdxError(f"term_map has {term_map.numel()} entries, the state {self.n_terminals} terminals")
        ws = self._retire_ws(chunk_keys)
        check(_lib.load().fdx_stream_retire_apply(self._h, ops._ptr(cust_map), int(cust_kept), ops._ptr(term_map),
                                                  int(term_kept), ops._ptr(ws), ws.numel(), ops._s(stream)),
              "fdx_stream_retire_apply")

    def check(self, stream=None):
        """Synchronise and raise if a kernel reported a problem since the last check."""
        f = ctypes.c_int32()
        check(_lib.load().fdx_stream_status(self._h, ctypes.byref(f), ops._s(stream)), "fdx_stream_status")
        if f.value:
            raise FdxUnsupported("stream state: " + "; ".join(m for b, m in _STATUS.items() if f.value & b))

    def watch(self, stream=None):
        """Enqueue a non-blocking copy of the status bits (pinned host memory + event); the
        next poll() raises if the batch that preceded this call reported a problem."""
        if getattr(self, "_pin", None) is None:
            self._pin = torch.zeros(1, dtype=torch.int32, pin_memory=True)
            self._ev = torch.cuda.Event()
        check(_lib.load().fdx_stream_status_async(self._h, ctypes.c_void_p(self._pin.data_ptr()), ops._s(stream)),
              "fdx_stream_status_async")
        self._ev.record(stream or torch.cuda.current_stream())
        self._watching = True

    def poll(self, block: bool = False):
        """Raise (and clear the bits) if the last watch() saw a problem.  Non-blocking unless
        block: a copy still in flight is looked at by a later poll()."""
        if not getattr(self, "_watching", False):
            return
        if not block and not self._ev.query():
            return
        self._ev.synchronize()
        self._watching = False
        if int(self._pin.item()):
            self.check()  # synchronises, clears and raises with the decoded bits


class StreamScorer:
    """Features + scaler + forest per micro-batch on one GPU (config 5 at N = 1)."""

    def __init__(self, forest: ops.Forest, n_customers: int, n_terminals: int, windows_days=(1, 7, 30),
                 delay_days=7, customer_ring=256, terminal_ring=256, max_batch=65536,
                 flags_mode=_lib.FDX_FLAGS_NOTEBOOK, fused=True, terminal_lateness_days=0, raw_ids=False):
        """raw_ids: customer / terminal are raw int64 ids (any value but INT64_MIN, new ones in
        any batch) in score, score_graph, report_frauds and score_cdc; two KeyDirectory of
        capacities n_customers / n_terminals number them on the device, inside the batch (and
        inside score_graph's graph).  A key beyond a capacity raises like an id out of range:
        grow() before that.  False: dense int32 ids in [0, n), no directory, nothing added."""
        self.forest = forest
        self.raw_ids = bool(raw_ids)
        self.state = StreamState(n_customers, n_terminals, windows_days, delay_days, customer_ring, terminal_ring,
                                 max_batch, flags_mode, terminal_lateness_days=terminal_lateness_days)
        W = self.state.W
        if forest.n_features != 3 + 4 * W:
            raise FdxError(f"forest has {forest.n_features} features, the stream makes {3 + 4 * W}")
        dev = self.state.device
        self.flags_mode = int(flags_mode)
        self.fused = fused
        if fused:  # state kernels -> NB / SUM planes + count records -> scoring rows (no X matrix)
            self.cnb = torch.empty(W * max_batch, dtype=torch.int32, device=dev)
            self.csum = torch.empty(W * max_batch, dtype=torch.float64, device=dev)
            self.trec = torch.empty(max_batch * W, dtype=torch.int64, device=dev)
        else:
            self.X = torch.empty((max_batch, 3 + 4 * W), dtype=torch.float64, device=dev)
        self.ws = ops.workspace(forest.workspace_size_max(max_batch), dev)
        self.proba = torch.empty(max_batch, dtype=torch.float64, device=dev)
        if self.raw_ids:  # per-scorer id buffers, max_batch long: score_graph's key does not change
            self.customers, self.terminals = KeyDirectory(n_customers, max_batch), KeyDirectory(n_terminals, max_batch)
            self._cid = torch.empty(max_batch, dtype=torch.int32, device=dev)
            self._tid = torch.empty(max_batch, dtype=torch.int32, device=dev)

    def _dense(self, customer, terminal):
        """raw_ids: the batch's raw int64 ids -> dense ids (new keys inserted), on the stream."""
        if not self.raw_ids:
            return customer, terminal
        n = customer.numel()
        if n > self.state.max_batch:
            raise FdxError(f"batch of {n} rows > max_batch {self.state.max_batch}")
        return (self.customers.map(customer, True, self._cid[:n]), self.terminals.map(terminal, True, self._tid[:n]))

    def key_counts(self) -> dict:
        """raw_ids: synchronise; -> {"customers": KeyDirectory.counts(), "terminals": ...}."""
        self._need_raw("key_counts")
        return {"customers": self.customers.counts(), "terminals": self.terminals.counts()}

    def _need_raw(self, what):
        if not self.raw_ids:
            raise FdxError(f"{what} needs a scorer made with raw_ids=True")

    def snapshot_keys(self) -> dict:
        """raw_ids: -> {"customers": int64 tensor, "terminals": int64 tensor}, tensor[id] = raw key
        (save_keys / load_keys).  Taken with snapshot(), the pair restores the stream."""
        self._need_raw("snapshot_keys")
        return {"customers": self.customers.keys(), "terminals": self.terminals.keys()}

    def restore_keys(self, d):
        """raw_ids: load snapshot_keys()'s dict into the (empty) directories."""
        self._need_raw("restore_keys")
        self.customers.load(d["customers"])
        self.terminals.load(d["terminals"])

    def grow(self, n_customers=None, n_terminals=None):
        """New key capacities (None: unchanged), a cold path: the window state moves through
        snapshot -> StreamState.from_snapshot, the directories through keys -> resized.  Waits
        for the status of the batches so far (a flagged batch raises here).  Addresses move, so
        the graphs score_graph captured are dropped.  As after any restore, late terminal rows
        are accepted on the restored state's terms (StreamState.restore); late_counts restart."""
        st = self.state
        st.poll(block=True)
        nc = st.n_customers if n_customers is None else int(n_customers)
        nt = st.n_terminals if n_terminals is None else int(n_terminals)
        if nc < st.n_customers or nt < st.n_terminals:
            raise FdxError("grow cannot shrink a key capacity")
        new = StreamState.from_snapshot(st.snapshot(), n_customers=nc, n_terminals=nt, customer_ring=st.customer_ring,
                                        terminal_ring=st.terminal_ring, max_batch=st.max_batch)
        if st.terminal_lateness_ns:
            check(_lib.load().fdx_stream_set_terminal_lateness(new._h, st.terminal_lateness_ns),
                  "fdx_stream_set_terminal_lateness")
            new.terminal_lateness_ns = st.terminal_lateness_ns
        if self.raw_ids:
            if nc != st.n_customers:
                self.customers = self.customers.resized(nc)
            if nt != st.n_terminals:
                self.terminals = self.terminals.resized(nt)
        self.state = new
        self.__dict__.pop("_graphs", None)

    def retire_idle(self, watermark) -> dict:
        """raw_ids: let go of the keys that can no longer influence a feature, so that their ids,
        state rows and hash slots are reused (a cold path: hourly, daily).  watermark (int ns or
        numpy.datetime64): the caller's promise that no row fed from here on has ts < watermark,
        in either half, late terminal rows included (with a terminal lateness set: the next
        batch's first ts minus the lateness).  Retired: customers idle since watermark - the
        longest window, terminals idle since watermark - (delay + the longest window); such a key
        that comes back is a new key and its features are bit-identical (include/fdx.h).  The
        survivors keep their order (new id = rank), so state, snapshot() and snapshot_keys()
        equal those of a stream fed the history without the retired keys' rows.  Waits for the
        status of the batches so far; addresses do not move and score_graph's graphs stay valid.
        A fraud report for a retired terminal raises like one for a terminal never seen: drop
        reports older than watermark - (delay + the longest window) to avoid that.
        -> {"customers": {"kept", "retired"}, "terminals": {...}}; a half in which nothing is
        retired is not touched."""
        self._need_raw("retire_idle")
        st = self.state
        st.poll(block=True)
        import numpy as np

        if isinstance(watermark, np.datetime64):
            watermark = watermark.astype("datetime64[ns]").astype(np.int64)
        watermark = int(watermark)
        cmap, tmap, counts = st.retire_plan(watermark)
        go_c = cmap is not None and counts["customers"]["retired"] > 0
        go_t = tmap is not None and counts["terminals"]["retired"] > 0
        if go_c or go_t:
            st.retire_apply(cmap if go_c else None, counts["customers"]["kept"], tmap if go_t else None,
                            counts["terminals"]["kept"])
        if go_c:
            self.customers.remap(cmap, counts["customers"]["kept"])
        if go_t:
            self.terminals.remap(tmap, counts["terminals"]["kept"])
        return counts

    def _no_labels(self, n):
        """fraud = None: the batch's labels are not known yet (report_frauds brings them).  One
        zero buffer for every batch size, so score_graph's key (its address) stays stable."""
        z = getattr(self, "_zero_fraud", None)
        if z is None:
            z = self._zero_fraud = torch.zeros(self.state.max_batch, dtype=torch.uint8, device=self.state.device)
        return z[:n]

    def set_terminal_lateness(self, days):
        """StreamState.set_terminal_lateness; a change drops the graphs score_graph captured (the
        value is an argument of the kernels inside them)."""
        before = self.state.terminal_lateness_ns
        self.state.set_terminal_lateness(days)
        if self.state.terminal_lateness_ns != before:
            self.__dict__.pop("_graphs", None)

    def report_frauds(self, ts, terminal):
        """StreamState.report_frauds on the current stream, with score()'s status polling (a
        terminal id out of range raises at the next call or finish())."""
        self.state.poll()
        if self.raw_ids:  # lookup only: a terminal the stream never saw -> -1 -> status bit 4
            n = terminal.numel()
            if n > self.state.max_batch:
                raise FdxError(f"batch of {n} reports > max_batch {self.state.max_batch}")
            terminal = self.terminals.map(terminal, False, self._tid[:n])
        self.state.report_frauds(ts, terminal)
        self.state.watch()

    def snapshot(self, customers=None, terminals=None):
        """StreamState.snapshot on the current stream, after the status of the batches so far
        was waited for (a flagged batch raises here, as in finish())."""
        self.state.poll(block=True)
        return self.state.snapshot(customers, terminals)

    def restore(self, snap, customers_at=(0, 1), terminals_at=(0, 1), counters=True):
        """StreamState.restore on the current stream (status polled first).  The graphs captured
        by score_graph stay valid: the state's addresses do not move."""
        self.state.poll(block=True)
        self.state.restore(snap, customers_at, terminals_at, counters)

    def score(self, ts, customer, amount, terminal, fraud=None):
        """-> predict_proba[:, 1] of the batch (device view, valid until the next call).
        fraud None: no labels yet (zeros; report_frauds brings them later).
        Ring overflows, ids out of range and rows that go back in time are flagged by the
        kernels; every batch enqueues a non-blocking copy of those bits and the next score()
        (or finish()) raises FdxUnsupported for the batch that set them."""
        self.state.poll()
        n = ts.numel()
        if fraud is None:
            fraud = self._no_labels(n)
        customer, terminal = self._dense(customer, terminal)
        if not self.fused:
            X = self.state.update(ts, customer, amount, terminal, fraud, X=self.X[:n])
            out = self.forest.predict(X, ws=self.ws, out=self.proba[:n])
            self.state.watch()
            return out
        W = self.state.W
        cnb, csum = self.cnb[:W * n].view(W, n), self.csum[:W * n].view(W, n)
        trec = self.trec[:n * W].view(n, W)
        self.state.update(ts, customer, amount, terminal, fraud, term_records=trec, cust_nb=cnb, cust_sum=csum)
        # flags (from ts), averages = SUM / NB, risks = FRAUD / NB, scaling, threshold ranks
        ops.forest_prepare_grouped(self.forest, self.flags_mode, ts, amount, cnb, csum, None, None, trec, self.ws,
                                   n=n, val_is_sum=True)
        out = ops.forest_traverse(self.forest, n, self.ws, self.proba[:n])
        self.state.watch()
        return out

    def finish(self):
        """Wait for the last batch's status bits and raise if it reported a problem."""
        self.state.poll(block=True)

    def score_graph(self, ts, customer, amount, terminal, fraud=None, out_host=None, replay: bool = True):
        """score() replayed from a HIP graph: the batch's kernels (state update, row assembly,
        forest walk, tree sums), its status-word copy and -- with out_host (pinned, float64,
        >= n) -- the probabilities' copy to the host are captured once per (batch size, buffer
        addresses) and then launched as ONE graph per batch, so the host enqueues one call
        instead of ~10 (fused mode only).  Inputs must live at the same addresses on every call
        with that size (a consumer's staging buffers).  Same results and status semantics as
        score(); -> the device view of the probabilities.  replay=False: capture only (a consumer
        that knows its batch sizes captures them before the first batch arrives)."""
        if not self.fused:
            raise FdxError("score_graph needs the fused scorer")
        if replay:
            self.state.poll()
        n = ts.numel()
        if fraud is None:
            fraud = self._no_labels(n)
        key = (n, self.forest.epoch) + tuple(t.data_ptr() for t in (ts, customer, amount, terminal, fraud)) + \
            ((out_host.data_ptr(),) if out_host is not None else ())
        if self.state.terminal_lateness_ns:  # the late kernel's arguments: the lateness, the restored flag
            key += ("late", self.state.terminal_lateness_ns, self.state.restored)
        graphs = self.__dict__.setdefault("_graphs", {})
        g = graphs.get(key)
        if g is None:
            for k in [k for k in graphs if k[1] != self.forest.epoch]:
                del graphs[k]  # captured over a forest layout that no longer exists
            st = self.state
            if getattr(st, "_pin", None) is None:  # watch()'s pinned status word, captured below
                st._pin = torch.zeros(1, dtype=torch.int32, pin_memory=True)
                st._ev = torch.cuda.Event()
            W = st.W
            cnb, csum = self.cnb[:W * n].view(W, n), self.csum[:W * n].view(W, n)
            trec = self.trec[:n * W].view(n, W)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                customer, terminal = self._dense(customer, terminal)
                st.update(ts, customer, amount, terminal, fraud, term_records=trec, cust_nb=cnb, cust_sum=csum)
                ops.forest_prepare_grouped(self.forest, self.flags_mode, ts, amount, cnb, csum, None, None, trec,
                                           self.ws, n=n, val_is_sum=True)
                ops.forest_traverse(self.forest, n, self.ws, self.proba[:n])
                check(_lib.load().fdx_stream_status_async(st._h, ctypes.c_void_p(st._pin.data_ptr()), ops._s()),
                      "fdx_stream_status_async")
                if out_host is not None:
                    out_host[:n].copy_(self.proba[:n], non_blocking=True)
            graphs[key] = g
        if not replay:
            return None
        g.replay()
        self.state._ev.record(torch.cuda.current_stream())
        self.state._watching = True
        return self.proba[:n]

    def score_cdc(self, tx_id, customer_id, terminal_id, amount_bytes, amount_offsets, tx_datetime_us, kafka_ts,
                  fraud=None):
        """One Debezium micro-batch scored from its wire columns, device-resident end to end --
        the reference's sink (pyspark/scripts/kafka_s3_sink_transactions.py) decodes tx_amount
        DECIMAL(10,2) bytes (:64-71), truncates tx_datetime microseconds to seconds (:167) and
        keeps the latest record per tx_id by Kafka timestamp (:180); then the scoring job scores
        the rows (fraud_detection.py:183-201).  Here: fdx_cdc_decode -> fdx_dedup_latest ->
        fdx_cdc_compact (kept records, batch order) -> score().  Inputs are device tensors:
        tx_id / customer_id / terminal_id / tx_datetime_us / kafka_ts int64 [n], amount_bytes
        uint8 (the records' bytes back to back), amount_offsets int64 [n + 1], fraud uint8 [n]
        or None (the CDC topic carries no label: zeros; the TERMINAL_ID_RISK features then see
        only what report_frauds delivered).  One host read per batch (the kept
        count).  -> (proba [m] device view, rows int32 [m] = batch position of each kept record)."""
        L = _lib.load()
        n = tx_id.numel()
        dev = tx_id.device
        for t, nm in ((tx_id, "tx_id"), (customer_id, "customer_id"), (terminal_id, "terminal_id"),
                      (tx_datetime_us, "tx_datetime_us"), (kafka_ts, "kafka_ts")):
            ops._dev(t, torch.int64, nm)
            if t.numel() != n:
                raise FdxError(f"{nm} has {t.numel()} rows, tx_id has {n}")
        ops._dev(amount_bytes, torch.uint8, "amount_bytes")
        ops._dev(amount_offsets, torch.int64, "amount_offsets")
        if amount_offsets.numel() != n + 1:
            raise FdxError("amount_offsets needs n + 1 entries")
        if fraud is not None:
            ops._dev(fraud, torch.uint8, "fraud")
        if n > self.state.max_batch:
            raise FdxError(f"batch of {n} records > max_batch {self.state.max_batch}")
        c = getattr(self, "_cdc", None)
        if c is None:  # per-scorer buffers for max_batch records
            m = self.state.max_batch
            c = self._cdc = dict(
                amt=torch.empty(m, dtype=torch.float64, device=dev), ts=torch.empty(m, dtype=torch.int64, device=dev),
                keep=torch.empty(m, dtype=torch.uint8, device=dev), cust=torch.empty(m, dtype=torch.int32, device=dev),
                term=torch.empty(m, dtype=torch.int32, device=dev), ts_k=torch.empty(m, dtype=torch.int64, device=dev),
                amt_k=torch.empty(m, dtype=torch.float64, device=dev), fr_k=torch.empty(m, dtype=torch.uint8, device=dev),
                rows=torch.empty(m, dtype=torch.int32, device=dev),
                status=torch.zeros(2, dtype=torch.int64, device=dev),  # [count, bad]
                ws=ops.workspace(max(L.fdx_dedup_latest_workspace_size(m), L.fdx_cdc_compact_workspace_size(m)), dev),
                host=torch.zeros(2, dtype=torch.int64, pin_memory=True))
        st = torch.cuda.current_stream()
        P, S = ops._ptr, ops._s()
        bad = c["status"][1:].view(torch.int32)[:1]  # low word of status[1]
        c["status"].zero_()
        if n:
            check(L.fdx_cdc_decode(P(amount_bytes), P(amount_offsets), P(tx_datetime_us), n, None, P(c["amt"]),
                                   P(c["ts"]), P(bad), S), "fdx_cdc_decode")
            check(L.fdx_dedup_latest(P(tx_id), P(kafka_ts), n, P(c["keep"]), P(bad), P(c["ws"]), c["ws"].numel(), S),
                  "fdx_dedup_latest")
        check(L.fdx_cdc_compact(P(c["keep"]), n, P(customer_id), P(terminal_id), P(c["ts"]), P(c["amt"]), P(fraud),
                                P(c["cust"]), P(c["term"]), P(c["ts_k"]), P(c["amt_k"]), P(c["fr_k"]), P(c["rows"]),
                                P(c["status"]), P(c["ws"]), c["ws"].numel(), S), "fdx_cdc_compact")
        c["host"].copy_(c["status"], non_blocking=True)
        st.synchronize()
        m, b = int(c["host"][0]), int(c["host"][1])
        if b:
            raise FdxUnsupported("CDC batch: a tx_amount field of 0 or > 8 bytes, or tx_id -1 (reserved)")
        if not self.raw_ids:
            out = self.score(c["ts_k"][:m], c["cust"][:m], c["amt_k"][:m], c["term"][:m], c["fr_k"][:m])
            return out, c["rows"][:m]
        # raw ids: the kept records' int64 ids, gathered by their batch positions (the compaction's
        # int32 columns narrow them); only kept records reach the directories
        if "cust64" not in c:
            c["cust64"] = torch.empty(self.state.max_batch, dtype=torch.int64, device=dev)
            c["term64"] = torch.empty(self.state.max_batch, dtype=torch.int64, device=dev)
        if m:
            for src, dst in ((customer_id, c["cust64"]), (terminal_id, c["term64"])):
                check(L.fdx_gather(P(src), 8, P(c["rows"]), m, P(dst), S), "fdx_gather")
        out = self.score(c["ts_k"][:m], c["cust64"][:m], c["amt_k"][:m], c["term64"][:m], c["fr_k"][:m])
        return out, c["rows"][:m]


def stream_terminal_exchange(K, records, ts, terminal, fraud, world, n_terminals_total, windows_days=(1, 7, 30),
                             delay_days=7, group=None):
    """The per-batch terminal exchange of the sharded stream: rows to their terminal's owner
    (RCCL all-to-all), the owner's incremental update `records(rts, rterm_local, rfraud)`,
    count records back.  -> (records [n, W] in send order, send_perm).  K: the kernel set
    (fdx.distributed.GpuKernels; the CPU tests pass numpy stand-ins)."""
    from . import distributed as D

    st = D.exchange_begin(K, terminal, world, group)
    return D.exchange_finish(K, st, ts, terminal, fraud, world, n_terminals_total, windows_days, delay_days, group,
                             records=records)


class ShardedStreamScorer:
    """Config 5 over `world` GPUs (this process = `rank`).  Each rank receives the rows of its
    customers [customer_base, customer_base + n_customers_local) (Kafka partitions keyed by
    customer); terminal t's state lives on rank t % world as local id t // world."""

    def __init__(self, forest: ops.Forest, world: int, rank: int, n_customers_local: int, customer_base: int,
                 n_terminals_total: int, windows_days=(1, 7, 30), delay_days=7, customer_ring=256,
                 terminal_ring=256, max_batch=65536, max_recv=None, flags_mode=_lib.FDX_FLAGS_NOTEBOOK,
                 group=None, terminal_lateness_days=0):
        """terminal_lateness_days: the owner-side terminal state accepts rows that late (the
        ranks' batches of one terminal need not be aligned in time); the customer half stays
        strict.  Not yet run on more than one GPU with a lateness set."""
        self.forest, self.world, self.rank, self.group = forest, world, rank, group
        self.customer_base = int(customer_base)
        self.n_terminals_total = int(n_terminals_total)
        n_term_local = (self.n_terminals_total + world - 1) // world
        # the owner side sees up to every rank's rows of its terminals in one batch
        self.state = StreamState(n_customers_local, n_term_local, windows_days, delay_days, customer_ring,
                                 terminal_ring, max(max_batch, max_recv or max_batch * world), flags_mode,
                                 terminal_lateness_days=terminal_lateness_days)
        self.windows_days, self.delay_days = self.state.windows_days, int(delay_days)
        W = self.state.W
        dev = self.state.device
        self.flags_mode = int(flags_mode)
        self.cnb = torch.empty(W * max_batch, dtype=torch.int32, device=dev)
        self.csum = torch.empty(W * max_batch, dtype=torch.float64, device=dev)
        self.ws = ops.workspace(forest.workspace_size_max(max_batch), dev)
        self.proba = torch.empty(max_batch, dtype=torch.float64, device=dev)

    def _owner_records(self, rts, rterm, rfr):
        rec = torch.empty((rts.numel(), self.state.W), dtype=torch.int64, device=rts.device)
        self.state.update(rts, terminal=rterm, fraud=rfr, term_records=rec)
        return rec

    def score(self, ts, customer, amount, terminal, fraud):
        from . import distributed as D

        self.state.poll()
        n = ts.numel()
        W = self.state.W
        K = D.GpuKernels
        cust = ops.key_map(customer, _lib.FDX_KEY_SUB, self.customer_base) if self.customer_base else customer
        cnb, csum = self.cnb[:W * n].view(W, n), self.csum[:W * n].view(W, n)
        self.state.update(ts, cust, amount, cust_nb=cnb, cust_sum=csum)  # customer half, local
        back, send_perm = stream_terminal_exchange(K, self._owner_records, ts, terminal, fraud, self.world,
                                                   self.n_terminals_total, self.windows_days, self.delay_days,
                                                   self.group)
        # row r's count record is back[inv[r]] (send order -> row order through the inverse)
        inv = ops.invert_perm(send_perm)
        ops.forest_prepare_grouped(self.forest, self.flags_mode, ts, amount, cnb, csum, None, inv, back, self.ws,
                                   n=n, val_is_sum=True)
        out = ops.forest_traverse(self.forest, n, self.ws, self.proba[:n])
        self.state.watch()
        return out

    def finish(self):
        self.state.poll(block=True)

    def snapshot(self, customers=None, terminals=None):
        """This rank's state (its customer range and the terminals it owns, by local id);
        rank-local, no collective.  To re-shard from N to M ranks, new rank r restores from
        every old rank's snapshot the selection of the keys it will own."""
        self.state.poll(block=True)
        return self.state.snapshot(customers, terminals)

    def restore(self, snap, customers_at=(0, 1), terminals_at=(0, 1), counters=True):
        """StreamState.restore into this rank's state (local ids); rank-local, no collective."""
        self.state.poll(block=True)
        self.state.restore(snap, customers_at, terminals_at, counters)
