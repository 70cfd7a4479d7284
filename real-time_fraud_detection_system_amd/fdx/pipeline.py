"""Whole-table featurize (+ score) pipeline on device tensors.

One call replaces the notebook's whole featurization sequence
(feature_transformation.ipynb:278, :319, :1092-1093, :2435-2436) and, with a forest, the
scoring UDF body (pyspark/scripts/fraud_detection.py:183-195):

    flags -> re-key by CUSTOMER_ID -> customer windows -> re-key by TERMINAL_ID
          -> terminal windows -> assemble the 15 input_features -> scale + forest

Input rows are in time order (the reference's order: read_from_files sorts by
TRANSACTION_ID, which the generator assigns in TX_DATETIME order,
shared_functions.py:74-90, data_generator.ipynb:1364-1369); ``time_sort=True`` first
sorts them on the GPU.  All outputs are returned in input row order.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib, ops
from ._lib import check


@dataclass
class Features:
    weekend: torch.Tensor        # uint8 [n]
    night: torch.Tensor          # uint8 [n]
    cust_perm: torch.Tensor      # int32 [n] grouped position -> row
    cust_seg: torch.Tensor       # int64 [n_customers+1]
    cust_nb: torch.Tensor        # int32 [W, n] grouped order
    cust_avg: torch.Tensor       # float64 [W, n] grouped order
    term_perm: torch.Tensor
    term_seg: torch.Tensor
    term_nb: torch.Tensor        # int32 [W, n] grouped order
    term_risk: torch.Tensor      # float64 [W, n] grouped order
    X: Optional[torch.Tensor] = None  # float64 [n, ld] input_features in row order


class FraudPipeline:
    """avg_mode: "exact" -- the customer averages bit for bit as pandas' roll_sum (the
    sequential Kahan add/remove recurrence, k_customer_walk) -- or "scan" -- float64 prefix
    sums, fully parallel, within ~1e-13 relative of pandas (the counts
    and every other feature stay exact)."""

    # run_fused: the terminal half starts once the customer re-key is done on the device, so that
    # re-key has the GPU to itself (started together, the two re-keys took 0.90 and 1.00 ms in step
    # instead of 0.56 and 0.46 alone), and then runs at the HIGHER stream priority (lower number):
    # the customer walk's one-wave blocks take 22 KB of LDS each, 7 per CU fill a CU's LDS, and
    # dispatched first they left the terminal scatter (37-42 KB blocks) no CU until the walk's
    # queue drained (1.2 ms for a 0.2 ms pass, profiles/r05am trace).  Front half + assembly:
    # 3.84 (both at the start, customer high) -> 3.74 (terminal after the customer re-key) ->
    # 3.58-3.60 ms (and at high priority); profiles/r05ak_stream_order_ab.txt, r05an_priority_ab.txt.
    crit_priority = 0
    side_priority = -1
    # 1: the row assembly with its 64-bit slot arithmetic (what it ran before it kept the loop's
    # bookkeeping in 32-bit scalars; tools/step_ab.py measures the two -- DESIGN §4)
    assembly_index64 = 0
    # 1: run_fused's re-keys carry ts as int32 seconds whenever every timestamp has that form exactly
    # (decided on the device inside the first radix pass, wide fallback otherwise:
    # ops.rekey_payload(narrow=); W = 3 with compact records and the exact walk).  0: the 8-byte
    # column, as before (tools/step_ab.py measures the two -- DESIGN §3)
    narrow_payloads = 1
    # 1: with narrow_payloads, the customer re-key also tries amount as int32 cents.  Off by default:
    # the handbook generator's scenario-3 frauds are a cents amount x 5 in float64 (385.45000000000005),
    # which has no exact cents form, so on such a table every step would pay the converting pass and
    # then the wide passes (DESIGN §3 has the measurement)
    narrow_amounts = 0
    # 1: with an ops.FeatureTable as rows_out (3 windows, the exact walk), run_fused's customer half
    # writes its table columns in place -- the walk cust_nb and cust_avg (the division moves into its
    # output stage), the layout fill the row index -- and the row assembly reads them there instead of
    # copying 40 B per slot out of scratch arrays into the table.  0: the scratch arrays, as before
    # (tools/step_ab.py measures the two -- DESIGN §4)
    table_in_place = 1
    # how long the host polls for the layout plan's slot count before a blocking wait: the plan of
    # step k lands only after step k - 1's forest (6.6 ms at configs[1]) when steps are queued back
    # to back, and a blocking hipEventSynchronize woke up ~150 us after it (profiles/r06t trace: plan
    # done at 0.64 ms, layout fill at 0.81 ms)
    plan_spin_s = 0.05

    def __init__(self, windows_days: Sequence[int] = (1, 7, 30), delay_days: int = 7,
                 flags_mode: int = _lib.FDX_FLAGS_NOTEBOOK, forest: Optional[ops.Forest] = None,
                 avg_mode: str = "exact", compact_records: bool = True):
        if avg_mode not in ("exact", "scan"):
            raise ValueError("avg_mode must be 'exact' or 'scan'")
        self.avg_mode = avg_mode
        # the scoring path's terminal count records in the 16-byte compact form (3 windows): one
        # 16-byte store / load per row at random instead of two for the 24-byte record
        # (terminal windows 0.65 -> 0.41 ms alone, profiles/r03ac_compact_records_ab.txt)
        self.compact_records = bool(compact_records)
        self.windows_days = tuple(int(w) for w in windows_days)
        self.delay_days = int(delay_days)
        self.flags_mode = flags_mode
        self.forest = forest
        self.n_features = 3 + 4 * len(self.windows_days)
        self._ws = None
        # the scoring step's own: two streams (run_fused) and the arena, created on first use on a
        # device; the last layout's buffer size (the next one-shot layout's first try) and slot count
        self._side = self._crit = self._arena = None
        self._slots_hint = self.last_slots = None
        # run_fused: which form each re-key's columns took in the last step -- [customer, terminal],
        # an ops.Narrow each (None: that re-key ran wide); for tests and tools
        self.narrow_flags = [None, None]

    def featurize(self, ts_ns, customer, terminal, amount, fraud, n_customers: int, n_terminals: int,
                  assemble: bool = True, time_sort: bool = False, stream=None) -> Features:
        """ts_ns int64, customer/terminal int32 (dense ids in [0, n_*)), amount float64,
        fraud uint8 -- all GPU tensors of length n in time order (see time_sort)."""
        if time_sort:
            tperm = ops.argsort_i64(ts_ns, stream)
            f = self.featurize(ops.gather(ts_ns, tperm, stream), ops.gather(customer, tperm, stream),
                               ops.gather(terminal, tperm, stream), ops.gather(amount, tperm, stream),
                               ops.gather(fraud, tperm, stream), n_customers, n_terminals, False,
                               False, stream)
            f = _to_caller_order(f, tperm, stream)
            if assemble:
                f.X = self.assemble(f, amount, stream)
            return f
        n = ts_ns.numel()
        we, ni = ops.time_flags(ts_ns, self.flags_mode, stream)
        cperm, cseg, cnb, cavg = self.customer_features(customer, n_customers, ts_ns, amount, stream)
        tperm, tseg, tgts, _ = ops.rekey_payload(terminal, n_terminals, ts_ns, stream=stream)
        tnb, trisk = ops.terminal_windows_grouped(tgts, tseg, gfraud=ops.gather(fraud, tperm, stream),
                                                  delay_days=self.delay_days, windows_days=self.windows_days,
                                                  records=False, stream=stream)
        f = Features(we, ni, cperm, cseg, cnb, cavg, tperm, tseg, tnb, trisk)
        if assemble:
            f.X = self.assemble(f, amount, stream)
        return f

    def customer_features(self, customer, n_customers: int, ts_ns, amount, stream=None, bad=None):
        """featurize's customer part -> (cust_perm, cust_seg, cust_nb, cust_avg): the re-key carries
        the columns the window kernels read (grouped, sequential); bad: ops.rekey_payload's count of
        ids outside [0, n_customers)."""
        cperm, cseg, gts, gamt = ops.rekey_payload(customer, n_customers, ts_ns, amount, stream=stream, bad=bad)
        if self.avg_mode == "scan":
            cnb, cavg = ops.customer_windows_scan(gts, gamt, cseg, self.windows_days, stream=stream)
        else:
            cnb, cavg = ops.customer_windows(gts, gamt, cseg, self.windows_days, stream)
        return cperm, cseg, cnb, cavg

    def assemble(self, f: Features, amount: torch.Tensor, stream=None) -> torch.Tensor:
        """f's terminal fields None: those columns are left for the caller to fill."""
        n = amount.numel()
        ld = 16 if self.n_features <= 16 else self.n_features
        X = torch.empty((n, ld), dtype=torch.float64, device=amount.device)
        W = len(self.windows_days)
        p = ops._ptr
        check(_lib.load().fdx_assemble_features(n, W, p(amount), p(f.weekend), p(f.night), p(f.cust_perm),
                                                p(f.cust_nb), p(f.cust_avg), p(f.term_perm), p(f.term_nb),
                                                p(f.term_risk), p(X), ld, ops._s(stream)),
              "fdx_assemble_features")
        return X[:, : self.n_features]

    def score(self, X: torch.Tensor, out: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
        if self.forest is None:
            raise _lib.FdxError("FraudPipeline has no forest")
        need = self.forest.workspace_size(X.shape[0])
        if self._ws is None or self._ws.numel() < need or self._ws.device != X.device:
            self._ws = ops.workspace(need, X.device)
        return self.forest.predict(X, ws=self._ws, out=out, stream=stream)

    def run(self, ts_ns, customer, terminal, amount, fraud, n_customers, n_terminals, stream=None):
        """featurize (with the float64 feature matrix) + score; returns (Features, proba)."""
        f = self.featurize(ts_ns, customer, terminal, amount, fraud, n_customers, n_terminals, True,
                           False, stream)
        return f, self.score(f.X, stream=stream)

    def run_fused(self, ts_ns, customer, terminal, amount, fraud, n_customers, n_terminals,
                  proba: torch.Tensor, ws: Optional[torch.Tensor] = None, stream=None, mark=None,
                  validate: bool = True, overlap: bool = True, rows_out=None):
        """The scoring path of bench.py: no float64 feature matrix.  The customer half is
        computed in the interleaved (lane-major) layout and the scoring rows follow that
        layout (customer features already in place, the terminal half one count record per
        row, read through the layout's irow); the last forest launch writes proba back in
        input row order.

        Streams: the terminal half (re-key + windows) runs on a side stream, concurrently with
        the customer half's layout plan, layout and walk (it waits for the customer re-key; only its
        first histogram pass runs beside that) -- the customer walk is a latency-bound recurrence with one
        lane per (customer, window) that leaves most SIMDs idle; the two meet at the row assembly.  The
        customer half, assembly and forest run on a stream of the pipeline's own, the terminal half
        on a higher-priority one (crit_priority / side_priority), ordered after the caller's stream
        on entry and before it on return.
        mark(stage, stream) is called after each stage is enqueued on its stream (bench.py
        records a HIP event there).  validate: the customer / terminal ids must lie in
        [0, n_customers) / [0, n_terminals) (counted on the device, read once everything is
        enqueued -- no extra stall).  overlap=False runs everything on the caller's stream
        (bench.py's isolated per-stage timings).  rows_out: the featurized table -- the 14
        feature columns the reference's featurization writes, with each transaction's input
        row -- from the same assembly pass: an ops.FeatureRecords(n) (one record per input row,
        time order: one random 80-byte write per row) or an ops.FeatureTable (columns by
        scoring slot, written coalesced; capacity >= self.last_slots, which a caller can size
        as n * 11 // 10 -- the layout pads < 1 %; padding slots' rows are -1)."""
        W = len(self.windows_days)
        mk = mark or (lambda _name, _st: None)
        caller = stream or torch.cuda.current_stream()
        check_rows_out(rows_out, ts_ns)
        if ts_ns.numel() == 0:  # an empty table: nothing to score
            return proba
        if self._side is None or self._side.device != ts_ns.device:
            self._side = torch.cuda.Stream(device=ts_ns.device, priority=self.side_priority)
            # two streams of the pipeline's own; their priorities: crit_priority / side_priority
            self._crit = torch.cuda.Stream(device=ts_ns.device, priority=self.crit_priority)
        main = self._crit if overlap else caller
        side = self._side if overlap else caller
        # the customer half (its re-key shares its scratch with the terminal one, which starts after it)
        half = _CustomerHalf(self, ts_ns.device, main, mk, shared=("rekey_ws",))
        ar = half.arena
        if main is not caller:
            main.wait_stream(caller)
            main.wait_stream(side)
            for t in (ts_ns, customer, terminal, amount, fraud, proba) + ((ws,) if ws is not None else ()) + \
                ((rows_out.buf,) if rows_out is not None else ()):
                t.record_stream(main)
        # an error raised after work was enqueued (a layout refused, an undersized feature table,
        # ids out of range) still joins the streams back to the caller's before it propagates
        try:
            with torch.cuda.stream(main):
                mk("start", main)
                side.wait_stream(main)
                compact = self.compact_records and W == 3
                # the narrow payload forms: the consumers that read them are the layout fill and the
                # compact terminal windows (windows and delay are whole days: whole seconds)
                narrow = None
                if self.narrow_payloads and compact and half.walk and not half.scan:
                    narrow = True if self.narrow_amounts else _lib.FDX_NARROW_TS
                # the id range checks ride on the re-keys' first histogram pass (bad counts), read once
                # everything is enqueued (out-of-range ids cannot make the re-keys write out of bounds)
                bad = ar("bad", 2, torch.int32) if validate else None
                th0 = None
                # the terminal re-key's first histogram pass (+ scan, + the terminal id-range count) on
                # the side stream at the step's start, beside the customer re-key, instead of after it
                # on the critical chain (fdx_rekey_hist0 / fdx_rekey_payload's hist0_d)
                # (overlapped mode only: on one stream it would just run first, and the per-stage
                # times bench.py takes in that mode would book it to the customer re-key)
                if overlap:
                    with torch.cuda.stream(side):
                        th0 = ops.rekey_hist0(terminal, n_terminals, side, bad=bad[1:2] if validate else None,
                                              alloc=ar.scope("th0"))
                        if validate:  # (the count's copy here too, off the terminal chain)
                            rc_t = ops.KeyRangeCheck.from_count(bad[1:2], n_terminals, "terminal ids", side)
                # customer half first (the critical path)
                if self.table_in_place and isinstance(rows_out, ops.FeatureTable) and half.walk and not half.scan \
                        and self.forest.in_table_ok(W, rows_out):
                    half.table = rows_out
                half.rekey(customer, n_customers, ts_ns, amount, bad[0:1] if validate else None, narrow=narrow)
                # (an ops.Narrow each, or None: which form that re-key's columns took; read by tests and tools)
                self.narrow_flags = [half.nflag, None]
                side.wait_stream(main)  # the terminal half waits for the re-key, not for the plan
                # the walk's layout plan goes right behind the re-key; its slot count is read only
                # after the terminal half is enqueued (no host wait between the two)
                half.plan()
                # terminal half (side stream): the re-key carries ts (and TX_FRAUD in bit 31 of the
                # perm); the records come out in input row order, read by the row assembly through irow.
                # Allocated under the side stream's context, so that the caching allocator hands
                # these buffers to nothing on the main stream while the side stream still uses them.
                with torch.cuda.stream(side):
                    mk("start", side)
                    tperm, tseg, tgts, _, *tnf = ops.rekey_payload(terminal, n_terminals, ts_ns, flag=fraud, stream=side,
                                                                   bad=bad[1:2] if validate and th0 is None else None,
                                                                   alloc=ar.scope("term", ("rekey_ws",)), hist0=th0,
                                                                   narrow=narrow)
                    if validate:
                        half.checks.append(rc_t if th0 is not None else
                                           ops.KeyRangeCheck.from_count(bad[1:2], n_terminals, "terminal ids", side))
                    mk("rekey_terminal", side)
                    self.narrow_flags[1] = tnf[0] if tnf else None
                    if compact:
                        trec = ops.terminal_windows_compact(tgts, tseg, rows=tperm, delay_days=self.delay_days,
                                                            windows_days=self.windows_days, stream=side,
                                                            alloc=ar.scope("trec"), narrow=tnf[0] if tnf else None)
                    else:
                        trec = ops.terminal_windows_grouped(tgts, tseg, rows=tperm, delay_days=self.delay_days,
                                                            windows_days=self.windows_days, stream=side)
                    mk("terminal_windows", side)
                for t in (ts_ns, customer, terminal, fraud) + ((bad,) if validate else ()):
                    t.record_stream(side)  # inputs in use on the side stream
                lay, inb, isum = half.windows()
                ws = self._forest_ws(lay.n_slots, ws, amount.device)
                # the assembly and the forest run on the stream that finishes its half LAST -- the
                # terminal half since round 5's reorder (it ends ~0.3 ms after the walk,
                # profiles/r05br_step_timeline.txt) -- so that no cross-stream wait (~20 us) sits
                # on the critical path; the workspace's NaN flag is cleared here, off it (5 us)
                if overlap:
                    ops.forest_clear_flag(self.forest, lay.n_slots, ws, main)
                    side.wait_stream(main)
                    for t in (lay.its, lay.iamt, lay.irow, inb, isum, ws, proba, amount) + \
                            ((rows_out.buf,) if rows_out is not None else ()):
                        t.record_stream(side)
                with torch.cuda.stream(side):
                    # (half.table: inb / isum / lay.irow are views of rows_out's columns, isum the averages)
                    ops.forest_prepare_grouped(self.forest, self.flags_mode, lay.its, lay.iamt, inb, isum, lay.irow,
                                               None, trec, ws, side, n=lay.n_slots, val_is_sum=half.table is None,
                                               term_compact=compact, rows_out=rows_out, flag_cleared=overlap,
                                               index64=bool(self.assembly_index64),
                                               cust_in_table=half.table is not None)
                    mk("assemble_rows", side)
                    ops.forest_traverse_perm(self.forest, lay.n_slots, ws, proba, lay.irow, side)
                    mk("forest_traverse", side)
                for c in half.checks:  # read once everything is enqueued (the counts ran in the re-keys)
                    c.check()
        finally:
            if main is not caller:
                main.wait_stream(side)
                caller.wait_stream(main)
        return proba

    def _forest_ws(self, n_rows, ws, device):
        need = self.forest.workspace_size(n_rows)
        if ws is not None and ws.numel() >= need:
            return ws
        if self._ws is None or self._ws.numel() < need:
            self._ws = ops.workspace(need, device)
        return self._ws


class _CustomerHalf:
    """The customer half of one scoring step, FraudPipeline.run_fused's and ShardedPipeline.run's
    alike: rekey(), plan(), windows() enqueue on `stream` in that order, and between them the caller
    enqueues its other half (the terminal re-key and windows, or the exchange).  The intermediates
    live in an arena of the pipeline's own (ops.Arena): a repeated step allocates nothing; its
    buffers are reused by the next step, which the caller's stream joins order after every use.
    Buffer names: `prefix` + cust / plan / lay / walk (`shared`: see ops.Arena.scope).
    checks: the step's pending id-range checks (the caller may append its own and reads them once
    everything is enqueued)."""

    def __init__(self, pipe: FraudPipeline, device, stream, mark, prefix: str = "", shared=()):
        if pipe._arena is None or pipe._arena.device != device:
            pipe._arena = ops.Arena(device)
        self.pipe, self.arena, self.stream, self.mark, self.checks = pipe, pipe._arena, stream, mark, []
        self.scope = lambda name: pipe._arena.scope(prefix + name, shared)
        self.scan = pipe.avg_mode == "scan"
        # the two-kernel walk serves >= 3 windows; fewer use the one-pass ring kernel
        self.walk = len(pipe.windows_days) >= 3
        # an ops.FeatureTable whose cust_nb / cust_avg / row columns the walk and the layout fill write
        # in place (set by run_fused before rekey(); 3 windows, exact walk); None: buffers of the arena
        self.table = None

    def rekey(self, customer, n_customers: int, ts_ns, amount, bad=None, what: str = "customer ids", narrow=None):
        """The re-key carries ts and amount into grouped order (narrow: ops.rekey_payload's); bad
        (int32 [1] on the device, or None): its count of ids outside [0, n_customers)."""
        self.ts_ns, self.bad = ts_ns, (bad, n_customers, what)
        self.cperm, self.cseg, self.gts, self.gamt, *nf = ops.rekey_payload(
            customer, n_customers, ts_ns, amount, stream=self.stream, bad=bad, alloc=self.scope("cust"), narrow=narrow)
        self.mark("rekey_customer", self.stream)
        self.nflag = nf[0] if nf else None

    def plan(self):
        """The walk's layout plan, enqueued without a host wait (windows() reads its slot count)."""
        self.pending = ops.customer_layout_plan_async(self.cseg, len(self.pipe.windows_days), self.stream,
                                                      alloc=self.scope("plan")) if self.walk and not self.scan else None
        if self.bad[0] is not None:  # (its pinned copy behind the plan, not in front of it: up to 38 us)
            self.checks.append(ops.KeyRangeCheck.from_count(*self.bad, self.stream))

    def windows(self):
        """Layout (host-synchronising: the slot count) and windows -> (lay, nb, rolling sum), by slot;
        with self.table: views of its columns, lay.irow included, and the AVERAGE in the sum's place."""
        p, st, cseg, gts, gamt = self.pipe, self.stream, self.cseg, self.gts, self.gamt
        tbl = self.table if self.pending is not None else None
        try:
            if self.pending is not None:
                plan = self.pending.result(p.plan_spin_s)
                # the fill and the walk write into the table before the assembly sees it: the slot
                # count is checked here, before either is enqueued (the assembly's own error)
                if tbl is not None and tbl.cap < plan.n_slots:
                    raise ValueError(f"the feature table holds {tbl.cap} slots < {plan.n_slots}")
                lay = ops.customer_layout_fill(plan, cseg, self.cperm, gts, gamt,
                                               p.windows_days, st, alloc=self.scope("lay"), narrow=self.nflag,
                                               ts_base=self.ts_ns, irow=None if tbl is None else tbl.row_column())
            else:
                lay = ops.customer_layout(cseg, self.cperm, gts, gamt, len(p.windows_days), st, p._slots_hint,
                                          p.windows_days if self.walk else None, grouped=True)
        except _lib.FdxError:
            for c in self.checks:  # ids outside the range are the likelier cause: report them
                c.check()
            raise
        self.mark("customer_layout", st)
        p._slots_hint = lay.its.numel()
        p.last_slots = lay.n_slots
        if self.scan:  # the windows straight from the grouped rows into the layout's slots
            inb, isum = ops.customer_windows_scan(gts, gamt, cseg, p.windows_days, lay=lay, stream=st)
        elif self.walk:
            inb, isum = ops.customer_windows_walk(lay, cseg, st, alloc=self.scope("walk"), table=tbl)
        else:
            inb, isum = ops.customer_windows_interleaved(lay, cseg, p.windows_days, st)
        self.mark("customer_walk", st)
        return lay, inb, isum


def check_rows_out(rows_out, ts_ns: torch.Tensor) -> None:
    """rows_out of run_fused / ShardedPipeline.run, checked before anything is enqueued: an
    ops.FeatureRecords of >= n records or an ops.FeatureTable of >= n slots (the layout's slot
    count is >= n; its exact value is checked by the assembly, or -- table_in_place -- by the
    customer half before its layout fill writes into the table), on the inputs' device."""
    if rows_out is None:
        return
    if not isinstance(rows_out, (ops.FeatureRecords, ops.FeatureTable)):
        raise TypeError("rows_out must be an ops.FeatureRecords or an ops.FeatureTable")
    if rows_out.buf.device != ts_ns.device:
        raise ValueError("rows_out must be on the inputs' device")
    if rows_out.cap < ts_ns.numel():
        raise ValueError(f"rows_out holds {rows_out.cap} rows / slots < n = {ts_ns.numel()}")


def _to_caller_order(f: Features, tperm: torch.Tensor, stream) -> Features:
    """Outputs computed on time-sorted rows -> the caller's row order (tperm[j] = caller row
    of sorted row j).  Grouped outputs keep their order; only the perms are composed."""
    return Features(ops.scatter(f.weekend, tperm, stream=stream), ops.scatter(f.night, tperm, stream=stream),
                    ops.gather(tperm, f.cust_perm, stream), f.cust_seg, f.cust_nb, f.cust_avg,
                    ops.gather(tperm, f.term_perm, stream), f.term_seg, f.term_nb, f.term_risk)
