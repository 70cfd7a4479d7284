"""The narrow payload re-key (fdx_rekey_payload with narrow_flag_d): ts as int32 seconds relative to row 0
and amount as int32 cents through the radix passes whenever every value has that form exactly,
decided on the device inside the first pass, with the 8-byte passes as the fallback.

Every case runs the narrow call and the plain one; perm, seg_off and the grouped columns must be
bit-equal to each other and to numpy's stable argsort, in the customer form (ts + amount) and
the terminal form (ts, TX_FRAUD packed in bit 31 of perm) -- and the customer form with the
timestamps alone tried (the amounts stay 8 bytes) -- for one-, two- (8 + 8, 9 + 8 bit) and
three-pass digit schedules, full tiles plus a ragged tail, n = 1 and n = 64, with and without the
first digit table computed ahead.  A numpy model of the two predicates (checked on the CPU below) fixes which
inputs must fall back, and the device flag is read back: a silent fallback on exact data would
hide the kernels under test, a narrow run on inexact data would be wrong."""
import numpy as np
import pytest
import torch

from fdx import _lib, ops

NS = 10**9
TILE = 4096
N_BIG = 3 * TILE + 777
T0 = 1_522_540_800 * NS  # 2018-04-01, the generator's first day


# ------------------------------------------------------------------ the predicates, in numpy
def ts_exact(ts):
    """(ts - ts[0]) a whole number of seconds that fits int32 -- per row (Python ints: no wrap)"""
    d = [int(t) - int(ts[0]) for t in ts]
    return np.array([x % NS == 0 and -2**31 <= x // NS < 2**31 for x in d], bool)


def cents_exact(a):
    """c = rint(a * 100) with |c| < 2^31 and (double)c / 100.0 bit-equal to a"""
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.rint(a * 100.0)
        fits = np.abs(c) < 2.0**31
    ci = np.where(fits, c, 0.0).astype(np.int32)
    back = ci.astype(np.float64) / 100.0
    return fits & (back.view(np.int64) == a.view(np.int64))


def _base(n, seed):
    rng = np.random.default_rng(seed)
    ts = T0 + np.sort(rng.integers(0, 183 * 86_400, n)).astype(np.int64) * NS
    amt = np.rint(rng.uniform(-50, 500, n) * 100.0) / 100.0
    amt[0] = 0.0
    fraud = (rng.random(n) < 0.3).astype(np.uint8)
    return ts, amt, fraud


# name -> (edit(ts, amt, n, rng) in place, windows in ns); the row that is edited is the only
# inexact one of its case
def _set(col, where, value):
    def f(ts, amt, n, rng):
        (ts if col == "ts" else amt)[where(n)] = value(ts) if callable(value) else value
    return f


def _shuffle(ts, amt, n, rng):
    ts[:] = ts[rng.permutation(n)]


first, last = (lambda n: min(5, n - 1)), (lambda n: n - 1)
DAYS = (86_400 * NS, 7 * 86_400 * NS)
CASES = {
    "exact": (lambda *a: None, DAYS),
    "subsecond_first_tile": (_set("ts", first, lambda ts: ts[0] + 5 * NS + 1), DAYS),
    "subsecond_last_partial_tile": (_set("ts", last, lambda ts: ts[0] + 7 * NS - 1), DAYS),
    "span_2p31_seconds": (_set("ts", last, lambda ts: ts[0] + 2**31 * NS), DAYS),
    "span_2p31_minus_1_seconds": (_set("ts", last, lambda ts: ts[0] + (2**31 - 1) * NS), DAYS),
    "span_minus_2p31_seconds": (_set("ts", last, lambda ts: ts[0] - 2**31 * NS), DAYS),
    "shuffled_ts": (_shuffle, DAYS),
    "amount_0.1+0.2": (_set("amt", last, 0.1 + 0.2), DAYS),
    "amount_nan": (_set("amt", first, np.nan), DAYS),
    "amount_inf": (_set("amt", last, np.inf), DAYS),
    "amount_minus_zero": (_set("amt", first, -0.0), DAYS),
    "amount_cents_overflow": (_set("amt", last, 3e7 + 0.01), DAYS),
    "amount_denormal": (_set("amt", first, 1e-320), DAYS),
    "window_1.5s": (lambda *a: None, (1_500_000_000,)),
}
# what the cases must do at N_BIG rows, whatever the model says (the model is checked against it)
MUST_NARROW = {"exact", "span_2p31_minus_1_seconds", "span_minus_2p31_seconds", "shuffled_ts"}


def _case(name, n, seed):
    ts, amt, fraud = _base(n, seed)
    edit, windows = CASES[name]
    edit(ts, amt, n, np.random.default_rng(seed + 1))
    return ts, amt, fraud, windows


def _windows_whole(windows):
    return all(w % NS == 0 for w in windows)


def test_predicate_model_on_the_case_inputs():
    """The numpy model on the same inputs the GPU tests use: which cases have an exact narrow
    form (no GPU)."""
    for name in CASES:
        ts, amt, _, windows = _case(name, N_BIG, 11)
        t_ok, a_ok = ts_exact(ts), cents_exact(amt)
        narrow = bool(t_ok.all() and a_ok.all() and _windows_whole(windows))
        assert narrow == (name in MUST_NARROW), name
        if name.startswith("amount_"):
            assert t_ok.all() and int((~a_ok).sum()) == 1, name
        if name.startswith(("subsecond", "span_2p31_seconds")):
            assert a_ok.all() and int((~t_ok).sum()) == 1, name
    # the model itself: round trips and the rejected values
    assert cents_exact(np.array([0.0, 12.34, -7.01, 21474836.47, -21474836.47])).all()
    assert not cents_exact(np.array([0.1 + 0.2, np.nan, np.inf, -np.inf, -0.0, 3e7 + 0.01, 1e-320,
                                     21474836.48, 0.005])).any()
    assert ts_exact(np.array([5, 5 + NS, 5 - 3 * NS, 5 + (2**31 - 1) * NS, 5 - 2**31 * NS])).all()
    assert list(ts_exact(np.array([0, 1, NS + 1, 2**31 * NS, -(2**31 + 1) * NS]))) == [True] + [False] * 4


def T(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("ahead", [False, True])
@pytest.mark.parametrize("n", [N_BIG, 1, 64])
# 9 bits: one pass (the converting pass writes the outputs; its wide fallback is the returning launch);
# 8 + 8 and 9 + 8 bits: two passes; 8 + 8 + 8 bits: three (the narrow streams ping-pong in the workspace)
@pytest.mark.parametrize("n_keys", [300, 1 << 16, 1 << 17, 1 << 19])
def test_rekey_narrow_equals_wide(dev, n_keys, n, ahead):
    for name in CASES:
        ts, amt, fraud, windows = _case(name, n, 11)
        rng = np.random.default_rng(n + n_keys)
        keys = rng.integers(0, n_keys, n).astype(np.int32)
        keys[: n // 2] %= 300  # segments of several rows as well as single ones
        ref = np.argsort(keys, kind="stable")
        seg_ref = np.r_[0, np.cumsum(np.bincount(keys, minlength=n_keys))]
        allow = ops.narrow_windows_ok(windows)
        assert allow == _windows_whole(windows)
        kd, tsd, amd, frd = (T(keys, torch.int32, dev), T(ts, torch.int64, dev), T(amt, torch.float64, dev),
                             T(fraud, torch.uint8, dev))
        # (form, payloads, flag, the columns tried, must the narrow form hold)
        both = _lib.FDX_NARROW_TS | _lib.FDX_NARROW_AMOUNT
        forms = (("customer", (tsd, amd), None, True, allow and ts_exact(ts).all() and cents_exact(amt).all()),
                 ("customer_ts_only", (tsd, amd), None, _lib.FDX_NARROW_TS, allow and ts_exact(ts).all()),
                 ("terminal", (tsd,), frd, True, allow and ts_exact(ts).all()))
        for form, pay, fl, try_, want_narrow in forms:
            what = f"{name} {form} n={n} n_keys={n_keys} ahead={ahead}"
            if n == N_BIG and form == "customer":
                assert bool(want_narrow) == (name in MUST_NARROW), what
            out = {}
            for mode in ("wide", "narrow"):
                bad = None if ahead else torch.full((1,), 9, dtype=torch.int32, device=dev)
                h = ops.rekey_hist0(kd, n_keys) if ahead else None
                r = ops.rekey_payload(kd, n_keys, *pay, flag=fl, bad=bad, hist0=h,
                                      narrow=None if mode == "wide" else (try_ if allow else False))
                if bad is not None:
                    assert int(bad.item()) == 0, what
                out[mode] = r
            perm, seg, o0, o1, nflag = out["narrow"]
            assert nflag.mask == (0 if not allow else both if form == "customer" else _lib.FDX_NARROW_TS), what
            # the branch actually taken
            assert nflag.holds() == bool(want_narrow), what
            if want_narrow:  # the 4-byte streams themselves
                np.testing.assert_array_equal(o0.view(torch.int32)[:n].cpu().numpy(),
                                              ((ts[ref] - ts[0]) // NS).astype(np.int32), err_msg=what)
                if form == "customer":
                    np.testing.assert_array_equal(o1.view(torch.int32)[:n].cpu().numpy(),
                                                  np.rint(amt[ref] * 100.0).astype(np.int32), err_msg=what)
            g0 = ops.narrow_unpack(o0, nflag, tsd).cpu().numpy()
            pm = perm.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
            np.testing.assert_array_equal(pm & 0x7FFFFFFF, ref, err_msg=what)
            np.testing.assert_array_equal(pm >> 31, 0 if fl is None else fraud[ref], err_msg=what)
            np.testing.assert_array_equal(seg.cpu().numpy(), seg_ref, err_msg=what)
            np.testing.assert_array_equal(g0, ts[ref], err_msg=what)
            wp, wseg, w0, w1 = out["wide"]
            assert torch.equal(wp, perm) and torch.equal(wseg, seg), what
            np.testing.assert_array_equal(w0.cpu().numpy(), g0, err_msg=what)
            if o1 is not None:
                if form == "customer_ts_only":  # the amounts travel as they are, whatever the flag says
                    np.testing.assert_array_equal(o1.cpu().numpy().view(np.int64), amt[ref].view(np.int64), err_msg=what)
                g1 = ops.narrow_unpack(o1, nflag).cpu().numpy()
                np.testing.assert_array_equal(g1.view(np.int64), amt[ref].view(np.int64), err_msg=what)
                np.testing.assert_array_equal(w1.cpu().numpy().view(np.int64), g1.view(np.int64), err_msg=what)


@pytest.mark.gpu
def test_narrow_consumers_refuse_fractional_windows(dev):
    """The consumers compare seconds: with the narrow flag they take whole-second windows only
    (a caller with a 1.5 s window re-keys with narrow=False and uses the plain consumers)."""
    from fdx import _lib

    L = _lib.load()
    n = 8
    z64 = torch.zeros(5 * n, dtype=torch.int64, device=dev)
    z32 = torch.zeros(n, dtype=torch.int32, device=dev)
    seg = T(np.array([0, n]), torch.int64, dev)
    w = (ops.ctypes.c_int64 * 3)(NS, 1_500_000_000, 2 * NS)
    rc = L.fdx_terminal_windows_grouped(ops._ptr(z64), None, ops._ptr(z32), ops._ptr(seg), 1, n, NS, w, 3,
                                        _lib.FDX_TERM_COMPACT, None, None, ops._ptr(z64), ops._ptr(z32), ops._ptr(z32),
                                        None)
    assert rc == -1 and b"whole-second" in L.fdx_last_error()  # FDX_E_INVALID
    torch.cuda.synchronize()
