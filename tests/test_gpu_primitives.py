"""The sort, scan and key primitives of csrc/fdx_rekey.hip, each through its C entry point against
plain numpy (primitives_ref.py), at the sizes around the 4,096-key tile and the 8-tile scatter
grid, at the key classes where a radix pass, a carry or a tail goes wrong, and on the inputs
include/fdx.h documents as safe.  Every output lies in a buffer pre-filled with 0x5A bytes with
spare elements behind it: an element the kernel did not write, or one it wrote past the end, fails.
Everything is compared exactly.  Reference calls: the regrouping of pandas'
groupby('CUSTOMER_ID') / sort_values('TX_DATETIME') / groupby('TERMINAL_ID')
(feature_transformation.ipynb:604, :1092-1093, :1497, :2435-2436)."""
import ctypes

import numpy as np
import pytest
import torch

import primitives_ref as R
from fdx import _lib, ops
from fdx._lib import FdxError

pytestmark = pytest.mark.gpu

FDX_E_INVALID, FDX_E_WORKSPACE = -1, -4
PAD = 16
P = ops._ptr


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def out_buf(n, dtype, dev, pad=PAD):
    """n + pad elements of 0x5A bytes"""
    esz = torch.empty((), dtype=dtype).element_size()
    return torch.full(((n + pad) * esz,), 0x5A, dtype=torch.uint8, device=dev).view(dtype)


def untouched(buf, n=0):
    """the elements from n on still hold their 0x5A bytes"""
    return bool((buf[n:].contiguous().view(torch.uint8) == 0x5A).all())


def filled(a, dtype, dev, pad=PAD):
    """the array followed by pad sentinel elements (an in-place operand)"""
    b = out_buf(len(a), dtype, dev, pad)
    b[:len(a)] = T(a, dtype, dev)
    return b


# ------------------------------------------------------------------ 1. exclusive scan
@pytest.mark.parametrize("kind", R.SCAN_KINDS)
def test_exclusive_scan_u32(dev, kind):
    """In place, m around the 4,096-word chunk, at 256 partials and at 257 (the second trip of
    k_scan_single's carry loop), sums that wrap; nothing behind the m words or behind
    fdx_exclusive_scan_u32_workspace_size(m) bytes of workspace is written."""
    L = _lib.load()
    rng = np.random.default_rng(R.SCAN_KINDS.index(kind))
    for m in R.SCAN_SIZES:
        x = R.scan_input(kind, m, rng)
        data = filled(x.view(np.int32), torch.int32, dev)
        wsb = L.fdx_exclusive_scan_u32_workspace_size(m)
        ws = torch.full((wsb + 4096,), 0x5A, dtype=torch.uint8, device=dev)
        assert L.fdx_exclusive_scan_u32(P(data), m, P(ws), ops._s()) == 0
        got = data[:m].cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(got, R.scan_ref(x), err_msg=f"m={m}")
        assert untouched(data, m) and untouched(ws, wsb), m


def test_exclusive_scan_u32_empty(dev):
    L = _lib.load()
    data, ws = out_buf(8, torch.int32, dev), out_buf(L.fdx_exclusive_scan_u32_workspace_size(0), torch.uint8, dev)
    assert L.fdx_exclusive_scan_u32(P(data), 0, P(ws), ops._s()) == 0
    torch.cuda.synchronize()
    assert untouched(data) and untouched(ws)


# ------------------------------------------------------------------ 2. 64-bit argsort
def _argsort(L, keys, dev, short=0):
    n = len(keys)
    kd = T(keys, torch.int64, dev)
    perm = out_buf(n, torch.int32, dev)
    wsb = L.fdx_argsort_i64_workspace_size(n)
    ws = ops.workspace(wsb, dev)
    rc = L.fdx_argsort_i64(P(kd), n, P(perm), P(ws), wsb - short, ops._s())
    return rc, perm


@pytest.mark.parametrize("kind", R.ARGSORT_KINDS)
def test_argsort_i64_classes(dev, kind):
    """Stable against np.argsort(kind='stable') at every tile-edge size; byte<p>: only pass p sees
    more than one digit, so the other seven have to keep its order."""
    L = _lib.load()
    rng = np.random.default_rng(R.ARGSORT_KINDS.index(kind))
    for n in R.N_EDGE:
        k = R.argsort_keys(kind, n, rng)
        rc, perm = _argsort(L, k, dev)
        assert rc == 0
        want = np.argsort(k, kind="stable")
        if kind == "equal":
            np.testing.assert_array_equal(want, np.arange(n))
        np.testing.assert_array_equal(perm[:n].cpu().numpy(), want, err_msg=f"n={n}")
        assert untouched(perm, n), n


def test_argsort_i64_workspace_one_byte_short(dev):
    L = _lib.load()
    for n in (1, 4097):
        rc, perm = _argsort(L, R.argsort_keys("full", n, np.random.default_rng(n)), dev, short=1)
        torch.cuda.synchronize()
        assert rc == FDX_E_WORKSPACE and untouched(perm)


# ------------------------------------------------------------------ 3. is-sorted
def _is_sorted(L, keys, dev):
    kd = T(keys, torch.int64, dev) if len(keys) else torch.zeros(1, dtype=torch.int64, device=dev)
    flag = out_buf(1, torch.int32, dev)  # garbage before the call
    assert L.fdx_is_sorted_i64(P(kd), len(keys), P(flag), ops._s()) == 0
    v = int(flag[0].item())
    assert v in (0, 1) and untouched(flag, 1)
    return v


def test_is_sorted_i64_small_and_ties(dev):
    L = _lib.load()
    e = np.zeros(0, np.int64)
    assert _is_sorted(L, e, dev) == 1
    assert _is_sorted(L, np.array([5], np.int64), dev) == 1
    assert _is_sorted(L, np.array([5, 5], np.int64), dev) == 1
    assert _is_sorted(L, np.array([5, 6], np.int64), dev) == 1
    assert _is_sorted(L, np.array([6, 5], np.int64), dev) == 0
    k = np.repeat(np.arange(-300, 300, dtype=np.int64), 3)  # equal neighbours everywhere
    assert _is_sorted(L, k, dev) == 1
    assert _is_sorted(L, np.array([-5, R.I64_MAX, R.I64_MIN, R.I64_MIN, 3], np.int64), dev) == 0
    assert _is_sorted(L, np.array([R.I64_MIN, R.I64_MIN, -1, 0, R.I64_MAX, R.I64_MAX], np.int64), dev) == 1


@pytest.mark.parametrize("n,where", [(1000, (1, 255, 256, 257, 999)),
                                     (524_288 + 300, (524_287, 524_288, 524_289, 524_288 + 299))])
def test_is_sorted_i64_single_descent(dev, n, where):
    """One descent, everything else increasing: at the block edges, and around the grid-stride wrap
    of 2,048 blocks x 256 threads."""
    L = _lib.load()
    base = np.arange(n, dtype=np.int64) * 10 - 12345
    assert _is_sorted(L, base, dev) == 1
    for i in where:
        k = base.copy()
        k[i] = k[i - 1] - 5
        assert np.count_nonzero(np.diff(k) < 0) == 1
        assert _is_sorted(L, k, dev) == 0, i


# ------------------------------------------------------------------ 4. dense ids
@pytest.mark.parametrize("kind", R.DENSE_KINDS)
def test_dense_ids_i64_classes(dev, kind):
    L = _lib.load()
    rng = np.random.default_rng(40 + R.DENSE_KINDS.index(kind))
    for n in R.N_EDGE:
        k = R.dense_keys(kind, n, rng)
        u, inv = np.unique(k, return_inverse=True)
        kd = T(k, torch.int64, dev)
        ids, nu = out_buf(n, torch.int32, dev), out_buf(1, torch.int64, dev)
        wsb = L.fdx_dense_ids_i64_workspace_size(n)
        ws = ops.workspace(wsb, dev)
        assert L.fdx_dense_ids_i64(P(kd), n, P(ids), P(nu), P(ws), wsb, ops._s()) == 0
        np.testing.assert_array_equal(ids[:n].cpu().numpy(), inv.reshape(-1), err_msg=f"n={n}")
        assert int(nu[0].item()) == len(u) and untouched(ids, n) and untouched(nu, 1), n
        if kind == "equal":
            assert len(u) == 1
        if kind == "distinct":
            assert len(u) == n


# ------------------------------------------------------------------ 5. re-key digit plans
def _rekey_both(L, keys, bits, dev, rng):
    """fdx_rekey and fdx_rekey_payload (two payloads, the packed flag, bad_d, sorted keys; no
    offsets) over the same keys -> (perm, sorted keys), (perm, sorted keys, pay0, pay1, bad)."""
    n, n_keys = len(keys), 1 << bits
    kd = T(keys, torch.int32, dev)
    perm, sk = out_buf(n, torch.int32, dev), out_buf(n, torch.int32, dev)
    ws = ops.workspace(L.fdx_rekey_workspace_size(n, bits), dev)
    ops.check(L.fdx_rekey(P(kd), n, bits, n_keys, P(perm), P(sk), None, P(ws), ws.numel(), ops._s()), "fdx_rekey")
    pay0 = rng.integers(R.I64_MIN, R.I64_MAX, n, dtype=np.int64, endpoint=True)
    pay1 = rng.integers(R.I64_MIN, R.I64_MAX, n, dtype=np.int64, endpoint=True)  # any 64 bits (NaN payloads too)
    flag = rng.choice(np.array([0, 0, 1, 2, 255], np.uint8), n)
    d0, d1, fl = T(pay0, torch.int64, dev), T(pay1, torch.int64, dev), T(flag, torch.uint8, dev)
    perm2, sk2 = out_buf(n, torch.int32, dev), out_buf(n, torch.int32, dev)
    o0, o1, bad = out_buf(n, torch.int64, dev), out_buf(n, torch.int64, dev), out_buf(1, torch.int32, dev)
    assert sk2.data_ptr() % 16 == 0
    opts = _lib.RekeyPayloadOpts(bad_d=P(bad), sorted_keys_d=P(sk2))
    ws2 = ops.workspace(L.fdx_rekey_payload_workspace_size(n, bits, 2), dev)
    ops.check(L.fdx_rekey_payload(P(kd), n, bits, n_keys, P(fl), P(d0), P(d1), P(perm2), None, P(o0), P(o1),
                                  ctypes.byref(opts), P(ws2), ws2.numel(), ops._s()), "fdx_rekey_payload")
    torch.cuda.synchronize()
    for b, m in ((perm, n), (sk, n), (perm2, n), (sk2, n), (o0, n), (o1, n), (bad, 1)):
        assert untouched(b, m)
    c = lambda t: t[:n].cpu().numpy()  # noqa: E731
    return (c(perm), c(sk)), (c(perm2), c(sk2), c(o0), c(o1), int(bad[0].item())), (pay0, pay1, flag)


@pytest.mark.parametrize("bits", R.NEW_KEY_BITS)
def test_rekey_digit_plans(dev, bits):
    """Key widths whose (passes, 9-bit passes) no other test takes -- two and three 9-bit passes,
    an 8-bit pass after them, a fourth pass -- with n_keys = 2^bits and no offsets array."""
    L = _lib.load()
    rng = np.random.default_rng(bits)
    for n in (3 * 4096 + 17, 1):
        keys = R.rekey_keys(bits, n, rng)
        for k in ([keys] if n > 1 else [keys, np.zeros(1, np.int32)]):
            (perm, sk), (perm2, sk2, o0, o1, bad), (pay0, pay1, flag) = _rekey_both(L, k, bits, dev, rng)
            want = np.argsort(k, kind="stable")
            np.testing.assert_array_equal(perm, want)
            np.testing.assert_array_equal(sk, k[want])
            np.testing.assert_array_equal(perm2.view(np.uint32) & 0x7FFFFFFF, want)
            np.testing.assert_array_equal(perm2.view(np.uint32) >> 31, (flag[want] != 0).astype(np.uint32))
            np.testing.assert_array_equal(sk2, k[want])
            np.testing.assert_array_equal(o0, pay0[want])
            np.testing.assert_array_equal(o1, pay1[want])
            assert bad == 0


def test_rekey_31_bits_counts_negative_ids(dev):
    """fdx_rekey_payload's bad_d at the widest key: negative ids among ids of [0, 2^31)."""
    L = _lib.load()
    rng = np.random.default_rng(310)
    n = 3 * 4096 + 17
    k = R.with_negative_ids(R.rekey_keys(31, n, rng), rng)
    kd = T(k, torch.int32, dev)
    perm, bad = out_buf(n, torch.int32, dev), out_buf(1, torch.int32, dev)
    opts = _lib.RekeyPayloadOpts(bad_d=P(bad))
    ws = ops.workspace(L.fdx_rekey_payload_workspace_size(n, 31, 0), dev)
    ops.check(L.fdx_rekey_payload(P(kd), n, 31, 1 << 31, None, None, None, P(perm), None, None, None,
                                  ctypes.byref(opts), P(ws), ws.numel(), ops._s()), "fdx_rekey_payload")
    assert int(bad[0].item()) == int(np.count_nonzero(k < 0)) > 0
    assert untouched(perm, n) and untouched(bad, 1)


# ------------------------------------------------------------------ 6. segment offsets of sorted keys
def _seg_offsets(L, keys, n_keys, dev, misalign):
    n = len(keys)
    buf = out_buf(n + 4, torch.int32, dev)
    assert buf.data_ptr() % 16 == 0
    o = 1 if misalign else 0
    buf[o:o + n] = T(keys, torch.int32, dev)
    seg = out_buf(n_keys + 1, torch.int64, dev)
    ops.check(L.fdx_segment_offsets_sorted(buf.data_ptr() + 4 * o, n, n_keys, P(seg), ops._s()),
              "fdx_segment_offsets_sorted")
    got = seg[:n_keys + 1].cpu().numpy()
    assert untouched(seg, n_keys + 1)
    return got


@pytest.mark.parametrize("misalign", [False, True], ids=["k_seg_bounds4", "k_seg_bounds"])
def test_segment_offsets_sorted_patterns(dev, misalign):
    """Leading / trailing empty keys, a gap of 10,000 absent keys, one key value, n_keys = 1, every
    key once; n < 4 and every n % 4; the 16-byte-aligned kernel and the scalar one."""
    L = _lib.load()
    rng = np.random.default_rng(60 + misalign)
    for n in R.SEG_SIZES:
        for name in R.SEG_PATTERNS:
            k, nk = R.seg_pattern(name, n, rng)
            np.testing.assert_array_equal(_seg_offsets(L, k, nk, dev, misalign), R.seg_off_ref(k, nk),
                                          err_msg=f"{name} n={n}")


@pytest.mark.parametrize("misalign", [False, True], ids=["k_seg_bounds4", "k_seg_bounds"])
def test_segment_offsets_sorted_out_of_range_ids_stay_inside(dev, misalign):
    """include/fdx.h: keys outside [0, n_keys) never put an offset outside [0, n] -- ids >= n_keys
    and negative ids where an unsigned sort leaves them, behind the keys."""
    L = _lib.load()
    rng = np.random.default_rng(70 + misalign)
    for n in R.SEG_SIZES:
        for name in R.SEG_PATTERNS:
            k, nk = R.seg_pattern(name, n, rng)
            t = R.with_out_of_range_tail(k, nk)
            got = _seg_offsets(L, t, nk, dev, misalign)
            assert got.min() >= 0 and got.max() <= len(t), (name, n)


# ------------------------------------------------------------------ 7. key histogram -> offsets
def _key_segments(L, keys, n_keys, dev):
    n = len(keys)
    kd = T(keys, torch.int32, dev) if n else None
    seg, bad = out_buf(n_keys + 1, torch.int64, dev), out_buf(1, torch.int32, dev)
    wsb = L.fdx_key_segments_workspace_size(n_keys)
    ws = ops.workspace(wsb, dev)
    ops.check(L.fdx_key_segments(P(kd), n, n_keys, P(seg), P(bad), P(ws), wsb, ops._s()), "fdx_key_segments")
    got = seg[:n_keys + 1].cpu().numpy()
    assert untouched(seg, n_keys + 1) and untouched(bad, 1)
    return got, int(bad[0].item())


@pytest.mark.parametrize("n_keys", R.KEYSEG_N_KEYS)
def test_key_segments(dev, n_keys):
    """n_keys + 1 around the scan chunk and past 256 chunks; ids 0 and n_keys - 1 present;
    INT32_MIN, -1, n_keys and INT32_MAX counted and left out of the histogram; n = 0."""
    L = _lib.load()
    rng = np.random.default_rng(n_keys)
    k = R.keyseg_keys(n_keys, R.KEYSEG_N, rng)
    got, bad = _key_segments(L, k, n_keys, dev)
    np.testing.assert_array_equal(got, np.r_[0, np.cumsum(np.bincount(k, minlength=n_keys))])
    assert bad == 0
    b = R.keyseg_keys(n_keys, R.KEYSEG_N, rng, bad=True)
    got, bad = _key_segments(L, b, n_keys, dev)
    inside = b[(b >= 0) & (b.astype(np.int64) < n_keys)]
    np.testing.assert_array_equal(got, np.r_[0, np.cumsum(np.bincount(inside, minlength=n_keys))])
    assert bad == len(b) - len(inside) == 40
    got, bad = _key_segments(L, np.zeros(0, np.int32), n_keys, dev)
    assert not got.any() and bad == 0


# ------------------------------------------------------------------ 8. id-range count
def test_count_out_of_range(dev):
    L = _lib.load()
    rng = np.random.default_rng(80)
    for n in R.OOR_SIZES:
        for lo, hi in R.OOR_RANGES:
            for lay in R.OOR_LAYOUTS:
                k, _ = R.oor_keys(n, lo, hi, lay, rng)
                kd = T(k, torch.int32, dev) if n else torch.zeros(1, dtype=torch.int32, device=dev)
                cnt = out_buf(1, torch.int32, dev)  # garbage before the call: the call zeroes it
                ops.check(L.fdx_count_out_of_range(P(kd), n, lo, hi, P(cnt), ops._s()), "fdx_count_out_of_range")
                assert int(cnt[0].item()) == R.oor_count(k, lo, hi), (n, lo, hi, lay)
                assert untouched(cnt, 1)


def test_key_range_check_raises_exactly_when_the_count_is_nonzero(dev):
    rng = np.random.default_rng(81)
    for n in (1, 65, 100_003):
        for lay in R.OOR_LAYOUTS:
            good = rng.integers(0, R.OOR_N_KEYS, n).astype(np.int32)
            ops.KeyRangeCheck(T(good, torch.int32, dev), R.OOR_N_KEYS).check()
            k, pos = R.oor_keys(n, 0, R.OOR_N_KEYS, lay, rng)
            with pytest.raises(FdxError, match=f"^{len(pos)} keys outside"):
                ops.KeyRangeCheck(T(k, torch.int32, dev), R.OOR_N_KEYS).check()
            one = good.copy()
            one[n // 2] = R.OOR_N_KEYS  # the first id past the range, once
            with pytest.raises(FdxError, match="^1 keys outside"):
                ops.KeyRangeCheck(T(one, torch.int32, dev), R.OOR_N_KEYS).check()


# ------------------------------------------------------------------ 9. key map
def _key_map(L, kd, n, op, param, dev):
    out = out_buf(n, torch.int32, dev)
    rc = L.fdx_key_map(P(kd), n, op, param, P(out), ops._s())
    torch.cuda.synchronize()
    return rc, out


def test_key_map(dev):
    L = _lib.load()
    rng = np.random.default_rng(90)
    n = 4097
    k = rng.integers(0, 1 << 31, n).astype(np.int32)
    k[:4] = [0, 1, R.I32_MAX, R.I32_MAX - 1]
    kd = T(k, torch.int32, dev)
    for param in (1, 2, 3, 7, 8, 1 << 30):
        rc, mod = _key_map(L, kd, n, _lib.FDX_KEY_MOD, param, dev)
        rc2, div = _key_map(L, kd, n, _lib.FDX_KEY_DIV, param, dev)
        assert rc == 0 and rc2 == 0 and untouched(mod, n) and untouched(div, n)
        m, d = mod[:n].cpu().numpy(), div[:n].cpu().numpy()
        np.testing.assert_array_equal(m, k % param)
        np.testing.assert_array_equal(d, k // param)
        np.testing.assert_array_equal(m.astype(np.int64) + param * d.astype(np.int64), k)
    small = (k >> 1).astype(np.int32)  # [0, 2^30): key - param stays an int32
    sd = T(small, torch.int32, dev)
    for param in (1, 12_345, (1 << 30) - 1, -1, -54_321, -(1 << 30)):
        rc, sub = _key_map(L, sd, n, _lib.FDX_KEY_SUB, param, dev)
        assert rc == 0 and untouched(sub, n)
        np.testing.assert_array_equal(sub[:n].cpu().numpy().astype(np.int64), small.astype(np.int64) - param)
    for op, param in ((_lib.FDX_KEY_MOD, 0), (_lib.FDX_KEY_DIV, 0), (_lib.FDX_KEY_MOD, -3), (3, 5), (-1, 5)):
        rc, out = _key_map(L, kd, n, op, param, dev)
        assert rc == FDX_E_INVALID and untouched(out), (op, param)


# ------------------------------------------------------------------ 10. permutation ops
@pytest.mark.parametrize("elem", [1, 2, 4, 8])
def test_gather_scatter_invert(dev, elem):
    L = _lib.load()
    rng = np.random.default_rng(100 + elem)
    npdt, tdt = {1: (np.uint8, torch.uint8), 2: (np.int16, torch.int16), 4: (np.int32, torch.int32),
                 8: (np.int64, torch.int64)}[elem]
    for n in R.N_EDGE:
        x = rng.integers(0, 256, n * elem, dtype=np.uint8).view(npdt)
        p = rng.permutation(n).astype(np.int32)
        xd, pd = T(x, tdt, dev), T(p, torch.int32, dev)
        g, s, back, inv = (out_buf(n, tdt, dev), out_buf(n, tdt, dev), out_buf(n, tdt, dev),
                           out_buf(n, torch.int32, dev))
        assert L.fdx_gather(P(xd), elem, P(pd), n, P(g), ops._s()) == 0
        assert L.fdx_scatter(P(xd), elem, P(pd), n, P(s), ops._s()) == 0
        assert L.fdx_scatter(P(g), elem, P(pd), n, P(back), ops._s()) == 0  # scatter(gather(x, p), p) == x
        assert L.fdx_invert_perm(P(pd), n, P(inv), ops._s()) == 0
        np.testing.assert_array_equal(g[:n].cpu().numpy(), x[p], err_msg=f"n={n}")
        want = np.empty_like(x)
        want[p] = x
        np.testing.assert_array_equal(s[:n].cpu().numpy(), want, err_msg=f"n={n}")
        np.testing.assert_array_equal(back[:n].cpu().numpy(), x, err_msg=f"n={n}")
        winv = np.empty(n, np.int32)
        winv[p] = np.arange(n, dtype=np.int32)
        np.testing.assert_array_equal(inv[:n].cpu().numpy(), winv, err_msg=f"n={n}")
        for b in (g, s, back, inv):
            assert untouched(b, n), n


def test_gather_scatter_refuse_three_byte_elements(dev):
    L = _lib.load()
    n = 257
    xd, pd = torch.zeros(3 * n, dtype=torch.uint8, device=dev), T(np.arange(n, dtype=np.int32), torch.int32, dev)
    for fn in (L.fdx_gather, L.fdx_scatter):
        out = out_buf(3 * n, torch.uint8, dev)
        assert fn(P(xd), 3, P(pd), n, P(out), ops._s()) == FDX_E_INVALID
        torch.cuda.synchronize()
        assert untouched(out)


# ------------------------------------------------------------------ 11. the multi-GPU exchange records
def test_exchange_pack_unpack(dev):
    L = _lib.load()
    rng = np.random.default_rng(110)
    n = 4099
    ts = rng.integers(R.I64_MIN, R.I64_MAX, n, dtype=np.int64, endpoint=True)
    ts[:5] = [R.I64_MIN, R.I64_MAX, -1, 0, 1]
    term = rng.integers(0, 1 << 31, n).astype(np.int32)
    term[:3] = [0, R.I32_MAX, 1]
    fraud = rng.choice(np.array([0, 1, 2, 255], np.uint8), n)
    fraud[:4] = [255, 2, 1, 0]
    perm = rng.permutation(n).astype(np.int32)
    rec = out_buf(2 * n, torch.int64, dev)
    tsd, termd, frd, pd = (T(ts, torch.int64, dev), T(term, torch.int32, dev), T(fraud, torch.uint8, dev),
                           T(perm, torch.int32, dev))
    ops.check(L.fdx_exchange_pack(P(tsd), P(termd), P(frd), P(pd), n, P(rec), ops._s()), "fdx_exchange_pack")
    want = R.exchange_pack_ref(ts, term, fraud, perm)
    np.testing.assert_array_equal(rec[:2 * n].cpu().numpy().reshape(n, 2), want)
    assert untouched(rec, 2 * n)
    for world in (1, 3, 8):
        ots, oterm, ofr = out_buf(n, torch.int64, dev), out_buf(n, torch.int32, dev), out_buf(n, torch.uint8, dev)
        ops.check(L.fdx_exchange_unpack(P(rec), n, world, P(ots), P(oterm), P(ofr), ops._s()), "fdx_exchange_unpack")
        wts, wterm, wfr = R.exchange_unpack_ref(want, world)
        np.testing.assert_array_equal(ots[:n].cpu().numpy(), wts)
        np.testing.assert_array_equal(oterm[:n].cpu().numpy(), wterm)
        np.testing.assert_array_equal(ofr[:n].cpu().numpy(), wfr)
        np.testing.assert_array_equal(wterm, term[perm] // world)
        assert untouched(ots, n) and untouched(oterm, n) and untouched(ofr, n)


@pytest.mark.parametrize("W", [1, 3, 8])
def test_reply_assemble(dev, W):
    """ld = width + 3 and col0 = 3 + 2W: the padding and the other columns keep their bytes; NB = 0
    gives 0.0, FRAUD = NB gives 1.0, NB = 2^21 with FRAUD = 1 the exact IEEE quotient."""
    L = _lib.load()
    rng = np.random.default_rng(120 + W)
    n, width = 4099, 3 + 4 * W
    ld, col0 = width + 3, 3 + 2 * W
    nb = rng.integers(0, 41, (W, n)).astype(np.int32)
    fr = (rng.random((W, n)) * (nb + 1)).astype(np.int32)
    nb[:, 0], fr[:, 0] = 0, 0
    nb[:, 1], fr[:, 1] = 17, 17
    nb[:, 2], fr[:, 2] = 1 << 21, 1
    nb[:, 3], fr[:, 3] = R.I32_MAX, 3
    rec = R.count_records(nb, fr)
    perm = rng.permutation(n).astype(np.int32)
    X = out_buf(n * ld, torch.float64, dev)
    recd, pd = T(rec, torch.int64, dev), T(perm, torch.int32, dev)
    ops.check(L.fdx_reply_assemble(P(recd), P(pd), n, W, P(X), ld, col0, ops._s()), "fdx_reply_assemble")
    before = np.frombuffer(b"\x5a" * 8 * n * ld, np.float64).reshape(n, ld)
    want = R.reply_assemble_ref(before, rec, perm, col0)
    got = X[:n * ld].cpu().numpy().reshape(n, ld)
    np.testing.assert_array_equal(got.view(np.int64), want.view(np.int64))
    assert untouched(X, n * ld)
    assert got[perm[0], col0 + 1] == 0.0 and got[perm[1], col0 + 1] == 1.0 and got[perm[2], col0 + 1] == 1.0 / (1 << 21)
    assert L.fdx_reply_assemble(P(recd), P(pd), n, W, P(X), ld, ld - 2 * W + 1, ops._s()) == FDX_E_INVALID
