"""The retirement entry points (include/fdx.h, f-10) on tiny states against tests/retire_ref.py:
fdx_stream_retire_plan / fdx_stream_retire_apply through StreamState, fdx_keydir_remap through
KeyDirectory.  2,500 keys per half (the scan crosses the wave, the 256-thread block and 1,024),
rings of 8.  Every comparison is an equality of arrays or of snapshot bytes: after plan + apply
the state must be the state of a fresh stream fed the history without the retired keys' rows,
under the model's new ids."""
import ctypes

import numpy as np
import pytest
import torch

import retire_ref as M
import stream_label_ref as R
from fdx import _lib, ops
from fdx.streaming import KeyDirectory, StreamState

pytestmark = pytest.mark.gpu

K = 2500
DAY = R.DAY
PARAMS = [((1, 7, 30), 7), ((2, 5), 3)]
T_OLD, T_NEW = R.BASE, R.BASE + 100 * DAY     # the early rows; the rows only the survivors have
WATERMARK = T_NEW + 2 * DAY


def T(a, dt, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)


def dead_pattern(name):
    i = np.arange(K)
    return {"none": i < 0, "all": i >= 0, "first": i == 0, "last": i == K - 1, "alternating": i % 2 == 1,
            "run_255": (i >= 250) & (i < 262), "mixed": (i * 2654435761 % 7 < 3) | ((i >= 1000) & (i < 1100))}[name]


def history(dead_c, dead_t):
    """Three batches per half, one row per key each (amounts and labels vary by key and batch);
    the third, a hundred days on, only for the keys that stay.  -> per half a list of
    (ts, key, value) arrays."""
    out = []
    for h, dead in enumerate((dead_c, dead_t)):
        keys = np.arange(K)
        rows = []
        for b, (t0, who) in enumerate(((T_OLD, keys), (T_OLD + DAY, keys[::-1]), (T_NEW, keys[~dead]))):
            ts = t0 + (who * 7919 % 3600) * R.NS + b
            val = np.round((who * 37 + b * 11) % 1000 / 8.0, 3) if h == 0 else ((who + b) % 3 == 0).astype(np.uint8)
            rows.append((ts.astype(np.int64), who.astype(np.int32), val))
        out.append(rows)
    return out


def feed(st, hist, dev, id_of=(None, None)):
    """id_of[h]: old id -> new id (-1: the key's rows are left out), or None = as they are"""
    for h in range(2):
        for ts, key, val in hist[h]:
            if id_of[h] is not None:
                keep = id_of[h][key] >= 0
                ts, key, val = ts[keep], id_of[h][key[keep]], val[keep]
            if not len(ts):
                continue
            if h == 0:
                st.update(T(ts, torch.int64, dev), customer=T(key, torch.int32, dev), amount=T(val, torch.float64, dev),
                          X=torch.empty((len(ts), 3 + 4 * st.W), dtype=torch.float64, device=dev))
            else:
                st.update(T(ts, torch.int64, dev), terminal=T(key, torch.int32, dev), fraud=T(val, torch.uint8, dev),
                          term_records=torch.empty((len(ts), st.W), dtype=torch.int64, device=dev))
    st.check()


def new_state(windows, delay):
    return StreamState(K, K, windows, delay, customer_ring=8, terminal_ring=8, max_batch=K)


def snap(st):
    return bytes(st.snapshot().cpu().numpy())


@pytest.mark.parametrize("windows,delay", PARAMS)
@pytest.mark.parametrize("pattern", ["none", "all", "first", "last", "alternating", "run_255", "mixed"])
def test_plan_and_apply_equal_the_filtered_history(dev, pattern, windows, delay):
    dead_c, dead_t = dead_pattern(pattern), dead_pattern(pattern)[::-1].copy()
    hist = history(dead_c, dead_t)
    maps = [M.id_map(d) for d in (dead_c, dead_t)]
    want = new_state(windows, delay)
    feed(want, hist, dev, (maps[0][0], maps[1][0]))
    want = snap(want)
    if pattern == "all":
        assert want == snap(new_state(windows, delay))
    for chunk in (1, 7, 0):
        st = new_state(windows, delay)
        feed(st, hist, dev)
        before = snap(st)
        cmap, tmap, counts = st.retire_plan(WATERMARK)
        assert snap(st) == before                                  # the plan writes nothing
        np.testing.assert_array_equal(cmap.cpu().numpy(), maps[0][0])
        np.testing.assert_array_equal(tmap.cpu().numpy(), maps[1][0])
        assert counts == {"customers": {"kept": maps[0][1], "retired": int(dead_c.sum())},
                          "terminals": {"kept": maps[1][1], "retired": int(dead_t.sum())}}
        st.retire_apply(cmap, maps[0][1], tmap, maps[1][1], chunk_keys=chunk)
        assert snap(st) == want, chunk
        st.check()
    # the survivors go on as the filtered stream does: one more row per new id
    ts = np.full(K, WATERMARK + DAY, np.int64)
    ids = np.arange(K, dtype=np.int32)
    ref = new_state(windows, delay)
    feed(ref, hist, dev, (maps[0][0], maps[1][0]))
    for s in (st, ref):
        s.update(T(ts, torch.int64, dev), T(ids, torch.int32, dev), T(ids / 4.0, torch.float64, dev),
                 T(ids[::-1].copy(), torch.int32, dev), T(ids % 2, torch.uint8, dev))
    assert snap(st) == snap(ref)


@pytest.mark.parametrize("half", [0, 1])
def test_one_half_only(dev, half):
    windows, delay = PARAMS[half]
    dead = [dead_pattern("mixed"), dead_pattern("alternating")]
    hist = history(*dead)
    m, kept = M.id_map(dead[half])
    only = [None, None]
    only[half] = m
    want = new_state(windows, delay)
    feed(want, hist, dev, only)
    st = new_state(windows, delay)
    feed(st, hist, dev)
    maps = list(st.retire_plan(WATERMARK)[:2])
    np.testing.assert_array_equal(maps[half].cpu().numpy(), m)
    maps[1 - half] = None
    st.retire_apply(maps[0], kept, maps[1], kept, chunk_keys=7)
    assert snap(st) == snap(want)
    # a state without the other half: its map is None and the plan skips it
    lone = StreamState(K if half == 0 else 0, K if half == 1 else 0, windows, delay, 8, 8, max_batch=K)
    assert lone.retire_plan(WATERMARK)[1 - half] is None


def test_the_watermark_decides(dev):
    """The same state at three watermarks: a day before the survivors' horizon ends nothing more
    is retired; at last_ts + horizon (inclusive) everything is; an extreme one does not overflow."""
    windows, delay = PARAMS[0]
    hc, ht = M.horizons(windows, delay)
    st = new_state(windows, delay)
    hist = history(dead_pattern("alternating"), dead_pattern("first"))
    feed(st, hist, dev)
    c_last, t_last = hist[0][2][0], hist[1][2][0]          # the survivors' last rows
    for wm, want in ((int(c_last.min()) + hc - 1, (K // 2, K - 1)), (int(c_last.max()) + hc, (0, K - 1)),
                     (int(c_last.min()) + hc, (K // 2 - 1, K - 1)), (int(t_last.max()) + ht, (0, 0)),
                     (T_OLD, (K, K)), (-2 ** 63, (K, K)), (2 ** 63 - 1, (0, 0))):
        counts = st.retire_plan(wm)[2]
        assert (counts["customers"]["kept"], counts["terminals"]["kept"]) == want, wm


def test_refusals_write_nothing(dev):
    windows, delay = PARAMS[0]
    st = new_state(windows, delay)
    feed(st, history(dead_pattern("mixed"), dead_pattern("run_255")), dev)
    before = snap(st)
    cmap, tmap, counts = st.retire_plan(WATERMARK)
    ck, tk = counts["customers"]["kept"], counts["terminals"]["kept"]
    alive = np.flatnonzero(cmap.cpu().numpy() >= 0)
    swapped = cmap.clone()
    swapped[alive[3]], swapped[alive[4]] = cmap[alive[4]], cmap[alive[3]]      # not monotone
    gap = cmap.clone()
    gap[alive[-1]] += 1                                                        # not dense
    minus2 = cmap.clone()
    minus2[int(np.flatnonzero(cmap.cpu().numpy() < 0)[0])] = -2
    for bad_c, bad_ck, bad_t, bad_tk in ((swapped, ck, tmap, tk), (gap, ck, tmap, tk), (minus2, ck, tmap, tk),
                                         (cmap, ck - 1, tmap, tk), (cmap, ck, tmap, tk + 1), (cmap, ck, tmap, K + 1),
                                         (cmap, ck, swapped, ck)):
        with pytest.raises(_lib.FdxError) as e:
            st.retire_apply(bad_c, bad_ck, bad_t, bad_tk)
        assert not isinstance(e.value, _lib.FdxUnsupported)
        assert snap(st) == before
    L = _lib.load()
    need = L.fdx_stream_retire_workspace_size(st._h, 1)
    assert need < L.fdx_stream_retire_workspace_size(st._h, 7) < L.fdx_stream_retire_workspace_size(st._h, 0)
    ws = ops.workspace(need, dev)
    c4 = (ctypes.c_int64 * 4)()
    assert L.fdx_stream_retire_apply(st._h, ops._ptr(cmap), ck, ops._ptr(tmap), tk, ops._ptr(ws), need - 1, None) == -1
    assert L.fdx_stream_retire_plan(st._h, WATERMARK, ops._ptr(cmap), ops._ptr(tmap), c4, ops._ptr(ws), need - 1,
                                    None) == -1
    assert snap(st) == before
    # a status bit up: FDX_E_UNSUPPORTED from both, and the bit stays for the caller's status read
    st.update(T(np.array([WATERMARK]), torch.int64, dev), T(np.array([K]), torch.int32, dev),
              T(np.array([1.0]), torch.float64, dev), T(np.array([0]), torch.int32, dev),
              T(np.array([0]), torch.uint8, dev))
    with pytest.raises(_lib.FdxUnsupported, match="status bits"):
        st.retire_plan(WATERMARK)
    with pytest.raises(_lib.FdxUnsupported, match="status bits"):
        st.retire_apply(cmap, ck, tmap, tk)
    with pytest.raises(_lib.FdxUnsupported, match="outside the state's capacity"):
        st.check()
    # (the refused row's terminal half did land: terminal 0 has one more row; nothing else moved)
    st.retire_apply(cmap, ck, None, 0)
    ref = new_state(windows, delay)
    feed(ref, history(dead_pattern("mixed"), dead_pattern("run_255")), dev, (cmap.cpu().numpy(), None))
    ref.update(T(np.array([WATERMARK]), torch.int64, dev), terminal=T(np.array([0]), torch.int32, dev),
               fraud=T(np.array([0]), torch.uint8, dev), term_records=torch.empty((1, 3), dtype=torch.int64, device=dev))
    assert snap(st) == snap(ref)


def _check_directory(d, model, dev, probe):
    assert d.counts() == model.counts()
    np.testing.assert_array_equal(d.keys().cpu().numpy(), model.keys())
    got = d.map(T(probe, torch.int64, dev), insert=False).cpu().numpy()
    np.testing.assert_array_equal(got, model.map(probe, insert=False))


def test_keydir_remap_of_a_full_directory_with_garbage(dev):
    """Capacity 64, filled exactly by a batch that also brings 10 keys too many (they stay in the
    table as refused garbage); after the remap their slots are free and they can be held."""
    rng = np.random.default_rng(7)
    keys = rng.integers(-2 ** 62, 2 ** 62, 90)
    first = np.r_[keys[:74], keys[:20]]
    d, model = KeyDirectory(64, 256), M.DirModel(64)
    np.testing.assert_array_equal(d.map(T(first, torch.int64, dev)).cpu().numpy(), model.map(first))
    assert model.counts()["held"] == 64 and model.counts()["refused_full"] == 10
    dead = np.arange(64) % 3 == 1
    dead[[0, 63]] = True
    m, kept = M.id_map(dead)
    full = np.full(64, -1, np.int32)
    full[:64] = m
    d.remap(T(full, torch.int32, dev), kept)
    model.remap(full, kept)
    _check_directory(d, model, dev, keys)               # survivors hit, retired and garbage keys miss
    # retired keys that return, the former garbage and new keys: first-occurrence numbering, up to the capacity
    nxt = np.r_[keys[64:74], keys[[1, 0, 4]], keys[74:90], keys[:30]]
    np.testing.assert_array_equal(d.map(T(nxt, torch.int64, dev)).cpu().numpy(), model.map(nxt))
    _check_directory(d, model, dev, keys)
    assert model.counts()["held"] == 64


def test_keydir_remap_patterns_and_refusals(dev):
    rng = np.random.default_rng(8)
    keys = rng.integers(-2 ** 62, 2 ** 62, K + 200)
    for pattern in ("none", "all", "first", "last", "alternating", "run_255", "mixed"):
        d, model = KeyDirectory(K + 100, K + 200), M.DirModel(K + 100)
        d.map(T(keys[:K], torch.int64, dev))
        model.map(keys[:K])
        m, kept = M.id_map(dead_pattern(pattern))
        d.remap(T(m, torch.int32, dev), kept)           # a map over the keys held (shorter than the capacity)
        model.remap(m, kept)
        _check_directory(d, model, dev, keys[:K])
        nxt = np.r_[keys[K - 50:K + 200], keys[:300]][:K]
        np.testing.assert_array_equal(d.map(T(nxt, torch.int64, dev)).cpu().numpy(), model.map(nxt))
        _check_directory(d, model, dev, keys)
    d, model = KeyDirectory(K, K + 200), M.DirModel(K)
    d.map(T(keys[:K - 10], torch.int64, dev))
    model.map(keys[:K - 10])
    m, kept = M.id_map(dead_pattern("mixed")[:K - 10])
    swapped, gap = m.copy(), m.copy()
    alive = np.flatnonzero(m >= 0)
    swapped[alive[[5, 6]]] = m[alive[[6, 5]]]
    gap[alive[0]] = 1
    for bad, k in ((swapped, kept), (gap, kept), (m, kept + 1), (m, kept - 1), (m[:K - 11], kept), (m, -1)):
        with pytest.raises(_lib.FdxError):
            d.remap(T(bad, torch.int32, dev), k)
        _check_directory(d, model, dev, keys[:K])
    L = _lib.load()
    ws = ops.workspace(L.fdx_keydir_remap_workspace_size(d._h), dev)
    mt = T(m, torch.int32, dev)
    assert L.fdx_keydir_remap(d._h, ops._ptr(mt), mt.numel(), kept, ops._ptr(ws), ws.numel() - 1, None) == -1
    _check_directory(d, model, dev, keys[:K])
    # entries beyond the keys held are unused, whatever they say
    longer = np.r_[m, np.arange(10, dtype=np.int32)].astype(np.int32)
    d.remap(T(longer, torch.int32, dev), kept)
    model.remap(m, kept)
    _check_directory(d, model, dev, keys[:K])
