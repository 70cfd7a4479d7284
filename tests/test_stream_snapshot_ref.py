"""The snapshot model of tests/stream_snapshot_ref.py against the oracle, and the host-only
header parser fdx_stream_snapshot_info against the model's bytes (no GPU).

Stream [0, cut), snapshot, restore into other ring sizes, stream the rest: the features must
equal oracle.featurize_arrays over the whole table, for every stream_label_ref.PARAMS entry,
with the cut inside the 100-row tie run (1050) and at the first row after day 45.  Every
comparison is an equality."""
import ctypes

import numpy as np
import pytest

import stream_label_ref as R
import stream_snapshot_ref as S


@pytest.mark.parametrize("cut", S.cut_rows())
@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_model_continues_like_the_oracle(windows, delay, cut):
    n = len(R.table()["ts"])
    want = S.oracle_columns(windows, delay)
    head, snap = S.model_prefix(windows, delay, cut)
    np.testing.assert_array_equal(head, want[:cut])
    rings = [(512, 1024)] + ([(64, 64)] if (windows, delay) == R.PARAMS[1] else [])
    for cr, tr in rings:
        m = S.StateModel.from_snapshot(snap, customer_ring=cr, terminal_ring=tr)
        np.testing.assert_array_equal(S.feed(m, cut, n), want[cut:])
    d = S.decode(snap)
    assert S.encode(d) == snap
    if (windows, delay) == R.PARAMS[1]:
        assert max(d["max_live"]) < 32


def test_snapshot_drops_rows_and_rebases():
    windows, delay = R.PARAMS[1]
    cut = S.cut_rows()[1]
    d = S.decode(S.model_prefix(windows, delay, cut)[1])
    c = R.table()
    carried = sum(len(e) for _, e in d["terminals"])
    assert 0 < carried < cut                               # rows older than delay + the longest window left
    for half in ("customers", "terminals"):
        for key, (rec, ent) in enumerate(d[half]):
            assert rec[0] == len(ent)
            if half == "terminals":
                assert min(rec[2::2]) == 0 and (rec[0] >= 1) == bool(np.any(c["terminal"][:cut] == key))


def _info(b, nbytes=None):
    from fdx import _lib

    L = _lib.load()
    f = _lib.SnapshotInfo()
    rc = L.fdx_stream_snapshot_info(bytes(b[:512]), len(b) if nbytes is None else nbytes, ctypes.byref(f))
    return rc, f, L.fdx_last_error()


def test_header_parser_accepts_the_model_and_refuses_damage():
    windows, delay = R.PARAMS[0]
    snap = S.model_prefix(windows, delay, 1050)[1]
    rc, f, err = _info(snap)
    assert rc == 0, err
    d = S.decode(snap)
    assert (f.version, f.total_bytes, f.n_windows, f.delay_ns, f.flags_mode) == (1, len(snap), 3, 7 * R.DAY, 0)
    assert list(f.window_ns)[:3] == [w * R.DAY for w in windows] and list(f.window_ns)[3:] == [0] * 5
    assert (f.customer_ring, f.terminal_ring, f.customer_keys, f.terminal_keys) == (256, 256, 25, 40)
    assert f.customer_entries == sum(len(e) for _, e in d["customers"])
    assert f.terminal_entries == sum(len(e) for _, e in d["terminals"])
    assert (f.customer_max_live, f.terminal_max_live) == d["max_live"]
    assert list(f.label_counts) == [0] * 5
    assert list(f.section_offset) == sorted(f.section_offset) and f.section_offset[0] == 512

    def damaged(word, value):
        h = np.frombuffer(snap[:512], "<i8").copy()
        h[word] = value
        return h.tobytes() + snap[512:]

    h = np.frombuffer(snap[:512], "<i8")
    for what, (b, nbytes), msg in [
            ("magic", (damaged(S.H_MAGIC, S.MAGIC + 1), None), b"magic"),
            ("version 2", (damaged(S.H_VERSION, 2), None), b"version"),
            ("one byte short", (snap, len(snap) - 1), b"bytes"),
            ("section past the end", (damaged(S.H_OFF + 5, len(snap) + 16), None), b"section 5"),
            ("section offsets swapped", (damaged(S.H_OFF + 1, int(h[S.H_OFF + 2])), None), b"section 1"),
            ("n_windows 9", (damaged(S.H_WINDOWS, 9), None), b"n_windows"),
            ("n_windows 0", (damaged(S.H_WINDOWS, 0), None), b"n_windows"),
            ("less than a header", (snap[:511], None), b"header")]:
        rc, _, err = _info(b, nbytes)
        assert rc == -1 and msg in err, (what, err)
