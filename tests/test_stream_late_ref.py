"""The semantics of late terminal rows (f-8), pinned without a GPU: the plain model of
tests/stream_late_ref.py equals the C oracle over the full history on an in-order stream, and
over the SORTED history on a stream whose rows arrive late by no more than the delay; the inputs
of the GPU tests meet their preconditions; the scripts at the smallest shapes give the counts
and status bits worked out by hand.  tests/test_gpu_stream_late.py holds the HIP kernel to the
same inputs, model and scripts."""
import numpy as np

import stream_late_ref as R


class ModelBackend:
    def __init__(self, **kw):
        self.m = R.StreamLateModel(**kw)

    def update(self, ts, term, fraud):
        return self.m.update(ts, term, fraud)

    def take_status(self):
        return self.m.take_status()

    def late_counts(self):
        return self.m.late_counts()

    def reset(self):
        self.m.reset()

    def restore(self):
        self.m.restore()


def test_in_order_stream_equals_oracle_over_full_history():
    h = R.history()
    n = len(h["ts"])
    want = R.oracle_columns(h["ts"], h["terminal"], h["fraud"])
    for lateness in (0.0, 7.0):                            # the switch changes nothing on an in-order stream
        be = ModelBackend(lateness_days=lateness)
        nb, fr = R.drive(be, h, np.arange(n), R.in_order_cuts(n))
        np.testing.assert_array_equal(R.columns(nb, fr), want)
        assert be.m.take_status() == 0 and be.m.late_counts() == {"late_rows": 0, "late_past_delay": 0}
    assert want[:, 0::2].max() >= 5 and want[:, 1::2].max() > 0


def test_lateness_within_delay_equals_oracle_over_sorted_history():
    h = R.history()
    k = R.disordered(6.0)
    # the input is what the GPU test needs: many rows behind their terminal's latest row, none by
    # more than 6 days, all along the stream; every ts distinct, so no late row ties with any row
    assert k["n_late"] > 40 and 2 * R.DAY < k["worst"] <= 6 * R.DAY and k["last_late"] > len(k["cuts"]) - 8
    assert len(np.unique(h["ts"])) == len(h["ts"]) and len(k["cuts"]) > 30
    be = ModelBackend(lateness_days=7.0)
    nb, fr = R.drive(be, h, k["order"], k["cuts"])
    np.testing.assert_array_equal(R.columns(nb, fr), R.oracle_columns(h["ts"], h["terminal"], h["fraud"]))
    assert be.m.take_status() == 0
    assert be.m.late_counts() == {"late_rows": k["n_late"], "late_past_delay": 0}
    # without the switch the same stream is refused
    off = ModelBackend(lateness_days=0.0)
    R.drive(off, h, k["order"], k["cuts"])
    assert off.m.take_status() == R.ST_ORDER


def test_lateness_past_delay_differs_only_until_the_late_rows_landed():
    h = R.history()
    k = R.disordered(10.0, lag_until_day=30)
    assert k["n_late"] > 40 and 7 * R.DAY < k["worst"] <= 10 * R.DAY
    be = ModelBackend(lateness_days=12.0)
    nb, fr = R.drive(be, h, k["order"], k["cuts"])
    got, want = R.columns(nb, fr), R.oracle_columns(h["ts"], h["terminal"], h["fraud"])
    assert be.m.take_status() == 0
    c = be.m.late_counts()
    assert c["late_rows"] == k["n_late"] and 0 < c["late_past_delay"] < c["late_rows"]
    after = k["order"][k["cuts"][k["last_late"] + 1]:]      # the rows of the batches after the last late arrival
    assert len(after) > 100
    np.testing.assert_array_equal(got[after], want[after])
    assert not np.array_equal(got, want)                    # some row was scored before a row its window holds came
    # and some late row was fraud: the fraud counts were corrected, not only the row counts
    late_fraud = [i for i in np.flatnonzero(k["lag"]) if h["fraud"][i]]
    assert len(late_fraud) > 5


def test_ring_of_8_script():
    be = ModelBackend(ring=8, lateness_days=40.0)
    assert R.ring8_script(be) == R.RING8_EXPECTED
    assert be.late_counts() == {"late_rows": 4, "late_past_delay": 4}   # days 65, 40, 30 and 39; not day 75


def test_ties_script_equals_oracle_where_every_row_has_landed():
    be = ModelBackend(lateness_days=40.0)
    rows, nb, fr = R.ties_script(be)
    assert be.m.take_status() == 0 and be.m.late_counts() == {"late_rows": 6, "late_past_delay": 6}
    ts = np.array([R.d(r[0]) for r in rows], np.int64)
    o = np.argsort(ts, kind="stable")
    want = np.zeros((len(rows), 6))
    want[o] = R.oracle_columns(ts[o], [rows[i][1] for i in o], [rows[i][2] for i in o])
    got = R.columns(nb, fr)
    np.testing.assert_array_equal(got[-3:], want[-3:])       # the in-order rows after every late row
    assert got[-1, 4] == 6 and not np.array_equal(got, want)  # day 60: (23, 53] holds 29, 30, 41, 48, 50, 52


def test_too_late_script():
    assert R.too_late_script(ModelBackend(lateness_days=12.0)) == R.TOO_LATE_EXPECTED


def test_restore_script():
    be = ModelBackend(lateness_days=12.0)
    assert R.restore_script(be) == R.RESTORE_EXPECTED
    assert [t // R.DAY - R.BASE // R.DAY for t in be.m.terms[2].ts] == [90, 100]   # the refused row is not there
