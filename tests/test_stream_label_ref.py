"""The semantics of delayed fraud reports, pinned without a GPU: the numpy model of the
terminal state (tests/stream_label_ref.py) fed unlabelled rows plus reports equals the oracle
over the labels known before each batch; on-time reports give the true-label features on
every row; the five outcome counters are what the inputs imply.  tests/test_gpu_stream_labels.py
holds the HIP kernels to the same inputs, references and counters."""
import numpy as np
import pytest

import stream_label_ref as R


@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_on_time_inputs_meet_their_precondition(windows, delay):
    """Lags within [1 s, delay / 2 - batch span], every batch shorter than delay / 2, and --
    what makes a report on time -- no row of the report's terminal fed in an earlier batch has
    ts >= ts_i + delay.  Without this the GPU test could pass vacuously."""
    k = R.case("on_time", windows, delay)
    ts, fraud, c = k["cols"]["ts"], k["cols"]["fraud"], k["cuts"]
    span = R.max_span(ts, c)
    assert span < delay * R.DAY // 2
    assert R.NS <= k["lag"].min() and k["lag"].max() <= delay * R.DAY // 2 - span
    assert k["late"] == 0
    applied = np.concatenate(k["due"])
    assert len(applied) == len(set(applied)) == int(fraud.sum()) > 500
    assert sum(len(d) > 0 for d in k["due"]) > 12        # reports arrive all along the stream
    for j, d in enumerate(k["due"][:-1]):                  # a report never precedes its row
        assert np.all(d < c[j])
    tie = np.flatnonzero(fraud[1000:1100]) + 1000          # the tie run, cut at 1050, has reports
    assert 1050 in c and np.any(tie < 1050) and np.any(tie >= 1050)
    t3 = tie[k["cols"]["terminal"][tie] == 3]              # ... several tied on (terminal, ts)
    assert np.sum(t3 < 1050) >= 2 and np.sum(t3 >= 1050) >= 2


@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_model_on_time_equals_true_labels(windows, delay):
    k = R.case("on_time", windows, delay)
    be = R.ModelBackend(40, windows, delay)
    X = R.drive(be, k["cols"], k["cuts"], k["due"])
    np.testing.assert_array_equal(X, k["known"])
    np.testing.assert_array_equal(X, k["true"])
    assert be.label_counts() == {"on_time": int(k["cols"]["fraud"].sum()), "late": 0, "duplicate": 0, "expired": 0,
                                 "unmatched": 0}
    # the same rows with the labels fed inline (today's path)
    inline = R.StreamModel(40, windows, delay)
    c = k["cols"]
    Xi = np.concatenate([inline.update(c["ts"][a:b], c["terminal"][a:b], c["fraud"][a:b])
                         for a, b in zip(k["cuts"][:-1], k["cuts"][1:])])
    np.testing.assert_array_equal(Xi, k["true"])


@pytest.mark.parametrize("windows,delay", R.PARAMS)
def test_model_late_equals_known_before_batch(windows, delay):
    k = R.case("late", windows, delay)
    c, cuts = k["cols"], k["cuts"]
    be = R.ModelBackend(40, windows, delay)
    X = R.drive(be, c, cuts, k["due"])
    np.testing.assert_array_equal(X, k["known"])
    # the invariant: every outstanding report of a fed row went in before the last batch, and
    # that batch has the features of the true labels (its own rows' labels are younger than
    # the delay: the batch spans less than delay / 2)
    a = cuts[-2]
    assert not len(k["due"][-1]) and a < len(c["ts"])
    np.testing.assert_array_equal(X[a:], k["true"][a:])
    assert not np.array_equal(k["known"][:a], k["true"][:a])   # late labels did show in features
    applied = sum(len(d) for d in k["due"])
    assert applied == int(c["fraud"][:a].sum())
    assert 0 < k["late"] < applied
    assert be.label_counts() == {"on_time": applied - k["late"], "late": k["late"], "duplicate": 0, "expired": 0,
                                 "unmatched": 0}


def test_model_outcomes_at_the_smallest_shapes():
    be = R.ModelBackend(2, (1,), 1, ring=8)
    assert R.outcome_script(be) == R.OUTCOME_EXPECTED
    be.m.reset()
    assert be.label_counts() == dict.fromkeys(R.OUTCOMES, 0)
