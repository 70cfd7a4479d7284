"""The exact reference of tests/ranking_ref.py (the definition of fdx_ranking_metrics in
include/fdx.h) agrees with scikit-learn's roc_auc_score / average_precision_score on every named
input: this pins the definition to scikit-learn without a GPU."""
import math
import warnings

import numpy as np
import pytest

import ranking_ref as rr


def rel(a, ref):
    return abs(a - ref) / abs(ref) if ref else abs(a - ref)


@pytest.mark.parametrize("name", [n for n in rr.NAMES if rr.both_classes(n)])
def test_exact_reference_agrees_with_sklearn(name):
    e = rr.exact_of(name)
    auc, ap = rr.sklearn_of(name)
    print(name, "auc rel", rel(e["auc"], auc), "ap rel", rel(float(e["ap"]), ap))
    assert rel(e["auc"], auc) <= 1e-12
    assert rel(float(e["ap"]), ap) <= 1e-12


@pytest.mark.parametrize("name", ["no_pos", "no_neg"])
def test_one_class_values_are_sklearns(name):
    from sklearn.metrics import average_precision_score, roc_auc_score

    s, y = rr.named_inputs()[name]
    e = rr.exact_of(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        auc, ap = roc_auc_score(y, s), average_precision_score(y, s)
    assert math.isnan(auc) and math.isnan(e["auc"])
    assert float(e["ap"]) == ap


def test_named_inputs_are_what_the_gpu_tests_expect():
    c = rr.named_inputs()
    assert sorted(c) == sorted(rr.NAMES)
    e = rr.exact_of
    assert e("signs")["n_groups"] == 4098 and len(c["signs"][0]) == 4099  # the two zeros merge
    assert e("big")["n_groups"] == 926 and e("big")["n_pos"] == 14181
    assert e("alltie")["n_groups"] == 1 and e("alltie3")["n_groups"] == 1
    assert e("perfect")["auc"] == 1.0 and e("inverted")["auc"] == 0.0
    assert e("block")["auc_num"] == 2 * 70000 * 70000 > 2**32
    assert e("no_pos")["n_pos"] == 0 and e("no_neg")["n_neg"] == 0 and e("empty")["n_groups"] == 0
    assert float(e("empty")["ap"]) == 0.0 and math.isnan(e("empty")["auc"])
    np.testing.assert_array_equal(e("cont")["tps"] + e("cont")["fps"], np.arange(1, 4100))
