"""Host-side checks of the out-of-bag path (ForestRegressor.oob_predict / fit(oob_score=True) / oob_permutation_importance): the
scikit-learn fixture against the numpy restatement, the R^2 rule, the argument validation and the binding's tables.  Nothing here
touches a GPU.

The stored ``oob_score_`` is compared within 1e-12: two sums of at most 200 terms of order 1 in float64 carry an error of about
n 2^-53 = 2e-14, so the bound leaves a factor of 50."""
import warnings

import numpy as np
import pytest
import torch

import forest_fit_cases as fc
import forest_oob_cases as oc
from blackwater.native import _lib
from blackwater.nn import ForestRegressor
from blackwater.nn.forest import r2_score

CASES = oc.load_fixture()


def host_leaves(case):
    trees = {k: case[k] for k in oc.TREE_KEYS}
    return np.stack([fc.leaf_of_rows(trees, t, case["X"]) for t in range(case["T"])], axis=1)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_fixture_equals_the_numpy_restatement(i):
    case = CASES[i]
    n, K, T = case["n"], case["K"], case["T"]
    assert case["X"].shape == (n, case["F"]) and case["X"].dtype == np.float32 and case["counts"].shape == (T, n)
    assert case["counts"].dtype == np.int32 and (case["counts"].sum(axis=1) == n).all()
    pred, n_oob = oc.oob_restatement(host_leaves(case), case["tree_ptr"], case["value"], case["counts"])
    assert case["oob_prediction"].shape == (n, K) and np.array_equal(pred, case["oob_prediction"])
    assert np.array_equal(n_oob, (case["counts"] == 0).sum(axis=0)) and int((n_oob == 0).sum()) == case["empty_rows"]
    assert (pred[n_oob == 0] == 0.0).all()
    score = oc.r2_rule(case["y"], pred)
    print(f"case {i}: |restated R^2 - oob_score_| = {abs(score - float(case['oob_score'])):.3e}")
    assert abs(score - float(case["oob_score"])) <= 1e-12
    module_score = float(r2_score(torch.from_numpy(case["y"]), torch.from_numpy(pred)))
    assert abs(module_score - float(case["oob_score"])) <= 1e-12


def test_r2_rule_edge_cases():
    y = torch.tensor([[1.0, 2.0, 0.0], [1.0, 4.0, 2.0], [1.0, 6.0, 4.0]], dtype=torch.float64)
    pred = y.clone()
    pred[:, 2] += 1.0
    # column 0: constant target, exact prediction -> 1.0; column 1: exact -> 1.0; column 2: 1 - 3 / 8
    assert float(r2_score(y, pred)) == pytest.approx((1.0 + 1.0 + (1.0 - 3.0 / 8.0)) / 3.0, abs=1e-15)
    pred[:, 0] += 0.5                                    # constant target, wrong prediction -> 0.0
    assert float(r2_score(y, pred)) == pytest.approx((0.0 + 1.0 + (1.0 - 3.0 / 8.0)) / 3.0, abs=1e-15)
    assert np.isnan(float(r2_score(y[:1], pred[:1]))) and np.isnan(oc.r2_rule(y[:1].numpy(), pred[:1].numpy()))
    assert oc.r2_rule(y.numpy(), pred.numpy()) == pytest.approx(float(r2_score(y, pred)), abs=1e-15)
    assert float(r2_score(y[:, 1], pred[:, 1])) == 1.0   # 1-D targets


def host_forest(case):
    return ForestRegressor.from_arrays(*(case[k] for k in oc.TREE_KEYS), n_features=case["F"])


def test_bad_counts_are_refused_on_the_host():
    """CPU tensors throughout: a ValueError here comes before any device is looked at."""
    case = CASES[0]
    forest = host_forest(case)
    x, y = torch.from_numpy(case["X"]), torch.from_numpy(case["y"])
    counts = torch.from_numpy(case["counts"])
    negative = counts.clone()
    negative[1, 7] = -1
    bad = {"dtype": counts.to(torch.int64), "float": counts.to(torch.float32), "trees": counts[:2], "rows": counts[:, :-1],
           "1-D": counts[0], "negative": negative, "numpy": case["counts"]}
    for name, c in bad.items():
        with pytest.raises(ValueError, match="sample_counts"):
            forest.oob_predict(x, c)
        with pytest.raises(ValueError, match="sample_counts"):
            forest.oob_permutation_importance(x, y, c)
        if name not in ("trees",):                      # fit takes any number of trees from the counts' own shape
            with pytest.raises(ValueError, match="sample_counts"):
                ForestRegressor.fit(x, y, sample_counts=c, oob_score=True)
    with pytest.raises(ValueError, match="features"):
        forest.oob_predict(x[:, :-1], counts)
    with pytest.raises(ValueError, match="n_repeats"):
        forest.oob_permutation_importance(x, y, counts, n_repeats=0)
    with pytest.raises(ValueError, match="y must be"):
        forest.oob_permutation_importance(x, y[:-1], counts)


def test_oob_score_needs_bags():
    case = CASES[1]
    x, y = torch.from_numpy(case["X"]), torch.from_numpy(case["y"])
    with pytest.raises(ValueError, match="bootstrap"):
        ForestRegressor.fit(x, y, n_estimators=3, bootstrap=False, oob_score=True)


def test_state_dict_has_no_oob_entries():
    forest = host_forest(CASES[3])
    assert sorted(forest.state_dict()) == ["meta", "nodes", "tree_ptr", "value"]
    for name in ("oob_prediction_", "oob_count_", "oob_score_"):
        assert not hasattr(forest, name)


def test_binding_declares_the_entry():
    assert _lib.ABI_VERSION == 48
    restype, argtypes = _lib.SIGNATURES["mlqem_forest_predict_oob_f32"]
    plain = _lib.SIGNATURES["mlqem_forest_predict_f32"][1]
    assert restype is _lib._I and len(argtypes) == len(plain) + 3          # counts, ldc, n_oob
    assert argtypes[10:12] == [_lib._P, _lib._L]
    lib = _lib.load()
    assert lib.mlqem_abi_version() == 48 and hasattr(lib, "mlqem_forest_predict_oob_f32")
    fn = lib.mlqem_forest_predict_oob_f32
    # the argument checks run before any launch: ldc < n_rows, K beyond 16, no rows (OK without a launch), null counts
    assert fn(None, 4, 8, 4, None, None, 1, None, 1, 3, None, 7, None, None, None, None) == -1
    assert fn(None, 4, 8, 4, None, None, 1, None, 17, 3, None, 8, None, None, None, None) == _lib.ERR_UNSUPPORTED
    assert fn(None, 4, 0, 4, None, None, 1, None, 1, 3, None, 0, None, None, None, None) == 0
    assert fn(None, 4, 8, 4, None, None, 1, None, 1, 3, None, 8, None, None, None, None) == -1


def test_no_warning_machinery_leaks():
    """The module's wording is scikit-learn's."""
    from blackwater.nn.forest import OOB_WARNING

    assert OOB_WARNING.startswith("Some inputs do not have OOB scores")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ForestRegressor._warn_if_no_oob(torch.tensor([1, 2, 3], dtype=torch.int32))
    with pytest.warns(UserWarning, match="Some inputs do not have OOB scores"):
        ForestRegressor._warn_if_no_oob(torch.tensor([1, 0, 3], dtype=torch.int32))
