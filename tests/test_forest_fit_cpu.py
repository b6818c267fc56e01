"""Host side of ForestRegressor.fit: the checker of tests/forest_fit_cases.py against scikit-learn's own trees (the fixture) and
against four mutations of them, the argument checks of ``fit`` (all made before a device is touched) and the documented bag generator."""
import numpy as np
import pytest
import torch

import forest_fit_cases as fc
from blackwater.exception import BlackwaterException
from blackwater.native import ops
from blackwater.nn import ForestRegressor
from blackwater.nn.forest import bootstrap_counts

CASES, SKLEARN_L2 = fc.load_fixture()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_checker_accepts_the_trees_scikit_learn_grew(case):
    name, X, y, counts, params, trees, pred = case
    summary = fc.check_forest(X, y, counts, params, trees)
    print(name, summary)
    assert summary["nodes"] == len(trees["feature"]) and summary["min_gap"] >= 1e-9      # tie-free, as the generator promises
    # the stored predictions are the trees' own
    walked = np.mean([trees["value"][int(trees["tree_ptr"][t]) + fc.leaf_of_rows(trees, t, X)] for t in range(counts.shape[0])], axis=0)
    assert np.abs(walked - pred).max() <= 2 * counts.shape[0] * 2.0 ** -53 * np.abs(trees["value"]).max()
    fc.same_trees(trees, trees, X)


def test_fixture_holds_what_the_issue_describes():
    names = [c[0] for c in CASES]
    assert 3 <= len(names) <= 4 and SKLEARN_L2.shape == (20,)
    assert any(c[2].shape[1] == 1 for c in CASES)                                         # a K = 1 case
    dups = CASES[names.index("dups")][1]
    assert (dups[:, 3] == dups[0, 3]).all() and np.unique(dups[:, 0]).size < dups.shape[0]   # a constant column, duplicated values


def _root_runner_up(X, y, counts, params):
    idx = np.flatnonzero(counts[0] > 0)
    score, thr = fc.node_candidates(X, y.reshape(len(X), -1), counts[0], idx, params["min_samples_leaf"])
    flat = np.argsort(score, axis=None)[::-1]
    p, f = np.unravel_index(flat[1], score.shape)
    _, _, _, A, Y = fc.node_stats(y.reshape(len(X), -1), counts[0], idx)
    tol = (12 * idx.size + 4 * y.reshape(len(X), -1).shape[1] + 8) * 2.0 ** -53 * float((Y * A).sum())
    assert score.flat[flat[0]] - score.flat[flat[1]] > tol
    return int(f), float(thr[p, f])


@pytest.mark.parametrize("mutation,message", [("threshold", "midpoint"), ("runner_up", "below the best"),
                                               ("unsplit", "meets no leaf condition"), ("value", "value off")])
def test_checker_rejects_a_mutated_tree(mutation, message):
    name, X, y, counts, params, trees, pred = CASES[0]
    bad = {k: np.array(v, copy=True) for k, v in trees.items()}
    if mutation == "threshold":        # the root's threshold moved to the next float64
        bad["threshold"][0] = np.nextafter(bad["threshold"][0], np.inf)
    elif mutation == "runner_up":      # the root splits at its second-best candidate, further from the best than tol
        bad["feature"][0], bad["threshold"][0] = _root_runner_up(X, y, counts, params)
    elif mutation == "unsplit":        # the root, impure and with candidates, left a leaf (its subtree becomes unreachable, reported second)
        bad["left"][0] = bad["right"][0] = -1
    else:                              # one leaf's value off by 1e-9
        leaf = int(np.flatnonzero(bad["left"] < 0)[0])
        bad["value"][leaf, 0] += 1e-9
    with pytest.raises(AssertionError, match=message):
        fc.check_forest(X, y, counts, params, bad)


def _ok(n=8, F=3, K=2):
    return torch.zeros((n, F)), torch.zeros((n, K)), {}


BAD_ARGUMENTS = {
    "cpu tensors": (lambda: _ok(), BlackwaterException, "GPU"),
    "x dtype": (lambda: (torch.zeros((8, 3), dtype=torch.float64), torch.zeros(8), {}), ValueError, "x must be float32"),
    "x shape": (lambda: (torch.zeros(8), torch.zeros(8), {}), ValueError, "x must be float32"),
    "y rows": (lambda: (torch.zeros((8, 3)), torch.zeros(7), {}), ValueError, "y must be"),
    "y dtype": (lambda: (torch.zeros((8, 3)), torch.zeros(8, dtype=torch.int64), {}), ValueError, "y must be"),
    "no rows": (lambda: (torch.zeros((0, 3)), torch.zeros(0), {}), ValueError, "rows"),
    "too many rows": (lambda: (torch.empty((2 ** 22 + 1, 1)), torch.empty(2 ** 22 + 1), {}), ValueError, "rows"),
    "too many outputs": (lambda: (torch.zeros((8, 3)), torch.zeros((8, ops.FOREST_MAX_OUTPUTS + 1)), {}), ValueError, "outputs"),
    "too many features": (lambda: (torch.zeros((2, ops.FOREST_MAX_FEATURES + 1)), torch.zeros(2), {}), ValueError, "features"),
    "min_samples_split": (lambda: (*_ok()[:2], dict(min_samples_split=1)), ValueError, "min_samples_split"),
    "min_samples_leaf": (lambda: (*_ok()[:2], dict(min_samples_leaf=0)), ValueError, "min_samples_leaf"),
    "max_depth": (lambda: (*_ok()[:2], dict(max_depth=-1)), ValueError, "max_depth"),
    "n_estimators": (lambda: (*_ok()[:2], dict(n_estimators=0)), ValueError, "n_estimators"),
    "counts shape": (lambda: (*_ok()[:2], dict(sample_counts=torch.ones((2, 7), dtype=torch.int32))), ValueError, "sample_counts must"),
    "counts dtype": (lambda: (*_ok()[:2], dict(sample_counts=torch.ones((2, 8), dtype=torch.int64))), ValueError, "sample_counts must"),
    "negative count": (lambda: (*_ok()[:2], dict(sample_counts=torch.tensor([[1] * 8, [2, -1] + [1] * 6], dtype=torch.int32))),
                       ValueError, "negative"),
    "empty bag": (lambda: (*_ok()[:2], dict(sample_counts=torch.tensor([[1] * 8, [0] * 8], dtype=torch.int32))), ValueError,
                  "tree 1 has an empty bag"),
}


@pytest.mark.parametrize("name", list(BAD_ARGUMENTS))
def test_fit_refuses_bad_arguments_before_any_launch(name):
    """Host tensors throughout: every check but the last (the device) fires before ``fit`` asks where the tensors live; non-finite
    values need the device's reduction and are covered in tests/test_gpu_forest_fit.py."""
    make, error, message = BAD_ARGUMENTS[name]
    x, y, kwargs = make()
    with pytest.raises(error, match=message):
        ForestRegressor.fit(x, y, **kwargs)


def test_seeded_bags_are_reproducible_and_sum_to_n():
    a, b = bootstrap_counts(37, 5, seed=3), bootstrap_counts(37, 5, seed=3)
    assert a.dtype == torch.int32 and tuple(a.shape) == (5, 37) and torch.equal(a, b)
    assert a.sum(dim=1).tolist() == [37] * 5 and int(a.min()) >= 0
    assert not torch.equal(a, bootstrap_counts(37, 5, seed=4)) and not torch.equal(a[0], a[1])
    assert np.array_equal(a.numpy(), fc.bootstrap_counts(37, 5, 3))                     # the documented generator, restated
