"""Numpy helpers shared by tests/test_forest_oob_cpu.py, tests/test_gpu_forest_oob.py and tests/golden/make_forest_oob_fixture.py
(no test in here): the masked restatement of an out-of-bag prediction and scikit-learn's R^2 rule.

``oob_restatement`` is what scikit-learn's ``oob_prediction_`` computes, restated: for every row, add the float64 leaf values of the
trees that did not draw the row IN TREE ORDER, starting from 0.0, and divide once by their number (a row every tree drew keeps 0.0).
scikit-learn adds in estimator order as well, so with its own bags the two agree bit for bit; the device kernel forms the same sum
in the same order, so the bar for it is equality too.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ((120, 5, 4, 3, 0), (90, 3, 1, 2, 1), (200, 8, 2, 25, 2), (64, 4, 1, 1, 3))   # (n, F, K, T, seed)
EMPTY_ROWS = (26, 31, 0, 37)                                                          # rows with no out-of-bag tree, per case
TREE_KEYS = ("tree_ptr", "feature", "threshold", "left", "right", "value")


def oob_restatement(leaf, tree_ptr, value, counts):
    """(pred float64 [n, K], n_oob int32 [n]).  ``leaf`` [n, T]: the leaf of every (row, tree) pair within its tree (entries of in-bag
    pairs are not read); ``value`` [N, K] in the model's node order; ``counts`` [T, n]: 0 means tree t is out of bag for row r."""
    leaf, counts = np.asarray(leaf), np.asarray(counts)
    value = np.asarray(value, np.float64).reshape(int(tree_ptr[-1]), -1)
    n, T = leaf.shape
    assert counts.shape == (T, n)
    acc = np.zeros((n, value.shape[1]), np.float64)
    n_oob = np.zeros(n, np.int32)
    for t in range(T):                                   # tree order: the order of the additions is part of the statement
        out = counts[t] == 0
        acc[out] += value[int(tree_ptr[t]) + np.maximum(leaf[out, t], 0)]
        n_oob += out
    return acc / np.maximum(n_oob, 1)[:, None].astype(np.float64), n_oob


def r2_rule(y, pred):
    """scikit-learn's r2_score with the uniform average: per output 1 - sum (y - p)^2 / sum (y - mean y)^2 over all rows; a zero
    denominator gives 1.0 when the numerator is 0 and 0.0 otherwise; fewer than two rows give NaN."""
    y = np.asarray(y, np.float64).reshape(len(y), -1)
    pred = np.asarray(pred, np.float64).reshape(len(y), -1)
    if len(y) < 2:
        return float("nan")
    num = ((y - pred) ** 2).sum(axis=0)
    den = ((y - y.mean(axis=0)) ** 2).sum(axis=0)
    score = np.ones(y.shape[1])
    ok = den != 0
    score[ok] = 1.0 - num[ok] / den[ok]
    score[~ok & (num != 0)] = 0.0
    return float(score.mean())


def seeded_counts(seed, T, n):
    """int32 [T, n] of 0 / 1 / 2 entries; with two rows or more row 0 is in every bag and row n - 1 in none."""
    counts = np.random.default_rng(seed + 500).integers(0, 3, size=(T, n)).astype(np.int32)
    if n >= 2:
        counts[:, 0] = 1 + (np.arange(T) % 2)
        counts[:, n - 1] = 0
    return counts


def load_fixture():
    """[dict(n, F, K, T, seed, X, y, counts, trees..., oob_prediction, oob_score)] of tests/golden/forest_oob_g1.npz."""
    z = np.load(os.path.join(GOLDEN, "forest_oob_g1.npz"))
    cases = []
    for i, (n, F, K, T, seed) in enumerate(CASES):
        case = dict(n=n, F=F, K=K, T=T, seed=seed, empty_rows=EMPTY_ROWS[i])
        for key in ("X", "y", "counts", "oob_prediction", "oob_score") + TREE_KEYS:
            case[key] = z[f"c{i}_{key}"]
        cases.append(case)
    return cases
