"""Regenerates tests/golden/forest_oob_g1.npz: scikit-learn's out-of-bag predictions, for the tests of ForestRegressor.oob_predict.

Needs scikit-learn (the tests that read the fixture do not).  Per case (n, F, K, T, seed) of tests/forest_oob_cases.py:
``rng = default_rng(seed)``, ``X = rng.normal((n, F)).astype(float32)`` with column 0 rounded to one decimal,
``y = rng.normal((n, K)) + X[:, :1]`` (1-D when K == 1), ``RandomForestRegressor(n_estimators=T, oob_score=True, random_state=seed)``.
Stored as c<i>_<key>: X, y, counts (int32 [T, n]: the bincount of every estimator's ``_generate_sample_indices``, its own bag), the
concatenated trees (tree_ptr, feature, threshold, left, right, value [N, K]; children numbered within a tree), oob_prediction
([n, K]) and oob_score; and sklearn_version.

The script REFUSES a case unless its own numpy restatement (``tree_.apply``, a masked sum in tree order, one divide:
forest_oob_cases.oob_restatement) equals scikit-learn's ``oob_prediction_`` bit for bit, and unless the case has the number of rows
without an out-of-bag tree that forest_oob_cases.EMPTY_ROWS records.

    python tests/golden/make_forest_oob_fixture.py
"""
import os
import sys
import warnings

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]

MAX_BYTES = 608 * 1024   # forest_g1.npz's limit


def make_case(n, F, K, T, seed):
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.ensemble._forest import _generate_sample_indices, _get_n_samples_bootstrap

    import forest_oob_cases as oc

    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    X[:, 0] = np.round(X[:, 0], 1)
    y = rng.normal(size=(n, K)) + X[:, :1].astype(np.float64)
    if K == 1:
        y = y[:, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)     # "Some inputs do not have OOB scores": three of the cases are meant to
        rf = RandomForestRegressor(n_estimators=T, oob_score=True, random_state=seed).fit(X, y)
    draws = _get_n_samples_bootstrap(n, None)
    counts = np.stack([np.bincount(_generate_sample_indices(est.random_state, n, draws), minlength=n)
                       for est in rf.estimators_]).astype(np.int32)
    trees = [est.tree_ for est in rf.estimators_]
    cat = lambda key: np.concatenate([getattr(t, key) for t in trees])   # noqa: E731
    forest = dict(tree_ptr=np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int64),
                  feature=cat("feature").astype(np.int32), threshold=cat("threshold").astype(np.float64),
                  left=cat("children_left").astype(np.int32), right=cat("children_right").astype(np.int32),
                  value=cat("value")[:, :, 0].astype(np.float64))
    leaf = np.stack([t.apply(X) for t in trees], axis=1)
    pred, n_oob = oc.oob_restatement(leaf, forest["tree_ptr"], forest["value"], counts)
    want = np.asarray(rf.oob_prediction_, np.float64).reshape(n, K)
    if not np.array_equal(pred, want):
        raise SystemExit(f"case {(n, F, K, T, seed)}: the restatement differs from oob_prediction_ by {np.abs(pred - want).max():.3e}")
    return dict(X=X, y=y, counts=counts, oob_prediction=want, oob_score=np.asarray(rf.oob_score_, np.float64), **forest), n_oob


def main():
    import sklearn

    import forest_oob_cases as oc

    out = dict(sklearn_version=np.asarray(sklearn.__version__))
    for i, case in enumerate(oc.CASES):
        entries, n_oob = make_case(*case)
        empty = int((n_oob == 0).sum())
        if empty != oc.EMPTY_ROWS[i]:
            raise SystemExit(f"case {case}: {empty} rows have no out-of-bag tree, forest_oob_cases.EMPTY_ROWS says {oc.EMPTY_ROWS[i]}")
        score = oc.r2_rule(entries["y"], entries["oob_prediction"])
        print(f"case {case}: {int(entries['tree_ptr'][-1])} nodes, {empty} rows without an out-of-bag tree, oob_score "
              f"{float(entries['oob_score']):.6f} (restated: off by {abs(score - float(entries['oob_score'])):.1e})")
        out.update({f"c{i}_{k}": v for k, v in entries.items()})
    path = os.path.join(OUT, "forest_oob_g1.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, f"{size} bytes"
    print(f"forest_oob_g1.npz: {size} bytes")


if __name__ == "__main__":
    main()
