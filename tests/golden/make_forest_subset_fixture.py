"""Regenerates tests/golden/forest_subset_g1.npz: what scikit-learn gives with ``max_features`` below 1.0 on the G1 rows, for the
tests of ForestRegressor.fit(max_features=...) and ForestRegressor.feature_importances.

Needs scikit-learn (the tests that read the fixture do not).  The rows are ``forest_fit_cases.g1_problem()``: train on i % 3 != 0.
  sklearn_l2_m19, sklearn_l2_sqrt   held-out mean L2 of ``RandomForestRegressor(n_estimators=100, max_features=19 | "sqrt",
                                    random_state=s)`` for s = 0 .. 19 (float64 [20] each);
  forest_names and, per name, <name>_<key>: three forests ``RandomForestRegressor(n_estimators=20, random_state=3, ...)`` on the
                                    training rows -- m19: max_features=19; leaf3: min_samples_leaf=3; m7d4: max_features=7, max_depth=4
                                    -- as concatenated trees (tree_ptr, feature, threshold, left, right, value [N, K]; children
                                    numbered within a tree), counts (int32 [20, n]: the bincount of every estimator's
                                    ``_generate_sample_indices``) and importances (its ``feature_importances_``).

The script REFUSES a forest unless ``forest_subset_cases.mdi`` gives its ``feature_importances_`` within 1e-12.

    python tests/golden/make_forest_subset_fixture.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]

MAX_BYTES = 1000 * 1000
FORESTS = {"m19": dict(max_features=19), "leaf3": dict(min_samples_leaf=3), "m7d4": dict(max_features=7, max_depth=4)}


def main():
    import sklearn
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.ensemble._forest import _generate_sample_indices, _get_n_samples_bootstrap

    import forest_fit_cases as fc
    import forest_subset_cases as sc

    X, ideal, _, train = fc.g1_problem()
    Xt, yt, n = X[train], ideal[train], int(train.sum())
    out = dict(sklearn_version=np.asarray(sklearn.__version__), forest_names=np.asarray(list(FORESTS)))
    for key, mf in (("m19", 19), ("sqrt", "sqrt")):
        l2 = np.asarray([fc.mean_l2(RandomForestRegressor(n_estimators=100, max_features=mf, random_state=s).fit(Xt, yt).predict(X[~train]),
                                    ideal[~train]) for s in range(20)])
        print(f"max_features={mf!r}: held-out mean L2 over 20 seeds: mean {l2.mean():.7f}, sigma {l2.std():.7f}, mean + 5 sigma "
              f"{l2.mean() + 5 * l2.std():.6f}")
        out[f"sklearn_l2_{key}"] = l2
    draws = _get_n_samples_bootstrap(n, None)
    for name, kw in FORESTS.items():
        rf = RandomForestRegressor(n_estimators=20, random_state=3, **kw).fit(Xt, yt)
        trees = [est.tree_ for est in rf.estimators_]
        cat = lambda k: np.concatenate([getattr(t, k) for t in trees])   # noqa: E731
        forest = dict(tree_ptr=np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int64),
                      feature=cat("feature").astype(np.int32), threshold=cat("threshold").astype(np.float64),
                      left=cat("children_left").astype(np.int32), right=cat("children_right").astype(np.int32),
                      value=cat("value")[:, :, 0].astype(np.float64))
        counts = np.stack([np.bincount(_generate_sample_indices(est.random_state, n, draws), minlength=n)
                           for est in rf.estimators_]).astype(np.int32)
        want = np.asarray(rf.feature_importances_, np.float64)
        err = float(np.abs(sc.mdi(forest, Xt, counts) - want).max())
        if err > 1e-12:
            raise SystemExit(f"forest {name}: the restatement differs from feature_importances_ by {err:.3e}")
        print(f"forest {name}: {int(forest['tree_ptr'][-1])} nodes, |mdi - feature_importances_| <= {err:.1e}")
        out.update({f"{name}_{k}": v for k, v in forest.items()}, **{f"{name}_counts": counts, f"{name}_importances": want})
    path = os.path.join(OUT, "forest_subset_g1.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, f"{size} bytes"
    print(f"forest_subset_g1.npz: {size} bytes")


if __name__ == "__main__":
    main()
