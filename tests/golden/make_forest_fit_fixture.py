"""Regenerates tests/golden/forest_fit_g1.npz: what scikit-learn grows, for the tests of ForestRegressor.fit.

Needs scikit-learn (the tests that read the fixture do not).  Inputs: seeded arrays made here, forest_g1.npz (the G1 rows) and
g1_dataset.npz (``ideal``).

(a) Tie-free cases.  ``DecisionTreeRegressor(random_state=0, ...).fit(X, y, sample_weight=counts[t])`` per tree on continuous float32
    rows with explicit bag counts and a min_samples_split (or min_samples_leaf) large enough that no node has two candidates of
    equal score: scikit-learn breaks ties by a random feature order, the device by the lowest feature, so only such trees can be
    compared node for node.  The script walks every tree with the checker of tests/forest_fit_cases.py -- which recomputes every
    node's candidates -- and REFUSES a case whose smallest relative gap between a node's best and runner-up score is below 1e-9
    (it then tries the next seed; the seed used is stored).  Per case <name>: <name>_X float32 [n, F], _y float64 [n, K], _counts int32
    [T, n], _params (min_samples_split, min_samples_leaf, max_depth or -1), the trees (_tree_ptr, _feature, _threshold, _left,
    _right, _value [N, K]; children numbered within a tree) and _pred [n, K], the mean of the trees' predict(X).
      cont4    120 x 4, K = 4, T = 3, min_samples_split 10
      single    90 x 3, K = 1, T = 2, min_samples_split 8
      dups     100 x 5, K = 2, T = 2, min_samples_split 12; column 0 rounded to one decimal (duplicates), column 3 constant
      leaf3    150 x 6, K = 1, T = 2, min_samples_leaf 3, max_depth 5
(b) sklearn_g1_l2 [20]: held-out mean L2 of ``RandomForestRegressor(n_estimators=100, random_state=s)`` for s = 0..19, fitted on the G1
    rows with i % 3 != 0 against ``ideal`` and scored on the rows with i % 3 == 0.

    python tests/golden/make_forest_fit_fixture.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]

MAX_BYTES = 608 * 1024   # forest_g1.npz's limit
MIN_GAP = 1e-9
CASES = (("cont4", 120, 4, 4, 3, dict(min_samples_split=10)), ("single", 90, 3, 1, 2, dict(min_samples_split=8)),
         ("dups", 100, 5, 2, 2, dict(min_samples_split=12)), ("leaf3", 150, 6, 1, 2, dict(min_samples_leaf=3, max_depth=5)))


def make_case(name, n, F, K, T, params, seed):
    from sklearn.tree import DecisionTreeRegressor

    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    if name == "dups":
        X[:, 0] = np.round(X[:, 0], 1)
        X[:, 3] = np.float32(0.25)
    y = rng.normal(size=(n, K)) + X[:, :1].astype(np.float64)
    counts = np.stack([np.bincount(rng.integers(0, n, size=n), minlength=n) for _ in range(T)]).astype(np.int32)
    trees = [DecisionTreeRegressor(random_state=0, **params).fit(X, y, sample_weight=counts[t]).tree_ for t in range(T)]
    cat = lambda key: np.concatenate([getattr(t, key) for t in trees])   # noqa: E731
    forest = dict(tree_ptr=np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int64),
                  feature=cat("feature").astype(np.int32), threshold=cat("threshold").astype(np.float64),
                  left=cat("children_left").astype(np.int32), right=cat("children_right").astype(np.int32),
                  value=cat("value")[:, :, 0].astype(np.float64), n_node_samples=cat("n_node_samples"))
    pred = np.mean([t.predict(X).reshape(n, K) for t in trees], axis=0)
    return X, y, counts, forest, pred


def main():
    import sklearn
    from sklearn.ensemble import RandomForestRegressor

    import forest_fit_cases as fc

    out = dict(case_names=np.asarray([c[0] for c in CASES]), sklearn_version=np.asarray(sklearn.__version__))
    for name, n, F, K, T, params in CASES:
        full = {"min_samples_split": 2, "min_samples_leaf": 1, "max_depth": None, **params}
        for seed in range(100):
            X, y, counts, forest, pred = make_case(name, n, F, K, T, params, seed)
            summary = fc.check_forest(X, y, counts, full, forest)
            if summary["min_gap"] >= MIN_GAP:
                break
            print(f"{name}: seed {seed} refused, smallest relative score gap {summary['min_gap']:.3e}")
        else:
            raise SystemExit(f"{name}: no seed below 100 gives a tie-free case")
        print(f"{name}: seed {seed}, {summary['nodes']} nodes, depth {summary['max_depth']}, smallest relative score gap {summary['min_gap']:.3e}")
        forest.pop("n_node_samples")
        depth = -1 if full["max_depth"] is None else full["max_depth"]
        entries = dict(X=X, y=y, counts=counts, pred=pred, seed=np.asarray(seed),
                       params=np.asarray([full["min_samples_split"], full["min_samples_leaf"], depth], np.int64), **forest)
        out.update({f"{name}_{k}": v for k, v in entries.items()})

    Xg, ideal, _, train = fc.g1_problem()
    l2 = [fc.mean_l2(RandomForestRegressor(n_estimators=100, random_state=s).fit(Xg[train], ideal[train]).predict(Xg[~train]), ideal[~train])
          for s in range(20)]
    out["sklearn_g1_l2"] = np.asarray(l2, np.float64)
    print(f"scikit-learn on G1, 20 seeds: mean {np.mean(l2):.6f}, std {np.std(l2):.6f}, min {np.min(l2):.6f}, max {np.max(l2):.6f}")

    path = os.path.join(OUT, "forest_fit_g1.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, f"{size} bytes"
    print(f"forest_fit_g1.npz: {size} bytes")


if __name__ == "__main__":
    main()
