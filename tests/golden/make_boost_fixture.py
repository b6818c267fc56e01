"""Regenerates tests/golden/boost_g1.npz: what scikit-learn's GradientBoostingRegressor grows and predicts, for the tests of
BoostedRegressor.

Needs scikit-learn (the tests that read the fixture do not).  Inputs: seeded arrays made here, forest_g1.npz (the G1 rows) and
g1_dataset.npz (``ideal``).

(a) Tie-free cases.  ``GradientBoostingRegressor(random_state=0, ...).fit(X, y)`` on continuous float32 rows
    (``default_rng(seed).normal``) with targets ``y = 0.3 N(0, 1) + x_0 + sin(2 x_1)`` and a min_samples_split (or min_samples_leaf)
    large enough that no node of any stage has two candidates of equal score: scikit-learn breaks ties by a random feature order,
    the device by the lowest feature, so only such ensembles can be compared stage for stage.  The script runs ``check_stages`` of
    tests/boost_cases.py on scikit-learn's trees and REFUSES a seed whose smallest relative gap between a node's best and runner-up
    score is below 1e-9 (it then tries the next seed; the seed used is stored).  Per case <name>: <name>_X float32 [n, F], _y float64
    [n], _params (min_samples_split, min_samples_leaf, max_depth), _lr, _init (``init_.constant_``), the trees (_tree_ptr, _feature,
    _threshold, _left, _right, _value [N]; children numbered within a tree), _train_score [T], _pred [n] = ``predict(X)`` and
    _staged [T, n] = ``staged_predict(X)``.
      d3      160 x 5, 12 stages, depth 3, min_samples_split 12, learning rate 0.1
      stump    64 x 3, 20 stages, depth 1, min_samples_split 8, learning rate 0.5
      leaf4   130 x 6, 10 stages, depth 4, min_samples_leaf 4, learning rate 0.2
      dups    100 x 4,  8 stages, depth 2, min_samples_split 12, learning rate 0.3; column 0 rounded to one decimal, column 3 constant
(b) sklearn_g1_l2_sub05 [20]: held-out mean L2 of ``GradientBoostingRegressor(subsample=0.5, random_state=s)`` for s = 0..19, one
    model per column of ``ideal``, fitted on the G1 rows with i % 3 != 0 and scored on the rows with i % 3 == 0.
    sklearn_g1_l2_sub10 [20]: the same with subsample=1.0, for the record only (its spread comes from tie-breaking alone).

    python tests/golden/make_boost_fixture.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]

MAX_BYTES = 608 * 1024   # the limit the forest fixtures keep to
MIN_GAP = 1e-9
CASES = (("d3", 160, 5, 12, 3, dict(min_samples_split=12), 0.1), ("stump", 64, 3, 20, 1, dict(min_samples_split=8), 0.5),
         ("leaf4", 130, 6, 10, 4, dict(min_samples_leaf=4), 0.2), ("dups", 100, 4, 8, 2, dict(min_samples_split=12), 0.3))


def make_case(name, n, F, T, depth, params, lr, seed):
    from sklearn.ensemble import GradientBoostingRegressor

    rng = np.random.default_rng(seed)
    X = rng.normal(size=(n, F)).astype(np.float32)
    if name == "dups":
        X[:, 0] = np.round(X[:, 0], 1)
        X[:, 3] = np.float32(0.25)
    y = 0.3 * rng.normal(size=n) + X[:, 0].astype(np.float64) + np.sin(2.0 * X[:, 1].astype(np.float64))
    model = GradientBoostingRegressor(random_state=0, n_estimators=T, max_depth=depth, learning_rate=lr, **params).fit(X, y)
    trees = [est.tree_ for est in model.estimators_[:, 0]]
    cat = lambda key: np.concatenate([getattr(t, key) for t in trees])   # noqa: E731
    ensemble = dict(tree_ptr=np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int64),
                    feature=cat("feature").astype(np.int32), threshold=cat("threshold").astype(np.float64),
                    left=cat("children_left").astype(np.int32), right=cat("children_right").astype(np.int32),
                    value=cat("value")[:, 0, 0].astype(np.float64), n_node_samples=cat("n_node_samples"))
    return X, y, model, ensemble


def main():
    import sklearn
    from sklearn.ensemble import GradientBoostingRegressor

    import boost_cases as bc
    import forest_fit_cases as fc

    out = dict(case_names=np.asarray([c[0] for c in CASES]), sklearn_version=np.asarray(sklearn.__version__))
    for name, n, F, T, depth, params, lr in CASES:
        full = {"min_samples_split": 2, "min_samples_leaf": 1, **params, "max_depth": depth}
        for seed in range(100):
            X, y, model, ensemble = make_case(name, n, F, T, depth, params, lr, seed)
            init = float(np.ravel(model.init_.constant_)[0])
            gap = bc.check_stages(X, y, np.ones((T, n), np.int32), full, lr, init, ensemble)
            if gap >= MIN_GAP:
                break
            print(f"{name}: seed {seed} refused, smallest relative score gap {gap:.3e}")
        else:
            raise SystemExit(f"{name}: no seed below 100 gives a tie-free case")
        pred, staged = model.predict(X), np.stack(list(model.staged_predict(X)))
        assert np.array_equal(bc.staged_reference(ensemble, X, init, lr), staged), f"{name}: the numpy restatement is not predict_stages"
        print(f"{name}: seed {seed}, {len(ensemble['feature'])} nodes, smallest relative score gap {gap:.3e}")
        ensemble.pop("n_node_samples")
        entries = dict(X=X, y=y, pred=pred, staged=staged, seed=np.asarray(seed), lr=np.asarray(lr), init=np.asarray(init),
                       train_score=np.asarray(model.train_score_, np.float64),
                       params=np.asarray([full["min_samples_split"], full["min_samples_leaf"], depth], np.int64), **ensemble)
        out.update({f"{name}_{k}": v for k, v in entries.items()})

    Xg, ideal, noisy, train = fc.g1_problem()
    for key, subsample in (("sklearn_g1_l2_sub05", 0.5), ("sklearn_g1_l2_sub10", 1.0)):
        l2 = []
        for s in range(20):
            cols = [GradientBoostingRegressor(subsample=subsample, random_state=s).fit(Xg[train], ideal[train, k]).predict(Xg[~train])
                    for k in range(ideal.shape[1])]
            l2.append(fc.mean_l2(np.stack(cols, axis=1), ideal[~train]))
        out[key] = np.asarray(l2, np.float64)
        print(f"scikit-learn on G1, subsample {subsample}, 20 seeds: mean {np.mean(l2):.6f}, std {np.std(l2):.6f}, mean + 5 std "
              f"{np.mean(l2) + 5 * np.std(l2):.6f}, min {np.min(l2):.6f}, max {np.max(l2):.6f}")
    print(f"unmitigated: {fc.mean_l2(noisy[~train], ideal[~train]):.6f}")

    path = os.path.join(OUT, "boost_g1.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, f"{size} bytes"
    print(f"boost_g1.npz: {size} bytes")


if __name__ == "__main__":
    main()
