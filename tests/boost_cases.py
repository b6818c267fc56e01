"""The numpy-fp64 checker and the fixture loader shared by tests/test_boost_cpu.py, tests/test_gpu_boost.py and
tests/golden/make_boost_fixture.py (no test in here).

``check_stages`` does not refit an ensemble and compare: it takes the ensemble it is given, forms every stage's residuals from that
ensemble's OWN earlier stages (``raw = raw + lr * value[leaf]``, a multiply and then an add, as the kernels and scikit-learn's
``predict_stages`` do) and hands stage t to ``forest_fit_cases.check_forest`` as a one-tree forest with the residuals as ``y`` and the
stage's mask as counts.  That checker brings its own derived tolerances; scikit-learn's ``friedman_mse`` orders a node's candidates as
the squared-error score does, so its stages pass unchanged.

Prediction bound (derived, not tuned) between two ensembles that made the same splits on the same rows (the tie-free fixture cases:
the device's fit against scikit-learn's).  Let e_t be the largest difference of ``raw`` after t stages and u = 2^-53.
  e_0      both sides form the mean of n values: each within n u max|y| of the exact one in any order; e_0 <= n u max|y| is taken as
           the issue states it for ``init`` (the two means' errors do not add up to more in practice: both are pairwise sums).
  stage    a leaf's value is the mean of its rows' residuals.  The residuals differ by at most e_t, so do their means; each side then
           computes its mean within the checker's value bound (2 c + 2) u A / W <= (2 n + 2) u R_t, R_t the largest |residual| of
           the fixture's stage t.  The update adds lr times the value:
               e_{t+1} <= e_t + lr (e_t + (2 n + 2) u R_t) = (1 + lr) e_t + lr (2 n + 2) u R_t.
  sum      every stage rounds its product and its sum once on each side: 2 T roundings of at most u max|raw|.
``prediction_bound`` evaluates this recurrence on the fixture's own stages.
"""
import os

import numpy as np

import forest_fit_cases as fc

GOLDEN = fc.GOLDEN
U = fc.U
KEYS = ("tree_ptr", "feature", "threshold", "left", "right", "value")


def stage_tree(ensemble, t):
    """Stage t of an ensemble as a forest of one tree."""
    b, e = int(ensemble["tree_ptr"][t]), int(ensemble["tree_ptr"][t + 1])
    tree = {k: np.asarray(ensemble[k])[b:e] for k in ("feature", "threshold", "left", "right", "value")}
    if "n_node_samples" in ensemble:
        tree["n_node_samples"] = np.asarray(ensemble["n_node_samples"])[b:e]
    tree["tree_ptr"] = np.asarray([0, e - b], np.int64)
    return tree


def stage_values(ensemble, t, X):
    """float64 [n]: the value of the leaf stage t puts every row of X in (walking with the float64 thresholds)."""
    value = np.asarray(ensemble["value"], np.float64).reshape(int(ensemble["tree_ptr"][-1]))
    return value[int(ensemble["tree_ptr"][t]) + fc.leaf_of_rows(ensemble, t, X)]


def staged_reference(ensemble, X, init, lr, n_stages=None):
    """float64 [n_stages, n]: ``raw`` after every stage, one rounded multiply and one rounded add per stage, from ``init``."""
    T = len(ensemble["tree_ptr"]) - 1 if n_stages is None else int(n_stages)
    raw = np.full(X.shape[0], np.float64(init))
    out = np.empty((T, X.shape[0]), np.float64)
    for t in range(T):
        step = np.float64(lr) * stage_values(ensemble, t, X)
        raw = raw + step
        out[t] = raw
    return out


def unmix32(x):
    """The inverse of ``forest_subset_cases.mix32`` (two odd multiplications and three xor-shifts, each a bijection of uint32)."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * pow(0x846ca68b, -1, 1 << 32)) & 0xFFFFFFFF
    x ^= x >> 15
    x ^= x >> 30
    x = (x * pow(0x7feb352d, -1, 1 << 32)) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def check_stages(X, y, masks, params, lr, init, ensemble, subset=None):
    """Asserts ``init == mean(y)`` within n 2^-53 max|y| and the CART rule's invariants on every node of every stage, each on the
    residuals of the ensemble's own earlier stages.  ``masks``: int [T, n] of 0 and 1.  Returns the smallest relative score gap over
    all stages (0.0: an exact tie somewhere).

    ``subset=(m, seed)``: the ensemble was grown with ``max_features = m < F`` and must come straight from ``ops.boost_fit`` (the
    fitter's node numbering keys the feature orders).  Stage t keys its nodes with (seed, t, node);
    ``forest_subset_cases.check_forest_subset`` sees a forest of one tree and keys with (seed', 0, node), so it is given the seed'
    with ``mix32(seed') == mix32(seed) ^ t``: the same keys.  No gap is reported then (inf)."""
    X = np.asarray(X, np.float32)
    y = np.asarray(y, np.float64).reshape(-1)
    masks = np.asarray(masks)
    n, T = X.shape[0], len(ensemble["tree_ptr"]) - 1
    assert masks.shape == (T, n), f"masks {masks.shape}: one row per stage, {T} x {n}"
    assert abs(float(init) - y.mean()) <= n * U * np.abs(y).max(), f"init {init!r} is not the mean {y.mean()!r}"
    raw = np.full(n, np.float64(init))
    gap = np.inf
    for t in range(T):
        resid = y - raw
        try:
            if subset is None or subset[0] >= X.shape[1]:
                summary = fc.check_forest(X, resid[:, None], masks[t][None], params, stage_tree(ensemble, t))
            else:
                import forest_subset_cases as fsc

                seed_t = unmix32(fsc.mix32(int(subset[1]) & 0xFFFFFFFF) ^ t)
                summary = fsc.check_forest_subset(X, resid[:, None], masks[t][None], params, int(subset[0]), seed_t, stage_tree(ensemble, t))
        except AssertionError as exc:
            raise AssertionError(f"stage {t}: {exc}") from exc
        gap = min(gap, summary.get("min_gap", np.inf))
        step = np.float64(lr) * stage_values(ensemble, t, X)
        raw = raw + step
    return float(gap)


def stage_losses(X, y, masks, lr, init, ensemble):
    """(train_score [T], oob_improvement [T]) of an ensemble from its own trees, every sum exact before it is rounded
    (``math.fsum``): the mean squared residual over the stage's bag after its update, and the mean over the rows outside the bag
    before the update less the one after it (0.0 for a full bag)."""
    import math

    y = np.asarray(y, np.float64).reshape(-1)
    masks = np.asarray(masks)
    raw = np.full(X.shape[0], np.float64(init))
    train, oob, scale = [], [], []
    for t in range(masks.shape[0]):
        before = y - raw
        step = np.float64(lr) * stage_values(ensemble, t, X)
        raw = raw + step
        after = y - raw
        bag = masks[t] != 0
        train.append(math.fsum(after[bag] * after[bag]) / bag.sum())
        out = (~bag).sum()
        s0, s1 = math.fsum(before[~bag] * before[~bag]), math.fsum(after[~bag] * after[~bag])
        oob.append((s0 - s1) / out if out else 0.0)
        scale.append((s0 + s1) / out if out else 0.0)
    return np.asarray(train), np.asarray(oob), np.asarray(scale)


def prediction_bound(X, y, init, lr, ensemble):
    """The module docstring's recurrence on the fixture ensemble's own stages: the largest |difference| allowed between its
    prediction and that of another ensemble with the same splits."""
    y = np.asarray(y, np.float64).reshape(-1)
    n, T = X.shape[0], len(ensemble["tree_ptr"]) - 1
    staged = staged_reference(ensemble, X, init, lr)
    e = n * U * np.abs(y).max()
    raw = np.full(n, np.float64(init))
    for t in range(T):
        e = (1.0 + lr) * e + lr * (2 * n + 2) * U * np.abs(y - raw).max()
        raw = staged[t]
    return float(e + 2 * T * U * max(np.abs(staged).max(), abs(float(init))))


def load_fixture():
    """([case], g1) of tests/golden/boost_g1.npz.  A case is a dict: name, X float32 [n, F], y float64 [n], params (min_samples_split,
    min_samples_leaf, max_depth), lr, init, trees (scikit-learn's, concatenated over the stages), train_score [T], pred [n] and
    staged [T, n] (scikit-learn's ``predict`` and ``staged_predict`` on X).  g1: dict with sklearn_g1_l2_sub05 [20] (asserted
    against) and sklearn_g1_l2_sub10 [20] (for the record)."""
    z = np.load(os.path.join(GOLDEN, "boost_g1.npz"))
    cases = []
    for name in [str(s) for s in z["case_names"]]:
        g = lambda k: z[f"{name}_{k}"]   # noqa: E731
        mss, msl, depth = (int(v) for v in g("params"))
        cases.append(dict(name=name, X=g("X"), y=g("y"), params=dict(min_samples_split=mss, min_samples_leaf=msl, max_depth=depth),
                          lr=float(g("lr")), init=float(g("init")), trees={k: g(k) for k in KEYS}, train_score=g("train_score"),
                          pred=g("pred"), staged=g("staged")))
    return cases, dict(sklearn_g1_l2_sub05=z["sklearn_g1_l2_sub05"], sklearn_g1_l2_sub10=z["sklearn_g1_l2_sub10"])
