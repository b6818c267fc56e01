"""Inputs and the numpy-fp64 checker shared by tests/test_forest_fit_cpu.py, tests/test_gpu_forest_fit.py and
tests/golden/make_forest_fit_fixture.py (no test in here).

``check_forest`` does not regrow a forest and compare (equal scores are the norm on ``encode_data`` rows, and which of two equal
candidates wins is the fitter's own business): it walks every tree it is given and asserts, node by node, the invariants of the rule
in include/mlqem_hip.h.

Bounds (derived, not tuned).  A node of c rows with weights w (integer counts, exact in fp64) and outputs y:
  sums      S_k and every prefix of it add at most c terms w y_k (each product rounded once, the same on both sides); every addition
            rounds by at most 2^-53 of a partial sum <= A_k = sum |w y_k|, so a sum is within c 2^-53 A_k of the exact one, in
            whatever order it was formed;
  value     S_k / W: both sides carry the sum's error and one division, W >= 1 is exact:
            |value - S_k / W| <= (2 c + 2) 2^-53 A_k / W;
  score     sum_k sl_k^2 / wl + sum_k sr_k^2 / wr with sr_k = S_k - sl_k.  With e_k = c 2^-53 A_k the error of sl_k and of S_k,
            sr_k is off by 2 e_k (and its own rounding); |sl_k| / wl and |sr_k| / wr are weighted means of y_k, at most
            Y_k = max |y_k|.  So a score is off by at most sum_k (2 Y_k e_k + 4 Y_k e_k) from the sums and (2 K + 4) roundings of
            at most 2^-53 sum_k Y_k A_k each from its squares, divisions and additions.  The fitter's pick beats every other
            candidate in ITS arithmetic, this checker compares in its own, so twice that:
            tol = (12 c + 4 K + 8) 2^-53 sum_k Y_k A_k.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.220446e-16            # a node at or below this impurity is a leaf (the rule's constant)
FEATURE_GAP = np.float32(1e-7)
U = 2.0 ** -53


def bootstrap_counts(n, n_trees, seed):
    """What ForestRegressor.fit documents: ``default_rng(seed).integers(0, n, size=(T, n))``, counted per tree."""
    draws = np.random.default_rng(seed).integers(0, n, size=(n_trees, n))
    return np.stack([np.bincount(d, minlength=n) for d in draws]).astype(np.int32)


def make_pool_rows(seed, n, F):
    """float32 [n, F] as make_rows of tests/test_gpu_forest.py: every entry is one of 12 pool values of its feature or the float32 right
    after it (duplicates everywhere, neighbours one ulp apart); with more than one feature the last column is constant."""
    rng = np.random.default_rng(seed)
    pool = rng.normal(size=(F, 12)).astype(np.float32)
    pick = pool[np.arange(F)[None, :], rng.integers(12, size=(n, F))]
    X = np.where(rng.integers(2, size=(n, F)) == 0, pick, np.nextafter(pick, np.float32(np.inf))).astype(np.float32)
    if F > 1:
        X[:, -1] = pool[-1, 0]
    return X


def make_targets(seed, n, K):
    """float64 [n, K], distinct per row with spacing >= 1e-2 in the first output: two different rows never have an impurity near the
    leaf threshold (it is 0 for a single row and above 1e-6 otherwise)."""
    rng = np.random.default_rng(seed + 77)
    y = rng.uniform(-1.0, 1.0, size=(n, K))
    y[:, 0] = rng.permutation(n) * 1e-2 - n * 5e-3
    return y


def node_stats(y, w, idx):
    wn, yn = w[idx].astype(np.float64), y[idx]
    wy = wn[:, None] * yn
    W, S, Q = wn.sum(), wy.sum(axis=0), (wy * yn).sum()
    impurity = (Q / W - ((S / W) ** 2).sum()) / y.shape[1]
    return W, S, impurity, np.abs(wy).sum(axis=0), np.abs(yn).max(axis=0)


def node_candidates(X, y, w, idx, min_samples_leaf):
    """Every candidate of the node with rows ``idx``: (score [c - 1, F] with -inf where no candidate exists, threshold [c - 1, F]);
    entry [p - 1, f] separates positions p - 1 | p of the rows sorted (stably) by feature f."""
    c = idx.size
    xs = X[idx]
    order = np.argsort(xs, axis=0, kind="stable")
    v = np.take_along_axis(xs, order, axis=0)                                  # float32 [c, F]
    wn = w[idx].astype(np.float64)[order]                                      # [c, F]
    wy = wn[:, :, None] * y[idx][order]                                        # [c, F, K]
    wl, sl = np.cumsum(wn, axis=0)[:-1], np.cumsum(wy, axis=0)[:-1]
    W, S = wn[:, 0].sum(), wy[:, 0].sum(axis=0)
    p = np.arange(1, c)[:, None]
    exists = (v[1:] > v[:-1] + FEATURE_GAP) & (p >= min_samples_leaf) & (c - p >= min_samples_leaf)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = (sl ** 2).sum(axis=2) / wl + ((S - sl) ** 2).sum(axis=2) / (W - wl)
    lo, hi = v[:-1].astype(np.float64), v[1:].astype(np.float64)
    with np.errstate(over="ignore"):
        thr = lo / 2.0 + hi / 2.0
    thr = np.where((thr == hi) | np.isinf(thr), lo, thr)
    return np.where(exists, score, -np.inf), thr


def check_forest(X, y, counts, params, forest):
    """Asserts the rule's invariants on every node of every tree.  ``forest``: tree_ptr, feature, threshold, left, right, value
    (and n_node_samples, when the fitter reports it), children numbered within a tree in any order.  ``params``:
    min_samples_split, min_samples_leaf, max_depth (None: unbounded).  Returns {"nodes", "leaves", "max_depth", "min_gap"}, min_gap
    the smallest relative distance between a node's best and runner-up score (0.0: an exact tie somewhere)."""
    X = np.asarray(X, np.float32)
    y = np.asarray(y, np.float64).reshape(X.shape[0], -1)
    counts = np.asarray(counts)
    K = y.shape[1]
    mss, msl = int(params.get("min_samples_split", 2)), int(params.get("min_samples_leaf", 1))
    max_depth = params.get("max_depth")
    max_depth = np.inf if max_depth is None else int(max_depth)
    tree_ptr = np.asarray(forest["tree_ptr"], np.int64)
    assert tree_ptr.size == counts.shape[0] + 1, "one tree per bag"
    value = np.asarray(forest["value"], np.float64).reshape(int(tree_ptr[-1]), -1)
    assert value.shape[1] == K, "value: one column per output"
    summary = dict(nodes=0, leaves=0, max_depth=0, min_gap=np.inf)
    for t in range(counts.shape[0]):
        b, e = int(tree_ptr[t]), int(tree_ptr[t + 1])
        feature, threshold = np.asarray(forest["feature"][b:e]), np.asarray(forest["threshold"][b:e], np.float64)
        left, right, val = np.asarray(forest["left"][b:e]), np.asarray(forest["right"][b:e]), value[b:e]
        samples = np.asarray(forest["n_node_samples"][b:e]) if "n_node_samples" in forest else None
        w = counts[t]
        assert (w >= 0).all() and (w > 0).any()
        stack, seen = [(0, np.flatnonzero(w > 0), 0)], 0      # the root holds exactly the in-bag rows
        while stack:
            i, idx, depth = stack.pop()
            where = f"tree {t} node {i} (depth {depth}, {idx.size} rows)"
            assert 0 <= i < e - b, f"{where}: child index out of range"
            seen += 1
            assert seen <= e - b, f"tree {t}: the node table has a cycle"
            c = idx.size
            assert c >= 1, f"{where}: an empty node"
            if samples is not None:
                assert int(samples[i]) == c, f"{where}: n_node_samples is {int(samples[i])}"
            W, S, impurity, A, Y = node_stats(y, w, idx)
            bound = (2 * c + 2) * U * A / W
            err = np.abs(val[i] - S / W)
            assert (err <= bound).all(), f"{where}: value off by {err.max():.3e}, bound {bound.max():.3e}"
            must_be_leaf = depth >= max_depth or c < mss or c < 2 * msl or impurity <= EPS
            summary["nodes"] += 1
            summary["max_depth"] = max(summary["max_depth"], depth)
            is_leaf = left[i] < 0
            assert (right[i] < 0) == is_leaf, f"{where}: one child"
            if must_be_leaf:
                assert is_leaf, f"{where}: split although a leaf condition holds (impurity {impurity:.3e})"
            if is_leaf and (must_be_leaf or c < 2):
                summary["leaves"] += 1
                continue
            score, thr = node_candidates(X, y, w, idx, msl)
            best = score.max()
            if is_leaf:
                assert best == -np.inf, f"{where}: a leaf with impurity {impurity:.3e} that has a candidate and meets no leaf condition"
                summary["leaves"] += 1
                continue
            f = int(feature[i])
            assert 0 <= f < X.shape[1], f"{where}: feature {f}"
            hit = np.flatnonzero((score[:, f] > -np.inf) & (thr[:, f] == threshold[i]))
            assert hit.size == 1, (f"{where}: threshold {threshold[i]!r} of feature {f} is not the midpoint of two adjacent separable "
                                   "values of the node's rows")
            p = int(hit[0]) + 1
            tol = (12 * c + 4 * K + 8) * U * float((Y * A).sum())
            got = score[p - 1, f]
            assert got >= best - tol, f"{where}: score {got!r} is below the best {best!r} by more than tol {tol:.3e}"
            flat = np.sort(score[score > -np.inf])
            if flat.size > 1:
                summary["min_gap"] = min(summary["min_gap"], float((flat[-1] - flat[-2]) / max(abs(flat[-1]), 1e-300)))
            go_left = X[idx, f].astype(np.float64) <= threshold[i]
            assert int(go_left.sum()) == p and p >= msl and c - p >= msl, f"{where}: children of {int(go_left.sum())} and {c - p} rows"
            stack.append((int(right[i]), idx[~go_left], depth + 1))
            stack.append((int(left[i]), idx[go_left], depth + 1))
        assert seen == e - b, f"tree {t}: {e - b - seen} nodes are not reachable from the root"
    return summary


def leaf_of_rows(forest, t, X):
    """The leaf (index within tree t) of every row of X, walking with the float64 thresholds."""
    b = int(forest["tree_ptr"][t])
    feature, threshold, left, right = (np.asarray(forest[k])[b:int(forest["tree_ptr"][t + 1])] for k in ("feature", "threshold", "left", "right"))
    at = np.zeros(X.shape[0], np.int64)
    for _ in range(len(feature)):
        live = left[at] >= 0
        if not live.any():
            break
        go_left = X[np.arange(X.shape[0]), np.maximum(feature[at], 0)].astype(np.float64) <= threshold[at]
        at = np.where(live, np.where(go_left, left[at], right[at]), at)
    return at


def same_trees(a, b, X):
    """Recursive comparison of two forests whose nodes are numbered differently: feature and float64 threshold of every inner node
    exactly, the same shape, and every row of X in corresponding leaves."""
    assert np.array_equal(np.diff(a["tree_ptr"]), np.diff(b["tree_ptr"])), "node counts differ"
    for t in range(len(a["tree_ptr"]) - 1):
        ba, bb = int(a["tree_ptr"][t]), int(b["tree_ptr"][t])
        stack, pairs = [(0, 0)], {}
        while stack:
            i, j = stack.pop()
            la, lb = int(a["left"][ba + i]), int(b["left"][bb + j])
            assert (la < 0) == (lb < 0), f"tree {t}: node {i} / {j}: one is a leaf"
            if la < 0:
                pairs[i] = j
                continue
            assert int(a["feature"][ba + i]) == int(b["feature"][bb + j]), f"tree {t}: node {i} / {j}: features differ"
            assert float(a["threshold"][ba + i]) == float(b["threshold"][bb + j]), f"tree {t}: node {i} / {j}: thresholds differ"
            stack.append((la, lb))
            stack.append((int(a["right"][ba + i]), int(b["right"][bb + j])))
        leaf_a, leaf_b = leaf_of_rows(a, t, X), leaf_of_rows(b, t, X)
        assert np.array_equal(np.vectorize(pairs.get)(leaf_a), leaf_b), f"tree {t}: rows reach different leaves"


def load_fixture():
    """[(name, X, y, counts, params, trees, pred)] of tests/golden/forest_fit_g1.npz and the 20 scikit-learn held-out L2 values."""
    z = np.load(os.path.join(GOLDEN, "forest_fit_g1.npz"))
    cases = []
    for name in [str(s) for s in z["case_names"]]:
        g = lambda k: z[f"{name}_{k}"]   # noqa: E731
        mss, msl, depth = (int(v) for v in g("params"))
        params = dict(min_samples_split=mss, min_samples_leaf=msl, max_depth=None if depth < 0 else depth)
        trees = {k: g(k) for k in ("tree_ptr", "feature", "threshold", "left", "right", "value")}
        cases.append((name, g("X"), g("y"), g("counts"), params, trees, g("pred")))
    return cases, z["sklearn_g1_l2"]


def g1_problem():
    """(X float32 [300, 58], ideal [300, 4], noisy [300, 4], train mask): the G1 rows of forest_g1.npz, train on i % 3 != 0."""
    X = np.load(os.path.join(GOLDEN, "forest_g1.npz"))["X"]
    z = np.load(os.path.join(GOLDEN, "g1_dataset.npz"))
    return X, np.asarray(z["ideal"], np.float64), np.asarray(z["noisy"], np.float64), np.arange(300) % 3 != 0


def mean_l2(pred, ideal):
    return float(np.sqrt(((np.asarray(pred, np.float64) - np.asarray(ideal, np.float64)) ** 2).sum(axis=1)).mean())
