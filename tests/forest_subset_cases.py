"""The feature-subset rule of include/mlqem_hip.h (max_features per node) and the impurity importances, restated in Python integers
and numpy; shared by tests/test_forest_subset_cpu.py, tests/test_gpu_forest_subset.py and tests/golden/make_forest_subset_fixture.py
(no test in here).

``check_forest_subset`` is ``forest_fit_cases.check_forest``'s walk with the rule's three changes at a node that meets no leaf
condition: which features the node visits, that its split is one of them, and that its score is the best over THOSE.  The node
index that keys the permutation is the index in the fitter's own numbering, so the forest must come straight from
``ops.forest_fit``.  The bounds are ``check_forest``'s, derived in its module docstring.
"""
import os

import numpy as np

import forest_fit_cases as fc

M32 = 0xFFFFFFFF
TREE_KEYS = ("tree_ptr", "feature", "threshold", "left", "right", "value")


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def node_key(seed, t, node):
    return mix32(mix32(mix32(seed) ^ t) ^ node)


def half_bits(F):
    return max(1, ((F - 1).bit_length() + 1) // 2)


def perm(key, F, i):
    """pi(i) of the node with this key: the first of E(i), E(E(i)), ... below F."""
    h = half_bits(F)
    mask = (1 << h) - 1
    v = i
    while True:
        left, right = v >> h, v & mask
        for r in range(8):
            left, right = right, left ^ (mix32(right ^ key ^ ((r * 0x9e3779b9) & M32)) & mask)
        v = (left << h) | right
        if v < F:
            return v


def _mix32_many(x):
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def perm_many(keys, F, i):
    """``perm(key, F, i)`` for an array of keys at once (uint64 lanes holding uint32 values; tests compare it with ``perm``)."""
    keys = np.asarray(keys, np.uint64)
    h = np.uint64(half_bits(F))
    mask = np.uint64((1 << int(h)) - 1)
    v, out = np.full(keys.shape, i, np.uint64), np.full(keys.shape, -1, np.int64)
    while (out < 0).any():
        left, right = v >> h, v & mask
        for r in range(8):
            left, right = right, left ^ (_mix32_many(right ^ keys ^ np.uint64((r * 0x9e3779b9) & M32)) & mask)
        v = (left << h) | right
        out = np.where((out < 0) & (v < F), v.astype(np.int64), out)
    return out


def visited(key, F, m, has):
    """The features a node visits: the first c of pi, c the smallest count >= m at which one of them has a candidate (all F if none has)."""
    out, seen = [], False
    for i in range(F):
        f = perm(key, F, i)
        out.append(f)
        seen = seen or bool(has[f])
        if len(out) >= m and seen:
            break
    return out


def check_forest_subset(X, y, counts, params, m, seed, forest):
    """Asserts the rule's invariants on every node of every tree grown with ``max_features = m`` and ``seed``.  Arguments and the
    returned summary as ``check_forest``, plus ``nodes_where_subset_mattered``: split nodes whose best score over ALL features beats
    the chosen one by more than tol."""
    X = np.asarray(X, np.float32)
    y = np.asarray(y, np.float64).reshape(X.shape[0], -1)
    counts = np.asarray(counts)
    K, F = y.shape[1], X.shape[1]
    mss, msl = int(params.get("min_samples_split", 2)), int(params.get("min_samples_leaf", 1))
    max_depth = params.get("max_depth")
    max_depth = np.inf if max_depth is None else int(max_depth)
    tree_ptr = np.asarray(forest["tree_ptr"], np.int64)
    assert tree_ptr.size == counts.shape[0] + 1, "one tree per bag"
    value = np.asarray(forest["value"], np.float64).reshape(int(tree_ptr[-1]), -1)
    assert value.shape[1] == K, "value: one column per output"
    summary = dict(nodes=0, leaves=0, max_depth=0, nodes_where_subset_mattered=0)
    for t in range(counts.shape[0]):
        b, e = int(tree_ptr[t]), int(tree_ptr[t + 1])
        feature, threshold = np.asarray(forest["feature"][b:e]), np.asarray(forest["threshold"][b:e], np.float64)
        left, right, val = np.asarray(forest["left"][b:e]), np.asarray(forest["right"][b:e]), value[b:e]
        samples = np.asarray(forest["n_node_samples"][b:e]) if "n_node_samples" in forest else None
        w = counts[t]
        assert (w >= 0).all() and (w > 0).any()
        stack, seen = [(0, np.flatnonzero(w > 0), 0)], 0
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
            W, S, impurity, A, Y = fc.node_stats(y, w, idx)
            bound = (2 * c + 2) * fc.U * A / W
            err = np.abs(val[i] - S / W)
            assert (err <= bound).all(), f"{where}: value off by {err.max():.3e}, bound {bound.max():.3e}"
            must_be_leaf = depth >= max_depth or c < mss or c < 2 * msl or impurity <= fc.EPS
            summary["nodes"] += 1
            summary["max_depth"] = max(summary["max_depth"], depth)
            is_leaf = left[i] < 0
            assert (right[i] < 0) == is_leaf, f"{where}: one child"
            if must_be_leaf:
                assert is_leaf, f"{where}: split although a leaf condition holds (impurity {impurity:.3e})"
            if is_leaf and (must_be_leaf or c < 2):
                summary["leaves"] += 1
                continue
            score, thr = fc.node_candidates(X, y, w, idx, msl)
            has = (score > -np.inf).any(axis=0)                    # exact: float32 compares and integer counts
            if is_leaf:
                assert not has.any(), f"{where}: a leaf with impurity {impurity:.3e} that has a candidate and meets no leaf condition"
                summary["leaves"] += 1
                continue
            f = int(feature[i])
            assert 0 <= f < F, f"{where}: feature {f}"
            seen_f = visited(node_key(seed, t, i), F, m, has) if m < F else list(range(F))
            assert f in seen_f, f"{where}: splits on feature {f}, the node visits {seen_f}"
            hit = np.flatnonzero((score[:, f] > -np.inf) & (thr[:, f] == threshold[i]))
            assert hit.size == 1, (f"{where}: threshold {threshold[i]!r} of feature {f} is not the midpoint of two adjacent separable "
                                   "values of the node's rows")
            p = int(hit[0]) + 1
            tol = (12 * c + 4 * K + 8) * fc.U * float((Y * A).sum())
            got, best = score[p - 1, f], score[:, seen_f].max()
            assert got >= best - tol, f"{where}: score {got!r} is below the best of the visited features {best!r} by more than tol {tol:.3e}"
            if score.max() > got + tol:
                summary["nodes_where_subset_mattered"] += 1
            go_left = X[idx, f].astype(np.float64) <= threshold[i]
            assert int(go_left.sum()) == p and p >= msl and c - p >= msl, f"{where}: children of {int(go_left.sum())} and {c - p} rows"
            stack.append((int(right[i]), idx[~go_left], depth + 1))
            stack.append((int(left[i]), idx[go_left], depth + 1))
        assert seen == e - b, f"tree {t}: {e - b - seen} nodes are not reachable from the root"
    return summary


def mdi(forest, X, counts):
    """scikit-learn's ``feature_importances_`` restated (float64 [F]).  ``forest``: tree_ptr, feature, threshold, left, right, value
    with children numbered within a tree in any order; ``counts`` [T, n]: the bags of the rows ``X``.  Per tree: W of a leaf = the sum of
    the counts of the rows that reach it, W of an inner node = its children's; a split node i gains
    (W_l |v_l|^2 + W_r |v_r|^2 - W_i |v_i|^2) / K; the gains per feature are divided by their sum (trees of one node or with a sum
    <= 0 are left out), averaged over the trees and divided by the sum once more; zeros if no tree remains."""
    X = np.asarray(X, np.float32)
    tree_ptr = np.asarray(forest["tree_ptr"], np.int64)
    F, T = X.shape[1], tree_ptr.size - 1
    value = np.asarray(forest["value"], np.float64).reshape(int(tree_ptr[-1]), -1)
    K = value.shape[1]
    total, used = np.zeros(F), 0
    for t in range(T):
        b, e = int(tree_ptr[t]), int(tree_ptr[t + 1])
        feature, left, right = (np.asarray(forest[k])[b:e] for k in ("feature", "left", "right"))
        sq = (value[b:e] ** 2).sum(axis=1)
        W = np.zeros(e - b)
        np.add.at(W, fc.leaf_of_rows(forest, t, X), np.asarray(counts[t], np.float64))
        order, frontier = [], [0]                                  # parents before children
        while frontier:
            order += frontier
            frontier = [c for i in frontier if left[i] >= 0 for c in (int(left[i]), int(right[i]))]
        gain = np.zeros(F)
        for i in reversed(order):
            if left[i] >= 0:
                W[i] = W[left[i]] + W[right[i]]
        for i in order:
            if left[i] >= 0:
                gain[int(feature[i])] += (W[left[i]] * sq[left[i]] + W[right[i]] * sq[right[i]] - W[i] * sq[i]) / K
        if e - b > 1 and gain.sum() > 0.0:
            total += gain / gain.sum()
            used += 1
    if used == 0:
        return np.zeros(F)
    total /= used
    return total / total.sum()


def load_fixture():
    """(the two 20-seed scikit-learn L2 series, [dict(name, X, counts, importances, trees...)]) of tests/golden/forest_subset_g1.npz;
    the forests were fitted on the G1 training rows ``g1_problem()`` gives."""
    z = np.load(os.path.join(fc.GOLDEN, "forest_subset_g1.npz"))
    X, ideal, _, train = fc.g1_problem()
    forests = []
    for name in [str(s) for s in z["forest_names"]]:
        case = {k: z[f"{name}_{k}"] for k in TREE_KEYS + ("counts", "importances")}
        case.update(name=name, X=X[train], y=ideal[train])
        forests.append(case)
    return {"m19": z["sklearn_l2_m19"], "sqrt": z["sklearn_l2_sqrt"]}, forests
