"""Regression forests on the device: ``ForestRegressor`` scores a fitted random forest with the native forest kernel.

The reference's strongest mitigator is a scikit-learn ``RandomForestRegressor`` on ``encode_data`` rows
(docs/tutorials/vqe_rf*.py, docs/demos/demo1_rf_mimic_zne_100q_twirl.ipynb; blackwater/library/learning/estimator.py:90-148
calls ``model.predict`` once per Pauli term).  This module holds such a forest as registered buffers -- so ``.to(device)``,
``state_dict()`` and ``load_state_dict(strict=True)`` work and a checkpoint depends neither on pickle nor on the scikit-learn
version that fitted it -- and predicts with one launch of ``mlqem_forest_predict_f32`` for any number of rows.

Buffers (include/mlqem_hip.h documents the node record):
  ``nodes``     int32 [N, 4]: (threshold as float32 bits, feature or -1, right child, original index) per node, every tree in
                depth-first pre-order (the left child of node i is node i + 1);
  ``tree_ptr``  int64 [T + 1]: tree t owns nodes tree_ptr[t] .. tree_ptr[t + 1];
  ``value``     float64 [N, K]: the trees' node values in the model's own node order;
  ``meta``      int64 [2]: (number of features, maximum depth).

``ForestRegressor.fit`` grows the forest on the device as well (exact CART, scikit-learn's defaults: the ``mlqem_forest_fit_*`` kernels),
so the mitigator needs scikit-learn neither to be trained nor to be scored.  ``oob_predict`` scores every row with the trees whose
bag does not hold it (``mlqem_forest_predict_oob_f32``, scikit-learn's ``oob_prediction_``); ``fit(oob_score=True)``, ``score`` and
``oob_permutation_importance`` are built on it.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from ..exception import BlackwaterException
from ..native import ops

TREE_LEAF = -1   # scikit-learn's marker in children_left / children_right


def floor_to_float32(thr64: np.ndarray) -> np.ndarray:
    """The largest float32 <= each float64 threshold.  scikit-learn compares a float32 feature with the float64 threshold; for a
    float32 x, ``x <= thr64`` holds exactly when ``x <= floor_to_float32(thr64)`` (x is itself a float32 not above thr64, hence not
    above the largest such; the converse because the rounded threshold is not above thr64).  Rounding to nearest moves rows that
    sit on a split value to the other child."""
    thr64 = np.asarray(thr64, dtype=np.float64)
    with np.errstate(over="ignore"):
        thr32 = thr64.astype(np.float32)
    above = thr32.astype(np.float64) > thr64
    thr32[above] = np.nextafter(thr32[above], np.float32(-np.inf))
    return thr32


def bootstrap_counts(n: int, n_estimators: int, seed: int) -> torch.Tensor:
    """int32 [n_estimators, n]: how often each of ``n`` rows is drawn into each tree's bag.  The generator is
    ``numpy.random.default_rng(seed).integers(0, n, size=(n_estimators, n))`` (PCG64; row t holds tree t's n draws with replacement),
    counted per tree -- every row of the result sums to ``n``.  These are not scikit-learn's bags."""
    draws = np.random.default_rng(int(seed)).integers(0, int(n), size=(int(n_estimators), int(n)))
    counts = np.stack([np.bincount(d, minlength=int(n)) for d in draws]).astype(np.int32)
    return torch.from_numpy(counts)


def r2_score(y: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
    """scikit-learn's ``r2_score(y, pred)`` as a float64 scalar on ``y``'s device: per output 1 - sum (y - p)^2 / sum (y - mean y)^2
    over ALL rows, a zero denominator giving 1.0 when the numerator is 0 as well and 0.0 otherwise; then the uniform mean over the
    outputs.  ``y`` and ``pred`` are [n] or [n, K]; fewer than two rows give NaN."""
    n = int(y.shape[0])
    y = y.reshape(n, -1).to(torch.float64)
    pred = pred.reshape(n, -1).to(torch.float64)
    if y.shape != pred.shape:
        raise ValueError(f"r2_score: y is {tuple(y.shape)}, the prediction {tuple(pred.shape)}")
    if n < 2:
        return torch.full((), float("nan"), dtype=torch.float64, device=y.device)
    num = ((y - pred) ** 2).sum(dim=0)
    den = ((y - y.mean(dim=0, keepdim=True)) ** 2).sum(dim=0)
    ratio = 1.0 - num / torch.where(den != 0, den, torch.ones_like(den))
    flat = torch.where(num != 0, torch.zeros_like(num), torch.ones_like(num))
    return torch.where(den != 0, ratio, flat).mean()


OOB_WARNING = ("Some inputs do not have OOB scores. This probably means too few trees were used to compute any reliable OOB "
               "estimates.")   # scikit-learn's wording


def resolve_max_features(max_features, n_features: int) -> int:
    """scikit-learn's reading of ``max_features`` for ``n_features`` columns: an int is itself (1..F), a float in (0, 1] is
    ``max(1, int(f * F))``, "sqrt" / "log2" are ``max(1, int(sqrt(F)))`` / ``max(1, int(log2(F)))``, None is F.  ``ValueError`` otherwise."""
    f = int(n_features)
    m = None
    if max_features is None:
        m = f
    elif isinstance(max_features, bool):
        pass
    elif isinstance(max_features, (int, np.integer)):
        m = int(max_features) if 1 <= max_features <= f else None
    elif isinstance(max_features, (float, np.floating)):
        m = max(1, int(max_features * f)) if 0.0 < max_features <= 1.0 else None
    elif isinstance(max_features, str) and max_features in ("sqrt", "log2"):
        m = max(1, int(np.sqrt(f) if max_features == "sqrt" else np.log2(f)))
    if m is None:
        raise ValueError(f"forest fit: max_features must be an int in 1..{f}, a float in (0, 1], \"sqrt\", \"log2\" or None, got "
                         f"{max_features!r}")
    return m


def _pack(tree_ptr, feature, threshold, left, right, n_features):
    """Validates the forest and returns (nodes int32 [N, 4], tree_ptr int64, max_depth).  Works on whole levels of all trees at once."""
    tree_ptr = np.asarray(tree_ptr)
    if tree_ptr.ndim != 1 or tree_ptr.size < 2 or not np.issubdtype(tree_ptr.dtype, np.integer):
        raise ValueError("forest: tree_ptr must be a 1-D integer array with at least two entries")
    tree_ptr = tree_ptr.astype(np.int64)
    n = int(tree_ptr[-1])
    counts = np.diff(tree_ptr)
    if tree_ptr[0] != 0 or (counts < 1).any():
        raise ValueError("forest: tree_ptr must start at 0 and increase strictly (every tree has a root)")
    if counts.max() > 2**31 - 1:
        raise ValueError("forest: a tree has more nodes than an int32 indexes")
    arrays = {}
    for name, a in (("feature", feature), ("threshold", threshold), ("left", left), ("right", right)):
        a = np.asarray(a)
        if a.shape != (n,):
            raise ValueError(f"forest: {name} must have one entry per node ({n}), got shape {a.shape}")
        if name != "threshold" and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"forest: {name} must be an integer array")
        arrays[name] = a.astype(np.float64 if name == "threshold" else np.int64)
    feature, threshold, left, right = (arrays[k] for k in ("feature", "threshold", "left", "right"))
    n_features = int(n_features)
    if not 1 <= n_features <= ops.FOREST_MAX_FEATURES:
        raise ValueError(f"forest: n_features must be in 1..{ops.FOREST_MAX_FEATURES}, got {n_features}")

    offset = np.repeat(tree_ptr[:-1], counts)      # first node of the tree every node belongs to
    size_of = np.repeat(counts, counts)
    is_leaf = left == TREE_LEAF
    if ((right == TREE_LEAF) != is_leaf).any():
        raise ValueError("forest: a node has one child: left and right must both be -1 (a leaf) or both be nodes")
    inner = np.flatnonzero(~is_leaf)
    for name, child in (("left", left), ("right", right)):
        bad = (child[inner] < 0) | (child[inner] >= size_of[inner])
        if bad.any():
            raise ValueError(f"forest: node {int(inner[bad][0])}: {name} child {int(child[inner[bad][0]])} is out of range")
    bad = (feature[inner] < 0) | (feature[inner] >= n_features)
    if bad.any():
        raise ValueError(f"forest: node {int(inner[bad][0])} splits on feature {int(feature[inner[bad][0]])}, the rows have {n_features}")
    if np.isnan(threshold[inner]).any():
        raise ValueError("forest: a split threshold is NaN")
    gleft, gright = offset[inner] + left[inner], offset[inner] + right[inner]
    parents = np.bincount(np.concatenate([gleft, gright]), minlength=n)
    if (parents > 1).any():
        raise ValueError(f"forest: node {int(np.flatnonzero(parents > 1)[0])} has more than one parent")
    if parents[tree_ptr[:-1]].any():
        raise ValueError("forest: a root is some node's child (a cycle)")
    # every node now has at most one parent and the roots none: level-by-level descent from the roots visits a node at most once
    child_l, child_r = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    child_l[inner], child_r[inner] = gleft, gright
    levels, frontier, seen = [], tree_ptr[:-1].copy(), 0
    while frontier.size:
        levels.append(frontier)
        seen += frontier.size
        kids = np.concatenate([child_l[frontier], child_r[frontier]])
        frontier = kids[kids >= 0]
    if seen != n:
        raise ValueError(f"forest: {n - seen} nodes cannot be reached from their root (a cycle or a detached subtree)")
    max_depth = len(levels) - 1
    size = np.ones(n, np.int64)                    # nodes of the subtree under each node, deepest level first
    for lv in reversed(levels):
        p = lv[child_l[lv] >= 0]
        size[p] += size[child_l[p]] + size[child_r[p]]
    pos = np.zeros(n, np.int64)                    # pre-order position within the tree
    for lv in levels:
        p = lv[child_l[lv] >= 0]
        pos[child_l[p]] = pos[p] + 1
        pos[child_r[p]] = pos[p] + 1 + size[child_l[p]]
    dst = offset + pos
    nodes = np.zeros((n, 4), np.int32)
    thr32 = floor_to_float32(np.where(is_leaf, 0.0, threshold))
    nodes[dst, 0] = thr32.view(np.int32)
    nodes[dst, 1] = np.where(is_leaf, -1, feature)
    nodes[dst, 2] = np.where(is_leaf, pos, pos[np.maximum(child_r, 0)])
    nodes[dst, 3] = np.arange(n) - offset
    return nodes, tree_ptr, max_depth


class ForestRegressor(torch.nn.Module):
    """A fitted regression forest (mean of T regression trees with K outputs) as a torch module on the native kernel.

    Build one with ``fit``, ``from_sklearn``, ``from_arrays`` or ``from_state_dict``; both array constructors validate the forest on the
    host (``ValueError``), so a malformed one never reaches the device."""

    def __init__(self, nodes: torch.Tensor, tree_ptr: torch.Tensor, value: torch.Tensor, n_features: int, max_depth: int):
        super().__init__()
        self.register_buffer("nodes", nodes)
        self.register_buffer("tree_ptr", tree_ptr)
        self.register_buffer("value", value)
        self.register_buffer("meta", torch.tensor([int(n_features), int(max_depth)], dtype=torch.int64))
        self._set_meta()

    def _set_meta(self):
        self.n_features, self.max_depth = (int(v) for v in self.meta.tolist())   # host copies: predict() never reads a device value
        self.n_trees, self.n_outputs = int(self.tree_ptr.shape[0]) - 1, int(self.value.shape[1])

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._set_meta()

    @classmethod
    def from_arrays(cls, tree_ptr, feature, threshold, left, right, value, n_features) -> "ForestRegressor":
        """``tree_ptr`` [T + 1]; per node, concatenated over the trees: ``feature``, ``threshold`` (float64), ``left`` / ``right``
        (child index WITHIN the tree, -1 for a leaf) and ``value`` [N, K] (or [N], or scikit-learn's [N, K, 1])."""
        nodes, tree_ptr, max_depth = _pack(tree_ptr, feature, threshold, left, right, n_features)
        value = np.asarray(value, dtype=np.float64)
        n = nodes.shape[0]
        if value.ndim == 3 and value.shape[2] == 1:
            value = value[:, :, 0]
        if value.ndim == 1:
            value = value[:, None]
        if value.ndim != 2 or value.shape[0] != n or not 1 <= value.shape[1] <= ops.FOREST_MAX_OUTPUTS:
            raise ValueError(f"forest: value must be [{n}, K] with 1 <= K <= {ops.FOREST_MAX_OUTPUTS}, got shape {value.shape}")
        return cls(torch.from_numpy(nodes), torch.from_numpy(tree_ptr), torch.from_numpy(np.ascontiguousarray(value)),
                   n_features, max_depth)

    @classmethod
    def fit(cls, x: torch.Tensor, y: torch.Tensor, *, n_estimators: int = 100, bootstrap: bool = True, max_depth=None,
            min_samples_split: int = 2, min_samples_leaf: int = 1, seed: int = 0, sample_counts=None,
            workspace_bytes: int = 2 << 30, oob_score: bool = False, max_features=1.0, importances: bool = False) -> "ForestRegressor":
        """``RandomForestRegressor(n_estimators, ...).fit(x, y)`` with scikit-learn's defaults, grown on ``x.device``: exact CART with
        squared error and the best split over the node's features, one tree per bag (include/mlqem_hip.h states the rule node by node).

        ``x``: float32 [n, F] device tensor; ``y``: [n] or [n, K] on the same device, float32 or float64 (widened to float64 before
        anything is multiplied).  ``sample_counts``: int32 [T, n], how often each row is in each tree's bag; when given it overrides
        ``n_estimators`` and ``bootstrap``, and ``seed`` is ignored for the bags (it still seeds the feature draws of ``max_features``).
        Otherwise ``bootstrap=False`` gives every tree every row once, and ``bootstrap=True`` the counts of
        ``bootstrap_counts(n, n_estimators, seed)`` (numpy's ``default_rng(seed)``; not scikit-learn's bags).  A node's sample count
        is its number of distinct in-bag rows, as in scikit-learn's forest.

        Equal scores are broken by the lowest feature index, then the lowest position (scikit-learn: a random feature order), so a
        tree equals scikit-learn's where no two candidates tie.  Two fits give the same buffers bit for bit, whatever
        ``workspace_bytes`` (it bounds the fit's workspace: trees are grown in chunks that fit it).

        ``oob_score=True`` (scikit-learn's): once the forest is built and validated, ``oob_predict`` runs on the training rows with
        the fit's own counts and sets ``oob_prediction_`` (float64 [n] or [n, K], device), ``oob_count_`` (int32 [n], device: the trees
        that left each row out) and ``oob_score_`` (a Python float: ``r2_score(y, oob_prediction_)``, a row without an out-of-bag tree
        counting with its 0.0); the counts stay as ``fit_info["sample_counts"]``.  These are plain attributes, not buffers: the state
        dict does not change.  It needs bags: with ``bootstrap=False`` and no ``sample_counts`` it is a ``ValueError``.

        ``max_features`` (scikit-learn's: an int, a float in (0, 1], "sqrt", "log2", None; ``fit_info["max_features"]`` holds the
        resolved m): with m < F every node visits its own feature order, a pure function of (``seed``, tree, node), until it has seen
        m features and one with a candidate, and splits on the best of those (include/mlqem_hip.h has the rule and where it departs
        from scikit-learn; the draws are not scikit-learn's).  1.0, None or F is the search over all features, bit for bit.

        ``importances=True`` sets ``feature_importances_`` (float64 [F], host) to ``feature_importances(x, counts)`` of the fit's own
        rows and bags; a plain attribute as well.

        Not supported: criteria other than squared error, ``min_weight_fraction_leaf``, ``ccp_alpha``, missing values.  Every
        argument is checked on the host before anything is launched (``ValueError`` / ``BlackwaterException``); the finished node
        table goes through the validation of ``from_arrays``."""
        if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
            raise ValueError("forest fit: x and y must be torch tensors")
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError(f"forest fit: x must be float32 [n, F], got {tuple(x.shape)} {x.dtype}")
        n, f = int(x.shape[0]), int(x.shape[1])
        if y.dim() not in (1, 2) or y.shape[0] != n or y.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"forest fit: y must be float32 or float64 [{n}] or [{n}, K], got {tuple(y.shape)} {y.dtype}")
        k = 1 if y.dim() == 1 else int(y.shape[1])
        if n < 1 or n > ops.FOREST_FIT_MAX_ROWS:
            raise ValueError(f"forest fit: want 1 <= n <= {ops.FOREST_FIT_MAX_ROWS} rows, got {n}")
        if not 1 <= k <= ops.FOREST_MAX_OUTPUTS:
            raise ValueError(f"forest fit: want 1 <= K <= {ops.FOREST_MAX_OUTPUTS} outputs, got {k}")
        if not 1 <= f <= ops.FOREST_MAX_FEATURES:
            raise ValueError(f"forest fit: want 1 <= F <= {ops.FOREST_MAX_FEATURES} features, got {f}")
        if min_samples_split < 2 or min_samples_leaf < 1 or (max_depth is not None and max_depth < 0):
            raise ValueError("forest fit: want min_samples_split >= 2, min_samples_leaf >= 1 and max_depth >= 0 (or None), got "
                             f"{min_samples_split}, {min_samples_leaf}, {max_depth}")
        m = resolve_max_features(max_features, f)
        if sample_counts is None:
            if n_estimators < 1:
                raise ValueError(f"forest fit: n_estimators must be >= 1, got {n_estimators}")
            if oob_score and not bootstrap:
                raise ValueError("forest fit: out of bag estimation is only available with bootstrap=True or explicit sample_counts")
            counts = bootstrap_counts(n, n_estimators, seed) if bootstrap else torch.ones((int(n_estimators), n), dtype=torch.int32)
        else:
            counts = sample_counts
            if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[0] < 1 \
                    or counts.shape[1] != n:
                raise ValueError(f"forest fit: sample_counts must be an int32 [T, {n}] tensor with T >= 1")
            host = counts.cpu()
            if bool((host < 0).any()):
                raise ValueError("forest fit: sample_counts has a negative entry")
            if bool((host.max(dim=1).values < 1).any()):
                raise ValueError(f"forest fit: tree {int(torch.nonzero(host.max(dim=1).values < 1)[0])} has an empty bag")
        if not x.is_cuda or y.device != x.device:
            raise BlackwaterException(f"forest fit: x and y must live on one GPU (got {x.device} and {y.device}); there is no CPU path")
        if f == 1 and n > 1 and x.stride(1) != 1:   # a [n, 1] view may carry any column stride
            x = x.as_strided((n, 1), (x.stride(0), 1))
        y64 = y.reshape(n, k).to(torch.float64).contiguous()
        if not bool(torch.isfinite(x).all() & torch.isfinite(y64).all()):   # one reduction, one wait
            raise ValueError("forest fit: x or y holds a NaN or an infinity")
        counts = counts.to(x.device).contiguous()
        grown = ops.forest_fit(x, y64, counts, min_samples_split=int(min_samples_split),
                               min_samples_leaf=int(min_samples_leaf), max_depth=None if max_depth is None else int(max_depth),
                               workspace_bytes=int(workspace_bytes), max_features=m, seed=int(seed))
        forest = cls.from_arrays(*(grown[key] for key in ("tree_ptr", "feature", "threshold", "left", "right", "value")),
                                 n_features=f).to(x.device)
        forest.fit_info = {key: grown[key] for key in ("levels", "trees_per_chunk", "n_node_samples")}
        forest.fit_info["max_features"] = m
        if oob_score:
            pred, n_oob = forest._oob_run(x, counts)
            forest._warn_if_no_oob(n_oob)
            forest.oob_prediction_ = pred[:, 0] if k == 1 else pred
            forest.oob_count_ = n_oob
            forest.oob_score_ = float(r2_score(y64, pred))
            forest.fit_info["sample_counts"] = counts
        if importances:
            forest.feature_importances_ = forest._importances_run(x, counts)
        return forest

    @classmethod
    def from_sklearn(cls, model) -> "ForestRegressor":
        """From a fitted ``RandomForestRegressor``, ``ExtraTreesRegressor`` or ``DecisionTreeRegressor``."""
        try:
            from sklearn.ensemble import ExtraTreesRegressor, RandomForestRegressor
            from sklearn.tree import DecisionTreeRegressor
        except ImportError as exc:
            raise BlackwaterException("ForestRegressor.from_sklearn needs scikit-learn; use from_arrays or from_state_dict") from exc
        if isinstance(model, (RandomForestRegressor, ExtraTreesRegressor)):
            if not hasattr(model, "estimators_"):
                raise BlackwaterException(f"{type(model).__name__} is not fitted")
            trees = [est.tree_ for est in model.estimators_]
        elif isinstance(model, DecisionTreeRegressor):
            if not hasattr(model, "tree_"):
                raise BlackwaterException("DecisionTreeRegressor is not fitted")
            trees = [model.tree_]
        else:
            raise BlackwaterException("ForestRegressor.from_sklearn takes a fitted RandomForestRegressor, ExtraTreesRegressor or "
                                      f"DecisionTreeRegressor, got {type(model).__name__}")
        tree_ptr = np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int64)
        cat = lambda name: np.concatenate([getattr(t, name) for t in trees])  # noqa: E731
        return cls.from_arrays(tree_ptr, cat("feature"), cat("threshold"), cat("children_left"), cat("children_right"),
                               cat("value"), int(model.n_features_in_))

    @classmethod
    def from_state_dict(cls, state_dict) -> "ForestRegressor":
        """A module with buffers of the checkpoint's sizes, strict-loaded (buffer shapes depend on the forest, so there is no
        forest-independent module to load into)."""
        missing = [k for k in ("nodes", "tree_ptr", "value", "meta") if k not in state_dict]
        if missing:
            raise ValueError(f"forest checkpoint lacks {missing}")
        nodes, tree_ptr, value, meta = (state_dict[k] for k in ("nodes", "tree_ptr", "value", "meta"))
        if (nodes.dtype != torch.int32 or nodes.dim() != 2 or nodes.shape[1] != 4 or tree_ptr.dtype != torch.int64 or tree_ptr.dim() != 1
                or tree_ptr.numel() < 2 or value.dtype != torch.float64 or value.dim() != 2 or value.shape[0] != nodes.shape[0]
                or not 1 <= value.shape[1] <= ops.FOREST_MAX_OUTPUTS or meta.dtype != torch.int64 or tuple(meta.shape) != (2,)):
            raise ValueError("forest checkpoint: buffers have the wrong dtype or shape")
        counts = tree_ptr[1:] - tree_ptr[:-1]
        if int(tree_ptr[0]) != 0 or int(tree_ptr[-1]) != nodes.shape[0] or bool((counts < 1).any()):
            raise ValueError("forest checkpoint: tree_ptr does not partition the nodes")
        f, depth = (int(v) for v in meta.tolist())
        if not 1 <= f <= ops.FOREST_MAX_FEATURES or not 0 <= depth < nodes.shape[0]:
            raise ValueError("forest checkpoint: meta (n_features, max_depth) is out of range")
        module = cls(torch.empty_like(nodes, device="cpu"), torch.empty_like(tree_ptr, device="cpu"),
                     torch.empty_like(value, device="cpu"), f, depth)
        module.load_state_dict(state_dict, strict=True)
        return module

    def _run(self, x: torch.Tensor, want_leaf: bool):
        if x.dim() != 2 or x.shape[1] != self.n_features:
            raise ValueError(f"forest: want rows of {self.n_features} features, got {tuple(x.shape)}")
        return ops.forest_predict(x, self.nodes, self.tree_ptr, self.value, self.max_depth, want_leaf=want_leaf)

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """float64 [n, K] ([n] when K == 1, as scikit-learn): the mean over the trees of each row's leaf values."""
        out, _ = self._run(x, False)
        return out[:, 0] if self.n_outputs == 1 else out

    def apply(self, x: torch.Tensor) -> torch.Tensor:
        """int32 [n, T]: the leaf every tree puts each row in, in the model's own node numbering (scikit-learn's ``apply``)."""
        return self._run(x, True)[1]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """float32 [n, K]: ``predict`` rounded, so the module composes with float32 torch code."""
        return self._run(x, False)[0].to(torch.float32)

    def score(self, x: torch.Tensor, y: torch.Tensor) -> float:
        """R^2 of ``predict(x)`` against ``y`` ([n] or [n, K] on ``x``'s device): scikit-learn's ``score`` (see ``r2_score``)."""
        pred = self._run(x, False)[0]
        if not isinstance(y, torch.Tensor) or y.dim() not in (1, 2) or y.numel() != pred.numel() or y.shape[0] != pred.shape[0]:
            raise ValueError(f"forest score: y must be a [{pred.shape[0]}] or [{pred.shape[0]}, {self.n_outputs}] tensor")
        return float(r2_score(y.to(pred.device), pred))

    # ---- impurity importances --------------------------------------------------------------------------------------------------
    def feature_importances(self, x: torch.Tensor, sample_counts: torch.Tensor) -> np.ndarray:
        """scikit-learn's ``feature_importances_`` (mean decrease in impurity), float64 [F] on the host, from the training rows ``x``
        and their bags ``sample_counts`` (int32 [T, n], as ``oob_predict`` takes them; checked on the host first).  The weight W of a
        leaf is the sum of the counts of the rows ``apply`` puts there (integers: exact in any order), that of an inner node the sum
        of its children's.  A split node i with children l, r and values v gains
        ``(W_l sum_k v_l,k^2 + W_r sum_k v_r,k^2 - W_i sum_k v_i,k^2) / K`` -- its weighted impurity less its children's: a value is
        the weighted mean of its node, so the sum w y^2 terms cancel.  Per tree the gains are added per feature and divided by their
        sum (a tree of one node, or one whose gains sum to <= 0, is left out); the mean over the remaining trees is divided by its
        sum once more.  All zeros if no tree remains."""
        self._check_oob_args(x, sample_counts, "feature_importances")
        return self._importances_run(x, sample_counts.to(x.device))

    def _importances_run(self, x, counts, pairs_per_chunk: int = 1 << 24):
        n, t, nf, k = int(x.shape[0]), self.n_trees, self.n_features, self.n_outputs
        total = int(self.nodes.shape[0])
        weight = torch.zeros(total, dtype=torch.float64, device=x.device)
        first = self.tree_ptr[:-1].to(x.device)
        step = max(1, pairs_per_chunk // t)
        for r0 in range(0, n, step):
            leaf = self.apply(x[r0:r0 + step]).to(torch.int64) + first[None, :]                 # [rows, T] in the value table's numbering
            weight.index_add_(0, leaf.reshape(-1), counts[:, r0:r0 + step].t().to(torch.float64).reshape(-1))
        nodes, tree_ptr = self.nodes.cpu().numpy(), self.tree_ptr.cpu().numpy()
        offset = np.repeat(tree_ptr[:-1], np.diff(tree_ptr))
        orig = offset + nodes[:, 3]
        w = weight.cpu().numpy()[orig]                                                          # pre-order from here on
        sq = (self.value.cpu().numpy() ** 2).sum(axis=1)[orig]
        inner = nodes[:, 1] >= 0
        at = np.arange(total)
        left, right = np.where(inner, at + 1, -1), np.where(inner, offset + nodes[:, 2], -1)
        levels, frontier = [], tree_ptr[:-1]
        while frontier.size:
            levels.append(frontier)
            split = frontier[inner[frontier]]
            frontier = np.concatenate([left[split], right[split]])
        for lv in reversed(levels):                                                             # deepest level first
            split = lv[inner[lv]]
            w[split] = w[left[split]] + w[right[split]]
        split = np.flatnonzero(inner)
        gain = (w[left[split]] * sq[left[split]] + w[right[split]] * sq[right[split]] - w[split] * sq[split]) / float(k)
        tree_of = np.searchsorted(tree_ptr, split, side="right") - 1
        per_tree = np.bincount(tree_of * nf + nodes[split, 1], weights=gain, minlength=t * nf).reshape(t, nf)
        sums = per_tree.sum(axis=1)
        keep = (np.diff(tree_ptr) > 1) & (sums > 0.0)
        if not keep.any():
            return np.zeros(nf, np.float64)
        mean = (per_tree[keep] / sums[keep, None]).mean(axis=0)
        return mean / mean.sum()

    # ---- out-of-bag estimates -------------------------------------------------------------------------------------------------
    def _check_oob_args(self, x, sample_counts, what):
        """Host-side validation of (x, sample_counts), before anything is launched."""
        if not isinstance(x, torch.Tensor):
            raise ValueError(f"forest {what}: x must be a torch tensor, got {type(x).__name__}")
        if x.dim() != 2 or x.shape[1] != self.n_features or x.dtype != torch.float32:
            raise ValueError(f"forest {what}: want float32 rows of {self.n_features} features, got {tuple(x.shape)} {x.dtype}")
        n = int(x.shape[0])
        c = sample_counts
        if not isinstance(c, torch.Tensor) or c.dtype != torch.int32:
            raise ValueError(f"forest {what}: sample_counts must be an int32 tensor, got "
                             f"{c.dtype if isinstance(c, torch.Tensor) else type(c).__name__}")
        if c.dim() != 2 or tuple(c.shape) != (self.n_trees, n):
            raise ValueError(f"forest {what}: sample_counts must be [{self.n_trees}, {n}] (trees, rows of x), got {tuple(c.shape)}")
        if c.numel() and bool((c.cpu() < 0).any()):
            raise ValueError(f"forest {what}: sample_counts has a negative entry")

    def _oob_run(self, x, counts, out=None, n_oob=None):
        """(out float64 [n, K], n_oob int32 [n]) for arguments that are already checked."""
        out, n_oob, _ = ops.forest_predict_oob(x, self.nodes, self.tree_ptr, self.value, self.max_depth, counts, out=out, n_oob_out=n_oob)
        return out, n_oob

    @staticmethod
    def _warn_if_no_oob(n_oob):
        if n_oob.numel() and bool((n_oob == 0).any()):
            warnings.warn(OOB_WARNING, UserWarning, stacklevel=3)

    def oob_predict(self, x: torch.Tensor, sample_counts: torch.Tensor, return_counts: bool = False):
        """float64 [n, K] ([n] when K == 1, as ``predict``): every row scored by the trees that did not draw it -- the mean of the leaf
        values over the trees t with ``sample_counts[t, r] == 0``, scikit-learn's ``oob_prediction_`` (bit for bit with its own bags).
        ``sample_counts``: int32 [T, n], how often row r of ``x`` is in tree t's bag (``fit_info["sample_counts"]`` of a forest fitted
        with ``oob_score=True``; for a scikit-learn forest the ``bincount`` of its ``_generate_sample_indices``); checked on the host
        first (``ValueError``).  A row every tree drew gets 0.0 and one ``UserWarning`` is raised.  With ``return_counts`` the
        result is ``(prediction, n_oob)``, ``n_oob`` int32 [n] the number of out-of-bag trees per row."""
        self._check_oob_args(x, sample_counts, "oob_predict")
        out, n_oob = self._oob_run(x, sample_counts.to(x.device))
        self._warn_if_no_oob(n_oob)
        out = out[:, 0] if self.n_outputs == 1 else out
        return (out, n_oob) if return_counts else out

    def oob_permutation_importance(self, x: torch.Tensor, y: torch.Tensor, sample_counts: torch.Tensor, n_repeats: int = 1,
                                   seed: int = 0) -> np.ndarray:
        """Breiman's permutation importance from out-of-bag predictions, float64 [F] on the host:
        ``importance[f] = mean_j (mse(oob_predict(x with column f permuted by perm(f, j))) - mse(oob_predict(x)))`` with
        ``perm(f, j) = numpy.random.default_rng([seed, f, j]).permutation(n)`` and ``mse`` the float64 mean of ``(y - P)^2`` over the rows
        that have an out-of-bag tree and over the outputs (``ValueError`` if no row has one).  A feature no tree splits on scores
        exactly 0.0.  One working copy of ``x`` is made; a column is swapped in and back per feature."""
        self._check_oob_args(x, sample_counts, "oob_permutation_importance")
        n, nf, k = int(x.shape[0]), self.n_features, self.n_outputs
        if not isinstance(y, torch.Tensor) or y.dim() not in (1, 2) or y.shape[0] != n or y.numel() != n * k \
                or y.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"forest oob_permutation_importance: y must be float32 or float64 [{n}] or [{n}, {k}]")
        if int(n_repeats) < 1:
            raise ValueError(f"forest oob_permutation_importance: n_repeats must be >= 1, got {n_repeats}")
        counts = sample_counts.to(x.device)
        y64 = y.to(x.device).reshape(n, k).to(torch.float64)
        work = x.clone()
        out, n_oob = self._oob_run(work, counts)
        seen = (n_oob > 0).unsqueeze(1)
        rows = int(seen.sum())
        if rows == 0:
            raise ValueError("forest oob_permutation_importance: no row has an out-of-bag tree")

        def mse():
            return torch.where(seen, (y64 - out) ** 2, 0.0).sum() / float(rows * k)

        base = mse()
        importance = torch.zeros(nf, dtype=torch.float64, device=x.device)
        for f in range(nf):
            for j in range(int(n_repeats)):
                perm = torch.from_numpy(np.random.default_rng([int(seed), f, j]).permutation(n)).to(x.device)
                work[:, f] = x[perm, f]
                self._oob_run(work, counts, out=out, n_oob=n_oob)
                importance[f] += mse() - base
            work[:, f] = x[:, f]
        return (importance / float(n_repeats)).cpu().numpy()
