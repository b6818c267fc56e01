"""Gradient-boosted regression trees on the device: ``BoostedRegressor`` fits and scores scikit-learn's
``GradientBoostingRegressor`` (squared error) with the native kernels.

Every reference notebook that builds the random-forest mitigator imports ``GradientBoostingRegressor`` in the same line (h15, h18,
h19, h20, h21, h26, h33, h36, demo1, demo2) and ``ScikitLearningModelProcessor`` takes any fitted regressor.  This module holds such
an ensemble as registered buffers, in ``ForestRegressor``'s format, and scores it with one launch of ``mlqem_boost_predict_f32``.

Buffers (include/mlqem_hip.h documents the node record):
  ``nodes``, ``tree_ptr``, ``value`` (float64 [N, 1]), ``meta``: as in ``ForestRegressor``, one tree per stage;
  ``scale``     float64 [2]: (init, learning_rate).

``predict`` is ``((init + lr v_0) + lr v_1) + ...`` in stage order with one rounded multiply and one rounded add per stage: for an
imported model it equals scikit-learn's ``predict`` to the last bit.  ``fit`` grows the stages on the device (exact CART on the
residuals, ``mlqem_forest_fit_*``; the residual and loss update between two stages is ``mlqem_boost_update_f64``).
"""
from __future__ import annotations

import numpy as np
import torch

from ..exception import BlackwaterException
from ..native import ops
from .forest import ForestRegressor, _pack, floor_to_float32, r2_score, resolve_max_features   # noqa: F401  (floor_to_float32: _pack's rule)


def subsample_masks(n: int, n_estimators: int, subsample: float, seed: int) -> torch.Tensor:
    """int32 [n_estimators, n] of 0 and 1: stage t's bag is
    ``numpy.random.default_rng([seed, t]).permutation(n)[:max(1, int(subsample * n))]`` -- scikit-learn's bag size
    (``int(subsample * n)``, at least one row) with the project's own draws; ``subsample == 1.0`` gives all ones."""
    n, t_all = int(n), int(n_estimators)
    masks = np.ones((t_all, n), np.int32)
    if subsample < 1.0:
        take = max(1, int(subsample * n))
        masks[:] = 0
        for t in range(t_all):
            masks[t, np.random.default_rng([int(seed), t]).permutation(n)[:take]] = 1
    return torch.from_numpy(masks)


class BoostedRegressor(torch.nn.Module):
    """A fitted gradient-boosted ensemble (init + learning_rate * the sum of T single-output regression trees) as a torch module
    on the native kernels.  Build one with ``fit``, ``from_sklearn``, ``from_arrays`` or ``from_state_dict``; the array constructors
    validate the trees on the host (``ValueError``), so a malformed one never reaches the device."""

    def __init__(self, nodes: torch.Tensor, tree_ptr: torch.Tensor, value: torch.Tensor, n_features: int, max_depth: int, init: float,
                 learning_rate: float):
        super().__init__()
        self.register_buffer("nodes", nodes)
        self.register_buffer("tree_ptr", tree_ptr)
        self.register_buffer("value", value)
        self.register_buffer("meta", torch.tensor([int(n_features), int(max_depth)], dtype=torch.int64))
        self.register_buffer("scale", torch.tensor([float(init), float(learning_rate)], dtype=torch.float64))
        self._set_meta()

    def _set_meta(self):
        self.n_features, self.max_depth = (int(v) for v in self.meta.tolist())   # host copies: predict() never reads a device value
        self.init, self.learning_rate = (float(v) for v in self.scale.tolist())
        self.n_stages, self.n_outputs = int(self.tree_ptr.shape[0]) - 1, 1

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._set_meta()

    @staticmethod
    def _check_scale(init, learning_rate):
        try:
            init, learning_rate = float(init), float(learning_rate)
        except (TypeError, ValueError) as exc:
            raise ValueError("boost: scale (init, learning_rate) must be two finite numbers") from exc
        if not (np.isfinite(init) and np.isfinite(learning_rate)):
            raise ValueError(f"boost: scale (init, learning_rate) must be two finite numbers, got ({init}, {learning_rate})")
        return init, learning_rate

    @classmethod
    def from_arrays(cls, tree_ptr, feature, threshold, left, right, value, n_features, init, learning_rate) -> "BoostedRegressor":
        """``tree_ptr`` [T + 1] (one tree per stage); per node, concatenated over the stages: ``feature``, ``threshold`` (float64),
        ``left`` / ``right`` (child index WITHIN the tree, -1 for a leaf) and ``value`` [N] (or [N, 1], or scikit-learn's [N, 1, 1]);
        ``init`` and ``learning_rate`` finite floats."""
        nodes, tree_ptr, max_depth = _pack(tree_ptr, feature, threshold, left, right, n_features)
        value = np.asarray(value, dtype=np.float64)
        n = nodes.shape[0]
        if value.ndim == 3 and value.shape[2] == 1:
            value = value[:, :, 0]
        if value.ndim == 1:
            value = value[:, None]
        if value.ndim != 2 or value.shape[0] != n or value.shape[1] != 1:
            raise ValueError(f"boost: value must be [{n}] or [{n}, 1] (one output), got shape {value.shape}")
        init, learning_rate = cls._check_scale(init, learning_rate)
        value = value.reshape(n).copy().reshape(n, 1)   # unit strides, whatever view came in (a [:, None] view has column stride 0)
        return cls(torch.from_numpy(nodes), torch.from_numpy(tree_ptr), torch.from_numpy(value), n_features, max_depth, init, learning_rate)

    @classmethod
    def fit(cls, x: torch.Tensor, y: torch.Tensor, *, n_estimators: int = 100, learning_rate: float = 0.1, max_depth: int = 3,
            min_samples_split: int = 2, min_samples_leaf: int = 1, subsample: float = 1.0, max_features=None, seed: int = 0,
            sample_masks=None, eval_set=None) -> "BoostedRegressor":
        """``GradientBoostingRegressor(n_estimators, learning_rate, max_depth, ...).fit(x, y)`` with scikit-learn's defaults --
        squared-error loss, the mean of ``y`` as the initial prediction -- grown on ``x.device``: stage t is one exact CART tree
        (the rule of include/mlqem_hip.h; scikit-learn's ``friedman_mse`` orders a node's candidates as squared error does) on the
        residuals of the stages before it, and adds ``learning_rate * value[leaf]`` to every row's prediction.

        ``x``: float32 [n, F] device tensor; ``y``: [n] or [n, 1] on the same device, float32 or float64 (widened first).  Single
        output only: fit one model per column for more.  ``max_depth`` is an int >= 1 (it sizes the node store).  ``subsample`` < 1
        gives stage t the bag of ``subsample_masks(n, n_estimators, subsample, seed)`` (scikit-learn's bag size, the project's own
        draws); ``sample_masks``, int32 [T, n] of 0 and 1, overrides ``subsample`` and ``n_estimators``.  ``max_features``: as
        ``ForestRegressor.fit`` (with m < F a node's feature order is a function of (``seed``, stage, node)).  Equal scores are broken
        by the lowest feature, then the lowest position: a stage equals scikit-learn's where no two candidates tie.  Two fits give
        the same buffers bit for bit.

        Sets ``train_score_`` (float64 [T], host: the mean squared residual over stage t's bag after its update), ``oob_improvement_``
        (float64 [T], host, when any bag is partial: the mean squared residual over the rows outside the bag before stage t less the
        one after it) and ``fit_info`` (``levels``, ``n_node_samples``, ``sample_masks``).  With ``eval_set=(xv, yv)`` one staged predict
        after the fit gives ``validation_score_`` (float64 [T], host: the mean squared error on the set after every stage) and
        ``best_n_estimators_`` (its argmin + 1); the fit never stops early -- ``truncated(best_n_estimators_)`` is the shorter model.

        Not supported: other losses, ``n_iter_no_change``, ``warm_start``, ``ccp_alpha``, multi-output trees.  Every argument is
        checked on the host before anything is launched (``ValueError`` / ``BlackwaterException``); the finished node tables go through
        the validation of ``from_arrays``."""
        if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
            raise ValueError("boost fit: x and y must be torch tensors")
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError(f"boost fit: x must be float32 [n, F], got {tuple(x.shape)} {x.dtype}")
        n, f = int(x.shape[0]), int(x.shape[1])
        if y.dim() not in (1, 2) or y.shape[0] != n or y.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"boost fit: y must be float32 or float64 [{n}] or [{n}, 1], got {tuple(y.shape)} {y.dtype}")
        if y.dim() == 2 and y.shape[1] != 1:
            raise ValueError(f"boost fit: y has {int(y.shape[1])} outputs; boosted trees have one output: fit one model per column "
                             "(as scikit-learn's MultiOutputRegressor does)")
        if n < 1 or n > ops.FOREST_FIT_MAX_ROWS:
            raise ValueError(f"boost fit: want 1 <= n <= {ops.FOREST_FIT_MAX_ROWS} rows, got {n}")
        if not 1 <= f <= ops.FOREST_MAX_FEATURES:
            raise ValueError(f"boost fit: want 1 <= F <= {ops.FOREST_MAX_FEATURES} features, got {f}")
        if isinstance(max_depth, bool) or not isinstance(max_depth, (int, np.integer)) or not 1 <= max_depth <= ops.BOOST_MAX_DEPTH:
            raise ValueError(f"boost fit: max_depth must be an int in 1..{ops.BOOST_MAX_DEPTH} (it sizes the node store), got {max_depth!r}")
        if min_samples_split < 2 or min_samples_leaf < 1:
            raise ValueError(f"boost fit: want min_samples_split >= 2 and min_samples_leaf >= 1, got {min_samples_split}, {min_samples_leaf}")
        if not np.isfinite(learning_rate) or learning_rate <= 0.0:
            raise ValueError(f"boost fit: learning_rate must be a positive finite number, got {learning_rate}")
        m = resolve_max_features(max_features, f)
        if sample_masks is None:
            if n_estimators < 1:
                raise ValueError(f"boost fit: n_estimators must be >= 1, got {n_estimators}")
            if not 0.0 < subsample <= 1.0:
                raise ValueError(f"boost fit: subsample must be in (0, 1], got {subsample}")
            masks = subsample_masks(n, n_estimators, subsample, seed)
        else:
            masks = sample_masks
            if not isinstance(masks, torch.Tensor) or masks.dtype != torch.int32 or masks.dim() != 2 or masks.shape[0] < 1 \
                    or masks.shape[1] != n:
                raise ValueError(f"boost fit: sample_masks must be an int32 [T, {n}] tensor with T >= 1")
            host = masks.cpu()
            if bool(((host != 0) & (host != 1)).any()):
                raise ValueError("boost fit: sample_masks must hold 0 and 1 only")
            if bool((host.max(dim=1).values < 1).any()):
                raise ValueError(f"boost fit: stage {int(torch.nonzero(host.max(dim=1).values < 1)[0])} has an empty bag")
        if eval_set is not None:
            if not isinstance(eval_set, (tuple, list)) or len(eval_set) != 2 or not all(isinstance(a, torch.Tensor) for a in eval_set):
                raise ValueError("boost fit: eval_set must be (x, y), two torch tensors")
            xv, yv = eval_set
            if xv.dim() != 2 or xv.shape[1] != f or xv.dtype != torch.float32 or xv.shape[0] < 1 or yv.dim() not in (1, 2) \
                    or yv.numel() != xv.shape[0] or yv.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"boost fit: eval_set must be (float32 [m, {f}], float [m]) with m >= 1, got {tuple(xv.shape)} {xv.dtype} "
                                 f"and {tuple(yv.shape)} {yv.dtype}")
        if not x.is_cuda or y.device != x.device or (eval_set is not None and any(a.device != x.device for a in eval_set)):
            raise BlackwaterException(f"boost fit: x and y must live on one GPU (got {x.device} and {y.device}); there is no CPU path")
        if f == 1 and n > 1 and x.stride(1) != 1:   # a [n, 1] view may carry any column stride
            x = x.as_strided((n, 1), (x.stride(0), 1))
        y64 = y.reshape(n).to(torch.float64).contiguous()
        if not bool(torch.isfinite(x).all() & torch.isfinite(y64).all()):   # one reduction, one wait
            raise ValueError("boost fit: x or y holds a NaN or an infinity")
        masks = masks.to(x.device).contiguous()
        grown = ops.boost_fit(x, y64, masks, learning_rate=float(learning_rate), max_depth=int(max_depth),
                              min_samples_split=int(min_samples_split), min_samples_leaf=int(min_samples_leaf), max_features=m,
                              seed=int(seed))
        model = cls.from_arrays(*(grown[key] for key in ("tree_ptr", "feature", "threshold", "left", "right", "value")), n_features=f,
                                init=grown["init"], learning_rate=float(learning_rate)).to(x.device)
        model.train_score_ = grown["train_score"]
        if grown["oob_improvement"] is not None:
            model.oob_improvement_ = grown["oob_improvement"]
        model.fit_info = {"levels": grown["levels"], "n_node_samples": grown["n_node_samples"], "sample_masks": masks, "max_features": m}
        if eval_set is not None:
            staged = model.staged_predict(xv)
            err = staged - yv.reshape(1, -1).to(torch.float64)
            model.validation_score_ = (err * err).mean(dim=1).cpu().numpy()
            model.best_n_estimators_ = int(np.argmin(model.validation_score_)) + 1
        return model

    @classmethod
    def from_sklearn(cls, model) -> "BoostedRegressor":
        """From a fitted ``GradientBoostingRegressor`` with ``loss="squared_error"`` and ``init`` None (the mean) or ``"zero"``."""
        try:
            from sklearn.ensemble import GradientBoostingRegressor
        except ImportError as exc:
            raise BlackwaterException("BoostedRegressor.from_sklearn needs scikit-learn; use from_arrays or from_state_dict") from exc
        if not isinstance(model, GradientBoostingRegressor):
            raise BlackwaterException(f"BoostedRegressor.from_sklearn takes a fitted GradientBoostingRegressor, got {type(model).__name__}")
        if not hasattr(model, "estimators_"):
            raise BlackwaterException("GradientBoostingRegressor is not fitted")
        if model.loss != "squared_error":
            raise BlackwaterException(f"BoostedRegressor.from_sklearn: loss={model.loss!r} is not supported (squared_error only)")
        if model.init is None:
            init = float(np.ravel(model.init_.constant_)[0])   # DummyRegressor(strategy="mean")
        elif isinstance(model.init, str) and model.init == "zero":
            init = 0.0
        else:
            raise BlackwaterException(f"BoostedRegressor.from_sklearn: init={model.init!r} is not supported (None or \"zero\" only)")
        if model.estimators_.ndim != 2 or model.estimators_.shape[1] != 1:
            raise BlackwaterException(f"BoostedRegressor.from_sklearn: estimators_ of shape {model.estimators_.shape} is not supported "
                                      "(one tree per stage only)")
        trees = [est.tree_ for est in model.estimators_[:, 0]]
        tree_ptr = np.concatenate([[0], np.cumsum([t.node_count for t in trees])]).astype(np.int64)
        cat = lambda name: np.concatenate([getattr(t, name) for t in trees])  # noqa: E731
        return cls.from_arrays(tree_ptr, cat("feature"), cat("threshold"), cat("children_left"), cat("children_right"), cat("value"),
                               int(model.n_features_in_), init, float(model.learning_rate))

    @classmethod
    def from_state_dict(cls, state_dict) -> "BoostedRegressor":
        """A module with buffers of the checkpoint's sizes, strict-loaded (the forest's checks, and a finite ``scale``)."""
        missing = [k for k in ("nodes", "tree_ptr", "value", "meta", "scale") if k not in state_dict]
        if missing:
            raise ValueError(f"boost checkpoint lacks {missing}")
        nodes, tree_ptr, value, meta, scale = (state_dict[k] for k in ("nodes", "tree_ptr", "value", "meta", "scale"))
        if (nodes.dtype != torch.int32 or nodes.dim() != 2 or nodes.shape[1] != 4 or tree_ptr.dtype != torch.int64 or tree_ptr.dim() != 1
                or tree_ptr.numel() < 2 or value.dtype != torch.float64 or value.dim() != 2 or value.shape[0] != nodes.shape[0]
                or value.shape[1] != 1 or meta.dtype != torch.int64 or tuple(meta.shape) != (2,) or scale.dtype != torch.float64
                or tuple(scale.shape) != (2,)):
            raise ValueError("boost checkpoint: buffers have the wrong dtype or shape")
        counts = tree_ptr[1:] - tree_ptr[:-1]
        if int(tree_ptr[0]) != 0 or int(tree_ptr[-1]) != nodes.shape[0] or bool((counts < 1).any()):
            raise ValueError("boost checkpoint: tree_ptr does not partition the nodes")
        f, depth = (int(v) for v in meta.tolist())
        if not 1 <= f <= ops.FOREST_MAX_FEATURES or not 0 <= depth < nodes.shape[0]:
            raise ValueError("boost checkpoint: meta (n_features, max_depth) is out of range")
        if not bool(torch.isfinite(scale).all()):
            raise ValueError("boost checkpoint: scale (init, learning_rate) is not finite")
        module = cls(torch.empty_like(nodes, device="cpu"), torch.empty_like(tree_ptr, device="cpu"),
                     torch.empty_like(value, device="cpu"), f, depth, 0.0, 0.0)
        module.load_state_dict(state_dict, strict=True)
        return module

    def _check_rows(self, x):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != self.n_features:
            raise ValueError(f"boost: want rows of {self.n_features} features, got "
                             f"{tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")

    def _run(self, x: torch.Tensor, n_stages=None, staged: bool = False):
        self._check_rows(x)
        return ops.boost_predict(x, self.nodes, self.tree_ptr, self.value, self.max_depth, self.init, self.learning_rate,
                                 n_stages=n_stages, staged=staged)

    def predict(self, x: torch.Tensor, n_stages=None) -> torch.Tensor:
        """float64 [n]: ``init + learning_rate * (v_0 + ...)`` summed in stage order over the first ``n_stages`` stages (all when None)."""
        return self._run(x, n_stages)[0]

    def staged_predict(self, x: torch.Tensor) -> torch.Tensor:
        """float64 [T, n]: the prediction after every stage (scikit-learn's ``staged_predict``, as one tensor), from one launch."""
        return self._run(x, None, True)[1]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """float32 [n, 1]: ``predict`` rounded, so the module composes with float32 torch code."""
        return self._run(x)[0].to(torch.float32).unsqueeze(1)

    def apply(self, x: torch.Tensor) -> torch.Tensor:
        """int32 [n, T]: the leaf every stage puts each row in, in the model's own node numbering (scikit-learn's ``apply``); the
        forest kernel's walk over the same node records."""
        self._check_rows(x)
        return ops.forest_predict(x, self.nodes, self.tree_ptr, self.value, self.max_depth, want_leaf=True)[1]

    def score(self, x: torch.Tensor, y: torch.Tensor) -> float:
        """R^2 of ``predict(x)`` against ``y`` ([n] or [n, 1] on ``x``'s device): scikit-learn's ``score`` (see ``r2_score``)."""
        pred = self._run(x)[0]
        if not isinstance(y, torch.Tensor) or y.dim() not in (1, 2) or y.numel() != pred.numel() or y.shape[0] != pred.shape[0]:
            raise ValueError(f"boost score: y must be a [{pred.shape[0]}] or [{pred.shape[0]}, 1] tensor")
        return float(r2_score(y.to(pred.device), pred))

    def truncated(self, m: int) -> "BoostedRegressor":
        """A model of the first ``m`` stages (1 <= m <= T) on the same device: ``truncated(m).predict(x)`` equals
        ``predict(x, n_stages=m)``.  The value table keeps the model's own node order, so a prefix of the stages is a prefix of it."""
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= self.n_stages:
            raise ValueError(f"boost truncated: m must be an int in 1..{self.n_stages}, got {m!r}")
        tree_ptr = self.tree_ptr[:int(m) + 1].clone()
        end = int(tree_ptr[-1])
        nodes = self.nodes[:end].clone()
        host, ptr = nodes.cpu().numpy(), tree_ptr.cpu().numpy()
        depth = _packed_depth(host, ptr)
        return type(self)(nodes, tree_ptr, self.value[:end].clone(), self.n_features, depth, self.init, self.learning_rate).to(self.nodes.device)

    def feature_importances(self, x: torch.Tensor, sample_masks: torch.Tensor) -> np.ndarray:
        """scikit-learn's ``feature_importances_`` of a boosted ensemble, float64 [F] on the host, from the training rows ``x`` and the
        stages' bags ``sample_masks`` (int32 [T, n]; ``fit_info["sample_masks"]``): per stage the impurity gains are added per feature
        and divided by their sum, the mean over the stages that split is divided by its sum once more -- the forest's routine
        (``ForestRegressor.feature_importances`` states the gain) over the stages' trees."""
        as_forest = ForestRegressor(self.nodes, self.tree_ptr, self.value, self.n_features, self.max_depth)
        as_forest._check_oob_args(x, sample_masks, "feature_importances")
        return as_forest._importances_run(x, sample_masks.to(x.device))


def _packed_depth(nodes: np.ndarray, tree_ptr: np.ndarray) -> int:
    """The largest depth of a leaf in packed pre-order trees (nodes int32 [N, 4] = thr bits, feature or -1, right, orig)."""
    offset = np.repeat(tree_ptr[:-1], np.diff(tree_ptr))
    depth = np.zeros(nodes.shape[0], np.int64)
    frontier, d = tree_ptr[:-1].astype(np.int64), 0
    while frontier.size:
        depth[frontier] = d
        split = frontier[nodes[frontier, 1] >= 0]
        frontier = np.concatenate([split + 1, offset[split] + nodes[split, 2]])
        d += 1
    return int(depth.max())
