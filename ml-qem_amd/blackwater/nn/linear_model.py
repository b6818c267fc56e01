"""Linear least squares on the device: ``LinearRegressor`` fits and scores the reference's OLS mitigator with the native kernels.

The reference's OLS baseline is a scikit-learn ``LinearRegression`` on ``encode_data`` rows (docs/tutorials/h12_ols.ipynb fits it,
h17_compare_over_steps.ipynb scores it, the VQE drivers use it through ``ScikitLearningModelProcessor``).  Here the fit is one
streaming pass over the rows on the device -- ``ops.linreg_moments`` forms A^T A for A = [1 | x | y] in float64 -- and a solve of at
most 529 x 529 on the host (``solve_moments``); scoring is one launch of ``ops.linreg_predict``.

Buffers (so ``.to(device)``, ``state_dict()`` and ``load_state_dict(strict=True)`` work):
  ``coef``       float64 [K, F]   scikit-learn's ``coef_`` (a 1-D ``coef_`` is stored as one row);
  ``intercept``  float64 [K];
  ``meta``       int64 [3]: (number of features, rank of the fit or -1, rows seen by the fit or -1).
"""
from __future__ import annotations

import numpy as np
import torch

from ..exception import BlackwaterException
from ..native import ops


def solve_moments(moments, F, K, alpha=0.0, rcond=1e-10):
    """``(coef [K, F], intercept [K], rank)`` from the float64 moments M = A^T A of A = [1 | x | y] ([D, D], D = 1 + F + K).

    With n = M[0, 0], s = M[0, 1:], Cxx = Mxx - s_x s_x^T / n and Cxy = Mxy - s_x s_y^T / n (the centred scatter matrices):
    ``eigh(Cxx)``; the eigenpairs with lambda > rcond * lambda_max are kept (with ``alpha > 0`` all are, negatives clamped to 0);
    B = V diag(1 / (lambda + alpha)) V^T Cxy; intercept = ybar - xbar B; rank = the number of eigenpairs kept.  ``alpha = 0`` is
    the minimum-norm least-squares solution with an intercept (``LinearRegression``), ``alpha > 0`` is ``Ridge(alpha)``.

    When no column of x varies (lambda_max <= 0) and ``alpha == 0`` there is nothing to regress on: coef is 0, the intercept is
    ybar and the rank is 0.  ``ValueError`` for n < 1, a non-finite moment or a matrix of the wrong shape.

    Two limits.  Rank decisions: ``rcond`` acts on eigenvalues of the covariance, i.e. on SQUARED singular values of the centred
    rows, so a rank decision matches ``lstsq`` only where the singular-value gap is wider than about 1e-5 sigma_max
    (sqrt(rcond)).  Centring: Cxx is formed by subtraction, which loses digits once |mean| / std of a column approaches 1e5
    (about 2 log10(|mean| / std) of the 16); the ``encode_data`` columns are far from that."""
    F, K = int(F), int(K)
    M = np.asarray(moments, dtype=np.float64)
    D = 1 + F + K
    if F < 1 or K < 1 or M.shape != (D, D):
        raise ValueError(f"solve_moments: want moments [{D}, {D}] for F = {F}, K = {K}, got {M.shape}")
    if not np.isfinite(M).all():
        raise ValueError("solve_moments: a moment is not finite (a NaN or an infinity in the rows?)")
    if alpha < 0 or not rcond >= 0:
        raise ValueError("solve_moments: alpha and rcond must not be negative")
    n = M[0, 0]
    if n < 1:
        raise ValueError(f"solve_moments: the moments hold {n:g} rows; a fit needs at least one")
    sx, sy = M[0, 1:1 + F], M[0, 1 + F:]
    cxx = M[1:1 + F, 1:1 + F] - np.outer(sx, sx) / n
    cxy = M[1:1 + F, 1 + F:] - np.outer(sx, sy) / n
    lam, vec = np.linalg.eigh((cxx + cxx.T) / 2)
    lam_max = float(lam[-1])
    if alpha > 0:
        keep = np.ones(F, dtype=bool)
        inv = 1.0 / (np.maximum(lam, 0.0) + alpha)
    elif lam_max <= 0:
        keep = np.zeros(F, dtype=bool)
        inv = np.zeros(F)
    else:
        keep = lam > rcond * lam_max
        inv = np.where(keep, 1.0 / np.where(keep, lam, 1.0), 0.0)
    B = vec @ (inv[:, None] * (vec.T @ cxy))              # [F, K]
    intercept = sy / n - (sx / n) @ B
    return np.ascontiguousarray(B.T), intercept, int(keep.sum())


def _check_arrays(coef, intercept):
    """(coef float64 [K, F], intercept float64 [K]) from array-likes; a 1-D coef with a scalar intercept is one output."""
    coef, intercept = np.asarray(coef), np.asarray(intercept)
    for name, a in (("coef", coef), ("intercept", intercept)):
        if a.dtype.kind not in "fiu":
            raise ValueError(f"linear model: {name} must be a real numeric array, got dtype {a.dtype}")
    if coef.ndim == 1:
        if intercept.ndim != 0 and intercept.shape != (1,):
            raise ValueError(f"linear model: a 1-D coef takes a scalar intercept, got shape {intercept.shape}")
        coef, intercept = coef[None, :], intercept.reshape(1)
    if coef.ndim != 2:
        raise ValueError(f"linear model: coef must be [K, F] or [F], got shape {coef.shape}")
    k, f = coef.shape
    if not 1 <= f <= ops.LINREG_MAX_FEATURES or not 1 <= k <= ops.LINREG_MAX_OUTPUTS:
        raise ValueError(f"linear model: want 1 <= F <= {ops.LINREG_MAX_FEATURES} and 1 <= K <= {ops.LINREG_MAX_OUTPUTS}, got "
                         f"coef {coef.shape}")
    if intercept.ndim == 0 and k == 1:
        intercept = intercept.reshape(1)
    if intercept.shape != (k,):
        raise ValueError(f"linear model: intercept must have one entry per output ({k}), got shape {intercept.shape}")
    coef, intercept = coef.astype(np.float64), intercept.astype(np.float64)   # float32 (the reference's pickles) widens exactly
    if not np.isfinite(coef).all() or not np.isfinite(intercept).all():
        raise ValueError("linear model: coef and intercept must be finite")
    return np.ascontiguousarray(coef), np.ascontiguousarray(intercept)


class LinearRegressor(torch.nn.Module):
    """A linear model y = intercept + coef x with K outputs as a torch module on the native kernels.

    Build one with ``fit`` (on the device), ``from_sklearn``, ``from_arrays`` or ``from_state_dict``; the array constructors
    validate on the host (``ValueError``)."""

    def __init__(self, coef: torch.Tensor, intercept: torch.Tensor, n_features: int, rank: int = -1, n_rows_seen: int = -1):
        super().__init__()
        self.register_buffer("coef", coef)
        self.register_buffer("intercept", intercept)
        self.register_buffer("meta", torch.tensor([int(n_features), int(rank), int(n_rows_seen)], dtype=torch.int64))
        self._set_meta()

    def _set_meta(self):
        # host copies: predict() never reads a device value
        self.n_features, self.rank_, self.n_rows_seen = (int(v) for v in self.meta.tolist())
        self.n_outputs = int(self.coef.shape[0])

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._set_meta()

    @classmethod
    def from_arrays(cls, coef, intercept, rank: int = -1, n_rows_seen: int = -1) -> "LinearRegressor":
        """``coef`` [K, F] with ``intercept`` [K], or a 1-D ``coef`` [F] with a scalar intercept (then K = 1 and ``predict`` returns
        [n], as scikit-learn does)."""
        coef, intercept = _check_arrays(coef, intercept)
        return cls(torch.from_numpy(coef), torch.from_numpy(intercept), coef.shape[1], rank, n_rows_seen)

    @classmethod
    def from_sklearn(cls, model) -> "LinearRegressor":
        """From a fitted ``LinearRegression`` or ``Ridge``."""
        try:
            from sklearn.linear_model import LinearRegression, Ridge
        except ImportError as exc:
            raise BlackwaterException("LinearRegressor.from_sklearn needs scikit-learn; use from_arrays or from_state_dict") from exc
        if not isinstance(model, (LinearRegression, Ridge)):
            raise BlackwaterException(f"LinearRegressor.from_sklearn takes a fitted LinearRegression or Ridge, got {type(model).__name__}")
        if not hasattr(model, "coef_") or not hasattr(model, "intercept_"):
            raise BlackwaterException(f"{type(model).__name__} is not fitted")
        coef = np.asarray(model.coef_)
        intercept = np.asarray(model.intercept_, dtype=coef.dtype)
        if intercept.ndim == 0 and coef.ndim == 2:        # fit_intercept=False: the scalar 0.0 for every output
            intercept = np.full(coef.shape[0], float(intercept), dtype=coef.dtype)
        return cls.from_arrays(coef, intercept, rank=int(getattr(model, "rank_", -1)))

    @classmethod
    def from_state_dict(cls, state_dict) -> "LinearRegressor":
        """A module with buffers of the checkpoint's sizes, strict-loaded."""
        missing = [k for k in ("coef", "intercept", "meta") if k not in state_dict]
        if missing:
            raise ValueError(f"linear-model checkpoint lacks {missing}")
        coef, intercept, meta = (state_dict[k] for k in ("coef", "intercept", "meta"))
        if (coef.dtype != torch.float64 or coef.dim() != 2 or intercept.dtype != torch.float64 or intercept.dim() != 1
                or intercept.shape[0] != coef.shape[0] or meta.dtype != torch.int64 or tuple(meta.shape) != (3,)):
            raise ValueError("linear-model checkpoint: buffers have the wrong dtype or shape")
        f, rank, seen = (int(v) for v in meta.tolist())
        k = int(coef.shape[0])
        if (f != coef.shape[1] or not 1 <= f <= ops.LINREG_MAX_FEATURES or not 1 <= k <= ops.LINREG_MAX_OUTPUTS or not -1 <= rank <= f
                or seen < -1):
            raise ValueError("linear-model checkpoint: meta (n_features, rank, n_rows_seen) does not fit the buffers")
        module = cls(torch.empty_like(coef, device="cpu"), torch.empty_like(intercept, device="cpu"), f, rank, seen)
        module.load_state_dict(state_dict, strict=True)
        return module

    class Accumulator:
        """A streaming fit: ``update(x, y)`` adds a shard's moments on the device (``ops.linreg_moments(accumulate=True)``),
        ``solve`` copies the [D, D] matrix to the host once and solves."""

        def __init__(self, F: int, K: int, device="cuda"):
            F, K = int(F), int(K)
            if not 1 <= F <= ops.LINREG_MAX_FEATURES or not 1 <= K <= ops.LINREG_MAX_OUTPUTS:
                raise ValueError(f"linear model: want 1 <= F <= {ops.LINREG_MAX_FEATURES} and 1 <= K <= {ops.LINREG_MAX_OUTPUTS}, "
                                 f"got F = {F}, K = {K}")
            self.n_features, self.n_outputs = F, K
            self.moments = torch.zeros((1 + F + K, 1 + F + K), dtype=torch.float64, device=device)

        def update(self, x: torch.Tensor, y: torch.Tensor) -> "LinearRegressor.Accumulator":
            y = y[:, None] if y.dim() == 1 else y
            if x.dim() != 2 or y.dim() != 2 or x.shape[1] != self.n_features or y.shape[1] != self.n_outputs:
                raise ValueError(f"linear model: want x [n, {self.n_features}] and y [n, {self.n_outputs}], got {tuple(x.shape)} and "
                                 f"{tuple(y.shape)}")
            ops.linreg_moments(x, y, out=self.moments, accumulate=True)
            return self

        def solve(self, alpha: float = 0.0, rcond: float = 1e-10) -> "LinearRegressor":
            m = self.moments.cpu().numpy()                 # the fit's one device-to-host copy
            coef, intercept, rank = solve_moments(m, self.n_features, self.n_outputs, alpha=alpha, rcond=rcond)
            model = LinearRegressor(torch.from_numpy(coef), torch.from_numpy(np.ascontiguousarray(intercept)), self.n_features, rank,
                                    int(round(m[0, 0])))
            return model.to(self.moments.device)

    @classmethod
    def fit(cls, x: torch.Tensor, y: torch.Tensor, alpha: float = 0.0, rcond: float = 1e-10) -> "LinearRegressor":
        """Least squares (``alpha = 0``) or ridge regression of ``y`` (float32 [n, K] or [n]) on ``x`` (float32 [n, F]), both on the
        device: one moments launch, one [D, D] copy to the host, the host solve.  The model comes back on x's device."""
        if x.dim() != 2 or y.dim() not in (1, 2):
            raise ValueError(f"linear model: want x [n, F] and y [n, K] or [n], got {tuple(x.shape)} and {tuple(y.shape)}")
        y2 = y[:, None] if y.dim() == 1 else y
        acc = cls.Accumulator(x.shape[1], y2.shape[1], x.device)
        ops.linreg_moments(x, y2, out=acc.moments)
        return acc.solve(alpha, rcond)

    def _run(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 2 or x.shape[1] != self.n_features:
            raise ValueError(f"linear model: want rows of {self.n_features} features, got {tuple(x.shape)}")
        return ops.linreg_predict(x, self.coef, self.intercept)

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """float64 [n, K] ([n] when K == 1, as ``ForestRegressor.predict`` and as scikit-learn for a 1-D ``coef_``)."""
        out = self._run(x)
        return out[:, 0] if self.n_outputs == 1 else out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """float32 [n, K]: ``predict`` rounded, so the module composes with float32 torch code."""
        return self._run(x).to(torch.float32)
