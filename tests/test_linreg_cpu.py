"""Host-side checks of the least-squares path (blackwater.nn.LinearRegressor): the solve rule against lstsq, ridge, the
constructors' validation, the checkpoint route, the fixture and the entry points' argument checks.  Nothing here touches a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from blackwater.exception import BlackwaterException
from blackwater.nn import LinearRegressor
from blackwater.nn.linear_model import solve_moments
from linreg_cases import (EXACT_G5, GOLDEN, PRINTED_G5, fit_problems, lstsq_predictions, mean_l2, moments_oracle, predict_oracle,
                          seeded_problem)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "ols_g1.npz")))


@pytest.fixture(scope="module")
def ideal():
    return np.load(os.path.join(GOLDEN, "g1_dataset.npz"))["ideal"].astype(np.float64)


@pytest.mark.parametrize("name,X,Y,rank", fit_problems(), ids=[p[0] for p in fit_problems()])
def test_solve_moments_equals_lstsq(name, X, Y, rank):
    F, K = X.shape[1], Y.shape[1]
    coef, intercept, got_rank = solve_moments(moments_oracle(X, Y), F, K)
    assert coef.shape == (K, F) and intercept.shape == (K,) and coef.dtype == np.float64
    assert got_rank == rank
    gap = float(np.abs(predict_oracle(X, coef, intercept) - lstsq_predictions(X, Y)).max())
    print(f"{name}: rank {got_rank}, max |solve_moments - lstsq| on the training rows = {gap:.3e}")
    assert gap <= 1e-9


def test_ridge_equals_the_closed_form():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((500, 12)).astype(np.float32)
    Y = (X @ rng.standard_normal((12, 3)) + 0.1 * rng.standard_normal((500, 3))).astype(np.float32)
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    xc, yc = Xd - Xd.mean(0), Yd - Yd.mean(0)
    for alpha in (1e-3, 1.0, 50.0):
        coef, intercept, rank = solve_moments(moments_oracle(X, Y), 12, 3, alpha=alpha)
        B = np.linalg.solve(xc.T @ xc + alpha * np.eye(12), xc.T @ yc)
        assert rank == 12
        assert np.abs(coef - B.T).max() <= 1e-12 and np.abs(intercept - (Yd.mean(0) - Xd.mean(0) @ B)).max() <= 1e-12
    # alpha > 0 keeps every direction, a rank-deficient input included (the duplicated column shares its weight)
    X, Y = seeded_problem(65, 3, 1)
    coef, _, rank = solve_moments(moments_oracle(X, Y), 3, 1, alpha=1.0)
    assert rank == 3 and np.isfinite(coef).all() and abs(coef[0, 0] - coef[0, 2]) <= 1e-12


def test_solve_moments_refuses_what_it_cannot_fit():
    X, Y = seeded_problem(65, 3, 1)
    M = moments_oracle(X, Y)
    with pytest.raises(ValueError, match="at least one"):
        solve_moments(np.zeros((5, 5)), 3, 1)
    for bad in (np.nan, np.inf):
        Mb = M.copy()
        Mb[2, 3] = bad
        with pytest.raises(ValueError, match="not finite"):
            solve_moments(Mb, 3, 1)
    with pytest.raises(ValueError):
        solve_moments(M, 4, 1)            # wrong shape for F
    with pytest.raises(ValueError):
        solve_moments(M, 3, 1, alpha=-1.0)
    # no column varies: nothing to regress on -- coef 0, intercept = the mean of y, rank 0 (decided; documented in solve_moments)
    Xc = np.full((40, 3), 0.25, np.float32)
    Yc = np.random.default_rng(0).standard_normal((40, 2)).astype(np.float32)
    coef, intercept, rank = solve_moments(moments_oracle(Xc, Yc), 3, 2)
    assert rank == 0 and not coef.any() and np.abs(intercept - Yc.astype(np.float64).mean(0)).max() <= 1e-15


def test_constructors_validate_on_the_host():
    ok = LinearRegressor.from_arrays(np.ones((4, 58), np.float32), np.zeros(4, np.float32))
    assert (ok.n_features, ok.n_outputs, ok.rank_, ok.n_rows_seen) == (58, 4, -1, -1)
    assert ok.coef.dtype == torch.float64 and ok.intercept.dtype == torch.float64 and ok.meta.dtype == torch.int64
    assert not list(ok.parameters())
    one = LinearRegressor.from_arrays(np.arange(5.0), 2.0)          # a 1-D coef with a scalar intercept: one output
    assert (one.n_features, one.n_outputs) == (5, 1) and tuple(one.coef.shape) == (1, 5) and one.intercept.tolist() == [2.0]
    for coef, intercept in ((np.ones((4, 58)), np.zeros(3)), (np.ones((4, 58)), 0.0), (np.ones(5), np.zeros(2)),
                            (np.ones((17, 5)), np.zeros(17)), (np.ones((2, 513)), np.zeros(2)), (np.ones((2, 0)), np.zeros(2)),
                            (np.ones((2, 3, 4)), np.zeros(2)), (np.array([[1.0, np.nan]]), np.zeros(1)),
                            (np.ones((1, 2)), np.array([np.inf])), (np.ones((1, 2), dtype=complex), np.zeros(1)),
                            (np.array([["a", "b"]]), np.zeros(1))):
        with pytest.raises(ValueError):
            LinearRegressor.from_arrays(coef, intercept)
    for F, K in ((0, 1), (513, 1), (3, 0), (3, 17)):
        with pytest.raises(ValueError):
            LinearRegressor.Accumulator(F, K, "cpu")
    # float32 widens exactly
    c32 = np.random.default_rng(0).standard_normal((2, 7)).astype(np.float32)
    assert np.array_equal(LinearRegressor.from_arrays(c32, np.zeros(2, np.float32)).coef.numpy(), c32.astype(np.float64))


def test_from_sklearn_round_trip():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestRegressor
    from sklearn.linear_model import Lasso, LinearRegression, Ridge

    rng = np.random.default_rng(1)
    X = rng.standard_normal((120, 7)).astype(np.float32)
    Y = rng.standard_normal((120, 3)).astype(np.float32)
    for model in (LinearRegression().fit(X, Y), Ridge(alpha=0.5).fit(X, Y), LinearRegression(fit_intercept=False).fit(X, Y)):
        got = LinearRegressor.from_sklearn(model)
        assert (got.n_features, got.n_outputs) == (7, 3)
        assert np.array_equal(got.coef.numpy(), np.asarray(model.coef_, np.float64))
        assert np.array_equal(got.intercept.numpy(), np.broadcast_to(np.asarray(model.intercept_, np.float64), (3,)))
    one = LinearRegressor.from_sklearn(LinearRegression().fit(X, Y[:, 0]))    # 1-D coef_, scalar intercept_
    assert (one.n_features, one.n_outputs) == (7, 1) and one.rank_ == 7
    # our own solve agrees with scikit-learn's fit (fp64 inputs: scikit-learn fits float32 data in float32)
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    for model, alpha in ((LinearRegression().fit(Xd, Yd), 0.0), (Ridge(alpha=0.5).fit(Xd, Yd), 0.5)):
        coef, intercept, _ = solve_moments(moments_oracle(X, Y), 7, 3, alpha=alpha)
        assert np.abs(coef - model.coef_).max() <= 1e-12 and np.abs(intercept - model.intercept_).max() <= 1e-12
    for bad in (LinearRegression(), Ridge(), Lasso().fit(X, Y), RandomForestRegressor(n_estimators=2).fit(X, Y), object()):
        with pytest.raises(BlackwaterException):
            LinearRegressor.from_sklearn(bad)


def test_state_dict_round_trip(fx, tmp_path):
    model = LinearRegressor.from_arrays(fx["coef"], fx["intercept"], rank=int(fx["rank"]), n_rows_seen=1234)
    sd = model.state_dict()
    assert set(sd) == {"coef", "intercept", "meta"}
    path = tmp_path / "ols.pth"
    torch.save(sd, path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    again = LinearRegressor.from_state_dict(loaded)
    for k in sd:
        assert again.state_dict()[k].dtype == sd[k].dtype and again.state_dict()[k].numpy().tobytes() == sd[k].numpy().tobytes()
    assert (again.n_features, again.n_outputs, again.rank_, again.n_rows_seen) == (58, 4, 14, 1234)
    model.load_state_dict(loaded, strict=True)                      # same sizes: the plain route works too
    other = LinearRegressor.from_arrays(np.ones((2, 5)), np.zeros(2))
    with pytest.raises(RuntimeError):
        other.load_state_dict(loaded, strict=True)                  # another model's sizes
    for drop in sd:
        with pytest.raises(ValueError):
            LinearRegressor.from_state_dict({k: v for k, v in sd.items() if k != drop})
    for name, wrong in (("coef", sd["coef"].float()), ("intercept", sd["intercept"].float()), ("meta", sd["meta"].int()),
                        ("intercept", sd["intercept"][:3]), ("meta", sd["meta"][:2]), ("coef", sd["coef"][:, :57]),
                        ("meta", torch.tensor([58, 59, 0])), ("coef", sd["coef"][0])):
        with pytest.raises(ValueError):
            LinearRegressor.from_state_dict({**sd, name: wrong})


def test_fixture_reproduces_the_printed_golden(fx, ideal):
    assert fx["coef"].dtype == np.float32 and fx["coef"].shape == (4, 58)
    assert fx["intercept"].dtype == np.float32 and fx["intercept"].shape == (4,)
    assert fx["X"].dtype == np.float32 and fx["X"].shape == (300, 58) and fx["pred_sklearn"].shape == (300, 4)
    assert int(fx["rank"]) == 14 and ideal.shape == (300, 4)
    l2_f32 = mean_l2(fx["pred_sklearn"], ideal)
    exact = predict_oracle(fx["X"], fx["coef"].astype(np.float64), fx["intercept"].astype(np.float64))
    l2_f64 = mean_l2(exact, ideal)
    print(f"G5: float32 path {l2_f32:.9f}, exact fp64 {l2_f64:.9f}, gap {l2_f64 - l2_f32:.3e}; max |float32 path - fp64| = "
          f"{float(np.abs(fx['pred_sklearn'] - exact).max()):.3e}")
    assert abs(l2_f32 - PRINTED_G5) <= 5e-7
    assert abs(l2_f64 - EXACT_G5) <= 1e-8


def test_ops_refuse_cpu_tensors(fx):
    from blackwater.native import _lib, ops

    for name in ("mlqem_linreg_moments_workspace_bytes", "mlqem_linreg_moments_f32", "mlqem_linreg_predict_f32"):
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 46 and _lib.load().mlqem_abi_version() == _lib.ABI_VERSION
    assert (ops.LINREG_MAX_FEATURES, ops.LINREG_MAX_OUTPUTS) == (512, 16)
    model = LinearRegressor.from_arrays(fx["coef"], fx["intercept"])
    x = torch.from_numpy(fx["X"])
    y = torch.zeros((300, 4))
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.linreg_predict(x, model.coef, model.intercept)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.linreg_moments(x, y)
    for call in (model.predict, model):
        with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
            call(x)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        LinearRegressor.fit(x, y)
    with pytest.raises(ValueError):
        model.predict(x[:, :57])


def test_entry_points_validate_before_any_launch():
    from blackwater.native import _lib

    lib = _lib.load()
    ws = lib.mlqem_linreg_moments_workspace_bytes
    mom, pred = lib.mlqem_linreg_moments_f32, lib.mlqem_linreg_predict_f32
    tile = 64 * 64 * 8
    # one 64 x 64 fp64 tile per (tile of the lower triangle, chunk of rows): 1, 6 and 45 tiles; chunks of >= 256 rows, <= 1024 groups
    assert ws(1, 1, 1) == tile and ws(300, 58, 4) == 2 * tile and ws(1000, 170, 1) == 6 * 4 * tile and ws(257, 512, 16) == 45 * 2 * tile
    assert ws(10 ** 6, 58, 4) == 1009 * tile                                   # chunks of 992 rows
    assert ws(-1, 58, 4) == 0 and ws(8, 513, 4) == 0 and ws(8, 58, 17) == 0
    buf = ctypes.create_string_buffer(64)      # stands for non-null pointers: validation fails before anything is touched
    p = ctypes.addressof(buf)
    # moments(x, ldx, y, ldy, n_rows, F, K, moments, accumulate, workspace, workspace_bytes, stream)
    assert mom(p, 58, p, 4, -1, 58, 4, p, 0, p, 1 << 30, None) == -1           # negative rows
    assert mom(p, 57, p, 4, 8, 58, 4, p, 0, p, 1 << 30, None) == -1            # ldx < F
    assert mom(p, 58, p, 3, 8, 58, 4, p, 0, p, 1 << 30, None) == -1            # ldy < K
    assert mom(p, 58, p, 4, 8, 0, 4, p, 0, p, 1 << 30, None) == -1             # no features
    assert mom(p, 58, p, 4, 8, 58, 0, p, 0, p, 1 << 30, None) == -1            # no outputs
    assert mom(p, 513, p, 4, 8, 513, 4, p, 0, p, 1 << 30, None) == _lib.ERR_UNSUPPORTED
    assert mom(p, 58, p, 17, 8, 58, 17, p, 0, p, 1 << 30, None) == _lib.ERR_UNSUPPORTED
    assert mom(p, 58, p, 4, 8, 58, 4, p, 0, p, tile - 1, None) == _lib.ERR_WORKSPACE
    assert mom(p, 58, p, 4, 8, 58, 4, p, 0, None, 0, None) == _lib.ERR_WORKSPACE
    assert mom(None, 58, None, 4, 8, 58, 4, None, 0, None, 1 << 30, None) == -1      # null pointers
    assert mom(None, 58, None, 4, 0, 58, 4, None, 1, None, 0, None) == 0       # no rows to add: nothing to do
    assert mom(None, 58, None, 4, 0, 58, 4, None, 0, None, 0, None) == -1      # no rows, overwrite: needs somewhere to write zeros
    # predict(x, ldx, n_rows, F, coef, intercept, K, out, stream)
    assert pred(None, 58, 0, 58, None, None, 4, None, None) == 0               # no rows: nothing to do
    assert pred(p, 58, -1, 58, p, p, 4, p, None) == -1
    assert pred(p, 57, 8, 58, p, p, 4, p, None) == -1
    assert pred(p, 58, 8, 58, p, p, 0, p, None) == -1
    assert pred(p, 513, 8, 513, p, p, 4, p, None) == _lib.ERR_UNSUPPORTED
    assert pred(p, 58, 8, 58, p, p, 17, p, None) == _lib.ERR_UNSUPPORTED
    assert pred(None, 58, 8, 58, None, None, 4, None, None) == -1
