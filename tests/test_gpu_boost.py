"""Gradient-boosted trees on the device (mlqem_boost_predict_f32, mlqem_boost_update_f64 through ops.boost_predict / ops.boost_fit
and blackwater.nn.BoostedRegressor).

Scoring is compared BIT FOR BIT: with scikit-learn's stored ``predict`` / ``staged_predict`` on the fixture rows, and with the numpy
restatement of ``predict_stages`` (tests/boost_cases.py: a multiply, then an add, per stage) on resampled rows.  A fit is not compared
with a refitted host ensemble (equal scores are the norm on ``encode_data``-like rows and the tie rule is the device's own): every
stage is walked by the fp64 checker on the residuals of the ensemble's own earlier stages (``boost_cases.check_stages``, which brings
``forest_fit_cases.check_forest``'s derived tolerances).  Stage-for-stage equality with scikit-learn is asserted on the tie-free fixture
cases only, and predictions there within ``boost_cases.prediction_bound`` (derived in that module's docstring).

``train_score_`` / ``oob_improvement_``: the reference sums the device ensemble's own squared residuals exactly (``math.fsum``) -- the
terms are the same bits on both sides, only the device's summation rounds: a shuffle tree over 256 rows and then block order, at most
n additions of partial sums no larger than the total S, so |device - exact| <= n 2^-53 S.  ``train_score_`` = S / rows is held to
n 2^-53 relative; ``oob_improvement_`` = (S_before - S_after) / rows is a difference of two such sums and is held to n 2^-53 relative
to (S_before + S_after) / rows, the quantities that were summed."""
import numpy as np
import pytest
import torch

import boost_cases as bc
import forest_fit_cases as fc
from blackwater.data.backends import PauliObservable
from blackwater.library.learning.estimator import BoostedLearningModelProcessor, ScikitLearningModelProcessor, learning
from blackwater.native import ops
from blackwater.nn import BoostedRegressor
from blackwater.nn.boost import subsample_masks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUFFERS = ("nodes", "tree_ptr", "value", "meta", "scale")
CASES, G1 = bc.load_fixture()
IDS = [c["name"] for c in CASES]
ROW_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1025)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def module_of(case):
    return BoostedRegressor.from_arrays(*(case["trees"][k] for k in bc.KEYS), n_features=case["X"].shape[1], init=case["init"],
                                        learning_rate=case["lr"]).to(DEV)


# ---- predict, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predict_equals_scikit_learn_to_the_last_bit(case):
    model, x = module_of(case), dev(case["X"])
    T = model.n_stages
    assert np.array_equal(host(model.predict(x)), case["pred"])
    staged = model.staged_predict(x)
    assert tuple(staged.shape) == (T, len(case["X"])) and staged.dtype == torch.float64
    assert np.array_equal(host(staged), case["staged"])
    for m in sorted({1, T - 1, T}):
        assert np.array_equal(host(model.predict(x, n_stages=m)), case["staged"][m - 1]), m
        assert np.array_equal(host(model.truncated(m).predict(x)), case["staged"][m - 1]), m
    out = model(x)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(case["X"]), 1)
    assert np.array_equal(host(out)[:, 0], case["pred"].astype(np.float32))
    leaf = host(model.apply(x))
    assert leaf.dtype == np.int32 and leaf.shape == (len(case["X"]), T)
    assert all(np.array_equal(leaf[:, t], fc.leaf_of_rows(case["trees"], t, case["X"])) for t in range(T))
    with pytest.raises(ValueError, match="n_stages"):
        model.predict(x, n_stages=T + 1)
    with pytest.raises(ValueError, match="n_stages"):
        model.predict(x, n_stages=0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_predict_is_the_same_at_every_row_count_and_row_stride(case):
    model, T = module_of(case), len(case["trees"]["tree_ptr"]) - 1
    rng = np.random.default_rng(7)
    pick = rng.integers(0, len(case["X"]), size=max(ROW_COUNTS))
    X = case["X"][pick]
    want = bc.staged_reference(case["trees"], X, case["init"], case["lr"])               # once, for the largest count
    assert np.array_equal(want, case["staged"][:, pick])                                 # a row's sum does not depend on its neighbours
    for n in ROW_COUNTS:
        x = dev(X[:n])
        out, staged = ops.boost_predict(x, model.nodes, model.tree_ptr, model.value, model.max_depth, model.init, model.learning_rate,
                                        staged=True)
        assert np.array_equal(host(out), want[-1, :n]) and np.array_equal(host(staged), want[:, :n]), n
        for m in sorted({1, T - 1, T}):
            assert np.array_equal(host(model.predict(x, n_stages=m)), want[m - 1, :n]), (n, m)
        wide = torch.full((n, X.shape[1] + 3), float("nan"), device=DEV)                 # a row-strided x: the columns beyond F are never read
        wide[:, :X.shape[1]] = x
        assert np.array_equal(host(model.predict(wide[:, :X.shape[1]])), want[-1, :n]), n
    # caller buffers: out, and a staged_out with a row stride above n
    n = 257
    out = torch.empty(n, dtype=torch.float64, device=DEV)
    slab = torch.full((T, n + 5), -7.0, dtype=torch.float64, device=DEV)
    got, staged = ops.boost_predict(dev(X[:n]), model.nodes, model.tree_ptr, model.value, model.max_depth, model.init,
                                    model.learning_rate, out=out, staged_out=slab[:, :n])
    assert got is out and np.array_equal(host(out), want[-1, :n]) and np.array_equal(host(slab[:, :n]), want[:, :n])
    assert bool((slab[:, n:] == -7.0).all())
    with pytest.raises(ValueError, match="staged_out"):
        ops.boost_predict(dev(X[:n]), model.nodes, model.tree_ptr, model.value, model.max_depth, model.init, model.learning_rate,
                          staged_out=slab[:, :n - 1].t())


def test_predict_is_the_same_for_every_tile_size():
    """The launcher tiles 4 rows a workgroup below 8192 rows, 16 from there and 64 from 32768: the same bits at and around both edges."""
    case = CASES[IDS.index("d3")]
    model = module_of(case)
    pick = np.random.default_rng(11).integers(0, len(case["X"]), size=32768 + 65)
    X = case["X"][pick]
    want = case["staged"][:, pick]
    for n in (8191, 8192, 8193, 32767, 32768, 32768 + 65):
        out, staged = ops.boost_predict(dev(X[:n]), model.nodes, model.tree_ptr, model.value, model.max_depth, model.init,
                                        model.learning_rate, staged=True)
        assert np.array_equal(host(out), want[-1, :n]) and np.array_equal(host(staged), want[:, :n]), n


def test_predict_in_a_captured_graph():
    case = CASES[IDS.index("leaf4")]
    model, x = module_of(case), dev(case["X"])
    n, T = len(case["X"]), model.n_stages
    out = torch.zeros(n, dtype=torch.float64, device=DEV)
    staged = torch.zeros((T, n), dtype=torch.float64, device=DEV)
    args = (x, model.nodes, model.tree_ptr, model.value, model.max_depth, model.init, model.learning_rate)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.boost_predict(*args, out=out, staged_out=staged)                           # loads the code object before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = ops.boost_predict(*args, out=out, staged_out=staged)
    assert got[0] is out and got[1] is staged
    pick = np.random.default_rng(3).permutation(n)                                     # replayed on new rows in the same buffers
    x.copy_(dev(case["X"][pick]))
    out.zero_(), staged.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(host(out), case["pred"][pick]) and np.array_equal(host(staged), case["staged"][:, pick])


# ---- fit invariants ------------------------------------------------------------------------------------------------------------------
def problem(n, F, seed=0):
    return fc.make_pool_rows(seed + 13 * n + F, n, F), fc.make_targets(seed + n, n, 1)[:, 0]


def fit_and_check(X, y, T, depth, lr=0.1, subsample=1.0, seed=0, **params):
    """The kernels' own stages (host arrays in the fitter's numbering), walked by the checker; train_score / oob_improvement against
    the ensemble's own residuals (the module docstring derives the bounds)."""
    n, F = X.shape
    masks = subsample_masks(n, T, subsample, seed)
    grown = ops.boost_fit(dev(X), dev(y), masks.to(DEV), learning_rate=lr, max_depth=depth, seed=seed, **params)
    m = params.get("max_features")
    full = {"min_samples_split": 2, "min_samples_leaf": 1, **{k: v for k, v in params.items() if k != "max_features"}, "max_depth": depth}
    gap = bc.check_stages(X, y, masks.numpy(), full, lr, grown["init"], grown, subset=None if m is None else (m, seed))
    train, oob, oob_scale = bc.stage_losses(X, y, masks.numpy(), lr, grown["init"], grown)
    assert grown["train_score"].shape == (T,) and len(grown["tree_ptr"]) == T + 1 and grown["value"].shape[1] == 1
    err = np.abs(grown["train_score"] - train)
    print(f"rows {n} F {F} T {T} depth {depth} subsample {subsample} {params}: levels {grown['levels']}, nodes {int(grown['tree_ptr'][-1])}, "
          f"smallest gap {gap:.3e}, train_score off by {(err / np.maximum(train, 1e-300)).max():.3e} relative")
    assert (err <= n * bc.U * train).all()
    if (masks.numpy() == 0).any():
        oob_err = np.abs(grown["oob_improvement"] - oob)
        print(f"    oob_improvement off by {(oob_err / np.maximum(oob_scale, 1e-300)).max():.3e} of (before + after) / rows")
        assert (oob_err <= n * bc.U * oob_scale).all()
    else:
        assert grown["oob_improvement"] is None
    assert grown["levels"] <= depth + 1
    return grown


# n: one row, two, the wave and tile edges; F: 1, 58, 170; T: 1, 3, 33; depth 9 sizes a 1023-node store -- a sparse cross
GRID = [(1, 1, 1, 1), (2, 58, 3, 3), (63, 1, 3, 1), (64, 58, 33, 3), (65, 170, 1, 4), (257, 58, 33, 3), (1025, 1, 3, 9)]
VARIANTS = {"subsample": lambda F: dict(subsample=0.5), "min_samples_leaf": lambda F: dict(min_samples_leaf=3),
            "max_features": lambda F: dict(max_features=max(1, F // 3))}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("n,F,T,depth", GRID)
def test_fit_invariants_on_the_grid(n, F, T, depth, variant):
    X, y = problem(n, F)
    grown = fit_and_check(X, y, T, depth, **VARIANTS[variant](F))
    if F > 1:
        assert not (grown["feature"] == F - 1).any()          # the constant column never splits
    if variant == "min_samples_leaf":
        assert grown["n_node_samples"].min() >= min(3, n)


def test_fit_with_a_tree_too_large_for_lds():
    """Continuous rows, depth 9: a stage of more than 511 nodes is read from global memory by the update kernel (the pool rows of
    the grid's depth-9 case have 24 distinct values, so its trees stay small however large the store)."""
    rng = np.random.default_rng(5)
    X = rng.normal(size=(1025, 3)).astype(np.float32)
    y = X[:, 0].astype(np.float64) + 0.05 * rng.normal(size=1025)      # a smooth target splits evenly: about 700 nodes a stage
    grown = fit_and_check(X, y, 2, 9, lr=0.5)
    assert np.diff(grown["tree_ptr"]).min() > 511


def test_fit_and_predict_with_rows_too_wide_for_lds():
    """F = 3100: four rows of x no longer fit the predict kernel's LDS budget, it reads x from global memory."""
    rng = np.random.default_rng(6)
    X = rng.normal(size=(40, 3100)).astype(np.float32)
    y = X[:, 3000].astype(np.float64) + 0.1 * rng.normal(size=40)
    model = BoostedRegressor.fit(dev(X), dev(y), n_estimators=2, max_depth=2, learning_rate=0.5)
    trees = {k: host(v) for k, v in (("tree_ptr", model.tree_ptr), ("value", model.value))}
    want = host(model.staged_predict(dev(X)))
    # the same ensemble scored by the forest kernel's leaves: raw = init, then one multiply and one add per stage
    leaf = host(model.apply(dev(X))).astype(np.int64)
    raw = np.full(40, model.init)
    for t in range(2):
        step = np.float64(model.learning_rate) * trees["value"][trees["tree_ptr"][t] + leaf[:, t], 0]
        raw = raw + step
        assert np.array_equal(want[t], raw)
    assert model.train_score_[1] < model.train_score_[0] < float(np.var(y))


# ---- equality with scikit-learn where nothing ties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fit_equals_scikit_learn_where_nothing_ties(case):
    X, y, T = case["X"], case["y"], len(case["trees"]["tree_ptr"]) - 1
    grown = fit_and_check(X, y, T, case["params"]["max_depth"], lr=case["lr"], min_samples_split=case["params"]["min_samples_split"],
                          min_samples_leaf=case["params"]["min_samples_leaf"])
    fc.same_trees(grown, case["trees"], X)                                              # per stage: features and float64 thresholds exact
    model = BoostedRegressor.fit(dev(X), dev(y), n_estimators=T, learning_rate=case["lr"], **case["params"])
    limit = bc.prediction_bound(X, y, case["init"], case["lr"], case["trees"])
    err = float(np.abs(host(model.predict(dev(X))) - case["pred"]).max())
    staged_err = float(np.abs(host(model.staged_predict(dev(X))) - case["staged"]).max())
    print(f"{case['name']}: max |predict - scikit-learn| = {err:.3e}, staged {staged_err:.3e}, bound {limit:.3e}")
    assert err <= limit and staged_err <= limit
    assert abs(model.init - case["init"]) <= len(X) * bc.U * np.abs(y).max()
    # train_score_: residuals within `limit` of scikit-learn's, so their squares within (2 R + limit) limit, R its largest |residual|
    R = max(np.abs(y[None, :] - case["staged"]).max(), np.abs(y - case["init"]).max())
    assert np.abs(model.train_score_ - case["train_score"]).max() <= (2 * R + limit) * limit + 2 * len(X) * bc.U * case["train_score"].max()


# ---- determinism and the module ------------------------------------------------------------------------------------------------------
def test_two_fits_give_the_same_bits_and_full_masks_equal_no_subsampling():
    n, F, T = 257, 58, 7
    X, y = problem(n, F, seed=3)
    x_d, y_d = dev(X), dev(y)
    a = BoostedRegressor.fit(x_d, y_d, n_estimators=T, subsample=0.5, seed=1)
    b = BoostedRegressor.fit(x_d, y_d, n_estimators=T, subsample=0.5, seed=1)
    other = BoostedRegressor.fit(x_d, y_d, n_estimators=T, subsample=0.5, seed=2)
    for name in BUFFERS:
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.train_score_, b.train_score_) and np.array_equal(a.oob_improvement_, b.oob_improvement_)
    assert a.nodes.shape != other.nodes.shape or not torch.equal(a.nodes, other.nodes)
    assert torch.equal(a.fit_info["sample_masks"].cpu(), subsample_masks(n, T, 0.5, 1))
    full = BoostedRegressor.fit(x_d, y_d, n_estimators=T)
    ones = BoostedRegressor.fit(x_d, y_d, n_estimators=3, sample_masks=torch.ones((T, n), dtype=torch.int32))   # overrides n_estimators
    for name in BUFFERS:
        assert torch.equal(getattr(full, name), getattr(ones, name)), name
    assert np.array_equal(full.train_score_, ones.train_score_) and not hasattr(full, "oob_improvement_") and full.n_stages == T
    # the forest fit still chunks as before with the shared workspace allocation
    sub = BoostedRegressor.fit(x_d, y_d, n_estimators=3, max_features=19, seed=4)
    sub_again = BoostedRegressor.fit(x_d, y_d, n_estimators=3, max_features=19, seed=4)
    assert all(torch.equal(getattr(sub, k), getattr(sub_again, k)) for k in BUFFERS) and sub.fit_info["max_features"] == 19


def test_module_round_trip_eval_set_score_and_importances():
    n, F, T = 257, 58, 9
    X, y = problem(n, F, seed=4)
    x_d, y_d = dev(X), dev(y)
    xv, yv = dev(X[:65]), dev(y[:65].astype(np.float32))
    model = BoostedRegressor.fit(x_d, y_d.reshape(n, 1), n_estimators=T, learning_rate=0.3, eval_set=(xv, yv))
    assert model.nodes.device.type == "cuda" and (model.n_stages, model.n_features, model.n_outputs) == (T, F, 1)
    assert 1 <= model.fit_info["levels"] <= 4 and len(model.fit_info["n_node_samples"]) == model.nodes.shape[0]
    staged = host(model.staged_predict(xv))
    want = ((staged - host(yv).astype(np.float64)[None, :]) ** 2).mean(axis=1)
    assert model.validation_score_.shape == (T,) and np.abs(model.validation_score_ - want).max() <= 65 * bc.U * want.max()
    assert model.best_n_estimators_ == int(np.argmin(model.validation_score_)) + 1
    again = BoostedRegressor.from_state_dict(model.state_dict()).to(DEV)
    assert all(torch.equal(getattr(again, name), getattr(model, name)) for name in BUFFERS)
    assert torch.equal(again.predict(x_d), model.predict(x_d)) and (again.init, again.learning_rate) == (model.init, 0.3)
    pred = host(model.predict(x_d))
    r2 = 1.0 - ((y - pred) ** 2).sum() / ((y - y.mean()) ** 2).sum()
    assert abs(model.score(x_d, y_d) - r2) <= 1e-12 and model.score(x_d, y_d) > 0.0
    imp = model.feature_importances(x_d, model.fit_info["sample_masks"])
    assert imp.shape == (F,) and imp.dtype == np.float64 and abs(imp.sum() - 1.0) <= 1e-12 and (imp >= 0).all() and imp[F - 1] == 0.0
    used = np.unique(host(model.nodes)[:, 1])
    assert set(np.flatnonzero(imp > 0)) <= set(used[used >= 0].tolist())
    f32 = BoostedRegressor.fit(x_d, dev(y.astype(np.float32)), n_estimators=2)          # float32 targets are widened first
    f64 = BoostedRegressor.fit(x_d, dev(y.astype(np.float32)).double(), n_estimators=2)
    assert all(torch.equal(getattr(f32, name), getattr(f64, name)) for name in BUFFERS)


def test_non_finite_inputs_are_refused_before_any_launch():
    X, y = problem(65, 3)
    bad_x, bad_y = X.copy(), y.copy()
    bad_x[7, 1], bad_y[3] = np.nan, np.inf
    for xs, ys in ((bad_x, y), (X, bad_y)):
        with pytest.raises(ValueError, match="NaN or an infinity"):
            BoostedRegressor.fit(dev(xs), dev(ys), n_estimators=2)


# ---- quality ---------------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_g1_rows():
    """Held-out mean L2 on the G1 rows, one 100-stage depth-3 model per output column at subsample=0.5, seeds 0, 1, 2 of the
    documented bag generator, against scikit-learn's own 20-seed spread at subsample=0.5 (fixture): at most its mean plus 5
    standard deviations (0.020997; the bags and the tie rule are not scikit-learn's) and below the unmitigated L2 (0.025461).  The
    subsample=1.0 figure is printed for the record and not asserted against scikit-learn's (whose spread there, 3e-5, comes from
    its random tie-breaking alone)."""
    X, ideal, noisy, train = fc.g1_problem()
    sk = G1["sklearn_g1_l2_sub05"]
    limit = float(sk.mean() + 5.0 * sk.std())
    raw = fc.mean_l2(noisy[~train], ideal[~train])
    x_d, held = dev(X[train]), dev(X[~train])

    def l2_of(seed, subsample):
        cols = [host(BoostedRegressor.fit(x_d, dev(ideal[train, k]), subsample=subsample, seed=seed).predict(held)) for k in range(ideal.shape[1])]
        return fc.mean_l2(np.stack(cols, axis=1), ideal[~train])

    for seed in range(3):
        l2 = l2_of(seed, 0.5)
        print(f"G1 held-out mean L2, subsample 0.5, seed {seed}: {l2:.6f} (scikit-learn mean {sk.mean():.6f}, bound {limit:.6f}, unmitigated {raw:.6f})")
        assert l2 <= limit and l2 < raw
    print(f"G1 held-out mean L2, subsample 1.0: {l2_of(0, 1.0):.6f} (scikit-learn mean {G1['sklearn_g1_l2_sub10'].mean():.6f}, for the record)")


# ---- processor -------------------------------------------------------------------------------------------------------------------------
class _Result:
    def __init__(self, values):
        self.values, self.metadata = np.asarray(values, dtype=float), [{"shots": 7} for _ in values]


class _Job:
    def __init__(self, values):
        self._values = values

    def result(self):
        return _Result(self._values)

    def job_id(self):
        return "job-42"

    def status(self):
        return "DONE"


class FakeEstimator:
    def run(self, circuits, observables, parameter_values=None, **opts):
        return self._run(circuits, observables, parameter_values or [()] * len(circuits), **opts)

    def _run(self, circuits, observables, parameter_values, **opts):
        return _Job([0.5 + 0.01 * k for k in range(len(circuits))])


def _term_rows(lima_backend, jobs):
    from blackwater.data.utils import encode_pauli_sum_op, get_backend_properties_v1
    from blackwater.library.learning.features import encode_data

    props = get_backend_properties_v1(lima_backend)
    return torch.cat([encode_data(circuits=[text], properties=props, ideal_exp_vals=[[0.0]], noisy_exp_vals=[[value]], num_qubits=1,
                                  meas_bases=encode_pauli_sum_op([(label, 1.0)]))[0] for value, text, label in jobs]).to(torch.float32)


def _training_rows(lima_backend, g1):
    labels = ("IIIIZ", "IIIZI")
    train = [(float(g1["noisy"][i, q]), g1["qasm"][i], labels[q], float(g1["ideal"][i, q])) for i in range(24) for q in range(2)]
    return _term_rows(lima_backend, [t[:3] for t in train]), np.asarray([t[3] for t in train], np.float64)


def test_processor_end_to_end_with_a_device_fitted_model(lima_backend, g1):
    rows, targets = _training_rows(lima_backend, g1)
    assert tuple(rows.shape) == (48, 76)
    model = BoostedRegressor.fit(rows.to(DEV), dev(targets), n_estimators=20, seed=0)
    proc = BoostedLearningModelProcessor(model, lima_backend, device=DEV)
    assert proc.accepts_qasm_text
    circuits = [g1["qasm"][30], g1["qasm"][31]]
    obs = [PauliObservable([("IIIIZ", 0.5), ("IIIZI", -2.0)]), PauliObservable("IIIIZ")]
    got = learning(FakeEstimator, proc, skip_transpile=True)().run(circuits, obs).result()
    serial = [proc.process(0.5, circuits[0], obs[0], ()), proc.process(0.51, circuits[1], obs[1], ())]
    assert got.values.tolist() == serial and np.isfinite(got.values).all()
    pred = host(model.predict(_term_rows(lima_backend, [(0.5, circuits[0], "IIIIZ"), (0.5, circuits[0], "IIIZI"),
                                                        (0.51, circuits[1], "IIIIZ")]).to(DEV)))
    want = np.asarray([0.0 + pred[0] * 0.5 + pred[1] * -2.0, 0.0 + pred[2] * 1.0])
    print("processor with a device-fitted ensemble:", got.values, "from predict:", want)
    assert np.array_equal(got.values, want)
    assert got.metadata[0] == {"shots": 7, "original_value": 0.5}
    from blackwater.exception import BlackwaterException

    with pytest.raises(BlackwaterException):
        BoostedLearningModelProcessor(object(), lima_backend, device=DEV)


def test_processor_equals_the_scikit_processor_to_the_last_bit(lima_backend, g1):
    pytest.importorskip("sklearn")
    from sklearn.ensemble import GradientBoostingRegressor

    rows, targets = _training_rows(lima_backend, g1)
    gb = GradientBoostingRegressor(n_estimators=30, random_state=0).fit(rows.numpy(), targets)
    circuits = [g1["qasm"][30], g1["qasm"][31]]
    obs = [PauliObservable([("IIIIZ", 0.5), ("IIIZI", -2.0)]), PauliObservable("IIIIZ")]
    sk = learning(FakeEstimator, ScikitLearningModelProcessor(gb, lima_backend), skip_transpile=True)
    dv = learning(FakeEstimator, BoostedLearningModelProcessor(gb, lima_backend, device=DEV), skip_transpile=True)
    a = sk().run(circuits, obs).result().values
    b = dv().run(circuits, obs).result().values
    print("processor vs scikit-learn:", a, b)
    assert np.array_equal(a, b)
