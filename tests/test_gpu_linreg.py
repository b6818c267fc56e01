"""The least-squares kernels (mlqem_linreg_moments_f32, mlqem_linreg_predict_f32) through ops, nn.LinearRegressor and
LinearLearningModelProcessor, on the device.  The oracle everywhere is numpy fp64 (tests/linreg_cases.py).

Bounds, all derived from the arithmetic and computed from the inputs:
  moments   the products of widened float32 inputs are exact in fp64, only the n additions round: n 2^-53 sum|a_i b_i| per entry;
  predict   F fused multiply-adds from the intercept against numpy's dot product: (F + 2) 2^-53 (|b| + sum|c_j x_j|) per output;
  fit       the device differs from a numpy-fp64 restatement of the same solve rule only by the summation order inside M, so its
            gap to the lstsq oracle may be 100 x the restatement's own gap on that input (floor 1e-12).
Measured on an MI355X (max over entries / outputs):
  moments   error / bound <= 0.0084 in one call on every shape of the grid (4099 x 58 x 4: 0.0012; exact up to 65 rows) and
            <= 0.075 over three chunks;
  predict   error / bound <= 0.40 (three columns) and <= 0.093 from 58 columns on; fixture 0.024;
  G5        device mean L2 0.142318618, |device - exact fp64| = 6.9e-15, |device - printed| = 1.162e-05, max |device - scikit-learn's
            float32 path| = 8.635e-05;
  fit       gap to lstsq (in brackets the restatement's): g1 3.3e-13 (1.4e-11), three shards 4.2e-12; 4099x58x4 5.4e-13 (6.5e-13);
            1000x170x1 2.6e-12 (3.7e-12); 65x3x1 3.3e-16 (3.3e-16);
  processor max |device - host oracle| = 5.7e-14."""
import os

import numpy as np
import pytest
import torch

from blackwater.data.backends import PauliObservable
from blackwater.library.learning.estimator import LinearLearningModelProcessor, ScikitLearningModelProcessor, learning
from blackwater.native import _lib, ops
from blackwater.nn import LinearRegressor
from linreg_cases import (EXACT_G5, GOLDEN, PRINTED_G5, fit_problems, lstsq_predictions, mean_l2, moments_bound, moments_oracle,
                          predict_bound, predict_oracle)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (n, F, K): one row; around the 64-lane and 32-row-slab edges; more than one chunk of rows (4099 = 16 chunks of 256 + 3); several
# tiles (172 columns = 3 x 3 tiles); the largest the kernels serve (529 columns = 9 x 9 tiles, the last one column wide)
SHAPES = [(1, 1, 1), (63, 3, 1), (64, 3, 1), (65, 3, 1), (4099, 58, 4), (1000, 170, 1), (257, 512, 16)]


def rows(n, F, K, seed=0):
    rng = np.random.default_rng(1000 * seed + 7 * n + 3 * F + K)
    X = rng.standard_normal((n, F)).astype(np.float32)
    Y = rng.standard_normal((n, K)).astype(np.float32)
    if F > 1:
        X[:, 1] += np.float32(100.0)         # a badly centred column: large sums that cancel in the covariance
    return X, Y


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check_moments(got, X, Y, what):
    want, limit = moments_oracle(X, Y), moments_bound(X, Y)
    got = got.cpu().numpy()
    err = np.abs(got - want)
    ratio = float((err / np.maximum(limit, 1e-300)).max()) if X.shape[0] else 0.0
    print(f"moments {what} {X.shape[0]}x{X.shape[1]}+{Y.shape[1]}: max |M - oracle| = {float(err.max()):.3e}, max error / bound = {ratio:.3e}")
    assert (err <= limit).all()
    assert np.array_equal(got, got.T)
    assert got[0, 0] == X.shape[0]


@pytest.mark.parametrize("n,F,K", SHAPES)
def test_moments(n, F, K):
    X, Y = rows(n, F, K)
    x, y = dev(X), dev(Y)
    m = ops.linreg_moments(x, y)
    D = 1 + F + K
    assert m.dtype == torch.float64 and tuple(m.shape) == (D, D)
    check_moments(m, X, Y, "one shot")
    assert torch.equal(m, ops.linreg_moments(x, y))                           # bit-equal from call to call
    # wider rows whose pad columns hold NaN: never read
    wx = torch.full((n, F + 5), float("nan"), device=DEV)
    wy = torch.full((n, K + 3), float("nan"), device=DEV)
    wx[:, :F], wy[:, :K] = x, y
    if n > 1:
        assert wx[:, :F].stride(0) == F + 5 and wy[:, :K].stride(0) == K + 3
    assert torch.equal(m, ops.linreg_moments(wx[:, :F], wy[:, :K]))
    # three unequal chunks added up on the device: the same bound against the one-shot oracle
    cuts = [0, n // 5, n // 5 + n // 3, n]
    acc = torch.zeros((D, D), dtype=torch.float64, device=DEV)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert ops.linreg_moments(x[a:b], y[a:b], out=acc, accumulate=True) is acc
    check_moments(acc, X, Y, "three chunks")
    # out= overwrites whatever the buffer held
    again = torch.full((D, D), float("nan"), dtype=torch.float64, device=DEV)
    ops.linreg_moments(x, y, out=again)
    assert torch.equal(again, m)


def test_moments_of_no_rows_and_unsupported_widths():
    x, y = torch.zeros((0, 58), device=DEV), torch.zeros((0, 4), device=DEV)
    out = torch.full((63, 63), float("nan"), dtype=torch.float64, device=DEV)
    assert ops.linreg_moments(x, y, out=out) is out and not out.any()        # overwrite with no rows: all zeros
    out.fill_(2.0)
    ops.linreg_moments(x, y, out=out, accumulate=True)                          # add no rows: unchanged
    assert bool((out == 2.0).all())
    with pytest.raises(ValueError):
        ops.linreg_moments(x, y, accumulate=True)                               # nothing to add to
    with pytest.raises(ValueError):
        ops.linreg_moments(torch.zeros((8, 58), device=DEV), torch.zeros((7, 4), device=DEV))
    for F, K in ((513, 1), (3, 17)):
        with pytest.raises(_lib.NativeLibraryError, match="unsupported"):
            ops.linreg_moments(torch.zeros((8, F), device=DEV), torch.zeros((8, K), device=DEV))
        with pytest.raises(_lib.NativeLibraryError, match="unsupported"):
            ops.linreg_predict(torch.zeros((8, F), device=DEV), torch.zeros((K, F), dtype=torch.float64, device=DEV),
                               torch.zeros(K, dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()


def check_predict(X, coef, intercept, what):
    x, c, b = dev(X), dev(coef), dev(intercept)
    got = ops.linreg_predict(x, c, b)
    n, K = X.shape[0], coef.shape[0]
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, K)
    err = np.abs(got.cpu().numpy() - predict_oracle(X, coef, intercept))
    limit = predict_bound(X, coef, intercept)
    print(f"predict {what} {n}x{X.shape[1]}->{K}: max |out - oracle| = {float(err.max()):.3e}, max error / bound = "
          f"{float((err / np.maximum(limit, 1e-300)).max()):.3e}")
    assert (err <= limit).all()
    assert torch.equal(got, ops.linreg_predict(x, c, b))                        # bit-equal from call to call
    h = n // 2 + 1                                                              # ... and between the batch and its two halves
    halves = torch.cat([ops.linreg_predict(x[:h], c, b), ops.linreg_predict(x[h:], c, b)])
    assert torch.equal(got, halves)
    wide = torch.full((n, X.shape[1] + 6), float("nan"), device=DEV)
    wide[:, :X.shape[1]] = x
    assert torch.equal(got, ops.linreg_predict(wide[:, :X.shape[1]], c, b))
    return got


@pytest.mark.parametrize("n,F,K", SHAPES)
def test_predict(n, F, K):
    X, _ = rows(n, F, K, seed=1)
    rng = np.random.default_rng(n + F + K)
    coef = rng.standard_normal((K, F)) * 10.0 ** rng.integers(-3, 4, size=(K, F))     # magnitudes 1e-3 .. 1e3: sums that cancel
    intercept = rng.standard_normal(K)
    check_predict(X, coef, intercept, "grid")


def test_predict_fixture_and_g5():
    fx = dict(np.load(os.path.join(GOLDEN, "ols_g1.npz")))
    ideal = np.load(os.path.join(GOLDEN, "g1_dataset.npz"))["ideal"].astype(np.float64)
    coef, intercept = fx["coef"].astype(np.float64), fx["intercept"].astype(np.float64)
    assert np.abs(coef).max() > 5e3
    check_predict(fx["X"], coef, intercept, "fixture")
    model = LinearRegressor.from_arrays(fx["coef"], fx["intercept"]).to(DEV)
    x = dev(fx["X"])
    pred = model.predict(x)
    assert pred.dtype == torch.float64 and tuple(pred.shape) == (300, 4)
    got = pred.cpu().numpy()
    l2 = mean_l2(got, ideal)
    l2_exact = mean_l2(predict_oracle(fx["X"], coef, intercept), ideal)
    gap32 = float(np.abs(got - fx["pred_sklearn"]).max())
    print(f"G5: device mean L2 {l2:.9f}, exact fp64 {l2_exact:.9f} (|device - exact| = {abs(l2 - l2_exact):.3e}), printed {PRINTED_G5} "
          f"(|device - printed| = {abs(l2 - PRINTED_G5):.3e}); max |device - scikit-learn's float32 path| = {gap32:.3e}")
    assert abs(l2 - EXACT_G5) <= 1e-9
    assert abs(l2 - PRINTED_G5) <= 2e-5
    assert gap32 <= 2e-4
    fwd = model(x)
    assert fwd.dtype == torch.float32 and torch.equal(fwd, pred.to(torch.float32))
    one = LinearRegressor.from_arrays(fx["coef"][2], fx["intercept"][2]).to(DEV)       # a 1-D coef: predict returns [n]
    assert tuple(one.predict(x).shape) == (300,) and torch.equal(one.predict(x), pred[:, 2])
    assert tuple(model.predict(x[:0]).shape) == (0, 4)


def test_predict_captured_in_a_graph_and_replayed_on_new_rows():
    n, F, K = 4099, 58, 4
    X, _ = rows(n, F, K, seed=2)
    rng = np.random.default_rng(5)
    model = LinearRegressor.from_arrays(rng.standard_normal((K, F)), rng.standard_normal(K)).to(DEV)
    x = dev(X)
    out = torch.empty((n, K), dtype=torch.float64, device=DEV)

    def run():
        return ops.linreg_predict(x, model.coef, model.intercept, out=out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = run()
    assert got is out
    for k in range(3):
        fresh = dev(rows(n, F, K, seed=10 + k)[0])
        x.copy_(fresh)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, model.predict(fresh))


def restated_fit(X, Y, rcond=1e-10):
    """The solve rule restated in numpy fp64, independently of blackwater.nn.linear_model: fp64 moments, the centred covariance,
    an eigen-decomposition with the eigenvalues up to rcond * largest dropped.  What the device fit computes, up to the summation
    order inside M.  Returns (coef [K, F], intercept [K])."""
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    n = Xd.shape[0]
    sx, sy = Xd.sum(axis=0), Yd.sum(axis=0)
    cxx = Xd.T @ Xd - np.outer(sx, sx) / n
    cxy = Xd.T @ Yd - np.outer(sx, sy) / n
    lam, vec = np.linalg.eigh(cxx)
    keep = lam > rcond * lam[-1]
    B = vec[:, keep] @ ((vec[:, keep].T @ cxy) / lam[keep][:, None])
    return B.T, sy / n - (sx / n) @ B


@pytest.mark.parametrize("name,X,Y,rank", fit_problems(), ids=[p[0] for p in fit_problems()])
def test_fit_end_to_end(name, X, Y, rank):
    want = lstsq_predictions(X, Y)
    coef, intercept = restated_fit(X, Y)
    own = float(np.abs(predict_oracle(X, coef, intercept) - want).max())
    limit = max(100.0 * own, 1e-12)
    x, y = dev(X), dev(Y)
    model = LinearRegressor.fit(x, y)
    assert model.coef.is_cuda and model.rank_ == rank and model.n_rows_seen == X.shape[0]
    assert (model.n_features, model.n_outputs) == (X.shape[1], Y.shape[1])
    pred = model.predict(x).cpu().numpy().reshape(want.shape)
    gap = float(np.abs(pred - want).max())
    print(f"fit {name}: rank {model.rank_}, max |device fit - lstsq| = {gap:.3e} (numpy restatement of the rule: {own:.3e}, bound {limit:.3e})")
    assert gap <= limit
    # the same rows in three unequal shards
    n = X.shape[0]
    acc = LinearRegressor.Accumulator(X.shape[1], Y.shape[1], DEV)
    for a, b in ((0, n // 5), (n // 5, n // 5 + n // 3), (n // 5 + n // 3, n)):
        acc.update(x[a:b], y[a:b])
    streamed = acc.solve()
    assert streamed.rank_ == rank and streamed.n_rows_seen == n
    gap_s = float(np.abs(streamed.predict(x).cpu().numpy().reshape(want.shape) - want).max())
    print(f"fit {name}: three shards, max |device fit - lstsq| = {gap_s:.3e}")
    assert gap_s <= limit


def test_fit_takes_a_vector_of_targets_and_ridge():
    X, Y = rows(500, 12, 1, seed=3)
    x, y = dev(X), dev(Y)
    a, b = LinearRegressor.fit(x, y[:, 0]), LinearRegressor.fit(x, y)
    assert torch.equal(a.coef, b.coef) and tuple(a.predict(x).shape) == (500,)
    ridge = LinearRegressor.fit(x, y, alpha=2.0)
    Xd, Yd = X.astype(np.float64), Y.astype(np.float64)
    xc, yc = Xd - Xd.mean(0), Yd - Yd.mean(0)
    B = np.linalg.solve(xc.T @ xc + 2.0 * np.eye(12), xc.T @ yc)
    assert ridge.rank_ == 12 and np.abs(ridge.coef.cpu().numpy() - B.T).max() <= 1e-12


# ---- the decorator, end to end (FakeEstimator as in tests/test_estimators.py) -------------------------------------------------
QASM = ('OPENQASM 2.0;\ninclude "qelib1.inc";\nqreg q[5];\ncreg meas[2];\nrz(0.3) q[0];\nsx q[0];\ncx q[0],q[1];\n'
        'barrier q[0],q[1];\nmeasure q[0] -> meas[0];\nmeasure q[1] -> meas[1];\n')
QASM2 = QASM.replace("rz(0.3) q[0];", "rz(0.3) q[0];\nx q[1];\nsx q[1];")


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
    """Stand-in for a qiskit BaseEstimator: ``run`` forwards to ``_run`` with keyword arguments."""

    def run(self, circuits, observables, parameter_values=None, **opts):
        parameter_values = parameter_values or [()] * len(circuits)
        return self._run(circuits, observables, parameter_values, **opts)

    def _run(self, circuits, observables, parameter_values, **opts):
        return _Job([0.5 + 0.1 * k for k in range(len(circuits))])


class HostLinear:
    """A host object with scikit-learn's ``predict``: the fp64 oracle, for ScikitLearningModelProcessor."""

    def __init__(self, coef, intercept):
        self.coef, self.intercept = coef, intercept

    def predict(self, X):
        return predict_oracle(np.asarray(X, np.float32), self.coef, self.intercept)


def _term_rows(lima_backend, jobs):
    """The 76-wide encode_data rows of (noisy value, circuit, Pauli label) triples, as the processors build them."""
    from blackwater.data.utils import encode_pauli_sum_op, get_backend_properties_v1
    from blackwater.library.learning.features import encode_data

    props = get_backend_properties_v1(lima_backend)
    made = [encode_data(circuits=[text], properties=props, ideal_exp_vals=[[0.0]], noisy_exp_vals=[[value]], num_qubits=1,
                        meas_bases=encode_pauli_sum_op([(label, 1.0)]))[0] for value, text, label in jobs]
    return torch.cat(made).numpy().astype(np.float32)


def test_processor_equals_the_host_processor(lima_backend):
    from blackwater.exception import BlackwaterException

    two_terms = PauliObservable([("ZIIII", 0.5), ("IXIII", -2.0)])
    one_term = PauliObservable("IIIIZ")
    jobs = [(0.5, QASM, "ZIIII"), (0.5, QASM, "IXIII"), (0.6, QASM2, "IIIIZ")]
    X = _term_rows(lima_backend, jobs)
    assert X.shape == (3, 76)
    rng = np.random.default_rng(0)
    coef, intercept = rng.standard_normal((1, 76)) * 30.0, rng.standard_normal(1)
    limit = predict_bound(X, coef, intercept)[:, 0]
    limit = np.asarray([0.5 * limit[0] + 2.0 * limit[1], limit[2]]) + 2.0 ** -52 * 3.0 * np.abs(predict_oracle(X, coef, intercept)).max()
    proc = LinearLearningModelProcessor(LinearRegressor.from_arrays(coef, intercept), lima_backend, device=DEV)
    assert proc.accepts_qasm_text
    host = learning(FakeEstimator, ScikitLearningModelProcessor(HostLinear(coef, intercept), lima_backend), skip_transpile=True)
    device = learning(FakeEstimator, proc, skip_transpile=True)
    obs = [two_terms, one_term]
    want = host().run([QASM, QASM2], obs).result().values
    got = device().run([QASM, QASM2], obs).result()                            # OpenQASM text: process_batch, the native op scan
    serial = [proc.process(0.5, QASM, two_terms, ()), proc.process(0.6, QASM2, one_term, ())]
    assert got.values.tolist() == serial                                       # process and process_batch agree exactly
    print("processor: device", got.values, "host", want, "max |device - host| =", float(np.abs(got.values - want).max()), "bound", limit)
    assert (np.abs(got.values - want) <= limit).all()
    assert got.metadata[0] == {"shots": 7, "original_value": 0.5}
    # parsed circuits instead of text
    from blackwater.data.circuit import Circuit

    parsed = [Circuit.from_qasm_str(QASM), Circuit.from_qasm_str(QASM2)]
    got_parsed = device().run(parsed, obs).result().values
    serial_parsed = [proc.process(0.5, parsed[0], two_terms, ()), proc.process(0.6, parsed[1], one_term, ())]
    assert got_parsed.tolist() == serial_parsed
    assert (np.abs(got_parsed - want) <= limit).all()
    with pytest.raises(BlackwaterException):
        LinearLearningModelProcessor(object(), lima_backend, device=DEV)


def test_processor_takes_a_fitted_scikit_model(lima_backend):
    pytest.importorskip("sklearn")
    from sklearn.linear_model import LinearRegression

    jobs = [(0.1 * k, text, label) for k in range(12) for text in (QASM, QASM2) for label in ("ZIIII", "IXIII", "IIIIZ")]
    X = _term_rows(lima_backend, jobs)
    ols = LinearRegression().fit(X.astype(np.float64), np.random.default_rng(0).normal(size=len(X)))
    obs = [PauliObservable([("ZIIII", 0.5), ("IXIII", -2.0)]), PauliObservable("IIIIZ")]
    sk = learning(FakeEstimator, ScikitLearningModelProcessor(ols, lima_backend), skip_transpile=True)
    dv = learning(FakeEstimator, LinearLearningModelProcessor(ols, lima_backend, device=DEV), skip_transpile=True)
    a = sk().run([QASM, QASM2], obs).result().values
    b = dv().run([QASM, QASM2], obs).result().values
    scale = float(np.abs(ols.coef_).max() * np.abs(X).max() * 76)
    print("processor vs scikit-learn:", a, b, "scale", scale)
    assert np.abs(a - b).max() <= 78 * 2.0 ** -53 * 3.0 * scale
