"""The regression-forest kernel (mlqem_forest_predict_f32) through ops.forest_predict, nn.ForestRegressor and
ForestLearningModelProcessor, on the device.  Oracle: a numpy walk with the float64 thresholds (scikit-learn's rule on float32
features).  Leaves must match exactly.  Predictions: both sides add T float64 leaf values (in different orders) and divide by T
once, so they may differ by 2 T 2^-53 max|leaf value| (2.2e-14 for T = 100, |v| <= 1) -- derived, not tuned."""
import os

import numpy as np
import pytest
import torch

from blackwater.data.backends import PauliObservable
from blackwater.library.learning.estimator import ForestLearningModelProcessor, ScikitLearningModelProcessor, learning
from blackwater.native import _lib, ops
from blackwater.nn import ForestRegressor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def walk(tree_ptr, feature, threshold, left, right, X):
    """leaf[r, t] for all (row, tree) pairs at once: left iff x[feature] <= threshold (float64 compare), until ``left`` is -1."""
    n, T = X.shape[0], len(tree_ptr) - 1
    base = np.asarray(tree_ptr[:-1], np.int64)[None, :]
    at = np.zeros((n, T), np.int64)
    rows = np.arange(n)[:, None]
    while True:
        node = base + at
        live = left[node] >= 0
        if not live.any():
            return at
        go_left = X[rows, np.maximum(feature[node], 0)].astype(np.float64) <= threshold[node]
        at = np.where(live, np.where(go_left, left[node], right[node]), at)


def oracle(forest_arrays, X):
    tree_ptr, feature, threshold, left, right, value = forest_arrays
    leaf = walk(tree_ptr, feature, threshold, left, right, X)
    picked = value[np.asarray(tree_ptr[:-1], np.int64)[None, :] + leaf]           # [n, T, K]
    return leaf, picked.sum(axis=1) / (len(tree_ptr) - 1)


def bound(forest_arrays):
    tree_ptr, value = forest_arrays[0], forest_arrays[5]
    return 2.0 * (len(tree_ptr) - 1) * 2.0 ** -53 * float(np.abs(value).max())


def grow_tree(rng, pool, splits, max_depth, chain=False):
    """A random binary tree in APPEND order (children get the next two free indices, so the numbering is not depth-first):
    ``splits`` times a leaf above ``max_depth`` is split (``chain``: always the deepest one).  Thresholds are float64 midpoints
    of two adjacent float32 values of the feature's pool (not representable in float32), every fourth one a pool value itself."""
    F = pool.shape[0]
    feature, threshold, left, right, depth = [-2], [-2.0], [-1], [-1], [0]
    open_leaves = [0]
    for _ in range(splits):
        if not open_leaves:
            break
        i = open_leaves.pop(-1 if chain else int(rng.integers(len(open_leaves))))
        f = int(rng.integers(F))
        a = pool[f, int(rng.integers(pool.shape[1]))]
        up = np.nextafter(a, np.float32(np.inf))
        feature[i] = f
        threshold[i] = float(a) if rng.integers(4) == 0 else (float(a) + float(up)) / 2
        left[i], right[i] = len(feature), len(feature) + 1
        for _ in range(2):
            feature.append(-2); threshold.append(-2.0); left.append(-1); right.append(-1); depth.append(depth[i] + 1)
            if depth[-1] < max_depth:
                open_leaves.append(len(feature) - 1)
    return feature, threshold, left, right


def make_forest(seed, F, K, T, big=False):
    """(tree_ptr, feature, threshold, left, right, value) and the feature pool rows are drawn from.  Trees cycle through a root
    that is a leaf (depth 0), a chain of depth 24 and random trees of 1..60 splits; ``big``: tree 0 has >= 2^16 nodes."""
    rng = np.random.default_rng(seed)
    pool = rng.normal(size=(F, 12)).astype(np.float32)
    parts, counts = [], []
    for t in range(T):
        kind = (t + seed) % 7
        if big and t == 0:
            tree = grow_tree(rng, pool, 33000, 24)
        elif kind == 0:
            tree = grow_tree(rng, pool, 0, 24)
        elif kind == 1:
            tree = grow_tree(rng, pool, 24, 24, chain=True)
        else:
            tree = grow_tree(rng, pool, int(rng.integers(1, 61)), 24)
        parts.append(tree)
        counts.append(len(tree[0]))
    tree_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    feature, threshold, left, right = (np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(4))
    value = rng.uniform(-1.0, 1.0, size=(int(tree_ptr[-1]), K))
    return (tree_ptr, feature.astype(np.int64), threshold.astype(np.float64), left.astype(np.int64), right.astype(np.int64), value), pool


def make_rows(seed, pool, n):
    """Rows whose every entry is a pool value or the float32 right after it: they sit exactly on and next to the split values."""
    rng = np.random.default_rng(seed + 1000)
    F = pool.shape[0]
    pick = pool[np.arange(F)[None, :], rng.integers(pool.shape[1], size=(n, F))]
    return np.where(rng.integers(2, size=(n, F)) == 0, pick, np.nextafter(pick, np.float32(np.inf))).astype(np.float32)


def module_of(arrays, F):
    return ForestRegressor.from_arrays(*arrays, n_features=F).to(DEV)


def check(forest, arrays, X, x_dev=None):
    want_leaf, want_pred = oracle(arrays, X)
    x_dev = torch.from_numpy(X).to(DEV) if x_dev is None else x_dev
    leaf = forest.apply(x_dev)
    pred = forest.predict(x_dev)
    assert leaf.dtype == torch.int32 and tuple(leaf.shape) == want_leaf.shape and pred.dtype == torch.float64
    assert np.array_equal(leaf.cpu().numpy(), want_leaf)
    got = pred.cpu().numpy().reshape(want_pred.shape)
    err = float(np.abs(got - want_pred).max()) if got.size else 0.0
    print(f"rows {X.shape[0]} F {X.shape[1]} T {forest.n_trees} K {forest.n_outputs}: max |pred - oracle| = {err:.3e}, bound {bound(arrays):.3e}")
    assert err <= bound(arrays)
    return pred


def test_fixture_forest_matches_sklearn_on_the_device():
    fx = dict(np.load(os.path.join(GOLDEN, "forest_g1.npz")))
    arrays = tuple(fx[k] for k in ("tree_ptr", "feature", "threshold", "left", "right", "value"))
    forest = module_of(arrays, 58)
    x = torch.from_numpy(fx["X"]).to(DEV)
    leaf = forest.apply(x).cpu().numpy()
    assert leaf.shape == (300, 100) and np.array_equal(leaf, fx["leaf"])          # all 30 000 pairs
    pred = forest.predict(x)
    err = float(np.abs(pred.cpu().numpy() - fx["pred"]).max())
    limit = 2 * 100 * 2.0 ** -53 * float(np.abs(fx["value"]).max())
    print(f"fixture: max |predict - sklearn| = {err:.3e}, bound {limit:.3e}")
    assert tuple(pred.shape) == (300, 4) and err <= limit
    fwd = forest(x)
    assert fwd.dtype == torch.float32 and torch.equal(fwd, pred.to(torch.float32))


@pytest.mark.parametrize("T", [1, 3, 100, 300])
@pytest.mark.parametrize("K", [1, 4, 8, 16])
@pytest.mark.parametrize("F", [1, 58, 170])
def test_synthetic_forests(F, K, T):
    seed = 7 * F + 3 * K + T
    arrays, pool = make_forest(seed, F, K, T)
    forest = module_of(arrays, F)
    for n in (1, 63, 64, 65, 4099):
        pred = check(forest, arrays, make_rows(seed + n, pool, n))
        assert tuple(pred.shape) == ((n,) if K == 1 else (n, K))


def test_depth_zero_and_depth_24():
    for seed, want_depth in ((0, 0), (1, 24)):          # (t + seed) % 7: a lone root that is a leaf; a chain of 24 splits
        arrays, pool = make_forest(seed, 58, 4, 1)
        forest = module_of(arrays, 58)
        assert forest.max_depth == want_depth
        check(forest, arrays, make_rows(seed, pool, 65))


def test_tree_larger_than_any_lds_staging():
    arrays, pool = make_forest(11, 58, 4, 3, big=True)
    assert arrays[0][1] >= 2 ** 16
    check(module_of(arrays, 58), arrays, make_rows(11, pool, 4099))


def test_many_rows_take_the_wide_tiles():
    """Row counts past the launcher's tile switches (64-row and 16-row tiles), and a row width that does not fit the staging area."""
    arrays, pool = make_forest(5, 58, 4, 100)
    forest = module_of(arrays, 58)
    x = make_rows(5, pool, 40001)
    big = check(forest, arrays, x)
    small = torch.cat([forest.predict(torch.from_numpy(x[i:i + 5000]).to(DEV)) for i in range(0, 40001, 5000)])
    assert torch.equal(big, small)
    check(forest, arrays, x[:9001])
    arrays, pool = make_forest(6, 4000, 2, 5)
    check(module_of(arrays, 4000), arrays, make_rows(6, pool, 300))


def test_strided_rows_with_nan_in_the_pad_columns():
    arrays, pool = make_forest(3, 58, 4, 100)
    forest = module_of(arrays, 58)
    X = make_rows(3, pool, 4099)
    wide = torch.full((4099, 64), float("nan"), device=DEV)
    wide[:, :58] = torch.from_numpy(X).to(DEV)
    view = wide[:, :58]
    assert view.stride(0) == 64 and torch.isnan(wide[:, 58:]).all()
    check(forest, arrays, X, x_dev=view)


def test_deterministic_and_independent_of_row_tiling():
    arrays, pool = make_forest(9, 170, 8, 300)
    forest = module_of(arrays, 170)
    x = torch.from_numpy(make_rows(9, pool, 4099)).to(DEV)
    a, b = forest.predict(x), forest.predict(x)
    assert torch.equal(a, b) and torch.equal(forest.apply(x), forest.apply(x))
    parts = torch.cat([forest.predict(x[i:i + 1000]) for i in range(0, 4099, 1000)])
    assert torch.equal(a, parts)
    assert torch.equal(a[:1], forest.predict(x[:1])) and torch.equal(a[4098:], forest.predict(x[4098:]))


def test_captured_in_a_graph_and_replayed_on_new_rows():
    arrays, pool = make_forest(4, 58, 4, 100)
    forest = module_of(arrays, 58)
    n = 4099
    x = torch.from_numpy(make_rows(4, pool, n)).to(DEV)
    out = torch.empty((n, 4), dtype=torch.float64, device=DEV)
    leaf = torch.empty((n, 100), dtype=torch.int32, device=DEV)

    def run():
        return ops.forest_predict(x, forest.nodes, forest.tree_ptr, forest.value, forest.max_depth, out=out, leaf_out=leaf)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        got = run()
    assert got[0] is out and got[1] is leaf
    for k in range(3):
        fresh = torch.from_numpy(make_rows(40 + k, pool, n)).to(DEV)
        x.copy_(fresh)
        out.zero_()
        leaf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, forest.predict(fresh).reshape(n, 4)) and torch.equal(leaf, forest.apply(fresh))


def test_unsupported_shapes_are_refused_without_a_launch():
    arrays, pool = make_forest(2, 58, 16, 3)
    forest = module_of(arrays, 58)
    x = torch.from_numpy(make_rows(2, pool, 8)).to(DEV)
    wide = torch.zeros((forest.value.shape[0], 17), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.NativeLibraryError, match="unsupported"):
        ops.forest_predict(x, forest.nodes, forest.tree_ptr, wide, forest.max_depth)
    with pytest.raises(ValueError):
        ForestRegressor.from_arrays(*arrays[:5], np.zeros((len(arrays[1]), 17)), n_features=58)
    empty = forest.predict(x[:0])
    assert tuple(empty.shape) == (0, 16) and tuple(forest.apply(x[:0]).shape) == (0, 3)
    torch.cuda.synchronize()


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


def _term_rows(lima_backend, jobs):
    """The 76-wide encode_data rows of (noisy value, text, Pauli label) triples, as the processors build them."""
    from blackwater.data.utils import encode_pauli_sum_op, get_backend_properties_v1
    from blackwater.library.learning.features import encode_data

    props = get_backend_properties_v1(lima_backend)
    rows = [encode_data(circuits=[text], properties=props, ideal_exp_vals=[[0.0]], noisy_exp_vals=[[value]], num_qubits=1,
                        meas_bases=encode_pauli_sum_op([(label, 1.0)]))[0] for value, text, label in jobs]
    return torch.cat(rows).numpy().astype(np.float32)


def _row_forest(seed, rows):
    """A seeded forest over 76-wide rows whose split values come from the rows' own columns (so the walks branch both ways)."""
    rng = np.random.default_rng(seed)
    pool = np.stack([rng.choice(rows[:, f], size=12) for f in range(rows.shape[1])]).astype(np.float32)
    parts = [grow_tree(rng, pool, int(rng.integers(5, 40)), 12) for _ in range(20)]
    tree_ptr = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    feature, threshold, left, right = (np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(4))
    value = rng.uniform(-1.0, 1.0, size=(int(tree_ptr[-1]), 1))
    return (tree_ptr, feature.astype(np.int64), threshold.astype(np.float64), left.astype(np.int64), right.astype(np.int64), value)


def test_decorator_end_to_end(lima_backend):
    two_terms = PauliObservable([("ZIIII", 0.5), ("IXIII", -2.0)])
    one_term = PauliObservable("IIIIZ")
    jobs = [(0.5, QASM, "ZIIII"), (0.5, QASM, "IXIII"), (0.6, QASM2, "IIIIZ")]
    rows = _term_rows(lima_backend, jobs)
    assert rows.shape == (3, 76)
    arrays = _row_forest(0, rows)
    forest = ForestRegressor.from_arrays(*arrays, n_features=76)
    proc = ForestLearningModelProcessor(forest, lima_backend, device=DEV)
    assert proc.accepts_qasm_text
    got = learning(FakeEstimator, proc, skip_transpile=True)().run([QASM, QASM2], [two_terms, one_term]).result()
    serial = [proc.process(0.5, QASM, two_terms, ()), proc.process(0.6, QASM2, one_term, ())]
    assert got.values.tolist() == serial
    pred = oracle(arrays, rows)[1][:, 0]
    want = [pred[0] * 0.5 + pred[1] * -2.0, pred[2] * 1.0]
    print("decorator: max |device - oracle| =", float(np.abs(got.values - np.asarray(want)).max()))
    assert np.abs(got.values - np.asarray(want)).max() <= 1e-12
    assert got.metadata[0] == {"shots": 7, "original_value": 0.5} and got.metadata[1]["original_value"] == pytest.approx(0.6)


def test_decorator_equals_the_scikit_processor(lima_backend):
    pytest.importorskip("sklearn")
    from sklearn.ensemble import RandomForestRegressor

    from blackwater.exception import BlackwaterException

    jobs = [(0.1 * k, text, label) for k in range(12) for text in (QASM, QASM2) for label in ("ZIIII", "IXIII", "IIIIZ")]
    rows = _term_rows(lima_backend, jobs)
    rng = np.random.default_rng(0)
    rf = RandomForestRegressor(n_estimators=30, random_state=0).fit(rows, rng.normal(size=len(rows)))
    obs = [PauliObservable([("ZIIII", 0.5), ("IXIII", -2.0)]), PauliObservable("IIIIZ")]
    sk = learning(FakeEstimator, ScikitLearningModelProcessor(rf, lima_backend), skip_transpile=True)
    dev = learning(FakeEstimator, ForestLearningModelProcessor(rf, lima_backend, device=DEV), skip_transpile=True)
    a = sk().run([QASM, QASM2], obs).result().values
    b = dev().run([QASM, QASM2], obs).result().values
    print("decorator vs scikit-learn:", a, b)
    assert np.abs(a - b).max() <= 1e-12
    with pytest.raises(BlackwaterException):
        ForestLearningModelProcessor(object(), lima_backend, device=DEV)
