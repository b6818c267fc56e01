"""Out-of-bag prediction on the device (mlqem_forest_predict_oob_f32 through ops.forest_predict_oob and ForestRegressor.oob_predict /
fit(oob_score=True) / oob_permutation_importance).

The bar is EQUALITY, not a tolerance.  The kernel adds, per (row, output), the float64 leaf values of the trees that left the row
out, in tree order from 0.0, and divides once by their number; tests/forest_oob_cases.oob_restatement does the same in numpy, and so
does scikit-learn (estimator order), whose ``oob_prediction_`` is stored in tests/golden/forest_oob_g1.npz.  The leaves the restatement
reads come from the module's ``apply`` (the plain kernel: another instantiation, no counts) or, for the fixture, from nowhere at all:
the stored prediction is scikit-learn's own.  R^2 values are compared within 1e-12 (two float64 sums of <= 300 terms of order 1: about
n 2^-53 = 3e-14)."""
import warnings

import numpy as np
import pytest
import torch

import forest_fit_cases as fc
import forest_oob_cases as oc
from blackwater.native import ops
from blackwater.nn import ForestRegressor
from blackwater.nn.forest import r2_score
from test_gpu_forest import make_forest, make_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BUFFERS = ("nodes", "tree_ptr", "value", "meta")
OOB_MESSAGE = "Some inputs do not have OOB scores"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def oob_calls(fn):
    """(result of fn(), number of out-of-bag UserWarnings it raised)."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        result = fn()
    return result, sum(1 for w in caught if issubclass(w.category, UserWarning) and OOB_MESSAGE in str(w.message))


@pytest.fixture(scope="module")
def sk_cases():
    return oc.load_fixture()


@pytest.mark.parametrize("i", range(len(oc.CASES)))
def test_scikit_learn_oob_prediction_bit_for_bit(sk_cases, i):
    case = sk_cases[i]
    n, K = case["n"], case["K"]
    forest = ForestRegressor.from_arrays(*(case[k] for k in oc.TREE_KEYS), n_features=case["F"]).to(DEV)
    (pred, n_oob), warned = oob_calls(lambda: forest.oob_predict(dev(case["X"]), dev(case["counts"]), return_counts=True))
    assert pred.dtype == torch.float64 and tuple(pred.shape) == ((n,) if K == 1 else (n, K)) and n_oob.dtype == torch.int32
    got = pred.cpu().numpy().reshape(n, K)
    print(f"case {i}: max |device - scikit-learn| = {np.abs(got - case['oob_prediction']).max():.3e}")
    assert np.array_equal(got, case["oob_prediction"])
    assert np.array_equal(n_oob.cpu().numpy(), (case["counts"] == 0).sum(axis=0))
    assert warned == (1 if case["empty_rows"] else 0)
    score = float(r2_score(dev(case["y"]), pred))
    print(f"case {i}: |device R^2 - oob_score_| = {abs(score - float(case['oob_score'])):.3e}")
    assert abs(score - float(case["oob_score"])) <= 1e-12


# (n, F, K, T).  n: 1, 5 (the 4-row tile, two workgroups), 8192 + 3 (the 16-row tile), 32768 + 5 (the 64-row tile); T: 1, 17, 300 (past
# the 256-tree chunk of the 4-row tile); K: 1, 3, 16; F = 3100: no tile's rows fit the LDS budget, x is read from global memory.
# Forests of make_forest: tree t is a lone leaf, a chain of depth 24 or a random tree by (t + seed) % 7.
GRID = [(1, 4, 1, 1), (1, 6, 3, 17), (5, 3, 1, 17), (5, 5, 16, 300), (5, 4, 3, 1), (8195, 6, 3, 17), (8195, 4, 16, 1),
        (32773, 6, 1, 17), (32773, 5, 16, 17), (32773, 4, 3, 1), (6, 3100, 3, 17)]


@pytest.mark.parametrize("n,F,K,T", GRID)
def test_grid_against_the_numpy_restatement(n, F, K, T):
    seed = 11 * F + 5 * K + T + n % 97
    arrays, pool = make_forest(seed, F, K, T)
    forest = ForestRegressor.from_arrays(*arrays, n_features=F).to(DEV)
    x = dev(make_rows(seed, pool, n))
    counts = oc.seeded_counts(seed, T, n)
    if n >= 2:
        assert (counts[:, 0] > 0).all() and (counts[:, n - 1] == 0).all()
    apply = forest.apply(x).cpu().numpy()
    want, want_n = oc.oob_restatement(apply, arrays[0], arrays[5], counts)
    out, n_oob, leaf = ops.forest_predict_oob(x, forest.nodes, forest.tree_ptr, forest.value, forest.max_depth, dev(counts), want_leaf=True)
    assert out.dtype == torch.float64 and tuple(out.shape) == (n, K) and tuple(n_oob.shape) == (n,) and tuple(leaf.shape) == (n, T)
    assert np.array_equal(n_oob.cpu().numpy(), want_n)
    assert np.array_equal(leaf.cpu().numpy(), np.where(counts.T == 0, apply, -1))
    got = out.cpu().numpy()
    print(f"rows {n} F {F} K {K} T {T}: max |device - restatement| = {np.abs(got - want).max():.3e}")
    assert np.array_equal(got, want)
    (pred, cnt), warned = oob_calls(lambda: forest.oob_predict(x, dev(counts), return_counts=True))
    assert torch.equal(pred.reshape(n, K), out) and torch.equal(cnt, n_oob) and warned == int((want_n == 0).any())


def test_identities():
    F, K, T, n = 6, 3, 17, 33000
    arrays, pool = make_forest(21, F, K, T)
    forest = ForestRegressor.from_arrays(*arrays, n_features=F).to(DEV)
    x = dev(make_rows(21, pool, n))
    counts = dev(oc.seeded_counts(21, T, n))
    before = forest.predict(x)
    (full, full_n), _ = oob_calls(lambda: forest.oob_predict(x, counts, return_counts=True))
    (again, again_n), _ = oob_calls(lambda: forest.oob_predict(x, counts, return_counts=True))
    assert torch.equal(full, again) and torch.equal(full_n, again_n)                       # two calls, equal bits
    assert torch.equal(forest.predict(x), before)                                          # the plain entry is untouched
    # no tree drew any row: the plain mean, bit for bit
    (none, none_n), warned = oob_calls(lambda: forest.oob_predict(x, torch.zeros_like(counts), return_counts=True))
    assert torch.equal(none, before) and bool((none_n == T).all()) and warned == 0
    # every tree drew every row: zeros, and the warning
    (every, every_n), warned = oob_calls(lambda: forest.oob_predict(x, torch.full_like(counts, 2), return_counts=True))
    assert not every.any() and not every_n.any() and warned == 1
    # column slices of the counts (row stride n, no copy) with the matching rows: another tile (16 rows, 4 rows), another ldc
    for a, b in ((100, 8400), (5, 300), (32999, 33000)):
        view = counts[:, a:b]
        assert view.stride(0) == n and view.data_ptr() == counts.data_ptr() + 4 * a
        (part, part_n), _ = oob_calls(lambda: forest.oob_predict(x[a:b], view, return_counts=True))
        assert torch.equal(part, full[a:b]) and torch.equal(part_n, full_n[a:b])


def test_fit_with_oob_score():
    n, F, K, T = 300, 6, 2, 20
    X, y = fc.make_pool_rows(4, n, F), fc.make_targets(4, n, K)
    x, yd = dev(X), dev(y)
    plain = ForestRegressor.fit(x, yd, n_estimators=T, seed=3)
    forest, _ = oob_calls(lambda: ForestRegressor.fit(x, yd, n_estimators=T, seed=3, oob_score=True))
    for name in BUFFERS:
        assert torch.equal(getattr(plain, name), getattr(forest, name)), name
    assert not hasattr(plain, "oob_score_") and "sample_counts" not in plain.fit_info
    counts = forest.fit_info["sample_counts"]
    assert counts.dtype == torch.int32 and counts.is_cuda and np.array_equal(counts.cpu().numpy(), fc.bootstrap_counts(n, T, 3))
    (pred, cnt), _ = oob_calls(lambda: forest.oob_predict(x, counts, return_counts=True))
    assert forest.oob_prediction_.dtype == torch.float64 and forest.oob_prediction_.is_cuda and torch.equal(forest.oob_prediction_, pred)
    assert forest.oob_count_.dtype == torch.int32 and torch.equal(forest.oob_count_, cnt)
    assert np.array_equal(cnt.cpu().numpy(), (fc.bootstrap_counts(n, T, 3) == 0).sum(axis=0))
    want = oc.r2_rule(y, pred.cpu().numpy())
    print(f"fit: oob_score_ {forest.oob_score_!r}, host rule {want!r}")
    assert isinstance(forest.oob_score_, float) and abs(forest.oob_score_ - want) <= 1e-12
    held_in = forest.score(x, yd)
    assert abs(held_in - oc.r2_rule(y, forest.predict(x).cpu().numpy())) <= 1e-12 and held_in > forest.oob_score_
    state = forest.state_dict()
    assert sorted(state) == sorted(plain.state_dict()) == sorted(BUFFERS)
    back = ForestRegressor.from_state_dict(state).to(DEV)
    (pred2, cnt2), _ = oob_calls(lambda: back.oob_predict(x, counts, return_counts=True))
    assert torch.equal(pred2, pred) and torch.equal(cnt2, cnt) and not hasattr(back, "oob_score_")
    # explicit bags are allowed whatever bootstrap says
    explicit, _ = oob_calls(lambda: ForestRegressor.fit(x, yd, bootstrap=False, sample_counts=counts, oob_score=True))
    assert explicit.oob_score_ == forest.oob_score_ and torch.equal(explicit.oob_prediction_, pred)


def test_captured_in_a_graph():
    F, K, T, n = 6, 3, 17, 4099
    arrays, pool = make_forest(8, F, K, T)
    forest = ForestRegressor.from_arrays(*arrays, n_features=F).to(DEV)
    x = dev(make_rows(8, pool, n))
    counts = dev(oc.seeded_counts(8, T, n))
    want = ops.forest_predict_oob(x, forest.nodes, forest.tree_ptr, forest.value, forest.max_depth, counts, want_leaf=True)
    out = torch.empty((n, K), dtype=torch.float64, device=DEV)
    n_oob = torch.empty((n,), dtype=torch.int32, device=DEV)
    leaf = torch.empty((n, T), dtype=torch.int32, device=DEV)

    def run():
        return ops.forest_predict_oob(x, forest.nodes, forest.tree_ptr, forest.value, forest.max_depth, counts, out=out, n_oob_out=n_oob,
                                      leaf_out=leaf)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):          # one launch, a straight line
        got = run()
    assert got[0] is out and got[1] is n_oob and got[2] is leaf
    for _ in range(2):
        out.zero_()
        n_oob.zero_()
        leaf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want[0]) and torch.equal(n_oob, want[1]) and torch.equal(leaf, want[2])


def test_permutation_importance():
    """Against a host restatement that builds every permuted matrix explicitly, takes its leaves from ``apply`` and forms the masked
    means in numpy.  Bound: both sides hold the SAME float64 predictions (the tests above) and so the same squared residuals, each at
    most M = max (y - p)^2.  A mean of m <= n of them is a sum of m non-negative terms -- each addition rounds by at most 2^-53 of a
    partial sum <= m M, so the sum is within (m - 1) 2^-53 m M of the exact one in whatever order it is formed -- and one division:
    within n 2^-53 M of the exact mean on either side, 2 n 2^-53 M between the sides.  An importance is the difference of two such
    means (permuted, base): 4 n 2^-53 M."""
    n, F, K, T, repeats, seed = 200, 5, 1, 30, 2, 5
    rng = np.random.default_rng(17)
    X = np.concatenate([rng.normal(size=(n, F)).astype(np.float32), np.full((n, 1), 0.25, np.float32)], axis=1)   # a constant column appended
    y = 2.0 * X[:, 1].astype(np.float64) + 0.1 * rng.normal(size=n)
    x, yd = dev(X), dev(y)
    forest, _ = oob_calls(lambda: ForestRegressor.fit(x, yd, n_estimators=T, seed=1, oob_score=True))
    counts = forest.fit_info["sample_counts"]
    kept = x.clone()
    got, _ = oob_calls(lambda: forest.oob_permutation_importance(x, yd, counts, n_repeats=repeats, seed=seed))
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (F + 1,) and torch.equal(x, kept)

    host_counts = counts.cpu().numpy()
    tree_ptr, value = forest.tree_ptr.cpu().numpy(), forest.value.cpu().numpy()
    worst = 0.0

    def mse(rows):
        nonlocal worst
        pred, n_oob = oc.oob_restatement(forest.apply(dev(rows)).cpu().numpy(), tree_ptr, value, host_counts)
        sq = (y[:, None] - pred) ** 2
        worst = max(worst, float(sq.max()))
        return float(sq[n_oob > 0].mean())

    base = mse(X)
    want = np.zeros(F + 1)
    for f in range(F + 1):
        total = 0.0
        for j in range(repeats):
            shuffled = X.copy()
            shuffled[:, f] = X[np.random.default_rng([seed, f, j]).permutation(n), f]
            total += mse(shuffled)
        want[f] = total / repeats - base
    bound = 4 * n * 2.0 ** -53 * worst
    print(f"importance {got}, max |device - host| = {np.abs(got - want).max():.3e}, bound {bound:.3e}")
    assert np.abs(got - want).max() <= bound
    assert got[F] == 0.0                                 # no tree splits on the constant column
    assert int(np.argmax(got)) == 1 and got[1] > 0.0     # y was built from column 1
    again, _ = oob_calls(lambda: forest.oob_permutation_importance(x, yd, counts, n_repeats=repeats, seed=seed))
    assert np.array_equal(got, again)
    with pytest.raises(ValueError, match="out-of-bag"):
        forest.oob_permutation_importance(x, yd, torch.ones_like(counts))
