"""Host-side checks of the regression-forest path (blackwater.nn.ForestRegressor): the fixture, the packed node layout and its
float32 thresholds, the constructors' validation and the checkpoint route.  Nothing here touches a GPU."""
import io
import os

import numpy as np
import pytest
import torch

from blackwater.exception import BlackwaterException
from blackwater.nn import ForestRegressor
from blackwater.nn.forest import floor_to_float32

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "forest_g1.npz")))


def walk(tree_ptr, feature, threshold, left, right, X):
    """leaf[r, t]: tree t walked from its root, left iff x[feature] <= threshold, until ``left`` says leaf (-1).  The compare
    runs in float64 for float64 thresholds and in float32 for float32 ones (X is float32)."""
    n, T = X.shape[0], len(tree_ptr) - 1
    leaf = np.zeros((n, T), np.int64)
    rows = np.arange(n)
    for t in range(T):
        b = int(tree_ptr[t])
        at = np.zeros(n, np.int64)
        while True:
            live = left[b + at] >= 0
            if not live.any():
                break
            go_left = X[rows, np.maximum(feature[b + at], 0)] <= threshold[b + at]
            at = np.where(live, np.where(go_left, left[b + at], right[b + at]), at)
        leaf[:, t] = at
    return leaf


def predict_from_leaves(tree_ptr, value, leaf):
    return value[np.asarray(tree_ptr[:-1])[None, :] + leaf].mean(axis=1)


def unpack(module):
    """The packed buffers as (feature, thr32, left, right, orig) arrays the walk above takes: left child = next node."""
    nodes = module.nodes.numpy()
    feature, right, orig = nodes[:, 1].astype(np.int64), nodes[:, 2].astype(np.int64), nodes[:, 3].astype(np.int64)
    thr32 = nodes[:, 0].copy().view(np.float32)
    tree_ptr = module.tree_ptr.numpy()
    local = np.arange(nodes.shape[0]) - np.repeat(tree_ptr[:-1], np.diff(tree_ptr))
    left = np.where(feature < 0, -1, local + 1)
    return feature, thr32, left, right, orig


def arrays_of(fx):
    return fx["tree_ptr"], fx["feature"], fx["threshold"], fx["left"], fx["right"], fx["value"]


def test_fixture_is_self_consistent(fx):
    assert fx["X"].dtype == np.float32 and fx["X"].shape == (300, 58) and fx["leaf"].shape == (300, 100)
    assert fx["threshold"].dtype == np.float64
    leaf = walk(fx["tree_ptr"], fx["feature"], fx["threshold"], fx["left"], fx["right"], fx["X"])
    assert np.array_equal(leaf, fx["leaf"])
    pred = predict_from_leaves(fx["tree_ptr"], fx["value"], leaf)
    assert np.abs(pred - fx["pred"]).max() <= 1e-15
    # the fixture's power: thresholds rounded to the NEAREST float32 put some rows into other leaves
    nearest = walk(fx["tree_ptr"], fx["feature"], fx["threshold"].astype(np.float32), fx["left"], fx["right"], fx["X"])
    assert (nearest != fx["leaf"]).sum() > 0


def test_packed_float32_thresholds_reach_sklearns_leaves(fx):
    forest = ForestRegressor.from_arrays(*arrays_of(fx), n_features=58)
    assert forest.n_trees == 100 and forest.n_outputs == 4 and forest.n_features == 58 and forest.max_depth == 20
    assert forest.nodes.dtype == torch.int32 and forest.tree_ptr.dtype == torch.int64 and forest.value.dtype == torch.float64
    feature, thr32, left, right, orig = unpack(forest)
    assert thr32.dtype == np.float32
    packed_leaf = walk(forest.tree_ptr.numpy(), feature, thr32, left, right, fx["X"])
    leaf = orig[forest.tree_ptr.numpy()[:-1][None, :] + packed_leaf]
    assert np.array_equal(leaf, fx["leaf"])   # all 30 000 (row, tree) pairs
    # the packing is a permutation inside every tree, values stay in the model's order
    tp = fx["tree_ptr"]
    for t in (0, 57, 99):
        assert sorted(orig[tp[t]:tp[t + 1]].tolist()) == list(range(tp[t + 1] - tp[t]))
    assert np.array_equal(forest.value.numpy(), fx["value"])


def test_floor_to_float32_is_the_largest_float32_not_above():
    rng = np.random.default_rng(0)
    a = rng.normal(size=2000).astype(np.float32)
    mid = (a.astype(np.float64) + np.nextafter(a, np.float32(np.inf)).astype(np.float64)) / 2   # not representable
    thr = np.concatenate([mid, a.astype(np.float64), [0.0, -0.0, 1e-50, -1e-50, 3.5e38, -3.5e38]])
    got = floor_to_float32(thr)
    assert got.dtype == np.float32 and (got.astype(np.float64) <= thr).all()
    with np.errstate(over="ignore"):   # the float32 after the largest finite one is inf
        assert (np.nextafter(got, np.float32(np.inf)).astype(np.float64) > thr).all()
    assert np.array_equal(got[:2000], a) and np.array_equal(got[2000:4000], a)


def _same_buffers(a, b):
    return all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a.state_dict().values(), b.state_dict().values()))


def _from_trees(trees, n_features):
    tree_ptr = np.concatenate([[0], np.cumsum([t.node_count for t in trees])])
    cat = lambda name: np.concatenate([getattr(t, name) for t in trees])  # noqa: E731
    return ForestRegressor.from_arrays(tree_ptr, cat("feature"), cat("threshold"), cat("children_left"), cat("children_right"),
                                       cat("value"), n_features)


def test_from_sklearn_equals_from_arrays():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import ExtraTreesRegressor, RandomForestClassifier, RandomForestRegressor
    from sklearn.linear_model import LinearRegression
    from sklearn.tree import DecisionTreeRegressor

    rng = np.random.default_rng(1)
    X = rng.normal(size=(120, 7)).astype(np.float32)
    Y = rng.normal(size=(120, 3))
    for outputs in (Y, Y[:, 0]):
        k = 1 if outputs.ndim == 1 else 3
        rf = RandomForestRegressor(n_estimators=5, random_state=0).fit(X, outputs)
        et = ExtraTreesRegressor(n_estimators=4, random_state=0).fit(X, outputs)
        dt = DecisionTreeRegressor(random_state=0).fit(X, outputs)
        for model, trees in ((rf, [e.tree_ for e in rf.estimators_]), (et, [e.tree_ for e in et.estimators_]), (dt, [dt.tree_])):
            got = ForestRegressor.from_sklearn(model)
            assert got.n_outputs == k and got.n_trees == len(trees) and got.n_features == 7
            assert got.max_depth == max(t.max_depth for t in trees)
            assert _same_buffers(got, _from_trees(trees, 7))
            # and the packed walk reproduces the model's own apply()
            feature, thr32, left, right, orig = unpack(got)
            tp = got.tree_ptr.numpy()
            leaf = orig[tp[:-1][None, :] + walk(tp, feature, thr32, left, right, X)]
            want = model.apply(X)
            assert np.array_equal(leaf, want.reshape(len(X), -1))
    for bad in (RandomForestClassifier(n_estimators=2).fit(X, (Y[:, 0] > 0).astype(int)), RandomForestRegressor(), DecisionTreeRegressor(),
                ExtraTreesRegressor(), LinearRegression().fit(X, Y), object()):
        with pytest.raises(BlackwaterException):
            ForestRegressor.from_sklearn(bad)


def _tiny():
    """Two trees: a root with two leaves, and a three-level tree (node numbering as scikit-learn: depth-first)."""
    tree_ptr = np.array([0, 3, 8])
    feature = np.array([1, -2, -2, 0, 2, -2, -2, -2])
    threshold = np.array([0.5, -2.0, -2.0, 0.1, 0.7, -2.0, -2.0, -2.0])
    left = np.array([1, -1, -1, 1, 2, -1, -1, -1])
    right = np.array([2, -1, -1, 4, 3, -1, -1, -1])
    value = np.arange(8, dtype=np.float64)
    return dict(tree_ptr=tree_ptr, feature=feature, threshold=threshold, left=left, right=right, value=value, n_features=3)


def test_validation_refuses_malformed_forests():
    ok = ForestRegressor.from_arrays(**_tiny())
    assert ok.max_depth == 2 and ok.n_outputs == 1 and ok.n_trees == 2

    def broken(**edits):
        a = _tiny()
        for name, (i, v) in edits.items():
            a[name] = a[name].copy()
            a[name][i] = v
        return a

    for what, arrays in {
        "child out of range": broken(right=(0, 3)),            # tree 0 has three nodes
        "negative child": broken(left=(3, -5)),
        "cycle": broken(left=(4, 1)),                          # left[i] = i (global node 4 is node 1 of tree 1)
        "cycle through the root": broken(right=(4, 0)),
        "feature >= F": broken(feature=(3, 3)),
        "two parents": broken(right=(3, 2)),                   # node 2 of tree 1 is already node 1's child
        "half a leaf": broken(left=(5, 1)),
        "NaN threshold": broken(threshold=(0, np.nan)),
    }.items():
        with pytest.raises(ValueError):
            ForestRegressor.from_arrays(**arrays)
            pytest.fail(what)
    a = _tiny()
    a["left"][3], a["right"][3] = -1, -1                       # the root becomes a leaf: nodes 1..4 are unreachable
    with pytest.raises(ValueError, match="cannot be reached"):
        ForestRegressor.from_arrays(**a)
    for name, v in (("tree_ptr", np.array([0, 3, 3, 8])), ("tree_ptr", np.array([1, 3, 8])), ("value", np.zeros((8, 17))),
                    ("value", np.zeros(7)), ("n_features", 0), ("n_features", 40000), ("feature", np.zeros(7, np.int64))):
        a = _tiny()
        a[name] = v
        with pytest.raises(ValueError):
            ForestRegressor.from_arrays(**a)


def test_a_root_that_is_a_leaf_is_a_forest():
    f = ForestRegressor.from_arrays(np.array([0, 1]), np.array([-2]), np.array([-2.0]), np.array([-1]), np.array([-1]),
                                    np.array([[1.5, 2.5]]), 4)
    assert f.max_depth == 0 and f.n_outputs == 2 and f.nodes.tolist() == [[0, -1, 0, 0]]


def test_state_dict_round_trip(fx, tmp_path):
    forest = ForestRegressor.from_arrays(*arrays_of(fx), n_features=58)
    sd = forest.state_dict()
    assert set(sd) == {"nodes", "tree_ptr", "value", "meta"} and not list(forest.parameters())
    path = tmp_path / "forest.pth"
    torch.save(sd, path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    again = ForestRegressor.from_state_dict(loaded)
    assert _same_buffers(forest, again)
    for k in sd:
        assert again.state_dict()[k].numpy().tobytes() == sd[k].numpy().tobytes()
    assert (again.n_features, again.max_depth, again.n_trees, again.n_outputs) == (58, 20, 100, 4)
    forest.load_state_dict(loaded, strict=True)                  # same sizes: the plain route works too
    with pytest.raises(RuntimeError):
        ForestRegressor.from_arrays(**_tiny()).load_state_dict(loaded, strict=True)   # another forest's sizes
    for drop in sd:
        with pytest.raises(ValueError):
            ForestRegressor.from_state_dict({k: v for k, v in sd.items() if k != drop})
    with pytest.raises(ValueError):
        ForestRegressor.from_state_dict({**sd, "tree_ptr": sd["tree_ptr"][:-1]})
    buf = io.BytesIO()
    torch.save(sd, buf)
    assert buf.getbuffer().nbytes < 2 * (sd["nodes"].numel() * 4 + sd["value"].numel() * 8)


def test_forest_op_refuses_cpu_tensors(fx):
    from blackwater.native import _lib, ops

    forest = ForestRegressor.from_arrays(*arrays_of(fx), n_features=58)
    x = torch.from_numpy(fx["X"])
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.forest_predict(x, forest.nodes, forest.tree_ptr, forest.value, forest.max_depth)
    for call in (forest.predict, forest.apply, forest):
        with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
            call(x)
    with pytest.raises(ValueError):
        forest.predict(x[:, :57])


def test_forest_entry_point_validates_before_any_launch():
    from blackwater.native import _lib

    lib = _lib.load()
    assert "mlqem_forest_predict_f32" in _lib.SIGNATURES and _lib.ABI_VERSION >= 45
    f = lib.mlqem_forest_predict_f32
    assert f(None, 58, 0, 58, None, None, 100, None, 4, 20, None, None, None) == 0      # no rows: nothing to do
    assert f(None, 58, 8, 58, None, None, 100, None, 17, 20, None, None, None) == _lib.ERR_UNSUPPORTED   # K > 16
    assert f(None, 40000, 8, 40000, None, None, 100, None, 4, 20, None, None, None) == _lib.ERR_UNSUPPORTED   # F > 32767
    assert f(None, 58, 8, 58, None, None, 100, None, 4, 20, None, None, None) == -1    # null pointers
    assert f(None, 57, 8, 58, None, None, 100, None, 4, 20, None, None, None) == -1    # ldx < F
    assert f(None, 58, 8, 58, None, None, 0, None, 4, 20, None, None, None) == -1      # no trees
    assert f(None, 58, -1, 58, None, None, 1, None, 4, 20, None, None, None) == -1
