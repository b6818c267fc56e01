"""Host side of the gradient-boosted path (blackwater.nn.BoostedRegressor): the fixture against the checker of
tests/boost_cases.py, the constructors' validation, the checkpoint route, ``fit``'s argument checks (all made before a device is
touched), the documented bag generator and the new entry points' own argument checks.  Nothing here touches a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import boost_cases as bc
from blackwater.exception import BlackwaterException
from blackwater.native import _lib, ops
from blackwater.nn import BoostedRegressor
from blackwater.nn.boost import subsample_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, G1 = bc.load_fixture()
IDS = [c["name"] for c in CASES]


def module_of(case):
    return BoostedRegressor.from_arrays(*(case["trees"][k] for k in bc.KEYS), n_features=case["X"].shape[1], init=case["init"],
                                        learning_rate=case["lr"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_passes_check_stages(case):
    X, y, T = case["X"], case["y"], len(case["trees"]["tree_ptr"]) - 1
    gap = bc.check_stages(X, y, np.ones((T, len(X)), np.int32), case["params"], case["lr"], case["init"], case["trees"])
    print(case["name"], "smallest relative score gap", gap)
    assert gap >= 1e-9                                                            # tie-free, as the generator promises
    # the multiply-then-add restatement IS scikit-learn's predict_stages, and it reproduces train_score_
    staged = bc.staged_reference(case["trees"], X, case["init"], case["lr"])
    assert np.array_equal(staged, case["staged"]) and np.array_equal(staged[-1], case["pred"])
    train, _, _ = bc.stage_losses(X, y, np.ones((T, len(X)), np.int32), case["lr"], case["init"], case["trees"])
    assert np.abs(train - case["train_score"]).max() <= len(X) * bc.U * case["train_score"].max()
    assert 0.0 < bc.prediction_bound(X, y, case["init"], case["lr"], case["trees"]) < 1e-9    # stump: (1 + 0.5)^20 of a rounding


def test_fixture_holds_what_the_issue_describes():
    shapes = {c["name"]: (*c["X"].shape, len(c["trees"]["tree_ptr"]) - 1, c["params"]["max_depth"], c["lr"]) for c in CASES}
    assert shapes == {"d3": (160, 5, 12, 3, 0.1), "stump": (64, 3, 20, 1, 0.5), "leaf4": (130, 6, 10, 4, 0.2), "dups": (100, 4, 8, 2, 0.3)}
    dups = CASES[IDS.index("dups")]["X"]
    assert (dups[:, 3] == dups[0, 3]).all() and np.unique(dups[:, 0]).size < dups.shape[0]
    assert CASES[IDS.index("leaf4")]["params"]["min_samples_leaf"] == 4
    sub05, sub10 = G1["sklearn_g1_l2_sub05"], G1["sklearn_g1_l2_sub10"]
    assert sub05.shape == (20,) and sub10.shape == (20,)
    assert abs(sub05.mean() + 5 * sub05.std() - 0.020997) < 1e-6 and sub05.mean() + 5 * sub05.std() < 0.025461
    assert os.path.getsize(os.path.join(bc.GOLDEN, "boost_g1.npz")) < 608 * 1024


def test_checker_rejects_a_wrong_init_and_a_mutated_stage():
    case = CASES[0]
    X, y, T = case["X"], case["y"], len(case["trees"]["tree_ptr"]) - 1
    masks = np.ones((T, len(X)), np.int32)
    with pytest.raises(AssertionError, match="not the mean"):
        bc.check_stages(X, y, masks, case["params"], case["lr"], case["init"] + 1e-9, case["trees"])
    bad = {k: np.array(v, copy=True) for k, v in case["trees"].items()}
    leaf = int(np.flatnonzero(bad["left"] < 0)[0])
    bad["value"][leaf] += 1e-9                                                    # stage 0's first leaf
    with pytest.raises(AssertionError, match="stage 0: .*value off"):
        bc.check_stages(X, y, masks, case["params"], case["lr"], case["init"], bad)
    # a later stage sees the residuals of the mutated one: its values no longer fit either
    bad = {k: np.array(v, copy=True) for k, v in case["trees"].items()}
    b = int(bad["tree_ptr"][3])
    bad["threshold"][b] = np.nextafter(bad["threshold"][b], np.inf)
    with pytest.raises(AssertionError, match="stage 3: .*midpoint"):
        bc.check_stages(X, y, masks, case["params"], case["lr"], case["init"], bad)


def _tiny():
    """Two stages: a root with two leaves, and a three-level tree (node numbering as scikit-learn: depth-first)."""
    return dict(tree_ptr=np.array([0, 3, 8]), feature=np.array([1, -2, -2, 0, 2, -2, -2, -2]),
                threshold=np.array([0.5, -2.0, -2.0, 0.1, 0.7, -2.0, -2.0, -2.0]), left=np.array([1, -1, -1, 1, 2, -1, -1, -1]),
                right=np.array([2, -1, -1, 4, 3, -1, -1, -1]), value=np.arange(8, dtype=np.float64), n_features=3, init=0.25,
                learning_rate=0.1)


def test_validation_refuses_malformed_ensembles():
    ok = BoostedRegressor.from_arrays(**_tiny())
    assert (ok.max_depth, ok.n_outputs, ok.n_stages, ok.n_features, ok.init, ok.learning_rate) == (2, 1, 2, 3, 0.25, 0.1)
    assert ok.scale.dtype == torch.float64 and ok.scale.tolist() == [0.25, 0.1] and tuple(ok.value.shape) == (8, 1)

    def broken(**edits):
        a = _tiny()
        for name, (i, v) in edits.items():
            a[name] = a[name].copy()
            a[name][i] = v
        return a

    for message, arrays in {
        "right child 3 is out of range": broken(right=(0, 3)),
        "left child -5 is out of range": broken(left=(3, -5)),
        "more than one parent|cannot be reached": broken(left=(4, 1)),
        "a root is some node's child": broken(right=(4, 0)),
        "splits on feature 3": broken(feature=(3, 3)),
        "more than one parent": broken(right=(3, 2)),
        "has one child": broken(left=(5, 1)),
        "threshold is NaN": broken(threshold=(0, np.nan)),
    }.items():
        with pytest.raises(ValueError, match=message):
            BoostedRegressor.from_arrays(**arrays)
    a = _tiny()
    a["left"][3], a["right"][3] = -1, -1
    with pytest.raises(ValueError, match="cannot be reached"):
        BoostedRegressor.from_arrays(**a)
    for name, v, message in (("tree_ptr", np.array([0, 3, 3, 8]), "increase strictly"), ("tree_ptr", np.array([1, 3, 8]), "start at 0"),
                             ("tree_ptr", np.array([0.0, 3.0, 8.0]), "integer array"), ("value", np.zeros((8, 2)), "one output"),
                             ("value", np.zeros(7), "value must be"), ("n_features", 0, "n_features"), ("n_features", 40000, "n_features"),
                             ("feature", np.zeros(7, np.int64), "one entry per node"), ("left", np.zeros(8), "integer array"),
                             ("init", np.nan, "scale"), ("learning_rate", np.inf, "scale"), ("init", "mean", "scale"),
                             ("learning_rate", None, "scale")):
        a = _tiny()
        a[name] = v
        with pytest.raises(ValueError, match=message):
            BoostedRegressor.from_arrays(**a)
    stump = BoostedRegressor.from_arrays(np.array([0, 1]), np.array([-2]), np.array([-2.0]), np.array([-1]), np.array([-1]),
                                         np.array([[[1.5]]]), 4, 0.0, 1.0)      # scikit-learn's [N, 1, 1]
    assert stump.max_depth == 0 and stump.nodes.tolist() == [[0, -1, 0, 0]]


def test_state_dict_round_trip(tmp_path):
    model = module_of(CASES[0])
    sd = model.state_dict()
    assert set(sd) == {"nodes", "tree_ptr", "value", "meta", "scale"} and not list(model.parameters())
    path = tmp_path / "boost.pth"
    torch.save(sd, path)
    loaded = torch.load(path, map_location="cpu", weights_only=True)
    again = BoostedRegressor.from_state_dict(loaded)
    for k in sd:
        assert again.state_dict()[k].dtype == sd[k].dtype and again.state_dict()[k].numpy().tobytes() == sd[k].numpy().tobytes()
    assert (again.n_features, again.max_depth, again.n_stages, again.init, again.learning_rate) == (5, 3, 12, CASES[0]["init"], 0.1)
    model.load_state_dict(loaded, strict=True)
    with pytest.raises(RuntimeError):
        BoostedRegressor.from_arrays(**_tiny()).load_state_dict(loaded, strict=True)          # another ensemble's sizes
    for drop in sd:
        with pytest.raises(ValueError, match="lacks"):
            BoostedRegressor.from_state_dict({k: v for k, v in sd.items() if k != drop})
    for key, bad, message in (("tree_ptr", sd["tree_ptr"][:-1], "does not partition"), ("nodes", sd["nodes"].to(torch.int64), "dtype or shape"),
                              ("value", sd["value"].repeat(1, 2), "dtype or shape"), ("value", sd["value"].float(), "dtype or shape"),
                              ("meta", torch.tensor([0, 3]), "meta"), ("meta", torch.tensor([5, 10 ** 6]), "meta"),
                              ("scale", sd["scale"].float(), "dtype or shape"), ("scale", torch.zeros(3, dtype=torch.float64), "dtype or shape"),
                              ("scale", torch.tensor([float("nan"), 0.1], dtype=torch.float64), "scale"),
                              ("scale", torch.tensor([0.0, float("inf")], dtype=torch.float64), "scale")):
        with pytest.raises(ValueError, match=message):
            BoostedRegressor.from_state_dict({**sd, key: bad})


def test_truncated_is_a_prefix():
    model = module_of(CASES[0])
    with pytest.raises(ValueError, match="truncated"):
        model.truncated(0)
    with pytest.raises(ValueError, match="truncated"):
        model.truncated(13)
    short = model.truncated(5)
    end = int(model.tree_ptr[5])
    assert short.n_stages == 5 and torch.equal(short.nodes, model.nodes[:end]) and torch.equal(short.value, model.value[:end])
    assert torch.equal(short.scale, model.scale) and short.max_depth == 3
    one = BoostedRegressor.from_arrays(**_tiny()).truncated(1)
    assert one.max_depth == 1 and one.n_stages == 1


def _ok(n=8, F=3):
    return torch.zeros((n, F)), torch.zeros(n), {}


BAD_ARGUMENTS = {
    "cpu tensors": (lambda: _ok(), BlackwaterException, "GPU"),
    "x dtype": (lambda: (torch.zeros((8, 3), dtype=torch.float64), torch.zeros(8), {}), ValueError, "x must be float32"),
    "x shape": (lambda: (torch.zeros(8), torch.zeros(8), {}), ValueError, "x must be float32"),
    "y rows": (lambda: (torch.zeros((8, 3)), torch.zeros(7), {}), ValueError, "y must be"),
    "y dtype": (lambda: (torch.zeros((8, 3)), torch.zeros(8, dtype=torch.int64), {}), ValueError, "y must be"),
    "two outputs": (lambda: (torch.zeros((8, 3)), torch.zeros((8, 2)), {}), ValueError, "one model per column"),
    "no rows": (lambda: (torch.zeros((0, 3)), torch.zeros(0), {}), ValueError, "rows"),
    "too many rows": (lambda: (torch.empty((2 ** 22 + 1, 1)), torch.empty(2 ** 22 + 1), {}), ValueError, "rows"),
    "too many features": (lambda: (torch.zeros((2, ops.FOREST_MAX_FEATURES + 1)), torch.zeros(2), {}), ValueError, "features"),
    "min_samples_split": (lambda: (*_ok()[:2], dict(min_samples_split=1)), ValueError, "min_samples_split"),
    "min_samples_leaf": (lambda: (*_ok()[:2], dict(min_samples_leaf=0)), ValueError, "min_samples_leaf"),
    "max_depth none": (lambda: (*_ok()[:2], dict(max_depth=None)), ValueError, "max_depth"),
    "max_depth zero": (lambda: (*_ok()[:2], dict(max_depth=0)), ValueError, "max_depth"),
    "max_depth float": (lambda: (*_ok()[:2], dict(max_depth=3.0)), ValueError, "max_depth"),
    "learning_rate": (lambda: (*_ok()[:2], dict(learning_rate=0.0)), ValueError, "learning_rate"),
    "n_estimators": (lambda: (*_ok()[:2], dict(n_estimators=0)), ValueError, "n_estimators"),
    "subsample": (lambda: (*_ok()[:2], dict(subsample=1.5)), ValueError, "subsample"),
    "max_features": (lambda: (*_ok()[:2], dict(max_features=4)), ValueError, "max_features"),
    "masks shape": (lambda: (*_ok()[:2], dict(sample_masks=torch.ones((2, 7), dtype=torch.int32))), ValueError, "sample_masks must"),
    "masks dtype": (lambda: (*_ok()[:2], dict(sample_masks=torch.ones((2, 8), dtype=torch.int64))), ValueError, "sample_masks must"),
    "masks values": (lambda: (*_ok()[:2], dict(sample_masks=torch.tensor([[1] * 8, [2] + [1] * 7], dtype=torch.int32))), ValueError,
                     "0 and 1 only"),
    "empty bag": (lambda: (*_ok()[:2], dict(sample_masks=torch.tensor([[1] * 8, [0] * 8], dtype=torch.int32))), ValueError,
                  "stage 1 has an empty bag"),
    "eval_set": (lambda: (*_ok()[:2], dict(eval_set=(torch.zeros((4, 2)), torch.zeros(4)))), ValueError, "eval_set"),
}


@pytest.mark.parametrize("name", list(BAD_ARGUMENTS))
def test_fit_refuses_bad_arguments_before_any_launch(name):
    """Host tensors throughout: every check but the last (the device) fires before ``fit`` asks where the tensors live; non-finite
    values need the device's reduction and are covered in tests/test_gpu_boost.py."""
    make, error, message = BAD_ARGUMENTS[name]
    x, y, kwargs = make()
    with pytest.raises(error, match=message):
        BoostedRegressor.fit(x, y, **kwargs)


def test_the_bag_generator_is_the_documented_one():
    n, T, seed = 37, 5, 3
    a, b = subsample_masks(n, T, 0.5, seed), subsample_masks(n, T, 0.5, seed)
    assert a.dtype == torch.int32 and tuple(a.shape) == (T, n) and torch.equal(a, b)
    assert a.sum(dim=1).tolist() == [int(0.5 * n)] * T and set(a.unique().tolist()) == {0, 1}
    for t in range(T):
        want = np.zeros(n, np.int32)
        want[np.random.default_rng([seed, t]).permutation(n)[:max(1, int(0.5 * n))]] = 1
        assert np.array_equal(a[t].numpy(), want)
    assert not torch.equal(a, subsample_masks(n, T, 0.5, seed + 1)) and not torch.equal(a[0], a[1])
    assert subsample_masks(3, 2, 0.1, 0).sum(dim=1).tolist() == [1, 1]                     # at least one row
    assert torch.equal(subsample_masks(n, T, 1.0, seed), torch.ones((T, n), dtype=torch.int32))


def test_unmix32_inverts_the_subset_rule_s_mixer():
    import forest_subset_cases as fsc

    for x in [0, 1, 0xFFFFFFFF, 0x9e3779b9] + [int(v) for v in np.random.default_rng(0).integers(0, 1 << 32, size=200)]:
        assert fsc.mix32(bc.unmix32(x)) == x and bc.unmix32(fsc.mix32(x)) == x
    seed, t, node = 12345, 17, 6                       # stage t's key under (seed, t) is the one-tree checker's under (seed', 0)
    assert fsc.node_key(bc.unmix32(fsc.mix32(seed) ^ t), 0, node) == fsc.node_key(seed, t, node)


def test_from_sklearn_equals_from_arrays_and_names_what_it_refuses():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import GradientBoostingRegressor, RandomForestRegressor

    case = CASES[0]
    X, y = case["X"], case["y"]
    gb = GradientBoostingRegressor(random_state=0, n_estimators=12, max_depth=3, learning_rate=0.1, min_samples_split=12).fit(X, y)
    got, want = BoostedRegressor.from_sklearn(gb), module_of(case)
    for k, v in want.state_dict().items():
        assert torch.equal(got.state_dict()[k], v), k
    zero = BoostedRegressor.from_sklearn(GradientBoostingRegressor(n_estimators=2, init="zero").fit(X, y))
    assert zero.init == 0.0 and zero.n_stages == 2
    for bad, message in ((GradientBoostingRegressor(n_estimators=2, loss="huber").fit(X, y), "loss='huber'"),
                         (GradientBoostingRegressor(n_estimators=2, init=RandomForestRegressor(n_estimators=2)).fit(X, y), "init="),
                         (GradientBoostingRegressor(), "not fitted"), (RandomForestRegressor(n_estimators=2).fit(X, y), "GradientBoostingRegressor"),
                         (object(), "GradientBoostingRegressor")):
        with pytest.raises(BlackwaterException, match=message):
            BoostedRegressor.from_sklearn(bad)


def test_ops_and_module_refuse_cpu_tensors():
    model = module_of(CASES[0])
    x = torch.from_numpy(CASES[0]["X"])
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.boost_predict(x, model.nodes, model.tree_ptr, model.value, model.max_depth, model.init, model.learning_rate)
    for call in (model.predict, model.staged_predict, model.apply, model):
        with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
            call(x)
    with pytest.raises(ValueError, match="features"):
        model.predict(x[:, :4])
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.boost_fit(x, torch.zeros(160, dtype=torch.float64), torch.ones((2, 160), dtype=torch.int32), learning_rate=0.1, max_depth=3)


def test_new_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "mlqem_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in ("mlqem_boost_predict_f32", "mlqem_boost_update_f64", "mlqem_boost_update_blocks"):
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define MLQEM_ABI_VERSION 48 " in header and _lib.ABI_VERSION == 48 and lib.mlqem_abi_version() == 48   # additive


def test_entry_points_validate_before_any_launch():
    lib = _lib.load()
    p = lib.mlqem_boost_predict_f32
    assert p(None, 58, 0, 58, None, None, 100, None, 3, 0.0, 0.1, None, None, 0, None) == 0        # no rows: nothing to do
    assert p(None, 40000, 8, 40000, None, None, 100, None, 3, 0.0, 0.1, None, None, 0, None) == _lib.ERR_UNSUPPORTED
    assert p(None, 58, 8, 58, None, None, 100, None, 3, 0.0, 0.1, None, None, 0, None) == -1       # null pointers
    assert p(None, 57, 8, 58, None, None, 100, None, 3, 0.0, 0.1, None, None, 0, None) == -1       # ldx < F
    assert p(None, 58, 8, 58, None, None, 0, None, 3, 0.0, 0.1, None, None, 0, None) == -1         # no stages
    assert p(None, 58, -1, 58, None, None, 1, None, 3, 0.0, 0.1, None, None, 0, None) == -1
    assert p(None, 58, 8, 58, None, None, 1, None, -1, 0.0, 0.1, None, None, 0, None) == -1        # max_depth < 0
    assert [lib.mlqem_boost_update_blocks(n) for n in (-1, 0, 1, 256, 257, 1 << 22)] == [0, 0, 1, 1, 2, 1 << 14]
    u = lib.mlqem_boost_update_f64
    assert u(None, 58, 8, 58, None, None, None, 7, 3, 0.1, None, None, None, None, None, None) == -1     # null pointers
    assert u(None, 58, 0, 58, None, None, None, 7, 3, 0.1, None, None, None, None, None, None) == -1     # no rows
    assert u(None, 58, 8, 58, None, None, None, 0, 3, 0.1, None, None, None, None, None, None) == -1     # no nodes
    assert u(None, 57, 8, 58, None, None, None, 7, 3, 0.1, None, None, None, None, None, None) == -1     # ldx < F
    assert u(None, 58, (1 << 22) + 1, 58, None, None, None, 7, 3, 0.1, None, None, None, None, None, None) == _lib.ERR_UNSUPPORTED
