"""Host side of ``max_features`` and the impurity importances: the per-node feature permutation of include/mlqem_hip.h restated in
Python integers (a bijection, and uniform over the subsets), the argument checks of ``fit`` (all made before a device is touched),
the binding's new entry, and ``forest_subset_cases.mdi`` against scikit-learn's ``feature_importances_`` (the fixture).  Nothing here
touches a GPU.

Uniformity: over N keys a feature is among the first m of F with probability m / F and a pair with m (m - 1) / (F (F - 1)); every
count must lie within 5 binomial standard deviations of its expectation.  For an ideal permutation the largest of the 1 653 pair
counts at F = 58 exceeds 5 sd with probability about 1e-3, and the inputs are fixed: the cap is a condition on the permutation, not a
tuning knob."""
import itertools

import numpy as np
import pytest
import torch

import forest_subset_cases as sc
from blackwater.exception import BlackwaterException
from blackwater.native import _lib
from blackwater.nn import ForestRegressor
from blackwater.nn.forest import resolve_max_features

L2, FORESTS = sc.load_fixture()


@pytest.mark.parametrize("F", [1, 2, 3, 5, 58, 170, 1000])
def test_the_permutation_is_a_bijection(F):
    for key in (0, 1, 12345, 2 ** 32 - 1):
        assert sorted(sc.perm(key, F, i) for i in range(F)) == list(range(F))


def test_the_rule_is_in_uint32():
    assert sc.mix32(0) == 0 and sc.mix32(1) == sc.mix32(2 ** 32 + 1) and 0 <= sc.mix32(2 ** 32 - 1) < 2 ** 32
    assert sc.node_key(7, 3, 5) != sc.node_key(7, 5, 3) and sc.node_key(7, 3, 5) != sc.node_key(8, 3, 5)
    assert [sc.half_bits(F) for F in (1, 2, 3, 4, 5, 16, 17, 58, 64, 65, 170, 32767)] == [1, 1, 1, 1, 2, 2, 3, 3, 3, 4, 4, 8]


@pytest.mark.parametrize("F,m", [(2, 1), (3, 1), (4, 2), (5, 2), (9, 3), (17, 5), (58, 19), (170, 56)])
def test_subsets_are_uniform(F, m):
    N = 20000
    keys = [sc.node_key(7, j % 100, j // 100) for j in range(N)]
    first = np.stack([sc.perm_many(keys, F, i) for i in range(m)], axis=1)                 # [N, m]
    assert first[:40].tolist() == [[sc.perm(key, F, i) for i in range(m)] for key in keys[:40]]   # the vectorised form is the rule
    single = np.bincount(first.reshape(-1), minlength=F).astype(np.float64)
    pair = np.zeros((F, F))
    if m >= 2 and F <= 58:
        for a, b in itertools.combinations(range(m), 2):
            np.add.at(pair, (np.minimum(first[:, a], first[:, b]), np.maximum(first[:, a], first[:, b])), 1)
    p = m / F
    worst = float(np.abs(single - N * p).max() / np.sqrt(N * p * (1 - p)))
    print(f"F {F} m {m}: inclusion counts at most {worst:.2f} sd from N m / F")
    assert worst <= 5.0
    if m >= 2 and F <= 58:
        pp = m * (m - 1) / (F * (F - 1))
        upper = np.triu_indices(F, 1)
        worst = float(np.abs(pair[upper] - N * pp).max() / np.sqrt(N * pp * (1 - pp)))
        print(f"F {F} m {m}: pair counts at most {worst:.2f} sd from their expectation over {upper[0].size} pairs")
        assert worst <= 5.0


def test_max_features_is_resolved_as_scikit_learn_does():
    got = [resolve_max_features(v, 58) for v in (None, 1.0, 58, 1, 19, 0.5, 0.01, "sqrt", "log2", np.int64(7), np.float64(0.25))]
    assert got == [58, 58, 58, 1, 19, 29, 1, 7, 5, 7, 14]
    assert resolve_max_features("log2", 1) == 1 and resolve_max_features("sqrt", 3) == 1 and resolve_max_features(0.99, 3) == 2


@pytest.mark.parametrize("bad", [0, 4, 0.0, 1.5, "third", True], ids=repr)
def test_fit_refuses_a_bad_max_features_before_it_asks_for_a_device(bad):
    x, y = torch.zeros((8, 3)), torch.zeros((8, 2))
    with pytest.raises(ValueError, match="max_features"):
        ForestRegressor.fit(x, y, max_features=bad)


def test_importances_need_no_bootstrap():
    """Host tensors: the only complaint left is the device."""
    x, y = torch.zeros((8, 3)), torch.zeros((8, 2))
    for kwargs in (dict(importances=True, bootstrap=False), dict(importances=True), dict(max_features="sqrt", importances=True)):
        with pytest.raises(BlackwaterException, match="GPU"):
            ForestRegressor.fit(x, y, **kwargs)


def test_binding_declares_the_entry():
    assert _lib.ABI_VERSION == 48                                   # additive: the version does not move
    restype, argtypes = _lib.SIGNATURES["mlqem_forest_fit_select_subset"]
    plain = _lib.SIGNATURES["mlqem_forest_fit_select"][1]
    assert restype is _lib._I and len(argtypes) == len(plain) + 3   # max_features, seed, tree_base
    lib = _lib.load()
    assert lib.mlqem_abi_version() == 48 and hasattr(lib, "mlqem_forest_fit_select_subset")
    fn = lib.mlqem_forest_fit_select_subset
    assert fn(None, 0, 1, 0, 0, None) == -1                         # a null state
    null_state = _lib.ForestFitState(n=8, F=3, K=1, Tc=1, ldx=3, min_samples_split=2, min_samples_leaf=1, max_depth=4)
    import ctypes
    assert fn(ctypes.byref(null_state), 0, 0, 0, 0, None) == -1     # max_features 0 on a state whose buffers are null: no launch


@pytest.mark.parametrize("case", FORESTS, ids=[c["name"] for c in FORESTS])
def test_mdi_equals_scikit_learn(case):
    got = sc.mdi(case, case["X"], case["counts"])
    err = float(np.abs(got - case["importances"]).max())
    print(f"{case['name']}: max |mdi - feature_importances_| = {err:.3e}")
    assert err <= 1e-12 and abs(got.sum() - 1.0) <= 1e-12


def test_fixture_holds_what_the_issue_describes():
    assert [c["name"] for c in FORESTS] == ["m19", "leaf3", "m7d4"] and L2["m19"].shape == L2["sqrt"].shape == (20,)
    for c in FORESTS:
        assert c["counts"].shape == (20, c["X"].shape[0]) and (c["counts"].sum(axis=1) == c["X"].shape[0]).all()
        assert c["tree_ptr"].size == 21 and c["value"].shape == (int(c["tree_ptr"][-1]), 4) and c["importances"].shape == (58,)
