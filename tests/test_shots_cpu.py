"""Measurement shots without a GPU: the numpy Philox against Random123's known answers, the grouping rule, the lowering
(``compile_programs(..., shots=)``), the sampling rule on the oracle of tests/shots_cases.py, and the 5-sigma condition that clears
the seeds tests/test_gpu_shots.py samples with."""
import dataclasses

import numpy as np
import pytest

import shots_cases as shc
import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.sim import program as prog


# ---- Philox ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, want):
    got = shc.philox4x32_10(np.asarray([counter], dtype=np.uint64), key)[0]
    assert tuple(int(v) for v in got) == want


def test_uniforms_pair_the_philox_words():
    """Shot 2 i takes words (0, 1) of block i, shot 2 i + 1 words (2, 3); an odd shot count stops inside the last block."""
    u5, u6 = shc.uniforms(5, 7, 3, 1), shc.uniforms(6, 7, 3, 1)
    assert np.array_equal(u5, u6[:5]) and ((0 <= u6) & (u6 < 1)).all()
    x = shc.philox4x32_10(np.asarray([[2, 1, 3, 0]], dtype=np.uint64), (7, 0))[0].astype(np.uint64)
    assert u6[4] == (float(x[0] >> np.uint64(5)) * 2.0 ** 26 + float(x[1] >> np.uint64(6))) * 2.0 ** -53
    assert u6[5] == (float(x[2] >> np.uint64(5)) * 2.0 ** 26 + float(x[3] >> np.uint64(6))) * 2.0 ** -53
    big = shc.uniforms(2, 2 ** 64 - 1, -1, 0)   # a seed and a run key that fill both words
    x = shc.philox4x32_10(np.asarray([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF]], dtype=np.uint64), (0xFFFFFFFF, 0xFFFFFFFF))[0].astype(np.uint64)
    assert big[0] == (float(x[0] >> np.uint64(5)) * 2.0 ** 26 + float(x[1] >> np.uint64(6))) * 2.0 ** -53


# ---- grouping ----------------------------------------------------------------------------------------------------------------------------
def _lowered(labels):
    return prog._lower_terms([(label, 1.0) for label in labels], len(labels[0]), "test")[0]


def _all_label_sets():
    for _, (_, observables, _, _) in shc.batches().items():
        for terms in observables:
            yield [label for label, _ in terms]
    rng = np.random.default_rng(5)
    for n in (1, 2, 4, 6):
        for _ in range(20):
            yield [sc.random_label(rng, n) for _ in range(int(rng.integers(1, 12)))]


def test_grouping_partitions_the_terms_and_agrees_with_the_oracle():
    for labels in _all_label_sets():
        tg, bases = sim.measurement_groups(_lowered(labels))
        otg, obases = shc.group_terms(labels)
        assert tg == otg and len(bases) == len(obases) == max(tg) + 1          # every term in exactly one group, none empty
        n = len(labels[0])
        for (bx, by), basis in zip(bases, obases):
            assert ["X" if bx >> q & 1 else "Y" if by >> q & 1 else "Z" for q in reversed(range(n))] == list(basis)
        for label, g in zip(labels, tg):                                         # terms of a group agree qubit-wise with its basis
            assert all(ch == "I" or ch == b for ch, b in zip(label, obases[g]))
        assert sim.measurement_groups(_lowered(labels)) == (tg, bases)           # stable under a repeat


def test_grouping_examples():
    assert shc.group_terms(["ZZI", "IZZ", "ZIZ", "III"])[0] == [0, 0, 0, 0]      # all-Z: one group, the identity in group 0
    tg, bases = sim.measurement_groups(_lowered(["XX", "YY", "ZZ", "ZI"]))
    assert tg == [0, 1, 2, 2] and bases == [(3, 0), (0, 3), (0, 0)]             # ZI joins ZZ
    assert shc.group_terms(["XX", "YY", "ZZ", "ZI"]) == ([0, 1, 2, 2], ["XX", "YY", "ZZ"])
    assert sim.measurement_groups(_lowered(["II", "XI", "IY"])) == ([0, 0, 0], [(2, 1)])   # the basis is extended term by term
    assert sim.measurement_groups([]) == ([], [(0, 0)])                          # no terms: still one all-Z group to sample


# ---- lowering --------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype and np.array_equal(x, y), f.name
        else:
            assert x == y, f.name


@pytest.mark.parametrize("name", ["vector", "density", "readout"])
def test_without_shots_the_batch_is_what_it_was(name):
    circuits, observables, noise, _ = shc.batches()[name]
    a, b = sim.compile_programs(circuits, observables, noise), sim.compile_programs(circuits, observables, noise, shots=None)
    _same(a, b)
    assert a.group_ptr is None and a.prob_ptr is None and a.term_group is None and a.shots is None and (a.circ[:, 3] == 0).all()
    m = sim.compile_programs(circuits, observables, noise, shots=100)
    for k in range(len(a)):   # with shots a program is the plain one with a tail appended; the terms and the record map are untouched
        pa = a.ops[int(a.op_ptr[k]):int(a.op_ptr[k + 1])]
        pm = m.ops[int(m.op_ptr[k]):int(m.op_ptr[k + 1])]
        assert len(pm) == len(pa) + int(m.circ[k, 3]) and np.array_equal(pa[:, :3], pm[:len(pa), :3])
        for ra, rm in zip(pa, pm):
            size = {0: 8, 1: 4, 5: 32, 6: 1, 7: 1, 8: 2}.get(int(ra[0]), 0)
            assert np.array_equal(a.params[ra[3]:ra[3] + size], m.params[rm[3]:rm[3] + size])
    assert np.array_equal(a.circ[:, :3], m.circ[:, :3]) and np.array_equal(a.terms, m.terms) and np.array_equal(a.coeff, m.coeff)
    assert np.array_equal(a.ids, m.ids) and np.array_equal(a.gate_record, m.gate_record) and np.array_equal(a.gate_noise, m.gate_noise)


@pytest.mark.parametrize("name", ["vector", "density", "readout"])
def test_the_tail_is_rotations_measure_inverse_rotations(name):
    circuits, observables, noise, _ = shc.batches()[name]
    m = sim.compile_programs(circuits, observables, noise, shots=64)
    h = np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    sdg = np.diag([1, -1j])
    assert m.shots == 64 and m.group_ptr.dtype == np.int64 and m.prob_ptr.dtype == np.int64 and m.term_group.dtype == np.int32
    assert m.group_ptr.shape == (len(m) + 1,) and m.term_group.shape == (len(m.coeff),) and m.prob_ptr.shape == (int(m.group_ptr[-1]) + 1,)
    for k, (c, terms) in enumerate(zip(circuits, observables)):
        n = c.num_qubits
        tg, bases = shc.group_terms([label for label, _ in terms])
        g0, g1 = int(m.group_ptr[k]), int(m.group_ptr[k + 1])
        assert g1 - g0 == len(bases) and m.term_group[int(m.term_ptr[k]):int(m.term_ptr[k + 1])].tolist() == tg
        assert (np.diff(m.prob_ptr[g0:g1 + 1]) == 2 ** n).all() and (m.group_circ[g0:g1] == k).all()
        tail = m.ops[int(m.op_ptr[k + 1]) - int(m.circ[k, 3]):int(m.op_ptr[k + 1])].tolist()
        at = 0
        for gl, basis in enumerate(bases):
            qs = [q for q in range(n) if basis[n - 1 - q] != "Z"]
            rot = {}
            for q in qs:                                  # rotations: noise-free U1 records, H for X and H S^dagger for Y
                kind, q0, _, po = tail[at]
                mat = (m.params[po:po + 8][0::2] + 1j * m.params[po:po + 8][1::2]).reshape(2, 2)
                assert kind == prog.OP_U1 and q0 == q and np.allclose(mat, h if basis[n - 1 - q] == "X" else h @ sdg, atol=1e-15)
                rot[q] = mat
                at += 1
            assert tail[at] == [prog.OP_MEASURE, gl, 0, g0 + gl]
            at += 1
            for q in reversed(qs):                        # and their inverses: the next group sees the circuit's own state
                kind, q0, _, po = tail[at]
                mat = (m.params[po:po + 8][0::2] + 1j * m.params[po:po + 8][1::2]).reshape(2, 2)
                assert kind == prog.OP_U1 and q0 == q and np.allclose(mat @ rot[q], np.eye(2), atol=1e-15)
                at += 1
        assert at == len(tail)
        if name == "readout":   # one group, no rotation, and norm still before the readout ops
            assert len(tail) == 1 and int(m.circ[k, 2]) == n
    units, n_wave, n_wg = m.sample_units(2)
    outcomes = np.diff(m.prob_ptr)
    n_groups = len(outcomes)
    assert sorted(units.tolist()) == list(range(2 * n_groups)) and n_wave == 2 * int((outcomes <= 256).sum()) and n_wave + n_wg == 2 * n_groups
    assert (outcomes[units[:n_wave] % n_groups] <= 256).all() and (outcomes[units[n_wave:] % n_groups] > 256).all()


def test_the_schedules_carry_the_tail():
    circuits, observables, noise, _ = shc.batches()["readout"]
    m = sim.compile_programs(circuits, observables, noise, shots=8)
    sch = sim.build_schedules(m, circuits, (1, 3), sim.LocalFoldingAmplifier(gates_to_fold=2))
    plain = sim.build_schedules(sim.compile_programs(circuits, observables, noise), circuits, (1, 3), sim.LocalFoldingAmplifier(gates_to_fold=2))
    for r in range(2 * len(m)):
        k = r % len(m)
        got = sch.sched[int(sch.sched_ptr[r]):int(sch.sched_ptr[r + 1])]
        want = plain.sched[int(plain.sched_ptr[r]):int(plain.sched_ptr[r + 1])]
        n_ops, tail = int(m.op_counts[k]), int(m.circ[k, 3])
        assert np.array_equal(got[:len(want)], want) and got[len(want):].tolist() == [j << 1 for j in range(n_ops - tail, n_ops)]


def test_refusals_by_name():
    c = Circuit(2, 2, [CircuitOp("h", (0,)), CircuitOp("measure", (0,), (0,)), CircuitOp("measure", (1,), (1,))])
    noise = sim.NoiseModel({}, {0: (0.1, 0.1), 1: (0.1, 0.1)})
    with pytest.raises(ValueError, match="readout noise"):
        sim.compile_programs([c], [[("XI", 1.0)]], noise, shots=100)
    for bad in (0, -1, 2 ** 20 + 1, 1.5, True, "100"):
        with pytest.raises(ValueError, match="shots"):
            sim.compile_programs([c], [[("ZI", 1.0)]], None, shots=bad)
        with pytest.raises(ValueError, match="shots"):
            sim.DeviceEstimator(shots=bad)
    assert sim.compile_programs([c], [[("ZI", 1.0)]], None, shots=2 ** 20).shots == 2 ** 20
    with pytest.raises(ValueError, match="seed"):
        sim.DeviceEstimator(shots=10, seed=1.5)
    assert prog.check_seed(-1, "t") == 2 ** 64 - 1 and prog.check_seed(2 ** 64 + 5, "t") == 5
    with pytest.raises(ValueError, match="shots is required"):
        sim.sample_expectation_values([c], [[("ZI", 1.0)]])


# ---- the sampling rule on the oracle -------------------------------------------------------------------------------------------------------
def test_cdf_rule_is_the_chunked_order():
    rng = np.random.default_rng(0)
    for m in (2, 4, 8, 16, 256, 2048):
        p = rng.random(m)
        p[rng.integers(0, m)] = -1e-3                      # clamped to 0
        cdf = shc.cdf_rule(p)
        q = np.where(p > 0, p, 0.0)
        length = min(m, 8)
        chunks = q.reshape(-1, length)
        inside = np.zeros_like(chunks)
        for i in range(length):                            # left to right inside a chunk
            inside[:, i] = chunks[:, i] if i == 0 else inside[:, i - 1] + chunks[:, i]
        before = np.zeros(len(chunks))
        for k in range(1, len(chunks)):                    # left to right over the chunk totals
            before[k] = before[k - 1] + inside[k - 1, -1]
        assert np.array_equal(cdf, (before[:, None] + inside).reshape(-1)) and (np.diff(cdf) >= 0).all()


def test_deterministic_states_put_every_count_on_one_outcome():
    for n in (1, 3):
        zero = Circuit(n, 0, [])
        ones = Circuit(n, 0, [CircuitOp("x", (q,)) for q in range(n)])
        plus = Circuit(n, 0, [CircuitOp("h", (q,)) for q in range(n)])
        for circuit, basis, where in ((zero, "Z" * n, 0), (ones, "Z" * n, 2 ** n - 1), (plus, "X" * n, 0)):
            p, norm = shc.basis_probabilities(circuit, basis)
            counts = shc.sample_counts(p, 257, seed=11, run_key=2, group=0)
            assert abs(norm - 1) < 1e-15 and counts[where] == 257 and counts.sum() == 257, (n, basis)


def test_a_zero_tail_is_never_drawn():
    top = 1.0 - 2.0 ** -53
    for p in ([0.25, 0.75, 0.0, 0.0], [0.1] * 10 + [0.0] * 6, [1.0, 0.0], [0.3, 0.0, 0.7, 0.0, 0.0, 0.0, 0.0, 0.0], [1 / 3] * 3 + [0.0] * 5):
        cdf = shc.cdf_rule(p)
        last = max(i for i, v in enumerate(p) if v > 0)
        assert shc.pick(cdf, np.asarray([top]))[0] == last and shc.pick(cdf, np.asarray([0.0]))[0] == min(i for i, v in enumerate(p) if v > 0)
        counts = shc.sample_counts(p, 1000, 3, 0, 0, u=np.concatenate([np.full(10, top), shc.uniforms(990, 3, 0, 0)]))
        assert counts.sum() == 1000 and all(counts[i] == 0 for i, v in enumerate(p) if v <= 0)
    assert shc.pick(shc.cdf_rule([0.0, 0.0, 0.0, 0.0]), np.asarray([0.0, top])).tolist() == [0, 0]   # nothing to draw from: outcome 0


def test_estimates_and_variances():
    counts = np.asarray([5, 1, 0, 2])
    est = shc.estimates(counts, [0, 1, 2, 3], 8)
    assert est.tolist() == [1.0, (5 - 1 + 0 - 2) / 8, (5 + 1 - 0 - 2) / 8, (5 - 1 - 0 + 2) / 8]
    value, var = shc.value_and_variance([0.5, -2.0], est[1:3])
    assert value == 0.5 * est[1] - 2.0 * est[2] and var == 0.25 * (1 - est[1] ** 2) + 4.0 * (1 - est[2] ** 2)


# ---- the condition on the seeds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vector", "density", "readout"])
def test_the_seeds_of_the_device_grid_pass_five_sigma_on_the_oracle(name):
    """|estimate - exact| <= 5 sqrt((1 - exact^2) / shots) + 1 / shots for every term, every circuit and every shot count of the
    device grid, sampled by the oracle from the oracle's probabilities with the seeds and run keys the device tests use.  A
    condition on the chosen seeds (shots_cases.seed_for): if one fails, choose another; the 5 stays."""
    entries = shc.oracle(name)
    for e in entries:
        for p in e["probs"]:
            assert abs(p.sum() - e["norm"]) <= e["prob_bound"] and p.min() >= -e["prob_bound"] and e["prob_bound"] < sc.CAP
    worst = 0.0
    for shots in shc.SHOTS:
        for k, e in enumerate(entries):
            counts, est, value, var = shc.oracle_sample(e, shots, shc.seed_for(shots), k)
            assert all(c.sum() == shots for c in counts)
            ok = shc.five_sigma_ok(est, e["exact"], shots)
            assert ok.all(), (name, shots, k, est, e["exact"])
            sigma = np.sqrt(np.clip(1 - e["exact"] ** 2, 0, None) / shots)
            worst = max(worst, float((np.abs(est - e["exact"]) / np.maximum(sigma, 1e-300))[sigma > 1e-9].max(initial=0.0)))
    print(f"{name}: worst |estimate - exact| / sigma over the grid = {worst:.2f}")
