"""Thermal relaxation on the matrix-product-state path without a GPU: the lowering behind ``thermal_relaxation=True``, every
refusal, the interpreter of the NOISE1 / NOISE2 records (tests/mps_relax_cases.py) against the density-matrix oracle by full
enumeration of the outcomes, against dense vectors under forced outcomes, the per-trajectory certificate, and the conditions,
the recorded tolerances and the seeds that tests/test_gpu_mps_relax.py relies on."""
import math

import numpy as np
import pytest

import mps_cases as mc
import mps_relax_cases as mr
import relax_cases as rc
import sim_cases as sc
import traj_cases as tc
from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.data.synthetic import tfim_circuit
from blackwater.sim import NoiseModel, compile_mps, compile_programs


def _ops(batch, c=0):
    return batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist()


# ---- the lowering ------------------------------------------------------------------------------------------------------------------------
def test_one_noise_record_per_relaxed_gate_with_the_triples_of_compile_programs():
    circ = tc.corner_circuit(2)
    noise, obs = tc.model("corners"), mc.single_z(2)
    batch = compile_mps([circ], [obs], noise, 4, thermal_relaxation=True)
    dense = compile_programs([circ], [obs], noise, trajectories=4)
    want = [o for o in dense.ops[int(dense.op_ptr[0]):int(dense.op_ptr[1])].tolist() if o[0] in (rc.KIND_NOISE1, rc.KIND_NOISE2, 6, 7)]
    got = [o for o in _ops(batch) if o[0] in (6, 7, 10, 11)]
    assert [o[0] for o in got] == [o[0] for o in want] and batch.n_noise == [len(got)]
    for (kind, site, orient, po), (_, q0, q1, dpo) in zip(got, want):
        count = {6: 1, 7: 1, 10: 4, 11: 7}[kind]
        assert np.array_equal(batch.params[po:po + count], dense.params[dpo:dpo + count]), "lambda (or 0) and the checked triples"
        if kind in (7, 11):
            assert (site, orient) == (min(q0, q1), int(q0 > q1))
        else:
            assert (site, orient) == (q0, 0)
    assert {o[0] for o in got} == {10, 11}, "every keyed gate of the corners model relaxes"
    # a gate with a depolarising entry and no relaxation keeps its DEPOL record; a coherent error stays its own U2 in front
    mixed = NoiseModel(gate_lambda={("sx", (0,)): 0.1, ("cx", (0, 1)): 0.2}, gate_relaxation={("cx", (0, 1)): ((0.1, 0.9, 0.2), (0.2, 0.8, 0.0))})
    line = Circuit(2, 0, [CircuitOp("sx", (0,)), CircuitOp("cx", (0, 1))])
    plain = compile_mps([line], [obs], mixed, 2, thermal_relaxation=True)
    assert [o[0] for o in _ops(plain)] == [0, 6, 5, 11] and plain.gate_noise_len.tolist() == [1, 1]
    over = compile_mps([line], [obs], mixed.with_cx_over_rotation(0.2), 2, thermal_relaxation=True)
    assert [o[0] for o in _ops(over)] == [0, 6, 5, 5, 11] and over.gate_noise_len.tolist() == [1, 2] and over.gate_noise.tolist() == [1, 3]
    # lambda = 0 is written as 0.0 in the fused record
    only = NoiseModel(gate_relaxation={("sx", (0,)): ((0.1, 0.9, 0.2),)})
    rec = _ops(compile_mps([line], [obs], only, 2, thermal_relaxation=True))[1]
    assert rec[0] == 10 and compile_mps([line], [obs], only, 2, thermal_relaxation=True).params[rec[3]] == 0.0
    # without relaxation in the model the keyword changes nothing
    depol = mc.noise_model("depol", 11)
    a, b = compile_mps([line], [obs], depol, 2), compile_mps([line], [obs], depol, 2, thermal_relaxation=True)
    assert np.array_equal(a.ops, b.ops) and np.array_equal(a.params, b.params)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_offender():
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import encode_corpus, synthetic_backend
    from blackwater.sim import zne
    from blackwater.sim.mps import compile_mps_shots, compile_mps_templates

    circ = tc.corner_circuit(2)
    noise, obs = tc.model("corners"), mc.single_z(2)
    for lower in (compile_mps, compile_mps_shots):
        with pytest.raises(ValueError) as err:   # the default: today's text, plus the keyword and its cost
            lower([circ], [obs], noise, 4)
        text = str(err.value)
        assert "the noise model has thermal relaxation, whose jump probabilities depend on the state; the MPS path takes depolarising + " \
               "readout models (and coherent two-qubit errors) only" in text
        assert "thermal_relaxation=True" in text and "moves to every relaxed qubit" in text
    with pytest.raises(ValueError, match="thermal_relaxation = 1, want True or False"):
        compile_mps([circ], [obs], noise, 4, thermal_relaxation=1)
    with pytest.raises(ValueError, match="the noise model has thermal relaxation.*not for templates or folded runs"):
        compile_mps_templates([circ], [obs], noise, 4)
    with pytest.raises(TypeError):
        compile_mps_templates([circ], [obs], noise, 4, thermal_relaxation=True)
    # folded runs: through zne_run, and on a batch that holds a NOISE kind, lowered or built by hand
    amplifier = zne.ZNEStrategy().noise_amplifier
    batch = compile_mps([circ], [obs], noise, 4, thermal_relaxation=True)
    with pytest.raises(ValueError, match="build_mps_schedules: record 0 of the batch is a thermal-relaxation record"):
        zne.build_mps_schedules(batch, (1.0, 3.0), amplifier)
    hand = compile_mps([circ], [obs], NoiseModel(gate_lambda={("sx", (0,)): 0.1}), 4)
    schedules = zne.build_mps_schedules(hand, (1.0,), amplifier)
    at = int(np.flatnonzero(hand.ops[:, 0] == 6)[0])
    hand.ops[at, 0] = 10   # a batch built by hand
    with pytest.raises(ValueError, match=f"run_mps_folded: record {at} of the batch is a thermal-relaxation record"):
        zne.run_mps_folded(hand, schedules, device="cpu")
    with pytest.raises(ValueError, match=f"build_mps_schedules: record {at} of the batch"):
        zne.build_mps_schedules(hand, (1.0,), amplifier)
    with pytest.raises(ValueError, match="the noise model has thermal relaxation"):
        zne.zne_run([circ], [obs], noise, device="cpu", method="mps", trajectories=4)
    # the data layer and the estimator
    with pytest.raises(ValueError, match="encode_corpus: mps_relaxation without mps_bond"):
        encode_corpus([tfim_circuit(12, 1, 0.5, two_q="cx")], 12, two_q="cx", device="cpu", simulate=noise, mps_relaxation=True)
    with pytest.raises(ValueError, match="exp_value_generator: mps_relaxation without mps_bond"):
        next(exp_value_generator(synthetic_backend(12, "cx"), 12, 3, 2, device="cpu", mps_relaxation=True))
    with pytest.raises(ValueError, match="thermal_relaxation=True belongs to method='mps' and 'mps_shots'"):
        sim.DeviceEstimator(noise, "cpu", method="trajectories", thermal_relaxation=True)
    est = sim.DeviceEstimator(noise, "cpu", method="mps", trajectories=4, thermal_relaxation=True)
    assert est._relaxation is True and sim.DeviceEstimator(noise, "cpu", method="mps")._relaxation is False


# ---- the lowering on the old kinds ------------------------------------------------------------------------------------------------------
def test_a_model_without_relaxation_lowers_to_the_same_batch_under_the_keyword():
    case = mc.case("noisy-overrot-T64")
    today = mc.lower(case)
    batch = compile_mps(case["circuits"], case["observables"], mc.noise_model(case["noise"], 11), case["trajectories"], case["max_bond"],
                        thermal_relaxation=True)
    assert np.array_equal(batch.ops, today.ops) and np.array_equal(batch.params, today.params) and batch.n_noise == today.n_noise


# ---- enumeration against the density-matrix oracle -------------------------------------------------------------------------------------
def _generic():
    """Every outcome of every draw has a non-zero probability: d > 0, 0 < p1 < 1, 0 < lambda < 1."""
    return NoiseModel(gate_lambda={("sx", (0,)): 0.2, ("x", (1,)): 0.1, ("sx", (2,)): 0.3, ("cx", (1, 0)): 0.25},
                      gate_relaxation={("sx", (0,)): ((0.2, 0.7, 0.3),), ("x", (1,)): ((0.1, 0.9, 0.6),), ("sx", (2,)): ((0.3, 0.5, 0.2),),
                                       ("cx", (0, 1)): ((0.2, 0.7, 0.3), (0.15, 0.8, 0.4)), ("cx", (1, 0)): ((0.25, 0.6, 0.1), (0.1, 0.85, 0.5)),
                                       ("cx", (2, 1)): ((0.1, 0.85, 0.5), (0.25, 0.6, 0.1))}, name="generic")


def _rot(n):
    return [CircuitOp("ry", (q,), (), (0.5 + 0.3 * q,)) for q in range(n)]


# (id, model, circuit, the NOISE kinds its records must hold)
ENUMERATED = [
    # three NOISE1: the entangling cz has no entry in either model, so it is noiseless
    ("three-noise1-generic", "generic", Circuit(3, 0, _rot(3) + [CircuitOp("cz", (0, 1)), CircuitOp("sx", (0,)), CircuitOp("cz", (1, 2)),
                                                                   CircuitOp("x", (1,)), CircuitOp("rx", (2,), (), (0.4,)), CircuitOp("sx", (2,))]),
     [10, 10, 10]),
    ("three-noise1-corners", "corners", Circuit(2, 0, _rot(2) + [CircuitOp("cz", (0, 1)), CircuitOp("sx", (0,)), CircuitOp("rx", (1,), (), (0.8,)),
                                                                   CircuitOp("cz", (0, 1)), CircuitOp("x", (0,)), CircuitOp("ry", (0,), (), (0.3,)),
                                                                   CircuitOp("id", (0,))]), [10, 10, 10]),
    # one NOISE2 and one NOISE1; the cx of the generic model is the upper-first orientation with lambda != 0
    ("noise2-noise1-generic", "generic", Circuit(3, 0, _rot(3) + [CircuitOp("cz", (1, 2)), CircuitOp("cx", (1, 0)), CircuitOp("rx", (1,), (), (0.6,)),
                                                                    CircuitOp("cz", (1, 2)), CircuitOp("sx", (2,))]), [11, 10]),
    ("noise2-noise1-corners", "corners", Circuit(3, 0, _rot(3) + [CircuitOp("cz", (1, 2)), CircuitOp("cx", (0, 1)), CircuitOp("rx", (1,), (), (0.6,)),
                                                                    CircuitOp("cz", (1, 2)), CircuitOp("sx", (0,))]), [11, 10]),
    # two NOISE2 at lambda = 0, on different bonds of four qubits: the centre moves both ways between them
    ("two-noise2-generic", "generic", Circuit(4, 0, _rot(4) + [CircuitOp("cz", (2, 3)), CircuitOp("cx", (2, 1)), CircuitOp("rx", (1,), (), (0.6,)),
                                                                 CircuitOp("cz", (2, 3)), CircuitOp("cx", (0, 1))]), [11, 11]),
    ("two-noise2-corners", "corners", Circuit(2, 0, _rot(2) + [CircuitOp("cx", (1, 0)), CircuitOp("rx", (1,), (), (0.6,)), CircuitOp("cx", (1, 0))]),
     [11, 11]),
]


def _model(name):
    return _generic() if name == "generic" else tc.model(name)


@pytest.mark.parametrize("name, model, circ, kinds", ENUMERATED, ids=[e[0] for e in ENUMERATED])
def test_enumerated_paths_sum_to_the_density_matrix(name, model, circ, kinds):
    noise = _model(model)
    obs = sc.term_set(circ.num_qubits, 5) + mc.single_z(circ.num_qubits)
    batch = compile_mps([circ], [obs], noise, trajectories=1, thermal_relaxation=True)
    assert [o[0] for o in _ops(batch) if o[0] in (6, 7, 10, 11)] == kinds
    if name == "two-noise2-generic":   # lambda = 0: no depolarising draw, 6 x 6 outcomes a record (the corners cx has lambda = 0.5)
        assert all(batch.params[o[3]] == 0.0 for o in _ops(batch) if o[0] == 11)
    paths, unpruned = mr.enumerate_paths(batch, 0)
    total, terms = 0.0, 0.0
    for prob, tv, _ in paths:
        assert prob > 0.0, "an outcome of probability 0 is never taken"
        total += prob
        terms = terms + prob * tv
    value, want, _ = rc.simulate(circ, obs, noise)
    print(f"{name}: {len(paths)} paths of non-zero probability of {unpruned}, sum of probabilities - 1 = {total - 1.0:.2e}, "
          f"worst term difference {np.max(np.abs(terms - want)):.2e}")
    assert abs(total - 1.0) <= 1e-12
    assert np.max(np.abs(terms - want)) <= 1e-12
    assert abs(float(np.dot([c for _, c in obs], terms)) - value) <= 1e-12
    assert len({p[2] for p in paths}) == len(paths)


# ---- forced outcomes against dense vectors ----------------------------------------------------------------------------------------------
FORCED = [("n2-corners-T16", 0), ("n2-corners-T16", 1), ("n3-line-p03-T8", 0), ("n5-line-p03-T8", 0), ("n4-overrot-T8", 0)]


@pytest.mark.parametrize("case_id, j", FORCED)
@pytest.mark.parametrize("method", ["lapack", "jacobi"])
def test_forced_outcomes_against_a_dense_vector(case_id, j, method):
    """The outcomes a seeded run took, forced again: the same run; and its terms are those of a dense vector carried through the
    same operators (nothing is truncated at bond 32, so the dense vector stays normalised and equal to the state)."""
    case, batch = mr.case(case_id), mr.lower(case_id)
    drawn = mc.interpret(batch, j, method, 3, case["seed"])
    res = mc.interpret(batch, j, method, forced=drawn["outcomes"])
    assert res["outcomes"] == drawn["outcomes"] and np.array_equal(res["terms"], drawn["terms"])
    n = res["n"]
    psi = mr.dense_replay(n, res["operators"])
    labels = [label for label, _ in case["observables"][j]]
    assert abs(float(np.vdot(psi, psi).real) - 1.0) <= 1e-12
    assert np.max(np.abs(mr.dense_of_tensors(res["tensors"]) - psi)) <= 1e-12
    assert np.max(np.abs(mr.dense_terms(psi, labels, n) - res["terms"])) <= 1e-12
    # every alternative of the first relaxation draw that has a non-zero probability is a valid forced path too
    first = next(k for k, size in enumerate(mr._draw_sizes(batch, j)) if size == 6)
    try:
        mc.interpret(batch, j, method, forced=drawn["outcomes"][:first])
    except mr.NeedOutcome as need:
        assert abs(sum(need.probs) - 1.0) <= 1e-12 and len(need.probs) == 6
    else:
        raise AssertionError("a forced list that ends before the draws do must ask for an outcome")


# ---- the certificate ---------------------------------------------------------------------------------------------------------------------
CERTIFIED = [(4, 2), (4, 3), (5, 2), (5, 3)]   # (program seed, bond cap): B from 0.04 to 0.31 on the path of seed 1, trajectory 0


@pytest.mark.parametrize("program, bond", CERTIFIED)
def test_the_certificate_bounds_the_distance_to_the_same_operators(program, bond):
    """Six qubits under the corners model at bond 2 or 3.  B bounds the distance between the MPS and the exact vector carried
    through the SAME operators (the MPS's normalisers); that vector is not normalised, | |psi~| - 1 | <= B, so its normalised
    form -- the same forced path at bond 32 -- is within 2 B, and a Pauli term within 4 B."""
    circ, obs = mc.line_program(6, 40, seed=program), mc.terms_of(6, 6)
    noise = tc.model("corners")
    cut = compile_mps([circ], [obs], noise, 1, bond, thermal_relaxation=True)
    res = mc.interpret(cut, 0, "lapack", 0, 1)
    assert res["bond"] == bond and res["gap"] < math.inf, "the case truncates"
    big = res["error_bound"]
    psi = mr.dense_replay(6, res["operators"])
    phi = mr.dense_of_tensors(res["tensors"])
    slack = 1e-12
    assert abs(float(np.vdot(phi, phi).real) - 1.0) <= slack
    dist = float(np.linalg.norm(psi - phi))
    norm = float(np.linalg.norm(psi))
    assert dist <= big + slack
    assert abs(norm - 1.0) <= big + slack
    assert float(np.linalg.norm(psi / norm - phi)) <= 2.0 * big + slack
    full = compile_mps([circ], [obs], noise, 1, 32, thermal_relaxation=True)
    exact = mc.interpret(full, 0, "lapack", forced=res["outcomes"])
    assert exact["error_bound"] <= mc.stat_floor(exact)[1] + slack, "bond 32 cuts nothing on six qubits"
    labels = [label for label, _ in obs]
    assert np.max(np.abs(mr.dense_terms(psi, labels, 6) - exact["terms"])) <= 1e-12, "the normalisers are scalars: the same ray"
    worst = float(np.max(np.abs(exact["terms"] - res["terms"])))
    print(f"program {program} bond {bond}: B = {big:.3f}, |psi~ - mps| = {dist:.3f}, | |psi~| - 1 | = {abs(norm - 1.0):.3f}, worst term {worst:.3f}")
    assert worst <= 4.0 * big + slack
    assert abs(exact["value"] - res["value"]) <= 4.0 * big * res["abs_coeff"] + slack
    assert 4.0 * big < 2.0, "the bound says something: a Pauli term lies in [-1, 1]"


# ---- the conditions of the device comparison ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", mr.IDS)
def test_conditions_hold(case_id):
    case = mr.case(case_id)
    units = [r for method in ("lapack", "jacobi") for per in mr.reference(case_id, method) for r in per]
    gap, cut = min(r["gap"] for r in units), min(r["cut_margin"] for r in units)
    margin, prob = min(r["margin"] for r in units), min(r["min_prob"] for r in units)
    print(f"{case_id}: margin {margin:.2e} gap {gap:.2e} cutoff factor {math.exp(min(cut, 700.0)):.3g} smallest operator probability {prob:.2e} "
          f"bond {max(r['bond'] for r in units)} decompositions {max(r['n_dec'] for r in units)}")
    assert margin >= mr.MARGIN
    assert gap >= mr.MIN_GAP
    assert cut >= math.log(mr.CUT_FACTOR)
    assert prob >= mr.MIN_PROB
    assert all(r["bond"] <= case["max_bond"] for r in units)
    kinds = set(mr.lower(case_id).ops[:, 0].tolist())
    assert kinds & {10, 11}, "the case holds relaxation records"
    if case_id.startswith("n6-b3"):
        assert gap < math.inf and max(r["bond"] for r in units) == 3, "the truncating case truncates"
    if case_id == "n4-overrot-T8":
        ops = _ops(mr.lower(case_id))
        assert any(a[0] == 5 and b[0] == 5 and c[0] == 11 for a, b, c in zip(ops, ops[1:], ops[2:])), "cx, its coherent U2, then NOISE2"
    if case_id == "n2-corners-T16":
        assert {o[2] for o in _ops(mr.lower(case_id), 0) if o[0] == 11} == {0, 1}, "both cx orientations"
    if case_id in ("n3-line-p03-T8", "n5-line-p03-T8"):   # a relaxation with the centre at or below the site, and one with it above
        assert _centre_moves(mr.lower(case_id)) == {"left", "right"}


def _centre_moves(batch):
    """Which way the centre has to move for the relaxations of circuit 0 (from the records alone)."""
    centre, moves = 0, set()
    for kind, site, orient, _ in _ops(batch):
        if kind == 5:
            centre = site + 1
        elif kind in (10, 11):
            sites = [site] if kind == 10 else ([site, site + 1] if centre <= site else [site + 1, site])
            for q in sites:
                if q != centre:
                    moves.add("left" if q < centre else "right")
                centre = q
    return moves


@pytest.mark.parametrize("case_id", mr.IDS)
def test_recorded_differences_still_hold(case_id):
    diff = mr.measured_difference(case_id)
    print(f"{case_id}: LAPACK against numpy Jacobi {diff:.3e}, recorded {mr.TABLE[case_id]:.3e}, tolerance {mr.tolerance(case_id):.3e}")
    assert mr.TABLE[case_id] <= mr.HEADROOM[case_id] <= max(5.0 * mr.TABLE[case_id], 1e-15), "the headroom is twice the measurement, rounded up"
    assert diff <= mr.HEADROOM[case_id]
    assert mr.tolerance(case_id) < 1e-9
    for ra, rb in zip(mr.reference(case_id, "lapack"), mr.reference(case_id, "jacobi")):
        for x, y in zip(ra, rb):   # the certificate of the two runs agrees as the device comparison demands
            tol = mr.tolerance(case_id)
            assert abs(x["error_bound"] - y["error_bound"]) <= tol * x["error_bound"] + mc.stat_floor(x)[1]
            assert abs(x["discarded"] - y["discarded"]) <= tol * x["discarded"] + mc.stat_floor(x)[0]
            assert x["bond"] == y["bond"]


# ---- statistics and shots: the conditions of their device tests -------------------------------------------------------------------------
def test_the_interpreters_trajectories_lie_within_five_standard_errors_of_the_oracle():
    rows, want = mr.stat_reference()
    mean, err = tc.mean_and_error(rows)
    print("statistics: |mean - oracle| / standard error =", np.abs(mean - want) / err)
    assert rows.shape == (mr.STAT["trajectories"], 4) and np.all(err > 1e-4), "every term has a standard error far above rounding"
    assert np.all(np.abs(mean - want) <= mr.STAT["sigmas"] * err)
    circ, obs, batch = mr.stat_case()
    units = [mc.interpret(batch, 0, "lapack", t, mr.STAT["seed"]) for t in (0, 100, 255)]
    assert min(r["margin"] for r in units) >= mr.MARGIN and any(o[0] == 11 for o in _ops(batch))


def test_the_shots_case_keeps_its_margin():
    lap, jac = mr.shots_reference("lapack"), mr.shots_reference("jacobi")
    margin, d = mr.shots_margin()
    print(f"shots: d = {d:.2e}, margin {margin:.2e}, smallest |u - p| {lap['margin']:.2e}, smallest |u' - flip| {lap['flip_margin']:.2e}")
    assert min(lap["margin"], jac["margin"]) > margin and min(lap["flip_margin"], jac["flip_margin"]) > 1e-12
    assert all(np.array_equal(a, b) for a, b in zip(lap["bits"], jac["bits"])) and np.array_equal(lap["term_sums"], jac["term_sums"])
    _, _, batch = mr.shots_case()
    assert set(batch.mps.ops[:, 0].tolist()) & {10, 11} and batch.flip[:4].any(), "relaxation records and readout noise"
