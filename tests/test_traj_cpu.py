"""Quantum trajectories without a GPU: the lowering of trajectory mode, its refusals, the unravelling against the Kraus density
oracle, and the margins of the seeds the device suite uses.  tests/traj_cases.py has the interpreter, the bounds and the grid."""
import dataclasses
import math

import numpy as np
import pytest

import relax_cases as rc
import sim_cases as sc
import traj_cases as tc

from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.sim import NoiseModel, compile_programs


def _small():
    c = Circuit(2, 0, [CircuitOp("h", (0,)), CircuitOp("cx", (0, 1)), CircuitOp("t", (1,))])
    return c, NoiseModel({("h", (0,)): 0.1, ("cx", (0, 1)): 0.2}, gate_relaxation={("cx", (0, 1)): ((0.1, 0.9, 0.2), (0.2, 0.8, 0.0))})


# ---- lowering --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in tc.grid() if max(c["sizes"]) <= 5], ids=lambda c: c["id"])
def test_records_are_density_modes(case):
    noise = tc.model(case["noise"])
    traj = tc.lower(case)
    dens = compile_programs(case["circuits"], case["observables"], noise)
    for name in ("op_ptr", "ops", "params", "term_ptr", "terms", "coeff", "gate_ptr", "gate_record", "gate_noise", "gate_noise_len"):
        assert np.array_equal(getattr(traj, name), getattr(dens, name)), name
    assert np.array_equal(traj.circ[:, [0, 2, 3]], dens.circ[:, [0, 2, 3]])
    assert (traj.circ[:, 1] == 2).all() and (dens.circ[:, 1] == 1).all()
    assert traj.trajectories == case["trajectories"] and dens.trajectories is None


def test_mode_variant_and_caps():
    for case in tc.grid():
        batch = tc.lower(case)
        assert (batch.circ[:, 1] == 2).all()
        assert batch.variant == ["wave" if 2 ** n <= sim.WAVE_AMPS else "workgroup" for n in case["sizes"]]
        assert list(batch.ids[:batch.n_wave]) == [j for j, n in enumerate(case["sizes"]) if n <= 8]
        assert batch.n_wave + batch.n_wg == 5
    c, noise = _small()
    wide = Circuit(11, 0, [CircuitOp("h", (10,))])
    assert compile_programs([wide], ["Z" * 11], noise, trajectories=1).variant == ["workgroup"]
    with pytest.raises(ValueError, match="12 qubits need 4096 amplitudes as a state vector"):
        compile_programs([Circuit(12, 0, [CircuitOp("h", (0,))])], ["Z" * 12], noise, trajectories=1)
    with pytest.raises(ValueError, match="6 qubits need 4096 amplitudes as a density matrix"):   # as ever without trajectories
        compile_programs([Circuit(6, 0, [CircuitOp("h", (0,))])], ["Z" * 6], noise)
    assert sim.MAX_TRAJECTORIES == 2 ** 20


def test_trajectories_none_is_todays_batch():
    c, noise = _small()
    for nm in (None, noise):
        a, b = compile_programs([c], ["XZ"], nm), compile_programs([c], ["XZ"], nm, trajectories=None)
        for f in dataclasses.fields(a):
            x, y = getattr(a, f.name), getattr(b, f.name)
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, f.name
        assert a.trajectories is None


def test_refusals():
    c, noise = _small()
    with pytest.raises(ValueError, match="trajectories without a noise model"):
        compile_programs([c], ["ZZ"], None, trajectories=8)
    with pytest.raises(ValueError, match="trajectories together with shots"):
        compile_programs([c], ["ZZ"], noise, shots=16, trajectories=8)
    for bad in (0, -1, 2 ** 20 + 1, 1.5, True, "8"):
        with pytest.raises(ValueError, match=r"trajectories = .*want an int in 1 \.\. 2\^20"):
            compile_programs([c], ["ZZ"], noise, trajectories=bad)
    measured = Circuit(2, 2, list(c.ops) + [CircuitOp("measure", (0,), (0,))])
    ro = NoiseModel({("h", (0,)): 0.1}, readout={0: (0.02, 0.03)})
    with pytest.raises(ValueError, match="readout noise on qubit 0 cannot be combined with an observable that has X or Y"):
        compile_programs([measured], ["XZ"], ro, trajectories=8)
    assert compile_programs([measured], ["ZZ"], ro, trajectories=8).circ[0, 2] == 1
    # anything density mode refuses
    with pytest.raises(ValueError, match="is 'reset', which is not simulated"):
        compile_programs([Circuit(1, 0, [CircuitOp("reset", (0,))])], ["Z"], noise, trajectories=8)
    with pytest.raises(ValueError, match="Pauli label 'Z' has 1 characters"):
        compile_programs([c], ["Z"], noise, trajectories=8)
    strict = tc.model("line-p0")
    with pytest.raises(ValueError, match="no calibration entry for cx on the qubit pair"):
        compile_programs([Circuit(3, 0, [CircuitOp("cx", (0, 2))])], ["ZZZ"], strict, trajectories=8)


def test_other_entry_points_refuse_a_trajectory_batch():
    c, noise = _small()
    batch = compile_programs([c], ["ZZ"], noise, trajectories=8)
    for call in (lambda: sim.run_batch(batch, device="cpu"), lambda: sim.sample_batch(batch, device="cpu"),
                 lambda: sim.build_schedules(batch, None, (1.0, 3.0), sim.GlobalFoldingAmplifier())):
        with pytest.raises(ValueError, match="lowered for quantum trajectories"):   # before any tensor exists
            call()
    with pytest.raises(ValueError, match="ZNE runs over quantum trajectories are not supported"):
        sim.zne_run([c], ["ZZ"], noise, method="trajectories")
    with pytest.raises(ValueError, match="lowered without trajectories"):
        sim.run_trajectories(compile_programs([c], ["ZZ"], noise), device="cpu")
    with pytest.raises(ValueError, match="trajectories is required"):
        sim.trajectory_expectation_values([c], ["ZZ"], noise)
    with pytest.raises(ValueError, match="noise is required"):
        sim.trajectory_expectation_values([c], ["ZZ"], None, trajectories=8)


def test_estimator_and_generators_refuse_by_name():
    c, noise = _small()
    assert sim.DeviceEstimator.METHODS == ("exact", "clifford", "auto", "trajectories")
    with pytest.raises(ValueError, match="noise=None"):
        sim.DeviceEstimator(None, method="trajectories")
    with pytest.raises(ValueError, match="shots= is not supported with it"):
        sim.DeviceEstimator(noise, method="trajectories", shots=100)
    with pytest.raises(ValueError, match="shots= is not supported with it"):
        sim.DeviceEstimator(noise, method="trajectories").run([c], ["ZZ"], shots=100)
    with pytest.raises(ValueError, match="trajectories = 0"):
        sim.DeviceEstimator(noise, method="trajectories", trajectories=0)
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import encode_corpus

    with pytest.raises(ValueError, match="trajectories together with shots"):
        next(exp_value_generator(tc.table(), 6, 2, 2, max_entries=1, shots=10, trajectories=4))
    with pytest.raises(ValueError, match="trajectories together with shots"):
        encode_corpus([tc.line_circuit(6, 1, measure=True)], 6, simulate=tc.model("line-p0"), shots=10, trajectories=4)
    with pytest.raises(ValueError, match="need simulate="):
        encode_corpus([tc.line_circuit(6, 1, measure=True)], 6, trajectories=4)


def test_ops_refuses_cpu_tensors():
    import torch

    from blackwater.native import _lib, ops

    c, noise = _small()
    t = compile_programs([c], ["ZZ"], noise, trajectories=4).to("cpu")
    with pytest.raises(_lib.NativeLibraryError, match="there is no CPU path"):
        ops.sim_run_trajectories(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"], 1, 0,
                                 torch.zeros(1, dtype=torch.int64), 4, 0)


# ---- the unravelling is the channel ----------------------------------------------------------------------------------------------------
def test_one_record_closed_form():
    """sum_k p_k (K_k rho K_k^+ / p_k) over the six operators of the contract equals noise1's closed form."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for g, c, p1 in [(0.3, 0.5, 0.2), (1.0, 0.0, 0.7), (0.0, 1.0, 0.4), (0.36, math.sqrt(1.0 - 0.36), 1.0), (0.2, 0.1, 0.0)] + \
            [(g, float(rng.uniform(0.0, math.sqrt(1.0 - g))), float(rng.uniform())) for g in rng.uniform(0.0, 1.0, size=20)]:
        psi = rng.normal(size=2) + 1j * rng.normal(size=2)
        psi /= np.linalg.norm(psi)
        rho = np.outer(psi, psi.conj())
        d = max(0.0, 1.0 - g - c * c)
        kraus = [(1.0 - p1, np.diag([1.0, c])), (1.0 - p1, math.sqrt(g) * np.array([[0.0, 1.0], [0.0, 0.0]])),
                 (1.0 - p1, math.sqrt(d) * np.diag([0.0, 1.0])), (p1, np.diag([c, 1.0])),
                 (p1, math.sqrt(g) * np.array([[0.0, 0.0], [1.0, 0.0]])), (p1, math.sqrt(d) * np.diag([1.0, 0.0]))]
        acc, total = np.zeros((2, 2), dtype=complex), 0.0
        for w, k in kraus:
            out = k @ rho @ k.conj().T
            p = w * float(np.trace(out).real)
            total += p
            if p > 0.0:
                acc += p * (w * out / p)
        want = rho.copy()
        rc._closed_relax(want, g, c, p1)
        worst = max(worst, float(np.abs(acc - want).max()), abs(total - 1.0))
    assert worst <= 1e-14, worst


@pytest.mark.parametrize("case,keep", tc.small_cases(6), ids=lambda v: v["id"] if isinstance(v, dict) else None)
def test_mean_is_the_channel(case, keep):
    """The interpreter's mean over 4 096 trajectories against the Kraus density oracle: within 5 standard errors of the
    interpreter's own sample (plus the rounding bound, which is what is left where the standard error is 0)."""
    noise = tc.model(case["noise"])
    ref = tc.long_reference(case["id"], 6)
    for j in keep:
        res = ref[j]
        _, want, norm = rc.simulate(case["circuits"][j], list(case["observables"][j]), noise)
        mean, se = tc.mean_and_error(res["terms"])
        slack = 5.0 * se + tc.mean_bound(tc.term_bound(res)[:, None], res["terms"])
        print(case["id"], j, "max |mean - oracle| / se", float(np.max(np.abs(mean - want) / np.maximum(se, 1e-300) * (se > 1e-12))))
        assert (np.abs(mean - want) <= slack).all(), (case["id"], j, mean - want, se)
        assert abs(norm - 1.0) < 1e-12 and np.abs(res["norm"] - 1.0).max() <= tc.norm_bound(res).max()


# ---- margins and bounds of the device suite's seeds ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tc.grid(), ids=lambda c: c["id"])
def test_margins_and_bounds(case):
    for j, res in enumerate(tc.reference(case["id"])):
        assert res["margin"].min() >= tc.MARGIN, (case["id"], j, res["margin"].min())
        assert tc.term_bound(res).max() < tc.CAP and tc.value_bound(res).max() < tc.CAP and tc.norm_bound(res).max() < tc.CAP
        assert np.abs(res["norm"] - 1.0).max() <= tc.norm_bound(res).max()


def test_margins_of_the_long_runs():
    """The device suite also runs the circuits of at most 5 qubits at T = 4 096 and compares their means."""
    for case, keep in tc.small_cases(5):
        for j, res in tc.long_reference(case["id"], 6).items():
            if j in keep:
                assert res["margin"].min() >= tc.MARGIN, (case["id"], j, res["margin"].min())
                assert tc.term_bound(res).max() < tc.CAP


def test_a_jump_of_probability_zero_is_never_drawn():
    """The first record of the corner circuit relaxes qubit 0 of |0..0>: pb = 0, so outcomes 1 and 2 have probability exactly 0 and
    every trajectory takes outcome 0 (p1 = 0): the state stays |0..0> whatever u is."""
    circ = Circuit(2, 0, [CircuitOp("id", (0,))])
    batch = compile_programs([circ], [[("IZ", 1.0), ("ZI", 1.0)]], tc.model("corners"), trajectories=256)
    res = tc.interpret(batch, 0, 256, seed=9)
    assert (res["terms"] == 1.0).all() and (res["norm"] == 1.0).all()


def test_prefix_and_key_independence():
    """A trajectory depends on (seed, run key, trajectory number, circuit) alone."""
    case = tc.grid()[6]
    batch = tc.lower(case, 64)
    a = tc.interpret(batch, 3, 64, case["seed"], run_key=7)
    b = tc.interpret(batch, 3, 27, case["seed"], run_key=7, first=37)
    assert np.array_equal(a["terms"][37:], b["terms"])
    assert not np.array_equal(a["terms"], tc.interpret(batch, 3, 64, case["seed"], run_key=8)["terms"])
