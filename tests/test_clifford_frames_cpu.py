"""Pauli-frame sampling of Clifford circuits, everything a host can check: the rule of include/mlqem_hip.h as
tests/clifford_frames_cases.py restates it against the state-vector / density-matrix oracle, the lowering, and the refusals."""
from fractions import Fraction

import numpy as np
import pytest

import clifford_cases as cc
import clifford_frames_cases as fc
import sim_cases
from blackwater import sim
from blackwater.sim import frames as fr

ALL_BASES = ("Z", "X", "Y", "mixed")


def _basis_terms(n, kind, seed):
    """One full-weight term fixes the basis of every qubit: a single group with that basis."""
    rng = np.random.default_rng([n, seed, 91])
    label = "".join(str(rng.choice(list("XYZ"))) for _ in range(n)) if kind == "mixed" else kind * n
    return [(label, 1.0)]


# ---- 1. the reference outcome is a possible outcome ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
def test_reference_outcome_has_probability_two_to_minus_rank(n):
    for seed in range(3):
        circ = cc.random_clifford_program(n, 6 * n + 4, seed, measure=True)
        for kind in ALL_BASES:
            batch = sim.compile_clifford_frames([circ], [_basis_terms(n, kind, seed)])
            assert len(batch.group_circ) == 1
            (m, rank), = fc.references(batch)
            p = fc.outcome_probabilities(circ, fc.basis_string(batch, 0))
            assert abs(p[m] - 2.0 ** -rank) <= 1e-9, (n, seed, kind, p[m], rank)
            assert int((p > 1e-9).sum()) == 2 ** rank


def test_reference_outcome_of_a_wide_ghz_state_is_all_equal():
    n = 130
    batch = sim.compile_clifford_frames([fc.ghz(n)], [[("Z" * n, 1.0)]])
    (m, rank), = fc.references(batch)
    assert rank == 1 and m in (0, (1 << n) - 1)


# ---- 2. the interpreter's ideal samples stay on the support and cover it ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 4, 6])
def test_ideal_samples_stay_on_the_support_and_cover_it(n):
    shots, covered = 4096, 0
    for seed in range(4):
        circ = cc.random_clifford_program(n, 5 * n + 3, seed + 10, measure=True)
        terms = cc.random_terms(n, 5, seed, alphabet="IXYZ")
        batch = sim.compile_clifford_frames([circ], [terms])
        out = fc.interpret(batch, shots, seed=seed)
        for g in range(len(batch.group_circ)):
            p = fc.outcome_probabilities(circ, fc.basis_string(batch, g))
            seen = set(fc.outcomes_as_integers(out["bits"][g]))
            support = set(np.flatnonzero(p > 1e-9).tolist())
            assert seen <= support, (n, seed, g)
            if out["rank"][g] <= 4:   # 2^-4 per outcome, 4 096 shots: an outcome is missed with probability 16 exp(-256)
                assert seen == support, (n, seed, g)
                covered += 1
    assert covered > 0


def test_noisy_samples_follow_the_density_matrix():
    """Depolarising and asymmetric readout noise on 4 qubits: every outcome frequency within five sigma of the oracle's probability."""
    n, shots = 4, 20000
    circ = cc.random_clifford_program(n, 14, 4, measure=True)
    noise = fc.FixedNoise(None, readout=(0.03, 0.11), seed=3)
    batch = sim.compile_clifford_frames([circ], [[("Z" * n, 1.0)]], noise)
    out = fc.interpret(batch, shots, seed=1)
    p = fc.outcome_probabilities(circ, "Z" * n, noise)
    freq = np.bincount(fc.outcomes_as_integers(out["bits"][0]), minlength=2 ** n) / shots
    assert (np.abs(freq - p) <= 5 * np.sqrt(p * (1 - p) / shots) + 1.0 / shots).all()


# ---- 3. the seeds of the grid are cleared -------------------------------------------------------------------------------------------------
def test_the_seeds_of_the_grid_are_cleared():
    """Every term of the grid (all widths, shots, noise kinds, Z-only and mixed groups) meets |estimate - exact| <= 5 sqrt((1 -
    exact^2) / shots) + 1 / shots with GRID_SEED, exact from ``clifford_cases.interpret`` (noise and readout included).
    Worst deviation recorded with GRID_SEED = 2024: 3.27 sigma."""
    worst = 0.0
    for kind, mixed in fc.GRID_COMBOS:
        exact = fc.grid_batch(kind, mixed)[4]
        for shots in fc.GRID_SHOTS:
            ok, sigma = fc.five_sigma(fc.grid_oracle(kind, mixed, shots)["term_values"], exact, shots)
            worst = max(worst, sigma)
            assert ok, (kind, mixed, shots, sigma)
    print(f"worst deviation over the grid: {worst:.2f} sigma")
    assert worst < 5.0


# ---- 4. lowering and refusals ---------------------------------------------------------------------------------------------------------------
def test_thresholds_are_exact_integers():
    circ = cc.random_clifford_program(5, 12, 1, measure=True)
    noise = fc.FixedNoise(None, readout=(0.03, 0.11), seed=5)
    batch = sim.compile_clifford_frames([circ], [[("ZZZZZ", 1.0)]], noise)
    lams = [noise.after_gate(i, op.name, tuple(op.qubits)) for i, op in enumerate(circ.ops) if op.name not in ("barrier", "measure")]
    assert 0.0 in lams and 1.0 in lams
    want = [int(Fraction(lam) * 2 ** 60) for lam in lams]
    assert batch.thresh.dtype == np.uint64 and batch.thresh[:len(want)].tolist() == want
    assert fr.depol_threshold(1.0) == 2 ** 60 and fr.depol_threshold(0.0) == 0 and fr.depol_threshold(0.1) == int(Fraction(0.1) * 2 ** 60)
    keep = batch.pool[:len(want)]
    assert (keep == 1.0 - np.asarray(lams)).all()   # beside the float64 pool, index for index
    ro = int(batch.ro_ptr[0])
    assert ro == len(want)
    table = batch.thresh[ro:ro + 10].tolist()
    assert table == [int(Fraction(0.11) * 2 ** 32), int(Fraction(0.03) * 2 ** 32)] * 5   # (p10, p01) per qubit
    assert fr.readout_threshold(1.0) == 2 ** 32
    assert len(batch.thresh) == ro + 10 + 32


def test_groups_masks_and_layout():
    widths = [129, 5, 512, 33]
    circs = [cc.random_clifford_program(n, 10, n, local=4) for n in widths]
    obs = [[("I" * (n - 2) + "XZ", 0.5), ("I" * (n - 2) + "ZZ", 0.25), ("I" * (n - 2) + "XI", -1.0), ("I" * n, 2.0)] for n in widths]
    batch = sim.compile_clifford_frames(circs, obs)
    assert batch.group_ptr.tolist() == [0, 2, 4, 6, 8] and batch.term_group.tolist() == [0, 1, 0, 0] * 4
    assert (batch.n_reg, batch.n_lds) == (4, 4) and batch.ids.tolist() == [2, 3, 6, 7, 0, 1, 4, 5]
    assert batch.gterm.tolist() == [0, 2, 3, 1, 4, 6, 7, 5, 8, 10, 11, 9, 12, 14, 15, 13]
    assert batch.ref_ptr.tolist() == [0, 5, 10, 11, 12, 28, 44, 46, 48] and batch.max_qubits == 512
    assert batch.n_rows == 2 * (129 * 11 + 5 * 3 + 512 * 33 + 33 * 5)
    assert fc.basis_string(batch, 2) == "ZZZXZ" and fc.basis_string(batch, 3) == "ZZZZZ"
    n_masks = len(batch.masks)
    support = [int(batch.masks[min(int(batch.term_mask[t]), n_masks - 1)]) for t in (4, 5, 6, 7)]
    assert support == [3, 3, 2, 0]
    empty = sim.compile_clifford_frames([], [])
    assert len(empty) == 0 and empty.group_ptr.tolist() == [0]


def test_refusals_are_by_name(monkeypatch):
    from blackwater.data.circuit import Circuit, CircuitOp
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import clifford_tfim_circuit, encode_corpus, tfim_circuit

    h = Circuit(2, 2, [CircuitOp("h", (0,)), CircuitOp("cx", (0, 1)), CircuitOp("measure", (0,), (0,)), CircuitOp("measure", (1,), (1,))])
    with pytest.raises(ValueError, match="is not a Clifford gate"):
        sim.compile_clifford_frames([Circuit(1, 0, [CircuitOp("rz", (0,), (), (0.3,))])], ["Z"])
    with pytest.raises(ValueError, match="513 qubits"):
        sim.compile_clifford_frames([Circuit(513, 0, [])], ["Z" * 513])
    with pytest.raises(ValueError, match="readout noise on qubit 0 cannot be combined"):
        sim.compile_clifford_frames([h], ["XX"], sim_cases.StepNoise(1, readout={0: (0.1, 0.2)}))

    class Relaxing(sim_cases.NoNoise):
        name, non_pauli = "relaxing", "it has thermal relaxation"

    with pytest.raises(ValueError, match="cannot run on the Clifford path"):
        sim.compile_clifford_frames([h], ["ZZ"], Relaxing())
    with pytest.raises(ValueError, match="cannot run on the Clifford path"):
        sim.DeviceEstimator(Relaxing(), method="frames", shots=10)
    assert fr.MAX_GROUPS == 4096
    monkeypatch.setattr(fr, "MAX_GROUPS", 2)   # 4 097 groups take 3^8 full-weight labels and a minute of grouping
    with pytest.raises(ValueError, match="its terms need 3 measurement groups"):
        sim.compile_clifford_frames([Circuit(1, 0, [])], [[("X", 1.0), ("Y", 1.0), ("Z", 1.0)]])
    monkeypatch.undo()
    batch = sim.compile_clifford_frames([h], ["ZZ"])
    for shots in (0, 2 ** 20 + 1, 1.5, None):
        with pytest.raises(ValueError, match="shots"):
            sim.run_clifford_frames(batch, shots, device="cpu")
    with pytest.raises(ValueError, match="run_keys must be 1 integers"):
        sim.run_clifford_frames(batch, 10, run_keys=[1, 2], device="cpu")
    with pytest.raises(ValueError, match="shots is required"):
        sim.sample_clifford_expectation_values([h], ["ZZ"])
    # the estimator: frames is chosen by name, needs shots, takes no template; "auto" never picks it
    assert sim.DeviceEstimator.METHODS == ("exact", "clifford", "auto", "trajectories") and sim.DeviceEstimator.SAMPLED_METHODS == ("frames",)
    with pytest.raises(ValueError, match=r"method='frames'\): shots=None"):
        sim.DeviceEstimator(method="frames")
    with pytest.raises(ValueError, match="method = 'stabilizer'"):
        sim.DeviceEstimator(method="stabilizer")
    est = sim.DeviceEstimator(method="frames", shots=100, seed=3)
    assert est._method == "frames"
    with pytest.raises(ValueError, match=r"method='frames'\): shots=None"):
        est.run([h], ["ZZ"], shots=None)

    template = sim.Template(1, 0, [CircuitOp("rx", (0,), (), (sim.Param(0),))])
    with pytest.raises(ValueError, match="template with free parameters"):
        est.run([template], ["Z"], [(0.1,)])
    with pytest.raises(ValueError, match="template with free parameters"):
        est.run([template], ["Z"], [(0.1,)], shots=None)
    # the refusals that pin the exact Clifford path stay
    wide, small = clifford_tfim_circuit(100, 1, 1, 1), clifford_tfim_circuit(6, 1, 1, 1, two_q="cx")
    with pytest.raises(ValueError, match="shots are not drawn on the Clifford path"):
        sim.DeviceEstimator(method="clifford", shots=100).run([wide], ["I" * 99 + "Z"])
    with pytest.raises(ValueError, match="shots are not drawn on the Clifford path"):
        sim.DeviceEstimator(method="auto", shots=100).run([wide], ["I" * 99 + "Z"])
    with pytest.raises(ValueError, match="shots are not drawn on the Clifford path"):
        encode_corpus([small], 6, simulate=sim.NoiseModel(), clifford=True, shots=10)
    with pytest.raises(ValueError):
        sim.zne_run([wide], ["I" * 99 + "Z"], sim.NoiseModel(), method="clifford", shots=10)
    # the corpus and the generator
    with pytest.raises(ValueError, match="frame_shots together with shots"):
        encode_corpus([small], 6, simulate=sim.NoiseModel(), frame_shots=10, shots=10)
    with pytest.raises(ValueError, match="frame_shots together with trajectories"):
        encode_corpus([small], 6, simulate=sim.NoiseModel(), frame_shots=10, trajectories=4)
    with pytest.raises(ValueError, match="frame_shots fills simulated labels"):
        encode_corpus([small], 6, frame_shots=10)
    with pytest.raises(ValueError, match="circuit 1 is not a Clifford circuit"):
        encode_corpus([small, tfim_circuit(6, 1, J=0.3, two_q="cx")], 6, simulate=sim.NoiseModel(), frame_shots=10)
    with pytest.raises(ValueError, match="frame_shots together with shots"):
        next(exp_value_generator(None, 6, 2, 2, max_entries=1, shots=10, frame_shots=10))
    with pytest.raises(ValueError, match="frame_shots together with trajectories"):
        next(exp_value_generator(None, 6, 2, 2, max_entries=1, trajectories=4, frame_shots=10))


def test_the_contract_is_declared_everywhere():
    import os

    from blackwater.native import _lib, ops

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mlqem_hip.h")).read()
    assert "int mlqem_clifford_sample_f64(" in header and "#define MLQEM_CLIFFORD_MAX_GROUPS 4096" in header
    assert "mlqem_clifford_sample_f64" in _lib.SIGNATURES and len(_lib.SIGNATURES["mlqem_clifford_sample_f64"][1]) == 41
    assert hasattr(_lib.load(), "mlqem_clifford_sample_f64") and callable(ops.clifford_sample)
    assert fr.MAX_GROUPS == ops.CLIFFORD_MAX_GROUPS == 4096
    assert "mlqem_clifford_sample_f64" in open(os.path.join(root, "INTEGRATION.md")).read()
    for name in ("compile_clifford_frames", "run_clifford_frames", "sample_clifford_expectation_values", "frame_counts", "FrameBatch"):
        assert name in sim.__all__ and hasattr(sim, name)
    # argument validation happens before any launch
    assert _lib.load().mlqem_clifford_sample_f64(*([1] + [None] * 3 + [0, None, 32, None, None, None, None, 1, None, 1, 0, None, 32, None,
                                                   None, None, 0, None, None, 0, None, 0, 0, 1, None, None, 1, None, None, 1, None, 0,
                                                   None, None, None, None, None])) == -1   # shots = 0
