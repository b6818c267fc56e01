"""The host side of shots from matrix-product states: the lowering, the oracles of tests/mps_shots_cases.py against each other,
the conditions under which tests/test_gpu_mps_shots.py compares the device's bits for equality, every refusal by its message and
the argument checks of the three entry points (no device is needed for any of it)."""
import math

import numpy as np
import pytest

import mps_cases as mc
import mps_shots_cases as ms
import sim_cases as sc
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.data.synthetic import tfim_circuit
from blackwater.sim import Param, Template


# ---- the lowering ------------------------------------------------------------------------------------------------------------------------
def test_lowering_groups_letters_masks_and_flip_table():
    from blackwater import sim
    from blackwater.sim import compile_mps, compile_mps_shots, measurement_groups
    from blackwater.sim.program import _lower_terms

    circ = Circuit(3, 3, [CircuitOp("h", (0,)), CircuitOp("cx", (0, 1)), CircuitOp("ry", (2,), (), (0.3,))])
    obs = [("IIZ", 1.0), ("ZZI", 0.5), ("IXX", 0.25), ("YIX", -1.0), ("ZIZ", 2.0), ("IYI", 0.5)]
    batch = compile_mps_shots([circ, circ], [obs, [("ZZZ", 1.0)]], max_bond=4)
    base = compile_mps([circ, circ], [obs, [("ZZZ", 1.0)]], max_bond=4)
    for name in ("n_qubits", "op_ptr", "ops", "params", "term_ptr", "coeff", "letters", "site_ptr", "readout"):
        assert np.array_equal(getattr(batch.mps, name), getattr(base, name)), name
    rows, _, _ = _lower_terms(obs, 3, "circuit 0")
    groups_of, bases = measurement_groups(rows)
    assert batch.group_ptr.tolist() == [0, len(bases), len(bases) + 1] and batch.max_groups == len(bases) >= 3
    assert batch.term_group.tolist() == groups_of + [0]
    assert batch.group_circ.tolist() == [0] * len(bases) + [1]
    for g, (gx, gy) in enumerate(bases):
        letters = batch.basis[int(batch.group_off[g]):int(batch.group_off[g]) + 3].tolist()
        assert letters == [1 if gx >> q & 1 else 2 if gy >> q & 1 else 3 for q in range(3)]
        members = batch.gterm[int(batch.gterm_ptr[g]):int(batch.gterm_ptr[g + 1])].tolist()
        assert members == [t for t, tg in enumerate(groups_of) if tg == g]
        for t in members:   # the group's basis agrees with the term wherever the term acts
            label = obs[t][0][::-1]
            assert all(ch == "I" or "IXYZ".index(ch) == letters[q] for q, ch in enumerate(label))
    for t, (label, _) in enumerate(obs):
        assert int(batch.masks[int(batch.term_mask[t])]) == sum(1 << q for q, ch in enumerate(reversed(label)) if ch != "I")
    assert batch.ref_ptr.tolist() == list(range(len(bases) + 2)) and not batch.flip.any()
    # 33 qubits: two words a shot, masks of two words
    wide = ms.lower("tfim-n33-s2-b4")
    assert wide.ref_ptr[1] == 2 and int(wide.masks[int(wide.term_mask[32]) + 1]) == 1 and int(wide.masks[int(wide.term_mask[32])]) == 0
    # the flip table: (P(read 1 | 0), P(read 0 | 1)) = (p10, p01) of the measured qubits, nothing elsewhere
    measured = Circuit(3, 2, circ.ops + [CircuitOp("measure", (0,), (0,)), CircuitOp("measure", (2,), (1,))])
    noise = sim.NoiseModel(readout={0: (0.02, 0.07), 1: (0.5, 0.5), 2: (0.03, 0.01)})   # {qubit: (p01, p10)}
    noisy = compile_mps_shots([measured], [[("ZIZ", 1.0)]], noise, trajectories=2, max_bond=4)
    assert noisy.flip[:3].tolist() == [[0.07, 0.02], [0.0, 0.0], [0.01, 0.03]]
    assert np.allclose(noisy.mps.readout[:3], [[1 - 0.09, 0.02 - 0.07], [1.0, 0.0], [1 - 0.04, 0.03 - 0.01]])
    for q in (0, 2):   # the mean of the reported Z of a definite bit: a z + b
        a, b = noisy.mps.readout[q]
        assert math.isclose(1 - 2 * noisy.flip[q, 0], a + b) and math.isclose(-(1 - 2 * noisy.flip[q, 1]), -a + b)


# ---- the conditions of the device comparison ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ms.IDS)
def test_conditions_hold_and_recorded_differences_still_hold(case_id):
    c = ms.case(case_id)
    d = ms.measured_d(case_id)
    lap, jac = ms.reference(case_id, "lapack"), ms.reference(case_id, "jacobi")
    margin = min(r["margin"] for r in lap + jac)
    flip_margin = min(r["flip_margin"] for r in lap + jac)
    draws = sum(p.size for r in lap for p in r["probs"])
    print(f"{case_id}: d {d:.2e} (recorded {ms.D_MEASURED[case_id]:.2e}), margin {ms.margin(case_id):.2e}, closest draw {margin:.2e}, "
          f"closest flip {flip_margin:.2e}, {draws} draws")
    # the recorded d within a factor two (a d of one or two ulps is a sample of rounding: floored at 4 u); the factor enters no tolerance
    assert d <= 2.0 * max(ms.D_MEASURED[case_id], 4.0 * sc.U)
    assert ms.margin(case_id) == max(1e-12, 16 * ms.D_MEASURED[case_id]) < 1e-11
    assert margin > ms.margin(case_id) and flip_margin > 1e-12
    for x, y in zip(lap, jac):
        assert all(np.array_equal(a, b) for a, b in zip(x["bits"], y["bits"]))
        assert np.array_equal(x["term_sums"], y["term_sums"]) and x["value"] == y["value"] and x["variance"] == y["variance"]
        assert x["bond"] == y["bond"]
    assert all(r["bits"][0].shape == (c["shots"], (circ.num_qubits + 31) // 32) for r, circ in zip(lap, c["circuits"]))


@pytest.mark.parametrize("case_id", [i for i in ms.IDS if ms.case(i)["dense"]])
def test_the_dense_sampler_draws_the_same_bits(case_id):
    """Oracle (b) against oracle (a), and the five-sigma bound of the device tests on the interpreter's bits."""
    c, batch = ms.case(case_id), ms.lower(case_id)
    ref = ms.reference(case_id)
    for k, circ in enumerate(c["circuits"]):
        n, g0 = circ.num_qubits, int(batch.group_ptr[k])
        for g in range(g0, int(batch.group_ptr[k + 1])):
            letters = batch.basis[int(batch.group_off[g]):int(batch.group_off[g]) + n]
            assert np.array_equal(ms.dense_shots(circ, letters, g - g0, c["shots"], c["seed"], k), ref[k]["reported"][g - g0]), (k, g)
    for r, exact in zip(ref, ms.exact_terms(case_id)):
        assert ms.five_sigma(r["term_values"], exact, c["shots"]).all()


def test_the_width_case_within_five_sigma_of_its_exact_values():
    """The 100-qubit Clifford case drops nothing but rounding (tests/test_mps_cpu.py), so its interpreter's term values are exact."""
    for r in ms.reference("width-clifford-n100-s3-b8"):
        assert ms.five_sigma(r["term_values"], r["mps_terms"], 256).all()


def test_reported_z_under_readout_noise_on_the_host():
    """The interpreter's reported bits at one trajectory (independent shots of one noise realisation): every term estimate, with the
    readout flips in the bits, within five sigma of the trajectory's value with a Z + b in the operators."""
    case_id = "noisy-readout-T1"
    c, batch = ms.case(case_id), ms.lower(case_id)
    for k, r in enumerate(ms.reference(case_id)):
        want = mc.interpret(batch.mps, k, "lapack", 0, c["seed"])["terms"]
        assert ms.five_sigma(r["term_values"], want, c["shots"]).all(), k


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    from blackwater import sim
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import encode_corpus, synthetic_backend

    line = tfim_circuit(6, 1, 0.5, two_q="cx")
    z = mc.single_z(6)
    measured = Circuit(6, 1, [op for op in line.ops if op.name != "measure"] + [CircuitOp("measure", (0,), (0,))])
    readout, depol = mc.noise_model("readout", 11), mc.noise_model("depol", 11)
    relax = sim.NoiseModel(gate_relaxation={("cx", (0, 1)): ((0.1, 0.9, 0.0), (0.1, 0.9, 0.0))})
    for args, message in (
            (([measured], [[("IIIIIX", 1.0)]], readout, 4), "readout noise on qubit 0 cannot be combined with an observable that has X or Y"),
            (([line], [z], relax, 4), "the noise model has thermal relaxation"),
            (([Circuit(3, 0, [CircuitOp("cx", (0, 2))])], [mc.single_z(3)], None, None), "are not neighbours on the line"),
            (([line], [z], depol, None), "compile_mps: noise without trajectories"),
            (([line], [z], None, 4), "compile_mps: trajectories without a noise model")):
        with pytest.raises(ValueError) as err:
            sim.compile_mps_shots(*args)
        assert message in str(err.value), str(err.value)
    with pytest.raises(ValueError, match="max_bond = 33"):
        sim.compile_mps_shots([line], [z], max_bond=33)
    batch = sim.compile_mps_shots([line], [z], depol, 8)
    with pytest.raises(ValueError, match="run_mps_shots: trajectories = 8 exceed shots = 7"):
        sim.run_mps_shots(batch, 7, device="cpu")
    for shots in (0, 2 ** 20 + 1, 1.5, True):
        with pytest.raises(ValueError, match="run_mps_shots: shots = "):
            sim.run_mps_shots(batch, shots, device="cpu")
    with pytest.raises(ValueError, match="sample_mps_expectation_values: shots is required"):
        sim.sample_mps_expectation_values([line], [z], device="cpu")
    with pytest.raises(ValueError, match="mps_counts: the result has no bits"):
        sim.mps_counts(sim.MpsShotsResult(*[None] * 10), 0)
    # the estimator
    with pytest.raises(ValueError, match=r"method='mps_shots'\): shots=None"):
        sim.DeviceEstimator(device="cpu", method="mps_shots")
    with pytest.raises(ValueError, match=r"method='mps_shots'\): shots=None"):
        sim.DeviceEstimator(device="cpu", method="mps_shots", shots=10).run([line], [z], shots=None)
    template = Template(1, 0, [CircuitOp("ry", (0,), (), (Param(0),))])
    with pytest.raises(ValueError, match="template with free parameters"):
        sim.DeviceEstimator(device="cpu", method="mps_shots", shots=10).run([template], [[("Z", 1.0)]], [[0.1]])
    with pytest.raises(ValueError, match="method='mps'.*shots= is not supported"):
        sim.DeviceEstimator(device="cpu", method="mps", shots=16)
    assert sim.DeviceEstimator.METHODS == ("exact", "clifford", "auto", "trajectories")
    assert sim.DeviceEstimator.SAMPLED_METHODS == ("frames",) and sim.DeviceEstimator.WIDE_METHODS == ("mps",)
    assert sim.DeviceEstimator.WIDE_SAMPLED_METHODS == ("mps_shots",)
    est = sim.DeviceEstimator(depol, "cpu", method="mps_shots", shots=64, trajectories=16, max_bond=8)
    assert (est._method, est._shots, est._trajectories, est._max_bond) == ("mps_shots", 64, 16, 8)
    # "auto" never picks it: a wide circuit that is no Clifford circuit is still refused
    with pytest.raises(ValueError, match="is not a Clifford circuit"):
        sim.DeviceEstimator(device="cpu", method="auto").run([tfim_circuit(14, 1, 0.5, two_q="cx")], [mc.single_z(14)])
    # data generation
    circuits = [tfim_circuit(12, 1, 0.5, two_q="cx")]
    for kwargs, message in ((dict(simulate=readout, mps_shots=100), "mps_shots without mps_bond"),
                            (dict(simulate=readout, mps_bond=8, trajectories=4, mps_shots=100, shots=10), "mps_shots together with shots"),
                            (dict(simulate=readout, mps_bond=8, mps_shots=100, frame_shots=10), "mps_shots together with frame_shots"),
                            (dict(simulate=readout, mps_bond=8, mps_shots=100), "mps_shots without trajectories"),
                            (dict(simulate=readout, mps_bond=8, shots=100), "mps_bond together with shots (no shots are drawn from a "
                                                                           "matrix-product state: its noisy values are means over trajectories=)"),
                            (dict(simulate=readout, mps_bond=8, frame_shots=100), "mps_bond together with frame_shots (no shots are drawn")):
        with pytest.raises(ValueError) as err:
            encode_corpus(circuits, 12, two_q="cx", device="cpu", **kwargs)
        assert message in str(err.value), str(err.value)
    for kwargs, message in ((dict(mps_shots=100, trajectories=4), "mps_shots without mps_bond"),
                            (dict(mps_bond=8, trajectories=4, mps_shots=100, shots=10), "mps_shots together with shots"),
                            (dict(mps_bond=8, trajectories=4, mps_shots=100, frame_shots=10), "mps_shots together with frame_shots"),
                            (dict(mps_bond=8, mps_shots=100), "mps_bond without trajectories"),
                            (dict(mps_bond=8, trajectories=4, shots=10), "mps_bond together with shots (no shots are drawn")):
        with pytest.raises(ValueError) as err:
            next(exp_value_generator(synthetic_backend(12, "cx"), 12, 3, 2, device="cpu", **kwargs))
        assert message in str(err.value), str(err.value)
    for name in ("MpsShotsBatch", "MpsShotsResult", "compile_mps_shots", "run_mps_shots", "sample_mps_expectation_values", "mps_counts"):
        assert name in sim.__all__ and hasattr(sim, name)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_argument_checks():
    import ctypes

    from blackwater.native import _lib, ops

    lib = _lib.load()
    assert _lib.ABI_VERSION == 48 and lib.mlqem_abi_version() == 48
    for name in ("mlqem_mps_sample_workspace_bytes", "mlqem_mps_sample_f64", "mlqem_mps_sample_finish_f64"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.mlqem_mps_sample_workspace_bytes(100, 32, 3) == 3 * 100 * 2 * 32 * 32 * 16
    assert lib.mlqem_mps_sample_workspace_bytes(513, 32, 1) == 0 and lib.mlqem_mps_sample_workspace_bytes(10, 33, 1) == 0
    assert (ops.MPS_SHOT_BLOCK, ops.MPS_MAX_GROUPS) == (16, 4096)
    OK, BAD, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4
    assert lib.mlqem_error_string(WORKSPACE).decode().startswith("workspace")
    assert lib.mlqem_error_string(UNSUPPORTED).decode() and lib.mlqem_error_string(BAD).decode()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf) // 16 * 16 + 16   # a 16-byte aligned address that is never read: every call below returns before a launch

    def sample(**over):
        a = dict(n_circuits=1, n_qubits=p, circ_first=0, circ_count=1, traj_first=0, traj_count=1, trajectories=1, max_bond=4, max_qubits=3,
                 workspace=p, workspace_bytes=1 << 30, sample_workspace=p, sample_workspace_bytes=1 << 30, group_first=0, group_count=1,
                 n_groups=1, max_groups=1, group_ptr=p, group_circ=p, group_off=p, basis=p, n_basis=35, site_ptr=p, flip=p, n_sites=4,
                 ref_ptr=p, gterm_ptr=p, gterm=p, term_first=0, term_count=1, n_terms=1, term_mask=p, masks=p, n_masks=33, run_keys=p,
                 shots=100, seed=0, term_sums=p, bits=None, n_bits=0, stream=None)
        assert set(over) <= set(a), over
        a.update(over)
        return lib.mlqem_mps_sample_f64(*a.values())

    assert sample(n_circuits=0) == OK
    for over in (dict(shots=0), dict(shots=2 ** 20 + 1), dict(group_count=-1), dict(n_terms=-1), dict(term_count=2), dict(max_bond=33),
                 dict(traj_count=2), dict(n_qubits=None), dict(flip=None), dict(term_sums=None), dict(workspace=p + 8),
                 dict(sample_workspace=p + 4), dict(run_keys=p + 4), dict(n_bits=10), dict(n_bits=-1), dict(max_groups=0)):
        assert sample(**over) == BAD, over
    for over in (dict(max_groups=4097), dict(n_groups=2 ** 31, group_count=1), dict(n_terms=2 ** 31),
                 dict(trajectories=2 ** 20, traj_count=2 ** 20, group_count=2 ** 12, n_groups=2 ** 12, workspace_bytes=0)):
        assert sample(**over) == UNSUPPORTED, over
    assert sample(workspace_bytes=16) == WORKSPACE and sample(sample_workspace_bytes=16) == WORKSPACE
    assert sample(sample_workspace_bytes=lib.mlqem_mps_sample_workspace_bytes(3, 4, 1) - 1) == WORKSPACE

    def finish(**over):
        a = dict(n_circuits=1, n_terms=1, shots=10, term_ptr=p, coeff=p, term_sums=p, term_values=p, values=p, variance=p, stream=None)
        a.update(over)
        return lib.mlqem_mps_sample_finish_f64(*a.values())

    assert finish(n_circuits=0) == OK
    for over in (dict(shots=0), dict(shots=2 ** 20 + 1), dict(n_circuits=-1), dict(n_terms=-1), dict(term_ptr=None), dict(values=None),
                 dict(coeff=None), dict(term_sums=None)):
        assert finish(**over) == BAD, over
    assert finish(n_circuits=2 ** 31) == UNSUPPORTED and finish(n_terms=2 ** 31) == UNSUPPORTED


def test_ops_refuse_cpu_tensors():
    import torch

    from blackwater.native import _lib, ops

    batch = ms.lower("n1-n2")
    t = batch.to("cpu")
    ws = torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.mps_run(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], torch.zeros(3, dtype=torch.int64), (0, 3), (0, 1), 1, 0, 32, 1e-26, 2,
                    ws, None)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.mps_sample(t["n_qubits"], (0, 3), (0, 1), 1, 32, 2, ws, ws, (0, len(batch.group_circ)), batch.max_groups, t["group_ptr"],
                       t["group_circ"], t["group_off"], t["basis"], t["site_ptr"], t["flip"], t["ref_ptr"], t["gterm_ptr"], t["gterm"],
                       (0, len(batch.gterm)), t["term_mask"], t["masks"], torch.zeros(3, dtype=torch.int64), 10, 0,
                       torch.zeros(len(batch.gterm), dtype=torch.int32))
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.mps_sample_finish(t["term_ptr"], t["coeff"], torch.zeros(len(batch.gterm), dtype=torch.int32), 10)
