"""The host side of the matrix-product-state simulator without a GPU: the lowering, every refusal, the interpreter of the record
format against the dense oracles, the conditions the device comparison relies on and the recorded tolerance table."""
import itertools
import math

import numpy as np
import pytest

import mps_cases as mc
import relax_cases as rc
import sim_cases as sc
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.data.synthetic import tfim_circuit
from blackwater.sim import NoiseModel, compile_mps
from blackwater.sim import mps as mps_mod

IDEAL = [c["id"] for c in mc.grid() if c["noise"] is None]
ALL = [c["id"] for c in mc.grid()]


def _ops(batch, c=0):
    return batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist()


# ---- lowering --------------------------------------------------------------------------------------------------------------------------
def test_ideal_lowering_fuses_the_gates_of_a_bond():
    n, steps = 10, 3
    batch = compile_mps([tfim_circuit(n, steps, 1.0, two_q="cx")], [mc.single_z(n)])
    ops = _ops(batch)
    # cx rz cx on a bond and the field rotations before it are one record: n - 1 bond records per step
    assert [o[0] for o in ops].count(mps_mod.OP_MPS_U2) == steps * (n - 1)
    assert all(o[2] == 0 for o in ops), "a fused record is stored over bit(lower) + 2 bit(upper)"
    assert all(o[0] in (mps_mod.OP_MPS_U1, mps_mod.OP_MPS_U2) for o in ops)
    assert batch.n_noise == [0] and batch.trajectories is None
    assert batch.letters.dtype == np.uint8 and batch.readout[:n].tolist() == [[1.0, 0.0]] * n


def test_noisy_lowering_fuses_nothing_and_keeps_the_orientation():
    circ = Circuit(3, 3, [CircuitOp("sx", (0,)), CircuitOp("cx", (0, 1)), CircuitOp("rz", (1,), (), (0.3,)), CircuitOp("cx", (2, 1)),
                          CircuitOp("id", (0,)), CircuitOp("measure", (1,), (1,))])
    noise = mc.noise_model("overrot", 11)
    batch = compile_mps([circ], [[("IZI", 1.0)]], noise, trajectories=4)
    ops = _ops(batch)
    # sx: U1 + DEPOL1; cx(0, 1): U2 + coherent U2 + DEPOL2, lower site 0, orientation 0; rz: U1 (its error is 0: no record);
    # cx(2, 1): the same on lower site 1 with orientation 1; id: no gate record, its noise record stays
    kinds = [o[0] for o in ops]
    assert kinds == [0, 6, 5, 5, 7, 0, 5, 5, 7] + ([6] if noise.after_gate(4, "id", (0,)) is not None else [])
    assert [(o[1], o[2]) for o in ops if o[0] in (5, 7)] == [(0, 0)] * 3 + [(1, 1)] * 3
    assert batch.n_noise == [kinds.count(6) + kinds.count(7)] and batch.trajectories == 4
    p01, p10 = noise.readout_of(1)
    assert batch.readout[1].tolist() == [1.0 - p01 - p10, p01 - p10] and batch.readout[0].tolist() == [1.0, 0.0]
    # the same circuit without noise: one record per bond visit
    ideal = _ops(compile_mps([circ], [[("IZI", 1.0)]]))
    assert [o[0] for o in ideal] == [5, 5] and [o[1] for o in ideal] == [0, 1]


def test_fused_records_are_the_product_of_their_gates():
    circ = mc.line_program(4, 60, seed=3)
    fused = compile_mps([circ], [mc.terms_of(4, 0)])
    res = mc.interpret(fused, 0)
    value, terms, _ = sc.simulate(circ, mc.terms_of(4, 0))
    assert len(_ops(fused)) < sum(1 for op in circ.ops if op.name != "id")
    assert np.max(np.abs(res["terms"] - terms)) <= sc.term_bound(circ) and abs(res["value"] - value) <= sc.value_bound(circ, mc.terms_of(4, 0))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _circ(*ops, n=3, measure=()):
    return Circuit(n, n, list(ops) + [CircuitOp("measure", (q,), (q,)) for q in measure])


REFUSALS = [
    (dict(circuits=[_circ(CircuitOp("cx", (0, 2)))]), "qubits 0 and 2 are not neighbours on the line; route with swaps first"),
    (dict(circuits=[Circuit(8, 0, [CircuitOp("cz", (7, 3))])], observables=[[("I" * 8, 1.0)]]),
     "qubits 7 and 3 are not neighbours on the line; route with swaps first"),
    (dict(circuits=[_circ(CircuitOp("ccx", (0, 1, 2)))]), "'ccx', which is not simulated"),
    (dict(circuits=[_circ(CircuitOp("reset", (0,)))]), "'reset', which is not simulated"),
    (dict(max_bond=0), "max_bond = 0, want an int in 1 .. 32"),
    (dict(max_bond=33), "max_bond = 33, want an int in 1 .. 32"),
    (dict(max_bond=64), "bond 64 needs theta outside LDS"),
    (dict(cutoff=1.0), "cutoff = 1.0, want a relative weight"),
    (dict(noise="depol"), "noise without trajectories"),
    (dict(trajectories=8), "trajectories without a noise model"),
    (dict(noise="depol", trajectories=0), "trajectories = 0, want an int in 1 .. 2^20"),
    (dict(noise="relax", trajectories=8), "thermal relaxation"),
    (dict(noise="readout", trajectories=8, circuits=[_circ(CircuitOp("sx", (0,)), measure=(0,))], observables=[[("IIX", 1.0)]]),
     "readout noise on qubit 0 cannot be combined with an observable that has X or Y terms (the readout channel of a trajectory"),
    (dict(circuits=[Circuit(2, 2, [CircuitOp("measure", (0,), (0,)), CircuitOp("x", (0,))])], observables=[[("II", 1.0)]]),
     "acts on qubit 0 after it was measured"),
    (dict(observables=[[("ZZ", 1.0)]]), "has 2 characters, the circuit has 3 qubits"),
    (dict(circuits=[Circuit(513, 0, [])], observables=[[("I" * 513, 1.0)]]), "513 qubits; the MPS path takes 1 .. 512"),
]


@pytest.mark.parametrize("kwargs, message", REFUSALS, ids=[m[:40] for _, m in REFUSALS])
def test_refusals_name_the_offender(kwargs, message):
    kwargs = dict(kwargs)
    name = kwargs.pop("noise", None)
    if name == "relax":
        noise = NoiseModel.from_backend(rc.lima(), readout=False, thermal_relaxation=True)
    else:
        noise = None if name is None else mc.noise_model(name, 11)
    circuits = kwargs.pop("circuits", [_circ(CircuitOp("sx", (0,)), CircuitOp("cx", (0, 1)))])
    observables = kwargs.pop("observables", [[("IIZ", 1.0)]] * len(circuits))
    with pytest.raises(ValueError) as err:
        compile_mps(circuits, observables, noise, **kwargs)
    assert message in str(err.value), str(err.value)


def test_a_coherent_error_is_accepted():
    circ = _circ(CircuitOp("cx", (1, 0)), CircuitOp("cx", (1, 2)))
    batch = compile_mps([circ], [[("ZZZ", 1.0)]], mc.noise_model("overrot", 11), trajectories=2)
    assert [o[0] for o in _ops(batch)] == [5, 5, 7, 5, 5, 7]


# ---- the interpreter against the dense oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", IDEAL)
def test_interpreter_against_the_dense_oracle(case_id):
    case = mc.case(case_id)
    batch = mc.lower(case)
    for j, (circ, obs) in enumerate(zip(case["circuits"], case["observables"])):
        circ = Circuit.from_any(circ)
        res = mc.reference(case_id)[j][0]
        value, terms, norm = sc.simulate(circ, obs)
        term_bound, value_bound = sc.term_bound(circ), sc.value_bound(circ, obs)
        assert term_bound < sc.CAP
        err_t, err_v = float(np.max(np.abs(res["terms"] - terms))), abs(res["value"] - value)
        print(f"{case_id}[{j}]: terms {err_t:.2e} value {err_v:.2e} B {res['error_bound']:.2e} bond {res['bond']} gap {res['gap']:.2e}")
        # the certificate, everywhere
        assert err_t <= 2.0 * res["error_bound"] + term_bound
        assert err_v <= 2.0 * res["error_bound"] * res["abs_coeff"] + value_bound
        assert abs(res["norm"] - norm) <= term_bound
        if math.isinf(res["gap"]):   # the bond cap dropped nothing: exact, and B stays under the floor of the cutoff
            assert err_t <= term_bound and err_v <= value_bound
            assert res["error_bound"] <= mps_mod.cutoff_floor(res["n_dec"], batch.max_bond, batch.cutoff)
            assert res["drop"] <= batch.cutoff
    if case_id.startswith("random-b32") or case_id.endswith("-b32") or case_id == "n1-n2":
        assert all(math.isinf(r[0]["gap"]) for r in mc.reference(case_id)), "meant to run without truncation"


def test_truncated_cases_truncate():
    hit = [cid for cid in IDEAL if any(not math.isinf(r[0]["gap"]) for r in mc.reference(cid))]
    assert {"random-b2", "random-b3", "random-b5", "tfim-n12-s8-b16"} <= set(hit)
    assert sum(cid.startswith("tfim-") for cid in hit) >= 13
    # the centre moves in both directions in the random circuits
    batch = mc.lower(mc.case("random-b32"))
    sites = [o[1] for o in _ops(batch, 2) if o[0] == 5]
    assert any(b > a for a, b in zip(sites, sites[1:])) and any(b < a for a, b in zip(sites, sites[1:]))


# ---- the noisy interpreter against the density-matrix oracle -----------------------------------------------------------------------------
ENUMERATED = [
    ("readout", Circuit(2, 2, [CircuitOp("sx", (0,)), CircuitOp("cx", (0, 1)), CircuitOp("rz", (1,), (), (0.4,)), CircuitOp("x", (1,)),
                               CircuitOp("measure", (0,), (0,)), CircuitOp("measure", (1,), (1,))]), "IZ"),
    ("overrot", Circuit(3, 3, [CircuitOp("sx", (2,)), CircuitOp("cx", (2, 1)), CircuitOp("rz", (1,), (), (-0.7,)), CircuitOp("ry", (0,), (), (0.8,)),
                               CircuitOp("cx", (0, 1)), CircuitOp("measure", (1,), (0,)), CircuitOp("measure", (2,), (1,))]), "IZ"),
    ("depol", Circuit(3, 0, [CircuitOp("sx", (1,)), CircuitOp("cx", (1, 2)), CircuitOp("rz", (2,), (), (1.1,)), CircuitOp("ry", (0,), (), (0.6,)),
                             CircuitOp("cx", (1, 0))]), "IXYZ"),
]


@pytest.mark.parametrize("name, circ, alphabet", ENUMERATED, ids=[e[0] for e in ENUMERATED])
def test_enumerated_trajectories_sum_to_the_density_matrix(name, circ, alphabet):
    noise = mc.noise_model(name, 11)
    obs = sc.term_set(circ.num_qubits, 5, alphabet) + mc.single_z(circ.num_qubits)
    batch = compile_mps([circ], [obs], noise, trajectories=1)
    sizes = [4 if o[0] == 6 else 16 for o in _ops(batch) if o[0] in (6, 7)]
    assert 1 <= len(sizes) <= 3 and batch.n_noise == [len(sizes)]
    terms, total = 0.0, 0.0
    for choice in itertools.product(*(range(s) for s in sizes)):
        res = mc.interpret(batch, 0, forced=choice)
        terms = terms + res["prob"] * res["terms"]
        total += res["prob"]
    value, want, _ = rc.simulate(circ, obs, noise)
    assert abs(total - 1.0) <= 1e-12
    assert np.max(np.abs(terms - want)) <= 1e-12
    assert abs(float(np.dot([c for _, c in obs], terms)) - value) <= 1e-12


# ---- the conditions of the device comparison ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ALL)
def test_conditions_hold(case_id):
    units = [r for per in mc.reference(case_id) for r in per]
    gap, cut, margin = min(r["gap"] for r in units), min(r["cut_margin"] for r in units), min(r["margin"] for r in units)
    print(f"{case_id}: gap {gap:.2e} cutoff factor {math.exp(min(cut, 700.0)):.3g} margin {margin:.2e}")
    assert gap >= mc.MIN_GAP
    assert cut >= math.log(mc.CUT_FACTOR)
    assert margin >= mc.MARGIN


@pytest.mark.parametrize("case_id", ALL + list(mc.WIDTH))
def test_recorded_differences_still_hold(case_id):
    diff = mc.measured_difference(case_id)
    print(f"{case_id}: LAPACK against numpy Jacobi {diff:.3e}, recorded {mc.TABLE[case_id]:.3e}, tolerance {mc.tolerance(case_id):.3e}")
    assert mc.TABLE[case_id] <= mc.HEADROOM[case_id] <= 5.0 * mc.TABLE[case_id], "the headroom is twice the measurement, rounded up"
    assert diff <= mc.HEADROOM[case_id]
    assert mc.tolerance(case_id) < 1e-9
    # discarded and error_bound of the two runs agree as the device comparison demands
    for ra, rb in zip(mc.reference(case_id, "lapack"), mc.reference(case_id, "jacobi")):
        for x, y in zip(ra, rb):
            fd, fb = mc.stat_floor(x)
            assert abs(x["discarded"] - y["discarded"]) <= mc.tolerance(case_id) * x["discarded"] + fd
            assert abs(x["error_bound"] - y["error_bound"]) <= mc.tolerance(case_id) * x["error_bound"] + fb
            assert x["bond"] == y["bond"] and x["n_free"] == y["n_free"]


@pytest.mark.parametrize("case_id", mc.WIDTH)
def test_width_cases_drop_nothing_but_rounding(case_id):
    """What the device tests of the width cases rely on: the bond cap never drops a column and no weight lies near the cutoff."""
    for per in mc.reference(case_id):
        assert per[0]["gap"] == math.inf and per[0]["n_free"] == per[0]["n_dec"]
        assert per[0]["cut_margin"] >= math.log(mc.CUT_FACTOR)
        assert per[0]["error_bound"] <= mc.stat_floor(per[0])[1]


def test_numpy_jacobi_orthogonalises():
    rng = np.random.default_rng(5)
    m = rng.normal(size=(12, 7)) + 1j * rng.normal(size=(12, 7))
    m[:, 3] = m[:, 1] * (0.3 - 0.2j)   # rank-deficient
    g = mc.jacobi_columns(m)
    gram = g.conj().T @ g
    norms = np.sqrt(np.abs(np.diag(gram)))
    off = np.abs(gram - np.diag(np.diag(gram))) / np.maximum(np.outer(norms, norms), 1e-300)
    assert off[np.outer(norms, norms) > 1e-20].max() <= 1e-14
    assert np.allclose(np.sort(norms)[::-1], np.linalg.svd(m, compute_uv=False), atol=1e-13)


# ---- the public surface, where it needs no device ------------------------------------------------------------------------------------------
def test_encode_corpus_and_generator_refuse_by_name():
    from blackwater import sim
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import encode_corpus, synthetic_backend

    circuits = [tfim_circuit(12, 1, 0.5, two_q="cx")]
    noise = mc.noise_model("readout", 11)
    for kwargs, message in ((dict(simulate=noise, mps_bond=8, shots=100), "mps_bond together with shots"),
                            (dict(simulate=noise, mps_bond=8, frame_shots=100), "mps_bond together with frame_shots"),
                            (dict(mps_bond=8), "mps_bond fills simulated labels, so it needs simulate="),
                            (dict(simulate=noise, mps_bond=33), "encode_corpus: max_bond = 33, want an int in 1 .. 32"),
                            (dict(simulate=noise, mps_bond=0), "encode_corpus: max_bond = 0, want an int in 1 .. 32")):
        with pytest.raises(ValueError) as err:
            encode_corpus(circuits, 12, two_q="cx", device="cpu", **kwargs)
        assert message in str(err.value), str(err.value)
    for kwargs, message in ((dict(mps_bond=8), "mps_bond without trajectories"),
                            (dict(mps_bond=8, trajectories=4, shots=10), "mps_bond together with shots"),
                            (dict(mps_bond=8, trajectories=4, frame_shots=10), "mps_bond together with frame_shots")):
        with pytest.raises(ValueError) as err:
            next(exp_value_generator(synthetic_backend(12, "cx"), 12, 3, 2, device="cpu", **kwargs))
        assert message in str(err.value), str(err.value)
    with pytest.raises(ValueError, match="method='mps'.*shots= is not supported"):
        sim.DeviceEstimator(device="cpu", method="mps", shots=16)
    with pytest.raises(ValueError, match="max_bond = 40"):
        sim.DeviceEstimator(device="cpu", method="mps", max_bond=40)
    est = sim.DeviceEstimator(device="cpu", method="mps", max_bond=16, cutoff=1e-20)
    assert (est._method, est._max_bond, est._cutoff) == ("mps", 16, 1e-20)
    assert sim.DeviceEstimator.METHODS == ("exact", "clifford", "auto", "trajectories") and sim.DeviceEstimator.WIDE_METHODS == ("mps",)
    assert sim.is_line_circuit(circuits[0]) and not sim.is_line_circuit(Circuit(3, 0, [CircuitOp("cx", (0, 2))]))
    assert (sim.MAX_BOND, sim.MAX_QUBITS_MPS) == (32, 512) and sim.MPS_BUFFER_BYTES > 0


def test_ops_refuse_cpu_tensors():
    import torch

    from blackwater.native import _lib, ops

    batch = mc.lower(mc.case("n1-n2"))
    t = batch.to("cpu")
    z = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.sim_run_mps(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], torch.zeros(3, dtype=torch.int64), t["term_circ"], t["term_off"],
                        t["letters"], t["site_ptr"], t["readout"], (0, 3), (0, 1), (0, 1), 1, 0, 32, 1e-26, 2, torch.zeros(1, dtype=torch.uint8),
                        z, z, torch.zeros((1, 3, ops.MPS_STATS), dtype=torch.float64))
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.sim_mps_finish(t["term_ptr"], t["coeff"], z, torch.zeros((1, 3), dtype=torch.float64), z)
