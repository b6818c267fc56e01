"""Host side of the batched simulator, no GPU: the numpy oracle of tests/sim_cases.py against hand-worked values and against the
reference's stored labels, ``compile_programs`` (refusals, op counts, variants, the lowered program interpreted record by record
against the oracle), the noise model, the generator with the oracle in the simulator's place, and ``encode_corpus``' default."""
import math

import numpy as np
import pytest

import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp, circuit_to_qasm
from blackwater.data.synthetic import encode_corpus, random_circuit, synthetic_backend


def circ(n, *ops):
    return Circuit(n, 0, [CircuitOp(name, tuple(q), (), tuple(p)) for name, q, p in ops])


def ev(circuit, label, noise=None):
    return sc.simulate(circuit, [(label, 1.0)], noise)[0]


# ---- the oracle against hand-worked values -------------------------------------------------------------------------------------------
def test_oracle_hand_worked_values():
    assert ev(circ(1), "Z") == 1.0
    assert ev(circ(1, ("x", [0], [])), "Z") == -1.0
    assert abs(ev(circ(1, ("h", [0], [])), "X") - 1.0) < 1e-15
    bell = circ(2, ("h", [0], []), ("cx", [0, 1], []))
    assert abs(ev(bell, "ZZ") - 1.0) < 1e-15 and abs(ev(bell, "XX") - 1.0) < 1e-15 and abs(ev(bell, "YY") + 1.0) < 1e-15
    sxsx = sc.gate_matrix("sx") @ sc.gate_matrix("sx")
    assert np.allclose(sxsx / sxsx[0, 1], sc.X, atol=1e-15)
    r = math.sqrt(0.5)
    ecr = r * np.array([[0, 1, 0, 1j], [1, 0, -1j, 0], [0, 1j, 0, 1], [-1j, 0, 1, 0]])
    assert np.allclose(sc.gate_matrix("ecr"), ecr, atol=1e-16)
    # qubit order: x on qubit 1 of 2 flips the LEFT character's qubit
    assert ev(circ(2, ("x", [1], [])), "ZI") == -1.0 and ev(circ(2, ("x", [1], [])), "IZ") == 1.0


def test_oracle_depolarising_and_readout():
    class Full:
        def after_gate(self, index, name, qubits):
            return 1.0 if index == 1 else None

        def readout_of(self, qubit):
            return None

    bell = circ(2, ("h", [0], []), ("cx", [0, 1], []), ("id", [1], []))
    # lambda = 1 after the cx (two-qubit): the maximally mixed pair; on one qubit of the pair (the id): also maximally mixed
    for label in ("ZZ", "XX", "YY", "ZI", "IX"):
        assert abs(ev(bell, label, Full())) < 1e-15

    class OneQubit(Full):
        def after_gate(self, index, name, qubits):
            return 1.0 if index == 2 else None

    for label in ("ZZ", "XX", "YY", "ZI", "IZ"):
        assert abs(ev(bell, label, OneQubit())) < 1e-15
    assert abs(ev(bell, "II", OneQubit()) - 1.0) < 1e-15

    class Readout(sc.NoNoise):
        def readout_of(self, qubit):
            return (0.03, 0.08)

    c = Circuit(1, 1, [CircuitOp("ry", (0,), (), (0.7,)), CircuitOp("measure", (0,), (0,))])
    z = ev(c, "Z")
    assert abs(ev(c, "Z", Readout()) - ((1 - 0.03 - 0.08) * z + (0.03 - 0.08))) < 1e-15


# ---- the reference anchor ------------------------------------------------------------------------------------------------------------
def test_reference_labels_within_four_sigma_of_the_exact_values():
    """All 900 golden circuits: the stored 10 000-shot ``ideal`` labels against v = -<Z> of the qubit measured into classical bit
    3 - k (column k), sigma = max(sqrt((1 - v^2) / 1e4), 1e-3): every one of the 3 600 within 4 sigma.  <Z> comes from the lowered
    program of ``compile_programs`` interpreted on the host, and must equal the oracle's within the derived bound."""
    texts, ideal, _ = sc.golden_circuits()
    circuits = [Circuit.from_any(t) for t in texts]
    observables = [sim.measured_z(c) for c in circuits]
    batch = sim.compile_programs(texts, observables)
    assert len(batch) == 900 and batch.n_wave == 900 and batch.n_wg == 0
    oracle = np.asarray([sc.simulate(c, o.to_list())[1] for c, o in zip(circuits, observables)])
    lowered = np.asarray([sc.interpret(batch, k)[1] for k in range(900)])
    bounds = np.asarray([sc.term_bound(c) for c in circuits])
    assert bounds.max() < sc.CAP and (np.abs(lowered - oracle).max(axis=1) <= bounds).all()
    for got in (oracle, lowered):
        sig = sc.anchor_sigmas(got, ideal)
        assert sig.shape == (900, 4) and sig.max() <= 4.0
    print(f"anchor: max {sc.anchor_sigmas(oracle, ideal).max():.3f} sigma over 3 600 values")


# ---- compile_programs ----------------------------------------------------------------------------------------------------------------
REFUSALS = [
    ("gate 'ccx'", lambda: sim.compile_programs([circ(3, ("ccx", [0, 1, 2], []))], ["III"]), "ccx"),
    ("reset", lambda: sim.compile_programs(["OPENQASM 2.0;\nqreg q[1];\nreset q[0];\n"], ["Z"]), "reset"),
    ("opaque custom gate", lambda: sim.compile_programs(["OPENQASM 2.0;\nqreg q[1];\ngate foo a { x a; }\nfoo q[0];\n"], ["Z"]), "foo"),
    ("after measure", lambda: sim.compile_programs([Circuit(1, 1, [CircuitOp("measure", (0,), (0,)), CircuitOp("x", (0,))])], ["Z"]),
     "after it was measured"),
    ("qubit out of range", lambda: sim.compile_programs([circ(2, ("x", [2], []))], ["ZZ"]), "qubit 2"),
    ("same qubit twice", lambda: sim.compile_programs([circ(2, ("cx", [1, 1], []))], ["ZZ"]), "qubit 1 twice"),
    ("non-finite angle", lambda: sim.compile_programs([circ(1, ("rz", [0], [float("nan")]))], ["Z"]), "non-finite"),
    ("label length", lambda: sim.compile_programs([circ(2)], ["ZZZ"]), "'ZZZ'"),
    ("label alphabet", lambda: sim.compile_programs([circ(2)], ["ZQ"]), "'Q'"),
    ("complex coefficient", lambda: sim.compile_programs([circ(1)], [[("Z", 1j)]]), "1j"),
    ("vector cap", lambda: sim.compile_programs([circ(12)], ["I" * 12]), "2048"),
    ("density cap", lambda: sim.compile_programs([circ(6)], ["I" * 6], sim.NoiseModel()), "2048"),
    ("readout with X", lambda: sim.compile_programs([Circuit(1, 1, [CircuitOp("measure", (0,), (0,))])], ["X"],
                                                     sim.NoiseModel(readout={0: (0.1, 0.1)})), "X or Y"),
]


@pytest.mark.parametrize("what,call,needle", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_compile_programs_refuses_by_name(what, call, needle, monkeypatch):
    from blackwater.native import _lib

    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a refusal must come before any device call"))
    with pytest.raises(ValueError, match=needle.replace("(", r"\(")):
        call()


def test_compile_programs_counts_variants_and_text():
    c = Circuit(3, 3, [CircuitOp("h", (0,)), CircuitOp("id", (1,)), CircuitOp("barrier", (0, 1, 2)), CircuitOp("cx", (0, 2)),
                       CircuitOp("rz", (2,), (), (0.3,)), CircuitOp("ecr", (1, 2)), CircuitOp("measure", (2,), (0,)),
                       CircuitOp("measure", (0,), (2,))])
    batch = sim.compile_programs([c, c, circ(9), circ(8), circ(5)], ["IIZ", "ZII", "I" * 9, "I" * 8, "I" * 5])
    assert batch.op_counts.tolist() == [4, 4, 0, 0, 0]   # id and barrier lower to nothing, measure to a map
    assert batch.ops[:4, 0].tolist() == [sim.program.OP_U1, sim.program.OP_CX, sim.program.OP_DIAG1, sim.program.OP_U2]
    assert batch.variant == ["wave", "wave", "workgroup", "wave", "wave"] and batch.ids.tolist() == [0, 1, 3, 4, 2]
    assert (batch.n_wave, batch.n_wg) == (4, 1) and batch.measured[0] == {0: 2, 2: 0}
    assert batch.params.shape[0] == 2 * (8 + 4 + 32) + 32 and batch.circ[0].tolist() == [3, 0, 0, 0]
    dens = sim.compile_programs([c, circ(5), circ(4)], ["IIZ", "I" * 5, "I" * 4], sim.NoiseModel())
    assert dens.variant == ["wave", "workgroup", "wave"] and dens.circ[:, 1].tolist() == [1, 1, 1]
    assert sim.measured_z(c).to_list() == [("ZII", 1.0), ("IIZ", 1.0)]
    # the lowered program of a QASM text equals that of its Circuit
    rc = random_circuit(4, 6, 3)
    a, b = sim.compile_programs([rc], ["ZIII"]), sim.compile_programs([circuit_to_qasm(rc)], ["ZIII"])
    for key in ("circ", "op_ptr", "ops", "params", "term_ptr", "terms", "coeff", "ids"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key


@pytest.mark.parametrize("n,mode", [(1, "vector"), (2, "vector"), (3, "vector"), (8, "vector"), (1, "density"), (2, "density"),
                                    (4, "density"), (5, "density"), (5, "readout")])
def test_lowered_programs_interpreted_against_the_oracle(n, mode):
    """The documented record layout, interpreted in numpy, reproduces the oracle on the random programs the device tests use."""
    c = sc.random_program(n, 40, seed=0, measure=mode == "readout")
    noise = {"vector": None, "density": sc.StepNoise(5), "readout": sc.StepNoise(6, readout={q: (0.02 * q, 0.05) for q in range(n)})}[mode]
    terms = sc.term_set(n, alphabet="IZ" if mode == "readout" else "IXYZ")
    batch = sim.compile_programs([c], [terms], noise)
    value, tv, norm = sc.interpret(batch, 0)
    ov, otv, onorm = sc.simulate(c, terms, noise)
    tb, vb = sc.term_bound(c, noise), sc.value_bound(c, terms, noise)
    assert tb < sc.CAP and vb < sc.CAP
    assert abs(value - ov) <= vb and np.abs(tv - otv).max() <= tb and abs(norm - 1.0) <= tb and abs(onorm - 1.0) <= tb


def test_noise_model_from_the_lima_table(lima_backend):
    noise = sim.NoiseModel.from_backend(lima_backend)
    props = lima_backend.properties()
    errs = {(g.gate, tuple(g.qubits)): next((p.value for p in g.parameters if p.name == "gate_error"), None) for g in props.gates}
    assert noise.after_gate(0, "sx", (1,)) == 2 * errs[("sx", (1,))]
    assert noise.after_gate(0, "cx", (0, 1)) == errs[("cx", (0, 1))] * 4 / 3
    assert noise.after_gate(0, "rz", (0,)) is None            # a zero gate_error emits nothing
    with pytest.raises(ValueError, match=r"\(0, 4\)"):
        noise.after_gate(0, "cx", (0, 4))                      # no such pair on lima
    qp = props.qubit_property(2)
    assert noise.readout_of(2) == (qp["prob_meas0_prep1"][0], qp["prob_meas1_prep0"][0])
    assert sim.NoiseModel.from_backend(lima_backend, readout=False).readout_of(2) is None
    sym = sim.NoiseModel.from_backend(synthetic_backend(3, "cx"))   # only a symmetric readout_error in this table
    e = synthetic_backend(3, "cx").properties().qubit_property(1)["readout_error"][0]
    assert sym.readout_of(1) == (e, e)
    with pytest.raises(ValueError, match="lambda"):
        sim.NoiseModel({("x", (0,)): 1.5})


# ---- the generator with the oracle in the simulator's place -------------------------------------------------------------------------
def test_exp_value_generator_with_the_oracle(monkeypatch):
    from blackwater.data.generators.exp_val import ExpValueEntry, exp_value_generator

    monkeypatch.setattr(sim, "expectation_values", sc.oracle_expectation_values)
    backend = synthetic_backend(4, "cx")
    a = list(exp_value_generator(backend, 4, 6, 3, max_entries=10, seed=5, batch=4))
    b = list(exp_value_generator(backend, 4, 6, 3, max_entries=10, seed=5, batch=7))
    other = list(exp_value_generator(backend, 4, 6, 3, max_entries=10, seed=6, batch=4))
    assert len(a) == 10 and [e.to_dict() for e in a] == [e.to_dict() for e in b]
    assert [e.ideal_exp_value for e in a] != [e.ideal_exp_value for e in other]
    for e in a:
        assert isinstance(e.ideal_exp_value, float) and len(e.noisy_exp_values) == 1 and abs(e.ideal_exp_value) <= 3.0 + 1e-12
        assert np.asarray(e.observable).shape == (3, 1 + 4 * 4) and 1 <= e.circuit_depth
        assert len(e.circuit_graph["nodes"]["DAGOpNode"][0]) == 22
        back = ExpValueEntry.from_json(e.to_dict())
        assert back.to_dict() == e.to_dict()
    assert any(e.noisy_exp_values[0] != e.ideal_exp_value for e in a)


def test_encode_corpus_default_labels_are_unchanged():
    """``simulate=None`` reproduces the arrays of the commit before the simulator, bit for bit (the same draws in the same order)."""
    circuits = [random_circuit(4, 3 + k, k) for k in range(5)]
    got = encode_corpus(circuits, 4, seed=7)
    rng = np.random.default_rng(7)
    for k, c in enumerate(circuits):
        ideal = rng.uniform(-1, 1, size=1)
        n2q = sum(1 for op in c.ops if op.name == "cx")
        noisy = ideal * math.exp(-5e-3 * n2q) + rng.normal(0, 0.01, size=1)
        qz = int(rng.integers(0, 4))
        assert got["y"][k, 0] == np.float32(ideal[0]) and got["noisy"][k, 0] == np.float32(noisy[0])
        assert got["observable"][k, 0, 2 + 4 * qz] == 1.0
    again = encode_corpus(circuits, 4, seed=7, simulate=None)
    assert all(np.array_equal(np.asarray(got[key]), np.asarray(again[key])) for key in ("y", "noisy", "depth", "observable"))
