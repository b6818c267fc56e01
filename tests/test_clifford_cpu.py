"""The Clifford path on the host: tables, lowering, refusals and the record format (``clifford_cases.interpret``) against the three
oracles of tests/clifford_cases.py.  Nothing here needs a GPU; tests/test_gpu_clifford.py holds the kernel to the interpreter."""
import itertools
import math
import os

import numpy as np
import pytest

import clifford_cases as cc
import sim_cases
from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.sim import clifford as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PI = math.pi / 2
ALL_GATES = sim_cases.ONE_QUBIT + sim_cases.TWO_QUBIT
LETTERS = "IXZY"   # by letter code: bit 0 = x, bit 1 = z


def _pauli(code, width):
    m = sim_cases.PAULI[LETTERS[code & 3]]
    return m if width == 1 else sim_cases.kron2(sim_cases.PAULI[LETTERS[code >> 2]], m)


def _decode(name, packed):
    a, b, c = packed
    if name in sim_cases.TWO_QUBIT:
        return [((a | b << 32) >> (4 * e) & 15, c >> e & 1) for e in range(15)]
    return [(a >> (3 * e) & 3, a >> (3 * e + 2) & 1) for e in range(3)]


def test_gate_lists_and_constants_match_the_header():
    assert len(ALL_GATES) == 24 and set(ALL_GATES) == set(sim.SUPPORTED_GATES)
    header = open(os.path.join(ROOT, "include", "mlqem_hip.h")).read()
    for name, value in (("MAX_QUBITS", cl.MAX_QUBITS_CLIFFORD), ("REG_QUBITS", cl.REG_QUBITS), ("PAD", cl.PAD), ("OP_C1", cl.CL_C1),
                        ("OP_C2", cl.CL_C2), ("OP_DEPOL1", cl.CL_DEPOL1), ("OP_DEPOL2", cl.CL_DEPOL2)):
        assert f"#define MLQEM_CLIFFORD_{name} {value}\n" in header
    assert (cc.REG_QUBITS, cc.MAX_QUBITS) == (cl.REG_QUBITS, cl.MAX_QUBITS_CLIFFORD) and sim.MAX_QUBITS_CLIFFORD == 512
    from blackwater.native import ops
    assert (ops.CLIFFORD_MAX_QUBITS, ops.CLIFFORD_REG_QUBITS, ops.CLIFFORD_PAD) == (512, 128, 32)


@pytest.mark.parametrize("name", ALL_GATES)
def test_every_table_is_the_numeric_conjugation(name):
    """All 24 gate names at every angle k pi / 2, k = -4 .. 4 (every combination for u2, u3, u): the packed table says U^dagger P U =
    +-P' and the oracle's own matrix (sim_cases.gate_matrix, built from Pauli algebra, not from program.py) agrees, entry by entry."""
    width = 2 if name in sim_cases.TWO_QUBIT else 1
    n_par = sim_cases.N_PARAMS.get(name, 0)
    for ks in itertools.product(range(-4, 5), repeat=n_par):
        params = tuple(k * HALF_PI for k in ks)
        packed = cl.gate_table(name, params)
        if name in ("t", "tdg"):
            assert packed is None
            continue
        if name == "id":
            assert packed == "id"
            continue
        assert packed is not None, (name, ks)
        u = sim_cases.gate_matrix(name, params)
        table = _decode(name, packed)
        assert len(table) == 4 ** width - 1
        for e, (image, s) in enumerate(table):
            got = u.conj().T @ _pauli(e + 1, width) @ u
            assert image != 0 and np.abs(got - (-1) ** s * _pauli(image, width)).max() < 1e-12, (name, ks, e)


@pytest.mark.parametrize("name, params", [("rz", (0.3,)), ("rz", (HALF_PI + 1e-6,)), ("rx", (1.0,)), ("ry", (math.pi / 4,)),
                                          ("p", (0.1,)), ("u1", (-2.2,)), ("u2", (0.0, 0.4)), ("u3", (0.7, 0.0, 0.0)),
                                          ("u", (HALF_PI, HALF_PI, 0.01)), ("rzz", (math.pi / 4,)), ("t", ()), ("tdg", ())])
def test_non_clifford_gates_are_refused_by_name(name, params):
    qubits = (1, 0) if name == "rzz" else (1,)
    circ = Circuit(2, 0, [CircuitOp("h", (0,)), CircuitOp(name, qubits, (), params)])
    assert not sim.is_clifford(circ)
    shown = f"{name}({', '.join(repr(v) for v in params)})" if params else name
    with pytest.raises(ValueError) as err:
        sim.compile_clifford([Circuit(2, 0, [CircuitOp("h", (0,))]), circ], ["ZZ", "ZZ"])
    assert "circuit 1: op 1" in str(err.value) and shown in str(err.value) and "is not a Clifford gate" in str(err.value)


def test_rz_just_inside_the_tolerance_is_taken_as_exact():
    assert cl.gate_table("rz", (HALF_PI + 1e-10,)) == cl.gate_table("rz", (HALF_PI,)) == cl.gate_table("s", ())


def test_is_clifford():
    from blackwater.data.synthetic import clifford_tfim_circuit, random_circuit, random_clifford_circuit, tfim_circuit

    assert sim.is_clifford(clifford_tfim_circuit(100, 2, 1, 3)) and sim.is_clifford(clifford_tfim_circuit(7, 1, 2, -1, two_q="cx"))
    assert sim.is_clifford(random_clifford_circuit(600, 3, 0))   # the width is compile_clifford's business
    assert not sim.is_clifford(tfim_circuit(5, 1, J=0.3)) and not sim.is_clifford(random_circuit(6, 8, 1))
    assert not sim.is_clifford(Circuit(1, 0, [CircuitOp("reset", (0,))]))
    assert not sim.is_clifford(Circuit(1, 0, [CircuitOp("rz", (0,), (), (float("nan"),))]))
    assert sim.is_clifford(Circuit(2, 2, [CircuitOp("barrier", (0, 1)), CircuitOp("measure", (0,), (0,))]))


def test_generated_clifford_circuits():
    from blackwater.data.synthetic import clifford_tfim_circuit, random_clifford_circuit, tfim_circuit

    a, b = random_clifford_circuit(9, 6, 3), random_clifford_circuit(9, 6, 3)
    assert a.ops == b.ops and a.ops != random_clifford_circuit(9, 6, 4).ops
    names = {op.name for s in range(8) for op in random_clifford_circuit(9, 6, s, two_q="ecr").ops}
    assert names == {"h", "s", "sdg", "x", "y", "z", "sx", "ecr", "barrier", "measure"}
    for s in range(8):   # basis=True is the same circuit in {rz, sx, x, two_q}, up to global phases
        plain, lowered = random_clifford_circuit(7, 5, s, measure=False), random_clifford_circuit(7, 5, s, measure=False, basis=True)
        assert {op.name for op in lowered.ops} <= {"rz", "sx", "x", "cx"} and sim.is_clifford(lowered)
        labels = [label for label, _ in cc.stabilizer_terms(plain, 8, s)]
        assert np.array_equal(cc.tableau_values(plain, labels), cc.tableau_values(lowered, labels))
    for layer_circ in (random_clifford_circuit(9, 1, s, measure=False) for s in range(8)):   # a layer's gates are disjoint
        touched = [q for op in layer_circ.ops for q in op.qubits]
        assert len(touched) == len(set(touched)) and all(abs(op.qubits[0] - op.qubits[1]) == 1 for op in layer_circ.ops if len(op.qubits) == 2)
    # clifford_tfim_circuit is tfim_circuit at theta = kx pi / 2, phi = kz pi / 2: dt = 0.5 makes theta = h and phi = -J
    assert clifford_tfim_circuit(6, 2, 1, 3).ops == tfim_circuit(6, 2, J=-3 * HALF_PI, h=HALF_PI).ops
    # and tfim_circuit itself is what it was: the angles of its first step
    t = tfim_circuit(4, 1, J=0.4)
    assert t.ops[2].params == (2 * 0.66 * math.pi * 0.5 + math.pi,) and [op.params for op in t.ops if op.params == (-2 * 0.4 * 0.5,)]


# ---- the record format against the oracles ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_interpreter_against_the_density_matrix_oracle(n):
    """Oracle (b) with StepNoise (lambda = 0 and lambda = 1 forced, a depolarising op after every gate, ``id`` included)."""
    for seed in range(4):
        circ = cc.random_clifford_program(n, 24, seed, measure=True)
        terms = cc.random_terms(n, 8, seed) + cc.stabilizer_terms(circ, 6, seed) + [("I" * n, 0.2)]
        noise = sim_cases.StepNoise(seed)
        batch = sim.compile_clifford([circ], [terms], noise)
        vi, vn, ti, tn, _, _ = cc.interpret(batch)
        v0, t0, _ = sim_cases.simulate(circ, terms, None)
        v1, t1, _ = sim_cases.simulate(circ, terms, noise)
        assert np.abs(ti).sum() >= 6
        assert np.abs(ti - t0).max() <= sim_cases.term_bound(circ) < sim_cases.CAP
        for j in range(len(terms)):
            bound = cc.noisy_bound(batch, 0, t1[j], sim_cases.term_bound(circ, noise))
            assert abs(tn[j] - t1[j]) <= bound < sim_cases.CAP
        assert abs(vi[0] - v0) <= sim_cases.value_bound(circ, terms) and abs(vn[0] - v1) <= sim_cases.value_bound(circ, terms, noise) + \
            (cc.depol_count(batch, 0) + 2) * sim_cases.U * sum(abs(c) for _, c in terms)
        # noise=None lowers no noise record and the noisy outputs equal the ideal ones
        plain = cc.interpret(sim.compile_clifford([circ], [terms]))
        assert (plain[2] == ti).all() and (plain[3] == ti).all() and (plain[0] == plain[1]).all()


@pytest.mark.parametrize("n", [6, 9, 11])
def test_interpreter_against_the_state_vector_oracle(n):
    circ = cc.random_clifford_program(n, 60, n)
    terms = cc.random_terms(n, 6, n) + cc.stabilizer_terms(circ, 10, n)
    _, _, ti, _, _, _ = cc.interpret(sim.compile_clifford([circ], [terms]))
    _, t0, _ = sim_cases.simulate(circ, terms, None)
    assert np.abs(ti - t0).max() <= sim_cases.term_bound(circ) < sim_cases.CAP and np.abs(ti).sum() >= 10


@pytest.mark.parametrize("n", [1, 2, 5, 31, 32, 33, 64, 65, 100, 128, 129, 512])
def test_interpreter_against_the_tableau(n):
    """Oracle (c), exactly: the values are -1, 0 or +1."""
    circ = cc.random_clifford_program(n, 4 * n + 20, n, local=6)
    terms = cc.random_terms(n, 4, n, weight=3) + cc.stabilizer_terms(circ, 12, n)
    vi, _, ti, _, _, _ = cc.interpret(sim.compile_clifford([circ], [terms]))
    want = cc.tableau_values(circ, [label for label, _ in terms])
    assert (ti == want).all() and set(np.unique(ti)) <= {-1.0, 0.0, 1.0} and np.abs(ti[4:]).min() == 1.0


BLOCKS = cc.BLOCKS


@pytest.mark.parametrize("n", sorted(BLOCKS))
def test_interpreter_against_the_block_oracle(n):
    """Oracle (d): noisy values at width, blocks across the word boundaries."""
    blocks = cc.BlockCircuit(n, BLOCKS[n], 10, n)
    noise = sim_cases.StepNoise(n)
    terms = blocks.stabilizer_terms(24, n) + blocks.random_terms(8, n)
    batch = sim.compile_clifford([blocks.wide], [terms], noise)
    _, _, ti, tn, _, _ = cc.interpret(batch)
    want, oracle_bound = blocks.term_values(terms, noise)
    assert (ti == cc.tableau_values(blocks.wide, [label for label, _ in terms])).all() and np.abs(ti).sum() >= 24
    assert np.count_nonzero((np.abs(tn) > 0) & (np.abs(tn) < 1)) >= 12   # the noise shows
    for j in range(len(terms)):
        bound = cc.noisy_bound(batch, 0, want[j], oracle_bound[j])
        assert abs(tn[j] - want[j]) <= bound < sim_cases.CAP


READOUTS = {"symmetric": lambda q: (0.02 + 0.01 * (q % 3), 0.02 + 0.01 * (q % 3)),
            "asymmetric": lambda q: (0.05 + 0.01 * (q % 4), 0.01 * (q % 3)),
            "zero": lambda q: (0.0, 0.0),
            "mixed": lambda q: [(0.0, 0.0), (0.03, 0.03), (0.04, 0.01), (1.0, 0.0)][q % 4]}


@pytest.mark.parametrize("kind", sorted(READOUTS))
def test_readout_expansion_against_simulate(kind):
    """Z terms of weight 1 .. 4 on measured qubits with readout noise, against oracle (b), and at width against oracle (d)."""
    for n in (1, 2, 4, 5):
        circ = cc.random_clifford_program(n, 16, n, measure=True)
        ro = {q: READOUTS[kind](q) for q in range(n)}
        noise = sim_cases.StepNoise(n, readout=ro)
        terms = [("".join("Z" if q in qs else "I" for q in reversed(range(n))), 0.1 * (len(qs) + 1))
                 for w in range(1, min(n, 4) + 1) for qs in itertools.combinations(range(n), w)]
        terms += [(label, c) for label, c in cc.stabilizer_terms(circ, 12, n) if set(label) <= {"I", "Z"}]
        batch = sim.compile_clifford([circ], [terms], noise)
        vi, vn, ti, tn, _, _ = cc.interpret(batch)
        v1, t1, _ = sim_cases.simulate(circ, terms, noise)
        _, t0, _ = sim_cases.simulate(circ, terms, None)
        assert np.abs(ti - t0).max() <= sim_cases.term_bound(circ)   # the ideal outputs know nothing of the readout
        for j, (label, _) in enumerate(terms):
            m = label.count("Z")
            bound = 2 ** m * cc.noisy_bound(batch, 0, 1.0, 0.0, readout_factors=m) + sim_cases.term_bound(circ, noise)
            assert abs(tn[j] - t1[j]) <= bound < sim_cases.CAP, (n, label)
        if kind in ("symmetric", "zero"):
            assert len(batch.units) == len(terms)   # b = 0: a factor, no expansion
        elif kind == "asymmetric":
            assert len(batch.units) == sum(2 ** label.count("Z") for label, _ in terms)
    blocks = cc.BlockCircuit(100, BLOCKS[100], 8, 4, names=cc.CLASSICAL)
    noise = sim_cases.StepNoise(6, readout={q: READOUTS[kind](q) for q in range(100)})
    terms = blocks.stabilizer_terms(20, 2)
    assert all(set(label) <= {"I", "Z"} for label, _ in terms) and max(label.count("Z") for label, _ in terms) >= 4
    batch = sim.compile_clifford([blocks.wide], [terms], noise)
    _, _, ti, tn, _, _ = cc.interpret(batch)
    want, oracle_bound = blocks.term_values(terms, noise)
    assert (np.abs(ti) == 1.0).all()
    for j, (label, _) in enumerate(terms):
        m = label.count("Z")
        assert abs(tn[j] - want[j]) <= 2 ** m * cc.noisy_bound(batch, 0, 1.0, 0.0, readout_factors=m) + oracle_bound[j] < sim_cases.CAP


def test_readout_needs_a_measured_qubit_and_nontrivial_probabilities():
    circ = Circuit(3, 3, [CircuitOp("x", (0,)), CircuitOp("h", (2,)), CircuitOp("measure", (0,), (0,))])
    noise = sim.NoiseModel(readout={0: (0.1, 0.02), 1: (0.3, 0.3), 2: (0.0, 0.0)})
    batch = sim.compile_clifford([circ], [[("IIZ", 1.0), ("IZI", 1.0)]], noise)
    _, _, ti, tn, _, _ = cc.interpret(batch)
    assert ti.tolist() == [-1.0, 1.0]
    assert tn[0] == (0.1 - 0.02) * 1.0 + (1.0 - 0.1 - 0.02) * -1.0 and tn[1] == 1.0   # qubit 1 is not measured
    trivial = sim.NoiseModel(readout={0: (0.0, 0.0), 1: (0.3, 0.3)})   # nothing non-trivial on a measured qubit: X terms may stay
    assert cc.interpret(sim.compile_clifford([circ], [[("XII", 1.0), ("IIZ", 1.0)]], trivial))[3].tolist() == [1.0, -1.0]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_shared_with_compile_programs_read_the_same():
    bad = [
        (Circuit(2, 2, [CircuitOp("measure", (0,), (0,)), CircuitOp("x", (0,))]), "ZZ"),            # gate after measure
        (Circuit(2, 0, [CircuitOp("rz", (0,), (), ())]), "ZZ"),                                       # parameter count
        (Circuit(2, 0, [CircuitOp("rz", (0,), (), (float("inf"),))]), "ZZ"),                          # non-finite angle
        (Circuit(2, 0, [CircuitOp("x", (2,))]), "ZZ"),                                                # qubit out of range
        (Circuit(2, 0, [CircuitOp("cx", (1, 1))]), "ZZ"),                                             # one qubit twice
        (Circuit(2, 0, [CircuitOp("reset", (0,))]), "ZZ"),                                            # unknown gate
        (Circuit(2, 0, [CircuitOp("x", (0,))]), [("ZZ", 1j)]),                                        # non-real coefficient
        (Circuit(2, 0, [CircuitOp("x", (0,))]), "ZZZ"),                                               # label length
        (Circuit(2, 0, [CircuitOp("x", (0,))]), "ZQ"),                                                # alphabet
    ]
    for circ, obs in bad:
        with pytest.raises(ValueError) as want:
            sim.compile_programs([circ], [obs])
        with pytest.raises(ValueError) as got:
            sim.compile_clifford([circ], [obs])
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match="1 circuits but 2 observables"):
        sim.compile_clifford([bad[0][0]], ["ZZ", "ZZ"])


def test_refusals_of_the_clifford_path():
    h = lambda n: Circuit(n, n, [CircuitOp("h", (0,))] + [CircuitOp("measure", (q,), (q,)) for q in range(n)])
    with pytest.raises(ValueError, match=r"circuit 1: 513 qubits.*512"):
        sim.compile_clifford([h(512), h(513)], ["I" * 512, "I" * 513])
    assert len(sim.compile_clifford([h(512)], ["Z" * 512]).masks) == 32 + cl.PAD
    asym = sim.NoiseModel(readout={q: (0.02, 0.01) for q in range(12)})
    with pytest.raises(ValueError, match="X or Y"):
        sim.compile_clifford([h(3)], ["IXZ"], asym)
    with pytest.raises(ValueError, match=r"term 'IZZZZZZZZZZZ'.*2\^11.*2\^10"):
        sim.compile_clifford([h(12)], [[("IIIIIIIIIIIZ", 1.0), ("IZZZZZZZZZZZ", 1.0)]], asym)
    assert len(sim.compile_clifford([h(12)], ["IIZZZZZZZZZZ"], asym).units) == 1024
    sym = sim.NoiseModel(readout={q: (0.02, 0.02) for q in range(12)})
    assert len(sim.compile_clifford([h(12)], ["ZZZZZZZZZZZZ"], sym).units) == 1   # symmetric readout only scales
    with pytest.raises(ValueError, match="depolarising parameter"):
        class Bad(sim_cases.NoNoise):
            def after_gate(self, index, name, qubits):
                return 1.5
        sim.compile_clifford([h(2)], ["ZZ"], Bad())


def test_layout_of_a_mixed_batch():
    """Units of circuits up to 128 qubits come first (the register instantiation), circuit order is kept inside each part, and the
    combine lists follow the units."""
    widths = [129, 5, 512, 128, 33]
    circs = [cc.random_clifford_program(n, 10, n, local=4) for n in widths]
    obs = [cc.random_terms(n, 3, n, weight=2) for n in widths]
    batch = sim.compile_clifford(circs, obs)
    assert (batch.n_reg, batch.n_lds) == (9, 6) and batch.units[:, 0].tolist() == [1] * 3 + [3] * 3 + [4] * 3 + [0] * 3 + [2] * 3
    assert batch.ops.dtype == np.uint32 and batch.masks.dtype == np.uint32 and batch.pool.shape == (cl.PAD,)
    assert batch.units[batch.comb_unit, 0].tolist() == np.repeat(np.arange(5), 3).tolist()
    alone = [cc.interpret(sim.compile_clifford([c], [o])) for c, o in zip(circs, obs)]
    both = cc.interpret(batch)
    assert (both[0] == np.concatenate([a[0] for a in alone])).all() and (both[2] == np.concatenate([a[2] for a in alone])).all()
    empty = sim.compile_clifford([], [])
    assert len(empty) == 0 and empty.ops.shape == (0, 4) and empty.units.shape == (0, 4)
    id_only = sim.compile_clifford([Circuit(1, 0, [CircuitOp("id", (0,))])], ["Z"], sim_cases.StepNoise(1, force=False))
    assert (id_only.ops[:, 0] & 15).tolist() == [cl.CL_DEPOL1]   # id: no gate record, its noise record stays


def test_tables_are_cached_per_gate_and_angle():
    from blackwater.data.synthetic import clifford_tfim_circuit

    cl._TABLES.clear()
    sim.compile_clifford([clifford_tfim_circuit(100, 2, 1, 1)], ["I" * 99 + "Z"])
    assert 0 < len(cl._TABLES) <= 12


# ---- the public interface, as far as it goes without a GPU -----------------------------------------------------------------------------
def test_estimator_methods_on_the_host():
    from blackwater.data.synthetic import clifford_tfim_circuit, tfim_circuit

    est = sim.DeviceEstimator()
    assert est._method == "exact" and sim.DeviceEstimator(method="exact")._method == "exact"
    with pytest.raises(ValueError, match="method = 'stabilizer'"):
        sim.DeviceEstimator(method="stabilizer")
    wide, small, wild = clifford_tfim_circuit(100, 1, 1, 1), clifford_tfim_circuit(4, 1, 1, 1), tfim_circuit(100, 1, J=0.3)
    auto = sim.DeviceEstimator(method="auto")
    assert not auto._use_clifford([small, small]) and auto._use_clifford([small, wide])
    assert not auto._use_clifford([tfim_circuit(11, 1, J=0.3)])                       # fits the state-vector cap
    assert sim.DeviceEstimator(sim.NoiseModel(), method="auto")._use_clifford([clifford_tfim_circuit(6, 1, 1, 1)])   # over the density cap
    with pytest.raises(ValueError, match="circuit 2 is not a Clifford circuit"):
        auto._use_clifford([small, wide, wild])
    assert sim.DeviceEstimator(method="clifford")._use_clifford([small])
    for est in (sim.DeviceEstimator(method="clifford", shots=100), sim.DeviceEstimator(method="auto", shots=100)):
        with pytest.raises(ValueError, match="shots are not drawn on the Clifford path"):
            est.run([wide], ["I" * 99 + "Z"])
    with pytest.raises(ValueError, match="shots are not drawn"):
        sim.DeviceEstimator(method="clifford").run([wide], ["I" * 99 + "Z"], shots=10)
    with pytest.raises(ValueError, match="must arrive bound"):
        sim.DeviceEstimator(method="clifford").run([wide], ["I" * 99 + "Z"], [(0.1,)])


def test_encode_corpus_defaults_are_byte_identical():
    from blackwater.data.synthetic import clifford_tfim_circuit, encode_corpus, random_circuit

    circs = [random_circuit(6, 5, s) for s in range(3)] + [clifford_tfim_circuit(6, 1, 1, 1, two_q="cx")]
    a, b = encode_corpus(circs, 6), encode_corpus(circs, 6, clifford=False)
    assert a.keys() == b.keys()
    for key in a:
        for u, v in zip(a[key], b[key]):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), key
    with pytest.raises(ValueError, match="needs simulate="):
        encode_corpus(circs, 6, clifford=True)
    with pytest.raises(ValueError, match="shots are not drawn"):
        encode_corpus(circs, 6, clifford=True, simulate=sim.NoiseModel(), shots=10)


def test_clifford_run_refuses_cpu_tensors_loudly():
    from blackwater.native import _lib, ops

    batch = sim.compile_clifford([cc.random_clifford_program(3, 5, 0)], ["ZZZ"])
    t = batch.to("cpu")
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.clifford_run(t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"], t["term_ptr"],
                         t["coeff"], t["comb_ptr"], t["comb_unit"], t["comb_weight"])
    lib = _lib.load()
    assert lib.mlqem_clifford_run_f64(1, None, None, None, 0, None, 31, None, 0, 0, None, 32, None, None, 0, None, None, None, 0, None,
                                      None, None, None, None, None, None) == -1   # n_pool < 32: refused before any launch
