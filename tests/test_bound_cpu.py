"""Parameter binding on the host (no GPU): ``Param`` / ``Template``, the lowering of ``compile_templates``, the interpreter of the
bound-run format against the numpy oracle on bound circuits, the parameter-shift rule against central differences, and every
refusal by name.  tests/test_gpu_bound.py checks the kernels."""
import math

import numpy as np
import pytest

import bound_cases as bc
import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.data.synthetic import tfim_template, two_local
from blackwater.sim import Param, Template, compile_programs, compile_templates
from blackwater.sim.template import OP_PP, OP_PRX, OP_PRY, OP_PRZ, OP_PRZZ


# ---- Param -------------------------------------------------------------------------------------------------------------------------
def test_param_algebra():
    p = Param(3)
    assert (p.index, p.scale, p.offset) == (3, 1.0, 0.0)
    q = -(2 * p + 1.5) / 4 - 0.25
    assert isinstance(q, Param) and (q.index, q.scale, q.offset) == (3, -0.5, -0.625)
    assert (1 - p) == Param(3, -1.0, 1.0) and (p - 1) == Param(3, 1.0, -1.0) and (p * 0.5) == Param(3, 0.5, 0.0)
    assert (0.5 + p) == Param(3, 1.0, 0.5) and (+p) is p
    assert q.value([0, 0, 0, 2.0]) == -0.5 * 2.0 + -0.625


def test_param_refusals():
    p, q = Param(0), Param(1)
    for f in (lambda: p * q, lambda: p + q, lambda: p - q, lambda: p / q, lambda: 1.0 / p, lambda: p * "x"):
        with pytest.raises(TypeError, match="only affine expressions of one parameter are supported"):
            f()
    with pytest.raises(TypeError, match=r"Template\.bind_parameters"):
        float(p)
    with pytest.raises(ValueError, match="index"):
        Param(-1)


# ---- Template ----------------------------------------------------------------------------------------------------------------------
def _hand_template():
    ops = [CircuitOp("h", (0,)), CircuitOp("rx", (0,), (), (Param(1, 2.0, 0.25),)), CircuitOp("cx", (0, 1)),
           CircuitOp("rzz", (0, 1), (), (Param(0, -1.0),)), CircuitOp("rz", (1,), (), (0.5,)), CircuitOp("p", (1,), (), (Param(1) / 3,))]
    return Template(2, 0, ops)


def test_bind_parameters_against_a_hand_built_circuit():
    t = _hand_template()
    assert t.num_parameters == 2 and isinstance(t, Circuit)
    bound = t.bind_parameters([0.3, -1.1])
    assert type(bound) is Circuit and t.assign_parameters([0.3, -1.1]).ops == bound.ops
    want = [("h", ()), ("rx", (2.0 * -1.1 + 0.25,)), ("cx", ()), ("rzz", (-1.0 * 0.3 + 0.0,)), ("rz", (0.5,)), ("p", ((1 / 3) * -1.1 + 0.0,))]
    assert [(op.name, op.params) for op in bound.ops] == want
    assert Circuit.from_any(t) is t
    from blackwater.library.primitives import transpile_and_bind

    again = transpile_and_bind(t, None, [0.3, -1.1], {})
    assert type(again) is Circuit and again.ops == bound.ops
    with pytest.raises(ValueError, match="got 3 values, the template has 2 parameters"):
        t.bind_parameters([1, 2, 3])


def test_template_refusals():
    for name, params in (("u3", (Param(0), 0.1, 0.2)), ("u2", (0.1, Param(0))), ("u", (Param(0), 0.0, 0.0))):
        with pytest.raises(ValueError, match=rf"op 0 \({name}\) has a free parameter.*rz \. ry \. rz"):
            Template(1, 0, [CircuitOp(name, (0,), (), params)])
    with pytest.raises(ValueError, match=r"op 0 \(h\) has a free parameter"):
        Template(1, 0, [CircuitOp("h", (0,), (), (Param(0),))])
    with pytest.raises(ValueError, match="uses parameter 4, the template has num_parameters = 2"):
        Template(1, 0, [CircuitOp("rx", (0,), (), (Param(4),))], [], 2)
    with pytest.raises(TypeError, match=r"Template\.bind_parameters"):   # a template where a bound circuit is wanted
        compile_programs([_hand_template()], ["ZZ"])


# ---- a qiskit-like circuit with free parameters ----------------------------------------------------------------------------------------
class FakeParameter:
    def __init__(self, name):
        self.name = name

    @property
    def parameters(self):
        return {self}

    def bind(self, values):
        return float(values[self])

    def __repr__(self):
        return self.name


class FakeExpression:
    """f(values of its parameters): what a ParameterExpression is to the reader."""

    def __init__(self, pars, f):
        self._pars, self._f = list(pars), f

    @property
    def parameters(self):
        return set(self._pars)

    def bind(self, values):
        return float(self._f(*[values[p] for p in self._pars]))


class FakeGate:
    def __init__(self, name, params=()):
        self.name, self.params = name, list(params)


class FakeInstruction:
    def __init__(self, operation, qubits, clbits=()):
        self.operation, self.qubits, self.clbits = operation, tuple(qubits), tuple(clbits)


class FakeQuantumCircuit:
    def __init__(self, n, parameters):
        self.qubits = [object() for _ in range(n)]
        self.clbits = []
        self.data = []
        self.parameters = list(parameters)

    def add(self, name, qubits, params=()):
        self.data.append(FakeInstruction(FakeGate(name, params), [self.qubits[q] for q in qubits]))


def test_qiskit_like_order_and_affine_recovery():
    a, b = FakeParameter("a"), FakeParameter("b")
    qc = FakeQuantumCircuit(2, [a, b])
    qc.add("h", [0])
    qc.add("ry", [1], [b])
    qc.add("rx", [0], [FakeExpression([a], lambda v: 2.0 * v - 0.75)])
    qc.add("rzz", [0, 1], [FakeExpression([b], lambda v: -0.5 * v)])
    qc.add("rz", [1], [0.125])
    t = Template.from_any(qc)
    assert t.num_parameters == 2 and t.num_qubits == 2
    assert [op.params for op in t.ops] == [(), (Param(1, 1.0, 0.0),), (Param(0, 2.0, -0.75),), (Param(1, -0.5, 0.0),), (0.125,)]
    assert Template.from_any(t) is t
    plain = Template.from_any(Circuit(1, 0, [CircuitOp("h", (0,))]))
    assert isinstance(plain, Template) and plain.num_parameters == 0 and plain.bind_parameters([]).ops == [CircuitOp("h", (0,))]


def test_qiskit_like_refusals():
    a, b = FakeParameter("a"), FakeParameter("b")
    qc = FakeQuantumCircuit(1, [a, b])
    qc.add("rx", [0], [FakeExpression([a, b], lambda u, v: u + v)])
    with pytest.raises(ValueError, match=r"parameter 0 of op 0 \(rx\) is an expression of 2 parameters.*only affine"):
        Template.from_any(qc)
    qc = FakeQuantumCircuit(1, [a])
    qc.add("h", [0])
    qc.add("rz", [0], [FakeExpression([a], lambda v: v * v)])
    with pytest.raises(ValueError, match=r"parameter 0 of op 1 \(rz\) is not affine in a"):
        Template.from_any(qc)


# ---- builders ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entanglement, n_pairs", [("full", 6), ("linear", 3)])
def test_two_local_order_and_counts(entanglement, n_pairs):
    t = two_local(4, reps=3, entanglement=entanglement)
    assert t.num_parameters == 16 and t.num_qubits == 4
    assert t.count_ops() == {"ry": 16, "cz": 3 * n_pairs}
    rot = [op for op in t.ops if op.name == "ry"]
    assert [op.params[0] for op in rot] == [Param(k) for k in range(16)]          # layer-major, then qubit
    assert [op.qubits[0] for op in rot] == [0, 1, 2, 3] * 4
    names = [op.name for op in t.ops]
    assert names[:4] == ["ry"] * 4 and names[4:4 + n_pairs] == ["cz"] * n_pairs and names[-4:] == ["ry"] * 4
    pairs = [op.qubits for op in t.ops[4:4 + n_pairs]]
    assert pairs == ([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] if entanglement == "full" else [(0, 1), (1, 2), (2, 3)])
    two = two_local(3, rotation_blocks=("ry", "rz"), entanglement_blocks="cx", entanglement="linear", reps=1)
    assert [(op.name, op.qubits[0], op.params[0].index) for op in two.ops[:6]] == [
        ("ry", 0, 0), ("ry", 1, 1), ("ry", 2, 2), ("rz", 0, 3), ("rz", 1, 4), ("rz", 2, 5)]   # within a layer block-major
    assert two.num_parameters == 12
    with pytest.raises(ValueError, match="entanglement = 'circular'"):
        two_local(3, entanglement="circular")


def test_tfim_template():
    t = tfim_template(4, 3)
    assert t.num_parameters == 2 and t.count_ops() == {"rzz": 9, "rx": 12}
    assert all(op.params[0] == Param(0, 2.0) for op in t.ops if op.name == "rzz")
    assert all(op.params[0] == Param(1, 2.0) for op in t.ops if op.name == "rx")


# ---- lowering ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [None, sc.StepNoise(4)], ids=["vector", "density"])
def test_zero_parameter_template_lowers_byte_identically(noise):
    circs = [sc.random_program(n, 30, seed=n, measure=True) for n in (1, 3, 5)]
    obs = [sc.term_set(n, alphabet="IZ") for n in (1, 3, 5)]
    want = compile_programs(circs, obs, noise)
    got = compile_templates([Template.from_any(c) for c in circs], obs, noise)
    for k in ("circ", "op_ptr", "ops", "params", "term_ptr", "terms", "coeff", "ids", "gate_record", "gate_noise"):
        a, b = getattr(want, k), getattr(got, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert (got.n_wave, got.n_wg, got.variant) == (want.n_wave, want.n_wg, want.variant)
    assert got.num_parameters.tolist() == [0, 0, 0] and got.occ_ptr.tolist() == [0, 0, 0, 0]


def test_lowering_of_parameterised_records_and_occurrences():
    t = _hand_template()
    for nm in (None, sc.StepNoise(2)):
        fixed = compile_programs([t.placeholder()], ["ZZ"], nm)
        got = compile_templates([t], ["ZZ"], nm)
        assert got.ops.shape == fixed.ops.shape and np.array_equal(got.ops[:, 1:3], fixed.ops[:, 1:3])
        kinds = {1: OP_PRX, 3: OP_PRZZ, 5: OP_PP}
        recs = [int(fixed.gate_record[g]) for g in range(len(t.ops))]
        for i, rec in enumerate(recs):
            if i in kinds:
                po = int(got.ops[rec, 3])
                par = t.ops[i].params[0]
                assert int(got.ops[rec, 0]) == kinds[i] and got.params[po:po + 3].tolist() == [par.index, par.scale, par.offset]
            else:   # fixed gates and the noise records after them: the same kind and the same values
                for r in range(rec, rec + 1 + int(fixed.gate_noise_len[i])):
                    size = int(fixed.ops[r + 1, 3] - fixed.ops[r, 3]) if r + 1 < len(fixed.ops) else 0
                    assert int(got.ops[r, 0]) == int(fixed.ops[r, 0])
                    assert np.array_equal(got.params[got.ops[r, 3]:got.ops[r, 3] + size], fixed.params[fixed.ops[r, 3]:fixed.ops[r, 3] + size])
        assert got.num_parameters.tolist() == [2] and got.occ_ptr.tolist() == [0, 3]
        assert got.occ_op.tolist() == [recs[1], recs[3], recs[5]] and got.occ_param.tolist() == [1, 0, 1]
        assert got.occ_scale.tolist() == [2.0, -1.0, 1 / 3]
        assert got.params.shape[0] == int(got.ops[-1, 3]) + (3 if nm is None else 1) + 32   # the last record's values, then the padding
    assert {OP_PRX, OP_PRY, OP_PRZ, OP_PP, OP_PRZZ} == {12, 13, 14, 15, 16}
    kinds = compile_templates([bc.chain_template(3, 10)], ["ZZZ"]).ops[:, 0].tolist()
    assert kinds == [OP_PRY, OP_PRX, OP_PRZ, OP_PP, OP_PRZZ] * 2


def test_caps_and_refusals_of_compile_programs_hold():
    with pytest.raises(ValueError, match="12 qubits need 4096 amplitudes as a state vector"):
        compile_templates([two_local(12, reps=1, entanglement="linear")], ["Z" * 12])
    with pytest.raises(ValueError, match="6 qubits need 4096 amplitudes as a density matrix"):
        compile_templates([two_local(6, reps=1, entanglement="linear")], ["Z" * 6], sc.NoNoise())
    t = Template(2, 2, [CircuitOp("ry", (0,), (), (Param(0),)), CircuitOp("measure", (0,), (0,))])
    with pytest.raises(ValueError, match="readout noise on qubit 0 cannot be combined with an observable that has X or Y"):
        compile_templates([t], ["XZ"], sc.StepNoise(1, readout={0: (0.1, 0.2)}))
    with pytest.raises(ValueError, match="1 circuits but 2 observables"):
        compile_templates([t], ["ZZ", "ZZ"])


# ---- the interpreter ---------------------------------------------------------------------------------------------------------------
CPU_GRID = [c for c in bc.grid() if c[1].num_qubits <= 5 or "mixed" in c[0]]


@pytest.mark.parametrize("case", CPU_GRID, ids=[c[0] for c in CPU_GRID])
def test_interpreter_against_the_oracle_on_bound_circuits(case):
    """``interpret_bound(run)`` equals ``sim_cases.simulate(template.bind_parameters(row))`` within the derived bound with K = 0 on
    the device side (both sides use numpy's trig), unshifted and with every shifted-op choice of the grid; each bound stays under
    the cap with the assumed K_DEV."""
    name, t, terms, noise, n_rows, span = case
    assert bc.term_bound(t, noise) < bc.CAP and bc.value_bound(t, terms, noise) < bc.CAP
    tb, vb = bc.term_bound(t, noise, k_dev=0), bc.value_bound(t, terms, noise, k_dev=0)
    batch = compile_templates([t], [terms], noise)
    theta = bc.thetas(n_rows, t.num_parameters, seed=3, span=span)
    worst = 0.0
    for row in range(min(n_rows, 2)):
        for sop in bc.shifted_ops(batch, 0):
            shift = 0.5 * math.pi if sop % 2 == 0 else -0.5 * math.pi
            got = bc.interpret_bound(batch, (0, row, sop), theta, shift)
            want = sc.simulate(bc.bound_circuit(t, batch, 0, theta[row, :t.num_parameters], sop, shift), terms, noise)
            dv, dt = abs(got[0] - want[0]), float(np.abs(got[1] - want[1]).max())
            worst = max(worst, dv)
            assert dv <= vb and dt <= tb and abs(got[2] - want[2]) <= tb, (name, row, sop, dv, dt)
    print(f"{name}: max |interpreter - oracle| {worst:.3e} <= {vb:.3e}")


def test_interpreter_clamps_as_the_header_states():
    t, terms = tfim_template(3, 2), sc.term_set(3)
    batch = compile_templates([t], [terms])
    theta = bc.thetas(3, 2, seed=5)
    n_rec = int(batch.op_ptr[1])
    ref = bc.interpret_bound(batch, (0, 2, -1), theta)
    for run in ((0, 7, -1), (5, 2, -1), (-3, 2, n_rec), (0, 2, -9), (0, 2, 10 ** 6)):   # row, template, shifted op out of range
        got = bc.interpret_bound(batch, run, theta, 0.3)
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
    assert bc.interpret_bound(batch, (0, -1, 0), theta, 0.3)[0] == bc.interpret_bound(batch, (0, 0, 0), theta, 0.3)[0]
    assert bc.interpret_bound(batch, (0, 0, 0), theta, 0.3)[0] != bc.interpret_bound(batch, (0, 0, -1), theta, 0.3)[0]
    one = bc.interpret_bound(batch, (0, 1, -1), theta[:, :1])   # ld_theta = 1: parameter index 1 is clamped to 0
    same = bc.interpret_bound(batch, (0, 1, -1), np.repeat(theta[:, :1], 2, axis=1))
    assert one[0] == same[0]
    assert bc.phi_of(3.0, 0.1, 0.2) == np.float64(np.float64(3.0) * np.float64(0.1)) + np.float64(0.2)


# ---- the parameter-shift rule ------------------------------------------------------------------------------------------------------
def _host_gradient(t, terms, row, noise, value):
    batch = compile_templates([t], [terms], noise)
    grad = np.zeros(t.num_parameters)
    for k in range(int(batch.occ_ptr[1])):
        sop, p, scale = int(batch.occ_op[k]), int(batch.occ_param[k]), float(batch.occ_scale[k])
        plus = value(bc.bound_circuit(t, batch, 0, row, sop, 0.5 * math.pi))
        minus = value(bc.bound_circuit(t, batch, 0, row, sop, -0.5 * math.pi))
        grad[p] += 0.5 * scale * (plus - minus)
    return grad


@pytest.mark.parametrize("noise", [None, sc.StepNoise(3, force=False)], ids=["ideal", "noisy"])
def test_shift_rule_against_central_differences(noise):
    """All five kinds, several occurrences per parameter with different scales: the rule is exact, central differences with
    h = 1e-5 agree to 1e-8."""
    ops = [CircuitOp("h", (0,)), CircuitOp("ry", (1,), (), (Param(0, 1.5, 0.1),)), CircuitOp("rx", (0,), (), (Param(1),)),
           CircuitOp("cx", (0, 2)), CircuitOp("rzz", (1, 2), (), (Param(0, -0.5),)), CircuitOp("rz", (2,), (), (Param(2, 2.0),)),
           CircuitOp("p", (0,), (), (Param(1, 0.75, -0.2),)), CircuitOp("h", (2,)), CircuitOp("u1", (1,), (), (Param(2),)),
           CircuitOp("ry", (2,), (), (Param(0),)), CircuitOp("sx", (1,))]
    t = Template(3, 0, ops)
    terms = sc.term_set(3, seed=1)
    row = np.asarray([0.37, -1.21, 2.05])

    def value(circ):
        return sc.simulate(circ, terms, noise)[0]

    grad = _host_gradient(t, terms, row, noise, value)
    h = 1e-5
    for p in range(3):
        e = np.zeros(3)
        e[p] = h
        central = (value(t.bind_parameters(row + e)) - value(t.bind_parameters(row - e))) / (2 * h)
        assert abs(grad[p] - central) <= 1e-8, (p, grad[p], central)
    assert np.abs(grad).max() > 1e-3


def test_shift_rule_is_zero_under_full_depolarising():
    """With lambda = 1 forced after a gate on every qubit the state is maximally mixed there whatever the angles were."""
    class Full(sc.NoNoise):
        def after_gate(self, index, name, qubits):
            return 1.0 if index >= 4 else None

    t = Template(2, 0, [CircuitOp("ry", (0,), (), (Param(0),)), CircuitOp("rx", (1,), (), (Param(1),)), CircuitOp("cx", (0, 1)),
                        CircuitOp("rzz", (0, 1), (), (Param(0, 2.0),)), CircuitOp("h", (0,)), CircuitOp("h", (1,))])
    terms = sc.term_set(2)
    grad = _host_gradient(t, terms, np.asarray([0.4, 1.3]), Full(), lambda c: sc.simulate(c, terms, Full())[0])
    assert np.abs(grad).max() <= 1e-15


def test_combine_order_matches_the_header():
    """grad[b][p] = sum over p's occurrences in circuit order of (0.5 scale_k) (v+ - v-), each step rounded: the host rule the GPU
    test compares bit for bit."""
    rng = np.random.default_rng(5)
    vp, vm = rng.normal(size=(7, 3)), rng.normal(size=(7, 3))
    par, scale = np.asarray([1, 0, 1, 1, 0, 2, 1]), rng.uniform(-2, 2, size=7)
    got = bc.host_combine(vp, vm, par, scale, 4)
    for b in range(3):
        acc = np.float64(0.0)
        for k in (0, 2, 3, 6):
            acc = acc + np.float64(np.float64(0.5 * scale[k]) * np.float64(vp[k, b] - vm[k, b]))
        assert got[b, 1] == acc
    assert np.all(got[:, 3] == 0.0) and got.shape == (3, 4)


# ---- refusals on the public surface (none of them reaches the device) ------------------------------------------------------------------
def test_estimator_refusals():
    t, obs = two_local(2, reps=1), "ZZ"
    row = [0.1] * t.num_parameters
    with pytest.raises(ValueError, match="circuit 0 comes with 3 parameter values; circuits must arrive bound"):
        sim.DeviceEstimator().run([t.bind_parameters(row)], [obs], [[0.1, 0.2, 0.3]])
    with pytest.raises(ValueError, match="circuit 0 comes with 3 parameter values, the template has 4 parameters"):
        sim.DeviceEstimator().run([t], [obs], [[0.1, 0.2, 0.3]])
    with pytest.raises(ValueError, match=r"shots= is set.*Template\.bind_parameters"):
        sim.DeviceEstimator(shots=100).run([t], [obs], [row])
    with pytest.raises(ValueError, match=r"shots= is set.*Template\.bind_parameters"):
        sim.DeviceEstimator().run([t], [obs], [row], shots=100)
    with pytest.raises(ValueError, match=r"method='trajectories'.*template with free parameters.*Template\.bind_parameters"):
        sim.DeviceEstimator(noise=bc.lima_noise(), method="trajectories").run([t], [obs], [row])
    with pytest.raises(ValueError, match=r"method='clifford'.*template with free parameters.*Template\.bind_parameters"):
        sim.DeviceEstimator(method="clifford").run([t], [obs], [row])
    wide = two_local(12, reps=1, entanglement="linear")
    with pytest.raises(ValueError, match=r"method='auto'.*template of 12 qubits, over the exact simulator's cap of 11"):
        sim.DeviceEstimator(method="auto").run([wide], ["Z" * 12], [[0.0] * wide.num_parameters])
    with pytest.raises(ValueError, match=r"ZNEDeviceEstimator: circuit 0 is a template.*Template\.bind_parameters"):
        sim.zne.zne(sim.DeviceEstimator)(noise=bc.lima_noise()).run([t], [obs], [row])


def test_bound_surface_refusals():
    t = two_local(2, reps=1)
    with pytest.raises(ValueError, match="row 0 has 3 parameter values, its template has 4 parameters"):
        sim.bound_expectation_values(t, "ZZ", [[0.1, 0.2, 0.3]])
    with pytest.raises(ValueError, match="2 templates need a list of as many observables"):
        sim.parameter_shift([t, t], "ZZ", [[0.0] * 4] * 2)
    with pytest.raises(ValueError, match="2 templates but 1 parameter rows"):
        sim.bound_expectation_values([t, t], ["ZZ", "ZZ"], [[0.0] * 4])
    with pytest.raises(ValueError, match="non-finite"):
        sim.parameter_shift(t, "ZZ", [[0.0, float("nan"), 0.0, 0.0]])
