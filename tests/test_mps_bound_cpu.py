"""Parameter binding on the matrix-product-state path, on the host: ``compile_mps_templates`` against ``compile_mps`` of the bound
copies (the same records, the factor program within the derived bound), ``tfim_circuit_template``, the parameter-shift rule
through the factor program against central differences, every refusal by name, and the guard conditions of tests/mps_cases.py on
the bound copies of every case, so that tests/test_gpu_mps_bound.py excludes none."""
import math

import numpy as np
import pytest

import bound_cases as bc
import mps_bound_cases as mbc
import mps_cases as mc
import traj_cases as tc
from blackwater import sim
from blackwater.data.circuit import CircuitOp
from blackwater.data.synthetic import tfim_circuit, tfim_circuit_template, two_local
from blackwater.sim import Param, Template, compile_mps, compile_mps_templates
from blackwater.sim.mps import FACTOR_FIXED, MpsBatch, mps_shift_runs

ALL = [c["id"] for c in mbc.grid()]
ARRAYS = ("n_qubits", "op_ptr", "ops", "params", "term_ptr", "term_circ", "term_off", "letters", "coeff", "site_ptr", "readout")


def test_a_template_without_parameters_lowers_to_the_bytes_of_compile_mps():
    for noise, traj in ((None, None), (mc.noise_model("depol", 11), 3)):
        circuits = [mc.line_program(n, 60, seed=n) if noise is None else tc.line_circuit(n, 900 + n, measure=True) for n in (1, 3, 6)]
        obs = [mc.terms_of(n, n) for n in (1, 3, 6)]
        want, got = compile_mps(circuits, obs, noise, traj, 8), compile_mps_templates(circuits, obs, noise, traj, 8)
        for k in MpsBatch.__dataclass_fields__:
            a, b = getattr(want, k), getattr(got, k)
            assert (a is None and b is None) or (np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b), k
        for k in ARRAYS:
            assert getattr(want, k).tobytes() == getattr(got, k).tobytes() and getattr(want, k).dtype == getattr(got, k).dtype, k
        assert got.fac_ptr[-1] == 0 and got.occ_ptr[-1] == 0 and not got.num_parameters.any()


@pytest.mark.parametrize("case_id", ALL)
def test_structure_is_that_of_the_bound_copy_and_the_pool_is_within_the_bound(case_id):
    c, batch, copies = mbc.case(case_id), mbc.lower(case_id), mbc.lower_copies(case_id)
    worst = 0.0
    for r, run in enumerate(mbc.plain_runs(c)):
        t = int(run[0])
        pool, ops = mbc.bind_host(batch, run, c["rows"])
        ob, oe = int(copies.op_ptr[r]), int(copies.op_ptr[r + 1])
        want_ops = copies.ops[ob:oe].copy()
        first = int(want_ops[0, 3]) if oe > ob else 0
        want_ops[:, 3] -= first
        assert np.array_equal(ops, want_ops), "kind, site, orientation, order and offsets do not depend on an angle"
        want = copies.params[first:first + pool.shape[0]]
        bound = mbc.mask_of(batch, t, mbc.lowering_bound)
        diff = np.abs(pool - want)
        assert np.array_equal(pool[bound == 0.0], want[bound == 0.0]), "copied entries are the host's, bit for bit"
        assert np.all(diff <= bound), (case_id, r, float(diff.max()))
        if np.any(bound > 0.0):
            worst = max(worst, float(np.max(diff[bound > 0.0] / bound[bound > 0.0])))
    print(f"{case_id}: bind_host against the bound copies' lowering, largest ratio to the bound {worst:.3f}")


@pytest.mark.parametrize("case_id", ALL)
def test_factor_programs_are_well_formed(case_id):
    c, batch = mbc.case(case_id), mbc.lower(case_id)
    n_param_gates = [sum(1 for op in t.ops if op.params and isinstance(op.params[0], Param)) for t in c["templates"]]
    assert np.array_equal(np.diff(batch.occ_ptr), n_param_gates), "an occurrence per parameterised gate"
    for t, tpl in enumerate(c["templates"]):
        ob = int(batch.op_ptr[t])
        occ = batch.occ[int(batch.occ_ptr[t]):int(batch.occ_ptr[t + 1])]
        pars = [op.params[0] for op in tpl.ops if op.params and isinstance(op.params[0], Param)]
        for (rec, fac), par, index, scale in zip(occ, pars, batch.occ_param[int(batch.occ_ptr[t]):], batch.occ_scale[int(batch.occ_ptr[t]):]):
            f = int(batch.fac_ptr[ob + rec]) + fac
            assert f < int(batch.fac_ptr[ob + rec + 1]) and batch.fac[f, 0] != FACTOR_FIXED
            assert (batch.fac[f, 2], batch.fac_val[f, 0], batch.fac_val[f, 1]) == (par.index, par.scale, par.offset)   # circuit order
            assert (index, scale) == (par.index, par.scale)
        for n_param, n_fac, n_gates, d in mbc.parameterised(batch, t):
            assert (n_fac == 0) == (n_param == 0), "a record without a parameter keeps its host matrix and has no factor list"
            assert n_fac <= n_gates + 1
            if c["noise"] is not None and n_fac:
                assert (n_param, n_fac) == (1, 1), "the noisy lowering fuses nothing"
    kinds = batch.fac[:-1, 0]
    fixed = np.flatnonzero(kinds == FACTOR_FIXED)
    for j in range(int(batch.ops.shape[0])):   # a FIXED factor is a MAXIMAL run of fixed gates: no two in a row
        run = kinds[int(batch.fac_ptr[j]):int(batch.fac_ptr[j + 1])]
        assert not np.any((run[1:] == FACTOR_FIXED) & (run[:-1] == FACTOR_FIXED))
    assert fixed.size == 0 or int(batch.fac[fixed, 3].max()) + 32 <= batch.fpool.shape[0]


def test_tfim_circuit_template_binds_to_tfim_circuit():
    for nq, steps, two_q in ((4, 3, "cx"), (12, 3, "cx"), (5, 2, "ecr"), (100, 1, "cx")):
        t = tfim_circuit_template(nq, steps, two_q)
        assert t.num_parameters == 2
        for j_coupling, h, dt in ((1.0, 0.66 * math.pi, 0.5), (1.9, 0.3, 0.25), (0.2, 1.1, 0.7)):
            assert t.bind_parameters([2 * h * dt, -2 * j_coupling * dt]).ops == tfim_circuit(nq, steps, j_coupling, h, dt, two_q).ops


def _shift_template():
    """All five kinds on a line of three qubits, several occurrences per parameter with different scales, fixed gates between."""
    ops = [CircuitOp("h", (0,)), CircuitOp("ry", (1,), (), (Param(0, 1.5, 0.1),)), CircuitOp("rx", (0,), (), (Param(1),)),
           CircuitOp("cx", (0, 1)), CircuitOp("rzz", (2, 1), (), (Param(0, -0.5),)), CircuitOp("rz", (2,), (), (Param(2, 2.0),)),
           CircuitOp("p", (0,), (), (Param(1, 0.75, -0.2),)), CircuitOp("h", (2,)), CircuitOp("u1", (1,), (), (Param(2),)),
           CircuitOp("cx", (2, 1)), CircuitOp("ry", (0,), (), (Param(2, -1.0, 0.3),)), CircuitOp("sx", (1,)),
           CircuitOp("rx", (2,), (), (Param(0),))]
    return Template(3, 0, ops, [], 3)


@pytest.mark.parametrize("noisy", [False, True])
def test_shift_rule_through_the_factor_program_against_central_differences(noisy):
    """The rule is exact, ideal and with the Pauli insertions held fixed (the same insertions in every run, as the device draws
    them from the row's key): central differences with h = 1e-5 agree to 1e-8, as in tests/test_bound_cpu.py."""
    t, terms = _shift_template(), [("ZIZ", 0.7), ("XXI", -0.4), ("IYZ", 0.5), ("ZZZ", 1.0)]
    lam = {(op.name, op.qubits): 0.02 + 0.01 * len(op.qubits) for op in t.ops}   # a depolarising op after every gate
    noise, traj = (sim.NoiseModel(lam), 1) if noisy else (None, None)
    batch = compile_mps_templates([t], [terms], noise, traj)
    row = np.array([0.37, -1.21, 0.83])
    forced = None
    if noisy:
        assert batch.n_noise[0] >= 8
        forced = [(3 * j + 1) % (16 if kind == 7 else 4) for j, kind in enumerate(k for k in batch.ops[:, 0] if k in (6, 7))]
        assert any(forced)

    def value(b):
        return mc.interpret(b, 0, forced=forced)["value"]

    runs, shift, groups = mps_shift_runs(batch, np.zeros(1, dtype=np.int64))
    k = int(batch.occ_ptr[1])
    assert runs.shape[0] == 1 + 2 * k and groups == [(0, groups[0][1], 0, k)]
    values = np.array([value(mbc.host_copy(batch, run, row[None, :], sh)) for run, sh in zip(runs, shift)])
    grad = bc.host_combine(values[1:1 + k].reshape(k, 1), values[1 + k:].reshape(k, 1), batch.occ_param, batch.occ_scale, 3)[0]
    h = 1e-5
    for p in range(3):
        e = np.zeros(3)
        e[p] = h
        plus, minus = (compile_mps([t.bind_parameters(row + s * e)], [terms], noise, traj) for s in (1.0, -1.0))
        central = (value(plus) - value(minus)) / (2 * h)
        assert abs(grad[p] - central) <= 1e-8, (p, grad[p], central)
    assert np.abs(grad).max() > 1e-3
    assert abs(values[0] - value(compile_mps([t.bind_parameters(row)], [terms], noise, traj))) <= 1e-13


@pytest.mark.parametrize("case_id", ALL)
def test_conditions_hold_on_the_bound_copies(case_id):
    units = [r for per in mbc.reference(case_id) for r in per]
    gap, cut, margin = min(r["gap"] for r in units), min(r["cut_margin"] for r in units), min(r["margin"] for r in units)
    print(f"{case_id}: gap {gap:.2e} cutoff factor {math.exp(min(cut, 700.0)):.3g} margin {margin:.2e}")
    assert gap >= mc.MIN_GAP
    assert cut >= math.log(mc.CUT_FACTOR)
    assert margin >= mc.MARGIN
    if case_id == "tfim-n12-s3-b4":
        assert all(not math.isinf(r["gap"]) and r["bond"] == 4 for r in units), "meant to truncate"
    elif mbc.case(case_id)["max_bond"] == 32:
        assert all(math.isinf(r["gap"]) for r in units), "meant to run without truncation"


def test_refusals_name_their_offender():
    rx = CircuitOp("rx", (0,), (), (Param(0),))
    far = Template(3, 0, [rx, CircuitOp("rzz", (0, 2), (), (Param(1),))])
    with pytest.raises(ValueError, match=r"circuit 1: op 1 \(rzz\): qubits 0 and 2 are not neighbours"):
        compile_mps_templates([Template(1, 0, [rx]), far], ["Z", "ZZZ"])
    with pytest.raises(ValueError, match=r"op 0 \(u3\) has a free parameter"):
        Template(1, 0, [CircuitOp("u3", (0,), (), (Param(0), 0.0, 0.0))])
    with pytest.raises(ValueError, match="compile_mps_templates: noise without trajectories"):
        compile_mps_templates([Template(1, 0, [rx])], ["Z"], mc.noise_model("depol", 11))
    with pytest.raises(ValueError, match="compile_mps_templates: trajectories without a noise model"):
        compile_mps_templates([Template(1, 0, [rx])], ["Z"], None, 4)
    with pytest.raises(ValueError, match=r"compile_mps_templates: max_bond = 64.*bond 64"):
        compile_mps_templates([Template(1, 0, [rx])], ["Z"], max_bond=64)
    with pytest.raises(ValueError, match="compile_mps_templates: 1 circuits but 2 observables"):
        compile_mps_templates([Template(1, 0, [rx])], ["Z", "Z"])
    with pytest.raises(ValueError, match="circuit 0: 513 qubits"):
        compile_mps_templates([Template(513, 0, [rx])], ["Z" * 513])
    t = Template(2, 0, [rx, CircuitOp("cx", (0, 1))])
    with pytest.raises(ValueError, match="bound_mps_expectation_values: row 0 has 2 parameter values, its template has 1"):
        sim.bound_mps_expectation_values(t, "ZZ", [[0.1, 0.2]], device="cpu")
    with pytest.raises(ValueError, match="parameter_shift: method = 'tensor'"):
        sim.parameter_shift(t, "ZZ", [[0.1]], method="tensor")
    with pytest.raises(ValueError, match="parameter_shift: trajectories, max_bond, cutoff and run_keys belong to method='mps'"):
        sim.parameter_shift(t, "ZZ", [[0.1]], max_bond=4)
    # the estimator: shots and the other wide methods refuse a template by name
    with pytest.raises(ValueError, match=r"method='mps'\): shots"):
        sim.DeviceEstimator(device="cpu", method="mps", shots=10)
    with pytest.raises(ValueError, match=r"template with free parameters and shots= is set"):
        sim.DeviceEstimator(device="cpu", method="mps").run([t], ["ZZ"], [[0.1]], shots=10)
    with pytest.raises(ValueError, match=r"circuit 0 is a template with free parameters and shots= is set"):
        sim.DeviceEstimator(device="cpu", method="mps_shots", shots=10).run([t], ["ZZ"], [[0.1]])
    with pytest.raises(ValueError, match=r"method='clifford'\): circuit 0 is a template with free parameters"):
        sim.DeviceEstimator(device="cpu", method="clifford").run([t], ["ZZ"], [[0.1]])
    with pytest.raises(ValueError, match="circuit 0 comes with 2 parameter values, the template has 1 parameters"):
        sim.DeviceEstimator(device="cpu", method="mps").run([t], ["ZZ"], [[0.1, 0.2]])
    with pytest.raises(ValueError, match=r"ZNEDeviceEstimator: circuit 0 is a template"):
        sim.zne.zne(sim.DeviceEstimator)(device="cpu", method="mps", noise=mc.noise_model("depol", 11), trajectories=2).run([t], ["ZZ"], [[0.1]])


def test_wide_ansatz_lowers_once():
    """A 100-qubit linear two_local: one lowering, 100-odd records, every parameter with one occurrence."""
    t = two_local(100, reps=1, entanglement="linear")
    batch = compile_mps_templates([t], [mc.single_z(100)])
    assert int(batch.occ_ptr[1]) == t.num_parameters == 200 and sorted(batch.occ_param.tolist()) == list(range(200))
    assert int(batch.op_ptr[1]) <= 200 and batch.ops[:, 0].tolist().count(5) >= 99
    for name in ("MpsBoundBatch", "MpsBoundRun", "bound_mps_expectation_values", "compile_mps_templates", "run_mps_bound"):
        assert name in sim.__all__ and hasattr(sim, name)


def test_abi_symbol_and_argument_checks():
    """mlqem_mps_bind_f64 is an additive symbol (the ABI number stays) and refuses bad arguments before anything is launched."""
    import ctypes

    from blackwater.native import _lib

    lib = _lib.load()
    assert _lib.ABI_VERSION == 48 and lib.mlqem_abi_version() == 48
    assert "mlqem_mps_bind_f64" in _lib.SIGNATURES and hasattr(lib, "mlqem_mps_bind_f64")
    OK, BAD, UNSUPPORTED = 0, -1, -2
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf) // 16 * 16 + 16   # a 16-byte aligned address that is never read: every call below returns before a launch

    def call(**kw):
        a = dict(n_templates=1, op_ptr=p, ops=p, n_ops=4, params=p, n_params=64, pool_ptr=p, fac_ptr=p, fac=p, fac_val=p, n_fac=2, fpool=p,
                 n_fpool=32, occ_ptr=p, occ=p, n_occ=1, theta=p, n_rows=1, ld_theta=1, runs=p, shift=p, n_runs=1, max_records=4, out_op_ptr=p,
                 out_pool_ptr=p, out_ops=p, n_out_ops=4, out_pool=p, n_out_pool=64)
        a.update(kw)
        return lib.mlqem_mps_bind_f64(*a.values(), None)

    assert call(n_runs=0) == OK and call(max_records=0) == OK, "nothing to do: nothing is launched"
    for bad in (dict(n_ops=-1), dict(n_params=31), dict(n_fpool=31), dict(n_out_pool=31), dict(n_fac=-1), dict(n_occ=-1), dict(n_runs=-1),
                dict(n_templates=0), dict(n_rows=0), dict(ld_theta=0), dict(op_ptr=None), dict(params=None), dict(pool_ptr=None),
                dict(fac_ptr=None), dict(fac=None), dict(fac_val=None), dict(fpool=None), dict(occ_ptr=None), dict(occ=None), dict(theta=None),
                dict(runs=None), dict(shift=None), dict(out_op_ptr=None), dict(out_pool_ptr=None), dict(out_ops=None), dict(out_pool=None),
                dict(ops=p + 4), dict(fac=p + 8), dict(runs=p + 4), dict(out_ops=p + 8), dict(out_pool=p + 4), dict(theta=p + 4)):
        assert call(**bad) == BAD, bad
    for big in (dict(n_params=2 ** 31), dict(n_out_pool=2 ** 31), dict(n_runs=2 ** 31), dict(n_fac=2 ** 31), dict(n_rows=2 ** 31)):
        assert call(**big) == UNSUPPORTED, big
