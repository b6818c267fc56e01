"""Zero-noise extrapolation, host side, no GPU: the fold rule, ``fold_circuit``, the schedules of every amplifier interpreted record
by record against the independent oracle of tests/zne_cases.py, the extrapolation weights, argument validation of the two new entry
points, the ``ops`` wrappers' refusals and the ``zne(cls)`` decorator around a host estimator."""
import math

import numpy as np
import pytest

import sim_cases as sc
import zne_cases as zc
from blackwater import sim, zne
from blackwater.data.circuit import Circuit, CircuitOp, circuit_to_qasm


def gates(names):
    return Circuit(3, 0, [CircuitOp(name, (0, 1) if name in sc.TWO_QUBIT else (k % 3,), (), tuple(0.1 * (j + 1) for j in range(sc.N_PARAMS.get(name, 0))))
                          for k, name in enumerate(names)])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def test_fold_counts_and_achieved_factors():
    assert zne.fold_counts(10, 1) == (0, 0) and zne.fold_counts(10, 3) == (1, 0) and zne.fold_counts(10, 5) == (2, 0)
    assert zne.fold_counts(10, 1.5) == (0, 3)      # floor(2.5 + 0.5)
    assert zne.fold_counts(10, 2.2) == (0, 6) and zne.fold_counts(4, 3.6) == (1, 1) and zne.fold_counts(3, 2) == (0, 2)
    assert zne.fold_counts(0, 7.5) == (0, 0) and zne.achieved_factor(0, 7.5) == 1.0
    assert zne.achieved_factor(10, 1.5) == 1.6 and zne.achieved_factor(10, 3) == 3.0 and zne.achieved_factor(4, 3.6) == 3.5
    for bad in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise factor"):
            zne.fold_counts(4, bad)
    for n in range(0, 7):
        for lam in (1, 1.3, 2, 2.9, 3, 4.4):
            assert zne.fold_counts(n, lam) == zc.counts(n, lam)[1:]


def names_of(circuit):
    return [op.name for op in circuit.ops]


def test_sub_folding_options_and_gate_selection():
    c = gates(["h", "cx", "barrier", "sx", "cz", "rz", "measure"])
    c.ops[2] = CircuitOp("barrier", (0, 1, 2))
    c.ops[6] = CircuitOp("measure", (0,), (0,))
    c.num_clbits = 1
    # 5 gates, factor 1.8: m = 2 -> the first two / the last two once
    first = zne.fold_circuit(c, 1.8, zne.LocalFoldingAmplifier())
    assert names_of(first) == ["h", "h", "h", "cx", "cx", "cx", "barrier", "sx", "cz", "rz", "measure"]
    last = zne.fold_circuit(c, 1.8, zne.LocalFoldingAmplifier(sub_folding_option="from_last"))
    assert names_of(last) == ["h", "cx", "barrier", "sx", "cz", "cz", "cz", "rz", "rz", "rz", "measure"]
    assert last.ops[8].params == (-0.1,) and last.ops[7].params == last.ops[9].params == (0.1,)
    rnd = zne.fold_circuit(c, 1.8, zne.LocalFoldingAmplifier(sub_folding_option="random", random_seed=3))
    pick = sorted(np.random.default_rng(3).choice(5, size=2, replace=False).tolist())
    want = []
    gate_names = ["h", "cx", "sx", "cz", "rz"]
    for op in c.ops:
        if op.name in ("barrier", "measure"):
            want.append(op.name)
            continue
        g = gate_names.index(op.name)
        inv = {"sx": "sxdg"}.get(op.name, op.name)
        want += [op.name, inv, op.name] if g in pick else [op.name]
    assert names_of(rnd) == want
    again = zne.fold_circuit(c, 1.8, zne.LocalFoldingAmplifier(sub_folding_option="random", random_seed=3))
    assert names_of(again) == names_of(rnd)
    # gate selection: two-qubit gates, one name, a mixed list; N = 0 leaves the circuit alone at any factor
    two = zne.fold_circuit(c, 3, zne.TwoQubitAmplifier())
    assert names_of(two) == ["h", "cx", "cx", "cx", "barrier", "sx", "cz", "cz", "cz", "rz", "measure"]
    assert names_of(zne.fold_circuit(c, 3, zne.CxAmplifier())) == ["h", "cx", "cx", "cx", "barrier", "sx", "cz", "rz", "measure"]
    mixed = zne.fold_circuit(c, 3, zne.LocalFoldingAmplifier(gates_to_fold=["sx", "cz"]))
    assert names_of(mixed) == ["h", "cx", "barrier", "sx", "sxdg", "sx", "cz", "cz", "cz", "rz", "measure"]
    assert names_of(zne.fold_circuit(c, 9, zne.LocalFoldingAmplifier(gates_to_fold="ecr"))) == names_of(c)
    # global: U (U^-1 U)^k L^-1 L, the extra passes after the last gate, before the measure
    glob = zne.fold_circuit(c, 3.4, zne.GlobalFoldingAmplifier())   # m = 6: k = 1, s = 1
    assert names_of(glob) == (["h", "cx", "barrier", "sx", "cz", "rz"] + ["rz", "cz", "sxdg", "cx", "h"] + ["h", "cx", "sx", "cz", "rz"]
                              + ["rz", "rz"] + ["measure"])
    gfirst = zne.fold_circuit(c, 1.8, zne.GlobalFoldingAmplifier("from_first"))   # m = 2: k = 0, s = 2: L = (h, cx)
    assert names_of(gfirst) == ["h", "cx", "barrier", "sx", "cz", "rz", "cx", "h", "h", "cx", "measure"]
    with pytest.raises(ValueError, match="sub_folding_option"):
        zne.GlobalFoldingAmplifier("random")
    with pytest.raises(ValueError, match="gates_to_fold"):
        zne.LocalFoldingAmplifier(gates_to_fold="measure")


ALL_DESCS = [zc.LOCAL_ALL, zc.LOCAL_2Q, zc.LOCAL_RANDOM, zc.GLOBAL, zc.GLOBAL_FIRST, ("local", "cx", "from_first", None),
             ("local", ["sx", 2], "random", 11)]


@pytest.mark.parametrize("desc", ALL_DESCS, ids=[str(d) for d in ALL_DESCS])
def test_fold_circuit_equals_the_independent_fold(desc):
    c = sc.random_program(4, 25, seed=40, measure=True)
    for lam in (1, 1.3, 2.2, 3, 4.6):
        got = zne.fold_circuit(c, lam, zc.make_amplifier(desc))
        want, _, _ = zc.fold_ir(c, lam, desc)
        assert [(o.name, o.qubits, o.clbits) for o in got.ops] == [(o.name, o.qubits, o.clbits) for o in want.ops], lam
        assert all(np.allclose(a.params, b.params, rtol=0, atol=0) for a, b in zip(got.ops, want.ops))


@pytest.mark.parametrize("name", sc.ONE_QUBIT + sc.TWO_QUBIT)
def test_fold_circuit_preserves_the_unitary(name):
    """gate, inverse, gate on a random state: the full noiseless state against the unfolded circuit's, at 1e-12, with the oracle's
    matrices (a wrong inverse by name would show here)."""
    rng = np.random.default_rng(7)
    n = 3
    qubits = (2, 0) if name in sc.TWO_QUBIT else (1,)
    params = tuple(float(v) for v in rng.uniform(-3, 3, size=sc.N_PARAMS.get(name, 0)))
    prep = [CircuitOp("u3", (q,), (), tuple(float(v) for v in rng.uniform(-3, 3, size=3))) for q in range(n)] + [CircuitOp("cx", (0, 1)), CircuitOp("cx", (1, 2))]
    c = Circuit(n, 0, prep + [CircuitOp(name, qubits, (), params)])
    folded = zne.fold_circuit(c, 3, zne.LocalFoldingAmplifier(gates_to_fold=name))
    if name not in ("u3", "cx"):
        assert len(folded.ops) == len(c.ops) + 2
    folded_global = zne.fold_circuit(c, 3, zne.GlobalFoldingAmplifier())
    assert len(folded_global.ops) == 3 * len(c.ops)

    def state(circuit):
        psi = np.zeros(2 ** n, dtype=complex)
        psi[0] = 1.0
        for op in circuit.ops:
            psi = sc.apply(sc.gate_matrix(op.name, op.params), list(op.qubits), psi, n)
        return psi

    want = state(c)
    assert np.abs(state(folded) - want).max() < 1e-12 and np.abs(state(folded_global) - want).max() < 1e-12
    assert circuit_to_qasm(folded).count("\n") == len(folded.ops) + 3


# ---- the schedules ----------------------------------------------------------------------------------------------------------------------
def check_schedules(circuits, observables, noise, factors, desc, degrees=zc.DEGREES, what=""):
    """The package's schedules, expanded and interpreted on the host, against the oracle; returns the largest bound."""
    batch = sim.compile_programs(circuits, observables, noise)
    sch = zne.build_schedules(batch, circuits, factors, zc.make_amplifier(desc))
    n_circ, worst = len(circuits), 0.0
    assert sch.sched_ptr.shape == (len(factors) * n_circ + 1,) and sch.sched.dtype == np.int32 and sch.sched_ptr[-1] == sch.sched.shape[0]
    assert sorted(sch.ids.tolist()) == list(range(len(factors) * n_circ)) and sch.n_wave + sch.n_wg == len(factors) * n_circ
    refs = [zc.oracle(c, o, noise, factors, desc, degrees[0]) for c, o in zip(circuits, observables)]
    got_values = np.zeros((len(factors), n_circ))
    got_terms = [np.zeros((len(factors), len(o))) for o in observables]
    for f in range(len(factors)):
        plain = zc.expand(batch, sch, f)
        for k in range(n_circ):
            value, tv, norm = sc.interpret(plain, k)
            ref = refs[k]
            assert sch.achieved[f, k] == ref["achieved"][f], (what, f, k)
            assert abs(value - ref["values"][f]) <= ref["value_bounds"][f], (what, f, k)
            assert len(tv) == 0 or np.abs(tv - ref["term_values"][f]).max() <= ref["term_bounds"][f], (what, f, k)
            assert abs(norm - 1.0) <= ref["term_bounds"][f] and abs(ref["norm"][f] - 1.0) <= ref["term_bounds"][f]
            got_values[f, k] = value
            got_terms[k][f] = tv
    for degree in degrees:
        ex = zne.PolynomialExtrapolator(degree)
        for k, (c, o) in enumerate(zip(circuits, observables)):
            ref = zc.oracle(c, o, noise, factors, desc, degree)
            assert ref["mitigated_value_bound"] < zc.CAP and (ref["mitigated_term_bound"] < zc.CAP).all(), (what, degree, ref["mitigated_value_bound"])
            worst = max(worst, ref["mitigated_value_bound"])
            mit = ex.extrapolate(factors, got_values[:, k])
            assert abs(mit - ref["mitigated_value"]) <= ref["mitigated_value_bound"], (what, degree, k)
            if len(o):
                mt = ex.extrapolate(factors, got_terms[k])
                assert (np.abs(mt - ref["mitigated_terms"]) <= ref["mitigated_term_bound"]).all(), (what, degree, k)
    return worst


@pytest.mark.parametrize("case", zc.density_cases(), ids=[c[0] for c in zc.density_cases()])
def test_density_grid_schedules_against_the_oracle(case):
    """Every case of the device's density grid: the bound stays below the cap of 1e-10 (a condition on the cases), and the
    schedule, expanded to a plain program with the daggers applied in numpy and interpreted record by record, meets the oracle."""
    _, n, desc, factors = case
    c, terms, noise = zc.density_program(n)
    worst = check_schedules([c], [terms], noise, factors, desc, what=case[0])
    print(f"{case[0]}: largest mitigated-value bound {worst:.3e} < {zc.CAP:.0e}")
    batch = sim.compile_programs([c], [terms], noise)
    lam = [batch.params[p] for kind, _, _, p in batch.ops.tolist() if kind in (sim.program.OP_DEPOL1, sim.program.OP_DEPOL2)]
    assert 0.0 in lam and 1.0 in lam and len(lam) == zc.N_OPS + 1 and "id" in [op.name for op in c.ops]


@pytest.mark.parametrize("n", [1, 3, 8])
def test_vector_grid_schedules_against_the_oracle(n):
    """The vector cases (the 9- and 11-qubit ones are left to the device: the host interpreter of tests/sim_cases.py walks 2^n
    entries in Python) with global folding at 3 and 5, against the oracle and against the unfolded value (U^-1 U = 1)."""
    c, terms = zc.vector_program(n)
    check_schedules([c], [terms], None, (1, 3, 5), zc.GLOBAL, what=f"vector n={n}")
    ref = zc.oracle(c, terms, None, (1, 3, 5), zc.GLOBAL, 1)
    for f in (1, 2):
        assert abs(ref["values"][f] - ref["values"][0]) <= ref["value_bounds"][f] + ref["value_bounds"][0]


@pytest.mark.parametrize("n", [9, 11])
def test_large_vector_cases_keep_the_cap(n):
    c, terms = zc.vector_program(n)
    for degree in zc.DEGREES:
        ref = zc.oracle(c, terms, None, (1, 3, 5), zc.GLOBAL, degree)
        assert ref["mitigated_value_bound"] < zc.CAP and (ref["mitigated_term_bound"] < zc.CAP).all()


@pytest.mark.parametrize("n", zc.READOUT_N)
@pytest.mark.parametrize("desc,factors", [(zc.LOCAL_ALL, (1, 3)), (zc.GLOBAL, zc.PARTIAL)], ids=["local", "global-partial"])
def test_readout_records_follow_every_schedule_once(n, desc, factors):
    c, terms, noise = zc.readout_program(n)
    check_schedules([c], [terms], noise, factors, desc, degrees=(1,), what=f"readout n={n}")
    batch = sim.compile_programs([c], [terms], noise)
    sch = zne.build_schedules(batch, [c], factors, zc.make_amplifier(desc))
    n_rec = int(batch.op_counts[0])
    for r in range(len(factors)):
        tail = sch.sched[int(sch.sched_ptr[r + 1]) - n:int(sch.sched_ptr[r + 1])]
        assert tail.tolist() == [(n_rec - n + j) << 1 for j in range(n)]
        body = sch.sched[int(sch.sched_ptr[r]):int(sch.sched_ptr[r + 1]) - n] >> 1
        assert (body < n_rec - n).all()


def test_schedules_of_a_mixed_batch_and_the_identity_schedule():
    """Circuits of different sizes, one without gates, one of ``id`` alone (noise records only), both variants: factor 1 gives the
    identity schedule 0, 2, 4, ...; N = 0 gives it at every factor; run numbers put the wave-per-circuit runs first."""
    noise = sc.StepNoise(33, force=False)
    circuits = [sc.random_program(2, 6, seed=41), Circuit(1, 0, []), Circuit(2, 0, [CircuitOp("id", (0,)), CircuitOp("id", (1,))]),
                sc.random_program(5, 4, seed=42), Circuit(3, 0, [CircuitOp("h", (0,)), CircuitOp("t", (1,))])]
    obs = [sc.term_set(c.num_qubits) for c in circuits]
    batch = sim.compile_programs(circuits, obs, noise)
    assert batch.gate_ptr.tolist() == [0, 6, 6, 8, 12, 14] and batch.gate_record[6:8].tolist() == [-1, -1] and batch.gate_noise[6:8].tolist() == [0, 1]
    sch = zne.build_schedules(batch, circuits, (1, 3), zne.TwoQubitAmplifier())
    for k in range(5):
        ident = (np.arange(int(batch.op_counts[k])) << 1).tolist()
        assert sch.sched[int(sch.sched_ptr[k]):int(sch.sched_ptr[k + 1])].tolist() == ident
        if k in (1, 2, 4):   # no two-qubit gate: unchanged at factor 3, achieved factor 1
            assert sch.sched[int(sch.sched_ptr[5 + k]):int(sch.sched_ptr[6 + k])].tolist() == ident and sch.achieved[1, k] == 1.0
    assert sch.ids.tolist() == [0, 1, 2, 4, 5, 6, 7, 9, 3, 8] and (sch.n_wave, sch.n_wg) == (8, 2)
    check_schedules(circuits, obs, noise, (1, 2.5, 3), zc.LOCAL_ALL, what="mixed batch")
    with pytest.raises(ValueError, match="3 circuits"):
        zne.build_schedules(batch, circuits[:3], (1, 3), zne.TwoQubitAmplifier())


# ---- the weights ------------------------------------------------------------------------------------------------------------------------
def test_extrapolation_weights():
    w = zne.LinearExtrapolator().weights((1, 3))
    assert w.tolist() == [1.5, -0.5]
    assert zne.ZNEStrategy().weights().tolist() == [1.5, -0.5]
    rng = np.random.default_rng(0)
    cases = [(zne.LinearExtrapolator(), 1, (1, 3, 5)), (zne.QuadraticExtrapolator(), 2, (1, 3, 5)), (zne.QuadraticExtrapolator(), 2, zc.PARTIAL),
             (zne.CubicExtrapolator(), 3, (1, 1.5, 2, 2.5, 3)), (zne.QuarticExtrapolator(), 4, (1, 2, 3, 4, 5)),
             (zne.PolynomialExtrapolator(2), 2, (1, 1.2, 2.2, 3, 4)), (zne.RichardsonExtrapolator(), 3, (1, 2, 3, 4)), (zne.RichardsonExtrapolator(), 1, (1, 3))]
    for ex, degree, factors in cases:
        w = ex.weights(factors)
        x = np.asarray(factors, dtype=np.float64)
        scale = np.abs(w).sum()
        assert abs(w.sum() - 1.0) <= 1e-12 * scale, (ex, factors)
        coeffs = rng.uniform(-1, 1, size=degree + 1)
        y = np.polyval(coeffs, x)
        assert abs(w @ y - coeffs[-1]) <= 1e-12 * scale, (ex, factors)          # a polynomial of the degree returns p(0)
        noise = rng.uniform(-1, 1, size=x.size)
        assert abs(w @ noise - np.polyfit(x, noise, degree)[-1]) <= 1e-12 * scale, (ex, factors)
        assert np.allclose(w, zc.polyfit_weights(factors, degree), rtol=0, atol=1e-12 * scale)
        assert abs(ex.extrapolate(factors, np.stack([y, noise], axis=1))[0] - coeffs[-1]) <= 1e-12 * scale


@pytest.mark.parametrize("what,call", [
    ("too few", lambda: zne.QuadraticExtrapolator().weights((1, 3))),
    ("too few for the strategy", lambda: zne.ZNEStrategy(noise_factors=(1,))),
    ("richardson one", lambda: zne.RichardsonExtrapolator().weights((1,))),
    ("repeated", lambda: zne.LinearExtrapolator().weights((1, 3, 3))),
    ("below one", lambda: zne.LinearExtrapolator().weights((0.5, 3))),
    ("nan", lambda: zne.LinearExtrapolator().weights((1, float("nan")))),
    ("inf", lambda: zne.LinearExtrapolator().weights((1, float("inf")))),
    ("degree", lambda: zne.PolynomialExtrapolator(0)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_extrapolators_refuse(what, call):
    with pytest.raises(ValueError):
        call()


# ---- the C ABI and the wrappers -------------------------------------------------------------------------------------------------------
def test_new_entry_points_validate_arguments_without_a_device():
    """Argument validation happens before any launch, so it runs without a device.  One real buffer serves for every pointer."""
    import ctypes

    from blackwater.native import _lib

    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    bad, unsupported = -1, _lib.ERR_UNSUPPORTED

    def folded(b=2, f=3, n_ops=4, n_params=64, n_terms=2, n_sched=8, n_wave=6, n_wg=0, circ=p, sched_ptr=p, sched=p, ids=p, values=p, ops=p):
        return lib.mlqem_sim_run_folded_f64(b, f, circ, p, ops, n_ops, p, n_params, p, p, p, n_terms, sched_ptr, sched, n_sched, ids, n_wave, n_wg,
                                            p, values, p, None)

    assert folded(b=-1) == bad and folded(f=0) == bad and folded(f=-2) == bad and folded(n_ops=-1) == bad and folded(n_terms=-1) == bad
    assert folded(n_sched=-1) == bad and folded(n_wave=-1) == bad and folded(n_wg=-1) == bad and folded(n_params=31) == bad
    assert folded(n_wave=7) == bad                                  # more runs than F * B
    assert folded(circ=None) == bad and folded(sched_ptr=None) == bad and folded(sched=None) == bad and folded(ids=None) == bad
    assert folded(values=None) == bad and folded(ops=None) == bad
    assert folded(circ=p + 4) == bad and folded(ops=p + 8) == bad and folded(sched_ptr=p + 4) == bad and folded(sched=p + 2) == bad
    assert folded(b=2 ** 30, f=4) == unsupported and folded(n_sched=2 ** 31) == unsupported and folded(b=2 ** 31) == unsupported
    assert folded(n_wave=0, n_wg=0) == 0                            # nothing to run: MLQEM_OK without a launch

    def combine(f=3, b=2, n_terms=4, tv=p, w=p, term_ptr=p, coeff=p, mt=p, mv=p):
        return lib.mlqem_zne_combine_f64(f, b, tv, w, term_ptr, coeff, n_terms, mt, mv, None)

    assert combine(f=0) == bad and combine(b=-1) == bad and combine(n_terms=-1) == bad
    assert combine(w=None) == bad and combine(tv=None) == bad and combine(term_ptr=None) == bad and combine(mt=None) == bad and combine(mv=None) == bad
    assert combine(coeff=None) == bad
    assert combine(b=2 ** 31) == unsupported and combine(n_terms=2 ** 31) == unsupported and combine(f=2 ** 31) == unsupported
    assert combine(b=0, n_terms=0) == 0


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    import torch

    from blackwater.native import _lib, ops

    c, terms, noise = zc.density_program(2)
    batch = sim.compile_programs([c], [terms], noise)
    sch = zne.build_schedules(batch, [c], (1, 3), zne.LocalFoldingAmplifier())
    t, s = batch.to("cpu"), sch.to("cpu")
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.sim_run_folded(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], s["sched_ptr"], s["sched"],
                           s["ids"], sch.n_wave, sch.n_wg, 2)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.zne_combine(torch.zeros(2, 12, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), t["term_ptr"], t["coeff"])


# ---- the decorator around a host estimator ----------------------------------------------------------------------------------------------
class OracleEstimator:
    """A host estimator on the numpy oracle with the ``_run`` protocol: the noise is looked up BY NAME in the folded circuit."""

    def __init__(self, noise=None):
        self._noise, self.calls = noise, []

    def run(self, circuits, observables, parameter_values=None, **run_options):
        circuits = list(circuits)
        return self._run(circuits, list(observables), list(parameter_values or [()] * len(circuits)), **run_options)

    def _run(self, circuits, observables, parameter_values, **run_options):
        self.calls.append((len(circuits), dict(run_options)))
        from blackwater.data.backends import pauli_terms

        values = np.asarray([sc.simulate(Circuit.from_any(c), list(pauli_terms(o)), self._noise)[0] for c, o in zip(circuits, observables)])
        return sim.SimulatedJob(values, f"oracle-{len(self.calls)}")


def test_zne_decorator_around_a_host_estimator():
    """Two-qubit local folding of cx / cz / swap / ecr / rzz: there the by-name noise of a host estimator and the fold-unit rule
    agree, so the generic path must reproduce the oracle's mitigated values (same folds, same weights)."""
    lam = {(g, pair): 0.02 + 0.01 * j for j, g in enumerate(sc.TWO_QUBIT) for pair in ((0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0))}
    noise = sim.NoiseModel(lam)
    circuits = [sc.random_program(3, 12, seed=50 + k) for k in range(3)]
    obs = [sc.term_set(3, seed=k) for k in range(3)]
    cls = zne.zne(OracleEstimator)
    assert cls.__name__ == "ZNEOracleEstimator"
    est = cls(noise, zne_strategy=zne.ZNEStrategy(noise_factors=(1, 3, 5), extrapolator=zne.QuadraticExtrapolator()))
    res = est.run(circuits, obs, shots=7).result()
    assert est.calls == [(9, {"shots": 7})]                         # F * B circuits in ONE job of the wrapped estimator
    for k, (c, o) in enumerate(zip(circuits, obs)):
        ref = zc.oracle(c, o, noise, (1, 3, 5), zc.LOCAL_2Q, 2)
        assert ref["mitigated_value_bound"] < zc.CAP and abs(res.values[k] - ref["mitigated_value"]) <= ref["mitigated_value_bound"]
        meta = res.metadata[k]["zne"]
        assert meta["noise_factors"] == (1.0, 3.0, 5.0) and meta["achieved_factors"] == tuple(ref["achieved"])
        assert np.abs(np.asarray(meta["values"]) - ref["values"]).max() <= ref["value_bounds"].max()
    # a strategy given as a run option wins over the constructor's
    res2 = est.run(circuits, obs, zne_strategy=zne.ZNEStrategy()).result()
    for k, (c, o) in enumerate(zip(circuits, obs)):
        ref = zc.oracle(c, o, noise, (1, 3), zc.LOCAL_2Q, 1)
        assert abs(res2.values[k] - ref["mitigated_value"]) <= ref["mitigated_value_bound"]
        assert res2.metadata[k]["zne"]["noise_factors"] == (1.0, 3.0)
    assert est.calls[-1] == (6, {})


def test_zne_processor_runs_the_estimator_once_per_run():
    from blackwater.data.backends import PauliObservable
    from blackwater.library.learning.estimator import ZNEProcessor, learning

    noise = sim.NoiseModel({("cx", (0, 1)): 0.05, ("cx", (1, 0)): 0.05})
    circuits = [Circuit(2, 0, [CircuitOp("h", (0,)), CircuitOp("cx", (0, 1)), CircuitOp("ry", (1,), (), (0.3 * (k + 1),))]) for k in range(4)]
    obs = [PauliObservable("ZZ"), PauliObservable([("XX", 0.5), ("ZI", -1.0)]), PauliObservable("IZ"), PauliObservable("YY")]
    inner = zne.zne(OracleEstimator)(noise)
    strategy = zne.ZNEStrategy()
    proc = ZNEProcessor(inner, strategy, backend=None, shots=100)
    job = learning(OracleEstimator, proc, skip_transpile=True)(noise).run(circuits, obs)
    out = job.result()
    assert inner.calls == [(8, {"shots": 100})]
    for k, (c, o) in enumerate(zip(circuits, obs)):
        ref = zc.oracle(c, o.to_list(), noise, (1, 3), zc.LOCAL_2Q, 1)
        assert abs(out.values[k] - ref["mitigated_value"]) <= ref["mitigated_value_bound"]
        assert abs(out.metadata[k]["original_value"] - ref["values"][0]) <= ref["value_bounds"][0]
        one = proc.process(0.0, c, o, ())
        assert abs(one - ref["mitigated_value"]) <= ref["mitigated_value_bound"]
