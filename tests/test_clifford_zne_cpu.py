"""Zero-noise extrapolation at width, on the host: inverse tables, the Clifford schedules against the folded IR, the folded
interpreter against the plain one, the closed form ideal * F1 * F2^x, the exponential extrapolator, the conditions on the cases of
tests/test_gpu_clifford_zne.py, and the refusals.  No GPU."""
import itertools
import math

import numpy as np
import pytest

import clifford_cases as cc
import clifford_zne_cases as czc
import sim_cases as sc
import zne_cases as zc
from blackwater import sim, zne
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.sim.clifford import gate_table, invert_table

ANGLES = [k * math.pi / 2 for k in range(-4, 5)]   # what clifford_cases.random_clifford_op draws


# ---- 1. inverse tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CLIFFORD_ONE + cc.CLIFFORD_TWO)
def test_invert_table_is_the_table_of_the_inverse_gate(name):
    qubits = (0, 1) if name in cc.CLIFFORD_TWO else (0,)
    seen = 0
    for params in itertools.product(ANGLES, repeat=sc.N_PARAMS.get(name, 0)):
        table = gate_table(name, tuple(params))
        assert table is not None, (name, params)
        inv = zne.inverse_op(CircuitOp(name, qubits, (), tuple(params)))
        assert invert_table(table) == gate_table(inv.name, tuple(inv.params)), (name, params)
        assert invert_table(invert_table(table)) == table
        seen += 1
    assert seen == len(ANGLES) ** sc.N_PARAMS.get(name, 0)
    assert invert_table("id") == "id" and gate_table("id", ()) == "id"


def test_invert_table_refuses_what_is_no_permutation():
    with pytest.raises(ValueError, match="no permutation"):
        invert_table((0o111, 0, 0))
    with pytest.raises(ValueError, match="no permutation"):
        invert_table((0x11111111, 0x01111111, 0))


# ---- 2. schedules against folded IR ----------------------------------------------------------------------------------------------------
def schedule_circuits():
    """Random Clifford programs with an ``id`` put in, measured; one wide grid circuit; one circuit without gates."""
    out = []
    for n in (1, 2, 5):
        c = cc.random_clifford_program(n, 10, 60 + n, measure=True)
        c.ops.insert(5, CircuitOp("id", (n - 1,)))
        out.append(c)
    out.append(czc.grid_circuit(100, 40, 1))
    out.append(Circuit(3, 0, []))
    return out


def z_terms(n, seed):
    return cc.random_terms(n, 3, seed, alphabet="IZ", weight=3)


@pytest.fixture(scope="module")
def lowered():
    circuits = schedule_circuits()
    obs = [z_terms(c.num_qubits, k) for k, c in enumerate(circuits)]
    noise = sc.StepNoise(31, readout={0: (0.02, 0.05)})
    return circuits, obs, noise, sim.compile_clifford(circuits, obs, noise)


@pytest.mark.parametrize("name", sorted(czc.AMPLIFIERS))
def test_schedules_equal_the_folded_ir_record_for_record(lowered, name):
    circuits, obs, noise, batch = lowered
    desc = czc.AMPLIFIERS[name]
    sch = zne.build_clifford_schedules(batch, zc.PARTIAL, zc.make_amplifier(desc))
    n_circ = len(circuits)
    assert sch.sched_ptr.dtype == np.int64 and sch.sched_ptr.shape == (len(zc.PARTIAL) * n_circ + 1,) and sch.sched.dtype == np.int32
    assert sch.n_wave == 0 and sch.n_wg == 0 and sch.ids.size == 0
    for f, lam in enumerate(zc.PARTIAL):
        got = czc.expand(batch, sch, f)
        for c, circ in enumerate(circuits):   # one lowering per folded circuit: its noise is keyed by ITS positions
            folded, source, achieved = zc.fold_ir(circ, lam, desc)
            want = sim.compile_clifford([folded], [obs[c]], zc.PositionNoise(noise, circ, source))
            mine = got.ops[int(got.op_ptr[c]):int(got.op_ptr[c + 1])]
            assert mine.shape == want.ops.shape, (name, lam, c)
            depol = np.isin(mine[:, 0] & 15, (cc.DEPOL1, cc.DEPOL2))
            assert np.array_equal(mine[:, 0], want.ops[:, 0]) and np.array_equal(mine[~depol], want.ops[~depol]), (name, lam, c)
            assert np.array_equal(got.pool[mine[depol, 1].astype(np.int64)], want.pool[want.ops[depol, 1].astype(np.int64)])
            assert sch.achieved[f, c] == achieved
    assert (sch.sched & 1).any() and np.diff(sch.sched_ptr)[:n_circ].tolist() == np.diff(batch.op_ptr).tolist()   # factor 1: as lowered


# ---- 3. interpreter against interpreter --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(czc.AMPLIFIERS))
def test_the_folded_interpreter_equals_the_plain_one_on_the_written_out_run(lowered, name):
    circuits, obs, noise, batch = lowered
    sch = zne.build_clifford_schedules(batch, zc.PARTIAL, zc.make_amplifier(czc.AMPLIFIERS[name]))
    got = czc.interpret_folded(batch, sch)
    for f in range(len(zc.PARTIAL)):
        want = cc.interpret(czc.expand(batch, sch, f))
        for g, w in zip(got, want):
            assert np.array_equal(g[f], w), (name, f)
    assert len(np.unique(got[1], axis=0)) > 1                      # the noise is amplified
    assert all(np.array_equal(got[k][0], got[k][f]) for k in (0, 2, 4) for f in range(1, len(zc.PARTIAL)))   # folding is the identity


def test_a_malformed_schedule_or_table_is_clamped_not_followed(lowered):
    circuits, obs, noise, batch = lowered
    sch = zne.build_clifford_schedules(batch, (1, 3), zne.GlobalFoldingAmplifier())
    import dataclasses

    bad = dataclasses.replace(sch, sched=np.where(np.arange(sch.sched.size) % 5 == 0, -7, sch.sched + (1 << 20)).astype(np.int32),
                              sched_ptr=sch.sched_ptr + np.arange(sch.sched_ptr.size) % 3 * 1000 - 500)
    out = czc.interpret_folded(batch, bad)
    assert all(np.isfinite(x).all() for x in out)
    assert czc._find((0o111, 0, 0), cc.C1, 2) == 0 and czc._find((0, 0, 0), cc.C2, 5) == 0
    assert czc._find((0, 0x50000000, 0), cc.C2, 5) == 14          # a match in the sixteenth nibble: the table's last entry


# ---- 4. the closed form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in czc.CLOSED if c[1] in (5, 100)], ids=lambda c: c[0])
def test_noisy_values_follow_the_closed_form_and_the_exponential_fit_recovers_it(case):
    _, n, desc = case
    k = czc.closed_case(n, desc)
    got = czc.interpret_folded(k["batch"], k["sch"])
    unit_ideal, unit_noisy, noisy_terms = got[4], got[5], got[3]
    amplified = k["f2"] < 1.0   # under two-qubit folding a unit may meet no folded gate: its value is then the same at every factor
    assert (np.abs(k["ideal"]) == 1.0).all() and amplified.sum() >= 3 and (amplified.all() or desc == zc.LOCAL_2Q)
    assert all(np.array_equal(unit_ideal[f], k["ideal"]) for f in range(len(czc.ODD)))
    assert np.array_equal(k["sch"].achieved, np.repeat(np.asarray(czc.ODD, dtype=np.float64)[:, None], 1, axis=1))
    assert (np.abs(unit_noisy - k["ref"]) <= k["bounds"]).all()
    assert (np.abs(unit_noisy[0] - unit_noisy[2])[amplified] > 1e-3).all()    # the factors differ by far more than any bound
    order = k["batch"].comb_unit   # no readout: term t is unit comb_unit[t] with weight 1
    values, terms, fallback = zne.ExponentialExtrapolator().extrapolate_terms(czc.ODD, noisy_terms, k["batch"].term_ptr, k["batch"].coeff)
    assert not fallback.any()
    assert (np.abs(terms - k["fit_ref"][order]) <= k["fit_bound"][order]).all()
    if desc in (zc.GLOBAL, zc.LOCAL_ALL):
        assert (k["f1"] == 1.0).all() and (np.abs(terms - k["ideal"][order]) <= k["fit_bound"][order]).all()
    else:
        assert (k["f1"] < 1.0).any()
    coeff = k["batch"].coeff
    vb = (np.abs(coeff) * k["fit_bound"][order]).sum() + (len(coeff) + 1) * czc.U * np.abs(coeff * k["fit_ref"][order]).sum()
    assert abs(values[0] - float((coeff * k["fit_ref"][order]).sum())) <= vb
    # a straight line leaves what the exponential removes
    lin = zne.LinearExtrapolator().extrapolate(czc.ODD, noisy_terms)
    assert np.abs(lin - k["fit_ref"][order]).max() > 1e3 * k["fit_bound"].max()


# ---- 5. the extrapolator ---------------------------------------------------------------------------------------------------------------
def test_exponential_extrapolator_cases():
    ex = zne.ExponentialExtrapolator()
    f = (1, 3, 5)
    w = zne.LinearExtrapolator().weights(f)
    assert np.array_equal(ex.weights(f), w)
    tv = np.array([[0.5, -0.5, 0.0, 0.4, 0.3, 0.0], [0.25, -0.25, 0.0, -0.2, 0.0, 0.1], [0.125, -0.125, 0.0, 0.1, 0.2, 0.0]]) * 0.9
    ptr, coeff = np.array([0, 3, 6]), np.array([1.0, 2.0, 3.0, 1.0, -1.0, 0.5])
    values, terms, fallback = ex.extrapolate_terms(f, tv, ptr, coeff)
    assert fallback.tolist() == [0, 0, 0, 1, 1, 1] and fallback.dtype == np.int32
    a = 0.9 * 0.5 * math.sqrt(2.0)                    # A r^x through 0.45, 0.225, 0.1125 at x = 1, 3, 5: r = 1 / sqrt 2
    assert abs(terms[0] - a) <= 64 * czc.U and terms[1] == -terms[0] and terms[2] == 0.0
    lin = zne.LinearExtrapolator().extrapolate(f, tv)
    assert np.array_equal(terms[3:], lin[3:])          # the fallback IS the straight line
    assert values[0] == 1.0 * terms[0] + 2.0 * terms[1] + 3.0 * terms[2]
    assert values[1] == (np.float64(0.0) + 1.0 * terms[3] + -1.0 * terms[4]) + 0.5 * terms[5]
    assert np.array_equal(ex.extrapolate(f, tv), terms) and repr(ex) == "ExponentialExtrapolator()"
    for bad in ((1,), (1, 1), (3, 3, 3)):
        with pytest.raises(ValueError, match="noise factor"):
            ex.weights(bad)
    with pytest.raises(ValueError, match="noise factor"):
        zne.ZNEStrategy(noise_factors=(2, 2), extrapolator=zne.ExponentialExtrapolator())
    assert zne.ZNEStrategy(noise_factors=(1, 3, 5), extrapolator=ex).weights().shape == (3,)


def test_generic_zne_path_takes_the_exponential_extrapolator():
    """Around an estimator that is no DeviceEstimator, ``zne(cls)`` folds the IR and extrapolates the VALUES on the host."""
    from blackwater.library.primitives import make_estimator_result

    class Job:
        def __init__(self, values):
            self._values = values

        def result(self):
            return make_estimator_result(np.asarray(self._values), [{} for _ in self._values])

    class Decay:
        def _run(self, circuits, observables, parameter_values, **options):
            return Job([0.8 * 0.9 ** sum(op.name == "cx" for op in Circuit.from_any(c).ops) for c in circuits])

    circ = Circuit(2, 0, [CircuitOp("h", (0,)), CircuitOp("cx", (0, 1))])
    est = zne.zne(Decay)(zne_strategy=zne.ZNEStrategy((1, 3, 5), zne.CxAmplifier(), zne.ExponentialExtrapolator()))
    res = est._run([circ], [[("ZZ", 1.0)]], [()]).result()
    assert abs(res.values[0] - 0.8) <= 64 * czc.U and res.metadata[0]["zne"]["extrapolator"] == "ExponentialExtrapolator()"


# ---- 6. conditions on the cases of the device suite -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", czc.SMALL, ids=lambda c: c[0])
def test_small_oracle_bounds_stay_below_the_cap(case):
    k = czc.small_case(case[1], case[2])
    assert k["term_bounds"].max() < czc.CAP and k["value_bounds"].max() < czc.CAP
    assert k["mitigated_term_bound"].max() < czc.CAP and k["mitigated_value_bound"] < czc.CAP
    assert len([op for op in k["circuit"].ops if op.name not in ("measure", "barrier")]) == zc.N_OPS + 1


@pytest.mark.parametrize("n", sorted(cc.BLOCKS))
def test_block_oracle_bounds_stay_below_the_cap(n):
    for desc in (zc.GLOBAL, zc.LOCAL_ALL):
        k = czc.block_case(n, desc)
        assert k["bounds"].max() < czc.CAP
        assert np.count_nonzero((np.abs(k["values"][0]) > 0) & (np.abs(k["values"][0]) < 1)) >= 4   # the noise shows


@pytest.mark.parametrize("case", czc.CLOSED, ids=lambda c: c[0])
def test_closed_form_bounds_stay_below_the_cap(case):
    k = czc.closed_case(case[1], case[2])
    assert k["bounds"].max() < czc.CAP and k["fit_bound"].max() < czc.CAP and (k["fit_bound"] > 0).all()


def test_the_mixed_batch_is_what_the_device_test_needs():
    circuits, obs, noise = czc.mixed_batch()
    batch = sim.compile_clifford(circuits, obs, noise)
    assert sorted(set(batch.n_qubits.tolist())) == list(czc.WIDTHS) and batch.n_reg > 0 and batch.n_lds > 0
    assert set(czc.RECORDS) <= set(np.diff(batch.op_ptr).tolist())
    assert (np.diff(batch.comb_ptr) == 4).any()                                   # asymmetric readout on two qubits: 4 sub-units
    names = {op.name for c in circuits for op in c.ops}
    assert {"id", "sx", "s", "u3", "ecr", "rzz"} <= names
    pairs = {tuple(sorted(op.qubits)) for c in circuits for op in c.ops if len(op.qubits) == 2}
    assert set(czc.BOUNDARIES) <= pairs
    two = zne.build_clifford_schedules(batch, zc.PARTIAL, zc.make_amplifier(zc.LOCAL_2Q))
    per_run = np.diff(two.sched_ptr).reshape(len(zc.PARTIAL), len(circuits))
    assert (per_run[-1] == per_run[0]).sum() >= 3 and (per_run[-1] > per_run[0]).any()   # circuits with no foldable gate, and others
    lengths = set()
    for name in czc.AMPLIFIERS:
        sch = zne.build_clifford_schedules(batch, zc.PARTIAL, zc.make_amplifier(czc.AMPLIFIERS[name]))
        lengths |= set((np.diff(sch.sched_ptr) % 4).tolist())
    assert lengths == {0, 1, 2, 3}                                                # every remainder of the chunk of four


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import dataclasses

    import torch

    from blackwater.native import _lib, ops

    circ = Circuit(2, 0, [CircuitOp("h", (0,)), CircuitOp("cx", (0, 1))])
    obs = [("ZZ", 1.0)]
    with pytest.raises(ValueError, match="shots are not drawn on the Clifford path"):
        zne.zne_run([circ], [obs], None, device="cpu", shots=100, method="clifford")
    est = zne.zne(sim.DeviceEstimator)(None, "cpu", method="clifford")
    with pytest.raises(ValueError, match="shots are not drawn on the Clifford path"):
        est.run([circ], [obs], shots=100)
    strategy = zne.ZNEStrategy((1, 3), extrapolator=zne.ExponentialExtrapolator())
    with pytest.raises(ValueError, match="ExponentialExtrapolator: shots"):
        zne.zne_run([circ], [obs], None, strategy, device="cpu", shots=100)
    with pytest.raises(ValueError, match="method = 'stabilizer'"):
        zne.zne_run([circ], [obs], method="stabilizer")
    batch = sim.compile_clifford([circ], [obs])
    assert batch.gate_ptr.tolist() == [0, 2] and batch.gate_record.tolist() == [0, 1] and batch.gate_noise.tolist() == [-1, -1]
    bare = dataclasses.replace(batch, gate_ptr=None)
    with pytest.raises(ValueError, match="no record map"):
        zne.build_clifford_schedules(bare, (1, 3), zne.GlobalFoldingAmplifier())
    with pytest.raises(ValueError, match="no noise factor"):
        zne.build_clifford_schedules(batch, (), zne.GlobalFoldingAmplifier())
    sch = zne.build_clifford_schedules(batch, (1, 3), zne.GlobalFoldingAmplifier())
    t = {k: torch.from_numpy(np.ascontiguousarray(v if v.dtype != np.uint32 else v.view(np.int32)))
         for k, v in dataclasses.asdict(batch).items() if isinstance(v, np.ndarray)}
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.clifford_run_folded(t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], batch.n_reg, batch.n_lds, t["masks"],
                                t["term_ptr"], t["coeff"], t["comb_ptr"], t["comb_unit"], t["comb_weight"],
                                torch.from_numpy(sch.sched_ptr), torch.from_numpy(sch.sched), 2)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.zne_combine_exp(torch.zeros(2, 1, dtype=torch.float64), torch.zeros(2, dtype=torch.float64), t["term_ptr"], t["coeff"])
    assert "ExponentialExtrapolator" in zne.__dict__ and sim.build_clifford_schedules is zne.build_clifford_schedules
    assert sim.ExponentialExtrapolator is zne.ExponentialExtrapolator
