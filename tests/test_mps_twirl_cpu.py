"""Pauli twirling on the matrix-product-state path without a GPU: the conjugation tables, the lowering behind ``pauli_twirl=``, every
refusal by name, the fold schedules with their twirl columns, the twirled channel against a dense oracle, and the conditions under
which tests/test_gpu_mps_twirl.py sets no case, circuit or trajectory aside (tests/mps_twirl_cases.py has the cases)."""
import dataclasses
import math

import numpy as np
import pytest

import mps_cases as mc
import mps_relax_cases as mr
import mps_twirl_cases as mt
import sim_cases as sc
import zne_cases as zc
from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.sim import NoiseModel, compile_mps
from blackwater.sim import zne
from blackwater.sim.mps import _matrix4, twirl_table

OPEN, CLOSE = mt.KIND_OPEN, mt.KIND_CLOSE


def _ops(batch, c=0):
    return batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist()


def _same_fields(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            assert x is not None and y is not None and x.dtype == y.dtype and np.array_equal(x, y), f.name
        else:
            assert x == y, f.name


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", mt.GATES)
def test_the_table_closes_every_code_up_to_a_phase(gate):
    table, g = twirl_table(gate), _matrix4(gate, ())
    assert sorted(table) == list(range(16)) and table[0] == 0
    for code in range(16):
        m = mt.pair_matrix(table[code]) @ g @ mt.pair_matrix(code)
        at = np.unravel_index(int(np.argmax(np.abs(g))), g.shape)
        phase = m[at] / g[at]
        assert abs(abs(phase) - 1.0) <= 1e-15, (gate, code)
        assert np.max(np.abs(m - phase * g)) <= 1e-15, (gate, code)


# ---- 2. the lowering ----------------------------------------------------------------------------------------------------------------------
# (noise model, thermal_relaxation, the kinds between OPEN and CLOSE)
ORDER = [("zero", False, [5]), ("depol", False, [5, 7]), ("overrot", False, [5, 5, 7]), ("line-p03", True, [5, 11])]


@pytest.mark.parametrize("name, relaxation, inner", ORDER, ids=[o[0] for o in ORDER])
@pytest.mark.parametrize("pair", [(0, 1), (1, 0)], ids=["q0-lower", "q0-upper"])
def test_record_order_and_the_record_map(name, relaxation, inner, pair):
    circ = Circuit(2, 0, [CircuitOp("sx", (0,)), CircuitOp("sx", (1,)), CircuitOp("cx", pair), CircuitOp("x", (0,))])
    obs = mc.single_z(2)
    noise = mt.model(name)
    plain = compile_mps([circ], [obs], noise, 4, thermal_relaxation=relaxation)
    batch = compile_mps([circ], [obs], noise, 4, thermal_relaxation=relaxation, pauli_twirl=True)
    ops = _ops(batch)
    kinds = [o[0] for o in ops]
    at = kinds.index(OPEN)
    assert kinds[at:at + len(inner) + 2] == [OPEN] + inner + [CLOSE] and kinds.count(OPEN) == kinds.count(CLOSE) == 1
    orient = int(pair[0] > pair[1])
    assert all(o[1] == 0 and o[2] == orient for o in ops[at:at + len(inner) + 2])   # the lower site, the gate's orientation
    assert batch.params[ops[at + len(inner) + 1][3]:ops[at + len(inner) + 1][3] + 16].tolist() == [float(v) for v in twirl_table("cx")]
    # the map: the cx is gate 2; its own record and its noise records are where they are, shifted by the OPEN before them
    assert batch.gate_twirl_open.dtype == np.int32 and batch.gate_twirl_close.dtype == np.int32
    assert batch.gate_twirl_open.tolist() == [-1, -1, at, -1] and batch.gate_twirl_close.tolist() == [-1, -1, at + len(inner) + 1, -1]
    assert int(batch.gate_record[2]) == at + 1 and int(batch.gate_noise_len[2]) == len(inner) - 1
    assert int(batch.gate_noise[2]) == (at + 2 if len(inner) > 1 else -1)
    assert batch.n_noise == plain.n_noise and np.array_equal(batch.gate_noise_len, plain.gate_noise_len)
    # without its twirl records the batch is the plain one, record for record
    rest = [o for o in ops if o[0] not in (OPEN, CLOSE)]
    assert [o[:3] for o in rest] == [o[:3] for o in _ops(plain)]
    for o, p in zip(rest, _ops(plain)):
        size = mt._SIZE[o[0]]
        assert np.array_equal(batch.params[o[3]:o[3] + size], plain.params[p[3]:p[3] + size])


def test_the_keyword_off_changes_nothing_and_names_select_gates():
    case = mt.case("n3-both-bonds")
    noise = mt.model(case["noise"])
    today = compile_mps(case["circuits"], case["observables"], noise, 4)
    for off in (False, None, np.False_):
        _same_fields(compile_mps(case["circuits"], case["observables"], noise, 4, pauli_twirl=off), today)
    assert today.gate_twirl_open is None and today.gate_twirl_close is None
    ideal = compile_mps(case["circuits"], case["observables"])
    _same_fields(compile_mps(case["circuits"], case["observables"], pauli_twirl=False), ideal)
    names = [sim.SUPPORTED_GATES[j] for j in today.gate_name.tolist()]
    for twirl, want in ((True, {"cx", "cz", "ecr"}), (("swap",), {"swap"}), ("cz", {"cz"}), (["ecr", "cx", "cx"], {"cx", "ecr"}),
                        (mt.GATES, set(mt.GATES))):
        batch = compile_mps(case["circuits"], case["observables"], noise, 4, pauli_twirl=twirl)
        assert [g for g, o in zip(names, batch.gate_twirl_open.tolist()) if o >= 0] == [g for g in names if g in want]
        for g, o, c in zip(names, batch.gate_twirl_open.tolist(), batch.gate_twirl_close.tolist()):
            if o >= 0:
                rec = batch.ops[c]
                assert rec[0] == CLOSE and batch.ops[o, 0] == OPEN and batch.params[rec[3]:rec[3] + 16].tolist() == [float(v) for v in twirl_table(g)]
    # the shots lowering goes through the same loop
    shots = sim.compile_mps_shots(case["circuits"], case["observables"], noise, 4, pauli_twirl=mt.GATES)
    _same_fields(shots.mps, compile_mps(case["circuits"], case["observables"], noise, 4, pauli_twirl=mt.GATES))


def test_refusals_name_the_offender():
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import encode_corpus, synthetic_backend, tfim_circuit
    from blackwater.sim.mps import compile_mps_shots, compile_mps_templates, run_mps_bound

    circ, obs, noise = mt.pair_circuit("cx", (0, 1)), mc.single_z(2), mt.model("depol")
    for lower in (compile_mps, compile_mps_shots):
        with pytest.raises(ValueError, match="pauli_twirl names 'rzz'; only the self-inverse two-qubit Clifford gates cx cz ecr swap"):
            lower([circ], [obs], noise, 4, pauli_twirl=("cx", "rzz"))
        with pytest.raises(ValueError, match="pauli_twirl on the ideal lowering"):
            lower([circ], [obs], pauli_twirl=True)
        with pytest.raises(ValueError, match="pauli_twirl = 3, want True, False or a sequence of gate names"):
            lower([circ], [obs], noise, 4, pauli_twirl=3)
    with pytest.raises(ValueError, match="pauli_twirl on the ideal lowering"):
        sim.mps_expectation_values([circ], [obs], device="cpu", pauli_twirl=("cx",))
    # templates: no keyword, and a batch that holds a twirl kind is refused by the bound run
    with pytest.raises(TypeError):
        compile_mps_templates([circ], [obs], noise, 4, pauli_twirl=True)
    hand = compile_mps_templates([circ], [obs], noise, 4)
    at = int(np.flatnonzero(hand.ops[:, 0] == 7)[0])
    hand.ops[at, 0] = CLOSE   # a batch built by hand
    with pytest.raises(ValueError, match=f"run_mps_bound: record {at} of the batch is a Pauli-twirl record"):
        run_mps_bound(hand, np.zeros((1, 0)), device="cpu")
    # folded runs with relaxation records stay refused exactly as they are
    relax = mt.lower("n3-relax")
    with pytest.raises(ValueError, match="build_mps_schedules: record .* of the batch is a thermal-relaxation record"):
        zne.build_mps_schedules(relax, (1.0, 3.0), zne.ZNEStrategy().noise_amplifier)
    # zne_run: the keyword belongs to the MPS path
    for method in ("exact", "clifford", "auto"):
        with pytest.raises(ValueError, match="zne_run: pauli_twirl= belongs to method='mps'"):
            zne.zne_run([circ], [obs], noise, device="cpu", method=method, pauli_twirl=True)
    with pytest.raises(ValueError, match="pauli_twirl names 'h'"):
        zne.zne_run([circ], [obs], noise, device="cpu", method="mps", trajectories=4, pauli_twirl=("h",))
    # the estimator and the data layer
    with pytest.raises(ValueError, match="pauli_twirl= belongs to method='mps' and 'mps_shots'"):
        sim.DeviceEstimator(noise, "cpu", method="trajectories", pauli_twirl=True)
    est = sim.DeviceEstimator(noise, "cpu", method="mps", trajectories=4, pauli_twirl=True)
    assert est._twirl == ("cx", "cz", "ecr") and sim.DeviceEstimator(noise, "cpu", method="mps")._twirl is None
    assert sim.DeviceEstimator(noise, "cpu", method="mps_shots", shots=8, trajectories=4, pauli_twirl=("swap",))._twirl == ("swap",)
    with pytest.raises(ValueError, match="encode_corpus: mps_twirl without mps_bond"):
        encode_corpus([tfim_circuit(12, 1, 0.5, two_q="cx")], 12, two_q="cx", device="cpu", simulate=noise, mps_twirl=True)
    with pytest.raises(ValueError, match="exp_value_generator: mps_twirl without mps_bond"):
        next(exp_value_generator(synthetic_backend(12, "cx"), 12, 3, 2, device="cpu", mps_twirl=True))


# ---- 3. the schedules ---------------------------------------------------------------------------------------------------------------------
def _fold_inputs(batch, amplifier):
    mask = zne._name_table(amplifier)[batch.gate_name.astype(np.int64)]
    owner = np.repeat(np.arange(len(batch), dtype=np.int64), np.diff(batch.gate_ptr))
    rec, noi, noi_len = (getattr(batch, k).astype(np.int64) for k in ("gate_record", "gate_noise", "gate_noise_len"))
    return batch.gate_ptr, mask, rec, noi, owner, len(batch)


@pytest.mark.parametrize("fold", ["local", "global"])
def test_without_the_columns_the_schedules_are_todays(fold):
    """``build_mps_schedules`` on an untwirled batch against ``_fold_entries`` called as it always was, entry for entry."""
    amplifier = zc.make_amplifier(mt.FOLDS[fold])
    for case_id in mt.FOLD_CASES:
        batch = mt.lower(case_id, 4, twirl=False)
        sch = zne.build_mps_schedules(batch, (1, 2.2, 3), amplifier)
        args = _fold_inputs(batch, amplifier)
        pieces, lengths = [], []
        for lam in (1.0, 2.2, 3.0):
            body, body_len, _ = zne._fold_entries(amplifier, *args, lam, batch.gate_noise_len.astype(np.int64))
            pieces.append(body.astype(np.int32))
            lengths.append(body_len)
        want = np.concatenate(pieces)
        assert sch.sched.dtype == want.dtype and sch.sched.tobytes() == want.tobytes()
        assert sch.sched_ptr.tolist() == np.concatenate([[0], np.cumsum(np.concatenate(lengths))]).tolist()
        # absent columns and None columns are the same call
        body, _, _ = zne._fold_entries(amplifier, *args, 3.0, batch.gate_noise_len.astype(np.int64), pre=None, post=None)
        assert body.tobytes() == zne._fold_entries(amplifier, *args, 3.0, batch.gate_noise_len.astype(np.int64))[0].tobytes()


def test_the_twirled_schedules_written_down_by_hand():
    """ry (0), cx (0, 1), ry (1) with a depolarising record after every gate: records 0 U1, 1 DEPOL1, 2 OPEN, 3 U2, 4 DEPOL2, 5 CLOSE,
    6 U1, 7 DEPOL1.  An entry is (record << 1) | dagger."""
    circ = Circuit(2, 0, [CircuitOp("ry", (0,), (), (0.4,)), CircuitOp("cx", (0, 1)), CircuitOp("ry", (1,), (), (0.7,))])
    batch = compile_mps([circ], [mc.single_z(2)], sc.StepNoise(5, force=False), 2, pauli_twirl=True)
    assert [o[0] for o in _ops(batch)] == [0, 6, OPEN, 5, 7, CLOSE, 0, 6]
    local = zne.build_mps_schedules(batch, (1, 3), zc.make_amplifier(zc.LOCAL_2Q))
    unit, dagger = [4, 6, 8, 10], [4, 7, 8, 10]
    once = [0, 2] + unit + [12, 14]
    assert local.sched_ptr.tolist() == [0, 8, 24]
    assert local.sched.tolist() == once + [0, 2] + unit + dagger + unit + [12, 14]
    glob = zne.build_mps_schedules(batch, (1, 3), zc.make_amplifier(zc.GLOBAL))
    assert glob.sched_ptr.tolist() == [0, 8, 32]
    assert glob.sched.tolist() == once + once + [13, 14] + dagger + [1, 2] + once
    # a twirl record is never daggered, and every pass of the gate has its own OPEN and CLOSE
    for sch in (local, glob):
        twirls = [e for e in sch.sched.tolist() if batch.ops[e >> 1, 0] in (OPEN, CLOSE)]
        assert all(e & 1 == 0 for e in twirls) and len(twirls) == 2 * (1 + 3)


# ---- 4. the twirled channel ---------------------------------------------------------------------------------------------------------------
def test_the_mean_over_the_codes_is_the_pauli_channel_of_the_error():
    transfer = mt.error_transfer_matrix()
    off = np.abs(transfer - np.diag(np.diag(transfer))).max()
    print(f"the over-rotation's transfer matrix: largest off-diagonal entry {off:.3e}")
    assert off > 1e-3, "before twirling the error is no Pauli channel"
    rows, dense = mt.channel_reference()
    assert rows.shape == (16, 15)
    print(f"mean over the 16 codes against the dense twirled channel: {np.max(np.abs(rows.mean(axis=0) - dense)):.3e}")
    assert np.max(np.abs(rows.mean(axis=0) - dense)) <= 1e-12
    # and untwirled the same circuit is somewhere else: the check above is no tautology
    plain = compile_mps([mt.channel_circuit()], [[(label, 1.0) for label in mt.PAIR_LABELS]], mt.model("overrot0"), 1)
    assert np.max(np.abs(mc.interpret(plain, 0)["terms"] - dense)) > 1e-3
    assert np.array_equal(rows[0], mc.interpret(plain, 0)["terms"]), "code 0 is the untwirled program"


def test_the_write_out_follows_the_host_draw():
    batch = mt.lower("n3-both-bonds")
    seed = mt.case("n3-both-bonds")["seed"]
    count = mt.twirl_count(batch, 0)
    assert count == 6
    for t in (0, 5):
        written, codes = mt.write_out(batch, 0, t, seed, 0)
        assert codes == mt.host_codes(count, t, seed, 0).tolist() and all(0 <= c < 16 for c in codes)
        assert not set(written.ops[:, 0].tolist()) & {OPEN, CLOSE} and written.n_noise == batch.n_noise
        letters = sum((c & 3 != 0) + (c >> 2 != 0) for c in codes)
        assert len(written.ops) >= len(batch.ops) - 2 * count + letters   # the images add their own letters
    a, b = mt.host_codes(4, 1, seed, 0), mt.host_codes(4, 1, seed, 1)
    assert not np.array_equal(a, b) and np.array_equal(a[:2], mt.host_codes(2, 1, seed, 0))


# ---- 5. the conditions under which no GPU case is set aside --------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", tuple(mt.SEEDS))
def test_conditions_hold_on_every_written_out_program(case_id):
    case = mt.case(case_id)
    units = [r for method in ("lapack", "jacobi") for per in mt.reference(case_id, method) for r in per]
    gap, cut = min(r["gap"] for r in units), min(r["cut_margin"] for r in units)
    margin, prob = min(r["margin"] for r in units), min(r["min_prob"] for r in units)
    print(f"{case_id}: margin {margin:.2e} gap {gap:.2e} cutoff factor {math.exp(min(cut, 700.0)):.3g} smallest operator probability "
          f"{prob:.2e} bond {max(r['bond'] for r in units)} decompositions {max(r['n_dec'] for r in units)}")
    assert margin >= mc.MARGIN and gap >= mc.MIN_GAP and cut >= math.log(mc.CUT_FACTOR) and prob >= mr.MIN_PROB
    assert all(r["bond"] <= case["max_bond"] for r in units)
    batch = mt.lower(case_id)
    assert {OPEN, CLOSE} <= set(batch.ops[:, 0].tolist())
    if case_id == "n5-line-b3":
        assert math.isfinite(gap) and max(r["bond"] for r in units) == 3, "the case truncates"
    if case_id == "n3-relax":
        assert 11 in batch.ops[:, 0].tolist() and max(r["bond"] for r in units) == 2
    if case_id == "n3-both-bonds":   # both bonds, the upper one at the site clamp n - 2
        assert {(o[1], o[2]) for o in _ops(batch) if o[0] == CLOSE} == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_every_gate_of_the_invariance_case_sees_all_sixteen_codes():
    case, batch = mt.case("invariance"), mt.lower("invariance")
    for j in range(len(batch)):
        assert mt.twirl_count(batch, j) == 1
        seen = {int(mt.host_codes(1, t, case["seed"], j)[0]) for t in range(case["trajectories"])}
        assert seen == set(range(16)), (j, sorted(seen))
    assert not set(batch.ops[:, 0].tolist()) & {6, 7, 10, 11}, "no Pauli is drawn by the noise"
    plain = mt.lower("invariance", twirl=False)
    for j, per in enumerate(mt.reference("invariance")):   # on the host the invariance is exact up to the interpreter's rounding
        want = mc.interpret(plain, j)["terms"]
        assert max(float(np.max(np.abs(r["terms"] - want))) for r in per) <= mt.tolerance("invariance")


@pytest.mark.parametrize("case_id", tuple(mt.SEEDS))
def test_recorded_differences_still_hold(case_id):
    diff = mt.measured_difference(case_id)
    print(f"{case_id}: LAPACK against numpy Jacobi {diff:.3e}, recorded {mt.TABLE[case_id]:.3e}, tolerance {mt.tolerance(case_id):.3e}")
    assert mt.TABLE[case_id] <= mt.HEADROOM[case_id] <= max(5.0 * mt.TABLE[case_id], 1e-15), "the headroom is twice the measurement, rounded up"
    assert diff <= mt.HEADROOM[case_id]
    assert mt.tolerance(case_id) < 1e-9


def test_the_statistics_seed_is_cleared_on_the_host():
    """T = 256 of the channel circuit: the interpreter's mean over the host draws lies within 5 standard errors of the dense
    twirled-channel value on every term that depends on the code."""
    batch = mt.channel_batch(mt.STAT["trajectories"])
    rows, dense = mt.channel_reference()
    keep = mt.stat_terms()
    assert keep.size >= 4
    codes = np.array([int(mt.host_codes(1, t, mt.STAT["seed"], 0)[0]) for t in range(mt.STAT["trajectories"])])
    assert set(codes.tolist()) == set(range(16)) and mt.twirl_count(batch, 0) == 1
    mean, err = mc.mean_and_error(rows[codes][:, keep])
    print("statistics on the host: |mean - oracle| / standard error =", np.abs(mean - dense[keep]) / err)
    assert np.all(err > 1e-4) and np.all(np.abs(mean - dense[keep]) <= mt.STAT["sigmas"] * err)


def test_the_shots_case_keeps_its_margin():
    import mps_shots_cases as msc

    margin, d = mt.shots_margin()
    ref = mt.shots_reference()
    print(f"shots: probability difference {d:.2e}, margin {margin:.2e}, smallest draw margin {ref['margin']:.2e}, flip {ref['flip_margin']:.2e}")
    assert ref["margin"] >= margin and ref["flip_margin"] >= msc.FLOOR
    assert {OPEN, CLOSE} <= set(mt.shots_case().mps.ops[:, 0].tolist())


def test_expand_writes_a_fold_out_with_its_twirl_records():
    batch, sch = mt.folded("n3-both-bonds", "local")
    one, three = mt.expand(batch, sch, 0), mt.expand(batch, sch, 1)
    assert np.array_equal(one.ops[:, :3], batch.ops[:, :3]) and one.n_noise == batch.n_noise
    folds = int((batch.gate_twirl_open >= 0).sum())
    assert int((three.ops[:, 0] == CLOSE).sum()) == 3 * folds and int((three.ops[:, 0] == OPEN).sum()) == 3 * folds
    assert three.n_noise[0] == batch.n_noise[0] + 2 * folds   # every two-qubit gate of the case is twirled and has a DEPOL2
    written, codes = mt.write_out(three, 0, 1, 3, run_key=1)
    assert len(codes) == 3 * folds and not set(written.ops[:, 0].tolist()) & {OPEN, CLOSE}
