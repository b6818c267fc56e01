"""Zero-noise extrapolation on the matrix-product-state path without a GPU: the record map ``compile_mps`` keeps, the schedules of
``build_mps_schedules`` against the independent fold of zne_cases, the interpreter on written-out runs against the density-matrix
oracle of the folded circuit, the conditions the device comparison relies on, the refusals and the recorded tolerance tables."""
import itertools
import math

import numpy as np
import pytest

import mps_cases as mc
import mps_zne_cases as mz
import relax_cases as rc
import sim_cases as sc
import zne_cases as zc
from blackwater import sim, zne
from blackwater.data.circuit import Circuit
from blackwater.sim import NoiseModel, compile_mps
from blackwater.sim.program import SUPPORTED_GATES

ALL = [c["id"] for c in mz.grid()]
_NOT_GATES = ("barrier", "measure")


def _matrix(batch, k, d):
    po = int(batch.ops[k, 3])
    v = batch.params[po:po + 2 * d * d]
    return (v[0::2] + 1j * v[1::2]).reshape(d, d)


# ---- the record map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ALL)
def test_record_map_names_the_right_records(case_id):
    """Gate by gate: ``gate_record`` is a U1 / U2 record on the gate's (lower) site with its orientation and the matrix of
    ``sim_cases.gate_matrix`` (none for ``id``); ``gate_noise`` .. ``gate_noise + gate_noise_len`` are the coherent U2 record where the
    model has one, then the DEPOL record with the model's lambda; every record of the circuit is named exactly once."""
    c = mz.case(case_id)
    batch, _ = mz.lowered(case_id)
    noise = mz.noise_of(c)
    coherent_after = getattr(noise, "coherent_after", None)
    assert batch.gate_ptr.dtype == np.int64 and batch.gate_ptr[0] == 0 and len(batch.gate_ptr) == len(batch) + 1
    for j, circ in enumerate(c["circuits"]):
        circ = Circuit.from_any(circ)
        gates = [(i, op) for i, op in enumerate(circ.ops) if op.name not in _NOT_GATES]
        g0, g1 = int(batch.gate_ptr[j]), int(batch.gate_ptr[j + 1])
        assert g1 - g0 == len(gates)
        base, named = int(batch.op_ptr[j]), []
        for g, (i, op) in zip(range(g0, g1), gates):
            assert SUPPORTED_GATES[int(batch.gate_name[g])] == op.name
            rec, noi, length = int(batch.gate_record[g]), int(batch.gate_noise[g]), int(batch.gate_noise_len[g])
            two = len(op.qubits) == 2
            reg = tuple(circ.qubit_reg_index[q] for q in op.qubits)
            if op.name == "id":
                assert rec == -1
            else:
                kind, site, orient, _ = batch.ops[base + rec].tolist()
                assert kind == (5 if two else 0) and site == min(op.qubits) and orient == (int(op.qubits[0] > op.qubits[1]) if two else 0)
                want = sc.gate_matrix(op.name, op.params)
                assert np.max(np.abs(_matrix(batch, base + rec, 4 if two else 2) - want)) <= 4 * sc.U, (op.name, op.qubits)
                named.append(rec)
            lam = noise.after_gate(i, op.name, reg)
            coherent = coherent_after(i, op.name, reg) if coherent_after is not None else None
            assert length == (coherent is not None) + (lam is not None) and (noi >= 0) == (length > 0)
            at = noi
            if coherent is not None:
                kind, site, orient, _ = batch.ops[base + at].tolist()
                assert kind == 5 and site == min(op.qubits) and orient == int(op.qubits[0] > op.qubits[1]) and at == rec + 1
                assert np.max(np.abs(_matrix(batch, base + at, 4) - np.asarray(coherent).reshape(4, 4))) <= 4 * sc.U
                named.append(at)
                at += 1
            if lam is not None:
                kind, site, orient, po = batch.ops[base + at].tolist()
                assert kind == (7 if two else 6) and site == min(op.qubits) and batch.params[po] == lam
                named.append(at)
        assert named == list(range(int(batch.op_ptr[j + 1]) - base)), "every record belongs to one gate, in order"


def test_the_ideal_lowering_keeps_no_map():
    c = mz.case("rzz-ecr")
    ideal = compile_mps(c["circuits"], c["observables"])
    assert all(getattr(ideal, k) is None for k in ("gate_ptr", "gate_name", "gate_record", "gate_noise", "gate_noise_len"))
    with pytest.raises(ValueError, match="build_mps_schedules: the batch carries no record map.*needs noise and trajectories"):
        zne.build_mps_schedules(ideal, (1, 3), zne.LocalFoldingAmplifier())


# ---- the schedules ---------------------------------------------------------------------------------------------------------------------------
AMPLIFIERS = [("local-all", zc.LOCAL_ALL, (1, 3, 5)), ("local-2q", zc.LOCAL_2Q, (1, 3, 5)), ("global", zc.GLOBAL, zc.PARTIAL),
              ("global-first", zc.GLOBAL_FIRST, zc.PARTIAL), ("local-random-partial", zc.LOCAL_RANDOM, zc.PARTIAL)]


@pytest.mark.parametrize("name, desc, factors", AMPLIFIERS, ids=[a[0] for a in AMPLIFIERS])
@pytest.mark.parametrize("case_id", ["n1", "n2", "rzz-ecr", "overrot"])
def test_schedules_against_the_independent_fold(case_id, name, desc, factors):
    """``achieved`` equals 1 + 2 m / N of ``zne_cases.counts``; every schedule names, in order, the records of the gates of
    ``zne_cases.fold_ir``'s folded circuit (a gate's own record, then its noise records); its length follows; a dagger bit sits on
    gate records only, never on a noise record -- the coherent-error U2 included -- and on as many entries as the fold has inverses."""
    c = mz.case(case_id)
    batch, _ = mz.lowered(case_id)
    sch = zne.build_mps_schedules(batch, factors, zc.make_amplifier(desc))
    b = len(batch)
    assert sch.sched_ptr.shape == (len(factors) * b + 1,) and sch.ids.size == 0 and sch.sched.dtype == np.int32
    kind, gates, _, _ = desc
    for f, lam in enumerate(factors):
        for j, circ in enumerate(c["circuits"]):
            circ = Circuit.from_any(circ)
            gate_of = {i: g for g, i in enumerate(i for i, op in enumerate(circ.ops) if op.name not in _NOT_GATES)}
            n_fold = sum(1 for op in circ.ops if op.name not in _NOT_GATES and (kind == "global" or zc._matches(gates, op)))
            m, _, _ = zc.counts(n_fold, lam)
            assert sch.achieved[f, j] == (1.0 + 2.0 * m / n_fold if n_fold else 1.0)
            _, source, achieved = zc.fold_ir(circ, lam, desc)
            assert achieved == sch.achieved[f, j]
            want, n_inverse, n_gate_entries = [], 0, 0
            seen = {}
            for src in source:
                if src not in gate_of:
                    continue
                g = int(batch.gate_ptr[j]) + gate_of[src]
                seen[src] = seen.get(src, 0) + 1
                inverse = seen[src] % 2 == 0 if kind == "local" else None
                rec, noi, length = int(batch.gate_record[g]), int(batch.gate_noise[g]), int(batch.gate_noise_len[g])
                if rec >= 0:
                    want.append(rec)
                    n_inverse += bool(inverse)
                    n_gate_entries += 1
                want += [noi + d for d in range(length)]
            r = f * b + j
            entries = sch.sched[int(sch.sched_ptr[r]):int(sch.sched_ptr[r + 1])]
            assert (entries >> 1).tolist() == want and len(entries) == len(want)
            kinds = batch.ops[int(batch.op_ptr[j]) + (entries >> 1), 0]
            noise_records = set(int(batch.gate_noise[g]) + d for g in range(int(batch.gate_ptr[j]), int(batch.gate_ptr[j + 1]))
                                for d in range(int(batch.gate_noise_len[g])))
            for e, k in zip(entries.tolist(), kinds.tolist()):
                if e & 1:
                    assert k in (0, 5) and (e >> 1) not in noise_records
            if kind == "local":   # an odd repetition of a gate is the gate, an even one its inverse
                assert int((entries & 1).sum()) == n_inverse
            else:                 # as many inverses as extra forward passes
                n_rec = sum(1 for g in range(int(batch.gate_ptr[j]), int(batch.gate_ptr[j + 1])) if batch.gate_record[g] >= 0)
                assert int((entries & 1).sum()) * 2 == n_gate_entries - n_rec


def test_expand_conjugate_transposes_daggered_records_only():
    batch, sch = mz.haar_case()
    out = mz.expand(batch, sch, 1)
    entries = sch.sched[int(sch.sched_ptr[1]):int(sch.sched_ptr[2])].tolist()
    assert len(out.ops) == len(entries) and out.gate_ptr is None and out.n_noise == [sum(batch.ops[e >> 1, 0] in (6, 7) for e in entries)]
    for k, e in enumerate(entries):
        kind, site, orient, _ = batch.ops[e >> 1].tolist()
        assert out.ops[k, :3].tolist() == [kind, site, orient], "the orientation of a daggered record is unchanged"
        if kind in (0, 5):
            d = 2 if kind == 0 else 4
            want = _matrix(batch, e >> 1, d)
            assert np.array_equal(_matrix(out, k, d), want.conj().T if e & 1 else want)
        else:
            assert out.params[out.ops[k, 3]] == batch.params[batch.ops[e >> 1, 3]]
    plain = mz.expand(batch, sch, 0)
    assert np.array_equal(plain.ops[:, :3], batch.ops[:, :3]) and np.array_equal(plain.params[:len(batch.params) - 32], batch.params[:-32])


# ---- the interpreter on written-out runs against the density-matrix oracle of the folded circuit -----------------------------------------------
class OnlyAfter:
    """A depolarising op after the listed op indices alone."""

    has_readout = False

    def __init__(self, lam):
        self._lam = dict(lam)

    def after_gate(self, index, name, qubits):
        return self._lam.get(index)

    def readout_of(self, qubit):
        return None


class PositionCoherent(zc.PositionNoise):
    """``zne_cases.PositionNoise`` that also hands the source gate's coherent error to the op at every position."""

    def __init__(self, base, circuit, source):
        super().__init__(base, circuit, source)
        self._coherent = {}
        for j, src in enumerate(source):
            op = circuit.ops[src]
            if op.name not in _NOT_GATES:
                self._coherent[j] = base.coherent_after(src, op.name, tuple(circuit.qubit_reg_index[q] for q in op.qubits))

    def coherent_after(self, index, name, qubits):
        return self._coherent[index]


def _enumerated():
    two = mz._circuit(2, [mz._op("ry", (0,), 0.9), mz._op("u3", (1,), 0.7, -1.3, 2.1), mz._op("cx", (1, 0)), mz._op("rx", (0,), 0.3),
                          mz._op("rzz", (0, 1), 0.8)])
    three = mz._circuit(3, [mz._op("ry", (0,), 0.6), mz._op("u3", (1,), 1.1, 0.4, -2.0), mz._op("ecr", (1, 2)), mz._op("rzz", (1, 0), -0.9),
                            mz._op("sx", (2,)), mz._op("ecr", (0, 1)), mz._op("t", (1,))])
    line = mz._circuit(2, [mz._op("ry", (0,), 0.8), mz._op("ry", (1,), 1.3), mz._op("cx", (0, 1)), mz._op("rx", (1,), 0.5)])
    over = NoiseModel(gate_lambda={("cx", (0, 1)): 0.3}).with_cx_over_rotation(0.2)
    return [("cx-local", two, OnlyAfter({2: 0.3}), ("local", "cx", "from_first", None), 3),
            ("u3-global", three, OnlyAfter({1: 0.4}), zc.GLOBAL, 3),
            ("ecr-global-partial", three, OnlyAfter({6: 0.5}), zc.GLOBAL, 1.5),
            ("coherent-cx", line, over, ("local", 2, "from_first", None), 3)]


@pytest.mark.parametrize("name, circ, noise, desc, factor", _enumerated(), ids=[e[0] for e in _enumerated()])
def test_enumerated_trajectories_of_a_written_out_run_sum_to_the_density_matrix(name, circ, noise, desc, factor):
    """At most 3 executed noise entries: every Pauli choice through ``forced=``, weighted by its probability, against the
    density-matrix oracle of ``zne_cases.fold_ir``'s folded circuit with the source gate's noise at every position, to 1e-12."""
    obs = sc.term_set(circ.num_qubits, 5) + mc.single_z(circ.num_qubits)
    batch = compile_mps([circ], [obs], noise, trajectories=1)
    sch = zne.build_mps_schedules(batch, (1, factor), zc.make_amplifier(desc))
    out = mz.expand(batch, sch, 1)
    sizes = [4 if k == 6 else 16 for k in out.ops[:, 0].tolist() if k in (6, 7)]
    assert 2 <= len(sizes) <= 3 and out.n_noise == [len(sizes)]
    assert (sch.sched[int(sch.sched_ptr[1]):] & 1).any(), "the run has daggered entries"
    terms, total = 0.0, 0.0
    for choice in itertools.product(*(range(s) for s in sizes)):
        res = mc.interpret(out, 0, forced=choice)
        terms = terms + res["prob"] * res["terms"]
        total += res["prob"]
    folded, source, _ = zc.fold_ir(circ, factor, desc)
    if hasattr(noise, "coherent_after"):
        value, want, _ = rc.simulate(folded, obs, PositionCoherent(noise, circ, source))
    else:
        value, want, _ = sc.simulate(folded, obs, zc.PositionNoise(noise, circ, source))
    assert abs(total - 1.0) <= 1e-12
    assert np.max(np.abs(terms - want)) <= 1e-12
    assert abs(float(np.dot([cf for _, cf in obs], terms)) - value) <= 1e-12


# ---- the conditions of the device comparison -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ALL)
def test_conditions_hold_for_every_expanded_program(case_id):
    c = mz.case(case_id)
    assert max(Circuit.from_any(x).num_qubits for x in c["circuits"]) <= 8 and c["trajectories"] <= 8 and len(c["factors"]) <= 3
    assert all(sum(op.name not in _NOT_GATES for op in Circuit.from_any(x).ops) <= 40 for x in c["circuits"])
    for f, rows in enumerate(mz.reference(case_id)):
        units = [r for per in rows for r in per]
        gap, cut, margin = min(r["gap"] for r in units), min(r["cut_margin"] for r in units), min(r["margin"] for r in units)
        print(f"{case_id} factor {c['factors'][f]}: gap {gap:.2e} cutoff factor {math.exp(min(cut, 700.0)):.3g} margin {margin:.2e}")
        assert gap >= mc.MIN_GAP
        assert cut >= math.log(mc.CUT_FACTOR)
        assert margin >= mc.MARGIN


def test_the_capped_case_cuts_inside_folded_runs_and_the_centre_moves_both_ways():
    for f in range(2):
        assert any(not math.isinf(r["gap"]) for per in mz.reference("n6-b4")[f] for r in per), f
    assert max(r["bond"] for rows in mz.reference("n6-b4") for per in rows for r in per) == 4
    out = mz.expanded("n3-global", 2)
    sites = [o[1] for o in out.ops.tolist() if o[0] == 5]
    assert any(b > a for a, b in zip(sites, sites[1:])) and any(b < a for a, b in zip(sites, sites[1:]))
    batch, sch = mz.lowered("overrot")
    # the coherent record follows the gate and the gate's inverse, and is never daggered
    base = int(batch.op_ptr[1])
    entries = sch.sched[int(sch.sched_ptr[3]):int(sch.sched_ptr[4])].tolist()
    coherent = {int(batch.gate_noise[g]) for g in range(int(batch.gate_ptr[1]), int(batch.gate_ptr[2])) if batch.gate_noise_len[g] == 2}
    gate_of = {int(batch.gate_noise[g]): int(batch.gate_record[g]) for g in range(int(batch.gate_ptr[1]), int(batch.gate_ptr[2]))}
    hits = [(a, b) for a, b in zip(entries, entries[1:]) if (b >> 1) in coherent]
    assert hits and all(b & 1 == 0 and (a >> 1) == gate_of[b >> 1] for a, b in hits) and {a & 1 for a, _ in hits} == {0, 1}
    assert all(batch.ops[base + k, 0] == 5 for k in coherent)


@pytest.mark.parametrize("case_id", ALL)
def test_recorded_differences_still_hold(case_id):
    diff = mz.measured_difference(case_id)
    print(f"{case_id}: LAPACK against numpy Jacobi {diff:.3e}, recorded {mz.TABLE[case_id]:.3e}, tolerance {mz.tolerance(case_id):.3e}")
    assert mz.TABLE[case_id] <= mz.HEADROOM[case_id] <= 5.0 * mz.TABLE[case_id], "the headroom is twice the measurement, rounded up"
    assert diff <= mz.HEADROOM[case_id]
    assert mz.tolerance(case_id) < 1e-9
    for fa, fb in zip(mz.reference(case_id, "lapack"), mz.reference(case_id, "jacobi")):
        for ra, rb in zip(fa, fb):
            for x, y in zip(ra, rb):
                fd, fb_ = mc.stat_floor(x)
                assert abs(x["discarded"] - y["discarded"]) <= mz.tolerance(case_id) * x["discarded"] + fd
                assert abs(x["error_bound"] - y["error_bound"]) <= mz.tolerance(case_id) * x["error_bound"] + fb_
                assert x["bond"] == y["bond"] and x["n_free"] == y["n_free"]


# ---- the width anchor --------------------------------------------------------------------------------------------------------------------------
def test_the_anchor_seed_keeps_the_interpreter_within_three_and_a_half_standard_errors():
    """What lets the GPU test ask for 4 standard errors plus the interpreter tolerance: at the chosen seed the interpreter's own means
    over the 32 trajectories lie within 3.5 standard errors of the exact per-factor values of the Clifford path, every standard error
    is far above the tolerance, the runs drop nothing but rounding and no draw lies near a threshold."""
    exact = mz.anchor_exact()
    ref = mz.anchor_reference()
    assert exact.shape == (2, 24) and (np.abs(exact[1]) < np.abs(exact[0])).all(), "factor 3 is noisier than factor 1"
    worst = 0.0
    for f in range(2):
        mean, err = mc.mean_and_error(np.stack([r["terms"] for r in ref[f]]))
        assert err.min() > 1e-3
        worst = max(worst, float(np.max(np.abs(mean - exact[f]) / err)))
        for r in ref[f]:
            assert r["gap"] == math.inf and r["cut_margin"] >= math.log(mc.CUT_FACTOR) and r["margin"] >= mc.MARGIN
    print(f"anchor: the interpreter's means lie within {worst:.2f} standard errors of the exact values")
    assert worst <= 3.5
    diff = 0.0
    for fa, fb in zip(ref, mz.anchor_reference("jacobi")):
        for x, y in zip(fa, fb):
            diff = max(diff, abs(x["value"] - y["value"]), abs(x["norm"] - y["norm"]), float(np.max(np.abs(x["terms"] - y["terms"]))))
    print(f"anchor: LAPACK against numpy Jacobi {diff:.3e}, recorded {mz.ANCHOR_MEASURED[0]:.3e}")
    assert mz.ANCHOR_MEASURED[0] <= mz.ANCHOR_MEASURED[1] <= 5.0 * mz.ANCHOR_MEASURED[0] and diff <= mz.ANCHOR_MEASURED[1]


# ---- refusals and the surface that needs no device ---------------------------------------------------------------------------------------------
def test_refusals_name_the_offender():
    import torch

    from blackwater.native import _lib, ops

    c = mz.case("u3")
    noise = mz.noise_of(c)
    args = (c["circuits"], c["observables"])
    with pytest.raises(ValueError, match=r"zne_run\(method='mps'\): shots= is not supported.*mps_shots"):
        zne.zne_run(*args, noise, device="cpu", shots=100, method="mps", trajectories=4)
    with pytest.raises(ValueError, match="needs noise and trajectories"):
        zne.zne_run(*args, noise, device="cpu", method="mps")
    with pytest.raises(ValueError, match="needs noise and trajectories"):
        zne.zne_run(*args, None, device="cpu", method="mps", trajectories=4)
    with pytest.raises(ValueError, match="method = 'trajectories'.*not supported"):
        zne.zne_run(*args, noise, device="cpu", method="trajectories")
    with pytest.raises(ValueError, match="belong to method='mps'"):
        zne.zne_run(*args, noise, device="cpu", trajectories=4)
    with pytest.raises(ValueError, match="method = 'stabilizer', want one of exact, clifford, auto, trajectories, mps"):
        zne.zne_run(*args, noise, device="cpu", method="stabilizer")
    with pytest.raises(ValueError, match="max_bond = 40"):
        zne.zne_run(*args, noise, device="cpu", method="mps", trajectories=4, max_bond=40)
    assert sim.DeviceEstimator.METHODS == ("exact", "clifford", "auto", "trajectories") and sim.DeviceEstimator.WIDE_METHODS == ("mps",)
    batch, sch = mz.lowered("u3")
    with pytest.raises(ValueError, match="run_keys must be 2 integers"):
        zne.run_mps_folded(batch, sch, run_keys=[0], device="cpu")
    ideal = compile_mps(*args)
    with pytest.raises(ValueError, match="lowered without trajectories.*needs noise and trajectories"):
        zne.run_mps_folded(ideal, sch, device="cpu")
    bare = zne.build_mps_schedules(batch, (1,), zne.LocalFoldingAmplifier())
    assert np.array_equal(bare.sched, np.arange(len(batch.ops), dtype=np.int32) << 1), "factor 1 is the program itself"
    with pytest.raises(ValueError, match="no noise factor"):
        zne.build_mps_schedules(batch, (), zne.LocalFoldingAmplifier())
    t, s = batch.to("cpu"), sch.to("cpu")
    tiled = {k: torch.from_numpy(v) for k, v in zne.tile_mps_runs(batch, 2).items()}
    z = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(_lib.NativeLibraryError, match="no CPU path"):
        ops.sim_run_mps_folded(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], s["sched_ptr"], s["sched"], 2, torch.zeros(2, dtype=torch.int64),
                               tiled["run_qubits"], tiled["term_circ"], tiled["term_off"], t["letters"], tiled["site_ptr"], t["readout"],
                               (0, 2), (0, 1), (0, 1), 1, 0, 32, 1e-26, 2, torch.zeros(1, dtype=torch.uint8), z, z, z)
    est = zne.zne(sim.DeviceEstimator)(noise, "cpu", method="mps", trajectories=8, max_bond=16)
    assert (est._method, est._trajectories, est._max_bond) == ("mps", 8, 16)
    with pytest.raises(ValueError, match="method='mps'.*shots= is not supported"):
        zne.zne(sim.DeviceEstimator)(noise, "cpu", method="mps", shots=10)


def test_tiled_runs_share_letters_and_readout_through_the_offsets():
    batch, _ = mz.lowered("overrot")
    b, n_terms = len(batch), len(batch.term_circ)
    tiled = zne.tile_mps_runs(batch, 3)
    assert tiled["run_qubits"].tolist() == batch.n_qubits.tolist() * 3 and tiled["run_qubits"].dtype == np.int32
    assert tiled["term_circ"].tolist() == [f * b + int(c) for f in range(3) for c in batch.term_circ]
    assert tiled["term_off"].tolist() == batch.term_off.tolist() * 3 and int(tiled["term_off"].max()) < len(batch.letters)
    assert tiled["site_ptr"].tolist() == batch.site_ptr[:-1].tolist() * 3 + [int(batch.site_ptr[-1])]
    assert tiled["term_ptr"].tolist() == [f * n_terms + int(p) for f in range(3) for p in batch.term_ptr[:-1]] + [3 * n_terms]
    assert np.array_equal(tiled["coeff"], np.tile(batch.coeff, 3))
