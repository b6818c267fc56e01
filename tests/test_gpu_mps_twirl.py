"""Pauli twirling on matrix-product states (the TWIRL_OPEN / TWIRL_CLOSE records of mlqem_mps_run_f64 and mlqem_mps_run_folded_f64)
on the device: every trajectory against the numpy interpreter on its written-out program and, bit for bit, against the device
run of that program; the invariance of a noiseless circuit; folded runs against their schedules written out; the bits under
batching, splitting, a prefix of the trajectories and graph replay; the mean against the dense twirled channel; shots; the public
surfaces.  tests/mps_twirl_cases.py has the cases, the host draw, the write-out and the measured tolerance table, and
tests/test_mps_twirl_cpu.py asserts the conditions under which no case, circuit or trajectory is set aside here."""
import numpy as np
import pytest
import torch

import mps_cases as mc
import mps_twirl_cases as mt
import traj_cases as tc
import zne_cases as zc
from blackwater import sim, zne
from blackwater.data.synthetic import encode_corpus
from blackwater.native import ops
from blackwater.sim import compile_mps, run_mps, run_mps_shots

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("values", "term_values", "norm", "discarded", "error_bound", "bond", "std_error", "term_std_error")


def _host(t):
    return t.cpu().numpy()


def _bits(res):
    return [_host(getattr(res, k)) for k in ("values", "term_values", "norm", "discarded", "error_bound", "bond", "traj_term_values", "traj_stats")]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _raw(batch, seed, keys):
    """``(traj_terms [T, n_terms], traj_norm [T, B], traj_stats [T, B, 6])`` of one launch of the whole batch, on the host: what
    ``run_mps`` reduces, with the per-trajectory norms it does not return."""
    t = batch.to(DEV)
    b, n_terms, count = len(batch), len(batch.term_circ), batch.trajectories
    widest = int(batch.n_qubits.max())
    workspace = torch.empty(ops.mps_workspace_bytes(widest, batch.max_bond, b * count), dtype=torch.uint8, device=DEV)
    traj_terms = torch.zeros((count, n_terms), dtype=torch.float64, device=DEV)
    traj_norm = torch.zeros((count, b), dtype=torch.float64, device=DEV)
    traj_stats = torch.zeros((count, b, ops.MPS_STATS), dtype=torch.float64, device=DEV)
    ops.sim_run_mps(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], torch.as_tensor(np.asarray(keys, dtype=np.int64), device=DEV),
                    t["term_circ"], t["term_off"], t["letters"], t["site_ptr"], t["readout"], (0, b), (0, n_terms), (0, count), count, seed,
                    batch.max_bond, batch.cutoff, widest, workspace, traj_terms, traj_norm, traj_stats)
    return _host(traj_terms), _host(traj_norm), _host(traj_stats)


# ---- every trajectory against the interpreter on its written-out program -----------------------------------------------------------------
@pytest.mark.parametrize("case_id", mt.IDS)
def test_device_against_the_interpreter(case_id):
    case, batch = mt.case(case_id), mt.lower(case_id)
    res = run_mps(batch, seed=case["seed"], device=DEV, keep_trajectories=True)
    ref, tol = mt.reference(case_id), mt.tolerance(case_id)
    traj, stats = _host(res.traj_term_values), _host(res.traj_stats)
    values, terms, norm = _host(res.values), _host(res.term_values), _host(res.norm)
    discarded, bound, bond = _host(res.discarded), _host(res.error_bound), _host(res.bond)
    count = case["trajectories"]
    assert traj.shape == (count, len(batch.term_circ)) and stats.shape == (count, len(batch), ops.MPS_STATS)
    assert not stats[:, :, 4].any(), "a decomposition reached the sweep cap while it still rotated"
    worst = 0.0
    for j, per in enumerate(ref):
        tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
        rows = np.stack([r["terms"] for r in per])
        worst = max(worst, float(np.max(np.abs(traj[:, tb:te] - rows))))
        print(f"{case_id}[{j}]: worst term difference {np.max(np.abs(traj[:, tb:te] - rows)):.2e}, tolerance {tol:.2e}")
        assert np.max(np.abs(traj[:, tb:te] - rows)) <= tol                     # every trajectory's terms
        scale = max(per[0]["abs_coeff"], 1.0)
        coeff = batch.coeff[tb:te]
        for t, r in enumerate(per):                                             # every trajectory's value and statistics
            assert abs(float(np.dot(coeff, traj[t, tb:te])) - r["value"]) <= tol * scale
            floor_d, floor_b = mt.stat_floor(r, batch, j)
            assert abs(stats[t, j, 0] - r["discarded"]) <= tol * r["discarded"] + floor_d
            assert abs(stats[t, j, 1] - r["error_bound"]) <= tol * r["error_bound"] + floor_b
            assert int(stats[t, j, 2]) == r["bond"] and int(stats[t, j, 3]) == r["n_dec"]   # a twirl moves no centre
        mean, err = mc.mean_and_error(rows)
        assert np.max(np.abs(terms[tb:te] - mean)) <= tol
        vmean, verr = mc.mean_and_error(np.array([r["value"] for r in per]))
        assert abs(values[j] - vmean) <= tol * scale
        assert abs(norm[j] - np.mean([r["norm"] for r in per])) <= tol
        se_tol = tol / np.sqrt(count - 1) + (count + 8) * mc.U * (err.max() + 1.0)
        assert np.max(np.abs(_host(res.term_std_error)[tb:te] - err)) <= se_tol
        assert abs(_host(res.std_error)[j] - verr) <= se_tol * scale
        want_d, want_b = np.mean([r["discarded"] for r in per]), np.mean([r["error_bound"] for r in per])
        floor_d, floor_b = (np.mean([mt.stat_floor(r, batch, j)[k] for r in per]) for k in (0, 1))
        assert abs(discarded[j] - want_d) <= tol * want_d + floor_d
        assert abs(bound[j] - want_b) <= tol * want_b + floor_b
        assert bond[j] == max(r["bond"] for r in per)
    print(f"{case_id}: worst term difference {worst:.2e}, tolerance {tol:.2e}, most sweeps {int(stats[:, :, 5].max())}")


# ---- bit-equality to the written-out program ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", mt.BIT_CASES)
def test_every_trajectory_equals_the_device_run_of_its_written_out_program(case_id):
    """Row t of the twirled run against row t of the run of trajectory t's written-out program, under the same T, seed and key:
    terms, norm and stats."""
    case, batch = mt.case(case_id), mt.lower(case_id)
    seed, count = case["seed"], case["trajectories"]
    terms, norm, stats = _raw(batch, seed, np.arange(len(batch)))
    for j in range(len(batch)):
        tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
        drawn = set()
        for t in range(count):
            written, codes = mt.written(case_id, j, t)
            drawn |= set(codes)
            w_terms, w_norm, w_stats = _raw(written, seed, [j])
            assert np.array_equal(terms[t, tb:te], w_terms[t]), (j, t, "terms")
            assert np.array_equal(norm[t, j], w_norm[t, 0]), (j, t, "norm")
            assert np.array_equal(stats[t, j], w_stats[t, 0]), (j, t, "stats")
        assert len(drawn) > 1, "the trajectories drew different twirls"
    plain = run_mps(mt.lower(case_id, twirl=False), seed=seed, device=DEV, keep_trajectories=True)
    assert not np.array_equal(_host(plain.traj_term_values), terms), "the twirl changes the trajectories"


# ---- invariance --------------------------------------------------------------------------------------------------------------------------
def test_a_twirl_leaves_a_noiseless_gate_alone():
    """Under a model whose every lambda is 0 nothing but the twirl is drawn, and P' G P = G up to a phase: every trajectory's terms
    are the untwirled run's, for each of the four gates (every one of which sees all 16 codes: asserted on the CPU)."""
    case, tol = mt.case("invariance"), mt.tolerance("invariance")
    twirled = run_mps(mt.lower("invariance"), seed=case["seed"], device=DEV, keep_trajectories=True)
    plain = run_mps(mt.lower("invariance", twirl=False), seed=case["seed"], device=DEV, keep_trajectories=True)
    got, want = _host(twirled.traj_term_values), _host(plain.traj_term_values)
    assert np.array_equal(want, np.broadcast_to(want[0], want.shape)), "without a draw every trajectory is the same state"
    batch = mt.lower("invariance")
    for j, gate in enumerate(mt.GATES):
        tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
        print(f"invariance, {gate}: worst term difference {np.max(np.abs(got[:, tb:te] - want[:, tb:te])):.2e}, tolerance {tol:.2e}")
        assert np.max(np.abs(got[:, tb:te] - want[:, tb:te])) <= tol, gate
    # a twirl is no decomposition and moves no centre: the same bonds and the same number of decompositions
    assert np.array_equal(_host(twirled.traj_stats)[:, :, 2:4], _host(plain.traj_stats)[:, :, 2:4])
    ref = mt.reference("invariance")
    for j, per in enumerate(ref):
        tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
        assert np.max(np.abs(got[:, tb:te] - np.stack([r["terms"] for r in per]))) <= tol


# ---- folded runs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", ["local", "global"])
@pytest.mark.parametrize("case_id", mt.FOLD_CASES)
def test_a_folded_run_equals_the_plain_kernel_on_its_schedule_written_out(case_id, fold):
    case = mt.case(case_id)
    batch, sch = mt.folded(case_id, fold)
    res = zne.run_mps_folded(batch, sch, seed=case["seed"], device=DEV, keep_trajectories=True)
    n_f, b, n_terms = len(mt.FOLD_FACTORS), len(batch), len(batch.term_circ)
    rows = {k: _host(getattr(res, k)).reshape(n_f, -1) for k in FIELDS}
    traj = _host(res.traj_term_values).reshape(-1, n_f, n_terms).transpose(1, 0, 2)
    stats = _host(res.traj_stats).reshape(-1, n_f, b, ops.MPS_STATS).transpose(1, 0, 2, 3)
    for f in range(n_f):
        expanded = mt.expand(batch, sch, f)
        assert int((expanded.ops[:, 0] == mt.KIND_CLOSE).sum()) == (1, 3)[f] * int((batch.gate_twirl_close >= 0).sum())
        plain = run_mps(expanded, seed=case["seed"], run_keys=f * b + np.arange(b), device=DEV, keep_trajectories=True)
        for k in FIELDS:
            assert np.array_equal(rows[k][f], _host(getattr(plain, k))), (f, k)
        assert np.array_equal(traj[f], _host(plain.traj_term_values)) and np.array_equal(stats[f], _host(plain.traj_stats)), f
    # every pass of a folded gate draws its own twirl: the codes of the factor-3 run's passes differ
    _, codes = mt.write_out(mt.expand(batch, sch, 1), 0, 0, case["seed"], run_key=b)
    assert len(codes) == 3 * int((batch.gate_twirl_close >= 0).sum()) and len(set(codes[:3])) > 1
    # zne_run lowers, folds and runs the same
    strategy = zne.ZNEStrategy(mt.FOLD_FACTORS, zc.make_amplifier(mt.FOLDS[fold]))
    run = zne.zne_run(case["circuits"], case["observables"], mt.model(case["noise"]), strategy, DEV, seed=case["seed"], method="mps",
                      trajectories=batch.trajectories, pauli_twirl=case["twirl"])
    assert np.array_equal(_host(run.values), rows["values"]) and np.array_equal(_host(run.term_values), rows["term_values"])
    assert np.array_equal(run.schedules.sched, sch.sched)
    untwirled = zne.zne_run(case["circuits"], case["observables"], mt.model(case["noise"]), strategy, DEV, seed=case["seed"], method="mps",
                            trajectories=batch.trajectories)
    assert not np.array_equal(_host(untwirled.values), rows["values"])


# ---- determinism -------------------------------------------------------------------------------------------------------------------------
def test_same_bits_alone_in_a_batch_in_any_split_and_as_a_prefix():
    ids = ("n2-cx", "n3-both-bonds", "n5-line-b3")
    circuits = [c for i in ids for c in mt.case(i)["circuits"]]
    observables = [o for i in ids for o in mt.case(i)["observables"]]
    noise = mt.model("step-53")
    lower = lambda cs, os_, t=8: compile_mps(cs, os_, noise, t, 32, pauli_twirl=mt.GATES)   # noqa: E731
    batch = lower(circuits, observables)
    assert {mt.KIND_OPEN, mt.KIND_CLOSE} <= set(batch.ops[:, 0].tolist())
    whole = run_mps(batch, seed=11, device=DEV, keep_trajectories=True)
    full = _bits(whole)
    ptr = _host(whole.term_ptr)
    for j in (0, 2, 3):   # alone, with its batch key
        alone = run_mps(lower([circuits[j]], [observables[j]]), seed=11, run_keys=[j], device=DEV, keep_trajectories=True)
        got = _bits(alone)
        assert np.array_equal(got[0], full[0][j:j + 1]) and np.array_equal(got[1], full[1][ptr[j]:ptr[j + 1]])
        assert np.array_equal(got[4], full[4][j:j + 1]) and np.array_equal(got[5], full[5][j:j + 1])
        assert np.array_equal(got[6], full[6][:, ptr[j]:ptr[j + 1]]) and np.array_equal(got[7][:, 0], full[7][:, j])
    per_unit = ops.mps_workspace_bytes(5, 32, 1)
    for budget in (per_unit * 8, per_unit * 3, 1):   # a circuit's trajectories per launch, a few units, one unit
        split = run_mps(batch, seed=11, device=DEV, keep_trajectories=True, buffer_bytes=budget)
        assert _same(_bits(split), full), budget
    short = run_mps(lower(circuits, observables, 5), seed=11, device=DEV, keep_trajectories=True)   # T = 5 is a prefix of T = 8
    assert np.array_equal(_host(short.traj_term_values), full[6][:5]) and np.array_equal(_host(short.traj_stats), full[7][:5])
    assert not np.array_equal(_host(run_mps(batch, seed=12, device=DEV).values), full[0]), "another seed is another sample"


def test_a_replayed_graph_gives_the_same_bits():
    case_id = "n2-cx"
    batch, seed = mt.lower(case_id), mt.case(case_id)["seed"]
    eager = run_mps(batch, seed=seed, device=DEV, keep_trajectories=True)
    t = batch.to(DEV)
    b, n_terms, count = len(batch), len(batch.term_circ), batch.trajectories
    keys = torch.arange(b, dtype=torch.int64, device=DEV)
    widest = int(batch.n_qubits.max())
    workspace = torch.empty(ops.mps_workspace_bytes(widest, batch.max_bond, b * count), dtype=torch.uint8, device=DEV)
    traj_terms = torch.zeros((count, n_terms), dtype=torch.float64, device=DEV)
    traj_norm = torch.zeros((count, b), dtype=torch.float64, device=DEV)
    traj_stats = torch.zeros((count, b, ops.MPS_STATS), dtype=torch.float64, device=DEV)

    def launch(out=None):   # one stream: the capture has no parallel branches
        ops.sim_run_mps(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], keys, t["term_circ"], t["term_off"], t["letters"], t["site_ptr"],
                        t["readout"], (0, b), (0, n_terms), (0, count), count, seed, batch.max_bond, batch.cutoff, widest, workspace,
                        traj_terms, traj_norm, traj_stats)
        return ops.sim_mps_finish(t["term_ptr"], t["coeff"], traj_terms, traj_norm, traj_stats, out=out)

    out = launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(out)
    for _ in range(2):
        for buf in (traj_terms, traj_norm, traj_stats, *out.values()):
            buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(traj_terms), _host(eager.traj_term_values)) and np.array_equal(_host(traj_stats), _host(eager.traj_stats))
        for k in ("values", "term_values", "norm", "discarded", "error_bound", "bond", "std_error", "term_std_error"):
            assert np.array_equal(_host(out[k]), _host(getattr(eager, k))), k


# ---- statistics ---------------------------------------------------------------------------------------------------------------------------
def test_the_mean_lies_within_five_standard_errors_of_the_twirled_channel():
    """Two qubits, ry on each, one over-rotated cx, T = 256: the mean over the device's twirls against the dense value under the
    Pauli channel of the error (the diagonal of its transfer matrix), on every term that depends on the code drawn."""
    batch = mt.channel_batch(mt.STAT["trajectories"])
    res = run_mps(batch, seed=mt.STAT["seed"], device=DEV)
    _, dense = mt.channel_reference()
    keep = mt.stat_terms()
    mean, err = _host(res.term_values)[keep], _host(res.term_std_error)[keep]
    print("statistics: |mean - oracle| / standard error =", np.abs(mean - dense[keep]) / err)
    assert np.all(np.abs(mean - dense[keep]) <= mt.STAT["sigmas"] * err)


# ---- shots --------------------------------------------------------------------------------------------------------------------------------
def test_shots_from_the_twirled_states_equal_the_host_draws():
    import mps_shots_cases as ms

    batch = mt.shots_case()
    res = run_mps_shots(batch, mt.SHOTS["shots"], seed=mt.SHOTS["seed"], return_bits=True, device=DEV)
    ref = mt.shots_reference()
    shots, n = mt.SHOTS["shots"], int(batch.mps.n_qubits[0])
    for g, want in enumerate(ref["bits"]):
        w = int(batch.ref_ptr[g + 1] - batch.ref_ptr[g])
        at = int(batch.ref_ptr[g]) * shots
        got = _host(res.bits[at:at + shots * w]).view(np.uint32).reshape(shots, w)
        assert np.array_equal(got, want), (g, int((got != want).any(axis=1).sum()), "shots differ")
    assert np.array_equal(_host(res.term_sums), ref["term_sums"])
    assert sim.mps_counts(res, 0) == [ms.counts_of(w, n) for w in ref["bits"]]
    plain = run_mps(batch.mps, seed=mt.SHOTS["seed"], device=DEV)
    assert np.array_equal(_host(res.error_bound), _host(plain.error_bound)) and np.array_equal(_host(res.bond), _host(plain.bond))


# ---- the public surfaces ------------------------------------------------------------------------------------------------------------------
def test_estimator_metadata_the_corpus_and_the_bound_refusal():
    from blackwater.sim.mps import compile_mps_templates, run_mps_bound

    case = mt.case("n4-readout")
    noise = mt.model(case["noise"])
    est = sim.DeviceEstimator(noise, DEV, method="mps", trajectories=8, seed=5, pauli_twirl=True)
    got = est.run(case["circuits"], case["observables"]).result()
    direct = sim.mps_expectation_values(case["circuits"], case["observables"], noise, trajectories=8, seed=5,
                                        run_keys=sim.default_run_keys(1, 1 << 32), device=DEV, pauli_twirl=True)
    assert np.array_equal(got.values, _host(direct.values))
    assert all(set(m) == {"truncation_error_bound", "max_bond", "std_error", "trajectories"} and m["trajectories"] == 8 for m in got.metadata)
    plain = sim.DeviceEstimator(noise, DEV, method="mps", trajectories=8, seed=5).run(case["circuits"], case["observables"]).result()
    assert [set(m) for m in plain.metadata] == [set(m) for m in got.metadata]   # (a Pauli channel's values do not move under a twirl)
    shot = sim.DeviceEstimator(noise, DEV, method="mps_shots", shots=32, trajectories=4, seed=5, pauli_twirl=True)
    meta = shot.run(case["circuits"], case["observables"]).result().metadata
    assert all(set(m) == {"variance", "shots", "truncation_error_bound", "max_bond", "trajectories"} for m in meta)
    # zne(DeviceEstimator) passes the keyword on to the folded runs
    from blackwater.data.backends import PauliObservable

    strategy = zne.ZNEStrategy((1, 3), zc.make_amplifier(zc.LOCAL_2Q))
    cls = zne.zne(sim.DeviceEstimator)
    obs = [PauliObservable(o) for o in case["observables"]]
    mitigated = cls(noise, DEV, method="mps", trajectories=8, seed=5, zne_strategy=strategy, pauli_twirl=True).run(case["circuits"], obs).result()
    keys = np.arange(2, dtype=np.int64) + (1 << 32)
    run = zne.zne_run(case["circuits"], case["observables"], noise, strategy, DEV, seed=5, run_keys=keys, method="mps", trajectories=8,
                      pauli_twirl=True)
    assert np.array_equal(mitigated.values, _host(run.mitigated_values))
    bare = cls(noise, DEV, method="mps", trajectories=8, seed=5, zne_strategy=strategy).run(case["circuits"], obs).result()
    assert [set(m) for m in mitigated.metadata] == [set(m) for m in bare.metadata]
    # encode_corpus on a 12-qubit line: with trajectories the exact paths take circuits up to 11 qubits, so 12 is the narrowest line
    # whose noisy labels come from the matrix-product-state path
    nq = 12
    circuits = [tc.line_circuit(nq, 930 + k) for k in range(3)]
    model = sim.NoiseModel.from_backend(tc.table(nq)).with_cx_over_rotation(0.2)
    corpus = encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=model, device=DEV, mps_bond=8, mps_twirl=True, trajectories=8)
    z_qubits = [int(np.flatnonzero(o[0, 2::4])[0]) for o in corpus["observable"]]
    labels = ["".join("Z" if q == z else "I" for q in reversed(range(nq))) for z in z_qubits]
    under = sim.mps_expectation_values(circuits, labels, model, max_bond=8, trajectories=8, seed=7, run_keys=np.arange(3), device=DEV,
                                       pauli_twirl=True)
    ideal = sim.mps_expectation_values(circuits, labels, max_bond=8, device=DEV)
    assert np.array_equal(corpus["noisy"][:, 0], _host(under.values).astype(np.float32))
    assert np.array_equal(corpus["y"][:, 0], _host(ideal.values).astype(np.float32))
    assert corpus["mps_error_bound"] == max(float(_host(ideal.error_bound).max()), float(_host(under.error_bound).max()))
    untwirled = encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=model, device=DEV, mps_bond=8, trajectories=8)
    assert not np.array_equal(untwirled["noisy"], corpus["noisy"]) and np.array_equal(untwirled["y"], corpus["y"])
    # a bound run refuses a batch that holds a twirl kind: the bind kernel would copy one value of its table of 16
    circ = mt.pair_circuit("cx", (0, 1))
    hand = compile_mps_templates([circ], [mc.single_z(2)], mt.model("depol"), 4)
    at = int(np.flatnonzero(hand.ops[:, 0] == 7)[0])
    hand.ops[at, 0] = mt.KIND_CLOSE
    with pytest.raises(ValueError, match=f"run_mps_bound: record {at} of the batch is a Pauli-twirl record"):
        run_mps_bound(hand, np.zeros((1, 0)), device=DEV)
