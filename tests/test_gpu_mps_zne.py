"""Folded matrix-product-state runs on the device (mlqem_mps_run_folded_f64 and ``zne_run(method="mps")``): every run against the
plain kernel on its written-out program, bit for bit; against the numpy interpreter; its bits under batching, chunking, a prefix of
the trajectories and graph replay; malformed schedules; a 24-qubit anchor against the Clifford path; the public surface.
tests/mps_zne_cases.py has the grid, the measured tolerance tables and the conditions that tests/test_mps_zne_cpu.py asserts."""
import numpy as np
import pytest
import torch

import mps_cases as mc
import mps_zne_cases as mz
import sim_cases as sc
import zne_cases as zc
from blackwater import sim, zne
from blackwater.native import ops
from blackwater.sim import run_mps

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = [c["id"] for c in mz.grid()]
FIELDS = ("values", "term_values", "norm", "discarded", "error_bound", "bond", "std_error", "term_std_error")


def _host(t):
    return t.cpu().numpy()


def _folded(case_id, **kwargs):
    c = mz.case(case_id)
    batch, sch = mz.lowered(case_id)
    return c, batch, sch, zne.run_mps_folded(batch, sch, seed=c["seed"], device=DEV, keep_trajectories=True, **kwargs)


def _rows(res, n_f, b, n_terms):
    """A folded result as per-factor rows: field -> array [F, ...]."""
    out = {k: _host(getattr(res, k)).reshape(n_f, -1) for k in FIELDS}
    out["traj_term_values"] = _host(res.traj_term_values).reshape(-1, n_f, n_terms).transpose(1, 0, 2)   # [F, T, n_terms]
    out["traj_stats"] = _host(res.traj_stats).reshape(-1, n_f, b, ops.MPS_STATS).transpose(1, 0, 2, 3)
    return out


def _assert_rows_equal_the_plain_kernel(batch, sch, res, seed, what):
    n_f, b, n_terms = len(sch.noise_factors), len(batch), len(batch.term_circ)
    rows = _rows(res, n_f, b, n_terms)
    for f in range(n_f):
        plain = run_mps(mz.expand(batch, sch, f), seed=seed, run_keys=f * b + np.arange(b), device=DEV, keep_trajectories=True)
        for k in FIELDS:
            assert np.array_equal(rows[k][f], _host(getattr(plain, k))), (what, f, k)
        assert np.array_equal(rows["traj_term_values"][f], _host(plain.traj_term_values)), (what, f)
        assert np.array_equal(rows["traj_stats"][f], _host(plain.traj_stats)), (what, f)
    return rows


# ---- bit-equality with the plain kernel on the written-out program ------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ALL)
def test_every_row_equals_the_plain_kernel_on_its_expanded_program(case_id):
    c, batch, sch, res = _folded(case_id)
    rows = _assert_rows_equal_the_plain_kernel(batch, sch, res, c["seed"], case_id)
    # factor 1 is the identity schedule: the unexpanded batch under the keys 0 .. B - 1
    assert c["factors"][0] == 1
    plain = run_mps(batch, seed=c["seed"], device=DEV, keep_trajectories=True)
    for k in FIELDS:
        assert np.array_equal(rows[k][0], _host(getattr(plain, k))), k
    assert np.array_equal(rows["traj_term_values"][0], _host(plain.traj_term_values))
    if case_id == "n6-b4":
        assert rows["bond"].max() == 4, "the runs reach the cap (that it cuts inside both is asserted on the CPU)"


def test_haar_records_plain_and_daggered_in_both_orientations():
    """The ops-level case: a hand-built batch whose U1 / U2 records are Haar-random, scheduled plain and daggered.  The interpreter
    on the written-out program says what the state must be, so a transpose without the conjugate, a conjugate without the transpose or
    an orientation applied on the wrong side cannot hide behind the plain kernel making the same mistake."""
    batch, sch = mz.haar_case()
    res = zne.run_mps_folded(batch, sch, seed=9, device=DEV, keep_trajectories=True)
    rows = _assert_rows_equal_the_plain_kernel(batch, sch, res, 9, "haar")
    # the tolerance of the grid, formed here: 16 x the interpreter's LAPACK-versus-Jacobi difference, floored at sim_cases.term_bound's
    # form u (2 S sum cost + N + N / 64 + 16) for a state vector of 3 qubits with each of the 21 entries costed as a dense two-qubit
    # gate (32); a wrong matrix moves a term by O(1)
    refs = {m: [[mc.interpret(mz.expand(batch, sch, f), 0, m, t, 9, run_key=f) for t in range(batch.trajectories)] for f in range(2)]
            for m in ("lapack", "jacobi")}
    diff = max(float(np.max(np.abs(x["terms"] - y["terms"]))) for fa, fb in zip(refs["lapack"], refs["jacobi"]) for x, y in zip(fa, fb))
    tol = max(mc.FACTOR * diff, mc.U * (2 * 2.0 * 32 * 21 + 8 + 8 / 64 + 16))
    for f in range(2):
        for t in range(batch.trajectories):
            assert np.max(np.abs(rows["traj_term_values"][f][t] - refs["lapack"][f][t]["terms"])) <= tol, (f, t)
    assert np.max(np.abs(rows["term_values"][1] - rows["term_values"][0])) > 1e-3, "the walk is another circuit"


# ---- against the interpreter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ALL)
def test_device_against_the_interpreter(case_id):
    c, batch, sch, res = _folded(case_id)
    n_f, b, n_terms = len(c["factors"]), len(batch), len(batch.term_circ)
    rows, ref, tol = _rows(res, n_f, b, n_terms), mz.reference(case_id), mz.tolerance(case_id)
    stats = rows["traj_stats"]
    assert not stats[..., 4].any(), "a decomposition reached the sweep cap while it still rotated"
    assert stats[..., 5].max() < 30, "no decomposition needed MLQEM_MPS_SWEEPS = 30 sweeps"
    worst = 0.0
    for f in range(n_f):
        for j, per in enumerate(ref[f]):
            tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
            want = np.stack([r["terms"] for r in per])
            got = rows["traj_term_values"][f][:, tb:te]
            worst = max(worst, float(np.max(np.abs(got - want))))
            assert np.max(np.abs(got - want)) <= tol, (f, j)
            mean, err = mc.mean_and_error(want)
            assert np.max(np.abs(rows["term_values"][f][tb:te] - mean)) <= tol
            count = c["trajectories"]
            se_tol = tol / np.sqrt(count - 1) + (count + 8) * mc.U * (err.max() + 1.0)
            assert np.max(np.abs(rows["term_std_error"][f][tb:te] - err)) <= se_tol
            scale = max(per[0]["abs_coeff"], 1.0)
            vmean, verr = mc.mean_and_error(np.array([r["value"] for r in per]))
            assert abs(rows["values"][f][j] - vmean) <= tol * scale and abs(rows["std_error"][f][j] - verr) <= se_tol * scale
            assert abs(rows["norm"][f][j] - np.mean([r["norm"] for r in per])) <= tol
            want_d, want_b = np.mean([r["discarded"] for r in per]), np.mean([r["error_bound"] for r in per])
            # the floor include/mlqem_hip.h documents: a decomposition at which the cap drops nothing drops at most 2 max_bond columns
            # of at most `cutoff` of the weight each.  (mps_cases.stat_floor counts the columns LAPACK returns, min(rows, columns);
            # the kernel rotates all `columns` of a wide theta, and the rounding in the surplus ones is dropped weight too.)
            chi, cutoff = batch.max_bond, batch.cutoff
            floor_d = np.mean([r["n_free"] for r in per]) * 2 * chi * cutoff
            floor_b = np.mean([r["n_free"] for r in per]) * np.sqrt(2.0 * 2 * chi * cutoff)
            assert abs(rows["discarded"][f][j] - want_d) <= tol * want_d + floor_d
            assert abs(rows["error_bound"][f][j] - want_b) <= tol * want_b + floor_b
            assert rows["bond"][f][j] == max(r["bond"] for r in per)
            assert np.array_equal(stats[f][:, j, 3], [r["n_dec"] for r in per]), "decompositions per run"
    print(f"{case_id}: worst term difference {worst:.2e}, tolerance {tol:.2e}, most sweeps {int(stats[..., 5].max())}")


# ---- invariance --------------------------------------------------------------------------------------------------------------------------------------
def _zne_bits(run):
    return [_host(getattr(run, k)) for k in ("values", "term_values", "norm", "std_error", "term_std_error", "error_bound", "discarded", "bond",
                                              "mitigated_values", "mitigated_terms", "mitigated_std_error", "traj_term_values")]


def _mixed():
    """Five circuits of 1 .. 3 qubits (the grid's own) under one model, with an observable each."""
    circuits = mz.case("n1")["circuits"] + mz.case("n2")["circuits"] + mz.case("rzz-ecr")["circuits"]
    observables = mz.case("n1")["observables"] + mz.case("n2")["observables"] + mz.case("rzz-ecr")["observables"]
    return circuits, observables, sc.StepNoise(51)


def test_same_bits_alone_in_batches_under_chunking_and_for_a_prefix_of_the_trajectories():
    circuits, observables, noise = _mixed()
    strategy = zne.ZNEStrategy((1, 2.2, 3), zc.make_amplifier(zc.LOCAL_ALL), zne.QuadraticExtrapolator())
    n_f, count = 3, 8

    def run(size, trajectories=count, **kwargs):
        keys = (np.arange(n_f)[:, None] * 5 + np.arange(size)[None, :]).reshape(-1)   # the keys the runs have in the batch of five
        return zne.zne_run(circuits[:size], observables[:size], noise, strategy, DEV, seed=21, run_keys=keys, method="mps",
                           trajectories=trajectories, keep_trajectories=True, **kwargs)

    whole = run(5)
    full = _zne_bits(whole)
    ptr = whole.batch.term_ptr
    for size in (1, 3, 5):
        part = run(size)
        e = int(ptr[size])
        assert np.array_equal(_host(part.values), full[0][:, :size]) and np.array_equal(_host(part.term_values), full[1][:, :e])
        assert np.array_equal(_host(part.mitigated_values), full[8][:size]) and np.array_equal(_host(part.mitigated_std_error), full[10][:size])
        assert np.array_equal(_host(part.bond), full[7][:, :size]) and np.array_equal(_host(part.error_bound), full[5][:, :size])
    k = 3   # alone, under its batch keys
    alone = zne.zne_run([circuits[k]], [observables[k]], noise, strategy, DEV, seed=21, run_keys=np.arange(n_f) * 5 + k, method="mps",
                        trajectories=count)
    assert np.array_equal(_host(alone.values)[:, 0], full[0][:, k]) and _host(alone.mitigated_values)[0] == full[8][k]
    assert np.array_equal(_host(alone.term_values), full[1][:, int(ptr[k]):int(ptr[k + 1])])
    # two budgets that force different chunkings: whole runs, three a launch; and 5 of a run's 8 trajectories a launch
    per_unit = ops.mps_workspace_bytes(3, 32, 1)
    for budget in (per_unit * count * 3, per_unit * 5):
        split = run(5, buffer_bytes=budget)
        assert all(np.array_equal(a, b) for a, b in zip(_zne_bits(split), full)), budget
    short = run(5, trajectories=3)   # a prefix of the trajectories
    n_terms = int(ptr[-1])
    assert np.array_equal(_host(short.traj_term_values), full[11][:3])
    assert short.trajectories == 3 and _host(short.traj_term_values).shape == (3, n_f * n_terms)
    assert not np.array_equal(_host(run(5, trajectories=count).values), _host(zne.zne_run(
        circuits, observables, noise, strategy, DEV, seed=22, method="mps", trajectories=count).values)), "another seed is another sample"


def test_folded_run_and_combine_in_a_captured_graph():
    c = mz.case("overrot")
    batch, sch = mz.lowered("overrot")
    strategy = zne.ZNEStrategy(c["factors"], zc.make_amplifier(c["amplifier"]))
    eager = zne.zne_run(c["circuits"], c["observables"], mz.noise_of(c), strategy, DEV, seed=3, method="mps", trajectories=c["trajectories"],
                        keep_trajectories=True)
    n_f, b, n_terms, count = len(c["factors"]), len(batch), len(batch.term_circ), c["trajectories"]
    t, s = batch.to(DEV), sch.to(DEV)
    r = {k: torch.from_numpy(v).to(DEV) for k, v in zne.tile_mps_runs(batch, n_f).items()}
    keys = torch.arange(n_f * b, dtype=torch.int64, device=DEV)
    w = torch.from_numpy(eager.weights).to(DEV)
    widest = int(batch.n_qubits.max())
    workspace = torch.empty(ops.mps_workspace_bytes(widest, batch.max_bond, n_f * b * count), dtype=torch.uint8, device=DEV)
    traj_terms = torch.zeros((count, n_f * n_terms), dtype=torch.float64, device=DEV)
    traj_norm = torch.zeros((count, n_f * b), dtype=torch.float64, device=DEV)
    traj_stats = torch.zeros((count, n_f * b, ops.MPS_STATS), dtype=torch.float64, device=DEV)
    mixed = {"mitigated_terms": torch.zeros(n_terms, dtype=torch.float64, device=DEV), "mitigated_values": torch.zeros(b, dtype=torch.float64, device=DEV)}

    def launch(out=None):
        ops.sim_run_mps_folded(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], s["sched_ptr"], s["sched"], n_f, keys, r["run_qubits"],
                               r["term_circ"], r["term_off"], t["letters"], r["site_ptr"], t["readout"], (0, n_f * b), (0, n_f * n_terms),
                               (0, count), count, 3, batch.max_bond, batch.cutoff, widest, workspace, traj_terms, traj_norm, traj_stats)
        out = ops.sim_mps_finish(r["term_ptr"], r["coeff"], traj_terms, traj_norm, traj_stats, out=out)
        ops.zne_combine(out["term_values"].view(n_f, n_terms), w, t["term_ptr"], t["coeff"], **mixed)
        return out

    out = launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(out)
    for _ in range(2):
        for buf in (traj_terms, traj_norm, traj_stats, *out.values(), *mixed.values()):
            buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(traj_terms), _host(eager.traj_term_values))
        for k in ("values", "term_values", "norm", "std_error", "term_std_error", "error_bound", "discarded", "bond"):
            assert np.array_equal(_host(out[k]).reshape(n_f, -1), _host(getattr(eager, k))), k
        assert np.array_equal(_host(mixed["mitigated_values"]), _host(eager.mitigated_values))
        assert np.array_equal(_host(mixed["mitigated_terms"]), _host(eager.mitigated_terms))


# ---- malformed schedules -----------------------------------------------------------------------------------------------------------------------------
def test_malformed_schedules_complete():
    """Indices are clamped: a schedule that names records out of range (daggered, negative), an empty schedule and offsets beyond the
    array complete without an error and write finite values; the empty schedule leaves |0..0>; a well-formed run beside them keeps
    its bits."""
    c = mz.case("n2")
    batch, sch = mz.lowered("n2")
    good = zne.run_mps_folded(batch, sch, seed=c["seed"], device=DEV, keep_trajectories=True)
    n_f, b, n_terms = len(c["factors"]), len(batch), len(batch.term_circ)
    n_runs = n_f * b
    ptr, sched = sch.sched_ptr.copy(), sch.sched.copy()
    b0, e0 = int(ptr[0]), int(ptr[1])
    sched[b0:e0:2] = (1 << 20) | 1     # run 0: far out of range, daggered
    sched[b0 + 1:e0:2] = -5            # ... and negative
    empty_run = b + 1                  # factor 1 of circuit 1: made empty below by equal offsets
    lengths = np.diff(ptr)
    lengths[empty_run] = 0
    pieces = [sched[int(ptr[r]):int(ptr[r + 1])] if r != empty_run else sched[:0] for r in range(n_runs)]
    new_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    new_ptr[-1] += 1000                # beyond n_sched: clamped
    bad = zne.Schedules(sched_ptr=new_ptr, sched=np.concatenate(pieces).astype(np.int32), ids=sch.ids, n_wave=0, n_wg=0,
                        noise_factors=sch.noise_factors, achieved=sch.achieved)
    res = zne.run_mps_folded(batch, bad, seed=c["seed"], device=DEV, keep_trajectories=True)
    torch.cuda.synchronize()
    got, want = _rows(res, n_f, b, n_terms), _rows(good, n_f, b, n_terms)
    assert all(np.isfinite(got[k]).all() for k in got)
    f, j = divmod(empty_run, b)
    assert (got["norm"][f][j] == 1.0) and got["bond"][f][j] == 1 and not got["traj_stats"][f][:, j, 3].any()
    tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
    for t in range(tb, te):   # |0..0>: a Z-only term is +1, a term with X or Y is 0
        letters = batch.letters[int(batch.term_off[t]):int(batch.term_off[t]) + int(batch.n_qubits[j])]
        assert got["term_values"][f][t] == (0.0 if ((letters == 1) | (letters == 2)).any() else 1.0)
    for run in range(n_runs - 1):      # the last run's end offset moved; every other untouched run keeps its bits
        f, j = divmod(run, b)
        if run in (0, empty_run):
            continue
        tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
        assert np.array_equal(got["traj_term_values"][f][:, tb:te], want["traj_term_values"][f][:, tb:te]), run
        assert all(got[k][f][j] == want[k][f][j] for k in ("values", "norm", "std_error", "discarded", "error_bound", "bond")), run


def test_ops_refuse_wrong_lengths_by_name():
    batch, sch = mz.lowered("u3")
    t, s = batch.to(DEV), sch.to(DEV)
    r = {k: torch.from_numpy(v).to(DEV) for k, v in zne.tile_mps_runs(batch, 2).items()}
    keys = torch.arange(2, dtype=torch.int64, device=DEV)
    workspace = torch.empty(ops.mps_workspace_bytes(2, 32, 8), dtype=torch.uint8, device=DEV)

    def call(sched_ptr=s["sched_ptr"], run_keys=keys, n_factors=2, seed=0, trajectories=4):
        return ops.sim_run_mps_folded(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], sched_ptr, s["sched"], n_factors, run_keys,
                                      r["run_qubits"], r["term_circ"], r["term_off"], t["letters"], r["site_ptr"], t["readout"], (0, 2),
                                      (0, len(r["term_circ"])), (0, 4), trajectories, seed, 32, 1e-26, 2, workspace, None, None, None)

    call()
    with pytest.raises(ValueError, match="sched_ptr has 2 entries, want 3"):
        call(sched_ptr=s["sched_ptr"][:2].contiguous())
    with pytest.raises(ValueError, match="sched_ptr has 4 entries, want 3"):
        call(sched_ptr=torch.cat([s["sched_ptr"], s["sched_ptr"][-1:]]))
    with pytest.raises(ValueError, match="run_keys has 3 entries, want 2"):
        call(run_keys=torch.arange(3, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="run_keys has 1 entries, want 2"):
        call(run_keys=keys[:1].contiguous())
    with pytest.raises(ValueError, match="n_factors = 0"):
        call(n_factors=0)
    with pytest.raises(ValueError, match="seed = -1"):
        call(seed=-1)
    with pytest.raises(ValueError, match="trajectories = 0"):
        call(trajectories=0)
    torch.cuda.synchronize()


# ---- the width anchor --------------------------------------------------------------------------------------------------------------------------------
def test_width_anchor_against_the_clifford_path():
    """24 qubits, past the density-matrix cap: the per-factor device means against the exact per-factor noisy values of
    ``zne_run(method="clifford")``, every term within 4 ``term_std_error`` plus the interpreter tolerance (the CPU suite asserts that
    the interpreter's means at this seed stay within 3.5 standard errors), and every trajectory against the interpreter."""
    circ, obs, noise = mz.anchor()
    a = mz.ANCHOR
    strategy = zne.ZNEStrategy(a["factors"], zne.LocalFoldingAmplifier(gates_to_fold=2))
    run = zne.zne_run([circ], [obs], noise, strategy, DEV, seed=a["seed"], method="mps", trajectories=a["trajectories"],
                      max_bond=a["max_bond"], keep_trajectories=True)
    exact = _host(zne.zne_run([circ], [obs], noise, strategy, DEV, method="clifford").term_values)
    assert np.array_equal(exact, mz.anchor_exact()), "the host interpreter of the folded Clifford format is exact too"
    tol = mz.anchor_tolerance()
    terms, se = _host(run.term_values), _host(run.term_std_error)
    sigma = np.abs(terms - exact) / se
    print(f"anchor: device means within {sigma.max():.2f} standard errors of the exact values; smallest standard error {se.min():.3e}")
    assert (np.abs(terms - exact) <= 4.0 * se + tol).all()
    ref = mz.anchor_reference()
    traj = _host(run.traj_term_values).reshape(a["trajectories"], 2, a["n"])
    for f in range(2):
        want = np.stack([r["terms"] for r in ref[f]])
        assert np.max(np.abs(traj[:, f] - want)) <= tol, f
    assert not _host(run.traj_stats)[..., 4].any()


# ---- the public surface ------------------------------------------------------------------------------------------------------------------------------
def test_estimator_and_processor_over_the_fused_path():
    from blackwater.data.backends import PauliObservable
    from blackwater.library.learning.estimator import ZNEProcessor, learning

    c = mz.case("overrot")
    noise = mz.noise_of(c)
    strategy = zne.ZNEStrategy(c["factors"], zc.make_amplifier(c["amplifier"]))
    cls = zne.zne(sim.DeviceEstimator)
    est = cls(noise, DEV, method="mps", trajectories=8, seed=5, zne_strategy=strategy)
    obs = [PauliObservable(o) for o in c["observables"]]
    res = est.run(c["circuits"], obs).result()
    n_f, b = 2, len(c["circuits"])
    keys = np.arange(n_f * b, dtype=np.int64) + (1 << 32)   # job 1
    run = zne.zne_run(c["circuits"], c["observables"], noise, strategy, DEV, seed=5, run_keys=keys, method="mps", trajectories=8)
    assert np.array_equal(res.values, _host(run.mitigated_values))
    wrapped = learning(cls, ZNEProcessor(cls(noise, DEV, method="mps", trajectories=8, seed=5), strategy), skip_transpile=True)(
        noise, DEV, method="mps", trajectories=8, seed=5).run(c["circuits"], obs).result()
    assert np.array_equal(wrapped.values, res.values), "the processor's inner estimator runs its first job under the same keys"
    w, se, bound = run.weights, _host(run.std_error), _host(run.error_bound)
    want_se = np.sqrt((w * w)[0] * se[0] ** 2 + (w * w)[1] * se[1] ** 2)
    assert np.allclose(_host(run.mitigated_std_error), want_se, rtol=4 * mc.U, atol=0.0)
    for k, m in enumerate(res.metadata):
        assert set(m) == {"zne", "std_error", "trajectories", "truncation_error_bound"} and m["trajectories"] == 8
        assert m["std_error"] == float(_host(run.mitigated_std_error)[k])
        assert m["truncation_error_bound"] == float(np.abs(w) @ bound[:, k])
        z = m["zne"]
        assert set(z) == {"noise_factors", "achieved_factors", "values", "noise_amplifier", "extrapolator", "std_errors", "truncation_error_bounds"}
        assert z["std_errors"] == tuple(se[:, k].tolist()) and z["truncation_error_bounds"] == tuple(bound[:, k].tolist())
        assert z["values"] == tuple(_host(run.values)[:, k].tolist()) and z["noise_factors"] == (1.0, 3.0) and z["achieved_factors"] == (1.0, 3.0)
    assert _host(run.norm).shape == (n_f, b) and run.trajectories == 8 and _host(run.bond).dtype == np.int32
    # the second job of the same estimator draws with other keys
    again = est.run(c["circuits"], obs).result()
    assert not np.array_equal(again.values, res.values)
    # the exponential fit: no std_error, no truncation_error_bound, the fallback count instead
    expo = zne.ZNEStrategy((1, 3), zc.make_amplifier(c["amplifier"]), zne.ExponentialExtrapolator())
    got = cls(noise, DEV, method="mps", trajectories=8, seed=5, zne_strategy=expo).run(c["circuits"], obs).result()
    assert all(set(m) == {"zne", "trajectories"} and "fallback_terms" in m["zne"] and "std_errors" in m["zne"] for m in got.metadata)
    assert zne.zne_run(c["circuits"], c["observables"], noise, expo, DEV, method="mps", trajectories=8).mitigated_std_error is None
    # auto keeps picking what it picks: the exact simulator within its cap
    assert isinstance(zne.zne_run(c["circuits"], c["observables"], noise, strategy, DEV, method="auto").batch, sim.SimBatch)
    with pytest.raises(ValueError, match="needs noise and trajectories"):
        cls(None, DEV, method="mps").run(c["circuits"], obs)
