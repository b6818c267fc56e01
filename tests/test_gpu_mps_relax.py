"""Thermal relaxation on matrix-product states (the NOISE1 / NOISE2 records of mlqem_mps_run_f64) on the device: every trajectory
against the numpy interpreter of the record format, the bits under batching, splitting, a prefix of the trajectories and graph
replay, the mean against the density-matrix oracle, shots from the relaxed states, and the public surfaces.
tests/mps_relax_cases.py has the cases, the measured tolerance table and the conditions that tests/test_mps_relax_cpu.py asserts,
so that no case, circuit or trajectory is set aside here."""
import numpy as np
import pytest
import torch

import mps_cases as mc
import mps_relax_cases as mr
import traj_cases as tc
from blackwater import sim
from blackwater.data.synthetic import encode_corpus
from blackwater.native import ops
from blackwater.sim import compile_mps, run_mps, run_mps_shots

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _host(t):
    return t.cpu().numpy()


def _bits(res):
    return [_host(getattr(res, k)) for k in ("values", "term_values", "norm", "discarded", "error_bound", "bond", "traj_term_values", "traj_stats")]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case_id", mr.IDS)
def test_device_against_the_interpreter(case_id):
    """Per trajectory: terms, values, the norm, ``discarded`` and ``error_bound`` (the relative rule of tests/test_gpu_mps.py with its
    floors, the floor under ``error_bound`` scaled by the t's as the bound is), the bond, and no unconverged decomposition."""
    case, batch = mr.case(case_id), mr.lower(case_id)
    res = run_mps(batch, seed=case["seed"], device=DEV, keep_trajectories=True)
    ref, tol = mr.reference(case_id), mr.tolerance(case_id)
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
            floor_d, floor_b = mc.stat_floor(r)
            assert abs(stats[t, j, 0] - r["discarded"]) <= tol * r["discarded"] + floor_d
            assert abs(stats[t, j, 1] - r["error_bound"]) <= tol * r["error_bound"] + floor_b
            assert int(stats[t, j, 2]) == r["bond"] and int(stats[t, j, 3]) == r["n_dec"]
        mean, err = mc.mean_and_error(rows)
        assert np.max(np.abs(terms[tb:te] - mean)) <= tol
        vmean, verr = mc.mean_and_error(np.array([r["value"] for r in per]))
        assert abs(values[j] - vmean) <= tol * scale
        assert abs(norm[j] - np.mean([r["norm"] for r in per])) <= tol
        se_tol = tol / np.sqrt(count - 1) + (count + 8) * mc.U * (err.max() + 1.0)
        assert np.max(np.abs(_host(res.term_std_error)[tb:te] - err)) <= se_tol
        assert abs(_host(res.std_error)[j] - verr) <= se_tol * scale
        want_d, want_b = np.mean([r["discarded"] for r in per]), np.mean([r["error_bound"] for r in per])
        floor_d, floor_b = np.mean([mc.stat_floor(r)[0] for r in per]), np.mean([mc.stat_floor(r)[1] for r in per])
        assert abs(discarded[j] - want_d) <= tol * want_d + floor_d
        assert abs(bound[j] - want_b) <= tol * want_b + floor_b
        assert bond[j] == max(r["bond"] for r in per)
    print(f"{case_id}: worst term difference {worst:.2e}, tolerance {tol:.2e}, most sweeps {int(stats[:, :, 5].max())}")


def test_same_bits_alone_in_a_batch_in_any_split_and_as_a_prefix():
    ids = ("n2-corners-T16", "n5-line-p03-T8", "n4-overrot-T8")
    circuits = [c for i in ids for c in mr.case(i)["circuits"]]
    observables = [o for i in ids for o in mr.case(i)["observables"]]
    # one model for the batch: the corners circuits under open-p03 too (what matters here is bits, not the model)
    noise = mr.model("open-p03").with_cx_over_rotation(0.2)
    lower = lambda cs, os_, t=8: compile_mps(cs, os_, noise, t, 32, thermal_relaxation=True)   # noqa: E731
    batch = lower(circuits, observables)
    assert {10, 11} <= set(batch.ops[:, 0].tolist())
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
    case_id = "n2-corners-T16"
    batch, seed = mr.lower(case_id), mr.case(case_id)["seed"]
    eager = run_mps(batch, seed=seed, device=DEV, keep_trajectories=True)
    t = batch.to(DEV)
    b, n_terms, count = len(batch), len(batch.term_circ), batch.trajectories
    keys = torch.arange(b, dtype=torch.int64, device=DEV)
    widest = int(batch.n_qubits.max())
    workspace = torch.empty(ops.mps_workspace_bytes(widest, batch.max_bond, b * count), dtype=torch.uint8, device=DEV)
    traj_terms = torch.zeros((count, n_terms), dtype=torch.float64, device=DEV)
    traj_norm = torch.zeros((count, b), dtype=torch.float64, device=DEV)
    traj_stats = torch.zeros((count, b, ops.MPS_STATS), dtype=torch.float64, device=DEV)

    def launch(out=None):
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


def test_the_mean_lies_within_five_standard_errors_of_the_density_matrix():
    """n = 4, line-p03, T = 256, a fixed seed that tests/test_mps_relax_cpu.py cleared for the interpreter's trajectories."""
    _, _, batch = mr.stat_case()
    res = run_mps(batch, seed=mr.STAT["seed"], device=DEV)
    _, want = mr.stat_reference()
    mean, err = _host(res.term_values), _host(res.term_std_error)
    print("statistics: |mean - oracle| / standard error =", np.abs(mean - want) / err)
    assert np.all(np.abs(mean - want) <= mr.STAT["sigmas"] * err)


def test_shots_from_the_relaxed_states_equal_the_host_draws():
    """One case: the counts against the host draw interpreter of tests/mps_shots_cases.py on this module's site tensors, bit for bit
    (its rule for noisy cases; tests/test_mps_relax_cpu.py asserts the margin condition)."""
    import mps_shots_cases as ms

    _, _, batch = mr.shots_case()
    res = run_mps_shots(batch, mr.SHOTS["shots"], seed=mr.SHOTS["seed"], return_bits=True, device=DEV)
    ref = mr.shots_reference()
    shots, n = mr.SHOTS["shots"], mr.SHOTS["n"]
    for g, want in enumerate(ref["bits"]):
        w = int(batch.ref_ptr[g + 1] - batch.ref_ptr[g])
        at = int(batch.ref_ptr[g]) * shots
        got = _host(res.bits[at:at + shots * w]).view(np.uint32).reshape(shots, w)
        assert np.array_equal(got, want), (g, int((got != want).any(axis=1).sum()), "shots differ")
    assert np.array_equal(_host(res.term_sums), ref["term_sums"])
    assert sim.mps_counts(res, 0) == [ms.counts_of(w, n) for w in ref["bits"]]
    plain = run_mps(batch.mps, seed=mr.SHOTS["seed"], device=DEV)
    assert np.array_equal(_host(res.error_bound), _host(plain.error_bound)) and np.array_equal(_host(res.bond), _host(plain.bond))


def test_estimator_metadata_and_the_corpus_surface():
    case_id = "n4-readout-T8"
    case, noise = mr.case(case_id), mr.model("readout")
    est = sim.DeviceEstimator(noise, DEV, method="mps", trajectories=8, seed=5, thermal_relaxation=True)
    got = est.run(case["circuits"], case["observables"]).result()
    direct = sim.mps_expectation_values(case["circuits"], case["observables"], noise, trajectories=8, seed=5,
                                        run_keys=sim.default_run_keys(1, 1 << 32), device=DEV, thermal_relaxation=True)
    assert np.array_equal(got.values, _host(direct.values))
    assert all(set(m) == {"truncation_error_bound", "max_bond", "std_error", "trajectories"} and m["trajectories"] == 8 for m in got.metadata)
    assert [m["std_error"] for m in got.metadata] == _host(direct.std_error).tolist()
    with pytest.raises(ValueError, match="the noise model has thermal relaxation"):
        sim.DeviceEstimator(noise, DEV, method="mps", trajectories=8).run(case["circuits"], case["observables"])
    shot = sim.DeviceEstimator(noise, DEV, method="mps_shots", shots=32, trajectories=4, seed=5, thermal_relaxation=True)
    meta = shot.run(case["circuits"], case["observables"]).result().metadata
    assert all(set(m) == {"variance", "shots", "truncation_error_bound", "max_bond", "trajectories"} for m in meta)
    # encode_corpus on a 12-qubit line: with trajectories the exact paths take circuits up to 11 qubits, so 12 is the narrowest line
    # whose noisy labels come from the matrix-product-state path
    nq = 12
    circuits = [tc.line_circuit(nq, 930 + k) for k in range(3)]
    model = sim.NoiseModel.from_backend(tc.table(nq), thermal_relaxation=True)
    with pytest.raises(ValueError, match="the noise model has thermal relaxation"):
        encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=model, device=DEV, mps_bond=8, trajectories=8)
    corpus = encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=model, device=DEV, mps_bond=8, mps_relaxation=True, trajectories=8)
    z_qubits = [int(np.flatnonzero(o[0, 2::4])[0]) for o in corpus["observable"]]
    labels = ["".join("Z" if q == z else "I" for q in reversed(range(nq))) for z in z_qubits]
    under = sim.mps_expectation_values(circuits, labels, model, max_bond=8, trajectories=8, seed=7, run_keys=np.arange(3), device=DEV,
                                       thermal_relaxation=True)
    ideal = sim.mps_expectation_values(circuits, labels, max_bond=8, device=DEV)
    assert np.array_equal(corpus["noisy"][:, 0], _host(under.values).astype(np.float32))
    assert np.array_equal(corpus["y"][:, 0], _host(ideal.values).astype(np.float32))
    assert corpus["mps_error_bound"] == max(float(_host(ideal.error_bound).max()), float(_host(under.error_bound).max()))
