"""The matrix-product-state kernels (mlqem_mps_run_f64, mlqem_mps_terms_f64, mlqem_mps_finish_f64) against the numpy interpreter of
the record format, against the dense oracle within the certificate, against the Clifford path at 100 qubits, and their bits
under batching, splitting and graph replay.  tests/mps_cases.py has the grid, the measured tolerance table and the conditions
that tests/test_mps_cpu.py asserts, so that no case is excluded here."""
import numpy as np
import pytest
import torch

import mps_cases as mc
import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import Circuit
from blackwater.data.synthetic import encode_corpus, tfim_circuit
from blackwater.native import ops
from blackwater.sim import compile_mps, run_mps

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = [c["id"] for c in mc.grid()]


def _host(t):
    return t.cpu().numpy()


def _bits(res):
    return [_host(getattr(res, k)) for k in ("values", "term_values", "norm", "discarded", "error_bound", "bond")]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case_id", ALL)
def test_device_against_the_interpreter(case_id):
    case = mc.case(case_id)
    batch = mc.lower(case)
    res = run_mps(batch, seed=case["seed"], device=DEV, keep_trajectories=True)
    ref, tol = mc.reference(case_id), mc.tolerance(case_id)
    traj = _host(res.traj_term_values)
    values, terms, norm = _host(res.values), _host(res.term_values), _host(res.norm)
    discarded, bound, bond = _host(res.discarded), _host(res.error_bound), _host(res.bond)
    count = case["trajectories"] or 1
    assert traj.shape == (count, len(batch.term_circ))
    stats = _host(res.traj_stats)
    assert not stats[:, :, 4].any(), "a decomposition reached the sweep cap while it still rotated"
    worst = 0.0
    for j, per in enumerate(ref):
        tb, te = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
        rows = np.stack([r["terms"] for r in per])
        worst = max(worst, float(np.max(np.abs(traj[:, tb:te] - rows))))
        assert np.max(np.abs(traj[:, tb:te] - rows)) <= tol                     # every trajectory's terms
        mean, err = mc.mean_and_error(rows)
        assert np.max(np.abs(terms[tb:te] - mean)) <= tol
        vals = np.array([r["value"] for r in per])
        vmean, verr = mc.mean_and_error(vals)
        scale = max(per[0]["abs_coeff"], 1.0)
        assert abs(values[j] - vmean) <= tol * scale
        assert abs(norm[j] - np.mean([r["norm"] for r in per])) <= tol
        if case["trajectories"] is None:
            assert res.std_error is None and res.term_std_error is None
        else:   # se = |x - mean| / sqrt(T (T - 1)): a perturbation of every x by tol moves it by at most tol / sqrt(T - 1)
            se_tol = 0.0 if count == 1 else tol / np.sqrt(count - 1) + (count + 8) * mc.U * (err.max() + 1.0)
            assert np.max(np.abs(_host(res.term_std_error)[tb:te] - err)) <= se_tol
            assert abs(_host(res.std_error)[j] - verr) <= se_tol * scale
        want_d, want_b = np.mean([r["discarded"] for r in per]), np.mean([r["error_bound"] for r in per])
        floor_d, floor_b = mc.stat_floor(per[0])
        assert abs(discarded[j] - want_d) <= tol * want_d + floor_d
        assert abs(bound[j] - want_b) <= tol * want_b + floor_b
        assert bond[j] == max(r["bond"] for r in per)
    print(f"{case_id}: worst term difference {worst:.2e}, tolerance {tol:.2e}, most sweeps {int(stats[:, :, 5].max())}")


@pytest.mark.parametrize("case_id", [c["id"] for c in mc.grid() if c["noise"] is None])
def test_device_against_the_dense_oracle_within_the_certificate(case_id):
    case = mc.case(case_id)
    res = run_mps(mc.lower(case), device=DEV)
    values, terms, bound, ptr = _host(res.values), _host(res.term_values), _host(res.error_bound), _host(res.term_ptr)
    for j, (circ, obs) in enumerate(zip(case["circuits"], case["observables"])):
        circ = Circuit.from_any(circ)
        value, want, _ = sc.simulate(circ, obs)
        total = sum(abs(c) for _, c in obs)
        assert np.max(np.abs(terms[ptr[j]:ptr[j + 1]] - want)) <= 2.0 * bound[j] + mc.tolerance(case_id)
        assert abs(values[j] - value) <= 2.0 * bound[j] * total + mc.tolerance(case_id) * max(total, 1.0)


def _width(case_id):
    """A width case on the device beside its interpreter run: norm, ``discarded``, ``error_bound`` and ``bond`` are compared here as on
    the grid (tests/test_mps_cpu.py asserts that these cases drop nothing but rounding), the terms by the caller."""
    case = mc.width(case_id)
    res = run_mps(mc.lower(case), device=DEV, keep_trajectories=True)
    ref, tol = [per[0] for per in mc.reference(case_id)], mc.tolerance(case_id)
    assert not _host(res.traj_stats)[:, :, 4].any()
    for j, r in enumerate(ref):
        floor_d, floor_b = mc.stat_floor(r)
        assert abs(_host(res.norm)[j] - r["norm"]) <= tol
        assert abs(_host(res.discarded)[j] - r["discarded"]) <= tol * r["discarded"] + floor_d
        assert abs(_host(res.error_bound)[j] - r["error_bound"]) <= tol * r["error_bound"] + floor_b
        assert int(_host(res.bond)[j]) == r["bond"]
    return case, res, ref, tol


def test_width_against_the_clifford_path():
    """100 qubits, 3 Trotter steps at Clifford angles: the MPS at bond 8 against the exact Clifford path on 100 single-Z terms
    (and against the interpreter).  Three steps at most double a bond three times, so bond 8 drops nothing but rounding.  The
    tolerance is the measured one of mps_cases.TABLE: the Clifford path is exact, and the interpreter's two runs differ from it as
    they differ from each other."""
    case, res, ref, tol = _width("width-clifford-n100-s3-b8")
    want = sim.clifford_expectation_values(case["circuits"], case["observables"], None, DEV)
    bound = _host(res.error_bound)
    terms, exact = _host(res.term_values).reshape(3, 100), _host(want[1]).reshape(3, 100)
    print("width: largest difference", np.abs(terms - exact).max(), "tolerance", tol, "certificates", bound, "bonds", _host(res.bond))
    for j in range(3):
        assert np.max(np.abs(terms[j] - exact[j])) <= 2.0 * bound[j] + tol
        assert np.max(np.abs(terms[j] - ref[j]["terms"])) <= tol
        assert bound[j] <= mc.stat_floor(ref[j])[1], "Clifford TFIM states of 3 steps fit bond 8: nothing but rounding is dropped"
    assert np.max(np.abs(_host(res.values) - _host(want[0]))) <= 100 * (2.0 * bound.max() + tol)   # 100 terms of coefficient 1


def test_width_against_the_interpreter():
    case, res, ref, tol = _width("width-tfim-n64-s2-b4")
    print("width: largest difference", np.abs(_host(res.term_values) - ref[0]["terms"]).max(), "tolerance", tol)
    assert np.max(np.abs(_host(res.term_values) - ref[0]["terms"])) <= tol
    assert abs(_host(res.values)[0] - ref[0]["value"]) <= 64 * tol   # 64 terms of coefficient 1
    assert ref[0]["bond"] == 4


def test_an_empty_noise_model_is_the_ideal_run():
    case = mc.case("random-b32")   # untruncated: the fused and the unfused lowering give the same state
    ideal = run_mps(mc.lower(case), device=DEV)
    noisy = run_mps(compile_mps(case["circuits"], case["observables"], sim.NoiseModel(), trajectories=5), device=DEV, keep_trajectories=True)
    traj = _host(noisy.traj_term_values)
    assert all(np.array_equal(traj[t], traj[0]) for t in range(5)), "no draw: every trajectory is the same run"
    # the noisy lowering fuses nothing, so it is another ordering of the same arithmetic
    assert np.max(np.abs(_host(noisy.term_values) - _host(ideal.term_values))) <= mc.tolerance("random-b32")
    assert np.max(np.abs(_host(noisy.std_error))) <= 1e-15 and np.max(np.abs(_host(noisy.term_std_error))) <= 1e-15
    one = run_mps(compile_mps(case["circuits"], case["observables"], sim.NoiseModel(), trajectories=1), device=DEV)
    assert not _host(one.std_error).any() and not _host(one.term_std_error).any()


def test_same_bits_alone_in_a_batch_and_in_any_split():
    case = mc.case("noisy-depol-T64")
    noise = mc.noise_model("depol", 11)
    whole = run_mps(mc.lower(case), seed=11, device=DEV, keep_trajectories=True)
    full = _bits(whole) + [_host(whole.traj_term_values)]
    ptr = _host(whole.term_ptr)
    for j in (0, 2):   # alone, with its batch key
        alone = run_mps(compile_mps([case["circuits"][j]], [case["observables"][j]], noise, 64, case["max_bond"]), seed=11, run_keys=[j],
                        device=DEV, keep_trajectories=True)
        assert np.array_equal(_host(alone.values), full[0][j:j + 1]) and np.array_equal(_host(alone.term_values), full[1][ptr[j]:ptr[j + 1]])
        assert np.array_equal(_host(alone.error_bound), full[4][j:j + 1]) and np.array_equal(_host(alone.bond), full[5][j:j + 1])
        assert np.array_equal(_host(alone.traj_term_values), full[6][:, ptr[j]:ptr[j + 1]])
    # two splits of the batch: by circuits (one circuit's trajectories per launch) and by trajectories (a few units per launch)
    per_unit = ops.mps_workspace_bytes(5, case["max_bond"], 1)
    for budget in (per_unit * 64, per_unit * 7, 1):
        split = run_mps(mc.lower(case), seed=11, device=DEV, keep_trajectories=True, buffer_bytes=budget)
        assert _same(_bits(split) + [_host(split.traj_term_values)], full), budget
    # a prefix of the trajectories
    short = run_mps(compile_mps(case["circuits"], case["observables"], noise, 16, case["max_bond"]), seed=11, device=DEV, keep_trajectories=True)
    assert np.array_equal(_host(short.traj_term_values), full[6][:16])
    # another seed is another sample
    assert not np.array_equal(_host(run_mps(mc.lower(case), seed=12, device=DEV).values), full[0])


def test_a_replayed_graph_gives_the_same_bits():
    case = mc.case("noisy-overrot-T64")
    batch = mc.lower(case)
    eager = run_mps(batch, seed=3, device=DEV, keep_trajectories=True)
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
                        t["readout"], (0, b), (0, n_terms), (0, count), count, 3, batch.max_bond, batch.cutoff, widest, workspace,
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
        assert np.array_equal(_host(traj_terms), _host(eager.traj_term_values))
        for k in ("values", "term_values", "norm", "discarded", "error_bound", "bond", "std_error", "term_std_error"):
            assert np.array_equal(_host(out[k]), _host(getattr(eager, k))), k


def test_estimator_metadata():
    case = mc.case("tfim-cx-J1.9-s3-b4")
    est = sim.DeviceEstimator(device=DEV, method="mps", max_bond=4)
    got = est.run(case["circuits"], case["observables"]).result()
    ref = mc.reference(case["id"])[0][0]
    assert abs(got.values[0] - ref["value"]) <= mc.tolerance(case["id"]) * max(ref["abs_coeff"], 1.0)
    assert set(got.metadata[0]) == {"truncation_error_bound", "max_bond"} and got.metadata[0]["max_bond"] == 4
    assert abs(got.metadata[0]["truncation_error_bound"] - ref["error_bound"]) <= mc.tolerance(case["id"]) * ref["error_bound"] + mc.stat_floor(ref)[1]
    noisy = mc.case("noisy-readout-T64")
    est = sim.DeviceEstimator(mc.noise_model("readout", 11), DEV, method="mps", trajectories=64, seed=5)
    got = est.run(noisy["circuits"], noisy["observables"]).result()
    direct = sim.mps_expectation_values(noisy["circuits"], noisy["observables"], mc.noise_model("readout", 11), trajectories=64, seed=5,
                                        run_keys=sim.default_run_keys(3, 1 << 32), device=DEV)
    assert np.array_equal(got.values, _host(direct.values))
    assert all(set(m) == {"truncation_error_bound", "max_bond", "std_error", "trajectories"} and m["trajectories"] == 64 for m in got.metadata)
    assert [m["std_error"] for m in got.metadata] == _host(direct.std_error).tolist()
    with pytest.raises(ValueError, match="method='mps'.*shots= is not supported"):
        sim.DeviceEstimator(device=DEV, method="mps", shots=100)
    with pytest.raises(ValueError, match="method='mps'.*shots= is not supported"):
        sim.DeviceEstimator(device=DEV, method="mps").run(case["circuits"], case["observables"], shots=100)


def test_encode_corpus_takes_wide_labels_from_the_mps_path():
    nq = 24
    circuits = [tfim_circuit(nq, s, j, two_q="cx") for s, j in ((1, 0.4), (2, 1.0), (3, 1.7))]
    noise = sim.NoiseModel.from_backend(mc.tc.table(nq))
    plain = encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=noise, device=DEV, trajectories=8)
    got = encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=noise, device=DEV, trajectories=8, mps_bond=8)
    assert "mps_error_bound" not in plain and "mps_error_bound" in got
    synthetic = encode_corpus(circuits, nq, two_q="cx", seed=7)
    assert np.array_equal(plain["y"], synthetic["y"]) and np.array_equal(plain["noisy"], synthetic["noisy"]), "over the caps: synthetic as ever"
    z_qubits = [int(np.flatnonzero(o[0, 2::4])[0]) for o in got["observable"]]
    labels = ["".join("Z" if q == z else "I" for q in reversed(range(nq))) for z in z_qubits]
    ideal = sim.mps_expectation_values(circuits, labels, max_bond=8, device=DEV)
    under = sim.mps_expectation_values(circuits, labels, noise, max_bond=8, trajectories=8, seed=7, run_keys=np.arange(3), device=DEV)
    assert np.array_equal(got["y"][:, 0], _host(ideal.values).astype(np.float32))
    assert np.array_equal(got["noisy"][:, 0], _host(under.values).astype(np.float32))
    assert got["mps_error_bound"] == max(float(_host(ideal.error_bound).max()), float(_host(under.error_bound).max()))
    assert all(np.array_equal(a, b) for a, b in zip(got["x"], plain["x"]))
