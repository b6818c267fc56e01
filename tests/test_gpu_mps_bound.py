"""Parameter binding on the matrix-product-state path, on the device: the pool mlqem_mps_bind_f64 writes against the host
interpreter of the factor program within the derived bound, the bound batch run by ``run_mps`` bit for bit, values and noisy
trajectories against the numpy interpreter of the bound copies' own lowering, gradients against the CPU's shift rule, the bits under
batching, splitting and graph replay, and the estimator.  tests/mps_bound_cases.py has the grid, the interpreter and the bounds;
tests/test_mps_bound_cpu.py asserts the conditions, so that no case is excluded here."""
import functools
import math

import numpy as np
import pytest
import torch

import bound_cases as bc
import mps_bound_cases as mbc
import mps_cases as mc
import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import CircuitOp
from blackwater.native import ops
from blackwater.sim import MpsBoundRun, Param, Template, compile_mps_templates, run_mps, run_mps_bound
from blackwater.sim.mps import mps_shift_runs

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL = [c["id"] for c in mbc.grid()]


def _host(t):
    return t.cpu().numpy()


def _bits(res):
    return [_host(getattr(res, k)) for k in ("values", "term_values", "norm", "discarded", "error_bound", "bond")]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _run(case_id):
    """The case's rows as one chunk on the device, once: ``(plan, result with the trajectories kept)``."""
    c = mbc.case(case_id)
    plan = MpsBoundRun(mbc.lower(case_id), c["rows"], mbc.plain_runs(c), None, c["seed"], None, DEV)
    assert len(plan.chunks) == 1
    plan.launch()
    torch.cuda.synchronize()
    return plan, plan.result(keep_trajectories=True)


@pytest.mark.parametrize("case_id", ALL)
def test_the_pool_against_bind_host(case_id):
    c, batch = mbc.case(case_id), mbc.lower(case_id)
    got = _run(case_id)[0].bound_batch()
    worst, at = 0.0, 0
    for r, run in enumerate(mbc.plain_runs(c)):
        pool, rows = mbc.bind_host(batch, run, c["rows"])
        ob, oe = int(got.op_ptr[r]), int(got.op_ptr[r + 1])
        want_rows = rows.copy()
        want_rows[:, 3] += at
        assert np.array_equal(got.ops[ob:oe], want_rows), "the template's rows with the pool offset rebased"
        have = got.params[at:at + pool.shape[0]]
        bound = mbc.mask_of(batch, int(run[0]), mbc.bind_bound)
        assert np.array_equal(have[bound == 0.0], pool[bound == 0.0]), "copied entries are bit-equal"
        diff = np.abs(have - pool)
        if np.any(bound > 0.0):
            worst = max(worst, float(np.max(diff[bound > 0.0] / bound[bound > 0.0])))
        assert np.all(diff <= bound), (case_id, r, float(diff.max()))
        at += pool.shape[0]
    assert got.params.shape[0] == at + 32
    print(f"{case_id}: device pool against bind_host, largest ratio to the bound {worst:.3f} (K_DEV = {mbc.K_DEV} is assumed)")


@pytest.mark.parametrize("case_id", ALL)
def test_run_mps_on_the_downloaded_batch_gives_the_same_bits(case_id):
    c = mbc.case(case_id)
    plan, res = _run(case_id)
    again = run_mps(plan.bound_batch(), seed=c["seed"], device=DEV, keep_trajectories=True)
    assert _same(_bits(again), _bits(res))
    assert np.array_equal(_host(again.traj_stats), _host(res.traj_stats)) and np.array_equal(_host(again.traj_term_values), _host(res.traj_term_values))


def _against_reference(case_id, res, ref, ptr):
    """Every trajectory's terms, the means, norm, ``discarded``, ``error_bound`` and ``bond`` as tests/test_gpu_mps.py compares them."""
    tol = mbc.tolerance(case_id)
    traj, values, terms, norm = _host(res.traj_term_values), _host(res.values), _host(res.term_values), _host(res.norm)
    discarded, bound, bond, stats = _host(res.discarded), _host(res.error_bound), _host(res.bond), _host(res.traj_stats)
    assert not stats[:, :, 4].any(), "a decomposition reached the sweep cap while it still rotated"
    worst = 0.0
    for j, per in enumerate(ref):
        tb, te = int(ptr[j]), int(ptr[j + 1])
        rows = np.stack([r["terms"] for r in per])
        worst = max(worst, float(np.max(np.abs(traj[:, tb:te] - rows))))
        assert np.max(np.abs(traj[:, tb:te] - rows)) <= tol
        mean, _ = mc.mean_and_error(rows)
        assert np.max(np.abs(terms[tb:te] - mean)) <= tol
        vmean, _ = mc.mean_and_error(np.array([r["value"] for r in per]))
        assert abs(values[j] - vmean) <= tol * max(per[0]["abs_coeff"], 1.0)
        assert abs(norm[j] - np.mean([r["norm"] for r in per])) <= tol
        want_d, want_b = np.mean([r["discarded"] for r in per]), np.mean([r["error_bound"] for r in per])
        floor_d, floor_b = mc.stat_floor(per[0])
        assert abs(discarded[j] - want_d) <= tol * want_d + floor_d
        assert abs(bound[j] - want_b) <= tol * want_b + floor_b
        assert bond[j] == max(r["bond"] for r in per)
    print(f"{case_id}: worst term difference {worst:.2e}, tolerance {tol:.2e}, most sweeps {int(stats[:, :, 5].max())}")


@pytest.mark.parametrize("case_id", mbc.IDEAL)
def test_values_against_the_interpreter_of_the_bound_copies(case_id):
    plan, res = _run(case_id)
    _against_reference(case_id, res, mbc.reference(case_id), plan.run_term_ptr)


@pytest.mark.parametrize("case_id", mbc.NOISY)
def test_noisy_trajectories_against_the_bound_copies(case_id):
    """T = 4 trajectories, the same seed and run keys: every trajectory against the interpreter, and, within the same tolerance,
    against ``run_mps`` on the host-bound copies."""
    c = mbc.case(case_id)
    plan, res = _run(case_id)
    _against_reference(case_id, res, mbc.reference(case_id), plan.run_term_ptr)
    host = run_mps(mbc.lower_copies(case_id), seed=c["seed"], device=DEV, keep_trajectories=True)
    assert np.array_equal(_host(host.term_ptr), plan.run_term_ptr)
    assert np.max(np.abs(_host(host.traj_term_values) - _host(res.traj_term_values))) <= mbc.tolerance(case_id)
    assert np.array_equal(_host(host.bond), _host(res.bond))
    assert res.std_error is not None and res.term_std_error is not None


def test_a_template_without_parameters_gives_the_bits_of_run_mps():
    c = mbc.case("fixed-n5")
    _, res = _run("fixed-n5")
    want = run_mps(mbc.lower_copies("fixed-n5"), seed=c["seed"], device=DEV)
    assert _same(_bits(want), _bits(res))
    noise = mc.noise_model("depol", 11)
    import traj_cases as tc

    circuits, obs = [tc.line_circuit(n, 900 + n, measure=True) for n in (3, 5)], [mc.terms_of(n, n) for n in (3, 5)]
    bound = run_mps_bound(compile_mps_templates(circuits, obs, noise, 4, 8), np.zeros((2, 1)), seed=9, device=DEV, keep_trajectories=True)
    plain = run_mps(sim.compile_mps(circuits, obs, noise, 4, 8), seed=9, device=DEV, keep_trajectories=True)
    assert _same(_bits(plain) + [_host(plain.traj_term_values), _host(plain.std_error)], _bits(bound) + [_host(bound.traj_term_values), _host(bound.std_error)])


def _shift_case(noisy):
    ops_ = [CircuitOp("h", (0,)), CircuitOp("ry", (1,), (), (Param(0, 1.5, 0.1),)), CircuitOp("rx", (0,), (), (Param(1),)),
            CircuitOp("cx", (0, 1)), CircuitOp("rzz", (2, 1), (), (Param(0, -0.5),)), CircuitOp("rz", (2,), (), (Param(2, 2.0),)),
            CircuitOp("p", (0,), (), (Param(1, 0.75, -0.2),)), CircuitOp("h", (2,)), CircuitOp("u1", (1,), (), (Param(2),)),
            CircuitOp("cx", (2, 1)), CircuitOp("ry", (0,), (), (Param(2, -1.0, 0.3),)), CircuitOp("sx", (1,)),
            CircuitOp("rx", (2,), (), (Param(0),))]
    t = Template(3, 0, ops_, [], 3)
    lam = {(op.name, op.qubits): 0.1 + 0.1 * len(op.qubits) for op in t.ops}
    return t, [("ZIZ", 0.7), ("XXI", -0.4), ("IYZ", 0.5), ("ZZZ", 1.0)], (sim.NoiseModel(lam) if noisy else None), (4 if noisy else None)


@pytest.mark.parametrize("noisy", [False, True])
def test_gradients_against_the_shift_rule_on_the_host(noisy):
    """Device gradients against the CPU's: the factor program through ``bind_host`` and the numpy MPS interpreter, run by run, with the
    row's run key in every run, combined by ``bound_cases.host_combine``.  Bound: the values bound (16 x the measured LAPACK-versus-
    Jacobi difference over these runs, floored at the term bound, times sum |coeff|) times the sum of |scale| over the parameter's
    occurrences -- each shifted pair enters as 0.5 scale (v+ - v-)."""
    t, terms, noise, traj = _shift_case(noisy)
    rows = np.array([[0.37, -1.21, 0.83], [2.9, 0.4, -2.2]])
    keys, seed = np.array([5, (7 << 32) + 1], dtype=np.int64), 21
    values, grads = sim.parameter_shift(t, terms, rows, noise, DEV, method="mps", trajectories=traj, seed=seed, run_keys=keys)
    values, grads = _host(values), _host(grads)
    batch = compile_mps_templates([t], [terms], noise, traj)
    runs, shift, groups = mps_shift_runs(batch, np.zeros(2, dtype=np.int64))
    k, b = int(batch.occ_ptr[1]), 2
    ref = {}
    for method in ("lapack", "jacobi"):
        ref[method] = np.array([np.mean([mc.interpret(mbc.host_copy(batch, run, rows, sh), 0, method, tr, seed, int(keys[run[1]]))["value"]
                                         for tr in range(traj or 1)]) for run, sh in zip(runs, shift)])
    margins = [mc.interpret(mbc.host_copy(batch, run, rows, sh), 0, "lapack", tr, seed, int(keys[run[1]]))["margin"]
               for run, sh in zip(runs, shift) for tr in range(traj or 1)] if noisy else [math.inf]
    assert min(margins) >= mc.MARGIN
    total = sum(abs(cf) for _, cf in terms)
    tol = max(mc.FACTOR * float(np.max(np.abs(ref["lapack"] - ref["jacobi"]))), sc.term_bound(t.placeholder())) * max(total, 1.0)
    want = ref["lapack"]
    assert np.max(np.abs(values - want[:b])) <= tol
    want_grad = bc.host_combine(want[b:b + k * b].reshape(k, b), want[b + k * b:].reshape(k, b), batch.occ_param, batch.occ_scale, 3)
    worst = 0.0
    for p in range(3):
        scale = float(np.sum(np.abs(batch.occ_scale[batch.occ_param == p])))
        worst = max(worst, float(np.max(np.abs(grads[:, p] - want_grad[:, p]))) / (tol * scale))
        assert np.max(np.abs(grads[:, p] - want_grad[:, p])) <= tol * scale, p
    assert np.abs(grads).max() > 1e-3
    print(f"gradients (noisy={noisy}): largest ratio to the bound {worst:.3f}, values bound {tol:.2e}")


@pytest.mark.parametrize("case_id", ["mixed-n2-n4-n5", "noisy-depol-T4"])
def test_the_same_bits_alone_in_a_batch_under_splits_and_in_a_replayed_graph(case_id):
    c, batch = mbc.case(case_id), mbc.lower(case_id)
    runs, n_rows = mbc.plain_runs(c), len(c["pair"])
    keys = np.arange(n_rows, dtype=np.int64) + (3 << 32)
    full = run_mps_bound(batch, c["rows"], runs, seed=c["seed"], run_keys=keys, device=DEV, keep_trajectories=True)
    bits = _bits(full) + [_host(full.traj_term_values), _host(full.traj_stats)]
    ptr = _host(full.term_ptr)
    for r in range(n_rows):   # alone
        one = run_mps_bound(batch, c["rows"], runs[r:r + 1], seed=c["seed"], run_keys=keys[r:r + 1], device=DEV, keep_trajectories=True)
        assert np.array_equal(_host(one.values), bits[0][r:r + 1]) and np.array_equal(_host(one.term_values), bits[1][ptr[r]:ptr[r + 1]])
        assert np.array_equal(_host(one.traj_stats)[:, 0], bits[7][:, r])
    widest = int(batch.n_qubits.max())
    per_unit = ops.mps_workspace_bytes(widest, c["max_bond"], 1)
    chunks = set()
    for budget in (per_unit * 2 * (c["trajectories"] or 1), per_unit * 3, 1):   # three splits: by runs, by a few units, one unit per launch
        plan = MpsBoundRun(batch, c["rows"], runs, None, c["seed"], keys, DEV, budget)
        chunks.add(len(plan.chunks))
        plan.launch()
        split = plan.result(keep_trajectories=True)
        assert _same(_bits(split) + [_host(split.traj_term_values), _host(split.traj_stats)], bits), budget
    assert len(chunks) >= 2 and min(chunks) > 1
    # the other limit of a launch, the pool entries a record can address, set to the largest bound copy
    most = int(np.diff(batch.pool_ptr)[runs[:, 0]].max())
    plan = MpsBoundRun(batch, c["rows"], runs, None, c["seed"], keys, DEV, None, pool_entries=most)
    assert len(plan.chunks) > 1 and all(size[1] <= most for size in plan.sizes)
    plan.launch()
    split = plan.result(keep_trajectories=True)
    assert _same(_bits(split) + [_host(split.traj_term_values), _host(split.traj_stats)], bits)
    with pytest.raises(ValueError, match="one bound copy holds"):
        MpsBoundRun(batch, c["rows"], runs, None, c["seed"], keys, DEV, None, pool_entries=most - 1)
    plan = MpsBoundRun(batch, c["rows"], runs, None, c["seed"], keys, DEV, per_unit * 3)   # bind + run of every chunk in one graph
    plan.launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.launch()
    for _ in range(2):
        for buf in (plan.out_pool, plan.out_ops, plan.traj_terms, plan.traj_norm, plan.traj_stats, *plan.out.values()):
            buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        again = plan.result(keep_trajectories=True)
        assert _same(_bits(again) + [_host(again.traj_term_values), _host(again.traj_stats)], bits)


def test_estimator_runs_templates_on_the_bound_path():
    c = mbc.case("mixed-n2-n4-n5")
    templates = [c["templates"][int(p)] for p in c["pair"]]
    observables = [c["observables"][int(p)] for p in c["pair"]]
    rows = [mbc.row_values(c, r) for r in range(len(templates))]
    est = sim.DeviceEstimator(device=DEV, method="mps", max_bond=8)
    job = est.run(templates, observables, rows)
    values, _, res = sim.bound_mps_expectation_values(templates, observables, rows, max_bond=8, run_keys=sim.default_run_keys(5, 1 << 32),
                                                      device=DEV, return_result=True)
    assert job.job_id() == "sim-1" and np.array_equal(job.result().values, _host(values))
    for m, b, k in zip(job.result().metadata, _host(res.error_bound), _host(res.bond)):
        assert m == {"truncation_error_bound": float(b), "max_bond": int(k)}
    assert est.run(templates, observables, rows).job_id() == "sim-2"
    c = mbc.case("noisy-depol-T4")
    templates, observables = [c["templates"][int(p)] for p in c["pair"]], [c["observables"][int(p)] for p in c["pair"]]
    rows = [mbc.row_values(c, r) for r in range(len(templates))]
    noise = mbc.noise_of(c)
    est = sim.DeviceEstimator(noise=noise, device=DEV, method="mps", max_bond=8, trajectories=4, seed=6)
    job = est.run(templates, observables, rows)
    values, terms, res = sim.bound_mps_expectation_values(templates, observables, rows, noise, 4, 8, seed=6,
                                                          run_keys=sim.default_run_keys(3, 1 << 32), device=DEV, return_result=True)
    assert np.array_equal(job.result().values, _host(values)) and terms.shape == (3, max(len(o) for o in observables))
    for m, e in zip(job.result().metadata, _host(res.std_error)):
        assert m["std_error"] == float(e) and m["trajectories"] == 4 and set(m) == {"truncation_error_bound", "max_bond", "std_error", "trajectories"}
    # bound circuits beside it keep their path, and the other methods keep their refusals
    t = templates[0]
    with pytest.raises(ValueError, match="template with free parameters"):
        sim.DeviceEstimator(noise=noise, device=DEV, method="trajectories").run([t], [observables[0]], [rows[0]])
    with pytest.raises(ValueError, match="template with free parameters"):
        sim.DeviceEstimator(device=DEV, method="mps_shots", shots=8).run([t], [observables[0]], [rows[0]])
    with pytest.raises(ValueError, match="template with free parameters"):
        sim.DeviceEstimator(device=DEV, method="clifford").run([t], [observables[0]], [rows[0]])
