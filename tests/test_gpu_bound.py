"""Parameter binding on the device: mlqem_sim_run_bound_f64 and mlqem_sim_shift_combine_f64 against the host interpreter of the
record format (tests/bound_cases.py) and the numpy oracle on the bound circuits (tests/sim_cases.py).

Every comparison uses the bound DERIVED in bound_cases.py, with the ASSUMED K_DEV = 4 ulp for the device library's double sin /
cos, and every case asserts that its bound stays under 1e-11.  Bit-equality is asserted where the contract promises it: a template
without parameters against mlqem_sim_run_f64, a run alone / in a batch / in a permuted batch / in a replayed graph, the table form
against the plain form, a gradient from call to call and against the header's combine order."""
import functools
import math

import numpy as np
import pytest
import torch

import bound_cases as bc
import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import Circuit
from blackwater.data.synthetic import tfim_template, two_local
from blackwater.native import ops
from blackwater.sim.bound import shift_runs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = bc.grid()


def host(t):
    return t.cpu().numpy()


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_run(batch, theta, runs, shift, form=ops.SIM_BOUND_TABLE, outs=None, tensors=None):
    """One call of ops.sim_run_bound on ``runs`` [R, 4]: ``(values [R], term_values [R, T], norm [R])`` as numpy arrays (or the
    tensors, with ``outs`` given).  T = the largest term count."""
    runs = np.asarray(runs, dtype=np.int32).reshape(-1, 4)
    width = int(np.diff(batch.term_ptr).max())
    wave = np.asarray([batch.variant[c] == "wave" for c in runs[:, 0]], dtype=bool)
    ids = np.concatenate([np.flatnonzero(wave), np.flatnonzero(~wave)]).astype(np.int32)
    t = tensors or {k: up(getattr(batch, k)) for k in ("circ", "op_ptr", "ops", "params", "term_ptr", "terms", "coeff")}
    args = (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], up(np.asarray(theta, dtype=np.float64)),
            up(runs), up(np.asarray(shift, dtype=np.float64)), up(ids), int(wave.sum()), int((~wave).sum()),
            up(np.arange(len(runs) + 1, dtype=np.int64) * width), len(runs) * width)
    if outs is not None:
        return args
    values, term_values, norm = ops.sim_run_bound(*args, form=form)
    return host(values), host(term_values).reshape(len(runs), width), host(norm)


@functools.lru_cache(maxsize=None)
def case_runs(name):
    """The runs of a grid case and their references, computed once: every row unshifted and with every shifted-op choice."""
    _, t, terms, noise, n_rows, span = next(c for c in GRID if c[0] == name)
    batch = sim.compile_templates([t], [terms], noise)
    theta = bc.thetas(n_rows, t.num_parameters, seed=3, span=span)
    runs, shift = [], []
    for row in range(n_rows):
        for j, sop in enumerate(bc.shifted_ops(batch, 0)):
            runs.append((0, row, sop, 0))
            shift.append(0.5 * math.pi if (row + j) % 2 == 0 else -0.5 * math.pi)
    interp = [bc.interpret_bound(batch, r, theta, s) for r, s in zip(runs, shift)]
    oracle = [sc.simulate(bc.bound_circuit(t, batch, 0, theta[r[1], :t.num_parameters], r[2], s), terms, noise) for r, s in zip(runs, shift)]
    return batch, theta, np.asarray(runs, dtype=np.int32), np.asarray(shift), interp, oracle


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID, ids=[c[0] for c in GRID])
def test_every_run_against_the_interpreter_and_the_oracle(case):
    """Vector n = 1, 2, 4, 8 (wave), 9, 11 (workgroup); density n = 1, 2, 4 (wave), 5 (workgroup); every parameterised kind in
    both modes; 0, 1, 64, 65 (and at n = 9: 256, 257) parameterised records; 1, 3, 5 rows (the last wave-variant workgroup partly
    filled); shifted op = first, last, a fixed record, none; one parameter in many records; |phi| up to 1e3.  No run is excluded."""
    name, t, terms, noise, n_rows, _ = case
    tb, vb = bc.term_bound(t, noise), bc.value_bound(t, terms, noise)
    assert tb < bc.CAP and vb < bc.CAP
    batch, theta, runs, shift, interp, oracle = case_runs(name)
    values, term_values, norm = device_run(batch, theta, runs, shift)
    worst = [0.0, 0.0]
    for r in range(len(runs)):
        for j, ref in enumerate((interp[r], oracle[r])):
            dv, dt = abs(values[r] - ref[0]), float(np.abs(term_values[r] - ref[1]).max())
            worst[j] = max(worst[j], dv, dt)
            assert dv <= vb and dt <= tb and abs(norm[r] - ref[2]) <= tb, (name, runs[r].tolist(), "interpreter" if j == 0 else "oracle", dv, dt)
    print(f"{name} ({batch.variant[0]}, {int(batch.op_counts[0])} records, {len(runs)} runs): max |device - interpreter| {worst[0]:.3e}, "
          f"|device - oracle| {worst[1]:.3e} <= {tb:.3e}")
    assert batch.variant == ["wave" if (t.num_qubits <= 8 if noise is None else t.num_qubits <= 4) else "workgroup"]


@pytest.mark.parametrize("case", GRID, ids=[c[0] for c in GRID])
def test_table_form_equals_plain_form(case):
    batch, theta, runs, shift, _, _ = case_runs(case[0])
    a, b = device_run(batch, theta, runs, shift, ops.SIM_BOUND_TABLE), device_run(batch, theta, runs, shift, ops.SIM_BOUND_PLAIN)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- bit-equalities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [None, sc.StepNoise(4)], ids=["vector", "density"])
def test_template_without_parameters_gives_the_bits_of_sim_run(noise):
    sizes = (1, 4, 8, 9, 11) if noise is None else (1, 3, 4, 5)
    circs = [sc.random_program(n, 30, seed=n, measure=noise is not None) for n in sizes]
    obs = [sc.term_set(n, alphabet="IXYZ" if noise is None else "IZ") for n in sizes]
    want = [host(x) for x in sim.run_batch(sim.compile_programs(circs, obs, noise), DEV)]
    batch = sim.compile_templates(circs, obs, noise)
    runs = np.asarray([(c, 0, -1, 0) for c in range(len(circs))], dtype=np.int32)
    for form in (ops.SIM_BOUND_TABLE, ops.SIM_BOUND_PLAIN):
        values, term_values, norm = device_run(batch, np.zeros((1, 1)), runs, np.zeros(len(circs)), form)
        assert np.array_equal(values, want[0]) and np.array_equal(norm, want[2])
        assert np.array_equal(term_values.reshape(-1), want[1])   # 12 terms each: the padded rows are the flat layout


def _mixed_batch():
    """Two templates, both variants, both with shifted runs: (batch, theta, runs, shift)."""
    ta, pa = bc.mixed_template(4, 24, seed=4)
    tb_, pb = bc.mixed_template(9, 24, seed=9)
    batch = sim.compile_templates([ta, tb_], [sc.term_set(4, seed=4), sc.term_set(9, seed=9)])
    theta = bc.thetas(3, max(pa, pb), seed=8)
    runs, shift = [], []
    for c in (0, 1):
        for row in range(3):
            for sop in (-1, int(batch.occ_op[int(batch.occ_ptr[c])]), int(batch.occ_op[int(batch.occ_ptr[c + 1]) - 1])):
                runs.append((c, row, sop, 0))
                shift.append(0.5 * math.pi if row != 1 else -0.5 * math.pi)
    return (ta, tb_), batch, theta, np.asarray(runs, dtype=np.int32), np.asarray(shift)


def test_the_same_bits_alone_in_a_batch_permuted_and_in_a_replayed_graph():
    (ta, tb_), batch, theta, runs, shift = _mixed_batch()
    assert batch.variant == ["wave", "workgroup"]
    eager = device_run(batch, theta, runs, shift)
    terms = [sc.term_set(4, seed=4), sc.term_set(9, seed=9)]
    for r in (0, 4, 9, 17):   # against the oracle, so that the batch is not only equal to itself
        c, row, sop, _ = (int(v) for v in runs[r])
        t = (ta, tb_)[c]
        ref = sc.simulate(bc.bound_circuit(t, batch, c, theta[row, :t.num_parameters], sop, shift[r]), terms[c], None)
        assert abs(eager[0][r] - ref[0]) <= bc.value_bound(t, terms[c])
    for r in range(0, len(runs), 3):
        one = device_run(batch, theta, runs[r:r + 1], shift[r:r + 1])
        assert one[0][0] == eager[0][r] and np.array_equal(one[1][0], eager[1][r]) and one[2][0] == eager[2][r]
    perm = np.random.default_rng(1).permutation(len(runs))
    shuffled = device_run(batch, theta, runs[perm], shift[perm])
    assert all(np.array_equal(s, e[perm]) for s, e in zip(shuffled, eager))
    width = eager[1].shape[1]
    outs = {"values": torch.zeros(len(runs), dtype=torch.float64, device=DEV),
            "term_values": torch.zeros(len(runs) * width, dtype=torch.float64, device=DEV),
            "norm": torch.zeros(len(runs), dtype=torch.float64, device=DEV)}
    args = device_run(batch, theta, runs, shift, outs=outs)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.sim_run_bound(*args, **outs)   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sim_run_bound(*args, **outs)
    for _ in range(2):
        for o in outs.values():
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(outs["values"]), eager[0]) and np.array_equal(host(outs["term_values"]).reshape(-1, width), eager[1])
        assert np.array_equal(host(outs["norm"]), eager[2])


def test_split_batches_give_the_same_bits():
    """run_bound splits its runs by a byte budget, as run_trajectories splits its batches: the results do not depend on the split."""
    _, batch, theta, runs, shift = _mixed_batch()
    whole = [host(x) for x in sim.run_bound(batch, theta, runs, shift, DEV)]
    split = [host(x) for x in sim.run_bound(batch, theta, runs, shift, DEV, buffer_bytes=5 * (52 + 8 * 12))]   # five runs per call
    assert all(np.array_equal(a, b) for a, b in zip(whole, split))
    direct = device_run(batch, theta, runs, shift)
    assert all(np.array_equal(a, b) for a, b in zip(whole, direct))


# ---- gradients ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [None, sc.StepNoise(3, force=False)], ids=["ideal", "noisy"])
def test_parameter_shift_against_the_host_rule_on_oracle_values(noise):
    """``parameter_shift`` on tfim_template(4, 3) (two parameters, 9 + 12 occurrences, scale 2) and on a mixed template: within the
    bound times sum |scale| of the host rule on oracle values, bit-equal to the header's combine on the device's own values, and
    the same bits from call to call."""
    mixed, _ = bc.mixed_template(3, 20, seed=6)
    for t, n_rows in ((tfim_template(4, 3), 3), (mixed, 2)):
        terms = sc.term_set(t.num_qubits, seed=2)
        theta = bc.thetas(n_rows, t.num_parameters, seed=12)
        values, grads = (host(x) for x in sim.parameter_shift(t, terms, theta, noise, DEV))
        again = [host(x) for x in sim.parameter_shift(t, terms, theta, noise, DEV)]
        assert np.array_equal(values, again[0]) and np.array_equal(grads, again[1])
        batch = sim.compile_templates([t], [terms], noise)
        vb = bc.value_bound(t, terms, noise)
        assert vb < bc.CAP
        k = int(batch.occ_ptr[1])
        want = np.zeros((n_rows, t.num_parameters))
        for row in range(n_rows):
            ref = sc.simulate(t.bind_parameters(theta[row]), terms, noise)[0]
            assert abs(values[row] - ref) <= vb
            for j in range(k):
                sop, p, scale = int(batch.occ_op[j]), int(batch.occ_param[j]), float(batch.occ_scale[j])
                plus = sc.simulate(bc.bound_circuit(t, batch, 0, theta[row], sop, 0.5 * math.pi), terms, noise)[0]
                minus = sc.simulate(bc.bound_circuit(t, batch, 0, theta[row], sop, -0.5 * math.pi), terms, noise)[0]
                want[row, p] += 0.5 * scale * (plus - minus)
        tol = vb * np.asarray([np.abs(batch.occ_scale[batch.occ_param == p]).sum() for p in range(t.num_parameters)])
        err = np.abs(grads - want)
        print(f"{t.num_qubits} qubits, {k} occurrences: max |grad - host rule| {err.max():.3e} <= {tol.max():.3e}")
        assert np.all(err <= tol[None, :]) and np.abs(want).max() > 1e-3
        # the combine's order: the device's own shifted values through the header's rule in numpy, bit for bit
        runs, shift, groups = shift_runs(batch, np.zeros(n_rows, dtype=np.int64))
        v = device_run(batch, theta, runs, shift)[0]
        vp, vm = v[n_rows:n_rows + k * n_rows].reshape(k, n_rows), v[n_rows + k * n_rows:].reshape(k, n_rows)
        assert np.array_equal(grads, bc.host_combine(vp, vm, batch.occ_param, batch.occ_scale, t.num_parameters))
        assert np.array_equal(values, v[:n_rows])


def test_phi_is_rounded_step_by_step():
    """phi = scale * theta + offset is a rounded product and a rounded sum, not one fused multiply-add: h, p(phi) on one qubit
    gives <X> = cos phi, and at |phi| up to 1e3 the two ways to form phi differ by up to half an ulp of phi, 5e-14, which the
    cosine shows.  Bound: (K_DEV + K_HOST) u for the two cosines plus 8 u for the kernel's own products and sums."""
    from blackwater.data.circuit import CircuitOp
    from blackwater.sim import Param, Template

    scale, offset = 1.7, 0.3
    t = Template(1, 0, [CircuitOp("h", (0,)), CircuitOp("p", (0,), (), (Param(0, scale, offset),))])
    theta = np.random.default_rng(6).uniform(-500.0, 500.0, size=(512, 1))
    _, tv = sim.bound_expectation_values(t, [("X", 1.0)], theta, None, DEV)
    stepwise = np.asarray([bc.phi_of(scale, v, offset) for v in theta[:, 0]])
    fused = (np.longdouble(scale) * theta[:, 0].astype(np.longdouble) + np.longdouble(offset)).astype(np.float64)
    assert np.abs(np.cos(fused) - np.cos(stepwise)).max() > 100 * bc.U   # the check can tell the two apart
    err = np.abs(host(tv)[:, 0] - np.cos(stepwise)).max()
    print(f"max |<X> - cos(phi)| = {err / bc.U:.1f} u")
    assert err <= (bc.K_DEV + bc.K_HOST + 8) * bc.U


def test_combine_is_bit_equal_to_the_header_rule():
    """Several occurrences per parameter with scales that are no powers of two: a fused multiply-add would show."""
    rng = np.random.default_rng(5)
    vp, vm = rng.normal(size=(7, 5)), rng.normal(size=(7, 5))
    par, scale = np.asarray([1, 0, 1, 1, 0, 2, 1]), rng.uniform(-2, 2, size=7)
    order = np.argsort(par, kind="stable").astype(np.int32)
    occ_ptr = np.concatenate([[0], np.cumsum(np.bincount(par, minlength=4))]).astype(np.int64)
    got = host(ops.sim_shift_combine(up(vp), up(vm), up(occ_ptr), up(order), up(scale)))
    assert got.shape == (5, 4) and np.array_equal(got, bc.host_combine(vp, vm, par, scale, 4))
    again = host(ops.sim_shift_combine(up(vp), up(vm), up(occ_ptr), up(order), up(scale)))
    assert np.array_equal(got, again)


def test_parameter_shift_over_two_templates():
    ta, tb_ = tfim_template(3, 2), two_local(2, reps=1)
    oa, ob = sc.term_set(3, seed=1), sc.term_set(2, seed=1)
    rows = [bc.thetas(1, 2, seed=1)[0], bc.thetas(1, 4, seed=2)[0], bc.thetas(1, 2, seed=3)[0]]
    values, grads = (host(x) for x in sim.parameter_shift([ta, tb_, ta], [oa, ob, oa], rows, None, DEV))
    assert grads.shape == (3, 4) and np.all(grads[[0, 2], 2:] == 0.0)
    for k, (t, o) in enumerate(((ta, oa), (tb_, ob), (ta, oa))):
        v1, g1 = (host(x) for x in sim.parameter_shift(t, o, rows[k][None, :], None, DEV))
        assert v1[0] == values[k] and np.array_equal(g1[0], grads[k, :t.num_parameters])


# ---- the public surface ------------------------------------------------------------------------------------------------------------
def test_estimator_with_templates_equals_bound_expectation_values():
    t = two_local(4, reps=2)
    terms = sc.term_set(4, seed=3)
    theta = bc.thetas(5, t.num_parameters, seed=21)
    values, term_values = sim.bound_expectation_values(t, terms, theta, None, DEV)
    assert tuple(term_values.shape) == (5, 12)
    est = sim.DeviceEstimator(device=DEV)
    job = est.run([t] * 5, [terms] * 5, [list(r) for r in theta])
    assert job.job_id() == "sim-1" and np.array_equal(job.result().values, host(values))
    auto = sim.DeviceEstimator(device=DEV, method="auto").run([t] * 5, [terms] * 5, [list(r) for r in theta])
    assert np.array_equal(auto.result().values, host(values))
    bound = est.run([t.bind_parameters(r) for r in theta], [terms] * 5)   # the old path on host-bound circuits, and the job counter
    assert bound.job_id() == "sim-2"
    vb = bc.value_bound(t, terms)
    assert np.abs(bound.result().values - host(values)).max() <= 2 * vb
    for row in range(5):
        assert abs(host(values)[row] - sc.simulate(t.bind_parameters(theta[row]), terms)[0]) <= vb
    noisy = sim.DeviceEstimator(noise=sc.StepNoise(2, force=False), device=DEV)
    got = noisy.run([t, t.bind_parameters(theta[1])], [terms, terms], [list(theta[0]), []]).result().values   # a template beside a bound circuit
    for k in (0, 1):
        ref = sc.simulate(t.bind_parameters(theta[k]), terms, sc.StepNoise(2, force=False))[0]
        assert abs(got[k] - ref) <= bc.value_bound(t, terms, sc.StepNoise(2, force=False))


def test_learning_processor_receives_bound_circuits():
    from blackwater.data.backends import PauliObservable
    from blackwater.library.learning.estimator import LearningMethodEstimatorProcessor, learning

    seen = []

    class Stub(LearningMethodEstimatorProcessor):   # records what it is given and returns the value
        def process(self, expectation_value, circuits, observables, parameter_values):
            seen.append(circuits)
            return expectation_value

    t = two_local(3, reps=1)
    theta = bc.thetas(2, t.num_parameters, seed=2)
    obs = PauliObservable("ZZZ")
    est = learning(sim.DeviceEstimator, processor=Stub(), backend=None, skip_transpile=True)(device=DEV)
    values = est.run([t, t], [obs, obs], [list(r) for r in theta]).result().values
    want = host(sim.bound_expectation_values(t, obs, theta, None, DEV)[0])
    assert np.array_equal(np.asarray(values, dtype=np.float64), want)
    assert len(seen) == 2 and all(type(c) is Circuit for c in seen)
    assert [c.ops[0].params[0] for c in seen] == [float(theta[0, 0]), float(theta[1, 0])]
