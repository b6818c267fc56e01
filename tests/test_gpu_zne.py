"""Zero-noise extrapolation on the device (mlqem_sim_run_folded_f64, mlqem_zne_combine_f64, blackwater.sim.zne) against the
independent oracle of tests/zne_cases.py.

Every comparison uses the bound DERIVED in zne_cases.py (the per-factor bounds of sim_cases.py on the explicitly folded circuit,
weighted by the extrapolation weights); tests/test_zne_cpu.py asserts that every case here keeps it below 1e-10.  Bit-equality is
asserted where the contract promises it: the identity schedule against ``ops.sim_run``, every run against ``ops.sim_run`` on its
host-expanded and host-daggered program, a run alone against the same run in a batch, a captured graph against eager.
"""
import numpy as np
import pytest
import torch

import sim_cases as sc
import zne_cases as zc
from blackwater import sim, zne
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.native import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.cpu().numpy()


def strategy_of(desc, factors, degree):
    return zne.ZNEStrategy(noise_factors=factors, noise_amplifier=zc.make_amplifier(desc), extrapolator=zne.PolynomialExtrapolator(degree))


def check(circuits, observables, noise, factors, desc, what, degrees=zc.DEGREES):
    """One fused run per degree; per-factor terms, per-factor values, norm and the mitigated values and terms against the oracle."""
    run = None
    for degree in degrees:
        run = zne.zne_run(circuits, observables, noise, strategy_of(desc, factors, degree), DEV)
        values, tvs, norm = host(run.values), host(run.term_values), host(run.norm)
        mv, mt, ptr = host(run.mitigated_values), host(run.mitigated_terms), run.batch.term_ptr
        assert values.shape == (len(factors), len(circuits)) and tvs.shape == (len(factors), int(ptr[-1]))
        for k, (c, terms) in enumerate(zip(circuits, observables)):
            ref = zc.oracle(c, terms, noise, factors, desc, degree)
            b, e = int(ptr[k]), int(ptr[k + 1])
            dv = np.abs(values[:, k] - ref["values"])
            dt = np.abs(tvs[:, b:e] - ref["term_values"]).max(axis=1) if e > b else np.zeros(len(factors))
            dn = np.abs(norm[:, k] - 1.0)
            dmt = np.abs(mt[b:e] - ref["mitigated_terms"]) if e > b else np.zeros(0)
            print(f"{what} degree {degree} circuit {k} ({run.batch.variant[k]}): per factor |value| {dv.max():.3e} <= {ref['value_bounds'].max():.3e}, "
                  f"|terms| {dt.max():.3e} <= {ref['term_bounds'].max():.3e}, |norm - 1| {dn.max():.3e}; mitigated |value| "
                  f"{abs(mv[k] - ref['mitigated_value']):.3e} <= {ref['mitigated_value_bound']:.3e}, |terms| {dmt.max() if e > b else 0.0:.3e}")
            assert ref["mitigated_value_bound"] < zc.CAP
            assert (dv <= ref["value_bounds"]).all() and (dt <= ref["term_bounds"]).all() and (dn <= ref["term_bounds"]).all(), (what, k)
            assert abs(mv[k] - ref["mitigated_value"]) <= ref["mitigated_value_bound"] and (dmt <= ref["mitigated_term_bound"]).all(), (what, k)
            assert np.array_equal(run.schedules.achieved[:, k], ref["achieved"])
    return run


def run_plain(batch):
    t = batch.to(DEV)
    return [host(x) for x in ops.sim_run(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"],
                                         t["n_wave"], t["n_wg"])]


def assert_runs_equal_their_expanded_programs(run, what):
    """Row f of the folded call, bit for bit, against ``ops.sim_run`` on the program of zne_cases.expand (records copied, daggers
    applied in numpy): the inverse is formed without any new rounding."""
    values, tvs, norm = host(run.values), host(run.term_values), host(run.norm)
    for f in range(values.shape[0]):
        pv, pt, pn = run_plain(zc.expand(run.batch, run.schedules, f))
        assert np.array_equal(values[f], pv) and np.array_equal(tvs[f], pt) and np.array_equal(norm[f], pn), (what, f)


# ---- the grids -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", zc.density_cases(), ids=[c[0] for c in zc.density_cases()])
def test_density_grid(case):
    """n = 1, 2, 4 run a wave per run, n = 5 a workgroup; a depolarising op after every gate with lambda = 0 and lambda = 1 forced;
    all-gate local, two-qubit local (N = 0 at n = 1), global and random local folding with partial folds; linear and quadratic."""
    name, n, desc, factors = case
    c, terms, noise = zc.density_program(n)
    run = check([c], [terms], noise, factors, desc, name)
    assert run.batch.variant == ["wave" if n <= 4 else "workgroup"]
    assert_runs_equal_their_expanded_programs(run, name)
    if desc == zc.LOCAL_2Q and n == 1:   # nothing to fold: the same schedule at every factor, and sum w = 1
        assert np.array_equal(run.schedules.achieved, np.ones((3, 1)))
        v = host(run.values)
        assert v[0, 0] == v[1, 0] == v[2, 0] and abs(host(run.mitigated_values)[0] - v[0, 0]) <= 4 * zc.U * 3 * abs(v[0, 0])


@pytest.mark.parametrize("n", zc.VECTOR_N)
def test_vector_grid_global_folding(n):
    """State vectors (wave for n <= 8, workgroup beyond) with the whole circuit folded at factors 3 and 5: every gate kind runs as
    its inverse on the large shapes.  Against the oracle, and against the unfolded values (U^-1 U = 1) within the two bounds."""
    c, terms = zc.vector_program(n)
    run = check([c], [terms], None, (1, 3, 5), zc.GLOBAL, f"vector n={n}")
    assert run.batch.variant == ["wave" if n <= 8 else "workgroup"]
    assert_runs_equal_their_expanded_programs(run, f"vector n={n}")
    ref = zc.oracle(c, terms, None, (1, 3, 5), zc.GLOBAL, 1)
    values, tvs = host(run.values), host(run.term_values)
    for f in (1, 2):
        assert abs(values[f, 0] - values[0, 0]) <= ref["value_bounds"][f] + ref["value_bounds"][0]
        assert np.abs(tvs[f] - tvs[0]).max() <= ref["term_bounds"][f] + ref["term_bounds"][0]


@pytest.mark.parametrize("n", zc.READOUT_N)
@pytest.mark.parametrize("desc,factors", [(zc.LOCAL_ALL, (1, 3)), (zc.GLOBAL, zc.PARTIAL)], ids=["local", "global-partial"])
def test_readout_ops_run_once_after_the_folds(n, desc, factors):
    """I/Z observables with readout ops: applied once (the oracle's folded circuit is measured once), norm = Tr rho before them."""
    c, terms, noise = zc.readout_program(n)
    run = check([c], [terms], noise, factors, desc, f"readout n={n}", degrees=(1,))
    assert run.batch.circ[0, 2] == n
    assert_runs_equal_their_expanded_programs(run, f"readout n={n}")


# ---- bit-equality ------------------------------------------------------------------------------------------------------------------------
def _mixed(mode):
    if mode == "vector":
        circuits = [sc.random_program(5, 12, seed=60, with_id=False), Circuit(1, 0, []), sc.random_program(9, 10, seed=61),
                    Circuit(3, 0, [CircuitOp("h", (2,))]), sc.random_program(8, 10, seed=62), sc.random_program(11, 7, seed=63),
                    sc.random_program(2, 10, seed=64)]
        observables = [sc.term_set(5), [("Z", 1.0)], sc.term_set(9), [], sc.long_observable(8), sc.term_set(11), [("XY", 0.5)]]
        return circuits, observables, None
    circuits = [sc.random_program(4, 12, seed=65, with_id=False), sc.random_program(5, 10, seed=66), Circuit(2, 0, []),
                sc.random_program(1, 1, seed=67, with_id=False), sc.random_program(5, 1, seed=68, with_id=False), sc.random_program(3, 10, seed=69),
                sc.random_program(2, 10, seed=70)]
    observables = [sc.term_set(4), sc.term_set(5), [], [("Y", 1.0)], sc.long_observable(5), sc.term_set(3), [("ZZ", -1.0)]]
    return circuits, observables, sc.StepNoise(71)


@pytest.mark.parametrize("mode", ["vector", "density"])
def test_a_run_is_bit_equal_alone_in_any_batch_and_to_the_plain_kernel(mode):
    """Seven circuits of both variants (0, 1 and 12 ops; 0 terms) at factors (1, 2.2, 5): 21 runs, 12 or 15 of them a wave per run, so
    a workgroup of the wave variant is partly empty and its four runs have schedules of different lengths.  Row 0 is the identity
    schedule and equals ``ops.sim_run`` on the same batch; every row equals ``ops.sim_run`` on its expanded program; batches of 1, 3,
    5 and 7 circuits and two calls give the same bits."""
    circuits, observables, noise = _mixed(mode)
    strategy = strategy_of(zc.LOCAL_ALL, (1, 2.2, 5), 2)
    alone = [zne.zne_run([c], [o], noise, strategy, DEV) for c, o in zip(circuits, observables)]
    for size in (1, 3, 5, 7):
        run = zne.zne_run(circuits[:size], observables[:size], noise, strategy, DEV)
        again = zne.zne_run(circuits[:size], observables[:size], noise, strategy, DEV)
        values, tvs, norm, mv, mt = (host(x) for x in (run.values, run.term_values, run.norm, run.mitigated_values, run.mitigated_terms))
        for a, b in zip((values, tvs, norm, mv, mt), (again.values, again.term_values, again.norm, again.mitigated_values, again.mitigated_terms)):
            assert np.array_equal(a, host(b))
        plain = run_plain(run.batch)
        assert np.array_equal(values[0], plain[0]) and np.array_equal(tvs[0], plain[1]) and np.array_equal(norm[0], plain[2])
        assert_runs_equal_their_expanded_programs(run, f"{mode} batch of {size}")
        ptr = run.batch.term_ptr
        for k in range(size):
            b, e = int(ptr[k]), int(ptr[k + 1])
            one = alone[k]
            assert np.array_equal(values[:, k], host(one.values)[:, 0]) and np.array_equal(norm[:, k], host(one.norm)[:, 0])
            assert np.array_equal(tvs[:, b:e], host(one.term_values)) and mv[k] == host(one.mitigated_values)[0]
            assert np.array_equal(mt[b:e], host(one.mitigated_terms))
            if e == b:
                assert (values[:, k] == 0.0).all() and mv[k] == 0.0
        if size == 7:
            assert set(run.batch.variant) == {"wave", "workgroup"} and run.schedules.n_wave % 4 != 0
            lengths = np.diff(run.schedules.sched_ptr).reshape(3, 7)
            assert (lengths[2] > lengths[0]).any() and 0 in lengths
    check(circuits, observables, noise, (1, 2.2, 5), zc.LOCAL_ALL, f"{mode} mixed batch", degrees=(2,))


def test_folded_run_and_combine_in_a_captured_graph():
    circuits, observables, noise = _mixed("density")
    strategy = strategy_of(zc.GLOBAL, zc.PARTIAL, 2)
    eager = zne.zne_run(circuits, observables, noise, strategy, DEV)
    t, s = eager.batch.to(DEV), eager.schedules.to(DEV)
    f, b, n_terms = 4, 7, int(eager.batch.term_ptr[-1])
    w = torch.from_numpy(eager.weights).to(DEV)
    outs = {"values": torch.zeros(f, b, dtype=torch.float64, device=DEV), "term_values": torch.zeros(f, n_terms, dtype=torch.float64, device=DEV),
            "norm": torch.zeros(f, b, dtype=torch.float64, device=DEV)}
    mixed = {"mitigated_terms": torch.zeros(n_terms, dtype=torch.float64, device=DEV), "mitigated_values": torch.zeros(b, dtype=torch.float64, device=DEV)}

    def both():
        ops.sim_run_folded(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], s["sched_ptr"], s["sched"],
                           s["ids"], eager.schedules.n_wave, eager.schedules.n_wg, f, **outs)
        ops.zne_combine(outs["term_values"], w, t["term_ptr"], t["coeff"], **mixed)

    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        both()   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for _ in range(2):
        for o in list(outs.values()) + list(mixed.values()):
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(outs["values"]), host(eager.values)) and np.array_equal(host(outs["term_values"]), host(eager.term_values))
        assert np.array_equal(host(outs["norm"]), host(eager.norm))
        assert np.array_equal(host(mixed["mitigated_values"]), host(eager.mitigated_values))
        assert np.array_equal(host(mixed["mitigated_terms"]), host(eager.mitigated_terms))


def test_combine_against_numpy():
    """mitigated terms and values of ``ops.zne_combine`` on random inputs: a sum of F (or T) products, so within (F + 1) u (or
    (T + 1) u) times the sum of the magnitudes of numpy's own sum; a circuit without terms gives 0.0; more circuits than terms."""
    rng = np.random.default_rng(3)
    f, counts = 4, [3, 0, 5, 1] + [0] * 300
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_terms = int(ptr[-1])
    tv, w, coeff = rng.uniform(-1, 1, size=(f, n_terms)), rng.uniform(-2, 2, size=f), rng.uniform(-1, 1, size=n_terms)
    mv, mt = ops.zne_combine(*(torch.from_numpy(x).to(DEV) for x in (tv, w, ptr, coeff)))
    mv, mt = host(mv), host(mt)
    want_t = w @ tv
    assert (np.abs(mt - want_t) <= (f + 1) * zc.U * (np.abs(w)[:, None] * np.abs(tv)).sum(axis=0)).all()
    for k, cnt in enumerate(counts):
        b, e = int(ptr[k]), int(ptr[k + 1])
        want = float(coeff[b:e] @ mt[b:e])
        assert abs(mv[k] - want) <= (cnt + 1) * zc.U * float(np.abs(coeff[b:e] * mt[b:e]).sum())
        if cnt == 0:
            assert mv[k] == 0.0


# ---- malformed schedules -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["vector", "density"])
def test_malformed_schedules_complete(mode):
    """The contract: indices are clamped, so a schedule that names ops out of range, an empty schedule, entries for a circuit
    without ops and offsets beyond the array all complete without an error and write finite-or-garbage values; an empty schedule
    leaves |0..0>; and a well-formed run beside them keeps its bits."""
    circuits, observables, noise = _mixed(mode)
    circuits, observables = circuits[:5], observables[:5]     # both variants; circuit 1 (vector) / 2 (density) has no ops
    strategy = strategy_of(zc.LOCAL_ALL, (1, 3), 1)
    good = zne.zne_run(circuits, observables, noise, strategy, DEV)
    batch, sch = good.batch, good.schedules
    t = batch.to(DEV)
    n_runs = 10
    lengths = np.diff(sch.sched_ptr)
    sched, ptr = sch.sched.copy(), sch.sched_ptr.copy()
    b0, e0 = int(ptr[0]), int(ptr[1])
    sched[b0:e0:2] = (1 << 20) | 1                 # run 0: far out of range, daggered
    sched[b0 + 1:e0:2] = -5                        # ... and negative
    empty_run = 5 + 3                              # factor 3 of circuit 3: made empty below by equal offsets
    no_ops = 1 if mode == "vector" else 2
    assert batch.op_counts[no_ops] == 0 and lengths[no_ops] == 0
    # rebuild the offsets: run `no_ops` gets 6 entries although its circuit has none, run `empty_run` gets none, the last one runs past n_sched
    new_len = lengths.copy()
    new_len[no_ops] = 6
    new_len[empty_run] = 0
    pieces = []
    for r in range(n_runs):
        piece = sched[int(ptr[r]):int(ptr[r + 1])]
        pieces.append(np.asarray([0, 3, 2, 7, 100, -1], dtype=np.int32) if r == no_ops else piece[:0] if r == empty_run else piece)
    new_sched = np.concatenate(pieces).astype(np.int32)
    new_ptr = np.concatenate([[0], np.cumsum(new_len)]).astype(np.int64)
    new_ptr[-1] += 1000                            # beyond n_sched: clamped
    out = ops.sim_run_folded(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"],
                             torch.from_numpy(new_ptr).to(DEV), torch.from_numpy(new_sched).to(DEV), torch.from_numpy(sch.ids).to(DEV),
                             sch.n_wave, sch.n_wg, 2)
    torch.cuda.synchronize()
    values, tvs, norm = (host(x) for x in out)
    assert values.shape == (2, 5) and tvs.shape[0] == 2
    # the empty schedule left |0..0>: norm 1 exactly, every Z-only term +1, every term with X or Y zero
    c3 = 3
    assert norm[1, c3] == 1.0
    pb, pe = int(batch.term_ptr[c3]), int(batch.term_ptr[c3 + 1])
    for j in range(pb, pe):
        xm = int(batch.terms[j, 0])
        assert tvs[1, j] == (1.0 if xm == 0 else 0.0)
    assert norm[0, no_ops] == 1.0                  # entries for a circuit without ops are skipped
    # the untouched runs keep their bits
    gv, gt, gn = host(good.values), host(good.term_values), host(good.norm)
    for r in range(n_runs - 1):
        f, c = divmod(r, 5)
        if r in (0, no_ops, empty_run):
            continue
        b, e = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
        assert values[f, c] == gv[f, c] and norm[f, c] == gn[f, c] and np.array_equal(tvs[f, b:e], gt[f, b:e]), r
    # out-of-range run numbers are clamped too
    ids = torch.from_numpy(np.asarray([10 ** 6, -3], dtype=np.int32)).to(DEV)
    ops.sim_run_folded(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"],
                       torch.from_numpy(new_ptr).to(DEV), torch.from_numpy(new_sched).to(DEV), ids, 2, 0, 2)
    torch.cuda.synchronize()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_zne_estimator_and_processor_on_the_golden_circuits(lima_backend, g1):
    """The 300 g1 circuits, ``measured_z`` observables (the value is the sum of <Z> over the measured bits), the lima noise model
    without readout, the default strategy (factors (1, 3), two-qubit local folding, a straight line).  ``zne(DeviceEstimator)`` on its
    own and ``learning(zne(DeviceEstimator), ZNEProcessor(...))`` give the same bits (one fused launch each), agree with the oracle
    within the bound on every circuit, and report factors and per-factor values in the metadata.

    Quality: mean |noisy - exact ideal| against mean |mitigated - exact ideal| over the 300 values.  The CPU twin (the numpy oracle
    of zne_cases.py, computed first and again in here: 3 s) gives 0.00146310 and 0.00011583, a ratio of 12.63 -- at least 1.5, so
    the device ratio is asserted to exceed 1; had the twin stayed below 1.5, only the agreement within the bound would be."""
    from blackwater.library.learning.estimator import ZNEProcessor, learning

    noise = sim.NoiseModel.from_backend(lima_backend, readout=False)
    texts = list(g1["qasm"])
    circuits = [Circuit.from_any(t) for t in texts]
    obs = [sim.measured_z(c) for c in circuits]
    strategy = zne.ZNEStrategy()
    cls = zne.zne(sim.DeviceEstimator)
    assert cls.__name__ == "ZNEDeviceEstimator"
    res = cls(noise, DEV, zne_strategy=strategy).run(texts, obs).result()
    inner = cls(noise, DEV)
    wrapped = learning(cls, ZNEProcessor(inner, strategy, lima_backend), skip_transpile=True)(noise, DEV).run(texts, obs).result()
    assert res.values.shape == (300,) and np.array_equal(wrapped.values, res.values)
    assert [m["original_value"] for m in wrapped.metadata] == res.values.tolist()
    ideal = host(sim.expectation_values(texts, obs, None, DEV)[0])
    noisy = host(sim.expectation_values(texts, obs, noise, DEV)[0])
    per_factor = np.asarray([m["zne"]["values"] for m in res.metadata])
    assert np.array_equal(per_factor[:, 0], noisy)                              # factor 1 is the plain noisy run
    assert all(m["zne"]["noise_factors"] == (1.0, 3.0) and m["zne"]["achieved_factors"][0] == 1.0 for m in res.metadata)
    # the CPU twin
    twin_ideal = np.asarray([sc.simulate(c, o.to_list())[0] for c, o in zip(circuits, obs)])
    twin_noisy, twin_mit, worst = np.zeros(300), np.zeros(300), 0.0
    for k, (c, o) in enumerate(zip(circuits, obs)):
        ref = zc.oracle(c, o.to_list(), noise, (1, 3), zc.LOCAL_2Q, 1)
        assert ref["mitigated_value_bound"] < zc.CAP and abs(res.values[k] - ref["mitigated_value"]) <= ref["mitigated_value_bound"], k
        assert np.abs(per_factor[k] - ref["values"]).max() <= ref["value_bounds"].max(), k
        assert res.metadata[k]["zne"]["achieved_factors"] == tuple(ref["achieved"])
        twin_noisy[k], twin_mit[k] = ref["values"][0], ref["mitigated_value"]
        worst = max(worst, abs(res.values[k] - ref["mitigated_value"]))
    err_noisy, err_mit = float(np.abs(noisy - ideal).mean()), float(np.abs(res.values - ideal).mean())
    twin_err_noisy, twin_err_mit = float(np.abs(twin_noisy - twin_ideal).mean()), float(np.abs(twin_mit - twin_ideal).mean())
    print(f"g1, 300 circuits: mean |noisy - ideal| {err_noisy:.8f}, mean |mitigated - ideal| {err_mit:.8f}, ratio {err_noisy / err_mit:.4f}; "
          f"CPU twin {twin_err_noisy:.8f}, {twin_err_mit:.8f}, ratio {twin_err_noisy / twin_err_mit:.4f}; max |device - oracle| {worst:.3e}")
    if twin_err_noisy / twin_err_mit >= 1.5:
        assert err_noisy / err_mit > 1.0
