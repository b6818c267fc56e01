"""Measurement shots on the device (mlqem_sim_run_measured_f64, mlqem_sim_sample_f64, blackwater.sim.sample_expectation_values)
against the oracle of tests/shots_cases.py.

Probabilities are compared within the bound DERIVED in shots_cases.py.  Sampling is compared EXACTLY: the device's own
probabilities, fed through the oracle's CDF rule, Philox and search, must give the device's counts, every entry of every case.  The
estimates are the integer sums divided once (bit for bit); values and variances are within (T + 2) u of their sums.  The seeds are
the ones tests/test_shots_cpu.py cleared against the 5-sigma condition.
"""
import dataclasses

import numpy as np
import pytest
import torch

import shots_cases as shc
import sim_cases as sc
import zne_cases as zc
from blackwater import sim
from blackwater.data.backends import PauliObservable
from blackwater.native import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = sc.U


def host(t):
    return t.cpu().numpy()


_RESULTS = {}


def sampled(name, shots):
    """One sampled call per (batch, shots), kept for the tests that look at different sides of it."""
    if (name, shots) not in _RESULTS:
        circuits, observables, noise, _ = shc.batches()[name]
        _RESULTS[(name, shots)] = sim.sample_expectation_values(circuits, observables, noise, shots=shots, seed=shc.seed_for(shots), device=DEV)
    return _RESULTS[(name, shots)]


BATCHES = ["vector", "density", "readout"]


# ---- 1. probabilities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", BATCHES)
def test_probabilities_against_the_oracle(name):
    res = sampled(name, 10000)
    probs, norm, prob_ptr, group_ptr = host(res.probs), host(res.norm), res.batch.prob_ptr, res.batch.group_ptr
    _, _, _, ids = shc.batches()[name]
    for k, e in enumerate(shc.oracle(name)):
        assert e["prob_bound"] < sc.CAP
        for gl, want in enumerate(e["probs"]):
            b = int(prob_ptr[int(group_ptr[k]) + gl])
            got = probs[b:b + len(want)]
            err, dsum = float(np.abs(got - want).max()), abs(float(got.sum()) - float(norm[k]))
            print(f"{ids[k]} group {gl} ({e['bases'][gl]}): |probs - oracle| {err:.3e} <= {e['prob_bound']:.3e}, |sum - norm| {dsum:.3e}")
            assert err <= e["prob_bound"] and dsum <= e["prob_bound"] and abs(norm[k] - e["norm"]) <= e["prob_bound"]
    # the exact values of the measured launch are the plain launch's within the rotations' cost (the tail returns to the same state)
    circuits, observables, noise, _ = shc.batches()[name]
    plain = host(sim.expectation_values(circuits, observables, noise, DEV)[1])
    bound = max(e["prob_bound"] for e in shc.oracle(name))
    assert np.abs(host(res.exact_term_values) - plain).max() <= 2 * bound


# ---- 2. - 4. exact sampling, estimates, sanity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shots", shc.SHOTS)
@pytest.mark.parametrize("name", BATCHES)
def test_counts_are_the_oracles_from_the_devices_probabilities(name, shots):
    res = sampled(name, shots)
    probs, counts, tv = host(res.probs), host(res.counts), host(res.term_values)
    values, variance = host(res.values), host(res.variance)
    batch = res.batch
    assert counts.dtype == np.int32 and counts.shape == probs.shape == (int(batch.prob_ptr[-1]),)
    for k, e in enumerate(shc.oracle(name)):
        g0, t0, t1 = int(batch.group_ptr[k]), int(batch.term_ptr[k]), int(batch.term_ptr[k + 1])
        dev_probs = [probs[int(batch.prob_ptr[g0 + gl]):int(batch.prob_ptr[g0 + gl + 1])] for gl in range(len(e["probs"]))]
        want_counts, want_est, want_value, want_var = shc.oracle_sample(e, shots, shc.seed_for(shots), k, probs=dev_probs)
        for gl, want in enumerate(want_counts):
            got = counts[int(batch.prob_ptr[g0 + gl]):int(batch.prob_ptr[g0 + gl + 1])]
            assert np.array_equal(got, want), (name, shots, k, gl)                               # no tolerance
            assert got.sum() == shots and (got[dev_probs[gl] <= 0] == 0).all()
        assert np.array_equal(tv[t0:t1], want_est), (name, shots, k)                             # (sum counts * sign) / shots, bit for bit
        coeffs = np.asarray(e["coeffs"])
        tol_v = (len(coeffs) + 2) * U * float(np.abs(coeffs * want_est).sum())
        tol_s = (len(coeffs) + 2) * U * float((coeffs ** 2 * (1 - want_est ** 2)).sum()) + 2 * U * float((coeffs ** 2).sum())
        assert abs(values[k] - want_value) <= tol_v and abs(variance[k] - want_var) <= tol_s, (name, shots, k)
        assert shc.five_sigma_ok(tv[t0:t1], e["exact"], shots).all(), (name, shots, k)          # the seeds the CPU suite cleared


def test_counts_dicts_are_qiskit_shaped():
    res = sampled("vector", 257)
    dicts = sim.counts_dicts(res)
    counts, batch = host(res.counts), res.batch
    assert len(dicts) == len(batch)
    for k, per in enumerate(dicts):
        n = int(batch.circ[k, 0])
        assert len(per) == int(batch.group_ptr[k + 1] - batch.group_ptr[k])
        for gl, d in enumerate(per):
            b = int(batch.prob_ptr[int(batch.group_ptr[k]) + gl])
            assert sum(d.values()) == 257 and all(len(key) == n and counts[b + int(key, 2)] == v and v > 0 for key, v in d.items())


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------------------
def _group_counts(res, k):
    b, e = int(res.batch.prob_ptr[int(res.batch.group_ptr[k])]), int(res.batch.prob_ptr[int(res.batch.group_ptr[k + 1])])
    return host(res.counts)[b:e]


def test_a_circuit_draws_the_same_shots_alone_and_in_the_batch():
    circuits, observables, noise, ids = shc.batches()["vector"]
    whole = sampled("vector", 10000)
    again = sim.sample_expectation_values(circuits, observables, noise, shots=10000, seed=shc.seed_for(10000), device=DEV)
    assert np.array_equal(host(again.counts), host(whole.counts)) and np.array_equal(host(again.values), host(whole.values))
    for k in (ids.index("vector-n5-xyz"), ids.index("vector-n1-z"), ids.index("vector-n9-yi"), ids.index("vector-n11-xyz")):
        alone = sim.sample_expectation_values([circuits[k]], [observables[k]], noise, shots=10000, seed=shc.seed_for(10000),
                                              run_keys=[k], device=DEV)
        assert np.array_equal(host(alone.counts), _group_counts(whole, k)), ids[k]
        assert host(alone.values)[0] == host(whole.values)[k] and host(alone.variance)[0] == host(whole.variance)[k]
    k = ids.index("vector-n5-xyz")
    base = _group_counts(whole, k)
    other_seed = sim.sample_expectation_values([circuits[k]], [observables[k]], noise, shots=10000, seed=shc.seed_for(10000) + 1,
                                               run_keys=[k], device=DEV)
    other_key = sim.sample_expectation_values([circuits[k]], [observables[k]], noise, shots=10000, seed=shc.seed_for(10000),
                                              run_keys=[k + 1], device=DEV)
    assert not np.array_equal(host(other_seed.counts), base) and not np.array_equal(host(other_key.counts), base)
    assert not np.array_equal(host(other_seed.counts), host(other_key.counts))


def test_a_captured_graph_replays_the_same_counts():
    circuits, observables, noise, _ = shc.batches()["vector"]
    eager = sampled("vector", 257)
    batch = eager.batch
    t = batch.to(DEV)
    n_out, b, n_terms = int(batch.prob_ptr[-1]), len(batch), len(batch.coeff)
    units, u_wave, u_wg = batch.sample_units(1)
    units = torch.from_numpy(units).to(DEV)
    keys = torch.from_numpy(sim.default_run_keys(b)).to(DEV)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
    sim_out = {"values": f64(b), "term_values": f64(n_terms), "norm": f64(b), "probs": f64(n_out)}
    smp_out = {"counts": torch.zeros(n_out, dtype=torch.int32, device=DEV), "term_values": f64(n_terms), "values": f64(b), "variance": f64(b)}

    def call():
        ops.sim_run_measured(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"],
                             t["prob_ptr"], n_out, t["ids"], t["n_wave"], t["n_wg"], **sim_out)
        ops.sim_sample(t["circ"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["term_group"], t["prob_ptr"], t["group_circ"],
                       sim_out["probs"], keys, 257, shc.seed_for(257), units, u_wave, u_wg, **smp_out)

    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        call()   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        for o in list(sim_out.values()) + list(smp_out.values()):
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(smp_out["counts"]), host(eager.counts)) and np.array_equal(host(sim_out["probs"]), host(eager.probs))
        assert np.array_equal(host(smp_out["values"]), host(eager.values)) and np.array_equal(host(smp_out["variance"]), host(eager.variance))
        assert np.array_equal(host(smp_out["term_values"]), host(eager.term_values))


# ---- 6. folded runs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, picks", [("density", ("density-n3-xyz", "density-n5-yi", "density-n1-z")),
                                         ("vector", ("vector-n5-xyz", "vector-n9-z4", "vector-n2-yi"))])
def test_folded_runs_are_sampled_per_factor(name, picks):
    circuits, observables, noise, ids = shc.batches()[name]
    idx = [ids.index(p) for p in picks]
    circuits, observables = [circuits[i] for i in idx], [observables[i] for i in idx]
    factors, shots, seed = (1, 3, 5), 257, 77
    strategy = sim.ZNEStrategy(noise_factors=factors, noise_amplifier=zc.make_amplifier(zc.LOCAL_2Q), extrapolator=sim.LinearExtrapolator())
    run = sim.zne_run(circuits, observables, noise, strategy, DEV, shots=shots, seed=seed)
    batch, n_circ = run.batch, len(circuits)
    probs, counts, tv = host(run.probs), host(run.counts), host(run.term_values)
    values, variance, w = host(run.values), host(run.variance), run.weights
    assert probs.shape == counts.shape == (3, int(batch.prob_ptr[-1])) and values.shape == variance.shape == (3, n_circ)
    for f in range(3):
        for k, i in enumerate(idx):
            e = shc.oracle(name)[i]
            g0, t0, t1 = int(batch.group_ptr[k]), int(batch.term_ptr[k]), int(batch.term_ptr[k + 1])
            dev_probs = [probs[f, int(batch.prob_ptr[g0 + gl]):int(batch.prob_ptr[g0 + gl + 1])] for gl in range(len(e["probs"]))]
            if f == 0:   # factor 1 is the circuit itself: the oracle's probabilities, within the bound
                assert all(np.abs(p - q).max() <= e["prob_bound"] for p, q in zip(dev_probs, e["probs"]))
            want_counts, want_est, _, _ = shc.oracle_sample(e, shots, seed, f * n_circ + k, probs=dev_probs)
            for gl, want in enumerate(want_counts):
                assert np.array_equal(counts[f, int(batch.prob_ptr[g0 + gl]):int(batch.prob_ptr[g0 + gl + 1])], want), (f, k, gl)
            assert np.array_equal(tv[f, t0:t1], want_est)
    # mitigated value = sum_f w_f value_f; both sides form F * T rounded products and additions: (F + 1) + (T + 2) units on each side
    for k in range(n_circ):
        t0, t1 = int(batch.term_ptr[k]), int(batch.term_ptr[k + 1])
        mags = float(np.abs(w[:, None] * batch.coeff[None, t0:t1] * tv[:, t0:t1]).sum())
        tol = 2 * (3 + 1 + (t1 - t0) + 2) * U * mags
        assert abs(host(run.mitigated_values)[k] - float((w * values[:, k]).sum())) <= tol, k
        want_var = float((w * w * variance[:, k]).sum())
        assert abs(host(run.mitigated_variance)[k] - want_var) <= (3 + 2) * U * float(np.abs(w * w * variance[:, k]).sum()), k
    if name == "density":   # noise grows with the factor, so the distributions differ
        assert not np.array_equal(probs[0], probs[2])


# ---- 7. surface --------------------------------------------------------------------------------------------------------------------------
def test_device_estimator_with_and_without_shots(lima_backend, g1):
    from blackwater.library.learning.estimator import EmptyProcessor, learning
    from blackwater.library.ngem.estimator import ngem

    noise = sim.NoiseModel.from_backend(lima_backend)
    circuits = list(g1["qasm"][:6])
    obs = [PauliObservable("IIIIZ") if k % 2 else PauliObservable([("IIIZI", 0.5), ("IIZII", -2.0)]) for k in range(6)]
    exact = sim.DeviceEstimator(noise, DEV).run(circuits, obs).result()
    today = host(sim.expectation_values(circuits, obs, noise, DEV)[0])
    assert exact.metadata == [{}] * 6 and np.array_equal(exact.values, today)          # no shots: the exact path, bit for bit

    est = sim.DeviceEstimator(noise, DEV, shots=1000, seed=3)
    first, second = est.run(circuits, obs).result(), est.run(circuits, obs).result()
    assert all(set(m) == {"variance", "shots"} and m["shots"] == 1000 and m["variance"] >= 0 for m in first.metadata)
    assert not np.array_equal(first.values, second.values)                              # successive runs do not repeat their draws
    twin = sim.DeviceEstimator(noise, DEV, shots=1000, seed=3)
    assert np.array_equal(twin.run(circuits, obs).result().values, first.values)        # the same seed, the same job number
    assert np.array_equal(twin.run(circuits, obs).result().values, second.values)
    sigma = np.sqrt(np.asarray([m["variance"] for m in first.metadata]) / 1000)
    assert (np.abs(first.values - today) <= 6 * sigma + 6 / 1000).all()
    over = sim.DeviceEstimator(noise, DEV).run(circuits, obs, shots=64, seed=9).result()   # run options override the constructor
    assert all(m["shots"] == 64 for m in over.metadata) and np.array_equal(over.values * 128, np.round(over.values * 128))   # coefficients 1, 0.5, -2

    wrapped = learning(sim.DeviceEstimator, EmptyProcessor(), skip_transpile=True)(noise, DEV, shots=1000, seed=3)
    out = wrapped.run(circuits, obs).result()
    assert np.array_equal(np.asarray(out.values), first.values)

    class Doubling(torch.nn.Module):
        def forward(self, exp_value, observable, circuit_depth, nodes, edge_index, batch):
            return exp_value * 2

    got = ngem(sim.DeviceEstimator, Doubling(), lima_backend)(noise, DEV, shots=1000, seed=3).run(circuits[:3], obs[:3]).result().values
    assert np.isfinite(got).all() and got.shape == (3,)


def test_zne_estimator_fills_the_error_bar(lima_backend, g1):
    from blackwater.zne import zne

    noise = sim.NoiseModel.from_backend(lima_backend)
    circuits, obs = list(g1["qasm"][:4]), [PauliObservable("IIIIZ")] * 4
    strategy = sim.ZNEStrategy(noise_factors=(1, 3, 5))
    est = zne(sim.DeviceEstimator)(noise, DEV, zne_strategy=strategy)
    exact = est.run(circuits, obs).result()
    assert all(set(m) == {"zne"} for m in exact.metadata)                               # no shots: as before
    res = est.run(circuits, obs, shots=4096, seed=5).result()
    w = strategy.weights()
    for k, m in enumerate(res.metadata):
        var = m["zne"]["variances"]
        assert m["shots"] == 4096 and len(var) == 3 and m["std_error"] == np.sqrt(m["variance"] / 4096) and m["std_error"] > 0
        assert abs(m["variance"] - float((w * w * np.asarray(var)).sum())) <= 5 * U * float((w * w * np.asarray(var)).sum())
        assert abs(res.values[k] - float((w * np.asarray(m["zne"]["values"])).sum())) <= 8 * U * float(np.abs(w * np.asarray(m["zne"]["values"])).sum())
        assert abs(res.values[k] - exact.values[k]) <= 6 * m["std_error"] + 6 / 4096
    mv, _, _, per = sim.zne_expectation_values(circuits, obs, noise, strategy, DEV, shots=4096, seed=5)   # the same four tensors
    run = sim.zne_run(circuits, obs, noise, strategy, DEV, shots=4096, seed=5)
    assert mv.shape == (4,) and per.shape == (3, 4) and np.array_equal(host(mv), host(run.mitigated_values))
    assert run.mitigated_variance.shape == (4,) and run.variance.shape == (3, 4) and np.array_equal(host(per), host(run.values))


def test_exp_value_generator_with_shots():
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import synthetic_backend

    backend = synthetic_backend(3, "cx")
    kw = dict(max_entries=12, batch=8, seed=4, device=DEV)
    exact = list(exp_value_generator(backend, 3, 5, 1, **kw))
    noisy = list(exp_value_generator(backend, 3, 5, 1, shots=128, **kw))
    both = list(exp_value_generator(backend, 3, 5, 1, shots=128, sample_ideal=True, **kw))
    rebatched = list(exp_value_generator(backend, 3, 5, 1, shots=128, **dict(kw, batch=5)))
    for e, s, b, r in zip(exact, noisy, both, rebatched):
        coeff = e.observable[0][0]   # one term: value = coeff * estimate, the estimate a multiple of 1 / shots
        for v in (s.noisy_exp_values[0], b.noisy_exp_values[0], b.ideal_exp_value):
            m = v / coeff * 128
            assert abs(m - round(m)) <= 1e-9 and abs(m) <= 128 + 1e-9
        assert s.ideal_exp_value == e.ideal_exp_value and s.noisy_exp_values == r.noisy_exp_values == b.noisy_exp_values
    assert any(s.noisy_exp_values != e.noisy_exp_values for s, e in zip(noisy, exact))


def test_encode_corpus_with_shots():
    """Noisy labels (and with ``sample_ideal`` the ideal ones) are multiples of 1 / shots, and a circuit's draws are keyed by its
    position in the corpus: the same at that position in a longer corpus."""
    from blackwater.data.synthetic import encode_corpus, random_circuit, synthetic_backend

    circuits = [random_circuit(4, 2 + k, k) for k in range(6)]
    noise = sim.NoiseModel.from_backend(synthetic_backend(4, "cx"))
    kw = dict(seed=7, simulate=noise, device=DEV)
    exact = encode_corpus(circuits, 4, **kw)
    got = encode_corpus(circuits, 4, shots=256, **kw)
    both = encode_corpus(circuits, 4, shots=256, sample_ideal=True, **kw)
    for arr in (got["noisy"], both["noisy"], both["y"]):      # one Z term of coefficient 1: an estimate k / 256, exact in float32
        assert np.array_equal(arr * 256, np.round(arr * 256)) and np.abs(arr).max() <= 1
    assert np.array_equal(got["y"], exact["y"]) and np.array_equal(got["noisy"], both["noisy"])
    assert not np.array_equal(got["noisy"], exact["noisy"]) and not np.array_equal(both["y"], both["noisy"])
    shorter = encode_corpus(circuits[:4], 4, shots=256, **kw)   # the observable qubits are drawn in order, so a prefix keeps them
    assert np.array_equal(shorter["observable"], got["observable"][:4]) and np.array_equal(shorter["noisy"], got["noisy"][:4])


# ---- 8. robustness -------------------------------------------------------------------------------------------------------------------------
def test_malformed_measure_records_touch_nothing_else():
    """An out-of-range slot in a MEASURE record and a prob_ptr past the pool: garbage for that circuit, MLQEM_OK (or a BAD_ARG from the
    host-side check), and the other circuits' outputs as they were.  Nothing here is meant to fault: every index is clamped or its
    store predicated."""
    circuits, observables, noise, ids = shc.batches()["vector"]
    good = sampled("vector", 65)
    batch = good.batch
    n_groups, n_out = len(batch.group_circ), int(batch.prob_ptr[-1])
    victim = ids.index("vector-n5-z")
    g = int(batch.group_ptr[victim])
    for what in ("slot", "prob_ptr"):
        bad_ops, bad_ptr = batch.ops.copy(), batch.prob_ptr.copy()
        if what == "slot":
            rec = int(batch.op_ptr[victim + 1]) - 1          # a single-Z observable: the tail is its one MEASURE record
            assert bad_ops[rec, 0] == 9
            bad_ops[rec, 3] = n_groups + 1000
        else:
            bad_ptr[g] = n_out + 12345
        bad = dataclasses.replace(batch, ops=bad_ops, prob_ptr=bad_ptr)
        t = bad.to(DEV)
        units, u_wave, u_wg = batch.sample_units(1)
        try:
            values, term_values, norm, probs = ops.sim_run_measured(
                t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["prob_ptr"], n_out,
                t["ids"], t["n_wave"], t["n_wg"])
            s_values, s_var, s_terms, counts = ops.sim_sample(
                t["circ"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["term_group"], t["prob_ptr"], t["group_circ"], probs,
                torch.from_numpy(sim.default_run_keys(len(batch))).to(DEV), 65, shc.seed_for(65), torch.from_numpy(units).to(DEV), u_wave, u_wg)
        except _lib.NativeLibraryError as err:               # a refusal by the host-side check is as good
            assert "code -1" in str(err), err                # MLQEM_ERR_BAD_ARG
            continue
        torch.cuda.synchronize()
        b, e = int(batch.prob_ptr[g]), int(batch.prob_ptr[g + 1])
        keep = np.ones(n_out, dtype=bool)
        keep[b:e] = False
        assert np.array_equal(host(probs)[keep], host(good.probs)[keep]) and np.array_equal(host(counts)[keep], host(good.counts)[keep])
        others = np.arange(len(batch)) != victim
        assert np.array_equal(host(s_values)[others], host(good.values)[others]) and np.array_equal(host(values)[others], host(good.exact_values)[others])
        assert (host(probs)[b:e] == 0).all()                                   # the malformed record stored nothing
        if what == "prob_ptr":
            assert (host(counts)[b:e] == 0).all()                              # nor did the sampler, whose range left the pool too
        else:
            assert host(counts)[b] == 65 and host(counts)[b:e].sum() == 65     # all-zero probabilities: every shot on outcome 0
