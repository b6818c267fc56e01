"""Shots from matrix-product states (mlqem_mps_sample_f64, mlqem_mps_sample_finish_f64) against the host interpreter of the draw
contract, bit for bit, and their bits under batching, splitting and graph replay.  tests/mps_shots_cases.py has the grid, the
oracles and the measured margins; tests/test_mps_shots_cpu.py asserts the conditions under which the device's bits must equal the
interpreter's, so that no case, circuit or shot is excluded here."""
import numpy as np
import pytest
import torch

import mps_cases as mc
import mps_shots_cases as ms
from blackwater import sim
from blackwater.data.synthetic import encode_corpus, tfim_circuit
from blackwater.native import ops
from blackwater.sim import compile_mps_shots, mps_counts, run_mps, run_mps_shots

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _host(t):
    return t.cpu().numpy()


def _words(res, batch, g):
    w = int(batch.ref_ptr[g + 1] - batch.ref_ptr[g])
    b = int(batch.ref_ptr[g]) * res.shots
    return _host(res.bits[b:b + res.shots * w]).view(np.uint32).reshape(res.shots, w)


def _run(case_id, **kw):
    c = ms.case(case_id)
    return run_mps_shots(ms.lower(case_id), c["shots"], seed=c["seed"], device=DEV, **kw)


@pytest.mark.parametrize("case_id", ms.IDS)
def test_device_against_the_interpreter(case_id):
    """Bits, sums, estimates, values and variances equal the interpreter's exactly; the counts are those of its bits; the run's
    statistics are ``run_mps``'s on the same batch."""
    c, batch = ms.case(case_id), ms.lower(case_id)
    res = _run(case_id, return_bits=True)
    ref = ms.reference(case_id)
    sums, terms, values, variance = _host(res.term_sums), _host(res.term_values), _host(res.values), _host(res.variance)
    mps = batch.mps
    for k, r in enumerate(ref):
        g0 = int(batch.group_ptr[k])
        for j, want in enumerate(r["bits"]):
            got = _words(res, batch, g0 + j)
            assert np.array_equal(got, want), (case_id, k, j, int((got != want).any(axis=1).sum()), "shots differ")
        tb, te = int(mps.term_ptr[k]), int(mps.term_ptr[k + 1])
        assert np.array_equal(sums[tb:te], r["term_sums"])
        assert np.array_equal(terms[tb:te], r["term_values"])
        assert values[k] == r["value"] and variance[k] == r["variance"]
        assert mps_counts(res, k) == [ms.counts_of(w, int(mps.n_qubits[k])) for w in r["bits"]]
    plain = run_mps(mps, seed=c["seed"], device=DEV)
    for name in ("discarded", "error_bound", "bond"):
        assert np.array_equal(_host(getattr(res, name)), _host(getattr(plain, name))), name
    assert res.trajectories == c["trajectories"] and res.shots == c["shots"]


@pytest.mark.parametrize("case_id", [i for i in ms.IDS if ms.case(i)["dense"]])
def test_estimates_lie_within_five_sigma_of_the_exact_values(case_id):
    res = _run(case_id)
    terms, ptr = _host(res.term_values), ms.lower(case_id).mps.term_ptr
    for k, exact in enumerate(ms.exact_terms(case_id)):
        assert ms.five_sigma(terms[int(ptr[k]):int(ptr[k + 1])], exact, res.shots).all()


def test_width_estimates_lie_within_five_sigma_of_the_clifford_path():
    case_id = "width-clifford-n100-s3-b8"
    c = ms.case(case_id)
    res = _run(case_id)
    exact = _host(sim.clifford_expectation_values(c["circuits"], c["observables"], None, DEV)[1])
    assert ms.five_sigma(_host(res.term_values), exact, res.shots).all()


def test_reported_z_of_a_product_state_under_readout_noise():
    """Readout noise alone on a product state: the mean reported Z is a <Z> + b of the readout table."""
    from blackwater.data.circuit import Circuit, CircuitOp

    n, shots = 4, 1000
    angles = (0.3, 1.1, 2.0, 2.8)
    circ = Circuit(n, n, [CircuitOp("ry", (q,), (), (angles[q],)) for q in range(n)] + [CircuitOp("measure", (q,), (q,)) for q in range(n)])
    noise = sim.NoiseModel(readout={q: (0.02 + 0.01 * q, 0.07 - 0.01 * q) for q in range(n)})
    batch = compile_mps_shots([circ], [mc.single_z(n)], noise, 1, 4)
    res = run_mps_shots(batch, shots, seed=21, device=DEV)
    a, b = batch.mps.readout[:n, 0], batch.mps.readout[:n, 1]
    exact = a * np.cos(np.asarray(angles)) + b
    assert ms.five_sigma(_host(res.term_values), exact, shots).all()
    assert np.abs(b).min() > 0.0, "an asymmetric table: a and b both matter"


def _sampled(res):
    return [_host(res.term_sums), _host(res.term_values), _host(res.values), _host(res.variance)]


def test_same_bits_alone_in_a_batch_and_in_any_split():
    case_id = "noisy-depol-T64"
    c, batch = ms.case(case_id), ms.lower(case_id)
    noise = ms.noise_of(c)
    whole = run_mps_shots(batch, c["shots"], seed=11, device=DEV, return_bits=True)
    full, ptr = _sampled(whole), batch.mps.term_ptr
    for j in (0, 2):   # alone, with its batch key
        one = compile_mps_shots([c["circuits"][j]], [c["observables"][j]], noise, 64, c["max_bond"])
        alone = run_mps_shots(one, c["shots"], seed=11, run_keys=[j], device=DEV, return_bits=True)
        assert np.array_equal(_host(alone.term_sums), full[0][int(ptr[j]):int(ptr[j + 1])])
        for g in range(len(one.group_circ)):
            assert np.array_equal(_words(alone, one, g), _words(whole, batch, int(batch.group_ptr[j]) + g))
    # three splits: one circuit's trajectories per launch, a few units per launch (a circuit's trajectories split), one unit each
    per_unit = ops.mps_workspace_bytes(5, c["max_bond"], 1) + ops.mps_sample_workspace_bytes(5, c["max_bond"], 1)
    for budget in (per_unit * 64, per_unit * 7, 1):
        split = run_mps_shots(batch, c["shots"], seed=11, device=DEV, return_bits=True, buffer_bytes=budget)
        assert all(np.array_equal(x, y) for x, y in zip(_sampled(split), full)), budget
        assert np.array_equal(_host(split.bits), _host(whole.bits)), budget
    without = run_mps_shots(batch, c["shots"], seed=11, device=DEV)
    assert without.bits is None and all(np.array_equal(x, y) for x, y in zip(_sampled(without), full))
    assert not np.array_equal(_host(run_mps_shots(batch, c["shots"], seed=12, device=DEV).term_sums), full[0])


def test_a_replayed_graph_gives_the_same_bits():
    case_id = "noisy-overrot-T64"
    c, batch = ms.case(case_id), ms.lower(case_id)
    mps, shots = batch.mps, c["shots"]
    eager = run_mps_shots(batch, shots, seed=3, device=DEV, return_bits=True)
    t = batch.to(DEV)
    b, n_terms, count, n_groups = len(batch), len(mps.term_circ), mps.trajectories, len(batch.group_circ)
    keys = torch.arange(b, dtype=torch.int64, device=DEV)
    widest = int(mps.n_qubits.max())
    workspace = torch.empty(ops.mps_workspace_bytes(widest, mps.max_bond, b * count), dtype=torch.uint8, device=DEV)
    env = torch.empty(ops.mps_sample_workspace_bytes(widest, mps.max_bond, b * count), dtype=torch.uint8, device=DEV)
    traj_stats = torch.zeros((count, b, ops.MPS_STATS), dtype=torch.float64, device=DEV)
    term_sums = torch.zeros(n_terms, dtype=torch.int32, device=DEV)
    bits = torch.zeros(int(batch.ref_ptr[-1]) * shots, dtype=torch.int32, device=DEV)
    outs = [torch.zeros(n, dtype=torch.float64, device=DEV) for n in (b, b, n_terms)]

    def launch():   # one stream, no parallel branches
        ops.mps_run(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], keys, (0, b), (0, count), count, 3, mps.max_bond, mps.cutoff, widest,
                    workspace, traj_stats)
        ops.mps_sample(t["n_qubits"], (0, b), (0, count), count, mps.max_bond, widest, workspace, env, (0, n_groups), batch.max_groups,
                       t["group_ptr"], t["group_circ"], t["group_off"], t["basis"], t["site_ptr"], t["flip"], t["ref_ptr"], t["gterm_ptr"],
                       t["gterm"], (0, n_terms), t["term_mask"], t["masks"], keys, shots, 3, term_sums, bits)
        ops.mps_sample_finish(t["term_ptr"], t["coeff"], term_sums, shots, values=outs[0], variance=outs[1], term_values=outs[2])

    launch()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for _ in range(2):
        for buf in (term_sums, bits, traj_stats, *outs):
            buf.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_host(bits), _host(eager.bits)) and np.array_equal(_host(term_sums), _host(eager.term_sums))
        for got, name in zip(outs, ("values", "variance", "term_values")):
            assert np.array_equal(_host(got), _host(getattr(eager, name))), name


def test_estimator_draws_and_metadata():
    c = ms.case("tfim-n10-s6-b16")
    make = lambda: sim.DeviceEstimator(device=DEV, method="mps_shots", shots=300, seed=5, max_bond=16)   # noqa: E731
    est, twin = make(), make()
    first, second = est.run(c["circuits"], c["observables"]).result(), est.run(c["circuits"], c["observables"]).result()
    assert not np.array_equal(first.values, second.values), "successive jobs do not repeat their draws"
    again = [twin.run(c["circuits"], c["observables"]).result() for _ in range(2)]
    assert np.array_equal(first.values, again[0].values) and np.array_equal(second.values, again[1].values)
    assert set(first.metadata[0]) == {"variance", "shots", "truncation_error_bound", "max_bond"}
    assert first.metadata[0]["shots"] == 300 and first.metadata[0]["max_bond"] == 16
    direct = sim.sample_mps_expectation_values(c["circuits"], c["observables"], shots=300, max_bond=16, seed=5,
                                               run_keys=sim.default_run_keys(1, 1 << 32), device=DEV)
    assert np.array_equal(first.values, _host(direct.values)) and first.metadata[0]["variance"] == float(_host(direct.variance)[0])
    noisy = ms.case("noisy-readout-T64")
    est = sim.DeviceEstimator(ms.noise_of(noisy), DEV, method="mps_shots", shots=500, trajectories=64, seed=5)
    got = est.run(noisy["circuits"], noisy["observables"]).result()
    assert all(set(m) == {"variance", "shots", "truncation_error_bound", "max_bond", "trajectories"} and m["trajectories"] == 64
               for m in got.metadata)
    assert not np.array_equal(got.values, est.run(noisy["circuits"], noisy["observables"]).result().values)


def test_data_generation_fills_labels_from_the_sampler():
    nq = 24
    circuits = [tfim_circuit(nq, s, j, two_q="cx") for s, j in ((1, 0.4), (2, 1.0), (3, 1.7))]
    noise = sim.NoiseModel.from_backend(mc.tc.table(nq))
    got = encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=noise, device=DEV, trajectories=8, mps_bond=8, mps_shots=200)
    means = encode_corpus(circuits, nq, two_q="cx", seed=7, simulate=noise, device=DEV, trajectories=8, mps_bond=8)
    assert np.array_equal(got["y"], means["y"]), "the ideal value stays the exact MPS value"
    z_qubits = [int(np.flatnonzero(o[0, 2::4])[0]) for o in got["observable"]]
    labels = ["".join("Z" if q == z else "I" for q in reversed(range(nq))) for z in z_qubits]
    under = sim.sample_mps_expectation_values(circuits, labels, noise, shots=200, max_bond=8, trajectories=8, seed=7, run_keys=np.arange(3),
                                              device=DEV)
    assert np.array_equal(got["noisy"][:, 0], _host(under.values).astype(np.float32))
    assert not np.array_equal(got["noisy"], means["noisy"])

    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import random_circuit, synthetic_backend
    from blackwater.data.utils import generate_random_pauli_sum_op

    backend = synthetic_backend(6, "cx")
    kw = dict(max_entries=4, device=DEV, seed=3, trajectories=4, mps_bond=8)
    plain = list(exp_value_generator(backend, 6, 3, 2, **kw))
    shot = list(exp_value_generator(backend, 6, 3, 2, mps_shots=100, **kw))
    assert [e.ideal_exp_value for e in shot] == [e.ideal_exp_value for e in plain]
    rng = np.random.default_rng(3)   # the generator's own draws of its circuits and observables
    circuits, observables = [], []
    for _ in range(4):
        depth, circuit_seed = int(rng.integers(1, 4)), int(rng.integers(0, 2 ** 31 - 1))
        circuits.append(random_circuit(6, depth, circuit_seed, two_q="cx"))
        observables.append(generate_random_pauli_sum_op(6, 2, 1.0, rng=rng))
    direct = sim.sample_mps_expectation_values(circuits, observables, sim.NoiseModel.from_backend(backend, readout=False), shots=100,
                                               max_bond=8, trajectories=4, seed=3, run_keys=np.arange(4), device=DEV)
    assert [e.noisy_exp_values[0] for e in shot] == _host(direct.values).tolist()
    assert [e.noisy_exp_values for e in shot] != [e.noisy_exp_values for e in plain]
