"""The batched simulator on the device (mlqem_sim_run_f64, blackwater.sim) against the numpy oracle of tests/sim_cases.py.

Every comparison uses the bound DERIVED in sim_cases.py (per-op rounding costs times the ops of the circuit at hand, plus the
reduction's term), and every case asserts that its bound stays below 1e-11.  Bit-equality is asserted where the contract promises
it: a circuit alone against the same circuit in a batch, two runs, a captured graph against eager.
"""
import numpy as np
import pytest
import torch

import sim_cases as sc
from blackwater import sim
from blackwater.data.backends import PauliObservable
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.native import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.cpu().numpy()


def run(circuits, observables, noise=None):
    """(values, term_values, norm, batch) of one call."""
    batch = sim.compile_programs(circuits, observables, noise)
    values, term_values, norm = sim.run_batch(batch, DEV)
    return host(values), host(term_values), host(norm), batch


def check_against_oracle(circuits, observables, noise, what):
    values, term_values, norm, batch = run(circuits, observables, noise)
    worst = 0.0
    for k, (c, terms) in enumerate(zip(circuits, observables)):
        ov, otv, onorm = sc.simulate(c, terms, noise)
        tb, vb = sc.term_bound(c, noise), sc.value_bound(c, terms, noise)
        assert tb < sc.CAP and vb < sc.CAP, (what, k, tb, vb)
        b, e = int(batch.term_ptr[k]), int(batch.term_ptr[k + 1])
        dv = abs(values[k] - ov)
        dt = float(np.abs(term_values[b:e] - otv).max()) if e > b else 0.0
        dn = abs(norm[k] - 1.0)
        print(f"{what} circuit {k} ({batch.variant[k]}, {int(batch.op_counts[k])} records, {e - b} terms): |value| {dv:.3e} <= {vb:.3e}, "
              f"|terms| {dt:.3e} <= {tb:.3e}, |norm - 1| {dn:.3e}, oracle |norm - 1| {abs(onorm - 1.0):.3e}")
        assert dv <= vb and dt <= tb and dn <= tb, (what, k)
        worst = max(worst, dt)
    return values, term_values, norm, batch


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 11])
def test_state_vector_grid(n):
    """40 random ops over the full gate list (forced pairs included), a 12-term and a 40-term observable.  Bounds at n = 11:
    term 2^-53 (4 sum cost + 2048 + 32 + 16) < 5e-13, value sum|coeff| (<= 3) times that: all below 1e-11 (asserted)."""
    c = sc.random_program(n, 40, seed=0)
    _, _, _, batch = check_against_oracle([c, c], [sc.term_set(n), sc.long_observable(n)], None, f"vector n={n}")
    assert batch.variant == ["wave" if n <= 8 else "workgroup"] * 2


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_density_grid_without_noise_equals_the_state_vector(n):
    c = sc.random_program(n, 40, seed=1)
    obs = [sc.term_set(n), sc.long_observable(n)]
    dv, dt, _, batch = check_against_oracle([c, c], obs, sc.NoNoise(), f"density n={n}")
    assert batch.variant == ["wave" if n <= 4 else "workgroup"] * 2
    vv, vt, _, _ = run([c, c], obs, None)
    tb = sc.term_bound(c) + sc.term_bound(c, sc.NoNoise())
    vb = max(sc.value_bound(c, o) + sc.value_bound(c, o, sc.NoNoise()) for o in obs)
    print(f"density vs vector n={n}: |terms| {np.abs(dt - vt).max():.3e} <= {tb:.3e}, |values| {np.abs(dv - vv).max():.3e} <= {vb:.3e}")
    assert np.abs(dt - vt).max() <= tb and np.abs(dv - vv).max() <= vb


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_density_grid_with_depolarising_noise(n):
    """A depolarising op after every gate, lambda in [0, 0.2] plus lambda = 0 and lambda = 1 once each, closed form (kernel) against
    the Kraus sum (oracle); Tr rho = 1 within the bound."""
    c = sc.random_program(n, 40, seed=2)
    noise = sc.StepNoise(11)
    _, _, _, batch = check_against_oracle([c, c], [sc.term_set(n), sc.long_observable(n)], noise, f"depolarising n={n}")
    lam = [batch.params[p] for kind, _, _, p in batch.ops.tolist() if kind in (sim.program.OP_DEPOL1, sim.program.OP_DEPOL2)]
    assert 0.0 in lam and 1.0 in lam and len(lam) == 2 * 40


@pytest.mark.parametrize("n", [1, 2, 4, 5])
def test_readout_ops_on_z_observables(n):
    c = sc.random_program(n, 40, seed=3, measure=True)
    noise = sc.StepNoise(12, readout={q: (0.01 + 0.02 * q, 0.06 - 0.01 * q) for q in range(n)})
    obs = [sc.term_set(n, alphabet="IZ"), sc.long_observable(n, alphabet="IZ")]
    _, _, _, batch = check_against_oracle([c, c], obs, noise, f"readout n={n}")
    assert batch.circ[:, 2].tolist() == [n, n]


# ---- batching ----------------------------------------------------------------------------------------------------------------------------
def _mixed_vector_batch():
    empty = Circuit(1, 0, [])
    one = Circuit(3, 0, [CircuitOp("h", (2,))])
    circuits = [sc.random_program(5, 101, seed=4, with_id=False), empty, sc.random_program(9, 40, seed=5), one, sc.random_program(8, 40, seed=6),
                sc.random_program(11, 17, seed=7), sc.random_program(2, 40, seed=8)]
    observables = [sc.term_set(5), [("Z", 1.0)], sc.term_set(9), [], sc.long_observable(8), sc.term_set(11), [("XY", 0.5)]]
    return circuits, observables


def _mixed_density_batch():
    circuits = [sc.random_program(4, 101, seed=9, with_id=False), sc.random_program(5, 40, seed=10), Circuit(2, 0, []),
                sc.random_program(1, 1, seed=11, with_id=False), sc.random_program(5, 1, seed=12, with_id=False), sc.random_program(3, 40, seed=13),
                sc.random_program(2, 40, seed=14)]
    observables = [sc.term_set(4), sc.term_set(5), [], [("Y", 1.0)], sc.long_observable(5), sc.term_set(3), [("ZZ", -1.0)]]
    return circuits, observables


@pytest.mark.parametrize("mode", ["vector", "density"])
def test_a_circuit_is_bit_equal_alone_and_in_any_batch(mode):
    """One launch with circuits of different n, op counts (0, 1, 101) and term counts (0 terms: value 0.0) and both variants; batch
    sizes 1, 3, 5 and 7 leave a workgroup of the wave variant partly empty."""
    circuits, observables = _mixed_vector_batch() if mode == "vector" else _mixed_density_batch()
    noise = None if mode == "vector" else sc.StepNoise(21)
    alone = [run([c], [o], noise) for c, o in zip(circuits, observables)]
    for size in (1, 3, 5, 7):
        values, term_values, norm, batch = check_against_oracle(circuits[:size], observables[:size], noise, f"{mode} batch of {size}")
        again = run(circuits[:size], observables[:size], noise)
        assert np.array_equal(values, again[0]) and np.array_equal(term_values, again[1]) and np.array_equal(norm, again[2])
        for k in range(size):
            b, e = int(batch.term_ptr[k]), int(batch.term_ptr[k + 1])
            assert values[k] == alone[k][0][0] and norm[k] == alone[k][2][0] and np.array_equal(term_values[b:e], alone[k][1])
            if e == b:
                assert values[k] == 0.0
        if size == 7:
            assert set(batch.variant) == {"wave", "workgroup"}
            counts = batch.op_counts.tolist()
            assert 0 in counts and min(c for c in counts if c) <= 2 and max(counts) >= 101


# ---- the golden circuits ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    texts, ideal, split = sc.golden_circuits()
    circuits = [Circuit.from_any(t) for t in texts]
    observables = [sim.measured_z(c).to_list() for c in circuits]
    oracle = np.asarray([sc.simulate(c, o)[1] for c, o in zip(circuits, observables)])
    return {"texts": texts, "circuits": circuits, "observables": observables, "oracle": oracle, "ideal": ideal, "split": split}


def test_golden_circuits_in_one_call(golden):
    """All 900 reference circuits (QASM text in) in one call: the oracle within the bound, and the reference's stored 10 000-shot
    labels within 4 sigma of -<Z> of classical bit 3 - k, all 3 600 of them."""
    values, term_values, norm, batch = run(golden["texts"], golden["observables"])
    got = term_values.reshape(900, 4)
    bounds = np.asarray([sc.term_bound(c) for c in golden["circuits"]])
    err = np.abs(got - golden["oracle"]).max(axis=1)
    print(f"900 golden circuits: max |device - oracle| {err.max():.3e}, largest bound {bounds.max():.3e}, max |norm - 1| {np.abs(norm - 1).max():.3e}")
    assert bounds.max() < sc.CAP and (err <= bounds).all() and (np.abs(norm - 1.0) <= bounds).all()
    sig = sc.anchor_sigmas(got, golden["ideal"])
    print(f"reference anchor: max {sig.max():.3f} sigma over {sig.size} stored values")
    assert sig.shape == (900, 4) and sig.max() <= 4.0
    assert set(batch.variant) == {"wave"}


def test_golden_circuits_in_a_captured_graph(golden):
    batch = sim.compile_programs(golden["texts"], golden["observables"])
    t = batch.to(DEV)
    args = (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"], t["n_wave"], t["n_wg"])
    eager = [host(x) for x in ops.sim_run(*args)]
    outs = {"values": torch.zeros(900, dtype=torch.float64, device=DEV), "term_values": torch.zeros(3600, dtype=torch.float64, device=DEV),
            "norm": torch.zeros(900, dtype=torch.float64, device=DEV)}
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.sim_run(*args, **outs)   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sim_run(*args, **outs)
    for _ in range(2):
        for o in outs.values():
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(outs["values"]), eager[0]) and np.array_equal(host(outs["term_values"]), eager[1])
        assert np.array_equal(host(outs["norm"]), eager[2])


# ---- the estimator -----------------------------------------------------------------------------------------------------------------------
def test_device_estimator_and_the_learning_decorator(lima_backend, g1):
    from blackwater.library.learning.estimator import LinearLearningModelProcessor, learning
    from blackwater.library.learning.features import encode_data
    from blackwater.data.utils import encode_pauli_sum_op, get_backend_properties_v1
    from blackwater.nn import LinearRegressor

    noise = sim.NoiseModel.from_backend(lima_backend)
    circuits = list(g1["qasm"][:40])
    obs = [PauliObservable("IIIIZ") if k % 2 else PauliObservable([("IIIZI", 0.5), ("IIZII", -2.0)]) for k in range(40)]
    plain = sim.DeviceEstimator(noise, DEV).run(circuits, obs)
    assert plain.status() == "DONE" and plain.job_id().startswith("sim-")
    res = plain.result()
    want = np.asarray([sc.simulate(Circuit.from_any(c), o.to_list(), noise)[0] for c, o in zip(circuits, obs)])
    bound = max(sc.value_bound(Circuit.from_any(c), o.to_list(), noise) for c, o in zip(circuits, obs))
    print(f"DeviceEstimator: max |device - oracle| {np.abs(res.values - want).max():.3e} <= {bound:.3e}")
    assert bound < sc.CAP and np.abs(res.values - want).max() <= bound and res.metadata == [{}] * 40

    props = get_backend_properties_v1(lima_backend)
    ideal = sim.expectation_values(circuits, ["IIIIZ"] * 40, None, DEV)[0]
    noisy = host(sim.expectation_values(circuits, ["IIIIZ"] * 40, noise, DEV)[0])
    rows = torch.cat([encode_data(circuits=[c], properties=props, ideal_exp_vals=[[0.0]], noisy_exp_vals=[[float(v)]], num_qubits=1,
                                  meas_bases=encode_pauli_sum_op([("IIIIZ", 1.0)]))[0] for c, v in zip(circuits, noisy)])
    model = LinearRegressor.fit(rows.to(DEV, dtype=torch.float32), ideal.to(torch.float32), alpha=1e-3)
    mitigated = learning(sim.DeviceEstimator, LinearLearningModelProcessor(model, lima_backend, device=DEV), skip_transpile=True)
    out = mitigated(noise, DEV).run(circuits, obs).result()
    assert out.values.shape == (40,) and np.isfinite(out.values).all()
    assert [m["original_value"] for m in out.metadata] == res.values.tolist()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def test_exp_value_generator_end_to_end():
    from blackwater.data.generators.exp_val import ExpValueEntry, exp_value_generator
    from blackwater.data.synthetic import random_circuit, synthetic_backend

    backend = synthetic_backend(4, "cx")
    entries = list(exp_value_generator(backend, 4, 6, 3, max_entries=64, batch=48, device=DEV))
    assert len(entries) == 64 and all(isinstance(e, ExpValueEntry) for e in entries)
    # the same draws again, for the oracle
    noise = sim.NoiseModel.from_backend(backend, readout=False)
    rng = np.random.default_rng(0)
    from blackwater.data.utils import generate_random_pauli_sum_op

    k = 0
    for count in (48, 16):
        drawn = []
        for _ in range(count):
            depth = int(rng.integers(1, 7))
            c = random_circuit(4, depth, int(rng.integers(0, 2 ** 31 - 1)), two_q="cx")
            drawn.append((c, generate_random_pauli_sum_op(4, 3, 1.0, rng=rng).to_list()))
        for c, terms in drawn:
            e = entries[k]
            total = sum(abs(cf) for _, cf in terms)
            assert abs(e.ideal_exp_value) <= total + 1e-12 and [row[0] for row in e.observable] == [cf for _, cf in terms]
            want_ideal, want_noisy = sc.simulate(c, terms)[0], sc.simulate(c, terms, noise)[0]
            bi, bn = sc.value_bound(c, terms), sc.value_bound(c, terms, noise)
            assert bi < sc.CAP and bn < sc.CAP
            assert abs(e.ideal_exp_value - want_ideal) <= bi and abs(e.noisy_exp_values[0] - want_noisy) <= bn, k
            noisy_gates = any(noise.after_gate(i, op.name, op.qubits) for i, op in enumerate(c.ops) if op.name not in ("barrier", "measure"))
            if noisy_gates and abs(want_noisy - want_ideal) > bi + bn:
                assert e.noisy_exp_values[0] != e.ideal_exp_value, k
            k += 1
    assert k == 64


def test_encode_corpus_with_simulated_labels():
    from blackwater.data.synthetic import encode_corpus, random_circuit, synthetic_backend

    circuits = [random_circuit(4, 2 + k, k) for k in range(6)]
    noise = sim.NoiseModel.from_backend(synthetic_backend(4, "cx"))
    plain = encode_corpus(circuits, 4, seed=7)
    got = encode_corpus(circuits, 4, seed=7, simulate=noise, device=DEV)
    assert all(np.array_equal(np.asarray(plain[k]), np.asarray(got[k])) for k in ("depth", "observable"))
    for k, c in enumerate(circuits):
        qz = int(np.argmax(got["observable"][k, 0, 2::4]))
        label = "".join("Z" if q == qz else "I" for q in reversed(range(4)))
        ideal, noisy = sc.simulate(c, [(label, 1.0)])[0], sc.simulate(c, [(label, 1.0)], noise)[0]
        assert got["y"][k, 0] == np.float32(ideal) or abs(got["y"][k, 0] - ideal) <= 6e-8 + sc.term_bound(c)
        assert abs(got["noisy"][k, 0] - noisy) <= 6e-8 + sc.term_bound(c, noise)   # float32 storage: 2^-24 of a value <= 1


# ---- quality (recorded first; the assertion depends on what the CPU twin earns) ---------------------------------------------------------
def test_linear_mitigation_of_simulated_ising_labels(lima_backend, golden):
    """The 600 Ising circuits, per-classical-bit <Z>: noisy from the lima model (depolarising + readout), ideal exact;
    ``encode_data_v2_ecr`` rows + noisy -> ideal fitted by the device's ``LinearRegressor`` on the train split and scored on the
    validation split as the ratio of the unmitigated to the mitigated mean L2.  The split is the project's ``pooled_split(seed=0)``
    (train = the step-0 file + 70 % of each later Trotter step, 510 circuits; validation = the other 90): the step-0 validation
    file alone is degenerate here -- all its circuits share one gate structure, so under a deterministic noise model ideal is an
    exact affine function of noisy and OLS recovers it to 1e-8.  The same pipeline on the CPU (numpy oracle, scikit-learn's
    LinearRegression) is the twin: its ratio is 5.16 (unmitigated 0.1211, mitigated 0.0235), at least 1.5, so the device ratio is
    asserted to exceed 1; had the twin stayed below 1.5, only agreement within 1 % would be asserted."""
    pytest.importorskip("sklearn")
    from sklearn.linear_model import LinearRegression

    from blackwater.library.learning.features import encode_data_v2_ecr
    from blackwater.nn import LinearRegressor

    pick = np.arange(300, 900)
    texts = [golden["texts"][i] for i in pick]
    circuits = [golden["circuits"][i] for i in pick]
    obs = [golden["observables"][i] for i in pick]
    from blackwater.metrics.accuracy import pooled_split

    train_ids, val_ids = pooled_split(golden["split"][pick], seed=0)
    train, val = np.zeros(600, dtype=bool), np.zeros(600, dtype=bool)
    train[train_ids], val[val_ids] = True, True
    assert train.sum() == 510 and val.sum() == 90
    noise = sim.NoiseModel.from_backend(lima_backend)

    def l2(a, b):
        return float(np.mean(np.linalg.norm(a - b, axis=1)))

    # the device
    ideal_d = host(sim.expectation_values(texts, obs, None, DEV)[1]).reshape(600, 4)
    noisy_d = host(sim.expectation_values(texts, obs, noise, DEV)[1]).reshape(600, 4)
    x_d, _ = encode_data_v2_ecr(texts, ideal_d.tolist(), noisy_d.tolist(), 4, two_q_gate="cx")
    model = LinearRegressor.fit(x_d[torch.from_numpy(train)].to(DEV), torch.from_numpy(ideal_d[train]).to(DEV, dtype=torch.float32))
    pred_d = host(model.predict(x_d[torch.from_numpy(val)].to(DEV)))
    ratio_d = l2(noisy_d[val], ideal_d[val]) / l2(pred_d, ideal_d[val])
    # the CPU twin
    ideal_c = golden["oracle"][pick]
    noisy_c = np.asarray([sc.simulate(c, o, noise)[1] for c, o in zip(circuits, obs)])
    bound = max(sc.term_bound(c, noise) for c in circuits)
    assert bound < sc.CAP and np.abs(noisy_d - noisy_c).max() <= bound
    x_c, _ = encode_data_v2_ecr(texts, ideal_c.tolist(), noisy_c.tolist(), 4, two_q_gate="cx")
    x_c = x_c.numpy().astype(np.float64)
    ols = LinearRegression().fit(x_c[train], ideal_c[train])
    ratio_c = l2(noisy_c[val], ideal_c[val]) / l2(ols.predict(x_c[val]), ideal_c[val])
    print(f"Ising validation split: unmitigated L2 {l2(noisy_d[val], ideal_d[val]):.6f}, mitigated {l2(pred_d, ideal_d[val]):.6f}; "
          f"unmitigated / mitigated: device {ratio_d:.6f}, CPU twin {ratio_c:.6f}")
    if ratio_c >= 1.5:
        assert ratio_d > 1.0
    else:
        assert abs(ratio_d / ratio_c - 1.0) <= 0.01


def test_ngem_decorator_around_the_device_estimator(lima_backend, g1):
    from blackwater.library.ngem.estimator import NgemJob, ngem

    class Doubling(torch.nn.Module):
        def forward(self, exp_value, observable, circuit_depth, nodes, edge_index, batch):
            return exp_value * 2

    noise = sim.NoiseModel.from_backend(lima_backend)
    circuits = list(g1["qasm"][:3])
    obs = [PauliObservable("IIIIZ"), PauliObservable([("IIIZI", 0.5)]), PauliObservable("IIZII")]
    plain = sim.DeviceEstimator(noise, DEV).run(circuits, obs).result().values
    job = ngem(sim.DeviceEstimator, Doubling(), lima_backend)(noise, DEV).run(circuits, obs)
    assert isinstance(job, NgemJob) and job.status() == "DONE"
    got = job.result().values
    want = 2.0 * plain   # the model sees the whole-observable value (in float32) and returns the mitigated one
    print("ngem around DeviceEstimator:", got, "plain:", plain)
    assert np.allclose(got, want, rtol=0, atol=1e-6)
