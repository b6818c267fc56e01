"""Quantum trajectories on the device (mlqem_sim_run_trajectories_f64) against the interpreter of tests/traj_cases.py, which follows
the contract of include/mlqem_hip.h draw by draw.

Every trajectory of every case is compared, none excluded: tests/test_traj_cpu.py asserts that no draw of these seeds lies within
1e-9 of a threshold, so the device and the interpreter choose the same operators and differ by rounding alone, within the bound
derived in traj_cases.py (asserted below 1e-11 there and here).  Bit-equality is asserted where the contract promises it: a
circuit alone and in a batch, any split of the batch, a prefix of a longer run, wave and workgroup units in one batch."""
import numpy as np
import pytest
import torch

import relax_cases as rc
import sim_cases as sc
import traj_cases as tc
from blackwater import sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = tc.grid()


def host(t):
    return t.cpu().numpy()


def case_named(noise, sizes):
    return next(c for c in GRID if c["noise"] == noise and c["sizes"] == sizes)


@pytest.mark.parametrize("case", GRID, ids=[c["id"] for c in GRID])
def test_device_against_the_interpreter(case):
    batch = tc.lower(case)
    res = sim.run_trajectories(batch, seed=case["seed"], device=DEV, keep_trajectories=True)
    traj, ptr = host(res.traj_term_values), batch.term_ptr
    assert traj.shape == (case["trajectories"], int(ptr[-1])) and res.trajectories == case["trajectories"]
    term_values, term_se, values, se, norm = (host(x) for x in (res.term_values, res.term_std_error, res.values, res.std_error, res.norm))
    for j, ref in enumerate(tc.reference(case["id"])):
        tb, vb, nb = tc.term_bound(ref), tc.value_bound(ref), tc.norm_bound(ref)
        assert tb.max() < tc.CAP and vb.max() < tc.CAP and nb.max() < tc.CAP
        got = traj[:, int(ptr[j]):int(ptr[j + 1])]
        worst = float(np.max(np.abs(got - ref["terms"]) / tb[:, None]))
        print(f"{case['id']} circuit {j} ({batch.variant[j]}, n = {ref['n']}): max |terms - interpreter| / bound = {worst:.3f}, "
              f"bound <= {tb.max():.3e}, margin {ref['margin'].min():.2e}")
        assert (np.abs(got - ref["terms"]) <= tb[:, None]).all()
        mean, err = tc.mean_and_error(ref["terms"])
        sl = slice(int(ptr[j]), int(ptr[j + 1]))
        assert (np.abs(term_values[sl] - mean) <= tc.mean_bound(tb[:, None], ref["terms"])).all()
        assert (np.abs(term_se[sl] - err) <= tc.error_bound(tb[:, None], ref["terms"])).all()
        vmean, verr = tc.mean_and_error(ref["values"])
        assert abs(values[j] - vmean) <= tc.mean_bound(vb, ref["values"])
        assert abs(se[j] - verr) <= tc.error_bound(vb, ref["values"])
        assert abs(norm[j] - ref["norm"].mean()) <= tc.mean_bound(nb, ref["norm"]) and abs(norm[j] - 1.0) <= nb.mean() + 64 * tc.U
        if case["trajectories"] == 1:
            assert se[j] == 0.0 and (term_se[sl] == 0.0).all()


def test_an_empty_noise_model_is_the_state_vector():
    circuits = [sc.random_program(n, 14, seed=500 + n) for n in (3, 8, 9)]
    observables = [sc.term_set(n, seed=n) for n in (3, 8, 9)]
    res = sim.trajectory_expectation_values(circuits, observables, sim.NoiseModel(), trajectories=5, seed=1, device=DEV)
    _, exact, ptr = sim.expectation_values(circuits, observables, None, DEV)
    batch = sim.compile_programs(circuits, observables, sim.NoiseModel(), trajectories=5)
    traj = host(sim.run_trajectories(batch, seed=1, device=DEV, keep_trajectories=True).traj_term_values)
    exact, ptr = host(exact), host(ptr)
    for j, c in enumerate(circuits):
        bound = sc.term_bound(c)
        assert bound < sc.CAP
        assert (np.abs(traj[:, ptr[j]:ptr[j + 1]] - exact[None, ptr[j]:ptr[j + 1]]) <= bound).all()
    assert (host(res.term_std_error) <= (5 + 8) * tc.U * 2.0).all() and (host(res.std_error) <= (5 + 8) * tc.U * 8.0).all()
    assert (np.abs(host(res.norm) - 1.0) <= 1e-13).all()


def test_same_bits_alone_split_prefix_and_mixed():
    wave, wg = case_named("line-p03", tc.WAVE), case_named("line-p03", tc.WORKGROUP)
    noise, seed = tc.model("line-p03"), 77
    circuits, observables = wave["circuits"] + wg["circuits"], wave["observables"] + wg["observables"]
    mixed = sim.compile_programs(circuits, observables, noise, trajectories=64)   # wave and workgroup units in one batch
    assert mixed.n_wave == 5 and mixed.n_wg == 5
    full = sim.run_trajectories(mixed, seed=seed, device=DEV, keep_trajectories=True)
    traj, ptr = host(full.traj_term_values), mixed.term_ptr
    # the two halves as batches of their own, with the run keys they had in the mixed batch
    for lo, case in ((0, wave), (5, wg)):
        part = sim.run_trajectories(sim.compile_programs(case["circuits"], case["observables"], noise, trajectories=64), seed=seed,
                                    run_keys=np.arange(lo, lo + 5), device=DEV, keep_trajectories=True)
        assert np.array_equal(host(part.traj_term_values), traj[:, int(ptr[lo]):int(ptr[lo + 5])])
        for name in ("values", "std_error", "norm"):
            assert np.array_equal(host(getattr(part, name)), host(getattr(full, name))[lo:lo + 5]), name
    # a circuit alone, with its run key
    for j in (3, 4, 6):
        alone = sim.run_trajectories(sim.compile_programs([circuits[j]], [observables[j]], noise, trajectories=64), seed=seed,
                                     run_keys=[j], device=DEV, keep_trajectories=True)
        assert np.array_equal(host(alone.traj_term_values), traj[:, int(ptr[j]):int(ptr[j + 1])])
        assert host(alone.values)[0] == host(full.values)[j] and host(alone.std_error)[0] == host(full.std_error)[j]
    # a buffer budget that forces one circuit per call
    split = sim.run_trajectories(mixed, seed=seed, device=DEV, keep_trajectories=True, buffer_bytes=1)
    for name in ("values", "std_error", "term_values", "term_std_error", "norm", "traj_term_values"):
        assert np.array_equal(host(getattr(split, name)), host(getattr(full, name))), name
    # T = 37 is a prefix of T = 64
    short = sim.run_trajectories(sim.compile_programs(circuits, observables, noise, trajectories=37), seed=seed, device=DEV,
                                 keep_trajectories=True)
    assert np.array_equal(host(short.traj_term_values), traj[:37])
    other = sim.run_trajectories(mixed, seed=seed + 1, device=DEV, keep_trajectories=True)
    assert not np.array_equal(host(other.traj_term_values), traj)


@pytest.mark.parametrize("case,keep", tc.small_cases(5), ids=lambda v: v["id"] if isinstance(v, dict) else None)
def test_mean_against_the_devices_exact_answer(case, keep):
    """n <= 5: the mean over 4 096 device trajectories against the density-matrix kernel, within 5 standard errors of the
    INTERPRETER's sample (plus the two rounding bounds)."""
    noise = tc.model(case["noise"])
    circuits, observables = [case["circuits"][j] for j in keep], [case["observables"][j] for j in keep]
    res = sim.trajectory_expectation_values(circuits, observables, noise, trajectories=tc.LONG, seed=case["seed"], run_keys=keep, device=DEV)
    _, exact, ptr = sim.expectation_values(circuits, observables, noise, DEV)
    got, exact, ptr = host(res.term_values), host(exact), host(ptr)
    ref = tc.long_reference(case["id"], 6)
    for k, j in enumerate(keep):
        _, err = tc.mean_and_error(ref[j]["terms"])
        rounding = tc.mean_bound(tc.term_bound(ref[j])[:, None], ref[j]["terms"]) + rc.term_bound(circuits[k], noise)
        sl = slice(int(ptr[k]), int(ptr[k + 1]))
        print(case["id"], j, "max |mean - exact| / se:", float(np.max(np.abs(got[sl] - exact[sl]) / np.maximum(err, 1e-300) * (err > 1e-12))))
        assert (np.abs(got[sl] - exact[sl]) <= 5.0 * err + rounding).all()


def test_estimator_generator_and_corpus():
    noise = tc.model("line-p03")
    circuit = tc.line_circuit(8, 901)
    assert not sim.is_clifford(circuit)
    obs = sc.term_set(8, seed=4)
    with pytest.raises(ValueError, match="8 qubits need 65536 amplitudes as a density matrix"):
        sim.DeviceEstimator(noise, DEV).run([circuit], [obs])
    est = sim.DeviceEstimator(noise, DEV, method="trajectories", trajectories=64, seed=3)
    result = est.run([circuit, circuit], [obs, obs]).result()
    want = sim.trajectory_expectation_values([circuit, circuit], [obs, obs], noise, trajectories=64, seed=3,
                                             run_keys=sim.default_run_keys(2, 1 << 32), device=DEV)
    assert np.array_equal(np.asarray(result.values), host(want.values))
    assert [m["trajectories"] for m in result.metadata] == [64, 64]
    assert [m["std_error"] for m in result.metadata] == host(want.std_error).tolist() and result.metadata[0]["std_error"] > 0.0
    assert result.values[0] != result.values[1]   # two run keys: two samples

    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import encode_corpus, random_circuit
    from blackwater.data.utils import generate_random_pauli_sum_op

    backend = tc.table(6)
    entries = {b: list(exp_value_generator(backend, 6, 3, 3, max_entries=5, seed=11, batch=b, device=DEV, trajectories=64)) for b in (1, 256)}
    rng = np.random.default_rng(11)   # the generator's own draws, in its order
    circuits, observables = [], []
    for _ in range(5):
        depth = int(rng.integers(1, 4))
        circuits.append(random_circuit(6, depth, int(rng.integers(0, 2 ** 31 - 1)), two_q="cx"))
        observables.append(generate_random_pauli_sum_op(6, 3, 1.0, rng=rng))
    model = sim.NoiseModel.from_backend(backend, readout=False)
    want = host(sim.trajectory_expectation_values(circuits, observables, model, trajectories=64, seed=11, run_keys=np.arange(5), device=DEV).values)
    ideal = host(sim.expectation_values(circuits, observables, None, DEV)[0])
    for b in (1, 256):
        assert [e.noisy_exp_values[0] for e in entries[b]] == want.tolist()
        assert [e.ideal_exp_value for e in entries[b]] == ideal.tolist()

    corpus_circuits = [random_circuit(6, 3, 40 + k, two_q="cx") for k in range(3)]
    corpus = encode_corpus(corpus_circuits, 6, two_q="cx", seed=7, simulate=noise, device=DEV, trajectories=32)
    zq = [int(np.flatnonzero(o[0, 2::4])[0]) for o in corpus["observable"]]
    labels = ["".join("Z" if q == z else "I" for q in reversed(range(6))) for z in zq]
    want = host(sim.trajectory_expectation_values(corpus_circuits, labels, noise, trajectories=32, seed=7, run_keys=np.arange(3), device=DEV).values)
    assert np.array_equal(corpus["noisy"][:, 0], want.astype(np.float32))
