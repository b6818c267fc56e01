"""Pauli-frame sampling on the device (mlqem_clifford_sample_f64) against the host interpreter of
tests/clifford_frames_cases.py, bit for bit, and against oracles that share nothing with it."""
import numpy as np
import pytest
import torch

import clifford_cases as cc
import clifford_frames_cases as fc
from blackwater import sim

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _group_bits(res, g):
    """uint32 [shots, W] of group ``g`` of a device result."""
    batch = res.batch
    _, _, w, _ = fc.group_shape(batch, g)
    b = int(batch.ref_ptr[g]) * res.shots
    return _u32(res.bits[b:b + res.shots * w]).reshape(res.shots, w)


def _assert_equal_to_interpreter(res, want, batch, exact=None):
    assert (_u32(res.reference) == want["reference"]).all()
    for g in range(len(batch.group_circ)):
        assert (_group_bits(res, g) == want["bits"][g]).all(), g
    assert (res.term_sums.cpu().numpy().astype(np.int64) == want["term_sums"]).all()
    tv = res.term_values.cpu().numpy()
    assert tv.tobytes() == want["term_values"].tobytes()
    values, variance = res.values.cpu().numpy(), res.variance.cpu().numpy()
    for c in range(len(batch)):
        bound = fc.value_bound(batch, c, want["scale"][c])
        print(f"circuit {c}: |values - sum| = {abs(values[c] - want['values'][c]):.3e}, |variance - sum| = "
              f"{abs(variance[c] - want['variance'][c]):.3e}, bound {bound:.3e}")
        assert abs(values[c] - want["values"][c]) <= bound and abs(variance[c] - want["variance"][c]) <= bound
    if exact is not None:   # the statistical condition: follows from bit-equality, asserted anyway
        ok, sigma = fc.five_sigma(tv, exact, res.shots)
        print(f"shots {res.shots}: worst deviation {sigma:.2f} sigma")
        assert ok


# ---- bit-equality over the grid ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mixed", fc.GRID_COMBOS)
def test_grid_equals_the_interpreter_bit_for_bit(kind, mixed):
    """n in {1, 2, 5, 31, 32, 33, 64, 65, 128, 129, 512} in one batch, at every shots of {1, 63, 64, 65, 255, 256, 257, 600}."""
    _, _, _, batch, exact = fc.grid_batch(kind, mixed)
    for shots in fc.GRID_SHOTS:
        res = sim.run_clifford_frames(batch, shots, fc.GRID_SEED, return_bits=True, device=DEV)
        _assert_equal_to_interpreter(res, fc.grid_oracle(kind, mixed, shots), batch, exact)


# ---- batch and replay ------------------------------------------------------------------------------------------------------------------------
def test_alone_in_a_batch_and_in_a_replayed_graph():
    from blackwater.native import ops

    widths, shots, seed = [5, 100, 129, 512, 33], 300, 11
    noise = fc.FixedNoise(None, seed=9)
    circs = [cc.random_clifford_program(n, 40, n + 1, measure=True, local=4) for n in widths]
    obs = [cc.random_terms(n, 5, n, alphabet="IXYZ", weight=3) for n in widths]
    keys = np.asarray([7, 2 ** 33 + 5, 11, 13, 2 ** 40], dtype=np.int64)
    batch = sim.compile_clifford_frames(circs, obs, noise)
    assert batch.n_reg > 0 and batch.n_lds > 0
    both = sim.run_clifford_frames(batch, shots, seed, run_keys=keys, return_bits=True, device=DEV)
    want = fc.interpret(batch, shots, seed, keys)
    _assert_equal_to_interpreter(both, want, batch)
    for k in range(len(widths)):
        alone = sim.run_clifford_frames(sim.compile_clifford_frames([circs[k]], [obs[k]], noise), shots, seed, run_keys=keys[k:k + 1],
                                        return_bits=True, device=DEV)
        tb, te = int(batch.term_ptr[k]), int(batch.term_ptr[k + 1])
        assert (alone.term_sums.cpu().numpy() == both.term_sums.cpu().numpy()[tb:te]).all()
        assert alone.values.cpu().numpy().tobytes() == both.values.cpu().numpy()[k:k + 1].tobytes()
        assert alone.variance.cpu().numpy().tobytes() == both.variance.cpu().numpy()[k:k + 1].tobytes()
        for j, g in enumerate(range(int(batch.group_ptr[k]), int(batch.group_ptr[k + 1]))):
            assert (_group_bits(alone, j) == _group_bits(both, g)).all()
    # captured once, replayed twice
    t = batch.to(DEV)
    dev_keys = torch.from_numpy(keys).to(DEV)
    n_ref, n_terms = int(batch.ref_ptr[-1]), len(batch.coeff)
    out = dict(rows=torch.zeros(batch.n_rows, dtype=torch.int32, device=DEV), reference=torch.zeros(n_ref, dtype=torch.int32, device=DEV),
               bits=torch.zeros(n_ref * shots, dtype=torch.int32, device=DEV), term_sums=torch.zeros(n_terms, dtype=torch.int32, device=DEV),
               term_values=torch.zeros(n_terms, dtype=torch.float64, device=DEV), values=torch.zeros(len(batch), dtype=torch.float64, device=DEV),
               variance=torch.zeros(len(batch), dtype=torch.float64, device=DEV))

    def call():
        ops.clifford_sample(t["n_qubits"], t["op_ptr"], t["ops"], t["thresh"], t["ro_ptr"], t["group_ptr"], t["group_circ"], t["group_mask"],
                            t["ids"], batch.n_reg, batch.n_lds, t["masks"], t["term_ptr"], t["coeff"], t["term_mask"], t["gterm_ptr"],
                            t["gterm"], dev_keys, shots, seed, batch.max_qubits, t["row_ptr"], batch.n_rows, t["ref_ptr"], n_ref, **out)

    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(2):
        for buf in out.values():
            buf.fill_(-1 if buf.dtype == torch.int32 else float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert (out["bits"] == both.bits).all() and (out["reference"] == both.reference).all()
        assert (out["term_sums"] == both.term_sums).all()
        for name in ("term_values", "values", "variance"):
            assert out[name].cpu().numpy().tobytes() == getattr(both, name).cpu().numpy().tobytes(), name


# ---- independent of the interpreter --------------------------------------------------------------------------------------------------------------
def test_ghz_over_130_qubits():
    n, shots = 130, 512
    res = sim.sample_clifford_expectation_values([fc.ghz(n)] * 2, [[("Z" * n, 1.0)], [("X" * n, 1.0)]], shots=shots, seed=3,
                                                 return_bits=True, device=DEV)
    z_outcomes = set(fc.outcomes_as_integers(_group_bits(res, 0)))
    assert z_outcomes == {0, (1 << n) - 1}   # every shot all-0 or all-1, and both occur
    x_bits = _group_bits(res, 1)
    assert len(set(fc.outcomes_as_integers(x_bits))) > shots // 2   # 2^129 outcomes
    parity = np.zeros(shots, dtype=np.uint32)
    for j in range(x_bits.shape[1]):
        parity ^= x_bits[:, j]
    assert all(bin(int(v)).count("1") % 2 == 0 for v in parity)   # X^(x)130 stabilises the state
    assert res.term_values.cpu().numpy().tolist() == [1.0, 1.0]   # 130 is even: both Z outcomes have even parity
    counts = sim.frame_counts(res, 0)
    assert len(counts) == 1 and set(counts[0]) == {"0" * n, "1" * n} and sum(counts[0].values()) == shots


@pytest.mark.parametrize("noisy", [False, True])
def test_blocks_across_word_boundaries_follow_their_simulated_probabilities(noisy):
    """Blocks of 4 qubits across 31|32, 127|128 and 255|256 of a 512-qubit register: the state is a product over the blocks, so a
    block's outcome frequencies are within five sigma of ``sim_cases.simulate``'s probabilities of the block alone (with noise:
    depolarising after every gate and asymmetric readout, a density matrix of 4 qubits)."""
    n, shots = 512, 4096
    positions = [[30, 31, 32, 33], [126, 127, 128, 129], [254, 255, 256, 257]]
    block = cc.BlockCircuit(n, positions, 12, seed=5)
    noise = fc.FixedNoise(None, readout=(0.02, 0.07), seed=4) if noisy else None
    res = sim.sample_clifford_expectation_values([block.wide], [[("I" * (n - 1) + "Z", 1.0)]], noise, shots=shots, seed=17,
                                                 return_bits=True, device=DEV)
    outcomes = fc.outcomes_as_integers(_group_bits(res, 0))
    for b, pos in enumerate(positions):
        p = fc.outcome_probabilities(block.block_circuit(b), "ZZZZ", block.block_noise(b, noise))
        local = [sum((v >> q & 1) << j for j, q in enumerate(pos)) for v in outcomes]
        freq = np.bincount(local, minlength=16) / shots
        assert (np.abs(freq - p) <= 5 * np.sqrt(np.maximum(p * (1 - p), 0.0) / shots) + 1.0 / shots).all(), (b, freq, p)
    rest = ~sum(1 << q for pos in positions for q in pos) & ((1 << n) - 1)
    if not noisy:
        assert all(v & rest == 0 for v in outcomes)   # the idle qubits read 0


def test_identity_circuits_give_zeros_and_hadamards_no_repeats():
    n, shots = 100, 1024
    res = sim.sample_clifford_expectation_values([fc.layer(n, "id"), fc.layer(n, "h"), fc.layer(5, "id")],
                                                 [[("Z" * n, 1.0)], [("Z" * n, 1.0)], [("ZZZZZ", 1.0)]], shots=shots, seed=5,
                                                 return_bits=True, device=DEV)
    assert not _group_bits(res, 0).any() and not _group_bits(res, 2).any()
    assert len(set(fc.outcomes_as_integers(_group_bits(res, 1)))) == shots   # 100-bit strings: a repeat has probability 2^-81
    assert res.term_values.cpu().numpy()[[0, 2]].tolist() == [1.0, 1.0]


# ---- the public interface ----------------------------------------------------------------------------------------------------------------------
def test_estimator_corpus_and_generator():
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import clifford_tfim_circuit, encode_corpus, synthetic_backend

    nq, shots = 100, 2000
    circs = [clifford_tfim_circuit(nq, s, 1, 2) for s in (1, 2)]
    obs = [[("I" * (nq - 1 - q) + "Z" + "I" * q, 1.0) for q in (3, 50)] for _ in circs]
    noise = sim.NoiseModel.from_backend(synthetic_backend(nq, "ecr"))
    exact = sim.clifford_expectation_values(circs, obs, noise, DEV)[0].cpu().numpy()
    est = sim.DeviceEstimator(noise, device=DEV, method="frames", shots=shots, seed=2)
    first, second = est.run(circs, obs).result(), est.run(circs, obs).result()
    assert [m["shots"] for m in first.metadata] == [shots, shots] and all(m["variance"] > 0 for m in first.metadata)
    assert (np.asarray(first.values) != np.asarray(second.values)).any()   # job 2 draws with other run keys
    again = sim.DeviceEstimator(noise, device=DEV, method="frames", shots=shots, seed=2).run(circs, obs).result()
    assert np.asarray(again.values).tobytes() == np.asarray(first.values).tobytes()
    direct = sim.sample_clifford_expectation_values(circs, obs, noise, shots=shots, seed=2, run_keys=np.arange(2) + (1 << 32), device=DEV)
    assert direct.values.cpu().numpy().tobytes() == np.asarray(first.values).tobytes()
    sd = np.sqrt([m["variance"] / shots for m in first.metadata])
    assert (np.abs(np.asarray(first.values) - exact) <= 5 * sd + 2.0 / shots).all()
    small = [clifford_tfim_circuit(6, s, 1, 1, two_q="cx") for s in (1, 2, 3)]
    model = sim.NoiseModel.from_backend(synthetic_backend(6, "cx"))
    sampled = encode_corpus(small, 6, simulate=model, device=DEV, frame_shots=4000)
    exactly = encode_corpus(small, 6, simulate=model, device=DEV, clifford=True)
    assert sampled["y"].tobytes() == exactly["y"].tobytes()   # the ideal value stays the exact one
    assert (np.abs(sampled["noisy"] - exactly["noisy"]) <= 5 / np.sqrt(4000) + 1e-3).all() and (sampled["noisy"] != exactly["noisy"]).any()
    entries = list(exp_value_generator(synthetic_backend(6, "cx"), 6, 3, 2, max_entries=3, seed=1, device=DEV, frame_shots=500))
    assert len(entries) == 3 and all(abs(e.noisy_exp_values[0]) <= 2.0 + 1e-9 for e in entries)
