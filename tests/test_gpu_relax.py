"""The fused noise records on the device (MLQEM_SIM_OP_NOISE1 / NOISE2 in every instantiation of the simulator kernel) against the
Kraus oracle of tests/relax_cases.py.

Every comparison uses the bound DERIVED in relax_cases.py (sim_cases' recursion carrying each relaxation's Frobenius operator
norm), and every case asserts that its bound stays below 1e-11.  Bit-equality is asserted where the contract promises it: a circuit
alone, in a batch of mixed variants and in a replayed graph; a folded run against the plain kernel on the host-folded program."""
import dataclasses

import numpy as np
import pytest
import torch

import relax_cases as rc
import shots_cases as shc
import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import Circuit
from blackwater.native import ops
from blackwater.sim import zne
from blackwater.sim.program import OP_NOISE1, OP_NOISE2, OP_U2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = rc.grid()


def host(t):
    return t.cpu().numpy()


def run_plain(batch):
    return [host(x) for x in sim.run_batch(batch, DEV)]


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID, ids=[c[0] for c in GRID])
def test_device_against_the_kraus_oracle(case):
    """The closed forms of the kernel against the Kraus sums of the oracle, and Tr rho = 1, within the derived bound: n = 1 .. 5 with
    40 random ops under a random relaxation model (NOISE1 alone at n = 1, NOISE2 on the whole state at n = 2, the wave variant up
    to n = 4, the workgroup variant at n = 5), the corners lambda in {0, 1}, g in {0, 1}, c in {0, sqrt(1 - g)}, p1 in {0, 0.5, 1},
    NOISE2 on every ordered pair of n = 3 and on (0, 4), (4, 0), (2, 3) of n = 5."""
    name, c, terms, noise = case
    terms = list(terms)
    tb, vb = rc.term_bound(c, noise), rc.value_bound(c, terms, noise)
    assert tb < rc.CAP and vb < rc.CAP
    batch = sim.compile_programs([c], [terms], noise)
    values, term_values, norm = run_plain(batch)
    ov, otv, _ = rc.grid_oracle()[name]
    dv, dt, dn = abs(values[0] - ov), float(np.abs(term_values - otv).max()), abs(norm[0] - 1.0)
    print(f"{name} ({batch.variant[0]}, {int(batch.op_counts[0])} records): |value| {dv:.3e} <= {vb:.3e}, |terms| {dt:.3e} <= {tb:.3e}, "
          f"|norm - 1| {dn:.3e}")
    assert dv <= vb and dt <= tb and dn <= tb
    assert batch.variant == ["wave" if c.num_qubits <= 4 else "workgroup"]
    assert {OP_NOISE1, OP_NOISE2} & set(batch.ops[:, 0].tolist())


def test_exact_identities():
    """lambda = 0 with g = 0, c = 1 is an exact identity of both passes: the same bits as the program without the records."""
    class Nothing(sc.NoNoise):
        def relaxation_after(self, index, name, qubits):
            return ((0.0, 1.0, 0.5),) * len(qubits)

    for n in (2, 5):
        c, terms = sc.random_program(n, 20, seed=33), sc.term_set(n)
        with_records, without = sim.compile_programs([c], [terms], Nothing()), sim.compile_programs([c], [terms], sc.NoNoise())
        assert {OP_NOISE1, OP_NOISE2} <= set(with_records.ops[:, 0].tolist()) and len(with_records.ops) > len(without.ops)
        a, b = run_plain(with_records), run_plain(without)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- batching ----------------------------------------------------------------------------------------------------------------------------
def test_the_same_bits_alone_in_a_mixed_batch_and_in_a_replayed_graph():
    cases = [g for g in GRID if g[0].startswith(("random", "corners", "pair-n5-04", "pair-n3-21"))]
    circuits, observables = [g[1] for g in cases], [list(g[2]) for g in cases]
    # every circuit has its own spec and compile_programs asks one model, so the batch is lowered circuit by circuit
    batches = [sim.compile_programs([c], [o], g[3]) for c, o, g in zip(circuits, observables, cases)]
    alone = [run_plain(b) for b in batches]
    # one batch of all of them: concatenate the lowered programs (records and parameters are position-independent but for offsets)
    ops_all, params, op_ptr, terms_all, coeff, term_ptr, circ = [], [], [0], [], [], [0], []
    for b in batches:
        o = b.ops.copy()
        o[:, 3] += len(params)
        ops_all.append(o)
        params += b.params[:len(b.params) - 32].tolist()
        op_ptr.append(op_ptr[-1] + len(o))
        terms_all.append(b.terms)
        coeff += b.coeff.tolist()
        term_ptr.append(term_ptr[-1] + len(b.terms))
        circ.append(b.circ[0])
    variant = [b.variant[0] for b in batches]
    wave, wg = [i for i, v in enumerate(variant) if v == "wave"], [i for i, v in enumerate(variant) if v != "wave"]
    assert wave and wg
    mixed = dataclasses.replace(batches[0], circ=np.asarray(circ, dtype=np.int32), op_ptr=np.asarray(op_ptr, dtype=np.int64),
                                ops=np.concatenate(ops_all), params=np.asarray(params + [0.0] * 32), term_ptr=np.asarray(term_ptr, dtype=np.int64),
                                terms=np.concatenate(terms_all), coeff=np.asarray(coeff), ids=np.asarray(wave + wg, dtype=np.int32),
                                n_wave=len(wave), n_wg=len(wg), variant=variant)
    t = mixed.to(DEV)
    args = (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"], t["n_wave"], t["n_wg"])
    eager = [host(x) for x in ops.sim_run(*args)]
    for k, one in enumerate(alone):
        b, e = term_ptr[k], term_ptr[k + 1]
        assert eager[0][k] == one[0][0] and np.array_equal(eager[1][b:e], one[1]) and eager[2][k] == one[2][0], cases[k][0]
    outs = {"values": torch.zeros(len(cases), dtype=torch.float64, device=DEV),
            "term_values": torch.zeros(term_ptr[-1], dtype=torch.float64, device=DEV),
            "norm": torch.zeros(len(cases), dtype=torch.float64, device=DEV)}
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


# ---- folded runs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coherent", [False, True], ids=["relaxation", "coherent+relaxation"])
def test_folded_runs_are_the_plain_kernel_on_host_folded_programs(coherent):
    """Factors (1, 3), both variants in one call: row f of the folded call, bit for bit, against the plain kernel on the program of
    relax_cases.expand (records copied, daggers applied in numpy, noise records as they are)."""
    strategy = zne.ZNEStrategy(noise_factors=(1, 3), noise_amplifier=zne.LocalFoldingAmplifier(), extrapolator=zne.PolynomialExtrapolator(1))
    circuits = [sc.random_program(n, 10, seed=44 + n) for n in (1, 2, 4, 5)]
    observables = [sc.term_set(n, seed=2) for n in (1, 2, 4, 5)]
    noise = rc.RelaxNoise(55, g_max=0.1, coherent=range(10) if coherent else ())
    run = zne.zne_run(circuits, observables, noise, strategy, DEV)
    assert set(run.batch.variant) == {"wave", "workgroup"}
    assert int(run.batch.gate_noise_len.max()) == (2 if coherent else 1)
    values, tvs, norm = host(run.values), host(run.term_values), host(run.norm)
    assert values.shape == (2, 4)
    for f in range(2):
        pv, pt, pn = run_plain(rc.expand(run.batch, run.schedules, f))
        assert np.array_equal(values[f], pv) and np.array_equal(tvs[f], pt) and np.array_equal(norm[f], pn), f
    plain = run_plain(run.batch)
    assert np.array_equal(values[0], plain[0]) and np.array_equal(tvs[0], plain[1])          # factor 1 is the circuit itself
    assert not np.array_equal(values[1], values[0])


# ---- measurement shots ---------------------------------------------------------------------------------------------------------------------
def test_measured_batch_at_64_shots():
    """Both variants: the stored probabilities against the diagonal of the oracle's rho within the bound, and the counts reproduced
    from the device's probabilities by the sampling rule of shots_cases (no tolerance)."""
    ns = (1, 3, 4, 5)
    circuits = [sc.random_program(n, 10, seed=60 + n) for n in ns]
    observables = [[("I" * (n - 1) + "Z", 1.0), ("Z" * n, -0.5)] for n in ns]
    noise = rc.RelaxNoise(66, g_max=0.1, coherent=(2, 5))
    res = sim.sample_expectation_values(circuits, observables, noise, shots=64, seed=shc.seed_for(64), device=DEV)
    probs, counts, norm, batch = host(res.probs), host(res.counts), host(res.norm), res.batch
    assert set(batch.variant) == {"wave", "workgroup"} and {OP_NOISE1, OP_NOISE2, OP_U2} <= set(batch.ops[:, 0].tolist())
    for k, c in enumerate(circuits):
        rho, _ = rc.final_state(c, noise)
        tb = rc.term_bound(c, noise)
        assert tb < rc.CAP
        g = int(batch.group_ptr[k])
        assert int(batch.group_ptr[k + 1]) == g + 1
        got = probs[int(batch.prob_ptr[g]):int(batch.prob_ptr[g + 1])]
        err = float(np.abs(got - np.diag(rho).real).max())
        print(f"measured n={c.num_qubits} ({batch.variant[k]}): |probs - oracle| {err:.3e} <= {tb:.3e}, |sum - norm| {abs(got.sum() - norm[k]):.3e}")
        assert err <= tb and abs(got.sum() - norm[k]) <= tb and abs(norm[k] - 1.0) <= tb
        want = shc.sample_counts(got, 64, shc.seed_for(64), k, 0)
        assert np.array_equal(counts[int(batch.prob_ptr[g]):int(batch.prob_ptr[g + 1])], want) and want.sum() == 64


# ---- robustness ------------------------------------------------------------------------------------------------------------------------------
def test_malformed_noise_records_touch_nothing_else():
    """Qubits out of range, q0 == q1 and a parameter offset past the pool in the NOISE records of one circuit: the call completes,
    and the other circuits' outputs are the bits they were.  Nothing here is meant to fault: qubits are clamped to the circuit,
    the offset to the pool, every amplitude index is masked to the state and the stores are predicated; the values are ignored."""
    circuits = [sc.random_program(n, 12, seed=70 + n) for n in (3, 5, 2, 5, 4)]
    observables = [sc.term_set(n, seed=4) for n in (3, 5, 2, 5, 4)]
    batch = sim.compile_programs(circuits, observables, rc.RelaxNoise(77, g_max=0.1))
    good = run_plain(batch)
    for victim in (0, 1):                      # a wave circuit and a workgroup circuit
        b, e = int(batch.op_ptr[victim]), int(batch.op_ptr[victim + 1])
        noise_records = [r for r in range(b, e) if batch.ops[r, 0] in (OP_NOISE1, OP_NOISE2)]
        pair_records = [r for r in noise_records if batch.ops[r, 0] == OP_NOISE2]
        assert len(noise_records) >= 6 and len(pair_records) >= 2
        for what in ("qubits", "same", "offset"):
            bad = batch.ops.copy()
            if what == "qubits":
                bad[noise_records[0::2], 1] = 1000
                bad[noise_records[1::2], 2] = -7
                bad[noise_records[1::2], 1] = 31
            elif what == "same":
                bad[pair_records, 2] = bad[pair_records, 1]
            else:
                bad[noise_records[0::2], 3] = len(batch.params) + 12345
                bad[noise_records[1::2], 3] = -5
            values, term_values, norm = run_plain(dataclasses.replace(batch, ops=bad))
            torch.cuda.synchronize()
            others = np.arange(len(batch)) != victim
            tb, te = int(batch.term_ptr[victim]), int(batch.term_ptr[victim + 1])
            keep = np.ones(len(term_values), dtype=bool)
            keep[tb:te] = False
            assert np.array_equal(values[others], good[0][others]) and np.array_equal(norm[others], good[2][others]), (victim, what)
            assert np.array_equal(term_values[keep], good[1][keep]), (victim, what)


# ---- the reference anchor --------------------------------------------------------------------------------------------------------------------
def test_the_references_noisy_labels_on_the_device(lima_backend):
    """All 900 golden circuits in one call under ``from_backend(lima, readout=False, thermal_relaxation=True)``: every one of the
    3 600 stored 10 000-shot ``noisy`` values within 4 sigma of the device's values (max 3.85 sigma, rms z 0.98: the figures of
    tests/test_relax_cpu.py, which asserts the same for the Kraus oracle on all 900), the Kraus oracle within the derived bound
    on every tenth circuit, and the default depolarising model beyond 4 sigma (114 values, max 12.2 sigma), so that the test
    discriminates.  The labels are reproduced WITHOUT readout noise only; see the CPU test."""
    texts, noisy = rc.golden_noisy()
    circuits = [Circuit.from_any(t) for t in texts]
    observables = [sim.measured_z(c).to_list() for c in circuits]
    noise = sim.NoiseModel.from_backend(lima_backend, readout=False, thermal_relaxation=True)
    batch = sim.compile_programs(texts, observables, noise)
    values, term_values, norm = run_plain(batch)
    got = term_values.reshape(900, 4)
    sig = sc.anchor_sigmas(got, noisy)
    v = -got[:, ::-1]
    z = (noisy - v) / np.maximum(np.sqrt(np.clip(1.0 - v * v, 0.0, None) / 1e4), 1e-3)
    print(f"noisy anchor (device): max {sig.max():.3f} sigma, rms z {np.sqrt((z * z).mean()):.3f} over {sig.size} stored values")
    assert sig.shape == (900, 4) and sig.max() <= 4.0
    for k in range(0, 900, 10):
        _, otv, _ = rc.simulate(circuits[k], observables[k], noise)
        tb = rc.term_bound(circuits[k], noise)
        assert tb < rc.CAP and np.abs(got[k] - otv).max() <= tb and abs(norm[k] - 1.0) <= tb, k
    today = run_plain(sim.compile_programs(texts, observables, sim.NoiseModel.from_backend(lima_backend, readout=False)))[1].reshape(900, 4)
    sig0 = sc.anchor_sigmas(today, noisy)
    print(f"noisy anchor (depolarising model, device): {(sig0 > 4).sum()} values beyond 4 sigma, max {sig0.max():.2f} sigma")
    assert sig0.max() > 4.0 and (sig0 > 4.0).sum() > 50
