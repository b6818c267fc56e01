"""Zero-noise extrapolation at width on the device (mlqem_clifford_run_folded_f64, mlqem_zne_combine_exp_f64, the Clifford path of
blackwater.zne) against tests/clifford_zne_cases.py: the folded interpreter to the last bit, the density-matrix and block oracles on
explicitly folded circuits within the derived bounds, the closed form ideal * F1 * F2^x and its exponential fit, and the public
interface on top."""
import numpy as np
import pytest
import torch

import clifford_cases as cc
import clifford_zne_cases as czc
import sim_cases as sc
import zne_cases as zc
from blackwater import sim, zne
from blackwater.native import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("ideal_values", "noisy_values", "ideal_terms", "noisy_terms", "unit_ideal", "unit_noisy")


def host(t):
    return t.cpu().numpy()


def args_of(t, s, n_factors):
    return (t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"], t["term_ptr"], t["coeff"],
            t["comb_ptr"], t["comb_unit"], t["comb_weight"], s["sched_ptr"], s["sched"], n_factors)


def run_and_compare(batch, sch):
    """One call; all six outputs must equal the folded interpreter bit for bit, at every factor."""
    got = [host(x) for x in sim.run_clifford_folded(batch, sch, DEV)]
    want = czc.interpret_folded(batch, sch)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and np.array_equal(g, w), name
    return got


@pytest.fixture(scope="module")
def mixed():
    circuits, obs, noise = czc.mixed_batch()
    return {"circuits": circuits, "obs": obs, "noise": noise, "batch": sim.compile_clifford(circuits, obs, noise)}


# ---- 1. the folded interpreter, to the last bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(czc.AMPLIFIERS))
def test_device_equals_the_folded_interpreter(mixed, name):
    batch = mixed["batch"]
    sch = zne.build_clifford_schedules(batch, zc.PARTIAL, zc.make_amplifier(czc.AMPLIFIERS[name]))
    assert batch.n_reg > 0 and batch.n_lds > 0 and (sch.sched & 1).any()
    got = run_and_compare(batch, sch)
    # every factor changes some term; the few two-qubit gates of these circuits fold alike at 1 and 1.5, and at 2.2 and 3
    assert len(np.unique(got[3], axis=0)) == (2 if name == "local-2q" else len(zc.PARTIAL))


# ---- 6. the ideal outputs do not depend on the factor ----------------------------------------------------------------------------------------
def test_ideal_outputs_are_equal_across_factors_and_equal_the_plain_run(mixed):
    batch = mixed["batch"]
    plain = [host(x) for x in sim.run_clifford(batch, DEV)]
    for name in ("global", "local-random"):
        sch = zne.build_clifford_schedules(batch, zc.PARTIAL, zc.make_amplifier(czc.AMPLIFIERS[name]))
        got = [host(x) for x in sim.run_clifford_folded(batch, sch, DEV)]
        for k in (0, 2, 4):
            for f in range(len(zc.PARTIAL)):
                assert np.array_equal(got[k][f], plain[k]), (name, NAMES[k], f)
        for k in (1, 3, 5):   # factor 1 is the circuit as lowered
            assert np.array_equal(got[k][0], plain[k]), (name, NAMES[k])
    assert np.count_nonzero(plain[2]) >= len(plain[2]) // 4


# ---- 2. the density-matrix oracle on explicitly folded circuits ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", czc.SMALL, ids=lambda c: c[0])
def test_small_circuits_against_the_folded_density_matrix_oracle(case):
    _, n, desc = case
    k = czc.small_case(n, desc)
    ora, terms = k["oracle"], k["terms"]
    strategy = zne.ZNEStrategy(zc.PARTIAL, zc.make_amplifier(desc), zne.LinearExtrapolator())
    run = zne.zne_run([k["circuit"]], [terms], k["noise"], strategy, DEV, method="clifford")
    assert run.norm is None and isinstance(run.batch, sim.CliffordBatch) and run.fallback_terms is None
    tv, v = host(run.term_values), host(run.values)
    assert k["term_bounds"].max() < czc.CAP and k["mitigated_value_bound"] < czc.CAP
    assert (np.abs(tv - ora["term_values"]) <= k["term_bounds"]).all()
    assert (np.abs(v[:, 0] - ora["values"]) <= k["value_bounds"]).all()
    assert (np.abs(host(run.mitigated_terms) - ora["mitigated_terms"]) <= k["mitigated_term_bound"]).all()
    assert abs(host(run.mitigated_values)[0] - ora["mitigated_value"]) <= k["mitigated_value_bound"]
    assert np.array_equal(run.schedules.achieved[:, 0], ora["achieved"])
    assert np.array_equal(host(run.ideal_terms), cc.tableau_values(k["circuit"], [label for label, _ in terms]))


# ---- 3. the block oracle at width ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("global", "local-all"))
@pytest.mark.parametrize("n", sorted(cc.BLOCKS))
def test_wide_circuits_against_the_folded_block_oracle(n, name):
    desc = czc.AMPLIFIERS[name]
    k = czc.block_case(n, desc)
    strategy = zne.ZNEStrategy(czc.ODD, zc.make_amplifier(desc), zne.LinearExtrapolator())
    run = zne.zne_run([k["blocks"].wide], [k["terms"]], k["noise"], strategy, DEV, method="clifford")
    tv = host(run.term_values)
    assert k["bounds"].max() < czc.CAP and (np.abs(tv - k["values"]) <= k["bounds"]).all()
    assert np.array_equal(host(run.ideal_terms), cc.tableau_values(k["blocks"].wide, [label for label, _ in k["terms"]]))
    assert np.array_equal(run.schedules.achieved[:, 0], np.asarray(czc.ODD, dtype=np.float64))


# ---- 4. the closed form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in czc.CLOSED if c[1] in (100, 512)], ids=lambda c: c[0])
def test_closed_form_and_exponential_fit_on_the_device(case):
    _, n, desc = case
    k = czc.closed_case(n, desc)
    got = run_and_compare(k["batch"], k["sch"])
    assert all(np.array_equal(got[4][f], k["ideal"]) for f in range(len(czc.ODD)))
    assert (np.abs(got[5] - k["ref"]) <= k["bounds"]).all()
    strategy = zne.ZNEStrategy(czc.ODD, zc.make_amplifier(desc), zne.ExponentialExtrapolator())
    run = zne.zne_run([k["circuit"]], [k["terms"]], k["noise"], strategy, DEV, method="clifford")
    order = k["batch"].comb_unit
    terms, values = host(run.mitigated_terms), host(run.mitigated_values)
    assert k["fit_bound"].max() < czc.CAP and not host(run.fallback_terms).any()
    assert (np.abs(terms - k["fit_ref"][order]) <= k["fit_bound"][order]).all()
    if desc in (zc.GLOBAL, zc.LOCAL_ALL):   # everything is folded: the fit recovers the ideal value itself
        assert (np.abs(terms - host(run.ideal_terms)) <= k["fit_bound"][order]).all()
    coeff = k["batch"].coeff
    vb = (np.abs(coeff) * k["fit_bound"][order]).sum() + (len(coeff) + 1) * czc.U * np.abs(coeff * k["fit_ref"][order]).sum()
    assert abs(values[0] - float((coeff * k["fit_ref"][order]).sum())) <= vb
    # the host form of the same fit agrees within both sides' bounds, and a straight line does not get there
    _, twin, _ = zne.ExponentialExtrapolator().extrapolate_terms(czc.ODD, got[3], k["batch"].term_ptr, coeff)
    assert (np.abs(terms - twin) <= czc.fit_agreement_bound(k["weights"], got[3])).all()
    line = zne.zne_run([k["circuit"]], [k["terms"]], k["noise"], zne.ZNEStrategy(czc.ODD, zc.make_amplifier(desc)), DEV, method="clifford")
    assert np.abs(host(line.mitigated_terms) - k["fit_ref"][order]).max() > 1e3 * k["fit_bound"].max()


def test_exponential_combine_cases_on_the_device():
    """All-zero terms, mixed signs, a zero among nonzeros, a negative term: values and flags, against the host form."""
    f = (1, 3, 5)
    tv = np.array([[0.5, -0.5, 0.0, 0.4, 0.3, 0.0, 0.9], [0.25, -0.25, 0.0, -0.2, 0.0, 0.1, 0.7], [0.125, -0.125, 0.0, 0.1, 0.2, 0.0, 0.5]])
    ptr, coeff = np.array([0, 3, 3, 7]), np.array([1.0, 2.0, 3.0, 1.0, -1.0, 0.5, 0.25])
    ex = zne.ExponentialExtrapolator()
    want_v, want_t, want_f = ex.extrapolate_terms(f, tv, ptr, coeff)
    w = torch.from_numpy(ex.weights(f)).to(DEV)
    values, terms, flags = ops.zne_combine_exp(torch.from_numpy(tv).to(DEV), w, torch.from_numpy(ptr).to(DEV), torch.from_numpy(coeff).to(DEV))
    assert host(flags).tolist() == want_f.tolist() == [0, 0, 0, 1, 1, 1, 0] and flags.dtype == torch.int32
    terms, values = host(terms), host(values)
    agree = czc.fit_agreement_bound(ex.weights(f), tv)   # exact inputs: only log, exp and the sums differ between the two
    assert (np.abs(terms - want_t) <= agree).all() and agree.max() < 1e-14
    assert terms[1] == -terms[0] and terms[2] == 0.0 and values[1] == 0.0
    lin_v, lin_t = ops.zne_combine(torch.from_numpy(tv).to(DEV), w, torch.from_numpy(ptr).to(DEV), torch.from_numpy(coeff).to(DEV))
    assert np.array_equal(terms[3:6], host(lin_t)[3:6])   # the fallback is mlqem_zne_combine_f64's sum, bit for bit
    assert (np.abs(values - want_v) <= czc.value_agreement_bound(coeff, want_t, agree, ptr)).all()
    # on the state-vector simulator's folded runs too
    circ, obs = cc.random_clifford_program(4, 10, 3), cc.random_terms(4, 5, 3)
    strategy = zne.ZNEStrategy(f, zne.GlobalFoldingAmplifier(), ex)
    run = zne.zne_run([circ], [obs], sc.StepNoise(4, force=False), strategy, DEV)
    _, twin, flags = ex.extrapolate_terms(f, host(run.term_values), host(run.term_ptr), run.batch.coeff)
    assert host(run.fallback_terms).tolist() == flags.tolist()
    assert (np.abs(host(run.mitigated_terms) - twin) <= czc.fit_agreement_bound(ex.weights(f), host(run.term_values))).all()


# ---- 5. the same bits alone, in any batch, in a replayed graph -----------------------------------------------------------------------------
def test_a_circuit_is_bit_equal_alone_in_any_batch_and_in_a_replayed_graph(mixed):
    circuits, obs, noise, batch = mixed["circuits"], mixed["obs"], mixed["noise"], mixed["batch"]
    amp = zc.make_amplifier(zc.LOCAL_RANDOM)
    strategy = zne.ZNEStrategy(zc.PARTIAL, amp, zne.ExponentialExtrapolator())
    whole = zne.zne_run(circuits, obs, noise, strategy, DEV, method="clifford")
    tp = batch.term_ptr
    w_tv, w_v, w_mt, w_mv = (host(x) for x in (whole.term_values, whole.values, whole.mitigated_terms, whole.mitigated_values))
    pick = [3, 4, 6, 8, 14]   # widths 33, 100, 129, 512 and a 100-qubit circuit of 40 records: both instantiations
    for k in pick:
        alone = zne.zne_run([circuits[k]], [obs[k]], noise, strategy, DEV, method="clifford")
        assert np.array_equal(host(alone.term_values), w_tv[:, tp[k]:tp[k + 1]]) and np.array_equal(host(alone.values)[:, 0], w_v[:, k])
        assert np.array_equal(host(alone.mitigated_terms), w_mt[tp[k]:tp[k + 1]]) and host(alone.mitigated_values)[0] == w_mv[k]
    order = [14, 8, 8, 3, 22, 6, 4]
    again = zne.zne_run([circuits[k] for k in order], [obs[k] for k in order], noise, strategy, DEV, method="clifford")
    a_tv, a_mv, ap = host(again.term_values), host(again.mitigated_values), again.batch.term_ptr
    for j, k in enumerate(order):
        assert np.array_equal(a_tv[:, ap[j]:ap[j + 1]], w_tv[:, tp[k]:tp[k + 1]]) and a_mv[j] == w_mv[k]
    # run + combine captured on one stream (no parallel branches), replayed twice
    sch = whole.schedules
    t, s = batch.to(DEV), sch.to(DEV)
    n_f = len(zc.PARTIAL)
    want = [host(x) for x in sim.run_clifford_folded(batch, sch, DEV)]
    outs = {name: torch.zeros_like(torch.from_numpy(g)).to(DEV) for name, g in zip(NAMES, want)}
    mt, mv = torch.zeros(len(batch.coeff), dtype=torch.float64, device=DEV), torch.zeros(len(batch), dtype=torch.float64, device=DEV)
    fb = torch.zeros(len(batch.coeff), dtype=torch.int32, device=DEV)
    w = torch.from_numpy(whole.weights).to(DEV)

    def both():
        ops.clifford_run_folded(*args_of(t, s, n_f), **outs)
        ops.zne_combine_exp(outs["noisy_terms"], w, t["term_ptr"], t["coeff"], mitigated_terms=mt, mitigated_values=mv, fallback=fb)

    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        both()   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for _ in range(2):
        for o in list(outs.values()) + [mt, mv]:
            o.fill_(7.0)
        fb.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for name, g in zip(NAMES, want):
            assert np.array_equal(host(outs[name]), g), name
        assert np.array_equal(host(mt), w_mt) and np.array_equal(host(mv), w_mv) and np.array_equal(host(fb), host(whole.fallback_terms))


# ---- 7. bad arguments are refused before any launch ----------------------------------------------------------------------------------------
def test_the_new_ops_check_their_arguments(mixed):
    batch = mixed["batch"]
    sch = zne.build_clifford_schedules(batch, (1, 3), zne.GlobalFoldingAmplifier())
    t, s = batch.to(DEV), sch.to(DEV)
    a = list(args_of(t, s, 2))
    with pytest.raises(ValueError, match="n_factors = 0"):
        ops.clifford_run_folded(*a[:15], 0)
    with pytest.raises(ValueError, match="sched_ptr"):
        ops.clifford_run_folded(*a[:15], 3)
    with pytest.raises(ValueError, match="sched_ptr"):
        ops.clifford_run_folded(*a[:13], a[13].to(torch.int32), a[14], 2)
    with pytest.raises(ValueError, match="sched"):
        ops.clifford_run_folded(*a[:14], a[14].to(torch.int64), 2)
    with pytest.raises(ValueError, match="add up to"):
        ops.clifford_run_folded(*a[:5], a[5] + 1, *a[6:])
    with pytest.raises(ValueError, match="unit_noisy"):
        ops.clifford_run_folded(*a, unit_noisy=torch.zeros(len(batch.units), dtype=torch.float64, device=DEV))
    tv = torch.zeros(2, len(batch.coeff), dtype=torch.float64, device=DEV)
    w = torch.zeros(2, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="F >= 2"):
        ops.zne_combine_exp(tv[:1].contiguous(), w[:1], t["term_ptr"], t["coeff"])
    with pytest.raises(ValueError, match="F >= 2"):
        ops.zne_combine_exp(tv.to(torch.float32), w, t["term_ptr"], t["coeff"])
    with pytest.raises(ValueError, match="weights"):
        ops.zne_combine_exp(tv, torch.zeros(3, dtype=torch.float64, device=DEV)[:1], t["term_ptr"], t["coeff"])
    with pytest.raises(ValueError, match="fallback"):
        ops.zne_combine_exp(tv, w, t["term_ptr"], t["coeff"], fallback=torch.zeros(len(batch.coeff), dtype=torch.int64, device=DEV))
    empty = sim.compile_clifford([], [])
    es = zne.build_clifford_schedules(empty, (1, 3), zne.GlobalFoldingAmplifier())
    assert all(x.numel() == 0 for x in sim.run_clifford_folded(empty, es, DEV))


# ---- 8. the public interface ---------------------------------------------------------------------------------------------------------------
def test_zne_device_estimator_on_100_qubit_circuits():
    from blackwater.data.backends import PauliObservable
    from blackwater.data.synthetic import clifford_tfim_circuit, synthetic_backend
    from blackwater.library.learning.estimator import ZNEProcessor

    noise = sim.NoiseModel.from_backend(synthetic_backend(100, "ecr"), readout=False)
    circuits = [clifford_tfim_circuit(100, 1 + k % 2, k % 4, (k // 4) % 4) for k in range(8)]
    z = lambda q: "".join("Z" if j == q else "I" for j in reversed(range(100)))
    obs = [PauliObservable(z(k)) if k % 2 else PauliObservable([(z(k), 0.5), (z(99 - k), -2.0)]) for k in range(8)]
    strategy = zne.ZNEStrategy((1, 3, 5), zne.LocalFoldingAmplifier(gates_to_fold=2), zne.ExponentialExtrapolator())
    est = zne.zne(sim.DeviceEstimator)(noise, DEV, method="clifford", zne_strategy=strategy)
    res = est.run(circuits, obs).result()          # on the parent commit: the exact simulator's cap, a ValueError
    run = zne.zne_run(circuits, [o.to_list() for o in obs], noise, strategy, DEV, method="clifford")
    assert np.array_equal(res.values, host(run.mitigated_values)) and isinstance(run.batch, sim.CliffordBatch) and run.norm is None
    per_factor, flags, tp = host(run.values), host(run.fallback_terms), host(run.term_ptr)
    for k, meta in enumerate(res.metadata):
        assert meta["zne"]["noise_factors"] == (1.0, 3.0, 5.0) and meta["zne"]["achieved_factors"] == (1.0, 3.0, 5.0)
        assert meta["zne"]["values"] == tuple(per_factor[:, k].tolist()) and meta["zne"]["extrapolator"] == "ExponentialExtrapolator()"
        assert meta["zne"]["fallback_terms"] == int(flags[tp[k]:tp[k + 1]].sum())
    # the per-factor values are the interpreter's, and the ideal values come with them
    want = czc.interpret_folded(run.batch, run.schedules)
    assert np.array_equal(per_factor, want[1]) and np.array_equal(host(run.ideal_values), want[0][0])
    # the default strategy (factors (1, 3), two-qubit folding, a straight line) carries no fallback count
    plain = zne.zne(sim.DeviceEstimator)(noise, DEV, method="clifford").run(circuits, obs).result()
    assert "fallback_terms" not in plain.metadata[0]["zne"] and plain.metadata[0]["zne"]["noise_factors"] == (1.0, 3.0)
    values = zne.zne_expectation_values(circuits, [o.to_list() for o in obs], noise, None, DEV, method="clifford")[0]
    assert np.array_equal(plain.values, host(values))
    # auto: a wide Clifford job goes here, a 4-qubit job to the exact simulator
    auto = zne.zne(sim.DeviceEstimator)(noise, DEV, method="auto", zne_strategy=strategy)
    assert np.array_equal(auto.run(circuits, obs).result().values, res.values)
    small = [cc.random_clifford_program(4, 12, k) for k in range(3)]
    step = sc.StepNoise(2)
    exact = zne.zne(sim.DeviceEstimator)(step, DEV).run(small, ["ZZIZ"] * 3).result().values
    assert np.array_equal(zne.zne(sim.DeviceEstimator)(step, DEV, method="auto").run(small, ["ZZIZ"] * 3).result().values, exact)
    assert isinstance(zne.zne_run(small, ["ZZIZ"] * 3, step, None, DEV, method="auto").batch, sim.SimBatch)
    with pytest.raises(ValueError, match="amplitudes|qubits"):
        zne.zne(sim.DeviceEstimator)(noise, DEV).run(circuits, obs)   # the default is the exact simulator and its cap, as ever
    with pytest.raises(ValueError, match="shots are not drawn on the Clifford path"):
        est.run(circuits, obs, shots=100)
    # ZNEProcessor works unchanged over such an estimator
    proc = ZNEProcessor(est, strategy)
    assert proc.process_batch([0.0] * 8, circuits, obs, None) == res.values.tolist()
    assert proc.process(0.0, circuits[3], obs[3], None) == res.values[3]


# ---- 9. quality (recorded; asserted only where the CPU twin's ratio reaches 1.5) --------------------------------------------------------------
# The CPU twin: the host interpreter (clifford_zne_cases.interpret_folded) on the whole corpus and the numpy extrapolators, mean
# |noisy - ideal| / mean |mitigated - ideal| over the 256 terms.  Filled in from that run; see DESIGN.md section 3.11.
TWIN = {(False, "default"): 1.2353, (False, "exponential"): 7.4e14, (True, "default"): 1.1632, (True, "exponential"): 3.8666}


@pytest.mark.parametrize("readout", (False, True), ids=("depolarising", "with-readout"))
def test_mitigation_quality_on_the_tfim_corpus_is_recorded(readout):
    """64 100-qubit ``clifford_tfim_circuit`` circuits, four single-Z terms each, the ``synthetic_backend`` model: mean |noisy - ideal|
    against mean |mitigated - ideal| for the default strategy (factors (1, 3), two-qubit local folding, a straight line) and for
    ``ExponentialExtrapolator`` at (1, 3, 5) with every gate folded.  Two circuits are held to the interpreter bit for bit at every
    factor (the interpreter takes seconds on all 64; a circuit's bits do not depend on the batch), and the device's fit to numpy's
    on the device's own per-factor values."""
    from blackwater.data.synthetic import synthetic_backend

    circuits, obs, _, _, _ = cc.quality_corpus()
    noise = sim.NoiseModel.from_backend(synthetic_backend(100, "ecr"), readout=readout)
    strategies = {"default": zne.ZNEStrategy(),
                  "exponential": zne.ZNEStrategy((1, 3, 5), zne.LocalFoldingAmplifier(), zne.ExponentialExtrapolator())}
    for name, strategy in strategies.items():
        run = zne.zne_run(circuits, obs, noise, strategy, DEV, method="clifford")
        ideal, tv, mit = host(run.ideal_terms), host(run.term_values), host(run.mitigated_terms)
        for k in (0, 42):
            alone = sim.compile_clifford([circuits[k]], [obs[k]], noise)
            sch = zne.build_clifford_schedules(alone, strategy.noise_factors, strategy.noise_amplifier)
            want = czc.interpret_folded(alone, sch)
            assert np.array_equal(tv[:, 4 * k:4 * k + 4], want[3]) and np.array_equal(ideal[4 * k:4 * k + 4], want[2][0])
        twin = strategy.extrapolator.extrapolate(strategy.noise_factors, tv)
        if name == "exponential":
            assert (np.abs(mit - twin) <= czc.fit_agreement_bound(strategy.weights(), tv)).all()
        else:
            assert (np.abs(mit - twin) <= 2 * (len(tv) + 1) * czc.U * (np.abs(strategy.weights())[:, None] * np.abs(tv)).sum(axis=0)).all()
        unmit, left = float(np.mean(np.abs(tv[0] - ideal))), float(np.mean(np.abs(mit - ideal)))
        ratio = unmit / left if left > 0 else float("inf")
        print(f"ZNE at width, 100-qubit TFIM, readout={readout}, {name}: mean |noisy - ideal| {unmit:.6e}, mean |mitigated - ideal| "
              f"{left:.6e}, ratio {ratio:.4g}; CPU twin {TWIN.get((readout, name))}")
        assert np.isfinite(unmit) and np.isfinite(left)
        if TWIN.get((readout, name), 0.0) >= 1.5:
            assert ratio > 1.0, (name, readout, ratio)
