"""The Clifford path on the device (mlqem_clifford_run_f64, blackwater.sim.clifford) against tests/clifford_cases.py: the host
interpreter of the record format to the last bit, the stabilizer tableau exactly, the density-matrix and block oracles within the
derived bound, and the public interface on top."""
import numpy as np
import pytest
import torch

import clifford_cases as cc
import sim_cases as sc
from blackwater import sim
from blackwater.data.circuit import Circuit, CircuitOp
from blackwater.native import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BLOCKS = cc.BLOCKS
NAMES = ("ideal_values", "noisy_values", "ideal_terms", "noisy_terms", "unit_ideal", "unit_noisy")


def host(t):
    return t.cpu().numpy()


def args_of(t):
    return (t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"], t["term_ptr"], t["coeff"],
            t["comb_ptr"], t["comb_unit"], t["comb_weight"])


def run_and_compare(circuits, observables, noise=None):
    """One call; every output must equal the host interpreter bit for bit.  Returns ``(batch, outputs as numpy arrays)``."""
    batch = sim.compile_clifford(circuits, observables, noise)
    got = [host(x) for x in sim.run_clifford(batch, DEV)]
    want = cc.interpret(batch)
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and np.array_equal(g, w), name
    return batch, got


def terms_of(circ, n, count, seed):
    """``count`` terms: stabilizer products (value +-1) and random low-weight labels, among them terms with 1, 2 and 3 Y."""
    half = count // 2
    terms = cc.stabilizer_terms(circ, count - half, seed) + cc.random_terms(n, half, seed, weight=3)
    shrink = max(1.0, count / 12.0)   # sum |coeff| <= 3 whatever the count, as in sim_cases: the value bounds stay under the cap
    return [(label, c / shrink) for label, c in terms[:count]]


# ---- widths, term counts, both instantiations ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid():
    """One circuit per width with a depolarising op after every gate (lambda = 0 and lambda = 1 forced), lowered and run ONCE."""
    widths = [1, 2, 5, 31, 32, 33, 64, 65, 100, 128, 129, 512]
    counts = [0, 1, 63, 64, 65, 300, 12, 12, 12, 12, 12, 12]
    circuits = [cc.random_clifford_program(n, 3 * n + 12, n, measure=True, local=5) for n in widths]
    obs = [terms_of(c, n, k, n) for c, n, k in zip(circuits, widths, counts)]
    circuits.append(Circuit(40, 0, []))   # a circuit with no ops
    obs.append([("I" * 39 + "Z", 0.5), ("I" * 39 + "X", 1.0), ("I" * 40, -1.0)])
    noise = sc.StepNoise(3)
    batch, got = run_and_compare(circuits, obs, noise)
    return {"widths": widths, "circuits": circuits, "obs": obs, "noise": noise, "batch": batch, "got": got}


def test_device_equals_the_interpreter_on_the_grid(grid):
    batch = grid["batch"]
    assert batch.n_reg > 0 and batch.n_lds > 0   # both instantiations ran in this one call, waves straddle circuits
    assert np.diff(batch.term_ptr).tolist() == [0, 1, 63, 64, 65, 300, 12, 12, 12, 12, 12, 12, 3]
    values = grid["got"][0]
    assert values[0] == 0.0 and values[12] == 0.5 * 1.0 + 1.0 * 0.0 - 1.0   # no terms; no ops: <Z> = 1, <X> = 0, <I> = 1


def test_ideal_values_equal_the_tableau_exactly(grid):
    ti = grid["got"][2]
    for k, (circ, terms) in enumerate(zip(grid["circuits"], grid["obs"])):
        b, e = int(grid["batch"].term_ptr[k]), int(grid["batch"].term_ptr[k + 1])
        want = cc.tableau_values(circ, [label for label, _ in terms])
        assert np.array_equal(ti[b:e], want) and set(np.unique(want)) <= {-1.0, 0.0, 1.0}, k
        assert e - b < 2 or np.count_nonzero(want) >= (e - b) // 2
    ys = {label.count("Y") for terms in grid["obs"] for label, _ in terms}
    assert {1, 2, 3} <= ys


def test_noisy_values_against_the_density_matrix_oracle(grid):
    """Oracle (b) for the widths it reaches, and the exact simulator on the device: the same circuits, noise and bound."""
    small = [k for k, n in enumerate(grid["widths"]) if n <= 5]
    circuits, obs = [grid["circuits"][k] for k in small], [grid["obs"][k] for k in small]
    dev_values, dev_terms, _ = sim.expectation_values(circuits, obs, grid["noise"], DEV)
    dev_values, dev_terms = host(dev_values), host(dev_terms)
    at = 0
    for j, k in enumerate(small):
        circ, terms = circuits[j], obs[j]
        b, e = int(grid["batch"].term_ptr[k]), int(grid["batch"].term_ptr[k + 1])
        v1, t1, _ = sc.simulate(circ, terms, grid["noise"])
        tb = sc.term_bound(circ, grid["noise"])
        for i in range(e - b):
            got = grid["got"][3][b + i]
            bound = cc.noisy_bound(grid["batch"], k, t1[i], tb)
            assert bound < sc.CAP and abs(got - t1[i]) <= bound and abs(got - dev_terms[at + i]) <= bound, (k, i)
        vb = sc.value_bound(circ, terms, grid["noise"]) + (cc.depol_count(grid["batch"], k) + 2) * sc.U * sum(abs(c) for _, c in terms)
        assert vb < sc.CAP and abs(grid["got"][1][k] - v1) <= vb and abs(grid["got"][1][k] - dev_values[j]) <= vb
        at += e - b
    assert np.count_nonzero(np.abs(grid["got"][3]) * (1 - np.abs(grid["got"][3])) > 0) > 50   # the noise shows


@pytest.mark.parametrize("n", sorted(BLOCKS))
def test_noisy_values_against_the_block_oracle(n):
    """Oracle (d): noise at width, blocks across the words 31|32, 63|64, 127|128, 255|256 and the register's ends."""
    blocks = cc.BlockCircuit(n, BLOCKS[n], 10, n)
    noise = sc.StepNoise(n)
    terms = blocks.stabilizer_terms(24, n) + blocks.random_terms(8, n)
    batch, got = run_and_compare([blocks.wide], [terms], noise)
    want, oracle_bound = blocks.term_values(terms, noise)
    assert np.array_equal(got[2], cc.tableau_values(blocks.wide, [label for label, _ in terms]))
    for j in range(len(terms)):
        bound = cc.noisy_bound(batch, 0, want[j], oracle_bound[j])
        assert bound < sc.CAP and abs(got[3][j] - want[j]) <= bound, j
    assert np.count_nonzero((np.abs(got[3]) > 0) & (np.abs(got[3]) < 1)) >= 12


def test_lambda_zero_lambda_one_and_id_with_noise():
    class Fixed(sc.NoNoise):
        def __init__(self, lam):
            self.lam = lam

        def after_gate(self, index, name, qubits):
            return self.lam

    ops_ = [CircuitOp("h", (0,)), CircuitOp("id", (1,)), CircuitOp("cx", (0, 2)), CircuitOp("id", (0,)), CircuitOp("id", (3,))]
    circ = Circuit(4, 0, ops_)
    obs = [("IXIX", 1.0), ("IIZI", 1.0), ("ZIII", 1.0), ("IIIZ", 1.0)]
    for lam, want in ((0.0, [1.0, 1.0, 1.0, 0.0]), (1.0, [0.0, 0.0, 0.0, 0.0]), (0.25, [0.75 ** 3, 0.75, 0.75, 0.0])):
        batch, got = run_and_compare([circ], [obs], Fixed(lam))
        assert got[2].tolist() == [1.0, 1.0, 1.0, 0.0] and got[3].tolist() == want, lam
        assert (batch.ops[:, 0] & 15).tolist() == [0, 2, 2, 1, 3, 2, 2]   # id: no gate record, its noise record stays
        t = sc.simulate(circ, obs, Fixed(lam))[1]
        assert np.abs(got[3] - t).max() <= sc.term_bound(circ, Fixed(lam))


def test_readout_on_the_device():
    blocks = cc.BlockCircuit(100, BLOCKS[100], 8, 4, names=cc.CLASSICAL)
    noise = sc.StepNoise(6, readout={q: (0.05 + 0.01 * (q % 4), 0.01 * (q % 3)) for q in range(100)})
    terms = blocks.stabilizer_terms(20, 2)
    batch, got = run_and_compare([blocks.wide], [terms], noise)
    want, oracle_bound = blocks.term_values(terms, noise)
    assert len(batch.units) > 4 * len(terms) and (np.abs(got[2]) == 1.0).all()
    for j, (label, _) in enumerate(terms):
        m = label.count("Z")   # 2^m addends of magnitude <= 1, each within (K + m + 2) u, and as many rounded additions
        bound = 2 ** m * cc.noisy_bound(batch, 0, 1.0, 0.0, readout_factors=m) + oracle_bound[j]
        assert bound < sc.CAP and abs(got[3][j] - want[j]) <= bound, j


# ---- the same bits alone, in any batch, in a replayed graph -------------------------------------------------------------------------------
def test_a_circuit_is_bit_equal_alone_in_any_batch_and_in_a_replayed_graph(grid):
    noise, circuits, obs = grid["noise"], grid["circuits"], grid["obs"]
    pick = [5, 8, 10, 11]   # widths 33, 100, 129, 512: both instantiations
    tp = grid["batch"].term_ptr
    for k in pick:
        alone = [host(x) for x in sim.run_clifford(sim.compile_clifford([circuits[k]], [obs[k]], noise), DEV)]
        assert alone[0][0] == grid["got"][0][k] and alone[1][0] == grid["got"][1][k]
        assert np.array_equal(alone[2], grid["got"][2][tp[k]:tp[k + 1]]) and np.array_equal(alone[3], grid["got"][3][tp[k]:tp[k + 1]])
    for order in ([11, 5, 10, 8], [8, 8, 11, 10, 5, 0, 12]):
        batch = sim.compile_clifford([circuits[k] for k in order], [obs[k] for k in order], noise)
        out = [host(x) for x in sim.run_clifford(batch, DEV)]
        for j, k in enumerate(order):
            assert out[0][j] == grid["got"][0][k] and out[1][j] == grid["got"][1][k]
            b, e = int(batch.term_ptr[j]), int(batch.term_ptr[j + 1])
            assert np.array_equal(out[3][b:e], grid["got"][3][tp[k]:tp[k + 1]]) and np.array_equal(out[2][b:e], grid["got"][2][tp[k]:tp[k + 1]])
    # the whole grid in a captured graph, replayed twice
    t = grid["batch"].to(DEV)
    outs = {name: torch.zeros_like(torch.from_numpy(g)).to(DEV) for name, g in zip(NAMES, grid["got"])}
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        ops.clifford_run(*args_of(t), **outs)   # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.clifford_run(*args_of(t), **outs)
    for _ in range(2):
        for o in outs.values():
            o.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for name, g in zip(NAMES, grid["got"]):
            assert np.array_equal(host(outs[name]), g), name


def test_ops_checks_its_arguments(grid):
    t = grid["batch"].to(DEV)
    a = list(args_of(t))
    with pytest.raises(ValueError, match="add up to"):
        ops.clifford_run(*a[:5], a[5] + 1, *a[6:])
    with pytest.raises(ValueError, match="unit_noisy"):
        ops.clifford_run(*a, unit_noisy=torch.zeros(3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="comb_weight"):
        ops.clifford_run(*a[:12], a[12].reshape(-1))
    empty = sim.compile_clifford([], [])
    assert all(x.numel() == 0 for x in sim.run_clifford(empty, DEV))


# ---- the public interface ----------------------------------------------------------------------------------------------------------------
def test_clifford_expectation_values(grid):
    circuits, obs, noise = grid["circuits"][6:9], grid["obs"][6:9], grid["noise"]
    tp = grid["batch"].term_ptr
    values, terms, term_ptr = sim.clifford_expectation_values(circuits, obs, None, DEV)
    assert np.array_equal(host(values), grid["got"][0][6:9]) and np.array_equal(host(terms), grid["got"][2][tp[6]:tp[9]])
    assert host(term_ptr).tolist() == [0, 12, 24, 36] and values.dtype == torch.float64
    noisy, nterms, _, ideal, iterms = sim.clifford_expectation_values(circuits, obs, noise, DEV, return_ideal=True)
    assert np.array_equal(host(noisy), grid["got"][1][6:9]) and np.array_equal(host(nterms), grid["got"][3][tp[6]:tp[9]])
    assert np.array_equal(host(ideal), host(values)) and np.array_equal(host(iterms), host(terms))


def test_device_estimator_clifford_under_the_learning_decorator():
    """100-qubit circuits through ``DeviceEstimator(method="clifford")``, plain and under the unchanged ``learning(...)``."""
    from blackwater.data.backends import PauliObservable
    from blackwater.data.synthetic import clifford_tfim_circuit, synthetic_backend
    from blackwater.data.utils import encode_pauli_sum_op, get_backend_properties_v1
    from blackwater.library.learning.estimator import LinearLearningModelProcessor, learning
    from blackwater.library.learning.features import encode_data
    from blackwater.nn import LinearRegressor

    backend = synthetic_backend(100, "ecr")
    noise = sim.NoiseModel.from_backend(backend, readout=False)
    circuits = [clifford_tfim_circuit(100, 1 + k % 2, k % 4, (k // 4) % 4) for k in range(16)]
    z = lambda q: "".join("Z" if j == q else "I" for j in reversed(range(100)))
    obs = [PauliObservable(z(k)) if k % 2 else PauliObservable([(z(k), 0.5), (z(99 - k), -2.0)]) for k in range(16)]
    want = cc.interpret(sim.compile_clifford(circuits, [o.to_list() for o in obs], noise))[1]
    for method in ("clifford", "auto"):
        job = sim.DeviceEstimator(noise, DEV, method=method).run(circuits, obs)
        assert job.status() == "DONE" and np.array_equal(job.result().values, want) and job.result().metadata == [{}] * 16
    with pytest.raises(ValueError, match="amplitudes"):
        sim.DeviceEstimator(noise, DEV).run(circuits, obs)   # the default is the exact simulator and its cap, as ever
    small = [cc.random_clifford_program(4, 12, k) for k in range(3)]
    step = sc.StepNoise(2)   # auto on circuits inside the cap is the exact simulator, bit for bit
    exact = sim.DeviceEstimator(step, DEV).run(small, ["ZZIZ"] * 3).result().values
    assert np.array_equal(sim.DeviceEstimator(step, DEV, method="auto").run(small, ["ZZIZ"] * 3).result().values, exact)

    props = get_backend_properties_v1(backend)
    single = [z(7)] * 16
    ideal = sim.clifford_expectation_values(circuits, single, None, DEV)[0]
    noisy = host(sim.clifford_expectation_values(circuits, single, noise, DEV)[0])
    rows = torch.cat([encode_data(circuits=[c], properties=props, ideal_exp_vals=[[0.0]], noisy_exp_vals=[[float(v)]], num_qubits=1,
                                  meas_bases=encode_pauli_sum_op([(z(7), 1.0)]))[0] for c, v in zip(circuits, noisy)])
    model = LinearRegressor.fit(rows.to(DEV, dtype=torch.float32), ideal.to(torch.float32), alpha=1e-3)
    mitigated = learning(sim.DeviceEstimator, LinearLearningModelProcessor(model, backend, device=DEV), skip_transpile=True)
    out = mitigated(noise, DEV, method="clifford").run(circuits, obs).result()
    assert out.values.shape == (16,) and np.isfinite(out.values).all()
    assert [m["original_value"] for m in out.metadata] == want.tolist()


def test_encode_corpus_with_clifford_labels():
    from blackwater.data.synthetic import (clifford_tfim_circuit, encode_corpus, random_circuit, random_clifford_circuit,
                                           synthetic_backend)

    nq = 40
    circuits = [random_clifford_circuit(nq, 3 + k, k, basis=True) for k in range(4)] + [clifford_tfim_circuit(nq, 1, 1, 2, two_q="cx"),
                                                                           random_circuit(nq, 4, 9)]
    noise = sim.NoiseModel.from_backend(synthetic_backend(nq, "cx"))
    plain = encode_corpus(circuits, nq, seed=7)
    kept = encode_corpus(circuits, nq, seed=7, simulate=noise, device=DEV)   # without clifford=True nothing this wide is simulated
    got = encode_corpus(circuits, nq, seed=7, simulate=noise, device=DEV, clifford=True)
    for key in plain:
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(plain[key], kept[key])), key
    assert all(np.array_equal(np.asarray(plain[k]), np.asarray(got[k])) for k in ("depth", "observable"))
    assert np.array_equal(got["y"][5], plain["y"][5]) and np.array_equal(got["noisy"][5], plain["noisy"][5])   # not Clifford: kept
    for k, c in enumerate(circuits[:5]):
        qz = int(np.argmax(got["observable"][k, 0, 2::4]))
        label = "".join("Z" if q == qz else "I" for q in reversed(range(nq)))
        ideal = cc.tableau_values(c, [label])[0]
        noisy = cc.interpret(sim.compile_clifford([c], [label], noise))[1][0]
        assert got["y"][k, 0] == np.float32(ideal) and got["noisy"][k, 0] == np.float32(noisy)   # float32 storage of the same bits


# ---- quality (recorded, not asserted) ------------------------------------------------------------------------------------------------------
def test_linear_mitigation_of_clifford_tfim_labels_is_recorded():
    """64 100-qubit ``clifford_tfim_circuit`` circuits, four single-Z terms each, noisy labels under the ``synthetic_backend`` model and
    ideal labels from the device; ``encode_data_v2_ecr`` rows -> ``LinearRegressor`` on 40 circuits, scored on the other 24 as the
    ratio of the unmitigated to the mitigated mean L2.  The CPU twin (host interpreter + scikit-learn's LinearRegression) gives
    0.905 (unmitigated 0.1557, mitigated 0.1720): a Clifford TFIM value is -1, 0 or +1 and a linear model of gate counts and the
    noisy value cannot tell a true 0 from a damped +-1, so it does not help here.  The twin stays below 1.5, so nothing about the
    ratio is asserted: both are printed (the device's float32 fit of these rank-deficient rows gave 1.037), and the labels of two
    of the circuits are held to the interpreter bit for bit."""
    from blackwater.nn import LinearRegressor

    circuits, obs, noise, train, val = cc.quality_corpus()
    got = [host(x) for x in sim.run_clifford(sim.compile_clifford(circuits, obs, noise), DEV)]
    ideal, noisy = got[2].reshape(-1, 4), got[3].reshape(-1, 4)
    for k in (0, 42):   # the interpreter takes seconds on all 64; a circuit's bits do not depend on the batch
        _, alone = run_and_compare([circuits[k]], [obs[k]], noise)
        assert np.array_equal(alone[2], ideal[k]) and np.array_equal(alone[3], noisy[k])

    def device_fit(xt, yt, xv):
        model = LinearRegressor.fit(xt.to(DEV), torch.from_numpy(yt).to(DEV, dtype=torch.float32))
        return host(model.predict(xv.to(DEV)))

    x = cc.quality_rows(circuits, noisy)
    unmit, mit = cc.quality_ratio(x, ideal, noisy, train, val, device_fit)
    line = f"Clifford TFIM, 100 qubits: unmitigated L2 {unmit:.6f}, mitigated {mit:.6f}; unmitigated / mitigated: device {unmit / mit:.6f}"
    try:
        from sklearn.linear_model import LinearRegression

        twin = cc.quality_ratio(x, ideal, noisy, train, val, lambda xt, yt, xv: LinearRegression().fit(
            xt.numpy().astype(np.float64), yt).predict(xv.numpy().astype(np.float64)))
        line += f", CPU twin {twin[0] / twin[1]:.6f}"
    except ImportError:
        pass
    print(line)
    assert np.isfinite(unmit) and np.isfinite(mit) and mit > 0
