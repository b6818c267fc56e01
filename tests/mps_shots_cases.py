"""The oracles, the measured margins and the case grid of the matrix-product-state sampler (mlqem_mps_sample_f64), shared by
tests/test_mps_shots_cpu.py and tests/test_gpu_mps_shots.py (no test in here).  numpy only.

Oracle (a), ``reference`` (``sweep`` per group and trajectory): the draw contract of include/mlqem_hip.h followed on the host, on the
site tensors of the host's own interpreter (``mps_cases.interpret(...)["tensors"]``).  Both decompositions, ``lapack`` and ``jacobi``.  The environments and the sweep are plain einsums, not the kernel's loops: another order of the same arithmetic.

Oracle (b), ``dense_shots``: for an ideal circuit within the dense cap, a sampler that never builds an MPS.  The state vector (the
gates of ``sim_cases``), rotated into the group's basis, and every conditional weight as a marginal sum of |amplitude|^2 over the
qubits not yet measured; the same draw rule on the same Philox words.

Margin (measured, not tuned).  d of a case is the largest |lapack - jacobi| over every normalised conditional probability p0 /
(p0 + p1) visited along the drawn paths; the case's margin is max(1e-12, 16 d).  ``D_MEASURED`` records d as it was measured;
the CPU test measures it again and asserts the recorded value within a factor two, which enters no tolerance.  The CPU test also
asserts the CONDITION: every draw of every case lies farther than the margin from its threshold and farther than 1e-12 from a
flip probability, and the oracles give identical bits.  The device is one more order of the same arithmetic, so its bits are
then compared for equality and no case, circuit or shot is excluded.  A seed that violates the condition is changed, never the
margin.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import mps_cases as mc
import sim_cases as sc
from shots_cases import philox4x32_10

FACTOR = 16
FLOOR = 1e-12
C = 0.7071067811865476


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def draw_uniforms(group, site, shots, seed, run_key):
    """``(u, u')`` float64 [len(shots)] of the shots ``shots`` (an int array) at ``site`` of group ``group`` (inside its circuit)."""
    seed, run_key = int(seed) % 2 ** 64, int(run_key) % 2 ** 64
    ctr = np.zeros((len(shots), 4), dtype=np.uint64)
    ctr[:, 0] = 0x80000000 | (int(group) << 9) | int(site)
    ctr[:, 1] = np.asarray(shots, dtype=np.uint64)
    ctr[:, 2], ctr[:, 3] = run_key & 0xFFFFFFFF, run_key >> 32
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)

    def unit(hi, lo):
        return ((hi >> np.uint64(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53

    return unit(x[:, 0], x[:, 1]), unit(x[:, 2], x[:, 3])


def draw_rule(p0, p1, u, u2, flip):
    """The contract's draw on arrays: ``(b, reported, margin, flip_margin)``; ``flip`` = (P(read 1 | 0), P(read 0 | 1)) of the site."""
    w0, w1 = np.where(p0 > 0.0, p0, 0.0), np.where(p1 > 0.0, p1, 0.0)
    target = u * (w0 + w1)
    b = np.where((target < w0) | ~(w1 > 0.0), 0, 1)
    fl = np.where(b == 1, flip[1], flip[0])
    reported = b ^ (u2 < fl)
    with np.errstate(divide="ignore", invalid="ignore"):
        prob = w0 / (w0 + w1)
    return b, reported.astype(np.int64), np.abs(u - prob), np.abs(u2 - fl), prob


def mix(x, letter):
    """[k, 2, r] physical components in the basis of ``letter`` (1 X, 2 Y; else unchanged)."""
    if letter == 1:
        return np.stack([(x[:, 0] + x[:, 1]) * C, (x[:, 0] - x[:, 1]) * C], axis=1)
    if letter == 2:
        return np.stack([(x[:, 0] - 1j * x[:, 1]) * C, (x[:, 0] + 1j * x[:, 1]) * C], axis=1)
    return x


def pack(reported):
    """int [shots, n] bits -> uint32 [shots, W], bit q in word q >> 5."""
    shots, n = reported.shape
    w = (n + 31) // 32
    words = np.zeros((shots, w), dtype=np.uint64)
    for q in range(n):
        words[:, q >> 5] |= reported[:, q].astype(np.uint64) << np.uint64(q & 31)
    return words.astype(np.uint32)


def environments(a):
    """``G[q][l, s, r'] = sum_r A[q][l, s, r] R[q + 1][r, r']`` for every site, R[n] = [1]."""
    r = np.ones((1, 1), dtype=complex)
    out = [None] * len(a)
    for q in range(len(a) - 1, -1, -1):
        out[q] = np.einsum("lsr,rp->lsp", a[q], r)
        r = np.einsum("lsp,msp->lm", out[q], a[q].conj())
    return out


def sweep(a, letters, flip, group, shot_ids, seed, run_key):
    """The shots ``shot_ids`` of one group on the tensors ``a``: ``(reported [k, n], probs [k, n], margin, flip_margin)``."""
    g_env = environments(a)
    k, n = len(shot_ids), len(a)
    v = np.ones((k, 1), dtype=complex)
    reported, probs = np.zeros((k, n), dtype=np.int64), np.zeros((k, n))
    margin = flip_margin = math.inf
    for q in range(n):
        av = mix(np.einsum("kl,lsr->ksr", v, a[q]), int(letters[q]))
        gv = mix(np.einsum("kl,lsr->ksr", v, g_env[q]), int(letters[q]))
        p = np.einsum("ksr,ksr->ks", gv, av.conj()).real
        u, u2 = draw_uniforms(group, q, shot_ids, seed, run_key)
        b, rep, m, fm, prob = draw_rule(p[:, 0], p[:, 1], u, u2, flip[q])
        reported[:, q], probs[:, q] = rep, prob
        margin, flip_margin = min(margin, float(m.min())), min(flip_margin, float(fm.min()))
        v = av[np.arange(k), b] / np.sqrt(p[np.arange(k), b])[:, None]
    return reported, probs, margin, flip_margin


# ---- oracle (b) ------------------------------------------------------------------------------------------------------------------------
_ROT = {1: np.array([[C, C], [C, -C]], dtype=complex), 2: np.array([[C, -1j * C], [C, 1j * C]], dtype=complex)}


def dense_state(circuit):
    """The state vector of an ideal circuit from the gates of ``sim_cases`` (bit q of the index is qubit q)."""
    n = circuit.num_qubits
    psi = np.zeros(2 ** n, dtype=complex)
    psi[0] = 1.0
    for op in circuit.ops:
        if op.name in ("barrier", "measure", "id"):
            continue
        psi = sc.apply(sc.gate_matrix(op.name, op.params), list(op.qubits), psi, n)
    return psi


def dense_shots(circuit, letters, group, shots, seed, run_key):
    """``reported [shots, n]`` of one ideal group without an MPS: conditional weights as marginal sums over the rotated state."""
    n = circuit.num_qubits
    psi = dense_state(circuit)
    for q in range(n):
        if int(letters[q]) in _ROT:
            psi = sc.apply(_ROT[int(letters[q])], [q], psi, n)
    cur = np.broadcast_to(np.abs(psi) ** 2, (shots, 2 ** n))
    ids = np.arange(shots)
    out = np.zeros((shots, n), dtype=np.int64)
    for q in range(n):
        pairs = cur.reshape(shots, -1, 2)          # the last axis is qubit q: the lowest bit left
        p = pairs.sum(axis=1)
        u, u2 = draw_uniforms(group, q, ids, seed, run_key)
        b, rep, _, _, _ = draw_rule(p[:, 0], p[:, 1], u, u2, (0.0, 0.0))
        out[:, q] = rep
        cur = pairs[ids, :, b]
    return out


# ---- the grid ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid():
    """``{id: case}``: circuits, observables, max_bond, noise (None or a model name of ``mps_cases``), trajectories, seed, shots,
    dense (whether oracle (b) and the exact values apply)."""
    from blackwater.data.synthetic import tfim_circuit

    cases = {}

    def add(name, src, shots, seed, dense, **over):
        c = dict(src, id=name, shots=shots, seed=seed, dense=dense)
        c.update(over)
        cases[name] = c

    add("n1-n2", mc.case("n1-n2"), 1000, 11, True)
    for bond in (32, 3):
        add(f"random-b{bond}", mc.case(f"random-b{bond}"), 500, 12, bond == 32)   # bond 3 truncates: the state sampled is not the exact one
    for bond in (32, 16):
        add(f"tfim-n10-s6-b{bond}", mc.case(f"tfim-cx-J1.0-s6-b{bond}"), 400, 13, bond == 32)
    wide = tfim_circuit(33, 2, 1.0, two_q="cx")
    # single Z on every qubit, and strings that cross the boundary between the two words of packed bits
    across = [("I" * 0 + "ZZ" + "I" * 31, 0.5), ("XX" + "I" * 31, 0.25), ("Y" + "I" * 31 + "Y", 0.25), ("Z" + "I" * 15 + "Z" + "I" * 16, 0.5)]
    add("tfim-n33-s2-b4", {"circuits": [wide], "observables": [mc.single_z(33) + across], "max_bond": 4, "noise": None,
                           "trajectories": None}, 256, 14, False)
    for noise in ("readout", "depol", "overrot"):
        for t in (1, 64):
            add(f"noisy-{noise}-T{t}", mc.case(f"noisy-{noise}-T{t}"), 1000, 15, False)
    add("noisy-depol-T64-s64", mc.case("noisy-depol-T64"), 64, 16, False)
    add("width-clifford-n100-s3-b8", mc.case("width-clifford-n100-s3-b8"), 256, 17, False)
    return cases


def case(case_id):
    return grid()[case_id]


IDS = ("n1-n2", "random-b32", "random-b3", "tfim-n10-s6-b32", "tfim-n10-s6-b16", "tfim-n33-s2-b4", "noisy-readout-T1", "noisy-readout-T64",
       "noisy-depol-T1", "noisy-depol-T64", "noisy-overrot-T1", "noisy-overrot-T64", "noisy-depol-T64-s64", "width-clifford-n100-s3-b8")


def noise_of(c):
    return None if c["noise"] is None else mc.noise_model(c["noise"], 11)


@functools.lru_cache(maxsize=None)
def lower(case_id):
    from blackwater.sim import compile_mps_shots

    c = case(case_id)
    return compile_mps_shots(c["circuits"], c["observables"], noise_of(c), c["trajectories"], c["max_bond"])


def fma(a, b, c):
    """round(a * b + c), exactly."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def finish(coeff, sums, shots):
    """``(term_values, value, variance)`` with the expressions of the finish kernel."""
    tv = [float(int(s)) / float(shots) for s in sums]
    value = var = 0.0
    for cf, t in zip(coeff, tv):
        cf = float(cf)
        value = fma(cf, t, value)
        var = fma(cf * cf, fma(-t, t, 1.0), var)
    return np.asarray(tv, dtype=np.float64), value, var


@functools.lru_cache(maxsize=None)
def reference(case_id, method="lapack"):
    """Oracle (a) on a whole case (run key = the circuit's position): a list per circuit of dicts with ``bits`` (uint32 [shots, W]
    per group), ``reported`` / ``probs`` ([shots, n] per group), ``term_sums``, ``term_values``, ``value``, ``variance``, ``margin``,
    ``flip_margin``, ``discarded`` / ``error_bound`` (means over the trajectories) and ``bond``, ``mps_terms`` (the first trajectory's term values)."""
    c, batch = case(case_id), lower(case_id)
    mps, shots, seed = batch.mps, c["shots"], c["seed"]
    n_traj = c["trajectories"] or 1
    out = []
    for k in range(len(batch)):
        n = int(mps.n_qubits[k])
        units = [mc.interpret(mps, k, method, t, seed) for t in range(min(n_traj, shots))]
        flip = batch.flip[int(mps.site_ptr[k]):int(mps.site_ptr[k]) + n]
        res = {"bits": [], "reported": [], "probs": [], "margin": math.inf, "flip_margin": math.inf,
               "discarded": sum(u["discarded"] for u in units) / len(units), "error_bound": sum(u["error_bound"] for u in units) / len(units),
               "bond": max(u["bond"] for u in units), "mps_terms": mc.contract_terms(mps, k, units[0]["tensors"])}
        g0, g1 = int(batch.group_ptr[k]), int(batch.group_ptr[k + 1])
        for g in range(g0, g1):
            letters = batch.basis[int(batch.group_off[g]):int(batch.group_off[g]) + n]
            reported, probs = np.zeros((shots, n), dtype=np.int64), np.zeros((shots, n))
            for t, unit in enumerate(units):
                ids = np.arange(t, shots, n_traj)
                rep, pr, m, fm = sweep(unit["tensors"], letters, flip, g - g0, ids, seed, k)
                reported[ids], probs[ids] = rep, pr
                res["margin"], res["flip_margin"] = min(res["margin"], m), min(res["flip_margin"], fm)
            res["reported"].append(reported)
            res["probs"].append(probs)
            res["bits"].append(pack(reported))
        tb, te = int(mps.term_ptr[k]), int(mps.term_ptr[k + 1])
        sums = []
        for t in range(tb, te):
            words = res["bits"][int(batch.term_group[t])]
            w = words.shape[1]
            support = batch.masks[int(batch.term_mask[t]):int(batch.term_mask[t]) + w]
            par = np.zeros(shots, dtype=np.int64)
            for j in range(w):
                x = words[:, j] & support[j]
                par ^= np.array([bin(int(v)).count("1") & 1 for v in x], dtype=np.int64)
            sums.append(int((1 - 2 * par).sum()))
        res["term_sums"] = np.asarray(sums, dtype=np.int64)
        res["term_values"], res["value"], res["variance"] = finish(mps.coeff[tb:te], sums, shots)
        out.append(res)
    return out


def measured_d(case_id):
    """The largest |lapack - jacobi| over every normalised conditional probability along the drawn paths of a case."""
    worst = 0.0
    for x, y in zip(reference(case_id, "lapack"), reference(case_id, "jacobi")):
        for px, py in zip(x["probs"], y["probs"]):
            d = float(np.max(np.abs(px - py)))
            assert math.isfinite(d), (case_id, d)
            worst = max(worst, d)
    return worst


# case: d as it was measured when the table was written (``measured_d``).  The margin is max(1e-12, 16 d).
D_MEASURED = {
    "n1-n2": 4.4e-16, "random-b32": 1.4e-14, "random-b3": 2.0e-14, "tfim-n10-s6-b32": 2.8e-14, "tfim-n10-s6-b16": 3.2e-14,
    "tfim-n33-s2-b4": 5.6e-15, "noisy-readout-T1": 2.2e-16, "noisy-readout-T64": 2.2e-16, "noisy-depol-T1": 3.3e-16,
    "noisy-depol-T64": 3.3e-16, "noisy-overrot-T1": 3.7e-15, "noisy-overrot-T64": 3.7e-15, "noisy-depol-T64-s64": 3.3e-16,
    "width-clifford-n100-s3-b8": 4.5e-14,
}


def margin(case_id):
    return max(FLOOR, FACTOR * D_MEASURED[case_id])


def counts_of(words, n):
    """``{bitstring: count}`` of uint32 [shots, W] words: n characters, qubit 0 rightmost."""
    out = {}
    for row in words.tolist():
        key = format(sum(int(v) << (32 * j) for j, v in enumerate(row)), f"0{n}b")
        out[key] = out.get(key, 0) + 1
    return out


def exact_terms(case_id):
    """Per circuit the exact term values of a dense ideal case (``sim_cases.simulate``)."""
    c = case(case_id)
    from blackwater.data.backends import pauli_terms
    from blackwater.data.circuit import Circuit

    return [sc.simulate(Circuit.from_any(circ), list(pauli_terms(obs)))[1] for circ, obs in zip(c["circuits"], c["observables"])]


def five_sigma(est, exact, shots):
    est, exact = np.asarray(est, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    return np.abs(est - exact) <= 5.0 * np.sqrt(np.maximum(1.0 - exact * exact, 0.0) / shots) + 1e-12
