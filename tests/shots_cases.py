"""The measurement-shots oracle, the derived bounds and the case grid shared by tests/test_shots_cpu.py and tests/test_gpu_shots.py
(no test in here).  numpy only; the circuit oracle is ``sim_cases.simulate``, by import.

Grouping.  :func:`group_terms` restates the rule from Pauli LABELS, independently of ``blackwater.sim.measurement_groups`` (which
works on lowered masks): greedy qubit-wise commuting in term order -- a term joins the first group whose basis agrees with it on
every qubit where the term is not ``I`` and extends that basis by its own qubits, else it opens a group; untouched qubits are
measured in Z.

Probabilities in a rotated basis.  The probability of outcome j when qubit q is measured in the basis B_q (X, Y or Z) is the
expectation value of the projector  prod_q (I + (-1)^(j_q) B_q) / 2  =  2^-n sum_S (-1)^popcount(j & S) P_S,  P_S the Pauli string
with B_q on the qubits of S.  So ``sim_cases.simulate`` is asked for the 2^n strings P_S and the outcome distribution is their
Walsh-Hadamard transform: no basis-change gate is added to the circuit (a position-keyed noise spec would see it).

Bound on the probabilities (derived, not fitted; u = 2^-53).  ``sim_cases.term_bound`` bounds |device - oracle| of the expectation
value of ANY observable of unit operator norm (vector mode: 2 |d psi|) or of Frobenius norm <= 2^(n/2) (density mode); a
projector qualifies (its norms are 1).  The device reaches group g's probabilities after the circuit AND the rotation records of
the measurement tail: at most every rotation and inverse rotation of the tail, 2 k one-qubit matrices for k rotated qubits over
all groups, each at the one-qubit cost 12 (twice that in density mode).  ``prob_bound`` is ``term_bound`` with that cost added to
the circuit's (counted on both sides, which only loosens it: the oracle applies no rotation).  Its sum term N + N / 64 + 16 covers
the oracle's transform (N addends of total magnitude <= 1) and the device's three rounded operations per entry.  The sum of a
group's probabilities is the expectation value of the identity, an observable of unit norm, formed with N additions: it equals
``norm`` within the SAME prob_bound (its N + N / 64 + 16 term is the summation's).

The CDF rule, as include/mlqem_hip.h states it.  p_j <- p_j if p_j > 0 else 0.  L = min(M, 8), C = M / L chunks of L consecutive
outcomes.  Inside chunk k: run_k[0] = p[k L], run_k[i] = run_k[i - 1] + p[k L + i]; tot[k] = run_k[L - 1]; before[0] = 0,
before[k] = before[k - 1] + tot[k - 1]; cdf[k L + i] = before[k] + run_k[i].

The sampler.  Shot s: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (s >> 1, group inside its circuit, run_key &
0xffffffff, run_key >> 32); an even s takes words (0, 1), an odd s (2, 3); u = ((a >> 5) 2^26 + (b >> 6)) 2^-53; target = u cdf[M - 1];
j = min(#{i : cdf[i] <= target}, #{i : cdf[i] < cdf[M - 1]}).  Estimates: S_t / shots with S_t = sum_j counts_j (-1)^popcount(j & support);
value = sum coeff * estimate in term order; variance = sum coeff^2 (1 - estimate^2).
"""
import functools

import numpy as np

import sim_cases as sc

U = sc.U
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


# ---- Philox4x32-10 -----------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """``counter`` uint [..., 4], ``key`` two ints -> uint32 [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & MASK for i in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def uniforms(shots, seed, run_key, group):
    """float64 [shots]: u of every shot of one (run, group)."""
    seed, run_key = int(seed) % 2 ** 64, int(run_key) % 2 ** 64
    pairs = (int(shots) + 1) // 2
    ctr = np.zeros((pairs, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(pairs)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = int(group), run_key & 0xFFFFFFFF, run_key >> 32
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).astype(np.uint64)
    a, b = x[:, [0, 2]].reshape(-1)[:shots], x[:, [1, 3]].reshape(-1)[:shots]   # shot 2 i: words 0, 1; shot 2 i + 1: words 2, 3
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53


# ---- the CDF and the sampler ---------------------------------------------------------------------------------------------------------
def cdf_rule(p):
    p = np.asarray(p, dtype=np.float64)
    p = np.where(p > 0.0, p, 0.0)
    m = p.shape[0]
    length = min(m, 8)
    cdf, before = np.empty(m, dtype=np.float64), np.float64(0.0)
    for k in range(m // length):
        run = np.float64(0.0)
        for i in range(length):
            run = p[k * length + i] if i == 0 else run + p[k * length + i]
            cdf[k * length + i] = before + run
        before = before + run
    return cdf


def pick(cdf, u):
    """Outcomes for uniforms ``u``: min(#{cdf <= u total}, #{cdf < total}).  The CDF is non-decreasing, so the counts are searches."""
    total = cdf[-1]
    target = np.asarray(u, dtype=np.float64) * total
    j_last = int(np.searchsorted(cdf, total, side="left"))
    return np.minimum(np.searchsorted(cdf, target, side="right"), j_last)


def sample_counts(p, shots, seed, run_key, group, u=None):
    """int64 [M] counts of one (run, group) from its probabilities ``p``."""
    cdf = cdf_rule(p)
    j = pick(cdf, uniforms(shots, seed, run_key, group) if u is None else u)
    return np.bincount(j, minlength=len(cdf)).astype(np.int64)


def parity_signs(m, support):
    j = np.arange(m)
    par = np.zeros(m, dtype=np.int64)
    s = int(support)
    while s:
        b = s & -s
        par ^= (j & b) != 0
        s ^= b
    return 1 - 2 * par


def estimates(counts, supports, shots):
    """float64 [T]: (sum_j counts_j (-1)^popcount(j & support_t)) / shots, the integer sum divided once."""
    counts = np.asarray(counts, dtype=np.int64)
    return np.asarray([float(int((counts * parity_signs(len(counts), s)).sum())) / float(shots) for s in supports], dtype=np.float64)


def value_and_variance(coeffs, est):
    value, var = 0.0, 0.0
    for c, t in zip(coeffs, est):
        value = value + float(c) * float(t)
        var = var + float(c) * float(c) * (1.0 - float(t) * float(t))
    return value, var


# ---- grouping ------------------------------------------------------------------------------------------------------------------------
def group_terms(labels):
    """``(term_group, bases)``: the group of every label and one basis string per group (rightmost character on qubit 0, Z where no
    term of the group acts).  No labels: one all-Z group cannot be formed without n, so ``bases`` is then empty."""
    bases, term_group = [], []
    for label in labels:
        for g, basis in enumerate(bases):
            if all(ch == "I" or b == "I" or ch == b for ch, b in zip(label, basis)):
                bases[g] = "".join(b if ch == "I" else ch for ch, b in zip(label, basis))
                term_group.append(g)
                break
        else:
            bases.append(label)
            term_group.append(len(bases) - 1)
    return term_group, [b.replace("I", "Z") for b in bases]


def support_of(label):
    return sum(1 << q for q, ch in enumerate(reversed(label)) if ch != "I")


# ---- probabilities in a basis ------------------------------------------------------------------------------------------------------------
def basis_probabilities(circuit, basis, noise=None):
    """float64 [2^n]: the outcome distribution of ``circuit`` measured in ``basis`` (a string over X, Y, Z, rightmost on qubit 0), from
    ``sim_cases.simulate`` on the 2^n strings P_S; and the oracle's norm."""
    n = circuit.num_qubits
    big_n = 2 ** n
    strings = []
    for s in range(big_n):
        strings.append(("".join(basis[n - 1 - q] if (s >> q) & 1 else "I" for q in reversed(range(n))), 1.0))
    _, tv, norm = sc.simulate(circuit, strings, noise)
    j = np.arange(big_n)
    signs = np.stack([parity_signs(big_n, s) for s in range(big_n)], axis=1)   # [j, S]
    assert signs.shape == (big_n, big_n) and (signs[j, 0] == 1).all()
    return (signs @ tv) / big_n, norm


def prob_bound(circuit, noise, bases):
    """|device - oracle| of one outcome probability: term_bound with the cost of the tail's rotation records added."""
    n = circuit.num_qubits
    big_n = 2 ** n
    rotated = sum(sum(1 for ch in b if ch != "Z") for b in bases)
    tail = 2 * rotated * 12 * (2 if noise is not None else 1)
    s = 2.0 if noise is None else np.sqrt(big_n)
    return U * (2 * s * (sc.op_cost_sum(circuit, noise) + tail) + big_n + big_n / 64 + 16)


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
SHOTS = (1, 2, 63, 64, 65, 257, 10000)
N_OPS = 10


def seed_for(shots):
    """The seed a batch is sampled with at ``shots`` (cleared by the 5-sigma condition in tests/test_shots_cpu.py)."""
    return 1000 + shots


def _pad(label, n):
    return "I" * (n - len(label)) + label


def observables_for(n, alphabet="IXYZ"):
    """(name, terms) for: a single Z, a 4-term all-Z sum, {XX, YY, ZZ, ZI}, one with a Y and an identity term (as far as n and the
    alphabet allow)."""
    out = [("z", [(_pad("Z", n), 1.0)])]
    z4 = [("I" * (n - 1 - q) + "Z" + "I" * q, c) for q, c in zip(range(min(n, 3)), (0.5, -0.25, 0.75))] + [("Z" * n, -0.4)]
    out.append(("z4", z4[:4] if n > 1 else [(_pad("Z", n), 0.5), ("I" * n, 0.3)]))
    if alphabet == "IXYZ":
        if n >= 2:
            out.append(("xyz", [(_pad("XX", n), 0.3), (_pad("YY", n), -0.2), (_pad("ZZ", n), 0.5), (_pad("ZI", n), 0.7)]))
        y = ["I"] * n
        y[0] = "Y"
        if n >= 3:
            y[1] = "X"
        out.append(("yi", [("I" * n, 0.25), ("".join(y), -0.6), (_pad("Z", n), 0.1)]))
    return out


@functools.lru_cache(maxsize=None)
def batches():
    """``{name: (circuits, observables (term lists), noise, ids)}``: the vector batch (n = 1, 2, 5, 8, 9, 11: either side of the wave /
    workgroup split and the cap), the density batch (n = 1, 3, 5, a depolarising op after every gate) and the readout batch (the
    same with readout ops, I / Z observables).  Programs of 10 gates.  Every batch mixes its sizes, so the waves of a workgroup have
    different trip counts."""
    out = {}
    circuits, observables, ids = [], [], []
    for n in (1, 2, 5, 8, 9, 11):
        c = sc.random_program(n, N_OPS, seed=40 + n)
        for name, terms in observables_for(n):
            circuits.append(c)
            observables.append(terms)
            ids.append(f"vector-n{n}-{name}")
    out["vector"] = (circuits, observables, None, ids)
    circuits, observables, ids = [], [], []
    for n in (1, 3, 5):
        c = sc.random_program(n, N_OPS, seed=50 + n)
        for name, terms in observables_for(n):
            circuits.append(c)
            observables.append(terms)
            ids.append(f"density-n{n}-{name}")
    out["density"] = (circuits, observables, sc.StepNoise(61), ids)
    circuits, observables, ids = [], [], []
    noise = sc.StepNoise(62, readout={q: (0.01 + 0.02 * q, 0.06 - 0.01 * q) for q in range(5)})
    for n in (1, 3, 5):
        c = sc.random_program(n, N_OPS, seed=60 + n, measure=True)
        for name, terms in observables_for(n, alphabet="IZ"):
            circuits.append(c)
            observables.append(terms)
            ids.append(f"readout-n{n}-{name}")
    out["readout"] = (circuits, observables, noise, ids)
    return out


@functools.lru_cache(maxsize=None)
def _probs_cached(batch_name, index, basis):
    circuits, _, noise, _ = batches()[batch_name]
    return basis_probabilities(circuits[index], basis, noise)


@functools.lru_cache(maxsize=None)
def oracle(batch_name):
    """Per circuit of a batch: ``term_group``, ``bases``, ``probs`` (one array per group), ``norm``, ``exact`` (term values),
    ``supports``, ``coeffs``, ``prob_bound``.  Computed once; circuits that share a program share their Z-basis distribution."""
    circuits, observables, noise, _ = batches()[batch_name]
    first = {}
    out = []
    for k, (c, terms) in enumerate(zip(circuits, observables)):
        labels = [label for label, _ in terms]
        tg, bases = group_terms(labels)
        src = first.setdefault(id(c), k)   # the cache is keyed by the first circuit that shares this program
        probs, norm = [], None
        for b in bases:
            p, norm = _probs_cached(batch_name, src, b)
            probs.append(p)
        _, exact, _ = sc.simulate(c, terms, noise)
        out.append({"term_group": tg, "bases": bases, "probs": probs, "norm": norm, "exact": exact,
                    "supports": [support_of(label) for label in labels], "coeffs": [float(cf) for _, cf in terms],
                    "prob_bound": prob_bound(c, noise, bases)})
    return out


def oracle_sample(entry, shots, seed, run_key, probs=None):
    """``(counts per group, estimates [T], value, variance)`` of one circuit from the oracle's (or the given) probabilities."""
    probs = entry["probs"] if probs is None else probs
    counts = [sample_counts(p, shots, seed, run_key, g) for g, p in enumerate(probs)]
    est = np.empty(len(entry["supports"]), dtype=np.float64)
    for t, (g, s) in enumerate(zip(entry["term_group"], entry["supports"])):
        est[t] = estimates(counts[g], [s], shots)[0]
    value, var = value_and_variance(entry["coeffs"], est)
    return counts, est, value, var


def five_sigma_ok(est, exact, shots):
    exact = np.asarray(exact, dtype=np.float64)
    return np.abs(np.asarray(est) - exact) <= 5.0 * np.sqrt(np.clip(1.0 - exact * exact, 0.0, None) / shots) + 1.0 / shots
