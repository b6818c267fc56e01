"""The host interpreter, the oracles and the case builders shared by tests/test_clifford_frames_cpu.py and
tests/test_gpu_clifford_frames.py (no test in here).  Builds on tests/clifford_cases.py, tests/sim_cases.py and tests/shots_cases.py
and leaves them alone.

(a) ``interpret``: the rule of mlqem_clifford_sample_f64 as include/mlqem_hip.h words it, step by step: the pull-back with Python
    integers, the reference outcome by the pivot procedure, one Pauli frame per shot (numpy over the shots, a Python loop over the
    records), Philox4x32-10 from ``shots_cases`` with the counter packing of the header, integer sums, one division per term.  The
    device must equal it to the last bit.
(b) ``outcome_probabilities``: ``shots_cases.basis_probabilities``, i.e. ``sim_cases.simulate`` on the 2^n parity strings of a
    basis -- the state-vector / density-matrix oracle, n <= 8 ideal and n <= 5 with noise.  Shares nothing with (a).
(c) ``exact_terms``: ``clifford_cases.interpret`` on the same circuits: the exact noisy value every estimate has as its limit.

The statistical condition (that of the shots path): |estimate - exact| <= 5 sqrt((1 - exact^2) / shots) + 1 / shots.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import clifford_cases as cc
import shots_cases
import sim_cases

C1, C2, DEPOL1, DEPOL2 = range(4)
DOMAIN_Z, DOMAIN_NOISE, DOMAIN_READOUT = 0, 1, 2
U = 2.0 ** -53


def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def _int_of(words):
    return sum(int(v) << (32 * j) for j, v in enumerate(words))


def _mask_words(batch, at, w):
    n_masks = len(batch.masks)
    return [int(batch.masks[_clamp(at + j, 0, n_masks - 1)]) for j in range(w)]


def group_shape(batch, g):
    """(circuit, n, W, group inside its circuit) of group ``g``."""
    c = int(batch.group_circ[g])
    n = int(batch.n_qubits[c])
    return c, n, (n + 31) // 32, g - int(batch.group_ptr[c])


def records(batch, c):
    base = batch.clifford
    return [tuple(int(v) for v in base.ops[k]) for k in range(int(base.op_ptr[c]), int(base.op_ptr[c + 1]))]


# ---- 1. the pull-back ----------------------------------------------------------------------------------------------------------------
def pullback(batch, g):
    """``[(x, z, sign)]`` per qubit: P_q = U^dagger B_q U as Python integers, noise records ignored."""
    c, n, w, _ = group_shape(batch, g)
    gm = int(batch.group_mask[g])
    bx, bz = _int_of(_mask_words(batch, gm, w)), _int_of(_mask_words(batch, gm + w, w))
    recs = records(batch, c)
    rows = []
    for q in range(n):
        x, z, sign = (bx >> q & 1) << q, (bz >> q & 1) << q, 0
        for head, a, b, cc_ in reversed(recs):
            kind, q0, q1 = head & 15, min(head >> 4 & 1023, n - 1), min(head >> 14 & 1023, n - 1)
            l0 = (x >> q0 & 1) | (z >> q0 & 1) << 1
            l1 = ((x >> q1 & 1) | (z >> q1 & 1) << 1) if kind == C2 else 0
            p = l0 | l1 << 2
            if kind == C1 and l0:
                img = a >> (3 * (l0 - 1)) & 7
                sign ^= img >> 2
                x = x & ~(1 << q0) | (img & 1) << q0
                z = z & ~(1 << q0) | (img >> 1 & 1) << q0
            elif kind == C2 and p:
                e = p - 1
                img = (a | b << 32) >> (4 * e) & 15
                sign ^= cc_ >> e & 1
                for qq, l in ((q0, img & 3), (q1, img >> 2)):
                    x = x & ~(1 << qq) | (l & 1) << qq
                    z = z & ~(1 << qq) | (l >> 1) << qq
        rows.append((x, z, sign))
    return rows


# ---- 2. the reference outcome --------------------------------------------------------------------------------------------------------
def _exponent(x1, z1, x2, z2):
    """The Aaronson-Gottesman exponent of i of (x1, z1) . (x2, z2), summed over the qubits: +1 and -1 counted apart."""
    plus = (x1 & z1 & z2 & ~x2) | (x1 & ~z1 & z2 & x2) | (~x1 & z1 & x2 & ~z2)
    minus = (x1 & z1 & x2 & ~z2) | (x1 & ~z1 & z2 & ~x2) | (~x1 & z1 & x2 & z2)
    return bin(plus).count("1") - bin(minus).count("1")


def reference_outcome(rows):
    """m as an integer (bit q = m_q), and the rank (the number of pivots: the outcome set has 2^rank members)."""
    pivots = {}   # position of the lowest x bit -> (x, z, sign, v)
    m = 0
    for q, (x, z, sign) in enumerate(rows):
        acc = 0
        while x:
            pos = (x & -x).bit_length() - 1
            if pos not in pivots:
                break
            px, pz, ps, pv = pivots[pos]
            t = _exponent(x, z, px, pz)
            assert t % 2 == 0, "the rows commute"
            sign ^= ps ^ ((t >> 1) & 1)
            x, z, acc = x ^ px, z ^ pz, acc ^ pv
        if x:
            pivots[(x & -x).bit_length() - 1] = (x, z, sign, acc)
        else:
            m |= (sign ^ acc) << q
    return m, len(pivots)


# ---- 3. draws --------------------------------------------------------------------------------------------------------------------------
def draw(seed, run_key, gl, shots, domain, block):
    """uint32 [shots, 4]: the Philox block of every shot."""
    seed, run_key = int(seed) % 2 ** 64, int(run_key) % 2 ** 64
    ctr = np.zeros((shots, 4), dtype=np.uint64)
    ctr[:, 0], ctr[:, 1] = run_key & 0xFFFFFFFF, run_key >> 32
    ctr[:, 2] = np.arange(shots, dtype=np.uint64) | np.uint64(gl << 20)
    ctr[:, 3] = domain << 30 | block
    return shots_cases.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))


# ---- 4, 5. frames and outcomes ----------------------------------------------------------------------------------------------------------
def _inverse_c1(a):
    inv = [0, 1, 1, 1]
    for j in (2, 1, 0):   # the lowest field wins
        if a >> (3 * j) & 3:
            inv[a >> (3 * j) & 3] = j + 1
    return np.asarray(inv, dtype=np.uint32)


def _inverse_c2(tab):
    inv = [1] * 16
    for e in range(14, -1, -1):
        inv[tab >> (4 * e) & 15] = e + 1
    inv[0] = 0
    return np.asarray(inv, dtype=np.uint32)


def sample_bits(batch, g, m, shots, seed, run_key):
    """uint32 [shots, W]: the outcome of every shot of group ``g``, the reference outcome ``m`` given."""
    c, n, w, gl = group_shape(batch, g)
    one = np.uint32(1)
    keep = np.asarray([((1 << n) - 1) >> (32 * j) & 0xFFFFFFFF for j in range(w)], dtype=np.uint32)
    xs = np.zeros((shots, w), dtype=np.uint32)
    zs = np.zeros((shots, w), dtype=np.uint32)
    for j in range(w):
        zs[:, j] = draw(seed, run_key, gl, shots, DOMAIN_Z, j >> 2)[:, j & 3] & keep[j]

    def letter(q):
        return ((xs[:, q >> 5] >> np.uint32(q & 31)) & one) | (((zs[:, q >> 5] >> np.uint32(q & 31)) & one) << one)

    def flip(q, d):   # d: uint32 [shots], the letter to XOR into qubit q
        xs[:, q >> 5] ^= (d & one) << np.uint32(q & 31)
        zs[:, q >> 5] ^= ((d >> one) & one) << np.uint32(q & 31)

    thresh = batch.thresh
    for i, (head, a, b, _) in enumerate(records(batch, c)):
        kind, q0, q1 = head & 15, min(head >> 4 & 1023, n - 1), min(head >> 14 & 1023, n - 1)
        if kind == C1:
            l0 = letter(q0)
            flip(q0, _inverse_c1(a)[l0] ^ l0)
        elif kind == C2:
            l0, l1 = letter(q0), letter(q1)
            p = l0 | l1 << np.uint32(2)
            d = _inverse_c2(a | b << 32)[p] ^ p
            flip(q0, d & np.uint32(3))
            flip(q1, d >> np.uint32(2))
        elif kind in (DEPOL1, DEPOL2):
            index = a - (1 << 32) if a >= 1 << 31 else a
            t = np.uint64(int(thresh[_clamp(index, 0, len(thresh) - 1)]))
            x = draw(seed, run_key, gl, shots, DOMAIN_NOISE, i >> 1).astype(np.uint64)
            v = x[:, 2 * (i & 1)] | x[:, 2 * (i & 1) + 1] << np.uint64(32)
            hit = (v >> np.uint64(4)) < t
            pl = np.where(hit, v & np.uint64(15 if kind == DEPOL2 else 3), np.uint64(0)).astype(np.uint32)
            flip(q0, pl & np.uint32(3))
            if kind == DEPOL2:
                flip(q1, pl >> np.uint32(2))
    gm = int(batch.group_mask[g])
    bx = np.asarray(_mask_words(batch, gm, w), dtype=np.uint32)
    bz = np.asarray(_mask_words(batch, gm + w, w), dtype=np.uint32)
    mw = np.asarray([m >> (32 * j) & 0xFFFFFFFF for j in range(w)], dtype=np.uint32)
    bits = (mw[None, :] ^ (xs & bz[None, :]) ^ (zs & bx[None, :])) & keep[None, :]
    ro = int(batch.ro_ptr[c])
    if ro >= 0:
        for q in range(n):
            u = draw(seed, run_key, gl, shots, DOMAIN_READOUT, q >> 2)[:, q & 3].astype(np.uint64)
            bit = (bits[:, q >> 5] >> np.uint32(q & 31)) & one
            t = np.where(bit == 1, np.uint64(int(thresh[ro + 2 * q + 1])), np.uint64(int(thresh[ro + 2 * q])))
            bits[:, q >> 5] ^= (u < t).astype(np.uint32) << np.uint32(q & 31)
    return bits


def parity_sum(bits, support_words):
    """S = sum over the shots of (-1)^popcount(bits & support), an integer."""
    par = np.zeros(bits.shape[0], dtype=np.uint32)
    for j, s in enumerate(support_words):
        par ^= bits[:, j] & np.uint32(s)
    for shift in (16, 8, 4, 2, 1):
        par ^= par >> np.uint32(shift)
    odd = int((par & np.uint32(1)).sum())
    return bits.shape[0] - 2 * odd


def references(batch):
    """``[(m, rank)]`` per group; kept on the batch (they do not depend on shots, seed or run keys)."""
    if not hasattr(batch, "_interpreted_references"):
        batch._interpreted_references = [reference_outcome(pullback(batch, g)) for g in range(len(batch.group_circ))]
    return batch._interpreted_references


# ---- (a) the whole call ------------------------------------------------------------------------------------------------------------------
def interpret(batch, shots, seed=0, run_keys=None):
    """dict: ``reference`` (uint32 [n_ref]), ``rank`` per group, ``bits`` (a list of uint32 [shots, W] per group), ``term_sums``
    (int64), ``term_values``, ``values``, ``variance`` (float64; values and variances as plain sums in term order: the device fuses
    its multiply-adds, so these two are compared within (T + 2) 2^-53 of their sums)."""
    b = len(batch)
    keys = np.arange(b, dtype=np.int64) if run_keys is None else np.asarray(run_keys, dtype=np.int64)
    n_groups = len(batch.group_circ)
    reference = np.zeros(int(batch.ref_ptr[-1]), dtype=np.uint32)
    rank, all_bits = [], []
    sums = np.zeros(len(batch.coeff), dtype=np.int64)
    for g in range(n_groups):
        c, n, w, _ = group_shape(batch, g)
        m, r = references(batch)[g]
        rank.append(r)
        reference[int(batch.ref_ptr[g]):int(batch.ref_ptr[g]) + w] = [m >> (32 * j) & 0xFFFFFFFF for j in range(w)]
        bits = sample_bits(batch, g, m, shots, seed, int(keys[c]))
        all_bits.append(bits)
        for t in batch.gterm[int(batch.gterm_ptr[g]):int(batch.gterm_ptr[g + 1])]:
            sums[t] = parity_sum(bits, _mask_words(batch, int(batch.term_mask[t]), w))
    term_values = np.asarray([float(int(s)) / float(shots) for s in sums], dtype=np.float64)
    values, variance, scale = np.zeros(b), np.zeros(b), np.zeros(b)
    for c in range(b):
        tb, te = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
        cf, tv = batch.coeff[tb:te], term_values[tb:te]
        values[c] = math.fsum(cf * tv)
        variance[c] = math.fsum(cf * cf * (1.0 - tv * tv))
        scale[c] = math.fsum(np.abs(cf)) + math.fsum(cf * cf)
    return {"reference": reference, "rank": rank, "bits": all_bits, "term_sums": sums, "term_values": term_values, "values": values,
            "variance": variance, "scale": scale}


def value_bound(batch, c, scale):
    """|device - the sum| allowed for ``values[c]`` and ``variance[c]``: (T + 2) 2^-53 of the sum of the absolute addends' bound.
    Every addend is at most |coeff| (or coeff^2) and each of the T fused multiply-adds rounds once; the interpreter's own sum is
    exact to one rounding (fsum)."""
    t = int(batch.term_ptr[c + 1]) - int(batch.term_ptr[c])
    return (t + 2) * U * max(scale, 1.0)


# ---- (b), (c) oracles ----------------------------------------------------------------------------------------------------------------------
def basis_string(batch, g):
    """The group's basis as a string over X, Y, Z, rightmost character on qubit 0."""
    _, n, w, _ = group_shape(batch, g)
    gm = int(batch.group_mask[g])
    bx, bz = _int_of(_mask_words(batch, gm, w)), _int_of(_mask_words(batch, gm + w, w))
    return "".join("IXZY"[(bx >> q & 1) | (bz >> q & 1) << 1] for q in reversed(range(n)))


def outcome_probabilities(circuit, basis, noise=None):
    """float64 [2^n] from ``sim_cases.simulate`` (through ``shots_cases.basis_probabilities``)."""
    return shots_cases.basis_probabilities(circuit, basis, noise)[0]


def outcomes_as_integers(bits):
    return [_int_of(row) for row in bits.tolist()]


def exact_terms(circuits, observables, noise=None):
    """The exact term values (noise and readout included) from ``clifford_cases.interpret``."""
    from blackwater import sim

    return cc.interpret(sim.compile_clifford(circuits, observables, noise))[3]


def five_sigma(est, exact, shots):
    """(ok, worst sigma): |est - exact| <= 5 sqrt((1 - exact^2) / shots) + 1 / shots per term; the worst excess in sigmas."""
    est, exact = np.asarray(est, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    sd = np.sqrt(np.maximum(1.0 - exact * exact, 0.0) / shots)
    ok = np.abs(est - exact) <= 5.0 * sd + 1.0 / shots
    sig = np.where(sd > 0, np.abs(est - exact) / np.where(sd > 0, sd, 1.0), 0.0)
    return bool(ok.all()), float(sig.max()) if len(sig) else 0.0


# ---- case builders ---------------------------------------------------------------------------------------------------------------------
def ghz(n, measure=True):
    """H on qubit 0 and a CX chain."""
    from blackwater.data.circuit import Circuit, CircuitOp

    ops = [CircuitOp("h", (0,))] + [CircuitOp("cx", (q, q + 1)) for q in range(n - 1)]
    if measure:
        ops += [CircuitOp("measure", (q,), (q,)) for q in range(n)]
    return Circuit(n, n if measure else 0, ops)


def layer(n, name, measure=True):
    from blackwater.data.circuit import Circuit, CircuitOp

    ops = [CircuitOp(name, (q,)) for q in range(n)]
    if measure:
        ops += [CircuitOp("measure", (q,), (q,)) for q in range(n)]
    return Circuit(n, n if measure else 0, ops)


class FixedNoise:
    """Depolarising lambda after every gate: ``lam`` everywhere (0, a calibrated value or 1), or drawn per op when ``lam`` is None
    (``sim_cases.StepNoise`` with 0 and 1 forced once each); readout ``(p01, p10)`` for every qubit when given."""

    def __init__(self, lam=None, readout=None, seed=0):
        self._lam, self._step = lam, sim_cases.StepNoise(seed)
        self._readout = readout
        self.has_readout = readout is not None

    def after_gate(self, index, name, qubits):
        return self._step.after_gate(index, name, qubits) if self._lam is None else self._lam

    def readout_of(self, qubit):
        return self._readout


GRID_N = (1, 2, 5, 31, 32, 33, 64, 65, 128, 129, 512)
GRID_SHOTS = (1, 63, 64, 65, 255, 256, 257, 600)
# name -> (noise or None, Z-only observables?)  Readout noise takes Z-only observables (X / Y beside it is refused).
GRID_NOISE = {
    "ideal": lambda: None,
    "depol0": lambda: FixedNoise(0.0),
    "depol": lambda: FixedNoise(None, seed=5),
    "depol1": lambda: FixedNoise(1.0),
    "readout0": lambda: FixedNoise(None, readout=(0.0, 0.0), seed=6),
    "readout": lambda: FixedNoise(None, readout=(0.03, 0.11), seed=7),
    "readout1": lambda: FixedNoise(0.0, readout=(1.0, 1.0)),
}


# (noise, mixed X/Y/Z groups?): readout noise and lambda = 1 take the Z-only observables, lambda = 0 the mixed ones, the rest both
GRID_COMBOS = (("ideal", False), ("ideal", True), ("depol0", True), ("depol", False), ("depol", True), ("depol1", False),
               ("readout0", False), ("readout", False), ("readout1", False))
# the seed of every grid run; cleared on the CPU (test_clifford_frames_cpu.py::test_the_seeds_of_the_grid_are_cleared records the
# worst sigma): every term of the grid then meets the five-sigma condition, on the host and -- by bit-equality -- on the device
GRID_SEED = 2024


def grid_case(n, mixed, seed=0):
    """(circuit, terms) of one grid entry: a random local Clifford program over the full gate list, and six terms of weight at most
    3 -- Z-only, or over X, Y, Z (several measurement groups) -- with the identity term."""
    circuit = cc.random_clifford_program(n, min(2 * n, 40) + 8, seed + n, measure=True, local=4)
    terms = cc.random_terms(n, 6, seed + 3 * n, alphabet="IXYZ" if mixed else "IZ", weight=3)
    return circuit, terms + [("I" * n, 0.125)]


@functools.lru_cache(maxsize=None)
def grid_batch(kind, mixed):
    """``(circuits, observables, noise, FrameBatch, exact term values)`` of one (noise, observables) combination: one circuit per
    width of GRID_N.  Computed once and shared; nothing modifies it."""
    from blackwater import sim

    cases = [grid_case(n, mixed) for n in GRID_N]
    circuits, observables = [c for c, _ in cases], [t for _, t in cases]
    noise = GRID_NOISE[kind]()
    batch = sim.compile_clifford_frames(circuits, observables, noise)
    return circuits, observables, noise, batch, exact_terms(circuits, observables, noise)


@functools.lru_cache(maxsize=None)
def grid_oracle(kind, mixed, shots):
    """The interpreter's result of one grid batch at ``shots``, with GRID_SEED and the default run keys."""
    return interpret(grid_batch(kind, mixed)[3], shots, GRID_SEED)


def threshold_fraction(lam):
    return int(Fraction(float(lam)) * 2 ** 60)
