"""Oracles, the derived tolerance and the case builders shared by tests/test_clifford_cpu.py and tests/test_gpu_clifford.py (no test
in here).  Builds on tests/sim_cases.py and leaves it alone.

(a) ``interpret``: the record format of mlqem_clifford_run_f64 followed on the host, record by record as include/mlqem_hip.h words
    it (Python integers for the Pauli words, one rounded float64 product per depolarising record, separate products and sums in the
    combine step).  The device must equal it to the last bit.
(b) ``sim_cases.simulate``: the state-vector / density-matrix oracle, for n <= 5 with noise and n <= 11 without.
(c) ``tableau_values``: a forward stabilizer tableau (Aaronson, Gottesman 2004) in numpy.  It shares nothing with the package: gates
    are decomposed BY NAME into h, s and cx (``generators``), the state is propagated forwards and a Pauli's value is read off the
    stabilizer group.  Ideal values at any width; they are exactly -1, 0 or +1.
(d) ``BlockCircuit``: disjoint blocks of at most 4 qubits placed anywhere in a wide register (across the word boundaries 31|32 and
    63|64 among others).  The state is a product over the blocks and the noise acts inside them, so a term's value is the product of
    ``simulate``'s values of the blocks it touches, noise included.

Tolerance for noisy values (derived; u = 2^-53).  The kernel's unit value is +-1 times a product of K rounded factors keep = 1 -
lambda (each within u of its real value, each product rounded once): relative error at most (2 K) u to first order; the readout
weight is a product of at most m <= K' rounded factors and the combine step adds one rounded product and sum per sub-unit.  With K
counting every depolarising record of the circuit plus the readout factors of the term this is within (K + 2) u |value| per unit (the
device's side; half the count is slack).  The oracle's side is ``sim_cases.term_bound`` of every block the term touches, plus u
per block for the product over the blocks.  ``noisy_bound`` adds these up; the suites assert that it stays below ``sim_cases.CAP``.
"""
import math

import numpy as np

import sim_cases
from sim_cases import U

# ---- (a) the record format on the host --------------------------------------------------------------------------------------------
REG_QUBITS, MAX_QUBITS = 128, 512
C1, C2, DEPOL1, DEPOL2 = range(4)


def _clamp(v, lo, hi):
    return min(max(int(v), lo), hi)


def interpret_unit(batch, u):
    """(ideal, noisy) of unit ``u``: the walk of include/mlqem_hip.h."""
    c, mask, _, _ = (int(v) for v in batch.units[u])
    c = _clamp(c, 0, len(batch.n_qubits) - 1)
    n = _clamp(batch.n_qubits[c], 1, REG_QUBITS if u < batch.n_reg else MAX_QUBITS)
    w = (n + 31) // 32
    n_masks = len(batch.masks)
    x = sum(int(batch.masks[_clamp(mask + j, 0, n_masks - 1)]) << (32 * j) for j in range(w))
    z = sum(int(batch.masks[_clamp(mask + w + j, 0, n_masks - 1)]) << (32 * j) for j in range(w))
    sign, factor = 0, np.float64(1.0)
    n_ops = len(batch.ops)
    ob = _clamp(batch.op_ptr[c], 0, n_ops)
    oe = _clamp(batch.op_ptr[c + 1], ob, n_ops)

    def letter(q):
        return (x >> q & 1) | (z >> q & 1) << 1

    for k in range(oe - 1, ob - 1, -1):
        head, a, b, cc = (int(v) for v in batch.ops[k])
        kind, q0, q1 = head & 15, min(head >> 4 & 1023, n - 1), min(head >> 14 & 1023, n - 1)
        l0 = letter(q0)
        l1 = letter(q1) if kind in (C2, DEPOL2) else 0
        p = l0 | l1 << 2
        if kind == C1 and l0:
            img = a >> (3 * (l0 - 1)) & 7
            sign ^= img >> 2
            x = x & ~(1 << q0) | (img & 1) << q0
            z = z & ~(1 << q0) | (img >> 1 & 1) << q0
        elif kind == C2 and p:
            e = p - 1
            img = (a | b << 32) >> (4 * e) & 15
            sign ^= cc >> e & 1
            for q, l in ((q0, img & 3), (q1, img >> 2)):
                x = x & ~(1 << q) | (l & 1) << q
                z = z & ~(1 << q) | (l >> 1) << q
        elif kind in (DEPOL1, DEPOL2) and p:
            index = a - (1 << 32) if a >= 1 << 31 else a   # the kernel reads the word as an int32
            factor = factor * np.float64(batch.pool[_clamp(index, 0, len(batch.pool) - 1)])
    ideal = np.float64(0.0 if x else (-1.0 if sign else 1.0))
    return ideal, ideal * factor


def interpret(batch):
    """``(ideal_values, noisy_values, ideal_terms, noisy_terms, unit_ideal, unit_noisy)`` of a ``CliffordBatch``, float64 arrays."""
    n_units = len(batch.units)
    ui, un = np.zeros(n_units), np.zeros(n_units)
    for u in range(n_units):
        ui[u], un[u] = interpret_unit(batch, u)
    n_terms = len(batch.coeff)
    ti, tn = np.zeros(n_terms), np.zeros(n_terms)
    for t in range(n_terms):
        si = sn = np.float64(0.0)
        for j in range(int(batch.comb_ptr[t]), int(batch.comb_ptr[t + 1])):
            uu = _clamp(batch.comb_unit[j], 0, n_units - 1)
            si = si + batch.comb_weight[j, 0] * ui[uu]
            sn = sn + batch.comb_weight[j, 1] * un[uu]
        ti[t], tn[t] = si, sn
    b = len(batch.n_qubits)
    vi, vn = np.zeros(b), np.zeros(b)
    for c in range(b):
        si = sn = np.float64(0.0)
        for t in range(int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])):
            si = si + batch.coeff[t] * ti[t]
            sn = sn + batch.coeff[t] * tn[t]
        vi[c], vn[c] = si, sn
    return vi, vn, ti, tn, ui, un


# ---- (c) the forward stabilizer tableau ---------------------------------------------------------------------------------------------
def _quarter_turns(angle, name):
    k = angle / (math.pi / 2)
    if abs(k - round(k)) > 1e-9:
        raise ValueError(f"{name}({angle}) is not a Clifford gate")
    return int(round(k)) % 4


def generators(name, qubits, params=()):
    """``[("h" | "s" | "cx", qubits)]`` in the order they act, equal to the gate up to a global phase.  From the gates' textbook
    identities: Z = S^2, X = H Z H, sqrt X = H S H, Rz(k pi / 2) ~ S^k, Rx = H Rz H, Ry = S Rx S^dagger, U3(t, p, l) ~ Rz(p) Ry(t) Rz(l),
    CZ = H_t CX H_t, SWAP = three CX, Rzz = CX Rz_t CX, and ECR ~ X_c . CX . (S_c, sqrt X_t)."""
    q = qubits[0]
    s = lambda k, qq=q: [("s", (qq,))] * (k % 4)
    rz = lambda ang, qq=q: s(_quarter_turns(ang, name), qq)
    rx = lambda ang, qq=q: [("h", (qq,))] + rz(ang, qq) + [("h", (qq,))]
    ry = lambda ang, qq=q: s(3, qq) + rx(ang, qq) + s(1, qq)
    if name == "id":
        return []
    if name == "h":
        return [("h", (q,))]
    if name in ("s", "sdg", "z"):
        return s({"s": 1, "z": 2, "sdg": 3}[name])
    if name == "x":
        return rx(math.pi)
    if name == "y":
        return s(2) + rx(math.pi)
    if name in ("sx", "sxdg"):
        return rx(math.pi / 2 if name == "sx" else -math.pi / 2)
    if name in ("rz", "p", "u1"):
        return rz(params[0])
    if name == "rx":
        return rx(params[0])
    if name == "ry":
        return ry(params[0])
    if name == "u2":
        return rz(params[1]) + ry(math.pi / 2) + rz(params[0])
    if name in ("u3", "u"):
        return rz(params[2]) + ry(params[0]) + rz(params[1])
    a, b = qubits
    if name == "cx":
        return [("cx", (a, b))]
    if name == "cz":
        return [("h", (b,)), ("cx", (a, b)), ("h", (b,))]
    if name == "swap":
        return [("cx", (a, b)), ("cx", (b, a)), ("cx", (a, b))]
    if name == "rzz":
        return [("cx", (a, b))] + rz(params[0], b) + [("cx", (a, b))]
    if name == "ecr":
        return s(1, a) + rx(math.pi / 2, b) + [("cx", (a, b))] + rx(math.pi, a)
    raise ValueError(f"{name} is not a Clifford gate")   # t, tdg and anything unknown


class Tableau:
    """Aaronson-Gottesman: rows 0 .. n - 1 destabilizers, n .. 2n - 1 stabilizers of the state, starting from |0..0>."""

    def __init__(self, n):
        self.n = n
        self.x = np.zeros((2 * n, n), dtype=np.uint8)
        self.z = np.zeros((2 * n, n), dtype=np.uint8)
        self.r = np.zeros(2 * n, dtype=np.uint8)
        self.x[np.arange(n), np.arange(n)] = 1
        self.z[n + np.arange(n), np.arange(n)] = 1

    def apply(self, kind, qubits):
        x, z, r = self.x, self.z, self.r
        if kind == "h":
            a = qubits[0]
            r ^= x[:, a] & z[:, a]
            x[:, a], z[:, a] = z[:, a].copy(), x[:, a].copy()
        elif kind == "s":
            a = qubits[0]
            r ^= x[:, a] & z[:, a]
            z[:, a] ^= x[:, a]
        else:
            a, b = qubits
            r ^= x[:, a] & z[:, b] & (x[:, b] ^ z[:, a] ^ 1)
            x[:, b] ^= x[:, a]
            z[:, a] ^= z[:, b]

    def run(self, circuit):
        for op in circuit.ops:
            if op.name in ("barrier", "measure"):
                continue
            for kind, qs in generators(op.name, tuple(op.qubits), tuple(op.params)):
                self.apply(kind, qs)
        return self

    def expectation(self, label):
        """<P> for a Pauli label (rightmost character on qubit 0): -1, 0 or +1."""
        n = self.n
        px = np.array([ch in "XY" for ch in reversed(label)], dtype=np.uint8)
        pz = np.array([ch in "ZY" for ch in reversed(label)], dtype=np.uint8)
        anti = (self.x.astype(np.int64) @ pz + self.z.astype(np.int64) @ px) % 2   # row i anticommutes with P
        if anti[n:].any():
            return 0.0
        ax, az, phase = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), 0   # the product so far is i^phase * (ax, az)
        for i in np.flatnonzero(anti[:n]):
            sx, sz = self.x[n + i].astype(np.int64), self.z[n + i].astype(np.int64)
            # exponent of i picked up when the Pauli (ax, az) is multiplied by (sx, sz), letter by letter (Hermitian Y)
            g = np.where((ax == 1) & (az == 1), sz - sx, np.where((ax == 1) & (az == 0), sz * (2 * sx - 1),
                         np.where((ax == 0) & (az == 1), sx * (1 - 2 * sz), 0)))
            phase = (phase + 2 * int(self.r[n + i]) + int(g.sum())) % 4
            ax, az = ax ^ sx, az ^ sz
        assert (ax == px).all() and (az == pz).all() and phase in (0, 2), "a Pauli that commutes with the group is in it, up to a sign"
        return 1.0 if phase == 0 else -1.0


    def stabilizer_label(self, rows):
        """The letters of the product of the stabilizer generators ``rows`` (its sign is left to ``expectation``): a Pauli whose value
        is +-1, which a random label of a deep circuit almost never is."""
        x = np.bitwise_xor.reduce(self.x[self.n + np.asarray(rows)], axis=0)
        z = np.bitwise_xor.reduce(self.z[self.n + np.asarray(rows)], axis=0)
        return "".join("IXZY"[int(a) | int(b) << 1] for a, b in zip(x[::-1], z[::-1]))


def stabilizer_terms(circuit, count, seed, max_rows=3):
    """``count`` terms whose ideal value is +-1: products of one to ``max_rows`` random stabilizer generators of the circuit's state."""
    t = Tableau(circuit.num_qubits).run(circuit)
    rng = np.random.default_rng([circuit.num_qubits, count, seed, 81])
    out = []
    for _ in range(count):
        rows = rng.choice(t.n, size=int(rng.integers(1, min(max_rows, t.n) + 1)), replace=False)
        out.append((t.stabilizer_label(rows), float(rng.uniform(-0.25, 0.25))))
    return out


def tableau_values(circuit, labels):
    t = Tableau(circuit.num_qubits).run(circuit)
    return np.array([t.expectation(label) for label in labels], dtype=np.float64)


# ---- case builders ------------------------------------------------------------------------------------------------------------------
CLIFFORD_ONE = ["id", "x", "y", "z", "h", "s", "sdg", "sx", "sxdg", "rx", "ry", "rz", "p", "u1", "u2", "u3", "u"]
CLIFFORD_TWO = ["cx", "cz", "swap", "ecr", "rzz"]
CLASSICAL = ["id", "x", "z", "s", "sdg", "cx", "swap", "cz"]   # basis states stay basis states: every Z string has a value of +-1


def random_clifford_op(rng, qubits_pool, names=None):
    """One random gate over the full gate list (or ``names``), every angle a multiple of pi / 2 in [-2 pi, 2 pi]."""
    from blackwater.data.circuit import CircuitOp

    one = [g for g in CLIFFORD_ONE if names is None or g in names]
    two = [g for g in CLIFFORD_TWO if names is None or g in names]
    if len(qubits_pool) >= 2 and two and rng.random() < 0.4:
        name = two[int(rng.integers(0, len(two)))]
        qubits = tuple(int(q) for q in rng.choice(qubits_pool, size=2, replace=False))
    else:
        name = one[int(rng.integers(0, len(one)))]
        qubits = (int(qubits_pool[int(rng.integers(0, len(qubits_pool)))]),)
    params = tuple(float(k) * math.pi / 2 for k in rng.integers(-4, 5, size=sim_cases.N_PARAMS.get(name, 0)))
    return CircuitOp(name, qubits, (), params)


def random_clifford_program(n, n_ops, seed, measure=False, local=None):
    """``n_ops`` random Clifford gates on ``n`` qubits; ``local``: two-qubit gates only between qubits at most that far apart."""
    from blackwater.data.circuit import Circuit, CircuitOp

    rng = np.random.default_rng([n, n_ops, seed, 77])
    ops = []
    for _ in range(n_ops):
        if local is None:
            pool = np.arange(n)
        else:
            lo = int(rng.integers(0, n))
            pool = np.arange(lo, min(n, lo + local + 1))
        ops.append(random_clifford_op(rng, pool))
    if measure:
        ops += [CircuitOp("measure", (q,), (q,)) for q in range(n)]
    return Circuit(n, n if measure else 0, ops)


def random_terms(n, count, seed, alphabet="IXYZ", weight=None):
    """``count`` random labels with coefficients in [-0.25, 0.25]; ``weight``: at most that many non-identity letters."""
    rng = np.random.default_rng([n, count, seed, 78])
    out = []
    for _ in range(count):
        if weight is None:
            label = sim_cases.random_label(rng, n, alphabet)
        else:
            chars = ["I"] * n
            for q in rng.choice(n, size=min(weight, n), replace=False):
                chars[n - 1 - int(q)] = alphabet[int(rng.integers(1, len(alphabet)))]
            label = "".join(chars)
        out.append((label, float(rng.uniform(-0.25, 0.25))))
    return out


# ---- (d) blocks in a wide register --------------------------------------------------------------------------------------------------
class _BlockNoise:
    """The wide circuit's noise as one block sees it: op indices and qubits mapped back to the wide circuit."""

    def __init__(self, noise, op_index, qubits):
        self._noise, self._op_index, self._qubits = noise, op_index, qubits
        self.has_readout = getattr(noise, "has_readout", False)

    def after_gate(self, index, name, qubits):
        return self._noise.after_gate(self._op_index[index], name, tuple(self._qubits[q] for q in qubits))

    def readout_of(self, qubit):
        return self._noise.readout_of(self._qubits[qubit])


class BlockCircuit:
    """Random Clifford gates inside disjoint blocks (``positions``: a list of qubit lists, at most 4 qubits each) of an ``n``-qubit
    register, the blocks' ops interleaved at random.  ``wide`` is the circuit; ``block_values`` evaluates terms with oracle (b)."""

    def __init__(self, n, positions, ops_per_block, seed, measure=True, names=None):
        from blackwater.data.circuit import Circuit, CircuitOp

        assert all(len(p) <= 4 for p in positions) and len({q for p in positions for q in p}) == sum(len(p) for p in positions)
        rng = np.random.default_rng([n, len(positions), ops_per_block, seed, 79])
        self.n, self.positions = n, [list(p) for p in positions]
        which = rng.permutation(np.repeat(np.arange(len(positions)), ops_per_block))
        wide_ops, self.block_ops, self.block_index = [], [[] for _ in positions], [[] for _ in positions]
        for b in which.tolist():
            local = random_clifford_op(rng, np.arange(len(positions[b])), names)
            self.block_index[b].append(len(wide_ops))
            self.block_ops[b].append(local)
            wide_ops.append(CircuitOp(local.name, tuple(positions[b][q] for q in local.qubits), (), local.params))
        self.measured = bool(measure)
        if measure:
            wide_ops += [CircuitOp("measure", (q,), (q,)) for p in positions for q in p]
        self.wide = Circuit(n, n if measure else 0, wide_ops)

    def block_circuit(self, b):
        from blackwater.data.circuit import Circuit, CircuitOp

        k = len(self.positions[b])
        ops = list(self.block_ops[b]) + ([CircuitOp("measure", (q,), (q,)) for q in range(k)] if self.measured else [])
        return Circuit(k, k if self.measured else 0, ops)

    def block_noise(self, b, noise):
        return None if noise is None else _BlockNoise(noise, self.block_index[b], self.positions[b])

    def random_terms(self, count, seed, alphabet="IXYZ"):
        """Labels over the blocks' qubits only (identity elsewhere), each touching one to three blocks."""
        rng = np.random.default_rng([self.n, count, seed, 80])
        out = []
        for _ in range(count):
            chars = ["I"] * self.n
            for b in rng.choice(len(self.positions), size=int(rng.integers(1, min(3, len(self.positions)) + 1)), replace=False):
                for q in self.positions[int(b)]:
                    chars[self.n - 1 - q] = alphabet[int(rng.integers(0, len(alphabet)))]
            out.append(("".join(chars), float(rng.uniform(-0.25, 0.25))))
        return out

    def stabilizer_terms(self, count, seed):
        """Labels whose ideal value is +-1: on one to three blocks, a product of the block state's stabilizer generators."""
        rng = np.random.default_rng([self.n, count, seed, 82])
        tabs = [Tableau(len(p)).run(self.block_circuit(b)) for b, p in enumerate(self.positions)]
        out = []
        for _ in range(count):
            chars = ["I"] * self.n
            for b in rng.choice(len(self.positions), size=int(rng.integers(1, min(3, len(self.positions)) + 1)), replace=False):
                k = len(self.positions[int(b)])
                local = tabs[int(b)].stabilizer_label(rng.choice(k, size=int(rng.integers(1, k + 1)), replace=False))
                for j, q in enumerate(self.positions[int(b)]):
                    chars[self.n - 1 - q] = local[k - 1 - j]
            out.append(("".join(chars), float(rng.uniform(-0.25, 0.25))))
        return out

    def term_values(self, terms, noise=None):
        """``(values, oracle bounds)`` per term: the product over the touched blocks of ``simulate``'s value, and the sum of the blocks'
        ``sim_cases.term_bound`` plus u per block."""
        values, bounds = [], []
        cache = {}
        for label, _ in terms:
            v, bound = 1.0, 0.0
            for b, pos in enumerate(self.positions):
                local = "".join(label[self.n - 1 - q] for q in reversed(pos))
                if set(local) == {"I"}:
                    continue
                if (b, local) not in cache:
                    circ, bn = self.block_circuit(b), self.block_noise(b, noise)
                    cache[(b, local)] = (sim_cases.simulate(circ, [(local, 1.0)], bn)[1][0], sim_cases.term_bound(circ, bn))
                bv, bb = cache[(b, local)]
                v, bound = v * bv, bound + bb + U
            values.append(v)
            bounds.append(bound)
        return np.asarray(values), np.asarray(bounds)


# block positions per width: across the words 31|32, 63|64, 127|128, 255|256 and around the register's ends
BLOCKS = {100: [[30, 31, 32, 33], [62, 63, 64, 65], [0, 1, 2], [99, 5, 40]],
          129: [[31, 32], [63, 64, 127, 128], [0], [95, 96, 97]],
          512: [[510, 511, 0, 1], [255, 256], [30, 31, 32, 33], [479, 480, 481], [62, 63, 64, 65]]}


def depol_count(batch, c):
    """The number of depolarising records of circuit ``c``: an upper bound on the factors of a unit's product."""
    kinds = batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1]), 0] & 15
    return int(np.isin(kinds, (DEPOL1, DEPOL2)).sum())


def noisy_bound(batch, c, value, oracle_bound, readout_factors=0):
    """|device - oracle| allowed for a noisy term value of circuit ``c``: (K + 2) u |value| + the oracle's own bound (module docstring)."""
    return (depol_count(batch, c) + readout_factors + 2) * U * abs(value) + oracle_bound


# ---- the quality experiment (recorded) ---------------------------------------------------------------------------------------------
def quality_corpus(nq=100):
    """64 ``clifford_tfim_circuit`` circuits (steps 1 .. 4, kx and kz 0 .. 3), four single-Z terms each on qubits that move with the
    circuit, the ``synthetic_backend`` noise model, and a seeded 40 / 24 split: ``(circuits, observables, noise, train, val)``."""
    from blackwater import sim
    from blackwater.data.synthetic import clifford_tfim_circuit, synthetic_backend

    circuits = [clifford_tfim_circuit(nq, s, kx, kz) for s in (1, 2, 3, 4) for kx in range(4) for kz in range(4)]
    obs = [[("".join("Z" if q == (7 * j + 13 * k) % nq else "I" for q in reversed(range(nq))), 1.0) for j in range(4)]
           for k in range(len(circuits))]
    perm = np.random.default_rng(0).permutation(len(circuits))
    return circuits, obs, sim.NoiseModel.from_backend(synthetic_backend(nq, "ecr")), np.sort(perm[:40]), np.sort(perm[40:])


def quality_rows(circuits, noisy):
    """The ``encode_data_v2_ecr`` rows of the corpus (through the native encoder: the rows are the same, it is only faster)."""
    from blackwater.data.circuit import circuit_to_qasm
    from blackwater.library.learning.features import encode_data_v2_ecr

    return encode_data_v2_ecr([circuit_to_qasm(c) for c in circuits], np.zeros_like(noisy).tolist(), noisy.tolist(), 4, native=True)[0]


def quality_ratio(x, ideal, noisy, train, val, fit_predict):
    """(unmitigated, mitigated) mean L2 on the validation split; ``fit_predict(x_train, y_train, x_val)`` is the regressor."""
    l2 = lambda a, b: float(np.mean(np.linalg.norm(a - b, axis=1)))
    pred = fit_predict(x[train], ideal[train], x[val])
    return l2(noisy[val], ideal[val]), l2(pred, ideal[val])
