"""The numpy-fp64 oracle, the derived tolerance and the case builders shared by tests/test_sim_cpu.py and tests/test_gpu_sim.py
(no test in here).

Oracle.  Written independently of ``blackwater.sim``'s lowering: it walks the circuit IR (``Circuit.ops``), builds its own matrices
from gate names out of Pauli algebra (rz = cos - i sin Z, cx = P0 (x) I + P1 (x) X, ecr = (IX - XY) / sqrt 2, ...), applies them to a
state vector with ``tensordot`` and to a density matrix as rho -> U rho U^dagger with the full 2^n x 2^n U.  Depolarising is the KRAUS
form, rho -> (1 - lam) rho + lam / d^2 sum_P P rho P over the d^2 Pauli strings on the gate's qubits (the kernel uses the closed
form: two routes to one map).  Readout is the column-stochastic matrix on the marginal distribution diag(rho).  The noise SPEC is
shared with the package (an object with ``after_gate(index, name, qubits)`` and ``readout_of(qubit)``); nothing else is.

Tolerance (derived, not tuned; u = 2^-53).  Both sides apply each op with a handful of rounded operations per entry, and every
op is norm-preserving or a contraction on the vector it acts on (psi in the 2-norm, rho in the Frobenius norm), so the error of
the state grows by at most  cost(op) * u * |state|  per op and per side, |state| <= 1:
  cost 12  a general one-qubit matrix: an entry is a real dot product of length 4 (4 u), re and im (sqrt 2), two entries of a pair
           (sqrt 2): 8 u, plus 4 u for the rounded matrix entries (cos, sin and exp are within an ulp);
  cost 32  a 4 x 4 matrix: dot products of length 8, four entries of a group: 8 sqrt 2 * 2 < 23 u, plus 8 u for its entries;
  cost 6   a diagonal gate: one complex product (2 sqrt 2 u) and its rounded phase (2 u); cost 0 for cx, cz, swap, id (exact);
  cost 20  a depolarising op (the oracle adds 16 terms with rounded weights; the kernel's closed form is cheaper); cost 8 readout.
In density mode a unitary acts twice (U on the rows, conj U on the columns): twice its cost.  The full-matrix products of the
oracle add only exact zeros to these sums, so the same costs hold for it.
An expectation value is bilinear in psi (|d<P>| <= 2 |d psi|) and linear in rho with |Tr(P d rho)| <= |P|_F |d rho|_F =
2^(n/2) |d rho|_F; the sum itself has N = 2^n addends of total magnitude <= 1, worth at most N u on the oracle's side (any order)
and (N / 64 + 12) u on the device's (lane-strided partials, a shuffle tree, four waves), plus 4 u for the products:
  term_bound = u * (2 sides * S * sum_ops cost + N + N / 64 + 16),   S = 2 (vector) or 2^(n/2) (density)
  value_bound = sum|coeff| * term_bound + (T + 2) u sum|coeff|       (T rounded products and additions)
``term_bound`` / ``value_bound`` evaluate this on the circuit at hand; every case of the suites asserts that they stay below 1e-11.
"""
import functools
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
CAP = 1e-11

I2 = np.eye(2, dtype=complex)
X = np.array([[0, 1], [1, 0]], dtype=complex)
Y = np.array([[0, -1j], [1j, 0]], dtype=complex)
Z = np.array([[1, 0], [0, -1]], dtype=complex)
P0 = np.array([[1, 0], [0, 0]], dtype=complex)
P1 = np.array([[0, 0], [0, 1]], dtype=complex)
PAULI = {"I": I2, "X": X, "Y": Y, "Z": Z}

ONE_QUBIT = ["id", "x", "y", "z", "h", "s", "sdg", "t", "tdg", "sx", "sxdg", "rx", "ry", "rz", "p", "u1", "u2", "u3", "u"]
TWO_QUBIT = ["cx", "cz", "swap", "ecr", "rzz"]
N_PARAMS = {"rx": 1, "ry": 1, "rz": 1, "p": 1, "u1": 1, "u2": 2, "u3": 3, "u": 3, "rzz": 1}


def _rot(axis, theta):
    return math.cos(theta / 2) * I2 - 1j * math.sin(theta / 2) * axis


def _phase(lam):
    return P0 + np.exp(1j * lam) * P1


def _u3(theta, phi, lam):
    return np.exp(0.5j * (phi + lam)) * (_rot(Z, phi) @ _rot(Y, theta) @ _rot(Z, lam))


def kron2(on_q1, on_q0):
    """A two-qubit operator over the basis index bit(q0) + 2 bit(q1)."""
    return np.kron(on_q1, on_q0)


def gate_matrix(name, params=()):
    p = [float(v) for v in params]
    if name == "id":
        return I2
    if name in ("x", "y", "z"):
        return PAULI[name.upper()]
    if name == "h":
        return (X + Z) / math.sqrt(2)
    if name == "s":
        return _phase(math.pi / 2)
    if name == "sdg":
        return _phase(-math.pi / 2)
    if name == "t":
        return _phase(math.pi / 4)
    if name == "tdg":
        return _phase(-math.pi / 4)
    if name == "sx":
        return np.exp(0.25j * math.pi) * _rot(X, math.pi / 2)
    if name == "sxdg":
        return np.exp(-0.25j * math.pi) * _rot(X, -math.pi / 2)
    if name == "rx":
        return _rot(X, p[0])
    if name == "ry":
        return _rot(Y, p[0])
    if name == "rz":
        return _rot(Z, p[0])
    if name in ("p", "u1"):
        return _phase(p[0])
    if name == "u2":
        return _u3(math.pi / 2, p[0], p[1])
    if name in ("u3", "u"):
        return _u3(p[0], p[1], p[2])
    if name == "cx":   # q0 controls
        return kron2(I2, P0) + kron2(X, P1)
    if name == "cz":
        return kron2(I2, P0) + kron2(Z, P1)
    if name == "swap":
        return 0.5 * (kron2(I2, I2) + kron2(X, X) + kron2(Y, Y) + kron2(Z, Z))
    if name == "ecr":
        return (kron2(I2, X) - kron2(X, Y)) / math.sqrt(2)
    if name == "rzz":
        return math.cos(p[0] / 2) * kron2(I2, I2) - 1j * math.sin(p[0] / 2) * kron2(Z, Z)
    raise KeyError(name)


def apply(mat, qubits, state, n):
    """``mat`` on ``qubits`` of a state [2^n, ...] (trailing axes ride along): tensordot over the qubits' axes."""
    tail = state.shape[1:]
    t = state.reshape((2,) * n + tail)
    k = len(qubits)
    axes = [n - 1 - q for q in reversed(qubits)]          # the matrix index is bit(q0) + 2 bit(q1): q1 is the slow axis
    m = np.asarray(mat, dtype=complex).reshape((2,) * (2 * k))
    t = np.tensordot(m, t, axes=(list(range(k, 2 * k)), axes))
    t = np.moveaxis(t, list(range(k)), axes)
    return t.reshape((2 ** n,) + tail)


def full_unitary(mat, qubits, n):
    return apply(mat, qubits, np.eye(2 ** n, dtype=complex), n)


def pauli_apply(label, state, n):
    """The Pauli string ``label`` (rightmost character on qubit 0) applied to a state [2^n, ...]."""
    for q, ch in enumerate(reversed(label)):
        if ch != "I":
            state = apply(PAULI[ch], [q], state, n)
    return state


@functools.lru_cache(maxsize=4096)
def pauli_matrix(label):
    """The full 2^n x 2^n matrix of a Pauli string (kept: the Kraus sums of a batch use the same few strings again and again)."""
    n = len(label)
    return pauli_apply(label, np.eye(2 ** n, dtype=complex), n)


def _kraus_depolarise(rho, qubits, lam, n):
    d2 = 4 ** len(qubits)
    acc = np.zeros_like(rho)
    for code in range(d2):
        label = ["I"] * n
        for j, q in enumerate(qubits):
            label[n - 1 - q] = "IXYZ"[(code >> (2 * j)) & 3]
        p = pauli_matrix("".join(label))
        acc = acc + p @ rho @ p.conj().T
    return (1.0 - lam) * rho + (lam / d2) * acc


def simulate(circuit, terms, noise=None):
    """``(value, term_values, norm)`` of one circuit (a ``blackwater`` Circuit) and its Pauli terms ``[(label, coeff)]``.
    ``noise=None``: a state vector.  Otherwise a density matrix with ``noise.after_gate`` / ``noise.readout_of`` applied."""
    n = circuit.num_qubits
    density = noise is not None
    psi = np.zeros(2 ** n, dtype=complex)
    psi[0] = 1.0
    rho = np.outer(psi, psi.conj()) if density else None
    measured = []
    for i, op in enumerate(circuit.ops):
        if op.name == "barrier":
            continue
        if op.name == "measure":
            measured.append(op.qubits[0])
            continue
        mat, qs = gate_matrix(op.name, op.params), list(op.qubits)
        if density:
            if op.name != "id":
                u = full_unitary(mat, qs, n)
                rho = u @ rho @ u.conj().T
            lam = noise.after_gate(i, op.name, tuple(circuit.qubit_reg_index[q] for q in qs))
            if lam is not None:
                rho = _kraus_depolarise(rho, qs, lam, n)
        elif op.name != "id":
            psi = apply(mat, qs, psi, n)
    if density:
        norm = float(np.trace(rho).real)
        readouts = [(q, noise.readout_of(circuit.qubit_reg_index[q])) for q in sorted(set(measured))]
        readouts = [(q, pr) for q, pr in readouts if pr is not None]
        if readouts:   # only the marginal distribution is meaningful from here on: I/Z terms only
            probs = np.diag(rho).real.copy()
            for q, (p01, p10) in readouts:
                probs = apply(np.array([[1 - p10, p01], [p10, 1 - p01]]), [q], probs.astype(complex), n).real
            tv = []
            for label, _ in terms:
                assert set(label) <= {"I", "Z"}, label
                signs = pauli_apply(label, np.ones(2 ** n, dtype=complex), n).real
                tv.append(float(np.sum(signs * probs)))
        else:
            tv = [float(np.trace(pauli_apply(label, rho, n)).real) for label, _ in terms]
    else:
        norm = float(np.vdot(psi, psi).real)
        tv = [float(np.vdot(psi, pauli_apply(label, psi, n)).real) for label, _ in terms]
    value = 0.0
    for (_, c), t in zip(terms, tv):
        value = value + float(np.real(c)) * t
    return value, np.asarray(tv, dtype=np.float64), norm


def oracle_expectation_values(circuits, observables, noise=None, device=None):
    """Drop-in for ``blackwater.sim.expectation_values`` on the host: numpy arrays ``(values, term_values, term_ptr)``."""
    from blackwater.data.backends import pauli_terms
    from blackwater.data.circuit import Circuit

    values, tvs, ptr = [], [], [0]
    for c, o in zip(circuits, observables):
        v, tv, _ = simulate(Circuit.from_any(c), pauli_terms(o), noise)
        values.append(v)
        tvs.append(tv)
        ptr.append(ptr[-1] + len(tv))
    return np.asarray(values), (np.concatenate(tvs) if tvs else np.zeros(0)), np.asarray(ptr, dtype=np.int64)


# ---- tolerance ---------------------------------------------------------------------------------------------------------------------
_COST = {"id": 0, "cx": 0, "cz": 0, "swap": 0, "ecr": 32, "rzz": 32}
_COST.update({g: 6 for g in ("z", "s", "sdg", "t", "tdg", "rz", "p", "u1")})
COST_DEPOL, COST_READOUT = 20, 8


def op_cost_sum(circuit, noise=None):
    """sum over the circuit's ops of the per-op cost of the module docstring (density mode: unitaries twice, plus the noise ops)."""
    total, measured = 0, set()
    for i, op in enumerate(circuit.ops):
        if op.name == "barrier":
            continue
        if op.name == "measure":
            measured.add(op.qubits[0])
            continue
        cost = _COST.get(op.name, 12)
        total += 2 * cost if noise is not None else cost
        if noise is not None and noise.after_gate(i, op.name, tuple(circuit.qubit_reg_index[q] for q in op.qubits)) is not None:
            total += COST_DEPOL
    if noise is not None:
        total += COST_READOUT * sum(1 for q in measured if noise.readout_of(circuit.qubit_reg_index[q]) is not None)
    return total


def term_bound(circuit, noise=None):
    """|device - oracle| of one Pauli term's value: u (2 S sum cost + N + N / 64 + 16), see the module docstring."""
    n = circuit.num_qubits
    big_n = 2 ** n
    s = 2.0 if noise is None else math.sqrt(big_n)
    return U * (2 * s * op_cost_sum(circuit, noise) + big_n + big_n / 64 + 16)


def value_bound(circuit, terms, noise=None):
    total = sum(abs(float(np.real(c))) for _, c in terms)
    return total * term_bound(circuit, noise) + (len(terms) + 2) * U * total


# ---- cases -------------------------------------------------------------------------------------------------------------------------
class StepNoise:
    """A noise spec for the tests: a depolarising op after EVERY gate, lambda drawn per op index in [0, 0.2] with lambda = 0 and
    lambda = 1 forced once each; optional readout probabilities per qubit."""

    has_readout = False

    def __init__(self, seed, readout=None, force=True):
        self._rng_seed, self._lam, self._force = seed, {}, force
        self.readout = dict(readout or {})
        self.has_readout = bool(self.readout)

    def after_gate(self, index, name, qubits):
        if index not in self._lam:
            rng = np.random.default_rng([self._rng_seed, index])
            self._lam[index] = float(rng.uniform(0.0, 0.2))
            if self._force and index == 3:
                self._lam[index] = 0.0
            if self._force and index == 7:
                self._lam[index] = 1.0
        return self._lam[index]

    def readout_of(self, qubit):
        return self.readout.get(qubit)


class NoNoise:
    """Density-matrix mode without any noise op."""

    has_readout = False

    def after_gate(self, index, name, qubits):
        return None

    def readout_of(self, qubit):
        return None


def _random_op(rng, name, qubits):
    from blackwater.data.circuit import CircuitOp

    params = tuple(float(v) for v in rng.uniform(-2 * math.pi, 2 * math.pi, size=N_PARAMS.get(name, 0)))
    return CircuitOp(name, tuple(qubits), (), params)


def random_program(n, n_ops=40, seed=0, measure=False, with_id=True):
    """``n_ops`` random gates over the full gate list on ``n`` qubits.  Forced in: one-qubit gates on qubit 0 and on qubit n - 1, and
    two-qubit gates on (0, 1), (1, 0), (0, n - 1), (n - 1, 0) and a non-adjacent middle pair (where n allows them).  ``with_id=False``
    leaves ``id`` out, so that every gate lowers to a record."""
    from blackwater.data.circuit import Circuit, CircuitOp

    rng = np.random.default_rng([n, n_ops, seed])
    forced = [("h", (0,)), ("u3", (n - 1,)), ("sx", (0,)), ("ry", (n - 1,))]
    if n >= 2:
        pairs = [(0, 1), (1, 0), (0, n - 1), (n - 1, 0)]
        if n >= 4:
            pairs.append((1, n - 2) if n - 2 > 2 else (1, 3))
        seen = []
        for pr in pairs:
            if pr not in seen:
                seen.append(pr)
        for j, pr in enumerate(seen):
            forced.append((TWO_QUBIT[(j + seed) % len(TWO_QUBIT)], pr))
        forced += [("ecr", seen[-1]), ("rzz", seen[0]), ("cx", seen[1 % len(seen)]), ("swap", seen[-1]), ("cz", seen[0])]
    forced = forced[:n_ops]
    ops = []
    slots = set(rng.choice(n_ops, size=len(forced), replace=False).tolist()) if n_ops else set()
    it = iter(forced)
    for k in range(n_ops):
        if k in slots:
            name, qubits = next(it)
        elif n >= 2 and rng.random() < 0.3:
            name = TWO_QUBIT[int(rng.integers(0, len(TWO_QUBIT)))]
            qubits = tuple(int(q) for q in rng.choice(n, size=2, replace=False))
        else:
            name = ONE_QUBIT[int(rng.integers(0 if with_id else 1, len(ONE_QUBIT)))]
            qubits = (int(rng.integers(0, n)),)
        ops.append(_random_op(rng, name, qubits))
    if measure:
        ops += [CircuitOp("measure", (q,), (q,)) for q in range(n)]
    return Circuit(n, n if measure else 0, ops)


def random_label(rng, n, alphabet="IXYZ"):
    return "".join(alphabet[int(c)] for c in rng.integers(0, len(alphabet), size=n))


def term_set(n, seed=0, alphabet="IXYZ"):
    """12 terms: all-I, a label with X, Y and Z together (as far as n allows), a label with an odd number of Y, random ones.
    Coefficients in [-0.25, 0.25], so that sum|coeff| <= 3."""
    rng = np.random.default_rng([n, seed, 12])
    labels = ["I" * n]
    if alphabet == "IXYZ":
        mixed = (["X", "Y", "Z"] * n)[:n]
        labels.append("".join(mixed))
        odd = ["I"] * n
        odd[0] = "Y"
        if n >= 3:
            odd[1] = odd[2] = "Y"
        labels.append("".join(odd))
    else:
        labels.append("Z" * n)
    while len(labels) < 12:
        labels.append(random_label(rng, n, alphabet))
    return [(label, float(c)) for label, c in zip(labels, rng.uniform(-0.25, 0.25, size=len(labels)))]


def long_observable(n, seed=0, alphabet="IXYZ", size=40):
    """A ``size``-term observable with coefficients in [-0.05, 0.05] (sum|coeff| <= 2)."""
    rng = np.random.default_rng([n, seed, size])
    return [(random_label(rng, n, alphabet), float(c)) for c in rng.uniform(-0.05, 0.05, size=size)]


# ---- the reference anchor ----------------------------------------------------------------------------------------------------------
_GOLDEN_FILES = (("g1_circuits.json", "g1_dataset.npz"), ("ising_trainval_circuits.json", "ising_trainval.npz"))


def golden_circuits():
    """``(qasm texts, stored ideal [900, 4], split [900] (-1 for g1; the Ising file's own split otherwise))``."""
    texts, ideal, split = [], [], []
    for cj, dz in _GOLDEN_FILES:
        with open(os.path.join(GOLDEN, cj)) as fh:
            t = json.load(fh)
        z = np.load(os.path.join(GOLDEN, dz))
        texts += t
        ideal.append(np.asarray(z["ideal"], dtype=np.float64))
        split.append(np.asarray(z["split"], dtype=np.int64) if "split" in z.files else np.full(len(t), -1, dtype=np.int64))
    return texts, np.concatenate(ideal), np.concatenate(split)


def anchor_sigmas(measured_z_values, stored):
    """|stored - v| / sigma for v = -<Z> of classical bit 3 - k in column k, sigma = max(sqrt((1 - v^2) / 1e4), 1e-3).
    ``measured_z_values`` [B, 4]: <Z> per classical bit 0..3."""
    v = -np.asarray(measured_z_values, dtype=np.float64)[:, ::-1]
    sigma = np.maximum(np.sqrt(np.clip(1.0 - v * v, 0.0, None) / 1e4), 1e-3)
    return np.abs(np.asarray(stored) - v) / sigma


# ---- the program format, interpreted on the host -------------------------------------------------------------------------------------
def interpret(batch, c):
    """``(value, term_values, norm)`` of circuit ``c`` of a ``SimBatch``, following the contract of include/mlqem_hip.h record by
    record in numpy.  It checks the LOWERING (and the documented layout) without a GPU; the kernel is checked against the oracle."""
    n, mode, n_ro, _ = (int(v) for v in batch.circ[c])
    nb = 2 * n if mode else n
    size = 1 << nb
    st = np.zeros(size, dtype=complex)
    st[0] = 1.0
    idx = np.arange(size)
    ops = batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])]
    n_main = len(ops) - n_ro

    def bit(b):
        return (idx >> b) & 1

    def mat2(b, m):
        i0 = idx[bit(b) == 0]
        i1 = i0 | (1 << b)
        a0, a1 = st[i0].copy(), st[i1].copy()
        st[i0], st[i1] = m[0, 0] * a0 + m[0, 1] * a1, m[1, 0] * a0 + m[1, 1] * a1

    def mat4(a, b, m):
        base = idx[(bit(a) == 0) & (bit(b) == 0)]
        ii = [base | ((k & 1) << a) | ((k >> 1) << b) for k in range(4)]
        e = [st[i].copy() for i in ii]
        for r in range(4):
            st[ii[r]] = sum(m[r, cc] * e[cc] for cc in range(4))

    def cplx(po, count):
        v = batch.params[po:po + 2 * count]
        return v[0::2] + 1j * v[1::2]

    def trace():
        if mode:
            d = np.arange(1 << n)
            return float(st[d | (d << n)].real.sum())
        return float((st.real ** 2 + st.imag ** 2).sum())

    norm = None
    for k, (kind, q0, q1, po) in enumerate(ops.tolist()):
        if k == n_main:
            norm = trace()
        if kind == 0:
            m = cplx(po, 4).reshape(2, 2)
            mat2(q0, m)
            if mode:
                mat2(q0 + n, m.conj())
        elif kind == 1:
            d = cplx(po, 2)
            st *= d[bit(q0)]
            if mode:
                st *= d.conj()[bit(q0 + n)]
        elif kind in (2, 3, 4):
            m = {2: gate_matrix("cx"), 3: gate_matrix("cz"), 4: gate_matrix("swap")}[kind]
            mat4(q0, q1, m)
            if mode:
                mat4(q0 + n, q1 + n, m.conj())
        elif kind == 5:
            m = cplx(po, 16).reshape(4, 4)
            mat4(q0, q1, m)
            if mode:
                mat4(q0 + n, q1 + n, m.conj())
        elif kind in (6, 7) and mode:
            lam = float(batch.params[po])
            qs = [q0] if kind == 6 else [q0, q1]
            d = 2 ** len(qs)
            rows = sum(((idx >> q) & 1) << j for j, q in enumerate(qs))
            cols = sum(((idx >> (q + n)) & 1) << j for j, q in enumerate(qs))
            rest = idx.copy()
            for q in qs:
                rest &= ~((1 << q) | (1 << (q + n)))
            new = (1.0 - lam) * st
            diag = rows == cols
            sums = np.zeros(size, dtype=complex)
            np.add.at(sums, rest[diag], st[diag])
            new[diag] += (lam / d) * sums[rest[diag]]
            st = new
        elif kind == 8 and mode:
            p01, p10 = float(batch.params[po]), float(batch.params[po + 1])
            dd = np.arange(1 << n)
            d0 = dd[((dd >> q0) & 1) == 0]
            i0, i1 = d0 | (d0 << n), (d0 | (1 << q0)) | ((d0 | (1 << q0)) << n)
            a0, a1 = st[i0].copy(), st[i1].copy()
            st[i0], st[i1] = (1 - p10) * a0 + p01 * a1, p10 * a0 + (1 - p01) * a1
    if norm is None:
        norm = trace()
    tv = []
    j = np.arange(1 << n)
    for t in range(int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])):
        xm, zm, ny, _ = (int(v) for v in batch.terms[t])
        sign = np.array([(-1) ** bin(int(v) & zm).count("1") for v in j])
        v = st[j | ((j ^ xm) << n)] if mode else st[j ^ xm].conj() * st[j]
        tv.append(float(((1j ** ny) * sign * v).sum().real))
    b, e = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    value = 0.0
    for cf, t in zip(batch.coeff[b:e], tv):
        value = value + float(cf) * t
    return value, np.asarray(tv, dtype=np.float64), norm
