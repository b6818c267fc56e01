"""The oracle, the derived tolerance and the case builders of the fused noise records (MLQEM_SIM_OP_NOISE1 / NOISE2: depolarising,
then thermal relaxation), shared by tests/test_relax_cpu.py and tests/test_gpu_relax.py (no test in here).  Everything that is not
about relaxation comes from tests/sim_cases.py, whose oracle, interpreter and bounds stay as they are.

Oracle.  ``simulate`` walks the circuit IR as ``sim_cases.simulate`` does and asks the noise spec for three things per gate: the
coherent error (``coherent_after``, a 4x4 unitary applied like a gate), the depolarising parameter (``after_gate``, the Pauli KRAUS
sum of sim_cases) and the relaxation triples (``relaxation_after``).  Relaxation is a KRAUS sum too, independent of the kernel's
closed form:  amplitude damping  K0 = diag(1, sqrt(1 - g)), K1 = sqrt(g) |0><1|,  with weight 1 - p1;  its excited-state twin
K0' = diag(sqrt(1 - g), 1), K1' = sqrt(g) |1><0|  with weight p1;  then a phase flip  rho -> (1 - p_z) rho + p_z Z rho Z  with
p_z = (1 - c / sqrt(1 - g)) / 2  (p_z = 0 at g = 1, where the coherences are gone already).  The order is the package's: coherent
error, depolarising, relaxation qubit by qubit.

Interpreter.  ``interpret`` follows include/mlqem_hip.h record by record on a density matrix, the two new kinds in the CLOSED form
the contract states; it checks the lowering without a GPU.  Vector-mode programs go to ``sim_cases.interpret`` (the noise kinds do
nothing there).

Tolerance (derived, not tuned; u = 2^-53).  sim_cases' recursion rests on every op being a contraction in the Frobenius norm.
Relaxation is NOT: it takes the maximally mixed state to a purer one.  In the orthonormal coordinates (tr, z) / sqrt 2 of a 2x2
block's diagonal it is [[1, 0], [g (1 - 2 p1), 1 - g]], and the two coherences scale by c, so its Frobenius operator norm is
  L(g, c, p1) = max(sigma_max([[1, 0], [g (1 - 2 p1), 1 - g]]), c)        (about 1 + g^2 / 2 ... 1 + g / 4 for small g; sqrt 2 at g = 1)
and on k qubits the norms multiply.  A true state still has |rho|_F <= 1, so the error of the state obeys
  E_0 = 0,   E_k = L_k E_(k-1) + cost_k u        (L_k = 1 for every op that is no relaxation)
per side.  Costs of the new passes, in the units of sim_cases (rounded operations per entry, the dearer side):
  cost 24  relaxation of one qubit.  The oracle: sqrt(1 - g) and sqrt(g) are 2 roundings each and enter squared (4 u), two
           sandwiches per twin and their sum (3 u), the weights 1 - p1 and p1 and the sum of the twins (4 u); p_z carries a
           subtraction, a square root, a quotient and a halving (4 u) and enters 1 - 2 p_z (8 u), the mix itself 3 u: 22 u, and
           the kernel's closed form (a sum, two products, a fused product per entry after the depolarising step) is well below it.
  cost 20  the depolarising part where the model has one (sim_cases.COST_DEPOL; lambda = 0 in a fused record is exact);
  cost 64  a coherent error: a 4 x 4 matrix on the rows and on the columns (2 x 32).
  term_bound = u (2 sides * 2^(n/2) * E_last + N + N / 64 + 16),  value_bound as in sim_cases.
Every case of the suites asserts that its bounds stay below sim_cases.CAP = 1e-11.
"""
import dataclasses
import functools
import math

import numpy as np

import sim_cases as sc

U = sc.U
CAP = sc.CAP
COST_RELAX, COST_COHERENT = 24, 64
KIND_NOISE1, KIND_NOISE2 = 10, 11


# ---- the Kraus oracle ----------------------------------------------------------------------------------------------------------------
def sandwich(k, qubits, rho, n):
    """K rho K^dagger with K on ``qubits``: K on the rows, conj(K) on the columns."""
    k = np.asarray(k, dtype=complex)
    return sc.apply(k, qubits, sc.apply(k.conj(), qubits, rho.T, n).T, n)


def kraus_relax(rho, q, g, c, p1, n):
    s, r = math.sqrt(1.0 - g), math.sqrt(g)
    down = sandwich(np.diag([1.0, s]), [q], rho, n) + sandwich(np.array([[0.0, r], [0.0, 0.0]]), [q], rho, n)
    up = sandwich(np.diag([s, 1.0]), [q], rho, n) + sandwich(np.array([[0.0, 0.0], [r, 0.0]]), [q], rho, n)
    rho = (1.0 - p1) * down + p1 * up
    pz = 0.0 if s == 0.0 else (1.0 - c / s) / 2.0
    return (1.0 - pz) * rho + pz * sandwich(sc.Z, [q], rho, n)


def kraus_depolarise(rho, qubits, lam, n):
    """sim_cases' Pauli Kraus sum with local sandwiches (the same 4^k terms, no 2^n x 2^n Pauli matrices)."""
    d2 = 4 ** len(qubits)
    acc = np.zeros_like(rho)
    for code in range(d2):
        term = rho
        for j, q in enumerate(qubits):
            ch = "IXYZ"[(code >> (2 * j)) & 3]
            if ch != "I":
                term = sandwich(sc.PAULI[ch], [q], term, n)
        acc = acc + term
    return (1.0 - lam) * rho + (lam / d2) * acc


def _hooks(noise):
    return getattr(noise, "relaxation_after", None), getattr(noise, "coherent_after", None)


def final_state(circuit, noise):
    """``(rho before the readout ops, measured qubits)`` of one circuit under ``noise``."""
    n = circuit.num_qubits
    rho = np.zeros((2 ** n, 2 ** n), dtype=complex)
    rho[0, 0] = 1.0
    relax_of, coherent_of = _hooks(noise)
    measured = []
    for i, op in enumerate(circuit.ops):
        if op.name == "barrier":
            continue
        if op.name == "measure":
            measured.append(op.qubits[0])
            continue
        qs = list(op.qubits)
        reg = tuple(circuit.qubit_reg_index[q] for q in qs)
        if op.name != "id":
            rho = sandwich(sc.gate_matrix(op.name, op.params), qs, rho, n)
        coherent = coherent_of(i, op.name, reg) if coherent_of else None
        if coherent is not None:
            rho = sandwich(coherent, qs, rho, n)
        lam = noise.after_gate(i, op.name, reg)
        if lam is not None:
            rho = kraus_depolarise(rho, qs, lam, n)
        relax = relax_of(i, op.name, reg) if relax_of else None
        if relax is not None:
            for q, (g, c, p1) in zip(qs, relax):
                rho = kraus_relax(rho, q, g, c, p1, n)
    return rho, measured


def simulate(circuit, terms, noise):
    """``(value, term_values, norm)`` as ``sim_cases.simulate`` returns them, density mode, relaxation and coherent errors included."""
    n = circuit.num_qubits
    rho, measured = final_state(circuit, noise)
    norm = float(np.trace(rho).real)
    readouts = [(q, noise.readout_of(circuit.qubit_reg_index[q])) for q in sorted(set(measured))]
    readouts = [(q, pr) for q, pr in readouts if pr is not None]
    if readouts:
        probs = np.diag(rho).real.copy()
        for q, (p01, p10) in readouts:
            probs = sc.apply(np.array([[1 - p10, p01], [p10, 1 - p01]]), [q], probs.astype(complex), n).real
        tv = []
        for label, _ in terms:
            assert set(label) <= {"I", "Z"}, label
            tv.append(float(np.sum(sc.pauli_apply(label, np.ones(2 ** n, dtype=complex), n).real * probs)))
    else:
        tv = [float(np.trace(sc.pauli_apply(label, rho, n)).real) for label, _ in terms]
    value = 0.0
    for (_, c), t in zip(terms, tv):
        value = value + float(np.real(c)) * t
    return value, np.asarray(tv, dtype=np.float64), norm


# ---- the program format, interpreted on the host -------------------------------------------------------------------------------------
def _blocks(rho, qubits, n):
    """A view of rho with the (row, column) axis pair of every qubit of ``qubits`` in front."""
    t = rho.reshape((2,) * (2 * n))
    axes = []
    for q in qubits:
        axes += [n - 1 - q, 2 * n - 1 - q]
    return np.moveaxis(t, axes, list(range(len(axes))))


def _closed_depol(t, k, lam):
    if k == 1:
        tr = t[0, 0] + t[1, 1]
        t *= 1.0 - lam
        t[0, 0] += 0.5 * lam * tr
        t[1, 1] += 0.5 * lam * tr
    else:
        tr = ((t[0, 0, 0, 0] + t[1, 1, 0, 0]) + t[0, 0, 1, 1]) + t[1, 1, 1, 1]
        t *= 1.0 - lam
        for a in (0, 1):
            for b in (0, 1):
                t[a, a, b, b] += 0.25 * lam * tr


def _closed_relax(t, g, c, p1):
    tr = t[0, 0] + t[1, 1]
    e00 = (1.0 - g) * t[0, 0] + g * (1.0 - p1) * tr
    e11 = (1.0 - g) * t[1, 1] + g * p1 * tr
    t[0, 0], t[1, 1] = e00, e11
    t[0, 1] *= c
    t[1, 0] *= c


def interpret(batch, c, with_probs=False):
    """``(value, term_values, norm)`` of circuit ``c`` of a ``SimBatch`` (and, ``with_probs``, the diagonal a MEASURE record would
    store per group), record by record as include/mlqem_hip.h states them."""
    n, mode, n_ro, n_tail = (int(v) for v in batch.circ[c])
    if not mode:
        assert not with_probs
        return sc.interpret(batch, c)
    rho = np.zeros((2 ** n, 2 ** n), dtype=complex)
    rho[0, 0] = 1.0
    ops = batch.ops[int(batch.op_ptr[c]):int(batch.op_ptr[c + 1])].tolist()
    n_main = len(ops) - n_ro - n_tail
    norm, probs = None, []

    def cplx(po, count):
        v = batch.params[po:po + 2 * count]
        return v[0::2] + 1j * v[1::2]

    for k, (kind, q0, q1, po) in enumerate(ops):
        if k == n_main:
            norm = float(np.trace(rho).real)
        if kind == 0:
            rho = sandwich(cplx(po, 4).reshape(2, 2), [q0], rho, n)
        elif kind == 1:
            rho = sandwich(np.diag(cplx(po, 2)), [q0], rho, n)
        elif kind in (2, 3, 4):
            rho = sandwich(sc.gate_matrix({2: "cx", 3: "cz", 4: "swap"}[kind]), [q0, q1], rho, n)
        elif kind == 5:
            rho = sandwich(cplx(po, 16).reshape(4, 4), [q0, q1], rho, n)
        elif kind in (6, 7, KIND_NOISE1, KIND_NOISE2):
            rho = np.ascontiguousarray(rho)
            two = kind in (7, KIND_NOISE2)
            t = _blocks(rho, [q0, q1] if two else [q0], n)
            _closed_depol(t, 2 if two else 1, float(batch.params[po]))
            if kind == KIND_NOISE1:
                _closed_relax(t, *(float(v) for v in batch.params[po + 1:po + 4]))
            elif kind == KIND_NOISE2:
                _closed_relax(t, *(float(v) for v in batch.params[po + 1:po + 4]))
                _closed_relax(np.moveaxis(t, [2, 3], [0, 1]), *(float(v) for v in batch.params[po + 4:po + 7]))
        elif kind == 8:
            p01, p10 = float(batch.params[po]), float(batch.params[po + 1])
            d = sc.apply(np.array([[1 - p10, p01], [p10, 1 - p01]]), [q0], np.diag(rho).astype(complex), n)
            rho = np.diag(d)   # only the diagonal is meaningful after a readout op
        elif kind == 9:
            probs.append(np.diag(rho).real.copy())
    if norm is None:
        norm = float(np.trace(rho).real)
    tv = []
    j = np.arange(1 << n)
    for t in range(int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])):
        xm, zm, ny, _ = (int(v) for v in batch.terms[t])
        sign = np.array([(-1) ** bin(int(v) & zm).count("1") for v in j])
        tv.append(float(((1j ** ny) * sign * rho[j, j ^ xm]).sum().real))
    b, e = int(batch.term_ptr[c]), int(batch.term_ptr[c + 1])
    value = 0.0
    for cf, t in zip(batch.coeff[b:e], tv):
        value = value + float(cf) * t
    out = (value, np.asarray(tv, dtype=np.float64), norm)
    return out + (probs,) if with_probs else out


_RECORD_SIZE = {0: 8, 1: 4, 5: 32, 6: 1, 7: 1, 8: 2, KIND_NOISE1: 4, KIND_NOISE2: 7}


def expand(batch, sch, f):
    """``zne_cases.expand`` with the new kinds: run ``f * B + c`` of the schedules written out as a plain program, a daggered
    entry's matrix conjugate-transposed (U1, U2) or its phases conjugated (DIAG1) in numpy; a noise record is copied as it is
    whatever its dagger bit says."""
    n_circ = len(batch)
    ops, params, op_ptr = [], [], [0]
    for c in range(n_circ):
        r = f * n_circ + c
        base = int(batch.op_ptr[c])
        for e in sch.sched[int(sch.sched_ptr[r]):int(sch.sched_ptr[r + 1])].tolist():
            kind, q0, q1, po = (int(v) for v in batch.ops[base + (e >> 1)])
            vals = np.array(batch.params[po:po + _RECORD_SIZE.get(kind, 0)], dtype=np.float64)
            if e & 1 and kind in (0, 5):
                d = 2 if kind == 0 else 4
                mat = (vals[0::2] + 1j * vals[1::2]).reshape(d, d).conj().T.reshape(-1)
                vals = np.stack([mat.real, mat.imag], axis=1).reshape(-1)
            elif e & 1 and kind == 1:
                vals[1::2] = -vals[1::2]
            ops.append((kind, q0, q1, len(params)))
            params.extend(vals.tolist())
        op_ptr.append(len(ops))
    return dataclasses.replace(batch, op_ptr=np.asarray(op_ptr, dtype=np.int64), ops=np.asarray(ops, dtype=np.int32).reshape(-1, 4),
                               params=np.asarray(params + [0.0] * 32, dtype=np.float64))


# ---- tolerance -------------------------------------------------------------------------------------------------------------------------
def op_norm(g, c, p1):
    """The Frobenius operator norm of one qubit's relaxation map (module docstring)."""
    return max(float(np.linalg.svd(np.array([[1.0, 0.0], [g * (1.0 - 2.0 * p1), 1.0 - g]]), compute_uv=False)[0]), float(c))


def error_units(circuit, noise, extra=0):
    """E_last of the module docstring, in units of u: the recursion over the circuit's ops (``extra``: cost of records appended to
    the program after them, such as a measurement tail's rotations)."""
    relax_of, coherent_of = _hooks(noise)
    e, measured = 0.0, set()
    for i, op in enumerate(circuit.ops):
        if op.name == "barrier":
            continue
        if op.name == "measure":
            measured.add(op.qubits[0])
            continue
        reg = tuple(circuit.qubit_reg_index[q] for q in op.qubits)
        e += 2 * sc._COST.get(op.name, 12)
        if coherent_of and coherent_of(i, op.name, reg) is not None:
            e += COST_COHERENT
        if noise.after_gate(i, op.name, reg) is not None:
            e += sc.COST_DEPOL
        relax = relax_of(i, op.name, reg) if relax_of else None
        if relax is not None:
            for g, c, p1 in relax:
                e = op_norm(g, c, p1) * e + COST_RELAX
    e += sc.COST_READOUT * sum(1 for q in measured if noise.readout_of(circuit.qubit_reg_index[q]) is not None)
    return e + extra


def term_bound(circuit, noise, extra=0):
    big_n = 2 ** circuit.num_qubits
    return U * (2 * math.sqrt(big_n) * error_units(circuit, noise, extra) + big_n + big_n / 64 + 16)


def value_bound(circuit, terms, noise):
    total = sum(abs(float(np.real(c))) for _, c in terms)
    return total * term_bound(circuit, noise) + (len(terms) + 2) * U * total


# ---- noise specs -----------------------------------------------------------------------------------------------------------------------
class RelaxNoise:
    """A duck-typed spec for the tests: after EVERY gate a depolarising parameter in [0, 0.2] and one relaxation triple per qubit
    with g in [0, g_max], c in [0, sqrt(1 - g)], p1 in [0, 1], drawn per op index.  ``corners`` (a dict op index -> (lambda,
    triple)) forces values; ``coherent`` (a set of op indices) puts a random 4x4 unitary after those two-qubit gates;
    ``depol=False`` leaves the depolarising part out (the fused record then carries lambda = 0)."""

    has_readout = False

    def __init__(self, seed, g_max=0.02, corners=None, coherent=(), readout=None, depol=True):
        self._seed, self._g_max, self._corners, self._coherent, self._depol = seed, g_max, dict(corners or {}), set(coherent), depol
        self.readout = dict(readout or {})
        self.has_readout = bool(self.readout)
        self.name = f"relax-{seed}"

    @functools.lru_cache(maxsize=None)
    def _draw(self, index, width):
        rng = np.random.default_rng([self._seed, index, 7])
        lam = float(rng.uniform(0.0, 0.2))
        triples = []
        for _ in range(width):
            g = float(rng.uniform(0.0, self._g_max))
            triples.append((g, float(rng.uniform(0.0, math.sqrt(1.0 - g))), float(rng.uniform(0.0, 1.0))))
        if index in self._corners:
            lam, triple = self._corners[index]
            triples = [triple] * width
        q, r = np.linalg.qr(rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4)))
        return lam, tuple(triples), q * (np.diag(r) / np.abs(np.diag(r)))

    def after_gate(self, index, name, qubits):
        return self._draw(index, len(qubits))[0] if self._depol or index in self._corners else None

    def relaxation_after(self, index, name, qubits):
        return self._draw(index, len(qubits))[1]

    def coherent_after(self, index, name, qubits):
        return self._draw(index, len(qubits))[2] if index in self._coherent and len(qubits) == 2 else None

    def readout_of(self, qubit):
        return self.readout.get(qubit)


def corner_triples(lams=(0.0, 1.0)):
    """(lambda, (g, c, p1)) at the corners: lambda in {0, 1}, g in {0, 1}, c in {0, sqrt(1 - g)}, p1 in {0, 0.5, 1}: 9 per lambda
    (at g = 1 the two values of c coincide)."""
    out = []
    for lam in lams:
        for g in (0.0, 1.0):
            for c in sorted({0.0, math.sqrt(1.0 - g)}):
                for p1 in (0.0, 0.5, 1.0):
                    out.append((lam, (g, c, p1)))
    return out


def corner_program(n, pair=None, lams=(0.0, 1.0)):
    """One gate per corner of ``corner_triples(lams)`` (h, sx and ry on qubit 0 in turn where ``pair`` is None, else cx / ecr / rzz
    on ``pair``), each followed by its corner's fused record, and the spec that forces the corners.  At g = 1 and p1 = 0 or 1 a
    relaxation has the norm sqrt 2, twice in a record on a pair; the pair programs therefore take one lambda each, which keeps
    the product of the norms at 4 and the bound below the cap."""
    from blackwater.data.circuit import Circuit, CircuitOp

    corners = corner_triples(lams)
    ops = []
    for k in range(len(corners)):
        if pair is None:
            ops.append(CircuitOp(("h", "sx", "ry")[k % 3], (0,), (), (0.7 + 0.1 * k,) if k % 3 == 2 else ()))
        else:
            ops.append(CircuitOp(("cx", "ecr", "rzz")[k % 3], tuple(pair), (), (0.4 + 0.1 * k,) if k % 3 == 2 else ()))
    return Circuit(n, 0, ops), RelaxNoise(90 + n, corners=dict(enumerate(corners)))


# ---- the reference anchor --------------------------------------------------------------------------------------------------------------
def lima():
    import os

    from blackwater.data.backends import StaticBackend

    return StaticBackend.from_json(os.path.join(sc.GOLDEN, "fake_lima_backend_props.json"))


def golden_noisy():
    """``(qasm texts, stored noisy [900, 4])``: the reference's 10 000-shot noisy labels of the 900 golden circuits."""
    import os

    texts, noisy = sc.golden_circuits()[0], []
    for _, dz in sc._GOLDEN_FILES:
        noisy.append(np.asarray(np.load(os.path.join(sc.GOLDEN, dz))["noisy"], dtype=np.float64))
    return texts, np.concatenate(noisy)


# ---- the device grid -------------------------------------------------------------------------------------------------------------------
def pair_program(n, pair, seed):
    """A short program that ends in two-qubit gates on the ordered ``pair``: a rotation on every qubit (so that every entry of rho
    is populated), rzz and cx on the pair with an h between.  Every gate gets a fused record with g up to 0.3."""
    from blackwater.data.circuit import Circuit, CircuitOp

    ops = [CircuitOp("ry", (q,), (), (0.5 + 0.3 * q,)) for q in range(n)] + [CircuitOp("rx", (q,), (), (0.9 - 0.2 * q,)) for q in range(n)]
    ops += [CircuitOp("rzz", tuple(pair), (), (0.8,)), CircuitOp("h", (pair[0],)), CircuitOp("cx", tuple(pair))]
    return Circuit(n, 0, ops), RelaxNoise(seed, g_max=0.3)


@functools.lru_cache(maxsize=None)
def grid():
    """``[(id, circuit, terms, noise)]``: the smallest shapes at which each pass can go wrong.  n = 1 .. 5 with 40 random ops
    (wave variant up to n = 4, workgroup at n = 5; NOISE1 alone at n = 1, NOISE2 on the whole state at n = 2), a coherent record
    after some two-qubit gates; the corners of the parameters on one qubit and on a pair; NOISE2 on every ordered pair of n = 3
    and on (0, 4), (4, 0), (2, 3) of n = 5."""
    cases = []
    for n in (1, 2, 3, 4, 5):
        cases.append((f"random-n{n}", sc.random_program(n, 40, seed=70 + n), tuple(sc.term_set(n, seed=n)),
                      RelaxNoise(80 + n, coherent=range(0, 40, 3))))
    c, noise = corner_program(1)
    cases.append(("corners-noise1-n1", c, tuple(sc.term_set(1, seed=6)), noise))
    for n, pair in ((2, (0, 1)), (2, (1, 0)), (5, (4, 1))):
        for lam in (0.0, 1.0):
            c, noise = corner_program(n, pair, (lam,))
            cases.append((f"corners-noise2-n{n}-{pair[0]}{pair[1]}-lam{int(lam)}", c, tuple(sc.term_set(n, seed=7)), noise))
    for a in range(3):
        for b in range(3):
            if a != b:
                c, noise = pair_program(3, (a, b), 100 + 3 * a + b)
                cases.append((f"pair-n3-{a}{b}", c, tuple(sc.term_set(3, seed=8)), noise))
    for pair in ((0, 4), (4, 0), (2, 3)):
        c, noise = pair_program(5, pair, 120 + pair[0])
        cases.append((f"pair-n5-{pair[0]}{pair[1]}", c, tuple(sc.term_set(5, seed=9)), noise))
    return cases


@functools.lru_cache(maxsize=None)
def grid_oracle():
    """``{id: (value, term_values, norm)}`` of the Kraus oracle on the grid, computed once."""
    return {name: simulate(c, list(terms), noise) for name, c, terms, noise in grid()}
