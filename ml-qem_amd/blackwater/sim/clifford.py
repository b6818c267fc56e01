"""Clifford circuits of up to 512 qubits: circuits -> the records ``mlqem_clifford_run_f64`` walks (include/mlqem_hip.h has the
layouts), and the calls on top of it.  Lowering runs on the host alone.

A Pauli observable is carried backwards through a Clifford circuit as a Pauli, so the ideal value on ``|0..0>`` and the value under
the project's noise model (:class:`~blackwater.sim.program.NoiseModel`) both come from one walk, exactly: a depolarising op scales a
Pauli that is not the identity on its qubits by ``1 - lambda``; a readout op turns ``Z_q`` into ``(1 - p01 - p10) Z_q + (p01 - p10) I``.

Gate records are TABLES, not gate names: for every gate the host takes the matrix ``program.py`` builds, conjugates every local Pauli
with it and decomposes the result in the Pauli basis.  The gate is a Clifford gate iff every image is +-one Pauli (to 1e-9, after
which the table is exact); anything else is refused by name.  Letters are I = 0, X = 1, Z = 2, Y = 3 (bit 0: x, bit 1: z), Y being
the Hermitian Pauli, so a unit is a sign and letters and nothing else.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..data.backends import pauli_terms
from ..data.circuit import Circuit
from .program import (OP_CX, OP_CZ, OP_DIAG1, OP_SWAP, SUPPORTED_GATES, _N_PARAMS, _TWO_QUBIT, _one_qubit, _two_qubit, upload,
                      upload_fields)

MAX_QUBITS_CLIFFORD = 512   # MLQEM_CLIFFORD_MAX_QUBITS
REG_QUBITS = 128            # MLQEM_CLIFFORD_REG_QUBITS: units of circuits up to here keep their words in registers
PAD = 32                    # MLQEM_CLIFFORD_PAD: entries of padding at the end of `pool` and `masks`
MAX_READOUT_EXPANSION = 10  # a term may expand into at most 2^10 sub-units
TABLE_TOL = 1e-9

CL_C1, CL_C2, CL_DEPOL1, CL_DEPOL2 = range(4)   # MLQEM_CLIFFORD_OP_*

_LETTER = {"I": 0, "X": 1, "Z": 2, "Y": 3}
_PAULI = [np.eye(2, dtype=complex), np.array([[0, 1], [1, 0]], dtype=complex), np.array([[1, 0], [0, -1]], dtype=complex),
          np.array([[0, -1j], [1j, 0]], dtype=complex)]   # by letter
_FIXED = {OP_CX: [1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0],    # basis index bit(q0) + 2 bit(q1); q0 controls
          OP_CZ: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1],
          OP_SWAP: [1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 0, 1]}


def _local_pauli(code: int, width: int) -> np.ndarray:
    """The Pauli with letter ``code & 3`` on q0 (and ``code >> 2`` on q1) over the basis index bit(q0) + 2 bit(q1)."""
    return _PAULI[code & 3] if width == 1 else np.kron(_PAULI[code >> 2], _PAULI[code & 3])


def gate_unitary(name: str, params: Tuple[float, ...]) -> Optional[np.ndarray]:
    """The matrix ``program.py`` lowers ``name`` to (None for ``id``): 2x2, or 4x4 over the basis index bit(q0) + 2 bit(q1)."""
    if name in _TWO_QUBIT:
        kind, entries = _two_qubit(name, params)
        return np.asarray(entries if entries else _FIXED[kind], dtype=complex).reshape(4, 4)
    lowered = _one_qubit(name, params)
    if lowered is None:
        return None
    kind, entries = lowered
    return np.diag(np.asarray(entries, dtype=complex)) if kind == OP_DIAG1 else np.asarray(entries, dtype=complex).reshape(2, 2)


def conjugation_table(mat: np.ndarray) -> Optional[List[Tuple[int, int]]]:
    """``[(image code, sign bit)]`` of ``U^dagger P U`` for the local Paulis P = 1 .. 3 (2x2) or 1 .. 15 (4x4), or None when some
    image is not +-one Pauli: every coefficient of the decomposition within 1e-9 of 0 or +-1 and of the real axis."""
    width = 1 if mat.shape[0] == 2 else 2
    d, count = mat.shape[0], 4 ** width
    basis = [_local_pauli(c, width) for c in range(count)]
    out = []
    for code in range(1, count):
        image = mat.conj().T @ basis[code] @ mat
        coeffs = np.array([np.trace(basis[c] @ image) / d for c in range(count)])
        if np.abs(coeffs.imag).max() > TABLE_TOL:
            return None
        big = np.flatnonzero(np.abs(np.abs(coeffs.real) - 1.0) <= TABLE_TOL)
        small = np.abs(coeffs.real) <= TABLE_TOL
        if len(big) != 1 or small.sum() != count - 1 or big[0] == 0:
            return None
        out.append((int(big[0]), 1 if coeffs.real[big[0]] < 0 else 0))
    return out


def pack_table(table: List[Tuple[int, int]]) -> Tuple[int, int, int]:
    """The three uint32 words (a, b, c) of a C1 (3 entries) or C2 (15 entries) record."""
    if len(table) == 3:
        word = 0
        for j, (code, s) in enumerate(table):
            word |= (code | s << 2) << (3 * j)
        return word, 0, 0
    letters = signs = 0
    for j, (code, s) in enumerate(table):
        letters |= code << (4 * j)
        signs |= s << j
    return letters & 0xFFFFFFFF, letters >> 32, signs


def invert_table(packed):
    """The packed table of ``U P U^dagger`` from the packed table of ``U^dagger P U`` (what a daggered schedule entry applies): if
    entry e maps p to (q, s), the inverse maps q to (p, s) -- the table is a signed permutation of the local Paulis.  ``"id"`` stays
    ``"id"``.  A C1 table is told from a C2 table by its second word (a C2 table's letters fill it; a C1 table leaves it 0)."""
    if isinstance(packed, str):
        if packed != "id":
            raise ValueError(f"invert_table: {packed!r} is no table")
        return packed
    a, b, c = (int(v) & 0xFFFFFFFF for v in packed)
    if b == 0:   # C1: three 3-bit fields, letter | sign << 2
        out: List[Optional[Tuple[int, int]]] = [None] * 3
        for j in range(3):
            field = a >> (3 * j) & 7
            code, s = field & 3, field >> 2
            if code == 0 or out[code - 1] is not None:
                raise ValueError(f"invert_table: {tuple(packed)!r} is no permutation of the letters X, Z, Y")
            out[code - 1] = (j + 1, s)
        return pack_table(out)
    letters = a | b << 32
    out = [None] * 15
    for e in range(15):
        code, s = letters >> (4 * e) & 15, c >> e & 1
        if code == 0 or out[code - 1] is not None:
            raise ValueError(f"invert_table: {tuple(packed)!r} is no permutation of the 15 two-qubit Paulis")
        out[code - 1] = (e + 1, s)
    return pack_table(out)


_TABLES: Dict[Tuple[str, Tuple[float, ...]], Optional[Tuple[int, int, int]]] = {}


def gate_table(name: str, params: Tuple[float, ...]):
    """The packed table of a gate, cached per (name, params): ``"id"`` for the identity, None for a gate that is no Clifford gate."""
    key = (name, params)
    if key not in _TABLES:
        if len(_TABLES) > 65536:
            _TABLES.clear()
        mat = gate_unitary(name, params)
        if mat is None:
            _TABLES[key] = "id"
        else:
            table = conjugation_table(mat)
            _TABLES[key] = None if table is None else pack_table(table)
    return _TABLES[key]


def is_clifford(circuit: Any) -> bool:
    """True iff every gate of ``circuit`` is one of ``SUPPORTED_GATES`` at an angle that makes it a Clifford gate (``barrier`` and
    ``measure`` do not count).  The width is not looked at: :func:`compile_clifford` has the cap."""
    circ = Circuit.from_any(circuit)
    for op in circ.ops:
        if op.name in ("barrier", "measure"):
            continue
        if op.name not in _N_PARAMS or len(op.params) != _N_PARAMS[op.name]:
            return False
        p = tuple(float(v) for v in op.params)
        if not all(math.isfinite(v) for v in p) or gate_table(op.name, p) is None:
            return False
    return True


@dataclass
class CliffordBatch:
    """A lowered batch: the host arrays of ``mlqem_clifford_run_f64``."""

    n_qubits: np.ndarray      # int32 [B]
    op_ptr: np.ndarray        # int64 [B + 1]
    ops: np.ndarray           # uint32 [n_ops, 4]: kind | q0 << 4 | q1 << 14, then the table words or the pool index
    pool: np.ndarray          # float64 [n_pool + 32]: keep = 1 - lambda
    units: np.ndarray         # int32 [n_units, 4]: circuit, first word in masks, number of Y, 0; the register units first
    masks: np.ndarray         # uint32 [n_masks + 32]: per unit W x words, then W z words
    n_reg: int
    n_lds: int
    term_ptr: np.ndarray      # int64 [B + 1]
    coeff: np.ndarray         # float64 [n_terms]
    comb_ptr: np.ndarray      # int64 [n_terms + 1]
    comb_unit: np.ndarray     # int32 [n_comb]
    comb_weight: np.ndarray   # float64 [n_comb, 2]: (weight of the unit's ideal value, of its noisy value)
    # the record map of the source gates, with the meaning it has in ``SimBatch``: what blackwater.sim.zne folds.  Record indices
    # are relative to op_ptr[c]; -1 = absent (``id`` has no gate record, a gate without noise no depolarising record)
    gate_ptr: Optional[np.ndarray] = None      # int64 [B + 1]: circuit c owns gates gate_ptr[c] .. gate_ptr[c + 1]
    gate_record: Optional[np.ndarray] = None   # int32 [n_gates]: the gate's own record
    gate_noise: Optional[np.ndarray] = None    # int32 [n_gates]: the depolarising record after it
    gate_name: Optional[np.ndarray] = None     # int16 [n_gates]: index of the gate's name in SUPPORTED_GATES
    gate_op: Optional[np.ndarray] = None       # int32 [n_gates]: index of the gate in the circuit's op list

    def __len__(self) -> int:
        return int(self.n_qubits.shape[0])

    def to(self, device) -> Dict[str, Any]:
        """The arrays as tensors on ``device``, keyed as ``ops.clifford_run`` names them (uint32 words travel as int32)."""
        out = upload_fields(self, ("n_qubits", "op_ptr", "pool", "units", "term_ptr", "coeff", "comb_ptr", "comb_unit", "comb_weight", "ops",
                                   "masks"), device, view={"ops": np.int32, "masks": np.int32})
        out["n_reg"], out["n_lds"] = self.n_reg, self.n_lds
        return out


def _words(mask: int, w: int) -> List[int]:
    return [(mask >> (32 * j)) & 0xFFFFFFFF for j in range(w)]


def refuse_non_pauli(noise: Any, who: str) -> None:
    """``ValueError`` naming the model and the reason where ``noise`` has a part the Clifford path cannot carry: thermal
    relaxation is no Pauli channel and a controlled rotation is no Clifford gate, so the walk would silently drop them."""
    why = getattr(noise, "non_pauli", None)
    if why:
        raise ValueError(f"{who}: the noise model {getattr(noise, 'name', type(noise).__name__)!r} cannot run on the Clifford path: {why}; "
                         "use the exact simulator (at most 5 qubits as a density matrix)")


def compile_clifford(circuits: Sequence[Any], observables: Sequence[Any], noise: Any = None) -> CliffordBatch:
    """Lowers Clifford ``circuits`` (anything ``Circuit.from_any`` takes) with one observable each (anything ``pauli_terms`` takes,
    any Pauli string with a real coefficient) to one :class:`CliffordBatch`.  ``noise``: None, a ``NoiseModel`` or any object with
    its ``after_gate(index, name, qubits)`` / ``readout_of(qubit)``.

    Gates are those of ``compile_programs`` (``SUPPORTED_GATES``; ``barrier`` ignored, ``measure`` records the measured qubit), each at
    any angle that makes it a Clifford gate, and the refusals are ``compile_programs``': unknown gates, a wrong parameter count, a
    gate after a measurement, a qubit out of range, a two-qubit gate on one qubit twice, a non-finite angle, a label of the wrong
    length or alphabet, a coefficient that is not real.  Also refused, by name: a gate that is not a Clifford gate (``rz(0.3)``), a
    circuit of more than 512 qubits, a noise model with thermal relaxation or a coherent error (:func:`refuse_non_pauli`), and, with non-trivial readout probabilities on a measured qubit, an observable with X or Y.

    Records: ``id`` has none but keeps its depolarising record; a depolarising record holds the index of ``keep = 1 - lambda`` in
    ``pool``.  Readout is no record: every ``Z_q`` of a term on a measured qubit with probabilities (p01, p10) becomes
    ``a_q Z_q + b_q I``, a = 1 - p01 - p10, b = p01 - p10.  A qubit with b = 0 only contributes its factor; m qubits with b != 0 expand
    the term into 2^m sub-units (at most 2^10), sub-unit s = 0 .. 2^m - 1 keeping Z on the j-th such qubit (ascending) iff bit j of s
    is set, weighted by the product of the a and b in ascending qubit order.  ``comb_*`` lists a term's sub-units in that order
    with (ideal weight, noisy weight): the ideal weight is 1 for the sub-unit that is the term itself and 0 otherwise."""
    circuits, observables = list(circuits), list(observables)
    if len(circuits) != len(observables):
        raise ValueError(f"compile_clifford: {len(circuits)} circuits but {len(observables)} observables")
    refuse_non_pauli(noise, "compile_clifford")
    relaxation_after, coherent_after = getattr(noise, "relaxation_after", None), getattr(noise, "coherent_after", None)
    nq_all, op_ptr, flat_ops, pool = [], [0], [], []
    unit_circ, unit_ny, unit_mask, masks = [], [], [], []
    coeffs, term_ptr, comb_ptr, comb_unit, comb_weight = [], [0], [0], [], []
    gate_ptr, gate_record, gate_noise, gate_name, gate_op = [0], [], [], [], []
    name_id = {g: j for j, g in enumerate(SUPPORTED_GATES)}

    for k, (obj, obs) in enumerate(zip(circuits, observables)):
        circ = Circuit.from_any(obj)
        where = f"circuit {k}"
        n = circ.num_qubits
        if n < 1 or n > MAX_QUBITS_CLIFFORD:
            raise ValueError(f"{where}: {n} qubits; the Clifford path takes 1 .. {MAX_QUBITS_CLIFFORD} qubits (the cap)")
        w = (n + 31) // 32
        measured: Dict[int, int] = {}
        done = set()
        n_rec = 0
        for i, op in enumerate(circ.ops):
            name = op.name
            if name == "barrier":
                continue
            for q in op.qubits:
                if not 0 <= q < n:
                    raise ValueError(f"{where}: op {i} ({name}) acts on qubit {q}, the circuit has {n}")
                if q in done:
                    raise ValueError(f"{where}: op {i} ({name}) acts on qubit {q} after it was measured")
            if name == "measure":
                if len(op.qubits) != 1 or len(op.clbits) != 1:
                    raise ValueError(f"{where}: op {i} (measure) wants one qubit and one classical bit")
                measured[int(op.clbits[0])] = int(op.qubits[0])
                done.add(op.qubits[0])
                continue
            if name not in _N_PARAMS:
                raise ValueError(f"{where}: op {i} is {name!r}, which is not simulated (supported: {' '.join(SUPPORTED_GATES)})")
            width = 2 if name in _TWO_QUBIT else 1
            if len(op.qubits) != width or len(op.params) != _N_PARAMS[name]:
                raise ValueError(f"{where}: op {i} ({name}) has {len(op.qubits)} qubits and {len(op.params)} parameters, want "
                                 f"{width} and {_N_PARAMS[name]}")
            p = tuple(float(v) for v in op.params)
            if not all(math.isfinite(v) for v in p):
                raise ValueError(f"{where}: op {i} ({name}) has the non-finite angle {p!r}")
            q0, q1 = (op.qubits[0], op.qubits[1]) if width == 2 else (op.qubits[0], 0)
            if width == 2 and q0 == q1:
                raise ValueError(f"{where}: op {i} ({name}) names qubit {q0} twice")
            table = gate_table(name, p)
            if table is None:
                shown = f"{name}({', '.join(repr(v) for v in p)})" if p else name
                raise ValueError(f"{where}: op {i}: {shown} is not a Clifford gate (every U^dagger P U must be +-one Pauli to "
                                 f"{TABLE_TOL:g}); the Clifford path takes no other gate")
            qs = q0 << 4 | q1 << 14
            rec = noi = -1
            if table != "id":
                rec = n_rec
                flat_ops += (CL_C2 | qs if width == 2 else CL_C1 | qs, table[0], table[1], table[2])
                n_rec += 1
            if noise is not None:
                reg = tuple(circ.qubit_reg_index[q] for q in op.qubits)
                for hook, why in ((relaxation_after, "thermal relaxation, which is not a Pauli channel"),
                                  (coherent_after, "a coherent error, which is not a Clifford gate")):
                    if hook is not None and hook(i, name, reg) is not None:   # a duck-typed model that does not say non_pauli
                        raise ValueError(f"{where}: op {i} ({name}): the noise model {getattr(noise, 'name', type(noise).__name__)!r} has "
                                         f"{why}; the Clifford path cannot carry it")
                lam = noise.after_gate(i, name, reg)
                if lam is not None:
                    if not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
                        raise ValueError(f"{where}: op {i} ({name}): depolarising parameter {lam!r}, want 0 <= lambda <= 1")
                    noi = n_rec
                    flat_ops += (CL_DEPOL2 | qs if width == 2 else CL_DEPOL1 | qs, len(pool), 0, 0)
                    pool.append(1.0 - float(lam))
                    n_rec += 1
            gate_record.append(rec)
            gate_noise.append(noi)
            gate_name.append(name_id[name])
            gate_op.append(i)
        readout: Dict[int, Tuple[float, float]] = {}
        if noise is not None:
            for q in sorted(set(measured.values())):
                pr = noise.readout_of(circ.qubit_reg_index[q])
                if pr is None:
                    continue
                p01, p10 = float(pr[0]), float(pr[1])
                if not all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in (p01, p10)):
                    raise ValueError(f"{where}: readout probabilities of qubit {q} are {(p01, p10)!r}, want both in [0, 1]")
                if p01 != 0.0 or p10 != 0.0:
                    readout[q] = (1.0 - p01 - p10, p01 - p10)
        for label, coeff in pauli_terms(obs):
            if len(label) != n:
                raise ValueError(f"{where}: Pauli label {label!r} has {len(label)} characters, the circuit has {n} qubits")
            c = complex(coeff)
            if c.imag != 0.0 or not math.isfinite(c.real):
                raise ValueError(f"{where}: coefficient {coeff!r} of {label!r} is not a finite real number")
            xm = zm = ny = 0
            for q, ch in enumerate(reversed(label)):
                if ch not in _LETTER:
                    raise ValueError(f"{where}: Pauli label {label!r} has the character {ch!r}, want only I, X, Y, Z")
                letter = _LETTER[ch]
                xm |= (letter & 1) << q
                zm |= (letter >> 1) << q
                ny += letter == 3
            if xm and readout:
                raise ValueError(f"{where}: readout noise on qubit {min(readout)} cannot be combined with an observable that has X or "
                                 f"Y terms ({label!r}: a readout op leaves only the measured distribution meaningful)")
            scale, expand = 1.0, []
            for q in sorted(readout):
                if zm >> q & 1:
                    a, b = readout[q]
                    if b == 0.0:
                        scale *= a
                    else:
                        expand.append((q, a, b))
            if len(expand) > MAX_READOUT_EXPANSION:
                raise ValueError(f"{where}: term {label!r} has Z on {len(expand)} measured qubits with asymmetric readout noise and would "
                                 f"expand into 2^{len(expand)} sub-units; the cap is 2^{MAX_READOUT_EXPANSION}")
            full = (1 << len(expand)) - 1
            for s in range(full + 1):
                weight, zs = scale, zm
                for j, (q, a, b) in enumerate(expand):
                    if s >> j & 1:
                        weight *= a
                    else:
                        weight *= b
                        zs &= ~(1 << q)
                comb_unit.append(len(unit_circ))
                comb_weight.append((1.0 if s == full else 0.0, weight))
                unit_circ.append(k)
                unit_ny.append(ny)
                unit_mask.append(len(masks))
                masks += _words(xm, w) + _words(zs, w)
            comb_ptr.append(len(comb_unit))
            coeffs.append(c.real)
        nq_all.append(n)
        op_ptr.append(op_ptr[-1] + n_rec)
        term_ptr.append(len(coeffs))
        gate_ptr.append(len(gate_record))

    if max(len(masks), len(pool), len(unit_circ)) + PAD > 2 ** 31 - 1:
        raise ValueError("compile_clifford: the batch exceeds the 2^31 - 1 entries one call can address; split it")
    nq = np.asarray(nq_all, dtype=np.int32)
    uc = np.asarray(unit_circ, dtype=np.int64)
    in_reg = nq[uc] <= REG_QUBITS if len(uc) else np.zeros(0, dtype=bool)
    n_reg = int(in_reg.sum())
    order = np.concatenate([np.flatnonzero(in_reg), np.flatnonzero(~in_reg)])   # stable: circuit order inside each part
    place = np.empty(len(uc), dtype=np.int64)
    place[order] = np.arange(len(uc))
    units = np.zeros((len(uc), 4), dtype=np.int32)
    if len(uc):
        units[:, 0] = uc[order]
        units[:, 1] = np.asarray(unit_mask, dtype=np.int64)[order]
        units[:, 2] = np.asarray(unit_ny, dtype=np.int64)[order]
    return CliffordBatch(
        n_qubits=nq, op_ptr=np.asarray(op_ptr, dtype=np.int64),
        ops=np.asarray(flat_ops, dtype=np.uint32).reshape(-1, 4),
        pool=np.asarray(pool + [1.0] * PAD, dtype=np.float64),
        units=units, masks=np.asarray(masks + [0] * PAD, dtype=np.uint32), n_reg=n_reg, n_lds=int(len(uc) - n_reg),
        term_ptr=np.asarray(term_ptr, dtype=np.int64), coeff=np.asarray(coeffs, dtype=np.float64),
        comb_ptr=np.asarray(comb_ptr, dtype=np.int64),
        comb_unit=(place[np.asarray(comb_unit, dtype=np.int64)] if comb_unit else np.zeros(0, dtype=np.int64)).astype(np.int32),
        comb_weight=np.asarray(comb_weight, dtype=np.float64).reshape(-1, 2),
        gate_ptr=np.asarray(gate_ptr, dtype=np.int64), gate_record=np.asarray(gate_record, dtype=np.int32),
        gate_noise=np.asarray(gate_noise, dtype=np.int32), gate_name=np.asarray(gate_name, dtype=np.int16),
        gate_op=np.asarray(gate_op, dtype=np.int32))


def run_clifford(batch: CliffordBatch, device="cuda"):
    """``(ideal_values, noisy_values, ideal_terms, noisy_terms, unit_ideal, unit_noisy)`` of a lowered batch: float64 tensors on
    ``device``, from one call."""
    from ..native import ops

    t = batch.to(device)
    return ops.clifford_run(t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"],
                            t["term_ptr"], t["coeff"], t["comb_ptr"], t["comb_unit"], t["comb_weight"])


def run_clifford_folded(batch: CliffordBatch, schedules, device="cuda"):
    """:func:`run_clifford` along the schedules of ``blackwater.sim.zne.build_clifford_schedules``: the same six tensors with a
    leading noise-factor axis, from one call (``ops.clifford_run_folded``)."""
    from ..native import ops

    t, s = batch.to(device), schedules.to(device)
    return ops.clifford_run_folded(t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"],
                                   t["term_ptr"], t["coeff"], t["comb_ptr"], t["comb_unit"], t["comb_weight"], s["sched_ptr"],
                                   s["sched"], len(schedules.noise_factors))


def clifford_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Any = None, device="cuda",
                                return_ideal: bool = False):
    """Exact expectation values of ``observables[k]`` after the Clifford circuit ``circuits[k]``, at any width up to 512 qubits:
    ``(values, term_values, term_ptr)`` in the form of :func:`~blackwater.sim.expectation_values`, noisy under ``noise`` when it is
    given and ideal otherwise.  ``return_ideal=True`` appends ``(ideal_values, ideal_term_values)`` from the same call."""
    batch = compile_clifford(circuits, observables, noise)
    ideal_values, noisy_values, ideal_terms, noisy_terms, _, _ = run_clifford(batch, device)
    term_ptr = upload(batch.term_ptr, ideal_values.device)
    head = (ideal_values, ideal_terms, term_ptr) if noise is None else (noisy_values, noisy_terms, term_ptr)
    return head + (ideal_values, ideal_terms) if return_ideal else head
