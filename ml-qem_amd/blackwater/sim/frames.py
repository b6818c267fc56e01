"""Measurement shots of Clifford circuits of up to 512 qubits: Pauli-frame sampling (``mlqem_clifford_sample_f64``;
include/mlqem_hip.h has the layouts and the rule of every draw).  Lowering runs on the host alone.

For a Clifford circuit under a Pauli noise model (the depolarising + readout form of :class:`~blackwater.sim.program.NoiseModel`)
the outcome distribution of a measurement basis is sampled exactly from one reference outcome and one Pauli frame per shot: 2 n
bits, a table look-up per gate and a random Pauli at every noise record that is hit.  No state vector, so the shots reach the widths
the exact Clifford path (:mod:`blackwater.sim.clifford`) reaches.  The circuits, the noise records and the refusals are
``compile_clifford``'s; the measurement groups are ``measurement_groups``; estimates, values and variances follow the rule of
``sample_expectation_values``.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..data.backends import pauli_terms
from ..data.circuit import Circuit
from .clifford import _LETTER, PAD, REG_QUBITS, CliffordBatch, _words, compile_clifford
from .program import MAX_SHOTS, _run_keys, check_seed, check_shots, measurement_groups, upload, upload_fields

MAX_GROUPS = 4096            # MLQEM_CLIFFORD_MAX_GROUPS: measurement groups per circuit (12 bits of a counter word)
DEPOL_BITS, READOUT_BITS = 60, 32


def depol_threshold(lam: float) -> int:
    """``floor(lambda 2^60)``, exactly: the float is taken as the rational it is."""
    return int(Fraction(float(lam)) * 2 ** DEPOL_BITS)


def readout_threshold(p: float) -> int:
    """``floor(p 2^32)``, exactly (0 .. 2^32)."""
    return int(Fraction(float(p)) * 2 ** READOUT_BITS)


@dataclass
class FrameBatch:
    """A batch lowered for frame sampling: the host arrays of ``mlqem_clifford_sample_f64``.  ``clifford`` is the same batch lowered
    for the exact path (its ``n_qubits``, ``op_ptr``, ``ops`` are the ones used here; ``pool`` is the float64 pool ``thresh`` sits
    beside)."""

    clifford: CliffordBatch
    thresh: np.ndarray        # uint64 [n_pool + readout tables + 32]: floor(lambda 2^60) per depolarising record, then the readout tables
    ro_ptr: np.ndarray        # int64 [B]: -1, or the circuit's readout table in thresh (2 n entries: floor(p10 2^32), floor(p01 2^32))
    group_ptr: np.ndarray     # int64 [B + 1]
    group_circ: np.ndarray    # int32 [n_groups]
    group_mask: np.ndarray    # int32 [n_groups]: the basis in masks, W words bx then W words bz
    ids: np.ndarray           # int32 [n_groups]: the groups of circuits up to 128 qubits first
    n_reg: int
    n_lds: int
    masks: np.ndarray         # uint32 [n_masks + 32]
    term_ptr: np.ndarray      # int64 [B + 1]
    coeff: np.ndarray         # float64 [n_terms]
    term_mask: np.ndarray     # int32 [n_terms]: the support in masks, W words
    term_group: np.ndarray    # int32 [n_terms]: the term's group inside its circuit
    gterm_ptr: np.ndarray     # int64 [n_groups + 1]
    gterm: np.ndarray         # int32 [n_terms]: the terms by group
    row_ptr: np.ndarray       # int64 [n_groups]: the group's n rows of 2 W + 1 words in the workspace
    n_rows: int
    ref_ptr: np.ndarray       # int64 [n_groups + 1]: the group's W words in `reference`; times shots, in `bits`
    max_qubits: int

    def __len__(self) -> int:
        return len(self.clifford)

    @property
    def n_qubits(self) -> np.ndarray:
        return self.clifford.n_qubits

    @property
    def pool(self) -> np.ndarray:
        return self.clifford.pool

    def to(self, device) -> Dict[str, Any]:
        """The arrays as tensors on ``device``, keyed as ``ops.clifford_sample`` names them (uint32 words travel as int32, the
        uint64 thresholds as int64: they are below 2^61)."""
        out = upload_fields(self, ("ro_ptr", "group_ptr", "group_circ", "group_mask", "ids", "term_ptr", "coeff", "term_mask", "gterm_ptr",
                                   "gterm", "row_ptr", "ref_ptr"), device)
        out.update(upload_fields(self.clifford, ("n_qubits", "op_ptr", "ops"), device, view={"ops": np.int32}))
        out.update(upload_fields(self, ("masks", "thresh"), device, view={"masks": np.int32, "thresh": np.int64}))
        return out


def compile_clifford_frames(circuits: Sequence[Any], observables: Sequence[Any], noise: Any = None) -> FrameBatch:
    """Lowers Clifford ``circuits`` with one observable each for frame sampling.  Circuits, noise records and every refusal are
    :func:`~blackwater.sim.compile_clifford`'s (a gate that is no Clifford gate, more than 512 qubits, a noise model with thermal
    relaxation or a coherent error, X or Y terms beside readout noise, ...), by name; also refused: a circuit whose terms need
    more than 4 096 measurement groups.

    Every depolarising record's lambda becomes the integer threshold ``floor(lambda 2^60)`` in ``thresh``, at the index its
    ``keep = 1 - lambda`` has in ``pool``; a circuit with readout noise gets a table of ``floor(p 2^32)``.  The terms of a circuit are
    partitioned by :func:`~blackwater.sim.measurement_groups`; a group's basis is one letter per qubit (Z where no term touches the
    qubit) and a term is a support mask inside its group: there are no rotation records."""
    circuits, observables = list(circuits), list(observables)
    base = compile_clifford(circuits, observables, noise)   # every check and refusal
    thresh: List[int] = []
    ro_tables: List[List[int]] = []
    ro_ptr, group_ptr, group_circ, group_mask, masks = [], [0], [], [], []
    term_mask, term_group, gterm_ptr, gterm, row_ptr, ref_ptr = [], [], [0], [], [], [0]
    n_rows = 0
    for k, (obj, obs) in enumerate(zip(circuits, observables)):
        circ = Circuit.from_any(obj)
        n = circ.num_qubits
        w = (n + 31) // 32
        measured = set()
        for i, op in enumerate(circ.ops):
            if op.name == "barrier":
                continue
            if op.name == "measure":
                measured.add(int(op.qubits[0]))
                continue
            if noise is not None:
                lam = noise.after_gate(i, op.name, tuple(circ.qubit_reg_index[q] for q in op.qubits))
                if lam is not None:
                    thresh.append(depol_threshold(lam))
        table = None
        if noise is not None:
            for q in sorted(measured):
                pr = noise.readout_of(circ.qubit_reg_index[q])
                if pr is None or (float(pr[0]) == 0.0 and float(pr[1]) == 0.0):
                    continue
                if table is None:
                    table = [0] * (2 * n)
                table[2 * q], table[2 * q + 1] = readout_threshold(pr[1]), readout_threshold(pr[0])   # (p01, p10) -> (p10, p01)
        ro_tables.append(table)
        rows = []
        first_term = len(term_mask)
        for label, _ in pauli_terms(obs):
            xm = zm = ny = 0
            for q, ch in enumerate(reversed(label)):
                letter = _LETTER[ch]
                xm |= (letter & 1) << q
                zm |= (letter >> 1) << q
                ny += letter == 3
            rows.append((xm, zm, ny, 0))
            term_mask.append(len(masks))
            masks += _words(xm | zm, w)
        groups_of, bases = measurement_groups(rows)
        if len(bases) > MAX_GROUPS:
            raise ValueError(f"circuit {k}: its terms need {len(bases)} measurement groups; frame sampling takes at most {MAX_GROUPS} "
                             "per circuit (split the observable)")
        term_group += groups_of
        full = (1 << n) - 1
        for g, (gx, gy) in enumerate(bases):
            group_circ.append(k)
            group_mask.append(len(masks))
            masks += _words(gx | gy, w) + _words(full & ~gx, w)
            members = [first_term + t for t, tg in enumerate(groups_of) if tg == g]
            gterm += members
            gterm_ptr.append(len(gterm))
            row_ptr.append(n_rows)
            n_rows += n * (2 * w + 1)
            ref_ptr.append(ref_ptr[-1] + w)
        group_ptr.append(len(group_circ))
    if len(thresh) + PAD != len(base.pool):
        raise ValueError(f"compile_clifford_frames: the noise model answered differently on the second pass ({len(thresh)} depolarising "
                         f"records, {len(base.pool) - PAD} on the first); after_gate must be a function of its arguments")
    for table in ro_tables:
        ro_ptr.append(-1 if table is None else len(thresh))
        if table is not None:
            thresh += table
    if max(len(masks), len(thresh)) + PAD > 2 ** 31 - 1 or n_rows > 2 ** 40:
        raise ValueError("compile_clifford_frames: the batch exceeds what one call can address; split it")
    gc = np.asarray(group_circ, dtype=np.int64)
    in_reg = base.n_qubits[gc] <= REG_QUBITS if len(gc) else np.zeros(0, dtype=bool)
    ids = np.concatenate([np.flatnonzero(in_reg), np.flatnonzero(~in_reg)]).astype(np.int32)
    return FrameBatch(
        clifford=base, thresh=np.asarray(thresh + [0] * PAD, dtype=np.uint64), ro_ptr=np.asarray(ro_ptr, dtype=np.int64),
        group_ptr=np.asarray(group_ptr, dtype=np.int64), group_circ=gc.astype(np.int32),
        group_mask=np.asarray(group_mask, dtype=np.int32), ids=ids, n_reg=int(in_reg.sum()), n_lds=int(len(gc) - in_reg.sum()),
        masks=np.asarray(masks + [0] * PAD, dtype=np.uint32), term_ptr=base.term_ptr, coeff=base.coeff,
        term_mask=np.asarray(term_mask, dtype=np.int32), term_group=np.asarray(term_group, dtype=np.int32),
        gterm_ptr=np.asarray(gterm_ptr, dtype=np.int64), gterm=np.asarray(gterm, dtype=np.int32),
        row_ptr=np.asarray(row_ptr, dtype=np.int64), n_rows=int(n_rows), ref_ptr=np.asarray(ref_ptr, dtype=np.int64),
        max_qubits=int(base.n_qubits.max()) if len(base) else 1)


@dataclass
class FrameResult:
    """What one sampled call produced: tensors on the device.  ``reference`` and ``bits`` are packed uint32 words carried as
    int32, CSR over ``ref_ptr`` (the W = ceil(n / 32) words of a group; a group's bits are ``[shots, W]`` from ``ref_ptr[g] * shots``)."""

    values: Any          # float64 [B]: sum coeff * sampled term estimate
    variance: Any        # float64 [B]: sum coeff^2 (1 - estimate^2)
    term_values: Any     # float64 [n_terms]
    term_ptr: Any        # int64 [B + 1]
    term_sums: Any       # int32 [n_terms]: S_t = sum over the shots of (-1)^popcount(bits & support)
    reference: Any       # int32 [n_ref]: the reference outcome of every group
    ref_ptr: Any         # int64 [n_groups + 1]
    group_ptr: Any       # int64 [B + 1]
    bits: Any = None     # int32 [n_ref * shots], with return_bits
    shots: int = 0
    seed: int = 0
    batch: Optional[FrameBatch] = None


def run_clifford_frames(batch: FrameBatch, shots: int, seed: int = 0, run_keys=None, return_bits: bool = False,
                        device="cuda") -> FrameResult:
    """Samples ``shots`` outcomes of every (circuit, group) of a lowered batch: one call, nothing read back.  ``run_keys``: one
    integer per circuit, by default its position in the batch; pass a circuit's batch key to draw the same shots for it alone."""
    from ..native import ops

    shots, seed = check_shots(shots, "run_clifford_frames"), check_seed(seed, "run_clifford_frames")
    keys = upload(_run_keys(run_keys, len(batch), "run_clifford_frames", per="circuit"), device)
    t = batch.to(device)
    values, variance, term_values, term_sums, reference, bits = ops.clifford_sample(
        t["n_qubits"], t["op_ptr"], t["ops"], t["thresh"], t["ro_ptr"], t["group_ptr"], t["group_circ"], t["group_mask"], t["ids"],
        batch.n_reg, batch.n_lds, t["masks"], t["term_ptr"], t["coeff"], t["term_mask"], t["gterm_ptr"], t["gterm"], keys, shots, seed,
        batch.max_qubits, t["row_ptr"], batch.n_rows, t["ref_ptr"], int(batch.ref_ptr[-1]), return_bits=return_bits)
    return FrameResult(values, variance, term_values, t["term_ptr"], term_sums, reference, t["ref_ptr"], t["group_ptr"], bits, shots,
                       seed, batch)


def sample_clifford_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Any = None, *, shots: int = None,
                                       seed: int = 0, run_keys=None, return_bits: bool = False, device="cuda") -> FrameResult:
    """Expectation values of ``observables[k]`` after the Clifford circuit ``circuits[k]`` estimated from ``shots`` measurement
    outcomes per measurement basis, at any width up to 512 qubits, ideal (``noise=None``) or under a depolarising + readout
    ``noise`` model.  The limit of every estimate is the value :func:`~blackwater.sim.clifford_expectation_values` gives."""
    if shots is None:
        raise ValueError("sample_clifford_expectation_values: shots is required (an int in 1 .. 2^20); clifford_expectation_values "
                         "gives the exact values")
    shots = check_shots(shots, "sample_clifford_expectation_values")
    return run_clifford_frames(compile_clifford_frames(circuits, observables, noise), shots, seed, run_keys, return_bits, device)


def frame_counts(result: FrameResult, k: int) -> List[Dict[str, int]]:
    """``{bitstring: count}`` per measurement group of circuit ``k``: qiskit's strings, n characters, qubit 0 the RIGHTMOST -- what
    ``cal_z_exp`` / ``counts_to_feature_vector`` take.  Needs ``return_bits=True``; reads that circuit's bits back from the device."""
    if result.bits is None:
        raise ValueError("frame_counts: the result has no bits (run it with return_bits=True)")
    batch = result.batch
    if not 0 <= k < len(batch):
        raise ValueError(f"frame_counts: circuit {k} of {len(batch)}")
    n, shots = int(batch.n_qubits[k]), result.shots
    w = (n + 31) // 32
    out = []
    for g in range(int(batch.group_ptr[k]), int(batch.group_ptr[k + 1])):
        b = int(batch.ref_ptr[g]) * shots
        words = result.bits[b:b + shots * w].cpu().numpy().view(np.uint32).reshape(shots, w)
        counts: Dict[str, int] = {}
        rows, freq = np.unique(words, axis=0, return_counts=True)
        for row, f in zip(rows, freq):
            value = sum(int(v) << (32 * j) for j, v in enumerate(row.tolist()))
            counts[format(value, f"0{n}b")] = int(f)
        out.append(counts)
    return out


__all__ = ["MAX_GROUPS", "MAX_SHOTS", "FrameBatch", "FrameResult", "compile_clifford_frames", "depol_threshold", "frame_counts",
           "readout_threshold", "run_clifford_frames", "sample_clifford_expectation_values"]
