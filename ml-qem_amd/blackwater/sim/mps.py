"""Matrix-product-state simulation of circuits on a line: labels for wide circuits that are not Clifford circuits.

``compile_mps`` lowers circuits whose two-qubit gates all act on neighbouring qubits (q, q + 1) to the records of
``mlqem_mps_run_f64`` (include/mlqem_hip.h has the layouts, the keep rule and the draw contract); nothing in it touches the GPU.
``run_mps`` runs a lowered batch on the device, ``mps_expectation_values`` is the one-call form.  Ideal values are exact while no
bond needs more than ``max_bond`` (TFIM circuits: through 5 Trotter steps at bond 32) and come with an a-priori certificate
beyond: ``error_bound`` B bounds the distance of the states, so |<O>_exact - <O>_mps| <= 2 B sum|coeff|.  With a depolarising +
readout noise model and ``trajectories`` the same kernel gives noisy values: every depolarising record inserts one drawn Pauli
string (its probabilities do not depend on the state), readout noise is folded into the measured operators.

``compile_mps_shots`` / ``run_mps_shots`` / ``sample_mps_expectation_values`` draw measurement shots from the same states
(``mlqem_mps_sample_f64``: perfect sampling, one sweep over the sites per shot), ``mps_counts`` gives the count dictionaries.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..data.circuit import Circuit
from .program import (_N_PARAMS, _TWO_QUBIT, OP_DIAG1, PARAM_PAD, SUPPORTED_GATES, NoiseModel, _check_coherent, _lower_terms,
                      _one_qubit, _two_qubit, check_seed, check_trajectories, measurement_groups)

MAX_BOND = 32            # MLQEM_MPS_MAX_BOND: theta, (2 chi) x (2 chi) complex128 = 64 KiB, sits in LDS beside a second workgroup
MAX_QUBITS_MPS = 512     # MLQEM_MPS_MAX_QUBITS
MPS_BUFFER_BYTES = 4 << 30   # the site-tensor workspace of one launch stays under this (``buffer_bytes=``): 1 300 units of 100 qubits
DEFAULT_CUTOFF = 1e-26   # relative weight below which a column is dropped: the numerically-zero columns of a rank-deficient theta
OP_MPS_U1, OP_MPS_U2, OP_MPS_DEPOL1, OP_MPS_DEPOL2 = 0, 5, 6, 7   # MLQEM_MPS_OP_*

_PERMUTATION = {"cx": (0, 3, 2, 1), "swap": (0, 2, 1, 3)}   # column j of the matrix has its 1 in row _PERMUTATION[name][j]


def cutoff_floor(n_decompositions: int, max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF) -> float:
    """The floor the cutoff puts under ``error_bound``: a decomposition that drops only numerically-zero columns (at most
    2 max_bond of them, each below ``cutoff`` of the weight) adds at most sqrt(2 * 2 max_bond * cutoff)."""
    return int(n_decompositions) * math.sqrt(2.0 * 2.0 * max_bond * cutoff)


def _matrix2(name: str, p) -> Optional[np.ndarray]:
    lowered = _one_qubit(name, p)
    if lowered is None:
        return None
    kind, entries = lowered
    e = [complex(v) for v in entries]
    return np.array([[e[0], 0.0], [0.0, e[1]]] if kind == OP_DIAG1 else [[e[0], e[1]], [e[2], e[3]]], dtype=complex)


def _matrix4(name: str, p) -> np.ndarray:
    """The gate over the basis index bit(q0) + 2 bit(q1), from ``program``'s tables."""
    if name in _PERMUTATION:
        m = np.zeros((4, 4), dtype=complex)
        for j, i in enumerate(_PERMUTATION[name]):
            m[i, j] = 1.0
        return m
    if name == "cz":
        return np.diag([1.0, 1.0, 1.0, -1.0]).astype(complex)
    return np.asarray([complex(v) for v in _two_qubit(name, p)[1]], dtype=complex).reshape(4, 4)


_FLIP = [0, 2, 1, 3]   # basis index bit(a) + 2 bit(b) -> bit(b) + 2 bit(a)


def _to_lower_basis(m: np.ndarray, orient: int) -> np.ndarray:
    """A 4x4 matrix over bit(q0) + 2 bit(q1) as one over bit(lower site) + 2 bit(upper site)."""
    return m[np.ix_(_FLIP, _FLIP)] if orient else m


@dataclass
class MpsBatch:
    """A batch lowered for ``mlqem_mps_run_f64``: the host arrays and what the host knows about every circuit."""

    n_qubits: np.ndarray    # int32 [B]
    op_ptr: np.ndarray      # int64 [B + 1]
    ops: np.ndarray         # int32 [n_ops, 4]: kind, (lower) site, orientation, offset into params
    params: np.ndarray      # float64 [n_params + 32]
    term_ptr: np.ndarray    # int64 [B + 1]
    term_circ: np.ndarray   # int32 [n_terms]
    term_off: np.ndarray    # int64 [n_terms]: the term's first letter in ``letters``
    letters: np.ndarray     # uint8 [n_letters]: 0 I, 1 X, 2 Y, 3 Z per site
    coeff: np.ndarray       # float64 [n_terms]
    site_ptr: np.ndarray    # int64 [B + 1]
    readout: np.ndarray     # float64 [n_sites, 2]: (a, b) of the Z slot a Z + b I of every site; (1, 0) without readout noise
    max_bond: int = MAX_BOND
    cutoff: float = DEFAULT_CUTOFF
    trajectories: Optional[int] = None
    n_noise: List[int] = field(default_factory=list)       # noise records per circuit
    abs_coeff: List[float] = field(default_factory=list)   # sum |coeff| per circuit
    measured: List[Dict[int, int]] = field(default_factory=list)
    # the record map of the noisy lowering, with ``SimBatch``'s meaning (record numbers are relative to the circuit's first record,
    # -1: none); ``blackwater.sim.zne.build_mps_schedules`` folds over it.  The ideal lowering fuses gates into bond records, so it
    # has no fold units and keeps no map (None)
    gate_ptr: Optional[np.ndarray] = None         # int64 [B + 1]: circuit c owns gates gate_ptr[c] .. gate_ptr[c + 1]
    gate_name: Optional[np.ndarray] = None        # int16 [n_gates]: index of the gate's name in SUPPORTED_GATES
    gate_record: Optional[np.ndarray] = None      # int32 [n_gates]: the gate's own U1 / U2 record
    gate_noise: Optional[np.ndarray] = None       # int32 [n_gates]: the first noise record after it
    gate_noise_len: Optional[np.ndarray] = None   # int32 [n_gates]: 0, 1 (DEPOL*) or 2 (a coherent U2, then DEPOL*)

    def __len__(self) -> int:
        return int(self.n_qubits.shape[0])

    def to(self, device) -> Dict[str, Any]:
        import torch

        dev = torch.device(device)
        return {k: torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(dev)
                for k in ("n_qubits", "op_ptr", "ops", "params", "term_ptr", "term_circ", "term_off", "letters", "coeff", "site_ptr",
                          "readout")}


def is_line_circuit(circuit: Any) -> bool:
    """Whether every two-qubit gate of the circuit acts on neighbouring qubits (q, q + 1), in either order."""
    return all(len(op.qubits) != 2 or op.name in ("barrier", "measure") or abs(op.qubits[0] - op.qubits[1]) == 1
               for op in Circuit.from_any(circuit).ops)


def _check_bond(max_bond: Any, who: str) -> int:
    if isinstance(max_bond, bool) or not isinstance(max_bond, (int, np.integer)) or not 1 <= int(max_bond) <= MAX_BOND:
        raise ValueError(f"{who}: max_bond = {max_bond!r}, want an int in 1 .. {MAX_BOND} (bond 64 needs theta outside LDS: not built)")
    return int(max_bond)


def _check_cutoff(cutoff: Any, who: str) -> float:
    if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float, np.floating)) or not 0.0 <= float(cutoff) < 1.0:
        raise ValueError(f"{who}: cutoff = {cutoff!r}, want a relative weight in [0, 1)")
    return float(cutoff)


def compile_mps(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                trajectories: Optional[int] = None, max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF) -> MpsBatch:
    """Lowers ``circuits`` with one observable each to one :class:`MpsBatch`.  Site = qubit index.

    ``noise=None`` (ideal): one ``U2`` record per bond visit -- a run of gates confined to one bond (its one-qubit gates included)
    is multiplied into a single 4x4 matrix over bit(lower) + 2 bit(upper) -- and one ``U1`` record per qubit whose last one-qubit
    gates no bond absorbed.  With ``noise`` and ``trajectories``: nothing is fused; one ``U1`` record per one-qubit gate, one ``U2``
    per two-qubit gate (the gate's own matrix and its orientation), a ``U2`` for a coherent error, and a ``DEPOL1`` / ``DEPOL2``
    record per depolarising op; readout noise of measured qubits goes into the ``readout`` table.

    Raises ``ValueError`` naming the offender for what ``compile_programs`` refuses (unknown gates, parameter counts, qubits out of
    range or used after their measurement, non-finite angles, malformed terms) and for: a two-qubit gate on qubits that are no
    neighbours, ``max_bond`` outside 1 .. 32, ``noise`` without ``trajectories`` or the reverse, a model with thermal relaxation,
    readout noise together with an X / Y term, a circuit over 512 qubits."""
    circuits, observables = list(circuits), list(observables)
    max_bond, cutoff = _check_bond(max_bond, "compile_mps"), _check_cutoff(cutoff, "compile_mps")
    if trajectories is not None:
        trajectories = check_trajectories(trajectories, "compile_mps")
        if noise is None:
            raise ValueError("compile_mps: trajectories without a noise model (a noiseless circuit has one trajectory: lower it "
                             "without trajectories)")
    elif noise is not None:
        raise ValueError("compile_mps: noise without trajectories (the MPS path unravels a noise model into Pauli-insertion "
                         "trajectories: pass trajectories=T)")
    if len(circuits) != len(observables):
        raise ValueError(f"compile_mps: {len(circuits)} circuits but {len(observables)} observables")
    noisy = noise is not None
    relaxation_after, coherent_after = getattr(noise, "relaxation_after", None), getattr(noise, "coherent_after", None)
    ops, params, op_ptr = [], [], [0]
    term_circ, term_off, letters, coeffs, term_ptr = [], [], [], [], [0]
    site_ptr, readout, n_noise_all, abs_coeff, measured_all, n_qubits = [0], [], [], [], [], []
    gate_ptr, gate_name, gate_record, gate_noise, gate_noise_len = [0], [], [], [], []
    name_id = {g: j for j, g in enumerate(SUPPORTED_GATES)}

    def emit(kind, site, orient, values):
        ops.append((kind, site, orient, len(params)))
        params.extend(values)

    def emit_matrix(kind, site, orient, m):
        flat = []
        for e in np.asarray(m, dtype=complex).reshape(-1):
            flat += [float(e.real), float(e.imag)]
        emit(kind, site, orient, flat)

    for k, (obj, obs) in enumerate(zip(circuits, observables)):
        circ = Circuit.from_any(obj)
        where = f"circuit {k}"
        n = circ.num_qubits
        if not 1 <= n <= MAX_QUBITS_MPS:
            raise ValueError(f"{where}: {n} qubits; the MPS path takes 1 .. {MAX_QUBITS_MPS}")
        measured: Dict[int, int] = {}
        done = set()
        pending: Dict[int, np.ndarray] = {}    # ideal lowering: one-qubit matrices no record has absorbed yet
        open_bond: Dict[int, np.ndarray] = {}  # ideal lowering: lower site -> the 4x4 matrix accumulated on its bond
        n_noise = 0

        def flush(site):
            emit_matrix(OP_MPS_U2, site, 0, open_bond.pop(site))

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
            first, rec, noi, noi_len = op_ptr[-1], -1, -1, 0
            if width == 2:
                q0, q1 = op.qubits
                if q0 == q1:
                    raise ValueError(f"{where}: op {i} ({name}) names qubit {q0} twice")
                if abs(q0 - q1) != 1:
                    raise ValueError(f"{where}: op {i} ({name}): qubits {q0} and {q1} are not neighbours on the line; route with "
                                     "swaps first")
                lower, orient = min(q0, q1), int(q0 > q1)
                m = _matrix4(name, p)
                if noisy:
                    rec = len(ops) - first
                    emit_matrix(OP_MPS_U2, lower, orient, m)
                else:
                    for other in (lower - 1, lower + 1):
                        if other in open_bond:
                            flush(other)
                    m = _to_lower_basis(m, orient)
                    before = open_bond.get(lower)
                    if before is None:
                        before = np.kron(pending.pop(lower + 1, np.eye(2)), pending.pop(lower, np.eye(2))).astype(complex)
                    open_bond[lower] = m @ before
            else:
                q0 = op.qubits[0]
                m = _matrix2(name, p)
                if m is not None:
                    if noisy:
                        rec = len(ops) - first
                        emit_matrix(OP_MPS_U1, q0, 0, m)
                    else:
                        site = q0 if q0 in open_bond else q0 - 1 if q0 - 1 in open_bond else None
                        if site is None:
                            pending[q0] = m @ pending[q0] if q0 in pending else m
                        else:
                            full = np.kron(np.eye(2), m) if site == q0 else np.kron(m, np.eye(2))
                            open_bond[site] = full @ open_bond[site]
            if noisy:
                reg = tuple(circ.qubit_reg_index[q] for q in op.qubits)
                lam = noise.after_gate(i, name, reg)
                if lam is not None and not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
                    raise ValueError(f"{where}: op {i} ({name}): depolarising parameter {lam!r}, want 0 <= lambda <= 1")
                coherent = coherent_after(i, name, reg) if coherent_after is not None else None
                if relaxation_after is not None and relaxation_after(i, name, reg) is not None:
                    raise ValueError(f"{where}: op {i} ({name}): the noise model has thermal relaxation, whose jump probabilities "
                                     "depend on the state; the MPS path takes depolarising + readout models (and coherent two-qubit "
                                     "errors) only")
                if coherent is not None:
                    if width != 2:
                        raise ValueError(f"{where}: op {i} ({name}): a coherent error is a 4x4 unitary, the gate has one qubit")
                    noi = len(ops) - first
                    emit_matrix(OP_MPS_U2, min(op.qubits), int(op.qubits[0] > op.qubits[1]), _check_coherent((name, reg), coherent))
                    noi_len += 1
                if lam is not None:
                    noi = len(ops) - first if noi < 0 else noi
                    noi_len += 1
                    if width == 2:
                        emit(OP_MPS_DEPOL2, min(op.qubits), int(op.qubits[0] > op.qubits[1]), [float(lam)])
                    else:
                        emit(OP_MPS_DEPOL1, op.qubits[0], 0, [float(lam)])
                    n_noise += 1
                gate_name.append(name_id[name])
                gate_record.append(rec)
                gate_noise.append(noi)
                gate_noise_len.append(noi_len)
        for site in sorted(open_bond):
            flush(site)
        for q in sorted(pending):
            emit_matrix(OP_MPS_U1, q, 0, pending[q])

        rows, cs, has_xy = _lower_terms(obs, n, where)
        table = [[1.0, 0.0] for _ in range(n)]
        if noisy:
            for q in sorted(set(measured.values())):
                pr = noise.readout_of(circ.qubit_reg_index[q])
                if pr is None:
                    continue
                if has_xy:
                    raise ValueError(f"{where}: readout noise on qubit {q} cannot be combined with an observable that has X or Y "
                                     "terms (the readout channel of a trajectory acts on the outcome distribution, which has "
                                     "only I / Z terms)")
                p01, p10 = float(pr[0]), float(pr[1])
                table[q] = [1.0 - p01 - p10, p01 - p10]
        for xm, zm, _, _ in rows:
            term_circ.append(k)
            term_off.append(len(letters))
            letters += [(1 if xm >> q & 1 else 0) * (2 if zm >> q & 1 else 1) + (3 if zm >> q & 1 and not xm >> q & 1 else 0)
                        for q in range(n)]
        coeffs += cs
        term_ptr.append(len(term_circ))
        readout += table
        site_ptr.append(len(readout))
        op_ptr.append(len(ops))
        n_noise_all.append(n_noise)
        abs_coeff.append(float(sum(abs(c) for c in cs)))
        measured_all.append(measured)
        n_qubits.append(n)
        gate_ptr.append(len(gate_record))

    if len(params) + PARAM_PAD > 2 ** 31 - 1:
        raise ValueError(f"compile_mps: {len(params)} gate parameters exceed the 2^31 - 1 a record can address; split the batch")
    return MpsBatch(
        n_qubits=np.asarray(n_qubits, dtype=np.int32), op_ptr=np.asarray(op_ptr, dtype=np.int64),
        ops=np.asarray(ops, dtype=np.int32).reshape(-1, 4), params=np.asarray(params + [0.0] * PARAM_PAD, dtype=np.float64),
        term_ptr=np.asarray(term_ptr, dtype=np.int64), term_circ=np.asarray(term_circ, dtype=np.int32),
        term_off=np.asarray(term_off, dtype=np.int64), letters=np.asarray(letters + [0], dtype=np.uint8),
        coeff=np.asarray(coeffs, dtype=np.float64), site_ptr=np.asarray(site_ptr, dtype=np.int64),
        readout=np.asarray(readout + [[1.0, 0.0]], dtype=np.float64).reshape(-1, 2), max_bond=max_bond, cutoff=cutoff,
        trajectories=trajectories, n_noise=n_noise_all, abs_coeff=abs_coeff, measured=measured_all,
        gate_ptr=np.asarray(gate_ptr, dtype=np.int64) if noisy else None, gate_name=np.asarray(gate_name, dtype=np.int16) if noisy else None,
        gate_record=np.asarray(gate_record, dtype=np.int32) if noisy else None,
        gate_noise=np.asarray(gate_noise, dtype=np.int32) if noisy else None,
        gate_noise_len=np.asarray(gate_noise_len, dtype=np.int32) if noisy else None)


@dataclass
class MpsResult:
    """What one MPS run produced: tensors on the device, the terms CSR over ``term_ptr``."""

    values: Any             # float64 [B]: sum coeff * term (the mean over the trajectories when there are any)
    term_values: Any        # float64 [n_terms]: <P> / <psi|psi>
    norm: Any               # float64 [B]: <psi|psi> of the final state (1 up to rounding)
    term_ptr: Any           # int64 [B + 1]
    discarded: Any          # float64 [B]: sum over the decompositions of the relative discarded weight (mean over trajectories)
    error_bound: Any        # float64 [B]: the certificate B = sum sqrt(2 eps) (mean over trajectories)
    bond: Any               # int32 [B]: the largest bond reached
    std_error: Any = None        # float64 [B], with trajectories
    term_std_error: Any = None   # float64 [n_terms], with trajectories
    trajectories: Optional[int] = None
    seed: int = 0
    traj_term_values: Any = None   # float64 [T, n_terms] with ``keep_trajectories``
    traj_stats: Any = None         # float64 [T, B, 6] with it: discarded, error_bound, largest bond, decompositions, those not converged, most sweeps
    batch: Optional[MpsBatch] = None


def _mps_chunks(batch: MpsBatch, trajectories: int, buffer_bytes: int, unit_bytes=None):
    """``(circuit range, trajectory range)`` pairs whose site-tensor workspace (n * chi * 2 * chi * 16 B per unit, plus the stash)
    stays under ``buffer_bytes``: whole circuits with all their trajectories while they fit, else one circuit with a part of them.
    A chunk holds at least one unit.  ``unit_bytes(width)``: the bytes of one unit where they are more than that workspace."""
    from ..native import ops

    if unit_bytes is None:
        def unit_bytes(width):
            return ops.mps_workspace_bytes(width, batch.max_bond, 1)

    chunks, lo, b = [], 0, len(batch)
    while lo < b:
        hi, widest = lo + 1, int(batch.n_qubits[lo])
        per = unit_bytes(widest)
        if per * trajectories > buffer_bytes:
            step = max(int(buffer_bytes // per), 1)
            chunks += [(range(lo, hi), range(t0, min(t0 + step, trajectories))) for t0 in range(0, trajectories, step)]
        else:
            while hi < b:
                wider = max(widest, int(batch.n_qubits[hi]))
                if unit_bytes(wider) * trajectories * (hi + 1 - lo) > buffer_bytes:
                    break
                widest, hi = wider, hi + 1
            chunks.append((range(lo, hi), range(0, trajectories)))
        lo = hi
    return chunks


def run_mps(batch: MpsBatch, seed: int = 0, run_keys=None, device="cuda", keep_trajectories: bool = False,
            buffer_bytes: int = None) -> MpsResult:
    """Runs a batch lowered by :func:`compile_mps` on the device.  ``run_keys``: one integer per circuit, by default its position in
    the batch; a unit's bits depend on (seed, run key, trajectory number, the circuit's records) alone, so a circuit gives the
    same values alone, in any batch and under any split.  The (circuit, trajectory) units are split into launches so that the
    site-tensor workspace stays under ``buffer_bytes`` (default :data:`MPS_BUFFER_BYTES`).  Returns an :class:`MpsResult`."""
    import torch

    from ..native import ops
    from .run import _run_keys

    seed = check_seed(seed, "run_mps")
    n_traj = 1 if batch.trajectories is None else check_trajectories(batch.trajectories, "run_mps")
    keys = _run_keys(run_keys, len(batch), "run_mps")
    buffer_bytes = MPS_BUFFER_BYTES if buffer_bytes is None else int(buffer_bytes)
    if buffer_bytes < 1:
        raise ValueError(f"run_mps: buffer_bytes = {buffer_bytes!r}, want a positive number of bytes")
    dev = torch.device(device)
    t = batch.to(dev)
    b, n_terms = len(batch), int(batch.term_circ.shape[0])
    if b == 0:
        empty = torch.zeros(0, dtype=torch.float64, device=dev)
        return MpsResult(empty, empty.clone(), empty.clone(), t["term_ptr"], empty.clone(), empty.clone(),
                         torch.zeros(0, dtype=torch.int32, device=dev), None if batch.trajectories is None else empty.clone(),
                         None if batch.trajectories is None else empty.clone(), batch.trajectories, seed, None, None, batch)
    keys_t = torch.from_numpy(keys).to(dev)
    traj_terms = torch.zeros((n_traj, n_terms), dtype=torch.float64, device=dev)
    traj_norm = torch.zeros((n_traj, b), dtype=torch.float64, device=dev)
    traj_stats = torch.zeros((n_traj, b, ops.MPS_STATS), dtype=torch.float64, device=dev)
    chunks = _mps_chunks(batch, n_traj, buffer_bytes)
    need = max(ops.mps_workspace_bytes(int(batch.n_qubits[list(cr)].max()), batch.max_bond, len(cr) * len(tr)) for cr, tr in chunks)
    workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    for cr, tr in chunks:
        ops.sim_run_mps(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], keys_t, t["term_circ"], t["term_off"], t["letters"],
                        t["site_ptr"], t["readout"], (cr.start, len(cr)),
                        (int(batch.term_ptr[cr.start]), int(batch.term_ptr[cr.stop] - batch.term_ptr[cr.start])), (tr.start, len(tr)),
                        n_traj, seed, batch.max_bond, batch.cutoff, int(batch.n_qubits[list(cr)].max()), workspace, traj_terms, traj_norm,
                        traj_stats)
    out = ops.sim_mps_finish(t["term_ptr"], t["coeff"], traj_terms, traj_norm, traj_stats)
    noisy = batch.trajectories is not None
    return MpsResult(out["values"], out["term_values"], out["norm"], t["term_ptr"], out["discarded"], out["error_bound"], out["bond"],
                     out["std_error"] if noisy else None, out["term_std_error"] if noisy else None, batch.trajectories, seed,
                     traj_terms if keep_trajectories else None, traj_stats if keep_trajectories else None, batch)


def mps_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                           max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF, trajectories: Optional[int] = None, seed: int = 0,
                           run_keys=None, device="cuda") -> MpsResult:
    """Expectation values of ``observables[k]`` after ``circuits[k]`` by matrix-product states of bond at most ``max_bond``:
    circuits of up to 512 qubits whose two-qubit gates act on neighbours, any angle.  ``noise`` + ``trajectories``: the values
    under a depolarising + readout model, as means over Pauli-insertion trajectories with their standard errors."""
    return run_mps(compile_mps(circuits, observables, noise, trajectories, max_bond, cutoff), seed, run_keys, device)


# ---- shots ------------------------------------------------------------------------------------------------------------------------
MAX_GROUPS_MPS = 4096    # MLQEM_MPS_MAX_GROUPS: measurement groups per circuit (12 bits of a Philox counter word)
_PAD = 32


def _mask_words(mask: int, w: int) -> List[int]:
    return [(mask >> (32 * j)) & 0xFFFFFFFF for j in range(w)]


@dataclass
class MpsShotsBatch:
    """A batch lowered for ``mlqem_mps_sample_f64``: ``mps`` is the same batch lowered by :func:`compile_mps` (its records, terms and
    ``site_ptr`` are the ones used here), the rest are the measurement groups."""

    mps: MpsBatch
    group_ptr: np.ndarray    # int64 [B + 1]
    group_circ: np.ndarray   # int32 [n_groups]
    group_off: np.ndarray    # int64 [n_groups]: the group's first letter in ``basis``
    basis: np.ndarray        # uint8 [n_basis + 32]: one letter per (group, site): 1 X, 2 Y, 3 Z (0: padding)
    flip: np.ndarray         # float64 [n_sites, 2]: (P(read 1 | 0), P(read 0 | 1)) of every site; (0, 0) without readout noise
    ref_ptr: np.ndarray      # int64 [n_groups + 1]: the group's W words of a shot; times shots, in ``bits``
    gterm_ptr: np.ndarray    # int64 [n_groups + 1]
    gterm: np.ndarray        # int32 [n_terms]: the terms by group
    term_mask: np.ndarray    # int32 [n_terms]: the support in masks, W words
    term_group: np.ndarray   # int32 [n_terms]: the term's group inside its circuit
    masks: np.ndarray        # uint32 [n_masks + 32]
    max_groups: int = 1

    def __len__(self) -> int:
        return len(self.mps)

    @property
    def n_qubits(self) -> np.ndarray:
        return self.mps.n_qubits

    @property
    def trajectories(self) -> Optional[int]:
        return self.mps.trajectories

    def to(self, device) -> Dict[str, Any]:
        import torch

        dev = torch.device(device)
        out = self.mps.to(dev)
        for k in ("group_ptr", "group_circ", "group_off", "basis", "flip", "ref_ptr", "gterm_ptr", "gterm", "term_mask"):
            out[k] = torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(dev)
        out["masks"] = torch.from_numpy(np.ascontiguousarray(self.masks).view(np.int32)).to(dev)
        return out


def compile_mps_shots(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                      trajectories: Optional[int] = None, max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF) -> MpsShotsBatch:
    """The lowering of :func:`compile_mps` plus the measurement groups of :func:`~blackwater.sim.measurement_groups`: one basis
    letter per (group, site) (Z where no term of the group touches the site), the ``flip`` table of the measured qubits' readout
    noise, a support mask per term and the group of each term.  What ``compile_mps`` refuses stays refused, by the same messages
    (X or Y terms beside readout noise, thermal relaxation, gates on qubits that are no neighbours, ...); also refused: a circuit
    whose terms need more than 4 096 measurement groups."""
    circuits, observables = list(circuits), list(observables)
    base = compile_mps(circuits, observables, noise, trajectories, max_bond, cutoff)   # every check and refusal
    group_ptr, group_circ, group_off, basis, ref_ptr = [0], [], [], [], [0]
    gterm_ptr, gterm, term_mask, term_group, masks, flip = [0], [], [], [], [], []
    max_groups = 1
    for k, (obj, obs) in enumerate(zip(circuits, observables)):
        circ = Circuit.from_any(obj)
        n = circ.num_qubits
        w = (n + 31) // 32
        rows, _, _ = _lower_terms(obs, n, f"circuit {k}")
        first_term = len(term_mask)
        for xm, zm, _, _ in rows:
            term_mask.append(len(masks))
            masks += _mask_words(xm | zm, w)
        groups_of, bases = measurement_groups(rows)
        if len(bases) > MAX_GROUPS_MPS:
            raise ValueError(f"circuit {k}: its terms need {len(bases)} measurement groups; MPS sampling takes at most {MAX_GROUPS_MPS} "
                             "per circuit (split the observable)")
        max_groups = max(max_groups, len(bases))
        term_group += groups_of
        for g, (gx, gy) in enumerate(bases):
            group_circ.append(k)
            group_off.append(len(basis))
            basis += [1 if gx >> q & 1 else 2 if gy >> q & 1 else 3 for q in range(n)]
            members = [first_term + t for t, tg in enumerate(groups_of) if tg == g]
            gterm += members
            gterm_ptr.append(len(gterm))
            ref_ptr.append(ref_ptr[-1] + w)
        group_ptr.append(len(group_circ))
        table = [[0.0, 0.0] for _ in range(n)]
        if noise is not None:
            for q in sorted(set(base.measured[k].values())):
                pr = noise.readout_of(circ.qubit_reg_index[q])
                if pr is not None:
                    table[q] = [float(pr[1]), float(pr[0])]   # (p01, p10) -> (P(read 1 | 0), P(read 0 | 1))
        flip += table
    if len(masks) + _PAD > 2 ** 31 - 1 or len(basis) + _PAD > 2 ** 31 - 1:
        raise ValueError("compile_mps_shots: the batch exceeds what one call can address; split it")
    return MpsShotsBatch(
        mps=base, group_ptr=np.asarray(group_ptr, dtype=np.int64), group_circ=np.asarray(group_circ, dtype=np.int32),
        group_off=np.asarray(group_off, dtype=np.int64), basis=np.asarray(basis + [0] * _PAD, dtype=np.uint8),
        flip=np.asarray(flip + [[0.0, 0.0]], dtype=np.float64).reshape(-1, 2), ref_ptr=np.asarray(ref_ptr, dtype=np.int64),
        gterm_ptr=np.asarray(gterm_ptr, dtype=np.int64), gterm=np.asarray(gterm, dtype=np.int32),
        term_mask=np.asarray(term_mask, dtype=np.int32), term_group=np.asarray(term_group, dtype=np.int32),
        masks=np.asarray(masks + [0] * _PAD, dtype=np.uint32), max_groups=max_groups)


@dataclass
class MpsShotsResult:
    """What one sampled MPS call produced: tensors on the device.  The fields of ``FrameResult`` (there is no reference outcome:
    every shot is drawn from the state), plus the run's ``discarded``, ``error_bound`` and ``bond``.  ``bits`` are packed uint32 words
    carried as int32, CSR over ``ref_ptr`` (the W = ceil(n / 32) words of a group; a group's bits are ``[shots, W]`` from
    ``ref_ptr[g] * shots``).

    ``variance`` is the per-shot variance sum coeff^2 (1 - estimate^2), as on the other sampled paths.  Under noise shot s comes
    from trajectory s mod T: every shot is marginally a draw from the noisy distribution, but with T < shots the shots of one
    trajectory share a noise realisation, so the standard error of the estimate also has the between-trajectory part that
    ``mps_expectation_values(...).std_error`` reports; T = shots gives independent shots.  The sampled distribution is that of the
    truncated state: its trace distance from the exact state's is at most ``error_bound``."""

    values: Any          # float64 [B]: sum coeff * sampled term estimate
    variance: Any        # float64 [B]: sum coeff^2 (1 - estimate^2)
    term_values: Any     # float64 [n_terms]
    term_ptr: Any        # int64 [B + 1]
    term_sums: Any       # int32 [n_terms]: S_t = sum over the shots of (-1)^popcount(bits & support)
    ref_ptr: Any         # int64 [n_groups + 1]
    group_ptr: Any       # int64 [B + 1]
    discarded: Any       # float64 [B] (mean over the trajectories)
    error_bound: Any     # float64 [B] (mean over the trajectories)
    bond: Any            # int32 [B]
    bits: Any = None     # int32 [n_ref * shots], with return_bits
    shots: int = 0
    seed: int = 0
    trajectories: Optional[int] = None
    batch: Optional[MpsShotsBatch] = None


def run_mps_shots(batch: MpsShotsBatch, shots: int, seed: int = 0, run_keys=None, return_bits: bool = False, device="cuda",
                  buffer_bytes: int = None) -> MpsShotsResult:
    """Samples ``shots`` outcomes of every (circuit, group) of a batch lowered by :func:`compile_mps_shots`.  Per chunk of (circuit,
    trajectory) units the MPS is run and then sampled; ``buffer_bytes`` (default :data:`MPS_BUFFER_BYTES`) bounds the site-tensor
    workspace and the environment workspace of a chunk together.  ``run_keys`` as in :func:`run_mps`; the bits of a (circuit,
    group, shot) depend on (seed, run key, group, shot, the circuit's records, max_bond, cutoff, trajectories) alone.  Nothing is
    read back."""
    import torch

    from ..native import ops
    from .program import check_shots
    from .run import _run_keys

    shots, seed = check_shots(shots, "run_mps_shots"), check_seed(seed, "run_mps_shots")
    mps = batch.mps
    n_traj = 1 if mps.trajectories is None else check_trajectories(mps.trajectories, "run_mps_shots")
    if n_traj > shots:
        raise ValueError(f"run_mps_shots: trajectories = {n_traj} exceed shots = {shots} (shot s comes from trajectory s mod "
                         "trajectories: the others would be simulated and never measured)")
    keys = _run_keys(run_keys, len(batch), "run_mps_shots")
    buffer_bytes = MPS_BUFFER_BYTES if buffer_bytes is None else int(buffer_bytes)
    if buffer_bytes < 1:
        raise ValueError(f"run_mps_shots: buffer_bytes = {buffer_bytes!r}, want a positive number of bytes")
    dev = torch.device(device)
    t = batch.to(dev)
    b, n_terms = len(batch), int(mps.term_circ.shape[0])
    zeros = lambda n, dtype=torch.float64: torch.zeros(n, dtype=dtype, device=dev)   # noqa: E731
    if b == 0:
        return MpsShotsResult(zeros(0), zeros(0), zeros(0), t["term_ptr"], zeros(0, torch.int32), t["ref_ptr"], t["group_ptr"], zeros(0),
                              zeros(0), zeros(0, torch.int32), zeros(0, torch.int32) if return_bits else None, shots, seed,
                              mps.trajectories, batch)
    keys_t = torch.from_numpy(keys).to(dev)
    traj_stats = zeros((n_traj, b, ops.MPS_STATS))
    term_sums = zeros(n_terms, torch.int32)
    bits = zeros(int(batch.ref_ptr[-1]) * shots, torch.int32) if return_bits else None

    def unit_bytes(width):
        return ops.mps_workspace_bytes(width, mps.max_bond, 1) + ops.mps_sample_workspace_bytes(width, mps.max_bond, 1)

    chunks = _mps_chunks(mps, n_traj, buffer_bytes, unit_bytes)
    widest = [int(mps.n_qubits[list(cr)].max()) for cr, _ in chunks]
    workspace = torch.empty((max(ops.mps_workspace_bytes(w, mps.max_bond, len(cr) * len(tr)) for w, (cr, tr) in zip(widest, chunks)),),
                            dtype=torch.uint8, device=dev)
    env = torch.empty((max(ops.mps_sample_workspace_bytes(w, mps.max_bond, len(cr) * len(tr)) for w, (cr, tr) in zip(widest, chunks)),),
                      dtype=torch.uint8, device=dev)
    for w, (cr, tr) in zip(widest, chunks):
        ops.mps_run(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], keys_t, (cr.start, len(cr)), (tr.start, len(tr)), n_traj, seed,
                    mps.max_bond, mps.cutoff, w, workspace, traj_stats)
        g0, g1 = int(batch.group_ptr[cr.start]), int(batch.group_ptr[cr.stop])
        t0, t1 = int(mps.term_ptr[cr.start]), int(mps.term_ptr[cr.stop])
        ops.mps_sample(t["n_qubits"], (cr.start, len(cr)), (tr.start, len(tr)), n_traj, mps.max_bond, w, workspace, env, (g0, g1 - g0),
                       batch.max_groups, t["group_ptr"], t["group_circ"], t["group_off"], t["basis"], t["site_ptr"], t["flip"], t["ref_ptr"],
                       t["gterm_ptr"], t["gterm"], (t0, t1 - t0), t["term_mask"], t["masks"], keys_t, shots, seed, term_sums, bits)
    stats = ops.sim_mps_finish(t["term_ptr"], t["coeff"], zeros((n_traj, n_terms)), zeros((n_traj, b)), traj_stats)
    values, variance, term_values = ops.mps_sample_finish(t["term_ptr"], t["coeff"], term_sums, shots)
    return MpsShotsResult(values, variance, term_values, t["term_ptr"], term_sums, t["ref_ptr"], t["group_ptr"], stats["discarded"],
                          stats["error_bound"], stats["bond"], bits, shots, seed, mps.trajectories, batch)


def sample_mps_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None, *,
                                  shots: int = None, trajectories: Optional[int] = None, max_bond: int = MAX_BOND,
                                  cutoff: float = DEFAULT_CUTOFF, seed: int = 0, run_keys=None, return_bits: bool = False,
                                  device="cuda") -> MpsShotsResult:
    """Expectation values of ``observables[k]`` after ``circuits[k]`` estimated from ``shots`` measurement outcomes per measurement
    basis, drawn from the matrix-product state of bond at most ``max_bond``: circuits of up to 512 qubits whose two-qubit gates act on
    neighbours, any angle; ideal, or under a depolarising + readout ``noise`` model with ``trajectories``.  The limit of every
    estimate is the value :func:`mps_expectation_values` gives."""
    from .program import check_shots

    if shots is None:
        raise ValueError("sample_mps_expectation_values: shots is required (an int in 1 .. 2^20); mps_expectation_values gives the "
                         "values without shot noise")
    shots = check_shots(shots, "sample_mps_expectation_values")
    return run_mps_shots(compile_mps_shots(circuits, observables, noise, trajectories, max_bond, cutoff), shots, seed, run_keys,
                         return_bits, device)


def mps_counts(result: MpsShotsResult, k: int) -> List[Dict[str, int]]:
    """``{bitstring: count}`` per measurement group of circuit ``k``: qiskit's strings, n characters, qubit 0 the RIGHTMOST -- what
    ``cal_z_exp`` / ``counts_to_feature_vector`` take.  Needs ``return_bits=True``; reads that circuit's bits back from the device."""
    if result.bits is None:
        raise ValueError("mps_counts: the result has no bits (run it with return_bits=True)")
    batch = result.batch
    if not 0 <= k < len(batch):
        raise ValueError(f"mps_counts: circuit {k} of {len(batch)}")
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
