"""Matrix-product-state simulation of circuits on a line: labels for wide circuits that are not Clifford circuits.

``compile_mps`` lowers circuits whose two-qubit gates all act on neighbouring qubits (q, q + 1) to the records of
``mlqem_mps_run_f64`` (include/mlqem_hip.h has the layouts, the keep rule and the draw contract); nothing in it touches the GPU.
``run_mps`` runs a lowered batch on the device, ``mps_expectation_values`` is the one-call form.  Ideal values are exact while no
bond needs more than ``max_bond`` (TFIM circuits: through 5 Trotter steps at bond 32) and come with an a-priori certificate
beyond: ``error_bound`` B bounds the distance of the states, so |<O>_exact - <O>_mps| <= 2 B sum|coeff|.  With a depolarising +
readout noise model and ``trajectories`` the same kernel gives noisy values: every depolarising record inserts one drawn Pauli
string (its probabilities do not depend on the state), readout noise is folded into the measured operators.  With
``thermal_relaxation=True`` a model with thermal relaxation (``NoiseModel.from_backend(..., thermal_relaxation=True)``) is taken too:
a ``NOISE1`` / ``NOISE2`` record per relaxed gate, unravelled into quantum jumps at the orthogonality centre; ``error_bound`` is then
a per-trajectory certificate, conditional on the jumps drawn, with the constant 4 in the place of 2.  Templates and folded runs
refuse such a model by name.  With ``pauli_twirl=`` (noisy lowering) the two-qubit gates cx, cz, ecr, swap are Pauli-twirled on the
device: ``TWIRL_OPEN`` / ``TWIRL_CLOSE`` records around the gate and its noise, one draw of 16 Pauli pairs per (run, trajectory) and
gate, the circuits lowered once; plain runs, shots and folded runs take such a batch, templates refuse it by name.

``compile_mps_shots`` / ``run_mps_shots`` / ``sample_mps_expectation_values`` draw measurement shots from the same states
(``mlqem_mps_sample_f64``: perfect sampling, one sweep over the sites per shot), ``mps_counts`` gives the count dictionaries.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..data.circuit import Circuit
from .program import (_N_PARAMS, _TWO_QUBIT, OP_DIAG1, PARAM_PAD, SUPPORTED_GATES, NoiseModel, _check_coherent, _check_relaxation,
                      _lower_terms, _one_qubit, _run_keys, _two_qubit, check_seed, check_trajectories, measurement_groups, upload,
                      upload_fields)

MAX_BOND = 32            # MLQEM_MPS_MAX_BOND: theta, (2 chi) x (2 chi) complex128 = 64 KiB, sits in LDS beside a second workgroup
MAX_QUBITS_MPS = 512     # MLQEM_MPS_MAX_QUBITS
MPS_BUFFER_BYTES = 4 << 30   # the site-tensor workspace of one launch stays under this (``buffer_bytes=``): 1 300 units of 100 qubits
DEFAULT_CUTOFF = 1e-26   # relative weight below which a column is dropped: the numerically-zero columns of a rank-deficient theta
OP_MPS_U1, OP_MPS_U2, OP_MPS_DEPOL1, OP_MPS_DEPOL2 = 0, 5, 6, 7   # MLQEM_MPS_OP_*
OP_MPS_NOISE1, OP_MPS_NOISE2 = 10, 11   # depolarising, then thermal relaxation of the gate's qubits (thermal_relaxation=True)
OP_MPS_TWIRL_OPEN, OP_MPS_TWIRL_CLOSE = 17, 18   # a Pauli twirl around a two-qubit gate and its noise (pauli_twirl=)
TWIRL_GATES = ("cx", "cz", "ecr", "swap")   # the self-inverse two-qubit Cliffords: one table serves the gate and its dagger
TWIRL_DEFAULT = ("cx", "cz", "ecr")         # what pauli_twirl=True twirls

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
    gate_noise_len: Optional[np.ndarray] = None   # int32 [n_gates]: 0, 1 (DEPOL* / NOISE*) or 2 (a coherent U2, then DEPOL* / NOISE*)
    # with ``pauli_twirl=`` (else None): the TWIRL_OPEN record before a twirled gate and the TWIRL_CLOSE record after its noise
    gate_twirl_open: Optional[np.ndarray] = None    # int32 [n_gates]
    gate_twirl_close: Optional[np.ndarray] = None   # int32 [n_gates]

    def __len__(self) -> int:
        return int(self.n_qubits.shape[0])

    def to(self, device) -> Dict[str, Any]:
        return upload_fields(self, ("n_qubits", "op_ptr", "ops", "params", "term_ptr", "term_circ", "term_off", "letters", "coeff", "site_ptr",
                                    "readout"), device)


def is_line_circuit(circuit: Any) -> bool:
    """Whether every two-qubit gate of the circuit acts on neighbouring qubits (q, q + 1), in either order."""
    return all(len(op.qubits) != 2 or op.name in ("barrier", "measure") or abs(op.qubits[0] - op.qubits[1]) == 1
               for op in Circuit.from_any(circuit).ops)


def refuse_records(batch: Any, who: str, kinds: Sequence[int], text: str) -> None:
    """Raises, naming the first one, where a batch holds a record of one of ``kinds``: ``text`` says what it is and who takes it."""
    hit = np.flatnonzero(np.isin(np.asarray(batch.ops).reshape(-1, 4)[:, 0], kinds))
    if hit.size:
        raise ValueError(f"{who}: record {int(hit[0])} of the batch is {text}")


def refuse_relaxation_records(batch: Any, who: str) -> None:
    """Raises where a batch holds a ``NOISE1`` / ``NOISE2`` record (``compile_mps(..., thermal_relaxation=True)``, or built by
    hand): the folded kernel and the bind kernel do not run them."""
    refuse_records(batch, who, (OP_MPS_NOISE1, OP_MPS_NOISE2),
                   "a thermal-relaxation record (NOISE1 / NOISE2, compile_mps(..., thermal_relaxation=True)); folded runs and templates on "
                   "the matrix-product-state path take depolarising + readout models only (relaxation there is not built: run_mps runs "
                   "such a batch)")


def refuse_twirl_records(batch: Any, who: str) -> None:
    """Raises where a batch holds a ``TWIRL_OPEN`` / ``TWIRL_CLOSE`` record (``compile_mps(..., pauli_twirl=)``, or built by hand):
    the bind kernel copies one value of a kind it does not know, and a ``TWIRL_CLOSE`` record has a table of 16."""
    refuse_records(batch, who, (OP_MPS_TWIRL_OPEN, OP_MPS_TWIRL_CLOSE),
                   "a Pauli-twirl record (TWIRL_OPEN / TWIRL_CLOSE, compile_mps(..., pauli_twirl=)); templates on the "
                   "matrix-product-state path do not take twirled batches (mlqem_mps_bind_f64 copies one value of a record it does not "
                   "know, a TWIRL_CLOSE table has 16: not built; run_mps and run_mps_folded run such a batch)")


def _check_twirl(pauli_twirl: Any, who: str) -> tuple:
    """The names ``pauli_twirl=`` asks to twirl, in the order of :data:`TWIRL_GATES`: () for ``False`` / ``None``."""
    if pauli_twirl is None or pauli_twirl is False or (isinstance(pauli_twirl, np.bool_) and not pauli_twirl):
        return ()
    if pauli_twirl is True or isinstance(pauli_twirl, np.bool_):
        return TWIRL_DEFAULT
    if isinstance(pauli_twirl, str):
        pauli_twirl = (pauli_twirl,)
    try:
        names = [g for g in pauli_twirl]
    except TypeError:
        names = None
    if names is None or not names or not all(isinstance(g, str) for g in names):
        raise ValueError(f"{who}: pauli_twirl = {pauli_twirl!r}, want True, False or a sequence of gate names from "
                         f"{' '.join(TWIRL_GATES)}")
    for g in names:
        if g not in TWIRL_GATES:
            raise ValueError(f"{who}: pauli_twirl names {g!r}; only the self-inverse two-qubit Clifford gates {' '.join(TWIRL_GATES)} "
                             "are twirled (folding a gate with G^dagger = G needs one table)")
    return tuple(g for g in TWIRL_GATES if g in names)


_MPS_TO_CLIFFORD = (0, 1, 3, 2)   # a letter 0 I, 1 X, 2 Y, 3 Z of this path as a letter of ``clifford`` (0 I, 1 X, 2 Z, 3 Y), and back


def _swap_yz(code: int) -> int:
    return _MPS_TO_CLIFFORD[code & 3] | _MPS_TO_CLIFFORD[code >> 2] << 2


def twirl_table(name: str) -> List[int]:
    """``table[code]`` of a ``TWIRL_CLOSE`` record: the code (letter ``& 3`` on q0, ``>> 2`` on q1; 0 I, 1 X, 2 Y, 3 Z) of the pair
    P' with P' ~ G P G^dagger for the gate's own matrix G, signs dropped.  Over the gate's (q0, q1): no orientation enters."""
    from .clifford import conjugation_table

    if name not in TWIRL_GATES:
        raise ValueError(f"twirl_table: {name!r} is not one of {' '.join(TWIRL_GATES)}")
    g = _matrix4(name, ())
    back, forth = conjugation_table(g), conjugation_table(g.conj().T)   # G^dagger P G and G P G^dagger
    assert back is not None and back == forth, f"{name} is not a self-inverse Clifford gate"
    table = [0] + [_swap_yz(forth[_swap_yz(code) - 1][0]) for code in range(1, 16)]
    assert sorted(table) == list(range(16))
    return table


def _check_bond(max_bond: Any, who: str) -> int:
    if isinstance(max_bond, bool) or not isinstance(max_bond, (int, np.integer)) or not 1 <= int(max_bond) <= MAX_BOND:
        raise ValueError(f"{who}: max_bond = {max_bond!r}, want an int in 1 .. {MAX_BOND} (bond 64 needs theta outside LDS: not built)")
    return int(max_bond)


def _check_cutoff(cutoff: Any, who: str) -> float:
    if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float, np.floating)) or not 0.0 <= float(cutoff) < 1.0:
        raise ValueError(f"{who}: cutoff = {cutoff!r}, want a relative weight in [0, 1)")
    return float(cutoff)


FACTOR_FIXED = 0   # MLQEM_MPS_FACTOR_FIXED; a PARAM factor carries its MLQEM_SIM_OP_P* kind (12 .. 16)
SLOT_LOWER, SLOT_UPPER, SLOT_BOND = 0, 1, 2   # what a PARAM factor of a U2 record acts on (a U1 record: SLOT_LOWER)


class _Chain:
    """The matrix of one record as the product F_k ... F_2 F_1: a FIXED factor is a numpy matrix (consecutive fixed gates are
    multiplied into one, by the operations ``compile_mps`` has always done), a PARAM factor the list [kind, slot, Param,
    occurrence].  A chain without a PARAM factor has exactly one factor: the record's host matrix."""

    __slots__ = ("factors", "trivial", "gates")

    def __init__(self, first: Optional[np.ndarray] = None, trivial: bool = False, gates: int = 1):
        self.factors: List[Any] = [] if first is None else [first]
        self.trivial = trivial   # the only factor is the identity of a bond that absorbed no pending gate
        self.gates = gates if first is not None else 0   # gates multiplied into the record (what its rounding grows with)

    def fixed(self, m: np.ndarray) -> None:
        if self.factors and isinstance(self.factors[-1], np.ndarray):
            self.factors[-1] = m @ self.factors[-1]
        else:
            self.factors.append(m)
        self.trivial = False
        self.gates += 1

    def param(self, kind: int, slot: int, par: Any, occ: int) -> None:
        if self.trivial:
            self.factors, self.trivial = [], False
        self.factors.append([kind, slot, par, occ])
        self.gates += 1

    @property
    def parameterised(self) -> bool:
        return any(not isinstance(f, np.ndarray) for f in self.factors)

    def placeholder(self, dim: int) -> np.ndarray:
        """The product with every free parameter at 0."""
        m = np.eye(dim, dtype=complex)
        for f in self.factors:
            m = (f if isinstance(f, np.ndarray) else param_matrix(f[0], f[1], dim, f[2].value(_Zeros()))) @ m
        return m


class _Zeros:
    def __getitem__(self, index):
        return 0.0


_PARAM_NAME = {12: "rx", 13: "ry", 14: "rz", 15: "p", 16: "rzz"}   # MLQEM_SIM_OP_PRX .. PRZZ


def param_matrix(kind: int, slot: int, dim: int, phi: float) -> np.ndarray:
    """The matrix of a PARAM factor at the angle ``phi``, from ``program``'s tables: 2x2 (``dim`` 2), or 4x4 over bit(lower) + 2
    bit(upper) with the gate on ``slot``."""
    if kind == 16:
        return _matrix4("rzz", (phi,))
    g = _matrix2(_PARAM_NAME[kind], (phi,))
    if dim == 2:
        return g
    return np.kron(np.eye(2), g) if slot == SLOT_LOWER else np.kron(g, np.eye(2))


class _Lowering:
    """The per-circuit loop of :func:`compile_mps`, shared with :func:`compile_mps_templates`: every check, refusal, fusion
    decision and noise record of the MPS lowering lives here and nowhere else.  ``add`` lowers one circuit; with ``free`` (the
    ``Param`` of every op of a template, or None) it also keeps, for every record whose matrix depends on a parameter, the factor
    program of the record and the occurrences of the parameters."""

    def __init__(self, who, circuits, observables, noise, trajectories, max_bond, cutoff, thermal_relaxation=False, pauli_twirl=None):
        self.who = who
        self.twirl = _check_twirl(pauli_twirl, who)
        if self.twirl and (noise is None or trajectories is None):
            raise ValueError(f"{who}: pauli_twirl on the ideal lowering (gates are fused into bond records there, and a twirl of an "
                             "ideal gate changes nothing: twirling needs noise= and trajectories=)")
        self.twirl_tables = {g: [float(v) for v in twirl_table(g)] for g in self.twirl}
        if not isinstance(thermal_relaxation, (bool, np.bool_)):
            raise ValueError(f"{who}: thermal_relaxation = {thermal_relaxation!r}, want True or False")
        self.relaxation = bool(thermal_relaxation)
        self.circuits, self.observables = list(circuits), list(observables)
        self.max_bond, self.cutoff = _check_bond(max_bond, who), _check_cutoff(cutoff, who)
        if trajectories is not None:
            trajectories = check_trajectories(trajectories, who)
            if noise is None:
                raise ValueError(f"{who}: trajectories without a noise model (a noiseless circuit has one trajectory: lower it "
                                 "without trajectories)")
        elif noise is not None:
            raise ValueError(f"{who}: noise without trajectories (the MPS path unravels a noise model into Pauli-insertion "
                             "trajectories: pass trajectories=T)")
        if len(self.circuits) != len(self.observables):
            raise ValueError(f"{who}: {len(self.circuits)} circuits but {len(self.observables)} observables")
        self.noise, self.trajectories, self.noisy = noise, trajectories, noise is not None
        self.ops, self.params, self.op_ptr = [], [], [0]
        self.term_circ, self.term_off, self.letters, self.coeffs, self.term_ptr = [], [], [], [], [0]
        self.site_ptr, self.readout, self.n_noise_all, self.abs_coeff, self.measured_all, self.n_qubits = [0], [], [], [], [], []
        self.gate_ptr, self.gate_name, self.gate_record, self.gate_noise, self.gate_noise_len = [0], [], [], [], []
        self.gate_twirl_open, self.gate_twirl_close = [], []
        self.name_id = {g: j for j, g in enumerate(SUPPORTED_GATES)}
        # the factor programs (templates): global record index -> its chain; the occurrences [record, factor, parameter, scale] with
        # the record relative to its circuit's first, in circuit order; pool_ptr: a circuit's slice of ``params``
        self.chains: Dict[int, _Chain] = {}
        self.occ: List[List[Any]] = []
        self.occ_ptr, self.pool_ptr = [0], [0]

    def emit(self, kind, site, orient, values):
        self.ops.append((kind, site, orient, len(self.params)))
        self.params.extend(values)

    def emit_matrix(self, kind, site, orient, m, chain: Optional[_Chain] = None):
        if chain is not None and chain.parameterised:
            self.chains[len(self.ops)] = chain
            for j, f in enumerate(chain.factors):
                if not isinstance(f, np.ndarray):
                    self.occ[f[3]][0], self.occ[f[3]][1] = len(self.ops) - self.op_ptr[-1], j
        flat = []
        for e in np.asarray(m, dtype=complex).reshape(-1):
            flat += [float(e.real), float(e.imag)]
        self.emit(kind, site, orient, flat)

    def emit_chain(self, kind, site, chain: _Chain):
        dim = 4 if kind == OP_MPS_U2 else 2
        self.emit_matrix(kind, site, 0, chain.placeholder(dim) if chain.parameterised else chain.factors[0], chain)

    def add(self, k: int, circ: Circuit, obs: Any, free: Optional[Sequence[Any]] = None) -> None:
        from .template import PARAM_KIND

        noise, noisy = self.noise, self.noisy
        relaxation_after, coherent_after = getattr(noise, "relaxation_after", None), getattr(noise, "coherent_after", None)
        ops, op_ptr = self.ops, self.op_ptr
        emit, emit_matrix = self.emit, self.emit_matrix
        where = f"circuit {k}"
        n = circ.num_qubits
        if not 1 <= n <= MAX_QUBITS_MPS:
            raise ValueError(f"{where}: {n} qubits; the MPS path takes 1 .. {MAX_QUBITS_MPS}")
        measured: Dict[int, int] = {}
        done = set()
        pending: Dict[int, _Chain] = {}    # ideal lowering: the one-qubit gates no record has absorbed yet
        open_bond: Dict[int, _Chain] = {}  # ideal lowering: lower site -> the gates accumulated on its bond
        n_noise = 0

        def flush(site):
            self.emit_chain(OP_MPS_U2, site, open_bond.pop(site))

        def occurrence(par):
            self.occ.append([-1, -1, par.index, par.scale])
            return len(self.occ) - 1

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
            par = free[i] if free is not None else None   # the gate's free parameter: its matrix is a PARAM factor
            first, rec, noi, noi_len = op_ptr[-1], -1, -1, 0
            t_open = t_close = -1
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
                    if name in self.twirl_tables:   # OPEN, the gate, its noise, CLOSE: the twirl acts on the noisy gate as a whole
                        t_open = len(ops) - first
                        emit(OP_MPS_TWIRL_OPEN, lower, orient, [])
                    rec = len(ops) - first
                    chain = None
                    if par is not None:
                        chain = _Chain()
                        chain.param(PARAM_KIND[name], SLOT_BOND, par, occurrence(par))
                    emit_matrix(OP_MPS_U2, lower, orient, m, chain)
                else:
                    for other in (lower - 1, lower + 1):
                        if other in open_bond:
                            flush(other)
                    chain = open_bond.get(lower)
                    if chain is None:
                        chain = open_bond[lower] = self._open(pending.pop(lower + 1, None), pending.pop(lower, None))
                    if par is None:
                        chain.fixed(_to_lower_basis(m, orient))
                    else:
                        chain.param(PARAM_KIND[name], SLOT_BOND, par, occurrence(par))
            else:
                q0 = op.qubits[0]
                m = _matrix2(name, p)
                if m is not None:
                    if noisy:
                        rec = len(ops) - first
                        chain = None
                        if par is not None:
                            chain = _Chain()
                            chain.param(PARAM_KIND[name], SLOT_LOWER, par, occurrence(par))
                        emit_matrix(OP_MPS_U1, q0, 0, m, chain)
                    else:
                        site = q0 if q0 in open_bond else q0 - 1 if q0 - 1 in open_bond else None
                        if site is None:
                            if par is not None:
                                pending.setdefault(q0, _Chain()).param(PARAM_KIND[name], SLOT_LOWER, par, occurrence(par))
                            elif q0 in pending:
                                pending[q0].fixed(m)
                            else:
                                pending[q0] = _Chain(m)
                        elif par is not None:
                            open_bond[site].param(PARAM_KIND[name], SLOT_LOWER if site == q0 else SLOT_UPPER, par, occurrence(par))
                        else:
                            open_bond[site].fixed(np.kron(np.eye(2), m) if site == q0 else np.kron(m, np.eye(2)))
            if noisy:
                reg = tuple(circ.qubit_reg_index[q] for q in op.qubits)
                lam = noise.after_gate(i, name, reg)
                if lam is not None and not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
                    raise ValueError(f"{where}: op {i} ({name}): depolarising parameter {lam!r}, want 0 <= lambda <= 1")
                coherent = coherent_after(i, name, reg) if coherent_after is not None else None
                relax = relaxation_after(i, name, reg) if relaxation_after is not None else None
                if relax is not None and not self.relaxation:
                    raise ValueError(f"{where}: op {i} ({name}): the noise model has thermal relaxation, whose jump probabilities "
                                     "depend on the state; the MPS path takes depolarising + readout models (and coherent two-qubit "
                                     "errors) only, unless thermal_relaxation=True is passed (quantum jumps at the orthogonality "
                                     "centre, which then moves to every relaxed qubit: about twice the decompositions; not "
                                     "for templates or folded runs)")
                if coherent is not None:
                    if width != 2:
                        raise ValueError(f"{where}: op {i} ({name}): a coherent error is a 4x4 unitary, the gate has one qubit")
                    noi = len(ops) - first
                    emit_matrix(OP_MPS_U2, min(op.qubits), int(op.qubits[0] > op.qubits[1]), _check_coherent((name, reg), coherent))
                    noi_len += 1
                if relax is not None:      # one fused record: depolarising (lambda = 0: none), then relaxation
                    relax = _check_relaxation((name, reg), relax, width)
                    noi = len(ops) - first if noi < 0 else noi
                    noi_len += 1
                    values = [float(lam or 0.0)] + [v for t in relax for v in t]
                    if width == 2:
                        emit(OP_MPS_NOISE2, min(op.qubits), int(op.qubits[0] > op.qubits[1]), values)
                    else:
                        emit(OP_MPS_NOISE1, op.qubits[0], 0, values)
                    n_noise += 1
                elif lam is not None:
                    noi = len(ops) - first if noi < 0 else noi
                    noi_len += 1
                    if width == 2:
                        emit(OP_MPS_DEPOL2, min(op.qubits), int(op.qubits[0] > op.qubits[1]), [float(lam)])
                    else:
                        emit(OP_MPS_DEPOL1, op.qubits[0], 0, [float(lam)])
                    n_noise += 1
                if t_open >= 0:
                    t_close = len(ops) - first
                    emit(OP_MPS_TWIRL_CLOSE, min(op.qubits), int(op.qubits[0] > op.qubits[1]), self.twirl_tables[name])
                self.gate_twirl_open.append(t_open)
                self.gate_twirl_close.append(t_close)
                self.gate_name.append(self.name_id[name])
                self.gate_record.append(rec)
                self.gate_noise.append(noi)
                self.gate_noise_len.append(noi_len)
        for site in sorted(open_bond):
            flush(site)
        for q in sorted(pending):
            self.emit_chain(OP_MPS_U1, q, pending[q])

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
            self.term_circ.append(k)
            self.term_off.append(len(self.letters))
            self.letters += [(1 if xm >> q & 1 else 0) * (2 if zm >> q & 1 else 1) + (3 if zm >> q & 1 and not xm >> q & 1 else 0)
                             for q in range(n)]
        self.coeffs += cs
        self.term_ptr.append(len(self.term_circ))
        self.readout += table
        self.site_ptr.append(len(self.readout))
        op_ptr.append(len(ops))
        self.n_noise_all.append(n_noise)
        self.abs_coeff.append(float(sum(abs(c) for c in cs)))
        self.measured_all.append(measured)
        self.n_qubits.append(n)
        self.gate_ptr.append(len(self.gate_record))
        self.occ_ptr.append(len(self.occ))
        self.pool_ptr.append(len(self.params))

    @staticmethod
    def _open(upper: Optional[_Chain], lower: Optional[_Chain]) -> _Chain:
        """The chain of a bond that opens: the pending one-qubit gates of its two sites.  Fixed ones enter as their ``kron``; a
        pending PARAM factor moves onto its slot, the fixed factors around it as ``kron`` with the identity (lower site first: the
        two sites commute)."""
        if not (upper is not None and upper.parameterised) and not (lower is not None and lower.parameterised):
            first = np.kron(upper.factors[0] if upper is not None else np.eye(2), lower.factors[0] if lower is not None else np.eye(2))
            return _Chain(first.astype(complex), trivial=upper is None and lower is None,
                          gates=sum(ch.gates for ch in (upper, lower) if ch is not None))
        chain = _Chain()
        for src, slot in ((lower, SLOT_LOWER), (upper, SLOT_UPPER)):
            for f in (src.factors if src is not None else ()):
                if isinstance(f, np.ndarray):
                    chain.fixed((np.kron(np.eye(2), f) if slot == SLOT_LOWER else np.kron(f, np.eye(2))).astype(complex))
                else:
                    f[1] = slot
                    chain.factors.append(f)
        chain.gates = sum(ch.gates for ch in (upper, lower) if ch is not None)
        return chain

    def fields(self) -> Dict[str, Any]:
        """The fields of the :class:`MpsBatch`."""
        noisy, params = self.noisy, self.params
        if len(params) + PARAM_PAD > 2 ** 31 - 1:
            raise ValueError(f"{self.who}: {len(params)} gate parameters exceed the 2^31 - 1 a record can address; split the batch")
        return dict(
            n_qubits=np.asarray(self.n_qubits, dtype=np.int32), op_ptr=np.asarray(self.op_ptr, dtype=np.int64),
            ops=np.asarray(self.ops, dtype=np.int32).reshape(-1, 4), params=np.asarray(params + [0.0] * PARAM_PAD, dtype=np.float64),
            term_ptr=np.asarray(self.term_ptr, dtype=np.int64), term_circ=np.asarray(self.term_circ, dtype=np.int32),
            term_off=np.asarray(self.term_off, dtype=np.int64), letters=np.asarray(self.letters + [0], dtype=np.uint8),
            coeff=np.asarray(self.coeffs, dtype=np.float64), site_ptr=np.asarray(self.site_ptr, dtype=np.int64),
            readout=np.asarray(self.readout + [[1.0, 0.0]], dtype=np.float64).reshape(-1, 2), max_bond=self.max_bond, cutoff=self.cutoff,
            trajectories=self.trajectories, n_noise=self.n_noise_all, abs_coeff=self.abs_coeff, measured=self.measured_all,
            gate_ptr=np.asarray(self.gate_ptr, dtype=np.int64) if noisy else None,
            gate_name=np.asarray(self.gate_name, dtype=np.int16) if noisy else None,
            gate_record=np.asarray(self.gate_record, dtype=np.int32) if noisy else None,
            gate_noise=np.asarray(self.gate_noise, dtype=np.int32) if noisy else None,
            gate_noise_len=np.asarray(self.gate_noise_len, dtype=np.int32) if noisy else None,
            gate_twirl_open=np.asarray(self.gate_twirl_open, dtype=np.int32) if self.twirl else None,
            gate_twirl_close=np.asarray(self.gate_twirl_close, dtype=np.int32) if self.twirl else None)


def compile_mps(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                trajectories: Optional[int] = None, max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF,
                thermal_relaxation: bool = False, pauli_twirl: Any = None) -> MpsBatch:
    """Lowers ``circuits`` with one observable each to one :class:`MpsBatch`.  Site = qubit index.

    ``noise=None`` (ideal): one ``U2`` record per bond visit -- a run of gates confined to one bond (its one-qubit gates included)
    is multiplied into a single 4x4 matrix over bit(lower) + 2 bit(upper) -- and one ``U1`` record per qubit whose last one-qubit
    gates no bond absorbed.  With ``noise`` and ``trajectories``: nothing is fused; one ``U1`` record per one-qubit gate, one ``U2``
    per two-qubit gate (the gate's own matrix and its orientation), a ``U2`` for a coherent error, and a ``DEPOL1`` / ``DEPOL2``
    record per depolarising op; readout noise of measured qubits goes into the ``readout`` table.

    ``thermal_relaxation=True`` takes a model with thermal relaxation (``NoiseModel.from_backend(..., thermal_relaxation=True)``):
    a gate with relaxation gets ONE ``NOISE1`` / ``NOISE2`` record (lambda or 0, then the checked (g, c, p1) triples, as
    ``compile_programs`` emits them) in the place of its ``DEPOL`` record, and the kernel unravels it into quantum jumps applied at
    the orthogonality centre, which moves to every relaxed qubit (about twice the decompositions).  ``error_bound`` is then a
    per-trajectory certificate, conditional on the jumps drawn: |<O>_exact - <O>_mps| <= 4 B sum|coeff| for the exact vector
    carried through the same operators (include/mlqem_hip.h).  Such a batch is refused by ``compile_mps_templates`` (the keyword
    does not exist there) and by the folded runs of ``blackwater.sim.zne``.

    ``pauli_twirl`` (noisy lowering only; ``True``: cx, cz and ecr; or names from cx, cz, ecr, swap) wraps every such gate into
    ``TWIRL_OPEN``, the gate's ``U2``, its coherent-error ``U2`` and ``DEPOL2`` / ``NOISE2`` where the model has them,
    ``TWIRL_CLOSE`` (the table of :func:`twirl_table`): the device draws one of the 16 Pauli pairs per (run, trajectory) and gate,
    applies it before and its image under the ideal gate after, P' (Lambda G) P = (P' Lambda P') G -- the circuits are lowered
    once, and the mean over the trajectories is the value under the twirled noise.  ``n_noise`` does not count twirl records;
    ``gate_twirl_open`` / ``gate_twirl_close`` locate them.  ``run_mps_bound`` refuses such a batch.

    Raises ``ValueError`` naming the offender for what ``compile_programs`` refuses (unknown gates, parameter counts, qubits out of
    range or used after their measurement, non-finite angles, malformed terms) and for: a two-qubit gate on qubits that are no
    neighbours, ``max_bond`` outside 1 .. 32, ``noise`` without ``trajectories`` or the reverse, a model with thermal relaxation
    without ``thermal_relaxation=True``, readout noise together with an X / Y term, a circuit over 512 qubits."""
    low = _Lowering("compile_mps", circuits, observables, noise, trajectories, max_bond, cutoff, thermal_relaxation, pauli_twirl)
    for k, (obj, obs) in enumerate(zip(low.circuits, low.observables)):
        low.add(k, Circuit.from_any(obj), obs)
    return MpsBatch(**low.fields())


@dataclass
class MpsBoundBatch(MpsBatch):
    """Templates lowered for ``mlqem_mps_bind_f64``: the arrays of an :class:`MpsBatch` (a template per "circuit", the matrices of
    parameterised records at the placeholder angle 0), the factor programs of the parameterised records and what the host knows
    about the parameters."""

    pool_ptr: Optional[np.ndarray] = None     # int64 [C + 1]: template c owns params[pool_ptr[c] .. pool_ptr[c + 1])
    # the factor CSR over the RECORDS: record j owns factors fac_ptr[j] .. fac_ptr[j + 1] (none: its host matrix is copied)
    fac_ptr: Optional[np.ndarray] = None      # int64 [n_ops + 1]
    fac: Optional[np.ndarray] = None          # int32 [n_fac + 1, 4]: kind (0 FIXED, 12 .. 16 PRX PRY PRZ PP PRZZ), slot, parameter, offset into fpool
    fac_val: Optional[np.ndarray] = None      # float64 [n_fac + 1, 2]: (scale, offset) of a PARAM factor
    fpool: Optional[np.ndarray] = None        # float64 [n + 32]: the FIXED factors, 32 (U2) or 8 (U1) float64 each, row-major (re, im)
    rec_gates: Optional[np.ndarray] = None    # int32 [n_ops]: the gates multiplied into a parameterised record (0: a copied record)
    num_parameters: Optional[np.ndarray] = None   # int32 [C]: the length of a parameter row of template c
    # the OCCURRENCES: every PARAM factor in circuit order -- what a parameter-shift gradient shifts
    occ_ptr: Optional[np.ndarray] = None      # int64 [C + 1]
    occ: Optional[np.ndarray] = None          # int32 [n_occ + 1, 2]: (record relative to op_ptr[c], factor inside the record)
    occ_param: Optional[np.ndarray] = None    # int32 [n_occ]
    occ_scale: Optional[np.ndarray] = None    # float64 [n_occ]


def compile_mps_templates(templates: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                          trajectories: Optional[int] = None, max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF) -> MpsBoundBatch:
    """Lowers ``templates`` (anything ``Template.from_any`` takes) with one observable each ONCE, by the rules of
    :func:`compile_mps` (the same loop: its refusals, caps, fusion decisions and noise records; the free angles stand at 0 where
    a rule wants a number, and no rule looks at an angle, so the records' kinds, sites, orientations and order are those of every
    bound copy).  A record whose matrix depends on a parameter also gets its FACTOR PROGRAM: the matrix is F_k ... F_2 F_1 with
    FIXED factors (the host product of a maximal run of consecutive fixed gates, the ``kron`` of the pending one-qubit matrices a
    bond absorbs included) and PARAM factors (kind, slot, parameter, scale, offset); ``mlqem_mps_bind_f64`` forms it per run on
    the device.  The noisy lowering fuses nothing: a parameterised record there has exactly one PARAM factor.  A template without
    parameters lowers to the arrays ``compile_mps`` gives.  A model with thermal relaxation is refused by name: there is no
    ``thermal_relaxation`` keyword here, and ``run_mps_bound`` refuses a batch that holds a ``NOISE1`` / ``NOISE2`` record."""
    from .template import Template

    templates = [Template.from_any(t) for t in templates]
    low = _Lowering("compile_mps_templates", templates, observables, noise, trajectories, max_bond, cutoff)
    for k, (t, obs) in enumerate(zip(templates, low.observables)):
        low.add(k, t.placeholder(), obs, [_free_parameter(op) for op in t.ops])
    fields = low.fields()
    n_ops = int(fields["ops"].shape[0])
    fac_ptr, fac, fac_val, fpool = [0], [], [], []
    for j in range(n_ops):
        chain = low.chains.get(j)
        for f in (chain.factors if chain is not None else ()):
            if isinstance(f, np.ndarray):
                fac.append((FACTOR_FIXED, 0, 0, len(fpool)))
                fac_val.append((0.0, 0.0))
                for e in f.reshape(-1):
                    fpool += [float(e.real), float(e.imag)]
            else:
                kind, slot, par, _ = f
                fac.append((kind, slot, par.index, 0))
                fac_val.append((par.scale, par.offset))
        fac_ptr.append(len(fac))
    if len(fpool) + PARAM_PAD > 2 ** 31 - 1 or len(fac) > 2 ** 31 - 2:
        raise ValueError("compile_mps_templates: the factor programs exceed the 2^31 - 1 entries a record can address; split the batch")
    occ = low.occ
    return MpsBoundBatch(
        **fields, pool_ptr=np.asarray(low.pool_ptr, dtype=np.int64), fac_ptr=np.asarray(fac_ptr, dtype=np.int64),
        fac=np.asarray(fac + [(0, 0, 0, 0)], dtype=np.int32).reshape(-1, 4),
        fac_val=np.asarray(fac_val + [(0.0, 0.0)], dtype=np.float64).reshape(-1, 2),
        fpool=np.asarray(fpool + [0.0] * PARAM_PAD, dtype=np.float64),
        rec_gates=np.asarray([low.chains[j].gates if j in low.chains else 0 for j in range(n_ops)], dtype=np.int32),
        num_parameters=np.asarray([t.num_parameters for t in templates], dtype=np.int32),
        occ_ptr=np.asarray(low.occ_ptr, dtype=np.int64),
        occ=np.asarray([(o[0], o[1]) for o in occ] + [(-1, -1)], dtype=np.int32).reshape(-1, 2),
        occ_param=np.asarray([o[2] for o in occ], dtype=np.int32), occ_scale=np.asarray([o[3] for o in occ], dtype=np.float64))


def _free_parameter(op) -> Any:
    from .template import Param

    return op.params[0] if op.params and isinstance(op.params[0], Param) else None


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


def _mps_chunks(widths, max_bond: int, trajectories: int, buffer_bytes: int, unit_bytes=None):
    """``(unit range, trajectory range)`` pairs over the circuits (or runs) of the widths ``widths`` whose site-tensor workspace
    (n * chi * 2 * chi * 16 B per unit, plus the stash) stays under ``buffer_bytes``: whole circuits with all their trajectories
    while they fit, else one circuit with a part of them.  A chunk holds at least one unit.  ``unit_bytes(width)``: the bytes of
    one unit where they are more than that workspace."""
    from ..native import ops

    if unit_bytes is None:
        def unit_bytes(width):
            return ops.mps_workspace_bytes(width, max_bond, 1)

    unit_bytes = functools.lru_cache(maxsize=None)(unit_bytes)   # a batch has few distinct widths and many circuits
    chunks, lo, b = [], 0, len(widths)
    while lo < b:
        hi, widest = lo + 1, int(widths[lo])
        per = unit_bytes(widest)
        if per * trajectories > buffer_bytes:
            step = max(int(buffer_bytes // per), 1)
            chunks += [(range(lo, hi), range(t0, min(t0 + step, trajectories))) for t0 in range(0, trajectories, step)]
        else:
            while hi < b:
                wider = max(widest, int(widths[hi]))
                if unit_bytes(wider) * trajectories * (hi + 1 - lo) > buffer_bytes:
                    break
                widest, hi = wider, hi + 1
            chunks.append((range(lo, hi), range(0, trajectories)))
        lo = hi
    return chunks


def _mps_plan(widths, max_bond: int, n_traj: int, buffer_bytes, who: str, dev, shots: bool = False):
    """The launches of a chunked driver: ``(chunks, workspace, environment workspace or None)``.  ``chunks``: ``(unit range,
    trajectory range, widest circuit)`` triples of :func:`_mps_chunks` under ``buffer_bytes`` (``None``: :data:`MPS_BUFFER_BYTES`;
    with ``shots`` a unit counts its environment workspace too); the workspaces are sized to the largest chunk."""
    import torch

    from ..native import ops

    buffer_bytes = MPS_BUFFER_BYTES if buffer_bytes is None else int(buffer_bytes)
    if buffer_bytes < 1:
        raise ValueError(f"{who}: buffer_bytes = {buffer_bytes!r}, want a positive number of bytes")
    sizes = (ops.mps_workspace_bytes, ops.mps_sample_workspace_bytes) if shots else (ops.mps_workspace_bytes,)
    chunks = [(ur, tr, int(widths[ur.start:ur.stop].max()))
              for ur, tr in _mps_chunks(widths, max_bond, n_traj, buffer_bytes, lambda width: sum(f(width, max_bond, 1) for f in sizes))]
    buffers = [torch.empty((max([f(w, max_bond, len(ur) * len(tr)) for ur, tr, w in chunks] + [16]),), dtype=torch.uint8, device=dev)
               for f in sizes]
    return chunks, buffers[0], buffers[1] if shots else None


def _mps_result(out, term_ptr, batch, seed, traj_terms, traj_stats, keep: bool, noisy: bool) -> MpsResult:
    """The :class:`MpsResult` of ``sim_mps_finish``'s dict ``out``: standard errors where ``noisy``, the per-trajectory arrays where
    ``keep``."""
    return MpsResult(out["values"], out["term_values"], out["norm"], term_ptr, out["discarded"], out["error_bound"], out["bond"],
                     out["std_error"] if noisy else None, out["term_std_error"] if noisy else None, batch.trajectories, seed,
                     traj_terms if keep else None, traj_stats if keep else None, batch)


def run_mps(batch: MpsBatch, seed: int = 0, run_keys=None, device="cuda", keep_trajectories: bool = False,
            buffer_bytes: int = None) -> MpsResult:
    """Runs a batch lowered by :func:`compile_mps` on the device.  ``run_keys``: one integer per circuit, by default its position in
    the batch; a unit's bits depend on (seed, run key, trajectory number, the circuit's records) alone, so a circuit gives the
    same values alone, in any batch and under any split.  The (circuit, trajectory) units are split into launches so that the
    site-tensor workspace stays under ``buffer_bytes`` (default :data:`MPS_BUFFER_BYTES`).  Returns an :class:`MpsResult`."""
    import torch

    from ..native import ops

    seed = check_seed(seed, "run_mps")
    n_traj = 1 if batch.trajectories is None else check_trajectories(batch.trajectories, "run_mps")
    keys = _run_keys(run_keys, len(batch), "run_mps")
    dev = torch.device(device)
    chunks, workspace, _ = _mps_plan(batch.n_qubits, batch.max_bond, n_traj, buffer_bytes, "run_mps", dev)
    t = batch.to(dev)
    b, n_terms, noisy = len(batch), int(batch.term_circ.shape[0]), batch.trajectories is not None
    if b == 0:
        empty = {k: torch.zeros(0, dtype=torch.float64, device=dev)
                 for k in ("values", "term_values", "norm", "discarded", "error_bound", "std_error", "term_std_error")}
        empty["bond"] = torch.zeros(0, dtype=torch.int32, device=dev)
        return _mps_result(empty, t["term_ptr"], batch, seed, None, None, False, noisy)
    keys_t = upload(keys, dev)
    traj_terms = torch.zeros((n_traj, n_terms), dtype=torch.float64, device=dev)
    traj_norm = torch.zeros((n_traj, b), dtype=torch.float64, device=dev)
    traj_stats = torch.zeros((n_traj, b, ops.MPS_STATS), dtype=torch.float64, device=dev)
    for cr, tr, widest in chunks:
        ops.sim_run_mps(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], keys_t, t["term_circ"], t["term_off"], t["letters"],
                        t["site_ptr"], t["readout"], (cr.start, len(cr)),
                        (int(batch.term_ptr[cr.start]), int(batch.term_ptr[cr.stop] - batch.term_ptr[cr.start])), (tr.start, len(tr)),
                        n_traj, seed, batch.max_bond, batch.cutoff, widest, workspace, traj_terms, traj_norm, traj_stats)
    out = ops.sim_mps_finish(t["term_ptr"], t["coeff"], traj_terms, traj_norm, traj_stats)
    return _mps_result(out, t["term_ptr"], batch, seed, traj_terms, traj_stats, keep_trajectories, noisy)


def mps_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                           max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF, trajectories: Optional[int] = None, seed: int = 0,
                           run_keys=None, device="cuda", thermal_relaxation: bool = False, pauli_twirl: Any = None) -> MpsResult:
    """Expectation values of ``observables[k]`` after ``circuits[k]`` by matrix-product states of bond at most ``max_bond``:
    circuits of up to 512 qubits whose two-qubit gates act on neighbours, any angle.  ``noise`` + ``trajectories``: the values
    under a depolarising + readout model, as means over Pauli-insertion trajectories with their standard errors; with
    ``thermal_relaxation=True`` also under a model with thermal relaxation (quantum jumps, :func:`compile_mps`);
    ``pauli_twirl`` twirls the named two-qubit gates on the device (:func:`compile_mps`)."""
    return run_mps(compile_mps(circuits, observables, noise, trajectories, max_bond, cutoff, thermal_relaxation, pauli_twirl), seed,
                   run_keys, device)


# ---- templates: bound on the device ---------------------------------------------------------------------------------------------------
MPS_POOL_ENTRIES = 2 ** 31 - 1 - PARAM_PAD   # float64 values of bound records one launch can address


class MpsBoundRun:
    """The runs ``(template, theta row, shifted occurrence or -1)`` of a batch lowered by :func:`compile_mps_templates`, prepared
    for the device: every table is uploaded and every buffer allocated here, so that :meth:`launch` only enqueues kernels (per
    chunk ``mlqem_mps_bind_f64``, ``mlqem_mps_run_f64`` and ``mlqem_mps_terms_f64``, then ``mlqem_mps_finish_f64``) on the current
    stream and can be captured in a graph and replayed.  :func:`run_mps_bound` is the one-call form."""

    def __init__(self, batch: "MpsBoundBatch", theta, runs=None, shift=None, seed: int = 0, run_keys=None, device="cuda",
                 buffer_bytes: int = None, pool_entries: int = MPS_POOL_ENTRIES):
        import torch

        from ..native import ops
        who = "run_mps_bound"
        self.batch, self.seed = batch, check_seed(seed, who)
        refuse_relaxation_records(batch, who)
        refuse_twirl_records(batch, who)
        self.n_traj = 1 if batch.trajectories is None else check_trajectories(batch.trajectories, who)
        dev = self.dev = torch.device(device)
        is_tensor = isinstance(theta, torch.Tensor)
        n_rows = int(theta.shape[0]) if (is_tensor and theta.dim() == 2) else None
        if not is_tensor:
            theta = np.asarray(theta, dtype=np.float64)
            theta = theta.reshape(1, -1) if theta.ndim < 2 else theta
            if theta.ndim != 2:
                raise ValueError(f"{who}: the parameter rows have the shape {theta.shape}, want [n_rows, P]")
            n_rows = int(theta.shape[0])
            if theta.shape[1] == 0:
                theta = np.zeros((max(n_rows, 1), 1), dtype=np.float64)
        elif n_rows is None or theta.dtype != torch.float64:
            raise ValueError(f"{who}: a tensor of parameter rows must be float64 [n_rows, P], got {tuple(theta.shape)} {theta.dtype}")
        c = len(batch)
        if runs is None:
            if c != 1 and c != n_rows:
                raise ValueError(f"{who}: {n_rows} parameter rows for {c} templates; pass runs= (template, row, shifted occurrence)")
            runs = np.zeros((n_rows, 4), dtype=np.int32)
            runs[:, 0], runs[:, 1], runs[:, 2] = (0 if c == 1 else np.arange(n_rows)), np.arange(n_rows), -1
        runs = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1, 4)
        r = self.n_runs = int(runs.shape[0])
        shift = np.zeros(r) if shift is None else np.ascontiguousarray(shift, dtype=np.float64).reshape(-1)
        if shift.shape[0] != r:
            raise ValueError(f"{who}: {r} runs but {shift.shape[0]} shifts")
        if r and (c < 1 or n_rows < 1 or runs[:, 0].min() < 0 or runs[:, 0].max() >= c or runs[:, 1].min() < 0 or runs[:, 1].max() >= n_rows):
            raise ValueError(f"{who}: a run names a template outside 0 .. {c - 1} or a parameter row outside 0 .. {n_rows - 1}")
        if r and theta.shape[1] < int(batch.num_parameters[np.unique(runs[:, 0])].max()):
            raise ValueError(f"{who}: the parameter rows have {int(theta.shape[1])} values, a template has "
                             f"{int(batch.num_parameters[np.unique(runs[:, 0])].max())} parameters")
        keys = _run_keys(run_keys, r, who)
        tpl = runs[:, 0].astype(np.int64)
        count = lambda ptr: np.diff(ptr)[tpl] if r else np.zeros(0, dtype=np.int64)   # noqa: E731
        rec_n, pool_n, term_n = count(batch.op_ptr), count(batch.pool_ptr), count(batch.term_ptr)
        cum = lambda v: np.concatenate([[0], np.cumsum(v)]).astype(np.int64)   # noqa: E731
        run_op, run_pool, self.run_term_ptr = cum(rec_n), cum(pool_n), cum(term_n)
        n_terms = int(self.run_term_ptr[-1])
        self.term_run = np.repeat(np.arange(r, dtype=np.int64), term_n)
        self.term_pos = np.arange(n_terms, dtype=np.int64) - np.repeat(self.run_term_ptr[:-1], term_n)
        term_src = np.repeat(batch.term_ptr[tpl], term_n) + self.term_pos if r else np.zeros(0, dtype=np.int64)
        widths = batch.n_qubits[tpl] if r else np.zeros(0, dtype=np.int32)
        if np.any(pool_n > pool_entries):
            raise ValueError(f"{who}: one bound copy holds {int(pool_n.max())} gate parameters, over the {pool_entries} a launch addresses")
        # chunks: by the workspace budget, as run_mps splits circuits, and by the pool entries a record can address
        plan, self.workspace, _ = _mps_plan(widths, batch.max_bond, self.n_traj, buffer_bytes, who, dev)
        chunks = []
        for cr, tr, _ in plan:
            lo = cr.start
            while lo < cr.stop:
                hi = lo + 1
                while hi < cr.stop and run_pool[hi + 1] - run_pool[lo] <= pool_entries:
                    hi += 1
                chunks.append((range(lo, hi), tr))
                lo = hi
        self.chunks = chunks
        self.tpl = upload_fields(batch, ("op_ptr", "ops", "params", "pool_ptr", "fac_ptr", "fac", "fac_val", "fpool", "occ_ptr", "occ", "letters",
                                         "readout"), dev)
        self.theta = theta.to(dev).contiguous() if is_tensor else upload(theta, dev)
        self.runs, self.shift, self.keys = upload(runs, dev), upload(shift, dev), upload(keys, dev)
        self.widths = upload(widths.astype(np.int32), dev)
        self.term_off, self.coeff = upload(batch.term_off[term_src], dev), upload(batch.coeff[term_src], dev)
        self.site_ptr = upload(np.concatenate([batch.site_ptr[tpl], batch.site_ptr[-1:]]).astype(np.int64), dev)
        self.term_ptr = upload(self.run_term_ptr, dev)
        # per chunk, relative to its first run: op_ptr [n + 1], out_pool_ptr [n + 1] and the run of each of its terms
        rel_op, rel_pool, rel_term, self.where = [], [], [], []
        for cr, _ in chunks:
            self.where.append((sum(len(a) for a in rel_op), sum(len(a) for a in rel_term)))
            rel_op.append(run_op[cr.start:cr.stop + 1] - run_op[cr.start])
            rel_pool.append(run_pool[cr.start:cr.stop + 1] - run_pool[cr.start])
            rel_term.append(self.term_run[self.run_term_ptr[cr.start]:self.run_term_ptr[cr.stop]] - cr.start)
        cat = lambda parts, dtype: upload(np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype=dtype), dev)   # noqa: E731
        self.rel_op, self.rel_pool, self.rel_term = cat(rel_op, np.int64), cat(rel_pool, np.int64), cat(rel_term, np.int32)
        self.sizes = [(int(run_op[cr.stop] - run_op[cr.start]), int(run_pool[cr.stop] - run_pool[cr.start]),
                       int(self.run_term_ptr[cr.stop] - self.run_term_ptr[cr.start]), int(rec_n[cr.start:cr.stop].max()),
                       int(widths[cr.start:cr.stop].max())) for cr, _ in chunks]
        zeros = lambda shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)   # noqa: E731
        self.out_ops = zeros((max([s[0] for s in self.sizes] + [1]), 4), torch.int32)
        self.out_pool = zeros(max([s[1] for s in self.sizes] + [0]) + PARAM_PAD)
        t = self.n_traj
        self.traj_terms, self.traj_norm, self.traj_stats = zeros((t, n_terms)), zeros((t, r)), zeros((t, r, ops.MPS_STATS))
        units = max([len(cr) for cr, _ in chunks] + [1])
        self.loc_terms, self.loc_norm = zeros(t * max([s[2] for s in self.sizes] + [1])), zeros(t * units)
        self.loc_stats = zeros(t * units * ops.MPS_STATS)
        self.out = {k: zeros(n) for k, n in (("term_values", n_terms), ("term_std_error", n_terms), ("values", r), ("std_error", r),
                                             ("norm", r), ("discarded", r), ("error_bound", r))}
        self.out["bond"] = zeros(r, torch.int32)

    def launch(self) -> None:
        """Enqueues the bind and run kernels of every chunk and the finish kernel.  No host read, no allocation, no upload."""
        from ..native import ops

        t, b, n_traj = self.tpl, self.batch, self.n_traj
        for (cr, tr), (n_ops, n_pool, n_terms, max_rec, widest), (op_at, term_at) in zip(self.chunks, self.sizes, self.where):
            lo, hi, n = cr.start, cr.stop, len(cr)
            t0 = int(self.run_term_ptr[lo])
            out_ops, out_pool = self.out_ops[:max(n_ops, 1)], self.out_pool[:n_pool + PARAM_PAD]
            op_ptr, pool_ptr = self.rel_op[op_at:op_at + n + 1], self.rel_pool[op_at:op_at + n + 1]
            ops.mps_bind(t["op_ptr"], t["ops"], t["params"], t["pool_ptr"], t["fac_ptr"], t["fac"], t["fac_val"], t["fpool"], t["occ_ptr"],
                         t["occ"], self.theta, self.runs[lo:hi], self.shift[lo:hi], max_rec, op_ptr, pool_ptr, out_ops, out_pool)
            loc_terms = self.loc_terms[:n_traj * n_terms].view(n_traj, n_terms)
            loc_norm = self.loc_norm[:n_traj * n].view(n_traj, n)
            loc_stats = self.loc_stats[:n_traj * n * ops.MPS_STATS].view(n_traj, n, ops.MPS_STATS)
            ops.sim_run_mps(self.widths[lo:hi], op_ptr, out_ops, out_pool, self.keys[lo:hi], self.rel_term[term_at:term_at + n_terms],
                            self.term_off[t0:t0 + n_terms], t["letters"], self.site_ptr[lo:hi + 1], t["readout"], (0, n), (0, n_terms),
                            (tr.start, len(tr)), n_traj, self.seed, b.max_bond, b.cutoff, widest, self.workspace, loc_terms, loc_norm,
                            loc_stats)
            ts = slice(tr.start, tr.stop)
            self.traj_terms[ts, t0:t0 + n_terms].copy_(loc_terms[ts])
            self.traj_norm[ts, lo:hi].copy_(loc_norm[ts])
            self.traj_stats[ts, lo:hi].copy_(loc_stats[ts])
        if self.n_runs:
            ops.sim_mps_finish(self.term_ptr, self.coeff, self.traj_terms, self.traj_norm, self.traj_stats, out=self.out)

    def bound_batch(self, chunk: int = 0):
        """Reads chunk ``chunk``'s bound records back as a plain :class:`MpsBatch` (after :meth:`launch`, before another chunk's bind
        overwrites them: with one chunk, any time): what ``compile_mps`` of the bound copies would have lowered, for ``run_mps``."""
        (cr, _), (n_ops, n_pool, n_terms, _, _), (op_at, term_at) = self.chunks[chunk], self.sizes[chunk], self.where[chunk]
        lo, n, t0, b = cr.start, len(cr), int(self.run_term_ptr[cr.start]), self.batch
        host = lambda x: x.cpu().numpy()   # noqa: E731
        site = host(self.site_ptr[lo:cr.stop + 1])
        return MpsBatch(
            n_qubits=host(self.widths[lo:cr.stop]), op_ptr=host(self.rel_op[op_at:op_at + n + 1]), ops=host(self.out_ops[:n_ops]),
            params=host(self.out_pool[:n_pool + PARAM_PAD]), term_ptr=self.run_term_ptr[lo:cr.stop + 1] - t0,
            term_circ=host(self.rel_term[term_at:term_at + n_terms]), term_off=host(self.term_off[t0:t0 + n_terms]), letters=b.letters,
            coeff=host(self.coeff[t0:t0 + n_terms]), site_ptr=site, readout=b.readout, max_bond=b.max_bond, cutoff=b.cutoff,
            trajectories=b.trajectories)

    def result(self, keep_trajectories: bool = False) -> MpsResult:
        return _mps_result(self.out, self.term_ptr, self.batch, self.seed, self.traj_terms, self.traj_stats, keep_trajectories,
                           self.batch.trajectories is not None)


def run_mps_bound(batch: MpsBoundBatch, rows, runs=None, shift=None, seed: int = 0, run_keys=None, device="cuda",
                  keep_trajectories: bool = False, buffer_bytes: int = None) -> MpsResult:
    """Runs templates lowered by :func:`compile_mps_templates`, bound on the device.  ``rows``: float64 [n_rows, P] (numpy, or a
    tensor on the device); ``runs`` int32 [R, 4] = (template, row, shifted occurrence or -1, 0) with ``shift`` float64 [R] (default:
    row r is one unshifted run of template r, or of the only template).  ``mlqem_mps_bind_f64`` writes the records and the
    parameter pool of the R bound copies, the MPS kernels run them as they run any batch; both go on one stream
    (:class:`MpsBoundRun` is the capturable form).  ``run_keys``: one integer per RUN, by default its position.  The runs are split
    so that the site-tensor workspace of a launch stays under ``buffer_bytes`` and its pool under 2^31 - 1 entries; a run's bits
    depend on (template, row, shift, seed, run key) alone, not on the split.  The result's CSR (``term_ptr``) is over the runs;
    ``result.batch`` is the template batch."""
    plan = MpsBoundRun(batch, rows, runs, shift, seed, run_keys, device, buffer_bytes)
    plan.launch()
    return plan.result(keep_trajectories)


def _mps_pairs(template, observable, rows, noise, trajectories, max_bond, cutoff, who):
    from .bound import _pairs

    tpls, obss, pair, theta, n_rows = _pairs(template, observable, rows, who)
    return compile_mps_templates(tpls, obss, noise, trajectories, max_bond, cutoff), pair, theta, n_rows


def bound_mps_expectation_values(template, observable, rows, noise: Optional[NoiseModel] = None, trajectories: Optional[int] = None,
                                 max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF, seed: int = 0, run_keys=None, device="cuda",
                                 buffer_bytes: int = None, return_result: bool = False):
    """Expectation values of one template of up to 512 qubits (two-qubit gates on neighbours) at many parameter vectors by
    matrix-product states: ``(values [B], term_values [B, T])``, float64 tensors on ``device``; with ``return_result`` also the
    :class:`MpsResult` over the B rows (``error_bound``, ``bond``, ``std_error``, ...: what :func:`mps_expectation_values` reports).
    ``template`` / ``observable``: single objects with ``rows`` [B, P], or equal-length lists with one row per pair (T is then the
    largest term count, rows padded with zeros).  Equal (template object, observable) pairs are lowered once
    (:func:`compile_mps_templates`); nothing is bound or lowered per row on the host.  ``noise`` + ``trajectories`` as in
    :func:`mps_expectation_values`."""
    import torch

    batch, pair, theta, n_rows = _mps_pairs(template, observable, rows, noise, trajectories, max_bond, cutoff, "bound_mps_expectation_values")
    runs = np.zeros((n_rows, 4), dtype=np.int32)
    runs[:, 0], runs[:, 1], runs[:, 2] = pair, np.arange(n_rows), -1
    plan = MpsBoundRun(batch, theta, runs, None, seed, run_keys, device, buffer_bytes)
    plan.launch()
    res = plan.result()
    width = int(np.diff(batch.term_ptr).max()) if len(batch) else 0
    term_values = torch.zeros((n_rows, width), dtype=torch.float64, device=plan.dev)
    if res.term_values.numel():
        term_values[torch.from_numpy(plan.term_run).to(plan.dev), torch.from_numpy(plan.term_pos).to(plan.dev)] = res.term_values
    return (res.values, term_values, res) if return_result else (res.values, term_values)


def mps_parameter_shift(template, observable, rows, noise: Optional[NoiseModel] = None, trajectories: Optional[int] = None,
                        max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF, seed: int = 0, run_keys=None, device="cuda",
                        buffer_bytes: int = None):
    """``parameter_shift(..., method="mps")``: values and parameter-shift gradients ``(values [B], gradients [B, P])`` from
    matrix-product states.  One bind launch (per chunk) covers the B unshifted and the 2 K B shifted runs (K occurrences), the MPS
    kernels follow, ``mlqem_sim_shift_combine_f64`` combines.  Under noise every run of a row uses the ROW's run key: the Pauli
    insertions are drawn from (seed, key, trajectory, noise record) and not from an angle, so the + and - runs share their
    insertions with the unshifted run, and the rule is exact for the mean over that trajectory set (each trajectory is a circuit
    of rotations and fixed Pauli gates).  With truncation (a bond over ``max_bond``) the rule differentiates the truncated values
    only up to their certificates."""
    import torch

    from ..native import ops

    batch, pair, theta, n_rows = _mps_pairs(template, observable, rows, noise, trajectories, max_bond, cutoff, "parameter_shift")
    runs, shift, groups = mps_shift_runs(batch, pair)
    row_keys = _run_keys(run_keys, n_rows, "parameter_shift")
    plan = MpsBoundRun(batch, theta, runs, shift, seed, row_keys[runs[:, 1]] if runs.shape[0] else None, device, buffer_bytes)
    plan.launch()
    all_values, dev = plan.result().values, plan.dev
    width = int(batch.num_parameters.max()) if len(batch) else 0
    values = torch.zeros(n_rows, dtype=torch.float64, device=dev)
    grads = torch.zeros((n_rows, width), dtype=torch.float64, device=dev)
    for c, rws, at, k in groups:
        b, p = int(rws.size), int(batch.num_parameters[c])
        ob = int(batch.occ_ptr[c])
        par = batch.occ_param[ob:ob + k]
        order = np.argsort(par, kind="stable").astype(np.int32)   # a parameter's occurrences, in circuit order
        occ_ptr = np.concatenate([[0], np.cumsum(np.bincount(par, minlength=p))]).astype(np.int64)
        v = all_values[at:at + b * (1 + 2 * k)]
        g = ops.sim_shift_combine(v[b:b + k * b].reshape(k, b), v[b + k * b:].reshape(k, b), upload(occ_ptr, dev), upload(order, dev),
                                  upload(batch.occ_scale[ob:ob + k], dev))
        idx = upload(rws, dev)
        values[idx] = v[:b]
        grads[idx, :p] = g
    return values, grads


def mps_shift_runs(batch: MpsBoundBatch, pair: np.ndarray):
    """The runs of a parameter-shift gradient, as ``blackwater.sim.bound.shift_runs`` lays them out: per template c with rows ``R``
    (B_c of them) and K_c occurrences, B_c unshifted runs, then K_c x B_c runs shifted by +pi/2 (occurrence-major), then as many
    by -pi/2.  The shifted entry of a run is the OCCURRENCE number.  Returns ``(runs, shift, groups)``, ``groups = [(c, rows, first
    run, K_c)]``."""
    runs, shift, groups, at = [], [], [], 0
    for c in range(len(batch)):
        rows = np.flatnonzero(pair == c)
        if rows.size == 0:
            continue
        k, b = int(batch.occ_ptr[c + 1] - batch.occ_ptr[c]), int(rows.size)
        block = np.zeros((b * (1 + 2 * k), 4), dtype=np.int32)
        block[:, 0] = c
        block[:, 1] = np.tile(rows, 1 + 2 * k)
        block[:b, 2] = -1
        block[b:, 2] = np.tile(np.repeat(np.arange(k), b), 2)
        sh = np.zeros(block.shape[0], dtype=np.float64)
        sh[b:b + k * b], sh[b + k * b:] = 0.5 * math.pi, -0.5 * math.pi
        runs.append(block)
        shift.append(sh)
        groups.append((c, rows, at, k))
        at += block.shape[0]
    if not runs:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0), groups
    return np.concatenate(runs), np.concatenate(shift), groups


# ---- shots ------------------------------------------------------------------------------------------------------------------------
MAX_GROUPS_MPS = 4096   # MLQEM_MPS_MAX_GROUPS: measurement groups per circuit (12 bits of a Philox counter word)
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
        out = self.mps.to(device)
        out.update(upload_fields(self, ("group_ptr", "group_circ", "group_off", "basis", "flip", "ref_ptr", "gterm_ptr", "gterm", "term_mask",
                                        "masks"), device, view={"masks": np.int32}))
        return out


def compile_mps_shots(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                      trajectories: Optional[int] = None, max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF,
                      thermal_relaxation: bool = False, pauli_twirl: Any = None) -> MpsShotsBatch:
    """The lowering of :func:`compile_mps` plus the measurement groups of :func:`~blackwater.sim.measurement_groups`: one basis
    letter per (group, site) (Z where no term of the group touches the site), the ``flip`` table of the measured qubits' readout
    noise, a support mask per term and the group of each term.  What ``compile_mps`` refuses stays refused, by the same messages
    (X or Y terms beside readout noise, thermal relaxation without ``thermal_relaxation=True``, gates on qubits that are no
    neighbours, ...); also refused: a circuit whose terms need more than 4 096 measurement groups.  ``pauli_twirl`` is
    ``compile_mps``'s: the shots of a trajectory are drawn from its twirled state."""
    circuits, observables = list(circuits), list(observables)
    base = compile_mps(circuits, observables, noise, trajectories, max_bond, cutoff, thermal_relaxation, pauli_twirl)   # every check and refusal
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

    shots, seed = check_shots(shots, "run_mps_shots"), check_seed(seed, "run_mps_shots")
    mps = batch.mps
    n_traj = 1 if mps.trajectories is None else check_trajectories(mps.trajectories, "run_mps_shots")
    if n_traj > shots:
        raise ValueError(f"run_mps_shots: trajectories = {n_traj} exceed shots = {shots} (shot s comes from trajectory s mod "
                         "trajectories: the others would be simulated and never measured)")
    keys = _run_keys(run_keys, len(batch), "run_mps_shots")
    dev = torch.device(device)
    chunks, workspace, env = _mps_plan(mps.n_qubits, mps.max_bond, n_traj, buffer_bytes, "run_mps_shots", dev, shots=True)
    t = batch.to(dev)
    b, n_terms = len(batch), int(mps.term_circ.shape[0])
    zeros = lambda n, dtype=torch.float64: torch.zeros(n, dtype=dtype, device=dev)   # noqa: E731
    if b == 0:
        return MpsShotsResult(zeros(0), zeros(0), zeros(0), t["term_ptr"], zeros(0, torch.int32), t["ref_ptr"], t["group_ptr"], zeros(0),
                              zeros(0), zeros(0, torch.int32), zeros(0, torch.int32) if return_bits else None, shots, seed,
                              mps.trajectories, batch)
    keys_t = upload(keys, dev)
    traj_stats = zeros((n_traj, b, ops.MPS_STATS))
    term_sums = zeros(n_terms, torch.int32)
    bits = zeros(int(batch.ref_ptr[-1]) * shots, torch.int32) if return_bits else None
    for cr, tr, w in chunks:
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
                                  device="cuda", thermal_relaxation: bool = False, pauli_twirl: Any = None) -> MpsShotsResult:
    """Expectation values of ``observables[k]`` after ``circuits[k]`` estimated from ``shots`` measurement outcomes per measurement
    basis, drawn from the matrix-product state of bond at most ``max_bond``: circuits of up to 512 qubits whose two-qubit gates act on
    neighbours, any angle; ideal, or under a depolarising + readout ``noise`` model with ``trajectories`` (one with thermal
    relaxation: ``thermal_relaxation=True``; ``pauli_twirl``: :func:`compile_mps`).  The limit of every estimate is the value
    :func:`mps_expectation_values` gives."""
    from .program import check_shots

    if shots is None:
        raise ValueError("sample_mps_expectation_values: shots is required (an int in 1 .. 2^20); mps_expectation_values gives the "
                         "values without shot noise")
    shots = check_shots(shots, "sample_mps_expectation_values")
    return run_mps_shots(compile_mps_shots(circuits, observables, noise, trajectories, max_bond, cutoff, thermal_relaxation, pauli_twirl),
                         shots, seed, run_keys, return_bits, device)


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
