"""Host side of the batched simulator: circuits -> the flat programs ``mlqem_sim_run_f64`` runs (include/mlqem_hip.h has the
record layouts).  Nothing here touches the GPU.

Conventions are qiskit's: qubit 0 is the least significant index bit, and the rightmost character of a Pauli label acts on qubit
0.  Gate matrices are built with Python's float64 ``math`` functions.  Everything is validated here, before anything is launched:
the kernel clamps what it reads, but a refused circuit must be refused by name, not simulated as something else.
"""
from __future__ import annotations

import cmath
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..data.backends import PauliObservable, _apply_unit_prefix, pauli_terms
from ..data.circuit import Circuit

WAVE_AMPS = 256     # MLQEM_SIM_WAVE_AMPS: a wave per circuit
MAX_AMPS = 2048     # MLQEM_SIM_MAX_AMPS: a workgroup per circuit; the cap
PARAM_PAD = 32      # float64 values of padding at the end of the parameter pool
MAX_QUBITS_VECTOR = 11
MAX_QUBITS_DENSITY = 5

MAX_SHOTS = 2 ** 20  # MLQEM_SIM_MAX_SHOTS: counts are int32 and a Philox counter word holds shot >> 1
MAX_TRAJECTORIES = 2 ** 20  # MLQEM_SIM_MAX_TRAJECTORIES: a Philox counter word holds sub-draw << 24 | trajectory
MODE_TRAJECTORY = 2  # circ[c, 1] of a batch lowered for mlqem_sim_run_trajectories_f64

OP_U1, OP_DIAG1, OP_CX, OP_CZ, OP_SWAP, OP_U2, OP_DEPOL1, OP_DEPOL2, OP_READOUT, OP_MEASURE = range(10)   # MLQEM_SIM_OP_*
OP_NOISE1, OP_NOISE2 = 10, 11   # the fused noise records: depolarising, then thermal relaxation of the gate's qubits

_N_PARAMS = {"id": 0, "x": 0, "y": 0, "z": 0, "h": 0, "s": 0, "sdg": 0, "t": 0, "tdg": 0, "sx": 0, "sxdg": 0, "rx": 1, "ry": 1,
             "rz": 1, "p": 1, "u1": 1, "u2": 2, "u3": 3, "u": 3, "cx": 0, "cz": 0, "swap": 0, "ecr": 0, "rzz": 1}
_TWO_QUBIT = {"cx", "cz", "swap", "ecr", "rzz"}
SUPPORTED_GATES = tuple(_N_PARAMS)

_R = math.sqrt(0.5)


def _u3(theta: float, phi: float, lam: float) -> List[complex]:
    c, s = math.cos(theta / 2), math.sin(theta / 2)
    return [c, -cmath.exp(1j * lam) * s, cmath.exp(1j * phi) * s, cmath.exp(1j * (phi + lam)) * c]


def _one_qubit(name: str, p: Tuple[float, ...]):
    """(kind, complex entries): two phases for a diagonal gate, a row-major 2x2 matrix otherwise; None for ``id``."""
    if name == "id":
        return None
    if name == "z":
        return OP_DIAG1, [1.0, -1.0]
    if name == "s":
        return OP_DIAG1, [1.0, 1j]
    if name == "sdg":
        return OP_DIAG1, [1.0, -1j]
    if name == "t":
        return OP_DIAG1, [1.0, cmath.exp(0.25j * math.pi)]
    if name == "tdg":
        return OP_DIAG1, [1.0, cmath.exp(-0.25j * math.pi)]
    if name == "rz":
        return OP_DIAG1, [cmath.exp(-0.5j * p[0]), cmath.exp(0.5j * p[0])]
    if name in ("p", "u1"):
        return OP_DIAG1, [1.0, cmath.exp(1j * p[0])]
    if name == "x":
        return OP_U1, [0.0, 1.0, 1.0, 0.0]
    if name == "y":
        return OP_U1, [0.0, -1j, 1j, 0.0]
    if name == "h":
        return OP_U1, [_R, _R, _R, -_R]
    if name == "sx":
        return OP_U1, [0.5 + 0.5j, 0.5 - 0.5j, 0.5 - 0.5j, 0.5 + 0.5j]
    if name == "sxdg":
        return OP_U1, [0.5 - 0.5j, 0.5 + 0.5j, 0.5 + 0.5j, 0.5 - 0.5j]
    if name == "rx":
        c, s = math.cos(p[0] / 2), math.sin(p[0] / 2)
        return OP_U1, [c, -1j * s, -1j * s, c]
    if name == "ry":
        c, s = math.cos(p[0] / 2), math.sin(p[0] / 2)
        return OP_U1, [c, -s, s, c]
    if name == "u2":
        return OP_U1, _u3(math.pi / 2, p[0], p[1])
    return OP_U1, _u3(p[0], p[1], p[2])   # u3, u


def _two_qubit(name: str, p: Tuple[float, ...]):
    """(kind, complex entries of a row-major 4x4 matrix over the basis index bit(q0) + 2 bit(q1), or [])."""
    if name == "cx":
        return OP_CX, []
    if name == "cz":
        return OP_CZ, []
    if name == "swap":
        return OP_SWAP, []
    if name == "ecr":   # (IX - XY) / sqrt(2), the left factor on q1
        r = _R
        return OP_U2, [0, r, 0, 1j * r, r, 0, -1j * r, 0, 0, 1j * r, 0, r, -1j * r, 0, r, 0]
    a, b = cmath.exp(-0.5j * p[0]), cmath.exp(0.5j * p[0])   # rzz
    return OP_U2, [a, 0, 0, 0, 0, b, 0, 0, 0, 0, b, 0, 0, 0, 0, a]


def _check_relaxation(key, triples, width: Optional[int] = None) -> Tuple[Tuple[float, float, float], ...]:
    """One (g, c, p1) triple per qubit, or a ``ValueError`` that names ``key`` and the value that is out of range."""
    out = tuple(tuple(float(v) for v in t) for t in triples)
    if not out or any(len(t) != 3 for t in out) or len(out) > 2 or (width is not None and len(out) != width):
        raise ValueError(f"NoiseModel: relaxation of {key} is {triples!r}, want one (g, c, p1) triple per qubit of the gate")
    for g, c, p1 in out:
        if not (math.isfinite(g) and 0.0 <= g <= 1.0):
            raise ValueError(f"NoiseModel: relaxation of {key}: reset probability g = {g!r}, want 0 <= g <= 1")
        if not (math.isfinite(p1) and 0.0 <= p1 <= 1.0):
            raise ValueError(f"NoiseModel: relaxation of {key}: excited-state population p1 = {p1!r}, want 0 <= p1 <= 1")
        if not (math.isfinite(c) and 0.0 <= c <= math.sqrt(1.0 - g)):
            raise ValueError(f"NoiseModel: relaxation of {key}: coherence factor c = {c!r}, want 0 <= c <= sqrt(1 - g) = "
                             f"{math.sqrt(1.0 - g)!r} (complete positivity: T2 <= 2 T1)")
    return out


def _check_coherent(key, matrix) -> np.ndarray:
    """A 4x4 unitary (to 1e-12), or a ``ValueError`` that names ``key``."""
    m = np.asarray(matrix, dtype=complex)
    if m.shape != (4, 4) or not np.all(np.isfinite(m)):
        raise ValueError(f"NoiseModel: coherent error of {key} has the shape {m.shape}, want a finite 4x4 matrix")
    dev = float(np.abs(m.conj().T @ m - np.eye(4)).max())
    if dev > 1e-12:
        raise ValueError(f"NoiseModel: coherent error of {key} is not unitary: max |U^dagger U - 1| = {dev:.3e}, want <= 1e-12")
    return m


class NoiseModel:
    """The noise model of the density-matrix mode.  After a gate come, in this order: an optional coherent error (a two-qubit
    unitary), a depolarising op, and thermal relaxation of the gate's qubits; a readout op per measured qubit ends the circuit.

    ``gate_lambda``: ``{(name, (qubits...)): lambda}``, the depolarising parameter of
    ``rho -> (1 - lambda) rho + lambda Tr_S(rho) (x) I/d`` applied after every such gate on its qubits S (d = 2 or 4);
    ``gate_relaxation``: ``{(name, (qubits...)): ((g, c, p1), ...)}``, one triple per qubit of the gate: the qubit is reset with
    probability ``g = 1 - exp(-t / T1)`` (to |1> with probability p1, the excited-state population, else to |0>) and its
    coherences shrink by ``c = exp(-t / T2)``; ``0 <= c <= sqrt(1 - g)`` keeps the map completely positive (T2 <= 2 T1);
    ``gate_coherent``: ``{(name, (q0, q1)): 4x4 unitary}`` over the basis index bit(q0) + 2 bit(q1), applied right after the gate;
    ``readout``: ``{qubit: (p01, p10)}`` with p01 = P(read 0 | prepared 1) and p10 = P(read 1 | prepared 0).  Qubits are
    indices inside their register (``Circuit.qubit_reg_index``), as calibration tables count them.  An empty model is the
    noiseless density-matrix mode.  Subclasses may override :meth:`after_gate` / :meth:`relaxation_after` /
    :meth:`coherent_after` / :meth:`readout_of`; a duck-typed model may leave ``relaxation_after`` and ``coherent_after`` out.

    :meth:`from_backend` has two forms.  The default is the project's own depolarising + readout model.  With
    ``thermal_relaxation=True`` it restates the device model of Aer's ``NoiseModel.from_backend`` (gate times, T1, T2, the
    depolarising part rebalanced against the relaxation part), and that form reproduces the ``noisy`` columns of the reference's
    datasets within their shot noise (tests/test_relax_cpu.py) -- without readout noise, which those datasets
    were evidently made without."""

    def __init__(self, gate_lambda: Optional[Dict[Tuple[str, Tuple[int, ...]], float]] = None,
                 readout: Optional[Dict[int, Tuple[float, float]]] = None, strict_two_qubit: bool = False, name: str = "custom",
                 gate_relaxation: Optional[Dict[Tuple[str, Tuple[int, ...]], Sequence[Tuple[float, float, float]]]] = None,
                 gate_coherent: Optional[Dict[Tuple[str, Tuple[int, ...]], Any]] = None):
        self.gate_lambda = dict(gate_lambda or {})
        self.readout = dict(readout or {})
        self.strict_two_qubit = bool(strict_two_qubit)
        self.name = name
        for key, lam in self.gate_lambda.items():
            if not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
                raise ValueError(f"NoiseModel: depolarising parameter of {key} is {lam!r}, want 0 <= lambda <= 1")
        for q, (p01, p10) in self.readout.items():
            if not all(math.isfinite(v) and 0.0 <= v <= 1.0 for v in (p01, p10)):
                raise ValueError(f"NoiseModel: readout probabilities of qubit {q} are {(p01, p10)!r}, want both in [0, 1]")
        self.gate_relaxation = {(str(k[0]), tuple(int(q) for q in k[1])): _check_relaxation(k, v, len(k[1]))
                                for k, v in (gate_relaxation or {}).items()}
        self.gate_coherent = {}
        for k, v in (gate_coherent or {}).items():
            if len(k[1]) != 2:
                raise ValueError(f"NoiseModel: coherent error of {k}: want a two-qubit gate (a 4x4 unitary on its pair)")
            self.gate_coherent[(str(k[0]), tuple(int(q) for q in k[1]))] = _check_coherent(k, v)

    def after_gate(self, index: int, name: str, qubits: Tuple[int, ...]) -> Optional[float]:
        """lambda of the depolarising op after op ``index`` (``name`` on register qubits ``qubits``), or None for none."""
        lam = self.gate_lambda.get((name, tuple(qubits)))
        if lam is None and self.strict_two_qubit and len(qubits) == 2 and (name, tuple(qubits)) not in self.gate_relaxation:
            raise ValueError(f"noise model {self.name!r} has no calibration entry for {name} on the qubit pair {tuple(qubits)}")
        return lam if lam else None

    def relaxation_after(self, index: int, name: str, qubits: Tuple[int, ...]):
        """``((g, c, p1), ...)`` of the thermal relaxation after op ``index``, one triple per qubit, or None for none."""
        return self.gate_relaxation.get((name, tuple(qubits)))

    def coherent_after(self, index: int, name: str, qubits: Tuple[int, ...]):
        """The 4x4 unitary applied right after op ``index`` (basis index bit(q0) + 2 bit(q1)), or None for none."""
        return self.gate_coherent.get((name, tuple(qubits)))

    def readout_of(self, qubit: int) -> Optional[Tuple[float, float]]:
        return self.readout.get(qubit)

    @property
    def has_readout(self) -> bool:
        return bool(self.readout)

    @property
    def non_pauli(self) -> Optional[str]:
        """Why the model is no Pauli channel after Clifford gates (the Clifford path refuses it with these words), or None."""
        if self.gate_relaxation:
            return "it has thermal relaxation, which is not a Pauli channel"
        if self.gate_coherent:
            return "it has a coherent error (a controlled rotation), which is not a Clifford gate"
        return None

    @staticmethod
    def from_backend(backend: Any, readout: bool = True, thermal_relaxation: bool = False,
                     excited_state_population: float = 0.0) -> "NoiseModel":
        """From the calibration table the data layer reads (``backend.properties()``).

        Default (``thermal_relaxation=False``), the project's own model: after every gate (name, qubits) with a ``gate_error``
        e > 0 a depolarising op with ``lambda = e d / (d - 1)`` (d = 2, 4: the relation between the average gate infidelity and
        the depolarising parameter, so lambda = 2 e and 4 e / 3); per measured qubit a readout op from ``prob_meas0_prep1`` /
        ``prob_meas1_prep0``, or from a symmetric ``readout_error`` when those are missing.  A two-qubit gate without a
        calibration entry is refused when a circuit uses it.

        ``thermal_relaxation=True`` restates the device model of Aer's ``NoiseModel.from_backend``.  A gate (name, qubits) with
        ``gate_error`` e and ``gate_length`` t > 0 (units as the table gives them) relaxes each of its qubits with
        ``g = 1 - exp(-t / T1)``, ``c = exp(-t / min(T2, 2 T1))`` and ``p1 = excited_state_population``.  That channel has the
        process fidelity ``F_pro = prod_q (1 + 2 c_q + (1 - g_q)) / 4`` and the average gate fidelity
        ``F = (d F_pro + 1) / (d + 1)``, d = 2^k.  Only where the calibrated error exceeds what relaxation already explains,
        ``e > 1 - F``, a depolarising op precedes it, with ``lambda = d (min(e, d / (d + 1)) - (1 - F)) / (d F - 1)`` capped at
        ``4^k / (4^k - 1)``, so that the composed channel has the calibrated infidelity (a table that would need lambda > 1 is
        refused by name, as in the default form).  A gate with t = 0 or without a gate
        length relaxes nothing (F = 1: lambda is the default form's).  Readout is as in the default form."""
        props = backend.properties()
        p1 = float(excited_state_population)
        if not (math.isfinite(p1) and 0.0 <= p1 <= 1.0):
            raise ValueError(f"NoiseModel.from_backend: excited_state_population = {excited_state_population!r}, want 0 <= p1 <= 1")
        lam: Dict[Tuple[str, Tuple[int, ...]], float] = {}
        relax: Dict[Tuple[str, Tuple[int, ...]], Tuple[Tuple[float, float, float], ...]] = {}
        times = [props.qubit_property(q) for q in range(len(props.qubits))] if thermal_relaxation else []
        for gate in props.gates:
            qubits = tuple(int(q) for q in gate.qubits)
            if len(qubits) not in (1, 2):
                continue
            err = next((float(p.value) for p in gate.parameters if p.name == "gate_error"), None)
            if err is None:
                continue
            d = 2 ** len(qubits)
            if thermal_relaxation:
                t = next((_apply_unit_prefix(float(p.value), p.unit) for p in gate.parameters if p.name == "gate_length"), 0.0)
                if not (math.isfinite(t) and t >= 0.0):
                    raise ValueError(f"NoiseModel.from_backend: gate_length {t!r} of {gate.gate} on {qubits}, want a finite time >= 0")
                f_pro, triples = 1.0, []
                for q in qubits:
                    t1, t2 = (times[q].get(k, (math.inf, None))[0] for k in ("T1", "T2"))
                    if not (t1 > 0.0 and t2 > 0.0):
                        raise ValueError(f"NoiseModel.from_backend: qubit {q} has T1 = {t1!r}, T2 = {t2!r}, want both > 0")
                    g, c = 1.0 - math.exp(-t / t1), math.exp(-t / min(t2, 2.0 * t1))
                    c = min(c, math.sqrt(1.0 - g))   # T2 capped at 2 T1 is c = sqrt(1 - g) up to rounding: keep it inside
                    triples.append((g, c, p1))
                    f_pro *= (1.0 + 2.0 * c + (1.0 - g)) / 4.0
                if t > 0.0:
                    relax[(str(gate.gate), qubits)] = tuple(triples)
                fid = (d * f_pro + 1.0) / (d + 1.0)
                value = 0.0
                if err > 1.0 - fid:
                    value = min(d * (min(err, d / (d + 1.0)) - (1.0 - fid)) / (d * fid - 1.0), d * d / (d * d - 1.0))
            else:
                value = err * d / (d - 1)
            if not (math.isfinite(value) and 0.0 <= value <= 1.0):
                raise ValueError(f"NoiseModel.from_backend: gate_error {err!r} of {gate.gate} on {qubits} gives lambda = {value!r}, "
                                 "want 0 <= lambda <= 1")
            if value or not thermal_relaxation:
                lam[(str(gate.gate), qubits)] = value
        ro: Dict[int, Tuple[float, float]] = {}
        if readout:
            for q in range(len(props.qubits)):
                qp = props.qubit_property(q)
                sym = qp.get("readout_error", (0.0, None))[0]
                p01 = qp.get("prob_meas0_prep1", (sym, None))[0]
                p10 = qp.get("prob_meas1_prep0", (sym, None))[0]
                ro[q] = (float(p01), float(p10))
        name = backend.name() if callable(getattr(backend, "name", None)) else getattr(backend, "name", "backend")
        return NoiseModel(lam, ro, strict_two_qubit=True, name=str(name), gate_relaxation=relax)

    def with_cx_over_rotation(self, theta: float, uniform: bool = True, seed: Optional[int] = None) -> "NoiseModel":
        """A new model in which every calibrated ``cx (control, target)`` over-rotates: a controlled-RX(theta), controlled on
        the cx's control and acting on its target, follows the gate and precedes its depolarising and relaxation part (so the
        gate acts as ``I (x) |0><0| + i RX(pi + theta) (x) |1><1|``, the over-rotated CNOT of the reference's noise study).
        ``uniform=False`` draws one angle ``theta_pair ~ U(0, theta)`` per calibrated direction, in the order of the table, from
        ``numpy.random.default_rng(seed)``: this model's own stream, not the global one the reference seeds, so its angles are
        not the reference's.  Everything else is copied."""
        theta = float(theta)
        if not math.isfinite(theta):
            raise ValueError(f"NoiseModel.with_cx_over_rotation: theta = {theta!r}, want a finite angle")
        pairs = [k for k in dict.fromkeys(list(self.gate_lambda) + list(self.gate_relaxation)) if k[0] == "cx" and len(k[1]) == 2]
        rng = None if uniform else np.random.default_rng(seed)
        coherent = dict(self.gate_coherent)
        for key in pairs:
            th = theta if uniform else float(rng.uniform(0.0, 1.0)) * theta
            c, s = math.cos(th / 2), math.sin(th / 2)
            m = np.eye(4, dtype=complex)   # basis index bit(control) + 2 bit(target): the rotation acts where the control is 1
            m[1, 1], m[1, 3], m[3, 1], m[3, 3] = c, -1j * s, -1j * s, c
            coherent[key] = m
        return NoiseModel(self.gate_lambda, self.readout, self.strict_two_qubit, self.name, self.gate_relaxation, coherent)


@dataclass
class SimBatch:
    """A lowered batch: the host arrays of ``mlqem_sim_run_f64`` plus what the host knows about every circuit."""

    circ: np.ndarray        # int32 [B, 4]: n_qubits, mode (0 vector, 1 density, 2 trajectory), trailing readout ops, measurement-tail records
    op_ptr: np.ndarray      # int64 [B + 1]
    ops: np.ndarray         # int32 [n_ops, 4]: kind, q0, q1, offset into params
    params: np.ndarray      # float64 [n_params + 32]
    term_ptr: np.ndarray    # int64 [B + 1]
    terms: np.ndarray       # int32 [n_terms, 4]: xmask, zmask, number of Y, 0
    coeff: np.ndarray       # float64 [n_terms]
    ids: np.ndarray         # int32 [B]: the wave-per-circuit circuits first, then the workgroup-per-circuit ones
    n_wave: int
    n_wg: int
    variant: List[str] = field(default_factory=list)            # "wave" | "workgroup" per circuit
    measured: List[Dict[int, int]] = field(default_factory=list)   # classical bit -> qubit per circuit
    # the record map of the source gates (barrier and measure are no gates): what blackwater.sim.zne folds.  Record indices are
    # relative to op_ptr[c]; -1 = absent (``id`` has no gate record, a gate without noise no depolarising record)
    gate_ptr: Optional[np.ndarray] = None      # int64 [B + 1]: circuit c owns gates gate_ptr[c] .. gate_ptr[c + 1]
    gate_record: Optional[np.ndarray] = None   # int32 [n_gates]: the gate's own record
    gate_noise: Optional[np.ndarray] = None    # int32 [n_gates]: the first noise record after it
    gate_name: Optional[np.ndarray] = None     # int16 [n_gates]: index of the gate's name in SUPPORTED_GATES
    gate_op: Optional[np.ndarray] = None       # int32 [n_gates]: index of the gate in the circuit's op list
    # noise records after the gate's own, from gate_noise on: 0, 1 (DEPOL* or NOISE*) or 2 (a coherent U2, then DEPOL* / NOISE*)
    gate_noise_len: Optional[np.ndarray] = None   # int32 [n_gates]
    # measurement (``compile_programs(..., shots=)``): the groups of qubit-wise commuting terms, one measurement basis each
    shots: Optional[int] = None
    group_ptr: Optional[np.ndarray] = None     # int64 [B + 1]: circuit c owns groups group_ptr[c] .. group_ptr[c + 1]
    term_group: Optional[np.ndarray] = None    # int32 [n_terms]: the term's group, counted inside its circuit
    prob_ptr: Optional[np.ndarray] = None      # int64 [n_groups + 1]: offsets into the pool of sum 2^n outcomes
    group_circ: Optional[np.ndarray] = None    # int32 [n_groups]: the circuit a group belongs to
    group_basis: Optional[np.ndarray] = None   # int32 [n_groups, 2]: (qubits measured in X, qubits measured in Y); the rest in Z
    # quantum trajectories (``compile_programs(..., trajectories=)``): density mode's records on a state vector, mode 2.  Only
    # ``blackwater.sim.run_trajectories`` runs such a batch; every other entry point refuses it (:meth:`refuse_trajectories`)
    trajectories: Optional[int] = None

    def refuse_trajectories(self, who: str) -> None:
        """A ``ValueError`` when the batch was lowered in trajectory mode: the kernels behind ``who`` read mode != 0 as a density matrix."""
        if self.trajectories is not None:
            raise ValueError(f"{who}: the batch was lowered for quantum trajectories (compile_programs(..., trajectories="
                             f"{self.trajectories})); only run_trajectories runs it (folded / ZNE runs and shot sampling over "
                             "trajectories are not supported)")

    def __len__(self) -> int:
        return int(self.circ.shape[0])

    @property
    def op_counts(self) -> np.ndarray:
        return np.diff(self.op_ptr)

    def to(self, device) -> Dict[str, Any]:
        """The arrays as tensors on ``device``, keyed as ``ops.sim_run`` names them."""
        out = upload_fields(self, ("circ", "op_ptr", "ops", "params", "term_ptr", "terms", "coeff", "ids"), device)
        out["n_wave"], out["n_wg"] = self.n_wave, self.n_wg
        if self.group_ptr is not None:
            out.update(upload_fields(self, ("group_ptr", "term_group", "prob_ptr", "group_circ"), device))
        return out

    def sample_units(self, n_factors: int = 1):
        """``(units int32 [F * n_groups], n_wave, n_wg)`` for ``ops.sim_sample``: every (noise factor, group) pair as
        ``f * n_groups + g``, those of at most 256 outcomes (a wave each) first, then the others (a workgroup each)."""
        if self.group_ptr is None:
            raise ValueError("sample_units: the batch carries no measurement groups (compile_programs was called without shots)")
        n_groups = int(self.group_circ.shape[0])
        outcomes = np.diff(self.prob_ptr)
        base = np.arange(int(n_factors), dtype=np.int64)[:, None] * n_groups
        wave = (base + np.flatnonzero(outcomes <= WAVE_AMPS)[None, :]).reshape(-1)
        wg = (base + np.flatnonzero(outcomes > WAVE_AMPS)[None, :]).reshape(-1)
        if int(n_factors) * n_groups > 2 ** 31 - 1:
            raise ValueError(f"sample_units: {int(n_factors) * n_groups} (factor, group) pairs exceed the 2^31 - 1 one call can take")
        return np.concatenate([wave, wg]).astype(np.int32), int(wave.size), int(wg.size)


def _lower_terms(observable: Any, n: int, where: str):
    rows, coeffs, has_xy = [], [], False
    for label, coeff in pauli_terms(observable):
        if len(label) != n:
            raise ValueError(f"{where}: Pauli label {label!r} has {len(label)} characters, the circuit has {n} qubits")
        c = complex(coeff)
        if c.imag != 0.0 or not math.isfinite(c.real):
            raise ValueError(f"{where}: coefficient {coeff!r} of {label!r} is not a finite real number")
        xm = zm = ny = 0
        for q, ch in enumerate(reversed(label)):
            if ch == "X":
                xm |= 1 << q
            elif ch == "Z":
                zm |= 1 << q
            elif ch == "Y":
                xm |= 1 << q
                zm |= 1 << q
                ny += 1
            elif ch != "I":
                raise ValueError(f"{where}: Pauli label {label!r} has the character {ch!r}, want only I, X, Y, Z")
        has_xy = has_xy or xm != 0
        rows.append((xm, zm, ny, 0))
        coeffs.append(c.real)
    return rows, coeffs, has_xy


def check_shots(shots: Any, who: str) -> int:
    """``shots`` as an int in 1 .. 2^20, or a ``ValueError`` that names it."""
    if isinstance(shots, bool) or not isinstance(shots, (int, np.integer)) or not 1 <= int(shots) <= MAX_SHOTS:
        raise ValueError(f"{who}: shots = {shots!r}, want an int in 1 .. 2^20 = {MAX_SHOTS}")
    return int(shots)


def check_trajectories(trajectories: Any, who: str) -> int:
    """``trajectories`` as an int in 1 .. 2^20, or a ``ValueError`` that names it."""
    if (isinstance(trajectories, bool) or not isinstance(trajectories, (int, np.integer))
            or not 1 <= int(trajectories) <= MAX_TRAJECTORIES):
        raise ValueError(f"{who}: trajectories = {trajectories!r}, want an int in 1 .. 2^20 = {MAX_TRAJECTORIES}")
    return int(trajectories)


def check_seed(seed: Any, who: str) -> int:
    """``seed`` as an int reduced mod 2^64, or a ``ValueError`` that names it."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"{who}: seed = {seed!r}, want an int (it is reduced mod 2^64)")
    return int(seed) % 2 ** 64


def default_run_keys(n_runs: int, offset: int = 0) -> np.ndarray:
    """int64 [n_runs]: ``offset + r`` for run r = f * B + c, the counter words a run draws with unless the caller passes its own."""
    return np.arange(int(n_runs), dtype=np.int64) + np.int64(offset)


def _run_keys(run_keys, n_runs: int, who: str, per: str = "run") -> np.ndarray:
    """``run_keys`` as int64 [n_runs] (None: :func:`default_run_keys`), or a ``ValueError`` that names ``who``."""
    if run_keys is None:
        return default_run_keys(n_runs)
    keys = np.asarray(run_keys)
    if keys.shape != (n_runs,) or keys.dtype.kind not in "iu":
        raise ValueError(f"{who}: run_keys must be {n_runs} integers (one per {per}), got shape {keys.shape} dtype {keys.dtype}")
    return keys.astype(np.int64)


def upload(array, dev):
    """A host array as a tensor on ``dev``: the one host-to-device copy of the package."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(array)).to(dev)


def upload_fields(obj: Any, names: Sequence[str], dev, view: Optional[Dict[str, Any]] = None) -> Dict[str, Any]:
    """``{name: upload(obj.name)}``; ``view`` names the dtype an array travels as (uint32 words as int32, uint64 as int64)."""
    import torch

    dev = torch.device(dev)
    if not view:
        return {k: upload(getattr(obj, k), dev) for k in names}
    return {k: upload(np.ascontiguousarray(getattr(obj, k)).view(view[k]) if k in view else getattr(obj, k), dev) for k in names}


def measurement_groups(term_rows: Sequence[Tuple[int, int, int, int]]):
    """Greedy qubit-wise commuting groups of one circuit's lowered terms ``(xmask, zmask, ny, 0)``, in term order: a term joins the
    first group whose basis agrees with it on every qubit where the term is not the identity (the group's basis is then extended by
    the term's qubits), else it opens a new group.  Returns ``(term_group, bases)``: the group of every term and ``(x, y)`` per
    group, the qubits measured in X and in Y (all others in Z).  A circuit without terms still gets one all-Z group."""
    groups: List[List[int]] = []   # [x, y, z] masks of the qubits whose basis is fixed
    term_group = []
    for xm, zm, _, _ in term_rows:
        tx, ty, tz = xm & ~zm, xm & zm, zm & ~xm
        for g, (gx, gy, gz) in enumerate(groups):
            if not (tx & (gy | gz) or ty & (gx | gz) or tz & (gx | gy)):
                groups[g] = [gx | tx, gy | ty, gz | tz]
                term_group.append(g)
                break
        else:
            groups.append([tx, ty, tz])
            term_group.append(len(groups) - 1)
    if not groups:
        groups.append([0, 0, 0])
    return term_group, [(g[0], g[1]) for g in groups]


# the basis changes of a measurement group, as noise-free U1 records: H for X; H S^dagger for Y, and its inverse S H
_ROT_X = [_R, _R, _R, -_R]
_ROT_Y = [_R, -1j * _R, _R, 1j * _R]
_ROT_Y_INV = [_R, _R, 1j * _R, -1j * _R]


def compile_programs(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                     shots: Optional[int] = None, trajectories: Optional[int] = None) -> SimBatch:
    """Lowers ``circuits`` (anything ``Circuit.from_any`` takes) with one observable each (anything ``pauli_terms`` takes) to one
    :class:`SimBatch`.  ``noise=None``: state vectors (at most 11 qubits); a :class:`NoiseModel`: density matrices (at most 5
    qubits) with its noise records (a depolarising record after a gate as ever; where the model has thermal relaxation for the gate,
    one fused ``NOISE1`` / ``NOISE2`` record in its place; before either, a ``U2`` record where it has a coherent error) and readout ops.

    Lowered: ``id x y z h s sdg t tdg sx sxdg rx ry rz p u1 u2 u3 u cx cz swap ecr rzz``; ``barrier`` is ignored; ``measure``
    records classical bit -> qubit (and gets the qubit's readout op, after every other op).  Raises ``ValueError`` naming the
    offender for: any other gate (opaque custom gates and ``reset`` included), a wrong parameter count, a gate on a qubit after
    it was measured, a qubit index out of range, a two-qubit gate on one qubit twice, a non-finite angle, a Pauli label of the
    wrong length or alphabet, a coefficient that is not real, a circuit over the amplitude cap of its mode, and readout noise
    together with a term that contains X or Y (a readout op leaves only the diagonal of rho meaningful).

    ``shots`` (an int in 1 .. 2^20; ``None``: the batch is what it always was): the batch is lowered for MEASUREMENT.  Every
    circuit's terms are partitioned into groups (:func:`measurement_groups`), and after the circuit's ops and its readout ops
    every group appends a tail to the program: its basis rotations as ``U1`` records (H for X, H S^dagger for Y, in qubit order),
    one ``MEASURE`` record (q0: the group inside its circuit, param: the group's number in ``prob_ptr``), and the inverse
    rotations, so that the next group and the exact term values see the circuit's own state.  ``circ[c, 3]`` counts these tail
    records; ``norm`` is still taken before the readout ops.  Such a batch runs through ``ops.sim_run_measured`` /
    ``ops.sim_run_folded_measured``; the plain entry points skip a MEASURE record and would misplace ``norm``.

    ``trajectories`` (an int in 1 .. 2^20, with a noise model; ``None``: the batch is what it always was): the batch is lowered in
    TRAJECTORY mode for ``blackwater.sim.run_trajectories``.  The records are the ones density mode emits, ``circ[c, 1] = 2``, and
    the state is a vector: the cap is 2^n <= 2 048 amplitudes (11 qubits) and ``variant`` is chosen on 2^n.  Everything density
    mode refuses is refused, and so are ``trajectories`` without a noise model and ``trajectories`` together with ``shots``."""
    circuits, observables = list(circuits), list(observables)
    if trajectories is not None:
        trajectories = check_trajectories(trajectories, "compile_programs")
        if noise is None:
            raise ValueError("compile_programs: trajectories without a noise model (a noiseless circuit has one trajectory: "
                             "lower it without trajectories and run it as a state vector)")
        if shots is not None:
            raise ValueError("compile_programs: trajectories together with shots (shot sampling over trajectories is not supported)")
    if shots is not None:
        shots = check_shots(shots, "compile_programs")
    if len(circuits) != len(observables):
        raise ValueError(f"compile_programs: {len(circuits)} circuits but {len(observables)} observables")
    density = noise is not None   # the records of density mode; in trajectory mode they act on a state vector
    matrix = density and trajectories is None
    cap_q = MAX_QUBITS_DENSITY if matrix else MAX_QUBITS_VECTOR
    circ_rows, ops, params, op_ptr, term_rows, coeffs, term_ptr = [], [], [], [0], [], [], [0]
    variant, measured_all = [], []
    gate_ptr, gate_record, gate_noise, gate_name, gate_op, gate_noise_len = [0], [], [], [], [], []
    # optional hooks: a duck-typed model with after_gate / readout_of alone lowers as it always did
    relaxation_after, coherent_after = getattr(noise, "relaxation_after", None), getattr(noise, "coherent_after", None)
    group_ptr, term_group, prob_ptr, group_circ, group_basis = [0], [], [0], [], []
    name_id = {g: j for j, g in enumerate(SUPPORTED_GATES)}

    def emit(kind, q0, q1, values):
        ops.append((kind, q0, q1, len(params)))
        params.extend(values)

    def emit_complex(kind, q0, q1, entries):
        flat = []
        for e in entries:
            e = complex(e)
            flat += [e.real, e.imag]
        emit(kind, q0, q1, flat)

    for k, (obj, obs) in enumerate(zip(circuits, observables)):
        circ = Circuit.from_any(obj)
        where = f"circuit {k}"
        n = circ.num_qubits
        amps = 4 ** n if matrix else 2 ** n
        if n < 1 or amps > MAX_AMPS:
            raise ValueError(f"{where}: {n} qubits need {amps} amplitudes as a {'density matrix' if matrix else 'state vector'}; "
                             f"the cap is {MAX_AMPS} amplitudes ({cap_q} qubits in this mode) and at least 1 qubit")
        measured: Dict[int, int] = {}
        done = set()
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
            first, rec, noi = op_ptr[-1], -1, -1
            if width == 2:
                q0, q1 = op.qubits
                if q0 == q1:
                    raise ValueError(f"{where}: op {i} ({name}) names qubit {q0} twice")
                kind, entries = _two_qubit(name, p)
                rec = len(ops) - first
                emit_complex(kind, q0, q1, entries)
            else:
                q0, q1 = op.qubits[0], 0
                lowered = _one_qubit(name, p)
                if lowered is not None:
                    rec = len(ops) - first
                    emit_complex(lowered[0], q0, 0, lowered[1])
            n_noise = 0
            if density:
                reg = tuple(circ.qubit_reg_index[q] for q in op.qubits)
                lam = noise.after_gate(i, name, reg)
                if lam is not None and not (math.isfinite(lam) and 0.0 <= lam <= 1.0):
                    raise ValueError(f"{where}: op {i} ({name}): depolarising parameter {lam!r}, want 0 <= lambda <= 1")
                coherent = coherent_after(i, name, reg) if coherent_after is not None else None
                relax = relaxation_after(i, name, reg) if relaxation_after is not None else None
                if coherent is not None:   # the coherent error: an ordinary U2 record, counted among the gate's noise records
                    if width != 2:
                        raise ValueError(f"{where}: op {i} ({name}): a coherent error is a 4x4 unitary, the gate has one qubit")
                    noi = len(ops) - first
                    emit_complex(OP_U2, q0, q1, _check_coherent((name, reg), coherent).reshape(-1))
                    n_noise += 1
                if relax is not None:      # one fused record: depolarising (lambda = 0: none), then relaxation
                    relax = _check_relaxation((name, reg), relax, width)
                    noi = len(ops) - first if noi < 0 else noi
                    emit(OP_NOISE2 if width == 2 else OP_NOISE1, q0, q1, [float(lam or 0.0)] + [v for t in relax for v in t])
                    n_noise += 1
                elif lam is not None:
                    noi = len(ops) - first if noi < 0 else noi
                    emit(OP_DEPOL2 if width == 2 else OP_DEPOL1, q0, q1, [float(lam)])
                    n_noise += 1
            gate_record.append(rec)
            gate_noise.append(noi)
            gate_noise_len.append(n_noise)
            gate_name.append(name_id[name])
            gate_op.append(i)
        rows, cs, has_xy = _lower_terms(obs, n, where)
        n_readout = 0
        if density:
            for q in sorted(set(measured.values())):
                pr = noise.readout_of(circ.qubit_reg_index[q])
                if pr is None:
                    continue
                if has_xy:
                    raise ValueError(f"{where}: readout noise on qubit {q} cannot be combined with an observable that has X or Y "
                                     "terms (a readout op leaves only the diagonal of the density matrix meaningful)"
                                     if matrix else
                                     f"{where}: readout noise on qubit {q} cannot be combined with an observable that has X or Y "
                                     "terms (the readout channel of a trajectory acts on the outcome distribution, which has "
                                     "only I / Z terms)")
                emit(OP_READOUT, q, 0, [float(pr[0]), float(pr[1])])
                n_readout += 1
        n_tail = 0
        if shots is not None:
            tg, bases = measurement_groups(rows)
            for gl, (bx, by) in enumerate(bases):
                qs = [q for q in range(n) if (bx | by) >> q & 1]
                for q in qs:
                    emit_complex(OP_U1, q, 0, _ROT_X if bx >> q & 1 else _ROT_Y)
                ops.append((OP_MEASURE, gl, 0, len(group_circ)))
                for q in reversed(qs):
                    emit_complex(OP_U1, q, 0, _ROT_X if bx >> q & 1 else _ROT_Y_INV)
                n_tail += 2 * len(qs) + 1
                group_circ.append(k)
                group_basis.append((bx, by))
                prob_ptr.append(prob_ptr[-1] + 2 ** n)
            term_group += tg
            group_ptr.append(len(group_circ))
        circ_rows.append((n, (1 if matrix else MODE_TRAJECTORY) if density else 0, n_readout, n_tail))
        op_ptr.append(len(ops))
        gate_ptr.append(len(gate_record))
        term_rows += rows
        coeffs += cs
        term_ptr.append(len(term_rows))
        variant.append("wave" if amps <= WAVE_AMPS else "workgroup")
        measured_all.append(measured)

    if len(params) + PARAM_PAD > 2 ** 31 - 1:
        raise ValueError(f"compile_programs: {len(params)} gate parameters exceed the 2^31 - 1 a record can address; split the batch")
    wave = [i for i, v in enumerate(variant) if v == "wave"]
    wg = [i for i, v in enumerate(variant) if v != "wave"]
    return SimBatch(
        circ=np.asarray(circ_rows, dtype=np.int32).reshape(-1, 4),
        op_ptr=np.asarray(op_ptr, dtype=np.int64),
        ops=np.asarray(ops, dtype=np.int32).reshape(-1, 4),
        params=np.asarray(params + [0.0] * PARAM_PAD, dtype=np.float64),
        term_ptr=np.asarray(term_ptr, dtype=np.int64),
        terms=np.asarray(term_rows, dtype=np.int32).reshape(-1, 4),
        coeff=np.asarray(coeffs, dtype=np.float64),
        ids=np.asarray(wave + wg, dtype=np.int32),
        n_wave=len(wave), n_wg=len(wg), variant=variant, measured=measured_all,
        gate_ptr=np.asarray(gate_ptr, dtype=np.int64), gate_record=np.asarray(gate_record, dtype=np.int32),
        gate_noise=np.asarray(gate_noise, dtype=np.int32), gate_name=np.asarray(gate_name, dtype=np.int16),
        gate_op=np.asarray(gate_op, dtype=np.int32), gate_noise_len=np.asarray(gate_noise_len, dtype=np.int32),
        trajectories=trajectories,
        **({} if shots is None else dict(
            shots=shots, group_ptr=np.asarray(group_ptr, dtype=np.int64), term_group=np.asarray(term_group, dtype=np.int32),
            prob_ptr=np.asarray(prob_ptr, dtype=np.int64), group_circ=np.asarray(group_circ, dtype=np.int32),
            group_basis=np.asarray(group_basis, dtype=np.int32).reshape(-1, 2))))


def measured_z(circuit: Any) -> PauliObservable:
    """One single-Z term per classical bit, in classical-bit order: term k is Z on the qubit measured into classical bit k (what
    the Ising datasets measure; their stored columns are ``-<Z>`` of classical bit 3 - k)."""
    circ = Circuit.from_any(circuit)
    where: Dict[int, int] = {}
    for op in circ.ops:
        if op.name == "measure":
            where[int(op.clbits[0])] = int(op.qubits[0])
    terms = []
    for c in sorted(where):
        label = ["I"] * circ.num_qubits
        label[circ.num_qubits - 1 - where[c]] = "Z"
        terms.append(("".join(label), 1.0))
    return PauliObservable(terms)
