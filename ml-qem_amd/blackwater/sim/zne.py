"""Zero-noise extrapolation on the batched simulator: noise amplification by gate folding, polynomial extrapolation to zero noise.

A folded circuit is the circuit's own gate records replayed in another order, some of them as their inverse.  So the circuits are
lowered ONCE (:func:`compile_programs`), every (circuit, noise factor) pair gets a *schedule* of 4 bytes per step
(:func:`build_schedules`), one call simulates all of them (``ops.sim_run_folded``) and one more extrapolates (``ops.zne_combine``):
:func:`zne_expectation_values`.  Names follow the ``zne`` prototype library the reference imports (``ZNEStrategy``,
``LocalFoldingAmplifier``, ``LinearExtrapolator``, the ``zne(cls)`` decorator); that library is not a dependency, and the semantics
are the ones written down here.

The fold rule.  The foldable set G of a circuit is its gates that match the amplifier, in circuit order (``barrier`` and
``measure`` are no gates); N = |G|.  For a noise factor lambda >= 1 (it may be fractional)::

    m = floor(N (lambda - 1) / 2 + 1/2),    (k, s) = divmod(m, N)

*Local* folding runs every gate g of G as g (g^-1 g)^k, and s of them once more: the first s of G, the last s, or
``default_rng(random_seed).choice(N, s, replace=False)`` (a fresh generator per choice, so the choice depends on (seed, N, s) alone:
the same alone and in any batch).  *Global* folding runs the whole circuit U as U (U^-1 U)^k and then L^-1 L for L = its last (or
first) s gates.  N = 0 runs the circuit unchanged at every factor.  The achieved factor 1 + 2 m / N is reported; the extrapolation
uses the REQUESTED factors, as the public ZNE libraries do.

Noise under folding (a modelling choice).  A fold unit is a gate together with the depolarising op the noise model puts after it: a
folded gate runs as G N G^-1 N G N, the inverse carrying the gate's OWN depolarising record (its name is not looked up again: for
``sx`` a by-name rule would find no calibration entry for ``sxdg`` and amplify nothing).  Readout ops run once, after everything.

Polynomial extrapolation of exact values is linear in them, so an extrapolator is a weight vector: ``weights(noise_factors)`` is
``e_0^T V^+`` for the Vandermonde matrix V of the factors, in float64 on the host.

Exponential extrapolation (:class:`ExponentialExtrapolator`) fits a straight line through (factor, ln|value|) per Pauli term and
exponentiates its value at zero noise: ``sign * exp(sum_f w_f ln|v_f|)`` with the degree-1 weights w.  It is exact for a value of
the form ``A * r^factor``, which is what a Clifford circuit's Pauli term is under this noise model (see below); a term whose values
are all 0 stays 0, and a term with a zero among nonzeros or with mixed signs falls back to the straight line and is counted.

At width.  ``method="clifford"`` (or ``"auto"``, by :class:`DeviceEstimator`'s rule) takes the same route on the Clifford path:
:func:`compile_clifford` once, :func:`build_clifford_schedules`, ``ops.clifford_run_folded``, then one combine.  A Pauli carried
backwards through a folded gate G N G^-1 N G N has the same support at the three N as at the one N of the unfolded gate (G^-1 undoes
what G did to it), so a folded gate's keep factor is multiplied in 1 + 2 folds times: the noisy value at an achieved factor x of a
circuit whose gates are all folded alike is ``ideal * F1 * F2^x``, F2 the product of the foldable gates' keeps that the unfolded walk
met and F1 that of the others.

Wide circuits at any angle.  ``method="mps"`` (by name alone) folds on matrix-product states: ``compile_mps`` with a noise model and
``trajectories`` once, :func:`build_mps_schedules` from the record map it keeps, every (run, trajectory) unit through
``ops.sim_run_mps_folded`` (:func:`run_mps_folded`), then the terms, finish and combine kernels with the F * B runs taken as a batch
of F * B circuits.  The per-factor values are means over Pauli-insertion trajectories, so the result carries their standard errors
and sqrt(sum_f w_f^2 se_f^2) for the mitigated value (polynomial extrapolators), and every run's truncation certificate.

Shots.  With ``shots=`` every (circuit, factor) run is measured (``ops.sim_run_folded_measured`` + ``ops.sim_sample``): per factor
the sampled values and their variances; the mitigated value is sum_f w_f value_f through the same combine, and the mitigated
variance is sum_f w_f^2 variance_f (the factors are sampled independently) -- the SAME ``mlqem_zne_combine_f64`` called with the
squared weights on an identity term layout (one "term" per circuit with coefficient 1), not a kernel of its own.  The standard error
of a mitigated value is sqrt(variance / shots).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Any, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from ..data.circuit import Circuit, CircuitOp
from ..library.primitives import make_estimator_result
from .clifford import CliffordBatch, compile_clifford, refuse_non_pauli
from .program import (_TWO_QUBIT, SUPPORTED_GATES, NoiseModel, SimBatch, _run_keys, check_seed, check_shots, check_trajectories, compile_programs,
                      upload, upload_fields)
from .run import _CLIFFORD_SHOTS, DeviceEstimator, use_clifford_path
from .template import has_free_parameters

_NOT_GATES = ("barrier", "measure")


# ---- amplifiers ------------------------------------------------------------------------------------------------------------------
def fold_counts(n_foldable: int, noise_factor: float) -> Tuple[int, int]:
    """``(k, s)`` of the fold rule: every foldable gate is folded k times and s of them once more.  (0, 0) for N = 0."""
    lam = float(noise_factor)
    if not math.isfinite(lam) or lam < 1.0:
        raise ValueError(f"noise factor {noise_factor!r}: want a finite number >= 1")
    if n_foldable <= 0:
        return 0, 0
    return divmod(int(math.floor(n_foldable * (lam - 1.0) / 2.0 + 0.5)), int(n_foldable))


def achieved_factor(n_foldable: int, noise_factor: float) -> float:
    k, s = fold_counts(n_foldable, noise_factor)
    return 1.0 + 2.0 * (k * n_foldable + s) / n_foldable if n_foldable > 0 else 1.0


class _Amplifier:
    kind = "local"
    sub_folding_option = "from_first"
    random_seed = None

    def matches(self, name: str, n_qubits: int) -> bool:
        raise NotImplementedError

    def _extra(self, n: int, s: int) -> np.ndarray:
        """Ranks (positions inside G) of the s gates that are folded once more."""
        if self.sub_folding_option == "from_first":
            return np.arange(s)
        if self.sub_folding_option == "from_last":
            return np.arange(n - s, n)
        return np.sort(np.random.default_rng(self.random_seed).choice(n, size=s, replace=False))


class LocalFoldingAmplifier(_Amplifier):
    """Folds gates one by one.  ``gates_to_fold``: ``None`` (every gate), an int (gates on exactly that many qubits), a gate name, or
    an iterable of names and ints."""

    def __init__(self, gates_to_fold: Union[None, int, str, Iterable[Union[int, str]]] = None, sub_folding_option: str = "from_first",
                 random_seed: Optional[int] = None):
        if sub_folding_option not in ("from_first", "from_last", "random"):
            raise ValueError(f"sub_folding_option {sub_folding_option!r}: want 'from_first', 'from_last' or 'random'")
        if gates_to_fold is None:
            self.gates_to_fold = None
        else:
            items = [gates_to_fold] if isinstance(gates_to_fold, (int, str)) else list(gates_to_fold)
            for it in items:
                if not isinstance(it, (int, str)) or isinstance(it, bool) or it in _NOT_GATES:
                    raise ValueError(f"gates_to_fold: {it!r} is neither a gate name nor a number of qubits")
            self.gates_to_fold = frozenset(items)
        self.sub_folding_option, self.random_seed = sub_folding_option, random_seed

    def matches(self, name, n_qubits):
        if name in _NOT_GATES:
            return False
        return self.gates_to_fold is None or name in self.gates_to_fold or n_qubits in self.gates_to_fold

    def __repr__(self):
        g = None if self.gates_to_fold is None else sorted(self.gates_to_fold, key=str)
        return f"{type(self).__name__}(gates_to_fold={g!r}, sub_folding_option={self.sub_folding_option!r})"


class TwoQubitAmplifier(LocalFoldingAmplifier):
    def __init__(self, sub_folding_option: str = "from_first", random_seed: Optional[int] = None):
        super().__init__(2, sub_folding_option, random_seed)


class CxAmplifier(LocalFoldingAmplifier):
    def __init__(self, sub_folding_option: str = "from_first", random_seed: Optional[int] = None):
        super().__init__("cx", sub_folding_option, random_seed)


class GlobalFoldingAmplifier(_Amplifier):
    """Folds the whole circuit: U (U^-1 U)^k, then L^-1 L for its last (``from_last``) or first (``from_first``) s gates."""

    kind = "global"

    def __init__(self, sub_folding_option: str = "from_last"):
        if sub_folding_option not in ("from_first", "from_last"):
            raise ValueError(f"sub_folding_option {sub_folding_option!r}: want 'from_last' or 'from_first'")
        self.sub_folding_option = sub_folding_option

    def matches(self, name, n_qubits):
        return name not in _NOT_GATES

    def __repr__(self):
        return f"GlobalFoldingAmplifier(sub_folding_option={self.sub_folding_option!r})"


def _within(counts: np.ndarray) -> np.ndarray:
    """0 .. counts[j] - 1 for every j, concatenated."""
    counts = np.asarray(counts, dtype=np.int64)
    starts = np.cumsum(counts) - counts
    return np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(starts, counts)


def _plan(amplifier: _Amplifier, gate_ptr: np.ndarray, mask: np.ndarray, noise_factor: float):
    """The fold rule on a batch of gate lists (circuit c owns gates gate_ptr[c] .. gate_ptr[c + 1], ``mask`` marks the foldable
    ones).  Returns ``(unit_gate, unit_dagger, slot, achieved)``: the fold units of all circuits in running order (a flat gate index
    and whether it runs as its inverse), the gate after which a unit is placed when the circuit is written out, and the achieved
    factor per circuit.  numpy throughout; Python touches a circuit only for a ``random`` choice."""
    lam = float(noise_factor)
    if not math.isfinite(lam) or lam < 1.0:
        raise ValueError(f"noise factor {noise_factor!r}: want a finite number >= 1")
    gate_ptr = np.asarray(gate_ptr, dtype=np.int64)
    per = np.diff(gate_ptr)
    n_circ, n_gates = per.shape[0], int(gate_ptr[-1])
    owner = np.repeat(np.arange(n_circ, dtype=np.int64), per)
    mask = np.asarray(mask, dtype=bool)
    big_n = np.bincount(owner, weights=mask, minlength=n_circ).astype(np.int64)
    m = np.floor(big_n * (lam - 1.0) / 2.0 + 0.5).astype(np.int64)
    safe = np.maximum(big_n, 1)
    k, s = m // safe, m % safe
    achieved = np.where(big_n > 0, 1.0 + 2.0 * m / safe, 1.0)
    if amplifier.kind == "local":
        before = np.cumsum(mask) - mask                       # foldable gates before this one, over the whole batch
        first = np.concatenate([[0], np.cumsum(big_n)[:-1]]) if n_circ else np.zeros(0, dtype=np.int64)
        rank = before - first[owner]                          # position inside G
        if amplifier.sub_folding_option == "from_first":
            extra = rank < s[owner]
        elif amplifier.sub_folding_option == "from_last":
            extra = rank >= (big_n - s)[owner]
        else:
            extra = np.zeros(n_gates, dtype=bool)
            where = np.flatnonzero(mask)
            for c in np.flatnonzero(s > 0):
                extra[where[first[c] + amplifier._extra(int(big_n[c]), int(s[c]))]] = True
        folds = np.where(mask, k[owner] + extra, 0)
        reps = 1 + 2 * folds
        unit_gate = np.repeat(np.arange(n_gates, dtype=np.int64), reps)
        unit_dagger = _within(reps) & 1
        return unit_gate, unit_dagger, unit_gate, achieved
    # global: big_n = per (every gate is foldable)
    body = per * (1 + 2 * k)
    total = body + 2 * s
    j = _within(total)
    own = np.repeat(np.arange(n_circ, dtype=np.int64), total)
    n_o, s_o, body_o = np.maximum(per[own], 1), s[own], body[own]
    p, i = j // n_o, j % n_o
    pos = np.where(p & 1, n_o - 1 - i, i)
    dag = p & 1
    tail = j - body_o
    lo = (per - s)[own] if amplifier.sub_folding_option == "from_last" else np.zeros_like(own)
    in_tail, inverse = tail >= 0, tail < s_o
    pos = np.where(in_tail, np.where(inverse, lo + s_o - 1 - tail, lo + tail - s_o), pos)
    dag = np.where(in_tail, inverse.astype(np.int64), dag)
    unit_gate = gate_ptr[own] + pos
    slot = np.where(j < per[own], unit_gate, gate_ptr[own] + per[own] - 1)   # the extra passes go after the last gate
    return unit_gate, dag, slot, achieved


_SELF_INVERSE = {"id", "x", "y", "z", "h", "cx", "cz", "swap", "ecr"}
_PAIRS = {"s": "sdg", "sdg": "s", "t": "tdg", "tdg": "t", "sx": "sxdg", "sxdg": "sx"}
_NEGATED = {"rx", "ry", "rz", "p", "u1", "rzz"}


def inverse_op(op: CircuitOp) -> CircuitOp:
    """The inverse of a gate, by name: self-inverse gates; s/sdg, t/tdg, sx/sxdg; a negated angle for rx ry rz p u1 rzz;
    u3(a, b, c)^-1 = u3(-a, -c, -b); u2(b, c) = u3(pi / 2, b, c)."""
    name, p = op.name, tuple(float(v) for v in op.params)
    if name in _SELF_INVERSE:
        return CircuitOp(name, op.qubits, op.clbits, p)
    if name in _PAIRS:
        return CircuitOp(_PAIRS[name], op.qubits, op.clbits, p)
    if name in _NEGATED and len(p) == 1:
        return CircuitOp(name, op.qubits, op.clbits, (-p[0],))
    if name in ("u3", "u") and len(p) == 3:
        return CircuitOp(name, op.qubits, op.clbits, (-p[0], -p[2], -p[1]))
    if name == "u2" and len(p) == 2:
        return CircuitOp("u3", op.qubits, op.clbits, (-math.pi / 2, -p[1], -p[0]))
    raise ValueError(f"fold_circuit: no inverse is known for the gate {name!r} with {len(p)} parameters")


def fold_circuit(circuit: Any, noise_factor: float, amplifier: _Amplifier) -> Circuit:
    """The folded circuit as IR, for use outside the simulator (``circuit_to_qasm``, the graph encoder, another estimator) and as
    the written-out form of the fold rule.  Inverses are by name (:func:`inverse_op`); barriers and measures stay where they are;
    the extra passes of a global fold follow the circuit's last gate."""
    circ = Circuit.from_any(circuit)
    gates = [i for i, op in enumerate(circ.ops) if op.name not in _NOT_GATES]
    mask = np.asarray([amplifier.matches(circ.ops[i].name, len(circ.ops[i].qubits)) for i in gates], dtype=bool)
    unit_gate, unit_dagger, slot, _ = _plan(amplifier, np.asarray([0, len(gates)]), mask, noise_factor)
    placed: List[List[CircuitOp]] = [[] for _ in gates]
    for g, d, at in zip(unit_gate.tolist(), unit_dagger.tolist(), slot.tolist()):
        op = circ.ops[gates[g]]
        placed[at].append(inverse_op(op) if d else op)
    out, g = [], 0
    for op in circ.ops:
        if op.name in _NOT_GATES:
            out.append(op)
        else:
            out += placed[g]
            g += 1
    return Circuit(circ.num_qubits, circ.num_clbits, out, list(circ.qubit_reg_index))


# ---- schedules -------------------------------------------------------------------------------------------------------------------
@dataclass
class Schedules:
    """The schedules of ``mlqem_sim_run_folded_f64`` for F noise factors over a lowered batch of B circuits."""

    sched_ptr: np.ndarray     # int64 [F * B + 1]
    sched: np.ndarray         # int32 [n_sched]: (k << 1) | dagger, k relative to the circuit's first record
    ids: np.ndarray           # int32 [F * B]: run numbers f * B + c, the wave-per-circuit runs first
    n_wave: int
    n_wg: int
    noise_factors: Tuple[float, ...]
    achieved: np.ndarray      # float64 [F, B]: 1 + 2 m / N per run

    def to(self, device):
        return upload_fields(self, ("sched_ptr", "sched", "ids"), device)


def _name_table(amplifier: _Amplifier) -> np.ndarray:
    return np.asarray([amplifier.matches(g, 2 if g in _TWO_QUBIT else 1) for g in SUPPORTED_GATES], dtype=bool)


def _fold_entries(amplifier: _Amplifier, gate_ptr: np.ndarray, mask: np.ndarray, rec: np.ndarray, noi: np.ndarray, owner: np.ndarray,
                  n_circ: int, noise_factor: float, noi_len: Optional[np.ndarray] = None, pre: Optional[np.ndarray] = None,
                  post: Optional[np.ndarray] = None):
    """The fold units of one noise factor as schedule entries, shared by both record formats: ``(entries, body_len, achieved)``
    with the entries of all circuits in running order (a unit's gate record with its dagger flag, then its noise records, never
    inverted: one depolarising or fused noise record, after a coherent-error record where the model has one; absent records left
    out) and their number per circuit.  ``noi_len`` counts a gate's noise records (None: one where ``noi`` names one).  ``pre`` /
    ``post`` (the matrix-product-state format's twirl records; -1: none): a record per gate that every pass of the unit runs
    before its gate record and after its noise records, never inverted.  Without them the entries are what they always were."""
    unit_gate, unit_dagger, _, ach = _plan(amplifier, gate_ptr, mask, noise_factor)
    r, n = rec[unit_gate], noi[unit_gate]
    columns = [np.where(r >= 0, (r << 1) | unit_dagger, -1), np.where(n >= 0, n << 1, -1)]
    if noi_len is not None and noi_len.size and int(noi_len.max()) > 1:
        columns.append(np.where((n >= 0) & (noi_len[unit_gate] > 1), (n + 1) << 1, -1))
    if pre is not None:
        columns.insert(0, np.where(pre[unit_gate] >= 0, pre[unit_gate] << 1, -1))
    if post is not None:
        columns.append(np.where(post[unit_gate] >= 0, post[unit_gate] << 1, -1))
    entries = np.stack(columns, axis=1)
    valid = entries >= 0
    body_len = np.bincount(owner[unit_gate], weights=valid.sum(axis=1), minlength=n_circ).astype(np.int64)
    return entries[valid], body_len, ach


def build_schedules(batch: SimBatch, circuits: Optional[Sequence[Any]], noise_factors: Sequence[float], amplifier: _Amplifier) -> Schedules:
    """One schedule per (noise factor, circuit) from the record map ``compile_programs`` keeps (``batch.gate_*``).  A fold unit is
    the gate's record, possibly inverted, followed by its ``gate_noise_len`` noise records, never inverted (either may be absent):
    the inverse of a gate carries the gate's own coherent error and noise again, which is how an over-rotated ``cx`` behaves when
    it is folded.  The circuit's readout records follow every schedule once.  ``circuits`` are the lowered circuits (only their number is checked: the map has everything).  numpy
    throughout: no Python per entry."""
    batch.refuse_trajectories("build_schedules")
    if batch.gate_ptr is None:
        raise ValueError("build_schedules: the batch carries no record map (it was not made by compile_programs)")
    n_circ = len(batch)
    if circuits is not None and len(circuits) != n_circ:
        raise ValueError(f"build_schedules: {len(circuits)} circuits but a batch of {n_circ}")
    factors = tuple(float(f) for f in noise_factors)
    if not factors:
        raise ValueError("build_schedules: no noise factor")
    mask = _name_table(amplifier)[batch.gate_name.astype(np.int64)] if batch.gate_name.size else np.zeros(0, dtype=bool)
    owner = np.repeat(np.arange(n_circ, dtype=np.int64), np.diff(batch.gate_ptr))
    # the trailing records of a program run once, in order, after every schedule: its readout ops and, in a batch lowered for
    # measurement, the measurement tail (circ[:, 3] records: rotations / MEASURE / inverse rotations per group)
    n_readout = (np.minimum(batch.circ[:, 2].astype(np.int64) + batch.circ[:, 3].astype(np.int64), batch.op_counts)
                 if n_circ else np.zeros(0, dtype=np.int64))
    readout = ((np.repeat(batch.op_counts - n_readout, n_readout) + _within(n_readout)) << 1).astype(np.int32)
    rec, noi = batch.gate_record.astype(np.int64), batch.gate_noise.astype(np.int64)
    noi_len = None if batch.gate_noise_len is None else batch.gate_noise_len.astype(np.int64)
    if noi_len is not None and noi_len.size and (int(noi_len.min()) < 0 or int(noi_len.max()) > 2):
        raise ValueError(f"build_schedules: gate_noise_len holds {int(noi_len.min())} .. {int(noi_len.max())}, want 0, 1 or 2")
    pieces, lengths, achieved = [], [], []
    for lam in factors:
        body, body_len, ach = _fold_entries(amplifier, batch.gate_ptr, mask, rec, noi, owner, n_circ, lam, noi_len)
        run_len = body_len + n_readout
        start = np.cumsum(run_len) - run_len
        piece = np.empty(int(run_len.sum()), dtype=np.int32)
        piece[np.repeat(start, body_len) + _within(body_len)] = body
        piece[np.repeat(start + body_len, n_readout) + _within(n_readout)] = readout
        pieces.append(piece)
        lengths.append(run_len)
        achieved.append(ach)
    lengths = np.concatenate(lengths) if lengths else np.zeros(0, dtype=np.int64)
    sched_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if int(sched_ptr[-1]) > 2 ** 31 - 1 or len(factors) * n_circ > 2 ** 31 - 1:
        raise ValueError(f"build_schedules: {int(sched_ptr[-1])} schedule entries over {len(factors) * n_circ} runs exceed the "
                         "2^31 - 1 one call can take; split the batch")
    base = np.arange(len(factors), dtype=np.int64)[:, None] * n_circ
    wave = (base + batch.ids[:batch.n_wave].astype(np.int64)[None, :]).reshape(-1)
    wg = (base + batch.ids[batch.n_wave:batch.n_wave + batch.n_wg].astype(np.int64)[None, :]).reshape(-1)
    return Schedules(sched_ptr=sched_ptr, sched=np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.int32),
                     ids=np.concatenate([wave, wg]).astype(np.int32), n_wave=int(wave.size), n_wg=int(wg.size), noise_factors=factors,
                     achieved=np.asarray(achieved, dtype=np.float64).reshape(len(factors), n_circ))


def build_clifford_schedules(batch: CliffordBatch, noise_factors: Sequence[float], amplifier: _Amplifier, noise: Any = None) -> Schedules:
    """:func:`build_schedules` for the Clifford format (``mlqem_clifford_run_folded_f64``): one schedule per (noise factor, circuit)
    from the record map ``compile_clifford`` keeps.  A fold unit is the gate's record followed by its depolarising record (either
    may be absent; the inverse carries the gate's own depolarising record); there are no trailing entries, readout being no record
    in this format, and no run numbers (``ids`` is empty: every unit of the batch walks every factor).  numpy throughout.
    ``noise``: the model the batch was lowered under, if the caller has it; one with thermal relaxation or a coherent error is
    refused by name here too (``compile_clifford`` refuses it first: such a batch holds none of its records)."""
    refuse_non_pauli(noise, "build_clifford_schedules")
    if batch.gate_ptr is None:
        raise ValueError("build_clifford_schedules: the batch carries no record map (it was not made by compile_clifford)")
    n_circ = len(batch)
    factors = tuple(float(f) for f in noise_factors)
    if not factors:
        raise ValueError("build_clifford_schedules: no noise factor")
    mask = _name_table(amplifier)[batch.gate_name.astype(np.int64)] if batch.gate_name.size else np.zeros(0, dtype=bool)
    owner = np.repeat(np.arange(n_circ, dtype=np.int64), np.diff(batch.gate_ptr))
    rec, noi = batch.gate_record.astype(np.int64), batch.gate_noise.astype(np.int64)
    pieces, lengths, achieved = [], [], []
    for lam in factors:
        body, body_len, ach = _fold_entries(amplifier, batch.gate_ptr, mask, rec, noi, owner, n_circ, lam)
        pieces.append(body.astype(np.int32))
        lengths.append(body_len)
        achieved.append(ach)
    sched_ptr = np.concatenate([[0], np.cumsum(np.concatenate(lengths))]).astype(np.int64)
    if int(sched_ptr[-1]) > 2 ** 31 - 1 or len(factors) * max(n_circ, len(batch.units)) > 2 ** 31 - 1:
        raise ValueError(f"build_clifford_schedules: {int(sched_ptr[-1])} schedule entries over {len(factors) * n_circ} runs exceed "
                         "the 2^31 - 1 one call can take; split the batch")
    return Schedules(sched_ptr=sched_ptr, sched=np.concatenate(pieces), ids=np.zeros(0, dtype=np.int32), n_wave=0, n_wg=0,
                     noise_factors=factors, achieved=np.asarray(achieved, dtype=np.float64).reshape(len(factors), n_circ))


def build_mps_schedules(batch: Any, noise_factors: Sequence[float], amplifier: _Amplifier) -> Schedules:
    """:func:`build_schedules` for the matrix-product-state format (``mlqem_mps_run_folded_f64``): one schedule per (noise factor,
    circuit) from the record map the noisy lowering of ``compile_mps`` keeps.  A fold unit is the gate's ``U1`` / ``U2`` record,
    possibly daggered, followed by its ``gate_noise_len`` noise records, never daggered: a coherent-error ``U2`` where the model has
    one, then the ``DEPOL`` record (the inverse of a gate carries the gate's own coherent error and noise again).  In a batch
    lowered with ``pauli_twirl=`` a twirled gate's unit is ``TWIRL_OPEN``, gate | dagger, noise records, ``TWIRL_CLOSE``: every pass
    draws its own twirl (the gates that are twirled are self-inverse, so one table closes the gate and its dagger).  A batch that
    holds a thermal-relaxation record (``NOISE1`` / ``NOISE2``) is refused by name, here and in :func:`run_mps_folded`.  There are no
    trailing entries, readout being a table in this format, and no run numbers (``ids`` is empty: every (run, trajectory) unit is
    a workgroup).  numpy throughout."""
    if getattr(batch, "gate_ptr", None) is None:
        raise ValueError("build_mps_schedules: the batch carries no record map: the ideal lowering of compile_mps fuses gates into "
                         "bond records and has no fold units; ZNE on this path needs noise and trajectories "
                         "(compile_mps(circuits, observables, noise, trajectories=T))")
    from .mps import refuse_relaxation_records

    refuse_relaxation_records(batch, "build_mps_schedules")
    n_circ = len(batch)
    factors = tuple(float(f) for f in noise_factors)
    if not factors:
        raise ValueError("build_mps_schedules: no noise factor")
    mask = _name_table(amplifier)[batch.gate_name.astype(np.int64)] if batch.gate_name.size else np.zeros(0, dtype=bool)
    owner = np.repeat(np.arange(n_circ, dtype=np.int64), np.diff(batch.gate_ptr))
    rec, noi, noi_len = (getattr(batch, k).astype(np.int64) for k in ("gate_record", "gate_noise", "gate_noise_len"))
    if noi_len.size and (int(noi_len.min()) < 0 or int(noi_len.max()) > 2):
        raise ValueError(f"build_mps_schedules: gate_noise_len holds {int(noi_len.min())} .. {int(noi_len.max())}, want 0, 1 or 2")
    t_open, t_close = getattr(batch, "gate_twirl_open", None), getattr(batch, "gate_twirl_close", None)
    twirl = {} if t_open is None or t_close is None else dict(pre=t_open.astype(np.int64), post=t_close.astype(np.int64))
    pieces, lengths, achieved = [], [], []
    for lam in factors:
        body, body_len, ach = _fold_entries(amplifier, batch.gate_ptr, mask, rec, noi, owner, n_circ, lam, noi_len, **twirl)
        pieces.append(body.astype(np.int32))
        lengths.append(body_len)
        achieved.append(ach)
    sched_ptr = np.concatenate([[0], np.cumsum(np.concatenate(lengths))]).astype(np.int64)
    if int(sched_ptr[-1]) > 2 ** 31 - 1 or len(factors) * n_circ > 2 ** 31 - 1:
        raise ValueError(f"build_mps_schedules: {int(sched_ptr[-1])} schedule entries over {len(factors) * n_circ} runs exceed the "
                         "2^31 - 1 one call can take; split the batch")
    return Schedules(sched_ptr=sched_ptr, sched=np.concatenate(pieces), ids=np.zeros(0, dtype=np.int32), n_wave=0, n_wg=0,
                     noise_factors=factors, achieved=np.asarray(achieved, dtype=np.float64).reshape(len(factors), n_circ))


# ---- extrapolators ---------------------------------------------------------------------------------------------------------------
class PolynomialExtrapolator:
    """Least-squares polynomial of ``degree`` through (noise factor, value), evaluated at zero noise."""

    def __init__(self, degree: int):
        if int(degree) != degree or degree < 1:
            raise ValueError(f"PolynomialExtrapolator: degree {degree!r}, want an integer >= 1")
        self.degree = int(degree)

    def _degree_for(self, n_factors: int) -> int:
        return self.degree

    def weights(self, noise_factors: Sequence[float]) -> np.ndarray:
        """float64 [F] with ``sum_f w[f] y[f]`` = the fitted polynomial at 0: ``e_0^T V^+``, V the Vandermonde matrix."""
        x = np.asarray([float(f) for f in noise_factors], dtype=np.float64)
        if x.ndim != 1 or not np.isfinite(x).all():
            raise ValueError(f"noise factors {tuple(noise_factors)!r}: want finite numbers")
        if (x < 1.0).any():
            raise ValueError(f"noise factors {tuple(noise_factors)!r}: every factor must be >= 1")
        if np.unique(x).size != x.size:
            raise ValueError(f"noise factors {tuple(noise_factors)!r}: a factor is repeated")
        degree = self._degree_for(x.size)
        if x.size < degree + 1:
            raise ValueError(f"{type(self).__name__}: degree {degree} needs at least {degree + 1} noise factors, got {x.size}")
        v = np.vander(x, degree + 1, increasing=True)
        if x.size == degree + 1:   # interpolation: V^T w = e_0 (exact for (1, 3) -> (1.5, -0.5))
            e0 = np.zeros(degree + 1)
            e0[0] = 1.0
            return np.linalg.solve(v.T, e0)
        return np.linalg.pinv(v)[0].copy()

    def extrapolate(self, noise_factors: Sequence[float], values) -> np.ndarray:
        """The weights applied along the first axis of ``values`` [F, ...], added in factor order."""
        w, y = self.weights(noise_factors), np.asarray(values, dtype=np.float64)
        if y.shape[0] != w.shape[0]:
            raise ValueError(f"extrapolate: {y.shape[0]} rows of values for {w.shape[0]} noise factors")
        out = w[0] * y[0]
        for f in range(1, w.shape[0]):
            out = out + w[f] * y[f]
        return out

    def __repr__(self):
        return f"{type(self).__name__}()" if type(self) is not PolynomialExtrapolator else f"PolynomialExtrapolator({self.degree})"


class LinearExtrapolator(PolynomialExtrapolator):
    def __init__(self):
        super().__init__(1)


class QuadraticExtrapolator(PolynomialExtrapolator):
    def __init__(self):
        super().__init__(2)


class CubicExtrapolator(PolynomialExtrapolator):
    def __init__(self):
        super().__init__(3)


class QuarticExtrapolator(PolynomialExtrapolator):
    def __init__(self):
        super().__init__(4)


class RichardsonExtrapolator(PolynomialExtrapolator):
    """The interpolating polynomial through all F factors: degree F - 1."""

    def __init__(self):
        self.degree = 0

    def _degree_for(self, n_factors):
        if n_factors < 2:
            raise ValueError(f"RichardsonExtrapolator: needs at least 2 noise factors, got {n_factors}")
        return n_factors - 1


class ExponentialExtrapolator:
    """A straight line through (noise factor, ln|value|) per Pauli term, exponentiated at zero noise.  With w the degree-1
    least-squares weights: all v_f nonzero with one sign -> ``sign * exp(sum_f w_f ln|v_f|)``; all v_f = 0 -> 0; anything else (a zero
    among nonzeros, mixed signs: the model does not hold) -> the linear ``sum_f w_f v_f``, counted as a fallback.  Needs at least two
    distinct factors.  The fused paths extrapolate per TERM on the device (``ops.zne_combine_exp``) and add ``coeff * term`` in term
    order; the generic ``zne(cls)`` path has only the values and extrapolates those (:meth:`extrapolate`)."""

    exponential = True

    def weights(self, noise_factors: Sequence[float]) -> np.ndarray:
        """The straight-line weights ``PolynomialExtrapolator(1).weights(noise_factors)`` (they refuse fewer than two factors, a
        repeated factor and a factor below 1)."""
        return PolynomialExtrapolator(1).weights(noise_factors)

    def fit(self, noise_factors: Sequence[float], values) -> Tuple[np.ndarray, np.ndarray]:
        """``(mitigated, fallback)`` along the first axis of ``values`` [F, ...]: float64 and bool arrays of the remaining shape.
        Sums are formed in factor order."""
        w, y = self.weights(noise_factors), np.asarray(values, dtype=np.float64)
        if y.shape[0] != w.shape[0]:
            raise ValueError(f"extrapolate: {y.shape[0]} rows of values for {w.shape[0]} noise factors")
        pos, neg, zero = (y > 0).all(axis=0), (y < 0).all(axis=0), (y == 0).all(axis=0)
        model = pos | neg
        with np.errstate(divide="ignore", invalid="ignore"):
            logs = np.log(np.abs(np.where(model, y, 1.0)))
        s, lin = w[0] * logs[0], w[0] * y[0]
        for f in range(1, w.shape[0]):
            s, lin = s + w[f] * logs[f], lin + w[f] * y[f]
        out = np.where(model, np.where(neg, -1.0, 1.0) * np.exp(s), np.where(zero, 0.0, lin))
        return out, ~(model | zero)

    def extrapolate(self, noise_factors: Sequence[float], values) -> np.ndarray:
        return self.fit(noise_factors, values)[0]

    def extrapolate_terms(self, noise_factors: Sequence[float], term_values, term_ptr, coeff):
        """The host form of ``ops.zne_combine_exp``: ``(mitigated_values [B], mitigated_terms [n_terms], fallback [n_terms])`` from
        ``term_values`` [F, n_terms]; the value of a circuit is ``sum coeff * term`` in term order."""
        terms, fallback = self.fit(noise_factors, term_values)
        term_ptr, coeff = np.asarray(term_ptr, dtype=np.int64), np.asarray(coeff, dtype=np.float64)
        values = np.zeros(len(term_ptr) - 1, dtype=np.float64)
        for c in range(len(values)):
            total = np.float64(0.0)
            for t in range(int(term_ptr[c]), int(term_ptr[c + 1])):
                total = total + coeff[t] * terms[t]
            values[c] = total
        return values, terms, fallback.astype(np.int32)

    def __repr__(self):
        return "ExponentialExtrapolator()"


@dataclass
class ZNEStrategy:
    """What the reference's tutorial uses by default: factors (1, 3), two-qubit local folding, a straight line."""

    noise_factors: Tuple[float, ...] = (1, 3)
    noise_amplifier: Any = field(default_factory=lambda: LocalFoldingAmplifier(gates_to_fold=2))
    extrapolator: Any = field(default_factory=LinearExtrapolator)

    def __post_init__(self):
        self.noise_factors = tuple(self.noise_factors)
        self.weights()   # refuses bad factors at construction

    def weights(self) -> np.ndarray:
        return self.extrapolator.weights(self.noise_factors)


# ---- the fused path --------------------------------------------------------------------------------------------------------------
@dataclass
class ZNERun:
    """Everything one fused ZNE call produced (tensors on the device) and what the host knew."""

    mitigated_values: Any     # float64 [B]
    mitigated_terms: Any      # float64 [n_terms]
    term_ptr: Any             # int64 [B + 1]
    values: Any               # float64 [F, B]: per noise factor
    term_values: Any          # float64 [F, n_terms]
    norm: Any                 # float64 [F, B]; None on the Clifford path (a Pauli walk has no state to normalise)
    batch: Any                # the SimBatch, or the CliffordBatch on the Clifford path
    schedules: Schedules
    weights: np.ndarray
    # with shots: ``values`` / ``term_values`` and the mitigated ones above are the SAMPLED ones, and
    shots: Optional[int] = None
    variance: Any = None              # float64 [F, B]: per factor, sum coeff^2 (1 - estimate^2)
    mitigated_variance: Any = None    # float64 [B]: sum_f w_f^2 variance_f
    counts: Any = None                # int32 [F, n_outcomes]
    probs: Any = None                 # float64 [F, n_outcomes]
    exact_values: Any = None          # float64 [F, B]: the exact per-factor values of the same launch
    # on the Clifford path the walk gives the ideal values too (equal across factors: folding is the identity without noise)
    ideal_values: Any = None          # float64 [B]
    ideal_terms: Any = None           # float64 [n_terms]
    # with ExponentialExtrapolator: int32 [n_terms], 1 where a term fell back to the straight line
    fallback_terms: Any = None
    # on the MPS path (``method="mps"``): every value is a mean over ``trajectories`` Pauli-insertion trajectories per run, ``batch``
    # is the ``MpsBatch`` and ``norm`` [F, B] the mean <psi|psi>
    std_error: Any = None             # float64 [F, B]: the standard error of ``values``
    term_std_error: Any = None        # float64 [F, n_terms]
    mitigated_std_error: Any = None   # float64 [B]: sqrt(sum_f w_f^2 std_error_f^2); None with ExponentialExtrapolator
    error_bound: Any = None           # float64 [F, B]: the truncation certificate of every run (mean over its trajectories)
    discarded: Any = None             # float64 [F, B]
    bond: Any = None                  # int32 [F, B]: the largest bond a run reached
    trajectories: Optional[int] = None
    traj_term_values: Any = None      # float64 [T, F * n_terms] with ``keep_trajectories``
    traj_stats: Any = None            # float64 [T, F * B, 6] with it: MpsResult.traj_stats per run


def _combine(strategy: "ZNEStrategy", weights: np.ndarray, term_values, term_ptr, coeff):
    """``(mitigated_values, mitigated_terms, fallback or None)`` by the strategy's extrapolator, in one launch."""
    from ..native import ops

    w = upload(weights, term_values.device)
    if getattr(strategy.extrapolator, "exponential", False):
        return ops.zne_combine_exp(term_values, w, term_ptr, coeff)
    return ops.zne_combine(term_values, w, term_ptr, coeff) + (None,)


def _combine_squared(weights: np.ndarray, per_factor):
    """``sum_f w_f^2 x_f`` per circuit for ``per_factor`` [F, B] (variances of independently sampled factors, squared standard
    errors): the same combine with the squared weights on one unit-coefficient "term" per circuit."""
    import torch

    from ..native import ops

    b, dev = int(per_factor.shape[1]), per_factor.device
    return ops.zne_combine(per_factor, upload(weights * weights, dev), torch.arange(b + 1, dtype=torch.int64, device=dev),
                           torch.ones(b, dtype=torch.float64, device=dev))[1]


def tile_mps_runs(batch: Any, n_factors: int) -> dict:
    """The terms side of an ``MpsBatch`` for its F * B folded runs taken as a batch of F * B circuits (what ``mlqem_mps_terms_f64`` and
    ``mlqem_mps_finish_f64`` are given): ``run_qubits`` [F * B], ``term_circ`` [F * n_terms] (run numbers), ``term_off``
    [F * n_terms], ``site_ptr`` [F * B + 1], ``term_ptr`` [F * B + 1] and ``coeff`` [F * n_terms] as host arrays.  ``letters`` and
    ``readout`` are not tiled: every factor's offsets point into the batch's own."""
    f, b, n_terms = int(n_factors), len(batch), int(batch.term_circ.shape[0])
    rows = np.arange(f, dtype=np.int64)[:, None]
    return {"run_qubits": np.tile(batch.n_qubits, f).astype(np.int32),
            "term_circ": (batch.term_circ.astype(np.int64)[None, :] + rows * b).reshape(-1).astype(np.int32),
            "term_off": np.tile(batch.term_off, f).astype(np.int64),
            "site_ptr": np.concatenate([np.tile(batch.site_ptr[:-1], f), batch.site_ptr[-1:]]).astype(np.int64),
            "term_ptr": np.concatenate([(batch.term_ptr[None, :-1] + rows * n_terms).reshape(-1), [f * n_terms]]).astype(np.int64),
            "coeff": np.tile(batch.coeff, f).astype(np.float64)}


def run_mps_folded(batch: Any, schedules: Schedules, seed: int = 0, run_keys=None, device="cuda", keep_trajectories: bool = False,
                   buffer_bytes: Optional[int] = None):
    """Runs the F * B folded runs of a batch lowered once by ``compile_mps`` (with noise and trajectories) along ``schedules``
    (:func:`build_mps_schedules`) on the device.  Returns an :class:`~blackwater.sim.mps.MpsResult` over the runs taken as a batch of
    F * B circuits, run r = f * B + c: ``values`` / ``norm`` / ``std_error`` / ``discarded`` / ``error_bound`` / ``bond`` [F * B],
    ``term_values`` / ``term_std_error`` [F * n_terms], ``term_ptr`` [F * B + 1] (tiled), ``batch`` the unreplicated batch.
    ``run_keys``: one integer per run, by default the run number; a unit's bits depend on (seed, run key, trajectory number, the
    run's schedule and records) alone.  The (run, trajectory) units are split into launches so that the site-tensor workspace stays
    under ``buffer_bytes`` (default :data:`~blackwater.sim.mps.MPS_BUFFER_BYTES`), as :func:`~blackwater.sim.mps.run_mps` splits."""
    import torch

    from ..native import ops
    from .mps import _mps_plan, _mps_result, refuse_relaxation_records

    refuse_relaxation_records(batch, "run_mps_folded")
    if batch.trajectories is None:
        raise ValueError("run_mps_folded: the batch was lowered without trajectories; ZNE on this path needs noise and trajectories "
                         "(compile_mps(circuits, observables, noise, trajectories=T))")
    n_traj, seed = check_trajectories(batch.trajectories, "run_mps_folded"), check_seed(seed, "run_mps_folded")
    n_f, b, n_terms = len(schedules.noise_factors), len(batch), int(batch.term_circ.shape[0])
    n_runs = n_f * b
    if schedules.sched_ptr.shape[0] != n_runs + 1:
        raise ValueError(f"run_mps_folded: the schedules hold {schedules.sched_ptr.shape[0] - 1} runs, the batch has {n_f} factors x {b} "
                         "circuits")
    keys = _run_keys(run_keys, n_runs, "run_mps_folded")
    dev = torch.device(device)
    tiled = tile_mps_runs(batch, n_f)
    chunks, workspace, _ = _mps_plan(tiled["run_qubits"], batch.max_bond, n_traj, buffer_bytes, "run_mps_folded", dev)
    t, s = batch.to(dev), schedules.to(dev)
    r = {k: upload(v, dev) for k, v in tiled.items()}
    keys_t = upload(keys, dev)
    traj_terms = torch.zeros((n_traj, n_f * n_terms), dtype=torch.float64, device=dev)
    traj_norm = torch.zeros((n_traj, n_runs), dtype=torch.float64, device=dev)
    traj_stats = torch.zeros((n_traj, n_runs, ops.MPS_STATS), dtype=torch.float64, device=dev)
    for rr, tr, w in chunks:
        t0, t1 = int(tiled["term_ptr"][rr.start]), int(tiled["term_ptr"][rr.stop])
        ops.sim_run_mps_folded(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], s["sched_ptr"], s["sched"], n_f, keys_t,
                               r["run_qubits"], r["term_circ"], r["term_off"], t["letters"], r["site_ptr"], t["readout"],
                               (rr.start, len(rr)), (t0, t1 - t0), (tr.start, len(tr)), n_traj, seed, batch.max_bond, batch.cutoff, w,
                               workspace, traj_terms, traj_norm, traj_stats)
    out = ops.sim_mps_finish(r["term_ptr"], r["coeff"], traj_terms, traj_norm, traj_stats)
    return _mps_result(out, r["term_ptr"], batch, seed, traj_terms, traj_stats, keep_trajectories, True)


def _zne_run_mps(circuits, observables, noise, strategy, weights, device, shots, seed, run_keys, trajectories, max_bond, cutoff,
                 buffer_bytes, keep_trajectories, pauli_twirl=None) -> ZNERun:
    from .mps import DEFAULT_CUTOFF, MAX_BOND, compile_mps

    if shots is not None:
        raise ValueError("zne_run(method='mps'): shots= is not supported with it (no shots are drawn from folded matrix-product-state "
                         "runs; the sampled values of an unfolded circuit are DeviceEstimator(method='mps_shots') / "
                         "sample_mps_expectation_values)")
    if noise is None or trajectories is None:
        raise ValueError("zne_run(method='mps'): ZNE on the matrix-product-state path needs noise and trajectories (a noise model and "
                         "trajectories=T: the noisy lowering keeps the gate records that are folded; the ideal one fuses them)")
    n_traj = check_trajectories(trajectories, "zne_run")
    batch = compile_mps(circuits, observables, noise, n_traj, MAX_BOND if max_bond is None else max_bond,
                        DEFAULT_CUTOFF if cutoff is None else cutoff, pauli_twirl=pauli_twirl)
    sch = build_mps_schedules(batch, strategy.noise_factors, strategy.noise_amplifier)
    n_f, b, n_terms = len(sch.noise_factors), len(batch), int(batch.term_circ.shape[0])
    res = run_mps_folded(batch, sch, seed, run_keys, device, keep_trajectories, buffer_bytes)
    term_ptr, coeff = upload(batch.term_ptr, res.values.device), upload(batch.coeff, res.values.device)
    term_values = res.term_values.reshape(n_f, n_terms)
    mitigated_values, mitigated_terms, fallback = _combine(strategy, weights, term_values, term_ptr, coeff)
    std_error = res.std_error.reshape(n_f, b)
    mitigated_std_error = None   # sqrt(sum_f w_f^2 se_f^2), for the polynomial extrapolators
    if not getattr(strategy.extrapolator, "exponential", False):
        mitigated_std_error = _combine_squared(weights, (std_error * std_error).contiguous()).sqrt()
    return ZNERun(mitigated_values, mitigated_terms, term_ptr, res.values.reshape(n_f, b), term_values, res.norm.reshape(n_f, b), batch,
                  sch, weights, fallback_terms=fallback, std_error=std_error, term_std_error=res.term_std_error.reshape(n_f, n_terms),
                  mitigated_std_error=mitigated_std_error, error_bound=res.error_bound.reshape(n_f, b),
                  discarded=res.discarded.reshape(n_f, b), bond=res.bond.reshape(n_f, b), trajectories=n_traj,
                  traj_term_values=res.traj_term_values, traj_stats=res.traj_stats)


def zne_run(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
            strategy: Optional[ZNEStrategy] = None, device="cuda", shots: Optional[int] = None, seed: int = 0, run_keys=None,
            method: str = "exact", trajectories: Optional[int] = None, max_bond: Optional[int] = None, cutoff: Optional[float] = None,
            buffer_bytes: Optional[int] = None, keep_trajectories: bool = False, pauli_twirl: Any = None) -> ZNERun:
    """Lowers once, builds the schedules, simulates every (circuit, factor) run in one call and extrapolates in one more.  With
    ``shots`` every run is also measured and the extrapolation is of the sampled values (see the module docstring); ``run_keys``:
    one integer per run f * B + c (by default the run number).  ``method``: ``"exact"`` (the default), ``"clifford"`` or ``"auto"``,
    with :class:`DeviceEstimator`'s meaning and ``auto`` rule; on the Clifford path ``batch`` is the ``CliffordBatch``, ``norm`` is
    None, ``ideal_values`` / ``ideal_terms`` come from the same call, and ``shots`` is refused.

    ``method="mps"`` (by name alone; ``auto`` never picks it) folds wide circuits at any angle on matrix-product states: needs
    ``noise`` and ``trajectories=T``; ``max_bond`` / ``cutoff`` / ``buffer_bytes`` as in :func:`~blackwater.sim.mps.run_mps`.  One
    lowering, :func:`build_mps_schedules`, then every (run, trajectory) unit through ``ops.sim_run_mps_folded`` in chunks that keep
    the site-tensor workspace under ``buffer_bytes``, one finish over the F * B runs and the combine.  The per-factor values are
    means over the trajectories; :class:`ZNERun` carries their standard errors, the truncation certificates and the bonds.  A
    model with thermal relaxation is refused by name (folded runs do not take the ``thermal_relaxation=True`` of ``compile_mps``).
    ``pauli_twirl`` (``method="mps"`` alone) is ``compile_mps``'s: every pass of a folded gate draws its own twirl on the device, which
    turns a coherent gate error into the Pauli channel the extrapolators assume."""
    from ..native import ops

    strategy = strategy or ZNEStrategy()
    weights = strategy.weights()
    circuits = list(circuits)
    exponential = getattr(strategy.extrapolator, "exponential", False)
    if shots is not None and exponential:
        raise ValueError("ExponentialExtrapolator: shots= is not supported with it (the variance of a sampled value is not "
                         "propagated through the exponential fit); use a polynomial extrapolator or run without shots")
    if method == "trajectories":
        raise ValueError("zne_run: method = 'trajectories': folded / ZNE runs over quantum trajectories are not supported; "
                         "want one of exact, clifford, auto, mps")
    if method == "mps":
        return _zne_run_mps(circuits, observables, noise, strategy, weights, device, shots, seed, run_keys, trajectories, max_bond, cutoff,
                            buffer_bytes, keep_trajectories, pauli_twirl)
    if pauli_twirl is not None and pauli_twirl is not False:
        raise ValueError(f"zne_run: pauli_twirl= belongs to method='mps' (the twirl is drawn per trajectory on the matrix-product-state "
                         f"path), not to method = {method!r}")
    if trajectories is not None or max_bond is not None or cutoff is not None or buffer_bytes is not None or keep_trajectories:
        raise ValueError(f"zne_run: trajectories=, max_bond=, cutoff=, buffer_bytes= and keep_trajectories= belong to method='mps', "
                         f"not to method = {method!r}")
    if method not in DeviceEstimator.METHODS:
        raise ValueError(f"zne_run: method = {method!r}, want one of {', '.join(DeviceEstimator.METHODS + ('mps',))}")
    clifford = method != "exact" and use_clifford_path(method, noise, circuits)
    if clifford:
        if shots is not None:
            raise ValueError(_CLIFFORD_SHOTS)
        batch = compile_clifford(circuits, observables, noise)
        sch = build_clifford_schedules(batch, strategy.noise_factors, strategy.noise_amplifier, noise)
    else:
        if shots is not None:
            shots, seed = check_shots(shots, "zne_run"), check_seed(seed, "zne_run")
        batch = compile_programs(circuits, observables, noise, shots=shots)
        sch = build_schedules(batch, circuits, strategy.noise_factors, strategy.noise_amplifier)
    t, s = batch.to(device), sch.to(device)
    n_f, extra = len(sch.noise_factors), {}
    if clifford:
        ideal_values, noisy_values, ideal_terms, noisy_terms, _, _ = ops.clifford_run_folded(
            t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"], t["term_ptr"], t["coeff"],
            t["comb_ptr"], t["comb_unit"], t["comb_weight"], s["sched_ptr"], s["sched"], n_f)
        values, term_values = (ideal_values, ideal_terms) if noise is None else (noisy_values, noisy_terms)
        norm, extra = None, dict(ideal_values=ideal_values[0], ideal_terms=ideal_terms[0])
    elif shots is not None:
        keys = upload(_run_keys(run_keys, n_f * len(batch), "zne_run"), device)
        units, u_wave, u_wg = batch.sample_units(n_f)
        exact, _, norm, probs = ops.sim_run_folded_measured(
            t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["prob_ptr"],
            int(batch.prob_ptr[-1]), s["sched_ptr"], s["sched"], s["ids"], sch.n_wave, sch.n_wg, n_f)
        values, variance, term_values, counts = ops.sim_sample(
            t["circ"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["term_group"], t["prob_ptr"], t["group_circ"], probs,
            keys, shots, seed, upload(units, keys.device), u_wave, u_wg)
        extra = dict(shots=shots, variance=variance, counts=counts, probs=probs, exact_values=exact)
    else:
        values, term_values, norm = ops.sim_run_folded(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"],
                                                       s["sched_ptr"], s["sched"], s["ids"], sch.n_wave, sch.n_wg, n_f)
    mitigated_values, mitigated_terms, fallback = _combine(strategy, weights, term_values, t["term_ptr"], t["coeff"])
    if shots is not None:   # the factors are sampled independently
        extra["mitigated_variance"] = _combine_squared(weights, variance)
    return ZNERun(mitigated_values, mitigated_terms, t["term_ptr"], values, term_values, norm, batch, sch, weights, fallback_terms=fallback,
                  **extra)


def zne_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                           strategy: Optional[ZNEStrategy] = None, device="cuda", shots: Optional[int] = None, seed: int = 0,
                           method: str = "exact"):
    """``(mitigated_values [B], mitigated_terms [n_terms], term_ptr [B + 1], per_factor_values [F, B])``, tensors on ``device``.
    ``noise=None`` is allowed (state vectors up to 11 qubits): pointless as mitigation, every factor then gives the same value up
    to rounding.  With ``shots`` the same four tensors hold the SAMPLED values; :func:`zne_run` returns the variances, counts and
    probabilities beside them (``ZNERun.mitigated_variance``, ``.variance``, ``.counts``, ``.probs``).  ``method`` as in
    :func:`zne_run`: ``"clifford"`` / ``"auto"`` extrapolate Clifford circuits of up to 512 qubits."""
    run = zne_run(circuits, observables, noise, strategy, device, shots=shots, seed=seed, method=method)
    return run.mitigated_values, run.mitigated_terms, run.term_ptr, run.values


# ---- the decorator ---------------------------------------------------------------------------------------------------------------
def _zne_metadata(strategy: ZNEStrategy, achieved: np.ndarray, per_factor: np.ndarray, k: int) -> dict:
    return {"noise_factors": tuple(float(f) for f in strategy.noise_factors), "achieved_factors": tuple(float(a) for a in achieved[:, k]),
            "values": tuple(float(v) for v in per_factor[:, k]), "noise_amplifier": repr(strategy.noise_amplifier),
            "extrapolator": repr(strategy.extrapolator)}


def _fused_rows(strategy: ZNEStrategy, run: ZNERun, n: int) -> List[Tuple[dict, dict]]:
    """Per circuit, what a fused run puts into ``metadata[k]`` and into ``metadata[k]["zne"]`` (``zne(cls)`` has the keys)."""
    values = run.values.cpu().numpy()
    rows = [({}, _zne_metadata(strategy, run.schedules.achieved, values, k)) for k in range(n)]
    if run.fallback_terms is not None:   # with ExponentialExtrapolator: the terms that fell back
        ptr, flags = run.term_ptr.cpu().numpy(), run.fallback_terms.cpu().numpy()
        for k, (_, z) in enumerate(rows):
            z["fallback_terms"] = int(flags[ptr[k]:ptr[k + 1]].sum())
    if run.trajectories is not None:   # the MPS path
        se, bound = run.std_error.cpu().numpy(), run.error_bound.cpu().numpy()
        mse = None if run.mitigated_std_error is None else run.mitigated_std_error.cpu().numpy()
        for k, (m, z) in enumerate(rows):
            m["trajectories"] = run.trajectories
            if mse is not None:   # polynomial: |mitigated - exact ZNE| <= 2 * truncation_error_bound * sum|coeff|
                m.update(std_error=float(mse[k]), truncation_error_bound=float(np.abs(run.weights) @ bound[:, k]))
            z.update(std_errors=tuple(float(v) for v in se[:, k]), truncation_error_bounds=tuple(float(v) for v in bound[:, k]))
    if run.shots is not None:   # the error bar of the mitigated value
        variance, per_factor = run.mitigated_variance.cpu().numpy(), run.variance.cpu().numpy()
        for k, (m, z) in enumerate(rows):
            var = float(variance[k])
            m.update(variance=var, shots=int(run.shots), std_error=math.sqrt(max(var, 0.0) / run.shots))
            z["variances"] = tuple(float(v) for v in per_factor[:, k])
    return rows


class ZNEJob:
    """The job of a ``zne(cls)`` run.  The fused path has its values and its metadata ``rows`` (per circuit: a dict merged into
    ``metadata[k]`` and the finished ``metadata[k]["zne"]``) when it is built; the generic path combines the F * B values of the
    wrapped estimator's job when ``result()`` is asked for."""

    def __init__(self, strategy: ZNEStrategy, achieved: np.ndarray, n_circuits: int, job_id: str, values=None, rows=None, base_job=None):
        self._strategy, self._achieved, self._n, self._job_id = strategy, achieved, n_circuits, job_id
        self._values, self._rows, self._base_job = values, rows, base_job

    def result(self):
        meta = [{} for _ in range(self._n)]
        if self._values is None:
            base = self._base_job.result()
            per_factor = np.asarray(base.values, dtype=np.float64).reshape(len(self._strategy.noise_factors), self._n)
            self._values = np.asarray(self._strategy.extrapolator.extrapolate(self._strategy.noise_factors, per_factor))
            self._rows = [({}, _zne_metadata(self._strategy, self._achieved, per_factor, k)) for k in range(self._n)]
            meta = [dict(m) for m in list(base.metadata)[:self._n]] if len(base.metadata) >= self._n else meta
        for m, (row, zne_row) in zip(meta, self._rows):
            m["zne"] = dict(zne_row)
            m.update(row)
        return make_estimator_result(np.asarray(self._values, dtype=np.float64), meta)

    def job_id(self) -> str:
        return self._job_id

    def status(self):
        return "DONE" if self._base_job is None else self._base_job.status()

    def submit(self):
        return None if self._base_job is None else self._base_job.submit()

    def cancel(self):
        return False if self._base_job is None else self._base_job.cancel()


def zne(cls):
    """Decorator in the style of ``learning(...)`` / ``ngem(...)``: ``zne(Estimator)`` is an estimator class that accepts
    ``zne_strategy=`` at construction and as a run option and returns zero-noise-extrapolated values;
    ``result().metadata[k]["zne"]`` holds the requested and achieved factors and the per-factor values.  Around
    :class:`DeviceEstimator`, ``shots=`` (constructor or run option) measures every run: ``metadata[k]`` gains ``variance``
    (sum_f w_f^2 variance_f), ``shots`` and ``std_error = sqrt(variance / shots)``, and ``metadata[k]["zne"]["variances"]`` the
    per-factor variances.

    Around :class:`DeviceEstimator` it takes the fused path (:func:`zne_run`: one lowering, schedules, two calls) and follows the
    estimator's ``method``: ``"clifford"`` (or ``"auto"`` on a job over the exact simulator's cap) extrapolates Clifford circuits of
    up to 512 qubits, without shots; ``"mps"`` (with ``trajectories=``, ``max_bond=``, ``cutoff=``) folds circuits on a line at any
    angle on matrix-product states: for polynomial extrapolators ``metadata[k]`` gains ``std_error``, ``trajectories`` and
    ``truncation_error_bound`` = sum_f |w_f| B_f (|mitigated - exact ZNE| <= 2 * that * sum|coeff|), and ``metadata[k]["zne"]`` the
    per-factor ``std_errors`` and ``truncation_error_bounds``; with :class:`ExponentialExtrapolator` ``std_error`` and
    ``truncation_error_bound`` are omitted.  With :class:`ExponentialExtrapolator` on a fused path ``metadata[k]["zne"]["fallback_terms"]``
    counts the circuit's terms that fell back to the straight line.  Around any other
    estimator class it folds the IR (:func:`fold_circuit`), submits the F * B circuits through the wrapped ``_run`` in one job and
    combines with the same weights on the host; circuits must arrive bound there."""
    fused = isinstance(cls, type) and issubclass(cls, DeviceEstimator)

    def __init__(self, *args, zne_strategy: Optional[ZNEStrategy] = None, **kwargs):
        cls.__init__(self, *args, **kwargs)
        self._zne_strategy = zne_strategy or ZNEStrategy()
        self._zne_count = 0

    def _run(self, circuits, observables, parameter_values, **run_options):
        strategy = run_options.pop("zne_strategy", None) or self._zne_strategy
        circuits, observables, parameter_values = list(circuits), list(observables), list(parameter_values)
        if fused:
            for k, c in enumerate(circuits):
                if has_free_parameters(c):
                    raise ValueError(f"{type(self).__name__}: circuit {k} is a template with free parameters, which zne(DeviceEstimator) "
                                     "does not fold; bind it first (Template.bind_parameters(values)) and pass the bound circuit")
            for k, p in enumerate(parameter_values):
                if len(p):
                    raise ValueError(f"{type(self).__name__}: circuit {k} comes with {len(p)} parameter values; circuits must arrive bound")
            shots, seed = run_options.pop("shots", self._shots), run_options.pop("seed", self._seed)
            mps = {}
            if self._method == "mps":
                mps = dict(trajectories=None if self._noise is None else self._trajectories, max_bond=self._max_bond, cutoff=self._cutoff,
                           pauli_twirl=self._twirl)
            elif shots is not None and self._method != "exact" and self._use_clifford(circuits):
                raise ValueError(_CLIFFORD_SHOTS)
            # job j's run r draws with the key j * 2^32 + r, as on the shots path; a call that zne_run refuses is no job
            job, n = self._zne_count + 1, len(circuits)
            keys = np.arange(len(strategy.noise_factors) * n, dtype=np.int64) + (np.int64(job) << 32)
            run = zne_run(circuits, observables, self._noise, strategy, self._device, shots=shots, seed=seed, run_keys=keys,
                          method=self._method, **mps)
            self._zne_count = job
            return ZNEJob(strategy, run.schedules.achieved, n, f"zne-sim-{job}", values=run.mitigated_values.cpu().numpy(),
                          rows=_fused_rows(strategy, run, n))
        parsed = [Circuit.from_any(c) for c in circuits]
        folded, achieved = [], []
        for lam in strategy.noise_factors:
            folded += [fold_circuit(c, lam, strategy.noise_amplifier) for c in parsed]
            achieved.append([achieved_factor(sum(strategy.noise_amplifier.matches(op.name, len(op.qubits)) for op in c.ops), lam)
                             for c in parsed])
        n_f = len(strategy.noise_factors)
        base = cls._run(self, folded, observables * n_f, parameter_values * n_f, **run_options)
        self._zne_count += 1
        return ZNEJob(strategy, np.asarray(achieved, dtype=np.float64).reshape(n_f, len(parsed)), len(parsed),
                      f"zne-{self._zne_count}", base_job=base)

    return type(f"ZNE{cls.__name__}", (cls,), {"__init__": __init__, "_run": _run, "__doc__": cls.__doc__})
