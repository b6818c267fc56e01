"""Synthetic TFIM-Trotter circuit corpora for benchmarking (no qiskit, no simulator).

The circuit STRUCTURE is the reference's Trotterised transverse-field Ising layer
(docs/tutorials/h13_ising_data_gen.ipynb:247; 100-qubit variant h24_ising_data_gen_zne_hardware_100q.ipynb cell [4]):
``rx(2 h dt)`` on every qubit | barrier | ``cx-rz(-2 J dt)-cx`` on even bonds | barrier | same on odd bonds | barrier,
repeated ``steps`` times, then ``measure_all``.  It is lowered with one fixed rule per gate to the basis
{rz, sx, x, ecr|cx} so that op counts land near what the reference's transpiled circuits hold (100 qubits:
~2.0k ops and 198 two-qubit gates per step; measured there: 1,584 / 8,999 / 20,711 ops at 1 / 6 / 10 steps).
Labels are synthetic by default (they only feed the loss and the MAE plumbing); ``encode_corpus(simulate=...)`` fills them with
simulated values from ``blackwater.sim`` for circuits small enough to simulate exactly, and with ``clifford=True`` also for wider
Clifford circuits (``clifford_tfim_circuit``, ``random_clifford_circuit``: up to 512 qubits).
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np

from .backends import StaticBackend
from .circuit import Circuit, CircuitOp
from .utils import circuit_to_graph_data_json, get_backend_properties_v1


def tfim_circuit(nq: int, steps: int, J: float, h: float = 0.66 * math.pi, dt: float = 0.5,
                 two_q: str = "ecr") -> Circuit:
    return _tfim(nq, steps, 2 * h * dt, -2 * J * dt, two_q)


def clifford_tfim_circuit(nq: int, steps: int, kx: int, kz: int, two_q: str = "ecr") -> Circuit:
    """:func:`tfim_circuit` with the field rotation ``theta = kx pi / 2`` and the bond rotation ``phi = kz pi / 2`` (integers): every
    gate is then a Clifford gate, so ``blackwater.sim.clifford_expectation_values`` gives its exact ideal and noisy values at any
    width."""
    return _tfim(nq, steps, int(kx) * math.pi / 2, int(kz) * math.pi / 2, two_q)


def tfim_circuit_template(nq: int, steps: int, two_q: str = "cx"):
    """The op sequence of :func:`tfim_circuit` as a ``blackwater.sim.Template`` with TWO parameters on its two ``rz`` angles:
    theta[0] is the field rotation (``rz(theta[0] + pi)`` between the ``sx`` of every ``rx``), theta[1] the bond rotation.  The
    offsets are those of ``tfim_circuit``, so ``bind_parameters([2 h dt, -2 J dt]).ops == tfim_circuit(nq, steps, J, h, dt, two_q).ops``
    exactly.  Its two-qubit gates act on neighbours: the matrix-product-state path binds it at any width up to 512 qubits."""
    from ..sim.template import Param, Template

    return Template(nq, nq, _tfim_ops(nq, steps, Param(0), Param(1), two_q), [], 2)


def _tfim(nq: int, steps: int, theta: float, phi: float, two_q: str) -> Circuit:
    return Circuit(nq, nq, _tfim_ops(nq, steps, theta, phi, two_q))


def _tfim_ops(nq: int, steps: int, theta, phi, two_q: str) -> List[CircuitOp]:
    """``theta`` / ``phi``: floats, or ``Param``s (``theta + pi`` is then a ``Param`` with the offset pi)."""
    ops: List[CircuitOp] = []
    all_q = tuple(range(nq))

    def rx(q):
        ops.extend([CircuitOp("rz", (q,), (), (math.pi / 2,)), CircuitOp("sx", (q,)),
                    CircuitOp("rz", (q,), (), (theta + math.pi,)), CircuitOp("sx", (q,)),
                    CircuitOp("rz", (q,), (), (5 * math.pi / 2,))])

    def cx(a, b):
        if two_q == "cx":
            ops.append(CircuitOp("cx", (a, b)))
            return
        ops.extend([CircuitOp("rz", (a,), (), (-math.pi / 2,)), CircuitOp("rz", (b,), (), (-math.pi,)),
                    CircuitOp("sx", (b,)), CircuitOp("rz", (b,), (), (-math.pi,)), CircuitOp(two_q, (a, b)),
                    CircuitOp("x", (a,)), CircuitOp("sx", (b,))])

    def bonds(first_qubits):
        for q0 in first_qubits:
            cx(q0, q0 + 1)
        for q0 in first_qubits:
            ops.append(CircuitOp("rz", (q0 + 1,), (), (phi,)))
        for q0 in first_qubits:
            cx(q0, q0 + 1)

    for _ in range(steps):
        for q in all_q:
            rx(q)
        ops.append(CircuitOp("barrier", all_q))
        bonds(range(0, nq - 1, 2))
        ops.append(CircuitOp("barrier", all_q))
        bonds(range(1, nq - 2, 2))
        ops.append(CircuitOp("barrier", all_q))
    ops.append(CircuitOp("barrier", all_q))
    ops.extend(CircuitOp("measure", (q,), (q,)) for q in all_q)
    return ops


def two_local(num_qubits: int, rotation_blocks=("ry",), entanglement_blocks="cz", entanglement: str = "full", reps: int = 3):
    """qiskit's ``TwoLocal`` as a ``blackwater.sim.Template``: ``reps`` times a rotation layer and an entanglement layer, then a
    final rotation layer.  Parameters are numbered as ``TwoLocal`` numbers them: layer-major, within a layer block-major, then by
    qubit (an entanglement block with an angle, ``rzz``, by pair).  ``rotation_blocks``: names out of ``rx ry rz p``;
    ``entanglement_blocks``: ``cx cz swap ecr`` (fixed) or ``rzz``; ``entanglement``: ``"full"`` (every pair i < j, in that order),
    ``"linear"`` (i, i + 1) or a list of qubit pairs."""
    from ..sim.template import Param, Template

    rot = [rotation_blocks] if isinstance(rotation_blocks, str) else list(rotation_blocks)
    ent = [entanglement_blocks] if isinstance(entanglement_blocks, str) else list(entanglement_blocks)
    for name in rot:
        if name not in ("rx", "ry", "rz", "p"):
            raise ValueError(f"two_local: rotation block {name!r}, want one of rx ry rz p")
    for name in ent:
        if name not in ("cx", "cz", "swap", "ecr", "rzz"):
            raise ValueError(f"two_local: entanglement block {name!r}, want one of cx cz swap ecr rzz")
    if entanglement == "full":
        pairs = [(i, j) for i in range(num_qubits) for j in range(i + 1, num_qubits)]
    elif entanglement == "linear":
        pairs = [(i, i + 1) for i in range(num_qubits - 1)]
    elif isinstance(entanglement, (list, tuple)):   # explicit pairs, e.g. a device's coupling map
        pairs = [(int(a), int(b)) for a, b in entanglement]
    else:
        raise ValueError(f"two_local: entanglement = {entanglement!r}, want 'full', 'linear' or a list of qubit pairs")
    if num_qubits < 1 or reps < 0:
        raise ValueError(f"two_local: num_qubits = {num_qubits}, reps = {reps}, want at least 1 qubit and reps >= 0")
    ops: List[CircuitOp] = []
    count = 0

    def rotation_layer():
        nonlocal count
        for name in rot:
            for q in range(num_qubits):
                ops.append(CircuitOp(name, (q,), (), (Param(count),)))
                count += 1

    for _ in range(reps):
        rotation_layer()
        for name in ent:
            for a, b in pairs:
                if name == "rzz":
                    ops.append(CircuitOp(name, (a, b), (), (Param(count),)))
                    count += 1
                else:
                    ops.append(CircuitOp(name, (a, b)))
    rotation_layer()
    return Template(num_qubits, 0, ops, [], count)


def tfim_template(num_qubits: int, steps: int):
    """A Trotterised transverse-field Ising evolution as a ``blackwater.sim.Template`` with TWO parameters, each used by many gates:
    per step ``rzz(2 theta[0])`` on every bond (i, i + 1) (theta[0] = J dt) and ``rx(2 theta[1])`` on every qubit (theta[1] = h dt)."""
    from ..sim.template import Param, Template

    ops: List[CircuitOp] = []
    for _ in range(steps):
        for q in range(num_qubits - 1):
            ops.append(CircuitOp("rzz", (q, q + 1), (), (Param(0, 2.0),)))
        for q in range(num_qubits):
            ops.append(CircuitOp("rx", (q,), (), (Param(1, 2.0),)))
    return Template(num_qubits, 0, ops, [], 2)


def random_circuit(nq: int, depth: int, seed: int, two_q: str = "cx", measure: bool = True) -> Circuit:
    """Layers of random disjoint one- and two-qubit gates, like the reference's use of
    ``qiskit.circuit.random.random_circuit`` (blackwater/data/generators/exp_val.py:116-120), already in the backend
    basis {rz, sx, x, two_q}; two-qubit gates act on neighbours of a line so that calibration entries exist."""
    rng = np.random.default_rng(seed)
    ops: List[CircuitOp] = []
    for _ in range(depth):
        q = 0
        while q < nq:
            if q + 1 < nq and rng.random() < 0.35:
                a, b = (q, q + 1) if rng.random() < 0.5 else (q + 1, q)
                ops.append(CircuitOp(two_q, (a, b)))
                q += 2
                continue
            kind = rng.integers(0, 4)
            if kind == 0:
                ops.append(CircuitOp("rz", (q,), (), (float(rng.uniform(-math.pi, math.pi)),)))
            elif kind == 1:
                ops.append(CircuitOp("sx", (q,)))
            elif kind == 2:
                ops.append(CircuitOp("x", (q,)))
            q += 1  # kind 3: idle wire in this layer
    if measure:
        ops.append(CircuitOp("barrier", tuple(range(nq))))
        ops.extend(CircuitOp("measure", (q,), (q,)) for q in range(nq))
    return Circuit(nq, nq if measure else 0, ops)


_CLIFFORD_IN_BASIS = {"h": (("rz", math.pi / 2), ("sx", None), ("rz", math.pi / 2)), "s": (("rz", math.pi / 2),),
                      "sdg": (("rz", -math.pi / 2),), "x": (("x", None),), "y": (("rz", math.pi), ("x", None)), "z": (("rz", math.pi),),
                      "sx": (("sx", None),)}   # equal up to a global phase


def random_clifford_circuit(nq: int, depth: int, seed: int, two_q: str = "cx", measure: bool = True, basis: bool = False) -> Circuit:
    """Layers of random disjoint Clifford gates on a line, in the style of :func:`random_circuit`: walking the line, a pair of
    neighbours gets ``two_q`` (either direction) with probability 0.35, otherwise the qubit gets one of h, s, sdg, x, y, z, sx or
    stays idle in this layer, each with probability 1/8.  ``basis=True`` writes the same draws in the backend basis {rz, sx, x, two_q}
    (h = rz sx rz, s = rz(pi / 2), y = x rz(pi), ...), which is what :func:`encode_corpus` and :func:`synthetic_backend` can encode."""
    rng = np.random.default_rng(seed)
    one = ("h", "s", "sdg", "x", "y", "z", "sx")
    ops: List[CircuitOp] = []
    for _ in range(depth):
        q = 0
        while q < nq:
            if q + 1 < nq and rng.random() < 0.35:
                a, b = (q, q + 1) if rng.random() < 0.5 else (q + 1, q)
                ops.append(CircuitOp(two_q, (a, b)))
                q += 2
                continue
            kind = int(rng.integers(0, len(one) + 1))
            if kind < len(one) and basis:
                ops.extend(CircuitOp(g, (q,), (), () if angle is None else (angle,)) for g, angle in _CLIFFORD_IN_BASIS[one[kind]])
            elif kind < len(one):
                ops.append(CircuitOp(one[kind], (q,)))
            q += 1
    if measure:
        ops.append(CircuitOp("barrier", tuple(range(nq))))
        ops.extend(CircuitOp("measure", (q,), (q,)) for q in range(nq))
    return Circuit(nq, nq if measure else 0, ops)


def pauli_twirl(circ: Circuit, seed: int, two_q=("cx", "ecr")) -> Circuit:
    """Random single-qubit Paulis (x, or rz(pi) for Z, or both for Y) before and after every two-qubit gate -- the
    structural effect of Pauli twirling on the circuit graph (cfg5 of BASELINE.json)."""
    rng = np.random.default_rng(seed)

    def pauli(q):
        k = rng.integers(0, 4)
        out = []
        if k in (1, 2):
            out.append(CircuitOp("x", (q,)))
        if k in (2, 3):
            out.append(CircuitOp("rz", (q,), (), (math.pi,)))
        return out

    ops: List[CircuitOp] = []
    for op in circ.ops:
        if op.name in two_q:
            for q in op.qubits:
                ops += pauli(q)
            ops.append(op)
            for q in op.qubits:
                ops += pauli(q)
        else:
            ops.append(op)
    return Circuit(circ.num_qubits, circ.num_clbits, ops)


def encode_corpus(circuits, nq: int, two_q: str = "cx", seed: int = 7, exp_value_size: int = 1,
                  add_self_loops: bool = True, simulate=None, device="cuda", shots=None, sample_ideal: bool = False,
                  clifford: bool = False, trajectories=None, frame_shots=None, mps_bond=None, mps_shots=None,
                  mps_relaxation: bool = False, mps_twirl=None) -> Dict[str, list]:
    """Arena-ready arrays (same keys as :func:`tfim_corpus`) for arbitrary circuits, encoded by the native encoder.

    ``simulate=None``: synthetic labels (a uniform draw and a made-up decay).  ``simulate=`` a ``blackwater.sim.NoiseModel``: ``y``
    and ``noisy`` of every circuit within the simulator's caps (5 qubits as a density matrix) are the exact and the noisy
    ``<Z>`` of the circuit's observable qubit, simulated on ``device`` in two launches; larger circuits keep the synthetic labels,
    unless ``clifford=True``: then every larger circuit that is a Clifford circuit of at most 512 qubits (``sim.is_clifford``) gets its
    exact and noisy ``<Z>`` from ``sim.clifford_expectation_values``, in one call (exact values only: ``shots`` with it is refused).
    ``shots`` (with ``simulate``; default ``None``: exact): the noisy value is a ``shots``-shot estimate drawn on the device with
    ``seed`` (``sim.sample_expectation_values``), and with ``sample_ideal=True`` the ideal one too.
    ``trajectories`` (with ``simulate``; default ``None``): the noisy value is the mean over that many quantum trajectories
    (``sim.trajectory_expectation_values``, keyed by ``seed`` and the circuit's position), and the cap of the simulated circuits
    rises from 5 to 11 qubits; the ideal value stays the exact one.  ``trajectories`` together with ``shots`` is refused.
    ``frame_shots`` (with ``simulate``; default ``None``): every circuit must be a Clifford circuit of at most 512 qubits, and its
    noisy value is a ``frame_shots``-shot estimate by Pauli-frame sampling (``sim.sample_clifford_expectation_values``, keyed by
    ``seed`` and the circuit's position); the ideal value stays the exact one (``sim.clifford_expectation_values``).  Together with
    ``shots`` or ``trajectories``, without ``simulate`` or on a circuit that is no Clifford circuit it is refused by name.
    ``mps_bond`` (with ``simulate``; default ``None``: as ever): every circuit wider than the exact caps (5 qubits, 11 with
    ``trajectories``) whose two-qubit gates all act on neighbouring qubits (``sim.is_line_circuit``) gets its ideal ``<Z>`` from the
    matrix-product-state path at that bond (``sim.mps_expectation_values``: exact while the bonds fit, certified beyond), and with
    ``trajectories`` its noisy ``<Z>`` from that many MPS trajectories (keyed by ``seed`` and the circuit's position; without
    ``trajectories`` its noisy label stays the synthetic one).  With ``clifford=True`` Clifford circuits keep going to the exact
    Clifford path.  The result then has the key ``"mps_error_bound"``: the worst certificate B of those circuits (|<Z> - exact| <=
    2 B; 0.0 where no circuit took the path).  Together with ``shots`` or ``frame_shots``, or without ``simulate``, it is refused.
    ``mps_shots`` (with ``mps_bond`` and ``trajectories``; default ``None``): the noisy ``<Z>`` of those circuits becomes the
    ``mps_shots``-shot estimate drawn from their matrix-product states (``sim.sample_mps_expectation_values``: shot s from trajectory
    s mod ``trajectories``, keyed by ``seed`` and the circuit's position); the ideal value stays the exact MPS value.  Without
    ``mps_bond`` or ``trajectories``, or together with ``shots`` or ``frame_shots``, it is refused by name.
    ``mps_relaxation`` (with ``mps_bond``; default ``False``): ``simulate`` may be a model with thermal relaxation
    (``NoiseModel.from_backend(..., thermal_relaxation=True)``), which the MPS path then unravels into quantum jumps
    (``sim.mps_expectation_values(..., thermal_relaxation=True)``; the centre moves to every relaxed qubit).  ``"mps_error_bound"``
    is then the mean of per-trajectory certificates, each conditional on the jumps drawn (|<Z> - exact| <= 4 B per trajectory).
    Without ``mps_bond`` it is refused by name.
    ``mps_twirl`` (with ``mps_bond``; default ``None``; ``True`` or gate names): the noisy MPS values are taken with the two-qubit
    gates Pauli-twirled on the device (``sim.mps_expectation_values(..., pauli_twirl=)``: one draw per trajectory and gate, the
    circuits lowered once).  Without ``mps_bond`` it is refused by name."""
    from .circuit import circuit_to_qasm
    from .native_encoder import NativeEncoder

    if frame_shots is not None:
        if shots is not None:
            raise ValueError("encode_corpus: frame_shots together with shots (shots= samples the exact simulator, frame_shots= the "
                             "Clifford path: choose one)")
        if trajectories is not None:
            raise ValueError("encode_corpus: frame_shots together with trajectories (choose one estimate of the noisy value)")
        if simulate is None:
            raise ValueError("encode_corpus: frame_shots fills simulated labels, so it needs simulate= (a noise model)")

    if mps_shots is not None:
        if shots is not None or frame_shots is not None:
            raise ValueError("encode_corpus: mps_shots together with " + ("shots" if shots is not None else "frame_shots") +
                             " (shots= samples the exact simulator, frame_shots= the Clifford path, mps_shots= the matrix-product "
                             "states: choose one)")
        if mps_bond is None:
            raise ValueError("encode_corpus: mps_shots without mps_bond (the shots are drawn from matrix-product states: pass "
                             "mps_bond=chi)")
        if trajectories is None:
            raise ValueError("encode_corpus: mps_shots without trajectories (the noisy states are Pauli-insertion trajectories: pass "
                             "trajectories=T, at most mps_shots)")
    if not isinstance(mps_relaxation, bool):
        raise ValueError(f"encode_corpus: mps_relaxation = {mps_relaxation!r}, want True or False")
    if mps_relaxation and mps_bond is None:
        raise ValueError("encode_corpus: mps_relaxation without mps_bond (thermal relaxation is unravelled on the matrix-product-state "
                         "path: pass mps_bond=chi)")
    if mps_twirl is not None and mps_twirl is not False and mps_bond is None:
        raise ValueError("encode_corpus: mps_twirl without mps_bond (the twirl is drawn per trajectory on the matrix-product-state "
                         "path: pass mps_bond=chi)")
    if mps_bond is not None:
        if shots is not None or frame_shots is not None:
            raise ValueError("encode_corpus: mps_bond together with " + ("shots" if shots is not None else "frame_shots") +
                             " (no shots are drawn from a matrix-product state: its noisy values are means over trajectories=)")
        if simulate is None:
            raise ValueError("encode_corpus: mps_bond fills simulated labels, so it needs simulate= (a noise model)")
        from ..sim.mps import _check_bond

        mps_bond = _check_bond(mps_bond, "encode_corpus")

    props = get_backend_properties_v1(synthetic_backend(nq, two_q))
    enc = NativeEncoder(props)
    rng = np.random.default_rng(seed)
    mps_error_bound = 0.0
    xs, eis, ys, noisy, depth, obs = [], [], [], [], [], []
    kept, z_qubits = [], []
    for circ in circuits:
        x, ei, _, d = enc.encode(circuit_to_qasm(circ))
        if add_self_loops:
            loops = np.arange(x.shape[0], dtype=np.int64)
            ei = np.concatenate([ei, np.stack([loops, loops])], axis=1)
        ideal = rng.uniform(-1, 1, size=exp_value_size)
        n2q = sum(1 for op in circ.ops if op.name == two_q)
        xs.append(x.astype(np.float32))
        eis.append(ei)
        ys.append(ideal)
        noisy.append(ideal * math.exp(-5e-3 * n2q) + rng.normal(0, 0.01, size=exp_value_size))
        depth.append([float(d)])
        o = np.zeros((1, 4 * nq + 1), dtype=np.float32)
        o[0, 0], o[0, 1::4] = 1.0, 1.0
        qz = int(rng.integers(0, nq))
        o[0, 1 + 4 * qz], o[0, 2 + 4 * qz] = 0.0, 1.0
        obs.append(o)
        kept.append(circ)
        z_qubits.append(qz)
    if clifford and simulate is None:
        raise ValueError("encode_corpus: clifford=True fills simulated labels, so it needs simulate= (a noise model)")
    if clifford and shots is not None:
        raise ValueError("encode_corpus: clifford=True gives exact values only; shots are not drawn on the Clifford path")
    if trajectories is not None and simulate is None:
        raise ValueError("encode_corpus: trajectories fill simulated labels, so they need simulate= (a noise model)")
    if trajectories is not None and shots is not None:
        raise ValueError("encode_corpus: trajectories together with shots (shot sampling over trajectories is not supported)")
    if frame_shots is not None:
        from .. import sim

        for k, circ in enumerate(kept):
            if not (1 <= circ.num_qubits <= sim.MAX_QUBITS_CLIFFORD and sim.is_clifford(circ)):
                raise ValueError(f"encode_corpus: frame_shots: circuit {k} is not a Clifford circuit of at most "
                                 f"{sim.MAX_QUBITS_CLIFFORD} qubits; frame sampling takes no other")
        labels = ["".join("Z" if q == z_qubits[k] else "I" for q in reversed(range(circ.num_qubits))) for k, circ in enumerate(kept)]
        if kept:
            exact = sim.clifford_expectation_values(kept, labels, None, device)[0].cpu().numpy()
            under = sim.sample_clifford_expectation_values(kept, labels, simulate, shots=frame_shots, seed=seed,
                                                           run_keys=np.arange(len(kept), dtype=np.int64), device=device).values.cpu().numpy()
            for k in range(len(kept)):
                ys[k] = np.full(exp_value_size, exact[k])
                noisy[k] = np.full(exp_value_size, under[k])
    elif simulate is not None:
        from .. import sim

        cap = sim.MAX_QUBITS_DENSITY if trajectories is None else sim.MAX_QUBITS_VECTOR
        wide = [k for k, circ in enumerate(kept) if clifford and cap < circ.num_qubits <= sim.MAX_QUBITS_CLIFFORD
                and sim.is_clifford(circ)]
        if wide:
            labels = ["".join("Z" if q == z_qubits[k] else "I" for q in reversed(range(kept[k].num_qubits))) for k in wide]
            under, _, _, exact, _ = sim.clifford_expectation_values([kept[k] for k in wide], labels, simulate, device, return_ideal=True)
            under, exact = under.cpu().numpy(), exact.cpu().numpy()
            for j, k in enumerate(wide):
                ys[k] = np.full(exp_value_size, exact[j])
                noisy[k] = np.full(exp_value_size, under[j])
        line = [k for k, circ in enumerate(kept) if mps_bond is not None and k not in wide
                and cap < circ.num_qubits <= sim.MAX_QUBITS_MPS and sim.is_line_circuit(circ)]
        if line:
            labels = ["".join("Z" if q == z_qubits[k] else "I" for q in reversed(range(kept[k].num_qubits))) for k in line]
            res = sim.mps_expectation_values([kept[k] for k in line], labels, max_bond=mps_bond, device=device)
            exact, mps_error_bound = res.values.cpu().numpy(), float(res.error_bound.max())
            for j, k in enumerate(line):
                ys[k] = np.full(exp_value_size, exact[j])
            if trajectories is not None:
                if mps_shots is not None:
                    res = sim.sample_mps_expectation_values([kept[k] for k in line], labels, simulate, shots=mps_shots, max_bond=mps_bond,
                                                            trajectories=trajectories, seed=seed,
                                                            run_keys=np.asarray(line, dtype=np.int64), device=device,
                                                            thermal_relaxation=mps_relaxation, pauli_twirl=mps_twirl)
                else:
                    res = sim.mps_expectation_values([kept[k] for k in line], labels, simulate, max_bond=mps_bond,
                                                     trajectories=trajectories, seed=seed, run_keys=np.asarray(line, dtype=np.int64),
                                                     device=device, thermal_relaxation=mps_relaxation, pauli_twirl=mps_twirl)
                under, mps_error_bound = res.values.cpu().numpy(), max(mps_error_bound, float(res.error_bound.max()))
                for j, k in enumerate(line):
                    noisy[k] = np.full(exp_value_size, under[j])
        inside = [k for k, circ in enumerate(kept) if 1 <= circ.num_qubits <= cap]
        if inside:
            labels = ["".join("Z" if q == z_qubits[k] else "I" for q in reversed(range(kept[k].num_qubits))) for k in inside]
            batch = [kept[k] for k in inside]
            if trajectories is not None:
                keys = np.asarray(inside, dtype=np.int64)   # the circuit's position in the corpus, as on the shots path
                exact = sim.expectation_values(batch, labels, None, device)[0].cpu().numpy()
                under = sim.trajectory_expectation_values(batch, labels, simulate, trajectories=trajectories, seed=seed, run_keys=keys,
                                                          device=device).values.cpu().numpy()
            elif shots is None:
                exact = sim.expectation_values(batch, labels, None, device)[0].cpu().numpy()
                under = sim.expectation_values(batch, labels, simulate, device)[0].cpu().numpy()
            else:
                keys = np.asarray(inside, dtype=np.int64)   # the circuit's position in the corpus
                under = sim.sample_expectation_values(batch, labels, simulate, shots=shots, seed=seed, run_keys=keys,
                                                      device=device).values.cpu().numpy()
                exact = (sim.sample_expectation_values(batch, labels, None, shots=shots, seed=seed, run_keys=keys + (1 << 40),
                                                       device=device).values if sample_ideal
                         else sim.expectation_values(batch, labels, None, device)[0]).cpu().numpy()
            for j, k in enumerate(inside):
                ys[k] = np.full(exp_value_size, exact[j])
                noisy[k] = np.full(exp_value_size, under[j])
    out = {"x": xs, "edge_index": eis, "y": np.asarray(ys, np.float32), "noisy": np.asarray(noisy, np.float32),
           "depth": np.asarray(depth, np.float32), "observable": np.asarray(obs, np.float32)}
    if mps_bond is not None:
        out["mps_error_bound"] = mps_error_bound
    return out


def synthetic_backend(nq: int, two_q: str = "ecr", seed: int = 0) -> StaticBackend:
    """FakeLima-like calibration table stretched to ``nq`` qubits on a line (seeded)."""
    rng = np.random.default_rng(seed)
    nduv = lambda name, unit, value: {"name": name, "unit": unit, "value": float(value)}
    qubits = [[nduv("T1", "us", rng.uniform(20, 120)), nduv("T2", "us", rng.uniform(20, 120)),
               nduv("readout_error", "", rng.uniform(0.01, 0.06))] for _ in range(nq)]
    log_u = lambda: math.exp(rng.uniform(math.log(1e-4), math.log(2e-2)))
    gates = []
    for q in range(nq):
        for g, length in (("id", 35.5), ("rz", 0.0), ("sx", 35.5), ("x", 35.5)):
            gates.append({"gate": g, "qubits": [q], "name": f"{g}{q}",
                          "parameters": [nduv("gate_error", "", 0.0 if g == "rz" else log_u()),
                                         nduv("gate_length", "ns", length)]})
        gates.append({"gate": "reset", "qubits": [q], "name": f"reset{q}",
                      "parameters": [nduv("gate_length", "ns", 5351.1)]})
    for q in range(nq - 1):
        for a, b in ((q, q + 1), (q + 1, q)):
            gates.append({"gate": two_q, "qubits": [a, b], "name": f"{two_q}{a}_{b}",
                          "parameters": [nduv("gate_error", "", log_u()), nduv("gate_length", "ns", 660.0)]})
    return StaticBackend(f"synthetic_{nq}q", {"backend_name": f"synthetic_{nq}q", "qubits": qubits, "gates": gates})


class TfimCorpus:
    """The (steps x J) grid of encoded TFIM-Trotter graphs, WITHOUT holding one feature matrix per circuit.

    The graph of a TFIM circuit depends on J only through the rz angle of the bond rotations (feature column 0), so each
    step count is encoded once with the real encoder ("template") and a circuit is (template, J).  Graph ids run
    step-major: ``g = steps_index * n_J + j``; J ~ U(0, 0.66 pi) from ``np.random.RandomState(seed)`` as in the reference's
    ``get_Js`` (h24 notebook cell [7]).  ``host_graphs(ids)`` materialises plain numpy graphs (what the CPU oracle and
    the host-side loaders consume); ``arena(device, ids)`` replicates the templates ON THE DEVICE straight into a
    :class:`GraphArena` -- an 8 200-circuit / 90 M-node corpus costs ten template uploads instead of 9 GB of host
    arrays."""

    def __init__(self, nq: int, steps_list, n_J: int, seed: int = 42, two_q: str = "ecr", exp_value_size: int = 1,
                 add_self_loops: bool = True):
        props = get_backend_properties_v1(synthetic_backend(nq, two_q))
        self.nq, self.n_J, self.steps_list = nq, int(n_J), list(steps_list)
        rs = np.random.RandomState(seed)
        self.Js = rs.uniform(0, 0.66 * math.pi, size=n_J)
        label_rng = np.random.default_rng(seed + 1)
        self.templates = []
        ys, noisy, depth, obs_z = [], [], [], []
        for steps in self.steps_list:
            circ = tfim_circuit(nq, steps, J=1.0, two_q=two_q)  # phi = -2*J*dt = -1.0: marks the J-dependent nodes
            graph = circuit_to_graph_data_json(circ, props, use_gate_features=True, use_qubit_features=True)
            x0 = np.asarray(graph["nodes"]["DAGOpNode"], dtype=np.float32)
            ei = np.asarray(graph["edges"]["DAGOpNode_wire_DAGOpNode"]["edge_index"], dtype=np.int64)
            if add_self_loops:  # the training path's dataset transform (loaders/exp_val.py:33)
                loops = np.arange(x0.shape[0], dtype=np.int64)
                ei = np.concatenate([ei, np.stack([loops, loops])], axis=1)
            bond_nodes = np.array([k for k, op in enumerate(circ.ops) if op.name == "rz" and op.params[0] == -1.0],
                                  dtype=np.int64)
            n2q = sum(1 for op in circ.ops if op.name == two_q)
            d = circ.depth()
            self.templates.append({"x": x0, "edge_index": ei, "bond_nodes": bond_nodes, "depth": float(d)})
            for _ in range(self.n_J):   # same draw order as ever: ideal, noise, observable qubit -- per circuit
                ideal = label_rng.uniform(-1, 1, size=exp_value_size)
                ys.append(ideal)
                noisy.append(ideal * math.exp(-2e-4 * n2q) + label_rng.normal(0, 0.01, size=exp_value_size))
                depth.append([float(d)])
                obs_z.append(int(label_rng.integers(0, nq)))
        self.y, self.noisy = np.asarray(ys, np.float32), np.asarray(noisy, np.float32)
        self.depth, self.obs_z = np.asarray(depth, np.float32), np.asarray(obs_z, np.int64)
        self.node_counts = np.repeat([t["x"].shape[0] for t in self.templates], self.n_J).astype(np.int64)

    def __len__(self):
        return len(self.templates) * self.n_J

    def observables(self, ids) -> np.ndarray:
        """[len(ids), 1, 4 nq + 1]: coefficient 1, identity everywhere except one Z."""
        ids = np.asarray(ids, dtype=np.int64)
        o = np.zeros((len(ids), 1, 4 * self.nq + 1), dtype=np.float32)
        o[:, 0, 0] = 1.0
        o[:, 0, 1::4] = 1.0
        rows = np.arange(len(ids))
        o[rows, 0, 1 + 4 * self.obs_z[ids]] = 0.0
        o[rows, 0, 2 + 4 * self.obs_z[ids]] = 1.0
        return o

    def graph_x(self, g: int) -> np.ndarray:
        t = self.templates[g // self.n_J]
        x = t["x"].copy()
        x[t["bond_nodes"], 0] = np.float32(-2 * self.Js[g % self.n_J] * 0.5)
        return x

    def host_graphs(self, ids=None) -> Dict[str, list]:
        ids = np.arange(len(self)) if ids is None else np.asarray(ids, dtype=np.int64)
        return {"x": [self.graph_x(int(g)) for g in ids],
                "edge_index": [self.templates[int(g) // self.n_J]["edge_index"] for g in ids],
                "y": self.y[ids], "noisy": self.noisy[ids], "depth": self.depth[ids], "observable": self.observables(ids)}

    def arena(self, device, ids=None, filler_nodes: int = 0):
        """The graphs ``ids`` (ascending global ids; default all) as a device-resident arena, built by replicating the
        templates on the device.  Under data parallelism every rank passes its own shard of ids."""
        import torch

        from .arena import GraphArena

        ids = np.arange(len(self)) if ids is None else np.asarray(ids, dtype=np.int64)
        if len(ids) > 1 and (np.diff(ids) <= 0).any():
            raise ValueError("TfimCorpus.arena: ids must be strictly ascending")
        dev = torch.device(device)
        f = self.templates[0]["x"].shape[1]
        f4 = (f + 3) // 4 * 4
        tmpl_of = ids // self.n_J
        n_total = int(self.node_counts[ids].sum())
        x = torch.zeros((max(n_total, 1), f4), dtype=torch.float32, device=dev)
        ei_parts, base = [], 0
        for t_idx, t in enumerate(self.templates):
            mine = ids[tmpl_of == t_idx]
            c = len(mine)
            if c == 0:
                continue
            n_t = t["x"].shape[0]
            x0 = torch.from_numpy(t["x"]).to(dev)
            block = x[base:base + c * n_t].view(c, n_t, f4)
            block[:, :, :f] = x0.unsqueeze(0)
            bond = torch.from_numpy(t["bond_nodes"]).to(dev)
            jv = torch.from_numpy((-2 * self.Js[mine % self.n_J] * 0.5).astype(np.float32)).to(dev)
            block[:, bond, 0] = jv.unsqueeze(1)
            ei_t = torch.from_numpy(t["edge_index"]).to(dev)
            offs = base + torch.arange(c, device=dev, dtype=torch.int64) * n_t
            ei_parts.append((ei_t.unsqueeze(1) + offs.view(1, c, 1)).reshape(2, -1))
            base += c * n_t
        ei = torch.cat(ei_parts, dim=1) if ei_parts else torch.zeros((2, 0), dtype=torch.int64, device=dev)
        return GraphArena.from_device(x[:n_total, :f], self.node_counts[ids], ei, self.y[ids], self.noisy[ids],
                                      self.depth[ids], self.observables(ids), filler_nodes=filler_nodes)


def tfim_corpus(nq: int, steps_list, n_J: int, seed: int = 42, two_q: str = "ecr", exp_value_size: int = 1,
                add_self_loops: bool = True) -> Dict[str, list]:
    """Encoded graphs for every (steps, J) pair as plain host arrays: ``steps_list`` x ``n_J`` circuits
    (see :class:`TfimCorpus`)."""
    return TfimCorpus(nq, steps_list, n_J, seed, two_q, exp_value_size, add_self_loops).host_graphs()
