"""Wire/disk record of one training example (reference: blackwater/data/generators/exp_val.py:31-89).

``exp_value_generator`` of that file (:92-170) runs Aer; here it runs the batched simulator of ``blackwater.sim`` on the device:
exact ideal values from state vectors, noisy ones from density matrices under the project's own depolarising noise model.
"""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Any, Dict, Iterator, List, Optional

import numpy as np
import torch

from ..graph import Data

OP_EDGE_KEY = "DAGOpNode_wire_DAGOpNode"


@dataclass
class ExpValueEntry:
    """Encoded circuit graph + observable + ideal / noisy expectation values (+ depth)."""

    circuit_graph: Dict[str, Any]
    observable: List[List[float]]
    ideal_exp_value: float
    noisy_exp_values: List[float]
    circuit_depth: int = 0

    def __repr__(self):
        return f"<ExpValueEntry (ideal: {self.ideal_exp_value}, noisy: {self.noisy_exp_values})>"

    def to_dict(self) -> Dict[str, Any]:
        return {
            "circuit_graph": self.circuit_graph,
            "observable": self.observable,
            "ideal_exp_value": self.ideal_exp_value,
            "noisy_exp_values": self.noisy_exp_values,
            "circuit_depth": self.circuit_depth,
        }

    @classmethod
    def from_json(cls, dictionary: Dict[str, Any]) -> "ExpValueEntry":
        return cls(**dictionary)

    def to_pyg_data(self) -> Data:
        """Tensor view used by the models: x[N,F] f32, edge_index[2,E] i64 over op->op wires (a graph
        without such edges raises ``KeyError`` -- the dataset relies on it to drop the entry),
        edge_attr[E,3], y[1,1(,k)], observable[1,T,1+4n], circuit_depth[1,1], noisy_i[1,1(,k)]."""
        wires = self.circuit_graph["edges"][OP_EDGE_KEY]
        fields = {
            "x": torch.tensor(self.circuit_graph["nodes"]["DAGOpNode"], dtype=torch.float),
            "edge_index": torch.tensor(wires["edge_index"], dtype=torch.long),
            "edge_attr": torch.tensor(wires["edge_attr"], dtype=torch.float),
            "y": torch.tensor([[self.ideal_exp_value]], dtype=torch.float),
            "observable": torch.tensor([self.observable], dtype=torch.float),
            "circuit_depth": torch.tensor([[self.circuit_depth]], dtype=torch.float),
        }
        for k, value in enumerate(self.noisy_exp_values):
            fields[f"noisy_{k}"] = torch.tensor([[value]], dtype=torch.float)
        return Data(**fields)


def exp_value_generator(backend: Any, n_qubits: int, circuit_depth: int, pauli_terms: int, pauli_coeff: float = 1.0,
                        max_entries: int = 1000, seed: int = 0, batch: int = 256, device="cuda", shots: Optional[int] = None,
                        sample_ideal: bool = False, trajectories: Optional[int] = None,
                        frame_shots: Optional[int] = None, mps_bond: Optional[int] = None,
                        mps_shots: Optional[int] = None, mps_relaxation: bool = False,
                        mps_twirl: Any = None) -> Iterator[ExpValueEntry]:
    """Yields ``max_entries`` dataset entries of random circuits with simulated labels (reference: exp_val.py:92-170, which
    transpiles ``qiskit.circuit.random.random_circuit`` and runs Aer twice per circuit).

    Circuits: ``synthetic.random_circuit`` on ``n_qubits`` qubits in the backend's basis (its two-qubit gate is taken from the
    calibration table), depth drawn in 1..``circuit_depth``.  Observable: ``generate_random_pauli_sum_op(n_qubits, pauli_terms,
    pauli_coeff)``.  ``ideal_exp_value``: the exact value, state-vector mode.  ``noisy_exp_values``: ``[v]`` with v from the
    density-matrix mode under ``NoiseModel.from_backend(backend, readout=False)`` -- the project's depolarising model, not Aer's.
    Readout noise is OFF: random Pauli sums contain X and Y, and a readout op leaves only the diagonal of the density matrix
    meaningful.  ``batch`` circuits are simulated per launch (two launches: ideal, noisy); entries are yielded one by one and are a
    function of ``seed`` alone.

    ``shots`` (default ``None``: exact labels): the noisy value is estimated from that many measurement outcomes per measurement
    basis, drawn on the device (``sim.sample_expectation_values``; the reference's labels are 10 000-shot estimates), and with
    ``sample_ideal=True`` the ideal one too.  The draws are keyed by ``seed`` and the entry's number, so an entry is still a
    function of ``seed`` (and ``shots``) alone, whatever ``batch`` is.

    ``trajectories`` (default ``None``): the noisy value is the mean over that many quantum trajectories
    (``sim.trajectory_expectation_values``), which reaches ``n_qubits`` of 6 to 11 where the density-matrix mode stops at 5; the
    ideal value stays the exact state-vector one.  The draws are keyed as the shots are, so an entry is a function of ``seed`` and
    ``trajectories`` alone, whatever ``batch`` is.  ``trajectories`` together with ``shots`` is refused.

    ``frame_shots`` (default ``None``): the circuits are Clifford circuits (``synthetic.random_clifford_circuit`` in the backend's
    basis) of up to 512 qubits, the noisy value is a ``frame_shots``-shot estimate by Pauli-frame sampling
    (``sim.sample_clifford_expectation_values``, keyed as the shots are) and the ideal value stays the exact one
    (``sim.clifford_expectation_values``).  Together with ``shots`` or ``trajectories`` it is refused by name.

    ``mps_bond`` (default ``None``; with ``trajectories``): both values come from the matrix-product-state path at that bond
    (``sim.mps_expectation_values``: ``n_qubits`` up to 512, the circuits' two-qubit gates act on neighbours), the noisy one as
    the mean over ``trajectories`` Pauli-insertion trajectories, keyed as the shots are.  Without ``trajectories``, or together
    with ``shots`` or ``frame_shots``, it is refused by name.

    ``mps_shots`` (default ``None``; with ``mps_bond`` and ``trajectories``): the noisy value becomes the ``mps_shots``-shot estimate
    drawn from the matrix-product states (``sim.sample_mps_expectation_values``, shot s from trajectory s mod ``trajectories``, keyed as
    the shots are); the ideal value stays the exact MPS value.  Without ``mps_bond``, or together with ``shots`` or ``frame_shots``,
    it is refused by name.

    ``mps_relaxation`` (default ``False``; with ``mps_bond``): the noisy value is taken under
    ``NoiseModel.from_backend(backend, readout=False, thermal_relaxation=True)`` -- Aer's device model restated -- which the MPS
    path unravels into quantum jumps (``thermal_relaxation=True`` there).  Without ``mps_bond`` it is refused by name.

    ``mps_twirl`` (default ``None``; with ``mps_bond``; ``True`` or gate names): the noisy value is taken with the two-qubit gates
    Pauli-twirled on the device (``pauli_twirl=`` there: one draw per trajectory and gate).  Without ``mps_bond`` it is refused by
    name."""
    if mps_twirl is not None and mps_twirl is not False and mps_bond is None:
        raise ValueError("exp_value_generator: mps_twirl without mps_bond (the twirl is drawn per trajectory on the "
                         "matrix-product-state path: pass mps_bond=chi)")
    if not isinstance(mps_relaxation, bool):
        raise ValueError(f"exp_value_generator: mps_relaxation = {mps_relaxation!r}, want True or False")
    if mps_relaxation and mps_bond is None:
        raise ValueError("exp_value_generator: mps_relaxation without mps_bond (thermal relaxation is unravelled on the "
                         "matrix-product-state path: pass mps_bond=chi)")
    if mps_shots is not None:
        if shots is not None or frame_shots is not None:
            raise ValueError("exp_value_generator: mps_shots together with " + ("shots" if shots is not None else "frame_shots") +
                             " (shots= samples the exact simulator, frame_shots= the Clifford path, mps_shots= the matrix-product "
                             "states: choose one)")
        if mps_bond is None:
            raise ValueError("exp_value_generator: mps_shots without mps_bond (the shots are drawn from matrix-product states: pass "
                             "mps_bond=chi)")
    if mps_bond is not None:
        if shots is not None or frame_shots is not None:
            raise ValueError("exp_value_generator: mps_bond together with " + ("shots" if shots is not None else "frame_shots") +
                             " (no shots are drawn from a matrix-product state: its noisy values are means over trajectories=)")
        if trajectories is None:
            raise ValueError("exp_value_generator: mps_bond without trajectories (the noisy value of the MPS path is a mean over "
                             "trajectories: pass trajectories=T)")
    if trajectories is not None and shots is not None:
        raise ValueError("exp_value_generator: trajectories together with shots (shot sampling over trajectories is not supported)")
    if frame_shots is not None and shots is not None:
        raise ValueError("exp_value_generator: frame_shots together with shots (shots= samples the exact simulator, frame_shots= the "
                         "Clifford path: choose one)")
    if frame_shots is not None and trajectories is not None:
        raise ValueError("exp_value_generator: frame_shots together with trajectories (choose one estimate of the noisy value)")
    from ... import sim
    from ..synthetic import random_circuit, random_clifford_circuit
    from ..utils import circuit_to_graph_data_json, encode_pauli_sum_op, generate_random_pauli_sum_op, get_backend_properties_v1

    properties = get_backend_properties_v1(backend)
    two_q = [g for g in properties["gates_set"] if g in ("cx", "ecr", "cz")]
    if len(two_q) != 1:
        raise ValueError(f"exp_value_generator: want one two-qubit basis gate among cx / ecr / cz, the backend has {two_q}")
    if batch < 1:
        raise ValueError(f"exp_value_generator: batch must be >= 1, got {batch}")
    noise = sim.NoiseModel.from_backend(backend, readout=False, thermal_relaxation=mps_relaxation)
    rng = np.random.default_rng(seed)
    done = 0
    while done < max_entries:
        count = min(int(batch), max_entries - done)
        circuits, observables = [], []
        for _ in range(count):
            depth = int(rng.integers(1, circuit_depth + 1))
            circuit_seed = int(rng.integers(0, 2 ** 31 - 1))
            circuits.append(random_circuit(n_qubits, depth, circuit_seed, two_q=two_q[0]) if frame_shots is None
                            else random_clifford_circuit(n_qubits, depth, circuit_seed, two_q=two_q[0], measure=False, basis=True))
            observables.append(generate_random_pauli_sum_op(n_qubits, pauli_terms, pauli_coeff, rng=rng))
        if frame_shots is not None:
            keys = np.arange(done, done + count, dtype=np.int64)   # the entry's number, as on the shots path
            ideal = _to_host(sim.clifford_expectation_values(circuits, observables, None, device)[0])
            noisy = _to_host(sim.sample_clifford_expectation_values(circuits, observables, noise, shots=frame_shots, seed=seed,
                                                                    run_keys=keys, device=device).values)
        elif mps_bond is not None:
            keys = np.arange(done, done + count, dtype=np.int64)   # the entry's number, as on the shots path
            ideal = _to_host(sim.mps_expectation_values(circuits, observables, max_bond=mps_bond, device=device).values)
            if mps_shots is not None:
                noisy = _to_host(sim.sample_mps_expectation_values(circuits, observables, noise, shots=mps_shots, max_bond=mps_bond,
                                                                   trajectories=trajectories, seed=seed, run_keys=keys,
                                                                   device=device, thermal_relaxation=mps_relaxation,
                                                                   pauli_twirl=mps_twirl).values)
            else:
                noisy = _to_host(sim.mps_expectation_values(circuits, observables, noise, max_bond=mps_bond, trajectories=trajectories,
                                                            seed=seed, run_keys=keys, device=device,
                                                            thermal_relaxation=mps_relaxation, pauli_twirl=mps_twirl).values)
        elif trajectories is not None:
            keys = np.arange(done, done + count, dtype=np.int64)   # the entry's number, as on the shots path
            ideal = _to_host(sim.expectation_values(circuits, observables, None, device)[0])
            noisy = _to_host(sim.trajectory_expectation_values(circuits, observables, noise, trajectories=trajectories, seed=seed,
                                                               run_keys=keys, device=device).values)
        elif shots is None:
            ideal = _to_host(sim.expectation_values(circuits, observables, None, device)[0])
            noisy = _to_host(sim.expectation_values(circuits, observables, noise, device)[0])
        else:
            keys = np.arange(done, done + count, dtype=np.int64)   # the entry's number; the ideal launch draws with keys 2^40 further on
            noisy = _to_host(sim.sample_expectation_values(circuits, observables, noise, shots=shots, seed=seed, run_keys=keys,
                                                           device=device).values)
            ideal = _to_host(sim.sample_expectation_values(circuits, observables, None, shots=shots, seed=seed, run_keys=keys + (1 << 40),
                                                           device=device).values if sample_ideal
                             else sim.expectation_values(circuits, observables, None, device)[0])
        for k, (circuit, observable) in enumerate(zip(circuits, observables)):
            graph = circuit_to_graph_data_json(circuit=circuit, properties=properties, use_qubit_features=True, use_gate_features=True)
            yield ExpValueEntry(circuit_graph=graph, observable=encode_pauli_sum_op(observable), ideal_exp_value=float(ideal[k]),
                                noisy_exp_values=[float(noisy[k])], circuit_depth=circuit.depth())
        done += count


def _to_host(values) -> np.ndarray:
    return np.asarray(values.cpu() if hasattr(values, "cpu") else values, dtype=np.float64)
