"""Device side of the batched simulator: one call of ``mlqem_sim_run_f64`` per batch, and an Estimator-shaped primitive on it."""
from __future__ import annotations

from typing import Any, Optional, Sequence

import numpy as np

from ..library.primitives import make_estimator_result
from .program import NoiseModel, SimBatch, compile_programs


def run_batch(batch: SimBatch, device="cuda"):
    """``(values, term_values, norm)`` of a lowered batch: float64 tensors on ``device``."""
    from ..native import ops

    t = batch.to(device)
    return ops.sim_run(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"],
                       t["n_wave"], t["n_wg"])


def expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None, device="cuda"):
    """Exact expectation values of ``observables[k]`` after ``circuits[k]``: ``(values, term_values, term_ptr)``, float64 [B],
    float64 [n_terms] and int64 [B + 1] tensors on ``device`` (``term_values[term_ptr[k] : term_ptr[k + 1]]`` are the Pauli terms
    of circuit k, without their coefficients).  ``noise=None`` simulates state vectors, a :class:`NoiseModel` density matrices;
    everything is lowered and validated on the host first (:func:`compile_programs`), then simulated in at most two launches."""
    import torch

    batch = compile_programs(circuits, observables, noise)
    values, term_values, _ = run_batch(batch, device)
    return values, term_values, torch.from_numpy(batch.term_ptr).to(values.device)


class SimulatedJob:
    """The job of a :class:`DeviceEstimator` run: the values are already on the host when it is built."""

    def __init__(self, values: np.ndarray, job_id: str):
        self._values, self._job_id = values, job_id

    def result(self):
        return make_estimator_result(self._values, [{} for _ in range(len(self._values))])

    def job_id(self) -> str:
        return self._job_id

    def status(self) -> str:
        return "DONE"

    def submit(self):
        return None

    def cancel(self) -> bool:
        return False


class DeviceEstimator:
    """An Estimator-shaped primitive on the batched simulator: ``run(circuits, observables, parameter_values)`` returns a job whose
    ``result().values[k]`` is the exact expectation value of ``observables[k]`` after ``circuits[k]`` (``noise=None``) or the one
    under ``noise`` (a :class:`NoiseModel`, density-matrix mode), ``metadata[k] = {}``.  It has the ``_run`` protocol the
    ``learning(...)`` and ``ngem(...)`` decorators patch.  Circuits arrive bound (QASM text, ``Circuit`` or a bound qiskit-like
    circuit); non-empty ``parameter_values`` are refused.  There is no host path: ``device`` must be a GPU."""

    def __init__(self, noise: Optional[NoiseModel] = None, device="cuda"):
        self._noise, self._device, self._count = noise, device, 0

    def run(self, circuits, observables, parameter_values=None, **run_options):
        circuits, observables = list(circuits), list(observables)
        if parameter_values is None:
            parameter_values = [()] * len(circuits)
        return self._run(circuits, observables, list(parameter_values), **run_options)

    def _run(self, circuits, observables, parameter_values, **run_options):
        for k, p in enumerate(parameter_values):
            if len(p):
                raise ValueError(f"DeviceEstimator: circuit {k} comes with {len(p)} parameter values; circuits must arrive bound")
        values, _, _ = expectation_values(circuits, observables, self._noise, self._device)
        self._count += 1
        return SimulatedJob(values.cpu().numpy(), f"sim-{self._count}")
