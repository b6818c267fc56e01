"""Learning-based estimator: wraps any qiskit-style Estimator class so that ``job.result()`` returns values
post-processed by a pluggable processor (reference: blackwater/library/learning/estimator.py:22-30,151-328).

In scope: the decorator, the job wrapper, the processor protocol, ``TorchLearningModelProcessor``,
``EmptyProcessor``, ``ScikitLearningModelProcessor`` (the random-forest / OLS baselines: same feature rows, the
model stays on the host CPU), ``ForestLearningModelProcessor``, ``BoostedLearningModelProcessor`` and
``LinearLearningModelProcessor`` (additions: the same random forests, gradient-boosted trees and OLS / ridge models scored on the
device by the forest, boosted-trees and least-squares kernels, one launch per ``run()``) and ``ZNEProcessor`` (no model: it runs
the circuits at amplified noise through a ZNE estimator, ``blackwater.zne.zne(cls)``, and extrapolates to zero noise; around
``blackwater.sim.DeviceEstimator`` a whole ``run()`` is one fused launch, reference :33-86).
"""
from __future__ import annotations

from functools import wraps
from typing import Any, Callable, Optional, Type

import numpy as np
import torch

from ...data.backends import is_pauli_observable
from ...data.utils import encode_pauli_sum_op, get_backend_properties_v1
from ...exception import BlackwaterException
from ..primitives import job_base, make_estimator_result, model_device, transpile_and_bind
from .features import encode_data


class LearningMethodEstimatorProcessor:
    """Protocol: ``process(expectation_value, circuits, observables, parameter_values) -> float | ndarray``, called
    once per (value, bound circuit, observable, parameters) tuple."""

    def process(self, expectation_value, circuits, observables, parameter_values):
        raise NotImplementedError


class TorchLearningModelProcessor(LearningMethodEstimatorProcessor):
    """Feeds ``encode_data`` rows to a torch model, one Pauli term at a time, and sums ``output * coeff``.

    As in the reference (:170-187) the WHOLE-observable expectation value is the noisy input of every term, so this is
    meant for single-Pauli observables (``separate_observables=True`` in the VQE drivers)."""

    accepts_qasm_text = True     # process_batch scans OpenQASM text natively: PostProcessedJob hands text over unparsed

    def __init__(self, model: torch.nn.Module, backend):
        self._model = model
        self._backend = backend
        self._properties = get_backend_properties_v1(backend)

    def process(self, expectation_value, circuits, observables, parameter_values):
        device = model_device(self._model)
        results = []
        for term in observables:
            coeff, label = term.coeffs, str(term.paulis[0])
            # OpenQASM text takes the C++ op scan (mlqem_circuit_features_qasm): same row, no Python circuit objects
            model_input, _ = encode_data(circuits=[circuits], properties=self._properties, ideal_exp_vals=[[0.0]],
                                         noisy_exp_vals=[[expectation_value]], num_qubits=1,
                                         meas_bases=encode_pauli_sum_op([(label, 1.0)]), native=isinstance(circuits, str))
            if device is not None:
                model_input = model_input.to(device)
            with torch.no_grad():
                output = self._model(model_input).item()
            results.append(output * coeff[0])
        return np.sum(results)

    def process_batch(self, expectation_values, circuits, observables, parameter_values):
        """All (circuit, Pauli term) rows of one ``run()`` through ONE model call (an addition: ``PostProcessedJob``
        uses it when the processor has it; results equal ``process`` applied circuit by circuit)."""
        rows, owners, coeffs, values, bases = [], [], [], [], []
        for k, (value, circuit, obs) in enumerate(zip(expectation_values, circuits, observables)):
            for term in obs:
                rows.append(circuit)
                owners.append(k)
                coeffs.append(term.coeffs[0])
                values.append([float(value)])
                bases.append(encode_pauli_sum_op([(str(term.paulis[0]), 1.0)])[0])
        if not rows:
            return [0.0] * len(circuits)
        # one feature matrix for the whole run(); OpenQASM text goes through the C++ op scan (mlqem_circuit_features_qasm)
        native = all(isinstance(c, str) for c in rows)
        model_input, _ = encode_data(circuits=rows, properties=self._properties, ideal_exp_vals=[[0.0]] * len(rows),
                                     noisy_exp_vals=values, num_qubits=1, meas_bases=bases, native=native)
        device = model_device(self._model)
        if device is not None:
            model_input = model_input.to(device)
        with torch.no_grad():
            out = self._model(model_input).reshape(len(rows), -1)[:, 0].cpu().tolist()
        totals = [0.0] * len(circuits)
        for k, o, c in zip(owners, out, coeffs):
            totals[k] = totals[k] + o * c
        return totals


class ScikitLearningModelProcessor(LearningMethodEstimatorProcessor):
    """The same per-term ``encode_data`` rows into anything with scikit-learn's ``predict`` (reference :90-148; the
    demos fit ``RandomForestRegressor`` / OLS on these rows).  Host CPU only: there is no tensor work to move."""

    def __init__(self, model, backend):
        if not hasattr(model, "predict"):
            raise BlackwaterException("ScikitLearningModelProcessor needs a fitted estimator with .predict(X)")
        self._model = model
        self._backend = backend
        self._properties = get_backend_properties_v1(backend)

    def process(self, expectation_value, circuits, observables, parameter_values):
        total = 0.0
        for term in observables:
            row, _ = encode_data(circuits=[circuits], properties=self._properties, ideal_exp_vals=[[0.0]],
                                 noisy_exp_vals=[[expectation_value]], num_qubits=1,
                                 meas_bases=encode_pauli_sum_op([(str(term.paulis[0]), 1.0)]))
            output = float(np.ravel(self._model.predict(row.numpy()))[0])
            total = total + output * float(np.real(term.coeffs[0]))
        return total


class _DeviceRegressorProcessor(LearningMethodEstimatorProcessor):
    """What the device-side scikit-learn replacements share: the per-term ``encode_data`` rows of
    ``ScikitLearningModelProcessor``, all (circuit, Pauli term) rows of a ``run()`` through ONE ``self._model.predict`` launch,
    ``output[:, 0] * coeff`` summed per circuit.  Subclasses set ``_model`` (a module on ``_device``), ``_device``, ``_backend`` and
    ``_properties``."""

    accepts_qasm_text = True     # process_batch scans OpenQASM text natively: PostProcessedJob hands text over unparsed

    def _score(self, rows: torch.Tensor) -> np.ndarray:
        """First output of the model for every row (float64, as scikit-learn's ``predict`` returns it)."""
        out = self._model.predict(rows.to(self._device, dtype=torch.float32))
        return out.reshape(rows.shape[0], -1)[:, 0].cpu().numpy()

    def process(self, expectation_value, circuits, observables, parameter_values):
        total = 0.0
        for term in observables:
            row, _ = encode_data(circuits=[circuits], properties=self._properties, ideal_exp_vals=[[0.0]],
                                 noisy_exp_vals=[[expectation_value]], num_qubits=1,
                                 meas_bases=encode_pauli_sum_op([(str(term.paulis[0]), 1.0)]), native=isinstance(circuits, str))
            total = total + float(self._score(row)[0]) * float(np.real(term.coeffs[0]))
        return total

    def process_batch(self, expectation_values, circuits, observables, parameter_values):
        """All (circuit, Pauli term) rows of one ``run()`` through ONE launch; results equal ``process`` applied circuit by
        circuit (the same rows, the same per-circuit order of the sum)."""
        rows, owners, coeffs, values, bases = [], [], [], [], []
        for k, (value, circuit, obs) in enumerate(zip(expectation_values, circuits, observables)):
            for term in obs:
                rows.append(circuit)
                owners.append(k)
                coeffs.append(float(np.real(term.coeffs[0])))
                values.append([float(value)])
                bases.append(encode_pauli_sum_op([(str(term.paulis[0]), 1.0)])[0])
        if not rows:
            return [0.0] * len(circuits)
        native = all(isinstance(c, str) for c in rows)
        model_input, _ = encode_data(circuits=rows, properties=self._properties, ideal_exp_vals=[[0.0]] * len(rows),
                                     noisy_exp_vals=values, num_qubits=1, meas_bases=bases, native=native)
        out = self._score(model_input).tolist()
        totals = [0.0] * len(circuits)
        for k, o, c in zip(owners, out, coeffs):
            totals[k] = totals[k] + o * c
        return totals


class ForestLearningModelProcessor(_DeviceRegressorProcessor):
    """The random-forest mitigator of the reference's demos and VQE drivers (``ScikitLearningModelProcessor(rfr, backend)``,
    reference :90-148) scored on the device: the same per-term ``encode_data`` rows, all (circuit, Pauli term) rows of a ``run()``
    through ONE launch of the forest kernel (``blackwater.nn.ForestRegressor``), ``output[:, 0] * coeff`` summed per circuit.

    ``model``: a fitted scikit-learn ``RandomForestRegressor`` / ``ExtraTreesRegressor`` / ``DecisionTreeRegressor`` (converted with
    ``ForestRegressor.from_sklearn``) or a ``ForestRegressor``.  There is no host path: ``device`` must be a GPU."""

    def __init__(self, model, backend, device="cuda"):
        from ...nn.forest import ForestRegressor

        if not isinstance(model, ForestRegressor):
            model = ForestRegressor.from_sklearn(model)   # BlackwaterException for anything that is not a fitted regression forest
        self._model = model.to(device)
        self._device = torch.device(device)
        self._backend = backend
        self._properties = get_backend_properties_v1(backend)


class LinearLearningModelProcessor(_DeviceRegressorProcessor):
    """The OLS mitigator of the reference's tutorials and VQE drivers (``ScikitLearningModelProcessor(ols, backend)``, reference
    :90-148) scored on the device: the same per-term ``encode_data`` rows, all (circuit, Pauli term) rows of a ``run()`` through ONE
    launch of the least-squares predict kernel (``blackwater.nn.LinearRegressor``), ``output[:, 0] * coeff`` summed per circuit.

    ``model``: a fitted scikit-learn ``LinearRegression`` / ``Ridge`` (converted with ``LinearRegressor.from_sklearn``) or a
    ``LinearRegressor`` (``LinearRegressor.fit`` fits one on the device).  There is no host path: ``device`` must be a GPU."""

    def __init__(self, model, backend, device="cuda"):
        from ...nn.linear_model import LinearRegressor

        if not isinstance(model, LinearRegressor):
            model = LinearRegressor.from_sklearn(model)   # BlackwaterException for anything that is not a fitted linear model
        self._model = model.to(device)
        self._device = torch.device(device)
        self._backend = backend
        self._properties = get_backend_properties_v1(backend)


class BoostedLearningModelProcessor(_DeviceRegressorProcessor):
    """A gradient-boosted mitigator (``ScikitLearningModelProcessor(GradientBoostingRegressor().fit(...), backend)``, reference
    :90-148; the notebooks import it beside the random forest) scored on the device: the same per-term ``encode_data`` rows, all
    (circuit, Pauli term) rows of a ``run()`` through ONE launch of the boosted-trees kernel (``blackwater.nn.BoostedRegressor``),
    ``output * coeff`` summed per circuit.

    ``model``: a fitted scikit-learn ``GradientBoostingRegressor`` with squared-error loss (converted with
    ``BoostedRegressor.from_sklearn``) or a ``BoostedRegressor`` (``BoostedRegressor.fit`` fits one on the device).  There is no host
    path: ``device`` must be a GPU."""

    def __init__(self, model, backend, device="cuda"):
        from ...nn.boost import BoostedRegressor

        if not isinstance(model, BoostedRegressor):
            model = BoostedRegressor.from_sklearn(model)   # BlackwaterException for anything that is not a fitted squared-error ensemble
        self._model = model.to(device)
        self._device = torch.device(device)
        self._backend = backend
        self._properties = get_backend_properties_v1(backend)


class ZNEProcessor(LearningMethodEstimatorProcessor):
    """Zero-noise extrapolation as a processor (reference :33-86): the value handed in is ignored, the circuit is run again through
    ``zne_estimator`` (an INSTANCE of a ``blackwater.zne.zne(cls)`` class) with ``zne_strategy`` and the extrapolated value is
    returned.  ``process_batch`` sends all circuits of a ``run()`` through one ``zne_estimator.run``: around
    ``blackwater.sim.DeviceEstimator`` that is one lowering and one fused launch for every (circuit, noise factor) pair.

    Circuits arrive bound and on physical qubits, with observables as wide as the circuit (wrap with ``skip_transpile=True``).  The
    reference transpiles at optimisation level 0, appends measurements and re-maps a 2-qubit observable onto 5 physical qubits
    through the last two measurements, all hard-coded; none of that is reproduced here.  ``backend`` is kept for the reference's
    constructor; ``shots``, when given, is passed on as a run option: around ``blackwater.sim.DeviceEstimator`` every (circuit, noise
    factor) run is then measured with that many shots per measurement basis and the SAMPLED values are extrapolated (the job's
    metadata carries ``variance``, ``shots`` and ``std_error``); without it the values are exact."""

    accepts_qasm_text = True     # the ZNE estimator takes OpenQASM text as it comes

    def __init__(self, zne_estimator, zne_strategy, backend=None, shots=None):
        if not hasattr(zne_estimator, "run"):
            raise BlackwaterException("ZNEProcessor needs an estimator instance with .run(circuits, observables, zne_strategy=...)")
        self._zne_estimator = zne_estimator
        self._zne_strategy = zne_strategy
        self._backend = backend
        self._shots = shots

    def _values(self, circuits, observables, parameter_values):
        options = {"zne_strategy": self._zne_strategy}
        if self._shots is not None:
            options["shots"] = self._shots
        job = self._zne_estimator.run(circuits, observables, parameter_values, **options)
        return np.asarray(job.result().values, dtype=np.float64)

    def process(self, expectation_value, circuits, observables, parameter_values):
        return float(self._values([circuits], [observables], None)[0])

    def process_batch(self, expectation_values, circuits, observables, parameter_values):
        """All circuits of one ``run()`` through ONE ZNE run; results equal ``process`` applied circuit by circuit (a run's bits
        do not depend on the batch).  The circuits arrive bound, so no parameter values are passed on."""
        if not circuits:
            return []
        return self._values(list(circuits), list(observables), None).tolist()


class EmptyProcessor(LearningMethodEstimatorProcessor):
    def process(self, expectation_value, circuits, observables, parameter_values):
        return expectation_value


def _options_dict(options) -> dict:
    if options is None:
        return {}
    return dict(options.__dict__) if hasattr(options, "__dict__") and not isinstance(options, dict) else dict(options)


class PostProcessedJob(job_base()):  # type: ignore[misc]
    def __init__(self, base_job, processor: LearningMethodEstimatorProcessor, circuits, observables, parameter_values,
                 skip_transpile: bool, backend, job_id: str, options=None, **kwargs) -> None:
        try:
            super().__init__(backend, job_id, **kwargs)
        except TypeError:  # plain ``object`` base when qiskit is absent
            self._backend, self._job_id = backend, job_id
        self._base_job = base_job
        self._processor = processor
        self._circuits = circuits
        self._observables = observables
        self._parameter_values = parameter_values
        self._options = options
        self._skip_transpile = skip_transpile
        self._wrapped_backend = backend

    def result(self):
        result = self._base_job.result()
        mitigated, metadata = [], []
        batch_fn = getattr(self._processor, "process_batch", None)
        bound_all = []
        for value, circuit, obs, params, meta in zip(result.values, self._circuits, self._observables,
                                                     self._parameter_values, result.metadata):
            if not is_pauli_observable(obs):
                raise BlackwaterException("Only `PauliSumOp` observables are supported by learning primitive.")
            opts = dict(optimization_level=3, **_options_dict(self._options))
            bound = transpile_and_bind(circuit, self._wrapped_backend, params, opts, do_transpile=not self._skip_transpile,
                                       keep_text=batch_fn is not None and getattr(self._processor, "accepts_qasm_text", False))
            metadata.append({**meta, "original_value": value})
            if batch_fn is not None:
                bound_all.append(bound)
                continue
            mitigated.append(self._processor.process(expectation_value=value, circuits=bound, observables=obs,
                                                     parameter_values=params))
        if batch_fn is not None and bound_all:
            mitigated = batch_fn(list(result.values), bound_all, list(self._observables), list(self._parameter_values))
        return make_estimator_result(np.array(mitigated), metadata)

    def submit(self):
        return self._base_job.submit()

    def status(self):
        return self._base_job.status()

    def cancel(self):
        return self._base_job.cancel()

    def __repr__(self):
        return f"<NgemJob: {self._base_job.job_id()}>"  # sic: the reference prints this name here too (:258-259)


def patch_run(run: Callable, processor: LearningMethodEstimatorProcessor, skip_transpile: bool, backend=None,
              options=None) -> Callable:
    @wraps(run)
    def patched_run(self, circuits, observables, parameter_values, **run_options):
        job = run(self, circuits=circuits, observables=observables, parameter_values=parameter_values, **run_options)
        return PostProcessedJob(job, job_id=job.job_id(), backend=backend, processor=processor, circuits=circuits,
                                observables=observables, parameter_values=parameter_values,
                                skip_transpile=skip_transpile, options=options)

    return patched_run


def learning(cls: Type, processor: LearningMethodEstimatorProcessor, skip_transpile: bool = False, backend=None,
             options=None):
    """Decorator turning an Estimator class into ``Learning<cls.__name__>``."""
    new_class: type = type(f"Learning{cls.__name__}", (cls,), {})
    new_class._run = patch_run(new_class._run, processor, skip_transpile, backend, options)  # type: ignore[attr-defined]
    return new_class
