"""Batched exact simulation of small circuits on the device: ideal (state vector) and noisy (density matrix) expectation values,
the labels the mitigators learn from.  ``compile_programs`` / ``NoiseModel`` / ``measured_z`` run on the host alone."""
from .program import (MAX_AMPS, MAX_QUBITS_DENSITY, MAX_QUBITS_VECTOR, SUPPORTED_GATES, WAVE_AMPS, NoiseModel, SimBatch,
                      compile_programs, measured_z)
from .run import DeviceEstimator, SimulatedJob, expectation_values, run_batch

__all__ = ["MAX_AMPS", "MAX_QUBITS_DENSITY", "MAX_QUBITS_VECTOR", "SUPPORTED_GATES", "WAVE_AMPS", "NoiseModel", "SimBatch",
           "compile_programs", "measured_z", "DeviceEstimator", "SimulatedJob", "expectation_values", "run_batch"]
