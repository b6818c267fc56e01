"""Batched exact simulation of small circuits on the device: ideal (state vector) and noisy (density matrix) expectation values,
the labels the mitigators learn from.  ``compile_programs`` / ``NoiseModel`` / ``measured_z`` run on the host alone.  ``blackwater.sim.zne`` (also ``blackwater.zne``) is
zero-noise extrapolation on it; the ``zne(cls)`` decorator lives there, so that ``sim.zne`` stays the module.
``run_trajectories`` / ``trajectory_expectation_values`` are the path for NOISY circuits of 6 to 11 qubits (any gate, any
``NoiseModel``): pure-state quantum trajectories, a mean and its standard error.
``blackwater.sim.clifford`` is the path for wide circuits: Clifford circuits of up to 512 qubits, ideal and noisy, by carrying the
observable backwards through the circuit (``compile_clifford`` / ``clifford_expectation_values``); ``zne_run(..., method="clifford")``
extrapolates there too (``build_clifford_schedules``, ``ExponentialExtrapolator``).
``blackwater.sim.frames`` draws measurement SHOTS there: Pauli-frame sampling of Clifford circuits under the depolarising + readout
model (``compile_clifford_frames`` / ``sample_clifford_expectation_values`` / ``frame_counts``), bit strings of up to 512 qubits.
``Template`` / ``Param`` / ``compile_templates`` are parameterised circuits: one template lowered once, bound on the device at many
parameter vectors (``bound_expectation_values``), with exact gradients by the parameter-shift rule (``parameter_shift``).
``blackwater.sim.mps`` is the path for wide circuits that are NOT Clifford circuits: matrix-product states of bond at most 32 for
circuits on a line (``compile_mps`` / ``run_mps`` / ``mps_expectation_values``; measurement shots from the same states:
``compile_mps_shots`` / ``run_mps_shots`` / ``sample_mps_expectation_values`` / ``mps_counts``), exact while the bonds fit and certified beyond, ideal
and, by Pauli-insertion trajectories, under a depolarising + readout model.  Templates run there too: ``compile_mps_templates`` lowers
an ansatz of up to 512 qubits once, ``run_mps_bound`` / ``bound_mps_expectation_values`` bind it on the device for every parameter row
and ``parameter_shift(..., method="mps")`` gives its gradients."""
from .program import (MAX_AMPS, MAX_QUBITS_DENSITY, MAX_QUBITS_VECTOR, SUPPORTED_GATES, WAVE_AMPS, NoiseModel, SimBatch,
                      compile_programs, measured_z)
from .program import MAX_SHOTS, measurement_groups
from .program import MAX_TRAJECTORIES
from .clifford import (MAX_QUBITS_CLIFFORD, CliffordBatch, clifford_expectation_values, compile_clifford, invert_table, is_clifford,
                       run_clifford, run_clifford_folded)
from .run import (DeviceEstimator, SampleResult, SimulatedJob, counts_dicts, default_run_keys, expectation_values, run_batch,
                  sample_batch, sample_expectation_values)
from .run import TrajectoryResult, run_trajectories, trajectory_expectation_values
from .frames import (MAX_GROUPS, FrameBatch, FrameResult, compile_clifford_frames, frame_counts, run_clifford_frames,
                     sample_clifford_expectation_values)
from .template import BoundBatch, Param, Template, compile_templates
from .bound import bound_expectation_values, parameter_shift, run_bound
from .mps import (MAX_BOND, MAX_GROUPS_MPS, MAX_QUBITS_MPS, MPS_BUFFER_BYTES, MpsBatch, MpsResult, MpsShotsBatch, MpsShotsResult,
                  compile_mps, compile_mps_shots, is_line_circuit, mps_counts, mps_expectation_values, run_mps, run_mps_shots,
                  sample_mps_expectation_values)
from .mps import MpsBoundBatch, MpsBoundRun, bound_mps_expectation_values, compile_mps_templates, run_mps_bound
from .zne import (CubicExtrapolator, CxAmplifier, ExponentialExtrapolator, GlobalFoldingAmplifier, LinearExtrapolator, LocalFoldingAmplifier,
                  PolynomialExtrapolator, QuadraticExtrapolator, QuarticExtrapolator, RichardsonExtrapolator, Schedules,
                  TwoQubitAmplifier, ZNEStrategy, build_clifford_schedules, build_mps_schedules, build_schedules, fold_circuit,
                  run_mps_folded, zne_expectation_values, zne_run)

__all__ = ["MAX_AMPS", "MAX_QUBITS_DENSITY", "MAX_QUBITS_VECTOR", "SUPPORTED_GATES", "WAVE_AMPS", "NoiseModel", "SimBatch",
           "compile_programs", "measured_z", "DeviceEstimator", "SimulatedJob", "expectation_values", "run_batch",
           "CubicExtrapolator", "CxAmplifier", "GlobalFoldingAmplifier", "LinearExtrapolator", "LocalFoldingAmplifier",
           "PolynomialExtrapolator", "QuadraticExtrapolator", "QuarticExtrapolator", "RichardsonExtrapolator", "Schedules",
           "TwoQubitAmplifier", "ZNEStrategy", "build_schedules", "fold_circuit", "zne_expectation_values", "zne_run",
           "MAX_SHOTS", "measurement_groups", "SampleResult", "counts_dicts", "default_run_keys", "sample_batch",
           "sample_expectation_values", "MAX_QUBITS_CLIFFORD", "CliffordBatch", "clifford_expectation_values", "compile_clifford",
           "is_clifford", "run_clifford", "ExponentialExtrapolator", "build_clifford_schedules", "invert_table", "run_clifford_folded",
           "MAX_TRAJECTORIES", "TrajectoryResult", "run_trajectories", "trajectory_expectation_values",
           "MAX_GROUPS", "FrameBatch", "FrameResult", "compile_clifford_frames", "frame_counts", "run_clifford_frames",
           "sample_clifford_expectation_values",
           "MAX_BOND", "MAX_QUBITS_MPS", "MPS_BUFFER_BYTES", "MpsBatch", "MpsResult", "compile_mps", "is_line_circuit",
           "mps_expectation_values", "run_mps", "MAX_GROUPS_MPS", "MpsShotsBatch", "MpsShotsResult", "compile_mps_shots", "mps_counts",
           "run_mps_shots", "sample_mps_expectation_values", "build_mps_schedules", "run_mps_folded",
           "BoundBatch", "Param", "Template", "compile_templates", "bound_expectation_values", "parameter_shift", "run_bound",
           "MpsBoundBatch", "MpsBoundRun", "bound_mps_expectation_values", "compile_mps_templates", "run_mps_bound"]
