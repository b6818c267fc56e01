"""Zero-noise extrapolation under the name the reference imports it by (``from zne import zne, ZNEStrategy``,
``from zne.noise_amplification import LocalFoldingAmplifier``, ``from zne.extrapolation import LinearExtrapolator``): everything
lives in :mod:`blackwater.sim.zne`."""
from .sim.zne import *  # noqa: F401,F403
from .sim.zne import (CubicExtrapolator, CxAmplifier, ExponentialExtrapolator, GlobalFoldingAmplifier, LinearExtrapolator, LocalFoldingAmplifier,  # noqa: F401
                      PolynomialExtrapolator, QuadraticExtrapolator, QuarticExtrapolator, RichardsonExtrapolator, Schedules,
                      TwoQubitAmplifier, ZNEJob, ZNERun, ZNEStrategy, achieved_factor, build_clifford_schedules, build_mps_schedules, build_schedules, fold_circuit, fold_counts,
                      inverse_op, run_mps_folded, zne, zne_expectation_values, zne_run)
