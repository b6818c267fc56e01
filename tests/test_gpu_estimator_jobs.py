"""The one job path of ``DeviceEstimator`` and of ``zne(DeviceEstimator)`` on the device, method by method: two successive jobs of one
estimator have the ids ``sim-1`` / ``sim-2``, the metadata keys the class docstring states, in that order, and the second job's values
and numeric metadata are bit-equal to the method's public entry point called with the run keys ``2 * 2^32 + k`` and the same seed.
Two circuits of 3 qubits on a line, 64 shots, 4 trajectories, bond 4: the kernels are tested elsewhere, the front end here."""
import math

import numpy as np
import pytest

from blackwater import sim
from blackwater.data.synthetic import clifford_tfim_circuit, tfim_circuit, tfim_circuit_template
from blackwater.sim import zne

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHOTS, TRAJECTORIES, BOND, SEED = 64, 4, 4, 7
CIRCUITS = [tfim_circuit(3, 1, J=0.3, two_q="cx"), tfim_circuit(3, 2, J=0.7, two_q="cx")]
CLIFFORDS = [clifford_tfim_circuit(3, 1, 1, 1, two_q="cx"), clifford_tfim_circuit(3, 2, 1, 3, two_q="cx")]
TEMPLATES = [tfim_circuit_template(3, 1), tfim_circuit_template(3, 2)]
ROWS = [(0.4, -0.3), (1.1, 0.6)]
OBSERVABLES = ["IIZ", [("ZZI", 0.5), ("IZI", -1.0)]]   # Z alone: the Clifford path takes them beside readout noise
NOISE = sim.NoiseModel({("cx", (0, 1)): 0.03, ("sx", (0,)): 0.002, ("sx", (1,)): 0.003, ("sx", (2,)): 0.001},
                       {0: (0.02, 0.03), 1: (0.01, 0.04), 2: (0.03, 0.01)}, name="depolarising + readout")
SAMPLED, MPS, NOISY = ["variance", "shots"], ["truncation_error_bound", "max_bond"], ["std_error", "trajectories"]


def host(t):
    return t.cpu().numpy()


def _sampled(res):
    return res.values, {"variance": res.variance}


def _mps(res, noisy, std_error=True):
    return {"truncation_error_bound": res.error_bound, "max_bond": res.bond, **({"std_error": res.std_error} if noisy and std_error else {})}


def _direct_mps(noise, keys, **kw):
    res = sim.mps_expectation_values(CIRCUITS, OBSERVABLES, noise, max_bond=BOND, trajectories=TRAJECTORIES if noise else None, seed=SEED,
                                     run_keys=keys, device=DEV, **kw)
    return res.values, _mps(res, noise is not None)


def _direct_mps_shots(noise, keys):
    res = sim.sample_mps_expectation_values(CIRCUITS, OBSERVABLES, noise, shots=SHOTS, trajectories=TRAJECTORIES if noise else None,
                                            max_bond=BOND, seed=SEED, run_keys=keys, device=DEV)
    return res.values, {"variance": res.variance, **_mps(res, noise is not None, std_error=False)}


def _direct_bound_mps(noise, keys):
    values, _, res = sim.bound_mps_expectation_values(TEMPLATES, OBSERVABLES, ROWS, noise, TRAJECTORIES if noise else None, BOND,
                                                      seed=SEED, run_keys=keys, device=DEV, return_result=True)
    return values, _mps(res, noise is not None)


def _direct_trajectories(noise, keys):
    res = sim.trajectory_expectation_values(CIRCUITS, OBSERVABLES, noise, trajectories=TRAJECTORIES, seed=SEED, run_keys=keys, device=DEV)
    return res.values, {"std_error": res.std_error}


# id: (constructor kwargs, noisy?, the job's circuits, its parameter rows, metadata keys, the entry point on (noise, keys))
CASES = {
    "exact": (dict(), True, CIRCUITS, None, [], lambda noise, keys: (sim.expectation_values(CIRCUITS, OBSERVABLES, noise, DEV)[0], {})),
    "exact-shots": (dict(shots=SHOTS), True, CIRCUITS, None, SAMPLED, lambda noise, keys: _sampled(
        sim.sample_expectation_values(CIRCUITS, OBSERVABLES, noise, shots=SHOTS, seed=SEED, run_keys=keys, device=DEV))),
    "clifford": (dict(method="clifford"), True, CLIFFORDS, None, [],
                 lambda noise, keys: (sim.clifford_expectation_values(CLIFFORDS, OBSERVABLES, noise, DEV)[0], {})),
    "frames": (dict(method="frames", shots=SHOTS), True, CLIFFORDS, None, SAMPLED, lambda noise, keys: _sampled(
        sim.sample_clifford_expectation_values(CLIFFORDS, OBSERVABLES, noise, shots=SHOTS, seed=SEED, run_keys=keys, device=DEV))),
    "trajectories": (dict(method="trajectories", trajectories=TRAJECTORIES), True, CIRCUITS, None, NOISY, _direct_trajectories),
    "mps": (dict(method="mps", max_bond=BOND), False, CIRCUITS, None, MPS, _direct_mps),
    "mps-noise": (dict(method="mps", max_bond=BOND, trajectories=TRAJECTORIES), True, CIRCUITS, None, MPS + NOISY, _direct_mps),
    "mps_shots": (dict(method="mps_shots", shots=SHOTS, max_bond=BOND), False, CIRCUITS, None, SAMPLED + MPS, _direct_mps_shots),
    "mps_shots-noise": (dict(method="mps_shots", shots=SHOTS, max_bond=BOND, trajectories=TRAJECTORIES), True, CIRCUITS, None,
                        SAMPLED + MPS + ["trajectories"], _direct_mps_shots),
    "bound-exact": (dict(), True, TEMPLATES, ROWS, [],
                    lambda noise, keys: (sim.bound_expectation_values(TEMPLATES, OBSERVABLES, ROWS, noise, DEV)[0], {})),
    "bound-mps": (dict(method="mps", max_bond=BOND), False, TEMPLATES, ROWS, MPS, _direct_bound_mps),
    "bound-mps-noise": (dict(method="mps", max_bond=BOND, trajectories=TRAJECTORIES), True, TEMPLATES, ROWS, MPS + NOISY, _direct_bound_mps),
}
CONSTANTS = {"shots": SHOTS, "trajectories": TRAJECTORIES}   # the metadata fields that are the estimator's own settings


@pytest.mark.parametrize("name", list(CASES))
def test_two_successive_jobs(name):
    kwargs, noisy, circuits, rows, keys, direct = CASES[name]
    noise = NOISE if noisy else None
    est = sim.DeviceEstimator(noise, DEV, seed=SEED, **kwargs)
    first, second = est.run(circuits, OBSERVABLES, rows), est.run(circuits, OBSERVABLES, rows)
    assert (first.job_id(), second.job_id()) == ("sim-1", "sim-2") and est._count == 2
    for result in (first.result(), second.result()):
        assert [list(m) for m in result.metadata] == [keys, keys]
    want_values, want = direct(noise, sim.default_run_keys(2, 2 << 32))
    got = second.result()
    assert np.array_equal(got.values, host(want_values)) and got.values.shape == (2,)
    assert set(want) | set(CONSTANTS) >= set(keys)
    for key in keys:
        column = [m[key] for m in got.metadata]
        assert column == ([CONSTANTS[key]] * 2 if key in CONSTANTS else host(want[key]).tolist()), key


BASE = ["noise_factors", "achieved_factors", "values", "noise_amplifier", "extrapolator"]
# id: (constructor kwargs, the keyword arguments of zne_run beside run_keys, metadata keys, the keys of metadata["zne"])
ZNE_CASES = {
    "exact": (dict(), dict(), ["zne"], BASE),
    "exact-shots": (dict(shots=SHOTS), dict(shots=SHOTS, seed=SEED), ["zne", "variance", "shots", "std_error"], BASE + ["variances"]),
    "mps-noise": (dict(method="mps", max_bond=BOND, trajectories=TRAJECTORIES),
                  dict(method="mps", max_bond=BOND, trajectories=TRAJECTORIES, seed=SEED),
                  ["zne", "trajectories", "std_error", "truncation_error_bound"], BASE + ["std_errors", "truncation_error_bounds"]),
}


@pytest.mark.parametrize("name", list(ZNE_CASES))
def test_two_successive_zne_jobs(name):
    kwargs, run_kwargs, keys, zne_keys = ZNE_CASES[name]
    strategy = zne.ZNEStrategy(noise_factors=(1, 3))
    est = zne.zne(sim.DeviceEstimator)(NOISE, DEV, seed=SEED, zne_strategy=strategy, **kwargs)
    first, second = est.run(CIRCUITS, OBSERVABLES), est.run(CIRCUITS, OBSERVABLES)
    assert (first.job_id(), second.job_id()) == ("zne-sim-1", "zne-sim-2") and est._zne_count == 2
    got = second.result()
    assert [list(m) for m in got.metadata] == [keys, keys] and [list(m["zne"]) for m in got.metadata] == [zne_keys, zne_keys]
    want = zne.zne_run(CIRCUITS, OBSERVABLES, NOISE, strategy, DEV, run_keys=np.arange(2 * 2, dtype=np.int64) + (2 << 32), **run_kwargs)
    assert np.array_equal(got.values, host(want.mitigated_values))
    per_factor = host(want.values)
    assert [m["zne"]["values"] for m in got.metadata] == [tuple(per_factor[:, k].tolist()) for k in range(2)]
    if name == "exact-shots":
        assert [m["variance"] for m in got.metadata] == host(want.mitigated_variance).tolist() and got.metadata[0]["shots"] == SHOTS
        assert [m["std_error"] for m in got.metadata] == [math.sqrt(max(v, 0.0) / SHOTS) for v in host(want.mitigated_variance).tolist()]
    if name == "mps-noise":
        assert [m["std_error"] for m in got.metadata] == host(want.mitigated_std_error).tolist() and got.metadata[0]["trajectories"] == TRAJECTORIES
