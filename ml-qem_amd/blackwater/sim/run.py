"""Device side of the batched simulator: one call of ``mlqem_sim_run_f64`` per batch, measurement shots on top of it
(``mlqem_sim_run_measured_f64`` + ``mlqem_sim_sample_f64``), quantum trajectories for noisy circuits past the density-matrix cap
(``mlqem_sim_run_trajectories_f64``), and an Estimator-shaped primitive on all three."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from ..library.primitives import make_estimator_result
from ..data.circuit import Circuit
from .clifford import clifford_expectation_values, is_clifford, refuse_non_pauli
from .frames import sample_clifford_expectation_values
from .program import (MAX_QUBITS_DENSITY, MAX_QUBITS_VECTOR, NoiseModel, SimBatch, _run_keys, check_seed, check_shots, check_trajectories,
                      compile_programs, default_run_keys, upload)
from .bound import bound_expectation_values
from .mps import (DEFAULT_CUTOFF, MAX_BOND, _check_bond, _check_cutoff, _check_twirl, bound_mps_expectation_values, mps_expectation_values,
                  sample_mps_expectation_values)
from .template import Template, has_free_parameters


def run_batch(batch: SimBatch, device="cuda"):
    """``(values, term_values, norm)`` of a lowered batch: float64 tensors on ``device``."""
    from ..native import ops

    batch.refuse_trajectories("run_batch")
    t = batch.to(device)
    return ops.sim_run(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"],
                       t["n_wave"], t["n_wg"])


def expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None, device="cuda"):
    """Exact expectation values of ``observables[k]`` after ``circuits[k]``: ``(values, term_values, term_ptr)``, float64 [B],
    float64 [n_terms] and int64 [B + 1] tensors on ``device`` (``term_values[term_ptr[k] : term_ptr[k + 1]]`` are the Pauli terms
    of circuit k, without their coefficients).  ``noise=None`` simulates state vectors, a :class:`NoiseModel` density matrices;
    everything is lowered and validated on the host first (:func:`compile_programs`), then simulated in at most two launches."""
    batch = compile_programs(circuits, observables, noise)
    values, term_values, _ = run_batch(batch, device)
    return values, term_values, upload(batch.term_ptr, values.device)


@dataclass
class SampleResult:
    """What one sampled call produced: tensors on the device, CSR over ``term_ptr`` (terms of a circuit), ``group_ptr`` (measurement
    groups of a circuit) and ``prob_ptr`` (the 2^n outcomes of a group; outcome j is the measured bit string as an integer, qubit 0
    the least significant bit).  Folded runs carry a leading noise-factor axis on everything but the pointers."""

    values: Any          # float64 [B]: sum coeff * sampled term estimate
    variance: Any        # float64 [B]: sum coeff^2 (1 - estimate^2), per term: no covariances between the terms of a group
    term_values: Any     # float64 [n_terms]: the sampled Pauli-term estimates
    term_ptr: Any        # int64 [B + 1]
    counts: Any          # int32 [n_outcomes]
    prob_ptr: Any        # int64 [n_groups + 1]
    group_ptr: Any       # int64 [B + 1]
    probs: Any           # float64 [n_outcomes]: the exact outcome probabilities the counts were drawn from
    shots: int = 0
    seed: int = 0
    exact_values: Any = None        # float64 [B]: the exact expectation values of the same launch
    exact_term_values: Any = None   # float64 [n_terms]
    norm: Any = None
    batch: Optional[SimBatch] = None


def sample_batch(batch: SimBatch, seed: int = 0, run_keys=None, device="cuda") -> SampleResult:
    """Simulates a batch lowered with ``shots`` and samples it: two calls (at most five launches), nothing read back."""
    from ..native import ops

    batch.refuse_trajectories("sample_batch")
    if batch.group_ptr is None:
        raise ValueError("sample_batch: the batch was lowered without shots (compile_programs(..., shots=))")
    seed = check_seed(seed, "sample_batch")
    keys = upload(_run_keys(run_keys, len(batch), "sample_batch"), device)
    t = batch.to(device)
    units, n_wave, n_wg = batch.sample_units(1)
    n_outcomes = int(batch.prob_ptr[-1])
    values, term_values, norm, probs = ops.sim_run_measured(
        t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["prob_ptr"], n_outcomes,
        t["ids"], t["n_wave"], t["n_wg"])
    s_values, variance, s_terms, counts = ops.sim_sample(
        t["circ"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["term_group"], t["prob_ptr"], t["group_circ"], probs, keys,
        batch.shots, seed, upload(units, keys.device), n_wave, n_wg)
    return SampleResult(s_values, variance, s_terms, t["term_ptr"], counts, t["prob_ptr"], t["group_ptr"], probs, batch.shots, seed,
                        values, term_values, norm, batch)


def sample_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None, shots: int = None,
                              seed: int = 0, run_keys=None, device="cuda") -> SampleResult:
    """Expectation values estimated from ``shots`` measurement outcomes per measurement basis, drawn on the device.

    The circuits are lowered with their terms partitioned into qubit-wise commuting groups (``compile_programs(..., shots=)``),
    simulated exactly, and every group's outcome distribution is sampled ``shots`` times (a Philox4x32-10 stream per (seed, run
    key, group, shot): include/mlqem_hip.h has the rule).  ``run_keys``: one integer per circuit, by default its position in the
    batch; pass a circuit's batch key to draw the same shots for it alone.  Returns a :class:`SampleResult`."""
    if shots is None:
        raise ValueError("sample_expectation_values: shots is required (an int in 1 .. 2^20); expectation_values gives the exact values")
    shots = check_shots(shots, "sample_expectation_values")
    return sample_batch(compile_programs(circuits, observables, noise, shots=shots), seed, run_keys, device)


@dataclass
class TrajectoryResult:
    """What one trajectory run produced: tensors on the device, the terms CSR over ``term_ptr``."""

    values: Any            # float64 [B]: the mean over the trajectories of sum coeff * term
    std_error: Any         # float64 [B]: sqrt(M2 / (T (T - 1))) of the per-trajectory values; 0 at T = 1
    term_values: Any       # float64 [n_terms]: the mean of every Pauli term
    term_std_error: Any    # float64 [n_terms]
    norm: Any              # float64 [B]: the mean of <psi|psi> at the end of a trajectory (1 up to rounding)
    term_ptr: Any          # int64 [B + 1]
    trajectories: int = 0
    seed: int = 0
    traj_term_values: Any = None   # float64 [T, n_terms] with ``keep_trajectories``: row t holds trajectory t of every circuit
    batch: Optional[SimBatch] = None


TRAJECTORY_BUFFER_BYTES = 256 << 20   # the per-trajectory buffers of one call stay under this (``buffer_bytes=``)


def _trajectory_chunks(batch: SimBatch, trajectories: int, buffer_bytes: int) -> List[range]:
    """Contiguous ranges of circuits whose per-trajectory buffers (T x (terms + circuits) float64) fit ``buffer_bytes`` and whose
    (circuit, trajectory) units fit one call; a range holds at least one circuit."""
    budget = max(int(buffer_bytes) // (8 * trajectories), 1)          # term and norm columns per call
    most = max((2 ** 31 - 1) // trajectories, 1)                      # circuits per call
    chunks, lo = [], 0
    n_circ = len(batch)
    while lo < n_circ:
        hi = lo + 1
        while hi < n_circ and hi - lo < most and int(batch.term_ptr[hi + 1] - batch.term_ptr[lo]) + (hi + 1 - lo) <= budget:
            hi += 1
        chunks.append(range(lo, hi))
        lo = hi
    return chunks


def run_trajectories(batch: SimBatch, seed: int = 0, run_keys=None, device="cuda", keep_trajectories: bool = False,
                     buffer_bytes: int = TRAJECTORY_BUFFER_BYTES) -> TrajectoryResult:
    """Runs a batch lowered with ``trajectories`` (``compile_programs(..., noise, trajectories=T)``): every circuit as T pure-state
    trajectories on the device, one Kraus operator drawn at every noise record (include/mlqem_hip.h has the unravelling), and
    the means and standard errors over them.  ``run_keys``: one integer per circuit, by default its position in the batch; a
    trajectory's bits depend on (seed, run key, trajectory number, circuit) alone, so a circuit gives the same values alone and
    in a batch, and the first T trajectories of a longer run are the same.  The batch is split by circuits so that the
    per-trajectory buffers of a call stay under ``buffer_bytes``; the results do not depend on the split.
    ``keep_trajectories``: also return ``traj_term_values`` [T, n_terms] (the whole buffer: it is then as large as it is)."""
    import torch

    from ..native import ops

    if batch.trajectories is None:
        raise ValueError("run_trajectories: the batch was lowered without trajectories (compile_programs(..., noise, trajectories=))")
    n_traj = check_trajectories(batch.trajectories, "run_trajectories")
    seed = check_seed(seed, "run_trajectories")
    keys = _run_keys(run_keys, len(batch), "run_trajectories")
    if int(buffer_bytes) < 1:
        raise ValueError(f"run_trajectories: buffer_bytes = {buffer_bytes!r}, want a positive number of bytes")
    dev = torch.device(device)
    params, term_ptr = upload(batch.params, dev), upload(batch.term_ptr, dev)
    out = {k: [] for k in ("values", "std_error", "term_values", "term_std_error", "norm", "traj")}
    for chunk in _trajectory_chunks(batch, n_traj, buffer_bytes):
        lo, hi = chunk.start, chunk.stop
        ob, oe, tb, te = (int(v) for v in (batch.op_ptr[lo], batch.op_ptr[hi], batch.term_ptr[lo], batch.term_ptr[hi]))
        wave = [k - lo for k in chunk if batch.variant[k] == "wave"]
        wg = [k - lo for k in chunk if batch.variant[k] != "wave"]
        values, std_error, term_values, term_std_error, norm, traj, _ = ops.sim_run_trajectories(
            upload(batch.circ[lo:hi], dev), upload(batch.op_ptr[lo:hi + 1] - ob, dev), upload(batch.ops[ob:oe], dev), params,
            upload(batch.term_ptr[lo:hi + 1] - tb, dev), upload(batch.terms[tb:te], dev), upload(batch.coeff[tb:te], dev),
            upload(np.asarray(wave + wg, dtype=np.int32), dev), len(wave), len(wg), upload(keys[lo:hi], dev), n_traj, seed)
        for k, v in zip(out, (values, std_error, term_values, term_std_error, norm, traj if keep_trajectories else None)):
            out[k].append(v)

    def cat(parts, dim=0):
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=dim)

    if not out["values"]:   # an empty batch
        empty = torch.zeros(0, dtype=torch.float64, device=dev)
        return TrajectoryResult(empty, empty.clone(), empty.clone(), empty.clone(), empty.clone(), term_ptr, n_traj, seed,
                                torch.zeros((n_traj, 0), dtype=torch.float64, device=dev) if keep_trajectories else None, batch)
    return TrajectoryResult(cat(out["values"]), cat(out["std_error"]), cat(out["term_values"]), cat(out["term_std_error"]),
                            cat(out["norm"]), term_ptr, n_traj, seed, cat(out["traj"], 1) if keep_trajectories else None, batch)


def trajectory_expectation_values(circuits: Sequence[Any], observables: Sequence[Any], noise: Optional[NoiseModel] = None,
                                  trajectories: int = None, seed: int = 0, run_keys=None, device="cuda") -> TrajectoryResult:
    """Expectation values under ``noise`` estimated from ``trajectories`` pure-state trajectories per circuit, for noisy circuits
    of up to 11 qubits, non-Clifford gates, thermal relaxation and coherent errors included (the density-matrix mode stops at 5
    qubits).  Returns a :class:`TrajectoryResult`: the means and their standard errors.  See :func:`run_trajectories`."""
    if trajectories is None:
        raise ValueError("trajectory_expectation_values: trajectories is required (an int in 1 .. 2^20)")
    trajectories = check_trajectories(trajectories, "trajectory_expectation_values")
    if noise is None:
        raise ValueError("trajectory_expectation_values: noise is required (a NoiseModel); expectation_values gives the noiseless values")
    return run_trajectories(compile_programs(circuits, observables, noise, trajectories=trajectories), seed, run_keys, device)


def counts_dicts(result: SampleResult) -> List[List[Dict[str, int]]]:
    """``{bitstring: count}`` per (circuit, group) of a plain (unfolded) result, outcomes with a count of 0 left out.  A bitstring
    is qiskit's: n characters, qubit 0 the RIGHTMOST, so that ``int(bitstring, 2)`` is the outcome index -- the order
    ``counts_to_feature_vector`` expects.  Reads the counts back from the device."""
    counts = result.counts.cpu().numpy()
    if counts.ndim != 1:
        raise ValueError("counts_dicts: want the result of a plain run (folded runs carry a noise-factor axis: index it first)")
    prob_ptr, group_ptr = result.prob_ptr.cpu().numpy(), result.group_ptr.cpu().numpy()
    out = []
    for c in range(len(group_ptr) - 1):
        per = []
        for g in range(int(group_ptr[c]), int(group_ptr[c + 1])):
            b, e = int(prob_ptr[g]), int(prob_ptr[g + 1])
            width = max((e - b).bit_length() - 1, 1)
            per.append({format(j, f"0{width}b"): int(v) for j, v in enumerate(counts[b:e].tolist()) if v})
        out.append(per)
    return out


_TRAJECTORY_SHOTS = ("DeviceEstimator(method='trajectories'): shots= is not supported with it (shot sampling over trajectories is "
                     "out of scope; the estimate's own standard error is in the metadata); run it without shots")


_TRAJECTORY_NOISE = ("DeviceEstimator(method='trajectories'): noise=None; trajectories unravel a noise model (the noiseless values are "
                     "method='exact')")


_FRAMES_SHOTS = ("DeviceEstimator(method='frames'): shots=None; frame sampling draws measurement shots (pass shots=N; the exact "
                 "values of Clifford circuits are method='clifford')")


_MPS_SHOTS = ("DeviceEstimator(method='mps'): shots= is not supported with it (no shots are drawn from a matrix-product state; a "
              "noisy estimate's own standard error is in the metadata); run it without shots")


_MPS_SHOTS_NONE = ("DeviceEstimator(method='mps_shots'): shots=None; it draws measurement shots from a matrix-product state (pass "
                   "shots=N; the values without shot noise are method='mps')")


_CLIFFORD_SHOTS = ("DeviceEstimator: shots are not drawn on the Clifford path (method='clifford', or 'auto' on circuits over the exact "
                   "simulator's cap); run it without shots")


class SimulatedJob:
    """The job of a :class:`DeviceEstimator` run: the values are already on the host when it is built."""

    def __init__(self, values: np.ndarray, job_id: str, metadata: Optional[List[dict]] = None):
        self._values, self._job_id, self._metadata = values, job_id, metadata

    def result(self):
        return make_estimator_result(self._values, self._metadata if self._metadata is not None else [{} for _ in range(len(self._values))])

    def job_id(self) -> str:
        return self._job_id

    def status(self) -> str:
        return "DONE"

    def submit(self):
        return None

    def cancel(self) -> bool:
        return False


def _shot_rows(variance, shots: int) -> List[dict]:
    """The metadata of a sampled job: every circuit's per-shot variance and the shot count."""
    return [{"variance": float(v), "shots": shots} for v in variance.cpu().numpy()]


def _mps_rows(res, trajectories: Optional[int], rows: Optional[List[dict]] = None, std_error: bool = True) -> List[dict]:
    """The metadata of a matrix-product-state job, added to ``rows`` (None: empty ones): every circuit's certificate and largest bond
    and, under noise (``trajectories`` is then set), its standard error (``std_error=False``: the sampled path reports none) and the
    trajectory count."""
    bound, bond = res.error_bound.cpu().numpy(), res.bond.cpu().numpy()
    rows = [{} for _ in bond] if rows is None else rows
    for m, b, k in zip(rows, bound, bond):
        m.update(truncation_error_bound=float(b), max_bond=int(k))
    if trajectories is not None:
        if std_error:
            for m, e in zip(rows, res.std_error.cpu().numpy()):
                m["std_error"] = float(e)
        for m in rows:
            m["trajectories"] = trajectories
    return rows


# ---- the runners of the method table: (estimator, circuits, observables, shots, seed, keys) -> (values on the device, metadata rows or None)
def _exact(est, circuits, observables, shots, seed, keys):
    if shots is None:
        return expectation_values(circuits, observables, est._noise, est._device)[0], None
    res = sample_expectation_values(circuits, observables, est._noise, shots=shots, seed=seed, run_keys=keys, device=est._device)
    return res.values, _shot_rows(res.variance, shots)


def _clifford(est, circuits, observables, shots, seed, keys):
    return clifford_expectation_values(circuits, observables, est._noise, est._device)[0], None


def _frames(est, circuits, observables, shots, seed, keys):
    res = sample_clifford_expectation_values(circuits, observables, est._noise, shots=shots, seed=seed, run_keys=keys, device=est._device)
    return res.values, _shot_rows(res.variance, shots)


def _trajectories(est, circuits, observables, shots, seed, keys):
    res = trajectory_expectation_values(circuits, observables, est._noise, trajectories=est._trajectories, seed=seed, run_keys=keys,
                                        device=est._device)
    return res.values, [{"std_error": float(e), "trajectories": est._trajectories} for e in res.std_error.cpu().numpy()]


def _mps_trajectories(est) -> Optional[int]:
    return None if est._noise is None else est._trajectories


def _mps(est, circuits, observables, shots, seed, keys):
    res = mps_expectation_values(circuits, observables, est._noise, max_bond=est._max_bond, cutoff=est._cutoff,
                                 trajectories=_mps_trajectories(est), seed=seed, run_keys=keys, device=est._device,
                                 thermal_relaxation=est._relaxation, pauli_twirl=est._twirl)
    return res.values, _mps_rows(res, _mps_trajectories(est))


def _mps_shots(est, circuits, observables, shots, seed, keys):
    res = sample_mps_expectation_values(circuits, observables, est._noise, shots=shots, max_bond=est._max_bond, cutoff=est._cutoff,
                                        trajectories=_mps_trajectories(est), seed=seed, run_keys=keys, device=est._device,
                                        thermal_relaxation=est._relaxation, pauli_twirl=est._twirl)
    return res.values, _mps_rows(res, _mps_trajectories(est), _shot_rows(res.variance, shots), std_error=False)


def _bound_exact(est, circuits, observables, shots, seed, keys, parameter_values):
    return bound_expectation_values(list(circuits), list(observables), list(parameter_values), est._noise, est._device)[0], None


def _bound_mps(est, circuits, observables, shots, seed, keys, parameter_values):
    values, _, res = bound_mps_expectation_values(list(circuits), list(observables), list(parameter_values), est._noise, _mps_trajectories(est),
                                                  est._max_bond, est._cutoff, seed, keys, est._device, return_result=True)
    return values, _mps_rows(res, _mps_trajectories(est))


@dataclass(frozen=True)
class _Method:
    """One row of the method table: what ``DeviceEstimator(method=...)`` checks, at construction and per job, and what it runs."""

    run: Any                               # the runner of a job of bound circuits
    shots: str = "optional"                # "optional", "required" or "refused" ...
    shots_message: Optional[str] = None    # ... with this text
    draws: bool = False                    # draws without shots too: the seed is checked for every job
    noise_message: Optional[str] = None    # ``noise=None`` is refused with this text (None: noise is optional)
    pauli_noise_only: bool = False         # a model that is no Pauli channel is refused at construction
    per_job: bool = False                  # ``use_clifford_path`` sends a job to the Clifford path (``_CLIFFORD_PATH``) or leaves it here
    bound: Any = None                      # the runner of a job of templates (a runner with ``parameter_values``); None: refused
    wide_options: bool = False             # ``thermal_relaxation`` and ``pauli_twirl`` apply

    def check_shots_rule(self, shots) -> None:
        if (self.shots == "required" and shots is None) or (self.shots == "refused" and shots is not None):
            raise ValueError(self.shots_message)


_CLIFFORD_PATH = _Method(_clifford, "refused", _CLIFFORD_SHOTS)   # not chosen at construction, so its shots rule holds per job alone
_METHODS = {
    "exact": _Method(_exact, bound=_bound_exact),
    "clifford": _Method(_clifford, per_job=True),
    "auto": _Method(_exact, per_job=True, bound=_bound_exact),
    "trajectories": _Method(_trajectories, "refused", _TRAJECTORY_SHOTS, draws=True, noise_message=_TRAJECTORY_NOISE),
    "frames": _Method(_frames, "required", _FRAMES_SHOTS, pauli_noise_only=True),
    "mps": _Method(_mps, "refused", _MPS_SHOTS, draws=True, bound=_bound_mps, wide_options=True),
    "mps_shots": _Method(_mps_shots, "required", _MPS_SHOTS_NONE, wide_options=True),
}


def use_clifford_path(method: str, noise: Optional[NoiseModel], circuits) -> bool:
    """Whether a job under ``method`` ("clifford" or "auto") takes the Clifford path: always under ``"clifford"``; under ``"auto"``
    when a circuit is over the exact simulator's cap and every circuit is a Clifford circuit (a ``ValueError`` names one that fits
    neither path).  A noise model the Clifford path cannot carry is refused by name."""
    if method == "clifford":
        refuse_non_pauli(noise, "DeviceEstimator(method='clifford')")
        return True
    cap = MAX_QUBITS_VECTOR if noise is None else MAX_QUBITS_DENSITY
    parsed = [Circuit.from_any(c) for c in circuits]
    over = [k for k, c in enumerate(parsed) if c.num_qubits > cap]
    if not over:
        return False
    why = (f"DeviceEstimator(method='auto'): circuit {over[0]} has {parsed[over[0]].num_qubits} qubits, over the exact simulator's cap of "
           f"{cap} in this mode, so the job needs the Clifford path")
    refuse_non_pauli(noise, why)
    for k in over + [k for k in range(len(parsed)) if k not in over]:   # name a circuit that fits neither path first
        if not is_clifford(parsed[k]):
            raise ValueError(f"{why}, and circuit {k} is not a Clifford circuit")
    return True


class DeviceEstimator:
    """An Estimator-shaped primitive on the batched simulator: ``run(circuits, observables, parameter_values)`` returns a job whose
    ``result().values[k]`` is the exact expectation value of ``observables[k]`` after ``circuits[k]`` (``noise=None``) or the one
    under ``noise`` (a :class:`NoiseModel`, density-matrix mode), ``metadata[k] = {}``.  It has the ``_run`` protocol the
    ``learning(...)`` and ``ngem(...)`` decorators patch.  Circuits arrive bound (QASM text, ``Circuit`` or a bound qiskit-like
    circuit); non-empty ``parameter_values`` are refused for them.  A :class:`Template` (or a qiskit-like circuit with free
    parameters) comes with its row of ``parameter_values`` and is bound on the device (:func:`bound_expectation_values`: one lowering
    per distinct template, one run per row), under ``method="exact"``, under ``"auto"`` within the cap and, at width, under
    ``"mps"``; ``shots``, the other methods and ``zne(DeviceEstimator)`` refuse a template by name.  There is no host path:
    ``device`` must be a GPU.

    ``shots`` (constructor, or the ``shots=`` run option, which wins; ``None``: exact, as above): the values are estimated from that
    many measurement outcomes per measurement basis (:func:`sample_expectation_values`) and ``metadata[k] = {"variance": v_k,
    "shots": shots}``, as qiskit's estimators report.  ``seed`` (constructor or run option) keys the draws.  Successive ``run()``
    calls of one estimator do not repeat their draws: circuit k of the estimator's j-th job (j = 1, 2, ...; exact jobs count too)
    draws with the run key ``j * 2^32 + k``, so two estimators with one seed that are asked the same things agree.

    ``method``: ``"exact"`` (the default: the state-vector / density-matrix simulator and its caps, as above); ``"clifford"``: the
    Clifford path (:func:`clifford_expectation_values`: Clifford circuits of up to 512 qubits, exact under the same noise model);
    ``"auto"``: the exact simulator when every circuit of a job fits its cap, else the Clifford path when every circuit is a Clifford
    circuit, else a ``ValueError`` naming a circuit that is neither.  The Clifford path draws no shots: ``shots`` with it is refused.
    ``"trajectories"``: quantum trajectories (:func:`trajectory_expectation_values`: noisy circuits of up to 11 qubits, any lowered
    gate, any :class:`NoiseModel`); the values are means over ``trajectories`` (constructor; default 1 024) trajectories per circuit
    and ``metadata[k] = {"std_error": e_k, "trajectories": T}``.  It needs a noise model and draws no shots: ``noise=None`` and
    ``shots`` with it are refused.  Run keys are those of the shots path, so successive jobs do not repeat their draws.  ``"auto"``
    never falls back to trajectories: an estimate with a standard error is chosen by name, not silently.
    ``"frames"``: measurement shots of Clifford circuits of up to 512 qubits by Pauli-frame sampling
    (:func:`sample_clifford_expectation_values`), ideal or under a depolarising + readout model; it needs ``shots`` (``shots=None``
    is refused by name, and so are templates), ``metadata[k] = {"variance": v_k, "shots": shots}`` and the run keys are those of the
    shots path.  ``"auto"`` never picks it.
    ``"mps"``: matrix-product states of bond at most ``max_bond`` (:func:`mps_expectation_values`: circuits of up to 512 qubits whose
    two-qubit gates act on neighbours, any angle; ``cutoff`` is the relative weight below which a column is dropped).  Without
    ``noise`` the values are the ideal ones and ``metadata[k] = {"truncation_error_bound": B_k, "max_bond": the largest bond
    reached}`` with |value - exact| <= 2 B_k sum|coeff|; with ``noise`` (depolarising + readout, coherent errors) they are means over
    ``trajectories`` trajectories and the metadata also has ``"std_error"`` and ``"trajectories"``.  ``shots`` with it is refused by
    name.  Templates run here too, bound on the device (:func:`bound_mps_expectation_values`), with the same job ids, run keys and
    metadata.  ``"auto"`` never picks it.  ``thermal_relaxation=True`` (``"mps"`` and ``"mps_shots"`` alone) takes a model with
    thermal relaxation (:func:`compile_mps`: quantum jumps at the orthogonality centre); the metadata keys are the same, and
    ``truncation_error_bound`` is then the mean of per-trajectory certificates, each conditional on the jumps drawn (|value - exact|
    <= 4 B sum|coeff| per trajectory).  Templates with it are refused by name.  ``pauli_twirl`` (``"mps"`` and ``"mps_shots"``
    alone, with ``noise``; ``True`` or gate names, :func:`compile_mps`) twirls the two-qubit gates on the device, one draw per
    trajectory and gate; ``zne(DeviceEstimator)`` passes it on to the folded runs.  The metadata keys are unchanged.
    ``"mps_shots"``: measurement shots drawn from those matrix-product states (:func:`sample_mps_expectation_values`), ideal or with
    ``noise`` and ``trajectories`` (shot s comes from trajectory s mod trajectories, so ``trajectories <= shots``); it needs ``shots``
    (``shots=None`` is refused by name, and so are templates), ``metadata[k] = {"variance": v_k, "shots": shots,
    "truncation_error_bound": B_k, "max_bond": the largest bond reached}`` plus ``"trajectories"`` under noise, and the run keys are
    those of the shots path.  ``variance`` is the per-shot variance; with fewer trajectories than shots the estimate's standard
    error also has a between-trajectory part (:class:`MpsShotsResult`).  ``"auto"`` never picks it."""

    METHODS = ("exact", "clifford", "auto", "trajectories")
    SAMPLED_METHODS = ("frames",)   # chosen by name alone; "auto" never picks one
    WIDE_METHODS = ("mps",)         # chosen by name alone too
    WIDE_SAMPLED_METHODS = ("mps_shots",)   # shots at width from matrix-product states; by name alone

    def __init__(self, noise: Optional[NoiseModel] = None, device="cuda", shots: Optional[int] = None, seed: int = 0,
                 method: str = "exact", trajectories: int = 1024, max_bond: int = MAX_BOND, cutoff: float = DEFAULT_CUTOFF,
                 thermal_relaxation: bool = False, pauli_twirl: Any = None):
        methods = self.METHODS + self.SAMPLED_METHODS + self.WIDE_METHODS + self.WIDE_SAMPLED_METHODS
        if method not in methods:
            raise ValueError(f"DeviceEstimator: method = {method!r}, want one of {', '.join(methods)}")
        self._method, entry = method, _METHODS[method]
        self._max_bond, self._cutoff = _check_bond(max_bond, "DeviceEstimator"), _check_cutoff(cutoff, "DeviceEstimator")
        if not isinstance(thermal_relaxation, bool):
            raise ValueError(f"DeviceEstimator: thermal_relaxation = {thermal_relaxation!r}, want True or False")
        if thermal_relaxation and not entry.wide_options:
            raise ValueError(f"DeviceEstimator(method={method!r}): thermal_relaxation=True belongs to method='mps' and 'mps_shots' (the "
                             "exact and trajectory paths take a model with thermal relaxation as it is)")
        self._relaxation = thermal_relaxation
        self._twirl = _check_twirl(pauli_twirl, "DeviceEstimator") or None
        if self._twirl and not entry.wide_options:
            raise ValueError(f"DeviceEstimator(method={method!r}): pauli_twirl= belongs to method='mps' and 'mps_shots' (the twirl is "
                             "drawn per trajectory on the matrix-product-state path)")
        if entry.noise_message is None:   # the order of these checks is the one a call with two faults has always met
            entry.check_shots_rule(shots)
            if entry.pauli_noise_only:
                refuse_non_pauli(noise, f"DeviceEstimator(method={method!r})")
        self._trajectories = check_trajectories(trajectories, "DeviceEstimator")
        if entry.noise_message is not None:
            if noise is None:
                raise ValueError(entry.noise_message)
            entry.check_shots_rule(shots)
        self._noise, self._device, self._count = noise, device, 0
        self._shots = None if shots is None else check_shots(shots, "DeviceEstimator")
        self._seed = check_seed(seed, "DeviceEstimator")

    def run(self, circuits, observables, parameter_values=None, **run_options):
        circuits, observables = list(circuits), list(observables)
        if parameter_values is None:
            parameter_values = [()] * len(circuits)
        return self._run(circuits, observables, list(parameter_values), **run_options)

    def _run(self, circuits, observables, parameter_values, **run_options):
        free = [has_free_parameters(c) for c in circuits]
        for k, p in enumerate(parameter_values):
            if len(p) and not free[k]:
                raise ValueError(f"DeviceEstimator: circuit {k} comes with {len(p)} parameter values; circuits must arrive bound")
        shots = run_options.pop("shots", self._shots)
        seed = run_options.pop("seed", self._seed)
        entry = _METHODS[self._method]
        if any(free):
            run = self._template_runner(entry, circuits, parameter_values, free.index(True), shots)
        else:
            if entry.per_job and self._use_clifford(circuits):
                entry = _CLIFFORD_PATH
            entry.check_shots_rule(shots)
            run = entry.run
        if shots is not None:
            shots = check_shots(shots, "DeviceEstimator.run")
        draws = entry.draws or shots is not None
        if draws:
            seed = check_seed(seed, "DeviceEstimator.run")
        self._count += 1   # the call is accepted: job j = 1, 2, ... draws with the run keys j * 2^32 + k (a job that draws nothing has none)
        keys = default_run_keys(len(circuits), self._count << 32) if draws else None
        values, metadata = run(self, circuits, observables, shots, seed, keys)
        return SimulatedJob(values.cpu().numpy(), f"sim-{self._count}", metadata)

    def _template_runner(self, entry: _Method, circuits, parameter_values, first: int, shots):
        """The runner of a job with templates (or qiskit-like circuits with free parameters): the bound path, one lowering per distinct
        (template, observable) pair and one run per row -- on the exact simulator, or under ``method="mps"`` on matrix-product
        states (:func:`bound_mps_expectation_values`).  Everything else is refused by name."""
        how = ("bind it first (Template.bind_parameters(values)) and pass the bound circuit, which takes that path as ever; "
               "templates run on the exact simulator (method='exact', or 'auto' within its cap) and on matrix-product states "
               "(method='mps'), without shots")
        if shots is not None:
            raise ValueError(f"DeviceEstimator: circuit {first} is a template with free parameters and shots= is set: shots are not "
                             f"drawn on the bound path; {how}")
        if entry.bound is None:
            raise ValueError(f"DeviceEstimator(method={self._method!r}): circuit {first} is a template with free parameters; {how}")
        templates = [Template.from_any(c) for c in circuits]
        for k, (t, p) in enumerate(zip(templates, parameter_values)):
            if len(p) != t.num_parameters:
                raise ValueError(f"DeviceEstimator: circuit {k} comes with {len(p)} parameter values, the template has "
                                 f"{t.num_parameters} parameters")
        if self._relaxation:
            raise ValueError(f"DeviceEstimator(method='mps', thermal_relaxation=True): circuit {first} is a template with free "
                             "parameters; thermal relaxation on templates is not built (bind the circuit first)")
        if self._twirl:
            raise ValueError(f"DeviceEstimator(method='mps', pauli_twirl=): circuit {first} is a template with free parameters; "
                             "twirled templates are not built (mlqem_mps_bind_f64 does not know the twirl records: bind the "
                             "circuit first)")
        if self._method == "auto":
            cap = MAX_QUBITS_VECTOR if self._noise is None else MAX_QUBITS_DENSITY
            for k, t in enumerate(templates):
                if t.num_qubits > cap:
                    raise ValueError(f"DeviceEstimator(method='auto'): circuit {k} is a template of {t.num_qubits} qubits, over the "
                                     f"exact simulator's cap of {cap} in this mode; {how}")
        return functools.partial(entry.bound, parameter_values=parameter_values)

    def _use_clifford(self, circuits) -> bool:
        return use_clifford_path(self._method, self._noise, circuits)
