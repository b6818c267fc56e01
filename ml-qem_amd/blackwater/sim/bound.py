"""Device side of parameter binding: runs of lowered templates (``mlqem_sim_run_bound_f64``) and parameter-shift gradients
(``mlqem_sim_shift_combine_f64``).  DESIGN.md 3.14."""
from __future__ import annotations

import math
from typing import Any, List, Optional, Tuple

import numpy as np

from ..data.backends import pauli_terms
from .program import NoiseModel, upload, upload_fields
from .template import BoundBatch, Template, compile_templates

BOUND_BUFFER_BYTES = 256 << 20   # the per-run buffers of one call stay under this (``buffer_bytes=``)
MAX_RUNS = 2 ** 31 - 1           # runs one call can take


def _pairs(template, observable, parameter_values, who: str):
    """``(templates, observables, pair_of_row, theta [max(B, 1), max(P, 1)], B)``: the unique (template object, observable) pairs,
    the pair of every row, and the rows padded with zeros to the longest."""
    if isinstance(template, (list, tuple)):
        tpls = list(template)
        if not isinstance(observable, (list, tuple)) or len(observable) != len(tpls):
            raise ValueError(f"{who}: {len(tpls)} templates need a list of as many observables")
        obss = list(observable)
        rows = [np.asarray(r, dtype=np.float64).reshape(-1) for r in parameter_values]
        if len(rows) != len(tpls):
            raise ValueError(f"{who}: {len(tpls)} templates but {len(rows)} parameter rows")
    else:
        theta = np.asarray(parameter_values, dtype=np.float64)
        theta = theta.reshape(1, -1) if theta.ndim < 2 else theta
        if theta.ndim != 2:
            raise ValueError(f"{who}: parameter_values has the shape {theta.shape}, want [B, P]")
        rows = list(theta)
        tpls, obss = [template] * len(rows), [observable] * len(rows)
    unique, u_tpl, u_obs, pair = {}, [], [], []
    for t, o in zip(tpls, obss):
        try:
            okey = tuple((str(l), complex(c)) for l, c in pauli_terms(o))
        except TypeError:
            okey = id(o)
        key = (id(t), okey)
        if key not in unique:
            unique[key] = len(u_tpl)
            u_tpl.append(Template.from_any(t))
            u_obs.append(o)
        pair.append(unique[key])
    for k, (r, c) in enumerate(zip(rows, pair)):
        if r.shape[0] != u_tpl[c].num_parameters:
            raise ValueError(f"{who}: row {k} has {r.shape[0]} parameter values, its template has {u_tpl[c].num_parameters} parameters")
        if not np.all(np.isfinite(r)):
            raise ValueError(f"{who}: row {k} has a non-finite parameter value")
    width = max([1] + [t.num_parameters for t in u_tpl])
    theta = np.zeros((max(len(rows), 1), width), dtype=np.float64)
    for k, r in enumerate(rows):
        theta[k, :r.shape[0]] = r
    return u_tpl, u_obs, np.asarray(pair, dtype=np.int64), theta, len(rows)


def run_bound(batch: BoundBatch, theta, runs: np.ndarray, shift: np.ndarray, device="cuda", buffer_bytes: int = BOUND_BUFFER_BYTES,
              form: Optional[int] = None):
    """``(values [n_runs], term_values [n_runs, T], norm [n_runs])`` of ``runs`` int32 [n_runs, 4] = (template, theta row, shifted
    record or -1, 0) with ``shift`` float64 [n_runs], on the lowered ``batch``.  T is the largest term count of a template; a run's
    row of ``term_values`` holds its template's terms and zeros after them.  ``theta``: float64 [n_rows, ld] (numpy or a tensor on
    the device).  The runs are split so that one call takes at most 2^31 - 1 of them and its per-run buffers stay under
    ``buffer_bytes``; a run's bits do not depend on the split."""
    import torch

    from ..native import ops

    dev = torch.device(device)
    if int(buffer_bytes) < 1:
        raise ValueError(f"run_bound: buffer_bytes = {buffer_bytes!r}, want a positive number of bytes")
    form = ops.SIM_BOUND_TABLE if form is None else form
    runs = np.ascontiguousarray(runs, dtype=np.int32).reshape(-1, 4)
    shift = np.ascontiguousarray(shift, dtype=np.float64).reshape(-1)
    n_runs = int(runs.shape[0])
    width = int(np.diff(batch.term_ptr).max()) if len(batch) else 0
    theta_d = theta.to(dev) if isinstance(theta, torch.Tensor) else upload(np.asarray(theta, dtype=np.float64), dev)
    t = upload_fields(batch, ("circ", "op_ptr", "ops", "params", "term_ptr", "terms", "coeff"), dev) if n_runs else {}
    values = torch.zeros(n_runs, dtype=torch.float64, device=dev)
    norm = torch.zeros(n_runs, dtype=torch.float64, device=dev)
    term_values = torch.zeros((n_runs, width), dtype=torch.float64, device=dev)
    per_run = 16 + 8 + 4 + 8 + 16 + 8 * width   # runs, shift, ids, run_term_ptr, values and norm, term values
    step = max(min(int(buffer_bytes) // per_run, MAX_RUNS), 1)
    is_wave = np.asarray([v == "wave" for v in batch.variant], dtype=bool)
    for lo in range(0, n_runs, step):
        hi = min(lo + step, n_runs)
        wave = is_wave[runs[lo:hi, 0]]
        ids = np.concatenate([np.flatnonzero(wave), np.flatnonzero(~wave)]).astype(np.int32)
        ops.sim_run_bound(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], theta_d,
                          upload(runs[lo:hi], dev), upload(shift[lo:hi], dev), upload(ids, dev), int(wave.sum()), int((~wave).sum()),
                          upload(np.arange(hi - lo + 1, dtype=np.int64) * width, dev), (hi - lo) * width, form=form,
                          term_values=term_values[lo:hi].reshape(-1), values=values[lo:hi], norm=norm[lo:hi])
    return values, term_values, norm


def bound_expectation_values(template, observable, parameter_values, noise: Optional[NoiseModel] = None, device="cuda",
                             buffer_bytes: int = BOUND_BUFFER_BYTES):
    """Exact expectation values of one template at many parameter vectors: ``(values [B], term_values [B, T])``, float64 tensors
    on ``device``.  ``template`` / ``observable``: single objects with ``parameter_values`` [B, P], or equal-length lists with one
    parameter row per pair (T is then the largest term count, rows padded with zeros).  Equal (template object, observable) pairs
    are lowered once (:func:`compile_templates`) and the rows become runs; nothing is bound or lowered per row on the host.
    ``noise=None`` simulates state vectors, a :class:`NoiseModel` density matrices."""
    tpls, obss, pair, theta, n_rows = _pairs(template, observable, parameter_values, "bound_expectation_values")
    batch = compile_templates(tpls, obss, noise)
    runs = np.zeros((n_rows, 4), dtype=np.int32)
    runs[:, 0], runs[:, 1], runs[:, 2] = pair, np.arange(n_rows), -1
    values, term_values, _ = run_bound(batch, theta, runs, np.zeros(n_rows), device, buffer_bytes)
    return values, term_values


def shift_runs(batch: BoundBatch, pair: np.ndarray) -> Tuple[np.ndarray, np.ndarray, List[Tuple[int, np.ndarray, int, int]]]:
    """The runs of a parameter-shift gradient: per template c with rows ``R`` (B_c of them) and K_c occurrences, B_c unshifted runs,
    then K_c x B_c runs shifted by +pi/2 (occurrence-major), then as many by -pi/2.  Returns ``(runs, shift, groups)`` with
    ``groups = [(c, rows, first run, K_c)]``."""
    runs, shift, groups, at = [], [], [], 0
    for c in range(len(batch)):
        rows = np.flatnonzero(pair == c)
        if rows.size == 0:
            continue
        occ = batch.occ_op[int(batch.occ_ptr[c]):int(batch.occ_ptr[c + 1])]
        k, b = int(occ.size), int(rows.size)
        block = np.zeros((b * (1 + 2 * k), 4), dtype=np.int32)
        block[:, 0] = c
        block[:, 1] = np.tile(rows, 1 + 2 * k)
        block[:b, 2] = -1
        block[b:, 2] = np.tile(np.repeat(occ, b), 2)
        sh = np.zeros(block.shape[0], dtype=np.float64)
        sh[b:b + k * b], sh[b + k * b:] = 0.5 * math.pi, -0.5 * math.pi
        runs.append(block)
        shift.append(sh)
        groups.append((c, rows, at, k))
        at += block.shape[0]
    if not runs:
        return np.zeros((0, 4), dtype=np.int32), np.zeros(0), groups
    return np.concatenate(runs), np.concatenate(shift), groups


def parameter_shift(template, observable, parameter_values, noise: Optional[NoiseModel] = None, device="cuda",
                    buffer_bytes: Optional[int] = None, method: str = "exact", trajectories: Optional[int] = None, max_bond: Optional[int] = None,
                    cutoff: Optional[float] = None, seed: int = 0, run_keys=None):
    """Values and exact gradients by the parameter-shift rule: ``(values [B], gradients [B, P])``, float64 tensors on ``device``.

    ``method="exact"`` (the default) runs the exact simulator, as described below.  ``method="mps"`` runs the same rule on
    matrix-product states (:func:`blackwater.sim.mps.mps_parameter_shift`: templates of up to 512 qubits whose two-qubit gates
    act on neighbours; ``max_bond``, ``cutoff``, and under ``noise`` ``trajectories``, ``seed`` and one run key per ROW:
    every run of a row draws the row's Pauli insertions, so the rule is exact for that trajectory set).  Those options are
    refused under ``"exact"``.

    Every parameterised gate is a rotation exp(-i phi G / 2) with G^2 = 1 (``p`` up to a phase), so ``d<O>/d phi = (<O>(phi + pi/2)
    - <O>(phi - pi/2)) / 2`` exactly, under noise too (the noise does not depend on the angle), and a parameter's derivative is the
    sum over its occurrences of ``scale`` times that.  One launch simulates the B unshifted runs and the 2 K B shifted ones (K
    occurrences), then ``mlqem_sim_shift_combine_f64`` adds them up in a fixed order: two calls return the same bits.  Arguments as
    :func:`bound_expectation_values`; with several templates P is the largest parameter count (columns past a template's own are 0)."""
    import torch

    from ..native import ops

    if method == "mps":
        from .mps import DEFAULT_CUTOFF, MAX_BOND, mps_parameter_shift

        return mps_parameter_shift(template, observable, parameter_values, noise, trajectories, MAX_BOND if max_bond is None else max_bond,
                                   DEFAULT_CUTOFF if cutoff is None else cutoff, seed, run_keys, device, buffer_bytes)
    if method != "exact":
        raise ValueError(f"parameter_shift: method = {method!r}, want 'exact' or 'mps'")
    if trajectories is not None or max_bond is not None or cutoff is not None or run_keys is not None:
        raise ValueError("parameter_shift: trajectories, max_bond, cutoff and run_keys belong to method='mps'; the exact simulator "
                         "takes none of them")
    buffer_bytes = BOUND_BUFFER_BYTES if buffer_bytes is None else buffer_bytes
    tpls, obss, pair, theta, n_rows = _pairs(template, observable, parameter_values, "parameter_shift")
    batch = compile_templates(tpls, obss, noise)
    runs, shift, groups = shift_runs(batch, pair)
    dev = torch.device(device)
    all_values, _, _ = run_bound(batch, theta, runs, shift, dev, buffer_bytes)
    width = max([0] + [t.num_parameters for t in tpls])
    values = torch.zeros(n_rows, dtype=torch.float64, device=dev)
    grads = torch.zeros((n_rows, width), dtype=torch.float64, device=dev)
    for c, rows, at, k in groups:
        b, p = int(rows.size), int(batch.num_parameters[c])
        ob = int(batch.occ_ptr[c])
        par = batch.occ_param[ob:ob + k]
        order = np.argsort(par, kind="stable").astype(np.int32)   # a parameter's occurrences, in circuit order
        occ_ptr = np.concatenate([[0], np.cumsum(np.bincount(par, minlength=p))]).astype(np.int64)
        v = all_values[at:at + b * (1 + 2 * k)]
        g = ops.sim_shift_combine(v[b:b + k * b].reshape(k, b), v[b + k * b:].reshape(k, b), upload(occ_ptr, dev), upload(order, dev),
                                  upload(batch.occ_scale[ob:ob + k], dev))
        if len(groups) == 1 and p == width and np.array_equal(rows, np.arange(n_rows)):
            return v[:b], g
        idx = upload(rows, dev)
        values[idx] = v[:b]
        grads[idx, :p] = g
    return values, grads
