"""Times shots from matrix-product states (csrc/mps.hip: mlqem_mps_sample_f64, mlqem_mps_sample_finish_f64) on the MI355X and
writes profiles/mps_shots_micro.json.

    python scripts/mps_shots_micro.py [--circuits 1024] [--noisy-circuits 1024] [--steps 1 3 5] [--modes ideal noisy]
                                      [--out profiles/mps_shots_micro.json]

Per shape: ``tfim_circuit(100, s, J, two_q="cx")`` with J ~ U(0, 0.66 pi), single-Z terms (one measurement group a circuit) at bond 32,
for s = 1, 3, 5 Trotter steps; ideal, and under the synthetic backend's depolarising + readout model with 16 trajectories per
circuit; 1 000 and 10 000 shots.  Reported per (shape, shots):
  ``sample_ms``  the sampling launches alone (environment pass + sampling pass of every chunk; device events around them, the MPS
                 runs of the chunks outside the events), one pass after a warm-up on the first 16 circuits;
  ``call_ms``    the whole ``run_mps_shots`` call (upload, the MPS run and the sampling of every chunk, both finish launches; host
                 clock around a device synchronisation), one call;
  ``run_mps_ms`` ``run_mps`` of the same batch beside it (the MPS run and the term contractions, no shots), one call,
and shots per second over all circuits from ``sample_ms``.  ``--circuits`` / ``--noisy-circuits``: fewer circuits (the rows say how
many); a call with a part of ``--steps`` or ``--modes`` keeps the other rows of ``--out``.  Nothing here asserts a speed or a ratio: these are first measurements.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mps_cases as mc  # noqa: E402
from blackwater import sim  # noqa: E402
from blackwater.data.synthetic import synthetic_backend, tfim_circuit  # noqa: E402
from blackwater.native import ops  # noqa: E402
from blackwater.sim.mps import MPS_BUFFER_BYTES, _mps_chunks  # noqa: E402

DEV = "cuda:0"


def sampling_alone(batch, shot_counts, seed=1):
    """``({shots: milliseconds}, chunks)``: the sampling launches of every chunk of ``run_mps_shots``'s loop by device events, for
    every shot count on the same MPS run of the chunk."""
    mps = batch.mps
    t = batch.to(DEV)
    b, n_terms, n_traj = len(batch), len(mps.term_circ), mps.trajectories or 1
    keys = torch.arange(b, dtype=torch.int64, device=DEV)
    stats = torch.zeros((n_traj, b, ops.MPS_STATS), dtype=torch.float64, device=DEV)
    sums = torch.zeros(n_terms, dtype=torch.int32, device=DEV)

    def unit_bytes(width):
        return ops.mps_workspace_bytes(width, mps.max_bond, 1) + ops.mps_sample_workspace_bytes(width, mps.max_bond, 1)

    chunks = _mps_chunks(mps.n_qubits, mps.max_bond, n_traj, MPS_BUFFER_BYTES, unit_bytes)
    units = max(len(cr) * len(tr) for cr, tr in chunks)
    width = int(mps.n_qubits.max())
    workspace = torch.empty(ops.mps_workspace_bytes(width, mps.max_bond, units), dtype=torch.uint8, device=DEV)
    env = torch.empty(ops.mps_sample_workspace_bytes(width, mps.max_bond, units), dtype=torch.uint8, device=DEV)
    total = {shots: 0.0 for shots in shot_counts}
    for cr, tr in chunks:
        ops.mps_run(t["n_qubits"], t["op_ptr"], t["ops"], t["params"], keys, (cr.start, len(cr)), (tr.start, len(tr)), n_traj, seed,
                    mps.max_bond, mps.cutoff, width, workspace, stats)
        g0, g1 = int(batch.group_ptr[cr.start]), int(batch.group_ptr[cr.stop])
        t0, t1 = int(mps.term_ptr[cr.start]), int(mps.term_ptr[cr.stop])
        for shots in shot_counts:
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            ops.mps_sample(t["n_qubits"], (cr.start, len(cr)), (tr.start, len(tr)), n_traj, mps.max_bond, width, workspace, env,
                           (g0, g1 - g0), batch.max_groups, t["group_ptr"], t["group_circ"], t["group_off"], t["basis"], t["site_ptr"],
                           t["flip"], t["ref_ptr"], t["gterm_ptr"], t["gterm"], (t0, t1 - t0), t["term_mask"], t["masks"], keys, shots, seed,
                           sums)
            stop.record()
            torch.cuda.synchronize()
            total[shots] += start.elapsed_time(stop)
    return total, len(chunks)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuits", type=int, default=1024)
    ap.add_argument("--noisy-circuits", type=int, default=1024)
    ap.add_argument("--steps", type=int, nargs="+", default=[1, 3, 5])
    ap.add_argument("--modes", nargs="+", choices=("ideal", "noisy"), default=["ideal", "noisy"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_shots_micro.json"))
    args = ap.parse_args()
    nq, trajectories = 100, 16
    rng = np.random.default_rng(42)
    couplings = rng.uniform(0.0, 0.66 * math.pi, size=1024)
    noise = sim.NoiseModel.from_backend(synthetic_backend(nq, "cx"))
    rows = []
    for steps in args.steps:
        for noisy in [m == "noisy" for m in args.modes]:
            count = args.noisy_circuits if noisy else args.circuits
            circuits = [tfim_circuit(nq, steps, float(j), two_q="cx") for j in couplings[:count]]
            obs = [mc.single_z(nq)] * count
            t0 = time.perf_counter()
            batch = sim.compile_mps_shots(circuits, obs, noise if noisy else None, trajectories if noisy else None)
            lower_s = time.perf_counter() - t0
            head = sim.compile_mps_shots(circuits[:16], obs[:16], noise if noisy else None, trajectories if noisy else None)
            sim.run_mps_shots(head, 1000, seed=1, device=DEV)   # warm-up: every kernel of the call has run once
            run_ms, plain = wall(lambda: sim.run_mps(batch.mps, seed=1, device=DEV))
            print(f"# {steps} steps, {count} circuits, noisy {noisy}: run_mps {run_ms:.0f} ms", flush=True)
            alone, n_chunks = sampling_alone(batch, (1000, 10000))
            print(f"# sampling alone {alone}", flush=True)
            for shots in (1000, 10000):
                sample_ms = alone[shots]
                call_ms, res = wall(lambda: sim.run_mps_shots(batch, shots, seed=1, device=DEV))
                worst = float((res.term_values - plain.term_values).abs().max())
                row = {"steps": steps, "circuits": count, "qubits": nq, "groups_per_circuit": 1, "max_bond": 32,
                       "trajectories": trajectories if noisy else None, "shots": shots, "chunks": n_chunks, "lowering_ms": 1e3 * lower_s,
                       "sample_ms": sample_ms, "call_ms": call_ms, "run_mps_ms": run_ms,
                       "shots_per_second": count * shots / (1e-3 * sample_ms), "largest_bond": int(res.bond.max()),
                       "worst_error_bound": float(res.error_bound.max()), "largest_estimate_minus_mean": worst}
                rows.append(row)
                print(json.dumps(row), flush=True)
    if os.path.exists(args.out):   # rows of shapes measured by an earlier call stay (a call may take a part of --steps)
        key = lambda r: (r["steps"], r["trajectories"], r["shots"])   # noqa: E731
        fresh = {key(r) for r in rows}
        rows = sorted([r for r in json.load(open(args.out))["rows"] if key(r) not in fresh] + rows,
                      key=lambda r: (r["steps"], r["trajectories"] or 0, r["shots"]))
    out = {"device": torch.cuda.get_device_name(0), "shot_block": ops.MPS_SHOT_BLOCK, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
