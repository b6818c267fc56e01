"""Times zero-noise extrapolation on the matrix-product-state path (csrc/mps.hip: mlqem_mps_run_folded_f64 through
``zne_run(method="mps")``) on the MI355X and writes profiles/mps_zne_micro.json.

    python scripts/mps_zne_micro.py [--quick] [--out profiles/mps_zne_micro.json]

Per shape: ``tfim_circuit(100, s, J, two_q="cx")`` with J ~ U(0, 0.66 pi), s = 1, 3 Trotter steps, 128 circuits x 100 single-Z
terms, 16 trajectories, factors (1, 3), two-qubit local folding, bond 32, under the synthetic backend's depolarising + readout
model.  (The 5-step shape is left out: its plain run alone takes over five minutes at 16 trajectories.)  Measured, each the median
of 3 after a warm-up on the first 16 circuits, the two routes alternating:

  fused         the whole ``zne_run(method="mps")``: one lowering, the schedules, every (run, trajectory) unit, terms, finish,
                combine; host clock around a device synchronisation.  Its host part (``compile_mps`` + ``build_mps_schedules``) and
                its device part (``run_mps_folded`` on the lowered batch: upload, launches, finish; host clock around a
                synchronisation, and device events around the same call) are also timed apart.
  host folding  the route without the schedules: per factor ``fold_circuit`` + ``compile_mps`` + ``run_mps`` on the folded circuits,
                under the keys the fused runs have; host and device parts apart.

Two-qubit local folding folds ``cx`` alone, which is its own inverse, so the folded circuits lower to the records the schedules
name and the two routes must give the same bits: ``bit_equal`` says whether they did.  Decompositions per (run, trajectory) come
from the stats, per factor.  Nothing here asserts a speed or a ratio.  ``--quick``: 16 circuits.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mps_cases as mc  # noqa: E402
from blackwater import sim, zne  # noqa: E402
from blackwater.data.synthetic import synthetic_backend, tfim_circuit  # noqa: E402

DEV = "cuda:0"
FACTORS, TRAJECTORIES, SEED = (1, 3), 16, 1


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fused(circuits, obs, noise, strategy):
    return zne.zne_run(circuits, obs, noise, strategy, DEV, seed=SEED, method="mps", trajectories=TRAJECTORIES, keep_trajectories=True)


def host_folded(circuits, obs, noise, strategy):
    """``(host seconds, device seconds, [MpsResult per factor])`` of the route without schedules."""
    host = device = 0.0
    out, b = [], len(circuits)
    for f, lam in enumerate(strategy.noise_factors):
        t0 = time.perf_counter()
        batch = sim.compile_mps([zne.fold_circuit(c, lam, strategy.noise_amplifier) for c in circuits], obs, noise, TRAJECTORIES)
        host += time.perf_counter() - t0
        seconds, res = clock(lambda: sim.run_mps(batch, seed=SEED, run_keys=f * b + np.arange(b), device=DEV, keep_trajectories=True))
        device += seconds
        out.append(res)
    return host, device, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_zne_micro.json"))
    args = ap.parse_args()
    nq, count = 100, 16 if args.quick else 128
    rng = np.random.default_rng(42)
    couplings = rng.uniform(0.0, 0.66 * math.pi, size=count)
    noise = sim.NoiseModel.from_backend(synthetic_backend(nq, "cx"))
    strategy = zne.ZNEStrategy(FACTORS, zne.TwoQubitAmplifier(), zne.LinearExtrapolator())
    obs = [mc.single_z(nq)] * count
    rows = []
    for steps in (1, 3):
        circuits = [tfim_circuit(nq, steps, float(j), two_q="cx") for j in couplings]
        t0 = time.perf_counter()
        batch = sim.compile_mps(circuits, obs, noise, TRAJECTORIES)
        lower_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        sch = zne.build_mps_schedules(batch, FACTORS, strategy.noise_amplifier)
        sched_s = time.perf_counter() - t0
        fused(circuits[:16], obs[:16], noise, strategy)          # warm-up: every kernel of both routes
        host_folded(circuits[:16], obs[:16], noise, strategy)
        t_fused, t_device, t_events, t_fold_host, t_fold_device = [], [], [], [], []
        for _ in range(3):
            seconds, run = clock(lambda: fused(circuits, obs, noise, strategy))
            t_fused.append(seconds)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            seconds, res = clock(lambda: (zne.run_mps_folded(batch, sch, seed=SEED, device=DEV, keep_trajectories=True), stop.record())[0])
            t_device.append(seconds)
            t_events.append(start.elapsed_time(stop) / 1e3)
            host, device, plain = host_folded(circuits, obs, noise, strategy)
            t_fold_host.append(host)
            t_fold_device.append(device)
        n_f, n_terms = len(FACTORS), len(batch.term_circ)
        values = run.term_values.cpu().numpy()
        equal = all(np.array_equal(values[f], plain[f].term_values.cpu().numpy()) for f in range(n_f))
        worst = max(float(np.max(np.abs(values[f] - plain[f].term_values.cpu().numpy()))) for f in range(n_f))
        stats = run.traj_stats.cpu().numpy().reshape(TRAJECTORIES, n_f, count, -1)
        med = statistics.median
        row = {"steps": steps, "circuits": count, "terms_per_circuit": nq, "max_bond": 32, "trajectories": TRAJECTORIES,
               "noise_factors": list(FACTORS), "records": int(batch.ops.shape[0]), "schedule_entries": int(sch.sched.shape[0]),
               "records_host_folded": [int(p.batch.ops.shape[0]) for p in plain],
               "fused_ms": 1e3 * med(t_fused), "fused_lowering_ms": 1e3 * lower_s, "fused_schedules_ms": 1e3 * sched_s,
               "fused_device_ms": 1e3 * med(t_device), "fused_device_events_ms": 1e3 * med(t_events),
               "host_folding_ms": 1e3 * med([h + d for h, d in zip(t_fold_host, t_fold_device)]),
               "host_folding_lowering_ms": 1e3 * med(t_fold_host), "host_folding_device_ms": 1e3 * med(t_fold_device),
               "fused_ms_all": [1e3 * t for t in t_fused], "host_folding_ms_all": [1e3 * (h + d) for h, d in zip(t_fold_host, t_fold_device)],
               "bit_equal": bool(equal), "largest_term_difference": worst,
               "decompositions_per_unit": [float(stats[:, f, :, 3].mean()) for f in range(n_f)],
               "decompositions_per_unit_host_folded": [float(p.traj_stats[:, :, 3].mean()) for p in plain],
               "unconverged": float(stats[..., 4].sum()), "largest_bond": int(run.bond.max()),
               "worst_error_bound": float(run.error_bound.max()), "worst_mitigated_std_error": float(run.mitigated_std_error.max()),
               "mean_term_std_error": [float(run.term_std_error[f].mean()) for f in range(n_f)]}
        assert n_terms == count * nq
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
