"""Times the matrix-product-state simulator (csrc/mps.hip: mlqem_mps_run_f64, mlqem_mps_terms_f64, mlqem_mps_finish_f64) on the
MI355X and writes profiles/mps_micro.json.

    python scripts/mps_micro.py [--quick] [--out profiles/mps_micro.json]

Per shape: ``tfim_circuit(100, s, J, two_q="cx")`` with J ~ U(0, 0.66 pi), 1 024 circuits x 100 single-Z terms at bond 32, for
s = 1, 3, 5 Trotter steps; ideal (one unit per circuit, the fused lowering) and under the synthetic backend's depolarising +
readout model with 16 trajectories per circuit (16 384 units, the unfused lowering).  The whole ``run_mps`` call (upload, the
launches of every chunk, the finish launch; host clock around a device synchronisation; ideal: the median of 3 after one warm-up;
noisy: one call after a warm-up on the first 64 circuits; the lowering on the host is timed apart).  Reported: ms, decompositions
(SVDs) per second over all units, the worst ``error_bound``, the largest bond.  Beside them the numpy interpreter of tests/mps_cases.py on ONE circuit of each shape (LAPACK SVDs, host clock).
``--quick``: 64 circuits.  Nothing here asserts a speed or a ratio.
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
from blackwater import sim  # noqa: E402
from blackwater.data.synthetic import synthetic_backend, tfim_circuit  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=3, warm=None):
    (warm or fn)()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_micro.json"))
    args = ap.parse_args()
    nq, count, trajectories = 100, 64 if args.quick else 1024, 16
    rng = np.random.default_rng(42)
    couplings = rng.uniform(0.0, 0.66 * math.pi, size=count)
    noise = sim.NoiseModel.from_backend(synthetic_backend(nq, "cx"))
    obs = [mc.single_z(nq)] * count
    rows = []
    for steps in (1, 3, 5):
        circuits = [tfim_circuit(nq, steps, float(j), two_q="cx") for j in couplings]
        for noisy in (False, True):
            t0 = time.perf_counter()
            batch = sim.compile_mps(circuits, obs, noise if noisy else None, trajectories if noisy else None)
            lower_s = time.perf_counter() - t0
            if noisy:
                head = sim.compile_mps(circuits[:64], obs[:64], noise, trajectories)
                seconds, res = timed(lambda: sim.run_mps(batch, seed=1, device=DEV, keep_trajectories=True), reps=1,
                                     warm=lambda: sim.run_mps(head, seed=1, device=DEV))
            else:
                seconds, res = timed(lambda: sim.run_mps(batch, seed=1, device=DEV, keep_trajectories=True))
            svds = float(res.traj_stats[:, :, 3].sum())
            row = {"steps": steps, "circuits": count, "terms_per_circuit": nq, "max_bond": 32, "trajectories": trajectories if noisy else None,
                   "records": int(batch.ops.shape[0]), "lowering_ms": 1e3 * lower_s, "run_ms": 1e3 * seconds, "decompositions": svds,
                   "decompositions_per_second": svds / seconds, "worst_error_bound": float(res.error_bound.max()),
                   "largest_bond": int(res.bond.max())}
            if noisy:
                row["worst_std_error"] = float(res.term_std_error.max())
            else:
                t0 = time.perf_counter()
                ref = mc.interpret(batch, count // 2)
                row["numpy_interpreter_one_circuit_ms"] = 1e3 * (time.perf_counter() - t0)
                row["numpy_interpreter_decompositions"] = ref["n_dec"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
