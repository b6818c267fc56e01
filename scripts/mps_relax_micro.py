"""Times thermal relaxation on the matrix-product-state path (csrc/mps.hip: the NOISE1 / NOISE2 records of mlqem_mps_run_f64) on
the MI355X beside the depolarising model on the same circuits and calibration table, and writes profiles/mps_relax_micro.json.

    python scripts/mps_relax_micro.py [--quick] [--parent-lib PATH] [--out profiles/mps_relax_micro.json]

Per shape: ``tfim_circuit(100, s, J, two_q="cx")`` with J ~ U(0, 0.66 pi), s = 1, 3 Trotter steps, 128 circuits x 16 trajectories
x 100 single-Z terms at bond 32, under two models of ``synthetic_backend(100, "cx")``:

  depolarising   ``NoiseModel.from_backend(table)``: DEPOL records, the Pauli insertions of DESIGN.md 3.16;
  relaxation     ``NoiseModel.from_backend(table, thermal_relaxation=True)`` lowered with ``thermal_relaxation=True``: one NOISE
                 record per gate, quantum jumps at the orthogonality centre.

Measured: the wall clock of ``run_mps`` on the lowered batch (upload, launches, finish; host clock around a device
synchronisation; the median of 3 after a warm-up on the first 16 circuits), the decompositions per (circuit, trajectory) unit
from the stats, the worst ``error_bound`` and the largest bond.  These are first measurements: nothing here asserts a speed or
a ratio.  ``--quick``: 16 circuits.

``--parent-lib PATH``: a libmlqem_hip.so built from the parent commit.  The outputs of every case of ``tests/mps_cases.grid()``
(values, terms, norms, discarded, error_bound, bond and the per-trajectory terms and stats) are then computed twice, each in a
fresh process, once under each library (``MLQEM_LIB``), and ``grid_byte_equal`` records whether their bytes are the same: a
program without the new kinds must be today's program.
"""
import argparse
import hashlib
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]

DEV = "cuda:0"
TRAJECTORIES, SEED = 16, 1


def grid_digests():
    """``{case id: sha256 of its output arrays}`` over ``mps_cases.grid()``, under the library this process loaded."""
    import mps_cases as mc
    from blackwater.sim import run_mps

    out = {}
    for case in mc.grid():
        res = run_mps(mc.lower(case), seed=case["seed"], device=DEV, keep_trajectories=True)
        h = hashlib.sha256()
        for k in ("values", "term_values", "norm", "discarded", "error_bound", "bond", "std_error", "term_std_error", "traj_term_values",
                  "traj_stats"):
            v = getattr(res, k)
            if v is not None:
                h.update(v.cpu().numpy().tobytes())
        out[case["id"]] = h.hexdigest()
    return out


def digests_under(lib):
    """``grid_digests`` in a fresh process that loads ``lib`` (None: the tree's own library)."""
    env = dict(os.environ)
    env.pop("MLQEM_LIB", None)
    if lib is not None:
        env["MLQEM_LIB"] = os.path.abspath(lib)
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "--digests"], env=env, check=True, capture_output=True, text=True)
    return json.loads(done.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--digests", action="store_true", help="print the digests of mps_cases.grid() under the loaded library and exit")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_relax_micro.json"))
    args = ap.parse_args()
    if args.digests:
        print(json.dumps(grid_digests()))
        return
    # the two comparison processes come first: this process has not opened the device yet
    equal = None
    if args.parent_lib is not None:
        parent, new = digests_under(args.parent_lib), digests_under(None)
        equal = {"cases": len(new), "byte_equal": parent == new, "differing": sorted(k for k in new if parent.get(k) != new[k])}
        print(json.dumps(equal), flush=True)

    import numpy as np
    import torch

    import mps_cases as mc
    from blackwater import sim
    from blackwater.data.synthetic import synthetic_backend, tfim_circuit

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    nq, count = 100, 16 if args.quick else 128
    couplings = np.random.default_rng(42).uniform(0.0, 0.66 * math.pi, size=count)
    table = synthetic_backend(nq, "cx")
    models = {"depolarising": (sim.NoiseModel.from_backend(table), False),
              "relaxation": (sim.NoiseModel.from_backend(table, thermal_relaxation=True), True)}
    obs = [mc.single_z(nq)] * count
    rows = []
    for steps in (1, 3):
        circuits = [tfim_circuit(nq, steps, float(j), two_q="cx") for j in couplings]
        for name, (noise, relax) in models.items():
            t0 = time.perf_counter()
            batch = sim.compile_mps(circuits, obs, noise, TRAJECTORIES, thermal_relaxation=relax)
            lower_s = time.perf_counter() - t0
            warm = sim.compile_mps(circuits[:16], obs[:16], noise, TRAJECTORIES, thermal_relaxation=relax)
            sim.run_mps(warm, seed=SEED, device=DEV)
            times = []
            for _ in range(3):
                seconds, res = clock(lambda: sim.run_mps(batch, seed=SEED, device=DEV, keep_trajectories=True))
                times.append(seconds)
            stats = res.traj_stats.cpu().numpy()
            kinds = np.bincount(batch.ops[:, 0], minlength=12)
            row = {"steps": steps, "model": name, "circuits": count, "trajectories": TRAJECTORIES, "terms_per_circuit": nq, "max_bond": 32,
                   "records": int(batch.ops.shape[0]), "depol_records": int(kinds[6] + kinds[7]), "noise_records": int(kinds[10] + kinds[11]),
                   "lowering_ms": 1e3 * lower_s, "run_mps_ms": 1e3 * statistics.median(times), "run_mps_ms_all": [1e3 * t for t in times],
                   "decompositions_per_unit": float(stats[:, :, 3].mean()), "unconverged": float(stats[:, :, 4].sum()),
                   "most_sweeps": int(stats[:, :, 5].max()), "largest_bond": int(res.bond.max()),
                   "worst_error_bound": float(res.error_bound.max()), "worst_trajectory_error_bound": float(stats[:, :, 1].max()),
                   "mean_term_std_error": float(res.term_std_error.mean()), "worst_norm_defect": float((res.norm - 1.0).abs().max())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    for steps in (1, 3):
        a, b = (next(r for r in rows if r["steps"] == steps and r["model"] == m) for m in ("depolarising", "relaxation"))
        print(f"steps {steps}: decompositions x{b['decompositions_per_unit'] / a['decompositions_per_unit']:.2f}, "
              f"run_mps x{b['run_mps_ms'] / a['run_mps_ms']:.2f}")
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "grid_of_tests_mps_cases": equal}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
