"""Times Pauli twirling on the matrix-product-state path (csrc/mps.hip: the TWIRL_OPEN / TWIRL_CLOSE records of mlqem_mps_run_f64 and
mlqem_mps_run_folded_f64) on the MI355X and writes profiles/mps_twirl_micro.json.

    python scripts/mps_twirl_micro.py [--quick] [--parent-lib PATH] [--out profiles/mps_twirl_micro.json]

Setup: 128 ``tfim_circuit(100, s, J, two_q="cx")`` with J ~ U(0, 0.66 pi), s = 1, 3 Trotter steps, x 16 trajectories x 100 single-Z
terms at bond 32, under ``NoiseModel.from_backend(synthetic_backend(100, "cx")).with_cx_over_rotation(0.2)``: the depolarising
model with the coherent cx error of the reference's noise study.  All numbers are first measurements: nothing here asserts a
speed, a ratio or an error.

  (a) ``run_mps`` on the batch lowered with ``pauli_twirl=True`` against the untwirled batch: wall clock (upload, launches, finish;
      host clock around a device synchronisation), the median of 3 after a warm-up on the first 16 circuits.
  (b) the device route -- ONE lowering with ``pauli_twirl=True`` plus ONE run of 16 trajectories, each with its own twirls -- against
      the host route: 16 instances of ``data.synthetic.pauli_twirl`` per circuit, each lowered and run with one trajectory.
  (c) a mitigation table on 64 circuits of 24 qubits (1 step; 64 trajectories): mean |error| against the ideal values of the ideal
      MPS run, unmitigated and with ZNE at factors (1, 3), linear and exponential, each with and without twirling.
  (d) ``--parent-lib PATH`` (a libmlqem_hip.so built from the parent commit): the output arrays of every case of
      ``tests/mps_cases.grid()`` under each library, each in a fresh process (``MLQEM_LIB``), and whether their bytes are equal: a
      program without the new kinds must be today's program.

``--quick``: 16 circuits in (a), (b) and (c).
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

DEV = "cuda:0"
TRAJECTORIES, SEED, THETA = 16, 1, 0.2


def main():
    import mps_relax_micro as base   # the digests of mps_cases.grid() under a library, each in a fresh process

    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_twirl_micro.json"))
    args = ap.parse_args()
    # the two comparison processes come first: this process has not opened the device yet
    equal = None
    if args.parent_lib is not None:
        parent, new = base.digests_under(args.parent_lib), base.digests_under(None)
        equal = {"cases": len(new), "byte_equal": parent == new, "differing": sorted(k for k in new if parent.get(k) != new[k])}
        print(json.dumps(equal), flush=True)

    import numpy as np
    import torch

    import mps_cases as mc
    from blackwater import sim
    from blackwater.data.synthetic import pauli_twirl, synthetic_backend, tfim_circuit
    from blackwater.sim import zne

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    nq, count = 100, 16 if args.quick else 128
    couplings = np.random.default_rng(42).uniform(0.0, 0.66 * math.pi, size=count)
    noise = sim.NoiseModel.from_backend(synthetic_backend(nq, "cx")).with_cx_over_rotation(THETA)
    obs = [mc.single_z(nq)] * count
    rows, routes = [], []
    for steps in (1, 3):
        circuits = [tfim_circuit(nq, steps, float(j), two_q="cx") for j in couplings]
        lowering = {}
        for twirl in (False, True):   # (a)
            t0 = time.perf_counter()
            batch = sim.compile_mps(circuits, obs, noise, TRAJECTORIES, pauli_twirl=twirl)
            lowering[twirl] = time.perf_counter() - t0
            sim.run_mps(sim.compile_mps(circuits[:16], obs[:16], noise, TRAJECTORIES, pauli_twirl=twirl), seed=SEED, device=DEV)
            times = []
            for _ in range(3):
                seconds, res = clock(lambda: sim.run_mps(batch, seed=SEED, device=DEV, keep_trajectories=True))
                times.append(seconds)
            stats = res.traj_stats.cpu().numpy()
            kinds = np.bincount(batch.ops[:, 0], minlength=19)
            row = {"steps": steps, "pauli_twirl": twirl, "circuits": count, "trajectories": TRAJECTORIES, "terms_per_circuit": nq, "max_bond": 32,
                   "records": int(batch.ops.shape[0]), "twirl_records": int(kinds[17] + kinds[18]), "lowering_ms": 1e3 * lowering[twirl],
                   "run_mps_ms": 1e3 * statistics.median(times), "run_mps_ms_all": [1e3 * t for t in times],
                   "decompositions_per_unit": float(stats[:, :, 3].mean()), "unconverged": float(stats[:, :, 4].sum()),
                   "largest_bond": int(res.bond.max()), "worst_error_bound": float(res.error_bound.max()),
                   "mean_term_std_error": float(res.term_std_error.mean())}
            rows.append(row)
            print(json.dumps(row), flush=True)
        # (b) the host route: 16 twirl instances per circuit, each lowered and run with one trajectory
        device_s = lowering[True] + 1e-3 * rows[-1]["run_mps_ms"]
        t0 = time.perf_counter()
        lower_s = run_s = 0.0
        for k in range(TRAJECTORIES):
            t1 = time.perf_counter()
            instance = sim.compile_mps([pauli_twirl(c, 1000 * k + j, two_q=("cx",)) for j, c in enumerate(circuits)], obs, noise, 1)
            lower_s += time.perf_counter() - t1
            seconds, _ = clock(lambda: sim.run_mps(instance, seed=SEED + k, device=DEV))
            run_s += seconds
        host_s = time.perf_counter() - t0
        route = {"steps": steps, "circuits": count, "instances": TRAJECTORIES, "device_route_ms": 1e3 * device_s,
                 "device_lowering_ms": 1e3 * lowering[True], "host_route_ms": 1e3 * host_s, "host_lowering_ms": 1e3 * lower_s,
                 "host_run_ms": 1e3 * run_s}
        routes.append(route)
        print(json.dumps(route), flush=True)

    # (c) the mitigation table
    nq, count, n_traj = 24, 16 if args.quick else 64, 64
    couplings = np.random.default_rng(43).uniform(0.0, 0.66 * math.pi, size=count)
    circuits = [tfim_circuit(nq, 1, float(j), two_q="cx") for j in couplings]
    obs = [mc.single_z(nq)] * count
    noise = sim.NoiseModel.from_backend(synthetic_backend(nq, "cx")).with_cx_over_rotation(THETA)
    ideal = sim.mps_expectation_values(circuits, obs, device=DEV).term_values.cpu().numpy()
    table = []
    for twirl in (False, True):
        plain = sim.mps_expectation_values(circuits, obs, noise, trajectories=n_traj, seed=SEED, device=DEV, pauli_twirl=twirl)
        entry = {"pauli_twirl": twirl, "unmitigated": float(np.abs(plain.term_values.cpu().numpy() - ideal).mean())}
        for name, extrapolator in (("zne_linear", zne.LinearExtrapolator()), ("zne_exponential", zne.ExponentialExtrapolator())):
            strategy = zne.ZNEStrategy((1, 3), zne.LocalFoldingAmplifier(gates_to_fold=2), extrapolator)
            run = zne.zne_run(circuits, obs, noise, strategy, DEV, seed=SEED, method="mps", trajectories=n_traj, pauli_twirl=twirl)
            entry[name] = float(np.abs(run.mitigated_terms.cpu().numpy() - ideal).mean())
        table.append(entry)
        print(json.dumps(entry), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "over_rotation": THETA, "rows": rows, "routes": routes,
           "mitigation": {"qubits": nq, "circuits": count, "trajectories": n_traj, "steps": 1, "factors": [1, 3], "mean_abs_error": table},
           "grid_of_tests_mps_cases": equal}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
