"""Times the quantum-trajectory kernels (csrc/sim_traj.hip) with the method of scripts/sim_micro.py: buffers uploaded once, outputs
given, device events around the op, 3 warm-ups, median of 20.

    python scripts/traj_micro.py [--out profiles/traj_micro.json] [--quick]

  line8, line11    1 024 eight-qubit and 256 eleven-qubit random circuits (``synthetic.random_circuit``, depth 8 and 6: the 40-odd
                   records of a lima-regime circuit) under ``NoiseModel.from_backend(synthetic_backend(n), readout=False,
                   thermal_relaxation=True)``, T = 1 024 trajectories: the three launches of ``ops.sim_run_trajectories``.  Beside
                   each, the FLOOR: the state-vector kernel (``ops.sim_run``, noise=None) on the same circuits repeated T times in
                   one batch -- the cost of the gates alone, which the trajectories cannot beat.
  lima5            the 4 096 tiled golden lima circuits (5 qubits) under the thermal lima model: the density-matrix run of the
                   batch (``ops.sim_run``) against T = 1 024 trajectories of it, and the T at which a circuit's standard error
                   reaches 1e-3 (T (se / 1e-3)^2 from the measured standard errors: their median and maximum over the batch).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import relax_cases as rc  # noqa: E402
import sim_cases as sc  # noqa: E402
from blackwater import sim  # noqa: E402
from blackwater.data.synthetic import random_circuit, synthetic_backend  # noqa: E402
from blackwater.native import ops  # noqa: E402

DEV = "cuda:0"


def timed(call):
    times = []
    for rep in range(23):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if rep >= 3:
            times.append(a.elapsed_time(b) * 1e-3)
    return {"seconds": statistics.median(times), "seconds_min": min(times), "seconds_max": max(times)}


def time_trajectories(batch, seed=0):
    t = batch.to(DEV)
    b, n_terms, n_traj = len(batch), int(batch.term_ptr[-1]), batch.trajectories
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=DEV)
    outs = dict(traj_term_values=z(n_traj, n_terms), traj_norm=z(n_traj, b), term_values=z(n_terms), term_std_error=z(n_terms),
                values=z(b), std_error=z(b), norm=z(b))
    keys = torch.arange(b, dtype=torch.int64, device=DEV)
    args = (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"], t["n_wave"], t["n_wg"], keys,
            n_traj, seed)
    out = timed(lambda: ops.sim_run_trajectories(*args, **outs))
    out["std_error"] = outs["std_error"].cpu().numpy()
    return out


def time_plain(batch, repeat=1):
    """``ops.sim_run`` on the batch with every circuit ``repeat`` times (the arrays tiled on the host: every copy its own records)."""
    b = len(batch)
    n_ops, n_terms = int(batch.op_ptr[-1]), int(batch.term_ptr[-1])
    rep = np.arange(repeat, dtype=np.int64)
    circ = np.tile(batch.circ, (repeat, 1))
    op_ptr = np.concatenate([(batch.op_ptr[None, :-1] + rep[:, None] * n_ops).reshape(-1), [repeat * n_ops]])
    term_ptr = np.concatenate([(batch.term_ptr[None, :-1] + rep[:, None] * n_terms).reshape(-1), [repeat * n_terms]])
    ids = (batch.ids[None, :].astype(np.int64) + rep[:, None] * b).astype(np.int32)
    ids = np.concatenate([ids[:, :batch.n_wave].reshape(-1), ids[:, batch.n_wave:].reshape(-1)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    args = (up(circ), up(op_ptr), up(np.tile(batch.ops, (repeat, 1))), up(batch.params), up(term_ptr), up(np.tile(batch.terms, (repeat, 1))),
            up(np.tile(batch.coeff, repeat)), up(ids), batch.n_wave * repeat, batch.n_wg * repeat)
    z = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
    outs = dict(values=z(b * repeat), term_values=z(n_terms * repeat), norm=z(b * repeat))
    return timed(lambda: ops.sim_run(*args, **outs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits and trajectories, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("traj_micro: needs the GPU (there is no host path to time)")
    scale = 16 if args.quick else 1
    n_traj = 1024 // scale
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "trajectories": n_traj, "points": [],
              "method": "device events around the op with the buffers resident and the outputs given, 3 warm-ups, median of 20 "
                        "(min and max beside it)"}

    def save(p):
        print(json.dumps(p), flush=True)
        result["points"].append(p)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)

    for name, n, count, depth in (("line8", 8, 1024, 8), ("line11", 11, 256, 6)):
        circuits = [random_circuit(n, depth, 7000 + k, two_q="cx", measure=False) for k in range(count // scale)]
        obs = ["Z" * n] * len(circuits)
        noise = sim.NoiseModel.from_backend(synthetic_backend(n, "cx"), readout=False, thermal_relaxation=True)
        batch = sim.compile_programs(circuits, obs, noise, trajectories=n_traj)
        traj = time_trajectories(batch)
        se = traj.pop("std_error")
        floor = time_plain(sim.compile_programs(circuits, obs, None), repeat=n_traj)
        save({"point": name, "qubits": n, "circuits": len(circuits), "records": int(batch.op_ptr[-1]),
              "noise_records": int(np.isin(batch.ops[:, 0], (6, 7, 10, 11)).sum()), "trajectories": traj, "vector_floor": floor,
              "ratio_to_floor": traj["seconds"] / floor["seconds"], "std_error_median": float(np.median(se)), "std_error_max": float(se.max())})

    texts, _, _ = sc.golden_circuits()
    tiled = [texts[k % len(texts)] for k in range(4096 // scale)]
    zs = [sim.measured_z(t) for t in tiled]
    noise = sim.NoiseModel.from_backend(rc.lima(), readout=False, thermal_relaxation=True)
    traj = time_trajectories(sim.compile_programs(tiled, zs, noise, trajectories=n_traj))
    se = traj.pop("std_error")
    density = time_plain(sim.compile_programs(tiled, zs, noise))
    need = n_traj * (se / 1e-3) ** 2
    save({"point": "lima5", "qubits": 5, "circuits": len(tiled), "trajectories": traj, "density": density,
          "ratio_to_density": traj["seconds"] / density["seconds"], "std_error_median": float(np.median(se)), "std_error_max": float(se.max()),
          "trajectories_for_1e-3_median": float(np.median(need)), "trajectories_for_1e-3_max": float(need.max())})
    print("wrote", args.out)


if __name__ == "__main__":
    main()
