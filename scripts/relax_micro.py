"""Times the fused noise records (MLQEM_SIM_OP_NOISE1 / NOISE2 of csrc/sim.hip) on the lima workload, with the method of
scripts/sim_micro.py: buffers uploaded once, outputs given, device events around ``ops.sim_run``, 3 warm-ups, median of 20.

    python scripts/relax_micro.py [--out profiles/relax_micro.json] [--quick] [--old-only] [--parent FILE]

  lima_relax           4 096 lima circuits (the 900 golden circuits tiled; 5-qubit density matrices, the workgroup variant) under
                       ``NoiseModel.from_backend(lima, readout=False, thermal_relaxation=True)``;
  lima_relax_readout   the same with the readout ops;
  lima_density         the same batch under the default depolarising + readout model, in the same process: the 323 us shape of
                       profiles/sim_micro.json;
  lima_vector, random11   the two other kernel shapes of profiles/sim_micro.json, which contain none of the new records.
The numpy Kraus oracle of tests/relax_cases.py is timed beside the relaxation points on the host clock (median of 3, on a subset,
scaled).  ``--old-only`` measures the three old shapes alone (they are all a library built from the parent commit can run:
``MLQEM_LIB=<that library>``), and ``--parent FILE`` copies such a run's points into the result as ``parent_points``, so that one
file holds both sides measured on one box.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import relax_cases as rc  # noqa: E402
import sim_cases as sc  # noqa: E402
import sim_micro  # noqa: E402
from blackwater import sim  # noqa: E402
from blackwater.data.circuit import Circuit  # noqa: E402
from blackwater.native import ops  # noqa: E402
from blackwater.sim import program as P  # noqa: E402

DEV = "cuda:0"
# a fused record is one pass in which every entry is read once and written once
sim_micro.PASSES.update({getattr(P, "OP_NOISE1", 10): (0, 1), getattr(P, "OP_NOISE2", 11): (0, 1)})


def point(name, circuits, observables, noise, oracle, oracle_circuits):
    t0 = time.perf_counter()
    batch = sim.compile_programs(circuits, observables, noise)
    lower_s = time.perf_counter() - t0
    t = batch.to(DEV)
    args = (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"], t["n_wave"], t["n_wg"])
    outs = {"values": torch.zeros(len(batch), dtype=torch.float64, device=DEV),
            "term_values": torch.zeros(int(batch.term_ptr[-1]), dtype=torch.float64, device=DEV),
            "norm": torch.zeros(len(batch), dtype=torch.float64, device=DEV)}
    times = []
    for rep in range(23):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.sim_run(*args, **outs)
        b.record()
        torch.cuda.synchronize()
        if rep >= 3:
            times.append(a.elapsed_time(b) * 1e-3)
    seconds = statistics.median(times)
    moved = sim_micro.lds_bytes(batch)
    n_ops = int(batch.op_ptr[-1])
    kinds = {int(k): int(v) for k, v in zip(*[x.tolist() for x in np.unique(batch.ops[:, 0], return_counts=True)])}
    p = {"point": name, "circuits": len(batch), "records": n_ops, "records_by_kind": kinds, "n_wave": batch.n_wave, "n_wg": batch.n_wg,
         "launch_seconds": seconds, "launch_seconds_min": min(times), "launch_seconds_max": max(times),
         "circuits_per_second": len(batch) / seconds, "host_lowering_seconds": lower_s, "lds_bytes": moved,
         "lds_bytes_per_record": moved / max(n_ops, 1), "lds_tb_per_s": moved / seconds * 1e-12}
    if oracle is not None:
        sub = [Circuit.from_any(c) for c in circuits[:oracle_circuits]]
        obs = [o.to_list() if hasattr(o, "to_list") else o for o in observables[:oracle_circuits]]

        def once():
            t1 = time.perf_counter()
            for c, o in zip(sub, obs):
                oracle(c, o, noise)
            return time.perf_counter() - t1

        o_s = statistics.median([once(), once(), once()]) * len(batch) / len(sub)
        p.update({"oracle_seconds": o_s, "oracle_circuits": len(sub), "oracle_note": f"timed on {len(sub)} circuits, scaled to {len(batch)}",
                  "speedup_vs_oracle": o_s / seconds})
    print(json.dumps(p), flush=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits, not a measurement")
    ap.add_argument("--old-only", action="store_true", help="only the shapes that hold none of the new records")
    ap.add_argument("--parent", default=None, help="a result of --old-only under the parent commit's library, copied in as parent_points")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("relax_micro: needs the GPU (there is no host path to time)")
    scale = 16 if args.quick else 1
    texts, _, _ = sc.golden_circuits()
    tiled = [texts[k % len(texts)] for k in range(4096 // scale)]
    zs = [sim.measured_z(t) for t in tiled]
    lima = rc.lima()
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "library": os.environ.get("MLQEM_LIB", "this commit's"), "points": [],
              "method": "device events around ops.sim_run with the buffers resident and the outputs given, 3 warm-ups, median of 20 "
                        "(min and max beside it); the numpy Kraus oracle on the host clock, median of 3, on a subset and scaled"}

    def save(p):
        result["points"].append(p)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)

    if args.parent:
        with open(args.parent) as fh:
            parent = json.load(fh)
        result["parent_points"], result["parent_library"] = parent["points"], parent.get("library")
    if not args.old_only:
        for name, readout in (("lima_relax", False), ("lima_relax_readout", True)):
            noise = sim.NoiseModel.from_backend(lima, readout=readout, thermal_relaxation=True)
            save(point(name, tiled, zs, noise, rc.simulate, 32 // scale))
    save(point("lima_density", tiled, zs, sim.NoiseModel.from_backend(lima), None, 0))
    save(point("lima_vector", tiled, zs, None, None, 0))
    rand = [sc.random_program(11, 200, seed=k) for k in range(1024 // scale)]
    save(point("random11", rand, [sc.term_set(11, seed=k) for k in range(len(rand))], None, None, 0))
    if not args.old_only:   # once more, after the others: what two measurements of one shape in one process differ by
        save(point("lima_density_again", tiled, zs, sim.NoiseModel.from_backend(lima), None, 0))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
