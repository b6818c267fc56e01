"""Times zero-noise extrapolation on the batched simulator two ways, on the same box in the same call.

    python scripts/zne_micro.py [--out profiles/zne_micro.json] [--quick]

Shape: 4 096 lima-regime circuits (the 900 golden circuits tiled; 5 qubits), per-classical-bit <Z>, ``NoiseModel.from_backend(lima)``
(5-qubit density matrices: the workgroup-per-run kernel), noise factors (1, 3, 5), two-qubit local folding, a quadratic through them.

  fused      the path of ``blackwater.sim.zne.zne_run``: ``compile_programs`` ONCE, ``build_schedules``, upload, one
             ``ops.sim_run_folded`` over all 3 x 4 096 runs, one ``ops.zne_combine``;
  unfused    the same work the way it had to be done before the schedules existed: ``fold_circuit`` per factor on the host,
             ``compile_programs`` per factor, upload, one ``ops.sim_run`` per factor, the weighted sum in numpy.
Both are timed end to end on the host clock (device wait included, the QASM parsed once outside both), with the host stages beside the
total, and per launch with device events around the ops calls with the buffers resident and the outputs given.  3 warm-ups, median
of 20.  ``schedule_entries`` is the total schedule length (the records all runs apply); ``records_per_second`` is that over the
folded launch.  No speed-up is asserted anywhere: the numbers are recorded as they come.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sim_cases as sc  # noqa: E402
from blackwater import sim, zne  # noqa: E402
from blackwater.data.backends import StaticBackend  # noqa: E402
from blackwater.data.circuit import Circuit  # noqa: E402
from blackwater.native import ops  # noqa: E402

DEV = "cuda:0"
WARMUP, REPS = 3, 20


def event_seconds(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def median_of(fn):
    """Median over REPS calls after WARMUP of whatever dict of seconds ``fn`` returns."""
    rows = [fn() for _ in range(WARMUP + REPS)][WARMUP:]
    return {k: statistics.median(r[k] for r in rows) for k in rows[0]}


def sim_args(t):
    return (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"])


def fused(circuits, observables, noise, strategy):
    weights = strategy.weights()
    keep = {}

    def end_to_end():
        t0 = time.perf_counter()
        batch = sim.compile_programs(circuits, observables, noise)
        t1 = time.perf_counter()
        sch = zne.build_schedules(batch, circuits, strategy.noise_factors, strategy.noise_amplifier)
        t2 = time.perf_counter()
        t, s = batch.to(DEV), sch.to(DEV)
        w = torch.from_numpy(weights).to(DEV)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        values, term_values, norm = ops.sim_run_folded(*sim_args(t), s["sched_ptr"], s["sched"], s["ids"], sch.n_wave, sch.n_wg,
                                                       len(sch.noise_factors))
        mv, mt = ops.zne_combine(term_values, w, t["term_ptr"], t["coeff"])
        out = mv.cpu().numpy()
        t4 = time.perf_counter()
        keep.update(batch=batch, sch=sch, t=t, s=s, w=w, values=values, term_values=term_values, norm=norm, mv=mv, mt=mt, out=out)
        return {"total_seconds": t4 - t0, "lowering_seconds": t1 - t0, "schedule_seconds": t2 - t1, "upload_seconds": t3 - t2,
                "launch_and_copy_seconds": t4 - t3}

    p = median_of(end_to_end)
    batch, sch, t, s = keep["batch"], keep["sch"], keep["t"], keep["s"]

    def launches():
        a = event_seconds(lambda: ops.sim_run_folded(*sim_args(t), s["sched_ptr"], s["sched"], s["ids"], sch.n_wave, sch.n_wg,
                                                     len(sch.noise_factors), values=keep["values"], term_values=keep["term_values"],
                                                     norm=keep["norm"]))
        b = event_seconds(lambda: ops.zne_combine(keep["term_values"], keep["w"], t["term_ptr"], t["coeff"], mitigated_terms=keep["mt"],
                                                  mitigated_values=keep["mv"]))
        return {"folded_launch_seconds": a, "combine_launch_seconds": b}

    p.update(median_of(launches))
    entries = int(sch.sched_ptr[-1])
    p.update({"path": "fused", "circuits": len(batch), "runs": int(sch.ids.size), "records": int(batch.op_ptr[-1]), "schedule_entries": entries,
              "schedule_bytes": 4 * entries, "n_wave": sch.n_wave, "n_wg": sch.n_wg,
              "records_per_second": entries / p["folded_launch_seconds"],
              "entries_per_factor": [int(x) for x in np.diff(sch.sched_ptr).reshape(len(sch.noise_factors), -1).sum(axis=1)]})
    return p, keep["out"]


def unfused(circuits, observables, noise, strategy):
    weights = strategy.weights()
    keep = {}

    def end_to_end():
        t0 = time.perf_counter()
        folded = [[zne.fold_circuit(c, lam, strategy.noise_amplifier) for c in circuits] for lam in strategy.noise_factors]
        t1 = time.perf_counter()
        batches = [sim.compile_programs(f, observables, noise) for f in folded]
        t2 = time.perf_counter()
        ts = [b.to(DEV) for b in batches]
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        outs = [ops.sim_run(*sim_args(t), t["ids"], t["n_wave"], t["n_wg"]) for t in ts]
        per_factor = np.stack([o[0].cpu().numpy() for o in outs])
        mitigated = weights[0] * per_factor[0]
        for f in range(1, len(weights)):
            mitigated = mitigated + weights[f] * per_factor[f]
        t4 = time.perf_counter()
        keep.update(batches=batches, ts=ts, outs=outs, out=mitigated)
        return {"total_seconds": t4 - t0, "fold_seconds": t1 - t0, "lowering_seconds": t2 - t1, "upload_seconds": t3 - t2,
                "launch_copy_and_combine_seconds": t4 - t3}

    p = median_of(end_to_end)
    ts, outs = keep["ts"], keep["outs"]

    def launches():
        per = [event_seconds(lambda t=t, o=o: ops.sim_run(*sim_args(t), t["ids"], t["n_wave"], t["n_wg"], values=o[0], term_values=o[1], norm=o[2]))
               for t, o in zip(ts, outs)]
        return {"launch_seconds": sum(per), **{f"launch_seconds_factor_{k}": v for k, v in enumerate(per)}}

    p.update(median_of(launches))
    p.update({"path": "unfused", "circuits": len(circuits), "records": int(sum(int(b.op_ptr[-1]) for b in keep["batches"]))})
    return p, keep["out"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zne_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("zne_micro: needs the GPU (there is no host path to time)")
    scale = 16 if args.quick else 1
    texts, _, _ = sc.golden_circuits()
    circuits = [Circuit.from_any(texts[k % len(texts)]) for k in range(4096 // scale)]
    observables = [sim.measured_z(c) for c in circuits]
    lima = StaticBackend.from_json(os.path.join(sc.GOLDEN, "fake_lima_backend_props.json"))
    noise = sim.NoiseModel.from_backend(lima)
    strategy = zne.ZNEStrategy(noise_factors=(1, 3, 5), noise_amplifier=zne.TwoQubitAmplifier(), extrapolator=zne.QuadraticExtrapolator())
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "noise_factors": [1, 3, 5], "points": [],
              "method": f"host clock end to end (device wait included, QASM parsed outside), device events per launch with the buffers "
                        f"resident and the outputs given; {WARMUP} warm-ups, median of {REPS}"}
    a, out_a = fused(circuits, observables, noise, strategy)
    print(json.dumps(a), flush=True)
    b, out_b = unfused(circuits, observables, noise, strategy)
    print(json.dumps(b), flush=True)
    result["points"] = [a, b]
    result["max_abs_difference_of_the_mitigated_values"] = float(np.abs(out_a - out_b).max())
    result["ratios"] = {"end_to_end_unfused_over_fused": b["total_seconds"] / a["total_seconds"],
                        "host_lowering_unfused_over_fused": (b["fold_seconds"] + b["lowering_seconds"]) / (a["lowering_seconds"] + a["schedule_seconds"]),
                        "launches_unfused_over_fused": b["launch_seconds"] / (a["folded_launch_seconds"] + a["combine_launch_seconds"])}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
