"""Times measurement shots on the batched simulator (csrc/sim.hip: mlqem_sim_run_measured_f64, mlqem_sim_sample_f64) and, beside
them, the host cost of the same draws with ``numpy.random.Generator.multinomial`` on the same box in the same call.

    python scripts/shots_micro.py [--out profiles/shots_micro.json] [--quick]

  lima_vector    4 096 lima-regime circuits (the 900 golden circuits tiled; 5 qubits), per-classical-bit <Z> (one all-Z group, 32
                 outcomes), state-vector mode, 10 000 shots;
  lima_density   the same under ``NoiseModel.from_backend(lima)`` with readout ops;
  random11       1 024 random 11-qubit circuits of 200 gates, 12 Pauli terms over I X Y Z (several groups of 2 048 outcomes each: the
                 workgroup variant of the sampler), 10 000 shots.
Per point the SIMULATE launch (``ops.sim_run_measured``: the exact values plus the outcome probabilities of every group) and the
SAMPLE launch (``ops.sim_sample``: CDF, draws, counts, estimates, values, variances) are timed separately: buffers resident, outputs
given, device events, 3 warm-ups, median of 20.  ``draws`` = groups x shots, ``draws_per_second`` = draws over the sample launch.
``simulate_plain_seconds`` is ``ops.sim_run`` on the same circuits lowered without shots, for what the measurement tail adds.  The
host figure draws the same number of outcomes per group with ``Generator.multinomial`` from the device's probabilities (read back,
clipped at 0 and normalised: they are the oracle's within 1e-12), host clock, median of 3, on the first ``host_groups`` groups and
scaled to the point's size (said so in the result).  No ratio is asserted anywhere.
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
from blackwater import sim  # noqa: E402
from blackwater.data.backends import StaticBackend  # noqa: E402
from blackwater.native import ops  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    times = []
    for rep in range(23):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if rep >= 3:
            times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times)


def point(name, circuits, observables, noise, shots, host_groups):
    t0 = time.perf_counter()
    batch = sim.compile_programs(circuits, observables, noise, shots=shots)
    lower_s = time.perf_counter() - t0
    plain = sim.compile_programs(circuits, observables, noise)
    t, tp = batch.to(DEV), plain.to(DEV)
    b, n_terms, n_out, n_groups = len(batch), int(batch.term_ptr[-1]), int(batch.prob_ptr[-1]), len(batch.group_circ)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)   # noqa: E731
    sim_out = {"values": f64(b), "term_values": f64(n_terms), "norm": f64(b), "probs": f64(n_out)}
    smp_out = {"counts": torch.zeros(n_out, dtype=torch.int32, device=DEV), "term_values": f64(n_terms), "values": f64(b), "variance": f64(b)}
    plain_out = {"values": f64(b), "term_values": f64(n_terms), "norm": f64(b)}
    units, u_wave, u_wg = batch.sample_units(1)
    units = torch.from_numpy(units).to(DEV)
    keys = torch.from_numpy(sim.default_run_keys(b)).to(DEV)

    def simulate():
        ops.sim_run_measured(t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"],
                             t["prob_ptr"], n_out, t["ids"], t["n_wave"], t["n_wg"], **sim_out)

    def sample():
        ops.sim_sample(t["circ"], t["term_ptr"], t["terms"], t["coeff"], t["group_ptr"], t["term_group"], t["prob_ptr"], t["group_circ"],
                       sim_out["probs"], keys, shots, 0, units, u_wave, u_wg, **smp_out)

    def simulate_plain():
        ops.sim_run(tp["circ"], tp["op_ptr"], tp["ops"], tp["params"], tp["term_ptr"], tp["terms"], tp["coeff"], tp["ids"], tp["n_wave"],
                    tp["n_wg"], **plain_out)

    sim_s, smp_s, plain_s = timed(simulate), timed(sample), timed(simulate_plain)
    counts = smp_out["counts"].cpu().numpy()
    assert int(counts.sum()) == n_groups * shots
    draws = n_groups * shots
    p = {"point": name, "circuits": b, "groups": n_groups, "outcomes_per_group": int(n_out // n_groups), "shots": shots, "draws": draws,
         "sample_n_wave": u_wave, "sample_n_wg": u_wg, "simulate_seconds": sim_s, "simulate_plain_seconds": plain_s,
         "sample_seconds": smp_s, "draws_per_second": draws / smp_s, "host_lowering_seconds": lower_s,
         "tail_records": int(batch.circ[:, 3].sum())}
    probs = np.clip(sim_out["probs"].cpu().numpy(), 0.0, None)
    ptr = batch.prob_ptr
    sub = [probs[int(ptr[g]):int(ptr[g + 1])] for g in range(min(host_groups, n_groups))]
    sub = [q / q.sum() for q in sub]

    def host():
        rng = np.random.default_rng(0)
        t1 = time.perf_counter()
        for q in sub:
            rng.multinomial(shots, q)
        return time.perf_counter() - t1

    h_s = statistics.median([host(), host(), host()]) * n_groups / len(sub)
    p.update({"host_multinomial_seconds": h_s, "host_groups": len(sub), "host_draws_per_second": draws / h_s,
              "host_note": f"Generator.multinomial timed on {len(sub)} groups, scaled to {n_groups}"})
    print(json.dumps(p), flush=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shots_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits, not a measurement")
    ap.add_argument("--workload", action="store_true",
                    help="only launch (for `rocprofv3 --pmc <counters> -- python scripts/shots_micro.py --workload`): lima_vector in "
                         "full and random11 at an eighth, nothing written")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shots_micro: needs the GPU (there is no host path to time)")
    if args.workload:
        texts, _, _ = sc.golden_circuits()
        tiled = [texts[k % len(texts)] for k in range(4096)]
        point("lima_vector", tiled, [sim.measured_z(t) for t in tiled], None, 10000, 64)
        rand = [sc.random_program(11, 200, seed=k) for k in range(128)]
        point("random11_eighth", rand, [sc.term_set(11, seed=k) for k in range(128)], None, 10000, 4)
        return
    scale = 16 if args.quick else 1
    texts, _, _ = sc.golden_circuits()
    tiled = [texts[k % len(texts)] for k in range(4096 // scale)]
    zs = [sim.measured_z(t) for t in tiled]
    lima = StaticBackend.from_json(os.path.join(sc.GOLDEN, "fake_lima_backend_props.json"))
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "points": [],
              "method": "device events around ops.sim_run_measured and ops.sim_sample separately, buffers resident and outputs given, 3 "
                        "warm-ups, median of 20; numpy's Generator.multinomial on the host clock, median of 3, on a subset and scaled"}

    def save(p):
        result["points"].append(p)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)

    save(point("lima_vector", tiled, zs, None, 10000, 1024 // scale))
    save(point("lima_density", tiled, zs, sim.NoiseModel.from_backend(lima), 10000, 1024 // scale))
    rand = [sc.random_program(11, 200, seed=k) for k in range(1024 // scale)]
    save(point("random11", rand, [sc.term_set(11, seed=k) for k in range(len(rand))], None, 10000, 64 // scale))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
