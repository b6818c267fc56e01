"""Times Pauli-frame sampling (csrc/clifford_frames.hip: mlqem_clifford_sample_f64) on the MI355X and writes
profiles/clifford_frames_micro.json.

    python scripts/clifford_frames_micro.py [--quick] [--out profiles/clifford_frames_micro.json]

Kernel points: buffers uploaded once, every output and the workspace given, device events around ``ops.clifford_sample``, 3 warm-ups,
median of 20, at 10 000 shots, on the shapes of scripts/clifford_micro.py:
  tfim100x100    1 024 ``clifford_tfim_circuit`` circuits of 100 qubits x 100 single-Z terms (one all-Z group per circuit);
  tfim512x100    256 circuits of 512 qubits (the LDS instantiation) x 100 single-Z terms;
  small5         4 096 five-qubit random Clifford circuits x 5 single-Z terms.
Beside each: ``ops.clifford_run`` (the exact path) on the same batch, and the numpy interpreter of tests/clifford_frames_cases.py on
a subset of the circuits on the host clock.  ``frame_steps`` = shots x the records of every (circuit, group): what the lanes walk.
  quality        the 64 100-qubit circuits of ``clifford_cases.quality_corpus`` at 10 000 shots: mean |sampled - exact noisy|.
Nothing here asserts a speed or a ratio.
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

import clifford_cases as cc  # noqa: E402
import clifford_frames_cases as fc  # noqa: E402
import sim_cases as sc  # noqa: E402
from blackwater import sim  # noqa: E402
from blackwater.data.synthetic import clifford_tfim_circuit, synthetic_backend  # noqa: E402
from blackwater.native import ops  # noqa: E402

DEV = "cuda:0"
SHOTS = 10000


def event_seconds(fn):
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


def single_z(n, count, shift):
    return [("".join("Z" if q == (shift + j * max(n // count, 1)) % n else "I" for q in reversed(range(n))), 1.0) for j in range(count)]


def frames_point(name, circuits, observables, noise, subset, shots):
    t0 = time.perf_counter()
    batch = sim.compile_clifford_frames(circuits, observables, noise)
    lower_s = time.perf_counter() - t0
    t = batch.to(DEV)
    keys = torch.arange(len(batch), dtype=torch.int64, device=DEV)
    n_ref, n_terms, b = int(batch.ref_ptr[-1]), len(batch.coeff), len(batch)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
    outs = {"rows": i32(batch.n_rows), "reference": i32(n_ref), "term_sums": i32(n_terms), "term_values": f64(n_terms), "values": f64(b),
            "variance": f64(b)}
    args = (t["n_qubits"], t["op_ptr"], t["ops"], t["thresh"], t["ro_ptr"], t["group_ptr"], t["group_circ"], t["group_mask"], t["ids"],
            batch.n_reg, batch.n_lds, t["masks"], t["term_ptr"], t["coeff"], t["term_mask"], t["gterm_ptr"], t["gterm"], keys, shots, 0,
            batch.max_qubits, t["row_ptr"], batch.n_rows, t["ref_ptr"], n_ref)
    seconds = event_seconds(lambda: ops.clifford_sample(*args, **outs))
    base = batch.clifford
    c = base.to(DEV)
    cargs = (c["n_qubits"], c["op_ptr"], c["ops"], c["pool"], c["units"], c["n_reg"], c["n_lds"], c["masks"], c["term_ptr"], c["coeff"],
             c["comb_ptr"], c["comb_unit"], c["comb_weight"])
    couts = {"unit_ideal": f64(len(base.units)), "unit_noisy": f64(len(base.units)), "ideal_terms": f64(n_terms),
             "noisy_terms": f64(n_terms), "ideal_values": f64(b), "noisy_values": f64(b)}
    exact_s = event_seconds(lambda: ops.clifford_run(*cargs, **couts))
    steps = int(np.diff(base.op_ptr)[batch.group_circ].sum()) * shots
    sampled, exact = outs["term_values"].cpu().numpy(), couts["noisy_terms"].cpu().numpy()
    p = {"point": name, "circuits": b, "qubits_max": batch.max_qubits, "records": int(base.op_ptr[-1]), "groups": len(batch.group_circ),
         "terms": n_terms, "shots": shots, "n_reg": batch.n_reg, "n_lds": batch.n_lds, "frame_steps": steps, "launch_seconds": seconds,
         "frame_steps_per_second": steps / seconds, "shots_per_second": len(batch.group_circ) * shots / seconds,
         "clifford_run_seconds": exact_s, "host_lowering_seconds": lower_s,
         "mean_abs_sampled_minus_exact_noisy": float(np.abs(sampled - exact).mean())}
    sub = sim.compile_clifford_frames(circuits[:subset], observables[:subset], noise)
    t0 = time.perf_counter()
    want = fc.interpret(sub, shots, 0)
    p["interpreter_circuits"] = subset
    p["interpreter_seconds"] = time.perf_counter() - t0
    te = int(sub.term_ptr[-1])
    p["interpreter_term_sums_equal"] = bool((outs["term_sums"].cpu().numpy()[:te] == want["term_sums"]).all())
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clifford_frames_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits and of the shots, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clifford_frames_micro: needs the GPU (there is no host path to time)")
    scale = 16 if args.quick else 1
    shots = SHOTS // scale
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "points": [],
              "method": "device events around ops.clifford_sample (and ops.clifford_run) with the buffers resident and the outputs "
                        "given, 3 warm-ups, median of 20; lowering and the numpy interpreter on the host clock"}

    def save(p):
        result["points"].append(p)
        print(json.dumps(p), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)

    def tfim(nq, count, max_steps):
        grid = [(s, kx, kz) for s in range(1, max_steps + 1) for kx in range(4) for kz in range(4)]
        made = {g: clifford_tfim_circuit(nq, *g) for g in grid}
        return [made[grid[k % len(grid)]] for k in range(count)]

    circuits = tfim(100, 1024 // scale, 6)
    noise = sim.NoiseModel.from_backend(synthetic_backend(100, "ecr"), readout=False)
    save(frames_point("tfim100x100", circuits, [single_z(100, 100, k) for k in range(len(circuits))], noise, 2, shots))

    circuits = tfim(512, 256 // scale, 2)
    noise512 = sim.NoiseModel.from_backend(synthetic_backend(512, "ecr"), readout=False)
    save(frames_point("tfim512x100", circuits, [single_z(512, 100, k) for k in range(len(circuits))], noise512, 1, shots))

    small = [cc.random_clifford_program(5, 40, k, measure=True) for k in range(4096 // scale)]
    save(frames_point("small5", small, [single_z(5, 5, 0)] * len(small), sc.StepNoise(1, force=False), 16, shots))

    qc, qobs, qnoise, _, _ = cc.quality_corpus(100)
    exact = sim.clifford_expectation_values(qc, qobs, qnoise, DEV)[1].cpu().numpy()
    res = sim.sample_clifford_expectation_values(qc, qobs, qnoise, shots=shots, seed=0, device=DEV)
    diff = np.abs(res.term_values.cpu().numpy() - exact)
    save({"point": "quality", "circuits": len(qc), "qubits": 100, "terms": int(len(exact)), "shots": shots,
          "mean_abs_sampled_minus_exact_noisy": float(diff.mean()), "max_abs_sampled_minus_exact_noisy": float(diff.max()),
          "mean_standard_deviation_of_an_estimate": float(np.sqrt(np.maximum(1 - exact * exact, 0) / shots).mean())})


if __name__ == "__main__":
    main()
