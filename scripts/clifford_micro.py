"""Times the Clifford path (csrc/clifford.hip: mlqem_clifford_run_f64) on the MI355X and writes profiles/clifford_micro.json.

    python scripts/clifford_micro.py [--quick] [--out profiles/clifford_micro.json]

Kernel points: buffers uploaded once, the six outputs given, device events around ``ops.clifford_run``, 3 warm-ups, median of 20.
``record_steps`` is the sum over the units of the records their circuit holds: what the lanes walk.
  tfim100x100    1 024 ``clifford_tfim_circuit`` circuits of 100 qubits (steps 1 .. 6, kx and kz 0 .. 3, a depolarising record after
                 every calibrated gate) x 100 single-Z terms;
  tfim100x1      the same circuits x 1 term: the ``encode_corpus`` case, a few waves on the whole device;
  small5         4 096 five-qubit random Clifford circuits x 5 single-Z terms, and ``ops.sim_run`` in density-matrix mode on the same
                 circuits with the same noise, on the same device;
  tfim512x100    256 circuits of 512 qubits (the LDS instantiation) x 100 single-Z terms;
  encode_corpus  ``encode_corpus(clifford=True)`` end to end on the host clock, with the share spent in ``compile_clifford``.
Nothing here asserts a speed or a ratio.
"""
import argparse
import dataclasses
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
import sim_cases as sc  # noqa: E402
from blackwater import sim  # noqa: E402
from blackwater.data.synthetic import clifford_tfim_circuit, encode_corpus, synthetic_backend  # noqa: E402
from blackwater.native import ops  # noqa: E402
from blackwater.sim import clifford as cl  # noqa: E402

DEV = "cuda:0"


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


def clifford_point(name, batch, lower_s=None):
    t = batch.to(DEV)
    args = (t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"], t["term_ptr"], t["coeff"],
            t["comb_ptr"], t["comb_unit"], t["comb_weight"])
    n_units, n_terms, b = len(batch.units), len(batch.coeff), len(batch)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
    outs = {"unit_ideal": f64(n_units), "unit_noisy": f64(n_units), "ideal_terms": f64(n_terms), "noisy_terms": f64(n_terms),
            "ideal_values": f64(b), "noisy_values": f64(b)}
    seconds = event_seconds(lambda: ops.clifford_run(*args, **outs))
    per_circuit = np.diff(batch.op_ptr)
    steps = int(per_circuit[batch.units[:, 0]].sum())
    p = {"point": name, "circuits": b, "qubits_max": int(batch.n_qubits.max()), "records": int(batch.op_ptr[-1]), "units": n_units,
         "n_reg": batch.n_reg, "n_lds": batch.n_lds, "record_steps": steps, "launch_seconds": seconds,
         "units_per_second": n_units / seconds, "record_steps_per_second": steps / seconds, "circuits_per_second": b / seconds}
    if lower_s is not None:
        p["host_lowering_seconds"] = lower_s
    return p, outs


def one_term_per_circuit(batch):
    """The same circuits with the first term of each alone (every unit of these batches is its own term)."""
    first = batch.comb_unit[batch.comb_ptr[batch.term_ptr[:-1]]]
    b = len(batch)
    in_reg = first < batch.n_reg
    order = np.concatenate([first[in_reg], first[~in_reg]])
    where = np.concatenate([np.flatnonzero(in_reg), np.flatnonzero(~in_reg)])
    comb_unit = np.empty(b, dtype=np.int32)
    comb_unit[where] = np.arange(b, dtype=np.int32)
    return dataclasses.replace(batch, units=batch.units[order], n_reg=int(in_reg.sum()), n_lds=int((~in_reg).sum()),
                               term_ptr=np.arange(b + 1, dtype=np.int64), coeff=np.ones(b), comb_ptr=np.arange(b + 1, dtype=np.int64),
                               comb_unit=comb_unit, comb_weight=np.ones((b, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clifford_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clifford_micro: needs the GPU (there is no host path to time)")
    scale = 16 if args.quick else 1
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "points": [],
              "method": "device events around ops.clifford_run (and ops.sim_run) with the buffers resident and the outputs given, 3 "
                        "warm-ups, median of 20; lowering and encode_corpus on the host clock"}

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

    # 100 qubits
    circuits = tfim(100, 1024 // scale, 6)
    noise = sim.NoiseModel.from_backend(synthetic_backend(100, "ecr"), readout=False)
    t0 = time.perf_counter()
    batch = sim.compile_clifford(circuits, [single_z(100, 100, k) for k in range(len(circuits))], noise)
    lower_s = time.perf_counter() - t0
    p, outs = clifford_point("tfim100x100", batch, lower_s)
    p["nonzero_ideal_terms"] = int(torch.count_nonzero(outs["ideal_terms"]).item())
    save(p)
    save(clifford_point("tfim100x1", one_term_per_circuit(batch))[0])
    del batch

    # 5 qubits, against the density-matrix simulator
    small = [cc.random_clifford_program(5, 40, k, measure=True) for k in range(4096 // scale)]
    obs = [single_z(5, 5, 0)] * len(small)
    step_noise = sc.StepNoise(1, force=False)
    t0 = time.perf_counter()
    batch = sim.compile_clifford(small, obs, step_noise)
    p, outs = clifford_point("small5", batch, time.perf_counter() - t0)
    dense = sim.compile_programs(small, obs, step_noise)
    t = dense.to(DEV)
    sargs = (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], t["ids"], t["n_wave"], t["n_wg"])
    souts = {"values": torch.zeros(len(dense), dtype=torch.float64, device=DEV),
             "term_values": torch.zeros(int(dense.term_ptr[-1]), dtype=torch.float64, device=DEV),
             "norm": torch.zeros(len(dense), dtype=torch.float64, device=DEV)}
    p["sim_run_density_seconds"] = event_seconds(lambda: ops.sim_run(*sargs, **souts))
    p["sim_run_over_clifford_run"] = p["sim_run_density_seconds"] / p["launch_seconds"]
    p["max_abs_difference_of_values"] = float((souts["values"] - outs["noisy_values"]).abs().max().item())
    save(p)
    del batch, dense

    # 512 qubits
    circuits = tfim(512, 256 // scale, 2)
    noise512 = sim.NoiseModel.from_backend(synthetic_backend(512, "ecr"), readout=False)
    t0 = time.perf_counter()
    batch = sim.compile_clifford(circuits, [single_z(512, 100, k) for k in range(len(circuits))], noise512)
    save(clifford_point("tfim512x100", batch, time.perf_counter() - t0)[0])
    del batch

    # encode_corpus(clifford=True) end to end
    corpus = [clifford_tfim_circuit(100, 1 + k % 3, k % 4, (k // 4) % 4, two_q="cx") for k in range(256 // scale)]
    noise_cx = sim.NoiseModel.from_backend(synthetic_backend(100, "cx"))
    spent = {"compile_clifford": 0.0}
    real = cl.compile_clifford

    def timed(*a, **k):
        t1 = time.perf_counter()
        out = real(*a, **k)
        spent["compile_clifford"] += time.perf_counter() - t1
        return out

    cl.compile_clifford = timed
    try:
        encode_corpus(corpus[:4], 100, two_q="cx", simulate=noise_cx, device=DEV, clifford=True)   # warm-up
        spent["compile_clifford"] = 0.0
        t0 = time.perf_counter()
        plain_s = 0.0
        encode_corpus(corpus, 100, two_q="cx", simulate=noise_cx, device=DEV, clifford=True)
        total = time.perf_counter() - t0
        t0 = time.perf_counter()
        encode_corpus(corpus, 100, two_q="cx")
        plain_s = time.perf_counter() - t0
    finally:
        cl.compile_clifford = real
    save({"point": "encode_corpus", "circuits": len(corpus), "qubits": 100, "seconds": total, "circuits_per_second": len(corpus) / total,
          "compile_clifford_seconds": spent["compile_clifford"], "compile_clifford_share": spent["compile_clifford"] / total,
          "without_simulation_seconds": plain_s})


if __name__ == "__main__":
    main()
