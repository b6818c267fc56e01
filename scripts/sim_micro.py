"""Times the batched simulator (csrc/sim.hip, blackwater.sim) and, beside it, the numpy oracle of tests/sim_cases.py on the same
box in the same call.  No claim against Aer: it is not installed anywhere this project runs.

    python scripts/sim_micro.py [--out profiles/sim_micro.json] [--quick]

  lima_vector    4 096 lima-regime circuits (the 900 golden circuits tiled; 5 qubits, 31-101 ops), per-classical-bit <Z>, state-vector
                 mode: the wave-per-circuit kernel;
  lima_density   the same circuits under ``NoiseModel.from_backend(lima)`` with readout: 5-qubit density matrices, the
                 workgroup-per-circuit kernel;
  random11       1 024 random 11-qubit circuits of 200 gates over the full gate list, 12 Pauli terms: the cap of the vector mode;
  generator      one ``exp_value_generator`` run of 4 096 entries end to end on the host clock (drawing, lowering, both launches, graph
                 encoding), with the seconds spent in ``compile_programs`` and in the launches (device wait included) beside it.
Kernel points: buffers uploaded once, outputs given, device events around ``ops.sim_run``, 3 warm-ups, median of 20.  ``lds_bytes`` is
what the passes of all ops move through LDS (16 bytes read and 16 written per amplitude and pass; the two-qubit depolarising op reads
a quarter more), and ``lds_tb_per_s`` that over the launch time, to set against the LDS rates of an MI355X (about 150 TB/s for 16-byte
reads and 38-51 TB/s for stores with every CU streaming).  The oracle is timed on the host clock, median of 3, on the first
``oracle_circuits`` circuits of the point and scaled to the point's size (said so in the result).
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
from blackwater.data.circuit import Circuit  # noqa: E402
from blackwater.native import ops  # noqa: E402
from blackwater.sim import program as P  # noqa: E402

DEV = "cuda:0"
PASSES = {P.OP_U1: (1, 2), P.OP_DIAG1: (1, 1), P.OP_CX: (1, 1), P.OP_CZ: (1, 1), P.OP_SWAP: (1, 1), P.OP_U2: (1, 2),
          P.OP_DEPOL1: (0, 1), P.OP_DEPOL2: (0, 1.125), P.OP_READOUT: (0, 0)}   # passes over the state: (vector, density)


def lds_bytes(batch):
    amps = np.where(batch.circ[:, 1] != 0, 4 ** batch.circ[:, 0].astype(np.int64), 2 ** batch.circ[:, 0].astype(np.int64))
    per_op_amps = np.repeat(amps, np.diff(batch.op_ptr))
    per_op_mode = np.repeat(batch.circ[:, 1], np.diff(batch.op_ptr))
    passes = np.asarray([PASSES[int(k)][int(m)] for k, m in zip(batch.ops[:, 0], per_op_mode)], dtype=np.float64)
    return float((passes * per_op_amps * 32).sum())


def kernel_point(name, circuits, observables, noise, oracle_circuits):
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
    moved = lds_bytes(batch)
    n_ops = int(batch.op_ptr[-1])
    p = {"point": name, "circuits": len(batch), "records": n_ops, "terms": int(batch.term_ptr[-1]), "n_wave": batch.n_wave,
         "n_wg": batch.n_wg, "launch_seconds": seconds, "circuits_per_second": len(batch) / seconds, "host_lowering_seconds": lower_s,
         "lds_bytes": moved, "lds_bytes_per_record": moved / max(n_ops, 1), "lds_tb_per_s": moved / seconds * 1e-12}
    sub = [Circuit.from_any(c) for c in circuits[:oracle_circuits]]
    obs = [o.to_list() if hasattr(o, "to_list") else o for o in observables[:oracle_circuits]]

    def oracle():
        t1 = time.perf_counter()
        for c, o in zip(sub, obs):
            sc.simulate(c, o, noise)
        return time.perf_counter() - t1

    o_s = statistics.median([oracle(), oracle(), oracle()]) * len(batch) / len(sub)
    p.update({"oracle_seconds": o_s, "oracle_circuits": len(sub), "oracle_note": f"timed on {len(sub)} circuits, scaled to {len(batch)}",
              "speedup_vs_oracle": o_s / seconds})
    print(json.dumps(p), flush=True)
    return p


def generator_point(entries):
    from blackwater.data.generators.exp_val import exp_value_generator
    from blackwater.data.synthetic import synthetic_backend
    import blackwater.sim.run as simrun

    spent = {"compile_programs": 0.0, "launches": 0.0}
    real_compile, real_run = simrun.compile_programs, simrun.run_batch

    def timed_compile(*a, **k):
        t0 = time.perf_counter()
        out = real_compile(*a, **k)
        spent["compile_programs"] += time.perf_counter() - t0
        return out

    def timed_run(*a, **k):
        t0 = time.perf_counter()
        out = real_run(*a, **k)
        torch.cuda.synchronize()
        spent["launches"] += time.perf_counter() - t0
        return out

    simrun.compile_programs, simrun.run_batch = timed_compile, timed_run
    try:
        backend = synthetic_backend(4, "cx")
        list(exp_value_generator(backend, 4, 6, 3, max_entries=256, device=DEV))   # warm-up
        spent.update(compile_programs=0.0, launches=0.0)
        t0 = time.perf_counter()
        n = sum(1 for _ in exp_value_generator(backend, 4, 6, 3, max_entries=entries, device=DEV))
        total = time.perf_counter() - t0
    finally:
        simrun.compile_programs, simrun.run_batch = real_compile, real_run
    p = {"point": "generator", "entries": n, "seconds": total, "entries_per_second": n / total,
         "compile_programs_seconds": spent["compile_programs"], "launch_and_copy_seconds": spent["launches"],
         "other_host_seconds": total - spent["compile_programs"] - spent["launches"]}
    print(json.dumps(p), flush=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sim_micro: needs the GPU (there is no host path to time)")
    scale = 16 if args.quick else 1
    texts, _, _ = sc.golden_circuits()
    tiled = [texts[k % len(texts)] for k in range(4096 // scale)]
    zs = [sim.measured_z(t) for t in tiled]
    lima = StaticBackend.from_json(os.path.join(sc.GOLDEN, "fake_lima_backend_props.json"))
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "points": [],
              "method": "device events around ops.sim_run with the buffers resident and the outputs given, 3 warm-ups, median of 20; "
                        "the numpy oracle on the host clock, median of 3, on a subset and scaled; the generator on the host clock"}

    def save(p):
        result["points"].append(p)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)

    save(kernel_point("lima_vector", tiled, zs, None, 256 // scale))
    save(kernel_point("lima_density", tiled, zs, sim.NoiseModel.from_backend(lima), 64 // scale))
    rand = [sc.random_program(11, 200, seed=k) for k in range(1024 // scale)]
    save(kernel_point("random11", rand, [sc.term_set(11, seed=k) for k in range(len(rand))], None, 32 // scale))
    save(generator_point(4096 // scale))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
