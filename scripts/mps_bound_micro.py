"""Times parameter binding on the matrix-product-state path (csrc/mps_bind.hip: mlqem_mps_bind_f64, then the kernels of csrc/mps.hip)
on the MI355X and writes profiles/mps_bound_micro.json.

    python scripts/mps_bound_micro.py [--quick] [--out profiles/mps_bound_micro.json]

Per shape: 1 024 rows of ``tfim_circuit_template(100, s)`` for s = 1, 3, 5 Trotter steps, 100 single-Z terms, bond 32, ideal; the
rows are (2 h dt, -2 J dt) with J ~ U(0, 0.66 pi) as in scripts/mps_micro.py.  Host clock around a device synchronisation, one
warm-up, the median of 3 unless said otherwise:
  bound_total_ms        ``bound_mps_expectation_values``: the template's lowering, the upload, bind + run + finish;
  template_lowering_ms  ``compile_mps_templates`` alone (once);
  bound_launch_ms       ``MpsBoundRun.launch()`` on prepared tables: the bind, run, terms and finish kernels alone;
  bind_kernel_ms        ``mlqem_mps_bind_f64`` alone (device events, the median of 5), with the bytes it writes;
  copies_lowering_ms    ``compile_mps`` of the 1 024 bound copies, the host path of ``mps_expectation_values`` (ONCE: it takes
                        seconds to tens of seconds, and a median of 3 of it would spend the run on the host);
  run_mps_ms            ``run_mps`` on that lowering (upload, run, terms, finish): the device part of the path before templates;
  copies_total_ms       copies_lowering_ms + run_mps_ms: ``mps_expectation_values`` on the bound copies.
Then one gradient: a 100-qubit ``two_local(100, ry, cx, "linear", reps=1)`` whose 200 rotations share 16 parameters (index mod
16), 64 rows: ``parameter_shift(method="mps")`` binds and runs 64 x (1 + 2 x 200) copies.
``--quick``: 64 rows and 4 gradient rows.  Nothing here asserts a speed or a ratio.
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
from blackwater.data.circuit import CircuitOp  # noqa: E402
from blackwater.data.synthetic import tfim_circuit_template, two_local  # noqa: E402
from blackwater.native import ops  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(times), out


def bind_alone(plan, reps=5):
    """The bind kernel of the plan's first chunk, by device events."""
    t = plan.tpl
    (cr, _), (n_ops, n_pool, _, max_rec, _), (op_at, _) = plan.chunks[0], plan.sizes[0], plan.where[0]
    n = len(cr)

    def launch():
        ops.mps_bind(t["op_ptr"], t["ops"], t["params"], t["pool_ptr"], t["fac_ptr"], t["fac"], t["fac_val"], t["fpool"], t["occ_ptr"], t["occ"],
                     plan.theta, plan.runs[cr.start:cr.stop], plan.shift[cr.start:cr.stop], max_rec, plan.rel_op[op_at:op_at + n + 1],
                     plan.rel_pool[op_at:op_at + n + 1], plan.out_ops[:max(n_ops, 1)], plan.out_pool[:n_pool + 32])

    launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        launch()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times), 8 * n_pool + 16 * n_ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mps_bound_micro.json"))
    args = ap.parse_args()
    nq, count = 100, 64 if args.quick else 1024
    rng = np.random.default_rng(42)
    couplings = rng.uniform(0.0, 0.66 * math.pi, size=count)
    theta = np.stack([np.full(count, 2 * 0.66 * math.pi * 0.5), -2.0 * couplings * 0.5], axis=1)
    terms = mc.single_z(nq)
    rows = []
    for steps in (1, 3, 5):
        template = tfim_circuit_template(nq, steps, "cx")
        t0 = time.perf_counter()
        batch = sim.compile_mps_templates([template], [terms])
        template_lowering_ms = 1e3 * (time.perf_counter() - t0)
        total_ms, (values, _, res) = timed(lambda: sim.bound_mps_expectation_values(template, terms, theta, device=DEV, return_result=True))
        plan = sim.MpsBoundRun(batch, theta, device=DEV)
        launch_ms, _ = timed(plan.launch)
        bind_ms, bind_bytes = bind_alone(plan)
        copies = [template.bind_parameters(r) for r in theta]
        t0 = time.perf_counter()
        lowered = sim.compile_mps(copies, [terms] * count)
        copies_lowering_ms = 1e3 * (time.perf_counter() - t0)
        run_ms, want = timed(lambda: sim.run_mps(lowered, device=DEV))
        row = {"steps": steps, "rows": count, "qubits": nq, "max_bond": 32, "records_per_copy": int(batch.ops.shape[0]),
               "factors_per_copy": int(batch.fac_ptr[-1]), "chunks": len(plan.chunks), "bound_total_ms": total_ms,
               "template_lowering_ms": template_lowering_ms, "bound_launch_ms": launch_ms, "bind_kernel_ms": bind_ms,
               "bind_bytes_written": bind_bytes, "bind_gb_per_s": bind_bytes / (1e6 * bind_ms), "copies_lowering_ms": copies_lowering_ms,
               "run_mps_ms": run_ms, "copies_total_ms": copies_lowering_ms + run_ms,
               "largest_value_difference": float((values - want.values).abs().max()), "worst_error_bound": float(res.error_bound.max()),
               "largest_bond": int(res.bond.max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    base = two_local(nq, rotation_blocks=("ry",), entanglement_blocks="cx", entanglement="linear", reps=1)
    shared = sim.Template(nq, 0, [CircuitOp(op.name, op.qubits, op.clbits, (sim.Param(op.params[0].index % 16),)) if op.params else op
                                  for op in base.ops], [], 16)
    n_rows = 4 if args.quick else 64
    points = rng.uniform(-math.pi, math.pi, size=(n_rows, 16))
    grad_ms, (values, grads) = timed(lambda: sim.parameter_shift(shared, terms, points, None, DEV, method="mps"))
    gradient = {"qubits": nq, "parameters": 16, "occurrences": 200, "rows": n_rows, "runs": n_rows * 401, "parameter_shift_ms": grad_ms,
                "largest_gradient": float(grads.abs().max())}
    print(json.dumps(gradient), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "rows": rows, "gradient": gradient}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
