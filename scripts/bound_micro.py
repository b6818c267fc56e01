"""Times parameter binding on the device (csrc/sim_bound.hip: mlqem_sim_run_bound_f64, mlqem_sim_shift_combine_f64) on the MI355X
and writes profiles/bound_micro.json.

    python scripts/bound_micro.py [--quick] [--out profiles/bound_micro.json]

Kernel alone (buffers resident, outputs given, device events around the op, 3 warm-ups, median of 20), per shape the bound kernel
in its table form and in its plain form against ``ops.sim_run`` on the host-bound, host-lowered copies of the same circuits:
  vec4      4 096 bindings of ``two_local(4, reps=3)`` (state vectors, the wave variant);
  rho5      4 096 bindings of a five-qubit ry / cx ansatz on the lima fixture's coupling map under its noise model (density
            matrices, the workgroup variant);
  vec11     1 024 bindings of ``two_local(11, entanglement="linear", reps=3)`` (the workgroup variant).
End to end (host clock, the median of 5 after one warm-up): one ``DeviceEstimator.run`` of the 4 096 vec4 bindings against the
only route without templates -- ``bind_parameters`` per row on the host, ``compile_programs``, upload, ``ops.sim_run``, values
back -- with the host lowering time and the bytes uploaded of both.  A full gradient: ``parameter_shift`` for 256 rows of vec4
against the same 256 x 33 runs as host-bound circuits.  A probe of the device library's sin / cos through the kernel: h, p(phi)
on one qubit gives <X> = cos phi and <Y> = sin phi up to a few u of its own rounding.
Nothing here asserts a speed or a ratio.
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

import sim_cases as sc  # noqa: E402
from blackwater import sim  # noqa: E402
from blackwater.data.backends import StaticBackend  # noqa: E402
from blackwater.data.circuit import CircuitOp  # noqa: E402
from blackwater.data.synthetic import two_local  # noqa: E402
from blackwater.native import ops  # noqa: E402
from blackwater.sim.bound import shift_runs  # noqa: E402

DEV = "cuda:0"
LIMA_PAIRS = [(0, 1), (1, 2), (1, 3), (3, 4)]


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


def host_seconds(fn, reps=5):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def f64(*shape):
    return torch.zeros(shape, dtype=torch.float64, device=DEV)


def nbytes(*arrays):
    return int(sum(np.asarray(a).nbytes for a in arrays))


BASE = ("circ", "op_ptr", "ops", "params", "term_ptr", "terms", "coeff")


def bound_call(batch, theta, runs, shift):
    """The resident arguments and outputs of one ops.sim_run_bound call, and the bytes that were uploaded for it."""
    width = int(np.diff(batch.term_ptr).max())
    wave = np.asarray([batch.variant[c] == "wave" for c in runs[:, 0]], dtype=bool)
    ids = np.concatenate([np.flatnonzero(wave), np.flatnonzero(~wave)]).astype(np.int32)
    rtp = np.arange(len(runs) + 1, dtype=np.int64) * width
    host = [getattr(batch, k) for k in BASE] + [theta, runs, shift, ids, rtp]
    t = [up(a) for a in host]
    args = tuple(t[:10]) + (t[10], int(wave.sum()), int((~wave).sum()), t[11], len(runs) * width)
    outs = {"values": f64(len(runs)), "term_values": f64(len(runs) * width), "norm": f64(len(runs))}
    return args, outs, nbytes(*host)


def plain_call(batch):
    t = batch.to(DEV)
    args = tuple(t[k] for k in BASE) + (t["ids"], t["n_wave"], t["n_wg"])
    outs = {"values": f64(len(batch)), "term_values": f64(len(batch.coeff)), "norm": f64(len(batch))}
    return args, outs, nbytes(*[getattr(batch, k) for k in BASE], batch.ids)


def kernel_point(name, template, terms, noise, n_rows):
    theta = np.random.default_rng(1).uniform(-2 * math.pi, 2 * math.pi, size=(n_rows, template.num_parameters))
    batch = sim.compile_templates([template], [terms], noise)
    runs = np.zeros((n_rows, 4), dtype=np.int32)
    runs[:, 1], runs[:, 2] = np.arange(n_rows), -1
    args, outs, _ = bound_call(batch, theta, runs, np.zeros(n_rows))
    table = event_seconds(lambda: ops.sim_run_bound(*args, form=ops.SIM_BOUND_TABLE, **outs))
    values_table = outs["values"].clone()
    plain = event_seconds(lambda: ops.sim_run_bound(*args, form=ops.SIM_BOUND_PLAIN, **outs))
    same = bool(torch.equal(values_table, outs["values"]))
    copies = sim.compile_programs([template.bind_parameters(r) for r in theta], [terms] * n_rows, noise)
    pargs, pouts, _ = plain_call(copies)
    base = event_seconds(lambda: ops.sim_run(*pargs, **pouts))
    diff = float((pouts["values"] - values_table).abs().max())
    point = {"shape": name, "rows": n_rows, "qubits": template.num_qubits, "records": int(batch.op_counts[0]),
             "parameterised_records": int(batch.occ_ptr[1]), "mode": "vector" if noise is None else "density", "variant": batch.variant[0],
             "bound_table_s": table, "bound_plain_s": plain, "sim_run_host_bound_s": base, "table_over_sim_run": table / base,
             "plain_over_sim_run": plain / base, "table_equals_plain_bits": same, "max_abs_bound_minus_host_bound": diff}
    print(json.dumps(point), flush=True)
    return point


def end_to_end(template, terms, n_rows):
    theta = np.random.default_rng(2).uniform(-2 * math.pi, 2 * math.pi, size=(n_rows, template.num_parameters))
    rows = [list(r) for r in theta]
    est = sim.DeviceEstimator(device=DEV)
    new_s = host_seconds(lambda: est.run([template] * n_rows, [terms] * n_rows, rows).result().values)

    def old():
        batch = sim.compile_programs([template.bind_parameters(r) for r in theta], [terms] * n_rows)
        return sim.run_batch(batch, DEV)[0].cpu().numpy()

    old_s = host_seconds(old)
    t0 = time.perf_counter()
    bound = [template.bind_parameters(r) for r in theta]
    bind_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    copies = sim.compile_programs(bound, [terms] * n_rows)
    lower_old_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    batch = sim.compile_templates([template], [terms])
    lower_new_s = time.perf_counter() - t0
    runs = np.zeros((n_rows, 4), dtype=np.int32)
    _, _, new_bytes = bound_call(batch, theta, runs, np.zeros(n_rows))
    _, _, old_bytes = plain_call(copies)
    diff = float(np.abs(est.run([template] * n_rows, [terms] * n_rows, rows).result().values - old()).max())
    point = {"rows": n_rows, "estimator_run_s": new_s, "host_bound_route_s": old_s, "speedup": old_s / new_s,
             "host_lowering_new_s": lower_new_s, "host_bind_old_s": bind_s, "host_lowering_old_s": lower_old_s,
             "bytes_uploaded_new": new_bytes, "bytes_uploaded_old": old_bytes, "max_abs_difference": diff}
    print(json.dumps(point), flush=True)
    return point


def gradient(template, terms, n_rows):
    theta = np.random.default_rng(3).uniform(-2 * math.pi, 2 * math.pi, size=(n_rows, template.num_parameters))
    new_s = host_seconds(lambda: sim.parameter_shift(template, terms, theta, None, DEV)[1].cpu())
    batch = sim.compile_templates([template], [terms])
    runs, shift, _ = shift_runs(batch, np.zeros(n_rows, dtype=np.int64))
    k = int(batch.occ_ptr[1])
    gate_of = {int(batch.gate_record[g]): int(batch.gate_op[g]) for g in range(int(batch.gate_ptr[1]))}

    def old():
        circuits = []
        for (_, row, sop, _), sh in zip(runs.tolist(), shift.tolist()):
            c = template.bind_parameters(theta[row])
            if sop >= 0:
                i = gate_of[sop]
                op = c.ops[i]
                c.ops[i] = CircuitOp(op.name, op.qubits, op.clbits, (op.params[0] + sh,))
            circuits.append(c)
        v = sim.run_batch(sim.compile_programs(circuits, [terms] * len(circuits)), DEV)[0].cpu().numpy()
        d = (v[n_rows:n_rows + k * n_rows] - v[n_rows + k * n_rows:]).reshape(k, n_rows)
        grad = np.zeros((n_rows, template.num_parameters))
        for j in range(k):
            grad[:, int(batch.occ_param[j])] += 0.5 * float(batch.occ_scale[j]) * d[j]
        return grad

    old_s = host_seconds(old, reps=3)
    diff = float(np.abs(sim.parameter_shift(template, terms, theta, None, DEV)[1].cpu().numpy() - old()).max())
    point = {"rows": n_rows, "runs": int(len(runs)), "parameter_shift_s": new_s, "host_bound_route_s": old_s, "speedup": old_s / new_s,
             "max_abs_difference": diff}
    print(json.dumps(point), flush=True)
    return point


def trig_probe(n_rows):
    """<X> = cos phi and <Y> = sin phi of h, p(phi) on one qubit: the device library's cos / sin seen through the kernel, against
    numpy's, in units of u = 2^-53 (the kernel's own products add a few u)."""
    from blackwater.sim import Param, Template

    t = Template(1, 0, [CircuitOp("h", (0,)), CircuitOp("p", (0,), (), (Param(0),))])
    out = {}
    for span in (2 * math.pi, 1e3):
        phi = np.random.default_rng(4).uniform(-span, span, size=(n_rows, 1))
        _, tv = sim.bound_expectation_values(t, [("X", 1.0), ("Y", 1.0)], phi, None, DEV)
        tv = tv.cpu().numpy()
        out[f"span_{span:.4g}"] = {"max_abs_cos_error_u": float(np.abs(tv[:, 0] - np.cos(phi[:, 0])).max() / sc.U),
                                   "max_abs_sin_error_u": float(np.abs(tv[:, 1] - np.sin(phi[:, 0])).max() / sc.U)}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bound_micro.json"))
    a = ap.parse_args()
    scale = 8 if a.quick else 1
    lima = sim.NoiseModel.from_backend(StaticBackend.from_json(os.path.join(sc.GOLDEN, "fake_lima_backend_props.json")))
    vec4, terms4 = two_local(4, reps=3), sc.term_set(4)
    rho5 = two_local(5, entanglement_blocks="cx", entanglement=LIMA_PAIRS, reps=3)
    vec11 = two_local(11, entanglement="linear", reps=3)
    result = {"device": torch.cuda.get_device_name(0),
              "kernel": [kernel_point("vec4", vec4, terms4, None, 4096 // scale),
                         kernel_point("rho5", rho5, sc.term_set(5), lima, 4096 // scale),
                         kernel_point("vec11", vec11, sc.term_set(11), None, 1024 // scale)],
              "end_to_end": end_to_end(vec4, terms4, 4096 // scale),
              "gradient": gradient(vec4, terms4, 256 // scale),
              "trig_probe": trig_probe(4096 // scale)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
