"""Times zero-noise extrapolation on the Clifford path (csrc/clifford.hip: mlqem_clifford_run_folded_f64, and the combine of
csrc/sim.hip) on the MI355X and writes profiles/clifford_zne_micro.json.

    python scripts/clifford_zne_micro.py [--quick] [--out profiles/clifford_zne_micro.json]

Per shape two routes to the same mitigated values:
  fused     compile_clifford once, build_clifford_schedules, one upload, ``ops.clifford_run_folded`` + ``ops.zne_combine`` (a straight
            line; ``ops.zne_combine_exp`` is timed beside it);
  unfused   what the parent commit allows: per noise factor ``fold_circuit`` on the IR, ``compile_clifford`` of the folded circuits,
            an upload and ``ops.clifford_run``; the weighted sum in numpy.
Kernel figures: buffers resident, outputs given, device events around the op, 3 warm-ups, median of 20.  Host stages (lowering,
schedules or folding, upload, launches, end to end) on the host clock, once.  ``entry_steps`` is the sum over (factor, unit) of the
entries the unit's run holds, what the lanes of the folded walk go through; ``record_steps`` the same for the unfolded walk of
factor 1.
  tfim100x100    1 024 ``clifford_tfim_circuit`` circuits of 100 qubits x 100 single-Z terms, factors (1, 3), two-qubit local folding;
  tfim100x1      the same circuits x 1 term;
  tfim512x100    256 circuits of 512 qubits (the LDS instantiation) x 100 terms, factors (1, 3);
  small5         4 096 five-qubit random Clifford circuits x 5 terms at factors (1, 3, 5), every gate folded, and
                 ``ops.sim_run_folded`` in density-matrix mode on the same circuits with the same noise.
Nothing here asserts a speed or a ratio.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import clifford_cases as cc  # noqa: E402
import sim_cases as sc  # noqa: E402
from blackwater import sim, zne  # noqa: E402
from blackwater.data.synthetic import clifford_tfim_circuit, synthetic_backend  # noqa: E402
from blackwater.native import ops  # noqa: E402
from clifford_micro import event_seconds, one_term_per_circuit, single_z  # noqa: E402

DEV = "cuda:0"


def clifford_args(t):
    return (t["n_qubits"], t["op_ptr"], t["ops"], t["pool"], t["units"], t["n_reg"], t["n_lds"], t["masks"], t["term_ptr"], t["coeff"],
            t["comb_ptr"], t["comb_unit"], t["comb_weight"])


def f64(*shape):
    return torch.zeros(shape, dtype=torch.float64, device=DEV)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def fused(batch, strategy, lower_s):
    """The fused route on an already lowered batch; returns the point's figures and the mitigated values."""
    factors, weights = strategy.noise_factors, strategy.weights()
    n_f, b, n_units, n_terms = len(factors), len(batch), len(batch.units), len(batch.coeff)
    sch, sched_s = clock(lambda: zne.build_clifford_schedules(batch, factors, strategy.noise_amplifier))
    (t, s, w), upload_s = clock(lambda: (batch.to(DEV), sch.to(DEV), torch.from_numpy(weights).to(DEV)))
    outs = {"unit_ideal": f64(n_f, n_units), "unit_noisy": f64(n_f, n_units), "ideal_terms": f64(n_f, n_terms),
            "noisy_terms": f64(n_f, n_terms), "ideal_values": f64(n_f, b), "noisy_values": f64(n_f, b)}
    mt, mv, fb = f64(n_terms), f64(b), torch.zeros(n_terms, dtype=torch.int32, device=DEV)
    args = clifford_args(t) + (s["sched_ptr"], s["sched"], n_f)

    def launches():
        ops.clifford_run_folded(*args, **outs)
        ops.zne_combine(outs["noisy_terms"], w, t["term_ptr"], t["coeff"], mitigated_terms=mt, mitigated_values=mv)

    _, first_s = clock(launches)
    run_s = event_seconds(lambda: ops.clifford_run_folded(*args, **outs))
    lin_s = event_seconds(lambda: ops.zne_combine(outs["noisy_terms"], w, t["term_ptr"], t["coeff"], mitigated_terms=mt, mitigated_values=mv))
    exp_s = event_seconds(lambda: ops.zne_combine_exp(outs["noisy_terms"], w, t["term_ptr"], t["coeff"], mitigated_terms=mt,
                                                      mitigated_values=mv, fallback=fb))
    launches()
    torch.cuda.synchronize()
    per_run = np.diff(sch.sched_ptr).reshape(n_f, b)
    steps = int(per_run[:, batch.units[:, 0]].sum())
    equal = all(bool(torch.equal(outs[k][0], outs[k][f])) for k in ("unit_ideal", "ideal_terms", "ideal_values") for f in range(1, n_f))
    point = {"circuits": b, "qubits_max": int(batch.n_qubits.max()), "records": int(batch.op_ptr[-1]), "units": n_units,
             "n_reg": batch.n_reg, "n_lds": batch.n_lds, "factors": list(factors), "amplifier": repr(strategy.noise_amplifier),
             "schedule_entries": int(sch.sched_ptr[-1]), "entry_steps": steps, "ideal_equal_across_factors": equal,
             "fused": {"lowering_seconds": lower_s, "schedules_seconds": sched_s, "upload_seconds": upload_s,
                       "first_launches_seconds": first_s, "end_to_end_seconds": lower_s + sched_s + upload_s + first_s,
                       "run_folded_seconds": run_s, "combine_linear_seconds": lin_s, "combine_exponential_seconds": exp_s,
                       "entry_steps_per_second": steps / run_s, "nanoseconds_per_entry_step": run_s / steps * 1e9}}
    return point, mv.cpu().numpy(), t, outs


def unfolded_point(batch, t):
    """``ops.clifford_run`` on the same resident batch: the time per record step the folded walk is compared with."""
    n_units, n_terms, b = len(batch.units), len(batch.coeff), len(batch)
    outs = {"unit_ideal": f64(n_units), "unit_noisy": f64(n_units), "ideal_terms": f64(n_terms), "noisy_terms": f64(n_terms),
            "ideal_values": f64(b), "noisy_values": f64(b)}
    seconds = event_seconds(lambda: ops.clifford_run(*clifford_args(t), **outs))
    steps = int(np.diff(batch.op_ptr)[batch.units[:, 0]].sum())
    return {"run_seconds": seconds, "record_steps": steps, "nanoseconds_per_record_step": seconds / steps * 1e9}


def unfused(circuits, observables, noise, strategy, pick=None):
    """The parent commit's route: fold the IR, lower, upload and run per factor; numpy combine.  ``noise`` must be by name (a
    ``NoiseModel``) so that a folded gate finds its calibration entry; ``pick`` narrows a lowered batch (the one-term shape)."""
    factors, weights = strategy.noise_factors, strategy.weights()
    stage = {"folding_seconds": 0.0, "lowering_seconds": 0.0, "upload_seconds": 0.0, "launches_seconds": 0.0, "run_seconds": []}
    values = []
    for lam in factors:
        folded, s = clock(lambda: [zne.fold_circuit(c, lam, strategy.noise_amplifier) for c in circuits])
        stage["folding_seconds"] += s
        batch, s = clock(lambda: sim.compile_clifford(folded, observables, noise))
        stage["lowering_seconds"] += s
        if pick is not None:
            batch = pick(batch)
        t, s = clock(lambda: batch.to(DEV))
        stage["upload_seconds"] += s
        out, s = clock(lambda: ops.clifford_run(*clifford_args(t)))
        stage["launches_seconds"] += s
        stage["run_seconds"].append(event_seconds(lambda: ops.clifford_run(*clifford_args(t))))
        values.append(out[1].cpu().numpy())
    t0 = time.perf_counter()
    mitigated = strategy.extrapolator.extrapolate(factors, np.asarray(values))
    stage["numpy_combine_seconds"] = time.perf_counter() - t0
    stage["end_to_end_seconds"] = sum(stage[k] for k in ("folding_seconds", "lowering_seconds", "upload_seconds", "launches_seconds",
                                                         "numpy_combine_seconds"))
    stage["run_seconds_total"] = float(sum(stage["run_seconds"]))
    return stage, mitigated


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clifford_zne_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a sixteenth of the circuits, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("clifford_zne_micro: needs the GPU (there is no host path to time)")
    scale = 16 if args.quick else 1
    result = {"device": torch.cuda.get_device_name(0), "quick": args.quick, "points": [],
              "method": "device events around the op with the buffers resident and the outputs given, 3 warm-ups, median of 20; host "
                        "stages once on the host clock, the device idle before and after each"}

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

    def shape(name, circuits, observables, noise, strategy, one_term=False):
        batch, lower_s = clock(lambda: sim.compile_clifford(circuits, observables, noise))
        if one_term:
            batch = one_term_per_circuit(batch)
        point, mitigated, t, _ = fused(batch, strategy, lower_s)
        point["point"] = name
        point["unfolded_walk"] = unfolded_point(batch, t)
        point["unfused"], want = unfused(circuits, observables, noise, strategy, one_term_per_circuit if one_term else None)
        point["max_abs_difference_of_mitigated_values"] = float(np.abs(mitigated - want).max())
        point["end_to_end_unfused_over_fused"] = point["unfused"]["end_to_end_seconds"] / point["fused"]["end_to_end_seconds"]
        return point, batch

    default = zne.ZNEStrategy()   # factors (1, 3), two-qubit local folding, a straight line
    circuits = tfim(100, 1024 // scale, 6)
    obs = [single_z(100, 100, k) for k in range(len(circuits))]
    noise = sim.NoiseModel.from_backend(synthetic_backend(100, "ecr"), readout=False)
    save(shape("tfim100x100", circuits, obs, noise, default)[0])
    save(shape("tfim100x1", circuits, obs, noise, default, one_term=True)[0])

    circuits = tfim(512, 256 // scale, 2)
    obs = [single_z(512, 100, k) for k in range(len(circuits))]
    noise512 = sim.NoiseModel.from_backend(synthetic_backend(512, "ecr"), readout=False)
    save(shape("tfim512x100", circuits, obs, noise512, default)[0])

    # five qubits at (1, 3, 5), every gate folded, against the density-matrix simulator's folded run
    small = [cc.random_clifford_program(5, 40, k, measure=True) for k in range(4096 // scale)]
    obs = [single_z(5, 5, 0)] * len(small)
    # by name AND the same for every name on a qubit, so that the unfused route's inverse gates (sxdg for sx, u3 for u2) carry the
    # depolarising parameter of the gate they invert, as the fused route's schedules do
    by_name = sim.NoiseModel({(g, (q,)): 0.01 + 0.002 * q for g in sc.ONE_QUBIT for q in range(5)} |
                             {(g, (a, b)): 0.03 + 0.004 * (a + b) for g in sc.TWO_QUBIT for a in range(5) for b in range(5) if a != b})
    strategy = zne.ZNEStrategy((1, 3, 5), zne.LocalFoldingAmplifier(), zne.LinearExtrapolator())
    point, batch = shape("small5", small, obs, by_name, strategy)
    dense = sim.compile_programs(small, obs, by_name)
    sch = zne.build_schedules(dense, small, strategy.noise_factors, strategy.noise_amplifier)
    t, s = dense.to(DEV), sch.to(DEV)
    souts = {"values": f64(3, len(dense)), "term_values": f64(3, int(dense.term_ptr[-1])), "norm": f64(3, len(dense))}
    sargs = (t["circ"], t["op_ptr"], t["ops"], t["params"], t["term_ptr"], t["terms"], t["coeff"], s["sched_ptr"], s["sched"], s["ids"],
             sch.n_wave, sch.n_wg, 3)
    point["sim_run_folded_density_seconds"] = event_seconds(lambda: ops.sim_run_folded(*sargs, **souts))
    point["sim_run_folded_over_clifford_run_folded"] = point["sim_run_folded_density_seconds"] / point["fused"]["run_folded_seconds"]
    got = sim.run_clifford_folded(batch, zne.build_clifford_schedules(batch, strategy.noise_factors, strategy.noise_amplifier), DEV)
    point["max_abs_difference_of_values_to_density"] = float((souts["values"] - got[1]).abs().max().item())
    save(point)


if __name__ == "__main__":
    main()
