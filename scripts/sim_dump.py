"""Runs every case of the grids the simulator's GPU tests iterate and writes every output tensor to one .npz, so that two builds of
the library can be compared bit for bit (MLQEM_LIB selects the build; compare the files array for array).

    python scripts/sim_dump.py --out a.npz
    MLQEM_LIB=/path/to/other/libmlqem_hip.so python scripts/sim_dump.py --out b.npz
    python scripts/sim_dump.py --compare a.npz b.npz

The grids: sim_cases (vector, density, depolarising, readout), relax_cases.grid, zne_cases (folded runs, one of them measured),
shots_cases.batches at every shot count (measured runs + sampled counts), traj_cases.grid with the per-trajectory values,
bound_cases.grid in both forms with every shifted run, clifford_frames_cases' grid, and the matrix-product-state drivers: mps_cases.grid
and mps_relax_cases.grid through run_mps, mps_shots_cases.grid through run_mps_shots with the bits, mps_zne_cases.grid through
run_mps_folded, mps_bound_cases.grid through run_mps_bound (plain and shifted runs), mps_twirl_cases.grid through run_mps and
run_mps_folded -- each once at the default buffer_bytes and once at the workspace of ONE unit of the case's widest circuit, which
splits every circuit's trajectories over launches.  The estimator section runs two successive jobs of DeviceEstimator under every
method, and of zne(DeviceEstimator) where it folds, and keeps the values, every metadata field, the job ids and the key lists.

--package-root DIR imports blackwater from another tree (a worktree of another commit, built in place) while the case modules
stay this tree's: the MPS and estimator sections call only public names of blackwater.sim.
"""
import argparse
import dataclasses
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE_ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[:-1] else ROOT
sys.path[:0] = [PACKAGE_ROOT, os.path.join(PACKAGE_ROOT, "ml-qem_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

DEV = "cuda:0"


def compare(a, b):
    x, y = np.load(a), np.load(b)
    differ = [k for k in x.files if k not in y.files or x[k].dtype != y[k].dtype or x[k].shape != y[k].shape
              or x[k].tobytes() != y[k].tobytes()]
    differ += [k for k in y.files if k not in x.files]
    print(f"{len(x.files)} arrays in {a}, {len(y.files)} in {b}, {len(differ)} differ")
    for k in differ[:20]:
        print("  differs:", k)
    return 1 if differ else 0


def dump(out):
    import torch

    import bound_cases as bc
    import clifford_frames_cases as fc
    import mps_bound_cases as mbc
    import mps_cases as mc
    import mps_relax_cases as mr
    import mps_shots_cases as ms
    import mps_twirl_cases as mt
    import mps_zne_cases as mz
    import relax_cases as rc
    import shots_cases as shc
    import sim_cases as sc
    import traj_cases as tc
    import zne_cases as zc
    from blackwater import sim
    from blackwater.native import ops
    from blackwater.sim import zne
    from blackwater.sim.bound import run_bound, shift_runs
    from blackwater.sim.mps import mps_shift_runs

    arrays = {}

    def put(name, obj):
        if torch.is_tensor(obj):
            arrays[name] = obj.cpu().numpy()
        elif dataclasses.is_dataclass(obj):
            for f in dataclasses.fields(obj):
                if f.name != "batch":
                    put(f"{name}/{f.name}", getattr(obj, f.name))
        elif isinstance(obj, dict):
            for k, v in obj.items():
                put(f"{name}/{k}", v)
        elif isinstance(obj, (tuple, list)):
            for k, v in enumerate(obj):
                put(f"{name}/{k}", v)

    def section(name):
        print(f"{name}: {len(arrays)} arrays so far", flush=True)

    def exact(name, circuits, observables, noise):
        put(name, sim.run_batch(sim.compile_programs(circuits, observables, noise), DEV))

    for n in (1, 2, 3, 8, 9, 11):
        c = sc.random_program(n, 40, seed=0)
        exact(f"sim/vector-n{n}", [c, c], [sc.term_set(n), sc.long_observable(n)], None)
    for n in (1, 2, 4, 5):
        obs = [sc.term_set(n), sc.long_observable(n)]
        c = sc.random_program(n, 40, seed=1)
        exact(f"sim/density-n{n}", [c, c], obs, sc.NoNoise())
        c = sc.random_program(n, 40, seed=2)
        exact(f"sim/depol-n{n}", [c, c], obs, sc.StepNoise(11))
        c = sc.random_program(n, 40, seed=3, measure=True)
        noise = sc.StepNoise(12, readout={q: (0.01 + 0.02 * q, 0.06 - 0.01 * q) for q in range(n)})
        exact(f"sim/readout-n{n}", [c, c], [sc.term_set(n, alphabet="IZ"), sc.long_observable(n, alphabet="IZ")], noise)
    section("relax")
    for name, c, terms, noise in rc.grid():
        exact(f"relax/{name}", [c], [list(terms)], noise)

    def folded(name, c, terms, noise, desc, factors, **kw):
        strategy = zne.ZNEStrategy(noise_factors=factors, noise_amplifier=zc.make_amplifier(desc), extrapolator=zne.PolynomialExtrapolator(1))
        put(name, zne.zne_run([c], [terms], noise, strategy, DEV, **kw))

    section("zne")
    for name, n, desc, factors in zc.density_cases():
        folded(f"zne/{name}", *zc.density_program(n), desc, factors)
    for n in zc.VECTOR_N:
        folded(f"zne/vector-n{n}", *zc.vector_program(n), None, zc.GLOBAL, (1, 3, 5))
    for n in zc.READOUT_N:   # the two folds tests/test_gpu_zne.py runs on the readout programs
        folded(f"zne/readout-n{n}-local", *zc.readout_program(n), zc.LOCAL_ALL, (1, 3))
        folded(f"zne/readout-n{n}-global-partial", *zc.readout_program(n), zc.GLOBAL, zc.PARTIAL)
    for n in (2, 5):
        folded(f"zne/measured-n{n}", *zc.density_program(n), zc.LOCAL_ALL, (1, 3), shots=65, seed=7)
    section("shots")
    for name, (circuits, observables, noise, _) in shc.batches().items():
        for shots in shc.SHOTS:
            put(f"shots/{name}-{shots}", sim.sample_batch(sim.compile_programs(circuits, observables, noise, shots=shots), shc.seed_for(shots), None, DEV))
    section("traj")
    for case in tc.grid():
        put(f"traj/{case['id']}", sim.run_trajectories(tc.lower(case), case["seed"], None, DEV, keep_trajectories=True))
    section("bound")
    for name, template, terms, noise, n_rows, span in bc.grid():
        batch = sim.compile_templates([template], [terms], noise)
        theta = bc.thetas(n_rows, template.num_parameters, span=span)
        runs, shift, _ = shift_runs(batch, np.zeros(n_rows, dtype=np.int64))
        for form, tag in ((ops.SIM_BOUND_TABLE, "table"), (ops.SIM_BOUND_PLAIN, "plain")):
            put(f"bound/{name}-{tag}", run_bound(batch, theta, runs, shift, DEV, form=form))

    def split(name, batch, run):
        """``run(buffer_bytes)`` at the default budget and at one unit of the batch's widest circuit."""
        put(name, run(None))
        put(f"{name}/split", run(ops.mps_workspace_bytes(int(batch.n_qubits.max()), batch.max_bond, 1)))

    section("mps")
    for case in mc.grid():
        batch = mc.lower(case)
        split(f"mps/{case['id']}", batch, lambda bb: sim.run_mps(batch, case["seed"], None, DEV, True, bb))
    section("mps_relax")
    for cid, case in mr.grid().items():
        batch = mr.lower(cid)
        split(f"mps_relax/{cid}", batch, lambda bb: sim.run_mps(batch, case["seed"], None, DEV, True, bb))
    section("mps_shots")
    for cid, case in ms.grid().items():
        batch = ms.lower(cid)
        split(f"mps_shots/{cid}", batch.mps, lambda bb: sim.run_mps_shots(batch, case["shots"], case["seed"], None, True, DEV, bb))
    section("mps_zne")
    for case in mz.grid():
        batch, sch = mz.lowered(case["id"])
        split(f"mps_zne/{case['id']}", batch, lambda bb: zne.run_mps_folded(batch, sch, case["seed"], None, DEV, True, bb))
    section("mps_bound")
    for case in mbc.grid():
        batch = mbc.lower(case["id"])
        shifted, shift, _ = mps_shift_runs(batch, case["pair"])
        for tag, runs, sh in (("plain", mbc.plain_runs(case), None), ("shifted", shifted, shift)):
            split(f"mps_bound/{case['id']}-{tag}", batch,
                  lambda bb: sim.run_mps_bound(batch, case["rows"], runs, sh, case["seed"], None, DEV, True, bb))
    section("mps_twirl")
    for cid, case in mt.grid().items():
        batch = mt.lower(cid)
        split(f"mps_twirl/{cid}", batch, lambda bb: sim.run_mps(batch, case["seed"], None, DEV, True, bb))
        if not case["relaxation"]:   # folded runs refuse relaxation records
            sch = zne.build_mps_schedules(batch, mt.FOLD_FACTORS, zc.make_amplifier(zc.LOCAL_2Q))
            split(f"mps_twirl/{cid}-folded", batch, lambda bb: zne.run_mps_folded(batch, sch, case["seed"], None, DEV, True, bb))
    section("frames")
    for kind, mixed in fc.GRID_COMBOS:
        cases = [fc.grid_case(n, mixed) for n in fc.GRID_N]   # fc.grid_batch's lowering, without its host oracle
        batch = sim.compile_clifford_frames([c for c, _ in cases], [t for _, t in cases], fc.GRID_NOISE[kind]())
        for shots in fc.GRID_SHOTS:
            put(f"frames/{kind}-{int(mixed)}-{shots}", sim.run_clifford_frames(batch, shots, fc.GRID_SEED, None, False, DEV))
    section("estimator")
    import json

    def jobs(name, est, circuits, observables, rows=None):
        """Two successive jobs of one estimator: the values, every metadata field as an array, the job id and the key lists."""
        for j in (1, 2):
            job = est.run(circuits, observables, rows)
            res, tag = job.result(), f"estimator/{name}/job{j}"
            arrays[f"{tag}/values"], arrays[f"{tag}/job_id"] = np.asarray(res.values), np.asarray(job.job_id())
            arrays[f"{tag}/keys"] = np.asarray([",".join(m) for m in res.metadata])
            for key in res.metadata[0]:
                if key == "zne":
                    arrays[f"{tag}/zne/keys"] = np.asarray([",".join(m["zne"]) for m in res.metadata])
                    for k in res.metadata[0]["zne"]:
                        arrays[f"{tag}/zne/{k}"] = np.asarray([m["zne"][k] for m in res.metadata])
                else:
                    arrays[f"{tag}/{key}"] = np.asarray([m[key] for m in res.metadata])

    # the circuits come from the golden files and this tree's case modules, the estimators from blackwater.sim alone
    with open(os.path.join(ROOT, "tests", "golden", "g1_circuits.json")) as fh:
        g1 = list(json.load(fh)[:6])
    g1_obs = [[("IIIIZ", 1.0)] if k % 2 else [("IIIZI", 0.5), ("IIZII", -2.0)] for k in range(6)]
    lima = bc.lima_noise()
    ideal, noisy = mc.case("tfim-cx-J1.9-s3-b4"), mc.case("noisy-readout-T64")   # lines: what the matrix-product-state methods take
    line, line_obs, line_noise = noisy["circuits"], noisy["observables"], mc.noise_model("readout", 11)
    cliffords, clifford_obs = zip(*(fc.grid_case(n, False) for n in (5, 33)))
    clifford_noise = fc.GRID_NOISE["readout"]()
    bound, bound_noisy = mbc.case("tfim-n12-s3-b4"), mbc.case("noisy-readout-T4")
    per_row = [[bound_noisy[k][c] for c in bound_noisy["pair"]] for k in ("templates", "observables")]
    theta = [row[:t.num_parameters] for row, t in zip(bound_noisy["rows"].tolist(), per_row[0])]
    wide = dict(max_bond=4, trajectories=4)
    for cls, tag in ((sim.DeviceEstimator, ""), (zne.zne(sim.DeviceEstimator), "zne-")):
        jobs(f"{tag}exact", cls(lima, DEV), g1, g1_obs)
        jobs(f"{tag}exact-shots", cls(lima, DEV, shots=1000, seed=3), g1, g1_obs)
        jobs(f"{tag}clifford", cls(clifford_noise, DEV, method="clifford"), cliffords, clifford_obs)
        jobs(f"{tag}mps-noise", cls(line_noise, DEV, method="mps", seed=5, **wide), line, line_obs)
    jobs("frames", sim.DeviceEstimator(clifford_noise, DEV, method="frames", shots=64, seed=3), cliffords, clifford_obs)
    jobs("trajectories", sim.DeviceEstimator(lima, DEV, method="trajectories", trajectories=16, seed=3), g1, g1_obs)
    jobs("mps", sim.DeviceEstimator(None, DEV, method="mps", max_bond=4), ideal["circuits"], ideal["observables"])
    jobs("mps_shots", sim.DeviceEstimator(None, DEV, method="mps_shots", shots=64, seed=3, max_bond=4), ideal["circuits"], ideal["observables"])
    jobs("mps_shots-noise", sim.DeviceEstimator(line_noise, DEV, method="mps_shots", shots=64, seed=3, **wide), line, line_obs)
    jobs("bound-exact", sim.DeviceEstimator(line_noise, DEV), *per_row, theta)
    jobs("bound-mps", sim.DeviceEstimator(None, DEV, method="mps", max_bond=4), bound["templates"] * 2, bound["observables"] * 2,
         bound["rows"].tolist())
    jobs("bound-mps-noise", sim.DeviceEstimator(line_noise, DEV, method="mps", seed=5, **wide), *per_row, theta)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"wrote {len(arrays)} arrays to {out} with {os.environ.get('MLQEM_LIB') or f'the library of {PACKAGE_ROOT}'}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="the .npz to write (a few MB: keep it out of the repository)")
    ap.add_argument("--package-root", metavar="DIR", help="import blackwater from this tree (default: the script's own)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"), help="compare two dumps array for array and exit (1: some differ)")
    args = ap.parse_args()
    if not args.compare and not args.out:
        ap.error("give --out FILE to dump, or --compare A B")
    sys.exit(compare(*args.compare) if args.compare else dump(args.out))
