"""Times ``ForestRegressor.fit`` (csrc/forest_fit.hip) against what it replaces, on one box in one call: scikit-learn's
``RandomForestRegressor(n_estimators=T).fit`` on the same rows.

    python scripts/forest_fit_micro.py [--out profiles/forest_fit_micro.json] [--shapes demo1,demo2,g1,scale] [--quick]
    python scripts/forest_fit_micro.py --max-features [--out profiles/forest_subset_micro.json] [--shapes ...] [--quick]

Shapes (rows x F x K, T): demo1 100 x 170 x 1, 100; demo2 2 500 x 169 x 1, 100; the G1 regime 2 000 x 58 x 4, 300; one scale point
100 000 x 58 x 4, 100.  Rows are seeded stand-ins for ``encode_data`` rows: the first half of the columns standard normal, the second
half small integer counts (duplicates everywhere); y is a smooth function of three columns plus noise.
  fit        ``ForestRegressor.fit`` end to end on the host clock with a final device wait (argsort, bags, every level's launches and
             read, the copy of the node table, host validation and packing, the buffers back on the device): 1 warm-up, median of 5;
  kernels    one more fit through ``ops.forest_fit(profile=...)`` with device events around every launch: seconds per kernel and its
             share of their sum (the events cost launches a little: this run is not the end-to-end number);
  scikit     ``RandomForestRegressor(n_estimators=T, random_state=0, n_jobs=j).fit`` for j = 1 and 16 on the host clock, median of
             3 (one run where a run takes longer than 20 s).  At the scale point j = 1 is timed on T / 10 trees and scaled by 10
             (said so in the result): trees are independent, and a full run would take tens of minutes.

``--max-features`` measures feature subsets per node instead (no scikit-learn run): per shape, ``fit(max_features=F)`` and
``fit(max_features=max(1, F // 3))`` alternated in one process, 1 warm-up each, median of 5 rounds, then one fit each with device
events around every launch.  ``search`` and ``partition`` walk all F lists either way, so no speed-up is expected; what is watched is
the share of ``select``, whose loop over the features becomes the node's keyed permutation.  There is no threshold.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from blackwater.native import ops  # noqa: E402
from blackwater.nn import ForestRegressor  # noqa: E402
from blackwater.nn.forest import bootstrap_counts  # noqa: E402

DEV = "cuda:0"
SHAPES = {"demo1": (100, 170, 1, 100), "demo2": (2500, 169, 1, 100), "g1": (2000, 58, 4, 300), "scale": (100000, 58, 4, 100)}

try:
    import sklearn
    from sklearn.ensemble import RandomForestRegressor
except ImportError as exc:   # the device side is still measured; the comparison fields say why they are empty
    sklearn, NO_SKLEARN = None, f"scikit-learn is not importable here ({exc})"


def make_rows(n, F, K, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[:, F // 2:] = rng.poisson(3.0, size=(n, F - F // 2)).astype(np.float32)
    y = np.sin(X[:, :1]) + 0.3 * X[:, 1:2] * (X[:, -1:] > 2) + 0.1 * rng.standard_normal((n, K))
    return X, y.astype(np.float64)


def clocked(fn, reps, warm):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def sklearn_seconds(X, y, trees, jobs):
    def run():
        t0 = time.perf_counter()
        RandomForestRegressor(n_estimators=trees, random_state=0, n_jobs=jobs).fit(X, y if y.shape[1] > 1 else y[:, 0])
        return time.perf_counter() - t0
    first = run()
    return first if first > 20.0 else statistics.median([first, run(), run()])


def point(name, n, F, K, T):
    X, y = make_rows(n, F, K, seed=n + F)
    x_d, y_d = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    forest = None

    def fit():
        nonlocal forest
        forest = ForestRegressor.fit(x_d, y_d, n_estimators=T, seed=0)

    seconds, runs = clocked(fit, reps=5, warm=1)
    p = {"shape": name, "rows": n, "features": F, "outputs": K, "trees": T, "fit_end_to_end_seconds": seconds, "fit_runs_seconds": runs,
         "levels": forest.fit_info["levels"], "nodes": int(forest.nodes.shape[0]), "max_depth": forest.max_depth,
         "trees_per_chunk": forest.fit_info["trees_per_chunk"], "workspace_bytes_per_tree": ops.forest_fit_tree_bytes(n, F, K)}
    p["workspace_bytes"] = p["workspace_bytes_per_tree"] * p["trees_per_chunk"] + 4 * F * n
    p.update(kernel_split(x_d, y_d, bootstrap_counts(n, T, 0).to(DEV)))
    if sklearn is not None:
        if n >= 50000:
            p["sklearn_seconds_1_job"] = 10.0 * sklearn_seconds(X, y, T // 10, 1)
            p["sklearn_1_job_note"] = f"timed on {T // 10} trees and scaled by 10"
        else:
            p["sklearn_seconds_1_job"] = sklearn_seconds(X, y, T, 1)
        p["sklearn_seconds_16_jobs"] = sklearn_seconds(X, y, T, 16)
        p["speedup_vs_1_job"] = p["sklearn_seconds_1_job"] / seconds
        p["speedup_vs_16_jobs"] = p["sklearn_seconds_16_jobs"] / seconds
    else:
        p["sklearn_missing"] = NO_SKLEARN
    print(json.dumps(p), flush=True)
    return p


def kernel_split(x_d, y_d, counts, **kw):
    profile = {}
    ops.forest_fit(x_d, y_d, counts, profile=profile, **kw)
    torch.cuda.synchronize()
    per_kernel = {k: sum(a.elapsed_time(b) for a, b in v) * 1e-3 for k, v in profile.items()}
    total = sum(per_kernel.values())
    return {"kernel_seconds": total,
            "kernels": {k: {"seconds": s, "launches": len(profile[k]), "share_of_kernel_time": s / total} for k, s in per_kernel.items()}}


def subset_point(name, n, F, K, T):
    """``max_features = F`` against ``max(1, F // 3)``: alternated end-to-end fits, then one profiled fit each."""
    X, y = make_rows(n, F, K, seed=n + F)
    x_d, y_d = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    counts = bootstrap_counts(n, T, 0).to(DEV)
    settings = {"all_features": F, "subset": max(1, F // 3)}
    runs, forests = {k: [] for k in settings}, {}
    for rnd in range(6):                       # round 0 warms both up
        for key, m in settings.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            forests[key] = ForestRegressor.fit(x_d, y_d, n_estimators=T, seed=0, max_features=m)
            torch.cuda.synchronize()
            if rnd:
                runs[key].append(time.perf_counter() - t0)
    p = {"shape": name, "rows": n, "features": F, "outputs": K, "trees": T}
    for key, m in settings.items():
        forest = forests[key]
        p[key] = {"max_features": m, "fit_end_to_end_seconds": statistics.median(runs[key]), "fit_runs_seconds": runs[key],
                  "levels": forest.fit_info["levels"], "nodes": int(forest.nodes.shape[0]), "max_depth": forest.max_depth,
                  **kernel_split(x_d, y_d, counts, max_features=m, seed=0)}
    p["fit_ratio_subset_over_all"] = p["subset"]["fit_end_to_end_seconds"] / p["all_features"]["fit_end_to_end_seconds"]
    print(json.dumps(p), flush=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/forest_fit_micro.json, or profiles/forest_subset_micro.json with --max-features")
    ap.add_argument("--max-features", action="store_true", help="measure max_features = F against max(1, F // 3) instead (no scikit-learn)")
    ap.add_argument("--shapes", default="demo1,demo2,g1,scale")
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a tenth of the rows and trees, not a measurement")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "forest_subset_micro.json" if args.max_features else "forest_fit_micro.json")
    if not torch.cuda.is_available():
        sys.exit("forest_fit_micro: needs the GPU (there is no host path to time)")
    points = []
    if args.max_features:
        result = {"device": torch.cuda.get_device_name(0),
                  "method": "per shape: ForestRegressor.fit(max_features=F) and fit(max_features=max(1, F // 3)) alternated in one process, "
                            "host clock with a final device wait, 1 warm-up each, median of 5; then one fit each through "
                            "ops.forest_fit(profile=...) with device events around every launch",
                  "quick": args.quick, "points": points}
    else:
        result = {"device": torch.cuda.get_device_name(0), "sklearn": None if sklearn is None else sklearn.__version__,
                  "method": "host clock around ForestRegressor.fit with a final device wait, 1 warm-up, median of 5; device events around "
                            "every launch in one further fit; scikit-learn on the host clock, n_jobs 1 and 16, median of 3 (one run above "
                            "20 s)",
                  "quick": args.quick, "points": points}
    for name in args.shapes.split(","):
        n, F, K, T = SHAPES[name]
        points.append((subset_point if args.max_features else point)(name, *((max(n // 10, 10), F, K, max(T // 10, 2)) if args.quick else (n, F, K, T))))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # after every point: a long run that is cut short keeps what it measured
            json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
