"""Times ``BoostedRegressor.fit`` and ``predict`` (csrc/boost.hip, csrc/forest_fit.hip) against what they replace, on one box in one
call: scikit-learn's ``GradientBoostingRegressor(n_estimators=T, max_depth=3)`` on the same rows.

    python scripts/boost_micro.py [--out profiles/boost_micro.json] [--shapes demo1,demo2,g1,scale] [--quick]

Shapes (rows x F), each with T = 100 stages of depth 3: demo1 100 x 170; demo2 2 500 x 169; the G1 regime 2 000 x 58; one scale point
100 000 x 58.  Rows are the seeded stand-ins of scripts/forest_fit_micro.py; y is a smooth function of three columns plus noise.
  fit        ``BoostedRegressor.fit`` end to end on the host clock with a final device wait (argsort, every stage's launches and
             per-level reads, the update kernel, the one copy of the node store, host validation and packing): 1 warm-up, median of 5;
  kernels    one more fit through ``ops.boost_fit(profile=...)`` with device events around every launch: seconds per kernel and its
             share of their sum -- ``update`` is the boosting step (the events cost launches a little: not the end-to-end number);
  scikit     ``GradientBoostingRegressor(random_state=0).fit`` on the host clock, median of 3 (one run where a run takes longer than
             20 s).  It is single-threaded by design (stages are sequential and its tree builder does not thread).  At the scale
             point it is timed on T / 10 stages and scaled by 10 (said so in the result): every stage costs the same passes;
  predict    the model of the g1 shape on 1 024, 100 000 and 1 000 000 rows: ``predict`` with device events, 3 warm-ups, median of
             20, the output buffer given; scikit-learn's ``predict`` of its own 100-stage model on the same rows, host clock, median
             of 3.
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
from blackwater.nn import BoostedRegressor  # noqa: E402

DEV = "cuda:0"
SHAPES = {"demo1": (100, 170), "demo2": (2500, 169), "g1": (2000, 58), "scale": (100000, 58)}
PREDICT_ROWS = (1024, 100000, 1000000)

try:
    import sklearn
    from sklearn.ensemble import GradientBoostingRegressor
except ImportError as exc:   # the device side is still measured; the comparison fields say why they are empty
    sklearn, NO_SKLEARN = None, f"scikit-learn is not importable here ({exc})"


def make_rows(n, F, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)
    X[:, F // 2:] = rng.poisson(3.0, size=(n, F - F // 2)).astype(np.float32)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] * (X[:, -1] > 2) + 0.1 * rng.standard_normal(n)
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


def host_clocked(fn):
    def run():
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0
    first = run()
    return first if first > 20.0 else statistics.median([first, run(), run()])


def point(name, n, F, T):
    X, y = make_rows(n, F, seed=n + F)
    x_d, y_d = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    model = None

    def fit():
        nonlocal model
        model = BoostedRegressor.fit(x_d, y_d, n_estimators=T, max_depth=3)

    seconds, runs = clocked(fit, reps=5, warm=1)
    p = {"shape": name, "rows": n, "features": F, "stages": T, "max_depth": 3, "fit_end_to_end_seconds": seconds, "fit_runs_seconds": runs,
         "levels": model.fit_info["levels"], "nodes": int(model.nodes.shape[0]), "train_score_first_last": [float(model.train_score_[0]),
                                                                                                          float(model.train_score_[-1])]}
    profile = {}
    ops.boost_fit(x_d, y_d, torch.ones((T, n), dtype=torch.int32, device=DEV), learning_rate=0.1, max_depth=3, profile=profile)
    torch.cuda.synchronize()
    per_kernel = {k: sum(a.elapsed_time(b) for a, b in v) * 1e-3 for k, v in profile.items()}
    total = sum(per_kernel.values())
    p["kernel_seconds"] = total
    p["kernels"] = {k: {"seconds": s, "launches": len(profile[k]), "share_of_kernel_time": s / total} for k, s in per_kernel.items()}
    if sklearn is not None:
        if n >= 50000:
            p["sklearn_fit_seconds"] = 10.0 * host_clocked(lambda: GradientBoostingRegressor(n_estimators=T // 10, random_state=0).fit(X, y))
            p["sklearn_note"] = f"timed on {T // 10} stages and scaled by 10"
        else:
            p["sklearn_fit_seconds"] = host_clocked(lambda: GradientBoostingRegressor(n_estimators=T, random_state=0).fit(X, y))
        p["speedup_vs_sklearn"] = p["sklearn_fit_seconds"] / seconds
    else:
        p["sklearn_missing"] = NO_SKLEARN
    print(json.dumps(p), flush=True)
    return p, model, (X, y)


def predict_points(model, X, y, T, rows):
    out = []
    sk = GradientBoostingRegressor(n_estimators=T, random_state=0).fit(X, y) if sklearn is not None else None
    for n in rows:
        pick = np.random.default_rng(n).integers(0, len(X), size=n)
        Xn = X[pick]
        x_d = torch.from_numpy(Xn).to(DEV)
        buf = torch.empty(n, dtype=torch.float64, device=DEV)
        times = []
        for rep in range(23):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.boost_predict(x_d, model.nodes, model.tree_ptr, model.value, model.max_depth, model.init, model.learning_rate, out=buf)
            b.record()
            torch.cuda.synchronize()
            if rep >= 3:
                times.append(a.elapsed_time(b) * 1e-3)
        p = {"rows": n, "stages": T, "predict_seconds": statistics.median(times), "rows_per_second": n / statistics.median(times)}
        if sk is not None:
            p["sklearn_predict_seconds"] = host_clocked(lambda: sk.predict(Xn))
            p["speedup_vs_sklearn"] = p["sklearn_predict_seconds"] / p["predict_seconds"]
        print(json.dumps(p), flush=True)
        out.append(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boost_micro.json"))
    ap.add_argument("--shapes", default="demo1,demo2,g1,scale")
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a tenth of the rows and stages, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("boost_micro: needs the GPU (there is no host path to time)")
    points, predict = [], []
    result = {"device": torch.cuda.get_device_name(0), "sklearn": None if sklearn is None else sklearn.__version__,
              "method": "host clock around BoostedRegressor.fit with a final device wait, 1 warm-up, median of 5; device events around "
                        "every launch in one further fit; scikit-learn (single-threaded by design) on the host clock, median of 3 (one "
                        "run above 20 s); predict with device events, 3 warm-ups, median of 20",
              "quick": args.quick, "points": points, "predict": predict}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # after every point: a long run that is cut short keeps what it measured
            json.dump(result, fh, indent=1)

    for name in args.shapes.split(","):
        n, F = SHAPES[name]
        T = 100
        if args.quick:
            n, T = max(n // 10, 10), 10
        p, model, (X, y) = point(name, n, F, T)
        points.append(p)
        save()
        if name == "g1":
            predict.extend(predict_points(model, X, y, T, [r // 10 for r in PREDICT_ROWS] if args.quick else PREDICT_ROWS))
            save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
