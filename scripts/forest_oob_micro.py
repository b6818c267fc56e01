"""Times the out-of-bag prediction (``mlqem_forest_predict_oob_f32``, csrc/forest.hip with OOB = true) against the plain prediction of
the same forest on the same rows, and ``ForestRegressor.fit(oob_score=True)`` against ``fit()``, on one box in one call.

    python scripts/forest_oob_micro.py [--out profiles/forest_oob_micro.json] [--shapes g1,demo2,scale,wide] [--quick]

Shapes (rows x F x K, T), those of the fit table: g1 2 000 x 58 x 4, 300; demo2 2 500 x 169 x 1, 100; scale 100 000 x 58 x 4, 100; and
wide, 1 000 000 rows x 100 trees for the 64-row tile: the forest of the scale point (fitted on its 100 000 rows) scoring 1 000 000
seeded rows, with counts drawn as Poisson(1) per (tree, row) -- the share of zeros of a bootstrap, e^-1 -- because a forest fitted
on a million rows is not what this point is about.  Rows are the seeded stand-ins of scripts/forest_fit_micro.py.
  predict    device events around ONE call with preallocated outputs, 5 warm-ups of each kind, then 20 rounds of
             (plain, masked, plain) in one process; ``plain`` and ``masked`` are the medians of the 40 and the 20 times.
             ``ratio`` = masked / plain.  ``plain_spread`` = (the larger over the smaller) of the medians of the first and the second
             plain call of the rounds: what two measurements of the SAME kernel differ by here;
  fit        host clock around ``ForestRegressor.fit`` with a final device wait, 1 warm-up each, 5 rounds of (fit(), fit(oob_score=True),
             fit()), medians, ratio and spread formed the same way.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ml-qem_amd"), os.path.join(ROOT, "scripts")]
import torch  # noqa: E402

from blackwater.native import ops  # noqa: E402
from blackwater.nn import ForestRegressor  # noqa: E402
from forest_fit_micro import make_rows  # noqa: E402

DEV = "cuda:0"
SHAPES = {"g1": (2000, 58, 4, 300, None), "demo2": (2500, 169, 1, 100, None), "scale": (100000, 58, 4, 100, None),
          "wide": (100000, 58, 4, 100, 1000000)}   # (fit rows, F, K, T, rows scored when they are not the fit's)


def event_seconds(fn):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e-3


def clock_seconds(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(plain, masked, timer, warm, rounds):
    """Rounds of (plain, masked, plain): medians, their ratio, and the spread of the two plain series."""
    for _ in range(warm):
        plain()
        masked()
    first, mid, second = [], [], []
    for _ in range(rounds):
        first.append(timer(plain))
        mid.append(timer(masked))
        second.append(timer(plain))
    a, b = statistics.median(first), statistics.median(second)
    p, m = statistics.median(first + second), statistics.median(mid)
    return {"plain_seconds": p, "masked_seconds": m, "ratio": m / p, "plain_spread": max(a, b) / min(a, b),
            "plain_min_max_seconds": [min(first + second), max(first + second)], "masked_min_max_seconds": [min(mid), max(mid)]}


def point(name, n, F, K, T, scored, with_fit):
    X, y = make_rows(n, F, K, seed=n + F)
    x_d, y_d = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        forest = ForestRegressor.fit(x_d, y_d, n_estimators=T, seed=0, oob_score=True)
    p = {"shape": name, "fit_rows": n, "features": F, "outputs": K, "trees": T, "nodes": int(forest.nodes.shape[0]),
         "max_depth": forest.max_depth, "oob_score": forest.oob_score_}
    if scored is None:
        rows, counts = x_d, forest.fit_info["sample_counts"]
    else:
        rows = torch.from_numpy(make_rows(scored, F, K, seed=scored + F)[0]).to(DEV)
        counts = torch.poisson(torch.ones((T, scored), device=DEV)).to(torch.int32)
        p["counts_note"] = "Poisson(1) per (tree, row), not the fit's bags"
    m = int(rows.shape[0])
    p["rows"] = m
    p["out_of_bag_share"] = float((counts == 0).to(torch.float64).mean())
    out = torch.empty((m, K), dtype=torch.float64, device=DEV)
    n_oob = torch.empty((m,), dtype=torch.int32, device=DEV)
    args = (rows, forest.nodes, forest.tree_ptr, forest.value, forest.max_depth)
    p["predict"] = alternate(lambda: ops.forest_predict(*args, out=out), lambda: ops.forest_predict_oob(*args, counts, out=out, n_oob_out=n_oob),
                             event_seconds, warm=5, rounds=20)
    p["predict"]["extra_bytes_read"] = 4 * T * m
    if with_fit:
        def fit(flag):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                ForestRegressor.fit(x_d, y_d, n_estimators=T, seed=0, oob_score=flag)
        p["fit"] = alternate(lambda: fit(False), lambda: fit(True), clock_seconds, warm=1, rounds=5)
    print(json.dumps(p), flush=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_oob_micro.json"))
    ap.add_argument("--shapes", default="g1,demo2,scale,wide")
    ap.add_argument("--quick", action="store_true", help="a rehearsal: a tenth of the rows and trees, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("forest_oob_micro: needs the GPU (there is no host path to time)")
    torch.manual_seed(0)
    points = []
    result = {"device": torch.cuda.get_device_name(0),
              "method": "predict: device events around one call, 5 warm-ups, 20 rounds of (plain, masked, plain), medians; fit: host clock "
                        "with a final device wait, 1 warm-up, 5 rounds of (fit, fit with oob_score, fit); plain_spread = ratio of the "
                        "medians of the two plain series", "quick": args.quick, "points": points}
    for name in args.shapes.split(","):
        n, F, K, T, scored = SHAPES[name]
        if args.quick:
            n, T, scored = max(n // 10, 10), max(T // 10, 2), None if scored is None else scored // 10
        points.append(point(name, n, F, K, T, scored, with_fit=scored is None))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:      # after every point: a long run that is cut short keeps what it measured
            json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
