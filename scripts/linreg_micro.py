"""Times the least-squares kernels (csrc/linreg.hip) against what they replace, on one box in one call: scikit-learn's
``LinearRegression().fit`` and ``.predict`` on the same rows.

    python scripts/linreg_micro.py [--out profiles/linreg_micro.json] [--quick]

Points: 1 000 000 rows of F + K = 58 + 4 (the encode_data rows of the tutorials) and 170 + 1 (encode_data_v2_ecr, demo1).
Device time: device events around one call, 5 warm-ups, then the median of 20, on THREE sets of input buffers used in turn (one set is
236 / 684 MB, so a call never finds its rows in the 256 MB Infinity Cache).  ``moments`` is the whole ``ops.linreg_moments`` call: the
tile kernel, the reduction over the chunks' partial sums and the workspace allocation from torch's caching allocator.
  predict   algorithmic bytes (4 n F in, 8 n K out) over the time as a share of the 8 TB/s HBM peak;
  moments   algorithmic bytes (4 n (F + K)) as a share of 8 TB/s, and fp64 FLOP/s twice: the USEFUL count 2 n D (D + 1) / 2 (one
            triangle) and the count the kernel EXECUTES, 2 n 4096 per 64 x 64 tile of the lower triangle (diagonal tiles are
            computed whole and the last tile of a row is padded), the latter as a share of the 78.6 TFLOP/s fp64 vector peak;
  fit       ``LinearRegressor.fit`` end to end on the host clock: moments, the [D, D] copy, the host solve, the model back on the
            device.
Host: ``LinearRegression().fit(X, Y)`` and ``.predict(X)`` on the same float32 arrays, host clock, median of 3.
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
from blackwater.nn import LinearRegressor  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12        # bytes/s
FP64_VECTOR_PEAK = 78.6e12   # FLOP/s
ROTATE = 3

try:
    import sklearn
    from sklearn.linear_model import LinearRegression
    NO_SKLEARN = None
except ImportError as exc:   # the device side is still measured; the comparison fields say why they are empty
    sklearn, NO_SKLEARN = None, f"scikit-learn is not importable here ({exc})"


def device_time(fn, warm=5, reps=20):
    """Median device time of ``fn(i)``; i counts calls, so the caller can rotate its buffers."""
    for i in range(warm):
        fn(i)
    times = []
    for i in range(reps):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        fn(warm + i)
        end.record()
        end.synchronize()
        times.append(beg.elapsed_time(end) * 1e-3)
    return statistics.median(times)


def host_time(fn, reps=3):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def point(n, F, K):
    rng = np.random.default_rng(1000 * F + K)
    true = rng.standard_normal((F, K)) / np.sqrt(F)
    hosts = []
    for _ in range(ROTATE):
        X = rng.standard_normal((n, F), dtype=np.float32)
        Y = (X @ true.astype(np.float32) + 0.1 * rng.standard_normal((n, K), dtype=np.float32)).astype(np.float32)
        hosts.append((X, Y))
    xs = [torch.from_numpy(X).to(DEV) for X, _ in hosts]
    ys = [torch.from_numpy(Y).to(DEV) for _, Y in hosts]
    D = 1 + F + K
    tiles_1d = (D + 63) // 64
    tiles = tiles_1d * (tiles_1d + 1) // 2
    moments = torch.empty((D, D), dtype=torch.float64, device=DEV)
    out = torch.empty((n, K), dtype=torch.float64, device=DEV)
    p = {"rows": n, "features": F, "outputs": K, "rotated_buffer_sets": ROTATE}

    t = device_time(lambda i: ops.linreg_moments(xs[i % ROTATE], ys[i % ROTATE], out=moments))
    useful, executed = 2.0 * n * D * (D + 1) / 2, 2.0 * n * 4096 * tiles
    p["moments"] = {"seconds": t, "algorithmic_bytes": 4 * n * (F + K), "GBps": 4 * n * (F + K) / t / 1e9,
                    "hbm_fraction_of_8TBps": 4 * n * (F + K) / t / HBM_PEAK, "useful_fp64_TFLOPs": useful / t / 1e12,
                    "executed_fp64_TFLOPs": executed / t / 1e12, "executed_fraction_of_78.6_TFLOPs": executed / t / FP64_VECTOR_PEAK,
                    "tiles": tiles}
    model = LinearRegressor.fit(xs[0], ys[0])
    p["fit_end_to_end_seconds"] = host_time(lambda: LinearRegressor.fit(xs[1], ys[1]))
    p["rank"] = model.rank_
    t = device_time(lambda i: ops.linreg_predict(xs[i % ROTATE], model.coef, model.intercept, out=out))
    nbytes = 4 * n * F + 8 * n * K
    p["predict"] = {"seconds": t, "algorithmic_bytes": nbytes, "GBps": nbytes / t / 1e9, "hbm_fraction_of_8TBps": nbytes / t / HBM_PEAK}
    if sklearn is not None:
        X, Y = hosts[0]
        ols = LinearRegression().fit(X, Y)
        p["sklearn_fit_seconds"] = host_time(lambda: LinearRegression().fit(X, Y))
        p["sklearn_predict_seconds"] = host_time(lambda: ols.predict(X))
        ols64 = LinearRegression().fit(X[:100000].astype(np.float64), Y[:100000].astype(np.float64))
        sub = LinearRegressor.fit(xs[0][:100000], ys[0][:100000])
        p["max_abs_coef_diff_vs_sklearn_fp64_on_100k_rows"] = float(np.abs(sub.coef.cpu().numpy() - np.atleast_2d(ols64.coef_)).max())
        p["fit_speedup_vs_sklearn"] = p["sklearn_fit_seconds"] / p["fit_end_to_end_seconds"]
        p["predict_speedup_vs_sklearn"] = p["sklearn_predict_seconds"] / p["predict"]["seconds"]
    else:
        p["sklearn_fit_seconds"], p["sklearn_predict_seconds"], p["sklearn_missing"] = None, None, NO_SKLEARN
    print(json.dumps(p), flush=True)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linreg_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: small sizes, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("linreg_micro: needs the GPU (there is no host path to time)")
    n = 20000 if args.quick else 1000000
    result = {"device": torch.cuda.get_device_name(0), "sklearn": None if sklearn is None else sklearn.__version__,
              "method": "device events, 5 warm-ups, median of 20, three input buffer sets in turn; host clock, median of 3, for the "
                        "end-to-end fit and scikit-learn",
              "quick": args.quick, "points": [point(n, 58, 4), point(n, 170, 1)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
