"""Times the regression-forest kernel (csrc/forest.hip) and the decorator path built on it against what they replace, on one box in
one call: scikit-learn's ``predict`` on the same forest and rows, and ``ScikitLearningModelProcessor`` through ``learning(...)``.

    python scripts/forest_micro.py [--out profiles/forest_micro.json] [--quick]

Kernel points: forests of 100 and 300 trees, depth <= 20, on rows of F = 58 and 170 features, scored on 1 024 / 100 000 / 1 000 000
rows.  With scikit-learn importable the forests are fitted by it (``RandomForestRegressor(max_depth=20, max_features="sqrt")`` on
2 000 seeded rows: about 2 600 nodes a tree) and converted with ``ForestRegressor.from_sklearn``, so both sides score the SAME forest;
without it they are grown from a seed and the scikit-learn fields are null with the reason.  Device time: device events around one
call, 5 warm-ups, then the median of 20.  ``hbm_fraction`` is the ALGORITHMIC bytes (4 rows F + forest bytes + 8 rows K) over the
kernel time as a share of the 8 TB/s peak: the walk is a chain of dependent reads, so a low share is expected and is not a defect.
Decorator point: 1 024 distinct 4-qubit OpenQASM texts with a one-term observable each, a 300-tree forest on the 76-wide rows; host
clock around ``run().result()`` (which ends in a device-to-host copy), one warm-up, median of 3 (the scikit-learn path: one run).
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

from blackwater.data.backends import PauliObservable, StaticBackend  # noqa: E402
from blackwater.library.learning.estimator import (ForestLearningModelProcessor, ScikitLearningModelProcessor,  # noqa: E402
                                                   learning)
from blackwater.nn import ForestRegressor  # noqa: E402

DEV = "cuda:0"
HBM_PEAK = 8.0e12   # bytes/s
K = 4

try:
    import sklearn
    from sklearn.ensemble import RandomForestRegressor
    NO_SKLEARN = None
except ImportError as exc:   # the device side is still measured; the comparison fields say why they are empty
    sklearn, NO_SKLEARN = None, f"scikit-learn is not importable here ({exc})"


def seeded_forest(rng, F, T, depth=20, splits=1300):
    """Without scikit-learn: T random trees of ``splits`` splits, no deeper than ``depth``, thresholds from N(0, 1)."""
    parts = []
    for _ in range(T):
        feature, threshold, left, right, dep, open_leaves = [-2], [-2.0], [-1], [-1], [0], [0]
        for _ in range(splits):
            if not open_leaves:
                break
            i = open_leaves.pop(int(rng.integers(len(open_leaves))))
            feature[i], threshold[i], left[i], right[i] = int(rng.integers(F)), float(rng.normal()), len(feature), len(feature) + 1
            for _ in range(2):
                feature.append(-2); threshold.append(-2.0); left.append(-1); right.append(-1); dep.append(dep[i] + 1)
                if dep[-1] < depth:
                    open_leaves.append(len(feature) - 1)
        parts.append((feature, threshold, left, right))
    tree_ptr = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.int64)
    cols = [np.concatenate([np.asarray(p[i]) for p in parts]) for i in range(4)]
    value = rng.uniform(-1, 1, size=(int(tree_ptr[-1]), K))
    return ForestRegressor.from_arrays(tree_ptr, cols[0].astype(np.int64), cols[1], cols[2].astype(np.int64), cols[3].astype(np.int64), value, F)


def device_time(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record()
        fn()
        end.record()
        end.synchronize()
        times.append(beg.elapsed_time(end) * 1e-3)
    return statistics.median(times)


def host_time(fn, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def kernel_points(sizes, configs):
    points = []
    for F, T in configs:
        rng = np.random.default_rng(1000 * F + T)
        rf = None
        if sklearn is not None:
            xt = rng.normal(size=(2000, F)).astype(np.float32)
            yt = xt[:, :K] * 0.5 + rng.normal(size=(2000, K))
            rf = RandomForestRegressor(n_estimators=T, max_depth=20, max_features="sqrt", random_state=0, n_jobs=16).fit(xt, yt)
            rf.n_jobs = None
            forest = ForestRegressor.from_sklearn(rf)
        else:
            forest = seeded_forest(rng, F, T)
        forest_bytes = sum(b.numel() * b.element_size() for b in forest.buffers())
        forest = forest.to(DEV)
        for n in sizes:
            x_host = rng.normal(size=(n, F)).astype(np.float32)
            x = torch.from_numpy(x_host).to(DEV)
            out = torch.empty((n, K), dtype=torch.float64, device=DEV)
            from blackwater.native import ops
            seconds = device_time(lambda: ops.forest_predict(x, forest.nodes, forest.tree_ptr, forest.value, forest.max_depth, out=out))
            algo_bytes = 4 * n * F + forest_bytes + 8 * n * K
            point = {"features": F, "trees": T, "rows": n, "nodes": int(forest.nodes.shape[0]), "max_depth": forest.max_depth,
                     "forest_bytes": forest_bytes, "kernel_seconds": seconds, "rows_per_second": n / seconds,
                     "algorithmic_bytes": algo_bytes, "hbm_fraction_of_8TBps": algo_bytes / seconds / HBM_PEAK}
            if rf is not None:
                want = rf.predict(x_host)    # warm-up of the host path, and the check that both sides score the same forest
                point["max_abs_diff_vs_sklearn"] = float(np.abs(out.cpu().numpy() - want).max())
                point["sklearn_predict_seconds"] = host_time(lambda: rf.predict(x_host), 1 if n > 100000 else 3)
                point["speedup_vs_sklearn"] = point["sklearn_predict_seconds"] / seconds
            else:
                point["sklearn_predict_seconds"], point["sklearn_missing"] = None, NO_SKLEARN
            print(json.dumps(point), flush=True)
            points.append(point)
            del x, out
    return points


class _Result:
    def __init__(self, values):
        self.values, self.metadata = np.asarray(values, dtype=float), [{} for _ in values]


class _Job:
    def __init__(self, values):
        self._values = values

    def result(self):
        return _Result(self._values)

    def job_id(self):
        return "job"


class FakeEstimator:
    """Stand-in for a qiskit BaseEstimator whose noisy values are seeded numbers (no simulator in the timing)."""

    def run(self, circuits, observables, parameter_values=None, **opts):
        return self._run(circuits, observables, parameter_values or [()] * len(circuits), **opts)

    def _run(self, circuits, observables, parameter_values, **opts):
        return _Job(np.random.default_rng(len(circuits)).uniform(-1, 1, size=len(circuits)).tolist())


def random_texts(count, seed=0):
    rng = np.random.default_rng(seed)
    texts = []
    for _ in range(count):
        lines = ['OPENQASM 2.0;', 'include "qelib1.inc";', "qreg q[4];", "creg c[4];"]
        for _ in range(int(rng.integers(20, 60))):
            kind = int(rng.integers(4))
            a = int(rng.integers(4))
            if kind == 0:
                lines.append(f"rz({rng.uniform(-3.0, 3.0)!r}) q[{a}];")
            elif kind == 1:
                lines.append(f"sx q[{a}];")
            elif kind == 2:
                lines.append(f"x q[{a}];")
            else:
                lines.append(f"cx q[{a}],q[{(a + 1) % 4}];")
        lines += [f"measure q[{i}] -> c[{i}];" for i in range(4)]
        texts.append("\n".join(lines) + "\n")
    return texts


def decorator_point(count):
    backend = StaticBackend.from_json(os.path.join(ROOT, "tests", "golden", "fake_lima_backend_props.json"))
    texts = random_texts(count)
    labels = ["ZIIII", "IZIII", "IIZII", "IIIZI"]
    obs = [PauliObservable(labels[k % 4]) for k in range(count)]
    from blackwater.data.utils import encode_pauli_sum_op, get_backend_properties_v1
    from blackwater.library.learning.features import encode_data

    props = get_backend_properties_v1(backend)
    rows, _ = encode_data(circuits=texts, properties=props, ideal_exp_vals=[[0.0]] * count, noisy_exp_vals=[[0.1]] * count, num_qubits=1,
                          meas_bases=[encode_pauli_sum_op([(labels[k % 4], 1.0)])[0] for k in range(count)], native=True)
    rows = rows.numpy().astype(np.float32)
    rng = np.random.default_rng(7)
    point = {"circuits": count, "trees": 300, "row_width": int(rows.shape[1])}
    if sklearn is not None:
        rf = RandomForestRegressor(n_estimators=300, random_state=0, n_jobs=16).fit(rows, rng.normal(size=count))
        rf.n_jobs = None
        forest = ForestRegressor.from_sklearn(rf)
    else:
        forest = seeded_forest(rng, rows.shape[1], 300)
    device_cls = learning(FakeEstimator, ForestLearningModelProcessor(forest, backend, device=DEV), skip_transpile=True)
    got = device_cls().run(texts, obs).result().values   # warm-up
    point["device_seconds"] = host_time(lambda: device_cls().run(texts, obs).result(), 3)
    point["device_circuits_per_second"] = count / point["device_seconds"]
    if sklearn is not None:
        host_cls = learning(FakeEstimator, ScikitLearningModelProcessor(rf, backend), skip_transpile=True)
        t0 = time.perf_counter()
        want = host_cls().run(texts, obs).result().values
        point["sklearn_seconds"] = time.perf_counter() - t0
        point["max_abs_diff_vs_sklearn"] = float(np.abs(got - want).max())
        point["speedup_vs_sklearn"] = point["sklearn_seconds"] / point["device_seconds"]
    else:
        point["sklearn_seconds"], point["sklearn_missing"] = None, NO_SKLEARN
    print(json.dumps(point), flush=True)
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_micro.json"))
    ap.add_argument("--quick", action="store_true", help="a rehearsal: small sizes, not a measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("forest_micro: needs the GPU (there is no host path to time)")
    sizes = [1024, 20000] if args.quick else [1024, 100000, 1000000]
    configs = [(58, 100)] if args.quick else [(58, 100), (58, 300), (170, 100), (170, 300)]
    result = {"device": torch.cuda.get_device_name(0), "sklearn": None if sklearn is None else sklearn.__version__,
              "method": "device events, 5 warm-ups, median of 20; scikit-learn: host clock, median of 3 (one run above 100 000 rows)",
              "quick": args.quick, "kernel": kernel_points(sizes, configs), "decorator": decorator_point(64 if args.quick else 1024)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
