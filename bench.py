"""Benchmark of the hot path: circuits/sec of one GNN train step on synthetic 100-qubit TFIM-Trotter graphs.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--batch B] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One step = device batch assembly -> forward -> MSE -> backward -> (gradient all-reduce) -> Adam, nothing skipped.
``--gpus N`` with N > 1 and no WORLD_SIZE in the environment starts the N ranks itself (a child ``torch.distributed.run``,
launched BEFORE this process makes any HIP call) and relays rank 0's line.  The corpus is 8 x batch x N circuits
(">= 8 x batch"), sharded by circuit: rank r builds only its 1/N of the arena in its own HBM
(``DataParallelShard.split`` balances node counts), so per-GPU work is fixed as N grows ("weak").
Rank 0 prints ONE JSON line (contract in the task statement).  A plain run sets up, warms up, times exactly ``--steps``
steps and prints it.  ``--full`` then also measures the host's enqueue time per step and ``roofline`` (the CSR aggregation
kernel, timed live with HIP events on the stream it runs on) and, at N=1, ``cpu_baseline`` (the CPU oracle on a bounded
sample of the same workload), ``parity``, ``accuracy`` and the other legs.  ``--dump-outputs DIR`` writes what the last
timed step computed (``dump_outputs``).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "ml-qem_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import torch


# Circuits per step per GPU.  Sized for 288 GB of HBM rather than for the reference's host-collated batches of 32: one step
# then moves 11 M graph nodes (~20 GB of activations), launches are long enough for their tails not to matter and the
# host has 10 ms to enqueue 2 ms of work.  Measured on one MI355X: 256 -> 88 k, 1024 -> 99-101 k, 2048 -> 101 k circuits/s.
DEFAULT_BATCH = 1024
CORPUS_BATCHES = 8          # corpus = CORPUS_BATCHES x batch x world circuits
STEPS_LIST = list(range(1, 11))
PMC_SUMMARY = os.path.join(ROOT, "profiles", "r05_aggregate_pmc.json")
# per-kernel-name HBM traffic of one replayed Family A step (scripts/make_pmc_step.sh): the newest committed summary
STEP_PMC = [os.path.join(ROOT, "profiles", f"r{r:02d}_step_pmc.json") for r in (6, 5)]


def step_pmc_traffic(kernel_tag):
    """(bytes per launch, source file) of the kernel whose name contains ``kernel_tag`` in the newest committed step PMC summary
    (rocprofv3 --pmc passes cannot run inside this process), or (None, None)."""
    for path in STEP_PMC:
        try:
            with open(path) as fh:
                rows = json.load(fh)["rows"]
        except (OSError, KeyError, ValueError):
            continue
        for r in rows:
            if kernel_tag in r["kernel"].replace(" ", ""):
                return int(r["traffic_GB"] * 1e9), os.path.relpath(path, ROOT)
    return None, None


_T0 = time.perf_counter()


def progress(msg):
    """One line on stderr per leg (stdout carries the ONE JSON line): a run that prints nothing for minutes looks hung."""
    print(f"[bench {time.perf_counter() - _T0:7.1f} s] {msg}", file=sys.stderr, flush=True)


def fixed_ids(n_graphs, batch=DEFAULT_BATCH):
    """The representative batch the roofline leg (and the profiling scripts) use: every step count, evenly."""
    return np.arange(batch) * n_graphs // batch


def build_corpus(n_j, seed=42):
    from blackwater.data.synthetic import TfimCorpus

    return TfimCorpus(100, STEPS_LIST, n_j, seed=seed, two_q="ecr", exp_value_size=1)


def agg_bytes(n, e_with_loops, c):
    """Algorithmic bytes of one CSR aggregation: rowptr + col + norm scalar + one source row per
    edge + one output row per node, fp32 data / int32 indices, no cache credit."""
    return 4 * (n + 1) + 4 * e_with_loops + 4 * n + 4 * c * (e_with_loops + n)


def _timed_launches(run, reps, nbuf):
    """Average seconds per launch of ``run(k)`` with HIP events on the launch stream (torch's current stream IS the stream
    the C ABI is handed, native/ops._stream); ``nbuf`` rotated operand sets are touched first."""
    for k in range(nbuf):
        run(k)
    stream = torch.cuda.current_stream()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record(stream)
    for k in range(reps):
        run(k)
    end.record(stream)
    end.synchronize()
    return beg.elapsed_time(end) * 1e-3 / reps


def in_step_aggregation_times(arena, ids, n_qubits, steps=3):
    """Every CSR aggregation launch of a real train step timed IN the step: an eager, single-stream step of a fresh Family A
    model on the representative batch with ``ops.csr_aggregate`` wrapped in HIP events.  Returns {variant: [us, bytes, count]}
    (variant = what the launch carries: epilogue / z operand / self term / which CSR)."""
    from blackwater.native import ops
    from blackwater.nn import ExpValCircuitGraphModelA
    from blackwater.train import Trainer

    prev = os.environ.get("MLQEM_SINGLE_STREAM")
    os.environ["MLQEM_SINGLE_STREAM"] = "1"
    keep_counter = ops._seed_counter
    ops.set_seed_counter(None)
    records = []
    orig = ops.csr_aggregate
    batch = arena.batch(ids)
    st = batch.structure
    in_ptr = st.in_ptr.data_ptr()
    e_real = st.num_edges

    def wrapped(x, ptr, idx, **kw):
        epi = kw.get("bias") is not None or kw.get("relu") or kw.get("drop_p", 0.0) > 0
        pooled = kw.get("pool") is not None and kw.get("ell") is not None and ops._POOL_FUSED
        name = ("pooled " if pooled else "") + ("epilogue (bias+ReLU+dropout)" if epi else "plain") + (" +z" if kw.get("z") is not None else "") + \
               (" +self" if kw.get("dself") is not None else "") + (" forward CSR" if ptr.data_ptr() == in_ptr else " transposed CSR")
        n, c = x.shape
        by = agg_bytes(n, e_real + (n if kw.get("dself") is not None else 0), c) + (4 * n * c if kw.get("z") is not None else 0)
        b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        out = orig(x, ptr, idx, **kw)
        e.record()
        records.append((name, c, by, b, e))
        return out

    orig_pg = ops.PooledGrad.aggregate

    def wrapped_pg(self, ptr, idx, ell, cscale, rscale=None, dself=None, alpha=1.0, want_g=True):
        # the first backward aggregation of a branch with its source COMPUTED (csrc/pooled_grad.hip): per entry (and the row itself)
        # two scalars and 2 bytes of gate bits instead of a 4 C-byte row; g written or not
        n = self.num_nodes
        c = (self.g_wmean if self.g_wmean is not None else self.g_mean).shape[1]
        e = e_real + n
        by = 4 * (n + 1) + 4 * e + 4 * n + 10 * (e + n) + 4 * c * n * (2 if want_g else 1)
        name = "plain, source computed from the pooled gradient" + (" +g written" if want_g else "") + \
               (" +self" if dself is not None else "") + " transposed CSR"
        b, e_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        b.record()
        out = orig_pg(self, ptr, idx, ell, cscale, rscale=rscale, dself=dself, alpha=alpha, want_g=want_g)
        e_.record()
        records.append((name, c, by, b, e_))
        return out

    try:
        torch.manual_seed(0)
        tr = Trainer(ExpValCircuitGraphModelA(n_qubits, 22, 10).to(st.in_ptr.device), lr=1e-3)
        tr.step(batch)                              # allocator warm-up, untimed
        torch.cuda.synchronize()
        ops.csr_aggregate = wrapped
        ops.PooledGrad.aggregate = wrapped_pg
        for _ in range(steps):
            tr.step(batch)
        torch.cuda.synchronize()
    finally:
        ops.csr_aggregate = orig
        ops.PooledGrad.aggregate = orig_pg
        ops.set_seed_counter(keep_counter)
        if prev is None:
            os.environ.pop("MLQEM_SINGLE_STREAM", None)
        else:
            os.environ["MLQEM_SINGLE_STREAM"] = prev
    agg = {}
    for name, c, by, b, e in records:
        key = f"C={c} {name}"
        t = agg.setdefault(key, [0.0, by, 0])
        t[0] += b.elapsed_time(e) * 1e3
        t[2] += 1
    del tr
    return {k: [v[0] / v[2], v[1], v[2] // steps] for k, v in agg.items()}


def roofline_leg(batch, arena=None, ids=None, n_qubits=100, reps=20):
    """Times the dominant kernel -- the CSR aggregation at C = 10 (the hidden width of the model) -- on the benchmark batch with
    HIP events on the launch stream, in each instantiation the model launches: the plain form (no epilogue; every backward
    aggregation) and the full-epilogue form of the GCN forward (bias + ReLU + dropout: a separate instantiation built for
    seven waves per SIMD), alone with rotated buffers and, when ``arena`` is given, inside a real single-stream train step."""
    from blackwater.native import ops

    s = batch.structure
    n = s.num_nodes
    e_loops = s.num_edges + n  # the self-loop of every node is one more source row (E')
    c = 10
    dev = s.in_ptr.device
    # Four input/output buffer pairs are rotated so that no launch finds its operands in the 256 MiB Infinity Cache left
    # there by the previous one.  Operands in the padded row layout the model uses.
    nbuf = 4
    hs = [ops.padded_empty(n, c, dev).normal_() for _ in range(nbuf)]
    zs = [ops.padded_empty(n, c, dev).normal_() for _ in range(nbuf)]
    outs = [ops.padded_empty(n, c, dev) for _ in range(nbuf)]
    bias = torch.randn(c, device=dev)
    dinv = s.gcn_dinv
    forms = [
        ("csr_aggregate_ell_kernel<4,false,2,false,8> plain: GCN-normalised forward aggregation without epilogue", e_loops, 0,
         lambda k: ops.csr_aggregate(hs[k % nbuf], s.in_ptr, s.in_src, ell=s.in_ell, rscale=dinv, dself=dinv, out=outs[k % nbuf])),
        ("csr_aggregate_ell_kernel<4,false,2,true,7> epilogue: the GCN layer's forward launch (bias + ReLU + dropout 0.1)", e_loops, 0,
         lambda k: ops.csr_aggregate(hs[k % nbuf], s.in_ptr, s.in_src, ell=s.in_ell, rscale=dinv, dself=dinv, bias=bias, relu=True,
                                     drop_p=0.1, seed=1234 + k, out=outs[k % nbuf])),
        ("plain, transposed CSR + self term: the GCN layer's backward launch", e_loops, 0,
         lambda k: ops.csr_aggregate(hs[k % nbuf], s.out_ptr, s.out_dst, ell=s.out_ell, cscale=dinv, rscale=dinv, dself=s.derived("gcn_dself"),
                                     out=outs[k % nbuf])),
        ("plain, transposed CSR, no self term: the Cheb / SAGE backward launches", s.num_edges, 0,
         lambda k: ops.csr_aggregate(hs[k % nbuf], s.out_ptr, s.out_dst, ell=s.out_ell, out=outs[k % nbuf])),
        ("epilogue with a z operand (alpha A x + beta z): the Cheb recurrence / SAGE forward launches", s.num_edges, 4 * n * c,
         lambda k: ops.csr_aggregate(hs[k % nbuf], s.in_ptr, s.in_src, ell=s.in_ell, z=zs[k % nbuf], alpha=2.0, beta=-1.0, out=outs[k % nbuf])),
    ]
    peak = 8000.0  # GB/s, MI355X HBM3E (guide: MI355X_MICROARCH.md chip table)
    variants = []
    for name, e_eff, extra, run in forms:
        sec = _timed_launches(run, reps, nbuf)
        b = agg_bytes(n, e_eff, c) + extra
        variants.append({"launch": name, "bytes_per_launch": int(b), "us_isolated": round(sec * 1e6, 2),
                         "GBps_isolated": round(b / sec / 1e9, 1), "frac_isolated": round(b / sec / 1e9 / peak, 4)})
    sec = variants[0]["us_isolated"] * 1e-6
    b = variants[0]["bytes_per_launch"]
    in_step = None
    if arena is not None:
        rec = in_step_aggregation_times(arena, ids, n_qubits)
        in_step = [{"launch": k, "launches_per_step": v[2], "bytes_per_launch": int(v[1]), "us_in_step": round(v[0], 2),
                    "frac_in_step": round(v[1] / (v[0] * 1e-6) / 1e9 / peak, 4)} for k, v in sorted(rec.items())]
        tot_b = sum(v[1] * v[2] for v in rec.values())
        tot_t = sum(v[0] * v[2] for v in rec.values()) * 1e-6
    del hs, zs, outs
    # the box's own stream-copy rate, for context (SURVEY section 8d asks for the measured peak next to the vendor one)
    stream = torch.cuda.current_stream()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    src_buf = torch.empty(256 << 20, dtype=torch.float32, device=dev).normal_()
    dst_bufs = [torch.empty_like(src_buf) for _ in range(2)]
    for k in range(2):
        dst_bufs[k].copy_(src_buf)
    beg.record(stream)
    for k in range(6):
        dst_bufs[k % 2].copy_(src_buf)
    end.record(stream)
    end.synchronize()
    copy_gbps = 6 * 2 * src_buf.numel() * 4 / (beg.elapsed_time(end) * 1e-3) / 1e9
    # torch's copy kernel is not the fastest streaming kernel on this part: an element-wise read+write kernel (add) and a
    # pure fill run well above it; both are reported so that "fraction of what the box can do" has an honest denominator
    for k in range(2):
        torch.add(src_buf, 1.0, out=dst_bufs[k])
    beg.record(stream)
    for k in range(6):
        torch.add(src_buf, 1.0, out=dst_bufs[k % 2])
    end.record(stream)
    end.synchronize()
    add_gbps = 6 * 2 * src_buf.numel() * 4 / (beg.elapsed_time(end) * 1e-3) / 1e9
    beg.record(stream)
    for k in range(6):
        dst_bufs[k % 2].fill_(1.0)
    end.record(stream)
    end.synchronize()
    fill_gbps = 6 * src_buf.numel() * 4 / (beg.elapsed_time(end) * 1e-3) / 1e9
    del src_buf, dst_bufs
    ach = b / sec / 1e9
    # HBM traffic per launch comes from rocprofv3 PMC passes (they cannot run inside this process); the committed
    # summary applies only if it was taken on exactly this batch.
    traffic, src = None, None
    try:
        with open(PMC_SUMMARY) as fh:
            pmc = json.load(fh)
        if pmc["nodes"] == n and pmc["edges_with_loops"] == e_loops and pmc["C"] == c:
            traffic, src = pmc["traffic_bytes_per_launch"], os.path.relpath(PMC_SUMMARY, ROOT) + " (FETCH_SIZE x2 + WRITE_SIZE)"
    except (OSError, KeyError, ValueError):
        pass
    out = {"bound": "hbm", "kernel": "csr_aggregate_ell_kernel<4,false,2,false,8> (the plain instantiation, timed alone; `variants` has "
                                     "every instantiation the model launches, alone and inside a train step)",
           "achieved": round(ach, 1), "peak": peak, "unit": "GB/s", "frac": round(ach / peak, 4), "traffic": traffic,
           "traffic_source": src, "bytes_per_launch": int(b), "us_per_launch": round(sec * 1e6, 2), "nodes": n,
           "edges_with_loops": e_loops, "variants": variants, "measured_copy_GBps": round(copy_gbps, 1),
           "measured_add_GBps": round(add_gbps, 1), "measured_fill_GBps": round(fill_gbps, 1),
           "note": "achieved/frac use ALGORITHMIC bytes (one source row per edge, no cache credit); hbm_GBps/hbm_frac "
                   "use the PMC-counted HBM traffic, i.e. what the memory system really moved (L2-served re-reads "
                   "excluded); frac_isolated = launches alone with rotated buffers, frac_in_step = the same launches inside an "
                   "eager single-stream train step (HIP events around each call)"}
    if in_step is not None:
        out["in_step"] = in_step
        out["in_step_all_aggregations"] = {"bytes_per_step": int(tot_b), "us_per_step": round(tot_t * 1e6, 1),
                                           "frac": round(tot_b / tot_t / 1e9 / peak, 4)}
        # The step's dominant kernel by rocprof (profiles/*_bench_kernel_stats.csv) is the POOLED epilogue instantiation
        # csr_aggregate_ell_kernel<4,false,2,true,7,true>: the last hidden aggregation of each of the three branches, whose
        # launch also reduces the per-graph means and the gate bits.  The headline record quotes THIS launch, in the step.
        dom = [v for k, v in rec.items() if k.split(" ", 1)[1].startswith("pooled ")]        # keys read "C=10 pooled epilogue ..."
        if dom:
            d_n = sum(v[2] for v in dom)
            d_b = sum(v[1] * v[2] for v in dom) / d_n
            d_t = sum(v[0] * v[2] for v in dom) / d_n * 1e-6
            out["step_dominant"] = {"kernel": "csr_aggregate_ell_kernel<4,false,2,true,7,true>", "launches_per_step": int(d_n),
                                    "bytes_per_launch": int(d_b), "us_per_launch": round(d_t * 1e6, 2),
                                    "achieved": round(d_b / d_t / 1e9, 1), "frac": round(d_b / d_t / 1e9 / peak, 4)}
            tr, tr_src = step_pmc_traffic("csr_aggregate_ell_kernel<4,false,2,true,7,true>")
            out["step_dominant"].update(traffic=tr, traffic_source=(tr_src + " (FETCH_SIZE x2 + WRITE_SIZE, mean over its launches)") if tr_src else None)
    if traffic:
        out["hbm_GBps"] = round(traffic / sec / 1e9, 1)
        out["hbm_frac"] = round(traffic / sec / 1e9 / peak, 4)
    return out


def parity_leg(model, arena, corpus, local_ids, n_qubits, n_check=10):
    """Predictions of the trained device model vs the CPU oracle carrying the same weights, on one circuit per
    Trotter step count (eval mode, fp32 oracle = the reference's CPU arithmetic, fp64 oracle = the exact value).
    tests/test_gpu_cfg4_parity.py is the asserted form of this comparison."""
    from oracle.models import FamilyA

    n_graphs = len(arena)
    sel = np.arange(n_check) * n_graphs // n_check
    host = corpus.host_graphs(local_ids[sel])
    was_training = model.training
    model.eval()
    with torch.no_grad():
        b = arena.batch(sel)
        got = model(*b.model_args()).double().cpu()
    model.train(was_training)
    state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    out = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        ref = FamilyA(n_qubits, 22, 10).eval()
        ref.load_state_dict(state)
        ref = ref.to(dt)
        want = []
        with torch.no_grad():
            for g in range(len(sel)):
                x = torch.from_numpy(host["x"][g]).to(dt)
                t = lambda k: torch.from_numpy(host[k][g:g + 1]).to(dt)
                want.append(ref(t("noisy"), t("observable"), t("depth"), x, torch.from_numpy(host["edge_index"][g]),
                                torch.zeros(x.shape[0], dtype=torch.long)).double())
        err = (got - torch.cat(want)).abs()
        out[name] = {"mae": float(err.mean()), "max": float(err.max()), "want": torch.cat(want)}
    cpu_gap = float((out["f32"]["want"] - out["f64"]["want"]).abs().max())     # the fp32 CPU path's own distance from exact
    return {"circuits": int(n_check), "tolerance": 1e-5, "criterion": "1e-5 vs fp64-exact",
            "cpu_f32_max_abs_err_vs_cpu_f64": cpu_gap, "exp_val_mae_vs_cpu_f64": out["f64"]["mae"],
            "max_abs_err_vs_cpu_f64": out["f64"]["max"], "within_tolerance_of_exact": out["f64"]["max"] < 1e-5,
            "exp_val_mae_vs_cpu_f32": out["f32"]["mae"], "max_abs_err_vs_cpu_f32": out["f32"]["max"],
            "prediction_scale": float(got.abs().mean()),
            "note": "f64 = exact value of the reference's expression; the fp32 CPU path is itself further from it than "
                    "the device on graphs of this size (asserted in tests/test_gpu_cfg4_parity.py)"}


def cpu_baseline_leg(corpus, ids, n_qubits, large_batch=256):
    """the CPU oracle (pure-torch restatement of the reference's PyG math) doing the same train
    step on the same synthetic inputs -- median of 12 steps after 3 warm-ups at the reference's batch size 32
    (__ml_models.py:105), plus a bounded large-batch sample (a prefix of the very batch the roofline leg uses)."""
    from oracle.models import FamilyA

    torch.manual_seed(0)
    model = FamilyA(n_qubits, 22, 10).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    host_cache = {}

    def graph(g):
        if g not in host_cache:
            h = corpus.host_graphs([g])
            host_cache[g] = {k: (v[0] if isinstance(v, list) else v) for k, v in h.items()}
        return host_cache[g]

    def collate(sel):
        xs, eis, bs, off = [], [], [], 0
        rows = {k: [] for k in ("noisy", "observable", "depth", "y")}
        for b, g in enumerate(sel):
            h = graph(int(g))
            x = torch.from_numpy(h["x"])
            xs.append(x)
            eis.append(torch.from_numpy(h["edge_index"]) + off)
            bs.append(torch.full((x.shape[0],), b, dtype=torch.long))
            off += x.shape[0]
            for k in rows:
                rows[k].append(torch.from_numpy(h[k]))
        t = lambda k: torch.cat(rows[k])
        return (t("noisy"), t("observable"), t("depth"), torch.cat(xs), torch.cat(eis, 1), torch.cat(bs)), t("y")

    def one_step(sel):
        t0 = time.perf_counter()
        args, y = collate(sel)
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(model(*args), y)
        loss.backward()
        opt.step()
        return time.perf_counter() - t0

    ncpu = os.cpu_count() or 1
    # torch's intra-op pool does not scale on these scatter/gather ops (measured in round 1: 256 threads is ~400x slower
    # than 8 on the GPU box's host -- a single probe step would take minutes), so "all cores" is neither the fastest setting
    # nor one this bounded leg can afford to try: probe 1/8/16/32 threads on one batch each and keep the best.
    probe = ids[:32]
    best_t, best_n = None, 1
    for nt in (1, 8, 16, 32):
        if nt > ncpu:
            continue
        torch.set_num_threads(nt)
        one_step(probe)
        dt = one_step(probe)
        if best_t is None or dt < best_t:
            best_t, best_n = dt, nt
    # SURVEY section 8d's setting, torch.set_num_threads(os.cpu_count()), printed rather than asserted: ONE bounded step on two
    # circuits (after a one-circuit warm-up) at all cores, and the same two circuits at the best setting beside it
    all_cores = None
    if ncpu > best_n:
        torch.set_num_threads(ncpu)
        one_step(ids[:1])
        t_all = one_step(ids[:2])
        torch.set_num_threads(best_n)
        one_step(ids[:2])
        t_best = one_step(ids[:2])
        all_cores = {"threads": ncpu, "circuits": 2, "ms_per_step": round(t_all * 1e3, 1), "circuits_per_s": round(2 / t_all, 2),
                     "same_step_at_best_threads_ms": round(t_best * 1e3, 1), "best_threads": best_n}
    torch.set_num_threads(best_n)
    rng = np.random.RandomState(0)
    small = [one_step(rng.choice(ids, size=32, replace=False)) for _ in range(15)][3:]      # ~6 s of CPU work
    med32 = float(np.median(small))
    big = ids[:large_batch]
    one_step(big)
    big_t = one_step(big)
    return {"value": round(32 / med32, 2), "unit": "circuits/s", "cores": best_n, "kind": "port",
            "sample": f"batch 32 (the reference's setting): median of 12 steps after 3 warm-ups, batches drawn from the "
                      f"bench's representative batch; oracle/models.py FamilyA, fp32, full train step (collate + forward "
                      f"+ MSE + backward + Adam), torch {best_n} threads = fastest of 1/8/16/32 on this {ncpu}-core host",
            "batch32_ms_per_step": round(med32 * 1e3, 1), "all_cores": all_cores,
            "large_batch": {"circuits": int(len(big)), "value": round(len(big) / big_t, 2), "ms_per_step": round(big_t * 1e3, 1),
                            "sample": f"the first {len(big)} circuits of the same representative batch as ONE step, timed once after 1 warm-up"}}


def accuracy_leg(dev):
    """The "exp-val MAE" half of the metric: Family B and MLP1 trained with the reference's loop and settings on the
    reference's own circuits (tests/golden/ising_trainval.npz; blackwater/metrics/accuracy.py states the split), validation
    MSE next to the curve the reference recorded, and the evaluation cell's MAE / RMSE / mean-L2 before and after
    mitigation.  tests/test_gpu_accuracy.py asserts the band."""
    from blackwater.data.backends import StaticBackend
    from blackwater.data.utils import get_backend_properties_v1
    from blackwater.metrics.accuracy import load_trainval, train_family_b, train_mlp1

    golden = os.path.join(ROOT, "tests", "golden")
    z = load_trainval(golden)
    props = get_backend_properties_v1(StaticBackend.from_json(os.path.join(golden, "fake_lima_backend_props.json")))
    from blackwater.metrics.accuracy import SPLIT_NOTE

    out = {"data": "reference circuits: docs/tutorials/data/ising_init_from_qasm_no_readout/{train/step_0,val/step_0..2}.pk, "
                   "pooled split (510 train / 90 validation), batch 32, Adam 1e-3, 100 epochs, seed 0",
           "split": SPLIT_NOTE}
    for key, rec in (("family_b", train_family_b(z, dev)), ("mlp1", train_mlp1(z, props, dev))):
        rep = rec["report"]
        out[key] = {"model": rec["model"], "val_mse": round(rec["val_mse_final"], 6),
                    "reference_recorded_val_mse_on_its_own_split": round(rec["reference_val_mse_final"], 6),
                    "train_mse": round(rec["train_mse_final"], 6),
                    "exp_val_mae_noisy": round(rep["MAE_noisy"], 5), "exp_val_mae_mitigated": round(rep["MAE_mitigated"], 5),
                    "rmse_noisy": round(rep["RMSE_noisy"], 5), "rmse_mitigated": round(rep["RMSE_mitigated"], 5),
                    "mean_l2_noisy": round(rep["L2_noisy"], 5), "mean_l2_mitigated": round(rep["L2_mitigated"], 5)}
    return out


def family_b_leg(dev, steps=30):
    """The reference's own model family (docs/tutorials/gnn.py:70-122: TransformerConv / ASAPooling x2, hidden 15, 4 outputs)
    as a measured workload: full train steps on cfg2 (synthetic 4-qubit TFIM-Trotter circuits, steps 0-14) at 1024
    circuits per step and at the reference's 32, plus the roofline of its dominant graph kernel, the attention forward
    (4(N+1) + 4E' + 4HC(N [q] + E' [k] + E' [v] + N [out]), E' counts the self-loop entry)."""
    from blackwater.data.arena import GraphArena
    from blackwater.data.synthetic import TfimCorpus
    from blackwater.native import ops
    from blackwater.nn import ExpValCircuitGraphModel
    from blackwater.train import Trainer

    corpus = TfimCorpus(4, list(range(15)), 70, seed=42, two_q="cx", exp_value_size=4)
    h = corpus.host_graphs()
    arena = GraphArena.from_arrays(h["x"], h["edge_index"], h["y"][:, None, :], h["noisy"][:, None, :], h["depth"], h["observable"],
                                   device=dev)
    torch.manual_seed(0)
    model = ExpValCircuitGraphModel(22, 15, 4).to(dev)
    trainer = Trainer(model, lr=1e-3)
    rng = np.random.RandomState(7)
    out = {"model": "family B: TransformerConv(22,15,h3) ASAP TransformerConv(45,15,h2) ASAP mean-pool head, 13 645 parameters",
           "workload": "cfg2: 4-qubit TFIM Trotter steps 0-14 x 70 J values (1 050 circuits, %.0f nodes per circuit)"
                       % (arena.num_nodes / len(arena))}
    for batch, n_steps in ((1024, steps), (32, 4 * steps)):
        draw = lambda: rng.randint(0, len(arena), size=batch)
        for _ in range(5):
            trainer.step(arena.batch(draw()))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_steps):
            trainer.step(arena.batch(draw()))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[f"batch{batch}"] = {"circuits_per_s": round(batch * n_steps / dt, 1), "ms_per_step": round(dt / n_steps * 1e3, 3),
                                "steps": n_steps}
    # the reference's regime (32 circuits per step) with the whole step replayed from a hipGraph: ASAPooling's shapes follow
    # the per-graph sizes, which size-stratified batches repeat, so one capture serves every batch (train.BucketedTrainer)
    from blackwater.native import ops as _ops
    from blackwater.train import BucketedTrainer, StratifiedBatches

    arena_f = GraphArena.from_arrays(h["x"], h["edge_index"], h["y"][:, None, :], h["noisy"][:, None, :], h["depth"], h["observable"],
                                     device=dev, filler_nodes=1024)
    n_f = len(arena_f)
    for bsz, variants, n_steps in ((32, (False, True), 4 * steps), (1024, (True,), steps)):
        sampler = StratifiedBatches(arena_f.node_counts[:n_f], arena_f.edge_counts[:n_f], bsz, seed=11)
        for graphs in variants:
            torch.manual_seed(0)
            bt = BucketedTrainer(ExpValCircuitGraphModel(22, 15, 4).to(dev), arena_f, lr=1e-3, graphs=graphs, node_quantum=256,
                                 edge_quantum=512)
            for _ in range(5):
                bt.step_ids(sampler.draw())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                last = bt.step_ids(sampler.draw())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out["batch%d_stratified_%s" % (bsz, "hipgraph" if graphs else "eager")] = {
                "circuits_per_s": round(bsz * n_steps / dt, 1), "ms_per_step": round(dt / n_steps * 1e3, 3), "steps": n_steps,
                "final_loss": round(float(last.item()), 6), "captures": len(bt._entries)}
            _ops.set_seed_counter(None)
            del bt
    # ... and with the reference's loader ITSELF: DataLoader(batch_size=32, shuffle=True) (docs/tutorials/__ml_models.py:105) --
    # uniformly shuffled epochs, the last short batch of an epoch dropped.  No size sequence repeats, but the size-stable buckets do
    # (train.stable_padding: a few dozen for this corpus), each captured at first sight; the timed region starts after ten epochs.
    for graphs in (False, True):
        torch.manual_seed(0)
        bt = BucketedTrainer(ExpValCircuitGraphModel(22, 15, 4).to(dev), arena_f, lr=1e-3, graphs=graphs, node_quantum=1024, edge_quantum=4096)
        rng_s = np.random.RandomState(5)

        def shuffled(n_batches):
            done = 0
            while done < n_batches:
                order = rng_s.permutation(n_f)
                for i in range(0, n_f - 31, 32):
                    if done == n_batches:
                        return
                    done += 1
                    yield order[i:i + 32]

        for ids in shuffled(320 if graphs else 10):
            bt.step_ids(ids)
        torch.cuda.synchronize()
        before = len(bt._entries)
        n_steps = 12 * steps
        t0 = time.perf_counter()
        for ids in shuffled(n_steps):
            last = bt.step_ids(ids)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out["batch32_shuffled_%s" % ("hipgraph" if graphs else "eager")] = {
            "circuits_per_s": round(32 * n_steps / dt, 1), "ms_per_step": round(dt / n_steps * 1e3, 3), "steps": n_steps,
            "final_loss": round(float(last.item()), 6), "size_stable_buckets": bool(bt.stable), "captures": len(bt._entries),
            "captures_made_inside_the_timed_region": len(bt._entries) - before, "capture_budget": bt.max_pattern_captures}
        _ops.set_seed_counter(None)
        del bt
    del arena_f
    # the same model on the headline workload's graphs (100-qubit circuits, 2-20 k nodes each): ASAPooling's coarsening takes the
    # wave-per-cluster form there (mlqem_asap_coarsen_rows_*: no sort, one host read per pooling) and is computed for the first
    # pooling only (nothing reads the second one's: GraphStructure.deferred); the coarsened graph has 27 edges per node in
    # rows of 100-500, which the attention / ASAPooling kernels walk in chunks with one lane per edge for the scalar work
    torch.cuda.reset_peak_memory_stats()
    mem_before = torch.cuda.memory_allocated()
    # 104 J values per Trotter step count: a size-stratified batch of 1024 holds 102-103 circuits of every size.  The arena is built on
    # the device from one encoded template per step count (TfimCorpus.arena), as the headline workload's
    big_corpus = TfimCorpus(100, list(range(1, 11)), 104, seed=42, exp_value_size=4)
    big_arena = big_corpus.arena(dev, filler_nodes=1024)
    nb_graphs = len(big_arena)
    cfg4 = {"nodes_per_circuit": round(big_arena.num_nodes / nb_graphs), "circuits_in_the_arena": nb_graphs,
            "coarsened_edge_capacity_per_node": round(float(big_arena.coarse_caps[:nb_graphs].sum()) / big_arena.num_nodes, 1),
            "note": "batch 64 is the point every round has reported (circuits_per_s / ms_per_step below); 256, 512 and 1024 separate what the "
                    "kernels cost per circuit from what a step costs whatever its size (VERDICT r03 item 1c)"}
    # size-stratified batches (the same number of circuits of each Trotter step count in every batch) through the bucketed trainer:
    # eager at 64, then captured at 64 / 256 / 512.  The coarsened edge arrays are sized by a structural bound
    # (GraphArena.coarse_caps), so the step reads nothing from the device and the whole of it -- assembly, two TransformerConv +
    # ASAPooling levels, head, backward, Adam -- replays from ONE graph.
    # (the 1024-circuit step runs eagerly: its structural edge bound, 2.1e9, is beyond the 2^30 entries a batch may size its edge arrays
    # to, so its coarsening reads the sizes back -- a captured step may not)
    for big_batch, graphs, big_steps in ((64, False, max(6, steps // 2)), (64, True, max(6, steps // 2)), (256, True, 10), (512, True, 8), (1024, False, 6)):
        torch.manual_seed(0)
        torch.cuda.reset_peak_memory_stats()
        sampler = StratifiedBatches(big_arena.node_counts[:nb_graphs], big_arena.edge_counts[:nb_graphs], big_batch, seed=13)
        bt = BucketedTrainer(ExpValCircuitGraphModel(22, 15, 4).to(dev), big_arena, lr=1e-3, graphs=graphs, node_quantum=1024,
                             edge_quantum=4096)
        progress(f"  family B, 100-qubit circuits: {big_batch} per step, {'captured' if graphs else 'eager'}")
        for _ in range(4 if big_batch == 64 else 2):
            bt.step_ids(sampler.draw())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(big_steps):
            last = bt.step_ids(sampler.draw())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rec = {"circuits_per_s": round(big_batch * big_steps / dt, 1), "ms_per_step": round(dt / big_steps * 1e3, 2),
               "ms_per_64_circuits": round(dt / big_steps * 1e3 * 64 / big_batch, 2), "steps": big_steps,
               "final_loss": round(float(last.item()), 6), "nodes_per_step": int(sampler.nodes_per_batch),
               "peak_mem_GB": round((torch.cuda.max_memory_allocated() - mem_before) / 1e9, 2)}
        cfg4["batch%d_%s" % (big_batch, "hipgraph" if graphs else "eager")] = rec
        _ops.set_seed_counter(None)
        del bt
        torch.cuda.empty_cache()
    cfg4["hipgraph"], cfg4["eager"] = cfg4["batch64_hipgraph"], cfg4["batch64_eager"]
    cfg4["circuits_per_s"] = cfg4["batch64_hipgraph"]["circuits_per_s"]
    cfg4["ms_per_step"] = cfg4["batch64_hipgraph"]["ms_per_step"]
    points = ("batch64_hipgraph", "batch256_hipgraph", "batch512_hipgraph", "batch1024_eager")
    cfg4["best_point"] = max(points, key=lambda k: cfg4[k]["circuits_per_s"])
    cfg4["best_circuits_per_s"] = cfg4[cfg4["best_point"]]["circuits_per_s"]
    b64 = big_arena.batch(np.arange(64) * nb_graphs // 64)
    cfg4["attention_roofline"] = attention_roofline(b64.structure, dev, "64 100-qubit circuits (the first TransformerConv's graph: the circuit DAGs)")
    cfg4["attention_roofline"]["level1"] = level1_attention_roofline(b64, dev)
    del b64
    out["cfg4_100q"] = cfg4
    out["cfg4_100q_batch64"] = {"renamed": "cfg4_100q (batch points 64 / 256 / 512 / 1024)", "circuits_per_s": cfg4["circuits_per_s"],
                                "ms_per_step": cfg4["ms_per_step"]}
    del big_arena, big_corpus
    torch.cuda.empty_cache()
    # the CPU oracle doing the same step at the reference's batch size (bounded: 6 steps, the first one untimed)
    from oracle.models import FamilyB

    torch.manual_seed(0)
    ref = FamilyB(22, 15, 4).train()
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    times = []
    for k in range(6):
        sel = rng.randint(0, len(arena), size=32)
        t0 = time.perf_counter()
        xs, eis, bs, off = [], [], [], 0
        for bi, g in enumerate(sel):
            x = torch.from_numpy(h["x"][g])
            xs.append(x)
            eis.append(torch.from_numpy(h["edge_index"][g]) + off)
            bs.append(torch.full((x.shape[0],), bi, dtype=torch.long))
            off += x.shape[0]
        opt.zero_grad()
        pred = ref(torch.from_numpy(h["noisy"][sel][:, None, :]), None, torch.from_numpy(h["depth"][sel]), torch.cat(xs),
                   torch.cat(eis, 1), torch.cat(bs))
        torch.nn.functional.mse_loss(pred, torch.from_numpy(h["y"][sel])).backward()
        opt.step()
        times.append(time.perf_counter() - t0)
    out["cpu_oracle_batch32"] = {"circuits_per_s": round(32 / float(np.median(times[1:])), 1),
                                 "sample": "oracle/models.py FamilyB, full train step, median of 5 steps of 32 circuits, torch default threads"}
    out["roofline"] = attention_roofline(arena.batch(np.arange(1024) * len(arena) // 1024).structure, dev,
                                         "1024 4-qubit circuits (0.23 M nodes: a small launch, the step spreads over ~100 of them)")
    return out


def _lib_mod():
    from blackwater.native import _lib

    return _lib


def level1_attention_roofline(batch, dev, heads=2, ch=15):
    """The SECOND TransformerConv's forward (docs/tutorials/gnn.py:86-91) on the graph ASAPooling coarsens out of ``batch`` -- where
    most of the attention time of a 100-qubit step goes (what's weak 3).  Same byte model as ``attention_roofline``
    (no cache credit); dropout keyed by (destination, head, source) as in the model's step."""
    from blackwater.native import ops
    from blackwater.nn import ExpValCircuitGraphModel

    torch.manual_seed(0)
    model = ExpValCircuitGraphModel(22, 15, 4).to(dev).train()
    with torch.no_grad():
        g = model.transformer1(batch.nodes, batch.structure)
        g, s, _ = model.pooling1(g, batch.structure)
    n = s.num_nodes
    e_cap, e = s.edge_count(), int(s.in_ptr[n].item())
    qk = []
    for _ in range(4):
        t = ops.padded_empty(n, 4 * heads * 16, dev).normal_()
        t.view(n, 4 * heads, 16)[:, :, ch:] = 0.0
        qk.append(t)
    run_edge = lambda k: ops.transformer_attention_train(qk[k % 4], s.in_ptr, s.in_src, s.loops, e_cap, heads, ch, 0.1, 1234 + k, pair_key=True, head_pitch=16)
    sec_edge = _timed_launches(run_edge, 20, 4)
    # what the step runs since round 5: the rows of 32+ entries as dense blocks on the f32 matrix cores (csrc/dense_block.hip), the other
    # rows in the per-edge kernel, one call; the plan is built once per structure and direction and shared with ASAPooling's walks
    plan = s.dense_plan("in")
    run = lambda k: ops.dense_attention_train(qk[k % 4], s.in_ptr, s.in_src, s.loops, e_cap, heads, ch, plan, drop_p=0.1, seed=1234 + k)
    sec = _timed_launches(run, 20, 4)
    stride = _lib_mod().load().mlqem_dense_plan_record_ints()
    nb = int(plan.counter.item()) // 16
    rec = plan.records[: nb * stride].view(nb, stride)[:, :4].cpu().numpy()
    usable = rec[:, 2] == 1
    cells = int((16 * ((rec[usable, 1] + 15) // 16 * 16)).sum())
    flag = plan.row_flag.bool()
    hc = heads * ch
    by_r02 = 4 * (n + 1) + 4 * e + 4 * hc * (n + e + e + n)                      # the coarsened graph has no self entries
    deg = (s.in_ptr[1:n + 1] - s.in_ptr[:n]).long()
    n_long = int((deg > 4).sum().item())
    by = 4 * (n + 1) + 4 * e + 4 * heads * 16 * (2 * n + 2 * e) + 4 * hc * (n + n_long) + 8 * n * heads
    deg_h = deg.cpu().numpy()
    flag_h = flag.cpu().numpy()
    flops = cells * heads * (2 * 16 + 2 * 16) * 1.0                               # scores and weighted values of every cell, 16 channels each
    return {"bound": "hbm by the contract's byte model (no cache credit: a key / value row is counted once per ENTRY, the block kernel reads it "
                     "once per 16 rows, so the figure exceeds 1); the per-edge kernel alone is bound by vector instructions (0.69 of the SIMD "
                     "cycles busy, profiles/r05_level1_pmc.json), the block kernel by the latency of its gathers",
            "kernel": f"dense_attn_fwd_kernel<2> + transformer_attn_train_q4_kernel<4> over the rows outside the blocks (H={heads}, C={ch}, head "
                      "pitch 16, pair-keyed dropout 0.1)",
            "workload": "the graph ASAPooling makes of 64 100-qubit circuits", "achieved": round(by / sec / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
            "frac": round(by / sec / 1e9 / 8000.0, 4), "frac_r02_model": round(by_r02 / sec / 1e9 / 8000.0, 4), "traffic": None,
            "bytes_per_launch": int(by), "us_per_launch": round(sec * 1e6, 2), "nodes": n, "edges": e, "mean_row_length": round(e / max(n, 1), 1),
            "per_edge_kernel_alone": {"us_per_launch": round(sec_edge * 1e6, 2), "frac": round(by / sec_edge / 1e9 / 8000.0, 4),
                                      "note": "every row in transformer_attn_train_q4_kernel<4>: the r04 form of this launch"},
            "dense_blocks": {"blocks": nb, "usable": int(usable.sum()), "rows_in_blocks": int(flag_h.sum()),
                             "share_of_the_entries": round(float(deg_h[flag_h].sum()) / max(float(deg_h.sum()), 1.0), 4),
                             "cells": cells, "cells_per_entry": round(cells / max(float(deg_h[flag_h].sum()), 1.0), 3),
                             "mfma_flops_per_launch": int(flops),
                             "note": "16 rows x the union of their sources per block; scores and weighted values on v_mfma_f32_16x16x4_f32 "
                                     "(157.3 TFLOP/s dense f32 peak: the products are a few percent of it, the kernel waits on its gathers)"}}


def attention_roofline(s, dev, what, heads=3, ch=15):
    """TransformerConv's training forward (mlqem_transformer_attention_train_f32) on the structure ``s``, timed alone: algorithmic
    bytes = index arrays + the [N, 4 H C] projections read once per row (query, skip) and once per entry (key, value; entries =
    in-edges + the self-loop entry) + the [N, H C] output, attn_out for the rows the backward needs it of (more than four entries) +
    the two [N, H] softmax statistics + the ELL side table, over the average launch time.  (Until round 3 the model left out the skip read, attn_out and the
    statistics: ``frac_r02_model`` keeps that figure for comparison.)"""
    from blackwater.native import ops

    import blackwater.native.functional as Fn

    n, e = s.num_nodes, s.num_edges
    hc = heads * ch
    # the layout the model's step hands over (functional._TransformerConv): a head's channels at a pitch of 16 floats, pads zero
    cp = Fn._ATTN_PITCH if (Fn._ATTN_PITCH > ch and Fn._ATTN_PITCH - ch < 4) else 0
    pitch = cp or ch
    qk = []
    for _ in range(4):
        t = ops.padded_empty(n, 4 * heads * pitch, dev).normal_()
        if cp:
            t.view(n, 4 * heads, pitch)[:, :, ch:] = 0.0
        qk.append(t)
    ell = s.in_ell
    run = lambda k: ops.transformer_attention_train(qk[k % 4], s.in_ptr, s.in_src, s.loops, e, heads, ch, 0.1, 1234 + k, ell=ell, head_pitch=cp)
    for k in range(4):
        run(k)
    stream = torch.cuda.current_stream()
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record(stream)
    for k in range(20):
        run(k)
    end.record(stream)
    end.synchronize()
    sec = beg.elapsed_time(end) * 1e-3 / 20
    e1 = e + n
    by_r02 = 4 * (n + 1) + 4 * e1 + 4 * hc * (n + e1 + e1 + n)
    # attn_out is written for rows of more than four entries only (round 4: the backward forms g . attn_out of a shorter row itself)
    deg = (s.in_ptr[1:n + 1] - s.in_ptr[:n]).long() + (s.loops[:n] > 0).long()
    n_long = int((deg > 4).sum().item())
    hp = heads * pitch                               # columns of a part as stored (pads included: they are moved)
    by = 4 * (n + 1) + 8 * n + 4 * e1 + 4 * hp * (2 * n + 2 * e1) + 4 * hc * (n + n_long) + 8 * n * heads
    return {"bound": "hbm", "kernel": f"transformer_attn_train_q4_kernel<4> (H={heads}, C={ch}, head pitch {pitch}, attention dropout 0.1)", "workload": what,
            "achieved": round(by / sec / 1e9, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(by / sec / 1e9 / 8000.0, 4),
            "frac_r02_model": round(by_r02 / sec / 1e9 / 8000.0, 4),
            "traffic": None, "bytes_per_launch": int(by), "us_per_launch": round(sec * 1e6, 2), "nodes": n, "edges_with_loops": e1,
            "note": "four channels per lane (csrc/attn_q4.hpp): a (row, head) is 4 lanes, a key / value segment one 16-byte load, entries "
                    "four at a time with one lane per entry for the scalar work; the one-channel-per-lane form it replaces was bound by "
                    "instruction issue (0.29 of the HBM peak on the 100-qubit circuit DAGs)"}


def replicated_arena(enc, copies, dev, filler_nodes=0, scalar_labels=False, seed=0):
    """A device-resident arena of ``copies[t]`` copies of every encoded template graph ``t`` (``synthetic.encode_corpus``): distinct
    circuit STRUCTURES are encoded once on the host and replicated by torch ops on the GPU (labels random per copy), the way
    ``TfimCorpus.arena`` builds the headline corpus.  Returns (arena, template index of every circuit)."""
    from blackwater.data.arena import GraphArena

    copies = np.asarray(copies, dtype=np.int64)
    sizes = np.array([x.shape[0] for x in enc["x"]])
    f = enc["x"][0].shape[1]
    f4 = (f + 3) // 4 * 4
    n_total = int((sizes * copies).sum())
    x = torch.zeros((n_total, f4), dtype=torch.float32, device=dev)
    eis, base, tmpl_of = [], 0, []
    for t, (xt, et, c) in enumerate(zip(enc["x"], enc["edge_index"], copies)):
        n_t, c = xt.shape[0], int(c)
        x[base:base + c * n_t].view(c, n_t, f4)[:, :, :f] = torch.from_numpy(xt).to(dev).unsqueeze(0)
        offs = base + torch.arange(c, device=dev, dtype=torch.int64) * n_t
        eis.append((torch.from_numpy(et).to(dev).unsqueeze(1) + offs.view(1, c, 1)).reshape(2, -1))
        base += c * n_t
        tmpl_of.append(np.full(c, t))
    tmpl_of = np.concatenate(tmpl_of)
    g = len(tmpl_of)
    rng = np.random.default_rng(seed)
    width = 1 if scalar_labels else enc["y"].shape[-1]
    y = rng.uniform(-1, 1, size=(g, width) if scalar_labels else (g, 1, width)).astype(np.float32)
    noisy = (y * 0.9 + rng.normal(0, 0.01, size=y.shape)).astype(np.float32)
    arena = GraphArena.from_device(x[:, :f], sizes[tmpl_of], torch.cat(eis, dim=1), y, noisy, enc["depth"][tmpl_of], enc["observable"][tmpl_of],
                                   filler_nodes=filler_nodes)
    return arena, tmpl_of


def _timed_steps(run, warm, steps):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        last = run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps, last


def _agg_frac(arena, ids, n_qubits):
    """Byte-weighted fraction of the 8 TB/s HBM peak over every CSR aggregation launch of a Family A step on this batch."""
    rows = in_step_aggregation_times(arena, ids, n_qubits, steps=2)
    us = sum(v[0] * v[2] for v in rows.values())
    by = sum(v[1] * v[2] for v in rows.values())
    return {"frac": round(by / us / 1e3 / 8000.0, 4), "GBps": round(by / us / 1e3, 1), "launches_per_step": int(sum(v[2] for v in rows.values())),
            "bytes_per_step": int(by), "us_per_step": round(us, 1)}


def configs_leg(dev):
    """BASELINE.json's configs that the other legs do not time: cfg1 (MLP on the 169-wide circuit features of 3 000
    4-qubit circuits: the demo2 sizes), cfg3 (random 20-qubit depth-40 circuits, 100 k circuits on one GPU; Family A and Family B train
    steps) and cfg5 (one rank's 1/64 cut of the 1 M-circuit mixed corpus: 50 % 4-qubit TFIM, 30 % random 20-qubit, 20 % Pauli-twirled
    100-qubit TFIM; Family A in fp32 and Family B with the MLP3 head on the bf16 matrix cores).  Every graph leg: circuits/s, ms per
    step, and the byte-weighted fraction of the HBM peak over its aggregation (Family A) or first-level attention (Family B) launches,
    by the algorithmic bytes of SURVEY section 8(d)."""
    from blackwater.data.synthetic import encode_corpus, pauli_twirl, random_circuit, tfim_circuit
    from blackwater.native import ops
    from blackwater.nn import MLP1, ExpValCircuitGraphModel, ExpValCircuitGraphModel_3, ExpValCircuitGraphModelA
    from blackwater.train import BucketedTrainer, RowsTrainer, StratifiedBatches, Trainer

    out = {}
    # ---- cfg1: MLP1(169, 64, 1) on 3 000 feature rows (500 train / 2 500 test in demo2), one captured step per batch of 500
    torch.manual_seed(0)
    rows = torch.randn(3000, 169, device=dev)
    target = torch.randn(3000, 1, device=dev)
    tr = RowsTrainer(MLP1(169, 64, 1).to(dev), lr=1e-3)
    sel = [torch.arange(k * 500, (k + 1) * 500, device=dev) for k in range(6)]
    k = [0]

    def mlp_step():
        i = sel[k[0] % 6]
        k[0] += 1
        return tr.step_rows(rows[i], target[i])

    sec, loss = _timed_steps(mlp_step, 20, 200)
    out["cfg1_mlp1_169"] = {"workload": "cfg1: MLP1(169, 64, 1) train step on 500 of 3 000 feature rows (encode_data_v2_ecr width for two_q = 'cx')",
                            "circuits_per_s": round(500 / sec, 1), "ms_per_step": round(sec * 1e3, 4), "final_loss": round(float(loss.item()), 6),
                            "note": "launch-bound (a 500-row step is ~10 launches); the throughput shape of the same kernels is the mlp_head leg"}
    del tr
    # ---- cfg3: random 20-qubit depth-40 circuits
    progress("  cfg3: random 20-qubit depth-40 circuits")
    tmpl = [random_circuit(20, 40, seed=s, two_q="cx") for s in range(16)]
    cfg3 = {"workload": "cfg3: 100 000 random 20-qubit depth-40 circuits (16 distinct structures, replicated on the device)"}
    enc = encode_corpus(tmpl, 20, two_q="cx", exp_value_size=1)
    arena, _ = replicated_arena(enc, np.full(16, 6250), dev, filler_nodes=1024, scalar_labels=True)
    g = len(arena) - 1
    cfg3["nodes_per_circuit"] = round((arena.num_nodes - 1024) / g, 1)
    sampler = StratifiedBatches(arena.node_counts[:g], arena.edge_counts[:g], 4096, seed=5)
    torch.manual_seed(0)
    bt = BucketedTrainer(ExpValCircuitGraphModelA(20, 22, 10).to(dev), arena, lr=1e-3, graphs=True, node_quantum=1024)
    sec, loss = _timed_steps(lambda: bt.step_ids(sampler.draw()), 3, 20)
    cfg3["family_a"] = {"circuits_per_step": 4096, "circuits_per_s": round(4096 / sec, 1), "ms_per_step": round(sec * 1e3, 3),
                        "nodes_per_step": int(sampler.nodes_per_batch), "step_mode": "hipgraph replay", "final_loss": round(float(loss.item()), 6)}
    ops.set_seed_counter(None)
    del bt
    cfg3["family_a"]["aggregation_roofline"] = _agg_frac(arena, sampler.draw(), 20)
    del arena
    torch.cuda.empty_cache()
    enc4 = encode_corpus(tmpl, 20, two_q="cx", exp_value_size=4)
    arena, _ = replicated_arena(enc4, np.full(16, 1024), dev, filler_nodes=1024)
    g = len(arena) - 1
    sampler = StratifiedBatches(arena.node_counts[:g], arena.edge_counts[:g], 1024, seed=5)
    torch.manual_seed(0)
    bt = BucketedTrainer(ExpValCircuitGraphModel(22, 15, 4).to(dev), arena, lr=1e-3, graphs=True, node_quantum=1024, edge_quantum=4096)
    sec, loss = _timed_steps(lambda: bt.step_ids(sampler.draw()), 3, 10)
    cfg3["family_b"] = {"circuits_per_step": 1024, "circuits_per_s": round(1024 / sec, 1), "ms_per_step": round(sec * 1e3, 3),
                        "nodes_per_step": int(sampler.nodes_per_batch), "step_mode": "hipgraph replay", "final_loss": round(float(loss.item()), 6)}
    ops.set_seed_counter(None)
    del bt
    cfg3["family_b"]["attention_roofline"] = attention_roofline(arena.batch(sampler.draw()).structure, dev, "1024 random 20-qubit circuits (level 0)")
    del arena
    torch.cuda.empty_cache()
    out["cfg3_random_20q"] = cfg3
    # ---- cfg5: the mixed corpus, 1/64 of one rank's shard (15 625 circuits)
    progress("  cfg5: mixed corpus")
    total = 15_625
    n2, n3 = total // 2, total * 3 // 10
    n4 = total - n2 - n3
    small = [tfim_circuit(4, st, J=0.3 + 0.01 * st, two_q="cx") for st in range(15)]
    rand = [random_circuit(20, 40, seed=s, two_q="cx") for s in range(12)]
    twirled = [pauli_twirl(tfim_circuit(100, st, J=0.5, two_q="cx"), seed=100 + st, two_q=("cx",)) for st in range(1, 11)]
    enc5 = encode_corpus(small + rand + twirled, 100, two_q="cx", exp_value_size=4)
    copies = np.concatenate([np.full(15, -(-n2 // 15)), np.full(12, -(-n3 // 12)), np.full(10, -(-n4 // 10))])
    cfg5 = {"workload": "cfg5: %d circuits = 1/64 of one rank's shard of the 1 M-circuit mixed corpus (50 %% 4-qubit TFIM, 30 %% random 20-qubit "
                        "depth-40, 20 %% Pauli-twirled 100-qubit TFIM), device-resident" % int(copies.sum())}
    rs = np.random.RandomState(0)
    # (eager steps on random draws of the mix: host-bound, so 30 timed steps after 4 -- ten after two swung 440-720 k box to box)
    for name, make, batch, steps, scalar in (("family_a_f32", lambda: ExpValCircuitGraphModelA(100, 22, 10), 1024, 30, True),
                                             ("family_b_mlp3_head_bf16", lambda: ExpValCircuitGraphModel_3(22, 15, 4), 64, 30, False)):
        arena, _ = replicated_arena(enc5, copies, dev, scalar_labels=scalar)
        g = len(arena)
        cfg5.setdefault("nodes", int(arena.num_nodes))
        torch.manual_seed(0)
        model = make().to(dev)
        if not scalar:
            model.body_seq.mfma = "bf16"
        tr = Trainer(model, lr=1e-3)
        draw = lambda: rs.randint(0, g, size=batch)
        sec, loss = _timed_steps(lambda: tr.step(arena.batch(draw())), 4, steps)
        rec = {"circuits_per_step": batch, "circuits_per_s": round(batch / sec, 1), "ms_per_step": round(sec * 1e3, 3), "step_mode": "eager",
               "final_loss": round(float(loss.item()), 6)}
        del tr, model
        ids = draw()
        rec["nodes_in_the_roofline_batch"] = int(arena.node_counts[ids].sum())
        if scalar:
            rec["aggregation_roofline"] = _agg_frac(arena, ids, 100)
        else:
            rec["attention_roofline"] = attention_roofline(arena.batch(ids).structure, dev, "64 circuits of the mixed corpus (level 0)")
        cfg5[name] = rec
        del arena
        torch.cuda.empty_cache()
    out["cfg5_mixed"] = cfg5
    return out


def mlp_head_leg(dev, rows=262144, steps=50):
    """The MLP path of BASELINE.json's configs[0] / configs[4] (docs/tutorials/mlp.py:18-108; demo2's 169/170-wide
    `encode_data_v2_ecr` rows): MLP1(170, 128, 1) and MLP3(170, 125, 1) train steps (forward, MSE, backward, Adam) on `rows`
    synthetic feature rows, in fp32 (exact, v_mfma_f32_16x16x4_f32) and with `mfma = "bf16"` -- the "bf16 MFMA MLP head" of
    cfg5: v_mfma_f32_16x16x32_bf16, hidden activations kept as a bf16 stash.  The step is replayed from a hipGraph
    (train.RowsTrainer; `eager_ms_per_step` = the same step enqueued launch by launch).  GEMM model: a layer moves
    rows (in e_in + out e_out) + 4 in out bytes (e = the operand's STORAGE type: fp32 feature rows and outputs, fp32 or bf16
    hidden activations) and does 2 rows in out flops per pass; passes = forward + weight gradient + data gradient, except
    that the FIRST layer has no data gradient (the feature matrix needs none); the element-wise passes of MLP3 (BatchNorm,
    ReLU, dropout) are NOT in the model, so its fractions describe the whole step against its GEMM bytes only.  `kernels` times the two
    launches of the one-launch MLP1 head alone (HIP events on the launch stream) against their own bytes and flops."""
    from blackwater.native import ops as _ops
    from blackwater.nn.mlp import MLP1, MLP3
    from blackwater.train import RowsTrainer

    torch.manual_seed(0)
    x = _ops.padded_copy(torch.randn(rows, 170, device=dev))      # rows in the padded layout (16-byte aligned), as the arena's
    y = torch.randn(rows, 1, device=dev)
    out = {"rows_per_step": rows, "features": 170,
           "peaks": {"hbm_GBps": 8000.0, "mfma_f32_TFLOPs": 157.0, "mfma_bf16_TFLOPs": 2500.0}}

    def timed(fn, reps=20):
        for _ in range(3):
            fn()
        st = torch.cuda.current_stream()
        beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        beg.record(st)
        for _ in range(reps):
            fn()
        end.record(st)
        end.synchronize()
        return beg.elapsed_time(end) * 1e-3 / reps

    # the two launches of the fused MLP1 head, alone
    w1, b1 = torch.randn(128, 170, device=dev) / 13.0, torch.randn(128, device=dev)
    w2, b2 = torch.randn(1, 128, device=dev) / 11.0, torch.randn(1, device=dev)
    gout = torch.randn(rows, 1, device=dev)
    kern = {}
    for mode in ("f32", "bf16"):
        bf = mode == "bf16"
        _, hs, xp = _ops.mlp1_forward(x, w1, b1, w2, b2, bf16=bf)
        tf = timed(lambda: _ops.mlp1_forward(x, w1, b1, w2, b2, bf16=bf))
        tb = timed(lambda: _ops.mlp1_backward(gout, xp, hs, w2, 170, 128, bf16=bf))
        by = rows * (4 * 172 + (2 if bf else 4) * 128 + 4)        # x row + stash row + output / gout, per direction
        fl = 2 * rows * 170 * 128
        peak = 2500.0 if bf else 157.0
        kern[mode] = {"forward_us": round(tf * 1e6, 1), "backward_us": round(tb * 1e6, 1), "bytes_per_launch": by,
                      "forward_frac_hbm": round(by / tf / 8e12, 3), "backward_frac_hbm": round(by / tb / 8e12, 3),
                      "forward_frac_mfma": round(fl / tf / 1e12 / peak, 3), "backward_frac_mfma": round(fl / tb / 1e12 / peak, 3)}
        del hs, xp
    out["mlp1_head_kernels"] = kern
    for name, make, widths in (("mlp1_170_128_1", lambda: MLP1(170, 128, 1), [(170, 128), (128, 1)]),
                               ("mlp3_170_125_1", lambda: MLP3(170, 125, 1), [(170, 125), (125, 125), (125, 41), (41, 1)])):
        passes = [2] + [3] * (len(widths) - 1)       # no data gradient for the first layer
        gemm_flops = sum(p * 2 * rows * i * o for p, (i, o) in zip(passes, widths))

        def gemm_bytes_of(mode):
            """Bytes the GEMM passes must move with every tensor in the type it is STORED in: the feature rows and the final
            output fp32, hidden activations fp32 or -- mode bf16 -- bfloat16, weights fp32.  MLP1 is one launch per direction,
            so its hidden activation crosses memory twice (stash written, stash read), not once per layer pass."""
            elem = 2 if mode == "bf16" else 4
            if name.startswith("mlp1"):
                return 2 * rows * (4 * 172 + elem * 128 + 4)
            total = 0
            for li, (p_, (i, o)) in enumerate(zip(passes, widths)):
                ei, eo = (4 if li == 0 else elem), (4 if li == len(widths) - 1 else elem)
                total += p_ * (rows * (i * ei + o * eo) + 4 * i * o)
            return total

        for mode in ("f32", "bf16"):
            gemm_bytes = gemm_bytes_of(mode)
            rec = {}
            for graphs in (True, False):
                torch.manual_seed(1)
                model = make().to(dev)
                model.mfma = mode
                tr = RowsTrainer(model, lr=1e-3, graphs=graphs)
                for _ in range(3):
                    tr.step_rows(x, y)
                # the rows are resident in HBM when the timed region starts: in graph mode, in the graph's own input buffers
                xs, ys = tr.input_buffers(x.shape, y.shape) if graphs else (x, y)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    loss = tr.step_rows(xs, ys)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / steps
                if graphs:
                    rec = {"rows_per_s": round(rows / dt, 0), "ms_per_step": round(dt * 1e3, 3), "step_mode": "hipgraph replay",
                           "gemm_bytes_per_step": gemm_bytes,
                           "gemm_GBps_algorithmic": round(gemm_bytes / dt / 1e9, 1), "gemm_TFLOPs": round(gemm_flops / dt / 1e12, 3),
                           "frac_of_hbm_peak": round(gemm_bytes / dt / 1e9 / 8000.0, 4),
                           "frac_of_mfma_peak": round(gemm_flops / dt / 1e12 / (157.0 if mode == "f32" else 2500.0), 5),
                           "final_loss": round(float(loss.item()), 6)}
                else:
                    rec["eager_ms_per_step"] = round(dt * 1e3, 3)
                    rec["eager_final_loss"] = round(float(loss.item()), 6)
                _ops.set_seed_counter(None)
                del tr, model
            out[f"{name}_{mode}"] = rec
    return out


def inference_leg(dev):
    """The "inference" half of the path: the estimator decorators' post-processing (the reference's VQE inner loop calls it
    once per energy evaluation: blackwater/library/ngem/estimator.py:49-84, learning/estimator.py:220-245), from OpenQASM text
    to mitigated values.  `batched` = native C++ encoder + ONE collate + ONE device call per run();
    `serial` = the reference's shape, one encode (the C++ encoder since round 4) and one model call per circuit; `cpu_oracle` = the CPU restatement's
    per-circuit loop on the same circuits (bounded samples, sizes stated).  Synthetic TFIM-Trotter circuits, 4 and 100 qubits."""
    from blackwater.data.backends import PauliObservable
    from blackwater.data.circuit import circuit_to_qasm
    from blackwater.data.synthetic import synthetic_backend, tfim_circuit
    from blackwater.data.utils import get_backend_properties_v1
    from blackwater.library.learning.estimator import TorchLearningModelProcessor, learning
    from blackwater.library.ngem.estimator import ngem
    from blackwater.nn import ExpValCircuitGraphModel, ExpValCircuitGraphModelA
    from blackwater.nn.mlp import MLP1
    from oracle.models import FamilyA, FamilyB

    class _Result:
        def __init__(self, values):
            self.values, self.metadata = np.asarray(values, dtype=float), [{} for _ in values]

    class _Job:
        def __init__(self, values):
            self._values = values

        def result(self):
            return _Result(self._values)

        def job_id(self):
            return "bench"

        def status(self):
            return "DONE"

    class Est:       # stand-in for a qiskit BaseEstimator (no simulator in the loop: the post-processing is what is timed)
        def run(self, circuits, observables, parameter_values=None, **opts):
            return self._run(circuits, observables, parameter_values or [()] * len(circuits), **opts)

        def _run(self, circuits, observables, parameter_values, **opts):
            return _Job([0.1 + 0.001 * (k % 97) for k in range(len(circuits))])

    class ScalarNoisy(torch.nn.Module):
        """The decorator hands a model ``exp_value`` as [B, 1] (ngem/estimator.py:68-82); Family B squeezes a [B, 1, k] tensor
        (gnn.py:116): the one-output variant takes the decorator's value with one more axis."""

        def __init__(self, inner):
            super().__init__()
            self.inner = inner

        def forward(self, exp_value, observable, circuit_depth, nodes, edge_index, batch):
            return self.inner(exp_value.unsqueeze(-1), observable, circuit_depth, nodes, edge_index, batch)

    def wall(fn, runs=3):
        """Median wall time of `runs` calls (the box's CPU share is throttled after a burst -- the 64-thread scan, the oracle's
        torch threads -- so a single call is either side of a 2x step)."""
        times = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return sorted(times)[len(times) // 2], out

    out = {"note": "circuits/s from OpenQASM text to mitigated values; the median of three run() calls after one warm-up run"}
    rng = np.random.RandomState(3)
    for nq, two_q, steps_list, n_distinct in ((4, "cx", list(range(15)), 60), (100, "ecr", list(range(1, 11)), 20)):
        backend = synthetic_backend(nq, two_q)
        texts = [circuit_to_qasm(tfim_circuit(nq, steps_list[k % len(steps_list)], float(rng.uniform(0, 2.0)), two_q=two_q))
                 for k in range(n_distinct)]
        obs1 = PauliObservable("I" * (nq - 1) + "Z")
        torch.manual_seed(0)
        fam_a = ExpValCircuitGraphModelA(nq, 22, 10).to(dev).eval()
        fam_b = ScalarNoisy(ExpValCircuitGraphModel(22, 15, 1)).to(dev).eval()
        rec = {"distinct_circuits": n_distinct, "mean_ops_per_circuit": round(float(np.mean([t.count(";") for t in texts])), 0)}
        for name, model in (("family_a", fam_a), ("family_b", fam_b)):
            r = {}
            est_b = ngem(Est, model, backend, batched=True)()
            for count in (64, 1024):
                progress(f"  inference {nq}q {name}: batched run of {count}")
                qs = [texts[k % n_distinct] for k in range(count)]
                ob = [obs1] * count
                est_b.run(qs, ob).result()        # warm-up at the same size: pinned staging buffers, encoder scratch, allocator
                dt, vals = wall(lambda: est_b.run(qs, ob).result().values)
                r[f"batched_{count}_texts_repeated_as_buffers"] = {"circuits_per_s": round(count / dt, 1), "ms_per_run": round(dt * 1e3, 2),
                                                                   "distinct_buffers_scanned": min(count, n_distinct)}
                if count == 1024:
                    # the run() above names each of the distinct texts many times AS THE SAME BUFFER (what the reference's VQE drivers do:
                    # one bound circuit, one pair per Pauli term) and such a text is scanned once; the same run() with every text its
                    # own buffer -- 1024 circuits the scanner has to read in full -- is the other end
                    qs_own = [(t + " ")[:-1] for t in qs]
                    est_b.run(qs_own, ob).result()
                    dt, _ = wall(lambda: est_b.run(qs_own, ob).result().values)
                    # THE figure of this leg: every circuit of the run() scanned
                    r["batched_1024"] = {"circuits_per_s": round(count / dt, 1), "ms_per_run": round(dt * 1e3, 2),
                                         "note": "every text its own buffer: 1024 texts scanned in full"}
                    del qs_own
            n_serial = 32 if nq == 4 else 16      # the serial loop encodes natively since round 4: a 100-qubit circuit is milliseconds
            est_s = ngem(Est, model, backend)()
            progress(f"  inference {nq}q {name}: serial run of {n_serial}")
            qs, ob = [texts[k % n_distinct] for k in range(n_serial)], [obs1] * n_serial
            est_s.run(qs[:2], ob[:2]).result()
            dt, vals_s = wall(lambda: est_s.run(qs, ob).result().values)
            r["serial"] = {"circuits": n_serial, "circuits_per_s": round(n_serial / dt, 1), "ms_per_circuit": round(dt / n_serial * 1e3, 2)}
            vals_b = est_b.run(qs, ob).result().values
            r["max_abs_batched_minus_serial"] = float(np.abs(np.asarray(vals_b) - np.asarray(vals_s)).max())
            # the CPU oracle's per-circuit loop (the reference's arithmetic on the host), same circuits, bounded
            state = {k: v.detach().cpu() for k, v in model.state_dict().items()}
            ref = (FamilyA(nq, 22, 10) if name == "family_a" else ScalarNoisy(FamilyB(22, 15, 1))).eval()
            ref.load_state_dict(state)
            est_c = ngem(Est, ref, backend)()
            n_cpu = 8 if nq == 4 else (2 if name == "family_a" else 1)     # the oracle's ASAPooling on a 100-qubit graph: ~20 s a circuit
            progress(f"  inference {nq}q {name}: CPU oracle on {n_cpu}")
            qs, ob = qs[:n_cpu], ob[:n_cpu]
            t0 = time.perf_counter()
            vals_c = est_c.run(qs, ob).result().values
            dt = time.perf_counter() - t0
            r["cpu_oracle_serial"] = {"circuits": n_cpu, "circuits_per_s": round(n_cpu / dt, 2), "ms_per_circuit": round(dt / n_cpu * 1e3, 1)}
            r["max_abs_device_minus_cpu_oracle_f32"] = float(np.abs(np.asarray(vals_s[:n_cpu]) - np.asarray(vals_c)).max())
            # like for like: the device's serial loop on exactly the circuits the oracle just ran (the circuits of a run() grow in size)
            dt_same, _ = wall(lambda: est_s.run(qs, ob).result().values)
            r["serial_on_the_oracles_circuits"] = {"circuits": n_cpu, "circuits_per_s": round(n_cpu / dt_same, 1),
                                                   "ms_per_circuit": round(dt_same / n_cpu * 1e3, 2)}
            rec[name] = r
            del est_b, est_s, est_c
        # the MLP path: TorchLearningModelProcessor.process_batch (one feature matrix, one device call) vs process per circuit
        props = get_backend_properties_v1(backend)
        n_gates = len(props["gates_set"])
        torch.manual_seed(0)
        mlp = MLP1(8 + n_gates + 40 + 1 + (4 * nq + 1), 64, 1).to(dev).eval()
        proc = TorchLearningModelProcessor(mlp, backend)
        est_l = learning(Est, proc, skip_transpile=True)()
        r = {}
        for count in (64, 1024):
            progress(f"  inference {nq}q learning: process_batch of {count}")
            qs, ob = [texts[k % n_distinct] for k in range(count)], [obs1] * count
            est_l.run(qs, ob).result()
            dt, _ = wall(lambda: est_l.run(qs, ob).result().values)
            r[f"process_batch_{count}"] = {"circuits_per_s": round(count / dt, 1), "ms_per_run": round(dt * 1e3, 2)}
        n_serial = 32 if nq == 4 else 8
        qs = [texts[k % n_distinct] for k in range(n_serial)]
        t0 = time.perf_counter()
        for k, q in enumerate(qs):
            proc.process(0.1, q, obs1, ())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        r["process_serial"] = {"circuits": n_serial, "circuits_per_s": round(n_serial / dt, 1), "ms_per_circuit": round(dt / n_serial * 1e3, 2)}
        rec["learning_mlp1"] = r
        out[f"tfim_{nq}q"] = rec
        del fam_a, fam_b, mlp
    return out


def small_batch_leg(dev, steps=300):
    """The reference's batch size (32, docs/tutorials/__ml_models.py:105) on cfg2 (4-qubit TFIM circuits, Family A): the
    step is ~8 k graph nodes, i.e. launch-bound.  ``eager`` = the ordinary Trainer (one Python-enqueued launch sequence per
    step); ``hipgraph`` = BucketedTrainer: the whole step captured per size bucket and replayed with one launch."""
    from blackwater.data.synthetic import TfimCorpus
    from blackwater.native import ops
    from blackwater.nn import ExpValCircuitGraphModelA
    from blackwater.train import BucketedTrainer, Trainer

    corpus = TfimCorpus(4, list(range(15)), 70, seed=42, two_q="cx", exp_value_size=1)
    arena = corpus.arena(dev, filler_nodes=4096)
    rng = np.random.RandomState(11)
    plans = [rng.choice(len(arena), size=32, replace=False) for _ in range(steps + 200)]
    out = {"workload": "cfg2: 4-qubit TFIM Trotter steps 0-14 x 70 J values, family A, 32 circuits per step "
                       "(%.0f nodes per circuit)" % (arena.num_nodes / len(arena))}
    for mode in ("eager", "hipgraph"):
        torch.manual_seed(0)
        model = ExpValCircuitGraphModelA(4, 22, 10).to(dev)
        if mode == "eager":
            ops.set_seed_counter(None)
            tr = Trainer(model, lr=1e-3)
            run = lambda ids: tr.step(arena.batch(ids))
        else:
            tr = BucketedTrainer(model, arena, lr=1e-3, graphs=True, node_quantum=1024, edge_quantum=4096)
            run = tr.step_ids
        for ids in plans[:200]:          # allocator growth / every bucket captured
            run(ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for ids in plans[200:]:
            loss = run(ids)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[mode] = {"circuits_per_s": round(32 * steps / dt, 1), "ms_per_step": round(dt / steps * 1e3, 4),
                     "final_loss": round(float(loss.item()), 6)}
        if mode == "hipgraph":
            out[mode]["buckets_captured"] = len(tr._entries)
    ops.set_seed_counter(None)
    out["speedup"] = round(out["hipgraph"]["circuits_per_s"] / out["eager"]["circuits_per_s"], 2)
    return out


HEADLINE_MAX_BYTES = 8192     # the driver keeps ~11 KB of stdout tail; the r05 line (22.8 KB) came back unparsed
FULL_RECORD = os.environ.get("MLQEM_BENCH_FULL_RECORD", os.path.join("gpurun_out", "bench_full.json"))

# one scalar per BASELINE.json config: (key in the headline record, path into the full record)
FLAT_KEYS = {"cfg1_mlp1_169_circuits_per_s": ("configs", "cfg1_mlp1_169", "circuits_per_s"),
             "cfg2_family_a_batch32_circuits_per_s": ("small_batch", "hipgraph", "circuits_per_s"),
             "cfg2_family_b_batch32_circuits_per_s": ("family_b", "batch32_stratified_hipgraph", "circuits_per_s"),
             "cfg2_family_b_batch32_shuffled_circuits_per_s": ("family_b", "batch32_shuffled_hipgraph", "circuits_per_s"),
             "cfg3_family_a_circuits_per_s": ("configs", "cfg3_random_20q", "family_a", "circuits_per_s"),
             "cfg3_family_b_circuits_per_s": ("configs", "cfg3_random_20q", "family_b", "circuits_per_s"),
             "cfg4_family_b_best_circuits_per_s": ("family_b", "cfg4_100q", "best_circuits_per_s"),
             "cfg4_family_b_batch64_ms_per_step": ("family_b", "cfg4_100q", "ms_per_step"),
             "cfg5_family_a_circuits_per_s": ("configs", "cfg5_mixed", "family_a_f32", "circuits_per_s"),
             "cfg5_family_b_bf16_head_circuits_per_s": ("configs", "cfg5_mixed", "family_b_mlp3_head_bf16", "circuits_per_s"),
             "mlp3_head_f32_ms_per_step": ("mlp_head", "mlp3_170_125_1_f32", "ms_per_step"),
             "mlp3_head_bf16_ms_per_step": ("mlp_head", "mlp3_170_125_1_bf16", "ms_per_step")}


def _dig(node, path):
    for part in path:
        node = node.get(part) if isinstance(node, dict) else None
    return node


def _short(text, n):
    text = str(text)
    return text if len(text) <= n else text[:n - 1] + "~"


def headline_record(full):
    """The compact record the driver parses (the LAST stdout line): the contract keys, ``roofline`` re-based on the step's
    dominant kernel IN the step, ``cpu_baseline``, the parity scalars with the criterion spelt out, and one scalar per
    BASELINE.json config.  Scalars and short strings only; every leg's full output goes to FULL_RECORD and to an earlier
    stdout line.  Pure function of the full record (tests/test_bench_cli.py builds one from canned legs)."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data")
    rec = {k: full[k] for k in keep if k in full}
    cfg = full.get("config", {})
    host = cfg.get("host_ms_between_graph_replays_per_rank")
    rec["config"] = {
        "workload": _short(cfg.get("workload", ""), 160),
        "circuits_per_step_per_gpu": cfg.get("circuits_per_step_per_gpu"), "global_circuits_per_step": cfg.get("global_circuits_per_step"),
        "corpus_circuits": cfg.get("corpus_circuits"), "corpus_circuits_per_gpu": cfg.get("corpus_circuits_per_gpu"),
        "nodes_per_step_per_gpu": cfg.get("nodes_per_step_per_gpu"),
        "parallelism": cfg.get("parallelism"), "step_mode": _short(cfg.get("step_mode", ""), 80), "backend": cfg.get("backend"),
        "ranks_joined": cfg.get("ranks_joined"), "collective": _short(cfg.get("collective"), 120) if cfg.get("collective") else None,
        "host_ms_between_graph_replays_per_rank": (round(max(host), 4) if isinstance(host, (list, tuple)) and host else host),
        "gradient_floats_all_reduced": cfg.get("gradient_floats_all_reduced"), "rccl_version": cfg.get("rccl_version")}
    for k in ("ms_per_step_p10", "ms_per_step_p50", "ms_per_step_p90", "final_loss", "host_enqueue_ms_per_step"):
        if k in full:
            rec[k] = full[k]
    rf = full.get("roofline")
    if rf:
        dom = rf.get("step_dominant")
        out = {"bound": rf.get("bound"), "peak": rf.get("peak"), "unit": rf.get("unit")}
        if dom:
            out.update({"kernel": dom["kernel"], "achieved": dom["achieved"], "frac": dom["frac"],
                        "bytes_per_launch": dom["bytes_per_launch"], "us_per_launch": dom["us_per_launch"],
                        "launches_per_step": dom["launches_per_step"],
                        "basis": "the step-dominant instantiation (pooled epilogue form) timed IN an eager single-stream train "
                                 "step with HIP events on its stream; ALGORITHMIC bytes (SURVEY 8d B_agg), mean of its launches",
                        "traffic": dom.get("traffic"), "traffic_source": dom.get("traffic_source")})
        else:           # N > 1 (no arena leg): the plain instantiation alone, labelled as such
            out.update({"kernel": _short(rf.get("kernel", ""), 60), "achieved": rf.get("achieved"), "frac": rf.get("frac"),
                        "bytes_per_launch": rf.get("bytes_per_launch"), "us_per_launch": rf.get("us_per_launch"),
                        "basis": "plain instantiation timed alone with rotated buffers (no in-step leg at N > 1)",
                        "traffic": rf.get("traffic")})
        out["nodes"], out["edges_with_loops"] = rf.get("nodes"), rf.get("edges_with_loops")
        out["frac_isolated_plain"] = rf.get("frac")
        out["us_isolated_plain"] = rf.get("us_per_launch")
        out["traffic_isolated_plain"] = rf.get("traffic")
        out["hbm_frac_isolated_plain"] = rf.get("hbm_frac")
        out["in_step_all_aggregations_frac"] = _dig(rf, ("in_step_all_aggregations", "frac"))
        out["measured_copy_GBps"] = rf.get("measured_copy_GBps")
        out["measured_add_GBps"] = rf.get("measured_add_GBps")
        rec["roofline"] = out
    cb = full.get("cpu_baseline")
    if cb:
        rec["cpu_baseline"] = {"value": cb.get("value"), "unit": cb.get("unit"), "cores": cb.get("cores"), "kind": cb.get("kind"),
                               "sample": _short(cb.get("sample", ""), 200), "batch32_ms_per_step": cb.get("batch32_ms_per_step")}
    pr = full.get("parity")
    if pr:
        rec["parity"] = {"criterion": "max |device - fp64 oracle| < 1e-5 (fp64 = the exact value of the reference's expression); "
                                      "the reference's own fp32 CPU arithmetic is reported beside it",
                         "oracle_pin": "Family A (this workload): no reference-held artefact exists, oracle pinned by dense algebra "
                                       "only; Family B / MLP oracles pinned by the reference's goldens 0.117838 / 0.032910",
                         "circuits": pr.get("circuits"), "tolerance": pr.get("tolerance"),
                         "max_abs_err_vs_cpu_f64": pr.get("max_abs_err_vs_cpu_f64"), "exp_val_mae_vs_cpu_f64": pr.get("exp_val_mae_vs_cpu_f64"),
                         "max_abs_err_vs_cpu_f32": pr.get("max_abs_err_vs_cpu_f32"),
                         "cpu_f32_own_gap_vs_f64": pr.get("cpu_f32_max_abs_err_vs_cpu_f64"),
                         "within_tolerance_of_exact": pr.get("within_tolerance_of_exact")}
    for key, path in FLAT_KEYS.items():
        v = _dig(full, path)
        if isinstance(v, (int, float)):
            rec[key] = v
    rec["full_record"] = FULL_RECORD
    return rec


def emit(full, side_file=True):
    """stdout: ONE JSON line, the headline record (the task's contract: "rank 0 prints ONE JSON line").  With ``side_file``
    (``--full``) the full record of every leg lands in FULL_RECORD (best effort: the directory may not be writable where the
    benchmark runs); MLQEM_BENCH_FULL_STDOUT=1 also prints it as an EARLIER stdout line (scripts/refresh_profiles.sh reads it from there)."""
    if side_file:
        try:
            os.makedirs(os.path.join(ROOT, os.path.dirname(FULL_RECORD)), exist_ok=True)
            with open(os.path.join(ROOT, FULL_RECORD), "w") as fh:
                json.dump(full, fh, indent=1)
        except OSError as exc:
            progress(f"could not write {FULL_RECORD}: {exc}")
    head = headline_record(full)
    if not side_file:
        head.pop("full_record")
    text = json.dumps(head)
    if len(text) > HEADLINE_MAX_BYTES:          # never again a line the driver cannot parse: drop the optional scalars
        for k in list(FLAT_KEYS) + ["parity"]:
            head.pop(k, None)
        text = json.dumps(head)
    if os.environ.get("MLQEM_BENCH_FULL_STDOUT", "0") == "1":
        print(json.dumps(dict(full, record="full (every leg); the headline record is the next and last line")), flush=True)
    print(text, flush=True)


def dump_outputs(out_dir, loss, trainer):
    """``--dump-outputs``: what the last timed step hands its caller, as float32 ``out_dir/<name>.npy``: ``loss`` (that step's
    MSE), ``params`` (every model parameter after that step's Adam update, flattened in parameter order) and ``grad`` (that
    step's gradient in the same order; at N > 1 the all-reduced mean).  The corpus, the model and the batch order are seeded, so
    two builds given the same arguments can be compared output for output."""
    os.makedirs(out_dir, exist_ok=True)
    for name, t in (("loss", loss), ("params", trainer.flat_param), ("grad", trainer.flat_grad)):
        np.save(os.path.join(out_dir, name + ".npy"), t.detach().float().cpu().numpy())


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a child torch.distributed.run.  Nothing in
    this process has touched the GPU (torch.cuda.device_count() does not initialise it on this image); the parent only
    waits and passes the child's exit code on."""
    backend = os.environ.get("MLQEM_BENCH_BACKEND", "nccl")
    have = torch.cuda.device_count()
    if backend == "nccl" and have < n:
        sys.exit(f"bench.py --gpus {n}: only {have} GPU(s) visible; one rank per GPU is required (RCCL)")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    sys.exit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=DEFAULT_BATCH, help="circuits per step per GPU")
    ap.add_argument("--n-j", type=int, default=0, help="J values per Trotter step count; 0 = 8 x batch x gpus / 10")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure the host enqueue time, the roofline leg and, at N = 1, every other leg "
                         "(cpu_baseline, parity, accuracy, family_b, small_batch, mlp_head, configs, inference)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy (float32)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the CPU legs (cpu_baseline, parity, accuracy, family_b) and the legs after them")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling: --batch is the GLOBAL number of circuits per step (each rank takes batch / gpus) and the corpus does "
                         "not grow with the number of GPUs; default: weak scaling (--batch circuits per step PER GPU)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args.gpus, sys.argv[1:])
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the hot path has no CPU fallback")
    # MLQEM_BENCH_BACKEND=gloo lets two ranks share one GPU to rehearse the multi-rank control flow on a 1-GPU box;
    # the driver's runs use the default: one GPU per rank, RCCL ("nccl") over xGMI.
    backend = os.environ.get("MLQEM_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    distributed = world > 1
    if distributed:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=dev)
        else:
            torch.distributed.init_process_group(backend)

    from blackwater.nn import ExpValCircuitGraphModelA
    from blackwater.train import BucketedTrainer, DataParallelShard, StratifiedBatches

    global_batch = args.batch if args.strong else args.batch * world
    if args.strong:
        if args.batch % world:
            sys.exit(f"bench.py --strong: --batch {args.batch} is not a multiple of --gpus {world}")
        args.batch //= world               # circuits per step on THIS rank from here on
    n_j = args.n_j if args.n_j > 0 else -(-CORPUS_BATCHES * global_batch // len(STEPS_LIST))
    progress("building the corpus")
    corpus = build_corpus(n_j)
    # the data-parallel split by circuit: balanced by node count, every shard the same length
    local_ids = DataParallelShard.split(corpus.node_counts, world)[rank]
    node_quantum = 1024
    arena = corpus.arena(dev, local_ids, filler_nodes=node_quantum)
    n_local = len(arena)
    torch.manual_seed(0)
    model = ExpValCircuitGraphModelA(100, 22, 10).to(dev)

    # Every rank walks its own shard in size-stratified batches (StratifiedBatches: the same number of circuits of every
    # Trotter step count in every batch, each class in its own seeded epoch permutation), `batch` circuits per step.  All
    # batches then have the same node and edge totals, so the whole step -- device batch assembly, forward, loss, backward,
    # (eager gradient all-reduce,) Adam -- is captured ONCE in a hipGraph and replayed: the host uploads 1024 graph ids and
    # launches the graph.  MLQEM_BENCH_GRAPHS=0 enqueues the same bucketed step kernel by kernel (~70 launches, 2 ms of host
    # time on a quiet box, 6 ms on a loaded one -- the step takes 6.8 ms on the device).
    sampler = StratifiedBatches(arena.node_counts[:n_local], arena.edge_counts[:n_local], args.batch, seed=1000 + rank)
    use_graphs = os.environ.get("MLQEM_BENCH_GRAPHS", "1") != "0"
    # MLQEM_BENCH_CAPTURE_COLLECTIVE=1: the gradient all-reduce captured inside the step's graph (one replay per step instead of two
    # replays around an eager collective).  Off by default: the step is device-bound either way (0.2 ms of host time against 6.2 ms), and
    # a capture that hangs on a multi-GPU node this session cannot rehearse would cost the scaling run; tests cover it at world size 1.
    capture_coll = distributed and backend == "nccl" and os.environ.get("MLQEM_BENCH_CAPTURE_COLLECTIVE", "0") == "1"
    trainer = BucketedTrainer(model, arena, lr=1e-3, graphs=use_graphs, node_quantum=node_quantum, distributed=distributed,
                              capture_collective=capture_coll)
    step_mode = "hipgraph replay (one capture: size-stratified batches share one bucket)" if use_graphs else "eager (bucketed)"

    def step():
        return trainer.step_ids(sampler.draw())

    try:
        step()                      # the capture (or, eagerly, the allocator's first sight of the batch), untimed
    except Exception as exc:        # a box where the capture fails still gets a measured, correct, eager number
        if distributed:
            raise
        print(f"bench.py: hipGraph capture failed ({type(exc).__name__}: {exc}); enqueueing the bucketed step eagerly", file=sys.stderr)
        torch.cuda.synchronize()
        trainer.graphs = False
        step_mode = "eager (bucketed; capture failed: %s)" % type(exc).__name__
        step()
    for _ in range(args.warmup):
        step()
    if distributed:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]   # per-step device times (HIP events on the step's stream)
    t0 = time.perf_counter()
    loss = None
    marks[0].record()
    for k in range(args.steps):
        loss = step()
        marks[k + 1].record()
    if distributed:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    per_step = np.array([marks[k].elapsed_time(marks[k + 1]) for k in range(args.steps)])
    loss = loss.clone()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loss, trainer)
    joined = 1
    dp_host_ms = None
    if distributed:
        # per-rank host time of the eager RCCL all-reduce call between the two graph replays of a step (the only eager launch of
        # a data-parallel step), so that a multi-GPU number explains itself
        mine = torch.tensor([trainer.host_between_replays_s / max(trainer.host_between_replays_n, 1) * 1e3], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(every, mine)
        dp_host_ms = [round(float(v.item()), 4) for v in every]
        t = torch.tensor([elapsed, 0.0], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t[:1], op=torch.distributed.ReduceOp.MAX)
        ones = torch.ones(1, device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(ones, op=torch.distributed.ReduceOp.SUM)
        elapsed, joined = t[0].item(), int(round(ones.item()))

    if args.full:
        # how long the HOST needs to enqueue one step (the step is device-bound only while this stays below ms_per_step): a few
        # extra steps, timed up to the return of the last enqueue
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(4):
            step()
        host_ms = (time.perf_counter() - t1) / 4 * 1e3
        torch.cuda.synchronize()

    if rank == 0:
        total = args.batch * joined * args.steps
        progress(f"timed region done: {total / elapsed:.0f} circuits/s")
        line = {
            "metric": "circuits/sec (GNN train step), 100q TFIM Trotter",
            "value": round(total / elapsed, 2), "unit": "circuits/s", "n_gpus": joined, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "strong" if args.strong else "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "cfg4: 100-qubit TFIM Trotter steps 1-10 x %d J values, GNN family A "
                                   "(GCNx3 || Chebx2 || SAGEx2, hidden 10, F=22), full train step" % n_j,
                       "circuits_per_step_per_gpu": args.batch, "corpus_circuits": len(corpus),
                       "corpus_circuits_per_gpu": n_local, "arena_nodes_per_gpu": int(arena.num_nodes),
                       "mean_nodes_per_circuit": round(arena.num_nodes / n_local, 1), "parallelism": f"dp{joined}",
                       "nodes_per_step_per_gpu": sampler.nodes_per_batch, "step_mode": step_mode,
                       "sampling": "size-stratified: %s circuits of the 10 Trotter step counts per batch" % "/".join(map(str, sampler.quota)),
                       "backend": backend, "ranks_joined": joined, "host_ms_between_graph_replays_per_rank": dp_host_ms,
                       "gradient_floats_all_reduced": int(trainer.flat_grad.numel()),
                       "global_circuits_per_step": args.batch * joined,
                       "collective": (None if not distributed else "captured inside the step's hipGraph" if trainer.collective_in_graph
                                      else "eager all-reduce between two graph replays"
                                      + (" (capture refused: %s)" % trainer.collective_capture_error if trainer.collective_capture_error else "")),
                       "rccl_version": ".".join(map(str, torch.cuda.nccl.version())) if backend == "nccl" else None},
            "ms_per_step_percentiles": {"p10": round(float(np.percentile(per_step, 10)), 3), "p50": round(float(np.percentile(per_step, 50)), 3),
                                        "p90": round(float(np.percentile(per_step, 90)), 3), "min": round(float(per_step.min()), 3),
                                        "max": round(float(per_step.max()), 3), "note": "HIP events between consecutive steps on rank 0"},
            # the same percentiles as top-level numbers (a driver that keeps only scalar keys keeps these)
            "ms_per_step_p10": round(float(np.percentile(per_step, 10)), 3), "ms_per_step_p50": round(float(np.percentile(per_step, 50)), 3),
            "ms_per_step_p90": round(float(np.percentile(per_step, 90)), 3),
            "final_loss": round(float(loss.item()), 6),
        }
        if args.full:
            line["host_enqueue_ms_per_step"] = round(host_ms, 3)
            progress("roofline leg")
            fixed = arena.batch(fixed_ids(n_local, args.batch))
            line["roofline"] = roofline_leg(fixed, arena if world == 1 else None, fixed_ids(n_local, args.batch), 100)
        if args.full and world == 1 and not args.no_cpu_baseline:
            rep = local_ids[fixed_ids(n_local, args.batch)]
            progress("cpu_baseline leg")
            line["cpu_baseline"] = cpu_baseline_leg(corpus, rep, 100)
            progress("parity leg")
            line["parity"] = parity_leg(model, arena, corpus, local_ids, 100)   # the oracle as the checker, outside the timed region
            del trainer, model, arena, fixed
            from blackwater.native import ops as _ops
            _ops.set_seed_counter(None)       # the bucketed trainer's device-resident dropout counter
            torch.cuda.empty_cache()
            only = [k for k in os.environ.get("MLQEM_BENCH_LEGS", "").split(",") if k]     # diagnostics: a subset of the legs
            for key, leg in (("accuracy", accuracy_leg), ("family_b", family_b_leg), ("small_batch", small_batch_leg),
                             ("mlp_head", mlp_head_leg), ("configs", configs_leg), ("inference", inference_leg)):
                if only and key not in only:
                    continue
                progress(f"{key} leg")
                line[key] = leg(dev)
            progress("done")
        emit(line, side_file=args.full)
    if distributed:
        torch.distributed.barrier()  # rank 0 is still in its roofline leg: leave together
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
