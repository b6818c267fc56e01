"""Synced BatchNorm statistics (torch.nn.SyncBatchNorm semantics) for the MLP2 / MLP3 heads under data parallelism: the record / merge
kernels of csrc/bn_sync.hpp on both BatchNorm pipelines, two ranks over gloo against one process on the whole batch, uneven row
counts, and world size 1 left exactly as it was."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "dp_sync_bn_worker.py")
N, C = 1000, 125
SPLITS = {1: [1000], 2: [1, 999], 3: [400, 1, 599], 8: [1, 200, 13, 100, 300, 86, 150, 150]}
BIG = 7          # the column with mean 1e3 and spread 1e-2


def _matrix(storage):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, generator=gen, dtype=torch.float64) * torch.linspace(0.5, 2.0, C, dtype=torch.float64) \
        + torch.linspace(1.0, 3.0, C, dtype=torch.float64)
    x[:, BIG] = 1e3 + 1e-2 * torch.randn(N, generator=gen, dtype=torch.float64)
    x = x.float()
    if storage == "bf16":
        x = x.bfloat16().float()          # the statistics of what the pipeline stores
    g = (1.0 + 0.5 * (x.double() - x.double().mean(0)) / x.double().std(0).clamp_min(1e-6)
         + 0.5 * torch.randn(N, C, generator=gen, dtype=torch.float64)).float()
    return x, g


def _close(got, want, rtol, atol=0.0):
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs() - rtol * want.abs() - atol
    assert err.max().item() <= 0.0, (got - want).abs().max().item()


def _bounds(sizes):
    off = np.concatenate([[0], np.cumsum(sizes)])
    return list(zip(off[:-1], off[1:]))


@pytest.mark.parametrize("storage", ["bn", "f32", "bf16"])
@pytest.mark.parametrize("k", sorted(SPLITS))
def test_records_of_row_chunks_merge_to_the_statistics_of_the_whole_matrix(storage, k):
    from blackwater.native import ops

    x, g = _matrix(storage)
    xd = x.double()
    mean_ref, var_ref = xd.mean(0), xd.var(0, unbiased=False)
    eps, mom = 1e-5, 0.1
    gamma = torch.linspace(0.5, 1.5, C, device=DEV)
    beta = torch.linspace(-0.2, 0.3, C, device=DEV)
    recs = torch.zeros((k, 2 * C + 1), dtype=torch.float64, device=DEV)
    rm, rv = torch.full((C,), 0.25, device=DEV), torch.full((C,), 2.0, device=DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    if storage == "bn":
        xg = ops.padded_copy(x.to(DEV))
        for i, (a, b) in enumerate(_bounds(SPLITS[k])):
            ops.batch_norm_sync_record(0, xg[a:b], recs[i])
        y, mean, var, invstd = ops.batch_norm_sync_train(recs, xg, gamma, beta, eps, running=(rm, rv, mom, nbt))
    else:
        act = torch.zeros((N, 128), dtype=torch.float32 if storage == "f32" else torch.bfloat16, device=DEV)
        act[:, :C] = x.to(DEV)
        for i, (a, b) in enumerate(_bounds(SPLITS[k])):
            ops.layer_colstats_record(0, act[a:b], recs[i], int(b - a), C)
        mean, var, invstd, scale, shift = ops.layer_colstats_merge(0, recs, C, gamma, beta, eps, running=(rm, rv, mom, nbt))
        assert not mean[C:].any() and not scale[C:].any() and not shift[C:].any()      # the layout of colstats: zeros beyond C
        mean, var, invstd = mean[:C], var[:C], invstd[:C]
        y = act[:, :C].float() * scale[:C] + shift[:C]
    assert recs[:, 0].sum().item() == N
    rest = [c for c in range(C) if c != BIG]
    _close(mean, mean_ref, 1e-6)
    _close(var[rest], var_ref[rest], 1e-6)
    _close(var[BIG:BIG + 1], var_ref[BIG:BIG + 1], 1e-5, 1e-12)   # bf16 stores that column as one value: var 0
    _close(invstd[rest], 1.0 / torch.sqrt(var_ref[rest] + eps), 1e-6)
    # the running buffers: ONE update with the global N
    _close(rm, 0.9 * 0.25 + mom * mean_ref, 1e-6, 1e-7)
    _close(rv, 0.9 * 2.0 + mom * var_ref * N / (N - 1), 1e-6, 1e-7)
    assert nbt.item() == 1
    ref_y = (xd - mean_ref) / torch.sqrt(var_ref + eps) * gamma.double().cpu() + beta.double().cpu()
    _close(y[:, rest], ref_y[:, rest], 1e-5, 1e-5)

    # backward records (sum g, sum g xhat with the merged mean / invstd) -> k1, k2 (and dx for bn.hip)
    mu, inv = mean.double().cpu(), invstd.double().cpu()
    xhat = (xd - mu) * inv
    k1_ref, k2_ref = g.double().mean(0), (g.double() * xhat).mean(0)
    brecs = torch.zeros_like(recs)
    db_sum = torch.zeros(C, dtype=torch.float64)
    dg_sum = torch.zeros(C, dtype=torch.float64)
    if storage == "bn":
        gd = ops.padded_copy(g.to(DEV))
        for i, (a, b) in enumerate(_bounds(SPLITS[k])):
            dg_i, db_i = ops.batch_norm_sync_record(1, xg[a:b], brecs[i], dy=gd[a:b], mean=mean, invstd=invstd)
            db_sum += db_i.double().cpu()
            dg_sum += dg_i.double().cpu()
        dx = ops.batch_norm_sync_train_bwd(brecs, gd, xg, gamma, mean, invstd)
        dx_ref = gamma.double().cpu() * inv * (g.double() - k1_ref - xhat * k2_ref)
        _close(dx[:, rest], dx_ref[:, rest], 1e-5, 1e-5)
    else:
        gd = g.to(DEV)
        for i, (a, b) in enumerate(_bounds(SPLITS[k])):
            db_i, dg_i = ops.layer_colstats_record(1, act[a:b], brecs[i], int(b - a), C, g=gd[a:b], scale=scale, shift=shift,
                                                   mean=torch.cat([mean, torch.zeros(128 - C, device=DEV)]),
                                                   invstd=torch.cat([invstd, torch.zeros(128 - C, device=DEV)]), relu=False)
            assert not db_i[C:].any() and not dg_i[C:].any()
            db_sum += db_i[:C].double().cpu()
            dg_sum += dg_i[:C].double().cpu()
        gs, k1, k2 = ops.layer_colstats_merge(1, brecs, C, gamma, invstd=torch.cat([invstd, torch.zeros(128 - C, device=DEV)]))
        _close(k1[:C], k1_ref, 1e-6, 1e-7)
        _close(k2[:C], k2_ref, 1e-6, 1e-7)
        _close(gs[:C], gamma.double().cpu() * inv, 1e-6)
        assert not gs[C:].any() and not k1[C:].any() and not k2[C:].any()
    assert brecs[:, 0].sum().item() == N
    _close(db_sum, g.double().sum(0), 1e-5, 1e-4)        # this rank's sums: the parameter gradients of its rows
    _close(dg_sum, (g.double() * xhat).sum(0), 1e-5, 1e-4)


def test_merge_entry_points_refuse_bad_arguments():
    from blackwater.native import _lib

    lib = _lib.load()
    one = torch.ones(128, device=DEV)
    recs = torch.zeros((2, 2 * 130 + 1), dtype=torch.float64, device=DEV)
    p = one.data_ptr()
    assert lib.mlqem_layer_colstats_merge(0, recs.data_ptr(), 2, 130, p, p, None, 1e-5, p, p, p, p, p, None, None, 0.1, None, None) == -1
    assert lib.mlqem_layer_colstats_merge(0, recs.data_ptr(), 0, 8, p, p, None, 1e-5, p, p, p, p, p, None, None, 0.1, None, None) == -1
    assert lib.mlqem_batch_norm_sync_record_f32(2, p, 8, None, 0, None, None, 4, 8, recs.data_ptr(), None, None, None, 0, None) == -1


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}


def _two_ranks(tmp_path, case):
    port = _port()
    outs = [str(tmp_path / f"{case}_rank{r}.pt") for r in (0, 1)]
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), "2", str(port), outs[r], case], env=_env(), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in (0, 1)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=600)[0])
    finally:
        for p in procs:          # exactly the two children this test started
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(log[-2000:] for log in logs)
    return [torch.load(o, weights_only=False) for o in outs]


def _one_process(tmp_path, case):
    out = str(tmp_path / f"{case}_single.pt")
    one = subprocess.run([sys.executable, WORKER, "0", "1", "0", out, case], env=_env(), capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, (one.stdout + one.stderr)[-2000:]
    return torch.load(out, weights_only=False)


def _grad_gap(ref, r):
    return (ref["grad0"] - r["grad0"]).norm().item() / ref["grad0"].norm().item()


@pytest.mark.parametrize("case", ["mlp3_f32", "mlp3_bf16", "gnn3"])
def test_two_synced_ranks_equal_one_process_on_the_whole_batch(tmp_path, case):
    """Two ranks share the GPU over gloo, each stepping on its half of every batch with SyncBatchNorm heads, against one process on
    the whole batch: the same gradient (the statistics are the batch's), the same first running-buffer update, ranks in lock-step."""
    r0, r1 = _two_ranks(tmp_path, case)
    ref = _one_process(tmp_path, case)
    assert _grad_gap(ref, r0) <= 1e-5, _grad_gap(ref, r0)
    assert torch.equal(r0["grad0"], r1["grad0"])
    assert torch.equal(r0["param"], r1["param"])                       # lock-step, bit for bit
    assert r0["bn"].keys() == r1["bn"].keys() == ref["bn"].keys() and len(ref["bn"]) == 6
    for key in r0["bn"]:
        assert torch.equal(r0["bn"][key], r1["bn"][key]), key           # identical records -> identical buffers on every rank
        assert torch.equal(r0["bn0"][key], r1["bn0"][key]), key
        if "num_batches" in key:
            assert r0["bn"][key].item() == ref["bn"][key].item() == 4
        else:
            assert (r0["bn0"][key] - ref["bn0"][key]).abs().max().item() <= 1e-6, key
    assert r0["losses"] != r1["losses"]                                 # ... on different halves
    mean = [(a + b) / 2 for a, b in zip(r0["losses"], r1["losses"])]    # equal halves: the whole batch's MSE is their mean
    assert np.allclose(mean, ref["losses"], rtol=1e-4, atol=1e-7)
    if case == "gnn3":
        assert r0["graphs"] and r0["eager_reason"] and "SyncBatchNorm" in r0["eager_reason"]
        assert ref["eager_reason"] is None


def test_plain_batchnorm_keeps_per_rank_statistics(tmp_path):
    """The control: the same harness with plain BatchNorm1d is far from the single process -- the default is unchanged, and the
    comparison above can tell the two apart."""
    r0, r1 = _two_ranks(tmp_path, "mlp3_plain")
    ref = _one_process(tmp_path, "mlp3_plain")
    assert _grad_gap(ref, r0) > 1e-3
    assert torch.equal(r0["param"], r1["param"])
    assert not torch.equal(r0["bn"]["bn1.running_mean"], r1["bn"]["bn1.running_mean"])


def test_uneven_row_counts_and_a_single_row_rank(tmp_path):
    """Ranks with 40 / 24 rows and 1 / 63 rows: each rank's output rows (bn.hip and the fp32 layer pipeline) and input-gradient rows
    are the matching rows of whole-batch BatchNorm, and the running buffers are the whole batch's update."""
    r0, r1 = _two_ranks(tmp_path, "uneven")
    gen = torch.Generator().manual_seed(99)
    x = (torch.randn(64, 96, generator=gen) * 2.0 + torch.linspace(-3.0, 3.0, 96)).double()
    g = torch.randn(64, 96, generator=gen).double()
    for split in (40, 1):
        a, b = r0[split], r1[split]
        assert a["grouped"] and b["grouped"]
        assert a["rows"] == (0, split) and b["rows"] == (split, 64)
        gamma, beta = a["gamma"].double(), a["beta"].double()
        mean, var = x.mean(0), x.var(0, unbiased=False)
        inv = 1.0 / torch.sqrt(var + 1e-5)
        xhat = (x - mean) * inv
        y = xhat * gamma + beta
        dx = gamma * inv * (g - g.mean(0) - xhat * (g * xhat).mean(0))
        for r in (a, b):
            lo, hi = r["rows"]
            _close(r["y"], y[lo:hi], 1e-6, 1e-6)
            _close(r["layer_y"], y[lo:hi], 1e-6, 1e-6)
            _close(r["dx"], dx[lo:hi], 1e-5, 1e-6)
            _close(r["bn"]["running_mean"], 0.1 * mean, 1e-6, 1e-7)
            _close(r["bn"]["running_var"], 0.9 + 0.1 * var * 64 / 63, 1e-6, 1e-7)
            assert r["bn"]["num_batches_tracked"].item() == 1
            _close(r["layer_run"][0], 0.1 * mean, 1e-6, 1e-7)
            _close(r["layer_run"][1], 0.9 + 0.1 * var * 64 / 63, 1e-6, 1e-7)
            assert r["layer_run"][2] == 1
        for key in a["bn"]:
            assert torch.equal(a["bn"][key], b["bn"][key]), key


def test_rank_without_rows_raises():
    """A synced BatchNorm on a rank with zero rows refuses loudly (its statistics would be no one's)."""
    from unittest import mock

    from blackwater.native import functional as F

    bn = torch.nn.SyncBatchNorm(16).to(DEV).train()
    with mock.patch.object(F, "sync_group", lambda m: "group"):
        with pytest.raises(ValueError, match="no rows"):
            F.batch_norm_train(torch.empty((0, 16), device=DEV), bn)


def _mlp3_run(convert, steps=5):
    from blackwater.native import ops
    from blackwater.nn.mlp import MLP3
    from blackwater.train import RowsTrainer

    torch.manual_seed(3)
    model = MLP3(170, 128, 4)
    if convert:
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    model = model.to(DEV)
    gen = torch.Generator().manual_seed(8)
    x, y = torch.randn(512, 170, generator=gen).to(DEV), torch.randn(512, 4, generator=gen).to(DEV)
    tr = RowsTrainer(model, lr=1e-3, graphs=True)
    losses = [tr.step_rows(x, y).clone() for _ in range(steps)]
    ops.set_seed_counter(None)
    return torch.stack(losses).cpu(), tr.flat_param.detach().cpu().clone(), {k: v.cpu() for k, v in model.state_dict().items()}


def _gnn3_run(g1, convert, steps=5):
    from helpers import g1_graph

    from blackwater.data.arena import GraphArena
    from blackwater.native import ops
    from blackwater.nn.family_b import ExpValCircuitGraphModel_3
    from blackwater.train import BucketedTrainer

    xs, eis = [], []
    for i in range(64):
        x, ei, _ = g1_graph(g1, i)
        loops = np.arange(x.shape[0])
        xs.append(x.astype(np.float32))
        eis.append(np.concatenate([ei, np.stack([loops, loops])], axis=1))
    arena = GraphArena.from_arrays(xs, eis, g1["ideal"][:64, None, :].astype(np.float32), g1["noisy"][:64, None, :].astype(np.float32),
                                   g1["depth"][:64, None].astype(np.float32), np.zeros((64, 1, 1), np.float32), device=DEV,
                                   filler_nodes=1024)
    torch.manual_seed(4)
    model = ExpValCircuitGraphModel_3(22, 15, 4)
    if convert:
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    model = model.to(DEV)
    tr = BucketedTrainer(model, arena, lr=1e-3, graphs=True, node_quantum=1024)
    assert tr.eager_reason is None
    losses = [tr.step_ids(list(range(k, k + 32))).clone() for k in (0, 8, 16, 0, 8)[:steps]]
    ops.set_seed_counter(None)
    return torch.stack(losses).cpu(), tr.flat_param.detach().cpu().clone(), {k: v.cpu() for k, v in model.state_dict().items()}


def test_world_size_one_converted_models_are_bit_equal_to_unconverted(g1):
    """Without a process group a converted model takes today's path: captured steps, per-batch statistics, bit for bit."""
    for run in (_mlp3_run, lambda conv: _gnn3_run(g1, conv)):
        plain, conv = run(False), run(True)
        assert torch.equal(plain[0], conv[0])
        assert torch.equal(plain[1], conv[1])
        assert plain[2].keys() == conv[2].keys()
        for key in plain[2]:
            assert torch.equal(plain[2][key], conv[2][key]), key
