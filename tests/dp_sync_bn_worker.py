"""One rank of the SyncBatchNorm rehearsal (tests/test_gpu_sync_batchnorm.py starts two of these, both on cuda:0, over gloo, and one
with ``world == 1``: the single process on the whole batch that the two ranks must reproduce).

Cases: ``mlp3_f32`` / ``mlp3_bf16`` (MLP3(170, 128, 4) through RowsTrainer), ``gnn3`` (ExpValCircuitGraphModel_3(22, 15, 4) on the G1
graphs through BucketedTrainer), ``mlp3_plain`` (the f32 case with plain BatchNorm1d: the control), ``uneven`` (synced BatchNorm alone
on 40 / 24 and 1 / 63 rows, bn.hip and the fp32 layer pipeline).  Dropout is 0 everywhere: masks are keyed by rows, so they differ
between a rank and the single process.  Writes what it measured to ``out``."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "ml-qem_amd")]
DEV = "cuda:0"
STEPS = 4


def _bn_state(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}


def _mlp(rank, world, case):
    from blackwater.nn.mlp import MLP3
    from blackwater.train import RowsTrainer

    gen = torch.Generator().manual_seed(1234)
    x_all = torch.randn(256, 170, generator=gen)
    y_all = torch.randn(256, 4, generator=gen)
    torch.manual_seed(rank)                 # different seeds: the Trainer brings every replica to rank 0's parameters
    model = MLP3(170, 128, 4, dropout_rate=0.0)
    if case != "mlp3_plain":
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    model.mfma = "bf16" if case == "mlp3_bf16" else "f32"
    model = model.to(DEV)
    trainer = RowsTrainer(model, lr=1e-3, graphs=False, distributed=world > 1)
    losses, bn0 = [], None
    for step in range(STEPS):
        rows = torch.arange(step * 32, step * 32 + 64)[rank::world]     # equal halves: the mean of the two MSEs is the batch's
        losses.append(float(trainer.step_rows(x_all[rows].to(DEV), y_all[rows].to(DEV))))
        if step == 0:
            grad0 = trainer.flat_grad.detach().cpu().clone()             # after the all-reduce: the mean over the ranks
            bn0 = _bn_state(model)                                       # the first update: made from identical parameters
    return {"param": trainer.flat_param.detach().cpu(), "losses": losses, "grad0": grad0, "bn0": bn0, "bn": _bn_state(model)}


def _gnn(rank, world):
    from helpers import g1_graph

    from blackwater.data.arena import GraphArena
    from blackwater.native import ops
    from blackwater.nn.family_b import ExpValCircuitGraphModel_3
    from blackwater.train import BucketedTrainer

    z = dict(np.load(os.path.join(HERE, "golden", "g1_dataset.npz")))
    xs, eis = [], []
    for i in range(128):
        x, ei, _ = g1_graph(z, i)
        loops = np.arange(x.shape[0])
        xs.append(x.astype(np.float32))
        eis.append(np.concatenate([ei, np.stack([loops, loops])], axis=1))
    arena = GraphArena.from_arrays(xs, eis, z["ideal"][:128, None, :].astype(np.float32), z["noisy"][:128, None, :].astype(np.float32),
                                   z["depth"][:128, None].astype(np.float32), np.zeros((128, 1, 1), np.float32), device=DEV,
                                   filler_nodes=1024)
    torch.manual_seed(rank)
    model = ExpValCircuitGraphModel_3(22, 15, 4, dropout=0.0)
    model.transformer1.dropout = model.transformer2.dropout = 0.0        # attention dropout off too
    model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model).to(DEV)
    trainer = BucketedTrainer(model, arena, lr=1e-3, graphs=world > 1, node_quantum=1024, distributed=world > 1)
    losses, bn0 = [], None
    for step in range(STEPS):
        ids = np.arange(step * 16, step * 16 + 64)
        losses.append(float(trainer.step_ids(ids[rank::world])))
        if step == 0:
            grad0 = trainer.flat_grad.detach().cpu().clone()
            bn0 = _bn_state(model)
    ops.set_seed_counter(None)
    return {"param": trainer.flat_param.detach().cpu(), "losses": losses, "grad0": grad0, "bn0": bn0, "bn": _bn_state(model),
            "eager_reason": trainer.eager_reason, "graphs": trainer.graphs}


def _uneven(rank, world):
    """Synced BatchNorm alone: this rank's output rows, input gradient rows and running buffers for two splits of 64 rows."""
    from blackwater.native import functional as F
    from blackwater.native import ops

    gen = torch.Generator().manual_seed(99)
    x_all = torch.randn(64, 96, generator=gen) * 2.0 + torch.linspace(-3.0, 3.0, 96)
    g_all = torch.randn(64, 96, generator=gen)
    res = {}
    for split in (40, 1):
        lo, hi = (0, split) if rank == 0 else (split, 64)
        torch.manual_seed(7)
        bn = torch.nn.SyncBatchNorm(96)
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.5, 0.5)
        bn = bn.to(DEV).train()
        x = ops.padded_copy(x_all[lo:hi].to(DEV)).requires_grad_(True)
        y = F.batch_norm_train(x, bn)
        y.backward(g_all[lo:hi].to(DEV))
        # the fp32 layer pipeline: an activation [n, 128] through the synced statistics and the affine map (no ReLU)
        act = torch.zeros((hi - lo, 128), device=DEV)
        act[:, :96] = x_all[lo:hi].to(DEV)
        rm, rv = torch.zeros(96, device=DEV), torch.ones(96, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        group = F.sync_group(bn)
        _, _, _, sc, sh = F._colstats_fwd(act, bn.weight.detach(), bn.bias.detach(), bn.eps, hi - lo, 96, (rm, rv, 0.1, nbt), group)
        z = ops.layer_act_bf16(act, sc, sh, hi - lo, 96, relu=False)
        res[split] = {"rows": (lo, hi), "y": y.detach().cpu(), "dx": x.grad.detach().cpu(), "gamma": bn.weight.detach().cpu(),
                      "beta": bn.bias.detach().cpu(), "bn": {k: v.detach().cpu() for k, v in bn.state_dict().items()},
                      "layer_y": z[:, :96].cpu(), "layer_run": (rm.cpu(), rv.cpu(), int(nbt.item())), "grouped": group is not None}
    return res


def main():
    rank, world, port, out, case = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    if case == "gnn3":
        res = _gnn(rank, world)
    elif case == "uneven":
        res = _uneven(rank, world)
    else:
        res = _mlp(rank, world, case)
    torch.save(res, out)
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
