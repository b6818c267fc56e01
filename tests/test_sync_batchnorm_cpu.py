"""SyncBatchNorm conversion of the BatchNorm heads, on the CPU: ``torch.nn.SyncBatchNorm.convert_sync_batchnorm`` keeps every
state-dict key, so checkpoints of the unconverted models (the reference's among them) strict-load into converted ones; and without
a process group no module counts as synced."""
import pytest
import torch


def _models():
    from blackwater.nn.family_b import ExpValCircuitGraphModel_2, ExpValCircuitGraphModel_3, ExpValCircuitGraphModel_4
    from blackwater.nn.mlp import MLP2, MLP3

    return {"mlp2": lambda: MLP2(58, 64, 4), "mlp3": lambda: MLP3(170, 128, 4), "gnn2": lambda: ExpValCircuitGraphModel_2(22, 15, 4),
            "gnn3": lambda: ExpValCircuitGraphModel_3(22, 15, 4), "gnn4": lambda: ExpValCircuitGraphModel_4(22, 15, 4)}


@pytest.mark.parametrize("name", ["mlp2", "mlp3", "gnn2", "gnn3", "gnn4"])
def test_convert_sync_batchnorm_keeps_state_dict_keys_and_strict_loads(name):
    from blackwater.native import functional as F

    torch.manual_seed(0)
    plain = _models()[name]()
    saved = {k: v.clone() for k, v in plain.state_dict().items()}
    torch.manual_seed(1)
    conv = torch.nn.SyncBatchNorm.convert_sync_batchnorm(_models()[name]())
    bns = [m for m in conv.modules() if isinstance(m, torch.nn.SyncBatchNorm)]
    assert len(bns) == 2 and not any(type(m) is torch.nn.BatchNorm1d for m in conv.modules())
    assert list(conv.state_dict().keys()) == list(saved.keys())
    conv.load_state_dict(saved, strict=True)
    for k, v in conv.state_dict().items():
        assert torch.equal(v, saved[k]), k
    # no process group: every module keeps per-batch statistics (today's path)
    assert all(F.sync_group(m) is None for m in conv.modules())


def test_plain_batchnorm_is_never_synced():
    from blackwater.native import functional as F

    assert F.sync_group(torch.nn.BatchNorm1d(8)) is None
    assert F.sync_group(torch.nn.SyncBatchNorm(8)) is None
