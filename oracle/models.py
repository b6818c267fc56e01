"""The reference's models restated on top of ``pyg_restatement`` (oracle; test infra only).

State-dict keys and shapes equal the reference checkpoints' (docs/tutorials/model/**.pth), so those load
with ``strict=True``.
  Family B: docs/tutorials/gnn.py:70-122 (ExpValCircuitGraphModel), :178-224 (_3), :229-276 (_4); _2 (:126-173)
            is restated from its checkpoint (model/haoran_mbd2/cliffords_and_mbd3.pth) since the source
            references an unimported MLP2.
  Family A: docs/tutorials/01_ngem.ipynb cell [9].
  MLP1/2/3: docs/tutorials/mlp.py:18-108.
"""
from __future__ import annotations

import torch
from torch import nn

from .pyg_restatement import (ASAPooling, ChebConv, GCNConv, SAGEConv, TransformerConv, global_mean_pool)


class MLP1(nn.Module):
    def __init__(self, input_size, hidden_size, output_size):
        super().__init__()
        self.fc1 = nn.Linear(input_size, hidden_size)
        self.fc2 = nn.Linear(hidden_size, output_size)

    def forward(self, x):
        return self.fc2(torch.relu(self.fc1(x)))


class MLP2(nn.Module):
    def __init__(self, input_size, hidden_size, output_size, dropout_rate=0.5):
        super().__init__()
        self.fc1, self.bn1 = nn.Linear(input_size, hidden_size), nn.BatchNorm1d(hidden_size)
        self.fc2, self.bn2 = nn.Linear(hidden_size, hidden_size), nn.BatchNorm1d(hidden_size)
        self.fc3 = nn.Linear(hidden_size, output_size)
        self.drop = nn.Dropout(dropout_rate)

    def _drop(self, t, masks, name):
        """``masks`` (optional): a mapping from ``block1``, ``block2``, ``tail`` to a keep tensor of that activation -- a present entry
        replaces ``self.drop`` by ``t * keep / (1 - p)`` (a test hands in the masks the device drew), as FamilyA.forward's does."""
        if masks and name in masks:
            return t * masks[name].to(t.dtype) / (1.0 - self.drop.p)
        return self.drop(t)

    def trunk(self, x, masks=None):
        x1 = self._drop(torch.relu(self.bn1(self.fc1(x))), masks, "block1")
        x2 = self._drop(torch.relu(self.bn2(self.fc2(x1))), masks, "block2")
        return x1 + x2

    def forward(self, x, masks=None):
        return self.fc3(self.trunk(x, masks))


class MLP3(MLP2):
    def __init__(self, input_size, hidden_size, output_size, dropout_rate=0.3):
        super().__init__(input_size, hidden_size, output_size, dropout_rate)
        self.fc3 = nn.Linear(hidden_size, hidden_size // 3)
        self.fc4 = nn.Linear(hidden_size // 3, output_size)

    def forward(self, x, masks=None):
        return self.fc4(self._drop(torch.relu(self.fc3(self.trunk(x, masks))), masks, "tail"))


class _Identity2(nn.Module):
    """Placeholder so that ``body_seq`` keeps indices 0 and 2 for its two Linear layers."""

    def __init__(self, p):
        super().__init__()
        self.p = p

    def forward(self, x):
        return nn.functional.dropout(x, self.p, self.training)


class FamilyB(nn.Module):
    """TransformerConv -> ASAPooling -> TransformerConv -> ASAPooling -> mean pool -> head (gnn.py:100-122)."""

    def __init__(self, num_node_features, hidden_channels, exp_value_size=4, dropout=0.2, heads=(3, 2),
                 head="linear", head_hidden=None):
        super().__init__()
        h1, h2 = heads
        self.transformer1 = TransformerConv(num_node_features, hidden_channels, heads=h1, dropout=0.1)
        self.pooling1 = ASAPooling(hidden_channels * h1, 0.5)
        self.transformer2 = TransformerConv(hidden_channels * h1, hidden_channels, heads=h2, dropout=0.1)
        self.pooling2 = ASAPooling(hidden_channels * h2, 0.5)
        width = hidden_channels * h2 + 1 + exp_value_size
        if head == "linear":
            self.body_seq = nn.Sequential(nn.Linear(width, hidden_channels), _Identity2(dropout),
                                          nn.Linear(hidden_channels, exp_value_size))
        elif head == "mlp2":
            self.body_seq = MLP2(width, head_hidden or hidden_channels, exp_value_size, dropout)
        else:
            self.body_seq = MLP3(width, head_hidden or hidden_channels * h1, exp_value_size, dropout)

    def forward(self, exp_value, observable, circuit_depth, nodes, edge_index, batch):
        g = self.transformer1(nodes, edge_index)
        g, edge_index, _, batch, _ = self.pooling1(g, edge_index, batch=batch)
        g = self.transformer2(g, edge_index)
        g, edge_index, _, batch, _ = self.pooling2(g, edge_index, batch=batch)
        num_graphs = exp_value.shape[0]
        g = global_mean_pool(g, batch, num_graphs)
        merged = torch.cat((g, torch.squeeze(exp_value, 1), circuit_depth), dim=1)
        return self.body_seq(merged)


def family_b_from_state_dict(sd) -> FamilyB:
    """Builds the Family-B variant whose shapes match a reference checkpoint, and loads it strictly."""
    f = sd["transformer1.lin_key.weight"].shape[1]
    hc1 = sd["transformer1.lin_key.weight"].shape[0]
    hc2 = sd["transformer2.lin_key.weight"].shape[0]
    if "body_seq.0.weight" in sd:
        hidden = sd["body_seq.0.weight"].shape[0]
        out = sd["body_seq.2.weight"].shape[0]
        model = FamilyB(f, hidden, out, heads=(hc1 // hidden, hc2 // hidden), head="linear")
    else:
        head_hidden = sd["body_seq.fc1.weight"].shape[0]
        width = sd["body_seq.fc1.weight"].shape[1]
        if "body_seq.fc4.weight" in sd:
            out = sd["body_seq.fc4.weight"].shape[0]
            kind = "mlp3"
        else:
            out = sd["body_seq.fc3.weight"].shape[0]
            kind = "mlp2"
        hidden = _infer_hidden(hc1, hc2, width - 1 - out)
        model = FamilyB(f, hidden, out, heads=(hc1 // hidden, hc2 // hidden), head=kind, head_hidden=head_hidden)
    model.load_state_dict(sd, strict=True)
    return model


def _infer_hidden(hc1, hc2, pooled_width):
    assert pooled_width == hc2
    for heads in ((5, 3), (3, 2)):
        if hc1 % heads[0] == 0 and hc2 % heads[1] == 0 and hc1 // heads[0] == hc2 // heads[1]:
            return hc1 // heads[0]
    raise ValueError("unrecognised Family-B shape")


class FamilyA(nn.Module):
    """GCNx3 || Chebx2 || SAGEx2 -> mean pools; observable MLP; 6-wide body (01_ngem.ipynb cell [9])."""

    def __init__(self, n_qubits, num_node_features, hidden_channels):
        super().__init__()
        hc = hidden_channels
        self.conv1, self.conv2, self.conv3 = GCNConv(num_node_features, hc), GCNConv(hc, hc), GCNConv(hc, 1)
        self.cheb_conv1, self.cheb_conv2 = ChebConv(num_node_features, hc, K=3), ChebConv(hc, 1, K=2)
        self.sage_conv1, self.sage_conv2 = SAGEConv(num_node_features, hc), SAGEConv(hc, 1)
        self.obs_seq = nn.Sequential(nn.Linear(n_qubits * 4 + 1, hc), _Identity2(0.2), nn.Linear(hc, 1))
        self.body_seq = nn.Sequential(nn.Linear(6, hc), nn.Linear(hc, 1))
        self.p_gcn, self.p_other = 0.1, 0.2

    def forward(self, exp_value, observable, circuit_depth, nodes, edge_index, batch, masks=None):
        """``masks`` (optional): a mapping from ``conv1``, ``conv2``, ``cheb_conv1``, ``sage_conv1``, ``obs_seq`` to a keep tensor
        of that layer's activation -- a present entry replaces the generator's dropout by ``t * keep / (1 - p)`` (a test hands in the
        masks the device drew); an absent one leaves ``nn.functional.dropout``."""
        masks = masks or {}

        def drop(t, p, name):
            if name in masks:
                return t * masks[name].to(t.dtype) / (1.0 - p)
            return nn.functional.dropout(t, p=p, training=self.training)

        b = exp_value.shape[0]
        g = drop(self.conv1(nodes, edge_index).relu(), self.p_gcn, "conv1")
        g = drop(self.conv2(g, edge_index).relu(), self.p_gcn, "conv2")
        g = global_mean_pool(self.conv3(g, edge_index), batch, b)
        c = drop(self.cheb_conv1(nodes, edge_index).relu(), self.p_other, "cheb_conv1")
        c = global_mean_pool(self.cheb_conv2(c, edge_index), batch, b)
        s = drop(self.sage_conv1(nodes, edge_index).relu(), self.p_other, "sage_conv1")
        s = global_mean_pool(self.sage_conv2(s, edge_index), batch, b)
        if "obs_seq" in masks:
            lin1, mid, lin2 = self.obs_seq
            obs = torch.mean(lin2(drop(lin1(observable), mid.p, "obs_seq")), dim=1)
        else:
            obs = torch.mean(self.obs_seq(observable), dim=1)
        merged = torch.cat((g, c, s, obs, circuit_depth, exp_value), dim=1)
        return self.body_seq(merged)
