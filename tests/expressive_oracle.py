"""Oracle helpers of the expressiveness runs (test infrastructure, CPU only).

* NestedGINRef: the NestedGIN class that run_sr.py:139-214 and run_exp.py:143-218 define inline, restated on the oracle
  primitives (oracle/ref_model.py).  The head's dropout is taken as an argument: `drop` is the multiplier F.dropout
  applies (0 or 1 / (1 - p) = 2 per element), so a mask drawn anywhere can be replayed here.
* expressive_oracle_from_recipe: the golden's parameters from its seed recipe.
* cpu_features / collate / digest: the fixtures' ESC features on the CPU (oracle/ref_features.py), collated with the
  product's host Batch, and the integer digests tests/golden/model_expressive.npz records per graph.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import BatchNorm1d, Linear, ReLU, Sequential

import ref_model as rm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SR25_FILE = os.path.join(GOLDEN, "sr251256.g6")
EXP_FILE = os.path.join(GOLDEN, "exp_first40.txt")
FEATURE_KEYS = ("edge_index", "pos_enc", "pos_index", "pos_batch")
_MOD = (1 << 61) - 1


def _conv(n_in, hidden):
    return rm.GINEConv(Sequential(Linear(n_in, hidden), ReLU(), Linear(hidden, hidden), ReLU()), train_eps=False,
                       edge_dim=hidden)


class NestedGINRef(torch.nn.Module):
    """Same module tree, construction order and state_dict keys as the reference class."""

    def __init__(self, num_features, num_layers, hidden):
        super().__init__()
        self.conv1 = _conv(num_features, hidden)
        self.convs = torch.nn.ModuleList([_conv(hidden, hidden) for _ in range(num_layers - 1)])
        self.lin1 = Linear(hidden, hidden)
        self.lin2 = Linear(hidden, hidden)
        self.z_initial = torch.nn.Embedding(1800, hidden)
        self.z_embedding = Sequential(BatchNorm1d(hidden), ReLU(), Linear(hidden, hidden), BatchNorm1d(hidden), ReLU())

    def reset_parameters(self):
        self.conv1.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        for layer in self.z_embedding.children():
            if hasattr(layer, "reset_parameters"):
                layer.reset_parameters()
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()

    def logits(self, x, edge_index, pos_enc, pos_index, pos_batch, batch, drop=None):
        z = rm.global_add_pool(self.z_initial.weight[pos_index] * pos_enc.view(-1, 1), pos_batch)
        z = self.z_embedding(z)
        h = self.conv1(x, edge_index, z)
        for conv in self.convs:
            h = conv(h, edge_index, z)
        h = rm.global_add_pool(h, batch)
        h = F.relu(self.lin1(h))
        if self.training:
            h = h * drop.to(h.dtype)
        return self.lin2(h)

    def forward(self, x, edge_index, pos_enc, pos_index, pos_batch, batch, drop=None):
        return F.log_softmax(self.logits(x, edge_index, pos_enc, pos_index, pos_batch, batch, drop), dim=1)


def expressive_oracle_from_recipe(z, num_features):
    """torch.manual_seed(seed) BEFORE construction, then reset_parameters() — the recipe of the golden"""
    torch.manual_seed(int(z["seed"]))
    m = NestedGINRef(int(num_features), int(z["layers"]), int(z["hidden"]))
    m.reset_parameters()
    return m


def digest(a):
    """int64 [3] of an integer array: length, sum, position-weighted sum modulo 2^61 - 1"""
    v = [int(t) for t in np.asarray(a).reshape(-1)]
    return np.array([len(v), sum(v), sum((k + 1) * t for k, t in enumerate(v)) % _MOD], dtype=np.int64)


def graph_digests(graphs):
    """[G, 4, 3]: digest of edge_index / pos_enc / pos_index / pos_batch of every graph (Data objects or dicts)"""
    return np.stack([np.stack([digest(g[k].cpu().numpy() if torch.is_tensor(g[k]) else g[k]) for k in FEATURE_KEYS])
                     for g in graphs])


def cpu_features(raw, h=3):
    """create_subgraphs(g, h, use_rd=False, self_loop=True) of product `Data` graphs on the CPU oracle"""
    import ref_features as orc
    from esc_gnn_amd import Data
    out = []
    for d in raw:
        ei = d.edge_index.numpy()
        e = orc.encode_graph(ei[0], ei[1], int(d.x.size(0)), h, False, True)
        out.append(Data(x=d.x, edge_index=torch.tensor(np.stack([e["edge_src"], e["edge_dst"]])), y=d.y,
                        pos_enc=torch.tensor(e["pos_enc"]), pos_index=torch.tensor(e["pos_index"]),
                        pos_batch=torch.tensor(e["pos_batch"])))
    return out


def collate(graphs):
    """host collate -> the oracle's positional arguments (x, edge_index, pos_enc, pos_index, pos_batch, batch)"""
    from esc_gnn_amd import Batch
    b = Batch.from_data_list(list(graphs))
    return (b.x.float(), b.edge_index, b.pos_enc, b.pos_index, b.pos_batch, b.batch)


def grad_digest(g):
    return np.array([float(g.double().sum()), float(g.double().abs().sum())])
