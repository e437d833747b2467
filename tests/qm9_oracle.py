"""Oracle helpers of the QM9 feature (test infrastructure, CPU only).

* distance_ref: the reference's distance.py:25-47 restated in fp64 — edge length from `pos` (row = edge_index[0],
  col = edge_index[1]), divided by the graph's maximum (or max_value), appended to the edge attributes.
* NestedGINEffQm9Ref: qm9_models.py:25-139 on the oracle primitives — the ZINC composition with ReLU, the dense node input
  cat([x, pos], 1) + node_type_embedding(node_type), edge term [z_emb | edge_attr], mean-pool readout, flat output.
* qm9_batch_inputs: the seeded x / pos / node_type / 5-wide edge_attr laid over the `zinc3` collate batch (the golden's
  inputs are recorded too; this is the recipe that made them).
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import BatchNorm1d, Dropout, Linear, Sequential

import ref_model as rm

NUM_FEATURES = 8


def distance_ref(pos, edge_index, edge_attr=None, norm=True, max_value=None, cat=True, relative_pos=False, squared=False):
    """float64 [E, A + 1 (+3)] of one graph: [edge_attr | d | pos[col] - pos[row]]"""
    pos = torch.as_tensor(pos).double()
    ei = torch.as_tensor(edge_index).long().reshape(2, -1)
    row, col = ei[0], ei[1]
    rel = pos[col] - pos[row]
    dist = (rel ** 2).sum(1)
    if not squared:
        dist = dist.sqrt()
    dist = dist.view(-1, 1)
    if norm and dist.numel() > 0:
        dist = dist / (dist.max() if max_value is None else max_value)
    if edge_attr is not None and cat:
        pseudo = torch.as_tensor(edge_attr).double()
        pseudo = pseudo.view(-1, 1) if pseudo.dim() == 1 else pseudo
        out = torch.cat([pseudo, dist], dim=-1)
    else:
        out = dist
    if relative_pos:
        out = torch.cat([out, rel], dim=-1)
    return out


class NestedGINEffQm9Ref(torch.nn.Module):
    """Same module tree / state_dict keys (and construction order: the seeded init matches) as qm9_models.py:26-90."""

    def __init__(self, num_layers, num_features=NUM_FEATURES, edge_attr_dim=5, hidden=256):
        super().__init__()
        self.z_initial = torch.nn.Embedding(1800, hidden)
        self.z_embedding = Sequential(Dropout(0.0), BatchNorm1d(hidden), torch.nn.ReLU(), Linear(hidden, hidden),
                                      Dropout(0.0), BatchNorm1d(hidden), torch.nn.ReLU())
        input_dim = num_features + 3
        self.conv1 = rm.GINEConv(rm._mlp(input_dim, hidden, 0.0), train_eps=True, edge_dim=hidden + edge_attr_dim)
        self.convs = torch.nn.ModuleList([rm.GINEConv(rm._mlp(hidden, hidden, 0.0), train_eps=True,
                                                      edge_dim=hidden + edge_attr_dim) for _ in range(num_layers - 1)])
        self.lin1 = Linear(num_layers * hidden, hidden)
        self.bn_lin1 = BatchNorm1d(hidden, eps=1e-5, momentum=0.1)
        self.lin2 = Linear(hidden, 1)
        self.node_type_embedding = torch.nn.Embedding(5, input_dim)

    def forward(self, x, pos, node_type, edge_index, edge_attr, pos_enc, pos_index, pos_batch, batch):
        h = torch.cat([x, pos], 1) + self.node_type_embedding(node_type)
        z = rm.global_add_pool(self.z_initial.weight[pos_index] * pos_enc.view(-1, 1), pos_batch)
        z = torch.cat((self.z_embedding(z), edge_attr), dim=-1)
        h = self.conv1(h, edge_index, z)
        xs = [h]
        for conv in self.convs:
            h = conv(h, edge_index, z)
            xs.append(h)
        o = rm.global_mean_pool(torch.cat(xs, dim=1), batch)
        o = self.lin1(o)
        if o.size(0) > 1:
            o = self.bn_lin1(o)
        return self.lin2(F.relu(o)).view(-1)


def perturb(m):
    """0.1 * randn on every 1-d non-bias parameter (BatchNorm weights, eps), so that each one matters"""
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1 and "bias" not in name:
                p.add_(0.1 * torch.randn_like(p))
    return m


def qm9_oracle_from_recipe(z):
    """the golden's parameters: seeded construction, then `perturb`"""
    torch.manual_seed(int(z["seed"]))
    return perturb(NestedGINEffQm9Ref(int(z["layers"])))


def qm9_batch_inputs(num_nodes, num_edges, num_graphs, seed):
    """seeded QM9-shaped inputs for a collated batch: x [N, 8] (atomic number, six binary columns, a small count),
    pos [N, 3], node_type [N] in [0, 5), edge_attr [E, 5] (bond one-hot + a distance in [0, 1]), y [G]"""
    rng = np.random.RandomState(seed)
    node_type = rng.randint(0, 5, size=num_nodes)
    x = np.zeros((num_nodes, NUM_FEATURES), dtype=np.float32)
    x[:, 0] = np.array([1, 6, 7, 8, 9])[node_type]
    x[:, 1:7] = rng.randint(0, 2, size=(num_nodes, 6))
    x[:, 7] = rng.randint(0, 4, size=num_nodes)
    pos = rng.randn(num_nodes, 3).astype(np.float32) * 1.5
    ea = np.zeros((num_edges, 5), dtype=np.float32)
    ea[np.arange(num_edges), rng.randint(0, 4, size=num_edges)] = 1.0
    ea[:, 4] = rng.rand(num_edges).astype(np.float32)
    y = rng.randn(num_graphs).astype(np.float32)
    return dict(x=torch.tensor(x), pos=torch.tensor(pos), node_type=torch.tensor(node_type, dtype=torch.int64),
                edge_attr=torch.tensor(ea), y=torch.tensor(y))


def model_args(b):
    return (b["x"], b["pos"], b["node_type"], b["edge_index"], b["edge_attr"], b["pos_enc"], b["pos_index"], b["pos_batch"],
            b["batch"])
