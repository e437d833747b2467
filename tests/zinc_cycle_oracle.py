"""Oracle helpers of the ZINC cycle-counting feature (test infrastructure, CPU only).

* cycle_labels: the reference's dataset_zinc_cycle.py:45-61 (pkl2data) restated — remove_self_loops, to_undirected,
  to_networkx (a DiGraph with both directions), networkx.simple_cycles, cycles of length 3..6, +1 per node, halved.
* NestedGINEffZincCycleRef: zinc_cycle_models.py:506-613 on the oracle primitives — the ZINC composition of
  oracle/ref_model.NestedGINEffZincRef without global_add_pool (lin1 / bn_lin1 / lin2 on the node rows).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import ref_model as rm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def cycle_labels(n, edge_index):
    """float32 [n, 4]: undirected simple 3-, 4-, 5- and 6-cycles through every node (networkx)"""
    import networkx as nx
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    pairs = {(int(a), int(b)) for a, b in ei.T if a != b}            # remove_self_loops
    pairs |= {(b, a) for a, b in pairs}                               # to_undirected (coalesced: a set)
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_edges_from(sorted(pairs))
    out = np.zeros((n, 4), dtype=np.float32)
    for c in nx.simple_cycles(G, length_bound=6):
        if 3 <= len(c) <= 6:
            out[c, len(c) - 3] += 1
    return out / 2


def batch_cycle_labels(edge_index, batch):
    """cycle_labels of every graph of a collated batch (global node ids, `batch` sorted by graph): [N, 4]"""
    b = np.asarray(batch, dtype=np.int64)
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(b))])
    out = []
    for g in range(len(ptr) - 1):
        lo, hi = ptr[g], ptr[g + 1]
        keep = (ei[0] >= lo) & (ei[0] < hi)
        out.append(cycle_labels(hi - lo, ei[:, keep] - lo))
    return np.concatenate(out, axis=0)


class NestedGINEffZincCycleRef(rm.NestedGINEffZincRef):
    """zinc_cycle_models.py:506-613: the ZINC model with a node-level readout.  Same state_dict keys."""

    def forward(self, x, edge_index, edge_attr, pos_enc, pos_index, pos_batch, batch):
        h = self.node_type_embedding(x)
        z = rm.global_add_pool(self.z_initial.weight[pos_index] * pos_enc.view(-1, 1), pos_batch)
        z = torch.cat((self.z_embedding(z), self.edge_type_embedding(edge_attr)), dim=-1)
        h = self.conv1(h, edge_index, z)
        xs = [h]
        for conv in self.convs:
            h = conv(h, edge_index, z)
            xs.append(h)
        o = self.lin1(torch.cat(xs, dim=1))
        if o.size(0) > 1:
            o = self.bn_lin1(o)
        return self.lin2(F.elu(o))


def zinc_cycle_oracle_from_recipe(z):
    """the golden's parameters: seeded construction, then 0.1 * randn on every 1-d non-bias parameter"""
    torch.manual_seed(int(z["seed"]))
    m = NestedGINEffZincCycleRef(int(z["layers"]))
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1 and "bias" not in name:
                p.add_(0.1 * torch.randn_like(p))
    return m
