"""Oracle helpers of the CSL run (test infrastructure, CPU only).

* NestedGINCslRef: the NestedGIN class that run_csl.py:145-225 defines inline, restated on the oracle primitives
  (oracle/ref_model.py) with torch's ELU.  The head's dropout is taken as an argument: `drop` is the multiplier F.dropout
  applies (0 or 1 / (1 - p) = 2 per element), so a mask drawn anywhere can be replayed here.  Returns raw logits.
* csl_oracle_from_recipe: the golden's parameters from its seed recipe.
* fixture_graphs: the 20 graphs of tests/golden/model_csl.npz — every class as its identity copy plus one relabelled copy,
  the ten permutations drawn in class order from np.random.RandomState(7).  Built here in plain numpy, independently of
  esc_gnn_amd.datasets.csl_graphs.
* cpu_features: create_subgraphs(g, h, use_rd=True, self_loop=True) on the CPU oracle (oracle/ref_features.py);
  feature_multiset: a relabelling-invariant signature of one graph's ESC features.
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F
from torch.nn import BatchNorm1d, ELU, Linear, Sequential

import ref_model as rm
from expressive_oracle import FEATURE_KEYS, collate, digest, grad_digest, graph_digests  # noqa: F401  (shared helpers)

NUM_NODES, SKIPS, PERM_SEED, NUM_CLASSES = 41, (2, 3, 4, 5, 6, 9, 11, 12, 13, 16), 7, 10


def _conv(n_in, hidden):
    return rm.GINEConv(Sequential(Linear(n_in, hidden), ELU(), Linear(hidden, hidden), ELU()), train_eps=False,
                       edge_dim=hidden)


class NestedGINCslRef(torch.nn.Module):
    """Same module tree, construction order and state_dict keys as the reference class.  As in the reference's forward
    (run_csl.py:194-222), z_embedding is constructed, reset and carried in the state_dict but never applied: the bag output
    feeds the convolutions directly, and its parameters receive no gradient."""

    def __init__(self, num_layers, hidden):
        super().__init__()
        self.conv1 = _conv(1, hidden)
        self.convs = torch.nn.ModuleList([_conv(hidden, hidden) for _ in range(num_layers - 1)])
        self.lin1 = Linear(hidden, hidden)
        self.lin2 = Linear(hidden, NUM_CLASSES)
        self.z_initial = torch.nn.Embedding(1800, hidden)
        self.z_embedding = Sequential(BatchNorm1d(hidden), ELU(), Linear(hidden, hidden), BatchNorm1d(hidden), ELU())

    def reset_parameters(self):
        self.conv1.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        for layer in self.z_embedding.children():
            if hasattr(layer, "reset_parameters"):
                layer.reset_parameters()
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()

    def forward(self, x, edge_index, pos_enc, pos_index, pos_batch, batch, drop=None):
        z = rm.global_add_pool(self.z_initial.weight[pos_index] * pos_enc.view(-1, 1), pos_batch)
        h = self.conv1(x, edge_index, z)
        for conv in self.convs:
            h = conv(h, edge_index, z)
        h = rm.global_add_pool(h, batch)
        h = F.elu(self.lin1(h))
        if self.training:
            h = h * drop.to(h.dtype)
        return self.lin2(h)


def csl_oracle_from_recipe(z):
    """torch.manual_seed(seed) BEFORE construction, then reset_parameters() — the recipe of the golden"""
    torch.manual_seed(int(z["seed"]))
    m = NestedGINCslRef(int(z["layers"]), int(z["hidden"]))
    m.reset_parameters()
    return m


def csl_edges(n, skip, perm=None):
    """int64 [2, 4n]: cycle + skip links, node i renamed perm[i], both directions, sorted by (src, dst)"""
    i = np.arange(n)
    a = np.concatenate([i, i])
    b = np.concatenate([(i + 1) % n, (i + skip) % n])
    if perm is not None:
        a, b = perm[a], perm[b]
    both = sorted(set(zip(a.tolist(), b.tolist())) | set(zip(b.tolist(), a.tolist())))
    return np.array(both, dtype=np.int64).T


def fixture_graphs():
    """20 product `Data` graphs, class by class: [identity copy, relabelled copy] x 10; y = int64 [1]"""
    from esc_gnn_amd import Data
    rng = np.random.RandomState(PERM_SEED)
    out = []
    for k, skip in enumerate(SKIPS):
        for perm in (None, rng.permutation(NUM_NODES)):
            out.append(Data(x=torch.ones(NUM_NODES, 1), edge_index=torch.tensor(csl_edges(NUM_NODES, skip, perm)),
                            y=torch.tensor([k], dtype=torch.int64), num_nodes=NUM_NODES))
    return out


def cpu_features(raw, h=4):
    """create_subgraphs(g, h, use_rd=True, self_loop=True) of product `Data` graphs on the CPU oracle"""
    import ref_features as orc
    from esc_gnn_amd import Data
    out = []
    for d in raw:
        ei = d.edge_index.numpy()
        e = orc.encode_graph(ei[0], ei[1], int(d.x.size(0)), h, True, True)
        out.append(Data(x=d.x, edge_index=torch.tensor(np.stack([e["edge_src"], e["edge_dst"]])), y=d.y,
                        pos_enc=torch.tensor(e["pos_enc"]), pos_index=torch.tensor(e["pos_index"]),
                        pos_batch=torch.tensor(e["pos_batch"])))
    return out


def feature_multiset(g):
    """Counter over the edge rows of one graph of the row's sorted (pos_index, pos_enc) entries, keyed with whether the row
    is a self loop: equal for two relabellings of one graph"""
    idx, enc, seg = (g[k].numpy() for k in ("pos_index", "pos_enc", "pos_batch"))
    ei = g["edge_index"].numpy()
    rows = collections.defaultdict(list)
    for i, v, s in zip(idx.tolist(), enc.tolist(), seg.tolist()):
        rows[s].append((i, v))
    return collections.Counter((bool(ei[0, s] == ei[1, s]), tuple(sorted(r))) for s, r in rows.items())


def distance_matrix(pred):
    """[G, G] Euclidean distances in fp64, difference form (no cancellation between near-equal rows); the squares are added
    column by column with elementwise operations only, so the bits do not depend on how a host vectorises a reduction"""
    p = pred.double()
    d2 = torch.zeros(p.size(0), p.size(0), dtype=torch.float64)
    for c in range(p.size(1)):
        diff = p[:, None, c] - p[None, :, c]
        d2 = d2 + diff * diff
    return d2.sqrt()


def class_distances(pred):
    """(smallest distance between graphs of different classes, largest between the two copies of a class) of [20, C] rows
    ordered as fixture_graphs()"""
    d = distance_matrix(pred)
    cls = torch.arange(pred.size(0)) // 2
    same = cls.view(-1, 1) == cls.view(1, -1)
    return float(d[~same].min()), float(d[same].max())
