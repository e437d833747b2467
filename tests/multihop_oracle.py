"""Oracle of the GINE+ baseline's new ground (TEST INFRASTRUCTURE, numpy / CPU torch only):

* multihop_graph / multihop_batch — the multi-hop edges of modules/gine_operations.py:256-303 restated as one bounded BFS per
  node over the out-edges: {(i, i) at 0} u {(i, j) at d(i -> j), 1 <= d <= k}, sorted by (row, col); a batch without any edge
  has no pairs at all.  tools/make_golden_multihop.py checks it bit for bit against the reference's matrix powers + coalesce.
* hand_cases — the hand-made graphs of tests/golden/multihop_edges.npz.
* aggregate64 — the GINE+ aggregate (what GINEPLUS / NAIVEGINEPLUS compute before self.nn) in fp64 with autograd.
* RefNet — the network of modules/gine_operations.py:23-253 (conv_type 'gin+' / 'naivegin+') on plain torch.nn, with the
  reference's module nesting and state_dict keys; the golden tool asserts that it equals the reference's own class bodies bit
  for bit (outputs, gradients, buffers) before it records anything, and the fixture pins it with the reference's predictions
  and a digest per gradient.
* fill_params — seed-free deterministic parameters (an integer hash of the key and the position), so that no fixture stores
  weights.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ATOM_DIMS = (119, 5, 12, 12, 10, 6, 6, 2, 2)
BOND_DIMS = (5, 6, 2)
CONFIGS = [(layers, vn) for layers in (1, 2, 4) for vn in (False, True)]
HIDDEN, OUT_DIM, K = 32, 2, 3
NET_MOLECULES = 8            # the batch of model_gineplus_net.npz (tools/make_golden_multihop.py says why not 3)


# ---- multi-hop edges ------------------------------------------------------------------------------------------------------
def multihop_graph(n, src, dst, k):
    """(row, col, distance) int64 of one graph, sorted by (row, col)"""
    adj = [set() for _ in range(n)]
    for s, t in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        adj[s].add(t)
    rows, cols, dist = [], [], []
    for r in range(n):
        hop = {r: 0}
        frontier = [r]
        for d in range(1, k + 1):
            nxt = []
            for u in frontier:
                for v in adj[u]:
                    if v not in hop:
                        hop[v] = d
                        nxt.append(v)
            frontier = nxt
            if not frontier:
                break
        for j in sorted(hop):
            rows.append(r); cols.append(j); dist.append(hop[j])
    return np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(dist, dtype=np.int64)


def multihop_batch(ns, eis, k):
    """(multihop_edge_index [2, M], distance [M]) of the collated batch of graphs (ns[g] nodes, eis[g] = [2, E_g] local ids)"""
    if sum(int(np.asarray(e).shape[1]) for e in eis) == 0:
        return np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64)
    rows, cols, dist, off = [], [], [], 0
    for n, ei in zip(ns, eis):
        ei = np.asarray(ei).reshape(2, -1)
        r, c, d = multihop_graph(n, ei[0], ei[1], k)
        rows.append(r + off); cols.append(c + off); dist.append(d)
        off += n
    return np.stack([np.concatenate(rows), np.concatenate(cols)]), np.concatenate(dist)


def _und(pairs):
    e = sorted(set(pairs) | {(b, a) for a, b in pairs})
    return np.array(e, dtype=np.int64).T.reshape(2, -1)


def _dir(pairs):
    return np.array(pairs, dtype=np.int64).T.reshape(2, -1)


def hand_cases():
    """(name, [(n, edge_index), ...], ks): every case is a batch of one or more graphs"""
    ks = (1, 2, 3, 4)
    none = np.zeros((2, 0), dtype=np.int64)
    star = _und([(0, i) for i in range(1, 201)])
    out = [
        ("single_edge", [(2, _dir([(0, 1)]))], ks),
        ("path6", [(6, _und([(i, i + 1) for i in range(5)]))], ks),
        ("triangle", [(3, _und([(0, 1), (1, 2), (0, 2)]))], ks),                  # k larger than the diameter from k = 2 on
        ("directed_chain", [(5, _dir([(i, i + 1) for i in range(4)]))], ks),
        ("directed_2cycle", [(2, _dir([(0, 1), (1, 0)]))], ks),
        ("selfloops_repeats", [(3, _dir([(0, 0), (0, 1), (0, 1), (1, 2), (2, 2), (2, 0), (0, 1)]))], ks),
        ("isolated_in_batch", [(4, _und([(0, 1), (1, 2)])), (1, none), (3, _dir([(2, 0)]))], ks),
        ("two_components", [(7, _und([(0, 1), (1, 2), (3, 4), (4, 5), (5, 6)]))], ks),
        ("star200", [(201, star)], (2,)),                                          # every row holds 201 pairs: more than one wave
        ("ring65", [(65, _und([(i, (i + 1) % 65) for i in range(65)]))], ks),       # rows and columns across the 64-lane boundary
        ("ring129", [(129, _und([(i, (i + 1) % 129) for i in range(129)]))], ks),
    ]
    return out


# ---- the aggregate in fp64 ------------------------------------------------------------------------------------------------
def aggregate64(xs, e, eps, mei, dist, k):
    """out = (1+eps[0]) xs[0] + sum_d (1+eps[d]) sum_{pairs at distance d} relu(xs[d-1][row] + [d=1] e), at the column; torch
    fp64 tensors (autograd gives the gradients); the rows of e follow the order of the distance-1 pairs in mei"""
    out = (1 + eps[0]) * xs[0]
    for d in range(1, k + 1):
        keep = dist == d
        row, col = mei[0][keep], mei[1][keep]
        msg = xs[d - 1][row]
        if d == 1:
            msg = msg + e
        out = out + (1 + eps[d]) * torch.zeros_like(xs[0]).index_add_(0, col, F.relu(msg))
    return out


# ---- the network on plain torch.nn ---------------------------------------------------------------------------------------
def global_add_pool(x, batch, size=None):
    size = int(batch.max()) + 1 if size is None else size
    return torch.zeros((size, x.size(1)), dtype=x.dtype).index_add_(0, batch, x)


def global_mean_pool(x, batch, size=None):
    size = int(batch.max()) + 1 if size is None else size
    cnt = torch.zeros(size, dtype=x.dtype).index_add_(0, batch, torch.ones(x.size(0), dtype=x.dtype))
    return global_add_pool(x, batch, size) / cnt.clamp(min=1).unsqueeze(1)


class _Encoder(nn.Module):
    """ogb's AtomEncoder / BondEncoder: the sum over the feature columns of one xavier-initialised table per column"""

    def __init__(self, dims, emb_dim, attr):
        super().__init__()
        tables = nn.ModuleList()
        for d in dims:
            emb = nn.Embedding(d, emb_dim)
            nn.init.xavier_uniform_(emb.weight.data)
            tables.append(emb)
        setattr(self, attr, tables)
        self._attr = attr

    def forward(self, x):
        out = 0
        for i, t in enumerate(getattr(self, self._attr)):
            out = out + t(x[:, i])
        return out


class AtomEncoder(_Encoder):
    def __init__(self, emb_dim):
        super().__init__(ATOM_DIMS, emb_dim, "atom_embedding_list")


class BondEncoder(_Encoder):
    def __init__(self, emb_dim):
        super().__init__(BOND_DIMS, emb_dim, "bond_embedding_list")


class _MLP(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.main = nn.Sequential(nn.Linear(dim, 2 * dim), nn.BatchNorm1d(2 * dim), nn.ReLU(), nn.Linear(2 * dim, dim))

    def forward(self, x):
        return self.main(x)


class _Conv(nn.Module):
    def __init__(self, dim, k, naive):
        super().__init__()
        self.k, self.naive = k, naive
        self.nn = _MLP(dim)
        self.eps = nn.Parameter(torch.zeros(k + 1, dim))

    def forward(self, XX, mei, dist, ea):
        xs = [XX] * self.k if self.naive else XX
        result = (1 + self.eps[0]) * xs[0]
        for i in range(self.k):
            ei = mei[:, dist == i + 1]
            msg = xs[i].index_select(0, ei[0])
            msg = F.relu(msg + ea) if i == 0 else F.relu(msg)
            result += (1 + self.eps[i + 1]) * torch.zeros_like(xs[i]).index_add_(0, ei[1], msg)
        result = self.nn(result)
        return result if self.naive else [result] + XX


class _VNAgg(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.mlp = nn.Sequential(_MLP(dim), nn.BatchNorm1d(dim), nn.ReLU())

    def forward(self, v, h, b):
        return self.mlp(v + global_add_pool(h, b))


class _Block(nn.Module):
    def __init__(self, dim, k, naive, virtual_node, agg, last):
        super().__init__()
        self.edge_embed = BondEncoder(dim)
        self.conv = _Conv(dim, k, naive)
        self.norm = nn.BatchNorm1d(dim)
        self.naive, self.virtual_node, self.agg, self.last = naive, virtual_node, agg, last
        if virtual_node and agg:
            self.vn_aggregator = _VNAgg(dim)

    def forward(self, st):
        h = st["x"]
        if self.virtual_node:
            if self.naive:
                h = h + st["v"][st["batch"]]
            else:
                h[0] = h[0] + st["v"][st["batch"]]
        H = self.conv(h, st["mei"], st["dist"], self.edge_embed(st["edge_attr"]))
        h = H if self.naive else H[0]
        h = self.norm(h)
        if not self.last:
            h = F.relu(h)
        if self.virtual_node and self.agg:
            st["v"] = self.vn_aggregator(st["v"], h, st["batch"])
        if not self.naive:
            H[0] = h
            h = H
        st["x"] = h
        return st


class _Embed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.atom_embedding = AtomEncoder(dim)


class RefNet(nn.Module):
    """ClassifierNetwork(hidden, out_dim, layers, dropout=0, virtual_node, k, conv_type) at dropout 0"""

    def __init__(self, hidden, out_dim, layers, virtual_node, k, conv_type="gin+"):
        super().__init__()
        naive = conv_type == "naivegin+"
        self.naive, self.k = naive, k
        blocks = [_Block(hidden, min(i + 1, k), naive, virtual_node, True, False) for i in range(layers - 1)]
        blocks.append(_Block(hidden, min(layers, k), naive, virtual_node, False, True))
        self.main = nn.Sequential(_Embed(hidden), *blocks)
        self.aggregate = nn.Sequential(nn.Identity(), nn.Linear(hidden, out_dim))
        self.virtual_node = virtual_node
        if virtual_node:
            self.v0 = nn.Parameter(torch.zeros(1, hidden))

    def forward(self, x, edge_attr, batch, mei, dist, num_graphs):
        h = self.main[0].atom_embedding(x)
        st = dict(x=h if self.naive else [h], edge_attr=edge_attr, batch=batch, mei=mei, dist=dist)
        if self.virtual_node:
            st["v"] = self.v0.expand(num_graphs, self.v0.shape[-1])
        for blk in list(self.main)[1:]:
            st = blk(st)
        h = st["x"] if self.naive else st["x"][0]
        return self.aggregate[1](global_mean_pool(h, batch, num_graphs))


def fill_params(model):
    """every parameter and buffer from an integer hash of (key, position): exact in fp32 on every platform"""
    with torch.no_grad():
        for key, t in model.state_dict().items():
            if key.endswith("num_batches_tracked"):
                t.zero_()
                continue
            n = t.numel()
            idx = np.arange(n, dtype=np.uint64)
            hsh = (idx * np.uint64(2654435761) + np.uint64(zlib.crc32(key.encode()))) % np.uint64(1 << 32)
            v = ((hsh >> np.uint64(16)).astype(np.float32) / np.float32(65536.0) - np.float32(0.5)).reshape(tuple(t.shape))
            if key.endswith("running_var"):
                a = np.float32(1.0) + np.float32(0.5) * v
            elif key.endswith("running_mean"):
                a = np.float32(0.2) * v
            elif t.dim() == 1 and key.endswith("weight"):                    # BatchNorm gamma
                a = np.float32(1.0) + np.float32(0.4) * v
            elif t.dim() == 1:                                               # biases
                a = np.float32(0.4) * v
            elif key.endswith("eps") or key == "v0":
                a = np.float32(0.6) * v
            else:                                                            # Linear weights and embedding tables
                a = np.float32(2.0 / math.sqrt(t.shape[1])) * v
            t.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return model


def loss_weights(G, out_dim):
    idx = np.arange(G * out_dim, dtype=np.float32).reshape(G, out_dim)
    return torch.from_numpy((idx % np.float32(5.0) - np.float32(2.0)) / np.float32(4.0))


def digest(t):
    t = t.detach().double()
    return np.array([float(t.sum()), float(t.abs().sum())])
