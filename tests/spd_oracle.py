"""Plain restatement of the shortest-path attention bias, the oracle of tests/test_spd_cpu.py and tests/test_hip_spd.py: the
all-pairs distances by breadth-first search (held equal to networkx's, the reference's path, by the CPU test), the ragged
biased attention with an explicit keep mask in its per-pair form (embedding lookup, MLP) and in its table form, the padded
torch.nn.MultiheadAttention with the float attn_mask built the reference's way, and GPSLayer / GPSModel with the bias on
(gps_oracle's classes with the attention branch replaced).  CPU, any dtype; imports nothing from the package under test."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import gps_oracle as go

NO_PATH = 100          # the reference's fill for a pair without a path, and the padding row of Embedding(101, heads, padding_idx=100)
ROWS = 101
MAX_NODES = 256        # esc_graph_spd_max_nodes()


# ---- graphs -----------------------------------------------------------------------------------------------------------------------
def _e(pairs):
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T.copy()


def _both(pairs):
    return _e([p for a, b in pairs for p in ((a, b), (b, a))])


def _path(n):
    return [(i, i + 1) for i in range(n - 1)]


def _random_sparse(n, seed, extra):
    """a random forest, one tree per block of 29 nodes, plus `extra` chords inside the blocks, both directions: long distances
    and several components"""
    rng = np.random.RandomState(seed)
    pairs = [(int(rng.randint(max(v - v % 29, v - 6), v)), v) for v in range(1, n) if v % 29]      # v % 29 == 0 starts a new component
    for a in rng.randint(0, n, size=extra):
        lo = int(a) - int(a) % 29
        pairs.append((int(a), lo + int(rng.randint(0, min(29, n - lo)))))
    return _both(pairs)


GRAPHS = [  # (name, n, edges [2, m] int64)
    ("one-node", 1, _e([])),
    ("two-isolated", 2, _e([])),
    ("path-5", 5, _both(_path(5))),
    ("cycle-6-chord", 6, _both([(i, (i + 1) % 6) for i in range(6)] + [(0, 3)])),
    ("two-components-7", 7, _both([(0, 1), (1, 2), (2, 0), (3, 4), (4, 5), (5, 6)])),
    ("loops-and-duplicates", 5, _e([(0, 0), (0, 1), (1, 0), (0, 1), (1, 2), (2, 1), (2, 2), (1, 2), (3, 3)])),
    ("one-direction-only", 6, _e([(1, 0), (1, 2), (3, 2), (3, 4)])),
    ("path-104", 104, _both(_path(104))),
]
DEVICE_GRAPHS = [  # what only the GPU test adds: the word-count boundaries and the node limit
    ("random-64", 64, _random_sparse(64, 1, 8)),
    ("random-65", 65, _random_sparse(65, 2, 8)),
    ("random-129", 129, _random_sparse(129, 3, 12)),
    ("random-256", MAX_NODES, _random_sparse(MAX_NODES, 4, 20)),
]
NAMES = [g[0] for g in GRAPHS]


def spd_bfs(n, edges):
    """uint8 [n, n]: min(d, 100) on the undirected graph, 100 where there is no path"""
    nbr = [set() for _ in range(n)]
    for a, b in edges.T.tolist():
        nbr[a].add(b)
        nbr[b].add(a)
    out = np.full((n, n), NO_PATH, dtype=np.int64)
    for s in range(n):
        out[s, s] = 0
        frontier, seen, d = [s], {s}, 0
        while frontier:
            d += 1
            nxt = []
            for v in frontier:
                for w in nbr[v]:
                    if w not in seen:
                        seen.add(w)
                        out[s, w] = d
                        nxt.append(w)
            frontier = nxt
    return np.minimum(out, NO_PATH).astype(np.uint8)


def spd_networkx(n, edges):
    """int64 [n, n] filled as GraphGPS/graphgps/loader/utils_escgnn.py:29-38 fills it from nx.all_pairs_shortest_path_length, on
    the undirected graph in which an edge listed in either direction connects both ends (for the symmetric edge lists of the
    reference's datasets that is the graph its to_networkx(..., to_undirected=True) builds)"""
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(edges.T.tolist())
    SPT = dict(nx.all_pairs_shortest_path_length(G))
    out = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            out[i, j] = SPT[i][j] if j in SPT[i] else NO_PATH
    return out


def collate(graphs):
    """(edge_index [2, E] of batch rows, sizes, flat spd bytes) of a list of (name, n, edges)"""
    ei, o = [], 0
    for _, n, e in graphs:
        ei.append(e + o)
        o += n
    flat = np.concatenate([spd_bfs(n, e).reshape(-1) for _, n, e in graphs]) if graphs else np.zeros(0, np.uint8)
    return np.concatenate(ei, 1) if ei else np.zeros((2, 0), np.int64), [g[1] for g in graphs], flat


def split_spd(flat, sizes):
    """flat bytes (tensor or array) -> one [n, n] long tensor per graph"""
    flat = torch.as_tensor(flat).reshape(-1).long()
    out, o = [], 0
    for n in sizes:
        out.append(flat[o:o + n * n].reshape(n, n))
        o += n * n
    return out


# ---- the bias ---------------------------------------------------------------------------------------------------------------------
def make_bias_modules(heads, dtype=torch.float64):
    emb = torch.nn.Embedding(ROWS, heads, padding_idx=NO_PATH)
    mlp = torch.nn.Sequential(torch.nn.Linear(heads, heads), torch.nn.ReLU(), torch.nn.Linear(heads, heads), torch.nn.ReLU(),
                              torch.nn.Linear(heads, heads))
    return emb.to(dtype), mlp.to(dtype)


def bias_table(emb, mlp):
    """[101, heads]: the MLP of every row of the embedding, through the lookup (padding_idx keeps row 100's gradient zero)"""
    return mlp(emb(torch.arange(ROWS)))


def pair_bias(emb, mlp, spd):
    """the reference's order for one graph: lookup per pair, MLP over [n, n, heads] -> [heads, n, n]"""
    return mlp(emb(spd.clamp(max=NO_PATH))).permute(2, 0, 1)


def ragged_biased_attention(qkv, sizes, heads, bias, keep=None, p=0.0):
    """gps_oracle.ragged_attention with bias[g] [heads, n, n] added to the scores"""
    N, H = qkv.size(0), qkv.size(1) // 3
    d = H // heads
    outs, lses, o = [], [], 0
    for g, n in enumerate(sizes):
        rows = qkv[o:o + n]
        q, k, v = (rows[:, t * H:(t + 1) * H].reshape(n, heads, d).transpose(0, 1) for t in range(3))
        s = q @ k.transpose(1, 2) / math.sqrt(d) + bias[g]
        lse = torch.logsumexp(s, dim=2) if n else s.new_zeros((heads, 0))
        pr = torch.softmax(s, dim=2)
        if keep is not None:
            pr = pr * keep[g].to(pr.dtype) / (1.0 - p)
        outs.append((pr @ v).transpose(0, 1).reshape(n, H))
        lses.append(lse)
        o += n
    assert o == N
    return torch.cat(outs, 0), torch.cat(lses, 1)


def table_bias(table, spds):
    """the table form: bias[g][a, i, j] = table[min(spd_ij, 100), a]"""
    return [table[s.clamp(max=NO_PATH)].permute(2, 0, 1) for s in spds]


def padded_biased_attention(mha, emb, mlp, x, sizes, spds):
    """what the reference runs under BiasedTransformer (gps_layer.py:234-239,269-286): to_dense_batch, attn_bias padded to
    [B, n_max, n_max] with the padding index, _sa_block's embedding -> MLP -> permute -> reshape as the float attn_mask, and
    key_padding_mask; gather back"""
    B, n_max, H = len(sizes), max(sizes), x.size(1)
    dense = x.new_zeros((B, n_max, H))
    valid = torch.zeros((B, n_max), dtype=torch.bool)
    attn_bias = torch.full((B, n_max, n_max), NO_PATH, dtype=torch.long)
    o = 0
    for g, n in enumerate(sizes):
        dense[g, :n] = x[o:o + n]
        valid[g, :n] = True
        attn_bias[g, :n, :n] = spds[g].clamp(max=NO_PATH)
        o += n
    attn_mask = emb(attn_bias)
    num_node = attn_mask.size(1)
    attn_mask = mlp(attn_mask)
    attn_mask = attn_mask.permute(0, 3, 1, 2).reshape(-1, num_node, num_node)
    return mha(dense, dense, dense, attn_mask=attn_mask, key_padding_mask=~valid, need_weights=False)[0][valid]


def ragged_biased_mha(mha, emb, mlp, x, sizes, spds):
    qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias)
    return mha.out_proj(ragged_biased_attention(qkv, sizes, mha.num_heads, table_bias(bias_table(emb, mlp), spds))[0])


# ---- the model ------------------------------------------------------------------------------------------------------------------
class GPSLayer(go.GPSLayer):
    """gps_oracle.GPSLayer under BiasedTransformer: the same modules, edge_attn_emb / edge_attn_linear in the forward"""

    def forward(self, h, edge_attr, b, sizes):
        w = self.z_initial.weight[b["pos_index"]] * b["pos_enc"].to(h.dtype).view(-1, 1)
        z = torch.zeros((edge_attr.size(0), h.size(1)), dtype=h.dtype).index_add_(0, b["pos_batch"], w)
        edge_attr = edge_attr + self.z_embedding(z)
        h_local = self.norm1_local(h + self.local_model(h, b["edge_index"], edge_attr))
        spds = split_spd(b["attn_bias"], sizes)
        h_attn = self.norm1_attn(h + ragged_biased_mha(self.self_attn, self.edge_attn_emb, self.edge_attn_linear, h, sizes, spds))
        h = h_local + h_attn
        h = h + self.ff_linear2(torch.relu(self.ff_linear1(h)))
        return self.norm2(h), edge_attr


class GPSModel(go.GPSModel):
    """forward(b): b as for gps_oracle.GPSModel plus attn_bias, the flat distance bytes"""

    def __init__(self, layers=10, dim_hidden=64, n_heads=4, dropout=0.0, attn_dropout=0.0, node_types=28, edge_types=4, dim_out=1):
        torch.nn.Module.__init__(self)
        self.encoder = go._Encoder(dim_hidden, node_types, edge_types)
        self.layers = torch.nn.Sequential(*[GPSLayer(dim_hidden, n_heads, dropout, attn_dropout) for _ in range(layers)])
        self.post_mp = go._Head(dim_hidden, dim_out)
