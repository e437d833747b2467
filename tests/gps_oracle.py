"""Plain-torch restatement of the graph transformer, the oracle of tests/test_gps_cpu.py and tests/test_hip_gps.py: the ragged
multi-head attention with an explicit keep mask, GPSLayer / GPSModel built from torch.nn modules with the state_dict key layout of
the reference's classes, and the lambda of the cosine schedule with warm-up.  Runs on the CPU in whatever dtype it is given (the
tests use fp64); differentiable through autograd.  Imports nothing from the package under test."""
import math

import torch
import torch.nn.functional as F

Z_TABLE_ROWS = 1800


def graph_ptr_of(sizes):
    out = [0]
    for n in sizes:
        out.append(out[-1] + int(n))
    return out


def unpack_mask(mask, sizes, heads):
    """the kernel's byte layout -> one [heads, n, n] tensor per graph: M of (graph g, head a) sits at
    a * total + pair_ptr[g] + i * n + j, total = sum of n^2"""
    total = sum(int(n) * int(n) for n in sizes)
    flat = mask.reshape(-1)[:heads * total].reshape(heads, total)
    out, o = [], 0
    for n in sizes:
        out.append(flat[:, o:o + n * n].reshape(heads, n, n))
        o += n * n
    return out


def ragged_attention(qkv, sizes, heads, keep=None, p=0.0):
    """qkv [N, 3H] = [q | k | v], head a at columns a*d.. of each third; per graph and head softmax(q k^T / sqrt(d)) (o keep /
    (1-p)) v.  keep: None or one [heads, n, n] tensor per graph.  Returns out [N, H] and lse [heads, N]."""
    N, H = qkv.size(0), qkv.size(1) // 3
    d = H // heads
    outs, lses, o = [], [], 0
    for g, n in enumerate(sizes):
        rows = qkv[o:o + n]
        q, k, v = (rows[:, t * H:(t + 1) * H].reshape(n, heads, d).transpose(0, 1) for t in range(3))     # [heads, n, d]
        s = q @ k.transpose(1, 2) / math.sqrt(d)
        lse = torch.logsumexp(s, dim=2) if n else s.new_zeros((heads, 0))
        pr = torch.softmax(s, dim=2)
        if keep is not None:
            pr = pr * keep[g].to(pr.dtype) / (1.0 - p)
        outs.append((pr @ v).transpose(0, 1).reshape(n, H))
        lses.append(lse)
        o += n
    assert o == N
    return torch.cat(outs, 0), torch.cat(lses, 1)


def padded_attention(mha, x, sizes):
    """what the reference runs: pad to [B, n_max, H], torch.nn.MultiheadAttention with key_padding_mask, gather back"""
    B, n_max, H = len(sizes), max(sizes), x.size(1)
    dense = x.new_zeros((B, n_max, H))
    valid = torch.zeros((B, n_max), dtype=torch.bool)
    o = 0
    for g, n in enumerate(sizes):
        dense[g, :n] = x[o:o + n]
        valid[g, :n] = True
        o += n
    return mha(dense, dense, dense, attn_mask=None, key_padding_mask=~valid, need_weights=False)[0][valid]


def ragged_mha(mha, x, sizes):
    """the same layer on the ragged rows: in_proj, ragged_attention, out_proj"""
    qkv = F.linear(x, mha.in_proj_weight, mha.in_proj_bias)
    return mha.out_proj(ragged_attention(qkv, sizes, mha.num_heads)[0])


def cosine_lambda(num_warmup_epochs, max_epoch):
    def factor(epoch):
        if epoch < num_warmup_epochs:
            return max(1e-6, float(epoch) / float(max(1, num_warmup_epochs)))
        progress = float(epoch - num_warmup_epochs) / float(max(1, max_epoch - num_warmup_epochs))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))
    return factor


class GINE(torch.nn.Module):
    """nn((1 + eps) x_i + sum_{j -> i} relu(x_j + e_ji)) with a constant eps = 0 kept as a buffer"""

    def __init__(self, nn):
        super().__init__()
        self.nn = nn
        self.register_buffer("eps", torch.Tensor([0.0]))

    def forward(self, x, edge_index, edge_attr):
        msg = torch.relu(x[edge_index[0]] + edge_attr)
        return self.nn((1.0 + self.eps) * x + torch.zeros_like(x).index_add_(0, edge_index[1], msg))


class GPSLayer(torch.nn.Module):
    def __init__(self, dim_h, num_heads, dropout=0.0, attn_dropout=0.0):
        super().__init__()
        nn = torch.nn
        assert dropout == 0.0 and attn_dropout == 0.0, "the oracle models run without dropout"
        self.local_model = GINE(nn.Sequential(nn.Linear(dim_h, dim_h), nn.ReLU(), nn.Linear(dim_h, dim_h)))
        self.edge_attn_emb = nn.Embedding(101, num_heads, padding_idx=100)
        self.edge_attn_linear = nn.Sequential(nn.Linear(num_heads, num_heads), nn.ReLU(), nn.Linear(num_heads, num_heads), nn.ReLU(),
                                              nn.Linear(num_heads, num_heads))
        self.self_attn = nn.MultiheadAttention(dim_h, num_heads, dropout=attn_dropout, batch_first=True)
        self.norm1_local = nn.BatchNorm1d(dim_h)
        self.norm1_attn = nn.BatchNorm1d(dim_h)
        self.dropout_local = nn.Dropout(dropout)
        self.dropout_attn = nn.Dropout(dropout)
        self.ff_linear1 = nn.Linear(dim_h, dim_h * 2)
        self.ff_linear2 = nn.Linear(dim_h * 2, dim_h)
        self.act_fn_ff = nn.ReLU()
        self.norm2 = nn.BatchNorm1d(dim_h)
        self.ff_dropout1 = nn.Dropout(dropout)
        self.ff_dropout2 = nn.Dropout(dropout)
        self.z_initial = nn.Embedding(Z_TABLE_ROWS, dim_h)
        self.z_embedding = nn.Sequential(nn.Dropout(dropout), nn.BatchNorm1d(dim_h), nn.ELU(), nn.Linear(dim_h, dim_h), nn.Dropout(dropout),
                                         nn.BatchNorm1d(dim_h), nn.ELU())

    def forward(self, h, edge_attr, b, sizes):
        w = self.z_initial.weight[b["pos_index"]] * b["pos_enc"].to(h.dtype).view(-1, 1)
        z = torch.zeros((edge_attr.size(0), h.size(1)), dtype=h.dtype).index_add_(0, b["pos_batch"], w)
        edge_attr = edge_attr + self.z_embedding(z)
        h_local = self.norm1_local(h + self.local_model(h, b["edge_index"], edge_attr))
        h_attn = self.norm1_attn(h + ragged_mha(self.self_attn, h, sizes))
        h = h_local + h_attn
        h = h + self.ff_linear2(torch.relu(self.ff_linear1(h)))
        return self.norm2(h), edge_attr


class _TypeDict(torch.nn.Module):
    def __init__(self, num_types, dim):
        super().__init__()
        self.encoder = torch.nn.Embedding(num_types, dim)


class _Encoder(torch.nn.Module):
    def __init__(self, dim, node_types, edge_types):
        super().__init__()
        self.node_encoder = _TypeDict(node_types, dim)
        self.edge_encoder = _TypeDict(edge_types, dim)


class _Head(torch.nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.FC_layers = torch.nn.ModuleList([torch.nn.Linear(dim_in, dim_in // 2), torch.nn.Linear(dim_in // 2, dim_in // 4),
                                              torch.nn.Linear(dim_in // 4, dim_out)])


class GPSModel(torch.nn.Module):
    def __init__(self, layers=10, dim_hidden=64, n_heads=4, dropout=0.0, attn_dropout=0.0, node_types=28, edge_types=4, dim_out=1):
        super().__init__()
        self.encoder = _Encoder(dim_hidden, node_types, edge_types)
        self.layers = torch.nn.Sequential(*[GPSLayer(dim_hidden, n_heads, dropout, attn_dropout) for _ in range(layers)])
        self.post_mp = _Head(dim_hidden, dim_out)

    def forward(self, b):
        """b: dict of CPU tensors x, edge_index, edge_attr, pos_enc, pos_index, pos_batch, batch (non-decreasing)"""
        G = int(b["batch"][-1]) + 1
        sizes = torch.bincount(b["batch"], minlength=G).tolist()
        h = self.encoder.node_encoder.encoder(b["x"].view(b["x"].size(0), -1)[:, 0])
        edge_attr = self.encoder.edge_encoder.encoder(b["edge_attr"].view(-1))
        for layer in self.layers:
            h, edge_attr = layer(h, edge_attr, b, sizes)
        g = torch.zeros((G, h.size(1)), dtype=h.dtype).index_add_(0, b["batch"], h)
        fc = self.post_mp.FC_layers
        return fc[2](torch.relu(fc[1](torch.relu(fc[0](g)))))
