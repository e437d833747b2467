"""Plain-torch restatement of the per-graph LayerNorm, the oracle of tests/test_layernorm_cpu.py and tests/test_hip_layernorm.py:
the segment form that include/escgnn_layernorm.h states, the PyG form (norm.LayerNorm.forward with a batch vector, PyG 2.0.4 /
2.2) spelled out in torch ops, the cases of the GPU comparison with their shared references, and GPSLayer / GPSModel with the
reference's two normalisation switches built on the oracle models of tests/pna_oracle.py.  Runs on the CPU in whatever dtype it is
given; differentiable through autograd.  Imports nothing from the package under test."""
import torch

import gps_oracle as go
import pna_oracle as po

EPS = 1e-5


def batch_of(sizes):
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.as_tensor(sizes, dtype=torch.int64))


def segment_layer_norm(x, sizes, weight=None, bias=None, eps=EPS, residual=None, return_stats=False):
    """the header's expression, graph by graph: h = x (+ r), mean = sum h / M, c = h - mean, var = sum c c / M (the centred
    second pass), rstd = 1 / sqrt(var + eps), y = c rstd w + b.  stats [G, 2] = (mean, rstd), (0, 0) for an empty graph."""
    h = x if residual is None else x + residual
    C = h.size(1)
    out, stats, o = [], [], 0
    for n in sizes:
        rows = h[o:o + n]
        o += n
        if n == 0:
            stats.append(h.new_zeros(2))
            continue
        M = n * C
        mean = rows.sum() / M
        c = rows - mean
        rstd = 1.0 / torch.sqrt((c * c).sum() / M + eps)
        y = c * rstd
        out.append(y * weight + bias if weight is not None else y)
        stats.append(torch.stack([mean, rstd]))
    assert o == h.size(0)
    y = torch.cat(out, 0) if out else h.new_zeros((0, C))
    return (y, torch.stack(stats) if stats else h.new_zeros((0, 2))) if return_stats else y


def pyg_layer_norm(x, batch, weight=None, bias=None, eps=EPS, batch_size=None):
    """torch_geometric.nn.norm.LayerNorm.forward(x, batch), statement by statement, with degree() and scatter(reduce='add')
    written as the index_add they are"""
    if batch_size is None:
        batch_size = int(batch.max()) + 1
    norm = torch.zeros(batch_size, dtype=x.dtype).index_add_(0, batch, torch.ones(batch.numel(), dtype=x.dtype)).clamp_(min=1)   # degree(...).clamp_(min=1)
    norm = norm.mul_(x.size(-1)).view(-1, 1)
    mean = torch.zeros((batch_size, x.size(1)), dtype=x.dtype).index_add(0, batch, x).sum(dim=-1, keepdim=True) / norm
    x = x - mean.index_select(0, batch)
    var = torch.zeros((batch_size, x.size(1)), dtype=x.dtype).index_add(0, batch, x * x).sum(dim=-1, keepdim=True)
    var = var / norm
    out = x / (var + eps).sqrt().index_select(0, batch)
    if weight is not None:
        out = out * weight + bias
    return out


# ---- the cases of the GPU comparison ------------------------------------------------------------------------------------------------
RAGGED = [23, 1, 30, 0, 9, 37, 2]
# name -> (sizes, C, offset of the values, constant graph or None)
CASES = {
    "ragged-4": (RAGGED, 4, 0.0, None),
    "ragged-12": (RAGGED, 12, 0.0, None),
    "ragged-64": (RAGGED, 64, 0.0, None),
    "ragged-300": (RAGGED, 300, 0.0, None),
    "ragged-128": (RAGGED, 128, 0.0, None),                # the 512-thread workgroup
    "one-graph-70x300": ([70], 300, 0.0, None),            # the 1024-thread workgroup beyond its registers (13 row lanes x 4 rows)
    "one-graph-260x64": ([260], 64, 0.0, None),            # beyond the rows a thread keeps in registers: the re-read passes
    "one-node-4": ([1], 4, 0.0, None),                     # M = 4
    "130-one-node-graphs-12": ([1] * 130, 12, 0.0, None),  # more graphs than one trip of the second launch's 64 chains
    "offset-100-64": (RAGGED, 64, 100.0, None),            # values at 100 + randn: E[h^2] - mean^2 loses the variance here
    "constant-graph-64": ([5, 7, 3], 64, 0.0, 1),          # graph 1 is constant: var = 0
}
CONSTANT = 1.5          # a dyadic value: every partial sum of up to 2^22 copies is exact in fp32 in ANY order, so mean == 1.5, c == 0
_REFS = {}


def inputs_of(name):
    """fp32 x, residual, weight, bias and the upstream gradient cos(arange) of a case, seeded by its name"""
    sizes, C, offset, constant = CASES[name]
    N = sum(sizes)
    gen = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    x = torch.randn((N, C), generator=gen) + offset
    r = torch.randn((N, C), generator=gen)
    if constant is not None:
        o = sum(sizes[:constant])
        x[o:o + sizes[constant]] = CONSTANT
        r[o:o + sizes[constant]] = 0.0
    weight = torch.rand(C, generator=gen) + 0.5
    bias = torch.randn(C, generator=gen) * 0.1
    gy = torch.cos(torch.arange(N * C, dtype=torch.float64)).reshape(N, C).float()
    return x, r, weight, bias, gy


def reference(name, residual=False):
    """(inputs, fp64 results, fp32 CPU results) of a case: y, stats, d_x, d_weight, d_bias; computed once, shared, never modified"""
    key = (name, residual)
    if key not in _REFS:
        sizes = CASES[name][0]
        x, r, weight, bias, gy = inputs_of(name)
        res = []
        for dtype in (torch.float64, torch.float32):
            xs = x.clone().to(dtype).requires_grad_(True)
            w, b = weight.clone().to(dtype).requires_grad_(True), bias.clone().to(dtype).requires_grad_(True)
            y, stats = segment_layer_norm(xs, sizes, w, b, EPS, r.to(dtype) if residual else None, return_stats=True)
            y.backward(gy.to(dtype))
            res.append(dict(y=y.detach(), stats=stats.detach(), d_x=xs.grad, d_weight=w.grad, d_bias=b.grad))
        _REFS[key] = ((x, r, weight, bias, gy), res[0], res[1])
    return _REFS[key]


# ---- the layer and the model with the two switches -----------------------------------------------------------------------------------
class LayerNorm(torch.nn.Module):
    """pygnn.norm.LayerNorm(in_channels): weight (ones), bias (zeros); forward(x, batch)"""

    def __init__(self, in_channels, eps=EPS):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(in_channels))
        self.bias = torch.nn.Parameter(torch.zeros(in_channels))

    def forward(self, x, batch):
        return pyg_layer_norm(x, batch, self.weight, self.bias, self.eps)


class GPSLayer(po.GPSLayer):
    """gps_layer.py:139-165,226-229,249-252,261-264 on top of the batch_norm oracle: layer_norm swaps the three norms for
    LayerNorm modules IN PLACE (the state_dict keeps the reference's order), neither removes them"""

    def __init__(self, dim_h, num_heads, local_gnn_type="GINE", global_model_type="Transformer", layer_norm=False, batch_norm=True):
        super().__init__(dim_h, num_heads, local_gnn_type, global_model_type)
        if layer_norm and batch_norm:
            raise ValueError("Cannot apply two types of normalization together")
        self.layer_norm, self.batch_norm = layer_norm, batch_norm
        for name in ("norm1_local", "norm1_attn", "norm2"):
            if layer_norm:
                setattr(self, name, LayerNorm(dim_h))
            elif not batch_norm:
                delattr(self, name)

    def _norm(self, name, h, batch):
        if self.layer_norm:
            return getattr(self, name)(h, batch)
        return getattr(self, name)(h) if self.batch_norm else h

    def forward(self, h, edge_attr, b, sizes):
        w = self.z_initial.weight[b["pos_index"]] * b["pos_enc"].to(h.dtype).view(-1, 1)
        z = torch.zeros((edge_attr.size(0), h.size(1)), dtype=h.dtype).index_add_(0, b["pos_batch"], w)
        edge_attr = edge_attr + self.z_embedding(z)
        if self.gated:
            h_local, edge_attr = self.local_model(h, edge_attr, b["edge_index"])
        else:
            h_local = h + self.local_model(h, b["edge_index"], edge_attr)
        h_local = self._norm("norm1_local", h_local, b["batch"])
        if self.self_attn is not None:
            h_local = h_local + self._norm("norm1_attn", h + go.ragged_mha(self.self_attn, h, sizes), b["batch"])
        h = h_local
        h = h + self.ff_linear2(torch.relu(self.ff_linear1(h)))
        return self._norm("norm2", h, b["batch"]), edge_attr


class GPSModel(go.GPSModel):
    def __init__(self, layers=10, dim_hidden=64, n_heads=4, node_types=28, edge_types=4, dim_out=1, local_gnn_type="GINE",
                 global_model_type="Transformer", layer_norm=False, batch_norm=True):
        super().__init__(0, dim_hidden, n_heads, 0.0, 0.0, node_types, edge_types, dim_out)
        self.layers = torch.nn.Sequential(*[GPSLayer(dim_hidden, n_heads, local_gnn_type, global_model_type, layer_norm, batch_norm)
                                            for _ in range(layers)])
