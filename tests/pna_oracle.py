"""Plain-torch restatement of the PNA local layer, the oracle of tests/test_pna_cpu.py and tests/test_hip_pna.py: the aggregate
mean | max | sum with its tie rule stated explicitly, PyG's PNAConv as the reference's GPSLayer constructs it
(GraphGPS/graphgps/layer/gps_layer.py:78-93: aggregators mean / max / sum, identity scaler, one tower, one pre- and one
post-layer), and the GPSLayer / GPSModel variants built from torch.nn modules with that state_dict key layout.  CPU, any dtype
(the tests use fp64 and fp32), differentiable through autograd.  Imports nothing from the package under test; the graph cases
and the batch are tests/gatedgcn_oracle.py's, the shared pieces of the transformer come from tests/gps_oracle.py through it.

The tie rule: the maximum of a node and column is held by the LOWEST edge position among its maxima, found by the comparison
m > best that starts from the node's first message, and its value is taken by gather of that position - so autograd routes the
whole gradient to it.  (scatter_reduce 'amax' is not used: its backward splits the gradient evenly among ties.)"""
import torch

import gatedgcn_oracle as gg

WIDTHS = (4, 64, 68, 256)
CASES, WHERE, edges_of, rel = gg.CASES, gg.WHERE, gg.edges_of, gg.rel


def arg_of(m, dst, N):
    """[N, C] int64: for every node and column the lowest edge position that holds the largest message, -1 without in-edges"""
    m = m.detach()
    best = torch.zeros((N, m.size(1)), dtype=m.dtype)
    arg = torch.full((N, m.size(1)), -1, dtype=torch.int64)
    for k, i in enumerate(dst.tolist()):                        # ascending edge position
        take = (arg[i] < 0) | (m[k] > best[i])                  # the first message, or a strictly larger one
        best[i] = torch.where(take, m[k], best[i])
        arg[i] = torch.where(take, torch.full_like(arg[i], k), arg[i])
    return arg


def aggregate_messages(m, dst, N):
    """(agg [N, 3C] = mean | max | sum of the messages m [E, C] over every node's in-edges, arg [N, C])"""
    C = m.size(1)
    deg = torch.bincount(dst, minlength=N).view(-1, 1)
    total = torch.zeros((N, C), dtype=m.dtype).index_add_(0, dst, m)
    mean = total / deg.clamp(min=1).to(m.dtype)
    arg = arg_of(m, dst, N)
    if m.size(0):
        top = torch.where(arg >= 0, m.gather(0, arg.clamp(min=0)), torch.zeros((), dtype=m.dtype))
    else:
        top = torch.zeros((N, C), dtype=m.dtype)
    return torch.cat([mean, top, total], 1), arg


def messages(P, Q, R, src, dst):
    return (P[dst] + Q[src]) + R


def aggregate(P, Q, R, src, dst):
    """(agg [N, 3C], arg [N, C]) for the edges k = (src[k] -> dst[k]) and the messages (P[i] + Q[j]) + R[k]"""
    return aggregate_messages(messages(P, Q, R, src, dst), dst, P.size(0))


def top_two_gap(m, dst, N):
    """(the smallest gap between a node's largest and second-largest message over all nodes with two or more in-edges and all
    columns - 0 at a tie -, the largest |m|); (inf, .) where no node has two in-edges"""
    m = m.detach().double()
    order = torch.sort(dst, stable=True).indices
    ptr = [0] + torch.cumsum(torch.bincount(dst, minlength=N), 0).tolist()
    gap = float("inf")
    for i in range(N):
        if ptr[i + 1] - ptr[i] >= 2:
            two = m[order[ptr[i]:ptr[i + 1]]].topk(2, dim=0).values
            gap = min(gap, float((two[0] - two[1]).min()))
    return gap, (float(m.abs().max()) if m.numel() else 0.0)


# ---- inputs and references of the kernel cases ------------------------------------------------------------------------------------
def inputs_of(name, C):
    """unit-variance fp32 operands P, Q [N, C], R [E, C] and the upstream gradient g [N, 3C]"""
    n, src, _ = edges_of(name)
    gen = torch.Generator().manual_seed(gg._seed(name, C) + 7)
    mk = lambda rows, cols: torch.randn((rows, cols), generator=gen)     # noqa: E731
    return [mk(n, C), mk(n, C), mk(src.numel(), C)], mk(n, 3 * C)


def run(ops, g, src, dst, dtype):
    """dict(agg, arg, d_P, d_Q, d_R) of the oracle in `dtype`, the loss being sum(agg * g)"""
    x = [t.clone().to(dtype).requires_grad_(True) for t in ops]
    agg, arg = aggregate(*x, src, dst)
    (agg * g.to(dtype)).sum().backward()
    return dict(agg=agg.detach(), arg=arg, **{"d_" + k: t.grad for k, t in zip("PQR", x)})


_REFS = {}


def reference(name, C):
    """{dtype: dict(agg, arg, d_P, d_Q, d_R)} in fp64 and fp32 on the CPU.  Computed once per case, shared, never modified."""
    key = (name, C)
    if key not in _REFS:
        ops, g = inputs_of(name, C)
        _, src, dst = edges_of(name)
        _REFS[key] = {dtype: run(ops, g, src, dst, dtype) for dtype in (torch.float64, torch.float32)}
    return _REFS[key]


# ---- the layer and the transformer variants ---------------------------------------------------------------------------------------
class PNAConv(torch.nn.Module):
    """edge_encoder, pre_nns.0.0, post_nns.0.0, lin in that order; the message is the one Linear of the concatenation, as PyG
    writes it - not the split into P, Q and R that the package under test computes.  The messages of the last forward and their
    destinations stay on the module for the conditioning check."""

    def __init__(self, dim):
        super().__init__()
        nn = torch.nn
        self.edge_encoder = nn.Linear(dim, dim)
        self.pre_nns = nn.ModuleList([nn.Sequential(nn.Linear(3 * dim, dim))])
        self.post_nns = nn.ModuleList([nn.Sequential(nn.Linear(4 * dim, dim))])
        self.lin = nn.Linear(dim, dim)
        self.last = None

    def forward(self, x, edge_index, edge_attr):
        src, dst = edge_index[0], edge_index[1]
        m = self.pre_nns[0](torch.cat([x[dst], x[src], self.edge_encoder(edge_attr)], 1))
        self.last = (m.detach(), dst)
        agg, _ = aggregate_messages(m, dst, x.size(0))
        return self.lin(self.post_nns[0](torch.cat([x, agg], 1)))


class GPSLayer(gg.GPSLayer):
    """gps_layer.py:216-229: PNA takes the place and the treatment of GINE - the residual, norm1_local, edge attributes untouched"""

    def __init__(self, dim_h, num_heads, local_gnn_type="PNA", global_model_type="Transformer"):
        super().__init__(dim_h, num_heads, "GINE" if local_gnn_type == "PNA" else local_gnn_type, global_model_type)
        if local_gnn_type == "PNA":
            self.local_model = PNAConv(dim_h)                   # the same slot: the key order is the reference's


class GPSModel(gg.go.GPSModel):
    def __init__(self, layers=10, dim_hidden=64, n_heads=4, node_types=28, edge_types=4, dim_out=1, local_gnn_type="PNA",
                 global_model_type="Transformer"):
        super().__init__(0, dim_hidden, n_heads, 0.0, 0.0, node_types, edge_types, dim_out)
        self.layers = torch.nn.Sequential(*[GPSLayer(dim_hidden, n_heads, local_gnn_type, global_model_type) for _ in range(layers)])

    def worst_gap(self):
        """the smallest top-two gap of any layer's messages in the last forward, over that layer's largest |message|"""
        worst = float("inf")
        for layer in self.layers:
            m, dst = layer.local_model.last
            gap, top = top_two_gap(m, dst, int(dst.max()) + 1)
            worst = min(worst, gap / top)
        return worst
