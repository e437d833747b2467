"""Plain-torch restatement of the GatedGCN local layer, the oracle of tests/test_gatedgcn_cpu.py and tests/test_hip_gatedgcn.py:
the gate as gather / sigmoid / index_add_ (GraphGPS/graphgps/layer/gatedgcn_layer.py:90-136), the layer and the GPSLayer /
GPSModel variants built from torch.nn modules with the reference's state_dict key layout, and the graph cases both test files
run.  CPU, any dtype (the tests use fp64 and fp32), differentiable through autograd.  Imports nothing from the package under
test; the shared pieces of the transformer (attention, GINE, encoders, head) come from tests/gps_oracle.py."""
import torch

import gps_oracle as go

EPS = 1e-6
WIDTHS = (4, 64, 68, 256)


def gate(Ax, Bx, Dx, Ex, Ce, src, dst):
    """(out [N, C], e_ij [E, C], den [N, C]) for the edges k = (src[k] -> dst[k])"""
    e = Dx[dst] + Ex[src] + Ce
    s = torch.sigmoid(e)
    num = torch.zeros_like(Ax).index_add_(0, dst, s * Bx[src])
    den = torch.zeros_like(Ax).index_add_(0, dst, s)
    return Ax + num / (den + EPS), e, den


# ---- graph cases: (number of nodes, src list, dst list) ---------------------------------------------------------------------------
def _star():
    """310 nodes: leaves 1..300 -> hub 0, a path 301 -> ... -> 307 walked both ways, 308 and 309 isolated"""
    src, dst = list(range(1, 301)), [0] * 300
    for a in range(301, 307):
        src += [a, a + 1]
        dst += [a + 1, a]
    return 310, src, dst


def _molecule():
    """30 nodes: a chain with three ring closures and two branches, every bond in both directions, a self-loop on every node
    (create_subgraphs_eff(self_loop=True) adds them), the edge list shuffled: sorted by neither end"""
    bonds = [(a, a + 1) for a in range(0, 23)] + [(0, 5), (8, 13), (16, 21), (3, 24), (24, 25), (11, 26), (26, 27), (27, 28), (19, 29)]
    pairs = [p for a, b in bonds for p in ((a, b), (b, a))] + [(a, a) for a in range(30)]
    order = torch.randperm(len(pairs), generator=torch.Generator().manual_seed(30)).tolist()
    pairs = [pairs[i] for i in order]
    src, dst = [p[0] for p in pairs], [p[1] for p in pairs]
    assert src != sorted(src) and dst != sorted(dst)
    return 30, src, dst


def _ladder():
    """18 nodes, node i with the in-edges 0 .. i-1 -> i (153 edges): in-degrees 0 .. 17 and out-degrees 17 .. 0 in one launch - an
    empty range, every tail length of a batch of 4 and of 8, exact multiples, two full batches and a tail, in both views"""
    pairs = [(j, i) for i in range(18) for j in range(i)]
    return 18, [p[0] for p in pairs], [p[1] for p in pairs]


LADDER_WIDTH = 260    # beyond WIDTHS, on "degree-ladder" and "molecule-30" alone: 64 lanes cover 256 columns, so a second pass with one live lane


def _cases():
    n, s, d = _star()
    out = {
        "one-node": (1, [], []),
        "pair": (2, [0], [1]),
        "self-loop": (1, [0], [0]),
        "repeated-edge": (2, [0, 0, 1], [1, 1, 0]),
        "star-in-300": (n, s, d),
        "star-out-300": (n, d, s),
        "molecule-30": _molecule(),
        "no-edge-3": (3, [], []),
        "empty": (0, [], []),
    }
    N, src, dst, where = 0, [], [], {}
    for name, (n, s, d) in out.items():                     # all of them as one batch, and where each one sits in it
        where[name] = (N, N + n, len(src), len(src) + len(s))
        src += [N + a for a in s]
        dst += [N + a for a in d]
        N += n
    out["batch"] = (N, src, dst)
    return out, where


CASES, WHERE = _cases()           # WHERE[name] = (first node, end node, first edge, end edge) of the case inside "batch"
LADDER = {"degree-ladder": _ladder()}     # beside CASES, not in them: the batch, every seed and every loop over CASES stay what they were


def edges_of(name):
    n, s, d = CASES[name] if name in CASES else LADDER[name]
    return n, torch.tensor(s, dtype=torch.int64), torch.tensor(d, dtype=torch.int64)


def _seed(name, C):
    return 1000 * ((list(CASES) + list(LADDER)).index(name) + 1) + C


def inputs_of(name, C, scale=1.0):
    """unit-variance (times scale) fp32 operands Ax, Bx, Dx, Ex [N, C], Ce [E, C] and upstream gradients g_out [N, C], g_e [E, C]"""
    n, src, _ = edges_of(name)
    gen = torch.Generator().manual_seed(_seed(name, C))
    mk = lambda rows: torch.randn((rows, C), generator=gen) * scale
    ops = [mk(n), mk(n), mk(n), mk(n), mk(src.numel())]
    return ops, mk(n) / scale, mk(src.numel()) / scale


_REFS = {}


def reference(name, C, with_ge=True, scale=1.0):
    """{dtype: dict(out, e_out, den, d_Ax, d_Bx, d_Dx, d_Ex, d_Ce)} in fp64 and fp32 on the CPU, the loss being
    sum(out * g_out) (+ sum(e_out * g_e)).  Computed once per case, shared, never modified."""
    key = (name, C, with_ge, scale)
    if key not in _REFS:
        ops, g_out, g_e = inputs_of(name, C, scale)
        _, src, dst = edges_of(name)
        res = {}
        for dtype in (torch.float64, torch.float32):
            x = [t.clone().to(dtype).requires_grad_(True) for t in ops]
            out, e, den = gate(*x, src, dst)
            loss = (out * g_out.to(dtype)).sum()
            if with_ge:
                loss = loss + (e * g_e.to(dtype)).sum()
            loss.backward()
            res[dtype] = dict(out=out.detach(), e_out=e.detach(), den=den.detach(),
                              **{"d_" + k: t.grad for k, t in zip(("Ax", "Bx", "Dx", "Ex", "Ce"), x)})
        _REFS[key] = res
    return _REFS[key]


# ---- where the edge gradients are a cancellation residue ------------------------------------------------------------------------------
# d_e[k] = g_e[k] + r_i (Bx_j - aggr_i) s (1 - s).  At a node whose in-edges all come from ONE neighbour j, aggr_i =
# Bx_j * den / (den + 1e-6): the difference is Bx_j * 1e-6 / (den + 1e-6), six orders below its two terms, and no fp32 evaluation
# - torch's included, 4e-2 .. 2e-3 of the largest value - carries digits of it.  In the cases below (almost) every node with
# in-edges is of that kind, so without g_e the tensors d_Dx, d_Ex and d_Ce hold nothing else and "the largest |want|" is that
# residue.  There, and only there, the error is measured over the scale of the terms that cancel,
#   T = max over edges and columns of |r_i s (1 - s)| * (|Bx_j| + |aggr_i|)        (fp64, from the oracle)
# which is what bounds the rounding error of a difference; the bound itself stays 1e-5 and the cap 2e-6.  Everywhere else the
# project's measure applies unchanged: tests/test_gatedgcn_cpu.py holds every other case and tensor to the cap under it.
CANCELLING = ("pair", "self-loop", "repeated-edge", "star-out-300")
EDGE_GRADS = ("d_Dx", "d_Ex", "d_Ce")


def scale_floor(name, C, with_ge, key, scale=1.0):
    """0.0 (the project's measure: the largest |want| alone), or T for the cancelling cases' edge gradients without g_e"""
    if with_ge or name not in CANCELLING or key not in EDGE_GRADS:
        return 0.0
    ops, g_out, _ = inputs_of(name, C, scale)
    _, src, dst = edges_of(name)
    Ax, Bx, Dx, Ex, Ce = (t.double() for t in ops)
    out, e, den = gate(Ax, Bx, Dx, Ex, Ce, src, dst)
    s = torch.sigmoid(e)
    r = g_out.double() / (den + EPS)
    return float(((r[dst] * s * (1 - s)).abs() * (Bx[src].abs() + (out - Ax)[dst].abs())).max())


def rel(got, want, floor=0.0):
    """tests/gps_cases.py's measure - max |got - want| over the largest |want|, zeros matched exactly - with the scale not
    below `floor`"""
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if not want.numel():
        return 0.0
    top, err = max(float(want.abs().max()), floor), float((got - want).abs().max())
    return err / top if top > 0 else (0.0 if err == 0 else float("inf"))


# ---- the layer and the transformer variants -----------------------------------------------------------------------------------------
class GatedGCNLayer(torch.nn.Module):
    """gatedgcn_layer.py:11-88 with act relu, no EquivStableLapPE: A, B, C, D, E, bn_node_x, bn_edge_e in that order"""

    def __init__(self, in_dim, out_dim, dropout=0.0, residual=True):
        super().__init__()
        assert dropout == 0.0, "the oracle models run without dropout"
        nn = torch.nn
        self.A, self.B, self.C = nn.Linear(in_dim, out_dim), nn.Linear(in_dim, out_dim), nn.Linear(in_dim, out_dim)
        self.D, self.E = nn.Linear(in_dim, out_dim), nn.Linear(in_dim, out_dim)
        self.bn_node_x = nn.BatchNorm1d(out_dim)
        self.bn_edge_e = nn.BatchNorm1d(out_dim)
        self.residual = residual

    def forward(self, x, e, edge_index):
        h, e_ij, _ = gate(self.A(x), self.B(x), self.D(x), self.E(x), self.C(e), edge_index[0], edge_index[1])
        h, e_ij = torch.relu(self.bn_node_x(h)), torch.relu(self.bn_edge_e(e_ij))
        return (x + h, e + e_ij) if self.residual else (h, e_ij)


class GPSLayer(torch.nn.Module):
    """gps_layer.py:19-267 for local_gnn_type GINE | CustomGatedGCN and global_model_type Transformer | None, batch_norm"""

    def __init__(self, dim_h, num_heads, local_gnn_type="GINE", global_model_type="Transformer"):
        super().__init__()
        nn = torch.nn
        if local_gnn_type == "GINE":
            self.local_model = go.GINE(nn.Sequential(nn.Linear(dim_h, dim_h), nn.ReLU(), nn.Linear(dim_h, dim_h)))
        elif local_gnn_type == "CustomGatedGCN":
            self.local_model = GatedGCNLayer(dim_h, dim_h)
        else:
            raise ValueError(f"Unsupported local GNN model: {local_gnn_type}")
        self.gated = local_gnn_type == "CustomGatedGCN"
        self.edge_attn_emb = nn.Embedding(101, num_heads, padding_idx=100)
        self.edge_attn_linear = nn.Sequential(nn.Linear(num_heads, num_heads), nn.ReLU(), nn.Linear(num_heads, num_heads), nn.ReLU(),
                                              nn.Linear(num_heads, num_heads))
        if global_model_type == "None":
            self.self_attn = None
        elif global_model_type == "Transformer":
            self.self_attn = nn.MultiheadAttention(dim_h, num_heads, dropout=0.0, batch_first=True)
        else:
            raise ValueError(f"Unsupported global x-former model: {global_model_type}")
        self.norm1_local = nn.BatchNorm1d(dim_h)
        self.norm1_attn = nn.BatchNorm1d(dim_h)
        self.ff_linear1 = nn.Linear(dim_h, dim_h * 2)
        self.ff_linear2 = nn.Linear(dim_h * 2, dim_h)
        self.norm2 = nn.BatchNorm1d(dim_h)
        self.z_initial = nn.Embedding(go.Z_TABLE_ROWS, dim_h)
        self.z_embedding = nn.Sequential(nn.Dropout(0.0), nn.BatchNorm1d(dim_h), nn.ELU(), nn.Linear(dim_h, dim_h), nn.Dropout(0.0),
                                         nn.BatchNorm1d(dim_h), nn.ELU())

    def forward(self, h, edge_attr, b, sizes):
        w = self.z_initial.weight[b["pos_index"]] * b["pos_enc"].to(h.dtype).view(-1, 1)
        z = torch.zeros((edge_attr.size(0), h.size(1)), dtype=h.dtype).index_add_(0, b["pos_batch"], w)
        edge_attr = edge_attr + self.z_embedding(z)
        if self.gated:
            h_local, edge_attr = self.local_model(h, edge_attr, b["edge_index"])
            h_local = self.norm1_local(h_local)
        else:
            h_local = self.norm1_local(h + self.local_model(h, b["edge_index"], edge_attr))
        if self.self_attn is not None:
            h_local = h_local + self.norm1_attn(h + go.ragged_mha(self.self_attn, h, sizes))
        h = h_local
        h = h + self.ff_linear2(torch.relu(self.ff_linear1(h)))
        return self.norm2(h), edge_attr


class GPSModel(go.GPSModel):
    def __init__(self, layers=10, dim_hidden=64, n_heads=4, node_types=28, edge_types=4, dim_out=1, local_gnn_type="GINE",
                 global_model_type="Transformer"):
        super().__init__(0, dim_hidden, n_heads, 0.0, 0.0, node_types, edge_types, dim_out)
        self.layers = torch.nn.Sequential(*[GPSLayer(dim_hidden, n_heads, local_gnn_type, global_model_type) for _ in range(layers)])
