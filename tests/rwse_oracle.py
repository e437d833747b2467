"""Plain numpy / torch restatement of the random-walk structural encoding, the oracle of tests/test_rwse_cpu.py and
tests/test_hip_rwse.py: the landing probabilities straight from their definition in dense fp64, the reference's own expression
(get_rw_landing_probs with edge_weight None and space_dim 0) restated with plain torch in fp32 - both of its branches -, the test
graphs with the reason each is there, the RWSE node encoder and the two composed node encoders built the reference's way, and the
graph transformer with them.  Written by reading GraphGPS/graphgps/transform/posenc_stats.py:185-231,
encoder/kernel_pos_encoder.py and encoder/composed_encoders.py (torch_geometric is not needed).  Imports nothing from the
package under test."""
import numpy as np
import torch

import gps_oracle as go
import lappe_oracle as lo
from lappe_oracle import _both, _cycle, _path, batch_of, molecule_like, random_graph      # noqa: F401  (the graph builders are shared)

MAX_NODES = 256           # the kernel's limits per graph (test_hip_rwse checks the library agrees)
MAX_EDGES = 7678
KSTEPS = list(range(1, 21))                  # the run's default: 20 consecutive steps
GAPPED = [1, 2, 4, 8, 16, 63]
SINGLE = [3]


# ---- the statistic ----------------------------------------------------------------------------------------------------------------
def transition(n, edges):
    """dense fp64 P = D^-1 A: A[u, j] = the number of listed edges u -> j (directed, self-loops kept, duplicates add up),
    deg = the row sums, rows of deg = 0 zero"""
    e = np.asarray(edges, dtype=np.int64).reshape(2, -1)
    A = np.zeros((n, n))
    np.add.at(A, (e[0], e[1]), 1.0)
    deg = A.sum(1)
    P = np.zeros((n, n))
    P[deg > 0] = A[deg > 0] / deg[deg > 0, None]
    return P


def rw_landing64(n, edges, ksteps):
    """[n, K] fp64: (P^k)[i, i] for every k of ksteps, by repeated products P^k = P^(k-1) P"""
    P = transition(n, edges)
    out, Pk = np.zeros((n, len(ksteps))), np.eye(n)
    for k in range(1, max(ksteps) + 1):
        Pk = Pk @ P
        if k in ksteps:
            out[:, list(ksteps).index(k)] = np.diagonal(Pk)
    return out


def rw_landing_ref32(n, edges, ksteps):
    """the reference's expression in fp32 torch: the out-degree by index_add, its inverse with inf replaced by 0, the dense
    adjacency by index_put_(accumulate=True), P = diag(deg_inv) @ A; a consecutive list walks Pk <- Pk @ P from
    matrix_power(min), any other list takes matrix_power(k) for every k.  [n, K] fp32"""
    e = torch.as_tensor(np.asarray(edges, dtype=np.int64).reshape(2, -1))
    src, dst = e[0], e[1]
    weight = torch.ones(e.size(1))
    deg = torch.zeros(n).index_add(0, src, weight)
    deg_inv = deg.pow(-1.0)
    deg_inv.masked_fill_(deg_inv == float("inf"), 0)
    if e.numel() == 0:
        P = torch.zeros((1, n, n))
    else:
        A = torch.zeros((n, n)).index_put_((src, dst), weight, accumulate=True)
        P = (torch.diag(deg_inv) @ A).unsqueeze(0)
    ksteps = list(ksteps)
    rws = []
    if ksteps == list(range(min(ksteps), max(ksteps) + 1)):
        Pk = P.clone().matrix_power(min(ksteps))
        for k in range(min(ksteps), max(ksteps) + 1):
            rws.append(torch.diagonal(Pk, dim1=-2, dim2=-1))
            Pk = Pk @ P
    else:
        for k in ksteps:
            rws.append(torch.diagonal(P.matrix_power(k), dim1=-2, dim2=-1))
    return torch.cat(rws, dim=0).transpose(0, 1).contiguous()


def within_one_ulp(got, want64):
    """(ok, worst distance in units of the last place): |got - fp32(want)| <= spacing(fp32(want)) elementwise, and exact zeros
    where the oracle is exactly 0.  got fp32 [n, K], want64 fp64 [n, K]"""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    ulp = np.spacing(np.abs(want))
    dist = np.abs(got.astype(np.float64) - want.astype(np.float64))
    zeros_ok = bool((got[np.asarray(want64) == 0.0] == 0.0).all())
    worst = float((dist / ulp).max()) if got.size else 0.0
    return bool((dist <= ulp).all()) and zeros_ok and bool(np.isfinite(got).all()), worst


# ---- the test graphs ------------------------------------------------------------------------------------------------------------
def random_multigraph(n, m, seed):
    """m directed edges with ends drawn uniformly: duplicates, self-loops and sinks all occur"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, n, size=(2, m)).astype(np.int64)


def with_self_loops(n, edges):
    """the N self-loops create_subgraphs(..., self_loop=True) appends behind the molecule's edges"""
    return np.concatenate([edges, np.arange(n, dtype=np.int64)[None, :].repeat(2, 0)], 1)


_PETERSEN = _cycle(5) + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)]
_TRI_PATH = _cycle(3) + _path(4, 3)                      # nodes 0..6; the graphs below have 8 nodes: node 7 is isolated
_TP = _both(_TRI_PATH)
_DESC = _both(_cycle(7) + [(0, 3), (2, 5)])
_DESC = _DESC[:, np.argsort(-_DESC[0], kind="stable")].copy()

GRAPHS = [  # (name, n, edge_index, reason)
    ("one-node", 1, _both([]), "no edge: zeros"),
    ("two-node-edge", 2, _both([(0, 1)]), "odd steps 0, even steps 1"),
    ("path-3", 3, _both(_path(3)), "the walk from the middle returns with certainty every second step"),
    ("triangle", 3, _both(_cycle(3)), "k = 1, 2, 3 gives 0, 1/2, 1/4"),
    ("cycle-12", 12, _both(_cycle(12)), "bipartite: odd steps exactly 0, k = 2 is 1/2"),
    ("star-6", 6, _both([(0, i) for i in range(1, 6)]), "two degrees; bipartite"),
    ("K5", 5, _both([(i, j) for i in range(5) for j in range(i + 1, 5)]), "k = 2 is 1/4"),
    ("petersen", 10, _both(_PETERSEN), "3-regular, girth 5: k = 3 is 0, k = 5 is not"),
    ("triangle+path-isolated", 8, _TP, "two components and an isolated node: a zero row of P"),
    ("triangle+path-directed", 8, np.array(_TRI_PATH, dtype=np.int64).T.copy(), "every edge listed once: node 6 is a sink, deg = 0"),
    ("triangle+path-self-loop", 8, np.concatenate([_TP, np.array([[2], [2]], dtype=np.int64)], 1), "a self-loop is kept"),
    ("triangle+path-duplicate", 8, np.concatenate([_TP, np.array([[4], [5]], dtype=np.int64)], 1), "a duplicated edge counts twice"),
    ("descending-sources", 7, _DESC, "edges listed in descending source order: the kernel groups them itself"),
    ("molecule-37", 37, with_self_loops(37, molecule_like()), "the run's own shape: ZINC's largest size with the appended self-loops"),
    ("random-65", 65, random_graph(65, 11), "a second lane trip on 64-wide waves"),
    ("random-256", MAX_NODES, random_graph(MAX_NODES, 3), "the node limit"),
    ("multigraph-edge-limit", 128, random_multigraph(128, MAX_EDGES, 5), "the edge limit: duplicates, self-loops and sinks"),
]
NAMES = [g[0] for g in GRAPHS]


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
class RWSEEncoder(torch.nn.Module):
    """KernelPENodeEncoder for kernel_type RWSE with expand_x False, constructed in the reference's order: the raw norm first,
    then the Linear or the Sequential of Linear / ReLU pairs"""

    def __init__(self, dim_pe, num_steps, model="linear", layers=1, raw_norm="batchnorm"):
        super().__init__()
        nn = torch.nn
        self.raw_norm = nn.BatchNorm1d(num_steps) if str(raw_norm).lower() == "batchnorm" else None
        model = model.lower()
        if model == "mlp":
            seq = []
            if layers == 1:
                seq += [nn.Linear(num_steps, dim_pe), nn.ReLU()]
            else:
                seq += [nn.Linear(num_steps, 2 * dim_pe), nn.ReLU()]
                for _ in range(layers - 2):
                    seq += [nn.Linear(2 * dim_pe, 2 * dim_pe), nn.ReLU()]
                seq += [nn.Linear(2 * dim_pe, dim_pe), nn.ReLU()]
            self.pe_encoder = nn.Sequential(*seq)
        elif model == "linear":
            self.pe_encoder = nn.Linear(num_steps, dim_pe)
        else:
            raise ValueError("RWSENodeEncoder: Does not support '%s' encoder model." % model)

    def forward(self, pestat):
        if self.raw_norm is not None:
            pestat = self.raw_norm(pestat)
        return self.pe_encoder(pestat)


# ---- the model -------------------------------------------------------------------------------------------------------------------
class _Concat(torch.nn.Module):
    """Concat2NodeEncoder (rwse alone) / Concat3NodeEncoder (LapPE + RWSE): encoder1 at the width left over, then the encoders"""

    def __init__(self, num_types, dim, lap, rw):
        super().__init__()
        self.encoder1 = go._TypeDict(num_types, dim - (lap["dim_pe"] if lap else 0) - rw["dim_pe"])
        if lap:
            self.encoder2 = lo.LapPEEncoder(lap["dim_pe"], lap["max_freqs"])
            self.encoder3 = RWSEEncoder(**rw)
        else:
            self.encoder2 = RWSEEncoder(**rw)


class _Encoder(torch.nn.Module):
    def __init__(self, dim, node_types, edge_types, lap, rw):
        super().__init__()
        self.node_encoder = _Concat(node_types, dim, lap, rw)
        self.edge_encoder = go._TypeDict(edge_types, dim)


class GPSModel(torch.nn.Module):
    """gps_oracle.GPSModel with the node encoder TypeDictNode+RWSE, or TypeDictNode+LapPE+RWSE when `lap_pe`: b carries
    pestat_RWSE (and EigVecs / EigVals); `signs` stands for LapPE's training-time sign flip"""

    def __init__(self, layers=10, dim_hidden=64, n_heads=4, node_types=28, edge_types=4, dim_out=1, lap_pe=False, dim_pe=8, max_freqs=8,
                 rwse_dim_pe=28, rwse_steps=20, rwse_model="linear", rwse_layers=1, rwse_raw_norm="batchnorm"):
        super().__init__()
        rw = dict(dim_pe=rwse_dim_pe, num_steps=rwse_steps, model=rwse_model, layers=rwse_layers, raw_norm=rwse_raw_norm)
        self.encoder = _Encoder(dim_hidden, node_types, edge_types, dict(dim_pe=dim_pe, max_freqs=max_freqs) if lap_pe else None, rw)
        self.layers = torch.nn.Sequential(*[go.GPSLayer(dim_hidden, n_heads) for _ in range(layers)])
        self.post_mp = go._Head(dim_hidden, dim_out)
        self.lap_pe = bool(lap_pe)

    def forward(self, b, signs=None):
        G = int(b["batch"][-1]) + 1
        sizes = torch.bincount(b["batch"], minlength=G).tolist()
        ne = self.encoder.node_encoder
        dtype = ne.encoder1.encoder.weight.dtype
        parts = [ne.encoder1.encoder(b["x"].view(b["x"].size(0), -1)[:, 0])]
        if self.lap_pe:
            parts.append(ne.encoder2(b["EigVecs"].to(dtype), b["EigVals"].to(dtype), None if signs is None else signs.to(dtype)))
            parts.append(ne.encoder3(b["pestat_RWSE"].to(dtype)))
        else:
            parts.append(ne.encoder2(b["pestat_RWSE"].to(dtype)))
        h = torch.cat(parts, 1)
        edge_attr = self.encoder.edge_encoder.encoder(b["edge_attr"].view(-1))
        for layer in self.layers:
            h, edge_attr = layer(h, edge_attr, b, sizes)
        g = torch.zeros((G, h.size(1)), dtype=h.dtype).index_add_(0, b["batch"], h)
        fc = self.post_mp.FC_layers
        return fc[2](torch.relu(fc[1](torch.relu(fc[0](g)))))
