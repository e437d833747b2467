"""Plain numpy / torch restatement of the Laplacian positional encoding, the oracle of tests/test_lappe_cpu.py and
tests/test_hip_lappe.py: the eigen-decomposition statistics of the reference's compute_posenc_stats for pe_types ['LapPE'] with
laplacian_norm none and eigvec_norm L2 (in fp64 throughout), the test graphs with the reason each is there, the sign- and
basis-free comparison (i)-(vi), the DeepSet LapPENodeEncoder built the reference's way, a step-by-step evaluation of its forward
on the concatenated tensor, and the graph transformer with the TypeDictNode+LapPE node encoder.  Written by reading
GraphGPS/graphgps/transform/posenc_stats.py, encoder/laplace_pos_encoder.py and encoder/composed_encoders.py (torch_geometric is
not needed).  Imports nothing from the package under test."""
import numpy as np
import torch

import gps_oracle as go

K_DEFAULT = 8
LDS_NODES = 90            # the largest graph whose matrices the kernel keeps in LDS (test_hip_lappe checks the library agrees)
MAX_NODES = 256           # the kernel's size limit
BOUND = 1e-5              # the project's bound: 1e-5 of the tensor's largest value
GAP = 1e-3                # the conditioning the test graphs keep: distinct eigenvalue clusters among the first K+1 this far apart


# ---- the decomposition -----------------------------------------------------------------------------------------------------------
def laplacian(n, edges):
    """dense fp64 L = D - A; A_ij = 1 if an edge (i, j) or (j, i) with i != j is listed (to_undirected + get_laplacian on a
    simple graph: self-loops dropped, a pair listed in both directions counts once)"""
    A = np.zeros((n, n))
    for s, t in np.asarray(edges, dtype=np.int64).reshape(2, -1).T:
        if s != t:
            A[s, t] = A[t, s] = 1.0
    return np.diag(A.sum(1)) - A


def lap_pe(n, edges, K=K_DEFAULT):
    """(EigVals [n, K, 1], EigVecs [n, K]) in fp64: eigh, the K smallest, eigenvalues clamped at 0, each eigenvector over
    max(its 2-norm, 1e-12), NaN in the columns j >= n"""
    evals, evects = np.linalg.eigh(laplacian(n, edges))
    idx = evals.argsort()[:K]
    evals, evects = np.maximum(evals[idx], 0.0), evects[:, idx]
    evects = evects / np.maximum(np.sqrt((evects ** 2).sum(0, keepdims=True)), 1e-12)
    vecs, vals = np.full((n, K), np.nan), np.full((n, K), np.nan)
    vecs[:, :idx.size] = evects
    vals[:, :idx.size] = evals[None, :]
    return vals[:, :, None], vecs


def clusters(evals):
    """[(first, last+1)] of the runs of consecutive ascending eigenvalues closer than 1e-8 * max(1, lambda_max)"""
    tol = 1e-8 * max(1.0, float(evals[-1])) if len(evals) else 0.0
    out, a = [], 0
    for i in range(1, len(evals) + 1):
        if i == len(evals) or evals[i] - evals[i - 1] >= tol:
            out.append((a, i))
            a = i
    return out


def smallest_gap(n, edges, K=K_DEFAULT):
    """the least distance between neighbouring clusters among the first K+1 eigenvalues (inf when there is one cluster)"""
    evals = np.maximum(np.linalg.eigh(laplacian(n, edges))[0], 0.0)[:K + 1]
    cl = clusters(evals)
    return min([evals[b[0]] - evals[a[1] - 1] for a, b in zip(cl, cl[1:])] or [np.inf])


def _rel(err, scale):
    """err as a fraction of the tensor's largest value; a tensor of zeros must be matched exactly"""
    return err / scale if scale > 0 else (0.0 if err == 0 else np.inf)


def compare(name, n, edges, vals, vecs, K=K_DEFAULT, bound=BOUND):
    """(i)-(vi) for one graph: vals [n, K] or [n, K, 1] and vecs [n, K] as computed by the code under test against
    numpy.linalg.eigh in fp64.  Prints every measured figure next to the bound, then asserts.  Returns the figures."""
    vals, vecs = np.asarray(vals, dtype=np.float64).reshape(n, K), np.asarray(vecs, dtype=np.float64).reshape(n, K)
    L = laplacian(n, edges)
    w, U = np.linalg.eigh(L)
    w = np.maximum(w, 0.0)
    kept = min(n, K)
    fig = {}
    # (v) the NaN pattern, exactly
    nan_ok = (not np.isnan(vals[:, :kept]).any() and not np.isnan(vecs[:, :kept]).any() and np.isnan(vals[:, kept:]).all() and
              np.isnan(vecs[:, kept:]).all())
    lam, V = vals[0, :kept], vecs[:, :kept]
    # (i) eigenvalues, the same on every row.  A difference inside the reference's own error - eigh is backward stable, its
    # eigenvalues are exact for a matrix within n * eps * ||L|| of L - is no difference: a true 0 comes out of eigh as +-1e-16
    # before the clamp, and when K keeps nothing but such values the tensor's largest value is 0
    rows_equal = bool((vals[:, :kept] == lam[None, :]).all())
    diff = np.abs(lam - w[:kept])
    diff[diff <= n * np.finfo(np.float64).eps * np.abs(L).sum(1).max()] = 0.0
    fig["eigenvalues"] = _rel(float(diff.max()), float(np.abs(w[:kept]).max()))
    # (ii) residual, as a fraction of the largest value L v can take for |v| <= 1 (the largest absolute row sum), and orthonormality
    fig["residual"] = _rel(float(np.abs(L @ V - V * lam[None, :]).max()), float(np.abs(L).sum(1).max()))
    fig["orthonormality"] = float(np.abs(V.T @ V - np.eye(kept)).max())
    # (vi) column norms
    fig["norms"] = float(np.abs(np.sqrt((V ** 2).sum(0)) - 1.0).max())
    # (iii) projectors of the clusters wholly inside the first K, (iv) membership for a cluster K cuts
    fig["projectors"], fig["membership"] = 0.0, 0.0
    for a, b in clusters(w):
        if a >= kept:
            break
        P = U[:, a:b] @ U[:, a:b].T
        if b <= kept:
            mine = V[:, a:b] @ V[:, a:b].T
            fig["projectors"] = max(fig["projectors"], _rel(float(np.abs(mine - P).max()), float(np.abs(P).max())))
        else:
            out = V[:, a:kept] - P @ V[:, a:kept]
            fig["membership"] = max(fig["membership"], float(np.sqrt((out ** 2).sum(0)).max()))
    print("%-28s n %3d  " % (name, n) + "  ".join("%s %.3g" % kv for kv in fig.items()) + "   bound %g" % bound)
    assert nan_ok, "%s: NaN pattern" % name
    assert rows_equal, "%s: the eigenvalues differ between rows" % name
    for what, v in fig.items():
        assert v <= bound, "%s: %s %.3g, bound %g" % (name, what, v, bound)
    return fig


# ---- the test graphs ------------------------------------------------------------------------------------------------------------
def _both(pairs):
    """every listed pair in both directions, as edge_index"""
    pairs = [(int(a), int(b)) for a, b in pairs]
    return np.array([[a for a, b in pairs] + [b for a, b in pairs], [b for a, b in pairs] + [a for a, b in pairs]], dtype=np.int64).reshape(2, -1)


def _path(n, at=0):
    return [(at + i, at + i + 1) for i in range(n - 1)]


def _cycle(n, at=0):
    return _path(n, at) + [(at + n - 1, at)]


def random_graph(n, seed, degree=6.0):
    """a seeded G(n, p) with mean degree `degree`, plus a spanning path so that it is connected"""
    rng = np.random.RandomState(seed)
    upper = np.triu(rng.rand(n, n) < degree / n, 1)
    pairs = set(zip(*np.nonzero(upper))) | set(_path(n))
    return _both(sorted(pairs))


def molecule_like(n=37, seed=4):
    """rings of five and six joined by short chains with a few pendant atoms: what a large ZINC molecule looks like"""
    rng = np.random.RandomState(seed)
    pairs, at = [], 0
    while at < n:
        ring = int(rng.choice([5, 6]))
        if at + ring > n:
            pairs += [(at - 1, v) for v in range(at, n)] if at else _path(n)
            break
        pairs += _cycle(ring, at)
        if at:
            pairs.append((int(rng.randint(max(0, at - 4), at)), at))
        at += ring
        tail = int(rng.randint(0, 3))
        for _ in range(min(tail, n - at)):
            pairs.append((at - 1, at))
            at += 1
    return _both(sorted(set(pairs)))


_PETERSEN = _cycle(5) + [(i, i + 5) for i in range(5)] + [(5 + i, 5 + (i + 2) % 5) for i in range(5)]
_TRI_PATH = _cycle(3) + _path(4, 3)
SEED_LDS, SEED_OVER, SEED_MAX = 1, 2, 3

GRAPHS = [  # (name, n, edge_index, reason)
    ("one-node", 1, _both([]), "n < K"),
    ("edgeless-4", 4, _both([]), "all eigenvalues zero"),
    ("isolated-node", 5, _both(_path(4)), "isolated node"),
    ("path-9", 9, _both(_path(9)), "simple spectrum"),
    ("cycle-6", 6, _both(_cycle(6)), "pairs of equal eigenvalues"),
    ("cycle-12", 12, _both(_cycle(12)), "its 8th and 9th eigenvalues are equal: K = 8 cuts an eigenspace"),
    ("star-8", 8, _both([(0, i) for i in range(1, 8)]), "eigenvalue 1 six times"),
    ("K5", 5, _both([(i, j) for i in range(5) for j in range(i + 1, 5)]), "complete graph"),
    ("petersen", 10, _both(_PETERSEN), "K = 8 cuts the five-fold eigenspace"),
    ("triangle+path", 7, _both(_TRI_PATH), "two components"),
    ("triangle+path-directed", 7, np.array(_TRI_PATH, dtype=np.int64).T.copy(), "every edge listed once only"),
    ("triangle+path-self-loop", 7, np.concatenate([_both(_TRI_PATH), np.array([[2], [2]], dtype=np.int64)], 1), "a self-loop added"),
    ("molecule-37", 37, molecule_like(), "ZINC's largest size"),
    ("random-lds-limit", LDS_NODES, random_graph(LDS_NODES, SEED_LDS), "boundary of the LDS path"),
    ("random-over-lds", LDS_NODES + 1, random_graph(LDS_NODES + 1, SEED_OVER), "first size on the global-scratch path"),
    ("random-256", MAX_NODES, random_graph(MAX_NODES, SEED_MAX), "the size limit"),
]


def batch_of(graphs, empty_after=()):
    """the graphs as one batch: (edge_index with shifted ids, graph_ptr, edge_ptr, sizes); an empty graph (no nodes) follows
    every position listed in `empty_after`"""
    ei, gp, ep, sizes = [], [0], [0], []
    for i, (name, n, e, _) in enumerate(graphs):
        ei.append(e + gp[-1])
        gp.append(gp[-1] + n)
        ep.append(ep[-1] + e.shape[1])
        sizes.append(n)
        if i in empty_after:
            gp.append(gp[-1])
            ep.append(ep[-1])
            sizes.append(0)
    return np.concatenate(ei, 1), np.array(gp, dtype=np.int64), np.array(ep, dtype=np.int64), sizes


# ---- the encoder ----------------------------------------------------------------------------------------------------------------
class LapPEEncoder(torch.nn.Module):
    """the DeepSet LapPENodeEncoder with 2 layers, no post-MLP, no raw norm and expand_x False, constructed in the reference's
    order: Linear(2, dim_pe) first, replaced by Linear(2, 2 dim_pe), then Sequential(ReLU, Linear(2 dim_pe, dim_pe), ReLU)"""

    def __init__(self, dim_pe=8, max_freqs=8):
        super().__init__()
        nn = torch.nn
        self.linear_A = nn.Linear(2, dim_pe)
        self.linear_A = nn.Linear(2, 2 * dim_pe)
        self.pe_encoder = nn.Sequential(nn.ReLU(), nn.Linear(2 * dim_pe, dim_pe), nn.ReLU())

    def forward(self, eigvecs, eigvals, signs=None):
        """eigvecs [N, K], eigvals [N, K, 1] or [N, K], signs [K] or None -> [N, dim_pe]: per (node, frequency) the two-layer
        network on (v * sign, lambda) with NaNs read as 0, summed over the frequencies whose v is not NaN"""
        v = eigvecs if signs is None else eigvecs * signs.view(1, -1)
        lam = eigvals.reshape(v.shape)
        live = ~torch.isnan(v)
        pair = torch.stack([torch.nan_to_num(v, nan=0.0), torch.nan_to_num(lam, nan=0.0)], 2)
        h = self.pe_encoder(self.linear_A(pair))
        return (h * live.unsqueeze(2).to(h.dtype)).sum(1)


def stepwise_forward(enc, eigvecs, eigvals, signs=None):
    """the same result the long way, one tensor operation of the reference's forward at a time: scale by the signs, concatenate
    to [N, K, 2], take the NaN mask, zero the masked entries, linear_A, pe_encoder, zero the rows of masked frequencies on a
    copy, sum over the frequencies"""
    vec = eigvecs
    if signs is not None:
        vec = vec * signs.unsqueeze(0)
    pe = torch.cat((vec.unsqueeze(2), eigvals.reshape(vec.shape).unsqueeze(2)), dim=2)
    mask = torch.isnan(pe)
    pe = pe.clone()
    pe[mask] = 0
    pe = enc.pe_encoder(enc.linear_A(pe))
    pe = pe.clone().masked_fill_(mask[:, :, 0].unsqueeze(2), 0.0)
    return torch.sum(pe, 1, keepdim=False)


# ---- the model -------------------------------------------------------------------------------------------------------------------
class _Concat2(torch.nn.Module):
    def __init__(self, num_types, dim, dim_pe, max_freqs):
        super().__init__()
        self.encoder1 = go._TypeDict(num_types, dim - dim_pe)
        self.encoder2 = LapPEEncoder(dim_pe, max_freqs)


class _Encoder(torch.nn.Module):
    def __init__(self, dim, node_types, edge_types, dim_pe, max_freqs):
        super().__init__()
        self.node_encoder = _Concat2(node_types, dim, dim_pe, max_freqs)
        self.edge_encoder = go._TypeDict(edge_types, dim)


class GPSModel(torch.nn.Module):
    """gps_oracle.GPSModel with the node encoder TypeDictNode+LapPE: b carries EigVecs / EigVals too; `signs` stands for the
    training-time sign flip"""

    def __init__(self, layers=10, dim_hidden=64, n_heads=4, node_types=28, edge_types=4, dim_out=1, dim_pe=8, max_freqs=8):
        super().__init__()
        self.encoder = _Encoder(dim_hidden, node_types, edge_types, dim_pe, max_freqs)
        self.layers = torch.nn.Sequential(*[go.GPSLayer(dim_hidden, n_heads) for _ in range(layers)])
        self.post_mp = go._Head(dim_hidden, dim_out)

    def forward(self, b, signs=None):
        G = int(b["batch"][-1]) + 1
        sizes = torch.bincount(b["batch"], minlength=G).tolist()
        ne = self.encoder.node_encoder
        dtype = ne.encoder1.encoder.weight.dtype
        pe = ne.encoder2(b["EigVecs"].to(dtype), b["EigVals"].to(dtype), None if signs is None else signs.to(dtype))
        h = torch.cat([ne.encoder1.encoder(b["x"].view(b["x"].size(0), -1)[:, 0]), pe], 1)
        edge_attr = self.encoder.edge_encoder.encoder(b["edge_attr"].view(-1))
        for layer in self.layers:
            h, edge_attr = layer(h, edge_attr, b, sizes)
        g = torch.zeros((G, h.size(1)), dtype=h.dtype).index_add_(0, b["batch"], h)
        fc = self.post_mp.FC_layers
        return fc[2](torch.relu(fc[1](torch.relu(fc[0](g)))))
