"""Oracle helpers of the NGNN baseline (test infrastructure, CPU only).

* expand_graph: the rooted-subgraph expansion of ONE graph in numpy, restated from the reference's utils.py:18-132 /
  k_hop_subgraph :135-229 and put into the canonical order the device kernels write (root, then ascending (hop, node id);
  sub-edges in their original order).  `rd` is computed the way the reference computes it — scipy's csgraph.laplacian and
  scipy.linalg.pinv on the subgraph in the REFERENCE's node order (the iteration order of a CPython set of the level's new
  nodes, rebuilt here with the same set operations) — and then permuted, so the reference's values are met bit for bit.
* labels: the reference's spd / drnl label columns from (hop + 1, number of frontier edges into the node).
* GINConv / NGNNRef: zinc_models.py:615-645 and :306-405 on the oracle primitives of oracle/ref_model.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

import ref_model as rm


def _bfs(n, src, dst, root, h):
    """hop[x] (or -1), the number of frontier edges into x, and the reference's subset order"""
    hop = np.full(n, -1, dtype=np.int64)
    paths = np.zeros(n, dtype=np.int64)
    hop[root] = 0
    subsets, visited, frontier = [[root]], {root}, np.zeros(n, dtype=bool)
    for d in range(1, h + 1):
        frontier[:] = False
        frontier[subsets[-1]] = True
        tmp = [int(v) for v in src[frontier[dst]] if int(v) not in visited]      # col[edge_mask], walking target -> source
        if not tmp:
            break
        for v in tmp:
            paths[v] += 1
        new = set(tmp)
        visited = visited.union(new)
        new = list(new)                                    # the reference's order inside a level: CPython set iteration
        hop[new] = d
        subsets.append(new)
    return hop, paths, [v for s in subsets for v in s]


def _rd(sub_src, sub_dst, m, pinv=None):
    """the reference's :61-73 on a subgraph whose root is local node 0, in fp64 (the reference then casts to fp32);
    pinv: scipy.linalg.pinv as in the reference, or another implementation to compare it with"""
    import scipy.sparse as ssp
    from scipy import linalg
    adj = ssp.coo_matrix((np.ones(len(sub_src)), (sub_src, sub_dst)), (m, m)).tocsr()
    lap = ssp.csgraph.laplacian(adj).toarray()
    P = (linalg.pinv if pinv is None else pinv)(lap)
    idx = list(range(m))
    return P[0, 0] + P[idx, idx] - P[0, :] - P[:, 0]


def expand_graph(n, src, dst, h, use_rd=False, pinv=None):
    src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
    out = dict(orig_node=[], z=[], paths=[], node_to_subgraph=[], sub_src=[], sub_dst=[], orig_edge=[], rd=[])
    node_ptr, edge_ptr = [0], [0]
    for r in range(n):
        hop, paths, ref_order = _bfs(n, src, dst, r, h)
        inside = hop >= 0
        order = np.array([r] + sorted((v for v in range(n) if inside[v] and v != r), key=lambda v: (hop[v], v)), dtype=np.int64)
        loc = np.full(n, -1, dtype=np.int64)
        loc[order] = np.arange(len(order))
        keep = np.nonzero(inside[src] & inside[dst])[0] if len(src) else np.zeros(0, dtype=np.int64)
        base = node_ptr[-1]
        out["orig_node"].append(order); out["z"].append(hop[order] + 1); out["paths"].append(paths[order])
        out["node_to_subgraph"].append(np.full(len(order), r, dtype=np.int64))
        out["sub_src"].append(loc[src[keep]] + base); out["sub_dst"].append(loc[dst[keep]] + base); out["orig_edge"].append(keep)
        if use_rd:
            ref_loc = np.full(n, -1, dtype=np.int64)
            ref_loc[np.array(ref_order, dtype=np.int64)] = np.arange(len(ref_order))
            rd_ref = _rd(ref_loc[src[keep]], ref_loc[dst[keep]], len(order), pinv)
            out["rd"].append(rd_ref[ref_loc[order]])
        node_ptr.append(base + len(order)); edge_ptr.append(edge_ptr[-1] + len(keep))
    cat = lambda k, dt=np.int64: np.concatenate(out[k]).astype(dt) if out[k] else np.zeros(0, dtype=dt)   # noqa: E731
    res = dict(orig_node=cat("orig_node"), z=cat("z"), paths=cat("paths"), node_to_subgraph=cat("node_to_subgraph"),
               edge_index=np.stack([cat("sub_src"), cat("sub_dst")]), orig_edge=cat("orig_edge"),
               sub_node_ptr=np.array(node_ptr, dtype=np.int64), sub_edge_ptr=np.array(edge_ptr, dtype=np.int64))
    if use_rd:
        res["rd64"] = cat("rd", np.float64)
        res["rd"] = res["rd64"].astype(np.float32)
    return res


def labels(z, paths, h, node_label="spd"):
    """utils.py:192-216: the label list of a node holds hop + 1 once per frontier edge into it"""
    z, paths = np.asarray(z, dtype=np.int64), np.asarray(paths, dtype=np.int64)
    if node_label == "spd":
        return np.stack([z, np.where(paths >= 2, z, 0)], axis=1)
    return np.where(paths >= 2, z * (h + 1) + z, z).reshape(-1, 1)


def expand_batch(node_counts, edge_lists, h, use_rd=False, pinv=None):
    """the expansion of several graphs laid end to end (batch_I2.py:61-66 offsets): edge_lists hold graph-local ids"""
    parts, n_off, e_off, s_off = [], 0, 0, 0
    for g, (n, ei) in enumerate(zip(node_counts, edge_lists)):
        ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
        p = expand_graph(n, ei[0], ei[1], h, use_rd, pinv)
        ns = len(p["orig_node"])
        p["batch"] = np.full(ns, g, dtype=np.int64)
        p["orig_node"] = p["orig_node"] + n_off
        p["orig_edge"] = p["orig_edge"] + e_off
        p["node_to_subgraph"] = p["node_to_subgraph"] + n_off
        p["edge_index"] = p["edge_index"] + s_off
        parts.append(p)
        n_off, e_off, s_off = n_off + n, e_off + ei.shape[1], s_off + ns
    out = {k: np.concatenate([p[k] for p in parts], axis=-1) for k in parts[0] if not k.endswith("_ptr")}
    for k in ("sub_node_ptr", "sub_edge_ptr"):
        acc, off = [np.zeros(1, dtype=np.int64)], 0
        for p in parts:
            acc.append(p[k][1:] + off)
            off += int(p[k][-1])
        out[k] = np.concatenate(acc)
    return out


class GINConv(torch.nn.Module):
    def __init__(self, M_in, M_out):
        super().__init__()
        self.mlp = torch.nn.Sequential(torch.nn.Linear(M_in, 2 * M_in), torch.nn.BatchNorm1d(2 * M_in), torch.nn.ReLU(),
                                       torch.nn.Linear(2 * M_in, M_out))
        self.eps = torch.nn.Parameter(torch.Tensor([0]))
        self.edge_encoder = torch.nn.Embedding(5, M_in)

    def forward(self, x, edge_index, edge_attr):
        e = self.edge_encoder(edge_attr)
        msg = F.relu(x.index_select(0, edge_index[0]) + e)
        return self.mlp((1 + self.eps) * x + torch.zeros_like(x).index_add_(0, edge_index[1], msg))


class NGNNRef(torch.nn.Module):
    """Same module tree, construction order and state_dict keys as the reference's NGNN (use_pos / RNI off)."""

    def __init__(self, num_layers=5, subgraph_pooling="mean", use_rd=False):
        super().__init__()
        self.subgraph_pooling, self.use_rd = subgraph_pooling, use_rd
        if use_rd:
            self.rd_projection_list = torch.nn.ModuleList()
        self.z_embedding_list = torch.nn.ModuleList()
        self.node_type_embedding = torch.nn.Embedding(100, 8)
        self.norms = torch.nn.ModuleList()
        self.convs = torch.nn.ModuleList()
        M_in, M_out = 9, 64
        for _ in range(num_layers):
            self.z_embedding_list.append(torch.nn.Embedding(100, M_in))
            if use_rd:
                self.rd_projection_list.append(torch.nn.Linear(1, M_in))
            self.convs.append(GINConv(2 * M_in, M_out))
            self.norms.append(torch.nn.BatchNorm1d(M_out))
            M_in, M_out = M_out, 64
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(M_out, 32), torch.nn.Linear(32, 16), torch.nn.Linear(16, 1)

    def forward(self, x, z, rd, edge_index, edge_attr, node_to_subgraph, subgraph_to_graph):
        dt = self.fc1.weight.dtype
        h = torch.cat([self.node_type_embedding(x), x.view(-1, 1).to(dt)], -1)
        h0 = None
        for layer, conv in enumerate(self.convs):
            z_emb = self.z_embedding_list[layer](z)
            if z_emb.ndim == 3:
                z_emb = z_emb.sum(dim=1)
            if self.use_rd:
                z_emb = z_emb + self.rd_projection_list[layer](rd.to(dt))
            h = F.elu(self.norms[layer](conv(torch.cat([h, z_emb], dim=-1), edge_index, edge_attr)))
            if layer > 0:
                h = h + h0
            h0 = h
        if self.subgraph_pooling == "center":
            first = np.unique(node_to_subgraph.numpy(), return_index=True)[1]
            h = h[first]
        else:
            h = rm.global_mean_pool(h, node_to_subgraph)
        h = rm.global_mean_pool(h, subgraph_to_graph)
        return self.fc3(F.elu(self.fc2(F.elu(self.fc1(h)))))


def perturb(m):
    """0.1 * randn on every 1-d non-bias parameter (BatchNorm weights, eps), so that each one matters"""
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1 and "bias" not in name:
                p.add_(0.1 * torch.randn_like(p))
    return m


def ngnn_from_recipe(seed, layers, pooling, use_rd):
    torch.manual_seed(int(seed))
    return perturb(NGNNRef(int(layers), pooling, bool(use_rd)))


def model_args(b):
    return (b["x"], b["z"], b.get("rd"), b["edge_index"], b["edge_attr"], b["node_to_subgraph"], b["subgraph_to_graph"])
