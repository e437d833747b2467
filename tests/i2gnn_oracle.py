"""Oracle helpers of the I2GNN baseline (test infrastructure, CPU only), built on tests/ngnn_oracle.py.

* expand_graph2: the second-root expansion of ONE graph in numpy, restated from the reference's utils_edge_I2.py:132-256
  (create_subgraphs2), :371-472 (k_hop_subgraph), :475-561 (find_all_spd), :620-633 (compute_rd) and :726-813
  (subgraph_to_subgraph2_with_idx) with center_idx=True, node_label='spd', self_loop=False, in the canonical order the device
  kernels write (per root: the root, then ascending (hop, node id); sub-edges in batch order; copies in the order of the
  sub-edges that leave the root).  `rd` is computed the way the reference computes it — scipy's laplacian and pinv on the
  subgraph in the REFERENCE's node order, l_i + l_j - P - P.T in fp64 — and then permuted, so its values are met bit for bit.
* I2GNNRef: zinc_cycle_models.py:116-307 on the oracle primitives (GINConv of ngnn_oracle, global_mean_pool / global_add_pool
  of oracle/ref_model.py).
"""
import numpy as np
import torch
import torch.nn.functional as F

import ngnn_oracle as no
import ref_model as rm


def _rd_matrix(sub_src, sub_dst, m, pinv=None):
    """compute_rd (:620-633) in fp64: R[a, b] = ((P[a,a] + P[b,b]) - P[a,b]) - P[b,a]"""
    import scipy.sparse as ssp
    from scipy import linalg
    adj = ssp.coo_matrix((np.ones(len(sub_src)), (sub_src, sub_dst)), (m, m)).tocsr()
    lap = ssp.csgraph.laplacian(adj).toarray()
    P = (linalg.pinv if pinv is None else pinv)(lap)
    diag = P[list(range(m)), list(range(m))]
    l_i = np.tile(np.expand_dims(diag, axis=1), [1, m])
    l_j = np.tile(np.expand_dims(diag, axis=0), [m, 1])
    return l_i + l_j - P - P.T


def expand_graph2(n, src, dst, h, use_rd=False, pinv=None):
    src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
    keys = ("orig_node", "z", "node_to_subgraph2", "sub_src", "sub_dst", "orig_edge", "rd", "subgraph2_to_subgraph", "center_idx")
    out = {k: [] for k in keys}
    node_ptr, edge_ptr, s2_ptr, s2_node_ptr = [0], [0], [0], [0]
    for r in range(n):
        hop, paths, ref_order = no._bfs(n, src, dst, r, h)
        inside = hop >= 0
        order = np.array([r] + sorted((v for v in range(n) if inside[v] and v != r), key=lambda v: (hop[v], v)), dtype=np.int64)
        m = len(order)
        loc = np.full(n, -1, dtype=np.int64)
        loc[order] = np.arange(m)
        keep = np.nonzero(inside[src] & inside[dst])[0] if len(src) else np.zeros(0, dtype=np.int64)
        ls, lt = loc[src[keep]], loc[dst[keep]]                     # the sub-edges, canonical local ids
        z_root = no.labels(hop[order] + 1, paths[order], h, "spd")    # [m, 2]
        neighbours = lt[ls == 0]                                    # :728: targets of the sub-edges whose source is the root
        if use_rd:
            ref_loc = np.full(n, -1, dtype=np.int64)
            ref_loc[np.array(ref_order, dtype=np.int64)] = np.arange(m)
            R = _rd_matrix(ref_loc[src[keep]], ref_loc[dst[keep]], m, pinv)
            to_ref = ref_loc[order]
            R = R[np.ix_(to_ref, to_ref)]                           # canonical ids
        copies = list(neighbours) if len(neighbours) else [None]
        for j in copies:
            base, s2 = s2_node_ptr[-1], len(s2_node_ptr) - 1
            if j is None:                                           # :736-747
                z = np.tile(z_root, [1, 2])
                side = 0
            else:                                                   # :776-798: find_all_spd inside the subgraph, unbounded
                hj, pj, _ = no._bfs(m, ls, lt, int(j), m + 1)
                zj = np.where((hj >= 0)[:, None], no.labels(hj + 1, pj, h, "spd"), 0)
                z = np.concatenate([z_root, zj + h + 3], axis=1)
                side = int(j)
            out["orig_node"].append(order); out["z"].append(z)
            out["node_to_subgraph2"].append(np.full(m, s2, dtype=np.int64))
            out["sub_src"].append(ls + base); out["sub_dst"].append(lt + base); out["orig_edge"].append(keep)
            out["subgraph2_to_subgraph"].append(np.array([r], dtype=np.int64))
            out["center_idx"].append(np.array([[base, base + side]], dtype=np.int64))
            if use_rd:
                out["rd"].append(np.stack([R[0, :], R[side, :]], axis=1))
            s2_node_ptr.append(base + m)
        node_ptr.append(s2_node_ptr[-1]); edge_ptr.append(edge_ptr[-1] + len(copies) * len(keep)); s2_ptr.append(len(s2_node_ptr) - 1)

    def cat(k, dt=np.int64, shape=(0,)):
        return np.concatenate(out[k]).astype(dt) if out[k] else np.zeros(shape, dtype=dt)
    res = dict(orig_node=cat("orig_node"), z=cat("z", shape=(0, 4)), node_to_subgraph2=cat("node_to_subgraph2"),
               edge_index=np.stack([cat("sub_src"), cat("sub_dst")]), orig_edge=cat("orig_edge"),
               subgraph2_to_subgraph=cat("subgraph2_to_subgraph"), center_idx=cat("center_idx", shape=(0, 2)),
               sub_node_ptr=np.array(node_ptr, dtype=np.int64), sub_edge_ptr=np.array(edge_ptr, dtype=np.int64),
               sub2_ptr=np.array(s2_ptr, dtype=np.int64), s2_node_ptr=np.array(s2_node_ptr, dtype=np.int64))
    if use_rd:
        res["rd64"] = cat("rd", np.float64, (0, 2))
        res["rd"] = res["rd64"].astype(np.float32)
    return res


_PER_NODE = ("orig_node", "z", "node_to_subgraph2", "rd", "rd64", "batch")


def expand_batch2(node_counts, edge_lists, h, use_rd=False, pinv=None):
    """the expansion of several graphs laid end to end (batch_I2.py offsets): edge_lists hold graph-local ids"""
    parts, n_off, e_off, s_off, s2_off = [], 0, 0, 0, 0
    for g, (n, ei) in enumerate(zip(node_counts, edge_lists)):
        ei = np.asarray(ei, dtype=np.int64).reshape(2, -1)
        p = expand_graph2(n, ei[0], ei[1], h, use_rd, pinv)
        ns, n2 = len(p["orig_node"]), len(p["subgraph2_to_subgraph"])
        p["batch"] = np.full(ns, g, dtype=np.int64)
        p["orig_node"] = p["orig_node"] + n_off
        p["orig_edge"] = p["orig_edge"] + e_off
        p["node_to_subgraph2"] = p["node_to_subgraph2"] + s2_off
        p["subgraph2_to_subgraph"] = p["subgraph2_to_subgraph"] + n_off
        p["edge_index"] = p["edge_index"] + s_off
        p["center_idx"] = p["center_idx"] + s_off
        parts.append(p)
        n_off, e_off, s_off, s2_off = n_off + n, e_off + ei.shape[1], s_off + ns, s2_off + n2
    out = {}
    for k in parts[0]:
        if k.endswith("_ptr"):
            acc, off = [np.zeros(1, dtype=np.int64)], 0
            for p in parts:
                acc.append(p[k][1:] + off)
                off += int(p[k][-1])
            out[k] = np.concatenate(acc)
        else:
            out[k] = np.concatenate([p[k] for p in parts], axis=-1 if k == "edge_index" else 0)
    out["subgraph_to_graph"] = np.repeat(np.arange(len(node_counts), dtype=np.int64), node_counts)
    return out


class I2GNNRef(torch.nn.Module):
    """Same module tree, construction order and state_dict keys as the reference's I2GNN (use_pos / RNI / virtual node off)."""

    def __init__(self, num_layers=5, subgraph_pooling="mean", subgraph2_pooling="mean", use_pooling_nn=False, use_rd=False,
                 double_pooling=False, gate=False):
        super().__init__()
        nn = torch.nn
        self.subgraph_pooling, self.subgraph2_pooling = subgraph_pooling, subgraph2_pooling
        s2_dim = 2 if subgraph2_pooling == "mean-center" else 3 if subgraph2_pooling == "mean-center-side" else 1
        s2_dim = s2_dim + 1 if subgraph_pooling == "mean-context" else s2_dim
        self.use_rd, self.double_pooling, self.gate, self.use_pooling_nn = use_rd, double_pooling, gate, use_pooling_nn
        if use_rd:
            self.rd_projection = nn.Linear(2, 8)
        self.node_type_embedding = nn.Embedding(100, 8)
        if gate:
            self.subgraph_gate = nn.ModuleList()
        self.convs, self.norms, self.z_embedding_list = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        if use_rd:
            self.rd_projection_list = nn.ModuleList()
        if double_pooling:
            self.double_nns = nn.ModuleList()
        M_in, M_out = 9, 64
        for layer in range(num_layers):
            if layer == 0:
                self.convs.append(no.GINConv(2 * M_in, M_out))
            self.z_embedding_list.append(nn.Embedding(100, M_in))
            if use_rd:
                self.rd_projection_list.append(nn.Linear(2, M_in))
            if gate:
                self.subgraph_gate.append(nn.Sequential(nn.Linear(M_in, M_out), nn.Sigmoid()))
            if layer > 0:
                self.convs.append(no.GINConv(2 * M_in, M_out))
            self.norms.append(nn.BatchNorm1d(M_out))
            if double_pooling:
                self.double_nns.append(nn.Sequential(nn.Linear(M_out * (1 + s2_dim), 128), nn.ReLU(), nn.Linear(128, M_out)))
            M_in, M_out = M_out, 64
        if use_pooling_nn:
            w = s2_dim * M_out
            self.edge_pooling_nn = nn.Sequential(nn.Linear(w, w), nn.ReLU(), nn.Linear(w, w))
            self.node_pooling_nn = nn.Sequential(nn.Linear(w, w), nn.ReLU(), nn.Linear(w, w))
        self.z_embedding_list.append(nn.Embedding(100, M_out))
        if use_rd:
            self.rd_projection_list.append(nn.Linear(2, M_out))
        if gate:
            self.subgraph_gate.append(nn.Sequential(nn.Linear(M_out, M_out), nn.Sigmoid()))
        self.fc1, self.fc2, self.fc3 = nn.Linear(s2_dim * M_out, 32), nn.Linear(32, 16), nn.Linear(16, 1)

    def graph_pooling(self, x, b, z, layer, node_emb_only=False):
        n2s2, s2s, ci = b["node_to_subgraph2"], b["subgraph2_to_subgraph"], b["center_idx"]
        if self.subgraph_pooling == "mean-context":
            x_node = rm.global_mean_pool(x, b["node_to_original_node"])       # (index_add: the index need not be sorted)
        p2 = self.subgraph2_pooling
        if p2 == "mean":
            if self.gate:
                x = self.subgraph_gate[layer](z) * x
            x = rm.global_mean_pool(x, n2s2)
        elif p2 == "add":
            x = rm.global_add_pool(x, n2s2)
        elif p2 == "center":
            x = x[ci[:, 0]]
        elif p2 == "mean-center":
            first = np.unique(n2s2.numpy(), return_index=True)[1]
            x = torch.cat([rm.global_mean_pool(x, n2s2), x[first]], dim=-1)
        elif p2 == "mean-center-side":
            if self.gate:
                x = self.subgraph_gate[layer](z) * x
            x = torch.cat([rm.global_mean_pool(x, n2s2), x[ci[:, 0]], x[ci[:, 1]]], dim=-1)
        if self.use_pooling_nn:
            x = self.edge_pooling_nn(x)
        if self.subgraph_pooling == "mean":
            x = rm.global_mean_pool(x, s2s)
        elif self.subgraph_pooling == "add":
            x = rm.global_add_pool(x, s2s)
        else:
            x = torch.cat([rm.global_mean_pool(x, s2s), x_node], dim=-1)
        if node_emb_only:
            return x
        if self.use_pooling_nn:
            x = self.node_pooling_nn(x)
        return x                                                    # aggr = 'no': node level

    def forward(self, b):
        dt = self.fc1.weight.dtype
        x = torch.cat([self.node_type_embedding(b["x"]), b["x"].view(-1, 1).to(dt)], -1)
        x0 = None

        def z_of(layer):
            z_emb = self.z_embedding_list[layer](b["z"]).sum(dim=1)
            return z_emb + self.rd_projection_list[layer](b["rd"].to(dt)) if self.use_rd else z_emb
        for layer, conv in enumerate(self.convs):
            z_emb = z_of(layer)
            x = conv(torch.cat([x, z_emb], dim=-1), b["edge_index"], b["edge_attr"])
            if self.double_pooling:
                ctxt = self.graph_pooling(x, b, z_emb, layer, node_emb_only=True)[b["node_to_original_node"]]
                x = self.double_nns[layer](torch.cat([x, ctxt], dim=-1))
            x = self.norms[layer](x)
            if layer < len(self.convs) - 1:
                x = F.elu(x)
            if layer > 0:
                x = x + x0
            x0 = x
        x = self.graph_pooling(x, b, z_of(-1), -1)
        return self.fc3(F.elu(self.fc2(F.elu(self.fc1(x)))))


CONFIGS = {   # the three recorded configurations: constructor keywords of I2GNN
    "default": dict(subgraph_pooling="mean-context", subgraph2_pooling="mean-center-side", use_pooling_nn=False, use_rd=True,
                    double_pooling=True, gate=True),
    "bare": dict(subgraph_pooling="mean", subgraph2_pooling="mean", use_pooling_nn=False, use_rd=False, double_pooling=False,
                 gate=False),
    "poolnn": dict(subgraph_pooling="add", subgraph2_pooling="mean-center", use_pooling_nn=True, use_rd=False,
                   double_pooling=False, gate=False),
}


def i2gnn_from_recipe(seed, layers, tag):
    torch.manual_seed(int(seed))
    return no.perturb(I2GNNRef(int(layers), **CONFIGS[tag]))
