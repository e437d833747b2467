"""Node-rooted h-hop subgraph expansion of a collated batch on the device (csrc/subgraphs.hip) — what feeds the NGNN
baseline.  The reference materialises every rooted subgraph once per dataset on the host (utils.py:18-132, a python loop
with one scipy pinv per root) and collates them per batch (batch_I2.py:61-66); here a plain batch is expanded per step.

Canonical order: the sub-nodes of a root are the root, then ascending (hop, node id); the sub-edges keep the
order of the batch's edges.  Field names are the reference's.
"""
import numpy as np
import torch

from . import _native as nv
from .batch import Batch
from .data import Data
from .utils_edge_efficient import _check_args

H_MAX = 98                   # z = hop + 1 indexes the model's 100-row tables
MAX_NODES = 4096
RD_MAX_NODES = 96            # largest subgraph whose two m x m fp64 matrices fit the LDS of one wave's workgroup
NODE_LABELS = ("spd", "drnl")


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("esc_gnn_amd.subgraphs needs a HIP device (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def collate_graphs(data_list, device=None):
    """Host collate of plain graphs (x, edge_index, edge_attr, y): one concatenation per key and one copy to the device.
    The batch carries its int64 node / edge pointers (device and host) so that the expansion derives nothing."""
    dev = _device() if device is None else torch.device(device)
    G = len(data_list)
    if G == 0:
        raise ValueError("collate_graphs: empty list")
    n = np.array([int(d.num_nodes) for d in data_list], dtype=np.int64)
    e = np.array([int(d.edge_index.size(1)) for d in data_list], dtype=np.int64)
    node_ptr, edge_ptr = np.zeros(G + 1, dtype=np.int64), np.zeros(G + 1, dtype=np.int64)
    np.cumsum(n, out=node_ptr[1:])
    np.cumsum(e, out=edge_ptr[1:])
    ei = torch.cat([d.edge_index.reshape(2, -1).to(torch.int64) for d in data_list], dim=1)
    ei += torch.from_numpy(np.repeat(node_ptr[:-1], e)).view(1, -1)
    out = Batch()
    if data_list[0].x is not None:
        out.x = torch.cat([d.x for d in data_list], dim=0).to(dev)
    out.edge_index = ei.to(dev)
    if data_list[0].edge_attr is not None:
        out.edge_attr = torch.cat([d.edge_attr for d in data_list], dim=0).to(dev)
    if data_list[0].y is not None:
        out.y = torch.cat([d.y.reshape(-1) if d.y.dim() <= 1 else d.y for d in data_list], dim=0).to(dev)
    out.batch = torch.from_numpy(np.repeat(np.arange(G, dtype=np.int64), n)).to(dev)
    object.__setattr__(out, "_num_graphs", G)
    ptrs = torch.from_numpy(np.stack([node_ptr, edge_ptr])).to(dev)
    object.__setattr__(out, "_esc_sub_ptrs", (ptrs[0], ptrs[1], node_ptr, edge_ptr, int(n.max())))
    seg = ptrs[0].to(torch.int32)
    out.batch._esc_seg = {(out.batch._version, None): seg, (out.batch._version, G): seg}     # pooling: no rebuild, no read-back
    return out


def _pointers(batch, G_known=None):
    """(node_ptr, edge_ptr int64 on the device, G, total_nodes, total_edges, max_nodes or None)"""
    tag = object.__getattribute__(batch, "__dict__").get("_esc_sub_ptrs")
    N, E = int(batch.batch.numel()), int(batch.edge_index.size(1))
    if tag is not None and int(tag[2][-1]) == N and int(tag[3][-1]) == E:
        return tag[0], tag[1], len(tag[2]) - 1, N, E, tag[4]
    from .plan import _csr
    b = batch.batch
    if b.device.type != "cuda":
        raise RuntimeError("esc_gnn_amd.subgraphs: the batch must be on the HIP device (batch.to(device)); there is no CPU fallback")
    G = int(G_known) if G_known is not None else (int(b[-1].item()) + 1 if N else 0)      # (a read-back without `sizes`)
    bad = torch.zeros(2, dtype=torch.int32, device=b.device)
    node_ptr = _csr(b, max(G, 1), want_perm=False, bad=bad[0:1])[0].to(torch.int64)
    edge_ptr = _csr(b[batch.edge_index[0]], max(G, 1), want_perm=False, bad=bad[1:2])[0].to(torch.int64)
    return node_ptr, edge_ptr, G, N, E, None                   # (a bad key shows up as ESC_ERANGE in the status of its graph)


def _count(batch, h, G_known=None, max_nodes=None):
    h = _check_h(h)
    node_ptr, edge_ptr, G, N, E, nmax = _pointers(batch, G_known)
    if nmax is None:
        nmax = max_nodes
    if nmax is None:
        nmax = int((node_ptr[1:] - node_ptr[:-1]).max().item()) if G else 1
    if nmax > MAX_NODES:
        raise ValueError("subgraphs: a graph of %d nodes exceeds the limit of %d nodes per graph" % (nmax, MAX_NODES))
    dev = batch.edge_index.device
    ei = batch.edge_index
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    sub_node_ptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    sub_edge_ptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)
    nv.call("esc_subgraph_count", nv.ptr(node_ptr), nv.ptr(edge_ptr), nv.ptr(src), nv.ptr(dst), G, N, E, max(int(nmax), 1), h,
            nv.ptr(sub_node_ptr), nv.ptr(sub_edge_ptr), nv.ptr(status), nv.stream())
    return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, G=G, N=N, E=E, nmax=max(int(nmax), 1), src=src, dst=dst,
                sub_node_ptr=sub_node_ptr, sub_edge_ptr=sub_edge_ptr, status=status, h=h)


def _check_h(h):
    h = _check_args(h, None, None)
    if h < 1 or h > H_MAX:
        raise ValueError("subgraphs: h=%d outside 1..%d (the model's z tables have 100 rows and z = hop + 1)" % (h, H_MAX))
    return h


def _raise_status(c, what):
    """raise for the first graph whose status is set, naming what it hit: a graph the COUNT pass refused has zero-length
    output ranges; one that was counted can only have failed in the fill pass"""
    st = c["status"].cpu()
    if bool((st != 0).any()):
        g = int(torch.nonzero(st)[0])
        a, b = (int(v) for v in c["node_ptr"][g:g + 2].tolist())
        counted = a < b and int(c["sub_node_ptr"][b]) > int(c["sub_node_ptr"][a])
        if counted:
            why = ("with use_rd, a subgraph of more than %d nodes (both m x m matrices of the pseudo-inverse must fit LDS), or "
                   "output totals that are not those of the count pass" % RD_MAX_NODES)
        else:
            why = ("a node id outside the graph, edges of one graph not contiguous, or a graph of more than %d nodes (limit %d)"
                   % (c["nmax"], MAX_NODES))
        raise ValueError("%s: graph %d cannot be expanded (status %d): %s" % (what, g, int(st[g]), why))


def subgraph_sizes(batch_or_list, h, chunk=4096, with_largest=False):
    """The count pass alone: int64 [G, 2] on the host, per graph (sub-nodes, sub-edges) of its rooted subgraphs.
    with_largest: also the node count of the largest single subgraph (what the rd limit of 96 is about)."""
    if isinstance(batch_or_list, (list, tuple)):
        parts = [subgraph_sizes(collate_graphs(batch_or_list[i:i + chunk]), h, with_largest=True)
                 for i in range(0, len(batch_or_list), chunk)]
        sizes = torch.cat([p[0] for p in parts], dim=0) if parts else torch.zeros((0, 2), dtype=torch.int64)
        return (sizes, max([p[1] for p in parts] or [0])) if with_largest else sizes
    c = _count(batch_or_list, h)
    _raise_status(c, "subgraph_sizes")
    at = c["node_ptr"]
    both = torch.stack([c["sub_node_ptr"][at], c["sub_edge_ptr"][at]], dim=1).cpu()
    sizes = both[1:] - both[:-1]
    if not with_largest:
        return sizes
    per_root = c["sub_node_ptr"][1:] - c["sub_node_ptr"][:-1]
    return sizes, (int(per_root.max()) if per_root.numel() else 0)


def expand_subgraphs(batch, h, node_label="spd", use_rd=False, sizes=None, max_nodes_per_hop=None,
                     subgraph_pretransform=None, check=None, max_nodes=None):
    """The rooted subgraphs of every node of a collated batch as one disconnected graph, on the batch's device.
    sizes: the batch's rows of a `subgraph_sizes` result (known on the host from the dataset build) — the output sizes are
    their sums and nothing is read back; without it the two totals are copied once.  check: read the per-graph status back
    and raise (default: only when `sizes` is absent, where the call synchronises anyway; with `sizes` the status tensor is
    returned as `status` and a bad graph simply has no rows; PlainGraphStore has checked the rd limit at build).
    max_nodes: the largest node count of a graph of the batch, when the host knows it and the batch does not carry the
    collate's pointers; without it and with `sizes`, a bound from `sizes` sizes the LDS tables (correct, but generous)."""
    _check_args(h, max_nodes_per_hop, subgraph_pretransform)
    if node_label == "hop":
        raise ValueError("node_label='hop' yields a dict of per-h graphs in the reference and cannot be batched; use 'spd' or 'drnl'")
    if node_label not in NODE_LABELS:
        raise ValueError("node_label=%r: one of %s" % (node_label, NODE_LABELS))
    h = _check_h(h)
    G_known = None
    if sizes is not None:
        sizes = torch.as_tensor(sizes, dtype=torch.int64).reshape(-1, 2)
        G_known = int(sizes.size(0))
    if max_nodes is None and sizes is not None:           # n_g <= its sub-node total: an upper bound known on the host
        max_nodes = min(MAX_NODES, int(sizes[:, 0].max()) if G_known else 1)
    c = _count(batch, h, G_known, max_nodes)
    if G_known is not None and G_known != c["G"]:
        raise ValueError("expand_subgraphs: sizes has %d rows for a batch of %d graphs" % (G_known, c["G"]))
    if sizes is not None:
        Ns, Es = int(sizes[:, 0].sum()), int(sizes[:, 1].sum())
    else:
        N = c["N"]
        Ns, Es = (int(v) for v in torch.stack([c["sub_node_ptr"][N], c["sub_edge_ptr"][N]]).tolist())
    if Ns >= 2 ** 31 - 1 or Es >= 2 ** 31 - 1:
        raise ValueError("expand_subgraphs: %d sub-nodes / %d sub-edges: totals must stay below 2^31" % (Ns, Es))
    dev = batch.edge_index.device
    nodes = torch.empty((5, Ns), dtype=torch.int64, device=dev)       # orig_node | hop + 1 | paths | node_to_subgraph | graph
    edges = torch.empty((3, Es), dtype=torch.int64, device=dev)       # sub_src | sub_dst | orig_edge
    rd = torch.empty((Ns, 1), dtype=torch.float32, device=dev) if use_rd else None
    nv.call("esc_subgraph_fill", nv.ptr(c["node_ptr"]), nv.ptr(c["edge_ptr"]), nv.ptr(c["src"]), nv.ptr(c["dst"]), c["G"], c["N"],
            c["E"], c["nmax"], h, nv.ptr(c["sub_node_ptr"]), nv.ptr(c["sub_edge_ptr"]), Ns, Es, int(bool(use_rd)),
            nv.ptr(nodes[0]), nv.ptr(nodes[1]), nv.ptr(nodes[2]), nv.ptr(nodes[3]), nv.ptr(nodes[4]), nv.ptr(edges[0]),
            nv.ptr(edges[1]), nv.ptr(edges[2]), nv.ptr(rd), nv.ptr(c["status"]), nv.stream())
    if check is None:
        check = sizes is None
    if check:
        _raise_status(c, "expand_subgraphs")
    out = Data()
    orig_node, hop1, paths, orig_edge = nodes[0], nodes[1], nodes[2], edges[2]
    # the reference's label list holds hop + 1 once per frontier edge into the node (utils.py:163-167): spd keeps two entries,
    # drnl folds the first two into d1 * (h + 1) + d2
    if node_label == "spd":
        out.z = torch.stack([hop1, torch.where(paths >= 2, hop1, torch.zeros_like(hop1))], dim=1)
        out.z._esc_known_range = (([1, 0], [h + 1, h + 1]), out.z._version)
    else:
        out.z = torch.where(paths >= 2, hop1 * (h + 2), hop1).view(-1, 1)
        out.z._esc_known_range = (([1], [(h + 1) * (h + 2)]), out.z._version)
    if batch.x is not None:
        out.x = batch.x[orig_node]
    out.edge_index = edges[:2]
    if batch.edge_attr is not None:
        out.edge_attr = batch.edge_attr[orig_edge]
    out.node_to_subgraph, out.subgraph_to_graph, out.batch = nodes[3], batch.batch, nodes[4]
    out.num_subgraphs = c["N"]
    out.num_nodes = Ns
    if use_rd:
        out.rd = rd
    if batch.y is not None:
        out.y = batch.y
    out.orig_node, out.orig_edge = orig_node, orig_edge
    out.sub_node_ptr, out.sub_edge_ptr, out.status = c["sub_node_ptr"], c["sub_edge_ptr"], c["status"]
    seg = c["sub_node_ptr"].to(torch.int32)                           # mean pooling over the subgraphs: no rebuild, no read-back
    v = out.node_to_subgraph._version
    out.node_to_subgraph._esc_seg = {(v, None): seg, (v, c["N"]): seg}
    return out


class PlainGraphStore(object):
    """A split of plain graphs for the NGNN run: host collate per batch (the device store keeps ESC bag tensors and does
    not take graphs without them) and the per-graph subgraph sizes from ONE count pass at build time, so that
    no training step reads a size back.  The same pass gives the largest single subgraph: `expand(use_rd=True)` refuses a
    split that the rd limit of 96 nodes does not cover, on the host, instead of training on unwritten rd rows."""

    def __init__(self, data_list, h, device=None):
        if len(data_list) == 0:
            raise ValueError("PlainGraphStore: empty dataset")
        self.graphs, self.h = list(data_list), int(h)
        self.device = _device() if device is None else torch.device(device)
        self.sizes, self.largest_subgraph = subgraph_sizes(self.graphs, h, with_largest=True)

    def __len__(self):
        return len(self.graphs)

    def collate(self, graph_ids):
        ids = torch.as_tensor(graph_ids, dtype=torch.int64).reshape(-1)
        if ids.numel() == 0:
            raise ValueError("collate: empty batch")
        out = collate_graphs([self.graphs[i] for i in ids.tolist()], self.device)
        object.__setattr__(out, "_esc_sub_sizes", self.sizes[ids])
        return out

    def expand(self, batch, node_label="spd", use_rd=False):
        if use_rd and self.largest_subgraph > RD_MAX_NODES:
            raise ValueError("PlainGraphStore: use_rd with a subgraph of %d nodes at h=%d: rd covers subgraphs of at most %d nodes"
                             % (self.largest_subgraph, self.h, RD_MAX_NODES))
        return expand_subgraphs(batch, self.h, node_label, use_rd, object.__getattribute__(batch, "__dict__").get("_esc_sub_sizes"))
