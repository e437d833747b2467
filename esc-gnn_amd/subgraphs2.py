"""Second-root expansion of a collated batch on the device (csrc/subgraphs.hip, esc_subgraph2_*) — what feeds the I2GNN
baseline.  The reference builds it once per dataset on the host (utils_edge_I2.py:132-256: per node a rooted subgraph, then
one copy per neighbour of the root with a find_all_spd BFS each, :726-813, and one scipy pinv per node); here a plain batch
is expanded per step.

Every rooted subgraph S_i of `subgraphs.expand_subgraphs` appears max(K_i, 1) times, once per neighbour j of its root (the
targets of the sub-edges that leave the root, in sub-edge order); a copy is a "subgraph2" and labels every node with its
distances to i and to j.  Field names are the reference's; `center_idx=True`, `node_label='spd'`,
`self_loop=False` are the only settings.
"""
import torch

from . import _native as nv
from .data import Data
from .expansion import (GraphStore, _below_2_31, _column_totals, _count_prologue, _known_sizes, _sizes_of_list, _tag_segments,
                        _wants_check, collate_graphs)
from .subgraphs import _raise_status, _refuse_rd
from .utils_edge_efficient import _check_args

H_MAX = 47                   # labels of the second root reach 2h + 5 on symmetric graphs; the model's tables have 100 rows
MAX_NODES = 1536             # 9 B of LDS tables per node beside the two 96 x 96 fp64 matrices of the pseudo-inverse


def check_args(h, node_label="spd", max_nodes_per_hop=None, subgraph_pretransform=None, self_loop=False):
    """h as an int in 1..H_MAX; raises for what the I2GNN expansion has no path for"""
    if self_loop:
        raise NotImplementedError("self_loop: the reference's node_to_original_node has the wrong length with --self_loop "
                                  "(utils_edge_I2.py:193-196 counts the root's degree without the loop); I2GNN runs without it")
    if node_label != "spd":
        raise ValueError("node_label=%r: the I2GNN expansion labels with 'spd' only" % (node_label,))
    if max_nodes_per_hop is not None:
        raise NotImplementedError("max_nodes_per_hop: random neighbour sampling is outside the ESC hot path")
    if subgraph_pretransform is not None:
        raise NotImplementedError("subgraph_pretransform: the k-GNN pre-transform has no path here")
    h = _check_args(h, None, None)
    if h < 1 or h > H_MAX:
        raise ValueError("subgraphs2: h=%d outside 1..%d (the model's z tables have 100 rows and the second root's labels "
                         "reach 2h + 5)" % (h, H_MAX))
    return h


def _count(batch, h, G_known=None, max_nodes=None):
    c = _count_prologue(batch, MAX_NODES, "subgraphs2", G_known, max_nodes)
    # sub-node | sub-edge | subgraph2 pointers per root
    ptrs = torch.empty((3, c["N"] + 1), dtype=torch.int64, device=batch.edge_index.device)
    nv.call("esc_subgraph2_count", nv.ptr(c["node_ptr"]), nv.ptr(c["edge_ptr"]), nv.ptr(c["src"]), nv.ptr(c["dst"]), c["G"], c["N"],
            c["E"], c["nmax"], h, nv.ptr(ptrs[0]), nv.ptr(ptrs[1]), nv.ptr(ptrs[2]), nv.ptr(c["status"]), nv.stream())
    c.update(ptrs=ptrs, sub_node_ptr=ptrs[0], sub_edge_ptr=ptrs[1], sub2_ptr=ptrs[2], h=h)
    return c


def subgraph2_sizes(batch_or_list, h, chunk=4096, with_largest=False):
    """The count pass alone: int64 [G, 3] on the host, per graph (sub-nodes, sub-edges, subgraph2s) over all its roots and
    copies.  with_largest: also the node count of the largest single rooted subgraph (what the rd limit of 96 is about)."""
    h = check_args(h)
    if isinstance(batch_or_list, (list, tuple)):
        both = _sizes_of_list(lambda b: subgraph2_sizes(b, h, with_largest=True), batch_or_list, chunk, lambda: 3)
        return both if with_largest else both[0]
    c = _count(batch_or_list, h)
    _raise_status(c, "subgraph2_sizes", MAX_NODES)
    at = c["ptrs"][:, c["node_ptr"]].t().cpu()
    sizes = at[1:] - at[:-1]
    if not with_largest:
        return sizes
    per_root = (c["sub_node_ptr"][1:] - c["sub_node_ptr"][:-1]) // (c["sub2_ptr"][1:] - c["sub2_ptr"][:-1]).clamp(min=1)
    return sizes, (int(per_root.max()) if per_root.numel() else 0)


def expand_subgraphs2(batch, h, use_rd=False, sizes=None, node_label="spd", max_nodes_per_hop=None, subgraph_pretransform=None,
                      self_loop=False, check=None, max_nodes=None):
    """Every subgraph2 of a collated batch as one disconnected graph, on the batch's device.
    sizes: the batch's rows of a `subgraph2_sizes` result (known on the host from the store's build) — the output sizes are
    their sums and nothing is read back; without it the three totals are copied once.  check / max_nodes: as
    subgraphs.expand_subgraphs (with `sizes` the status tensor is returned as `status` and a bad graph has no, or not all, rows;
    I2GraphStore has checked both limits at build)."""
    h = check_args(h, node_label, max_nodes_per_hop, subgraph_pretransform, self_loop)
    sizes, G_known, max_nodes = _known_sizes(sizes, 3, max_nodes, MAX_NODES)
    c = _count(batch, h, G_known, max_nodes)
    N = c["N"]
    Ns, Es, S2 = _column_totals("expand_subgraphs2", c, sizes, G_known, lambda: c["ptrs"][:, N].tolist())
    _below_2_31("expand_subgraphs2", "%d sub-nodes / %d sub-edges", Ns, Es)
    dev = batch.edge_index.device
    nodes = torch.empty((3, Ns), dtype=torch.int64, device=dev)       # orig_node | node_to_subgraph2 | graph
    z = torch.empty((Ns, 4), dtype=torch.int64, device=dev)
    edges = torch.empty((3, Es), dtype=torch.int64, device=dev)       # sub_src | sub_dst | orig_edge
    s2 = torch.empty(4 * S2 + 1, dtype=torch.int64, device=dev)       # subgraph2_to_subgraph | center_idx [S2, 2] | s2_node_ptr
    s2_to_sub, center_idx, s2_node_ptr = s2[:S2], s2[S2:3 * S2].view(S2, 2), s2[3 * S2:]
    rd = torch.empty((Ns, 2), dtype=torch.float32, device=dev) if use_rd else None
    if Ns == 0:
        s2_node_ptr.zero_()
    nv.call("esc_subgraph2_fill", nv.ptr(c["node_ptr"]), nv.ptr(c["edge_ptr"]), nv.ptr(c["src"]), nv.ptr(c["dst"]), c["G"], N,
            c["E"], c["nmax"], h, nv.ptr(c["sub_node_ptr"]), nv.ptr(c["sub_edge_ptr"]), nv.ptr(c["sub2_ptr"]), Ns, Es, S2,
            int(bool(use_rd)), nv.ptr(nodes[0]), nv.ptr(z), nv.ptr(nodes[1]), nv.ptr(nodes[2]), nv.ptr(edges[0]),
            nv.ptr(edges[1]), nv.ptr(edges[2]), nv.ptr(s2_to_sub), nv.ptr(center_idx), nv.ptr(s2_node_ptr), nv.ptr(rd),
            nv.ptr(c["status"]), nv.stream())
    if _wants_check(check, sizes):
        _raise_status(c, "expand_subgraphs2", MAX_NODES)
    out = Data()
    orig_node, orig_edge = nodes[0], edges[2]
    out.z = z
    out.z._esc_known_range = (([0, 0, 0, 0], [h + 1, h + 1, 2 * h + 5, 2 * h + 5]), out.z._version)
    if batch.x is not None:
        out.x = batch.x[orig_node]
    out.edge_index = edges[:2]
    if batch.edge_attr is not None:
        out.edge_attr = batch.edge_attr[orig_edge]
    out.node_to_subgraph2, out.subgraph2_to_subgraph, out.subgraph_to_graph = nodes[1], s2_to_sub, batch.batch
    out.node_to_original_node, out.batch, out.center_idx = orig_node, nodes[2], center_idx
    out.num_subgraphs, out.num_subgraphs2, out.num_original_nodes, out.num_nodes = N, S2, N, Ns
    if use_rd:
        out.rd = rd
    if batch.y is not None:
        out.y = batch.y
    out.orig_node, out.orig_edge = orig_node, orig_edge
    out.s2_node_ptr, out.sub2_ptr, out.status = s2_node_ptr, c["sub2_ptr"], c["status"]
    out.sub_node_ptr, out.sub_edge_ptr = c["sub_node_ptr"], c["sub_edge_ptr"]
    # mean / add pooling over the subgraph2s and over the subgraphs: no rebuild, no read-back
    _tag_segments(out.node_to_subgraph2, s2_node_ptr, S2)
    _tag_segments(out.subgraph2_to_subgraph, c["sub2_ptr"], N)
    return out


class I2GraphStore(GraphStore):
    """The I2GNN run's split (expansion.GraphStore): the per-graph (sub-nodes, sub-edges, subgraph2s) from the count pass at
    build time, and both limits checked there, so that no training step reads a size or a status: the rd limit of 96 nodes per
    rooted subgraph from the count pass, the label limit by the range of h alone (the largest label is 2h + 5 on every graph,
    DESIGN.md 6i)."""
    kind = "subgraph2"
    _check_param = staticmethod(check_args)
    h = property(lambda self: self.param)

    def __init__(self, data_list, h, use_rd=False, device=None):
        GraphStore.__init__(self, data_list, h, device)
        self.use_rd = bool(use_rd)
        _refuse_rd(self, self.use_rd)

    def _count_sizes(self):
        return subgraph2_sizes(self.graphs, self.h, with_largest=True)

    def expand(self, batch, use_rd=None):
        use_rd = self.use_rd if use_rd is None else bool(use_rd)
        _refuse_rd(self, use_rd)
        return expand_subgraphs2(batch, self.h, use_rd, self.sizes_of(batch))
