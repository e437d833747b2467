"""Node-rooted h-hop subgraph expansion of a collated batch on the device (csrc/subgraphs.hip) — what feeds the NGNN
baseline.  The reference materialises every rooted subgraph once per dataset on the host (utils.py:18-132, a python loop
with one scipy pinv per root) and collates them per batch (batch_I2.py:61-66); here a plain batch is expanded per step.

Canonical order: the sub-nodes of a root are the root, then ascending (hop, node id); the sub-edges keep the
order of the batch's edges.  Field names are the reference's.
"""
import torch

from . import _native as nv
from .data import Data
from .expansion import (GraphStore, _below_2_31, _column_totals, _count_prologue, _known_sizes, _raise_status as _raise_for,
                        _sizes_of_list, _tag_segments, _wants_check, collate_graphs)
from .utils_edge_efficient import _check_args

H_MAX = 98                   # z = hop + 1 indexes the model's 100-row tables
MAX_NODES = 4096
RD_MAX_NODES = 96            # largest subgraph whose two m x m fp64 matrices fit the LDS of one wave's workgroup
NODE_LABELS = ("spd", "drnl")


def _count(batch, h, G_known=None, max_nodes=None):
    h = _check_h(h)
    c = _count_prologue(batch, MAX_NODES, "subgraphs", G_known, max_nodes)
    dev = batch.edge_index.device
    sub_node_ptr = torch.empty(c["N"] + 1, dtype=torch.int64, device=dev)
    sub_edge_ptr = torch.empty(c["N"] + 1, dtype=torch.int64, device=dev)
    nv.call("esc_subgraph_count", nv.ptr(c["node_ptr"]), nv.ptr(c["edge_ptr"]), nv.ptr(c["src"]), nv.ptr(c["dst"]), c["G"], c["N"],
            c["E"], c["nmax"], h, nv.ptr(sub_node_ptr), nv.ptr(sub_edge_ptr), nv.ptr(c["status"]), nv.stream())
    c.update(sub_node_ptr=sub_node_ptr, sub_edge_ptr=sub_edge_ptr, h=h)
    return c


def _check_h(h):
    h = _check_args(h, None, None)
    if h < 1 or h > H_MAX:
        raise ValueError("subgraphs: h=%d outside 1..%d (the model's z tables have 100 rows and z = hop + 1)" % (h, H_MAX))
    return h


def _raise_status(c, what, node_limit=MAX_NODES):
    """as expansion._raise_status, with what a rooted-subgraph expansion can have hit (subgraphs2 shares the texts)"""
    _raise_for(c, what,
               "a node id outside the graph, edges of one graph not contiguous, or a graph of more than %d nodes (limit %d)"
               % (c["nmax"], node_limit),
               "with use_rd, a subgraph of more than %d nodes (both m x m matrices of the pseudo-inverse must fit LDS), or "
               "output totals that are not those of the count pass" % RD_MAX_NODES, c["sub_node_ptr"])


def subgraph_sizes(batch_or_list, h, chunk=4096, with_largest=False):
    """The count pass alone: int64 [G, 2] on the host, per graph (sub-nodes, sub-edges) of its rooted subgraphs.
    with_largest: also the node count of the largest single subgraph (what the rd limit of 96 is about)."""
    if isinstance(batch_or_list, (list, tuple)):
        both = _sizes_of_list(lambda b: subgraph_sizes(b, h, with_largest=True), batch_or_list, chunk, lambda: 2)
        return both if with_largest else both[0]
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
    sizes, G_known, max_nodes = _known_sizes(sizes, 2, max_nodes, MAX_NODES)
    c = _count(batch, h, G_known, max_nodes)
    Ns, Es = _column_totals("expand_subgraphs", c, sizes, G_known,
                            lambda: torch.stack([c["sub_node_ptr"][c["N"]], c["sub_edge_ptr"][c["N"]]]).tolist())
    _below_2_31("expand_subgraphs", "%d sub-nodes / %d sub-edges", Ns, Es)
    dev = batch.edge_index.device
    nodes = torch.empty((5, Ns), dtype=torch.int64, device=dev)       # orig_node | hop + 1 | paths | node_to_subgraph | graph
    edges = torch.empty((3, Es), dtype=torch.int64, device=dev)       # sub_src | sub_dst | orig_edge
    rd = torch.empty((Ns, 1), dtype=torch.float32, device=dev) if use_rd else None
    nv.call("esc_subgraph_fill", nv.ptr(c["node_ptr"]), nv.ptr(c["edge_ptr"]), nv.ptr(c["src"]), nv.ptr(c["dst"]), c["G"], c["N"],
            c["E"], c["nmax"], h, nv.ptr(c["sub_node_ptr"]), nv.ptr(c["sub_edge_ptr"]), Ns, Es, int(bool(use_rd)),
            nv.ptr(nodes[0]), nv.ptr(nodes[1]), nv.ptr(nodes[2]), nv.ptr(nodes[3]), nv.ptr(nodes[4]), nv.ptr(edges[0]),
            nv.ptr(edges[1]), nv.ptr(edges[2]), nv.ptr(rd), nv.ptr(c["status"]), nv.stream())
    if _wants_check(check, sizes):
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
    _tag_segments(out.node_to_subgraph, c["sub_node_ptr"], c["N"])    # mean pooling over the subgraphs
    return out


def _refuse_rd(store, use_rd):
    if use_rd and store.largest_subgraph > RD_MAX_NODES:
        raise ValueError("%s: use_rd with a subgraph of %d nodes at h=%d: rd covers subgraphs of at most %d nodes"
                         % (type(store).__name__, store.largest_subgraph, store.h, RD_MAX_NODES))


class PlainGraphStore(GraphStore):
    """The NGNN run's split (expansion.GraphStore).  The count pass also gives the largest single subgraph: `expand(use_rd=True)`
    refuses a split that the rd limit of 96 nodes does not cover, on the host, instead of training on unwritten rd rows."""
    kind = "subgraph"
    h = property(lambda self: self.param)

    def _count_sizes(self):
        return subgraph_sizes(self.graphs, self.h, with_largest=True)

    def expand(self, batch, node_label="spd", use_rd=False):
        _refuse_rd(self, use_rd)
        return expand_subgraphs(batch, self.h, node_label, use_rd, self.sizes_of(batch))
