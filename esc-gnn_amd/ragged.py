"""The host side of a ragged set of small graphs, for the kernels that run one workgroup per graph and write per-node
statistics (the device side: csrc/ragged_graphs.h).

Two callers.  The label wrappers (cycles.py, graphlets.py) come with one edge list per graph on the host: pack_edge_lists
turns them into the offsets and flat ends the kernels take, edge_list_labels uploads, launches a named entry point and reads
the per-graph status back.  The encoding tables (lappe.py, rwse.py) come with graphs already on the device: graph_ranges
finds the ranges of a graph or a collated batch, StoreTable is what a resident table of a DeviceGraphStore needs besides
its own kernel.  (ops._ragged_graphs resolves such a set for a launch.)"""
import torch

from . import _native as nv

ESC_ERANGE = nv.ESC_ERANGE
MAX_NODES = 64                    # the label kernels keep a graph's adjacency as 64-bit masks


# ---- edge lists on the host -> per-graph labels ------------------------------------------------------------------------
def pack_edge_lists(node_counts, edge_lists):
    """Host only.  node_counts: list[int]; edge_lists: one int tensor [2, m_g] (or flat, 2 m_g entries) of graph-local ids per
    graph.  Returns (node_ptr [G+1], edge_ptr [G+1], ends [2, E]), int64."""
    lists = [e.reshape(2, -1).to(torch.int64) for e in edge_lists]
    node_ptr = torch.zeros(len(node_counts) + 1, dtype=torch.int64)
    edge_ptr = torch.zeros(len(node_counts) + 1, dtype=torch.int64)
    node_ptr[1:] = torch.cumsum(torch.tensor([int(n) for n in node_counts], dtype=torch.int64), 0)
    edge_ptr[1:] = torch.cumsum(torch.tensor([e.size(1) for e in lists], dtype=torch.int64), 0)
    ends = torch.cat(lists, dim=1) if lists else torch.zeros((2, 0), dtype=torch.int64)
    return node_ptr, edge_ptr, ends


def raise_for_status(who, what, status, node_ptr):
    """Host only.  The kernels' per-graph verdicts as the wrappers' ValueError, for the first graph that has one."""
    bad = torch.nonzero(status)
    if bad.numel():
        g = int(bad[0])
        n = int(node_ptr[g + 1] - node_ptr[g])
        if int(status[g]) == ESC_ERANGE:
            raise ValueError("%s: graph %d has %d nodes; the %s-count kernel takes graphs of at most %d nodes" % (who, g, n, what, MAX_NODES))
        raise ValueError("%s: graph %d has a node id outside [0, %d)" % (who, g, n))


def split_rows(rows, node_ptr):
    """Host only.  [N, C] -> one [n_g, C] view per graph."""
    return [rows[int(node_ptr[g]):int(node_ptr[g + 1])] for g in range(node_ptr.numel() - 1)]


def _device(who):
    if not torch.cuda.is_available():
        raise RuntimeError("esc_gnn_amd.%s needs a HIP device (MI355X); there is no CPU fallback" % who)
    return torch.device("cuda", torch.cuda.current_device())


def edge_list_labels(who, what, entry, dtype, width, node_counts, edge_lists, ld_out=None):
    """One launch of the label kernel `entry` over the graphs of pack_edge_lists' arguments: one CPU tensor [n_g, width] of
    `dtype` per graph.  ld_out: the entry point takes the output's leading dimension behind it."""
    dev = _device(who)
    G = len(node_counts)
    if G == 0:
        return []
    node_ptr, edge_ptr, ends = pack_edge_lists(node_counts, edge_lists)
    Nn, Ein = int(node_ptr[-1]), int(edge_ptr[-1])
    src = ends[0].contiguous().to(dev) if Ein else None
    dst = ends[1].contiguous().to(dev) if Ein else None
    out = torch.zeros(Nn, width, dtype=dtype, device=dev)
    status = torch.zeros(G, dtype=torch.int32, device=dev)
    node_ptr_d, edge_ptr_d = node_ptr.to(dev), edge_ptr.to(dev)
    nv.call(entry, nv.ptr(node_ptr_d), nv.ptr(edge_ptr_d), nv.ptr(src), nv.ptr(dst), G, Nn, Ein, nv.ptr(out) if Nn else None,
            *(() if ld_out is None else (ld_out,)), nv.ptr(status), nv.stream())
    raise_for_status(who, what, status.cpu(), node_ptr)
    return split_rows(out.cpu(), node_ptr)


def _num_nodes(data):
    n = data.num_nodes
    return int(n.item()) if torch.is_tensor(n) else int(n)


def data_list_labels(edge_lists_fn, data_list, chunk):
    """edge_lists_fn over a list of Data (edge_index with graph-local ids), one launch per chunk"""
    out = []
    for i in range(0, len(data_list), chunk):
        part = data_list[i:i + chunk]
        out.extend(edge_lists_fn([_num_nodes(d) for d in part], [d.edge_index.cpu() for d in part]))
    return out


# ---- graphs on the device -> encoding tables ---------------------------------------------------------------------------
def graph_ranges(data):
    """(graph_ptr, edge_ptr, G, largest graph or None, N) of a graph or a collated batch on the device"""
    ei = data.edge_index
    N = int(data.num_nodes)
    batch = data["batch"]
    if batch is None:                                              # one graph
        ptr = torch.tensor([[0, N], [0, ei.size(1)]], dtype=torch.int64).to(ei.device)
        return ptr[0], ptr[1], 1, N, N
    G = int(data.num_graphs)
    bounds = torch.arange(G + 1, device=ei.device)
    graph_ptr = torch.searchsorted(batch, bounds)                  # `batch` is non-decreasing
    edge_ptr = torch.searchsorted(batch[ei[0]].contiguous(), bounds)   # ... and so is the graph of every edge: edges are contiguous per graph
    return graph_ptr, edge_ptr, G, getattr(data, "_esc_max_nodes", None), N


class StoreTable(object):
    """A per-node encoding of every graph of a DeviceGraphStore, resident in HBM.  A subclass computes its tables with
    self._build(...) in its constructor and sets its batch keys in _gather(batch, graph_ids, graph_ptr, N)."""

    def __init__(self, store):
        self.store = store
        self.max_nodes = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())           # host data
        self.max_edges = int((store.h_edge_ptr[1:] - store.h_edge_ptr[:-1]).max())

    def _build(self, op, what, **limits):
        """one launch of ops.<op> over the store's flat (graph-local) edge arrays, the sizes taken from its host offsets"""
        store = self.store
        return op(torch.stack([store.esrc_all, store.edst_all]), store.node_ptr, store.edge_ptr, what, max_nodes=self.max_nodes,
                  edges_local=True, num_nodes=int(store.h_node_ptr[-1]), **limits)

    def attach(self, batch, graph_ids):
        """Sets the table's keys on a batch that store.collate(graph_ids) made; graph_ids on the host (checked there: an id out
        of range raises IndexError).  One launch, no device-to-host copy."""
        plan = getattr(batch, "_esc_plan", None)
        graph_ptr = getattr(plan, "graph_ptr", None)
        if graph_ptr is None:
            raise ValueError("%s.attach: the batch does not come from DeviceGraphStore.collate" % type(self).__name__)
        self._gather(batch, graph_ids, graph_ptr, batch.x.size(0))
        return batch
