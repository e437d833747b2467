"""Shortest-path distances for the graph transformer's attention bias: the MI355X twin of what the reference's
create_subgraphs computes per graph with networkx and stores as the key attn_bias
(GraphGPS/graphgps/loader/utils_escgnn.py:29-38) - all-pairs distances on the undirected graph, 100 where there is no path -
computed on the device by esc_graph_spd (csrc/spd.hip), one workgroup per graph, one breadth-first search per thread over an
adjacency of bit rows.

add_spd(data_or_batch) sets the reference's key on one graph or on a collated batch: the concatenation of the graphs' flattened
n x n matrices, here as uint8 (the reference keeps int64; its collate never pads the key, loader/batch.py:132-141, so its
BiasedTransformer receives None - here the ragged layout is the one the attention kernels read, pair_ptr's, and nothing is
padded).  SPDTable(store) computes it for a whole split in ONE launch at build time, keeps it in HBM and hands every batch its
bytes with one gather launch.  The consumer is GPSLayer(global_model_type='BiasedTransformer').  The twin of rwse.py."""
import torch

from . import ops
from .ragged import StoreTable, graph_ranges


def add_spd(data):
    """Sets attn_bias (uint8 [sum n^2]) on a graph or a collated batch whose tensors are on the device, and returns the data.
    Torch plumbing for the ranges plus one launch; the batch's pair count is read back, and so is the largest graph unless the
    batch carries `_esc_max_nodes`.  A batch from DeviceGraphStore.collate keeps its own graph_ptr: the pair offsets cached on it
    are the ones the attention layers use."""
    graph_ptr, edge_ptr, G, widest, N = graph_ranges(data)
    own = getattr(getattr(data, "_esc_plan", None), "graph_ptr", None)
    if own is not None and own.numel() == graph_ptr.numel():
        graph_ptr = own
    data.attn_bias = ops.graph_spd(data.edge_index, graph_ptr, edge_ptr, max_nodes=widest, num_nodes=N)
    return data


class SPDTable(StoreTable):
    """The distances of every graph of a DeviceGraphStore, resident in HBM: spd uint8 [sum n^2] with pair_ptr_all, the int64 scan
    of n^2 taken from the store's host offsets.  Built with one esc_graph_spd launch over the store's flat (graph-local) edge
    arrays; attach() is one esc_spd_gather launch and sets batch.attn_bias, the batch's pair count summed on the host."""

    def __init__(self, store):
        super().__init__(store)
        n = (store.h_node_ptr[1:] - store.h_node_ptr[:-1]).to(torch.int64)                  # host data
        self.h_pairs = n * n
        h_pair_ptr = torch.zeros(n.numel() + 1, dtype=torch.int64)
        torch.cumsum(self.h_pairs, 0, out=h_pair_ptr[1:])
        self.pair_ptr = h_pair_ptr.to(store.node_ptr.device)
        self.spd = self._build(lambda edge_index, node_ptr, edge_ptr, pairs, **kw: ops.graph_spd(
            edge_index, node_ptr, edge_ptr, num_pairs=pairs, pair_ptr=self.pair_ptr, **kw), int(h_pair_ptr[-1]))

    def _gather(self, batch, graph_ids, graph_ptr, N):
        ids = torch.as_tensor(graph_ids, dtype=torch.int64).reshape(-1)
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= self.h_pairs.numel()):
            raise IndexError("spd_gather: graph id out of range (the table holds %d graphs)" % self.h_pairs.numel())
        batch.attn_bias = ops.spd_gather(self.spd, self.pair_ptr, self.store.node_ptr, ids, graph_ptr, num_pairs=int(self.h_pairs[ids].sum()))
