"""Random-walk structural encodings for the graph transformer: the MI355X twin of the reference's compute_posenc_stats for
pe_types ['RWSE'] (GraphGPS/graphgps/transform/posenc_stats.py:97-104,185-231) - the landing probabilities (P^k)[i, i] of the
k-step random walk, P = D^-1 A over the edge list as it stands - computed on the device by esc_rw_landing (csrc/rwse.hip), one
workgroup per graph, K sparse matrix-vector steps per start node instead of the reference's dense n x n matrix powers.

add_rwse(data_or_batch, ksteps) sets the reference's key on one graph or on a collated batch; RWSETable(store, ksteps) computes
it for a whole split in ONE launch at build time, keeps it in HBM and hands every batch its rows with one gather launch: what the
reference's dataset pre-transform plus collate do.  The encoder that consumes the key is nn.RWSENodeEncoder.  The twin of
lappe.py."""
from . import ops
from .ragged import StoreTable, graph_ranges


def add_rwse(data, ksteps):
    """Sets pestat_RWSE [N, K] (fp32) on a graph or a collated batch whose tensors are on the device, and returns it.  Torch
    plumbing for the ranges plus one launch; the largest node and edge count of a graph are read back (the node count is not
    when the batch carries `_esc_max_nodes`)."""
    graph_ptr, edge_ptr, G, widest, N = graph_ranges(data)
    data.pestat_RWSE = ops.rw_landing(data.edge_index, graph_ptr, edge_ptr, ksteps, max_nodes=widest, num_nodes=N)
    return data


class RWSETable(StoreTable):
    """The RWSE of every graph of a DeviceGraphStore, resident in HBM: pestat [N_all, K].  Built with one esc_rw_landing launch
    over the store's flat (graph-local) edge arrays, the largest graph taken from the store's host offsets; attach() is one
    esc_rwse_gather launch."""

    def __init__(self, store, ksteps):
        super().__init__(store)
        self.ksteps = [int(k) for k in ksteps]
        self.pestat = self._build(ops.rw_landing, self.ksteps, max_edges=self.max_edges)

    def _gather(self, batch, graph_ids, graph_ptr, N):
        batch.pestat_RWSE = ops.rwse_gather(self.pestat, self.store.node_ptr, graph_ids, graph_ptr, N)
