"""Laplacian positional encodings for the graph transformer: the MI355X twin of the reference's compute_posenc_stats for
pe_types ['LapPE'] (GraphGPS/graphgps/transform/posenc_stats.py) under zinc-GPS.yaml's posenc_LapPE block - laplacian_norm none,
eigvec_norm L2 - computed on the device by esc_laplacian_eig (csrc/lappe.hip), one workgroup per graph.

add_lap_pe(data_or_batch) sets the reference's two keys on one graph or on a collated batch; LapPETable(store) computes them for
a whole split in ONE launch at build time, keeps them in HBM and hands every batch its rows with one gather launch: what the
reference's dataset pre-transform plus collate do.  The encoder that consumes the keys is nn.LapPENodeEncoder.

The eigenvectors' signs, and the basis inside an eigenspace of equal eigenvalues, are whatever the deterministic solver yields
(numpy.linalg.eigh's are just as arbitrary); the encoder's random sign flips in training exist because of the former."""
from . import ops
from .ragged import StoreTable, graph_ranges


def add_lap_pe(data, max_freqs=8):
    """Sets EigVals [N, K, 1] and EigVecs [N, K] (fp32, NaN in the columns j >= n of a graph with n < K nodes) on a graph or a
    collated batch whose tensors are on the device, and returns it.  Torch plumbing for the ranges plus one launch; the largest
    graph is read back once unless the batch carries `_esc_max_nodes`."""
    graph_ptr, edge_ptr, G, widest, N = graph_ranges(data)
    data.EigVals, data.EigVecs = ops.laplacian_eig(data.edge_index, graph_ptr, edge_ptr, max_freqs, max_nodes=widest, num_nodes=N)
    return data


class LapPETable(StoreTable):
    """The LapPE of every graph of a DeviceGraphStore, resident in HBM: eigvecs / eigvals [N_all, K].  Built with one
    esc_laplacian_eig launch over the store's flat (graph-local) edge arrays; attach() is one esc_lappe_gather launch."""

    def __init__(self, store, max_freqs=8):
        super().__init__(store)
        self.max_freqs = int(max_freqs)
        vals, self.eigvecs = self._build(ops.laplacian_eig, self.max_freqs)
        self.eigvals = vals.view(-1, self.max_freqs)

    def _gather(self, batch, graph_ids, graph_ptr, N):
        batch.EigVals, batch.EigVecs = ops.lappe_gather(self.eigvecs, self.eigvals, self.store.node_ptr, graph_ids, graph_ptr, N)
