"""Laplacian positional encodings for the graph transformer: the MI355X twin of the reference's compute_posenc_stats for
pe_types ['LapPE'] (GraphGPS/graphgps/transform/posenc_stats.py) under zinc-GPS.yaml's posenc_LapPE block - laplacian_norm none,
eigvec_norm L2 - computed on the device by esc_laplacian_eig (csrc/lappe.hip), one workgroup per graph.

add_lap_pe(data_or_batch) sets the reference's two keys on one graph or on a collated batch; LapPETable(store) computes them for
a whole split in ONE launch at build time, keeps them in HBM and hands every batch its rows with one gather launch: what the
reference's dataset pre-transform plus collate do.  The encoder that consumes the keys is nn.LapPENodeEncoder.

The eigenvectors' signs, and the basis inside an eigenspace of equal eigenvalues, are whatever the deterministic solver yields
(numpy.linalg.eigh's are just as arbitrary); the encoder's random sign flips in training exist because of the former."""
import torch

from . import ops


def _ranges(data):
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


def add_lap_pe(data, max_freqs=8):
    """Sets EigVals [N, K, 1] and EigVecs [N, K] (fp32, NaN in the columns j >= n of a graph with n < K nodes) on a graph or a
    collated batch whose tensors are on the device, and returns it.  Torch plumbing for the ranges plus one launch; the largest
    graph is read back once unless the batch carries `_esc_max_nodes`."""
    graph_ptr, edge_ptr, G, widest, N = _ranges(data)
    data.EigVals, data.EigVecs = ops.laplacian_eig(data.edge_index, graph_ptr, edge_ptr, max_freqs, max_nodes=widest, num_nodes=N)
    return data


class LapPETable(object):
    """The LapPE of every graph of a DeviceGraphStore, resident in HBM: eigvecs / eigvals [N_all, K].  Built with one
    esc_laplacian_eig launch over the store's flat (graph-local) edge arrays; attach() is one esc_lappe_gather launch."""

    def __init__(self, store, max_freqs=8):
        self.store, self.max_freqs = store, int(max_freqs)
        n = store.h_node_ptr[1:] - store.h_node_ptr[:-1]           # host data
        self.max_nodes = int(n.max())
        N = int(store.h_node_ptr[-1])
        edge_index = torch.stack([store.esrc_all, store.edst_all])
        vals, self.eigvecs = ops.laplacian_eig(edge_index, store.node_ptr, store.edge_ptr, self.max_freqs, max_nodes=self.max_nodes,
                                               edges_local=True, num_nodes=N)
        self.eigvals = vals.view(N, self.max_freqs)

    def attach(self, batch, graph_ids):
        """Sets EigVals / EigVecs of a batch that store.collate(graph_ids) made; graph_ids on the host (checked there: an id out
        of range raises IndexError).  One launch, no device-to-host copy."""
        plan = getattr(batch, "_esc_plan", None)
        graph_ptr = getattr(plan, "graph_ptr", None)
        if graph_ptr is None:
            raise ValueError("LapPETable.attach: the batch does not come from DeviceGraphStore.collate")
        batch.EigVals, batch.EigVecs = ops.lappe_gather(self.eigvecs, self.eigvals, self.store.node_ptr, graph_ids, graph_ptr,
                                                        batch.x.size(0))
        return batch
