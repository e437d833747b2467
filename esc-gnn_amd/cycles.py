"""Per-node cycle-counting labels of the ZINC cycle task, computed on the device (csrc/cycles.hip, esc_cycle_counts).

Restates the reference's dataset_zinc_cycle.py:45-61 (pkl2data): self loops dropped, edges symmetrised, and for every
node the number of undirected simple cycles of length 3, 4, 5 and 6 through it (networkx simple_cycles, length 3..6,
+1 per node and cycle, halved).  Graphs of up to 64 nodes (ZINC molecules have at most 38 atoms).
"""
import torch

from . import _native as nv

ESC_ERANGE = nv.ESC_ERANGE
MAX_NODES = 64


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("esc_gnn_amd.cycle_counts needs a HIP device (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def cycle_counts_edge_lists(node_counts, edge_lists):
    """node_counts: list[int]; edge_lists: int64 [2, m_g] tensors with graph-local ids.  Returns one float32 [n_g, 4]
    CPU tensor per graph (columns: 3-, 4-, 5-, 6-cycles through the node)."""
    dev = _device()
    G = len(node_counts)
    if G == 0:
        return []
    n_t = torch.tensor([int(n) for n in node_counts], dtype=torch.int64)
    m_t = torch.tensor([int(e.reshape(2, -1).size(1)) for e in edge_lists], dtype=torch.int64)
    node_ptr = torch.zeros(G + 1, dtype=torch.int64)
    edge_ptr = torch.zeros(G + 1, dtype=torch.int64)
    node_ptr[1:] = torch.cumsum(n_t, 0)
    edge_ptr[1:] = torch.cumsum(m_t, 0)
    Nn, Ein = int(node_ptr[-1]), int(edge_ptr[-1])
    cat = torch.cat([e.reshape(2, -1).to(torch.int64) for e in edge_lists], dim=1) if Ein else None
    src = cat[0].contiguous().to(dev) if Ein else None
    dst = cat[1].contiguous().to(dev) if Ein else None
    out = torch.zeros(Nn, 4, dtype=torch.float32, device=dev)
    status = torch.zeros(G, dtype=torch.int32, device=dev)
    node_ptr_d, edge_ptr_d = node_ptr.to(dev), edge_ptr.to(dev)
    nv.call("esc_cycle_counts", nv.ptr(node_ptr_d), nv.ptr(edge_ptr_d), nv.ptr(src), nv.ptr(dst), G, Nn, Ein,
            nv.ptr(out) if Nn else None, nv.ptr(status), nv.stream())
    st = status.cpu()
    if bool((st != 0).any()):
        g = int(torch.nonzero(st)[0])
        if int(st[g]) == ESC_ERANGE:
            raise ValueError("cycle_counts: graph %d has %d nodes; the cycle-count kernel takes graphs of at most %d nodes"
                             % (g, int(n_t[g]), MAX_NODES))
        raise ValueError("cycle_counts: graph %d has a node id outside [0, %d)" % (g, int(n_t[g])))
    out = out.cpu()
    return [out[int(node_ptr[g]):int(node_ptr[g + 1])] for g in range(G)]


def _num_nodes(data):
    n = data.num_nodes
    return int(n.item()) if torch.is_tensor(n) else int(n)


def cycle_counts(data_list, chunk=65536):
    """per-graph float32 [n, 4] cycle labels of a list of Data (edge_index with graph-local ids), one launch per chunk"""
    out = []
    for i in range(0, len(data_list), chunk):
        part = data_list[i:i + chunk]
        out.extend(cycle_counts_edge_lists([_num_nodes(d) for d in part], [d.edge_index.cpu() for d in part]))
    return out
