"""Per-node graphlet-counting labels of the counting benchmark (count_graphlet targets 0..4), computed on the device
(csrc/graphlets.hip, esc_graphlet_counts).

The definition is the project's own: self loops dropped, edges symmetrised, duplicates collapsed; a copy of
a pattern is a subgraph isomorphic to it (not necessarily induced), counted once.  For every node the kernel gives, for
each orbit of each pattern, the number of copies in which the node sits at that orbit (11 columns, GRAPHLET_ORBITS); the
task label of target t is the sum of that pattern's orbit columns: the copies through the node, the convention of the
cycle labels.  Graphs of up to 64 nodes.
"""
import torch

from . import _native as nv

ESC_ERANGE = nv.ESC_ERANGE
MAX_NODES = 64
NUM_ORBITS = 11
GRAPHLET_NAMES = ("tailed_triangle", "chordal_cycle", "4_clique", "4_path", "triangle_rectangle")
GRAPHLET_ORBITS = ((0, 1, 2), (3, 4), (5,), (6, 7), (8, 9, 10))
FLOAT_EXACT = 1 << 24             # fp32 holds every integer up to here


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("esc_gnn_amd.graphlet_counts needs a HIP device (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def graphlet_orbit_counts_edge_lists(node_counts, edge_lists):
    """node_counts: list[int]; edge_lists: int64 [2, m_g] tensors with graph-local ids.  Returns one int32 [n_g, 11] CPU
    tensor per graph (columns: module docstring / GRAPHLET_ORBITS)."""
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
    out = torch.zeros(Nn, NUM_ORBITS, dtype=torch.int32, device=dev)
    status = torch.zeros(G, dtype=torch.int32, device=dev)
    node_ptr_d, edge_ptr_d = node_ptr.to(dev), edge_ptr.to(dev)
    nv.call("esc_graphlet_counts", nv.ptr(node_ptr_d), nv.ptr(edge_ptr_d), nv.ptr(src), nv.ptr(dst), G, Nn, Ein,
            nv.ptr(out) if Nn else None, NUM_ORBITS, nv.ptr(status), nv.stream())
    st = status.cpu()
    if bool((st != 0).any()):
        g = int(torch.nonzero(st)[0])
        if int(st[g]) == ESC_ERANGE:
            raise ValueError("graphlet_counts: graph %d has %d nodes; the graphlet-count kernel takes graphs of at most "
                             "%d nodes" % (g, int(n_t[g]), MAX_NODES))
        raise ValueError("graphlet_counts: graph %d has a node id outside [0, %d)" % (g, int(n_t[g])))
    out = out.cpu()
    return [out[int(node_ptr[g]):int(node_ptr[g + 1])] for g in range(G)]


def _num_nodes(data):
    n = data.num_nodes
    return int(n.item()) if torch.is_tensor(n) else int(n)


def graphlet_orbit_counts(data_list, chunk=65536):
    """per-graph int32 [n, 11] orbit counts of a list of Data (edge_index with graph-local ids), one launch per chunk"""
    out = []
    for i in range(0, len(data_list), chunk):
        part = data_list[i:i + chunk]
        out.extend(graphlet_orbit_counts_edge_lists([_num_nodes(d) for d in part], [d.edge_index.cpu() for d in part]))
    return out


def _exact_float(t, what):
    if t.numel() and int(t.max()) > FLOAT_EXACT:
        raise ValueError("%s: a count of %d exceeds 2^24, where float32 stops being exact; use graphlet_orbit_counts "
                         "(int32)" % (what, int(t.max())))
    return t.to(torch.float32)


def orbit_sums(orbits):
    """int64 [n, 5] from int32 [n, 11]: the copies of each pattern through the node, at any position"""
    o = orbits.to(torch.int64)
    return torch.stack([o[:, list(cols)].sum(dim=1) for cols in GRAPHLET_ORBITS], dim=1)


def graphlet_counts(data_list, chunk=65536):
    """per-graph float32 [n, 5] graphlet labels (the orbit sums); ValueError if a count is not exact in float32"""
    return [_exact_float(orbit_sums(o), "graphlet_counts") for o in graphlet_orbit_counts(data_list, chunk)]


def graphlet_orbit_counts_float(data_list, chunk=65536):
    """per-graph float32 [n, 11] orbit counts; ValueError if a count is not exact in float32"""
    return [_exact_float(o, "graphlet_orbit_counts_float") for o in graphlet_orbit_counts(data_list, chunk)]
