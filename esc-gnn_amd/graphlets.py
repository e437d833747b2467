"""Per-node graphlet-counting labels of the counting benchmark (count_graphlet targets 0..4), computed on the device
(csrc/graphlets.hip, esc_graphlet_counts).

The definition is the project's own: self loops dropped, edges symmetrised, duplicates collapsed; a copy of
a pattern is a subgraph isomorphic to it (not necessarily induced), counted once.  For every node the kernel gives, for
each orbit of each pattern, the number of copies in which the node sits at that orbit (11 columns, GRAPHLET_ORBITS); the
task label of target t is the sum of that pattern's orbit columns: the copies through the node, the convention of the
cycle labels.  Graphs of up to 64 nodes.
"""
import torch

from .ragged import ESC_ERANGE, MAX_NODES, data_list_labels, edge_list_labels  # noqa: F401  (the constants: part of the module's face)

NUM_ORBITS = 11
GRAPHLET_NAMES = ("tailed_triangle", "chordal_cycle", "4_clique", "4_path", "triangle_rectangle")
GRAPHLET_ORBITS = ((0, 1, 2), (3, 4), (5,), (6, 7), (8, 9, 10))
FLOAT_EXACT = 1 << 24             # fp32 holds every integer up to here


def graphlet_orbit_counts_edge_lists(node_counts, edge_lists):
    """node_counts: list[int]; edge_lists: int64 [2, m_g] tensors with graph-local ids.  Returns one int32 [n_g, 11] CPU
    tensor per graph (columns: module docstring / GRAPHLET_ORBITS)."""
    return edge_list_labels("graphlet_counts", "graphlet", "esc_graphlet_counts", torch.int32, NUM_ORBITS, node_counts, edge_lists,
                            ld_out=NUM_ORBITS)


def graphlet_orbit_counts(data_list, chunk=65536):
    """per-graph int32 [n, 11] orbit counts of a list of Data (edge_index with graph-local ids), one launch per chunk"""
    return data_list_labels(graphlet_orbit_counts_edge_lists, data_list, chunk)


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
