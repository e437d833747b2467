"""Per-node cycle-counting labels of the ZINC cycle task, computed on the device (csrc/cycles.hip, esc_cycle_counts).

Restates the reference's dataset_zinc_cycle.py:45-61 (pkl2data): self loops dropped, edges symmetrised, and for every
node the number of undirected simple cycles of length 3, 4, 5 and 6 through it (networkx simple_cycles, length 3..6,
+1 per node and cycle, halved).  Graphs of up to 64 nodes (ZINC molecules have at most 38 atoms).
"""
import torch

from .ragged import ESC_ERANGE, MAX_NODES, data_list_labels, edge_list_labels  # noqa: F401  (the constants: part of the module's face)


def cycle_counts_edge_lists(node_counts, edge_lists):
    """node_counts: list[int]; edge_lists: int64 [2, m_g] tensors with graph-local ids.  Returns one float32 [n_g, 4]
    CPU tensor per graph (columns: 3-, 4-, 5-, 6-cycles through the node)."""
    return edge_list_labels("cycle_counts", "cycle", "esc_cycle_counts", torch.float32, 4, node_counts, edge_lists)


def cycle_counts(data_list, chunk=65536):
    """per-graph float32 [n, 4] cycle labels of a list of Data (edge_index with graph-local ids), one launch per chunk"""
    return data_list_labels(cycle_counts_edge_lists, data_list, chunk)
