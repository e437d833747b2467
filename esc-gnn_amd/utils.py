"""`create_subgraphs` of the node-rooted baseline (the reference's utils.py:18-132) for ONE graph, computed by the HIP
subgraph expansion (csrc/subgraphs.hip).  Same signature and the same keys on the returned Data, as CPU tensors; the sub-nodes
of a root come in the canonical order (root, then ascending (hop, node id)) where the reference has the iteration order of a
python set.  Training does not come through here: run_zinc expands whole batches on the device (subgraphs.expand_subgraphs).
"""
import torch

from .data import Data
from .subgraphs import collate_graphs, expand_subgraphs

_COPIED_AWAY = ("x", "edge_index", "edge_attr", "pos", "num_nodes", "batch", "z", "rd", "node_type")


def create_subgraphs(data, h=1, sample_ratio=1.0, max_nodes_per_hop=None, node_label='hop', use_rd=False,
                     subgraph_pretransform=None, data_name=None):
    assert isinstance(data, Data)
    n = int(data.num_nodes)
    plain = Data(x=data.x, edge_index=data.edge_index, edge_attr=data.edge_attr, num_nodes=n)
    sub = expand_subgraphs(collate_graphs([plain]), h, node_label=node_label, use_rd=use_rd,
                           max_nodes_per_hop=max_nodes_per_hop, subgraph_pretransform=subgraph_pretransform, check=True)
    out = Data(x=None if data.x is None else sub.x.cpu(), edge_index=sub.edge_index.cpu(),
               edge_attr=None if data.edge_attr is None else sub.edge_attr.cpu(), z=sub.z.cpu())
    if use_rd:
        out.rd = sub.rd.cpu()
    out.num_nodes = int(sub.z.size(0))
    out.num_subgraphs = n
    out.original_edge_index, out.original_edge_attr, out.original_pos = data.edge_index, data.edge_attr, data.pos
    data.original_num_nodes = n                              # (the reference sets it on its input, :93)
    out.node_to_subgraph = sub.node_to_subgraph.cpu()
    out.node_id = sub.sub_node_ptr[:-1].cpu()                # first sub-node of every subgraph (:101)
    out.subgraph_to_graph = torch.zeros(n, dtype=torch.long)
    for k, v in data:                                        # the remaining graph attributes (:122-125)
        if k not in _COPIED_AWAY:
            out[k] = v
    return out
