"""NestedGIN of the CSL expressiveness run — the MI355X twin of the class the reference's run_csl.py defines inline
(:145-225).

It is the expressiveness model (expressive_models.py) with ELU in place of ReLU and a 10-class head: the GINEConv MLPs
are Linear, ELU, Linear, ELU with NO BatchNorm and a constant eps (`train_eps=False`: a buffer), conv1 reads one input
column, the readout is global_add_pool, and the head is elu(lin1) -> dropout(0.5) -> lin2: hidden -> 10, returned as raw logits (the driver's
loss is cross-entropy).  Same constructor, module tree and state_dict key order as the reference class.

z_embedding (BN, ELU, Linear, BN, ELU: children 0..4, built here as BatchNorm1d fused with its ELU) is constructed, reset and
carried in the state_dict exactly as the reference does, and exactly as in the reference's forward it is never applied: the
ESC bag output goes to the convolutions as it is, and the block's parameters receive no gradient.

Every op runs per launch through libescgnn_hip.so; the bare ELUs are csrc/activation.hip (ops.elu), the dropout mask comes
from torch's device generator.  A whole-step engine for this model is future work.
"""
import torch
import torch.nn.functional as F
from torch.nn import Sequential

from . import ops
from .nn import AbsorbedELU, BatchNorm1d, ELU, GINEConv, Linear, global_add_pool
from .plan import plan_of
from .run_graphcount import Z_TABLE_ROWS

NUM_CLASSES = 10


def _conv(n_in, hidden):
    return GINEConv(Sequential(Linear(n_in, hidden), ELU(), Linear(hidden, hidden), ELU()), train_eps=False,
                    edge_dim=hidden)


def _bn_elu(hidden):
    return BatchNorm1d(hidden, fuse_relu="elu"), AbsorbedELU()


class NestedGIN(torch.nn.Module):
    def __init__(self, num_layers, hidden):
        super().__init__()
        self.conv1 = _conv(1, hidden)
        self.convs = torch.nn.ModuleList(_conv(hidden, hidden) for _ in range(num_layers - 1))
        self.lin1 = Linear(hidden, hidden)
        self.lin2 = Linear(hidden, NUM_CLASSES)
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, hidden)
        self.z_embedding = Sequential(*_bn_elu(hidden), Linear(hidden, hidden), *_bn_elu(hidden))

    def reset_parameters(self):
        self.conv1.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        for layer in self.z_embedding.children():
            if hasattr(layer, "reset_parameters"):
                layer.reset_parameters()
        self.lin1.reset_parameters()
        self.lin2.reset_parameters()

    def logits(self, data):
        """raw class scores [num_graphs, 10] (the training loop feeds them to ops.log_softmax_nll)"""
        dev = self.lin1.weight.device
        data.to(dev)
        edge_index = data.edge_index
        plan = plan_of(data, Z_TABLE_ROWS)
        if "edge_pos" in data:                       # dense layout of the slow variant (run_csl.py:196-199)
            z = ops.linear(data.edge_pos.float(), self.z_initial.weight.t().contiguous())
        else:
            z = ops.esc_bag(self.z_initial.weight, plan)
        # as in the reference's forward (:194-211), z_embedding is NOT applied: the bag output feeds the convolutions
        x = data.x.float() if "x" in data else torch.ones([data.num_nodes, 1], device=dev)
        x = self.conv1(x, edge_index, z, plan)
        for conv in self.convs:
            x = conv(x, edge_index, z, plan)
        x = global_add_pool(x, data.batch)
        x = ops.elu(self.lin1(x))
        x = F.dropout(x, p=0.5, training=self.training)
        return self.lin2(x)

    def forward(self, data):
        return self.logits(data)

    def __repr__(self):
        return self.__class__.__name__
