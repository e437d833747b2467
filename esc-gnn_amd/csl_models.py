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

from . import nested, ops
from .nested import Z_TABLE_ROWS
from .nn import ELU, Linear, global_add_pool
from .plan import plan_of

NUM_CLASSES = 10


class NestedGIN(torch.nn.Module):
    def __init__(self, num_layers, hidden):
        super().__init__()
        self.conv1 = nested.plain_conv(1, hidden, ELU)
        self.convs = torch.nn.ModuleList(nested.plain_conv(hidden, hidden, ELU) for _ in range(num_layers - 1))
        self.lin1 = Linear(hidden, hidden)
        self.lin2 = Linear(hidden, NUM_CLASSES)
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, hidden)
        self.z_embedding = nested.z_embedding(hidden, "elu")

    def reset_parameters(self):
        nested.reset_parameters(self, "conv1", "convs", "z_embedding", "lin1", "lin2")

    def logits(self, data):
        """raw class scores [num_graphs, 10] (the training loop feeds them to ops.log_softmax_nll)"""
        dev = self.lin1.weight.device
        data.to(dev)
        edge_index = data.edge_index
        plan = plan_of(data, Z_TABLE_ROWS)
        # as in the reference's forward (:194-211), z_embedding is NOT applied: the bag output feeds the convolutions
        z = nested.edge_term(self.z_initial, data, plan)
        x = data.x.float() if "x" in data else torch.ones([data.num_nodes, 1], device=dev)
        x = global_add_pool(nested.conv_stack(self, x, edge_index, z, plan)[-1], data.batch)
        x = ops.elu(self.lin1(x))
        x = F.dropout(x, p=0.5, training=self.training)
        return self.lin2(x)

    def forward(self, data):
        return self.logits(data)

    def __repr__(self):
        return self.__class__.__name__
