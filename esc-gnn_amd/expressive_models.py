"""NestedGIN of the expressiveness experiments — the MI355X twin of the class both reference drivers define inline
(run_sr.py:139-214 = run_exp.py:143-218), which shadows the kernel/gin.py import they start with.

It differs from every other model here: the GINEConv MLPs are Linear, ReLU, Linear, ReLU with NO BatchNorm and a
constant eps (`train_eps=False`: a buffer), z_embedding has no Dropout entries (BN, ReLU, Linear, BN, ReLU: children
0..4), the readout is global_add_pool, and the head is relu(lin1) -> dropout(0.5) -> lin2: hidden -> hidden ->
log_softmax over `hidden` columns.  Same state_dict key order as the reference class (73 keys at 8 layers).

Every op runs per launch through libescgnn_hip.so (bag, Linear, BatchNorm, GINE aggregate, segment pool, log-softmax);
the dropout mask comes from torch's device generator, as in the other per-op models.  A whole-step engine for this
model is future work ("Expressiveness runs").
"""
import torch
import torch.nn.functional as F
from torch.nn import ReLU

from . import nested, ops
from .nested import Z_TABLE_ROWS
from .nn import Linear, global_add_pool
from .plan import plan_of


class NestedGIN(torch.nn.Module):
    def __init__(self, num_features, num_layers, hidden):
        super().__init__()
        self.conv1 = nested.plain_conv(num_features, hidden, ReLU)
        self.convs = torch.nn.ModuleList(nested.plain_conv(hidden, hidden, ReLU) for _ in range(num_layers - 1))
        self.lin1 = Linear(hidden, hidden)
        self.lin2 = Linear(hidden, hidden)
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, hidden)
        self.z_embedding = nested.z_embedding(hidden)

    def reset_parameters(self):
        nested.reset_parameters(self, "conv1", "convs", "z_embedding", "lin1", "lin2")

    def logits(self, data):
        """the head's input: everything up to lin2 (the training loop feeds it to ops.log_softmax_nll)"""
        dev = self.lin1.weight.device
        data.to(dev)
        edge_index = data.edge_index
        plan = plan_of(data, Z_TABLE_ROWS)
        z = self.z_embedding(nested.edge_term(self.z_initial, data, plan))
        x = data.x.float() if "x" in data else torch.ones([data.num_nodes, 1], device=dev)
        x = global_add_pool(nested.conv_stack(self, x, edge_index, z, plan)[-1], data.batch)
        x = F.relu(self.lin1(x))
        x = F.dropout(x, p=0.5, training=self.training)
        return self.lin2(x)

    def forward(self, data):
        return ops.log_softmax(self.logits(data))

    def __repr__(self):
        return self.__class__.__name__
