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
from torch.nn import ReLU, Sequential

from . import ops
from .nn import GINEConv, Linear, global_add_pool
from .plan import plan_of
from .run_graphcount import Z_TABLE_ROWS, _bn_relu


def _conv(n_in, hidden):
    return GINEConv(Sequential(Linear(n_in, hidden), ReLU(), Linear(hidden, hidden), ReLU()), train_eps=False,
                    edge_dim=hidden)


class NestedGIN(torch.nn.Module):
    def __init__(self, num_features, num_layers, hidden):
        super().__init__()
        self.conv1 = _conv(num_features, hidden)
        self.convs = torch.nn.ModuleList(_conv(hidden, hidden) for _ in range(num_layers - 1))
        self.lin1 = Linear(hidden, hidden)
        self.lin2 = Linear(hidden, hidden)
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, hidden)
        self.z_embedding = Sequential(*_bn_relu(hidden), Linear(hidden, hidden), *_bn_relu(hidden))

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
        """the head's input: everything up to lin2 (the training loop feeds it to ops.log_softmax_nll)"""
        dev = self.lin1.weight.device
        data.to(dev)
        edge_index = data.edge_index
        plan = plan_of(data, Z_TABLE_ROWS)
        if "edge_pos" in data:                       # dense layout of the slow variant (run_sr.py:186-189)
            z = ops.linear(data.edge_pos.float(), self.z_initial.weight.t().contiguous())
        else:
            z = ops.esc_bag(self.z_initial.weight, plan)
        z = self.z_embedding(z)
        x = data.x.float() if "x" in data else torch.ones([data.num_nodes, 1], device=dev)
        x = self.conv1(x, edge_index, z, plan)
        for conv in self.convs:
            x = conv(x, edge_index, z, plan)
        x = global_add_pool(x, data.batch)
        x = F.relu(self.lin1(x))
        x = F.dropout(x, p=0.5, training=self.training)
        return self.lin2(x)

    def forward(self, data):
        return ops.log_softmax(self.logits(data))

    def __repr__(self):
        return self.__class__.__name__
