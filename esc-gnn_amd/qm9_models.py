"""QM9 NestedGIN_eff — the MI355X twin of /root/reference/qm9_models.py:25-139.
The ZINC composition (zinc_models.py) with ReLU activations (fused into the HIP BatchNorm kernels), a dense node input
cat([x, pos], 1) + node_type_embedding(node_type) (ops.node_input: num_features + 3 columns, a 5-row table), dense float
edge features (bond one-hot + distance: edge_dim = 256 + edge_attr_dim), global_mean_pool readout and a flat output.
Same constructor and state_dict key layout as the reference class.  Per-op path only: the whole-step engines need widths
that are multiples of 4, and this model's are 11 and 261."""
import torch
import torch.nn.functional as F

from . import nested, ops
from .nested import Z_TABLE_ROWS
from .nn import BatchNorm1d, GINEConv, Linear, global_mean_pool
from .plan import plan_of


class NestedGIN_eff(torch.nn.Module):
    def __init__(self, dataset, num_layers, concat=False, use_pos=False, edge_attr_dim=5, use_max_dist=False, RNI=False,
                 **kwargs):
        super().__init__()
        self.use_z = True
        hidden, dropout = 256, 0.0
        self.dropout = dropout
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, hidden)
        self.z_embedding = nested.z_embedding(hidden, dropout=dropout)
        input_dim = dataset.num_features + 3
        self.conv1 = GINEConv(nested.mlp(input_dim, hidden, dropout), train_eps=True, edge_dim=hidden + edge_attr_dim)
        self.convs = torch.nn.ModuleList(
            GINEConv(nested.mlp(hidden, hidden, dropout), train_eps=True, edge_dim=hidden + edge_attr_dim)
            for _ in range(num_layers - 1))
        self.lin1 = Linear(num_layers * hidden, hidden)
        self.bn_lin1 = BatchNorm1d(hidden, eps=1e-5, momentum=0.1, fuse_relu=True)    # dropout is 0 => ReLU follows BN
        self.lin2 = Linear(hidden, 1)
        self.node_type_embedding = torch.nn.Embedding(5, input_dim)

    def reset_parameters(self):
        nested.reset_parameters(self, "z_embedding", "conv1", "convs", "lin1", "bn_lin1", "lin2", "node_type_embedding")

    def forward(self, data):
        data.to(self.lin1.weight.device)
        o = global_mean_pool(self._node_states(data), data.batch)
        o = self.lin1(o)
        o = self.bn_lin1(o) if o.size(0) > 1 else F.relu(o)      # reference :131-135 (dropout p = 0)
        return self.lin2(o).view(-1)

    def _node_states(self, data):
        """cat(xs) of the reference's :106-127: the node input, the edge term [z_emb | edge_attr] and the GINE layers"""
        x = ops.node_input(data.x, data.pos, data.node_type, self.node_type_embedding.weight)
        edge_index = data.edge_index
        plan = plan_of(data, Z_TABLE_ROWS)
        z = self.z_embedding(nested.edge_term(self.z_initial, data, plan))
        z = torch.cat((z, data.edge_attr), dim=-1)
        return torch.cat(nested.conv_stack(self, x, edge_index, z, plan), dim=1)
