"""ZINC NestedGIN_eff — the MI355X twin of /root/reference/zinc_models.py:504-611 (BASELINE config 4).
ELU activations (fused into the HIP BatchNorm kernels), 32-wide node/edge type embeddings (looked up through
the ESC bag kernels), edge term = [z_emb | edge_type_embedding] (edge_dim = 256 + 32), global_add_pool
readout (HIP segment-pool), dropout 0.  Same constructor and state_dict key layout as the reference class."""
import torch
import torch.nn.functional as F

from . import engine, nested
from .nested import Z_TABLE_ROWS
from .nn import BatchNorm1d, Embedding, GINEConv, Linear, global_add_pool
from .plan import plan_of


class NestedGIN_eff(torch.nn.Module):
    def __init__(self, dataset, num_layers, concat=False, use_pos=False, use_max_dist=False, RNI=False, **kwargs):
        super().__init__()
        self.use_z = True
        self.step_engine = True       # training-mode forward through the whole-step engine when the batch allows it
        hidden, dropout = 256, 0.0
        self.dropout = dropout
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, hidden)
        self.z_embedding = nested.z_embedding(hidden, "elu", dropout)
        input_dim, edge_attr_dim = 32, 32
        self.conv1 = GINEConv(nested.mlp(input_dim, hidden, dropout, "elu"), train_eps=True, edge_dim=hidden + edge_attr_dim)
        self.convs = torch.nn.ModuleList(
            GINEConv(nested.mlp(hidden, hidden, dropout, "elu"), train_eps=True, edge_dim=hidden + edge_attr_dim)
            for _ in range(num_layers - 1))
        self.lin1 = Linear(num_layers * hidden, hidden)
        self.bn_lin1 = BatchNorm1d(hidden, eps=1e-5, momentum=0.1, fuse_relu="elu")   # dropout is 0 => ELU follows BN
        self.lin2 = Linear(hidden, 1)
        self.node_type_embedding = Embedding(100, 32)
        self.edge_type_embedding = Embedding(100, 32)

    def reset_parameters(self):
        nested.reset_parameters(self, "z_embedding", "conv1", "convs", "lin1", "bn_lin1", "lin2", "node_type_embedding",
                                "edge_type_embedding")

    def forward(self, data):
        data.to(self.lin1.weight.device)
        if self.step_engine and self.training == torch.is_grad_enabled() and engine.zinc_engine_ready(self, data):
            if self.training:
                return engine.zinc_engine_forward(self, data)     # the whole step as one autograd node (esc_zinc_*)
            return engine.zinc_engine_predict(self, data)         # eval-mode forward as one call (esc_zinc_predict)
        return self._readout(self._node_states(data), data)

    def _readout(self, states, data):
        """what follows the engine dispatch (reference :600-610); zinc_cycle_models overrides it"""
        o = self.lin1(global_add_pool(states, data.batch))
        o = self.bn_lin1(o) if o.size(0) > 1 else F.elu(o)      # reference :606-609 (dropout p = 0)
        return self.lin2(o)

    def _node_states(self, data):
        """cat(xs) of the per-op path (reference :581-598): the embeddings, the edge term and the GINE layers"""
        x, edge_index = self.node_type_embedding(data.x.view(-1)), data.edge_index
        plan = plan_of(data, Z_TABLE_ROWS)
        z = self.z_embedding(nested.edge_term(self.z_initial, data, plan))
        z = torch.cat((z, self.edge_type_embedding(data.edge_attr.view(-1))), dim=-1)
        return torch.cat(nested.conv_stack(self, x, edge_index, z, plan), dim=1)
