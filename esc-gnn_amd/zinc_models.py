"""ZINC NestedGIN_eff — the MI355X twin of /root/reference/zinc_models.py:504-611 (BASELINE config 4).
ELU activations (fused into the HIP BatchNorm kernels), 32-wide node/edge type embeddings (looked up through
the ESC bag kernels), edge term = [z_emb | edge_type_embedding] (edge_dim = 256 + 32), global_add_pool
readout (HIP segment-pool), dropout 0.  Same constructor and state_dict key layout as the reference class."""
import torch
import torch.nn.functional as F

from . import engine, nested, ops
from .nested import Z_TABLE_ROWS
from .nn import AbsorbedReLU, BatchNorm1d, Embedding, GINEConv, Linear, global_add_pool, global_mean_pool
from .plan import BatchPlan, plan_of


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


class GINConv(torch.nn.Module):
    """The reference's GINConv (zinc_models.py:615-645): out = mlp((1 + eps) x_i + sum_{j->i} relu(x_j + edge_encoder(e_ji))),
    mlp = Linear -> BatchNorm -> ReLU -> Linear, on the HIP aggregate / Linear / BatchNorm+ReLU kernels.  Same state_dict keys
    (mlp.0, mlp.1, mlp.3, eps, edge_encoder)."""

    def __init__(self, M_in, M_out):
        super().__init__()
        self.mlp = torch.nn.Sequential(Linear(M_in, 2 * M_in), BatchNorm1d(2 * M_in, fuse_relu=True), AbsorbedReLU(),
                                       Linear(2 * M_in, M_out))
        self.eps = torch.nn.Parameter(torch.Tensor([0]))
        self.edge_encoder = Embedding(5, M_in)

    def forward(self, x, edge_index, edge_attr, plan=None):
        if plan is None:
            plan = BatchPlan.from_tensors(edge_index, x.size(0))
        edge_embedding = self.edge_encoder(edge_attr)          # materialised [E, M_in] (ops.embedding)
        return self.mlp(ops.gine_aggregate(x, edge_embedding, self.eps, plan))


class NGNN(torch.nn.Module):
    """The node-rooted nested GNN ESC-GNN is measured against — the twin of the reference's zinc_models.py:306-405, same
    constructor arguments and state_dict layout.  `data` is what subgraphs.expand_subgraphs returns: every rooted subgraph as
    one disconnected graph (z, rd, node_to_subgraph, subgraph_to_graph, sub_node_ptr)."""

    def __init__(self, dataset, num_layers=5, subgraph_pooling='mean', use_pos=False, edge_attr_dim=5, use_rd=False, RNI=False,
                 **kwargs):
        super().__init__()
        if use_pos or RNI:
            raise NotImplementedError("NGNN: use_pos / RNI have no run script in the reference and no path here")
        self.subgraph_pooling, self.use_pos, self.use_rd, self.RNI, self.res = subgraph_pooling, use_pos, use_rd, RNI, True
        if self.use_rd:
            self.rd_projection_list = torch.nn.ModuleList()
        self.z_embedding_list = torch.nn.ModuleList()
        self.node_type_embedding = Embedding(100, 8)
        self.norms = torch.nn.ModuleList()
        self.convs = torch.nn.ModuleList()
        M_in, M_out = 1 + 8, 64
        for _ in range(num_layers):
            self.z_embedding_list.append(Embedding(100, M_in))
            if self.use_rd:
                self.rd_projection_list.append(Linear(1, M_in))
            self.convs.append(GINConv(2 * M_in, M_out))
            self.norms.append(BatchNorm1d(M_out, fuse_relu="elu"))       # F.elu follows norms[layer] (:381-382)
            M_in, M_out = M_out, 64
        self.fc1, self.fc2, self.fc3 = Linear(M_out, 32), Linear(32, 16), Linear(16, 1)

    def forward(self, data):
        x_in = data.x.view(-1)
        x = torch.cat([self.node_type_embedding(x_in), x_in.view(-1, 1).to(torch.float32)], -1)
        plan = BatchPlan.from_tensors(data.edge_index, x.size(0))     # one plan per batch, shared by every layer
        z = data.z
        x0 = None
        for layer, conv in enumerate(self.convs):
            table = self.z_embedding_list[layer].weight
            # embedding(z).sum(dim=1) (:374-376): the label columns share one table
            z_emb = ops.embedding_sum([table] * z.size(1), z) if z.size(1) > 1 else ops.embedding(table, z.view(-1))
            if self.use_rd:
                z_emb = z_emb + self.rd_projection_list[layer](data.rd)
            x = conv(torch.cat([x, z_emb], dim=-1), data.edge_index, data.edge_attr.view(-1), plan)
            x = self.norms[layer](x)                                   # BatchNorm + ELU in one kernel
            if layer > 0 and self.res:
                x = x + x0
            x0 = x
        if self.subgraph_pooling == 'center':                          # the first node of each subgraph is its root
            x = ops.segment_first(x, data.sub_node_ptr, data.node_to_subgraph)
        else:
            x = global_mean_pool(x, data.node_to_subgraph)
        x = global_mean_pool(x, data.subgraph_to_graph)
        x = ops.elu(self.fc1(x))
        x = ops.elu(self.fc2(x))
        return self.fc3(x)
