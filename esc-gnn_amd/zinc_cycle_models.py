"""ZINC cycle counting: NestedGIN_eff of the reference's zinc_cycle_models.py:506-613, the node-level twin of
zinc_models.NestedGIN_eff.  The two class bodies differ in one line: the cycle model drops global_add_pool, so lin1 reads
cat(xs) row by row, bn_lin1 normalises over the nodes and lin2 predicts one value per node (the 3..6-cycles through it,
run_zinc_cycle.py).  Same constructor, parameters and state_dict keys as zinc_models.NestedGIN_eff; the training and eval
forwards run through the ZINC step engine with node_readout = 1 (csrc/engine.hip esc_zinc_*).

I2GNN (:116-307) is the subgraph GNN that counts cycles, the baseline of `run_zinc_cycle --model I2GNN`: per-op path, fed by
subgraphs2.expand_subgraphs2."""
import torch
import torch.nn.functional as F

from . import ops, zinc_models
from .nn import BatchNorm1d, Embedding, Linear, global_add_pool, global_mean_pool
from .plan import BatchPlan
from .zinc_models import GINConv


class NestedGIN_eff(zinc_models.NestedGIN_eff):
    node_readout = True            # esc_zinc_gin_t.node_readout: pred / y / loss per node

    def _readout(self, states, data):
        o = self.lin1(states)                              # reference :601-602: no pooling
        o = self.bn_lin1(o) if o.size(0) > 1 else F.elu(o)  # :603-607 (dropout p = 0; ELU fused into the BatchNorm)
        return self.lin2(o)


class _ReLU(torch.nn.ReLU):
    """torch.nn.ReLU on the HIP activation kernel: a ReLU between two Linear layers, with no BatchNorm in front to absorb it"""

    def forward(self, x):
        return ops.relu(x)


class I2GNN(torch.nn.Module):
    """The subgraph GNN that counts cycles, which ESC-GNN is measured against on this task — the twin of the reference's
    zinc_cycle_models.py:116-307: same constructor arguments, same state_dict keys and shapes.  `data` is what
    subgraphs2.expand_subgraphs2 returns: every rooted subgraph once per neighbour of its root as one disconnected graph
    (z [Ns, 4], rd [Ns, 2], node_to_subgraph2, subgraph2_to_subgraph, center_idx, node_to_original_node, s2_node_ptr).
    Node level: one prediction per original node (`graph_pooling(..., aggr='no')`).  Trains on the per-op path."""

    split_double_linear = True     # the first Linear of double_nns by column blocks of its weight (same keys; see forward)

    def __init__(self, dataset, num_layers=5, subgraph_pooling='mean', subgraph2_pooling='mean', use_pooling_nn=False,
                 use_pos=False, use_virtual_node=False, edge_attr_dim=5, use_rd=False, RNI=False, drop_ratio=0, degree=None,
                 double_pooling=False, gate=False, **kwargs):
        super().__init__()
        if subgraph_pooling not in ('mean', 'add', 'mean-context') or \
                subgraph2_pooling not in ('mean', 'add', 'center', 'mean-center', 'mean-center-side'):
            raise ValueError("I2GNN: subgraph_pooling=%r / subgraph2_pooling=%r" % (subgraph_pooling, subgraph2_pooling))
        for name, on in (("use_pos", use_pos), ("RNI", RNI), ("use_virtual_node", use_virtual_node)):
            if on:
                raise NotImplementedError("I2GNN: %s is accepted and never read by the reference's forward; there is no path "
                                          "for it here" % name)
        self.subgraph_pooling, self.subgraph2_pooling = subgraph_pooling, subgraph2_pooling
        s2_dim = 2 if subgraph2_pooling == 'mean-center' else 3 if subgraph2_pooling == 'mean-center-side' else 1
        s2_dim = s2_dim + 1 if subgraph_pooling == 'mean-context' else s2_dim
        self.use_rd = use_rd
        if self.use_rd:
            self.rd_projection = Linear(2, 8)              # (the reference builds it and never calls it; the key stays)
        self.node_type_embedding = Embedding(100, 8)
        self.double_pooling, self.res, self.gate, self.use_pooling_nn = double_pooling, True, gate, use_pooling_nn
        if self.gate:
            self.subgraph_gate = torch.nn.ModuleList()
        self.convs = torch.nn.ModuleList()
        self.norms = torch.nn.ModuleList()
        self.z_embedding_list = torch.nn.ModuleList()
        if self.use_rd:
            self.rd_projection_list = torch.nn.ModuleList()
        if self.double_pooling:
            self.double_nns = torch.nn.ModuleList()
        M_in, M_out = 1 + 8, 64
        for layer in range(num_layers):                    # construction order of the reference (:152-179): it fixes the seeds
            if layer == 0:
                self.convs.append(GINConv(2 * M_in, M_out))
            self.z_embedding_list.append(Embedding(100, M_in))
            if self.use_rd:
                self.rd_projection_list.append(Linear(2, M_in))
            if self.gate:                                  # the Sigmoid runs inside ops.sigmoid_mul; the module keeps its place
                self.subgraph_gate.append(torch.nn.Sequential(Linear(M_in, M_out), torch.nn.Sigmoid()))
            if layer > 0:
                self.convs.append(GINConv(2 * M_in, M_out))
            # F.elu follows every norm but the last (:280-282)
            self.norms.append(BatchNorm1d(M_out, fuse_relu="elu" if layer < num_layers - 1 else False))
            if self.double_pooling:
                self.double_nns.append(torch.nn.Sequential(Linear(M_out * (1 + s2_dim), 128), _ReLU(), Linear(128, M_out)))
            M_in, M_out = M_out, 64
        if use_pooling_nn:
            w = s2_dim * M_out
            self.edge_pooling_nn = torch.nn.Sequential(Linear(w, w), _ReLU(), Linear(w, w))
            self.node_pooling_nn = torch.nn.Sequential(Linear(w, w), _ReLU(), Linear(w, w))
        self.z_embedding_list.append(Embedding(100, M_out))
        if self.use_rd:
            self.rd_projection_list.append(Linear(2, M_out))
        if self.gate:
            self.subgraph_gate.append(torch.nn.Sequential(Linear(M_out, M_out), torch.nn.Sigmoid()))
        self.fc1 = Linear(s2_dim * M_out, 32)
        self.fc2 = Linear(32, 16)
        self.fc3 = Linear(16, 1)

    def _gated(self, x, z, layer):
        return ops.sigmoid_mul(self.subgraph_gate[layer][0](z), x) if self.gate else x

    def graph_pooling(self, x, data, z=None, layer=None, aggr='mean', node_emb_only=False):
        n2s2, s2s = data.node_to_subgraph2, data.subgraph2_to_subgraph
        S2, N = s2s.numel(), data.subgraph_to_graph.numel()
        if self.subgraph_pooling == 'mean-context':        # global_mean_pool over the UNSORTED node_to_original_node (:201-202)
            x_node = ops.group_mean(x, ops.group_plan(data.node_to_original_node, N))
        p2 = self.subgraph2_pooling
        if p2 == 'mean':
            x = global_mean_pool(self._gated(x, z, layer), n2s2, S2)
        elif p2 == 'add':
            x = global_add_pool(x, n2s2, S2)
        elif p2 == 'center':                               # the first row of every subgraph2 is its root: center_idx[:, 0]
            x = ops.segment_first(x, data.s2_node_ptr, n2s2)
        elif p2 == 'mean-center':
            x = torch.cat([global_mean_pool(x, n2s2, S2), ops.segment_first(x, data.s2_node_ptr, n2s2)], dim=-1)
        else:                                              # 'mean-center-side': one kernel for the three parts
            x = ops.pool_mean_center_side(self._gated(x, z, layer), data.s2_node_ptr, data.center_idx, n2s2)
        if self.use_pooling_nn:
            x = self.edge_pooling_nn(x)
        if self.subgraph_pooling == 'mean':
            x = global_mean_pool(x, s2s, N)
        elif self.subgraph_pooling == 'add':
            x = global_add_pool(x, s2s, N)
        else:
            x = torch.cat([global_mean_pool(x, s2s, N), x_node], dim=-1)
        if node_emb_only:
            return x
        if self.use_pooling_nn:
            x = self.node_pooling_nn(x)
        if aggr == 'mean':
            return global_mean_pool(x, data.subgraph_to_graph)
        if aggr == 'add':
            return global_add_pool(x, data.subgraph_to_graph)
        return x

    def _z_emb(self, data, layer):
        table = self.z_embedding_list[layer].weight        # embedding(z).sum(dim=1) (:264-266): the four columns share one table
        z_emb = ops.embedding_sum([table] * data.z.size(1), data.z)
        return z_emb + self.rd_projection_list[layer](data.rd) if self.use_rd else z_emb

    def forward(self, data):
        x_in = data.x.view(-1)
        x = torch.cat([self.node_type_embedding(x_in), x_in.view(-1, 1).to(torch.float32)], -1)
        plan = BatchPlan.from_tensors(data.edge_index, x.size(0))     # one plan per batch, shared by every layer
        N = data.subgraph_to_graph.numel()
        x0 = None
        for layer, conv in enumerate(self.convs):
            z_emb = self._z_emb(data, layer)
            x = conv(torch.cat([x, z_emb], dim=-1), data.edge_index, data.edge_attr.view(-1), plan)
            if self.double_pooling:                        # concat along subgraphs (:274-278)
                pooled = self.graph_pooling(x, data, z_emb, layer, node_emb_only=True)
                group = ops.group_plan(data.node_to_original_node, N)
                nn_ = self.double_nns[layer]
                if self.split_double_linear:
                    # Linear(cat[x, P[idx]]) = x W_x^T + (P W_p^T)[idx] + b: the wide part of the product runs on the N pooled
                    # rows instead of the ~30x expanded ones, and neither the 320-wide concatenation nor the 256-wide gather exists
                    C, w = x.size(1), nn_[0].weight
                    x = ops.linear(x, w[:, :C], nn_[0].bias) + ops.gather_rows(ops.linear(pooled, w[:, C:]), group)
                    x = nn_[2](nn_[1](x))
                else:
                    x = nn_(torch.cat([x, ops.gather_rows(pooled, group)], dim=-1))
            x = self.norms[layer](x)                       # BatchNorm (+ ELU in one kernel, except after the last layer)
            if layer > 0 and self.res:
                x = x + x0
            x0 = x
        x = self.graph_pooling(x, data, self._z_emb(data, -1), -1, aggr='no')
        x = ops.elu(self.fc1(x))
        x = ops.elu(self.fc2(x))
        return self.fc3(x)
