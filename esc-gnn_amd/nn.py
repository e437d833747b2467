"""torch.nn-compatible layers whose arithmetic runs in libescgnn_hip.so.

`Linear` keeps torch.nn.Linear's parameters / init / state_dict keys but multiplies on the fp32
matrix cores; `GINEConv` mirrors the constructor and state_dict layout of PyG 2.0.4's GINEConv as
the reference instantiates it (run_graphcount.py:77-89,97-109: nn=Sequential(...), train_eps=True,
edge_dim=hidden -> parameters `eps`, `nn.*`, `lin.{weight,bias}`).
"""
import torch

from . import ops
from .plan import plan_of


class Linear(torch.nn.Linear):
    def forward(self, x):
        lead = x.shape[:-1]
        y = ops.linear(x.reshape(-1, x.shape[-1]), self.weight, self.bias)
        return y.view(*lead, self.out_features)


class BatchNorm1d(torch.nn.BatchNorm1d):
    """torch.nn.BatchNorm1d (same parameters/buffers/state_dict) computed by the HIP norm kernels.
    `fuse_relu=True` also applies the ReLU that follows it in the reference's Sequential (the
    ReLU module stays in place as `AbsorbedReLU` so the child indices / checkpoint keys match)."""

    ACT = {None: 0, False: 0, "none": 0, True: 1, "relu": 1, "elu": 2}

    def __init__(self, num_features, eps=1e-5, momentum=0.1, fuse_relu=False):
        """fuse_relu: False/None | True/'relu' | 'elu' — the activation module that follows in the reference."""
        super().__init__(num_features, eps=eps, momentum=momentum)
        self.fuse_relu = self.ACT[fuse_relu]
        self.sync_group = False        # False: per-rank statistics; None / a ProcessGroup: statistics over that group

    @staticmethod
    def convert_sync(module, group=None):
        """Switch every esc BatchNorm1d under `module` to statistics over all ranks of `group` (default group if None)
        — the counterpart of torch.nn.SyncBatchNorm.convert_sync_batchnorm for graph-sharded data parallelism."""
        for m in module.modules():
            if isinstance(m, BatchNorm1d):
                m.sync_group = group
        return module

    def forward(self, x):
        if x.dim() != 2:
            raise ValueError("expected 2D input (got {}D input)".format(x.dim()))
        if self.training:
            if self.num_batches_tracked is not None:
                self.num_batches_tracked.add_(1)
            if self.sync_group is not False:
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.sync_group) > 1:
                    return ops.sync_batch_norm_act(x, self.weight, self.bias, self.running_mean, self.running_var,
                                                   self.eps, self.momentum, self.fuse_relu, self.sync_group)
            return ops.batch_norm_act(x, self.weight, self.bias, self.running_mean, self.running_var,
                                      self.eps, self.momentum, self.fuse_relu)
        return ops.bn_eval_act(x, self.weight, self.bias, self.running_mean, self.running_var, self.eps,
                               self.fuse_relu)


class AbsorbedReLU(torch.nn.ReLU):
    """Placeholder for a ReLU whose work is fused into the preceding BatchNorm1d(fuse_relu=True)."""

    def forward(self, x):
        return x


class AbsorbedELU(torch.nn.ELU):
    """Placeholder for an ELU fused into the preceding BatchNorm1d(fuse_relu='elu')."""

    def forward(self, x):
        return x


class ELU(torch.nn.ELU):
    """torch.nn.ELU(alpha = 1) computed by the HIP activation kernel (ops.elu) — an ELU with no BatchNorm in front of it to
    absorb it (reference run_csl.py:152-169).  No parameters: child indices and state_dict layout are torch.nn.ELU's."""

    def __init__(self, alpha=1.0, inplace=False):
        if alpha != 1.0:
            raise ValueError("esc_gnn_amd.nn.ELU: only alpha = 1.0 has a kernel (got %r)" % (alpha,))
        super().__init__(alpha=alpha, inplace=False)

    def forward(self, x):
        lead = x.shape[:-1]
        return ops.elu(x.reshape(-1, x.shape[-1])).view(*lead, x.shape[-1])


class ReLU(torch.nn.ReLU):
    """torch.nn.ReLU computed by the HIP activation kernel (ops.relu) — a ReLU with no BatchNorm in front of it to absorb it
    (the GINE MLP, the feed-forward block and the head of the reference's graph transformer)."""

    def __init__(self, inplace=False):
        super().__init__(inplace=False)

    def forward(self, x):
        lead = x.shape[:-1]
        return ops.relu(x.reshape(-1, x.shape[-1])).view(*lead, x.shape[-1])


class Embedding(torch.nn.Embedding):
    """torch.nn.Embedding whose lookup and gradient run through the ESC bag kernels (one entry of weight 1 per row)."""

    def forward(self, index):
        return ops.embedding(self.weight, index)


class GINEConv(torch.nn.Module):
    """out = nn( sum_{j->i} relu(x_j + lin(e_ji)) + (1 + eps) * x_i )"""

    def __init__(self, nn, eps=0.0, train_eps=False, edge_dim=None):
        super().__init__()
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.Tensor([eps]))
        else:
            self.register_buffer("eps", torch.Tensor([eps]))
        first = nn[0]
        in_channels = first.in_features if hasattr(first, "in_features") else first.in_channels
        self.lin = Linear(edge_dim, in_channels) if edge_dim is not None else None

    def reset_parameters(self):
        for m in self.nn.modules():
            if m is not self.nn and hasattr(m, "reset_parameters"):
                m.reset_parameters()
        self.eps.data.fill_(self.initial_eps)
        if self.lin is not None:
            self.lin.reset_parameters()

    def forward(self, x, edge_index, edge_attr=None, plan=None):
        if plan is None:
            from .plan import BatchPlan
            plan = BatchPlan.from_tensors(edge_index, x.size(0))
        if self.lin is None and x.size(-1) != edge_attr.size(-1):
            raise ValueError("Node and edge feature dimensionalities do not match. "
                             "Consider setting the 'edge_dim' attribute of 'GINEConv'")
        e = self.lin(edge_attr) if self.lin is not None else edge_attr
        return self.nn(ops.gine_aggregate(x, e, self.eps, plan))

    def __repr__(self):
        return "{}(nn={})".format(self.__class__.__name__, self.nn)


class GatedGCNLayer(torch.nn.Module):
    """The reference's GatedGCNLayer (GraphGPS/graphgps/layer/gatedgcn_layer.py:11-136, Residual Gated Graph ConvNets) without
    EquivStableLapPE: the same parameters, names and construction order - A, B, C, D, E (this module's Linear), bn_node_x,
    bn_edge_e (this module's BatchNorm1d with the ReLU that follows it absorbed) - so equal seeds give equal weights and a
    reference checkpoint loads.  forward(x, e, plan) -> (x, e): the five Linears, ops.gated_gcn_aggregate (one launch), the two
    BatchNorm+ReLU, F.dropout on both and, with `residual`, the two residual adds.  The edge attributes leave the layer
    updated: the only local layer of the reference's GPSLayer that carries them on."""

    def __init__(self, in_dim, out_dim, dropout, residual, act="relu", equivstable_pe=False):
        super().__init__()
        if equivstable_pe:
            raise ValueError("GatedGCNLayer: equivstable_pe (the EquivStableLapPE gate r_ij) is not supported")
        if act != "relu":
            raise ValueError("GatedGCNLayer: only act 'relu' is supported (got %r)" % (act,))
        if residual and in_dim != out_dim:
            raise ValueError("GatedGCNLayer: residual needs in_dim == out_dim (got %d and %d)" % (in_dim, out_dim))
        self.A = Linear(in_dim, out_dim, bias=True)
        self.B = Linear(in_dim, out_dim, bias=True)
        self.C = Linear(in_dim, out_dim, bias=True)
        self.D = Linear(in_dim, out_dim, bias=True)
        self.E = Linear(in_dim, out_dim, bias=True)
        self.bn_node_x = BatchNorm1d(out_dim, fuse_relu=True)
        self.bn_edge_e = BatchNorm1d(out_dim, fuse_relu=True)
        self.dropout = dropout
        self.residual = residual

    def forward(self, x, e, plan):
        Ax, Bx, Ce, Dx, Ex = self.A(x), self.B(x), self.C(e), self.D(x), self.E(x)       # gatedgcn_layer.py:57-61
        h, e_ij = ops.gated_gcn_aggregate(Ax, Bx, Dx, Ex, Ce, plan)
        h = torch.nn.functional.dropout(self.bn_node_x(h), self.dropout, training=self.training)
        e_ij = torch.nn.functional.dropout(self.bn_edge_e(e_ij), self.dropout, training=self.training)
        if self.residual:
            h, e_ij = x + h, e + e_ij
        return h, e_ij


class PNAConv(torch.nn.Module):
    """PyG's PNAConv (Principal Neighbourhood Aggregation) as the reference's GPSLayer constructs it
    (GraphGPS/graphgps/layer/gps_layer.py:78-93): aggregators ['mean', 'max', 'sum'], scaler 'identity', one tower, one pre-
    and one post-layer.  The modules, their names and their construction order are PyG's - edge_encoder, pre_nns.0.0,
    post_nns.0.0, lin (this module's Linear) - so equal seeds give equal weights and a state_dict in that layout loads; `deg`
    only feeds the degree scalers, which are not selected: no buffer comes of it.

        m_k = pre_nns.0.0(cat[x_i, x_j, edge_encoder(e_k)])       out = lin(post_nns.0.0(cat[x, mean, max, sum]))

    pre_nns.0.0 is one Linear, so with its weight cut by input columns, W = [W_i | W_j | W_e], the message is
    (P[i] + Q[j]) + R[k] with P = x W_i^T + b, Q = x W_j^T, R = edge_encoder(e) W_e^T: three GEMMs on slices of the one
    parameter, then ops.pna_aggregate (one launch; csrc/pna.hip).  forward(x, edge_index, edge_attr, plan) -> [N, out]."""

    def __init__(self, in_channels, out_channels, aggregators=("mean", "max", "sum"), scalers=("identity",), deg=None, edge_dim=None,
                 towers=1, pre_layers=1, post_layers=1, divide_input=False):
        super().__init__()
        if list(aggregators) != ["mean", "max", "sum"]:
            raise ValueError("PNAConv: aggregators %r: only ['mean', 'max', 'sum'], in this order, are supported" % (list(aggregators),))
        if list(scalers) != ["identity"]:
            raise ValueError("PNAConv: scalers %r: only ['identity'] is supported" % (list(scalers),))
        if towers != 1:
            raise ValueError("PNAConv: towers=%r: only one tower is supported" % (towers,))
        if pre_layers != 1:
            raise ValueError("PNAConv: pre_layers=%r: only one pre-layer is supported" % (pre_layers,))
        if post_layers != 1:
            raise ValueError("PNAConv: post_layers=%r: only one post-layer is supported" % (post_layers,))
        if edge_dim is None:
            raise ValueError("PNAConv: edge_dim=None: the layer is built for edge attributes (edge_dim is required)")
        if in_channels != out_channels:
            raise ValueError("PNAConv: in_channels=%d and out_channels=%d must be equal" % (in_channels, out_channels))
        self.in_channels, self.out_channels, self.edge_dim = in_channels, out_channels, edge_dim
        self.edge_encoder = Linear(edge_dim, in_channels)
        self.pre_nns = torch.nn.ModuleList([torch.nn.Sequential(Linear(3 * in_channels, in_channels))])
        self.post_nns = torch.nn.ModuleList([torch.nn.Sequential(Linear(4 * in_channels, out_channels))])
        self.lin = Linear(out_channels, out_channels)

    def forward(self, x, edge_index, edge_attr, plan=None):
        if plan is None:
            from .plan import BatchPlan
            plan = BatchPlan.from_tensors(edge_index, x.size(0))
        H, pre = self.in_channels, self.pre_nns[0][0]
        P = ops.linear(x, pre.weight[:, :H], pre.bias)
        Q = ops.linear(x, pre.weight[:, H:2 * H])
        R = ops.linear(self.edge_encoder(edge_attr), pre.weight[:, 2 * H:])
        agg = ops.pna_aggregate(P, Q, R, plan)                                       # [N, 3H]: mean | max | sum
        return self.lin(self.post_nns[0][0](torch.cat([x, agg], 1)))


def global_add_pool(x, batch, size=None):
    """PyG global_add_pool: segment sum by graph id (HIP segment_pool kernels)."""
    return ops.segment_pool(x, batch, size, mean=False)


def global_mean_pool(x, batch, size=None):
    """PyG global_mean_pool: segment sum / max(count, 1)."""
    return ops.segment_pool(x, batch, size, mean=True)


class GraphMultiheadAttention(torch.nn.Module):
    """torch.nn.MultiheadAttention(embed_dim, num_heads, dropout, batch_first=True) as self-attention inside every graph of a
    ragged batch: the same parameters, initialisation and state_dict keys (in_proj_weight, in_proj_bias, out_proj.weight,
    out_proj.bias - a reference checkpoint's attention block loads unchanged), computed as ops.linear -> ops.graph_attention ->
    ops.linear off graph_ptr instead of to_dense_batch + key_padding_mask + gather."""

    def __init__(self, embed_dim, num_heads, dropout=0.0):
        super().__init__()
        if embed_dim % num_heads:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.embed_dim, self.num_heads, self.dropout = embed_dim, num_heads, dropout
        self.in_proj_weight = torch.nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = torch.nn.Parameter(torch.empty(3 * embed_dim))
        self.out_proj = Linear(embed_dim, embed_dim)
        self.reset_parameters()

    def reset_parameters(self):
        """torch.nn.MultiheadAttention._reset_parameters"""
        torch.nn.init.xavier_uniform_(self.in_proj_weight)
        torch.nn.init.constant_(self.in_proj_bias, 0.0)
        torch.nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, x, graph_ptr, max_nodes=None, spd=None, bias_table=None):
        """spd (uint8, the batch's attn_bias) and bias_table [101, num_heads], both or neither: the float attn_mask of the
        reference's BiasedTransformer as the table it collapses to (ops.graph_attention)"""
        qkv = ops.linear(x, self.in_proj_weight, self.in_proj_bias)
        h = ops.graph_attention(qkv, graph_ptr, self.num_heads, p=self.dropout, training=self.training, max_nodes=max_nodes, spd=spd,
                                bias_table=bias_table)
        return self.out_proj(h)


class GraphLayerNorm(torch.nn.Module):
    """PyG's norm.LayerNorm(in_channels) in graph mode - the reference's gt.layer_norm calls it as norm(h, batch.batch)
    (gps_layer.py:226-227,249-250,261-262): one mean and one variance over all nodes and all channels of each graph.  The same
    parameters, initial values and state_dict keys (weight: ones, bias: zeros; none with affine=False), computed by
    ops.graph_layer_norm off graph_ptr: one launch forward, two backward.  forward(x, graph_ptr, residual=None) normalises
    x + residual with the add folded into the launch.  No running statistics: train and eval are the same computation."""

    def __init__(self, in_channels, eps=1e-5, affine=True):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps
        if affine:
            self.weight = torch.nn.Parameter(torch.empty(in_channels))
            self.bias = torch.nn.Parameter(torch.empty(in_channels))
        else:
            self.register_parameter("weight", None)
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        if self.weight is not None:
            torch.nn.init.ones_(self.weight)
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, graph_ptr, residual=None):
        return ops.graph_layer_norm(x, graph_ptr, self.weight, self.bias, self.eps, residual)

    def extra_repr(self):
        return "%d, eps=%g, affine=%s" % (self.in_channels, self.eps, self.weight is not None)


class LapPENodeEncoder(torch.nn.Module):
    """The reference's LapPENodeEncoder (GraphGPS/graphgps/encoder/laplace_pos_encoder.py) as zinc-GPS.yaml configures it and as
    Concat2NodeEncoder builds it (expand_x False): model DeepSet, `layers` 2, post_layers 0, raw_norm_type none.  The same
    parameters, names and initial values - linear_A.{weight,bias} [2 dim_pe, 2] and pe_encoder.1.{weight,bias}
    [dim_pe, 2 dim_pe] in Sequential(ReLU, Linear, ReLU) - computed by ops.lappe_encode: one launch forward, two backward.
    forward(batch) -> [N, dim_pe], the rows the reference concatenates to batch.x.  In training one vector of random signs is
    drawn per call (torch.rand(K) >= 0.5 -> +-1, on the batch's device as the reference does); `signs_override` (a [K] tensor
    of +-1, default None) replaces the draw."""

    def __init__(self, dim_pe=8, max_freqs=8, layers=2, model="DeepSet", post_layers=0, raw_norm_type="none"):
        super().__init__()
        if model != "DeepSet" or layers != 2 or post_layers != 0 or str(raw_norm_type).lower() != "none":
            raise ValueError("LapPENodeEncoder: supported are model 'DeepSet' (not %r), layers 2 (not %r), post_layers 0 (not %r) and "
                             "raw_norm_type 'none' (not %r)" % (model, layers, post_layers, raw_norm_type))
        self.dim_pe, self.max_freqs = dim_pe, max_freqs
        self.linear_A = torch.nn.Linear(2, dim_pe)               # laplace_pos_encoder.py:47 - replaced at once (line 67), but it
        self.linear_A = torch.nn.Linear(2, 2 * dim_pe)           # has consumed the generator: equal seeds give equal weights
        self.pe_encoder = torch.nn.Sequential(torch.nn.ReLU(), torch.nn.Linear(2 * dim_pe, dim_pe), torch.nn.ReLU())
        self.signs_override = None

    def forward(self, batch):
        if not (hasattr(batch, "EigVals") and hasattr(batch, "EigVecs")):
            raise ValueError("Precomputed eigen values and vectors are required for %s; set config 'posenc_LapPE.enable' to True"
                             % self.__class__.__name__)
        vecs, vals = batch.EigVecs, batch.EigVals
        signs = None
        if self.signs_override is not None:
            signs = self.signs_override.to(device=vecs.device, dtype=torch.float32)
        elif self.training:
            signs = torch.where(torch.rand(vecs.size(1), device=vecs.device) >= 0.5, 1.0, -1.0)
        lin = self.pe_encoder[1]
        return ops.lappe_encode(vecs, vals, signs, self.linear_A.weight, self.linear_A.bias, lin.weight, lin.bias)


class RWSENodeEncoder(torch.nn.Module):
    """The reference's RWSENodeEncoder (KernelPENodeEncoder with kernel_type 'RWSE', GraphGPS/graphgps/encoder/
    kernel_pos_encoder.py:8-110) as the composed node encoders build it (expand_x False): raw_norm = BatchNorm1d(num_steps) for
    'batchnorm' (anything else: None, as in the reference), pe_encoder = Linear(num_steps, dim_pe) for model 'linear' or the
    reference's Sequential of Linear / ReLU pairs for 'mlp'.  The same parameters, names and construction order, so equal seeds
    give equal weights; built from this module's Linear, ReLU and BatchNorm1d: forward and backward run the library's kernels.
    forward(batch) -> [N, dim_pe], the rows the reference concatenates to batch.x, off batch.pestat_RWSE [N, num_steps]
    (rwse.add_rwse, rwse.RWSETable.attach)."""

    def __init__(self, dim_pe, num_steps, model="linear", layers=1, raw_norm="batchnorm", expand_x=False, pass_as_var=False):
        super().__init__()
        if expand_x or pass_as_var:
            raise ValueError("RWSENodeEncoder: expand_x and pass_as_var are not supported (the composed node encoders use neither)")
        self.dim_pe, self.num_steps = int(dim_pe), int(num_steps)
        self.raw_norm = BatchNorm1d(self.num_steps) if str(raw_norm).lower() == "batchnorm" else None
        model_type = str(model).lower()
        if model_type == "mlp":
            seq = []
            if layers == 1:
                seq += [Linear(self.num_steps, self.dim_pe), ReLU()]
            else:
                seq += [Linear(self.num_steps, 2 * self.dim_pe), ReLU()]
                for _ in range(layers - 2):
                    seq += [Linear(2 * self.dim_pe, 2 * self.dim_pe), ReLU()]
                seq += [Linear(2 * self.dim_pe, self.dim_pe), ReLU()]
            self.pe_encoder = torch.nn.Sequential(*seq)
        elif model_type == "linear":
            self.pe_encoder = Linear(self.num_steps, self.dim_pe)
        else:
            raise ValueError(f"{self.__class__.__name__}: Does not support '{model_type}' encoder model.")

    def forward(self, batch):
        if not hasattr(batch, "pestat_RWSE"):
            raise ValueError(f"Precomputed 'pestat_RWSE' variable is required for {self.__class__.__name__}; set config "
                             f"'posenc_RWSE.enable' to True, and also set 'posenc.kernel.times' values")
        pos_enc = batch.pestat_RWSE
        if self.raw_norm is not None:
            pos_enc = self.raw_norm(pos_enc)
        return self.pe_encoder(pos_enc)
