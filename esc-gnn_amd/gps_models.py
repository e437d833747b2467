"""ESC-GNN inside a graph transformer — the MI355X twin of the reference's GraphGPS fork for what configs/GPS/zinc-GPS.yaml
selects: GPSLayer (GraphGPS/graphgps/layer/gps_layer.py) with `GINE+Transformer`, batch_norm True, layer_norm False, and
GPSModel (graphgps/network/gps_model.py) with the TypeDictNode / TypeDictEdge encoders, head `san_graph` and add pooling.
Same state_dict key layout as the reference classes, so a reference checkpoint loads.

Every GPSLayer first adds the ESC edge term to the edge attributes — z_embedding(bag over its own z_initial table), the
primitive this library is built around — and the reference adds it IN PLACE (gps_layer.py:188): layer l therefore sees the
terms of layers 0..l.  Here the sum is carried from layer to layer as a value, which is the same arithmetic.  It then runs a
GINE layer and full self-attention over each graph's nodes side by side, adds the two and applies a feed-forward block.

All arithmetic runs through the ops of this package (bag, GINE aggregate, Linear, BatchNorm, ReLU / ELU, embeddings, ragged
attention, sum pooling); residual adds and the model-level Dropout stay torch ops as in the other models.  Per-op path only.

`edge_attn_emb` and `edge_attn_linear` exist in the reference's state_dict although nothing uses them with `Transformer`: they
are created here so that checkpoints load, and take no part in that forward.  global_model_type='BiasedTransformer' is what
they are for (gps_layer.py:237-239,273-278, Graphormer's spatial encoding): the batch's attn_bias - every graph's all-pairs
shortest-path distances, 100 for no path (spd.add_spd, spd.SPDTable.attach) - goes through the embedding and the three Linears
and is added to the attention scores per head.  The reference's own collate leaves the key None (loader/batch.py:132-141), and
its dense form is a [B, n_max, n_max, heads] MLP per layer; here the bias depends on (distance, head) alone, so each layer
evaluates edge_attn_linear(edge_attn_emb(arange(101))) once per forward - 101 x heads values of torch plumbing, through the
Embedding lookup so that padding_idx keeps row 100's gradient zero - and the biased ragged attention reads that table
(csrc/attention.hip).  The state_dict is the same under both types.

The yaml's node encoder is TypeDictNode+LapPE.  GPSModel(lap_pe=True) builds it as the reference's Concat2NodeEncoder does:
encoder1 = the type embedding at width dim_hidden - dim_pe, encoder2 = nn.LapPENodeEncoder over the batch's EigVals / EigVecs
(lappe.py computes them on the device), the node state their concatenation.  The default, lap_pe=False, is TypeDictNode at full
width with the state_dict that has.  GPSModel(rwse=True) is TypeDictNode+RWSE the same way (encoder2 = nn.RWSENodeEncoder over the
batch's pestat_RWSE, rwse.py), and both flags give the reference's only three-way encoder, TypeDictNode+LapPE+RWSE
(Concat3NodeEncoder: encoder2 = LapPE, encoder3 = RWSE).

GPSLayer / GPSModel(local_gnn_type='CustomGatedGCN') swaps the GINE layer for nn.GatedGCNLayer (gatedgcn_layer.py), the one other
local type the fork implements: it also returns new edge attributes, which the next layer's ESC term is added to;
global_model_type='None' drops the attention branch (self_attn None, no keys; norm1_attn stays, unused, as in the reference).

local_gnn_type='PNA' swaps it for nn.PNAConv (PyG's PNAConv as gps_layer.py:78-93 constructs it: aggregators mean / max / sum,
identity scaler, one tower, one pre- and one post-layer, edge_dim = min(128, dim_h)): treated as GINE is - dropout_local, the
residual, norm1_local - and like GINE it leaves the edge attributes alone.

layer_norm / batch_norm are the yaml's gt.layer_norm / gt.batch_norm (gps_layer.py:139-165): with layer_norm the three norms of
a layer are nn.GraphLayerNorm - PyG's norm.LayerNorm in graph mode, one mean and one variance over all nodes and channels of
each graph, state_dict keys weight and bias alone - and the residual add in front of each rides in the norm's launch
(csrc/layernorm.hip); with neither, the layer has no norm modules and applies none; both is the reference's ValueError.  The
BatchNorms inside GatedGCN and z_embedding stay what they are.  Unlike BatchNorm, a graph gets the same output alone and inside
any batch, in training and in evaluation.

Out of scope: Performer and BigBird, Graphormer's own encoders, log_attn_weights, edge-feature biases, the local GNN types GCN / GIN / GENConv / GAT, PNA's other
aggregators (min, std), degree scalers, towers and deeper pre- / post-layers, the
EquivStableLapPE gate of GINE and GatedGCN, a fused BatchNorm on GatedGCN's edge rows, the other positional
encodings (SignNet, EquivStableLapPE, HKdiagSE, ElstaticSE) and LapPE's Transformer model, graphgym's config system and wandb,
a whole-step engine, data parallelism."""
import torch
from torch.nn import Dropout, ModuleList, Sequential

from . import nested
from .nested import Z_TABLE_ROWS
from .nn import BatchNorm1d, Embedding, GatedGCNLayer, GINEConv, GraphLayerNorm, GraphMultiheadAttention, LapPENodeEncoder, Linear, PNAConv, ReLU, RWSENodeEncoder, global_add_pool
from .plan import graph_ptr_of, plan_of


class GPSLayer(torch.nn.Module):
    """Local message passing + full graph attention + feed-forward (gps_layer.py:19-302 with act 'relu' and batch_norm).
    local_gnn_type 'GINE' (the yaml's), 'PNA' (gps_layer.py:78-93: nn.PNAConv, handled as GINE is, :216-229) or
    'CustomGatedGCN' (gps_layer.py:94-99: nn.GatedGCNLayer with its own dropout and
    residual, whose edge output becomes the layer's edge attributes, :197-208); global_model_type 'Transformer',
    'BiasedTransformer' (the same attention with the shortest-path bias of edge_attn_emb / edge_attn_linear on its scores,
    :237-239,273-278) or 'None' (self_attn None: the attention branch is skipped; norm1_attn exists all the same, :150-152).
    layer_norm / batch_norm (:139-165): norm1_local, norm1_attn and norm2 are nn.GraphLayerNorm (each takes the residual add in
    front of it into its launch), BatchNorm1d, or - with neither - absent; both raises as the reference does."""

    def __init__(self, dim_h, num_heads, dropout=0.0, attn_dropout=0.0, local_gnn_type="GINE", global_model_type="Transformer",
                 layer_norm=False, batch_norm=True):
        super().__init__()
        if layer_norm and batch_norm:
            raise ValueError("Cannot apply two types of normalization together")
        self.layer_norm, self.batch_norm = bool(layer_norm), bool(batch_norm)
        norm = (lambda: GraphLayerNorm(dim_h)) if layer_norm else (lambda: BatchNorm1d(dim_h)) if batch_norm else None
        self.dim_h, self.num_heads = dim_h, num_heads
        if local_gnn_type == "GINE":
            self.local_model = GINEConv(Sequential(Linear(dim_h, dim_h), ReLU(), Linear(dim_h, dim_h)))  # constant eps = 0, no edge Linear
        elif local_gnn_type == "PNA":
            if dim_h > 128:                                   # edge_dim = min(128, dim_h): the reference would fail inside the encoder
                raise ValueError("GPSLayer: local_gnn_type 'PNA' takes dim_h <= 128 (got %d): its edge_dim is min(128, dim_h), "
                                 "and the edge attributes are dim_h wide" % dim_h)
            self.local_model = PNAConv(dim_h, dim_h, aggregators=["mean", "max", "sum"], scalers=["identity"], deg=None,
                                       edge_dim=min(128, dim_h), towers=1, pre_layers=1, post_layers=1, divide_input=False)
        elif local_gnn_type == "CustomGatedGCN":
            self.local_model = GatedGCNLayer(dim_h, dim_h, dropout=dropout, residual=True)
        else:
            raise ValueError(f"Unsupported local GNN model: {local_gnn_type}")
        self.local_gnn_type = local_gnn_type
        self.edge_attn_emb = torch.nn.Embedding(101, num_heads, padding_idx=100)                         # BiasedTransformer's; else unused
        self.edge_attn_linear = Sequential(torch.nn.Linear(num_heads, num_heads), torch.nn.ReLU(),
                                           torch.nn.Linear(num_heads, num_heads), torch.nn.ReLU(),
                                           torch.nn.Linear(num_heads, num_heads))
        if global_model_type == "None":
            self.self_attn = None
        elif global_model_type in ("Transformer", "BiasedTransformer"):
            self.self_attn = GraphMultiheadAttention(dim_h, num_heads, dropout=attn_dropout)
        else:
            raise ValueError(f"Unsupported global x-former model: {global_model_type}")
        self.global_model_type = global_model_type
        if norm is not None:
            self.norm1_local = norm()
            self.norm1_attn = norm()
        self.dropout_local = Dropout(dropout)
        self.dropout_attn = Dropout(dropout)
        self.ff_linear1 = Linear(dim_h, dim_h * 2)
        self.ff_linear2 = Linear(dim_h * 2, dim_h)
        self.act_fn_ff = ReLU()
        if norm is not None:
            self.norm2 = norm()
        self.ff_dropout1 = Dropout(dropout)
        self.ff_dropout2 = Dropout(dropout)
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, dim_h)
        self.z_embedding = nested.z_embedding(dim_h, "elu", dropout)

    def bias_table(self):
        """[101, heads]: what the reference's MLP gives every pair at each distance (row 100: no path, the padding row)"""
        index = torch.arange(101, device=self.edge_attn_emb.weight.device)
        return self.edge_attn_linear(self.edge_attn_emb(index))

    def _normed(self, name, value, graph_ptr, residual=None):
        """norm `name` of residual + value: the LayerNorm adds inside its launch, the BatchNorm behind a torch add; without norms
        the sum alone (gps_layer.py:224-229,248-252,260-264)"""
        if self.layer_norm:
            return getattr(self, name)(value, graph_ptr, residual=residual)
        if residual is not None:
            value = residual + value
        return getattr(self, name)(value) if self.batch_norm else value

    def forward(self, h, edge_attr, data, plan, graph_ptr, max_nodes):
        """(node states, edge attributes) -> the same after this layer; the edge attributes carry this layer's ESC term on"""
        if "pos_index" in data:
            edge_attr = edge_attr + self.z_embedding(nested.edge_term(self.z_initial, data, plan))
        if self.local_gnn_type == "CustomGatedGCN":          # it drops out and adds its residuals itself (gps_layer.py:206-208)
            h_local, edge_attr = self.local_model(h, edge_attr, plan)
            h_local = self._normed("norm1_local", h_local, graph_ptr)
        else:
            h_local = self.dropout_local(self.local_model(h, data.edge_index, edge_attr, plan))
            h_local = self._normed("norm1_local", h_local, graph_ptr, residual=h)
        if self.self_attn is not None:
            if self.global_model_type == "BiasedTransformer":
                spd = data["attn_bias"] if "attn_bias" in data else None
                if spd is None:
                    raise ValueError("GPSLayer: global_model_type 'BiasedTransformer' needs the batch's attn_bias (the graphs' "
                                     "shortest-path distances): set it with spd.add_spd(batch) or spd.SPDTable(store).attach(batch, ids)")
                h_attn = self.self_attn(h, graph_ptr, max_nodes, spd=spd, bias_table=self.bias_table())
            else:
                h_attn = self.self_attn(h, graph_ptr, max_nodes)
            h_attn = self.dropout_attn(h_attn)
            h = h_local + self._normed("norm1_attn", h_attn, graph_ptr, residual=h)
        else:
            h = h_local
        ff = self.ff_dropout1(self.act_fn_ff(self.ff_linear1(h)))
        return self._normed("norm2", self.ff_dropout2(self.ff_linear2(ff)), graph_ptr, residual=h), edge_attr


class _TypeDict(torch.nn.Module):
    """TypeDictNodeEncoder / TypeDictEdgeEncoder (graphgps/encoder/type_dict_encoder.py:81-116): one embedding table"""

    def __init__(self, num_types, emb_dim):
        super().__init__()
        self.encoder = Embedding(num_types, emb_dim)

    def forward(self, index):
        return self.encoder(index)


class _ConcatPE(torch.nn.Module):
    """Concat2NodeEncoder / Concat3NodeEncoder (graphgps/encoder/composed_encoders.py:35-82) for TypeDictNode+LapPE,
    TypeDictNode+RWSE and TypeDictNode+LapPE+RWSE: encoder1 = the type embedding at the width the encodings leave, then
    encoder2 (and encoder3) = the positional encoders (expand_x False) in the reference's order, all concatenated.
    `pes`: [(name, dim_pe, constructor)] - constructed after encoder1 and in order, so equal seeds give equal weights."""

    def __init__(self, num_types, dim_emb, pes):
        super().__init__()
        left = dim_emb - sum(dim_pe for _, dim_pe, _ in pes)
        if left <= 0 or any(dim_pe <= 0 for _, dim_pe, _ in pes):
            raise ValueError("%s size %s is too large for desired embedding size of %d."
                             % ("+".join(name for name, _, _ in pes), "+".join(str(dim_pe) for _, dim_pe, _ in pes), dim_emb))
        self.encoder1 = _TypeDict(num_types, left)
        for k, (_, _, make) in enumerate(pes):
            setattr(self, "encoder%d" % (k + 2), make())
        self.count = len(pes)

    def forward(self, index, data):
        return torch.cat([self.encoder1(index)] + [getattr(self, "encoder%d" % (k + 2))(data) for k in range(self.count)], 1)


class FeatureEncoder(torch.nn.Module):
    """gps_model.py:12-51 with node_encoder TypeDictNode (lap_pe: TypeDictNode+LapPE, rwse: TypeDictNode+RWSE, both:
    TypeDictNode+LapPE+RWSE), edge_encoder TypeDictEdge and no encoder BatchNorm"""

    def __init__(self, dim_inner, node_types, edge_types, lap_pe=False, dim_pe=8, max_freqs=8, rwse=None):
        super().__init__()
        pes = []
        if lap_pe:
            pes.append(("LapPE", dim_pe, lambda: LapPENodeEncoder(dim_pe, max_freqs)))
        if rwse:
            pes.append(("RWSE", rwse["dim_pe"], lambda: RWSENodeEncoder(**rwse)))
        self.node_encoder = _ConcatPE(node_types, dim_inner, pes) if pes else _TypeDict(node_types, dim_inner)
        self.edge_encoder = _TypeDict(edge_types, dim_inner)


class SANGraphHead(torch.nn.Module):
    """graphgps/head/san_graph.py: pooling, then Linear(H, H/2), ReLU, Linear(H/2, H/4), ReLU, Linear(H/4, dim_out)"""

    def __init__(self, dim_in, dim_out, L=2):
        super().__init__()
        self.FC_layers = ModuleList([Linear(dim_in // 2 ** l, dim_in // 2 ** (l + 1)) for l in range(L)]
                                    + [Linear(dim_in // 2 ** L, dim_out)])
        self.L = L
        self.activation = ReLU()

    def forward(self, h, batch, num_graphs):
        g = global_add_pool(h, batch, num_graphs)
        for l in range(self.L):
            g = self.activation(self.FC_layers[l](g))
        return self.FC_layers[self.L](g)


class GPSModel(torch.nn.Module):
    """gps_model.py:54-108 under zinc-GPS.yaml; defaults = that file's values.  forward(data) -> [G, dim_out] predictions.
    The largest graph of the batch is read off `data._esc_max_nodes` when the loader left it there (the device store knows it
    on the host); otherwise the attention op reads it back once per batch.  lap_pe=True: the batch must carry EigVals / EigVecs
    (lappe.add_lap_pe, lappe.LapPETable.attach).  rwse=True: the node encoder gains nn.RWSENodeEncoder(rwse_dim_pe, rwse_steps,
    rwse_model, rwse_layers, rwse_raw_norm) as its last part and the batch must carry pestat_RWSE [N, rwse_steps]
    (rwse.add_rwse, rwse.RWSETable.attach); the rwse_* defaults are upstream GraphGPS's usual ZINC values - the reference ships
    no configuration that enables RWSE.  layer_norm / batch_norm: gt.layer_norm / gt.batch_norm, handed to every GPSLayer."""

    def __init__(self, layers=10, dim_hidden=64, n_heads=4, dropout=0.0, attn_dropout=0.5, node_types=28, edge_types=4, dim_out=1,
                 lap_pe=False, dim_pe=8, max_freqs=8, rwse=False, rwse_dim_pe=28, rwse_steps=20, rwse_model="linear", rwse_layers=1,
                 rwse_raw_norm="batchnorm", local_gnn_type="GINE", global_model_type="Transformer", layer_norm=False, batch_norm=True):
        super().__init__()
        if layer_norm and batch_norm:
            raise ValueError("Cannot apply two types of normalization together")
        self.lap_pe, self.rwse = bool(lap_pe), bool(rwse)
        rw = dict(dim_pe=rwse_dim_pe, num_steps=rwse_steps, model=rwse_model, layers=rwse_layers, raw_norm=rwse_raw_norm) if self.rwse else None
        self.encoder = FeatureEncoder(dim_hidden, node_types, edge_types, self.lap_pe, dim_pe, max_freqs, rw)
        self.layers = Sequential(*[GPSLayer(dim_hidden, n_heads, dropout, attn_dropout, local_gnn_type, global_model_type, layer_norm, batch_norm)
                                   for _ in range(layers)])
        self.has_attention = global_model_type != "None"
        self.post_mp = SANGraphHead(dim_hidden, dim_out)

    def forward(self, data):
        data.to(self.post_mp.FC_layers[0].weight.device)
        plan = plan_of(data, Z_TABLE_ROWS)
        graph_ptr, num_graphs = graph_ptr_of(data, plan)
        max_nodes = getattr(data, "_esc_max_nodes", None) if self.has_attention else None
        types = data.x.view(data.x.size(0), -1)[:, 0]                                 # type_dict_encoder.py:96: the first column
        h = self.encoder.node_encoder(types, data) if (self.lap_pe or self.rwse) else self.encoder.node_encoder(types)
        edge_attr = self.encoder.edge_encoder(data.edge_attr.view(-1))
        for layer in self.layers:
            h, edge_attr = layer(h, edge_attr, data, plan, graph_ptr, max_nodes)
        return self.post_mp(h, data.batch, num_graphs)
