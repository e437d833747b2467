"""GINE+ multi-hop convolutions — the MI355X twin of the aggregate primitive of
/root/reference/modules/gine_operations.py:306-362 (NAIVEGINEPLUS, GINEPLUS):

    result = (1 + eps[0]) * x_0 + sum_{d=1..k} (1 + eps[d]) * sum_{edges with distance d} relu(x_j (+ e if d == 1))

Given a plain pair of tensors, each per-distance neighbour sum runs through the HIP segmented gather-reduce
(csrc/aggregate.hip, no self term, optional edge term).  Given the tensors of a device-side expansion
(esc_gnn_amd.multihop, csrc/multihop.hip: they carry a MultihopPlan) and k <= 4, the whole aggregate is one launch per
direction (ops.gineplus_aggregate, csrc/gineplus.hip); k > 4 takes the per-distance path.

The network around the conv is the reference's (:23-253): MLP, OGBMolEmbedding, NodeEmbedding, VNAgg, ConvBlock, GlobalPool,
ClassifierNetwork and `new`, same constructor arguments, module nesting and state_dict keys, for conv_type 'gin+' and
'naivegin+' on plain graphs (`nested=True` and the 'gin' / 'gcn' convs are out of scope)."""
from copy import copy

import torch
import torch.nn.functional as F
from torch import nn

from .. import multihop, ops
from ..multihop import make_multihop_edges
from ..nn import AbsorbedReLU, BatchNorm1d, Embedding, Linear
from ..ogb_mol_gnn import AtomEncoder, BondEncoder
from ..plan import BatchPlan


def _plans(multihop_edge_index, distance, k, num_nodes):
    """One execution plan per distance class (esc_plan_csr, csrc/plan.hip).  They depend on the batch only, while every
    GINE+ layer of the model asks for them: cached on the edge tensor, keyed on the identity (address, shape, in-place
    version) of both inputs, so that L layers x forward/backward build them once per batch."""
    from ..plan import _sig
    key = (_sig(multihop_edge_index), _sig(distance), int(k), int(num_nodes))
    cached = getattr(multihop_edge_index, "_esc_gineplus_plans", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    out = []
    for d in range(1, k + 1):
        ei = multihop_edge_index[:, distance == d]
        out.append(BatchPlan.from_tensors(ei, num_nodes))
    multihop_edge_index._esc_gineplus_plans = (key, out)
    return out


class NAIVEGINEPLUS(nn.Module):
    def __init__(self, fun, dim, k=4, **kwargs):
        super().__init__()
        self.k = k
        self.nn = fun
        self.eps = nn.Parameter(torch.zeros(k + 1, dim), requires_grad=True)

    def forward(self, x, multihop_edge_index, distance, edge_attr):
        assert x.size(-1) == edge_attr.size(-1)
        mh = multihop.plan_of(multihop_edge_index, distance, x.size(0), self.k)
        if mh is not None and self.k <= multihop.FUSED_K_MAX:
            return self.nn(ops.gineplus_aggregate([x] * self.k, edge_attr, self.eps, mh))
        plans = _plans(multihop_edge_index, distance, self.k, x.size(0))
        result = (1 + self.eps[0]) * x
        for i in range(self.k):
            out = ops.neighbour_sum(x, edge_attr if i == 0 else None, plans[i])
            result = result + (1 + self.eps[i + 1]) * out
        return self.nn(result)

    def __repr__(self):
        return "{}(nn={}, k={})".format(self.__class__.__name__, self.nn, self.eps.size(0))


class GINEPLUS(nn.Module):
    def __init__(self, fun, dim, k=4, **kwargs):
        super().__init__()
        self.k = k
        self.nn = fun
        self.eps = nn.Parameter(torch.zeros(k + 1, dim), requires_grad=True)

    def forward(self, XX, multihop_edge_index, distance, edge_attr):
        """XX is the list of previous xs, XX[0] being the last layer's (reference :343)."""
        assert len(XX) >= self.k
        assert XX[-1].size(-1) == edge_attr.size(-1)
        mh = multihop.plan_of(multihop_edge_index, distance, XX[0].size(0), self.k)
        if mh is not None and self.k <= multihop.FUSED_K_MAX:
            return [self.nn(ops.gineplus_aggregate(XX[:self.k], edge_attr, self.eps, mh))] + XX
        plans = _plans(multihop_edge_index, distance, self.k, XX[0].size(0))
        result = (1 + self.eps[0]) * XX[0]
        for i, x in enumerate(XX):
            if i >= self.k:
                break
            out = ops.neighbour_sum(x, edge_attr if i == 0 else None, plans[i])
            result = result + (1 + self.eps[i + 1]) * out
        return [self.nn(result)] + XX


def new(data):
    """a new Data holding the same tensors (reference :365-374): fields may be re-assigned without touching the original"""
    out = copy(data)
    object.__setattr__(out, "_store", dict(object.__getattribute__(data, "_store")))
    return out


class MLP(nn.Module):
    def __init__(self, in_dim, out_dim):
        super().__init__()
        self.main = nn.Sequential(Linear(in_dim, 2 * in_dim), BatchNorm1d(2 * in_dim, fuse_relu=True), AbsorbedReLU(),
                                  Linear(2 * in_dim, out_dim))

    def forward(self, x):
        return self.main(x)


class OGBMolEmbedding(nn.Module):
    def __init__(self, dim, embed_edge=True, x_as_list=False):
        super().__init__()
        self.atom_embedding = AtomEncoder(emb_dim=dim)
        if embed_edge:
            self.edge_embedding = BondEncoder(emb_dim=dim)
        self.x_as_list = x_as_list

    def forward(self, data):
        data = new(data)
        data.x = self.atom_embedding(data.x)
        if self.x_as_list:
            data.x = [data.x]
        if hasattr(self, "edge_embedding"):
            data.edge_attr = self.edge_embedding(data.edge_attr)
        return data


class NodeEmbedding(nn.Module):
    def __init__(self, in_dim, out_dim, x_as_list=False):
        super().__init__()
        self.embedding = Embedding(num_embeddings=in_dim, embedding_dim=out_dim)
        self.x_as_list = x_as_list

    def forward(self, data):
        data = new(data)
        data.x = self.embedding(data.x)
        if self.x_as_list:
            data.x = [data.x]
        return data


def _conv_family(conv_type):
    """'gin+' and 'naivegin+' run; the reference's 'gin' (PyG GINEConv) and 'gcn' (GCNConv) blocks are not built here"""
    if conv_type in ("gin+", "naivegin+"):
        return
    if conv_type in ("gin", "gcn"):
        raise NotImplementedError("conv_type %r of the GINE+ network is not on the HIP path: use 'gin+' or 'naivegin+'" % conv_type)
    raise NotImplementedError("Unrecognised model conv : {}".format(conv_type))


class VNAgg(nn.Module):
    def __init__(self, dim, conv_type="gin"):
        super().__init__()
        self.conv_type = conv_type
        if "gin" not in conv_type:
            _conv_family(conv_type)
        self.mlp = nn.Sequential(MLP(dim, dim), BatchNorm1d(dim, fuse_relu=True), AbsorbedReLU())

    def forward(self, virtual_node, embeddings, batch_vector):
        if batch_vector.size(0) > 0:
            G = ops.segment_pool(embeddings, batch_vector, virtual_node.size(0), mean=False)
        else:
            G = torch.zeros_like(virtual_node)
        return self.mlp(virtual_node + G)


class ConvBlock(nn.Module):
    def __init__(self, dim, dropout=0.5, activation=F.relu, virtual_node=False, virtual_node_agg=True,
                 k=4, last_layer=False, conv_type="gin", edge_embedding=None):
        super().__init__()
        _conv_family(conv_type)
        self.edge_embed = edge_embedding
        self.conv_type = conv_type
        if conv_type == "gin+":
            self.conv = GINEPLUS(MLP(dim, dim), dim, k=k)
        else:
            self.conv = NAIVEGINEPLUS(MLP(dim, dim), dim, k=k)
        if activation is not None and activation is not F.relu:
            raise NotImplementedError("ConvBlock: only the default relu activation (fused into the BatchNorm) or None")
        self.last_layer = last_layer
        self.norm = BatchNorm1d(dim, fuse_relu=(activation is not None and not last_layer))     # reference :154-156
        self.act = activation or nn.Identity()
        self.dropout_ratio = dropout
        self.virtual_node = virtual_node
        self.virtual_node_agg = virtual_node_agg
        if self.virtual_node and self.virtual_node_agg:
            self.vn_aggregator = VNAgg(dim, conv_type=conv_type)

    def forward(self, data):
        data = new(data)
        x, ea, b = data.x, data.edge_attr, data.batch
        mhei, d = data.multihop_edge_index, data.distance
        h = x
        if self.virtual_node:
            vn_rows = ops.segment_broadcast(data.virtual_node, b, data.virtual_node.size(0))      # virtual_node[b]
            if self.conv_type == "gin+":
                h[0] = h[0] + vn_rows                        # entry 0 of the SHARED list: later layers read the sum (:139-141)
            else:
                h = h + vn_rows
        H = self.conv(h, mhei, d, self.edge_embed(ea))
        h = H[0] if self.conv_type == "gin+" else H
        h = self.norm(h)                                     # + ReLU unless this is the last block
        h = F.dropout(h, self.dropout_ratio, training=self.training)
        if self.virtual_node and self.virtual_node_agg:
            v = self.vn_aggregator(data.virtual_node, h, b)
            data.virtual_node = F.dropout(v, self.dropout_ratio, training=self.training)
        if self.conv_type == "gin+":
            H[0] = h
            h = H
        data.x = h
        return data


class GlobalPool(nn.Module):
    def __init__(self, fun, cat_size=False, cat_candidates=False, subgraph_to_graph="False"):
        super().__init__()
        if fun.lower() not in ("add", "mean"):
            raise NotImplementedError("GlobalPool: %r has no HIP kernel here (add / mean)" % fun)
        if cat_candidates:
            raise NotImplementedError("GlobalPool: cat_candidates is not on the HIP path")
        self.cat_size = cat_size
        self.mean = fun.lower() == "mean"
        self.cat_candidates = cat_candidates
        self.subgraph_to_graph = subgraph_to_graph

    def forward(self, batch):
        if self.subgraph_to_graph:
            raise NotImplementedError("GlobalPool over subgraph_to_graph: GINE+ on rooted subgraphs (nested) is out of scope")
        x, b = batch.x, batch.batch
        pooled = ops.segment_pool(x, b, _num_graphs(batch), mean=self.mean)
        if self.cat_size:
            sizes = ops.segment_pool(torch.ones(x.size(0), 1).type_as(x), b, _num_graphs(batch), mean=False)
            pooled = torch.cat([pooled, sizes], dim=1)
        return pooled


def _num_graphs(data):
    ng = object.__getattribute__(data, "__dict__").get("_num_graphs")        # the collate knows it on the host
    if ng is not None:
        return int(ng)
    ng = data["num_graphs"]
    return int(ng) if ng is not None else int(data.batch[-1].item()) + 1


class ClassifierNetwork(nn.Module):
    def __init__(self, hidden=100, out_dim=128, layers=3, dropout=0.5, virtual_node=False,
                 k=4, conv_type="gin", nested=False, subgraph_pooling="mean"):
        super().__init__()
        if nested:
            raise NotImplementedError("nested=True: GINE+ on rooted subgraphs is out of scope")
        _conv_family(conv_type)
        self.k = k
        self.conv_type = conv_type
        convs = [ConvBlock(hidden, dropout=dropout, virtual_node=virtual_node, k=min(i + 1, k), conv_type=conv_type,
                           edge_embedding=BondEncoder(emb_dim=hidden)) for i in range(layers - 1)]
        convs.append(ConvBlock(hidden, dropout=dropout, virtual_node=virtual_node,
                               virtual_node_agg=False,      # on the last layer, use but do not update the virtual node
                               last_layer=True, k=min(layers, k), conv_type=conv_type,
                               edge_embedding=BondEncoder(emb_dim=hidden)))
        self.main = nn.Sequential(OGBMolEmbedding(hidden, embed_edge=False, x_as_list=(conv_type == "gin+")), *convs)
        self.aggregate = nn.Sequential(GlobalPool("mean", subgraph_to_graph=nested), Linear(hidden, out_dim))
        self.virtual_node = virtual_node
        if self.virtual_node:
            self.v0 = nn.Parameter(torch.zeros(1, hidden), requires_grad=True)
        self.subgraph_pooling = subgraph_pooling

    def forward(self, data):
        if "node_to_subgraph" in data:
            raise NotImplementedError("data with node_to_subgraph: GINE+ on rooted subgraphs (nested) is out of scope")
        mei = data["multihop_edge_index"]
        if mei is None or data["distance"] is None or multihop.plan_of(mei, data["distance"], data.batch.numel(), self.k) is None:
            data = make_multihop_edges(data, self.k)         # (the store's expand has done this without a read-back)
        else:
            data = new(data)
        ng = _num_graphs(data)
        if self.virtual_node:
            data.virtual_node = self.v0.expand(ng, self.v0.shape[-1])
        g = self.main(data)
        if self.conv_type == "gin+":
            g.x = g.x[0]
        return self.aggregate(g)
