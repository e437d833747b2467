"""Writes the GINE+ fixtures under tests/golden/ (data only) from the reference checkout.

The reference's modules/gine_operations.py is never imported (it needs torch_sparse, torch_geometric and ogb): its
`make_multihop_edges`, `new` and the class bodies :23-253, :306-362 are extracted with ast and exec'd over stand-ins that
restate what they rely on — a dense-matrix SparseTensor / matmul / coalesce(op='min'), a MessagePassing whose propagate() is the
PyG 2.0.4 add aggregation (oracle/make_golden_gineplus.py), index_add pools, and ogb's sum-of-embeddings encoders.

* multihop_edges.npz — tests/multihop_oracle.hand_cases() at their k values plus one collated batch of 3 stand-in molecules:
  inputs and the reference's (multihop_edge_index, distance).  The oracle's bounded BFS must reproduce every case bit for bit.
* model_gineplus_net.npz — the reference's ClassifierNetwork(hidden 32, k 3, 'gin+', dropout 0) for layers in {1, 2, 4} x
  virtual_node in {False, True} on a batch of 8 stand-in molecules, with the seed-free parameters of
  multihop_oracle.fill_params: state_dict keys and shapes, inputs, predictions in eval and in train mode, the loss, and a (sum,
  abs-sum) digest of every gradient and of every BatchNorm buffer after the training forward.  Why 8 molecules and not the 3 of
  the edge fixture: with a virtual node a BatchNorm normalises one row per graph, and over 3 rows, four blocks deep, the
  reference's own fp32 gradients are 4.5e-4 of scale away from its fp64 run - no fp32 implementation can be held to 1e-4 there.
  A batch is admitted when the reference's fp32 gradients lie within a third of that bound of its fp64 ones (asserted below; 8
  molecules: 2.4e-5).  The weights and the full gradients would be 1 MB: instead
  tests/multihop_oracle.RefNet must equal the reference's classes bit for bit here (predictions, every gradient, every buffer),
  and the tests compare the HIP model with RefNet element by element and RefNet with the digests.

    python tools/make_golden_multihop.py /path/to/reference
"""
import ast
import copy
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import multihop_oracle as mo  # noqa: E402


class SparseTensor(object):
    """dense stand-in: what make_multihop_edges uses of torch_sparse.SparseTensor"""

    def __init__(self, row=None, col=None, value=None, sparse_sizes=None, is_sorted=False, dense=None):
        if dense is None:
            dense = torch.zeros(sparse_sizes, dtype=torch.float64)
            dense.index_put_((row, col), value.double(), accumulate=True)     # repeated edges add up, as a COO matrix does
        self.dense = dense

    def coo(self):
        row, col = torch.nonzero(self.dense, as_tuple=True)                   # row-major: sorted by (row, col)
        return row, col, self.dense[row, col]


def matmul(a, b):
    return SparseTensor(dense=a.dense @ b.dense)


def coalesce(index, value, m, n, op="min"):
    assert op == "min"
    key = index[0] * n + index[1]
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    out = torch.full((uniq.numel(),), torch.iinfo(value.dtype).max, dtype=value.dtype)
    out = out.scatter_reduce(0, inv, value, reduce="amin")
    return torch.stack([uniq // n, uniq % n]), out


class MessagePassing(torch.nn.Module):
    def __init__(self, aggr="add", **kw):
        super().__init__()
        assert aggr == "add"

    def propagate(self, edge_index, x, edge_attr=None):
        x_j = x.index_select(0, edge_index[0])
        return torch.zeros_like(x).index_add_(0, edge_index[1], self.message(x_j, edge_attr))


class Bag(object):
    """attribute container with `in` and copy(): what the reference uses of torch_geometric.data.Data here"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __contains__(self, key):
        return key in self.__dict__

    @property
    def num_edges(self):
        return self.edge_index.size(1)


def reference_namespace(ref_dir):
    ref_file = os.path.join(ref_dir, "modules", "gine_operations.py")
    tree = ast.parse(open(ref_file).read())
    want = {"MLP", "OGBMolEmbedding", "NodeEmbedding", "VNAgg", "ConvBlock", "GlobalPool", "ClassifierNetwork", "NAIVEGINEPLUS",
            "GINEPLUS", "make_multihop_edges", "new"}
    body = [n for n in tree.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name in want]
    assert {n.name for n in body} == want
    nng = types.SimpleNamespace(MessagePassing=MessagePassing, global_add_pool=mo.global_add_pool,
                                global_mean_pool=mo.global_mean_pool)
    ns = dict(torch=torch, nn=torch.nn, F=F, nng=nng, np=np, copy=copy.copy, SparseTensor=SparseTensor, coalesce=coalesce,
              torch_sparse=types.SimpleNamespace(matmul=matmul), BondEncoder=mo.BondEncoder, AtomEncoder=mo.AtomEncoder,
              global_add_pool=mo.global_add_pool, global_mean_pool=mo.global_mean_pool)
    exec(compile(ast.Module(body=body, type_ignores=[]), ref_file, "exec"), ns)
    return ns


def collate(graphs):
    ns = [n for n, _ in graphs]
    off = np.cumsum([0] + ns)
    ei = np.concatenate([np.asarray(e).reshape(2, -1) + off[g] for g, (_, e) in enumerate(graphs)], axis=1)
    return int(off[-1]), ei


def reference_multihop(ns_ref, n, ei, k):
    d = Bag(x=torch.zeros(n, 1), edge_index=torch.tensor(ei), num_nodes=n)
    out = ns_ref["make_multihop_edges"](d, k)
    return out.multihop_edge_index.numpy().astype(np.int64), out.distance.numpy().astype(np.int64)


def molecules(count=3):
    from esc_gnn_amd.datasets import synthetic_ogbmol_graphs
    return synthetic_ogbmol_graphs(0, count, mo.OUT_DIM, 0.0)


def write_edges(ns_ref):
    store, names = {}, []
    for name, graphs, ks in mo.hand_cases():
        n, ei = collate(graphs)
        store[name + "/ns"] = np.array([g[0] for g in graphs], dtype=np.int64)
        store[name + "/es"] = np.array([np.asarray(g[1]).reshape(2, -1).shape[1] for g in graphs], dtype=np.int64)
        store[name + "/edge_index"] = ei
        store[name + "/ks"] = np.array(ks, dtype=np.int64)
        for k in ks:
            mei, dist = reference_multihop(ns_ref, n, ei, k)
            want = mo.multihop_batch([g[0] for g in graphs], [g[1] for g in graphs], k)
            assert np.array_equal(mei, want[0]) and np.array_equal(dist, want[1]), (name, k)
            store["%s/k%d/multihop_edge_index" % (name, k)] = mei
            store["%s/k%d/distance" % (name, k)] = dist
        names.append(name)
    # a batch without any edge: the reference returns empty tensors, no diagonal
    mei, dist = reference_multihop(ns_ref, 3, np.zeros((2, 0), dtype=np.int64), 2)
    assert mei.shape == (2, 0) and dist.shape == (0,)
    raws = molecules()
    graphs = [(int(d.num_nodes), d.edge_index.numpy()) for d in raws]
    n, ei = collate(graphs)
    for j, d in enumerate(raws):
        for key in ("x", "edge_index", "edge_attr", "y"):
            store["mol/raw%d_%s" % (j, key)] = d[key].numpy()
    mei, dist = reference_multihop(ns_ref, n, ei, mo.K)
    want = mo.multihop_batch([g[0] for g in graphs], [g[1] for g in graphs], mo.K)
    assert np.array_equal(mei, want[0]) and np.array_equal(dist, want[1])
    store["mol/k"] = np.int64(mo.K)
    store["mol/multihop_edge_index"], store["mol/distance"] = mei, dist
    store["names"] = np.array(names)
    path = os.path.join(OUT, "multihop_edges.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", len(names), "hand cases; molecule batch:", n, "nodes,", mei.shape[1], "pairs")


def run(model, call, w):
    res = {}
    model.eval()
    with torch.no_grad():
        res["eval"] = call(model).clone()
    model.train()
    model.zero_grad()
    pred = call(model)
    loss = (pred * w).sum()
    loss.backward()
    res["train"], res["loss"] = pred.detach().clone(), loss.detach().clone()
    res["grads"] = {k: p.grad.clone() for k, p in model.named_parameters()}
    res["buffers"] = {k: b.clone() for k, b in model.named_buffers()}
    return res


def write_model(ns_ref):
    torch.set_num_threads(1)
    raws = molecules(mo.NET_MOLECULES)
    mei, dist = mo.multihop_batch([int(d.num_nodes) for d in raws], [d.edge_index.numpy() for d in raws], mo.K)
    x = torch.cat([d.x for d in raws])
    ea = torch.cat([d.edge_attr for d in raws])
    ns = [int(d.num_nodes) for d in raws]
    batch = torch.tensor(np.repeat(np.arange(len(ns)), ns))
    off = np.cumsum([0] + ns)
    ei = torch.cat([d.edge_index + int(off[g]) for g, d in enumerate(raws)], dim=1)
    G = len(ns)
    w = mo.loss_weights(G, mo.OUT_DIM)
    tmei, tdist = torch.tensor(mei), torch.tensor(dist)
    out = {"hidden": np.int64(mo.HIDDEN), "out_dim": np.int64(mo.OUT_DIM), "k": np.int64(mo.K), "w": w.numpy()}
    for j, d in enumerate(raws):
        for key in ("x", "edge_index", "edge_attr", "y"):
            out["raw%d_%s" % (j, key)] = d[key].numpy()
    for layers, vn in mo.CONFIGS:
        tag = "L%d_vn%d" % (layers, int(vn))
        ref = ns_ref["ClassifierNetwork"](hidden=mo.HIDDEN, out_dim=mo.OUT_DIM, layers=layers, dropout=0.0, virtual_node=vn, k=mo.K,
                                          conv_type="gin+", nested=False)
        mine = mo.RefNet(mo.HIDDEN, mo.OUT_DIM, layers, vn, mo.K, "gin+")
        assert list(mine.state_dict().keys()) == list(ref.state_dict().keys()), tag
        mo.fill_params(ref)
        sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
        mo.fill_params(mine)
        for k, v in mine.state_dict().items():
            assert torch.equal(v, sd0[k]), (tag, k)

        def call_ref(m):
            return m(Bag(x=x, edge_index=ei, edge_attr=ea, batch=batch, num_nodes=x.size(0), num_graphs=G))

        def call_mine(m):
            return m(x, ea, batch, tmei, tdist, G)
        a, b = run(ref, call_ref, w), run(mine, call_mine, w)
        a64 = run(ref.double(), call_ref, w.double())                        # the reference's own fp32 error: admits the batch
        own = max(float((a["grads"][k].double() - a64["grads"][k]).abs().max()) / max(1.0, float(a64["grads"][k].abs().max()))
                  for k in a["grads"])
        assert own <= 1e-4 / 3, (tag, own)
        for key in ("eval", "train", "loss"):
            assert torch.equal(a[key], b[key]), (tag, key)
        for grp in ("grads", "buffers"):
            assert a[grp].keys() == b[grp].keys(), (tag, grp)
            for k in a[grp]:
                assert torch.equal(a[grp][k], b[grp][k]), (tag, grp, k)
        out[tag + "/keys"] = np.array(list(sd0.keys()))
        out[tag + "/shapes"] = np.array(["x".join(map(str, v.shape)) or "scalar" for v in sd0.values()])
        out[tag + "/eval"], out[tag + "/train"], out[tag + "/loss"] = a["eval"].numpy(), a["train"].numpy(), a["loss"].numpy()
        out[tag + "/gsum"] = np.stack([mo.digest(v) for v in a["grads"].values()])          # rows in named_parameters() order
        out[tag + "/bsum"] = np.stack([mo.digest(v) for v in a["buffers"].values()])        # rows in named_buffers() order
        print(tag, "loss", float(a["loss"]), "keys", len(sd0), "reference fp32 vs fp64 gradients: %.2g of scale" % own)
    path = os.path.join(OUT, "model_gineplus_net.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    ns_ref = reference_namespace(sys.argv[1])
    write_edges(ns_ref)
    write_model(ns_ref)
