"""Writes the I2GNN fixtures under tests/golden/ (data only) from the reference checkout.

The reference's utils_edge_I2.py (create_subgraphs2 / subgraph_to_subgraph2_with_idx / find_all_spd / compute_rd) and
batch_I2.py are imported in place under oracle/pyg_shim.  Every graph gets x = arange(n), so the `x` of the reference's output
reveals the original node ids; each subgraph2 is then put into the canonical order of this project (root, then ascending
(hop, node id)) and its edges and centre rows relabelled.  The order of the copies is already the order of the sub-edges
that leave the root.

* subgraphs_i2gnn.npz — the cases of make_golden_ngnn.cases() plus a root whose only edges are self loops and a directed
  graph whose second-root distances exceed h; per case the inputs (n, edge_index, h) and every integer field, plus rd in fp32.
* collate_i2gnn3.npz — three synthetic ZINC molecules through create_subgraphs2(h=3, 'spd', use_rd, center_idx=True) and
  batch_I2's Batch.from_data_list, canonicalised.
* model_i2gnn.npz — the reference's I2GNN class body (zinc_cycle_models.py), extracted with ast and exec'd on the oracle
  primitives, 2 layers, seeded and perturbed, training mode, on collate_i2gnn3 with L1 loss on per-node cycle counts
  (tests/zinc_cycle_oracle.py); the three configurations of tests/i2gnn_oracle.CONFIGS.  Recorded: keys, shapes,
  predictions, loss and a (sum, abs-sum) digest per gradient.

Nothing is written that tests/i2gnn_oracle.py does not reproduce (integers and rd bit for bit, the model bit for bit).

    python tools/make_golden_i2gnn.py /path/to/reference
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
LAYERS, SEED = 2, 709
H_COLLATE, TARGET = 3, 3                     # column 3: the 6-cycles, which the synthetic molecules have


def _imports(ref_dir):
    sys.path[:0] = [os.path.join(ROOT, "oracle", "pyg_shim"), ref_dir, ROOT, os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
    import utils_edge_I2 as ref_utils                # the reference, imported in place
    from batch_I2 import Batch as RefBatch
    from torch_geometric.data import Data as ShimData
    return ref_utils, RefBatch, ShimData


def cases():
    """(name, n, edge_index [2, E], h): NGNN's cases and two of this expansion's own"""
    import make_golden_ngnn
    out = list(make_golden_ngnn.cases())
    # node 0 has self loops only (twice: two copies whose neighbour is the root itself); nodes 1-2 form an edge beside it
    out.append(("selfloops_only_h2", 3, np.array([[0, 0, 1, 2], [0, 0, 2, 1]], dtype=np.int64), 2))
    # a directed ring 0 -> 1 -> ... -> 5 -> 0 with a tail 6 -> 5: walking target -> source from the neighbour of a root goes the
    # long way round, so the distances to the second root exceed those to the first
    ring = [(i, (i + 1) % 6) for i in range(6)] + [(6, 5)]
    out.append(("directed_ring_h5", 7, np.array([[a for a, b in ring], [b for a, b in ring]], dtype=np.int64), 5))
    return out


FIELDS = ("orig_node", "z", "node_to_subgraph2", "subgraph2_to_subgraph", "center_idx", "edge_index", "orig_edge")


def canonical(ref_out, ids=None):
    """create_subgraphs2's output (x = original ids unless given) -> canonical order; returns the dict of arrays"""
    x = (ref_out.x if ids is None else ids).numpy().reshape(-1).astype(np.int64)
    z = ref_out.z.numpy().astype(np.int64)
    n2s2 = ref_out.node_to_subgraph2.numpy().astype(np.int64)
    ci = ref_out.center_idx.numpy().astype(np.int64)
    Ns = x.shape[0]
    is_root = np.zeros(Ns, dtype=bool)
    is_root[ci[:, 0]] = True
    order = np.lexsort((x, z[:, 0], ~is_root, n2s2))          # by subgraph2, root first, then (hop, id)
    inv = np.empty(Ns, dtype=np.int64)
    inv[order] = np.arange(Ns)
    res = dict(order=order, orig_node=x[order], z=z[order], node_to_subgraph2=n2s2[order],
               subgraph2_to_subgraph=ref_out.subgraph2_to_subgraph.numpy().astype(np.int64), center_idx=inv[ci],
               edge_index=inv[ref_out.edge_index.numpy()].astype(np.int64))
    assert np.array_equal(ref_out.node_to_original_node.numpy()[order], res["orig_node"])
    if "rd" in ref_out:
        res["rd"] = ref_out.rd.numpy()[order].astype(np.float32)
    return res


def run_reference(ref_utils, ShimData, n, ei, h, use_rd, edge_attr=None, x=None, y=None):
    E = ei.shape[1]
    d = ShimData(x=torch.arange(n) if x is None else x, edge_index=torch.tensor(ei),
                 edge_attr=torch.arange(E) if edge_attr is None else edge_attr, y=y)
    d.num_nodes = n
    return ref_utils.create_subgraphs2(d, h, node_label="spd", use_rd=use_rd, center_idx=True, self_loop=False)


def _same(name, got, want, keys):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(got["rd"].view(np.int32), want["rd"].view(np.int32)), (name, "rd", float(np.abs(got["rd"] - want["rd"]).max()))


def write_subgraphs(ref_utils, ShimData):
    import i2gnn_oracle as io
    store, names = {}, []
    for name, n, ei, h in cases():
        o = run_reference(ref_utils, ShimData, n, ei, h, True)
        c = canonical(o)
        got = {k: c[k] for k in FIELDS if k != "orig_edge"}
        got["rd"] = c["rd"]
        got["orig_edge"] = o.edge_attr.numpy().astype(np.int64)              # edge_attr = arange(E): the original edge ids
        _same(name, got, io.expand_graph2(n, ei[0], ei[1], h, use_rd=True), FIELDS)
        names.append(name)
        store[name + "/meta"] = np.array([n, h], dtype=np.int64)
        store[name + "/in_edge_index"] = ei
        for k, v in got.items():
            store[name + "/" + k] = v
    store["names"] = np.array(names)
    path = os.path.join(OUT, "subgraphs_i2gnn.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", len(names), "cases")


def write_collate(ref_utils, RefBatch, ShimData):
    import i2gnn_oracle as io
    from esc_gnn_amd.datasets import synthetic_zinc_graphs
    from zinc_cycle_oracle import cycle_labels
    store, datas, ids, raws = {}, [], [], synthetic_zinc_graphs(0, 3)
    for j, d in enumerate(raws):
        n, ei = int(d.num_nodes), d.edge_index.numpy()
        y = torch.tensor(cycle_labels(n, ei))                                # [n, 4] per-node cycle counts
        for k in ("x", "edge_index", "edge_attr"):
            store["raw%d_%s" % (j, k)] = d[k].numpy()
        store["raw%d_y" % j] = y.numpy()
        datas.append(run_reference(ref_utils, ShimData, n, ei, H_COLLATE, True, edge_attr=d.edge_attr, x=d.x, y=y))
        same = run_reference(ref_utils, ShimData, n, ei, H_COLLATE, True)    # the same graph with x = ids
        assert torch.equal(same.z, datas[-1].z) and torch.equal(same.edge_index, datas[-1].edge_index)
        ids.append(same.x.clone())
    b = RefBatch.from_data_list(datas)
    node_off = np.cumsum([0] + [int(d.num_nodes) for d in raws])
    gids = torch.cat([i + int(node_off[g]) for g, i in enumerate(ids)])
    c = canonical(b, gids)
    order = c["order"]
    out = dict(x=b.x.numpy()[order], z=c["z"], rd=c["rd"], node_to_subgraph2=c["node_to_subgraph2"],
               subgraph2_to_subgraph=c["subgraph2_to_subgraph"], center_idx=c["center_idx"], edge_index=c["edge_index"],
               edge_attr=b.edge_attr.numpy(), subgraph_to_graph=b.subgraph_to_graph.numpy(), batch=b.batch.numpy()[order],
               node_to_original_node=b.node_to_original_node.numpy()[order], y=b.y.numpy())
    want = io.expand_batch2([int(d.num_nodes) for d in raws], [d.edge_index.numpy() for d in raws], H_COLLATE, use_rd=True)
    x_all = np.concatenate([d.x.numpy() for d in raws])
    assert np.array_equal(out["x"], x_all[want["orig_node"]])
    assert np.array_equal(out["node_to_original_node"], want["orig_node"])
    assert np.array_equal(out["edge_attr"], np.concatenate([d.edge_attr.numpy() for d in raws])[want["orig_edge"]])
    _same("collate", out, want, ("z", "node_to_subgraph2", "subgraph2_to_subgraph", "center_idx", "edge_index", "batch",
                                 "subgraph_to_graph"))
    out["orig_node"], out["orig_edge"] = want["orig_node"], want["orig_edge"]
    for k, v in out.items():
        store["batch_" + k] = v
    store["num_graphs"], store["h"] = np.int64(3), np.int64(H_COLLATE)
    path = os.path.join(OUT, "collate_i2gnn3.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", len(order), "sub-nodes,", out["edge_index"].shape[1], "sub-edges,",
          len(out["subgraph2_to_subgraph"]), "subgraph2s")
    return out


def reference_i2gnn(ref_dir):
    import ngnn_oracle as no
    import ref_model as rm
    ref_file = os.path.join(ref_dir, "zinc_cycle_models.py")
    tree = ast.parse(open(ref_file).read())
    body = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name == "I2GNN") or
            (isinstance(n, ast.FunctionDef) and n.name == "center_pool")]
    ns = dict(torch=torch, F=F, np=np, GINConv=no.GINConv, global_mean_pool=rm.global_mean_pool, global_add_pool=rm.global_add_pool,
              Sequential=torch.nn.Sequential, Linear=torch.nn.Linear, ReLU=torch.nn.ReLU)
    exec(compile(ast.Module(body=body, type_ignores=[]), ref_file, "exec"), ns)
    return ns["I2GNN"]


def write_model(ref_dir, batch):
    from make_golden_model import Bag
    import i2gnn_oracle as io
    import ngnn_oracle as no
    torch.set_num_threads(1)
    b = {k: torch.tensor(v) for k, v in batch.items()}
    y = b["y"][:, TARGET].reshape(-1, 1).to(torch.float32)
    Ref = reference_i2gnn(ref_dir)
    out = {"layers": np.int64(LAYERS), "seed": np.int64(SEED), "target": np.int64(TARGET), "y": y.numpy()}
    for tag, kw in io.CONFIGS.items():
        torch.manual_seed(SEED)
        ref = no.perturb(Ref(None, num_layers=LAYERS, **kw))
        sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
        mine = io.i2gnn_from_recipe(SEED, LAYERS, tag)
        assert list(mine.state_dict().keys()) == list(sd0.keys()), tag
        for k, v in mine.state_dict().items():
            assert torch.equal(v, sd0[k]), (tag, k)
        res = []
        for m, call in ((ref, lambda m: m(Bag(batch=b["batch"], **{k: b[k] for k in (
                "x", "z", "rd", "edge_index", "edge_attr", "node_to_subgraph2", "subgraph2_to_subgraph", "subgraph_to_graph",
                "center_idx", "node_to_original_node")}))), (mine, lambda m: m(b))):
            m.train()
            pred = call(m)
            loss = F.l1_loss(pred, y)
            loss.backward()
            res.append((pred.detach(), loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), tag
        assert res[0][2].keys() == res[1][2].keys(), tag
        for k in res[0][2]:
            assert torch.equal(res[0][2][k], res[1][2][k]), (tag, k)
        out[tag + "/keys"] = np.array(list(sd0.keys()))
        out[tag + "/shapes"] = np.array(["x".join(map(str, v.shape)) or "scalar" for v in sd0.values()])
        out[tag + "/pred"], out[tag + "/loss"] = res[0][0].numpy(), res[0][1].numpy()
        for k, v in res[0][2].items():
            out[tag + "/gsum/" + k] = np.array([float(v.double().sum()), float(v.double().abs().sum())])
        print(tag, "loss", float(res[0][1]), "pred", tuple(res[0][0].shape))
    path = os.path.join(OUT, "model_i2gnn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    ref = sys.argv[1]
    ref_utils, RefBatch, ShimData = _imports(ref)
    write_subgraphs(ref_utils, ShimData)
    write_model(ref, write_collate(ref_utils, RefBatch, ShimData))
