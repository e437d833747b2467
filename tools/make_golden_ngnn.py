"""Writes the NGNN fixtures under tests/golden/ (data only) from the reference checkout.

The reference's utils.py (create_subgraphs / k_hop_subgraph) and batch_I2.py are imported in place under oracle/pyg_shim.
Every graph gets x = arange(n), so the `x` of the reference's output reveals the original node ids; each subgraph is then
put into the canonical order of this project (root, then ascending (hop, node id)) and its edges relabelled.

* subgraphs_ngnn.npz — per case the inputs (n, edge_index, h) and the canonical orig_node, z (node_label 'spd' and
  'drnl'), node_to_subgraph, edge_index, orig_edge, plus rd in fp32.
* collate_ngnn3.npz — three synthetic ZINC molecules through create_subgraphs(h=3, 'spd', use_rd) and batch_I2's
  Batch.from_data_list, canonicalised: the batch offsets of batch_I2.py:61-66.
* model_ngnn.npz — the reference's NGNN class body (zinc_models.py), extracted with ast and exec'd on the oracle primitives
  (GINConv and global_mean_pool of tests/ngnn_oracle.py / oracle/ref_model.py), 2 layers, seeded and perturbed, training
  mode, on collate_ngnn3 with L1 loss; both subgraph_pooling modes, with and without use_rd.  Recorded: keys, shapes,
  predictions, loss and a (sum, abs-sum) digest per gradient.

Nothing is written that tests/ngnn_oracle.py does not reproduce (integers and rd bit for bit, the model bit for bit).

    python tools/make_golden_ngnn.py /path/to/reference
"""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
LAYERS, SEED = 2, 613
H_COLLATE = 3


def _imports(ref_dir):
    sys.path[:0] = [os.path.join(ROOT, "oracle", "pyg_shim"), ref_dir, ROOT, os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests")]
    import utils as ref_utils                        # the reference, imported in place
    from batch_I2 import Batch as RefBatch
    from torch_geometric.data import Data as ShimData
    return ref_utils, RefBatch, ShimData


def cases():
    """(name, n, edge_index [2, E], h)"""
    from esc_gnn_amd.datasets import synthetic_zinc_graphs
    rng = np.random.RandomState(11)
    out = []

    def sym(pairs):
        return np.array([[a for a, b in pairs] + [b for a, b in pairs], [b for a, b in pairs] + [a for a, b in pairs]], dtype=np.int64)
    out.append(("cycle4_h2", 4, sym([(0, 1), (1, 2), (2, 3), (3, 0)]), 2))
    out.append(("path6_h9", 6, sym([(i, i + 1) for i in range(5)]), 9))               # h above the diameter
    out.append(("k5_h1", 5, sym([(a, b) for a in range(5) for b in range(a + 1, 5)]), 1))
    out.append(("single_h1", 1, np.zeros((2, 0), dtype=np.int64), 1))
    out.append(("isolated_h2", 5, sym([(1, 3)]), 2))
    for h in (1, 2, 3):
        d = synthetic_zinc_graphs(20 + h, 1)[0]
        out.append(("mol_h%d" % h, int(d.num_nodes), d.edge_index.numpy().astype(np.int64), h))
    for i, (n, m) in enumerate([(7, 12), (12, 30), (20, 45)]):                        # directed: reach is asymmetric
        out.append(("directed%d_h%d" % (i, 1 + i), n, np.stack([rng.randint(0, n, m), rng.randint(0, n, m)]).astype(np.int64),
                    1 + i))
    ei = sym([(0, 1), (1, 2), (2, 0), (2, 3)])
    ei = np.concatenate([ei, np.array([[0, 2, 1, 1], [0, 2, 2, 2]], dtype=np.int64)], axis=1)   # self loops, a repeated edge
    out.append(("loops_repeats_h2", 4, ei, 2))
    n = 40
    out.append(("sparse40_h3", n, sym([(i, (i + 1) % n) for i in range(n)] + [(int(a), int(b)) for a, b in rng.randint(0, n, (12, 2)) if a != b]), 3))
    return out


def canonical(ref_out, h):
    """the reference's create_subgraphs output (x = original ids) -> canonical order; returns the dict of arrays"""
    x = ref_out.x.numpy().reshape(-1)
    z = ref_out.z.numpy()
    n2s = ref_out.node_to_subgraph.numpy()
    Ns = x.shape[0]
    hop = z[:, 0]
    is_root = np.zeros(Ns, dtype=bool)
    is_root[ref_out.node_id.numpy()] = True
    order = np.lexsort((x, hop, ~is_root, n2s))             # by subgraph, root first, then (hop, id)
    inv = np.empty(Ns, dtype=np.int64)
    inv[order] = np.arange(Ns)
    res = dict(order=order, orig_node=x[order].astype(np.int64), z=z[order].astype(np.int64), node_to_subgraph=n2s[order].astype(np.int64),
               edge_index=inv[ref_out.edge_index.numpy()].astype(np.int64))
    if "rd" in ref_out:
        res["rd"] = ref_out.rd.numpy().reshape(-1)[order].astype(np.float32)
    return res


def run_reference(ref_utils, ShimData, n, ei, h, node_label, use_rd, edge_attr=None, x=None, y=None):
    E = ei.shape[1]
    d = ShimData(x=torch.arange(n) if x is None else x, edge_index=torch.tensor(ei),
                 edge_attr=torch.arange(E) if edge_attr is None else edge_attr, y=y)
    d.num_nodes = n
    return ref_utils.create_subgraphs(d, h, node_label=node_label, use_rd=use_rd)


def check_against_oracle(name, got, n, ei, h):
    import ngnn_oracle as no
    want = no.expand_graph(n, ei[0], ei[1], h, use_rd=True)
    for k in ("orig_node", "node_to_subgraph", "edge_index", "orig_edge"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(got["z_spd"], no.labels(want["z"], want["paths"], h, "spd")), (name, "spd")
    assert np.array_equal(got["z_drnl"], no.labels(want["z"], want["paths"], h, "drnl")), (name, "drnl")
    assert np.array_equal(got["rd"].view(np.int32), want["rd"].view(np.int32)), (name, "rd", float(np.abs(got["rd"] - want["rd"]).max()))


def write_subgraphs(ref_utils, ShimData):
    store, names, unordered, total = {}, [], 0, 0
    for name, n, ei, h in cases():
        o = run_reference(ref_utils, ShimData, n, ei, h, "spd", True)
        c = canonical(o, h)
        total += n
        unordered += sum(1 for s in range(n) if not np.array_equal(o.x.numpy()[o.node_to_subgraph.numpy() == s],
                                                                   c["orig_node"][c["node_to_subgraph"] == s]))
        got = dict(orig_node=c["orig_node"], node_to_subgraph=c["node_to_subgraph"], edge_index=c["edge_index"], z_spd=c["z"],
                   rd=c["rd"], orig_edge=o.edge_attr.numpy().astype(np.int64))       # edge_attr = arange(E): the original edge ids
        d = run_reference(ref_utils, ShimData, n, ei, h, "drnl", False)          # same set operations: same raw order
        assert torch.equal(d.x, o.x) and torch.equal(d.edge_index, o.edge_index)
        got["z_drnl"] = d.z.numpy()[c["order"]].astype(np.int64)
        check_against_oracle(name, got, n, ei, h)
        names.append(name)
        store[name + "/meta"] = np.array([n, h], dtype=np.int64)
        store[name + "/in_edge_index"] = ei
        for k, v in got.items():
            store[name + "/" + k] = v
    store["names"] = np.array(names)
    path = os.path.join(OUT, "subgraphs_ngnn.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", len(names), "cases;", unordered, "of", total,
          "subgraphs are not in (hop, id) order in the reference")


def write_collate(ref_utils, RefBatch, ShimData):
    import ngnn_oracle as no
    from esc_gnn_amd.datasets import synthetic_zinc_graphs
    store, datas, raws = {}, [], synthetic_zinc_graphs(0, 3)
    for j, d in enumerate(raws):
        n, ei = int(d.num_nodes), d.edge_index.numpy()
        for k in ("x", "edge_index", "edge_attr", "y"):
            store["raw%d_%s" % (j, k)] = d[k].numpy()
        datas.append(run_reference(ref_utils, ShimData, n, ei, H_COLLATE, "spd", True, edge_attr=d.edge_attr, x=d.x, y=d.y))
        # the same graph with x = ids, to learn the canonical permutation
        ids = run_reference(ref_utils, ShimData, n, ei, H_COLLATE, "spd", True)
        assert torch.equal(ids.z, datas[-1].z) and torch.equal(ids.edge_index, datas[-1].edge_index)
        datas[-1]._ids = ids.x.clone()
    b = RefBatch.from_data_list(datas)
    # canonicalise the whole batch: sub-node order by (subgraph, root first, hop, original id)
    ids = torch.cat([d._ids for d in datas]).numpy()
    n2s, z = b.node_to_subgraph.numpy(), b.z.numpy()
    Ns = ids.shape[0]
    first = np.ones(Ns, dtype=bool)
    first[1:] = n2s[1:] != n2s[:-1]
    order = np.lexsort((ids, z[:, 0], ~first, n2s))
    inv = np.empty(Ns, dtype=np.int64)
    inv[order] = np.arange(Ns)
    out = dict(x=b.x.numpy()[order], z=z[order], rd=b.rd.numpy()[order].astype(np.float32), node_to_subgraph=n2s[order],
               edge_index=inv[b.edge_index.numpy()], edge_attr=b.edge_attr.numpy(), subgraph_to_graph=b.subgraph_to_graph.numpy(),
               batch=b.batch.numpy()[order], y=b.y.numpy())
    node_off = np.cumsum([0] + [int(d.num_nodes) for d in raws])
    want = no.expand_batch([int(d.num_nodes) for d in raws], [d.edge_index.numpy() for d in raws], H_COLLATE, use_rd=True)
    x_all = np.concatenate([d.x.numpy() for d in raws])
    assert np.array_equal(out["x"], x_all[want["orig_node"]])
    assert np.array_equal(out["z"], no.labels(want["z"], want["paths"], H_COLLATE, "spd"))
    for k in ("node_to_subgraph", "edge_index", "batch"):
        assert np.array_equal(out[k], want[k]), k
    assert np.array_equal(out["edge_attr"], np.concatenate([d.edge_attr.numpy() for d in raws])[want["orig_edge"]])
    assert np.array_equal(out["subgraph_to_graph"], np.repeat(np.arange(3), np.diff(node_off)))
    assert np.array_equal(out["rd"].reshape(-1).view(np.int32), want["rd"].view(np.int32))
    out["orig_node"], out["orig_edge"] = want["orig_node"], want["orig_edge"]
    for k, v in out.items():
        store["batch_" + k] = v
    store["num_graphs"], store["h"] = np.int64(3), np.int64(H_COLLATE)
    path = os.path.join(OUT, "collate_ngnn3.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", Ns, "sub-nodes,", out["edge_index"].shape[1], "sub-edges")
    return out


def reference_ngnn(ref_dir):
    import ngnn_oracle as no
    import ref_model as rm
    ref_file = os.path.join(ref_dir, "zinc_models.py")
    tree = ast.parse(open(ref_file).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "NGNN")
    ns = dict(torch=torch, F=F, np=np, GINConv=no.GINConv, global_mean_pool=rm.global_mean_pool)
    exec(compile(ast.Module(body=[node], type_ignores=[]), ref_file, "exec"), ns)
    return ns["NGNN"]


def write_model(ref_dir, batch):
    from make_golden_model import Bag
    import ngnn_oracle as no
    torch.set_num_threads(1)
    b = {k: torch.tensor(v) for k, v in batch.items()}
    y = b["y"].view(-1, 1)
    y = (y - y.mean()) / y.std()
    Ref = reference_ngnn(ref_dir)
    out = {"layers": np.int64(LAYERS), "seed": np.int64(SEED), "y": y.numpy()}
    for pooling in ("mean", "center"):
        for use_rd in (False, True):
            tag = "%s_%s" % (pooling, "rd" if use_rd else "nord")
            torch.manual_seed(SEED)
            ref = no.perturb(Ref(None, num_layers=LAYERS, subgraph_pooling=pooling, use_rd=use_rd))
            sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
            mine = no.ngnn_from_recipe(SEED, LAYERS, pooling, use_rd)
            assert list(mine.state_dict().keys()) == list(sd0.keys()), tag
            for k, v in mine.state_dict().items():
                assert torch.equal(v, sd0[k]), (tag, k)
            res = []
            for m, call in ((ref, lambda m: m(Bag(x=b["x"], z=b["z"], rd=b["rd"], edge_index=b["edge_index"],
                                                 edge_attr=b["edge_attr"], node_to_subgraph=b["node_to_subgraph"],
                                                 subgraph_to_graph=b["subgraph_to_graph"]))),
                            (mine, lambda m: m(*no.model_args(b)))):
                m.train()
                pred = call(m)
                loss = F.l1_loss(pred, y)
                loss.backward()
                res.append((pred.detach(), loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), tag
            for k in res[0][2]:
                assert torch.equal(res[0][2][k], res[1][2][k]), (tag, k)
            out[tag + "/keys"] = np.array(list(sd0.keys()))
            out[tag + "/shapes"] = np.array(["x".join(map(str, v.shape)) or "scalar" for v in sd0.values()])
            out[tag + "/pred"], out[tag + "/loss"] = res[0][0].numpy(), res[0][1].numpy()
            for k, v in res[0][2].items():
                out[tag + "/gsum/" + k] = np.array([float(v.double().sum()), float(v.double().abs().sum())])
            print(tag, "loss", float(res[0][1]))
    path = os.path.join(OUT, "model_ngnn.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    ref = sys.argv[1]
    ref_utils, RefBatch, ShimData = _imports(ref)
    write_subgraphs(ref_utils, ShimData)
    write_model(ref, write_collate(ref_utils, RefBatch, ShimData))
