"""Writes the QM9 fixtures under tests/golden/ (data only) from the reference checkout.

* qm9_distance.npz — inputs and outputs of the reference's `Distance` class (distance.py, imported in place) on a dozen small
  graphs: every flag combination (norm, squared, relative_pos, max_value, cat) and the graph of self loops only (0/0 = NaN).
* model_qm9.npz — as tools/make_golden_zinc_cycle.py does for zinc_cycle_models: the reference's qm9_models.NestedGIN_eff
  class body exec'd on the oracle primitives (oracle/make_golden_model.reference_class), 2 layers, seeded, training mode, on
  the `zinc3` collate batch with seeded x / pos / node_type and a 5-wide edge_attr (tests/qm9_oracle.qm9_batch_inputs), with
  F.mse_loss.  tests/qm9_oracle.NestedGINEffQm9Ref must reproduce it bit for bit.  Recorded: the inputs, the key list with
  shapes, the predictions, the loss and a (sum, abs-sum) digest of every gradient.
* collate_qm9_3.npz — three synthetic QM9 graphs (esc_gnn_amd.datasets.synthetic_qm9_graphs) feature-built by the
  reference's create_subgraphs(h=3, use_rd=True, self_loop=True), y = y[:, 0], the reference's Distance, and their
  Batch.from_data_list from the reference's batch.py (through oracle/pyg_shim, as oracle/make_golden.py does).

    python tools/make_golden_qm9.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
OUT = os.path.join(ROOT, "tests", "golden")
LAYERS, SEED, INPUT_SEED = 2, 913, 41


def _reference_distance(ref_dir):
    spec = importlib.util.spec_from_file_location("reference_distance", os.path.join(ref_dir, "distance.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Distance


class _Bag(object):
    """attribute bag standing in for a PyG Data inside the reference transform"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __contains__(self, key):
        return key in self.__dict__


def distance_cases():
    """(name, pos, edge_index, edge_attr or None, flags)"""
    rng = np.random.RandomState(7)
    cases = []

    def graph(n, m, loops=False, attr=4):
        s, t = rng.randint(0, n, size=m), rng.randint(0, n, size=m)
        if loops:
            t = s.copy()
        ea = None
        if attr:
            ea = np.zeros((m, attr), dtype=np.float32)
            ea[np.arange(m), rng.randint(0, attr, size=m)] = 1.0
        return rng.randn(n, 3).astype(np.float32) * 1.3, np.stack([s, t]).astype(np.int64), ea

    for i, flags in enumerate([dict(), dict(squared=True), dict(norm=False), dict(relative_pos=True),
                               dict(norm=False, squared=True), dict(squared=True, relative_pos=True),
                               dict(norm=False, relative_pos=True), dict(max_value=2.5), dict(cat=False),
                               dict(cat=False, relative_pos=True, squared=True), dict(max_value=0.5, squared=True)]):
        cases.append(("flags%d" % i,) + graph(5 + i, 9 + 3 * i) + (flags,))
    cases.append(("self_loops_only",) + graph(4, 4, loops=True) + (dict(),))
    cases.append(("no_attr",) + graph(6, 10, attr=0) + (dict(),))
    cases.append(("one_edge",) + graph(3, 1) + (dict(),))
    return cases


def write_distance(ref_dir):
    Distance = _reference_distance(ref_dir)
    out, names = {}, []
    for name, pos, ei, ea, flags in distance_cases():
        d = _Bag(pos=torch.tensor(pos), edge_index=torch.tensor(ei), edge_attr=None if ea is None else torch.tensor(ea))
        got = Distance(**flags)(d).edge_attr
        names.append(name)
        out[name + "/pos"], out[name + "/edge_index"], out[name + "/out"] = pos, ei, got.numpy()
        if ea is not None:
            out[name + "/edge_attr"] = ea
        full = dict(norm=True, max_value=None, cat=True, relative_pos=False, squared=False)
        full.update(flags)
        out[name + "/flags"] = np.array([float(full["norm"]), float(full["squared"]), float(full["relative_pos"]),
                                         float(full["cat"]), np.nan if full["max_value"] is None else full["max_value"]])
    out["names"] = np.array(names)
    path = os.path.join(OUT, "qm9_distance.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", len(names), "cases")


def write_model(ref_dir):
    from make_golden_model import Bag, reference_class
    import qm9_oracle as qo
    torch.set_num_threads(1)
    g = np.load(os.path.join(OUT, "collate_zinc3.npz"))
    b = {k[len("batch_"):]: torch.tensor(g[k]) for k in g.files if k.startswith("batch_")}
    G = int(b["batch"].max()) + 1
    b.update(qo.qm9_batch_inputs(b["x"].numel(), b["edge_index"].size(1), G, INPUT_SEED))

    class DS(object):
        num_features = qo.NUM_FEATURES
    torch.manual_seed(SEED)
    ref = qo.perturb(reference_class(os.path.join(ref_dir, "qm9_models.py"))(DS, LAYERS))
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    mine = qo.qm9_oracle_from_recipe(dict(seed=SEED, layers=LAYERS))
    assert list(mine.state_dict().keys()) == list(sd0.keys())
    for k, v in mine.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    res = []
    for m, call in ((ref, lambda m: m(Bag(x=b["x"], pos=b["pos"], node_type=b["node_type"], edge_index=b["edge_index"],
                                         edge_attr=b["edge_attr"], batch=b["batch"], pos_enc=b["pos_enc"],
                                         pos_index=b["pos_index"], pos_batch=b["pos_batch"]))),
                    (mine, lambda m: m(*qo.model_args(b)))):
        m.train()
        out = call(m)
        loss = F.mse_loss(out, b["y"])
        loss.backward()
        res.append((out.detach(), loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert res[0][0].shape == (G,)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    out = {"keys": np.array(list(sd0.keys())), "shapes": np.array(["x".join(map(str, v.shape)) or "scalar" for v in sd0.values()]),
           "pred": res[0][0].numpy(), "loss": res[0][1].numpy(), "layers": np.int64(LAYERS), "seed": np.int64(SEED),
           "input_seed": np.int64(INPUT_SEED)}
    for k in ("x", "pos", "node_type", "edge_attr", "y"):
        out["in/" + k] = b[k].numpy()
    for k, v in res[0][2].items():
        out["gsum/" + k] = np.array([float(v.double().sum()), float(v.double().abs().sum())])
    path = os.path.join(OUT, "model_qm9.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; loss", float(res[0][1]))


def write_collate(ref_dir):
    import make_golden as mg                              # the reference's feature build and batch.py under the shim
    from esc_gnn_amd.datasets import synthetic_qm9_graphs
    Distance = _reference_distance(ref_dir)
    datas, store = [], {}
    for j, d in enumerate(synthetic_qm9_graphs(0, 3)):
        s = mg.ShimData(x=d.x, edge_index=d.edge_index, edge_attr=d.edge_attr, y=d.y, pos=d.pos, name=d.name,
                        node_type=d.node_type)
        for k in ("x", "edge_index", "edge_attr", "y", "pos", "node_type"):
            store["raw%d_%s" % (j, k)] = d[k].numpy()
        o = mg.ref_feat.create_subgraphs(s, 3, node_label="hop", use_rd=True, subgraph_pretransform=None, self_loop=True)
        o.y = o.y[:, 0]
        o = Distance()(o)
        datas.append(o)
        for k in o.keys:
            store["g%d_%s" % (j, k)] = o[k].numpy() if torch.is_tensor(o[k]) else np.array(o[k])
    b = mg.RefBatch.from_data_list(datas)
    store["keys"] = np.array(sorted(b.keys))
    for k in b.keys:
        store["batch_" + k] = b[k].numpy() if torch.is_tensor(b[k]) else np.array(b[k])
    store["num_graphs"] = np.int64(b.num_graphs)
    path = os.path.join(OUT, "collate_qm9_3.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB;", sorted(b.keys))


if __name__ == "__main__":
    ref = sys.argv[1]
    write_distance(ref)
    write_model(ref)
    write_collate(ref)
