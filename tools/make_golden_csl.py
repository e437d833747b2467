"""Writes tests/golden/model_csl.npz (data only) from the reference's CSL driver.

The reference's own create_subgraphs (utils_edge_efficient.py, imported in place under oracle/pyg_shim as
oracle/make_golden.py does) runs with h = 4, node_label='hop', use_rd=True, self_loop=True on the 20 fixture graphs of
tests/csl_oracle.fixture_graphs (every CSL class as its identity copy plus one RandomState(7) relabelling) and must equal
the oracle's feature build array for array; its batch.py collates them, and the `NestedGIN` class body that run_csl.py
defines inline is exec'd on the oracle primitives (oracle/ref_model.py) with torch's ELU / Embedding / F.elu and an `F`
whose dropout replays a recorded multiplier.  tests/csl_oracle.NestedGINCslRef must reproduce it bit for bit: the eval-mode
predictions, and one training step on all 20 graphs (output, cross-entropy loss, every parameter gradient).

Recorded: the seed recipe, the state_dict key list, per-graph digests of edge_index / pos_enc / pos_index / pos_batch, the
eval predictions in fp32 and fp64, err32 = max |pred32 - pred64|, the 20 x 20 fp64 distance matrix, the dropout multiplier,
the training output and loss, a digest (sum, abs-sum) of every gradient, the names of the parameters that receive none
(z_embedding.*: the reference's forward constructs that block but never applies it), and the driver's flag names and defaults parsed
from run_csl.py.

The expressiveness criterion (copies of one class coincide, different classes are apart) is only a meaningful fixture
when the fp32 error cannot blur it, so the margin is asserted before anything is written: with
tol = 3 * err32 + 1e-5 * max|pred64| and 10 output columns, min(cross-class dist64) / 2 > 2 * sqrt(10) * tol and
max(same-class dist64) < tol.  If a seed fails this, pick another one (SEED below) and say so in the commit.

    python tools/make_golden_csl.py /path/to/reference
"""
import ast
import copy
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS, HIDDEN, SEED, H, MASK_SEED = 3, 32, 1, 4, 20


def reference_nested_gin(ref_dir, drop_holder):
    """the inline NestedGIN of run_csl.py on the oracle primitives; F.dropout multiplies by drop_holder[0] when training"""
    import ref_model as rm
    path = os.path.join(ref_dir, "run_csl.py")
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "NestedGIN"][-1]

    def dropout(x, p=0.5, training=True):
        assert p == 0.5
        return x * drop_holder[0].to(x.dtype) if training else x

    Fm = types.SimpleNamespace(elu=F.elu, dropout=dropout)
    ns = dict(torch=torch, F=Fm, Linear=torch.nn.Linear, Sequential=torch.nn.Sequential, ELU=torch.nn.ELU,
              GINEConv=rm.GINEConv, global_add_pool=rm.global_add_pool)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["NestedGIN"]


def reference_flags(ref_dir):
    """{flag name: default} of the parser.add_argument calls of run_csl.py"""
    tree = ast.parse(open(os.path.join(ref_dir, "run_csl.py")).read())
    flags = {}
    for n in ast.walk(tree):
        if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == "add_argument":
            name = ast.literal_eval(n.args[0])
            default = [ast.literal_eval(k.value) for k in n.keywords if k.arg == "default"]
            flags[name.lstrip("-")] = default[0] if default else None
    return flags


def main(ref_dir):
    torch.set_num_threads(1)
    sys.path[:0] = [os.path.join(ROOT, "oracle", "pyg_shim"), ref_dir, os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests"), ROOT]
    import utils_edge_efficient as ref_feat            # the reference, imported in place
    from batch import Batch as RefBatch                 # the reference's batch.py
    from torch_geometric.data import Data as ShimData
    from make_golden_model import Bag
    import csl_oracle as co

    raw = co.fixture_graphs()
    graphs = [ref_feat.create_subgraphs(ShimData(x=d.x, edge_index=d.edge_index, edge_attr=None, y=d.y), H,
                                        node_label="hop", use_rd=True, subgraph_pretransform=None, self_loop=True)
              for d in raw]
    # the CPU restatement of the feature build gives the same tensors (the CPU test recomputes the digests with it)
    for a, b in zip(graphs, co.cpu_features(raw, H)):
        for k in co.FEATURE_KEYS:
            assert np.array_equal(a[k].numpy(), b[k].numpy()), k
    top = max(int(g["pos_index"].max()) for g in graphs)
    assert top < 1800, top
    print("features: %d edge rows, %d..%d bag entries per graph, largest table index %d" % (
        graphs[0]["edge_index"].size(1), min(g["pos_index"].numel() for g in graphs),
        max(g["pos_index"].numel() for g in graphs), top))
    b = RefBatch.from_data_list(graphs)
    bag = Bag(x=b.x, edge_index=b.edge_index, batch=b.batch, pos_enc=b.pos_enc, pos_index=b.pos_index,
              pos_batch=b.pos_batch, y=b.y)
    args = (b.x, b.edge_index, b.pos_enc, b.pos_index, b.pos_batch, b.batch)
    y = b.y.view(-1)
    assert y.dtype == torch.int64 and y.tolist() == [k for k in range(10) for _ in range(2)]
    recipe = dict(seed=SEED, layers=LAYERS, hidden=HIDDEN)
    out = {"seed": np.int64(SEED), "layers": np.int64(LAYERS), "hidden": np.int64(HIDDEN), "h": np.int64(H),
           "digests": co.graph_digests(graphs), "labels": y.numpy(),
           "flags_json": np.array(json.dumps(reference_flags(ref_dir), sort_keys=True))}

    # ---- eval-mode predictions of all 20 graphs, fp32 and fp64, and the separation margin ----
    drop = [None]
    torch.manual_seed(SEED)
    ref = reference_nested_gin(ref_dir, drop)(LAYERS, HIDDEN)
    ref.reset_parameters()
    ref.eval()
    mine = co.csl_oracle_from_recipe(recipe).eval()
    assert list(mine.state_dict().keys()) == list(ref.state_dict().keys())
    for k, v in ref.state_dict().items():
        assert torch.equal(v, mine.state_dict()[k]), k
    with torch.no_grad():
        p_ref, p32 = ref(bag), mine(*args)
        p64 = copy.deepcopy(mine).double()(b.x.double(), *args[1:])
    assert torch.equal(p_ref, p32), "the restatement differs from the reference class"
    err32 = float((p32.double() - p64).abs().max())
    tol = 3.0 * err32 + 1e-5 * float(p64.abs().max())
    cross, same = co.class_distances(p64)
    print("eval: max|pred64| %.4g, err32 %.4g, tol %.4g; min cross-class dist64 %.4g, max same-class dist64 %.4g; "
          "needs %.4g > %.4g and %.4g < %.4g" % (float(p64.abs().max()), err32, tol, cross, same, cross / 2,
                                                 2.0 * 10 ** 0.5 * tol, same, tol))
    assert cross / 2 > 2.0 * 10 ** 0.5 * tol and same < tol, "the margin does not hold for this seed: pick another one"
    out.update(keys=np.array(list(ref.state_dict().keys())), pred32=p32.numpy(), pred64=p64.numpy(),
               err32=np.float64(err32), dist64=co.distance_matrix(p64).numpy())

    # ---- one training step on the 20 graphs with a recorded dropout multiplier ----
    gen = torch.Generator().manual_seed(MASK_SEED)
    drop[0] = (torch.rand(len(graphs), HIDDEN, generator=gen) >= 0.5).float() * 2.0
    torch.manual_seed(SEED)
    ref = reference_nested_gin(ref_dir, drop)(LAYERS, HIDDEN)
    ref.reset_parameters()
    mine = co.csl_oracle_from_recipe(recipe)
    res = []
    for m, call in ((ref, lambda m: m(bag)), (mine, lambda m: m(*args, drop=drop[0]))):
        m.train()
        o = call(m)
        loss = F.cross_entropy(o, y)
        loss.backward()
        res.append((o.detach(), loss.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:                                 # z_embedding is never applied by the reference forward: no gradient
        assert (res[0][2][k] is None) == (res[1][2][k] is None) == k.startswith("z_embedding."), k
        assert res[0][2][k] is None or torch.equal(res[0][2][k], res[1][2][k]), k
    out.update(drop=drop[0].numpy(), train_out=res[0][0].numpy(), train_loss=res[0][1].numpy())
    for k, v in res[0][2].items():
        if v is not None:
            out["gsum/" + k] = co.grad_digest(v)
    out["no_grad"] = np.array([k for k, v in res[0][2].items() if v is None])
    path = os.path.join(ROOT, "tests", "golden", "model_csl.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; training loss", float(res[0][1]), "max|out|",
          float(res[0][0].abs().max()))


if __name__ == "__main__":
    main(sys.argv[1])
