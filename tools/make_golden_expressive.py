"""Writes tests/golden/model_expressive.npz (data only) from the reference's expressiveness drivers.

The reference's own create_subgraphs (utils_edge_efficient.py, imported in place under oracle/pyg_shim as
oracle/make_golden.py does) runs on the 15 SR25 graphs and the 40 EXP graphs of the two data fixtures, its batch.py
collates them, and the `NestedGIN` class body that run_sr.py defines inline is exec'd on the oracle primitives
(oracle/ref_model.py) with `dataset.num_features` injected and an `F` whose dropout replays a recorded mask.
tests/expressive_oracle.NestedGINRef must reproduce it bit for bit: the eval-mode SR25 predictions, and on the first 20
EXP graphs the train-mode output, the NLL loss and every parameter gradient.

Recorded: the seed recipe, the state_dict key list, per-graph digests of edge_index / pos_enc / pos_index / pos_batch,
the SR25 predictions in fp32 and fp64, err32 = max |pred32 - pred64|, the 105 fp64 distances, and for EXP the dropout
multiplier, the labels, output, loss and a digest (sum, abs-sum) of every gradient.

The SR25 criterion (`pdist < 1e-2`) is only a meaningful fixture when the fp32 error cannot move a distance across the
threshold, so the margin is asserted before anything is written: with tol = 3 * err32 and C = hidden,
min(dist64) - 1e-2 > 2 * sqrt(C) * tol.

    python tools/make_golden_expressive.py /path/to/reference
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
LAYERS, HIDDEN, SEED, H, MASK_SEED, EXP_TRAIN = 8, 64, 1, 3, 20, 20


def reference_nested_gin(ref_dir, num_features, drop_holder):
    """the inline NestedGIN of run_sr.py on the oracle primitives; F.dropout multiplies by drop_holder[0] when training"""
    import ref_model as rm
    path = os.path.join(ref_dir, "run_sr.py")
    tree = ast.parse(open(path).read())
    node = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "NestedGIN"][-1]

    def dropout(x, p=0.5, training=True):
        assert p == 0.5
        return x * drop_holder[0].to(x.dtype) if training else x

    Fm = types.SimpleNamespace(relu=F.relu, log_softmax=F.log_softmax, dropout=dropout)
    ns = dict(torch=torch, F=Fm, Linear=torch.nn.Linear, Sequential=torch.nn.Sequential, ReLU=torch.nn.ReLU,
              GINEConv=rm.GINEConv, global_add_pool=rm.global_add_pool,
              dataset=types.SimpleNamespace(num_features=num_features))
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns["NestedGIN"]


def main(ref_dir):
    torch.set_num_threads(1)
    sys.path[:0] = [os.path.join(ROOT, "oracle", "pyg_shim"), ref_dir, os.path.join(ROOT, "oracle"),
                    os.path.join(ROOT, "tests"), ROOT]
    import utils_edge_efficient as ref_feat            # the reference, imported in place
    from batch import Batch as RefBatch                 # the reference's batch.py
    from torch_geometric.data import Data as ShimData
    from make_golden_model import Bag
    import expressive_oracle as eo
    from esc_gnn_amd.datasets import load_exp_txt, load_sr25

    def featurise(raw):
        return [ref_feat.create_subgraphs(ShimData(x=d.x, edge_index=d.edge_index, edge_attr=None, y=d.y), H,
                                          node_label="hop", use_rd=False, subgraph_pretransform=None, self_loop=True)
                for d in raw]

    def bag_of(graphs):
        b = RefBatch.from_data_list(graphs)
        return Bag(x=b.x, edge_index=b.edge_index, batch=b.batch, pos_enc=b.pos_enc, pos_index=b.pos_index,
                   pos_batch=b.pos_batch, y=getattr(b, "y", None))

    def args_of(b):
        return (b.x, b.edge_index, b.pos_enc, b.pos_index, b.pos_batch, b.batch)

    sr_raw, exp_raw = load_sr25(eo.SR25_FILE), load_exp_txt(eo.EXP_FILE)
    sr, ex = featurise(sr_raw), featurise(exp_raw)
    # the CPU restatement of the feature build gives the same tensors (the CPU test recomputes the digests with it)
    for ref_graphs, raw in ((sr, sr_raw), (ex, exp_raw)):
        for a, b in zip(ref_graphs, eo.cpu_features(raw, H)):
            for k in eo.FEATURE_KEYS:
                assert np.array_equal(a[k].numpy(), b[k].numpy()), k
    recipe = dict(seed=SEED, layers=LAYERS, hidden=HIDDEN)
    out = {"seed": np.int64(SEED), "layers": np.int64(LAYERS), "hidden": np.int64(HIDDEN), "h": np.int64(H),
           "sr_digests": eo.graph_digests(sr), "exp_digests": eo.graph_digests(ex),
           "exp_nodes": np.array([int(g.x.size(0)) for g in ex], dtype=np.int64),
           "exp_labels": np.array([int(g.y) for g in ex], dtype=np.int64)}

    # ---- SR25: eval-mode predictions of all 15 graphs, fp32 and fp64, and the distance margin ----
    drop = [None]
    torch.manual_seed(SEED)
    ref = reference_nested_gin(ref_dir, 1, drop)(LAYERS, HIDDEN)
    ref.reset_parameters()
    ref.eval()
    mine = eo.expressive_oracle_from_recipe(recipe, 1).eval()
    assert list(mine.state_dict().keys()) == list(ref.state_dict().keys())
    for k, v in ref.state_dict().items():
        assert torch.equal(v, mine.state_dict()[k]), k
    b = bag_of(sr)
    with torch.no_grad():
        p_ref, p32 = ref(b), mine(*args_of(b))
        p64 = copy.deepcopy(mine).double()(b.x.double(), *args_of(b)[1:])
    assert torch.equal(p_ref, p32), "SR25: the restatement differs from the reference class"
    err32 = float((p32.double() - p64).abs().max())
    d64 = torch.pdist(p64, p=2)
    tol = 3.0 * err32
    margin = float(d64.min()) - 1e-2
    print("SR25: max|pred| %.4g, err32 %.4g, min dist64 %.4g, %d of %d pairs below 1e-2; margin %.4g vs %.4g" % (
        float(p64.abs().max()), err32, float(d64.min()), int((d64 < 1e-2).sum()), d64.numel(), margin,
        2.0 * HIDDEN ** 0.5 * tol))
    assert margin > 2.0 * HIDDEN ** 0.5 * tol, "the SR25 margin does not hold for this seed: pick another one"
    out.update(keys=np.array(list(ref.state_dict().keys())), sr_pred32=p32.numpy(), sr_pred64=p64.numpy(),
               sr_err32=np.float64(err32), sr_dist64=d64.numpy(), sr_wrong=np.int64(int((d64 < 1e-2).sum())))

    # ---- EXP: one training step on the first 20 graphs with a recorded dropout multiplier ----
    gen = torch.Generator().manual_seed(MASK_SEED)
    drop[0] = (torch.rand(EXP_TRAIN, HIDDEN, generator=gen) >= 0.5).float() * 2.0
    torch.manual_seed(SEED)
    ref = reference_nested_gin(ref_dir, 2, drop)(LAYERS, HIDDEN)
    ref.reset_parameters()
    mine = eo.expressive_oracle_from_recipe(recipe, 2)
    for k, v in ref.state_dict().items():
        assert torch.equal(v, mine.state_dict()[k]), k
    b = bag_of(ex[:EXP_TRAIN])
    y = b.y.view(-1)
    assert y.dtype == torch.int64
    res = []
    for m, call in ((ref, lambda m: m(b)), (mine, lambda m: m(*args_of(b), drop=drop[0]))):
        m.train()
        o = call(m)
        loss = F.nll_loss(o, y)
        loss.backward()
        res.append((o.detach(), loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    out.update(exp_drop=drop[0].numpy(), exp_out=res[0][0].numpy(), exp_loss=res[0][1].numpy())
    for k, v in res[0][2].items():
        out["gsum/" + k] = eo.grad_digest(v)
    path = os.path.join(ROOT, "tests", "golden", "model_expressive.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; EXP loss", float(res[0][1]), "max|out|",
          float(res[0][0].abs().max()))


if __name__ == "__main__":
    main(sys.argv[1])
