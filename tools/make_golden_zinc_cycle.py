"""Writes tests/golden/model_zinc_cycle.npz (data only) from the reference's zinc_cycle_models.NestedGIN_eff.

As oracle/make_golden_model.main_zinc does for zinc_models: the reference class body is exec'd on the oracle primitives
(oracle/ref_model.py), seeded, and run in training mode on the `zinc3` collate batch with node-level cycle targets
(tests/zinc_cycle_oracle.batch_cycle_labels, column `target`).  tests/zinc_cycle_oracle.NestedGINEffZincCycleRef must
reproduce it bit for bit.  Recorded: the seed recipe, the state_dict key list, the [N, 4] labels, the per-node
predictions, the L1 loss over the nodes and a digest (sum, abs-sum) of every parameter gradient.

    python tools/make_golden_zinc_cycle.py /path/to/reference/zinc_cycle_models.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
from make_golden_model import Bag, reference_class  # noqa: E402
import zinc_cycle_oracle as zco  # noqa: E402

LAYERS, SEED, TARGET = 2, 779, 3


def main(ref_file):
    torch.set_num_threads(1)
    g = np.load(os.path.join(ROOT, "tests", "golden", "collate_zinc3.npz"))
    b = {k[len("batch_"):]: torch.tensor(g[k]) for k in g.files if k.startswith("batch_")}
    labels = zco.batch_cycle_labels(b["edge_index"].numpy(), b["batch"].numpy())
    y = torch.tensor(labels[:, TARGET]).view(-1, 1)
    torch.manual_seed(SEED)
    ref = reference_class(ref_file)(None, LAYERS)
    with torch.no_grad():
        for name, p in ref.named_parameters():
            if p.dim() == 1 and "bias" not in name:
                p.add_(0.1 * torch.randn_like(p))
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    mine = zco.zinc_cycle_oracle_from_recipe(dict(seed=SEED, layers=LAYERS))
    assert list(mine.state_dict().keys()) == list(sd0.keys())
    for k, v in mine.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    res = []
    for m, call in ((ref, lambda m: m(Bag(x=b["x"], edge_index=b["edge_index"], edge_attr=b["edge_attr"], batch=b["batch"],
                                         pos_enc=b["pos_enc"], pos_index=b["pos_index"], pos_batch=b["pos_batch"]))),
                    (mine, lambda m: m(b["x"], b["edge_index"], b["edge_attr"], b["pos_enc"], b["pos_index"],
                                       b["pos_batch"], b["batch"]))):
        m.train()
        out = call(m)
        loss = F.l1_loss(out, y)
        loss.backward()
        res.append((out.detach(), loss.detach(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    assert res[0][0].shape == (b["x"].numel(), 1)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
    out = {"keys": np.array(list(sd0.keys())), "labels": labels, "target": np.int64(TARGET), "pred": res[0][0].numpy(),
           "loss": res[0][1].numpy(), "layers": np.int64(LAYERS), "seed": np.int64(SEED)}
    for k, v in res[0][2].items():
        out["gsum/" + k] = np.array([float(v.double().sum()), float(v.double().abs().sum())])
    path = os.path.join(ROOT, "tests", "golden", "model_zinc_cycle.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB; loss", float(res[0][1]), "labels per column",
          labels.sum(axis=0))


if __name__ == "__main__":
    main(sys.argv[1])
