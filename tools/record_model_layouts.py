"""Record the layout of every model class at its smallest meaningful size: tests/golden/model_layouts.json, the fixture
of tests/test_model_layouts_cpu.py.  Run it at the commit whose layout is the yardstick (the parent of a refactor), on the
CPU: per model the ordered (key, shape, dtype) of the state_dict, repr of the module tree, a sha256 over the state_dict
bytes after torch.manual_seed(0) + construction, a second one after torch.manual_seed(1) + reset_parameters() where the
class has it, and the next torch.rand(1) after construction (how much of the random stream the constructor consumed).

    python tools/record_model_layouts.py [--out tests/golden/model_layouts.json] [--no-values]
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


class _Dataset(object):
    num_features, num_classes = 7, 3


def constructions():
    """name -> (class, zero-argument constructor); imported lazily so the test can name a class without building it"""
    from esc_gnn_amd import (csl_models, expressive_models, kernel_gin, ogb_mol_gnn, qm9_models, run_graphcount,
                             zinc_cycle_models, zinc_models)
    ds = _Dataset()
    return {
        "counting": (run_graphcount.NestedGIN_eff, lambda: run_graphcount.NestedGIN_eff(
            None, 2, 16, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True)),
        "kernel_gin": (kernel_gin.NestedGIN_eff, lambda: kernel_gin.NestedGIN_eff(ds, 2, 16)),
        "zinc": (zinc_models.NestedGIN_eff, lambda: zinc_models.NestedGIN_eff(None, 2)),
        "zinc_cycle": (zinc_cycle_models.NestedGIN_eff, lambda: zinc_cycle_models.NestedGIN_eff(None, 2)),
        "qm9": (qm9_models.NestedGIN_eff, lambda: qm9_models.NestedGIN_eff(ds, 2)),
        "csl": (csl_models.NestedGIN, lambda: csl_models.NestedGIN(2, 16)),
        "expressive": (expressive_models.NestedGIN, lambda: expressive_models.NestedGIN(3, 2, 16)),
        "ogb": (ogb_mol_gnn.GNN, lambda: ogb_mol_gnn.GNN("ogbg-molhiv", 1, num_layer=2, emb_dim=16, gnn_type="gin_eff")),
    }


def tree_of(model):
    """repr of the module tree.  Two models print only their class name, so the tree is torch.nn.Module's own repr."""
    return torch.nn.Module.__repr__(model)


def digest(model):
    h = hashlib.sha256()
    for key, t in model.state_dict().items():
        h.update(key.encode())
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def layout(build):
    torch.manual_seed(0)
    model = build()
    rec = {"next_rand": torch.rand(1).item(),
           "keys": [[k, list(t.shape), str(t.dtype)] for k, t in model.state_dict().items()],
           "tree": tree_of(model),
           "sha256_constructed": digest(model)}
    if hasattr(model, "reset_parameters"):
        torch.manual_seed(1)
        model.reset_parameters()
        rec["sha256_reset"] = digest(model)
    return rec


VALUE_KEYS = ("next_rand", "sha256_constructed", "sha256_reset")


def record(values=True):
    out = {name: layout(build) for name, (_, build) in constructions().items()}
    if not values:
        for rec in out.values():
            for k in VALUE_KEYS:
                rec.pop(k, None)
    return out


def dumps(layouts):
    """JSON with one state_dict entry per line"""
    models = []
    for name in sorted(layouts):
        rec = dict(layouts[name])
        keys = ",\n".join("   " + json.dumps(k) for k in rec.pop("keys"))
        rest = ",\n".join("  %s: %s" % (json.dumps(k), json.dumps(rec[k])) for k in sorted(rec))
        models.append(' %s: {\n  "keys": [\n%s\n  ],\n%s\n }' % (json.dumps(name), keys, rest))
    return "{\n" + ",\n".join(models) + "\n}\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "model_layouts.json"))
    ap.add_argument("--no-values", action="store_true", help="leave out the digests that depend on torch's CPU generator")
    a = ap.parse_args()
    with open(a.out, "w") as fh:
        fh.write(dumps(record(not a.no_values)))
    print("wrote", a.out)
