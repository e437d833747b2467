"""Every model class keeps the layout recorded in tests/golden/model_layouts.json (tools/record_model_layouts.py, run at
the commit before the models moved onto esc_gnn_amd.nested): state_dict keys in order with shapes and dtypes, the module
tree child for child, the parameter values under a fixed seed after construction and after reset_parameters(), and how much
of the random stream the constructor consumes.  Also: zinc_cycle_models overrides only the readout, and no driver imports
another driver."""
import ast
import glob
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN, ROOT

_spec = importlib.util.spec_from_file_location("record_model_layouts", os.path.join(ROOT, "tools", "record_model_layouts.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

with open(os.path.join(GOLDEN, "model_layouts.json")) as _fh:
    RECORDED = json.load(_fh)
MODELS = ("counting", "kernel_gin", "zinc", "zinc_cycle", "qm9", "csl", "expressive", "ogb")


def test_fixture_names_the_eight_models():
    assert sorted(RECORDED) == sorted(MODELS) == sorted(rec.constructions())


@pytest.mark.parametrize("name", MODELS)
def test_layout_is_the_recorded_one(name):
    want, got = RECORDED[name], rec.layout(rec.constructions()[name][1])
    assert [k for k, _, _ in got["keys"]] == [k for k, _, _ in want["keys"]]         # state_dict keys, in order
    assert got["keys"] == want["keys"]                                               # ... their shapes and dtypes
    assert got["tree"] == want["tree"]                                               # child indices, Absorbed* included
    for key in rec.VALUE_KEYS:                                                       # same values from the same stream
        assert (key in got) == (key in want), key
        if key in want:
            assert got[key] == want[key], key
    assert ("sha256_reset" in want) == (name != "ogb")       # every NestedGIN twin has reset_parameters; OGB's GNN has none


def test_cycle_model_overrides_only_the_readout():
    from esc_gnn_amd import zinc_cycle_models, zinc_models
    cls = zinc_cycle_models.NestedGIN_eff
    assert "forward" not in vars(cls)
    assert cls.forward is zinc_models.NestedGIN_eff.forward
    assert sorted(k for k in vars(cls) if not k.startswith("__")) == ["_readout", "node_readout"]


def test_no_driver_imports_another_driver():
    drivers = sorted(glob.glob(os.path.join(ROOT, "esc-gnn_amd", "run_*.py")))
    assert len(drivers) >= 8
    for path in drivers:
        with open(path) as fh:
            tree = ast.parse(fh.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom):
                names = [node.module or ""] + [a.name for a in node.names]
            elif isinstance(node, ast.Import):
                names = [a.name for a in node.names]
            else:
                continue
            for n in names:
                assert not n.split(".")[-1].startswith("run_"), "%s imports %s" % (os.path.basename(path), n)
