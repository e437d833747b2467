"""Expressiveness runs, the parts that need no GPU: the SR25 / EXP readers on the two data fixtures, the fold
arithmetic of run_exp, and the plain-torch oracle (tests/expressive_oracle.py) against every array of
tests/golden/model_expressive.npz (written by tools/make_golden_expressive.py from the reference's own code)."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import expressive_oracle as eo


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "model_expressive.npz"))


def _sorted_both_directions(ei):
    pairs = list(map(tuple, ei.t().tolist()))
    return pairs == sorted(set(pairs)) and set(pairs) == {(b, a) for a, b in pairs}


def test_sr25_reader():
    from esc_gnn_amd.datasets import load_sr25
    graphs = load_sr25(eo.SR25_FILE)
    assert len(graphs) == 15
    for g in graphs:
        assert g.y is None and g.x.shape == (25, 1) and g.x.dtype == torch.float32 and bool((g.x == 1).all())
        assert g.edge_index.shape == (2, 300) and g.edge_index.dtype == torch.int64
        assert _sorted_both_directions(g.edge_index)
        assert torch.equal(torch.bincount(g.edge_index[0], minlength=25), torch.full((25,), 12))     # 12-regular


def test_exp_reader(golden):
    from esc_gnn_amd.datasets import load_exp_txt
    graphs = load_exp_txt(eo.EXP_FILE)
    assert len(graphs) == 40
    assert [int(g.y) for g in graphs] == [1, 0] * 20 == golden["exp_labels"].tolist()
    assert [g.x.size(0) for g in graphs] == golden["exp_nodes"].tolist()
    for g in graphs:
        assert g.y.dtype == torch.int64 and g.y.shape == (1,)
        assert g.x.dtype == torch.float32 and g.x.size(1) == 2 and bool((g.x.sum(dim=1) == 1).all())
        assert _sorted_both_directions(g.edge_index) and int(g.edge_index.max()) < g.x.size(0)
    assert len(load_exp_txt(eo.EXP_FILE, limit=7)) == 7
    with pytest.raises(ValueError, match="not supported"):
        load_exp_txt(os.path.join(GOLDEN, "GRAPHSAT.pkl"))


def test_exp_reader_matches_the_oracle_reader():
    import graph_sources as gs
    from esc_gnn_amd.datasets import load_exp_txt, load_sr25
    for mine, ref in ((load_exp_txt(eo.EXP_FILE), gs.read_exp_txt(eo.EXP_FILE, 40)), (load_sr25(eo.SR25_FILE), gs.read_g6(eo.SR25_FILE))):
        assert len(mine) == len(ref)
        for d, (n, s, t) in zip(mine, ref):
            assert d.x.size(0) == n and np.array_equal(d.edge_index.numpy(), np.stack([s, t]))


@pytest.mark.parametrize("split", range(10))
def test_exp_split(split):
    from esc_gnn_amd.datasets import exp_split
    p = exp_split(1200, split)
    assert (len(p["test"]), len(p["val"]), len(p["train"])) == (120, 108, 972)
    assert p["test"] == list(range(120 * split, 120 * (split + 1)))
    sets = [set(p[k]) for k in ("train", "val", "test")]
    assert all(not (a & b) for i, a in enumerate(sets) for b in sets[i + 1:])
    assert set().union(*sets) == set(range(1200))
    assert p["lrn"] == [i for i in p["test"] if i % 4 <= 1] and p["exp"] == [i for i in p["test"] if i % 4 > 1]
    assert len(p["lrn"]) == len(p["exp"]) == 60
    rest = [i for i in range(1200) if i not in sets[2]]
    assert p["val"] == rest[108 * split:108 * (split + 1)]          # the split-th tenth of what remains, in order
    assert p["train"] == sorted(p["train"])


def test_oracle_reproduces_the_golden(golden):
    from esc_gnn_amd.datasets import load_exp_txt, load_sr25
    torch.set_num_threads(1)
    z = golden
    h = int(z["h"])
    sr, ex = eo.cpu_features(load_sr25(eo.SR25_FILE), h), eo.cpu_features(load_exp_txt(eo.EXP_FILE), h)
    assert np.array_equal(eo.graph_digests(sr), z["sr_digests"])
    assert np.array_equal(eo.graph_digests(ex), z["exp_digests"])
    # SR25: eval predictions in fp32 and fp64, their difference, the 105 distances
    m = eo.expressive_oracle_from_recipe(z, 1).eval()
    assert list(m.state_dict().keys()) == [str(k) for k in z["keys"]] and len(z["keys"]) == 73
    args = eo.collate(sr)
    with torch.no_grad():
        p32 = m(*args)
        p64 = copy.deepcopy(m).double()(args[0].double(), *args[1:])
    assert np.array_equal(p32.numpy(), z["sr_pred32"]) and np.array_equal(p64.numpy(), z["sr_pred64"])
    assert float((p32.double() - p64).abs().max()) == float(z["sr_err32"])
    d64 = torch.pdist(p64, p=2)
    assert d64.shape == (105,) and np.array_equal(d64.numpy(), z["sr_dist64"])
    assert int((d64 < 1e-2).sum()) == int(z["sr_wrong"]) == 0
    # the margin the generator asserted: a per-element error of 3 * err32 cannot carry a distance across the threshold
    assert float(d64.min()) - 1e-2 > 2.0 * int(z["hidden"]) ** 0.5 * 3.0 * float(z["sr_err32"])
    # EXP: the training step on the first 20 graphs with the recorded dropout multiplier
    m = eo.expressive_oracle_from_recipe(z, 2).train()
    drop = torch.tensor(z["exp_drop"])
    n = drop.size(0)
    out = m(*eo.collate(ex[:n]), drop=drop)
    loss = torch.nn.functional.nll_loss(out, torch.tensor(z["exp_labels"][:n]))
    loss.backward()
    assert np.array_equal(out.detach().numpy(), z["exp_out"]) and np.array_equal(loss.detach().numpy(), z["exp_loss"])
    for k, p in m.named_parameters():
        assert np.array_equal(eo.grad_digest(p.grad), z["gsum/" + k]), k
    assert all(not k.endswith(".eps") for k, _ in m.named_parameters())          # eps is a buffer: no gradient


def test_driver_flags_match_the_reference():
    from esc_gnn_amd import run_exp, run_sr
    want = dict(model="GIN", h=3, layers=8, width=64, epochs=500, dataset="EXP", learnRate=0.001)
    for mod in (run_sr, run_exp):
        args = vars(mod.build_parser().parse_args([]))
        assert {k: args[k] for k in want} == want
    assert run_sr.build_parser().parse_args([]).data_root == "data/sr25"
    a = run_exp.build_parser().parse_args([])
    assert (a.splits, a.limit, a.seed, a.data_root) == (10, None, None, None)
    assert run_sr.find_data_file(GOLDEN, ("sr251256.g6",)) == eo.SR25_FILE
    assert run_sr.find_data_file(eo.EXP_FILE, ("GRAPHSAT.txt",)) == eo.EXP_FILE
    assert run_sr.find_data_file(os.path.join(GOLDEN, "nowhere"), ("GRAPHSAT.txt",)) is None
