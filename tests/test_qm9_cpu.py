"""QM9, host side: the run_qm9 CLI against the reference's argparse list (run_qm9.py:80-131) and conversion factors
(:24-31), the oracle model and distance against the goldens written from the reference (tools/make_golden_qm9.py), the
synthetic molecule generator, and the host collate of the QM9 keys against the reference's batch.py."""
import os

import numpy as np
import torch

from conftest import GOLDEN, load_collate
import qm9_oracle as qo

# name -> default of every flag of the reference's parser, in its order
REFERENCE_FLAGS = [
    ("target", 11), ("filter", False), ("convert", "post"), ("model", "NestedGIN_eff"), ("layers", 5), ("h", 3),
    ("max_nodes_per_hop", None), ("node_label", "spd"), ("use_rd", False), ("subgraph_pooling", "mean"), ("epochs", 200),
    ("batch_size", 64), ("lr", 1e-3), ("lr_decay_factor", 0.7), ("patience", 5), ("normalize_x", False),
    ("squared_dist", False), ("not_normalize_dist", False), ("use_max_dist", False), ("use_pos", False), ("RNI", False),
    ("use_relative_pos", False), ("seed", 1), ("save_appendix", ""), ("keep_old", False)]
HAR2EV, KCALMOL2EV = 27.2113825435, 0.04336414
REFERENCE_CONVERSION = [1., 1., HAR2EV, HAR2EV, HAR2EV, 1., HAR2EV, HAR2EV, HAR2EV, HAR2EV, HAR2EV, 1.]


def test_qm9_flags_and_defaults():
    import esc_gnn_amd.run_qm9 as rq
    a = rq.build_parser().parse_args([])
    for k, v in REFERENCE_FLAGS:
        assert getattr(a, k) == v, k
    assert [n.lstrip("-") for n in rq.REFERENCE_FLAGS] == [k for k, _ in REFERENCE_FLAGS]
    extra = sorted(set(vars(a)) - {k for k, _ in REFERENCE_FLAGS})
    assert extra == ["data_size", "res_dir"], extra                     # --epochs is the reference's own
    b = rq.build_parser().parse_args("--target 7 --layers 2 --data_size 96 --epochs 2 --convert pre --res_dir out".split())
    assert (b.target, b.layers, b.data_size, b.epochs, b.convert, b.res_dir) == (7, 2, 96, 2, "pre", "out")


def test_qm9_conversion_factors():
    import esc_gnn_amd.run_qm9 as rq
    assert list(rq.CONVERSION) == REFERENCE_CONVERSION


def test_qm9_oracle_reproduces_reference_golden_bitwise():
    from esc_gnn_amd.qm9_models import NestedGIN_eff as Qm9Model
    torch.set_num_threads(1)
    z = np.load(os.path.join(GOLDEN, "model_qm9.npz"))
    m = qo.qm9_oracle_from_recipe(z)
    keys = [str(k) for k in z["keys"]]
    shapes = ["x".join(map(str, v.shape)) or "scalar" for v in m.state_dict().values()]
    assert list(m.state_dict().keys()) == keys and shapes == [str(s) for s in z["shapes"]]

    class DS(object):
        num_features = qo.NUM_FEATURES
    mine = Qm9Model(DS, int(z["layers"])).state_dict()
    assert list(mine.keys()) == keys
    assert ["x".join(map(str, v.shape)) or "scalar" for v in mine.values()] == shapes
    assert tuple(mine["z_initial.weight"].shape) == (1800, 256) and tuple(mine["node_type_embedding.weight"].shape) == (5, 11)
    assert tuple(mine["conv1.lin.weight"].shape) == (11, 261) and tuple(mine["conv1.nn.0.weight"].shape) == (256, 11)
    _, b, G = load_collate("zinc3")
    b = {k: torch.tensor(v) for k, v in b.items()}
    rec = qo.qm9_batch_inputs(b["x"].numel(), b["edge_index"].size(1), G, int(z["input_seed"]))
    for k, v in rec.items():                                            # the recorded inputs are the recipe's
        assert torch.equal(v, torch.tensor(z["in/" + k])), k
    b.update(rec)
    m.train()
    out = m(*qo.model_args(b))
    assert out.shape == (G,)
    loss = torch.nn.functional.mse_loss(out, b["y"])
    loss.backward()
    assert np.array_equal(out.detach().numpy(), z["pred"])
    assert np.array_equal(loss.detach().numpy(), z["loss"])
    for n, p in m.named_parameters():
        s = z["gsum/" + n]
        assert float(p.grad.double().sum()) == s[0] and float(p.grad.double().abs().sum()) == s[1], n


def distance_golden_cases():
    z = np.load(os.path.join(GOLDEN, "qm9_distance.npz"))
    for name in (str(n) for n in z["names"]):
        f = z[name + "/flags"]
        flags = dict(norm=bool(f[0]), squared=bool(f[1]), relative_pos=bool(f[2]), cat=bool(f[3]),
                     max_value=None if np.isnan(f[4]) else float(f[4]))
        ea = z[name + "/edge_attr"] if (name + "/edge_attr") in z.files else None
        yield name, z[name + "/pos"], z[name + "/edge_index"], ea, flags, z[name + "/out"]


def test_distance_ref_agrees_with_reference_golden():
    names, nan_seen = [], False
    for name, pos, ei, ea, flags, want in distance_golden_cases():
        got = qo.distance_ref(pos, ei, ea, **flags).numpy()
        assert got.shape == want.shape, name
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        nan_seen |= bool(np.isnan(want).any())
        # fp64 against the reference's fp32: a norm and a division, 2 * 2^-23 relative at the most
        assert np.allclose(got, want.astype(np.float64), rtol=1e-6, atol=0, equal_nan=True), name
        names.append(name)
    assert len(names) >= 12 and nan_seen and "self_loops_only" in names


def test_synthetic_qm9_generator():
    from esc_gnn_amd.datasets import QM9_ATOMIC_NUMBERS, synthetic_qm9_graphs
    a, again = synthetic_qm9_graphs(0, 60), synthetic_qm9_graphs(0, 60)
    shifted = synthetic_qm9_graphs(10, 5)
    sizes = set()
    for g, (d, e) in enumerate(zip(a, again)):
        for k in ("x", "pos", "node_type", "edge_attr", "edge_index", "y"):
            assert torch.equal(d[k], e[k]), (g, k)                       # deterministic by seed
        assert d.name == e.name and isinstance(d.name, str)
        n, E = d.x.size(0), d.edge_index.size(1)
        sizes.add(n)
        assert 7 <= n <= 29
        assert d.x.dtype == torch.float32 and tuple(d.x.shape) == (n, 8)
        assert d.pos.dtype == torch.float32 and tuple(d.pos.shape) == (n, 3)
        assert d.node_type.dtype == torch.int64 and tuple(d.node_type.shape) == (n,)
        assert d.edge_attr.dtype == torch.float32 and tuple(d.edge_attr.shape) == (E, 4)
        assert d.y.dtype == torch.float32 and tuple(d.y.shape) == (1, 12) and bool(torch.isfinite(d.y).all())
        assert d.edge_index.dtype == torch.int64
        assert 0 <= int(d.node_type.min()) and int(d.node_type.max()) < 5
        assert torch.equal(d.x[:, 0], torch.tensor(QM9_ATOMIC_NUMBERS, dtype=torch.float32)[d.node_type])
        assert bool(((d.x[:, 1:7] == 0) | (d.x[:, 1:7] == 1)).all())
        assert bool((d.x[:, 7] >= 0).all()) and bool((d.x[:, 7] <= 4).all()) and bool((d.x[:, 7] == d.x[:, 7].round()).all())
        assert bool((d.edge_attr.sum(1) == 1).all()) and bool(((d.edge_attr == 0) | (d.edge_attr == 1)).all())
        pairs = [tuple(p) for p in d.edge_index.t().tolist()]
        assert pairs == sorted(set(pairs))                               # coalesced
        assert all(s != t for s, t in pairs) and all((t, s) in set(pairs) for s, t in pairs)   # no loops, symmetric
        lookup = {p: d.edge_attr[i] for i, p in enumerate(pairs)}
        assert all(torch.equal(lookup[(s, t)], lookup[(t, s)]) for s, t in pairs)            # one bond type per bond
        assert float(torch.pdist(d.pos.double()).min()) >= 0.69          # no two atoms coincide
    assert len(sizes) > 8
    for d, e in zip(shifted, a[10:15]):
        assert torch.equal(d.pos, e.pos) and torch.equal(d.y, e.y) and d.name == e.name       # seeded by graph id
    y = torch.cat([d.y for d in a])
    assert bool((y.std(0) > 0.05).all())                                 # every target varies over the set


def test_host_collate_reproduces_reference_qm9_batch():
    import esc_gnn_amd as E
    graphs, batch, G = load_collate("qm9_3")
    assert G == 3
    datas = []
    for g in graphs:
        kw = {k: (str(v) if k == "name" else torch.tensor(v)) for k, v in g.items()}
        datas.append(E.Data(**kw))
        assert kw["edge_attr"].shape[1] == 5 and kw["y"].shape == (1,)
    got = E.Batch.from_data_list(datas)
    assert sorted(got.keys) == sorted(batch)
    for k, want in batch.items():
        if k == "name":
            assert list(got.name) == [str(s) for s in want]
            continue
        assert got[k].dtype == torch.tensor(want).dtype and tuple(got[k].shape) == want.shape, k
        assert np.array_equal(got[k].numpy(), want, equal_nan=True), k
    assert got.num_graphs == 3
    from esc_gnn_amd.dataloader import _storable
    assert all(_storable(d) for d in datas)                              # the device store takes them
    loader = E.DataLoader(datas, batch_size=3, device=None)              # host path: the same batch
    (one,) = list(loader)
    for k, want in batch.items():
        if k != "name":
            assert np.array_equal(one[k].numpy(), want, equal_nan=True), k
