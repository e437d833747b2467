"""Graphlet counting on the MI355X: the orbit-count kernel (csrc/graphlets.hip) bit for bit against the networkx oracle
and the closed forms on complete graphs, its limits, the label options of the synthetic count dataset, and run_graphcount
training on the task's own labels (--synthetic_labels task)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_collate, require_gpu
import graphlet_oracle as go

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _kernel(node_counts, edge_lists):
    from esc_gnn_amd.graphlets import graphlet_orbit_counts_edge_lists
    got = graphlet_orbit_counts_edge_lists(node_counts, [torch.as_tensor(e) for e in edge_lists])
    assert all(t.dtype == torch.int32 and t.shape == (n, 11) for t, n in zip(got, node_counts))
    return [t.numpy() for t in got]


def _check_against_oracle(node_counts, edge_lists):
    got = _kernel(node_counts, edge_lists)
    for g, (n, ei) in enumerate(zip(node_counts, edge_lists)):
        assert np.array_equal(got[g], go.orbit_labels(n, ei)), g
    return got


def _data(n, ei):
    from esc_gnn_amd.data import Data
    return Data(x=torch.ones(n, 1), edge_index=torch.as_tensor(ei), num_nodes=n)


# ---- the kernel --------------------------------------------------------------------------------------------------------
def test_graphlet_kernel_hand_cases(E):
    cases = go.hand_cases()
    cases += [(nm,) + go.pattern_edges(nm) + (None,) for nm in ("tailed_triangle", "chordal_cycle")]
    n, messy, clean = go.messy_case()
    cases += [("messy", n, messy, go.orbit_labels(n, clean))]
    got = _check_against_oracle([c[1] for c in cases], [c[2] for c in cases])
    for (name, n, ei, want), g in zip(cases, got):
        assert want is None or np.array_equal(g, want), name


def test_graphlet_kernel_collate_graphs(E):
    ns, eis = [], []
    for tag in ("zinc3", "molhiv4"):
        gs, _, _ = load_collate(tag)
        ns += [int(g["x"].shape[0]) for g in gs]
        eis += [g["edge_index"] for g in gs]
    got = _check_against_oracle(ns, eis)
    assert sum(int(g.sum()) for g in got) > 0


def test_graphlet_kernel_count_shaped_and_molecule_graphs(E):
    from esc_gnn_amd.datasets import _ring_closing_edges, count_shape_adjacency
    ns, eis = [], []
    for g in range(24):                                        # all four (n, d) of the count shape, six times
        A = count_shape_adjacency(g)
        ns.append(A.shape[0])
        eis.append(np.stack(np.where(A == 1.0)).astype(np.int64))
    for g in range(40):
        n, ei, _ = _ring_closing_edges(90000 + g)
        ns.append(n)
        eis.append(ei)
    got = _check_against_oracle(ns, eis)
    allc = np.concatenate(got)
    assert ((allc > 0).sum(axis=0) > 0).all()                  # every orbit occurs
    again = _kernel(ns, eis)                                   # deterministic
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


def test_graphlet_kernel_complete_graphs(E):
    from esc_gnn_amd.graphlets import graphlet_counts, graphlet_orbit_counts
    sizes = (13, 24, 64)                                       # 64: mask bit 63 and the largest counts
    got = _kernel(list(sizes), [go.complete_graph_edges(n) for n in sizes])
    for n, g in zip(sizes, got):
        assert np.array_equal(g, np.tile(go.complete_graph_row(n), (n, 1))), n
    k64 = _data(64, go.complete_graph_edges(64))
    exact = graphlet_orbit_counts([k64])[0]
    assert exact.dtype == torch.int32 and np.array_equal(exact.numpy(), got[2])
    assert int(exact[0, 8:].sum()) == 35739900                 # 60 C(64,5) houses, 5 nodes each, over 64 nodes
    with pytest.raises(ValueError, match="2\\^24"):            # the house count through a node is not exact in float32
        graphlet_counts([k64])
    small = graphlet_counts([_data(13, go.complete_graph_edges(13))])[0]
    assert small.dtype == torch.float32 and np.array_equal(small.numpy(), go.orbit_sums(got[0]).astype(np.float32))


def test_graphlet_kernel_limits(E):
    small = np.array([[0, 1, 2], [1, 2, 0]], dtype=np.int64)
    ei65 = np.array([[i for i in range(65)], [(i + 1) % 65 for i in range(65)]], dtype=np.int64)
    with pytest.raises(ValueError, match="65 nodes"):
        _kernel([3, 65], [small, ei65])
    with pytest.raises(ValueError, match="outside"):
        _kernel([3], [np.array([[0, 1], [1, 3]], dtype=np.int64)])
    none = np.zeros((2, 0), dtype=np.int64)
    got = _kernel([4, 3], [none, small])                       # an edgeless graph, beside one with edges
    assert not got[0].any() and np.array_equal(got[1], go.orbit_labels(3, small))
    assert not _kernel([5], [none])[0].any()                   # no edge at all in the call
    assert _kernel([], []) == []


# ---- the dataset's label options ---------------------------------------------------------------------------------------
def test_synthetic_count_graph_labels(E):
    from esc_gnn_amd.datasets import count_shape_adjacency, synthetic_count_graphs
    from esc_gnn_amd.graphlets import GRAPHLET_ORBITS
    base = synthetic_count_graphs(0, 8)
    assert [d.y.shape for d in base] == [(d.x.size(0),) for d in base]
    for g, d in enumerate(base):                               # the default is what it was: triangles, host arithmetic
        A = count_shape_adjacency(g)
        assert d.y.dtype == torch.float32 and np.array_equal(d.y.numpy(), (np.diagonal(A @ A @ A) / 2.0).astype(np.float32))
    named = synthetic_count_graphs(0, 8, labels="triangle")
    cyc = synthetic_count_graphs(0, 8, labels="cycles")
    gl = synthetic_count_graphs(0, 8, labels="graphlets")
    orb = synthetic_count_graphs(0, 8, labels="graphlet_orbits")
    for b, t, c, s, o in zip(base, named, cyc, gl, orb):
        n = b.x.size(0)
        assert torch.equal(b.y, t.y)
        assert c.y.dtype == s.y.dtype == o.y.dtype == torch.float32
        assert c.y.shape == (n, 4) and s.y.shape == (n, 5) and o.y.shape == (n, 11)
        assert torch.equal(c.y[:, 0], b.y)                     # 3-cycles through a node = its triangles
        assert torch.equal(s.y, torch.stack([o.y[:, list(cols)].sum(1) for cols in GRAPHLET_ORBITS], dim=1))
        assert np.array_equal(o.y.numpy(), go.orbit_labels(n, b.edge_index.numpy()).astype(np.float32))
        for other in (t, c, s, o):                             # same graphs, edge order and x
            assert torch.equal(other.edge_index, b.edge_index) and torch.equal(other.x, b.x)
    with pytest.raises(ValueError, match="labels"):
        synthetic_count_graphs(0, 1, labels="other")


# ---- the driver --------------------------------------------------------------------------------------------------------
SMALL = "--epochs 2 --synthetic_graphs 40 --batch_size 8 --layers 2 --h 2 --lr 0.01 --synthetic_labels task "


def _run(rg, capsys, argv):
    rg.main(argv.split())
    out = capsys.readouterr().out
    m = re.search(r"Mean = (-?[0-9.]+), Std = (-?[0-9.]+)", out)
    assert m, out[-2000:]
    return float(m.group(1)), float(m.group(2)), out


def _train_val_labels(labels, column):
    from esc_gnn_amd.datasets import synthetic_count_graphs
    y = torch.cat([d.y[:, column] for d in synthetic_count_graphs(0, 20, labels=labels)])     # 30 % + 20 % of 40 graphs
    return float(y.mean()), float(y.std())


def test_cli_trains_on_the_task_labels(E, tmp_path, monkeypatch, capsys):
    import esc_gnn_amd.run_graphcount as rg
    monkeypatch.chdir(tmp_path)
    mean1, std1, out = _run(rg, capsys, SMALL + "--dataset count_graphlet --target 1 --save_appendix t1")
    assert "Epoch: 001" in out and "Validation MAE" in out
    res = os.path.join(tmp_path, "results", "count_graphlet_t1")
    log = open(os.path.join(res, "log.txt")).read()
    assert np.isfinite(float(log.splitlines()[0].split("Loss: ")[1].split(",")[0]))
    assert os.path.exists(os.path.join(res, "model_checkpoint2.pth"))
    want = _train_val_labels("graphlets", 1)                   # the chordal cycles through the node
    assert abs(mean1 - want[0]) <= 6e-4 and abs(std1 - want[1]) <= 6e-4       # printed with three decimals
    mean4, _, _ = _run(rg, capsys, SMALL + "--dataset count_graphlet --target 4 --save_appendix t4")
    assert mean4 != mean1
    assert abs(mean4 - _train_val_labels("graphlets", 4)[0]) <= 6e-4
    mean_o, _, _ = _run(rg, capsys, SMALL + "--dataset count_graphlet --target 4 --graphlet_orbit 0 --save_appendix t4o")
    assert abs(mean_o - _train_val_labels("graphlet_orbits", 8)[0]) <= 6e-4   # the house's apex orbit
    mean_c, _, out = _run(rg, capsys, SMALL + "--dataset count_cycle --target 2 --save_appendix c2")
    assert "Epoch: 001" in out and abs(mean_c - _train_val_labels("cycles", 2)[0]) <= 6e-4
    assert os.path.exists(os.path.join(tmp_path, "results", "count_cycle_c2", "model_checkpoint2.pth"))


def test_cli_rejects_targets_outside_the_task(E, tmp_path, monkeypatch, capsys):
    import esc_gnn_amd.datasets as ds
    import esc_gnn_amd.run_graphcount as rg
    monkeypatch.chdir(tmp_path)

    def no_build(*a, **k):
        raise AssertionError("the dataset was built before the flags were checked")
    monkeypatch.setattr(ds, "build_count_dataset", no_build)
    for argv, valid in (("--dataset count_graphlet --target 5", r"0\.\.4"), ("--dataset count_cycle --target 4", r"0\.\.3"),
                        ("--dataset count_graphlet --target 1 --graphlet_orbit 2", r"0\.\.1")):
        with pytest.raises(ValueError, match=valid):
            rg.main((SMALL + argv).split())
    with pytest.raises(ValueError, match="count_other"):
        rg.main((SMALL + "--dataset count_other --target 0").split())
