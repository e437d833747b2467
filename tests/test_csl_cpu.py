"""The CSL run, the parts that need no GPU: the graph generator, the ESC features of the family on the CPU oracle, the fold
protocol, the plain-torch oracle (tests/csl_oracle.py) against every array of tests/golden/model_csl.npz (written by
tools/make_golden_csl.py from the reference's own code), and the driver's flags."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import csl_oracle as co


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "model_csl.npz"))


@pytest.fixture(scope="module")
def fixture_features():
    """ESC features (h = 4, resistance distance, self loops) of the 20 fixture graphs on the CPU oracle: computed once"""
    return co.cpu_features(co.fixture_graphs(), 4)


def _pairs(g):
    return list(map(tuple, g.edge_index.t().tolist()))


def test_generator_properties():
    from esc_gnn_amd.datasets import CSL_SKIPS, csl_graphs
    assert CSL_SKIPS == co.SKIPS == (2, 3, 4, 5, 6, 9, 11, 12, 13, 16)
    graphs = csl_graphs()
    assert len(graphs) == 150
    assert [int(g.y) for g in graphs] == [k for k in range(10) for _ in range(15)]      # class by class
    for g in graphs:
        assert g.x.shape == (41, 1) and g.x.dtype == torch.float32 and bool((g.x == 1).all())
        assert g.y.dtype == torch.int64 and g.y.shape == (1,)
        assert g.edge_index.shape == (2, 164) and g.edge_index.dtype == torch.int64
        pairs = _pairs(g)
        assert pairs == sorted(set(pairs))                                              # sorted by (src, dst), no duplicates
        assert set(pairs) == {(b, a) for a, b in pairs}                                 # both directions
        assert all(a != b for a, b in pairs)
        assert torch.equal(torch.bincount(g.edge_index[0], minlength=41), torch.full((41,), 4))      # 4-regular
    for k, skip in enumerate(CSL_SKIPS):                                                # copy 0 keeps the cycle labelling
        assert np.array_equal(graphs[15 * k].edge_index.numpy(), co.csl_edges(41, skip))
        assert {(i, (i + 1) % 41) for i in range(41)} | {(i, (i + skip) % 41) for i in range(41)} <= set(_pairs(graphs[15 * k]))
        assert not torch.equal(graphs[15 * k + 1].edge_index, graphs[15 * k].edge_index)
    again = csl_graphs()
    assert all(torch.equal(a.edge_index, b.edge_index) for a, b in zip(graphs, again))  # same seed, same graphs
    other = csl_graphs(seed=1)
    assert any(not torch.equal(a.edge_index, b.edge_index) for a, b in zip(graphs, other))
    few = csl_graphs(copies=3, skips=(2, 3))
    assert [int(g.y) for g in few] == [0, 0, 0, 1, 1, 1]
    assert all(torch.equal(a.edge_index, b.edge_index) for a, b in zip(few[:3], graphs[:3]))


def test_relabelled_copies_are_isomorphic():
    """a generated copy is its class's cycle graph under SOME relabelling: same degree sequence is not enough, so check
    that the skip structure survives — the graph has a Hamiltonian cycle whose R-th powers are the remaining edges"""
    import networkx as nx
    from esc_gnn_amd.datasets import CSL_SKIPS, csl_graphs
    graphs = csl_graphs(copies=2)
    for k in range(len(CSL_SKIPS)):
        a, b = (nx.Graph(_pairs(g)) for g in graphs[2 * k:2 * k + 2])
        assert nx.is_isomorphic(a, b)


def test_oracle_features_tell_the_classes_apart(fixture_features):
    sets = [co.feature_multiset(g) for g in fixture_features]
    for k in range(10):
        assert sets[2 * k] == sets[2 * k + 1], "class %d: the relabelled copy has other features" % k
    for a in range(10):
        for b in range(a + 1, 10):
            assert sets[2 * a] != sets[2 * b], "classes %d and %d share a feature multiset" % (a, b)
    for g in fixture_features:
        assert g.edge_index.shape == (2, 205)                    # 164 edges + 41 self loops
        assert int(g.pos_index.max()) < 1800 and int(g.pos_batch.max()) == 204


def _check_folds(labels, folds=10):
    from esc_gnn_amd.datasets import csl_k_fold
    labels = np.asarray(labels)
    train, test, val = csl_k_fold(labels, folds)
    assert len(train) == len(test) == len(val) == folds
    n = len(labels)
    assert sorted(np.concatenate(test).tolist()) == list(range(n))                    # disjoint and covering
    for i in range(folds):
        assert test[i].dtype == np.int64 and np.array_equal(test[i], np.sort(test[i]))
        assert np.array_equal(val[i], test[i - 1])
        tr, te, va = set(train[i].tolist()), set(test[i].tolist()), set(val[i].tolist())
        assert not (tr & te) and not (tr & va) and not (te & va)
        assert tr | te | va == set(range(n))
    return train, test, val


def test_k_fold_150():
    from esc_gnn_amd.datasets import csl_k_fold
    labels = np.repeat(np.arange(10), 15)
    train, test, val = _check_folds(labels)
    for i in range(10):
        assert len(test[i]) == 15 and len(train[i]) == 120
        per_class = np.bincount(labels[test[i]], minlength=10)
        assert set(per_class.tolist()) <= {1, 2} and per_class.sum() == 15
    again = csl_k_fold(labels)
    assert all(np.array_equal(a, b) for a, b in zip(test, again[1]))
    assert any(not np.array_equal(a, b) for a, b in zip(test, csl_k_fold(labels, seed=1)[1]))     # shuffled by the seed
    with pytest.raises(ValueError):
        csl_k_fold(np.repeat(np.arange(10), 5))


def test_k_fold_ten_copies():
    labels = np.repeat(np.arange(10), 10)
    train, test, val = _check_folds(labels)
    for i in range(10):
        assert np.array_equal(np.bincount(labels[test[i]], minlength=10), np.ones(10, dtype=np.int64))
        assert len(train[i]) == 80


@pytest.mark.parametrize("copies", [15, 10, 13])
def test_k_fold_has_scikit_learn_sizes(copies):
    skm = pytest.importorskip("sklearn.model_selection")
    from esc_gnn_amd.datasets import csl_k_fold
    labels = np.repeat(np.arange(10), copies)
    _, test, _ = csl_k_fold(labels)
    skf = skm.StratifiedKFold(10, shuffle=True, random_state=12345)
    ref = [idx for _, idx in skf.split(np.zeros(len(labels)), labels)]
    for mine, theirs in zip(test, ref):
        assert len(mine) == len(theirs)
        assert np.array_equal(np.bincount(labels[mine], minlength=10), np.bincount(labels[theirs], minlength=10))


def test_oracle_reproduces_the_golden(golden, fixture_features):
    torch.set_num_threads(1)
    z = golden
    assert int(z["h"]) == 4 and (int(z["layers"]), int(z["hidden"])) == (3, 32)
    graphs = fixture_features
    assert np.array_equal(co.graph_digests(graphs), z["digests"])
    assert [int(g.y) for g in graphs] == z["labels"].tolist()
    m = co.csl_oracle_from_recipe(z).eval()
    assert list(m.state_dict().keys()) == [str(k) for k in z["keys"]]
    args = co.collate(graphs)
    with torch.no_grad():
        p32 = m(*args)
        p64 = copy.deepcopy(m).double()(args[0].double(), *args[1:])
    assert p32.shape == (20, 10)
    assert np.array_equal(p32.numpy(), z["pred32"]) and np.array_equal(p64.numpy(), z["pred64"])
    err32 = float((p32.double() - p64).abs().max())
    assert err32 == float(z["err32"])
    d64 = co.distance_matrix(p64)
    assert d64.shape == (20, 20) and np.array_equal(d64.numpy(), z["dist64"])
    # the margin the generator asserted: an error of tol per element cannot blur the verdict
    tol = 3.0 * err32 + 1e-5 * float(p64.abs().max())
    cross, same = co.class_distances(p64)
    assert cross / 2 > 2.0 * 10 ** 0.5 * tol and same < tol
    # the training step on the 20 graphs with the recorded dropout multiplier
    m = co.csl_oracle_from_recipe(z).train()
    out = m(*args, drop=torch.tensor(z["drop"]))
    loss = torch.nn.functional.cross_entropy(out, torch.tensor(z["labels"]))
    loss.backward()
    assert np.array_equal(out.detach().numpy(), z["train_out"]) and np.array_equal(loss.detach().numpy(), z["train_loss"])
    no_grad = [str(k) for k in z["no_grad"]]
    assert no_grad and all(k.startswith("z_embedding.") for k in no_grad)        # built, never applied (run_csl.py:194-222)
    for k, p in m.named_parameters():
        if k in no_grad:
            assert p.grad is None, k
        else:
            assert np.array_equal(co.grad_digest(p.grad), z["gsum/" + k]), k
    assert all(not k.endswith(".eps") for k, _ in m.named_parameters())          # eps is a buffer: no gradient


def test_driver_flags_match_the_reference(golden):
    from esc_gnn_amd import run_csl
    want = json.loads(str(golden["flags_json"]))
    assert want == dict(model="GIN", h=4, layers=5, width=128, epochs=500, dataset="CSL", learnRate=0.001)
    args = vars(run_csl.build_parser().parse_args([]))
    assert {k: args[k] for k in want} == want
    assert set(args) - set(want) == {"seed", "splits", "copies", "data_seed"}
    assert (args["seed"], args["splits"], args["copies"], args["data_seed"]) == (None, 10, 15, 0)
    assert run_csl.BATCH == 64
    with pytest.raises(NotImplementedError):
        run_csl.main(["--model", "GCN"])


def test_elu_module_keeps_the_torch_layout():
    import esc_gnn_amd as E
    m = E.nn.ELU()
    assert isinstance(m, torch.nn.ELU) and m.alpha == 1.0 and not list(m.state_dict())
    with pytest.raises(ValueError):
        E.nn.ELU(alpha=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ops.elu(torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ops.act(torch.zeros(2, 3), "relu")
    with pytest.raises(ValueError):
        E.ops.act(torch.zeros(2, 3), "gelu")
    from esc_gnn_amd.csl_models import NestedGIN
    net = NestedGIN(3, 32)
    ref = co.NestedGINCslRef(3, 32)
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    assert [type(c).__name__ for c in net.conv1.nn] == ["Linear", "ELU", "Linear", "ELU"]
    assert [type(c).__name__ for c in net.z_embedding] == ["BatchNorm1d", "AbsorbedELU", "Linear", "BatchNorm1d", "AbsorbedELU"]
    assert net.lin2.out_features == 10 and net.conv1.nn[0].in_features == 1
