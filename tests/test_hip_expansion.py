"""The typed size tag of the device-expanding stores (esc_gnn_amd/expansion.py) on the MI355X: a store expands the batches it
collated exactly as the expansion without `sizes` does, and refuses on the host, before any library call, a batch whose sizes
were counted by another kind of store or for another h; make_multihop_edges ignores sizes counted for another k."""
import numpy as np
import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = ([0, 1], [0, 1, 2])     # [G, 3] sizes read as [-1, 2]: three rows for two graphs; for three graphs no reshape at all


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _graph(E, n, pairs):
    ei = np.array([[a for a, b in pairs] + [b for a, b in pairs], [b for a, b in pairs] + [a for a, b in pairs]], dtype=np.int64)
    ei = torch.as_tensor(ei).reshape(2, -1)
    return E.Data(x=torch.arange(n), edge_index=ei, edge_attr=torch.arange(ei.size(1)) % 4, y=torch.zeros(1), num_nodes=n)


@pytest.fixture(scope="module")
def graphs(E):
    return [_graph(E, 3, [(0, 1), (1, 2), (2, 0)]), _graph(E, 4, [(0, 1), (1, 2), (2, 3)]), _graph(E, 1, [])]   # triangle, path, node


@pytest.fixture(scope="module")
def stores(E, graphs):
    from esc_gnn_amd.multihop import MultihopGraphStore
    from esc_gnn_amd.subgraphs import PlainGraphStore
    from esc_gnn_amd.subgraphs2 import I2GraphStore
    return dict(plain1=PlainGraphStore(graphs, 1, DEV), plain2=PlainGraphStore(graphs, 2, DEV),
                i2=I2GraphStore(graphs, 1, use_rd=False, device=DEV), mh2=MultihopGraphStore(graphs, 2, DEV))


SUB_KEYS = ("x", "z", "edge_index", "edge_attr", "node_to_subgraph", "subgraph_to_graph", "batch", "orig_node", "orig_edge",
            "sub_node_ptr", "sub_edge_ptr", "status")
SUB2_KEYS = ("x", "z", "edge_index", "edge_attr", "node_to_subgraph2", "subgraph2_to_subgraph", "subgraph_to_graph",
             "node_to_original_node", "batch", "center_idx", "orig_node", "orig_edge", "s2_node_ptr", "sub2_ptr", "sub_node_ptr",
             "sub_edge_ptr", "status")
PLAN_KEYS = ("row", "col", "distance", "out_ptr", "meta", "in_ptr", "in_meta", "status")


def _same_integers(got, want, keys, what):
    for k in keys:
        a, b = getattr(got, k), getattr(want, k)
        assert not a.dtype.is_floating_point and a.dtype == b.dtype and torch.equal(a, b), (what, k)


@pytest.mark.parametrize("ids", BATCHES)
def test_every_store_expands_its_own_batch_as_the_expansion_without_sizes(E, graphs, stores, ids):
    from esc_gnn_amd.multihop import expand_multihop
    from esc_gnn_amd.subgraphs import collate_graphs, expand_subgraphs
    from esc_gnn_amd.subgraphs2 import expand_subgraphs2
    def plain():                                                       # no tag: the totals are read back
        return collate_graphs([graphs[i] for i in ids], DEV)
    for name, h in (("plain1", 1), ("plain2", 2)):
        got, want = stores[name].expand(stores[name].collate(ids)), expand_subgraphs(plain(), h)
        _same_integers(got, want, SUB_KEYS, name)
        assert got.num_subgraphs == want.num_subgraphs and got.num_nodes == want.num_nodes
    got, want = stores["i2"].expand(stores["i2"].collate(ids)), expand_subgraphs2(plain(), 1)
    _same_integers(got, want, SUB2_KEYS, "i2")
    assert (got.num_subgraphs, got.num_subgraphs2, got.num_nodes) == (want.num_subgraphs, want.num_subgraphs2, want.num_nodes)
    out = stores["mh2"].expand(stores["mh2"].collate(ids))
    mei, dist, plan = expand_multihop(plain(), 2)
    assert torch.equal(out.multihop_edge_index, mei) and torch.equal(out.distance, dist)
    _same_integers(out.multihop_edge_index._esc_multihop_plan, plan, PLAN_KEYS, "mh2")
    assert out.multihop_edge_index._esc_multihop_plan.counts == torch.bincount(dist, minlength=3).tolist()


def _refused(monkeypatch, E, store, batch, *names):
    """store.expand(batch) raises a ValueError that holds every one of `names`, and raises it before any library call"""
    def no_call(*a, **kw):
        raise AssertionError("the library was called")
    with monkeypatch.context() as m:
        m.setattr(E._native, "call", no_call)
        with pytest.raises(ValueError) as err:
            store.expand(batch)
    for name in names:
        assert name in str(err.value), (name, str(err.value))


@pytest.mark.parametrize("ids", BATCHES)
def test_a_store_refuses_sizes_counted_for_another_h(E, stores, ids, monkeypatch):
    _refused(monkeypatch, E, stores["plain2"], stores["plain1"].collate(ids), "h=1", "h=2")
    _refused(monkeypatch, E, stores["plain1"], stores["plain2"].collate(ids), "h=2", "h=1")


@pytest.mark.parametrize("ids", BATCHES)
def test_a_store_refuses_sizes_counted_by_another_kind_of_store(E, stores, ids, monkeypatch):
    _refused(monkeypatch, E, stores["plain1"], stores["i2"].collate(ids), "'subgraph2'", "'subgraph'")      # the same h = 1
    _refused(monkeypatch, E, stores["i2"], stores["plain1"].collate(ids), "'subgraph'", "'subgraph2'")
    _refused(monkeypatch, E, stores["mh2"], stores["plain2"].collate(ids), "'subgraph'", "'multihop'", "h=2", "k=2")
    _refused(monkeypatch, E, stores["plain2"], stores["mh2"].collate(ids), "'multihop'", "'subgraph'", "k=2", "h=2")


@pytest.mark.parametrize("ids", BATCHES)
def test_make_multihop_edges_ignores_sizes_counted_for_another_k(E, graphs, stores, ids):
    from esc_gnn_amd.multihop import expand_multihop, make_multihop_edges
    from esc_gnn_amd.subgraphs import collate_graphs
    out = make_multihop_edges(stores["mh2"].collate(ids), 3)
    mei, dist, _ = expand_multihop(collate_graphs([graphs[i] for i in ids], DEV), 3)
    assert torch.equal(out.multihop_edge_index, mei) and torch.equal(out.distance, dist) and int(dist.max()) == 3
