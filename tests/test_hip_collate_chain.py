"""The collate chain on the step's end: one staged block + one copy, the column counts, ONE fill kernel over the store's
compact int32 views (csrc/collate.hip), and the BatchNorm step counters incremented inside the engine's own first launch.
Everything is integer gather work, so every comparison is torch.equal against the host oracles
(`Batch.from_data_list`, `BatchPlan.from_tensors`) — no tolerance anywhere."""
import os

import pytest
import torch

from conftest import load_collate, require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAGS = ["count3", "mixed4", "zinc3", "molhiv4"]
# the store views this file's change added (an older cache blob has none of them)
NEW_KEYS = ("in_ptr32", "out_ptr32", "in_edge32", "in_src32", "out_edge32", "out_dst32", "row_ptr32",
            "c_col32", "c_row32", "c_val32", "esrc32", "edst32", "pos_enc32", "pos_index32", "pos_batch32")


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


_cache = {}


def _store(E, tag):
    if tag not in _cache:
        graphs, _, _ = load_collate(tag)
        datas = [E.Data(**{k: torch.tensor(v) for k, v in g.items()}) for g in graphs]
        _cache[tag] = (E.DeviceGraphStore(datas, DEV), datas)
    return _cache[tag]


def _check(E, got, datas, ids):
    """every batch key (value, dtype, shape), every plan array and graph_ptr of a collated batch against the oracles"""
    want = E.Batch.from_data_list([datas[i] for i in ids])
    assert sorted(got.keys) == sorted(want.keys), ids
    for k in want.keys:
        g = got[k].cpu()
        assert g.dtype == want[k].dtype, (k, len(ids))
        assert tuple(g.shape) == tuple(want[k].shape), (k, len(ids))
        assert torch.equal(g, want[k]), (k, len(ids))
    assert got.num_graphs == len(ids)
    plan = got.__dict__["_esc_plan"]
    ref = E.BatchPlan.from_tensors(got.edge_index, got.x.size(0), got.pos_enc, got.pos_index, got.pos_batch)
    for f in E.BatchPlan.FIELDS:
        a, b = getattr(plan, f), getattr(ref, f)
        assert a.dtype == b.dtype and torch.equal(a, b), (f, len(ids))
    nodes = [0]
    for i in ids:
        nodes.append(nodes[-1] + datas[i].x.size(0))
    assert plan.graph_ptr.dtype == torch.int32 and plan.graph_ptr.cpu().tolist() == nodes, len(ids)


@pytest.mark.parametrize("B", [1, 64, 65, 130])
@pytest.mark.parametrize("tag", TAGS)
def test_batch_lengths_and_repeats(E, tag, B):
    """lengths around the 64-graph chunk of the column count; repeated ids make the column prefix a function of the
    batch POSITION, and the running offsets give the bag slices every destination / source alignment"""
    store, datas = _store(E, tag)
    G = len(datas)
    ids = [(7 * i) % G for i in range(B)]
    _check(E, store.collate(ids), datas, ids)


def test_back_to_back_collates(E):
    """eight collates with no synchronisation in between: a later call's staging must not disturb an earlier one's"""
    store, datas = _store(E, "mixed4")
    lists = [[0], [3, 2, 1, 0], [1] * 9, [(5 * i + 1) % 4 for i in range(70)], [2, 2, 3], [(3 * i) % 4 for i in range(33)],
             [0, 1, 2, 3] * 4, [3]]
    got = [store.collate(ids) for ids in lists]
    torch.cuda.synchronize()
    for ids, b in zip(lists, got):
        _check(E, b, datas, ids)


def test_old_cache_rebuilds_the_views(E, tmp_path):
    store, datas = _store(E, "zinc3")
    path, old = os.path.join(tmp_path, "new.pt"), os.path.join(tmp_path, "old.pt")
    store.save(path)
    blob = torch.load(path, map_location="cpu", weights_only=True)
    dropped = [k for k in NEW_KEYS if k in blob]
    assert len(dropped) == len(NEW_KEYS), sorted(set(NEW_KEYS) - set(dropped))      # save() writes every view
    for k in dropped:
        del blob[k]
    torch.save(blob, old)
    ids = [2, 0, 1, 1, 2]
    for p in (path, old):
        again = E.DeviceGraphStore.load(p, DEV)
        a, b = store.collate(ids), again.collate(ids)
        for k in a.keys:
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), (p, k)
        pa, pb = a.__dict__["_esc_plan"], b.__dict__["_esc_plan"]
        for f in E.BatchPlan.FIELDS:
            assert torch.equal(getattr(pa, f), getattr(pb, f)), (p, f)
        assert torch.equal(pa.graph_ptr, pb.graph_ptr)
        _check(E, b, datas, ids)


def test_wide_integers_stay_exact(E):
    """a pos_enc value beyond int32: the reference-visible int64 outputs keep every bit (the store falls back to its int64
    array for that output), the int32 plan keeps the (int) conversion"""
    big = 2 ** 40
    g0 = E.Data(x=torch.ones(3, 10), edge_index=torch.tensor([[0, 1, 2, 2], [1, 2, 0, 1]]), y=torch.zeros(3),
                pos_enc=torch.tensor([1, big, 3, -2, 5, 7, big + 5]), pos_index=torch.tensor([4, 4, 9, 0, 1799, 4, 9]),
                pos_batch=torch.tensor([0, 0, 1, 2, 2, 3, 3]))
    g1 = E.Data(x=torch.ones(2, 10), edge_index=torch.tensor([[0, 1, 1], [1, 0, 1]]), y=torch.zeros(2),
                pos_enc=torch.tensor([6, 2, 2, 9]), pos_index=torch.tensor([9, 4, 0, 9]),
                pos_batch=torch.tensor([0, 1, 1, 2]))
    datas = [g0, g1]
    store = E.DeviceGraphStore(datas, DEV)
    assert store.pos_enc32 is None and store.pos_batch32 is not None
    for ids in ([0, 1], [1, 0, 0], [1, 1, 0, 1, 0]):
        b = store.collate(ids)
        want = E.Batch.from_data_list([datas[i] for i in ids])
        for k in ("pos_enc", "pos_index", "pos_batch", "edge_index"):
            assert b[k].dtype == torch.int64 and torch.equal(b[k].cpu(), want[k]), (ids, k)
        assert int(b.pos_enc.max()) == big + 5
        _check(E, b, datas, ids)


def test_batchnorm_step_counters(E):
    """exactly one increment per BatchNorm per TRAINING forward, made by the engine itself: begin/end_step, train_step and
    the module as an autograd node; none by predict; the same on one stream"""
    from esc_gnn_amd import _native as nv
    store, datas = _store(E, "mixed4")
    try:
        for mode in (2, 0):
            nv.call("esc_engine_set_side_stream", mode)
            nv.call("esc_engine_set_two_stream_min_edges", 0)
            torch.manual_seed(0)
            m = E.NestedGIN_eff(None, 2, 32, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True).to(DEV).train()
            counters = [mod.num_batches_tracked for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm1d)]
            assert len(counters) == 2 + 2 + 2 * 2 + 1

            def expect(n):
                assert all(c.dtype == torch.int64 and int(c) == n for c in counters), (mode, n, [int(c) for c in counters])
            expect(0)
            opt = E.optim.FlatAdam(m.parameters(), lr=1e-3)
            eng = E.StepEngine(m)
            b = store.collate([0, 1, 2, 3])
            for _ in range(3):
                eng.begin_step(b)
                nxt = store.collate([3, 1])
                eng.end_step()
                opt.step()
            expect(3)
            for _ in range(3):
                eng.train_step(nxt)
            expect(6)
            eng.predict(b)
            expect(6)
            pred = m(b)                                      # training-mode module = one autograd node on the engine
            assert type(pred.grad_fn).__name__.startswith("_EngineNode")
            expect(7)
            pred.sum().backward()
            expect(7)
            m.eval()
            with torch.no_grad():
                m(b)
            expect(7)
    finally:
        nv.call("esc_engine_set_side_stream", 2)
        nv.call("esc_engine_set_two_stream_min_edges", 12000)
