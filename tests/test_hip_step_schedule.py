"""The two-stream training step signals its cross-stream dependencies on single kernels (edge terms, the head in front of
the loss, d_e of every aggregate backward) through the stop event of the producing launch (esc_engine_set_side_stream bit 6
clear, the default) instead of a hipEventRecord behind it (bit 6 set, the schedule before).  Every kernel keeps its stream,
its arguments and its arithmetic, so the two must agree bit for bit — a dependency that came loose would show here — and the
node-pipeline gradients must still be complete in node-stream order when begin_step returns (a multi-rank step all-reduces
them there)."""
import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OLD, NEW = 64 | 2, 2          # esc_engine_set_side_stream: edge stream on, bit 6 = dependencies as event records


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


@pytest.fixture
def knobs():
    """always back to the library's defaults, whatever a test set"""
    from esc_gnn_amd import _native as nv
    yield nv
    nv.call("esc_engine_set_side_stream", NEW)
    nv.call("esc_engine_set_two_stream_min_edges", 12000)


_stores = {}


def _store(E, bs, full):
    """`full`: the flagship's batches (h=3, two batches of `bs` graphs, targets standardised); otherwise small random ones"""
    key = (bs, full)
    if key not in _stores:
        from esc_gnn_amd.datasets import build_count_dataset
        if full:
            graphs = build_count_dataset(0, 2 * bs, h=3, use_rd=True, self_loop=True)
            y = torch.cat([g.y.view(-1) for g in graphs])
            for g in graphs:
                g.y = (g.y.view(-1) - y.mean()) / y.std()
        else:
            graphs = build_count_dataset(100, 2 * bs, h=3, use_rd=True, self_loop=True)
            gen = torch.Generator().manual_seed(bs)
            for g in graphs:
                g.x = torch.randn(g.x.shape, generator=gen)
                g.y = torch.randn(g.x.size(0), generator=gen)
        _stores[key] = E.DeviceGraphStore(graphs, DEV)
    return _stores[key]


def _model(E, L, H):
    torch.manual_seed(0)
    m = E.NestedGIN_eff(None, L, H, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True).to(DEV)
    with torch.no_grad():                        # x = ones makes the x_embedding BatchNorms degenerate: perturb the input path
        for p in m.parameters():
            p.add_(0.01 * torch.randn_like(p))
    return m.train()


def _engine_steps(E, nv, store, bs, L, H, mode, min_edges):
    nv.call("esc_engine_set_side_stream", mode)
    nv.call("esc_engine_set_two_stream_min_edges", min_edges)
    ids = [torch.arange(0, bs), torch.arange(bs, 2 * bs)]
    m = _model(E, L, H)
    opt = E.optim.FlatAdam(m.parameters(), lr=1e-3)
    eng = E.StepEngine(m)
    nxt, out = store.collate(ids[0]), []
    edges = E.plan_of(nxt).num_edges
    for i in range(3):
        b = nxt
        loss = eng.begin_step(b)
        nxt = store.collate(ids[(i + 1) % 2])
        eng.end_step()
        grad = opt.flat_grad.clone()
        opt.step()
        out.append((loss.clone(), grad, opt.flat_param.clone(), [t.clone() for t in m.buffers()]))
    torch.cuda.synchronize()
    return out, edges


@pytest.mark.parametrize("L,H,bs,full", [(4, 256, 128, True), (2, 64, 17, False), (1, 32, 3, False)],
                         ids=["cfg1_L4_H256_bs128", "L2_H64_bs17", "L1_H32_bs3"])
def test_old_and_new_schedule_agree_bitwise(E, knobs, L, H, bs, full):
    """Three consecutive steps (begin_step -> next collate -> end_step -> FlatAdam.step) from the same seed under both
    schedules: losses, flat_grad, flat_param and every BatchNorm buffer are torch.equal after every step."""
    store = _store(E, bs, full)
    min_edges = 12000 if full else 0
    old, edges = _engine_steps(E, knobs, store, bs, L, H, OLD, min_edges)
    new, _ = _engine_steps(E, knobs, store, bs, L, H, NEW, min_edges)
    if full:
        assert edges >= 12000, edges                # two streams by the library's own threshold
    for i, ((lo, go, po, bo), (ln, gn, pn, bn)) in enumerate(zip(old, new)):
        assert bool(torch.isfinite(lo).all()) and bool(torch.isfinite(go).all()), i
        assert float(go.abs().max()) > 0.0, i
        assert torch.equal(lo, ln), (i, float(lo), float(ln))
        assert torch.equal(go, gn), (i, int((go != gn).sum()))
        assert torch.equal(po, pn), (i, int((po != pn).sum()))
        assert len(bo) == len(bn) and all(torch.equal(a, c) for a, c in zip(bo, bn)), i


def _autograd_steps(E, nv, store, bs, L, H, mode, min_edges):
    nv.call("esc_engine_set_side_stream", mode)
    nv.call("esc_engine_set_two_stream_min_edges", min_edges)
    m = _model(E, L, H)
    b = store.collate(torch.arange(bs))
    out = []
    for _ in range(2):                                           # twice: event / scratch reuse across steps
        m.zero_grad(set_to_none=True)
        pred = m(b)
        assert pred.grad_fn is not None and type(pred.grad_fn).__name__.startswith("_EngineNode")
        loss = torch.nn.L1Loss()(pred, b.y.view(-1, 1))
        loss.backward()
        out.append((pred.detach().clone(), loss.detach().clone(), [p.grad.clone() for p in m.parameters()],
                    [t.clone() for t in m.buffers()]))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("L,H,bs,full", [(4, 256, 128, True), (2, 64, 17, False), (1, 32, 3, False)],
                         ids=["cfg1_L4_H256_bs128", "L2_H64_bs17", "L1_H32_bs3"])
def test_module_as_autograd_node_agrees_bitwise(E, knobs, L, H, bs, full):
    """`model(batch)` + a torch loss + backward() (esc_engine_forward_train / esc_engine_backward) under both schedules."""
    store = _store(E, bs, full)
    min_edges = 12000 if full else 0
    old = _autograd_steps(E, knobs, store, bs, L, H, OLD, min_edges)
    new = _autograd_steps(E, knobs, store, bs, L, H, NEW, min_edges)
    for i, ((po, lo, go, bo), (pn, ln, gn, bn)) in enumerate(zip(old, new)):
        assert bool(torch.isfinite(po).all()), i
        assert torch.equal(po, pn) and torch.equal(lo, ln), i
        assert len(go) == len(gn) and all(torch.equal(a, c) for a, c in zip(go, gn)), i
        assert len(bo) == len(bn) and all(torch.equal(a, c) for a, c in zip(bo, bn)), i


@pytest.mark.parametrize("mode", [NEW, OLD], ids=["new", "old"])
def test_node_bucket_is_complete_when_begin_step_returns(E, knobs, mode):
    """What a multi-rank step relies on: everything outside the edge-pipeline parameters may be read on the current stream as
    soon as begin_step has returned.  Clones queued there equal the gradients after end_step bit for bit."""
    bs, L, H = 128, 4, 256
    store = _store(E, bs, True)
    knobs.call("esc_engine_set_side_stream", mode)
    ids = [torch.arange(0, bs), torch.arange(bs, 2 * bs)]
    m = _model(E, L, H)
    opt = E.optim.FlatAdam(m.parameters(), lr=1e-3)
    eng = E.StepEngine(m)
    late = set(id(p) for p in E.parallel.edge_pipeline_parameters(m))
    early = [(n, p) for n, p in m.named_parameters() if id(p) not in late]
    assert late and len(early) > len(late)
    nxt = store.collate(ids[0])
    for i in range(4):
        b = nxt
        eng.begin_step(b)
        seen = [p.grad.clone() for _, p in early]
        nxt = store.collate(ids[(i + 1) % 2])
        eng.end_step()
        torch.cuda.synchronize()
        for (n, p), g in zip(early, seen):
            assert torch.equal(p.grad, g), (i, n)
            assert bool(torch.isfinite(g).all()), (i, n)
        opt.step()
