"""The three step-engine families (counting, ZINC, OGB) share one host path: what that path must keep per family — who
increments the BatchNorm step counters and when, when the OGB dropout stream advances, that a spent workspace refuses a
second backward, and that `model(batch)` is the one engine node."""
import pytest
import torch

from conftest import require_gpu

DEV = "cuda:0"


def _family(kind, seed=5):
    """a fresh seeded model of the family, its engine class and two 16-graph batches (32 synthetic graphs, 2 layers)"""
    import esc_gnn_amd as E
    from esc_gnn_amd.datasets import (build_count_dataset, build_feature_dataset, synthetic_ogbmol_graphs,
                                      synthetic_zinc_graphs)
    torch.manual_seed(seed)
    if kind == "ogb":
        from esc_gnn_amd.engine import OgbStepEngine as Eng
        from esc_gnn_amd.ogb_mol_gnn import GNN
        graphs = build_feature_dataset(synthetic_ogbmol_graphs(0, 32), 2, use_rd=True, self_loop=True)
        model = GNN("ogbg-molhiv", 1, num_layer=2, emb_dim=32, gnn_type="gin_eff", virtual_node=True, residual=True,
                    drop_ratio=0.3, use_rd=True)
    elif kind == "zinc":
        from esc_gnn_amd.engine import ZincStepEngine as Eng
        from esc_gnn_amd.zinc_models import NestedGIN_eff
        graphs = build_feature_dataset(synthetic_zinc_graphs(0, 32), 2, use_rd=True, self_loop=False)
        model = NestedGIN_eff(None, num_layers=2)
    else:
        from esc_gnn_amd.engine import StepEngine as Eng
        graphs = build_count_dataset(0, 32, h=2)
        model = E.NestedGIN_eff(None, 2, 64, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True)
    store = E.DeviceGraphStore(graphs, torch.device(DEV))
    return model.to(DEV).train(), Eng, [store.collate(torch.arange(16) + 16 * i) for i in range(2)]


def _counters(model):
    cs = [m.num_batches_tracked for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert len(cs) >= 1
    return cs


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zinc", "ogb"])
def test_batchnorm_step_counters_and_dropout_stream(kind):
    """one increment per BatchNorm per TRAINING call (train_step, the module as an autograd node), none by predict, the
    backward or an eval forward; the OGB dropout stream advances with exactly the training calls, not with prepare"""
    require_gpu()
    model, Eng, (b, _) = _family(kind)
    counters = _counters(model)

    def expect(n):
        assert all(int(c) == n for c in counters), (n, [int(c) for c in counters])
    expect(0)
    eng = Eng(model)
    for _ in range(2):
        eng.train_step(b)
    expect(2)
    eng.predict(b)
    expect(2)
    pred = model(b)
    assert type(pred.grad_fn).__name__.startswith("_EngineNode")
    expect(3)
    pred.sum().backward()
    expect(3)
    model.eval()
    with torch.no_grad():
        model(b)
    expect(3)
    eng.prepare(b)
    expect(3)
    if kind == "ogb":
        assert model.__dict__["_esc_drop_step"] == 3
    else:
        assert "_esc_drop_step" not in model.__dict__


@pytest.mark.gpu
@pytest.mark.parametrize("extra", ["prepare", "predict"])
def test_ogb_dropout_stream_ignores_prepare_and_predict(extra):
    """two identically seeded models, one stepped with `extra` calls interleaved: bit-equal losses (dropout 0.3: a seed
    consumed by prepare / predict would shift every later mask)"""
    require_gpu()
    import esc_gnn_amd as E
    losses = []
    for interleave in (False, True):
        model, Eng, batches = _family("ogb", seed=7)
        eng = Eng(model)
        opt = E.optim.FlatAdam(model.parameters(), lr=1e-3)
        run = []
        for i in range(4):
            b = batches[i % 2]
            if interleave:
                getattr(eng, extra)(b)
            run.append(eng.train_step(b))
            opt.step()
        assert model.__dict__["_esc_drop_step"] == 4
        losses.append(torch.stack(run).cpu())
    assert torch.equal(losses[0], losses[1]), (losses[0] - losses[1]).abs().max()
    assert len(set(losses[0].tolist())) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["count", "zinc", "ogb"])
def test_one_node_class_and_second_backward_refused(kind):
    """`model(batch)` in training mode is the one engine node for every family; its workspace is released by the first
    backward, so a second one through the same forward is refused on the host, before any native call"""
    require_gpu()
    model, _, (b, _) = _family(kind)
    pred = model(b)
    assert type(pred.grad_fn).__name__.startswith("_EngineNode")
    pred.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="workspace was released"):
        pred.sum().backward()


@pytest.fixture
def schedule_knobs():
    """always back to the library's defaults, whatever the test set"""
    from esc_gnn_amd import _native as nv
    yield nv
    nv.call("esc_engine_set_side_stream", 2)
    nv.call("esc_engine_set_two_stream_min_edges", 12000)


@pytest.mark.gpu
@pytest.mark.parametrize("live,with_retired", [(2, 2 | 1 | 4 | 8 | 16 | 32), (0, 61)], ids=["two_streams", "one_stream"])
def test_retired_setter_bits_are_inert(schedule_knobs, live, with_retired):
    """esc_engine_set_side_stream honours bit 1 (edge stream) and bit 6 (event records) only: bits 0, 2, 3, 4 and 5 selected
    schedules that no longer exist.  Two train_steps from the same seed with and without them: loss, predictions and every
    parameter gradient are bitwise equal.  Smallest counting shape on which every live fusion runs: L = 3 (batched edge
    GEMM), H = 64 (node activations applied by their consumers), batches of 3 graphs, second stream forced on."""
    require_gpu()
    import esc_gnn_amd as E
    from esc_gnn_amd.datasets import build_count_dataset
    nv = schedule_knobs
    bs, L, H = 3, 3, 64
    graphs = build_count_dataset(100, 2 * bs, h=3, use_rd=True, self_loop=True)
    gen = torch.Generator().manual_seed(bs)
    for g in graphs:
        g.x = torch.randn(g.x.shape, generator=gen)
        g.y = torch.randn(g.x.size(0), generator=gen)
    store = E.DeviceGraphStore(graphs, torch.device(DEV))
    batches = [store.collate(torch.arange(bs) + bs * i) for i in range(2)]

    def run(mode):
        nv.call("esc_engine_set_side_stream", mode)
        nv.call("esc_engine_set_two_stream_min_edges", 0)
        torch.manual_seed(0)
        m = E.NestedGIN_eff(None, L, H, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True).to(DEV)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.01 * torch.randn_like(p))
        eng = E.StepEngine(m.train())
        out = []
        for b in batches:
            loss, pred = eng.train_step(b, return_pred=True)
            out.append((loss.clone(), pred.clone(), [p.grad.clone() for p in m.parameters()]))
        torch.cuda.synchronize()
        return out

    ref, got = run(live), run(with_retired)
    for i, ((lr, pr, gr), (lg, pg, gg)) in enumerate(zip(ref, got)):
        assert bool(torch.isfinite(lr)) and bool(torch.isfinite(pr).all()), i
        assert len(gr) == len(gg) and any(float(g.abs().max()) > 0.0 for g in gr), i
        assert torch.equal(lr, lg), (i, float(lr), float(lg))
        assert torch.equal(pr, pg), (i, int((pr != pg).sum()))
        for k, (a, c) in enumerate(zip(gr, gg)):
            assert torch.equal(a, c), (i, k, int((a != c).sum()))
