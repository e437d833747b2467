"""The boundary between two training steps of the counting engine (*Step engine, step boundary*;
include/escgnn_step.h).  By default the edge stream runs its last slab reduce itself, FlatAdam.step() updates the optimiser's
late bucket there and the rest beside it on the caller's stream, and a step whose batch was collated between the two halves of
the step before starts its edge pipeline in edge-stream order (the fast seam).  Bit 8 of esc_engine_set_side_stream restores the
former boundary: last reduce and one Adam launch on the caller's stream, every step behind the z_ready record.  Same kernels, same
element order, other streams: everything a step leaves must agree with the former boundary BIT FOR BIT — a dependency that came
loose at the seam (a workspace array overwritten while the step before still reads it, a parameter read before its update, a
gradient updated before it is complete) would move data here.  Two alternating batches of different size, so that the two steps'
workspace layouts differ, and two streams forced for these small batches."""
import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEGACY, NEW = 256 | 2, 2      # esc_engine_set_side_stream: edge stream on; bit 8 = the former step boundary
STEPS = 6
SIZES = (6, 11)               # graphs of the two alternating batches


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


@pytest.fixture
def knobs():
    """two streams whatever the batch size; always back to the library's defaults"""
    from esc_gnn_amd import _native as nv
    nv.call("esc_engine_set_two_stream_min_edges", 0)
    yield nv
    nv.call("esc_engine_set_side_stream", NEW)
    nv.call("esc_engine_set_two_stream_min_edges", 12000)


_cache = {}


def _store(E):
    if "store" not in _cache:
        from esc_gnn_amd.datasets import build_count_dataset
        graphs = build_count_dataset(100, sum(SIZES), h=3, use_rd=True, self_loop=True)
        gen = torch.Generator().manual_seed(7)
        for g in graphs:
            g.x = torch.randn(g.x.shape, generator=gen)
            g.y = torch.randn(g.x.size(0), generator=gen)
        _cache["store"] = E.DeviceGraphStore(graphs, DEV)
    return _cache["store"]


def _ids(i):
    """the larger batch first: the engine's workspace is then allocated once (a step on a new workspace declines the fast seam)"""
    return torch.arange(SIZES[0], sum(SIZES)) if i % 2 == 0 else torch.arange(0, SIZES[0])


def _model(E, L, H):
    torch.manual_seed(0)
    m = E.NestedGIN_eff(None, L, H, use_rd=True, graph_pred=False, dropout=0, edge_nest=True, use_cycle=True).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.01 * torch.randn_like(p))
    return m.train()


def _counts(nv):
    h = nv.lib()
    return int(h.esc_engine_seam_count(0)), int(h.esc_engine_seam_count(1))


def _run(E, nv, L, H, mode, pattern):
    """STEPS steps from the same seed.  pattern: "between" (bench.py's: the next collate between begin_step and end_step),
    "after" (the batch collated after opt.step()), "denom" (step(grad_denom=1)), "decay" (weight_decay > 0), "one_call"
    (engine.train_step), "predict" (an eval forward in front of every other step); torch ops of the caller between end_step() and
    opt.step(): "clip" (clip_grad_norm_), "scale" (flat_grad.mul_), "clamp" (a late parameter clamped in place); and one between
    opt.step() and begin_step(): "edit_after" (a late parameter scaled in place).  Per step: the loss, flat_grad cloned on the
    caller's stream right behind end_step, an early and a late parameter cloned right behind opt.step(), then the whole state.
    Returns the records and how many fast seams / split optimiser steps the library counted."""
    key = (L, H, mode, pattern)
    if key in _cache:
        return _cache[key]
    store = _store(E)
    nv.call("esc_engine_set_side_stream", mode)
    m = _model(E, L, H)
    late = E.parallel.edge_pipeline_parameters(m)
    opt = E.optim.FlatAdam(m.parameters(), lr=1e-3, late=late, weight_decay=0.01 if pattern == "decay" else 0.0)
    assert 0 < opt.early_numel < opt.numel
    p_early, p_late = m.lin1.weight, m.z_embedding[3].weight
    assert any(p_late is q for q in late) and not any(p_early is q for q in late)
    eng = E.StepEngine(m)
    one = torch.ones(1, device=DEV)
    seams0, splits0 = _counts(nv)
    out = []
    nxt = store.collate(_ids(0))
    for i in range(STEPS):
        extra = None
        if pattern == "predict" and i % 2 == 1:
            m.eval()
            extra = eng.predict(nxt).clone()
            m.train()
        if pattern == "one_call":
            b = store.collate(_ids(i))
            loss = eng.train_step(b)
        elif pattern == "after":
            b = store.collate(_ids(i))
            loss = eng.begin_step(b)
            eng.end_step()
        else:
            b = nxt
            loss = eng.begin_step(b)
            nxt = store.collate(_ids(i + 1))
            eng.end_step()
        grad = opt.flat_grad.clone()
        if pattern == "clip":
            torch.nn.utils.clip_grad_norm_(m.parameters(), 0.05)
        elif pattern == "scale":
            opt.flat_grad.mul_(0.5)
        elif pattern == "clamp":
            with torch.no_grad():
                m.z_initial.weight.clamp_(-0.5, 0.5)
        if pattern == "denom":
            opt.step(grad_denom=one)
        else:
            opt.step()
        seen = (p_early.detach().clone(), p_late.detach().clone())
        if pattern == "edit_after":
            with torch.no_grad():
                m.z_initial.weight.mul_(0.999)
        out.append(dict(loss=loss.clone(), grad=grad, p_early=seen[0], p_late=seen[1], param=opt.flat_param.clone(),
                        exp_avg=opt.exp_avg.clone(), exp_avg_sq=opt.exp_avg_sq.clone(),
                        buffers=[t.clone() for t in m.buffers()], extra=extra))
    torch.cuda.synchronize()
    seams1, splits1 = _counts(nv)
    _cache[key] = (out, seams1 - seams0, splits1 - splits0)
    return _cache[key]


def _assert_same(want, got):
    assert len(want) == len(got) == STEPS
    for i, (a, b) in enumerate(zip(want, got)):
        assert bool(torch.isfinite(a["loss"]).all()) and bool(torch.isfinite(a["grad"]).all()) and float(a["grad"].abs().max()) > 0.0, i
        for k in ("loss", "grad", "p_early", "p_late", "param", "exp_avg", "exp_avg_sq"):
            assert torch.equal(a[k], b[k]), (i, k, int((a[k] != b[k]).sum()))
        assert len(a["buffers"]) == len(b["buffers"]) and all(torch.equal(s, t) for s, t in zip(a["buffers"], b["buffers"])), i
        assert (a["extra"] is None) == (b["extra"] is None) and (a["extra"] is None or torch.equal(a["extra"], b["extra"])), i


CONFIGS = pytest.mark.parametrize("L,H", [(2, 128), (1, 64)], ids=["L2_H128", "L1_H64"])


@CONFIGS
def test_alternating_batches_agree_with_the_former_boundary(E, knobs, L, H):
    """bench.py's call pattern on two alternating batches of 6 and 11 graphs: every step but the first takes the fast seam,
    every optimiser step runs split, and nothing differs from the former boundary — the read-backs on the caller's stream
    (flat_grad right behind end_step, an early and a late parameter right behind opt.step()) included."""
    old, seams_old, splits_old = _run(E, knobs, L, H, LEGACY, "between")
    new, seams_new, splits_new = _run(E, knobs, L, H, NEW, "between")
    assert (seams_old, splits_old) == (0, 0)
    assert (seams_new, splits_new) == (STEPS - 1, STEPS)
    _assert_same(old, new)


@CONFIGS
def test_batch_collated_after_the_optimiser_step_takes_the_old_chain(E, knobs, L, H):
    """the same batches, each collated after opt.step(): the optimiser step still runs split, no step takes the fast seam, and
    the bits are those of the former boundary"""
    old, _, _ = _run(E, knobs, L, H, LEGACY, "between")
    new, seams, splits = _run(E, knobs, L, H, NEW, "after")
    assert (seams, splits) == (0, STEPS)
    _assert_same(old, new)


@pytest.mark.parametrize("pattern", ["denom", "decay", "one_call", "predict", "clip", "scale", "clamp", "edit_after"])
def test_fallbacks_do_not_take_the_fast_seam(E, knobs, pattern):
    """step(grad_denom=...), weight_decay > 0 and engine.train_step in one call never split the optimiser step or take the
    fast seam; an eval forward in front of a step takes the seam from that step only.  A torch op that writes gradients or
    parameters between end_step() and opt.step() (clipping, scaling, a clamp) keeps the whole update on the caller's stream, behind
    that op — the split launch would not be ordered behind it — and one between opt.step() and begin_step() keeps the step behind
    the caller's stream.  Bitwise equal to the former boundary."""
    L, H = 2, 128
    old, seams_old, splits_old = _run(E, knobs, L, H, LEGACY, pattern)
    new, seams, splits = _run(E, knobs, L, H, NEW, pattern)
    assert (seams_old, splits_old) == (0, 0)
    if pattern == "predict":                 # steps 1, 3, 5 follow a predict; steps 2, 4 follow an optimiser step at once
        assert (seams, splits) == (STEPS // 2 - 1, STEPS)
    elif pattern == "edit_after":
        assert (seams, splits) == (0, STEPS)
    else:
        assert (seams, splits) == (0, 0)
    _assert_same(old, new)


def test_drop_fast_seam_is_honoured(E, knobs):
    """StepEngine.drop_fast_seam() between opt.step() and begin_step(): that step starts behind the caller's stream"""
    knobs.call("esc_engine_set_side_stream", NEW)
    store = _store(E)
    m = _model(E, 1, 64)
    opt = E.optim.FlatAdam(m.parameters(), lr=1e-3, late=E.parallel.edge_pipeline_parameters(m))
    eng = E.StepEngine(m)
    seams0, _ = _counts(knobs)
    nxt = store.collate(_ids(0))
    for i in range(3):
        b = nxt
        if i == 2:
            eng.drop_fast_seam()
        eng.begin_step(b)
        nxt = store.collate(_ids(i + 1))
        eng.end_step()
        opt.step()
    torch.cuda.synchronize()
    assert _counts(knobs)[0] - seams0 == 1            # step 1 only


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096 + 3])
def test_adam_entry_and_its_two_parts_equal_one_launch(E, knobs, n):
    """esc_engine_adam_step over (n, n_early) for n_early in {0, 16, n}, and the two launches it is made of ([0, k) and [k, n)
    through esc_adam_step_scaled), against ONE esc_adam_step_scaled over [0, n): bit for bit, over three steps.  With no engine
    step in front, the entry itself ("entry") is one launch on the caller's stream: it shows that the entry is esc_adam_step
    there, for every (n, n_early).  That the kernel does not depend on the launch's extent is what "parts" shows.  The split over
    the engine's two streams is covered by the engine tests above (their counters say that it ran), not here."""
    nv = knobs
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen).to(DEV)
    grads = [torch.randn(n, generator=gen).to(DEV) for _ in range(3)]
    hyper = (1e-3, 0.9, 0.999, 1e-8)

    def run(update):
        p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        for t, g in enumerate(grads, 1):
            update(p, g, m, v, t)
        torch.cuda.synchronize()
        return p, m, v

    def whole(p, g, m, v, t):
        nv.call("esc_adam_step_scaled", nv.ptr(p), nv.ptr(g), nv.ptr(m), nv.ptr(v), n, *hyper, t, None, nv.stream())

    def off(t, k):                                          # address of element k (NULL stays out of it: k < n)
        return t.data_ptr() + 4 * k

    want = run(whole)
    for k in sorted({0, 16, n}):
        if k > n:
            continue

        def entry(p, g, m, v, t):
            nv.call("esc_engine_adam_step", nv.ptr(p), nv.ptr(g), nv.ptr(m), nv.ptr(v), n, k, *hyper, t, nv.stream())

        def parts(p, g, m, v, t):
            nv.call("esc_adam_step_scaled", nv.ptr(p), nv.ptr(g), nv.ptr(m), nv.ptr(v), k, *hyper, t, None, nv.stream())
            if k < n:
                nv.call("esc_adam_step_scaled", off(p, k), off(g, k), off(m, k), off(v, k), n - k, *hyper, t, None, nv.stream())

        for name, update in (("entry", entry), ("parts", parts)):
            got = run(update)
            for a, b, what in zip(want, got, ("param", "exp_avg", "exp_avg_sq")):
                assert torch.equal(a, b), (n, k, name, what)
