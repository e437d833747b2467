"""What every run trains through at the end of a step, on every case of tests/loss_cases.py: the L1, MSE and masked
BCE-with-logits losses (csrc/optim.hip, csrc/geometry.hip) through the C ABI and through ops + autograd, and the Adam update
through FlatAdam, esc_adam_step and esc_adam_step_scaled.

Losses: every buffer the ABI is handed sits between guards (NaN around inputs, a sentinel around outputs); the loss and dpred
are held to fp64 by the criterion of tests/test_hip_expressive.py::_check with the floors DESIGN.md derives, and whatever the
mathematics makes exact is asserted exactly: a tie's L1 gradient, an unlabelled entry's gradient, a batch without labels (loss
and gradient 0, where torch's empty mean is NaN: the library differs on purpose), saturated logits against their own label,
dpred = NULL against dpred given, a second call against the first.

Adam: flat_param, exp_avg and exp_avg_sq against fp64 within the per-element bounds of loss_cases.adam_ref64; padding slots
0 after every step; untouched elements bit-identical; grad_denom against dividing first; late= against no late; the two entry
points against each other; a checkpoint resumed bit for bit; ReduceLROnPlateau against torch's.  The arithmetic is torch's up
to FMA contraction (csrc/optim.hip is not built with -ffp-contract=off), so nothing here asks for torch's fp32 bits.
Each line printed is `case  buffer  worst error / bound over the elements  (largest error)`.
"""
import numpy as np
import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import linear_cases as lin
import loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
ENTRY = {"l1": "esc_l1_loss", "mse": "esc_mse_loss", "bce": "esc_bce_logits_loss"}


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


_REFS = {}


def refs_of(case):
    """inputs, fp64 and torch-fp32 references and floors of a loss case: computed once, shared, never modified"""
    if case not in _REFS:
        pred, y = lc.loss_data(case)
        loss, grad = lc.loss_ref64(case, pred, y)
        l32, g32 = lc.loss_torch(case, pred, y, torch.float32)
        _REFS[case] = (pred, y, loss, grad, l32, g32) + lc.loss_floors(case, pred, y, loss, grad)
    return _REFS[case]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def exact_properties(case, pred, y, loss, grad, what):
    """what the mathematics makes exact; loss [1] or [], grad flat or None (CPU tensors)"""
    p, t = pred.reshape(-1), y.reshape(-1)
    assert bool(torch.isfinite(loss).all()), what
    if grad is None:
        return
    grad = grad.reshape(-1)
    assert bool(torch.isfinite(grad).all()), what
    if case.entry == "l1":
        assert bool((grad[p == t] == 0).all()), "%s: a tie's gradient is not 0" % what
        assert bool((grad[p != t] != 0).all()), what
    if case.entry == "bce":
        assert bool((grad[t != t] == 0).all()), "%s: an unlabelled entry has a gradient" % what
        if case.regime == "none_labelled":
            assert float(loss) == 0.0 and not bool(grad.any()), what
        if case.regime == "saturated":
            assert float(p[0]) == -1e4 and float(t[0]) == 0.0 and float(grad[0]) == 0.0, what
            if p.numel() >= 12:
                assert float(p[-1]) == 1e4 and float(t[-1]) == 1.0 and float(grad[-1]) == 0.0, what


class AbiLoss(object):
    """the guarded buffers of one call of a loss entry point"""

    def __init__(self, case, pred, y, want_dpred):
        M = pred.numel()
        self.case, self.M, self.want = case, M, want_dpred
        self.P = lin.Buf(1, M, M, 0, pred.reshape(1, M), NAN, 64, 64, DEV)
        self.Y = lin.Buf(1, M, M, 0, y.reshape(1, M), NAN, 64, 64, DEV)
        self.L = lin.Buf(1, 1, 1, 0, torch.full((1, 1), NAN), lin.sentinel(), 64, 64, DEV)
        self.D = lin.Buf(1, M, M, 0, torch.full((1, M), NAN), lin.sentinel(), 64, 64, DEV)

    def call(self, nv):
        c, dp = self.case, (self.D.ptr() if self.want else None)
        if c.entry == "bce":
            args = (self.P.ptr(), self.Y.ptr(), self.M, int(c.denom or 0), self.L.ptr(), dp, nv.stream())
        else:
            args = (self.P.ptr(), self.Y.ptr(), self.M, int(c.denom or self.M), float(c.grad_scale), self.L.ptr(), dp, nv.stream())
        nv.call(ENTRY[c.entry], *args)
        torch.cuda.synchronize()
        assert self.P.untouched() and self.Y.untouched(), "%s: an input was written" % c.name
        assert self.L.outside_changed() == 0, "%s: written around the loss" % c.name
        if self.want:
            assert self.D.outside_changed() == 0, "%s: written around dpred" % c.name
        else:
            assert self.D.untouched(), "%s: dpred = NULL, yet the buffer was written" % c.name
        return self.L.result().reshape(-1).clone(), (self.D.result().reshape(-1).clone() if self.want else None)


@pytest.mark.parametrize("name", [c.name for c in lc.LOSS_CASES])
def test_loss_through_the_abi(E, name):
    nv = E._native
    case = lc.LOSS_BY_NAME[name]._replace(upstream=1.0)                 # the ABI has no upstream gradient
    pred, y, loss64, grad64, l32, g32, floor_l, floor_g = refs_of(case)
    loss, grad = AbiLoss(case, pred, y, case.want_dpred).call(nv)
    lc.check(name + " loss", loss, l32, loss64, floor_l)
    if case.want_dpred:
        lc.check(name + " dpred", grad, g32, grad64, floor_g)
    exact_properties(case, pred, y, loss, grad, name)
    again = AbiLoss(case, pred, y, case.want_dpred).call(nv)          # fresh buffers, same bits
    assert same_bits(loss, again[0]) and (grad is None or same_bits(grad, again[1])), name
    other = AbiLoss(case, pred, y, not case.want_dpred).call(nv)      # dpred given or not: the same loss bits
    assert same_bits(loss, other[0]), "%s: the loss depends on whether dpred is wanted" % name


def _device_pred(pred, shape, sliced):
    """(leaf, view handed to ops, function taking the leaf's gradient to the view's): `sliced` is a column slice of a wider
    matrix whose other columns hold NaN"""
    if not sliced:
        leaf = pred.reshape(shape).to(DEV).requires_grad_(True)
        return leaf, leaf, (lambda g: g)
    G, T = shape
    wide = torch.full((G, T + 3), NAN)
    wide[:, 1:1 + T] = pred.reshape(G, T)
    leaf = wide.to(DEV).requires_grad_(True)
    view = leaf[:, 1:1 + T]
    assert G == 1 or not view.is_contiguous()

    def cut(g):
        rest = torch.cat([g[:, :1], g[:, 1 + T:]], 1)
        assert not bool(rest.any()), "a gradient outside the slice"
        return g[:, 1:1 + T]
    return leaf, view, cut


@pytest.mark.parametrize("name", [c.name for c in lc.LOSS_CASES if c.want_dpred])
def test_loss_through_ops_and_autograd(E, name):
    """pred as [M, 1], [M] (which ops.l1_loss's backward used to refuse), [G, T] and a non-contiguous column slice"""
    case = lc.LOSS_BY_NAME[name]._replace(grad_scale=1.0)               # ops always asks for grad_scale 1
    fn = {"l1": E.ops.l1_loss, "mse": E.ops.mse_loss, "bce": E.ops.bce_with_logits_loss}[case.entry]
    pred, y, loss64, grad64, l32, g32, floor_l, floor_g = refs_of(case)
    first = None
    for lay, (shape, sliced) in lc.pred_layouts(case).items():
        leaf, view, cut = _device_pred(pred, shape, sliced)
        yd = y.reshape(-1).to(DEV) if lay == "[M,1]" else y.reshape(shape).to(DEV)
        loss = fn(view, yd, denom=case.denom)
        assert loss.shape == ()
        (loss * case.upstream if case.upstream != 1.0 else loss).backward()
        grad = cut(leaf.grad)
        assert grad.shape == torch.Size(shape), (name, lay, tuple(grad.shape))
        what = "%s %s" % (name, lay)
        lc.check(what + " loss", loss, l32, loss64, floor_l)
        lc.check(what + " grad", grad, g32, grad64, floor_g)
        exact_properties(case, pred, y, loss.detach().cpu(), grad.cpu(), what)
        if first is None:
            first = (loss.detach().clone(), grad.reshape(-1).clone())
        else:                                                           # the layout of pred changes no bit
            assert same_bits(loss, first[0]) and same_bits(grad.reshape(-1), first[1]), what


@pytest.mark.parametrize("denom", [None, 7])
@pytest.mark.parametrize("M", [1, 2, 6])
@pytest.mark.parametrize("entry", ["l1", "mse", "bce"])
def test_elementwise_loss_heads_return_the_gradient_in_the_shape_of_pred(E, entry, M, denom):
    """The three heads are one Function behind a table: each keeps its divisor (M, M, the labelled count), bce takes a NaN
    label, and the gradient comes back as [M], [M, 1] or [2, M // 2], whichever pred was (ops.l1_loss's backward once
    returned [M, 1] whatever it was given).  [2, 0], what M = 1 makes of the third shape, is refused like every empty batch."""
    fn = {"l1": E.ops.l1_loss, "mse": E.ops.mse_loss, "bce": E.ops.bce_with_logits_loss}[entry]
    case = lc.Loss("heads-%s-%d-%s" % (entry, M, denom), entry, M, 1, "plain", denom, 1.0, True, 1.0)
    g = torch.Generator().manual_seed(lc.seed_of(case.name))
    pred, y = torch.randn(M, generator=g), torch.randn(M, generator=g)
    if entry == "bce":
        pred, y = pred * 3, (torch.rand(M, generator=g) > 0.5).float()
        y[M - 1] = NAN
    loss64, grad64 = lc.loss_ref64(case, pred, y)
    l32, g32 = lc.loss_torch(case, pred, y, torch.float32)
    floor_l, floor_g = lc.loss_floors(case, pred, y, loss64, grad64)
    for shape in ((M,), (M, 1), (2, M // 2)):
        what = "%s %s" % (case.name, list(shape))
        if 2 * (M // 2) != M and len(shape) == 2 and shape[0] == 2:
            with pytest.raises(RuntimeError):
                fn(torch.zeros(shape, device=DEV, requires_grad=True), torch.zeros(0, device=DEV), denom=denom)
            continue
        leaf = pred.reshape(shape).to(DEV).requires_grad_(True)
        loss = fn(leaf, y.to(DEV), denom=denom)
        assert loss.shape == ()
        loss.backward()
        assert leaf.grad.shape == torch.Size(shape), (what, tuple(leaf.grad.shape))
        lc.check(what + " loss", loss, l32, loss64, floor_l)
        lc.check(what + " grad", leaf.grad, g32, grad64, floor_g)
        exact_properties(case, pred, y, loss.detach().cpu(), leaf.grad.cpu(), what)


def test_loss_bad_arguments_raise_and_leave_the_device_usable(E):
    nv, ops = E._native, E.ops
    x, t = torch.randn(8, 1, device=DEV), torch.randn(8, device=DEV)
    for fn in (ops.l1_loss, ops.mse_loss, ops.bce_with_logits_loss):
        with pytest.raises(ValueError):
            fn(x, t[:7])
        with pytest.raises(TypeError):
            fn(x, t.double())
        with pytest.raises(TypeError):
            fn(x, t.long())
        with pytest.raises(RuntimeError):
            fn(x, t.cpu())
        with pytest.raises(RuntimeError):
            fn(x.cpu(), t)
    case = lc.LOSS_BY_NAME["l1-64x1-plain"]
    pred, y = lc.loss_data(case)
    for entry in ("l1", "mse", "bce"):
        run = AbiLoss(case._replace(entry=entry), pred, y, True)
        run.M = 0
        with pytest.raises(RuntimeError):
            run.call(nv)
        torch.cuda.synchronize()
        assert run.L.untouched() and run.D.untouched() and run.P.untouched() and run.Y.untouched()
    for name in ("l1-64x1-plain", "mse-64x1-plain", "bce-64x1-plain"):      # ... and the device still computes
        c = lc.LOSS_BY_NAME[name]
        pred, y, loss64, grad64, l32, g32, floor_l, floor_g = refs_of(c)
        loss, grad = AbiLoss(c, pred, y, True).call(nv)
        lc.check(name + " loss after the refusals", loss, l32, loss64, floor_l)
        lc.check(name + " dpred after the refusals", grad, g32, grad64, floor_g)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------
_ADAM_REFS = {}


def adam_refs(case):
    key = (case.n, case.steps, case.step0, case.lrs, case.betas, case.eps, case.regime, case.grad_denom)
    if key not in _ADAM_REFS:
        if len(_ADAM_REFS) > 4:
            _ADAM_REFS.clear()
        _ADAM_REFS[key] = lc.adam_ref64(case, lc.adam_data(case))
    return _ADAM_REFS[key]


def run_flat(E, case, data, predivide=False):
    """the case through FlatAdam: (p, exp_avg, exp_avg_sq) of the n live elements in the order the tensors were handed over,
    float32 numpy.  Padding slots of the three buffers are checked after every step.  predivide: the gradients are divided by
    grad_denom beforehand (one fp32 division, on the device) and the plain step is taken."""
    sizes = lc.tensor_sizes(case)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    params = [torch.nn.Parameter(torch.from_numpy(data.p0[a:b].copy()).to(DEV)) for a, b in zip(starts[:-1], starts[1:])]
    late = [params[i] for i in lc.late_tensors(case)]
    opt = E.optim.FlatAdam(params, lr=case.lrs[0], betas=case.betas, eps=case.eps, late=late or None)
    order, offsets, total = lc.flat_layout(case)
    assert opt.flat_param.numel() == total and opt.offsets == offsets and [id(p) for p in opt.params] == [id(params[i]) for i in order]
    idx = torch.from_numpy(lc.flat_index(case)).to(DEV)
    pad = torch.ones(total, dtype=torch.bool, device=DEV)
    pad[idx] = False
    assert int(pad.sum()) == total - case.n and all(p.data_ptr() % 64 == 0 and p.grad.data_ptr() % 64 == 0 for p in params)
    if case.step0:
        sd = opt.state_dict()
        m0, v0 = torch.zeros(total), torch.zeros(total)
        m0[idx.cpu()], v0[idx.cpu()] = torch.from_numpy(data.m0), torch.from_numpy(data.v0)
        opt.load_state_dict(dict(sd, step=case.step0, exp_avg=m0, exp_avg_sq=v0))
        assert opt.step_count == case.step0
    den = torch.tensor([case.grad_denom], dtype=torch.float32, device=DEV) if case.grad_denom else None
    for k in range(case.steps):
        opt.param_groups[0]["lr"] = case.lrs[k]
        opt.zero_grad()
        g = torch.from_numpy(data.grads[k]).to(DEV)
        if predivide:
            g = g / den
        for p, a, b in zip(params, starts[:-1], starts[1:]):
            p.grad.copy_(g[a:b])
        opt.step(grad_denom=None if predivide else den)
        for buf, what in ((opt.flat_param, "flat_param"), (opt.exp_avg, "exp_avg"), (opt.exp_avg_sq, "exp_avg_sq")):
            assert not bool(buf[pad].view(torch.int32).any()), "%s: padding of %s is not 0 after step %d" % (case.name, what, k + 1)
    assert opt.step_count == case.step0 + case.steps
    for p, a, b in zip(params, starts[:-1], starts[1:]):                    # the parameters still are views of the buffer
        assert same_bits(p.data.reshape(-1), opt.flat_param[idx[a:b]])
    return tuple(buf[idx].cpu().numpy() for buf in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq))


def hold_to_bounds(case, data, got, how):
    p, m, v, Bp, Bm, Bv = adam_refs(case)
    for mine, ref, bound, what in zip(got, (p, m, v), (Bp, Bm, Bv), ("flat_param", "exp_avg", "exp_avg_sq")):
        ratio, err = lc.worst_ratio(mine, ref, bound)
        print("%-44s %-7s %-10s %.3f  (%.3g)" % (case.name, how, what, ratio, err))
        assert ratio <= 1.0, "%s %s: %s is %.3g from fp64, %.3f of its bound" % (case.name, how, what, err, ratio)
    still = ~data.touched                                                   # elements no gradient ever reaches
    if still.any():
        assert np.array_equal(got[0][still].view(np.int32), data.p0[still].view(np.int32)), "%s: an untouched parameter moved" % case.name
        assert np.array_equal(got[1][still].view(np.int32), data.m0[still].view(np.int32)) and not data.m0[still].any()
        assert not got[2][still].view(np.int32).any(), case.name
    if case.regime == "all_zero":
        assert not still.size or still.all()


def equal_bits(a, b):
    return all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("name", [c.name for c in lc.ADAM_CASES])
def test_adam_through_flat_adam(E, name):
    case = lc.ADAM_BY_NAME[name]
    data = lc.adam_data(case)
    got = run_flat(E, case, data)
    hold_to_bounds(case, data, got, "flat")
    assert equal_bits(got, run_flat(E, case, data)), "%s: a second run gives other bits" % name
    if case.grad_denom and case.layout == "one":
        assert equal_bits(got, run_flat(E, case, data, predivide=True)), "%s: grad_denom is not dividing first" % name
    if case.layout == "late":                                               # the layout changes no bit of any parameter
        twin = lc.ADAM_BY_NAME[name[:-len("late")] + "padded"]
        assert equal_bits(got, run_flat(E, twin, data)), "%s: late= changes a result" % name


def run_abi(E, case, data, scaled):
    """the case through esc_adam_step_scaled (scaled) or esc_adam_step, n exactly the case's, every buffer between guards"""
    nv, n = E._native, case.n
    bufs = [lin.Buf(1, n, n, 0, torch.from_numpy(a).reshape(1, n), lin.sentinel(), 64, 64, DEV) for a in (data.p0, data.m0, data.v0)]
    den = torch.tensor([case.grad_denom], dtype=torch.float32, device=DEV) if case.grad_denom else None
    assert scaled or den is None
    for k in range(case.steps):
        G = lin.Buf(1, n, n, 0, torch.from_numpy(data.grads[k]).reshape(1, n), NAN, 64, 64, DEV)
        head = (bufs[0].ptr(), G.ptr(), bufs[1].ptr(), bufs[2].ptr(), n, float(case.lrs[k]), float(case.betas[0]),
                float(case.betas[1]), float(case.eps), case.step0 + k + 1)
        if scaled:
            nv.call("esc_adam_step_scaled", *(head + (nv.ptr(den), nv.stream())))
        else:
            nv.call("esc_adam_step", *(head + (nv.stream(),)))
        torch.cuda.synchronize()
        assert G.untouched(), "%s: the gradient was written" % case.name
    for b, what in zip(bufs, ("param", "exp_avg", "exp_avg_sq")):
        assert b.outside_changed() == 0, "%s: written around %s" % (case.name, what)
    return tuple(b.result().reshape(-1).numpy().copy() for b in bufs)


@pytest.mark.parametrize("name", [c.name for c in lc.adam_cases(layout="one")])
def test_adam_through_the_abi(E, name):
    case = lc.ADAM_BY_NAME[name]
    data = lc.adam_data(case)
    got = run_abi(E, case, data, True)
    hold_to_bounds(case, data, got, "abi")
    if not case.grad_denom:
        assert equal_bits(got, run_abi(E, case, data, False)), "%s: esc_adam_step differs from esc_adam_step_scaled(NULL)" % name
    else:
        assert equal_bits(got, run_abi(E, case, data, True)), name
    assert equal_bits(got, run_flat(E, case, data)), "%s: FlatAdam and the entry point on its own differ" % name


def test_adam_bad_arguments_raise_and_leave_the_device_usable(E):
    nv = E._native
    case = lc.ADAM_BY_NAME["adam-17-s3-plain"]
    data = lc.adam_data(case)
    t = torch.zeros(32, device=DEV)
    with pytest.raises(RuntimeError):
        nv.call("esc_adam_step", t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), 17, 1e-2, 0.9, 0.999, 1e-8, 0, nv.stream())
    with pytest.raises(RuntimeError):
        nv.call("esc_adam_step", t.data_ptr(), None, t.data_ptr(), t.data_ptr(), 17, 1e-2, 0.9, 0.999, 1e-8, 1, nv.stream())
    with pytest.raises(RuntimeError):
        E.optim.FlatAdam([torch.nn.Parameter(torch.zeros(3))])
    torch.cuda.synchronize()
    assert not bool(t.any())
    hold_to_bounds(case, data, run_abi(E, case, data, True), "abi")


class _Net(torch.nn.Module):
    """four parameters, a 1-element one among them (GINEConv.eps), so that the bucket has padding"""

    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(5, 7, generator=g))
        self.eps = torch.nn.Parameter(torch.randn(1, generator=g))
        self.b = torch.nn.Parameter(torch.randn(33, generator=g))
        self.c = torch.nn.Parameter(torch.randn(3, 5, generator=g))


def _train(opt, model, grads):
    for step in grads:
        opt.zero_grad()
        for p, g in zip(model.parameters(), step):
            p.grad.copy_(g.to(DEV))
        opt.step()


def test_checkpoint_resume_is_bit_exact(E, tmp_path):
    """k steps, torch.save of the model's and the optimiser's state_dict, both loaded into a fresh model and a fresh FlatAdam
    (the order of run_ogb_mol --continue_from), j more steps == k + j uninterrupted steps, bit for bit"""
    k, j = 3, 2
    g = torch.Generator().manual_seed(11)
    grads = [[torch.randn(p.shape, generator=g) for p in _Net(0).parameters()] for _ in range(k + j)]
    whole = _Net(0).to(DEV)
    wopt = E.optim.FlatAdam(whole.parameters(), lr=3e-3, betas=lc.OTHER_BETAS, eps=lc.OTHER_EPS)
    _train(wopt, whole, grads)
    first = _Net(0).to(DEV)
    fopt = E.optim.FlatAdam(first.parameters(), lr=3e-3, betas=lc.OTHER_BETAS, eps=lc.OTHER_EPS)
    _train(fopt, first, grads[:k])
    torch.save(first.state_dict(), str(tmp_path / "model.pth"))
    torch.save(fopt.state_dict(), str(tmp_path / "optimizer.pth"))
    second = _Net(1).to(DEV)                                                # other values, default hyper-parameters: all of it
    sopt = E.optim.FlatAdam(second.parameters())                            # must come from the two files
    second.load_state_dict(torch.load(str(tmp_path / "model.pth"), map_location=DEV))
    sopt.load_state_dict(torch.load(str(tmp_path / "optimizer.pth"), map_location=DEV))
    assert sopt.step_count == k and sopt.param_groups[0]["lr"] == 3e-3 and tuple(sopt.param_groups[0]["betas"]) == lc.OTHER_BETAS
    assert same_bits(sopt.flat_param, fopt.flat_param) and same_bits(sopt.exp_avg, fopt.exp_avg)
    _train(sopt, second, grads[k:])
    for buf in ("flat_param", "exp_avg", "exp_avg_sq"):
        assert same_bits(getattr(sopt, buf), getattr(wopt, buf)), buf
    for p, q in zip(second.parameters(), whole.parameters()):
        assert same_bits(p, q)
    assert sopt.step_count == wopt.step_count == k + j


def test_reduce_lr_on_plateau_side_by_side_with_torch(E):
    """the package's ReduceLROnPlateau on a FlatAdam and torch's on a torch.optim.Adam (fp64, CPU) see the same metrics: two
    reductions, equal learning rates at every epoch, and the parameters within the bound of the learning rates torch chose"""
    metrics = (1.0, 1.1, 0.5, 0.6, 0.3, 0.2)
    n = 257
    base = lc.ADAM_BY_NAME["adam-257-s3-plain"]
    tp = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
    topt = torch.optim.Adam([tp], lr=1e-2, foreach=False)
    tsch = torch.optim.lr_scheduler.ReduceLROnPlateau(topt, mode="min", factor=0.5, patience=0, min_lr=1e-5)
    mp = torch.nn.Parameter(torch.zeros(n, device=DEV))
    mopt = E.optim.FlatAdam([mp], lr=1e-2)
    msch = E.optim.ReduceLROnPlateau(mopt, mode="min", factor=0.5, patience=0, min_lr=1e-5)
    case = base._replace(name="plateau", steps=len(metrics), lrs=(1e-2,) * len(metrics))
    data = lc.AdamData(case)
    tp.data.copy_(torch.from_numpy(data.p0))
    mp.data.copy_(torch.from_numpy(data.p0))
    lrs = []
    for k, metric in enumerate(metrics):
        lrs.append(topt.param_groups[0]["lr"])
        assert mopt.param_groups[0]["lr"] == lrs[-1], (k, mopt.param_groups[0]["lr"], lrs[-1])
        tp.grad = torch.from_numpy(data.grads[k]).double()
        topt.step()
        mopt.zero_grad()
        mp.grad.copy_(torch.from_numpy(data.grads[k]))
        mopt.step()
        tsch.step(metric)
        msch.step(metric)
    assert mopt.param_groups[0]["lr"] == topt.param_groups[0]["lr"]
    assert len(set(lrs)) == 3 and lrs[-1] == 2.5e-3, lrs                   # two reductions happened
    case = case._replace(lrs=tuple(lrs))
    p, m, v, Bp, Bm, Bv = lc.adam_ref64(case, data)
    assert float(np.abs(p - tp.detach().numpy()).max()) <= 1e-12 * float(np.abs(p).max())
    got = (mopt.flat_param[:n].cpu().numpy(), mopt.exp_avg[:n].cpu().numpy(), mopt.exp_avg_sq[:n].cpu().numpy())
    for mine, ref, bound, what in zip(got, (p, m, v), (Bp, Bm, Bv), ("flat_param", "exp_avg", "exp_avg_sq")):
        ratio, err = lc.worst_ratio(mine, ref, bound)
        print("plateau %-10s %.3f  (%.3g)" % (what, ratio, err))
        assert ratio <= 1.0, (what, ratio, err)
