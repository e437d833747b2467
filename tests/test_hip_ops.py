"""Parity of each HIP kernel family with the CPU oracle (through the C ABI via ctypes).

Integer/index-driven sums with a defined order (bag forward, aggregate forward) must be
BIT-EXACT against the oracle's sequential scatter; matrix-core and reduction kernels are held to
rtol=atol=1e-5 against an fp64 reference (north_star tolerance: 1e-5 fp32)."""
import numpy as np
import pytest
import torch

from conftest import load_collate, require_gpu
import ref_model as rm

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-5, atol=1e-5)


def _chk(got, want, what, tol=1e-5):
    got, want = got.detach().cpu().double(), want.detach().double()
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max()) / scale
    assert err <= tol, "%s: max error %.3g of scale %.3g > %g" % (what, err, scale, tol)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _batch(tag="count3"):
    _, b, _ = load_collate(tag)
    return {k: torch.tensor(v) for k, v in b.items()}


def _plan(E, b, dev):
    return E.BatchPlan.from_tensors(b["edge_index"].to(dev), b["x"].shape[0], b["pos_enc"].to(dev),
                                    b["pos_index"].to(dev), b["pos_batch"].to(dev))


@pytest.mark.parametrize("H", [256, 64, 300, 10])
def test_bag_forward_bit_exact_and_backward(E, H):
    torch.manual_seed(H)
    dev = torch.device("cuda:0")
    b = _batch("mixed4")
    plan = _plan(E, b, dev)
    W = torch.randn(1800, H)
    torch.set_num_threads(1)
    ref = rm.global_add_pool(W[b["pos_index"]] * b["pos_enc"].view(-1, 1), b["pos_batch"], plan.num_edges)
    Wd = W.to(dev).requires_grad_(True)
    out = E.ops.esc_bag(Wd, plan)
    assert torch.equal(out.cpu(), ref), "bag forward must be bitwise a sequential scatter_add"
    g = torch.randn_like(ref)
    out.backward(g.to(dev))
    gref = torch.zeros(1800, H, dtype=torch.float64)
    gref.index_add_(0, b["pos_index"], g.double()[b["pos_batch"]] * b["pos_enc"].double().view(-1, 1))
    _chk(Wd.grad, gref, "table gradient")
    # deterministic: a second backward gives the same bits
    Wd.grad = None
    E.ops.esc_bag(Wd, plan).backward(g.to(dev))
    g2 = Wd.grad.clone()
    Wd.grad = None
    E.ops.esc_bag(Wd, plan).backward(g.to(dev))
    assert torch.equal(g2, Wd.grad)


@pytest.mark.parametrize("C", [256, 10, 64, 300])
def test_aggregate_forward_bit_exact_and_backward(E, C):
    torch.manual_seed(C)
    dev = torch.device("cuda:0")
    b = _batch("mixed4")
    plan = _plan(E, b, dev)
    N, Ed = b["x"].shape[0], b["edge_index"].shape[1]
    x, e, eps = torch.randn(N, C), torch.randn(Ed, C), torch.tensor([0.3])
    ei = b["edge_index"]
    torch.set_num_threads(1)
    msg = (x.index_select(0, ei[0]) + e).relu()
    ref = torch.zeros_like(x).index_add_(0, ei[1], msg)
    ref = ref + (1 + eps) * x
    xd, ed, epsd = (t.to(dev).requires_grad_(True) for t in (x, e, eps))
    out = E.ops.gine_aggregate(xd, ed, epsd, plan)
    assert torch.equal(out.cpu(), ref), "aggregate forward must equal the sequential scatter bit for bit"
    g = torch.randn(N, C)
    out.backward(g.to(dev))
    x64, e64, eps64 = (t.double().requires_grad_(True) for t in (x, e, eps))
    m64 = (x64.index_select(0, ei[0]) + e64).relu()
    r64 = torch.zeros_like(x64).index_add(0, ei[1], m64) + (1 + eps64) * x64
    r64.backward(g.double())
    assert torch.allclose(xd.grad.cpu().double(), x64.grad, **TOL)
    assert torch.allclose(ed.grad.cpu().double(), e64.grad, **TOL)
    assert torch.allclose(epsd.grad.cpu().double(), eps64.grad, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("M,N,K", [(1000, 256, 256), (333, 256, 10), (777, 10, 256), (130, 256, 1280),
                                   (257, 1, 256), (9000, 256, 256), (5, 48, 36),
                                   (1000, 300, 300), (777, 600, 300), (9000, 300, 600), (6500, 300, 44), (260, 36, 300),
                                   # molhiv's edge rows 300 -> 300, node rows 300 -> 600 and 600 -> 300: the 64- and 128-row LDS-DMA tiles
                                   # (the 128x160 tile is off unless ESC_TILE160=1: tests/test_hip_dense_dispatch.py runs it in a child process)
                                   (20000, 300, 300), (6500, 600, 300), (6500, 300, 600), (19999, 600, 300)])
def test_linear_forward_backward(E, M, N, K):
    torch.manual_seed(M + N + K)
    dev = torch.device("cuda:0")
    x, w, bias = torch.randn(M, K), torch.randn(N, K) / K ** 0.5, torch.randn(N)
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, bias))
    y = E.ops.linear(xd, wd, bd)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    r = x64 @ w64.t() + b64
    assert torch.allclose(y.cpu().double(), r, **TOL)
    g = torch.randn(M, N)
    y.backward(g.to(dev))
    r.backward(g.double())
    assert torch.allclose(xd.grad.cpu().double(), x64.grad, **TOL)
    scale = max(1.0, float(w64.grad.abs().max()))
    assert torch.allclose(wd.grad.cpu().double() / scale, w64.grad / scale, **TOL)
    assert torch.allclose(bd.grad.cpu().double() / scale, b64.grad / scale, **TOL)


@pytest.mark.parametrize("M,C,relu", [(15200, 256, True), (2400, 256, False), (37, 10, True), (2, 300, True)])
def test_batchnorm_relu(E, M, C, relu):
    torch.manual_seed(M)
    dev = torch.device("cuda:0")
    x = torch.randn(M, C) * 3 + 5
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    rm0, rv0 = torch.randn(C), torch.rand(C) + 0.5
    xd, gd, bd = (t.to(dev).requires_grad_(True) for t in (x, gamma, beta))
    rmd, rvd = rm0.to(dev), rv0.to(dev)
    y = E.ops.batch_norm_act(xd, gd, bd, rmd, rvd, 1e-5, 0.1, relu)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    rm64, rv64 = rm0.double(), rv0.double()
    r = torch.nn.functional.batch_norm(x64, rm64, rv64, g64, b64, True, 0.1, 1e-5)
    r = r.relu() if relu else r
    assert torch.allclose(y.cpu().double(), r, **TOL)
    assert torch.allclose(rmd.cpu().double(), rm64, **TOL) and torch.allclose(rvd.cpu().double(), rv64, **TOL)
    g = torch.randn(M, C)
    y.backward(g.to(dev))
    r.backward(g.double())
    # M=2: dx = (1 - xhat^2)(g1-g2)/2 with 1 - xhat^2 = eps/(var+eps) ~ 1e-6: ill-conditioned in ANY fp32
    # implementation (torch's fp32 kernel shows the same), so only a loose bound is meaningful there.
    _chk(xd.grad, x64.grad, "dx", tol=1e-5 if M > 2 else 2e-3)
    _chk(gd.grad, g64.grad, "dgamma")
    _chk(bd.grad, b64.grad, "dbeta")


def test_l1_loss_and_adam(E):
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    p, y = torch.randn(2400, 1), torch.randn(2400)
    pd = p.to(dev).requires_grad_(True)
    loss = E.ops.l1_loss(pd, y.to(dev))
    p64 = p.double().requires_grad_(True)
    r = torch.nn.functional.l1_loss(p64, y.double().view(-1, 1))
    r.backward()
    loss.backward()
    assert abs(float(loss.detach()) - float(r.detach())) < 1e-6
    assert torch.allclose(pd.grad.cpu().double(), p64.grad, rtol=1e-6, atol=1e-9)
    # Adam: 3 steps against torch.optim.Adam on CPU
    from esc_gnn_amd.optim import FlatAdam
    w = torch.randn(1000)
    ref = torch.nn.Parameter(w.clone())
    opt = torch.optim.Adam([ref], lr=1e-2)
    mine = torch.nn.Parameter(w.clone().to(dev))
    one = torch.nn.Parameter(torch.ones(1, device=dev))                 # a 1-element parameter (like GINEConv.eps) in front
    fopt = FlatAdam([one, mine], lr=1e-2)
    assert mine.data_ptr() % 64 == 0 and mine.grad.data_ptr() % 64 == 0   # every parameter starts 64-byte aligned
    for i in range(3):
        g = torch.randn(1000)
        ref.grad = g.clone()
        opt.step()
        fopt.zero_grad()
        mine.grad.copy_(g.to(dev))
        fopt.step()
    assert torch.allclose(mine.detach().cpu(), ref.detach(), rtol=1e-6, atol=1e-7)
    assert float(one.detach()) == 1.0 and float(fopt.flat_param.abs().sum()) == float(mine.detach().abs().sum()) + 1.0
    # scaled form: grad / denom inside the launch == dividing first
    a, b2 = torch.nn.Parameter(w.clone().to(dev)), torch.nn.Parameter(w.clone().to(dev))
    oa, ob = FlatAdam([a], lr=1e-2), FlatAdam([b2], lr=1e-2)
    den = torch.tensor([2400.0], device=dev)
    for i in range(3):
        g = (torch.randn(1000) * 100).to(dev)
        oa.zero_grad(); ob.zero_grad()
        a.grad.copy_(g); b2.grad.copy_(g / den)
        oa.step(grad_denom=den)
        ob.step()
    assert torch.equal(a.detach(), b2.detach())


def test_bad_arguments_raise(E):
    dev = torch.device("cuda:0")
    with pytest.raises((RuntimeError, ValueError)):
        E.ops.linear(torch.zeros(4, 8, device=dev), torch.zeros(3, 7, device=dev), None)
    b = _batch()
    plan = _plan(E, b, dev)
    with pytest.raises(ValueError):
        E.ops.gine_aggregate(torch.zeros(3, 8, device=dev), torch.zeros(5, 8, device=dev),
                             torch.zeros(1, device=dev), plan)
    with pytest.raises(IndexError):
        E.BatchPlan.from_tensors(b["edge_index"].to(dev), b["x"].shape[0], b["pos_enc"].to(dev),
                                 (b["pos_index"] + 1800).to(dev), b["pos_batch"].to(dev))
    with pytest.raises(IndexError):                       # an edge endpoint beyond the node count
        E.BatchPlan.from_tensors(b["edge_index"].to(dev), b["x"].shape[0] - 1, b["pos_enc"].to(dev), b["pos_index"].to(dev),
                                 b["pos_batch"].to(dev))
    with pytest.raises(ValueError):                       # a bag entry for an edge that does not exist
        E.BatchPlan.from_tensors(b["edge_index"].to(dev), b["x"].shape[0], b["pos_enc"].to(dev), b["pos_index"].to(dev),
                                 (b["pos_batch"] + 1).to(dev))
    with pytest.raises(ValueError):                       # unsorted bag
        E.BatchPlan.from_tensors(b["edge_index"].to(dev), b["x"].shape[0], b["pos_enc"].to(dev), b["pos_index"].to(dev),
                                 b["pos_batch"].flip(0).to(dev))


@pytest.mark.parametrize("C,mean", [(256, False), (1280, True), (10, True)])
def test_segment_pool(E, C, mean):
    torch.manual_seed(C)
    dev = torch.device("cuda:0")
    b = _batch("mixed4")
    x = torch.randn(b["x"].shape[0], C)
    torch.set_num_threads(1)
    ref = (rm.global_mean_pool if mean else rm.global_add_pool)(x, b["batch"])
    xd = x.to(dev).requires_grad_(True)
    out = (E.global_mean_pool if mean else E.global_add_pool)(xd, b["batch"].to(dev))
    if mean:
        assert torch.allclose(out.cpu(), ref, rtol=1e-6, atol=1e-6)
    else:
        assert torch.equal(out.cpu(), ref)
    g = torch.randn_like(ref)
    out.backward(g.to(dev))
    x64 = x.double().requires_grad_(True)
    r64 = (rm.global_mean_pool if mean else rm.global_add_pool)(x64, b["batch"])
    r64.backward(g.double())
    _chk(xd.grad, x64.grad, "pool dx")


def test_gineplus_against_message_passing_loop(E):
    """a-12: GINEPLUS / NAIVEGINEPLUS (modules/gine_operations.py:306-362) vs an fp64 restatement
    (index_select + relu + index_add_ per distance class, vector eps)."""
    from esc_gnn_amd.modules.gine_operations import GINEPLUS, NAIVEGINEPLUS
    torch.manual_seed(5)
    dev = torch.device("cuda:0")
    b = _batch("mixed4")
    N, dim, k = b["x"].shape[0], 64, 3
    ei = b["edge_index"][:, b["edge_index"][0] != b["edge_index"][1]]
    # synthetic multi-hop edge list: distance-1 = the graph's edges, distance 2/3 = random pairs
    far = torch.randint(0, N, (2, 400))
    mh = torch.cat([ei, far], dim=1)
    dist = torch.cat([torch.ones(ei.size(1), dtype=torch.long), torch.randint(2, k + 1, (400,))])
    ea = torch.randn(ei.size(1), dim)
    xs = [torch.randn(N, dim) for _ in range(k)]
    lin = torch.nn.Linear(dim, dim)

    def ref(XX, eps, W, bias):
        res = (1 + eps[0]) * XX[0]
        for i in range(k):
            sel = mh[:, dist == i + 1]
            msg = XX[i].index_select(0, sel[0])
            if i == 0:
                msg = msg + ea.double()
            res = res + (1 + eps[i + 1]) * torch.zeros_like(XX[i]).index_add(0, sel[1], msg.relu())
        return res @ W.t() + bias

    conv = GINEPLUS(E.Linear(dim, dim), dim, k=k)
    conv.nn.load_state_dict(lin.state_dict())
    with torch.no_grad():
        conv.eps.copy_(0.1 * torch.randn(k + 1, dim))
    eps0 = conv.eps.detach().clone()
    conv = conv.to(dev)
    xd = [t.to(dev).requires_grad_(True) for t in xs]
    ead = ea.to(dev).requires_grad_(True)
    out = conv(xd, mh.to(dev), dist.to(dev), ead)[0]
    x64 = [t.double().requires_grad_(True) for t in xs]
    r = ref(x64, eps0.double(), lin.weight.double(), lin.bias.double())
    _chk(out, r, "GINEPLUS forward")
    g = torch.randn(N, dim)
    out.backward(g.to(dev))
    r.backward(g.double())
    for a, b64 in zip(xd, x64):
        _chk(a.grad, b64.grad, "GINEPLUS dx")
    naive = NAIVEGINEPLUS(E.Linear(dim, dim), dim, k=k).to(dev)
    naive.nn.load_state_dict(lin.state_dict())
    with torch.no_grad():
        naive.eps.copy_(eps0.to(dev))
    o2 = naive(xs[0].to(dev), mh.to(dev), dist.to(dev), ea.to(dev))
    r2 = ref([xs[0].double()] * k, eps0.double(), lin.weight.double(), lin.bias.double())
    _chk(o2, r2, "NAIVEGINEPLUS forward")


@pytest.mark.parametrize("M,N,K", [(15200, 256, 256), (2400, 256, 256), (2401, 256, 1280), (333, 256, 10), (50, 300, 64),
                                   (33, 64, 16), (31, 40, 8), (2400, 300, 300), (9000, 600, 300), (256, 300, 600),
                                   (20000, 300, 300), (6500, 600, 300)])       # (the last two: 300 / 600-wide statistics epilogues of the 128x64 and 64x64 tiles)
@pytest.mark.parametrize("last_block", [0, 1])
def test_linear_with_fused_batchnorm_statistics(E, M, N, K, last_block):
    """esc_linear_bn_fwd: GEMM + statistics epilogue + merge (finalize launch, or knob 8: by the last workgroups of
    the GEMM), against fp64 BatchNorm."""
    import ctypes
    nv = E._native
    nv.call("esc_tune_set", 8, last_block)
    torch.manual_seed(M + N)
    dev = torch.device("cuda:0")
    x, w, bias = torch.randn(M, K) * 2 + 1, torch.randn(N, K) / K ** 0.5, torch.randn(N)
    gamma, beta = torch.rand(N) + 0.5, torch.randn(N)
    rm0, rv0 = torch.randn(N), torch.rand(N) + 0.5
    xd, wd, bd, gd, btd, rmd, rvd = (t.to(dev).contiguous() for t in (x, w, bias, gamma, beta, rm0, rv0))
    y = torch.empty(M, N, device=dev)
    stats = torch.zeros(((M + 31) // 32) * N * 2, device=dev)
    mean, invstd, scale, shift = (torch.empty(N, device=dev) for _ in range(4))
    for rep in range(3):                                   # the ticket counters must be reusable launch after launch
        f = nv.BnFuse(1e-5, 0.1, nv.ptr(mean), nv.ptr(invstd), nv.ptr(rmd) if rep == 0 else None,
                      nv.ptr(rvd) if rep == 0 else None, nv.ptr(gd), nv.ptr(btd), nv.ptr(scale), nv.ptr(shift))
        mean.fill_(float("nan"))
        nv.call("esc_linear_bn_fwd", nv.ptr(xd), K, nv.ptr(wd), K, nv.ptr(bd), None, None, M, N, K, nv.ptr(y), N,
                nv.ptr(stats), ctypes.byref(f), nv.stream())
        r = x.double() @ w.double().t() + bias.double()
        mu, var = r.mean(0), r.var(0, unbiased=False)
        _chk(y, r, "y")
        _chk(mean, mu, "mean")
        _chk(invstd, 1 / torch.sqrt(var + 1e-5), "invstd")
        sc = gamma.double() / torch.sqrt(var + 1e-5)
        _chk(scale, sc, "scale")
        _chk(shift, beta.double() - mu * sc, "shift")
    nv.call("esc_tune_set", 8, 0)
    _chk(rmd, 0.9 * rm0.double() + 0.1 * mu, "running_mean")
    _chk(rvd, 0.9 * rv0.double() + 0.1 * r.var(0, unbiased=True), "running_var")


@pytest.mark.parametrize("M,K", [(2400, 256), (333, 64), (5, 128)])
def test_prediction_head_leaves_the_l1_gradient(E, M, K):
    """esc_linear_fwd_l1 (the H -> 1 head of a training step) = esc_linear_fwd with the BatchNorm+ReLU prologue followed by
    esc_l1_loss's dpred: predictions and gradient identical bit for bit (ties pred == target give 0 like torch's sign)."""
    nv = E._native
    torch.manual_seed(M + K)
    dev = torch.device("cuda:0")
    x, w, b = torch.randn(M, K).to(dev), (torch.randn(1, K) / K ** 0.5).to(dev), torch.randn(1).to(dev)
    sc, sh = (torch.rand(K) + 0.5).to(dev), (torch.randn(K) * 0.3).to(dev)
    want_pred = torch.empty(M, device=dev)
    nv.call("esc_linear_fwd", nv.ptr(x), K, nv.ptr(w), K, nv.ptr(b), nv.ptr(sc), nv.ptr(sh), M, 1, K, nv.ptr(want_pred), 1, None, nv.stream())
    y = torch.randn(M, device=dev)
    y[::7] = want_pred[::7]                                          # exact ties
    loss, want_d = torch.empty(1, device=dev), torch.empty(M, device=dev)
    nv.call("esc_l1_loss", nv.ptr(want_pred), nv.ptr(y), M, M, 1.0, nv.ptr(loss), nv.ptr(want_d), nv.stream())
    assert nv.lib().esc_linear_fwd_l1_ok(nv.ptr(x), K, nv.ptr(w), K, nv.ptr(sc), nv.ptr(sh)) == 1
    pred, d = torch.full((M,), float("nan"), device=dev), torch.full((M,), float("nan"), device=dev)
    nv.call("esc_linear_fwd_l1", nv.ptr(x), K, nv.ptr(w), nv.ptr(b), nv.ptr(sc), nv.ptr(sh), M, K, nv.ptr(y), M, 1.0, nv.ptr(pred), nv.ptr(d),
            nv.stream())
    assert torch.equal(pred, want_pred) and torch.equal(d, want_d)
    assert float(d[::7].abs().max()) == 0.0


@pytest.mark.parametrize("M,N,K0,K1,pro", [(2400, 256, 1024, 256, True), (333, 64, 96, 32, False), (2401, 256, 256, 256, True),
                                          (15200, 256, 512, 256, True)])
def test_linear_forward_cut_in_two_over_its_reduction(E, M, N, K0, K1, pro):
    """esc_linear_fwd over the first K0 input columns (no bias) + esc_linear_fwd_from over the last K1 starting from that partial
    result = the one-launch Linear over all K0 + K1 columns (run_graphcount.py:183-185, the readout over the layer concat): outputs
    against fp64 and against the one-launch result (the same numbers up to the order of the fp32 additions), and the BatchNorm
    partials of the epilogue describe the COMPLETE sums (same mean / invstd as the one-launch partials)."""
    nv = E._native
    torch.manual_seed(M + K0)
    dev = torch.device("cuda:0")
    K = K0 + K1
    x, w, bias = torch.randn(M, K) + 0.3, torch.randn(N, K) / K ** 0.5, torch.randn(N)
    sc, sh = torch.rand(K) + 0.5, torch.randn(K) * 0.2
    xd, wd, bd, scd, shd = (t.to(dev).contiguous() for t in (x, w, bias, sc, sh))
    a = torch.relu(x.double() * sc.double() + sh.double()) if pro else x.double()
    want = a @ w.double().t() + bias.double()
    p_sc = (lambda off: scd.data_ptr() + 4 * off) if pro else (lambda off: None)
    p_sh = (lambda off: shd.data_ptr() + 4 * off) if pro else (lambda off: None)
    nstat = ((M + 31) // 32) * N * 2
    one, st_one = torch.empty(M, N, device=dev), torch.zeros(nstat, device=dev)
    nv.call("esc_linear_fwd", nv.ptr(xd), K, nv.ptr(wd), K, nv.ptr(bd), p_sc(0), p_sh(0), M, N, K, nv.ptr(one), N, nv.ptr(st_one), nv.stream())
    assert nv.lib().esc_linear_fwd_from_ok(xd.data_ptr() + 4 * K0, K, wd.data_ptr() + 4 * K0, K, M, N, K1, int(pro)) == 1
    part, two, st_two = torch.empty(M, N, device=dev), torch.full((M, N), float("nan"), device=dev), torch.zeros(nstat, device=dev)
    nv.call("esc_linear_fwd", nv.ptr(xd), K, nv.ptr(wd), K, None, p_sc(0), p_sh(0), M, N, K0, nv.ptr(part), N, None, nv.stream())
    nv.call("esc_linear_fwd_from", nv.ptr(part), N, xd.data_ptr() + 4 * K0, K, wd.data_ptr() + 4 * K0, K, nv.ptr(bd), p_sc(K0), p_sh(K0),
            M, N, K1, nv.ptr(two), N, nv.ptr(st_two), nv.stream())
    _chk(two, want, "two launches vs fp64")
    assert float((two - one).abs().max()) <= 1e-5 * float(one.abs().max()), "two launches vs one"
    outs = []
    for st, k in ((st_one, K), (st_two, K1)):
        mean, invstd = torch.empty(N, device=dev), torch.empty(N, device=dev)
        br = nv.lib().esc_linear_stats_block_rows(nv.ptr(xd), K, nv.ptr(wd), K, M, N, k)
        nv.call("esc_bn_stats_from_partials_rows", nv.ptr(st), M, N, br, 1e-5, 0.1, nv.ptr(mean), nv.ptr(invstd), None, None, None, None, None,
                None, nv.stream())
        outs.append((mean, invstd))
    _chk(outs[1][0], want.mean(0), "mean of the complete sums")
    _chk(outs[1][1], 1 / torch.sqrt(want.var(0, unbiased=False) + 1e-5), "invstd of the complete sums")
    assert torch.allclose(outs[0][0], outs[1][0], rtol=1e-5, atol=1e-6) and torch.allclose(outs[0][1], outs[1][1], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("M,N,K", [(2400, 256, 256), (2401, 256, 10), (333, 64, 64), (15200, 256, 256), (97, 128, 1280),
                                   (333, 64, 300)])
def test_batchnorm_folded_into_its_consumer(E, M, N, K):
    """esc_linear_fwd leaves BatchNorm partials (block height = esc_linear_stats_block_rows); the consumers merge them in
    their prologue: esc_linear_fwd_fold (MFMA tile and the wave-per-row narrow form) and esc_affine_act_fold, against fp64
    BatchNorm + ReLU.  Workgroup 0 must leave mean / invstd / scale / shift and the running statistics."""
    import ctypes
    nv = E._native
    torch.manual_seed(M + N + K)
    dev = torch.device("cuda:0")
    x, w, bias = torch.randn(M, K) * 2 + 1, torch.randn(N, K) / K ** 0.5, torch.randn(N)
    gamma, beta = torch.rand(N) + 0.5, torch.randn(N)
    rm0, rv0 = torch.randn(N), torch.rand(N) + 0.5
    N2 = 256
    w2, b2 = torch.randn(N2, N) / N ** 0.5, torch.randn(N2)
    w3, b3 = torch.randn(1, N) / N ** 0.5, torch.randn(1)
    xd, wd, bd, gd, btd = (t.to(dev).contiguous() for t in (x, w, bias, gamma, beta))
    w2d, b2d, w3d, b3d = (t.to(dev).contiguous() for t in (w2, b2, w3, b3))
    y = torch.empty(M, N, device=dev)
    stats = torch.zeros(((M + 31) // 32) * N * 2, device=dev)
    nv.call("esc_linear_fwd", nv.ptr(xd), K, nv.ptr(wd), K, nv.ptr(bd), None, None, M, N, K, nv.ptr(y), N, nv.ptr(stats), nv.stream())
    br = nv.lib().esc_linear_stats_block_rows(nv.ptr(xd), K, nv.ptr(wd), K, M, N, K)
    assert br in (32, 64, 128)
    r = x.double() @ w.double().t() + bias.double()
    mu, var = r.mean(0), r.var(0, unbiased=False)
    sc = gamma.double() / torch.sqrt(var + 1e-5)
    act = torch.relu(r * sc + (beta.double() - mu * sc))

    def fold(with_running):
        mean, invstd, scale, shift = (torch.full((N,), float("nan"), device=dev) for _ in range(4))
        rmd, rvd = rm0.to(dev), rv0.to(dev)
        f = nv.BnFold(nv.ptr(stats), M, br, N, 1e-5, 0.1, nv.ptr(gd), nv.ptr(btd), nv.ptr(mean), nv.ptr(invstd), nv.ptr(scale),
                      nv.ptr(shift), nv.ptr(rmd) if with_running else None, nv.ptr(rvd) if with_running else None)
        return f, (mean, invstd, scale, shift, rmd, rvd)

    def check_outputs(o, with_running):
        mean, invstd, scale, shift, rmd, rvd = o
        _chk(mean, mu, "mean"); _chk(invstd, 1 / torch.sqrt(var + 1e-5), "invstd")
        _chk(scale, sc, "scale"); _chk(shift, beta.double() - mu * sc, "shift")
        if with_running:
            _chk(rmd, 0.9 * rm0.double() + 0.1 * mu, "running_mean")
            _chk(rvd, 0.9 * rv0.double() + 0.1 * r.var(0, unbiased=True), "running_var")

    # 1. the elementwise consumer
    f, o = fold(True)
    out = torch.full((M, N), float("nan"), device=dev)
    nv.call("esc_affine_act_fold", nv.ptr(y), N, M, N, ctypes.byref(f), 1, nv.ptr(out), N, nv.stream())
    _chk(out, act, "affine_act_fold")
    check_outputs(o, True)
    # 2. the next Linear on the matrix cores (N % 32 == 0: every shape here), with its own statistics epilogue
    f, o = fold(False)
    y2 = torch.full((M, N2), float("nan"), device=dev)
    stats2 = torch.zeros(((M + 31) // 32) * N2 * 2, device=dev)
    nv.call("esc_linear_fwd_fold", nv.ptr(y), N, nv.ptr(w2d), N, nv.ptr(b2d), ctypes.byref(f), M, N2, N, nv.ptr(y2), N2,
            nv.ptr(stats2), nv.stream())
    r2 = act @ w2.double().t() + b2.double()
    _chk(y2, r2, "linear_fwd_fold")
    check_outputs(o, False)
    br2 = nv.lib().esc_linear_stats_block_rows(nv.ptr(y), N, nv.ptr(w2d), N, M, N2, N)
    m2, i2 = torch.empty(N2, device=dev), torch.empty(N2, device=dev)
    nv.call("esc_bn_stats_from_partials_rows", nv.ptr(stats2), M, N2, br2, 1e-5, 0.1, nv.ptr(m2), nv.ptr(i2), None, None, None, None,
            None, None, nv.stream())
    _chk(m2, r2.mean(0), "mean of the folded layer's output")
    _chk(i2, 1 / torch.sqrt(r2.var(0, unbiased=False) + 1e-5), "invstd of the folded layer's output")
    # 3. the wave-per-row narrow form (lin2: H -> 1)
    if N <= 256:
        f, o = fold(False)
        y3 = torch.full((M, 1), float("nan"), device=dev)
        nv.call("esc_linear_fwd_fold", nv.ptr(y), N, nv.ptr(w3d), N, nv.ptr(b3d), ctypes.byref(f), M, 1, N, nv.ptr(y3), 1, None, nv.stream())
        _chk(y3, act @ w3.double().t() + b3.double(), "narrow linear_fwd_fold")
        check_outputs(o, False)


@pytest.mark.parametrize("M,C", [(2400, 256), (50, 300), (4096, 64)])
def test_batchnorm_backward_with_last_block_finalize(E, M, C):
    """knob 8: the BatchNorm-backward column sums are folded by the last workgroup of the partial kernel."""
    nv = E._native
    torch.manual_seed(M + C)
    dev = torch.device("cuda:0")
    x = torch.randn(M, C) * 2 - 1
    gamma, beta = torch.rand(C) + 0.5, torch.randn(C)
    g = torch.randn(M, C)
    res = []
    for knob in (0, 1, 1):
        nv.call("esc_tune_set", 8, knob)
        xd, gd, bd = (t.to(dev).requires_grad_(True) for t in (x, gamma, beta))
        y = E.ops.batch_norm_act(xd, gd, bd, torch.zeros(C, device=dev), torch.ones(C, device=dev), 1e-5, 0.1, True)
        y.backward(g.to(dev))
        res.append((xd.grad.cpu(), gd.grad.cpu(), bd.grad.cpu()))
    nv.call("esc_tune_set", 8, 0)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    r = torch.nn.functional.batch_norm(x64, None, None, g64, b64, True, 0.1, 1e-5).relu()
    r.backward(g.double())
    for dx, dg, db in res:
        _chk(dx, x64.grad, "dx")
        _chk(dg, g64.grad, "dgamma")
        _chk(db, b64.grad, "dbeta")


def test_reduce_sum_jobs(E):
    import ctypes
    nv = E._native

    class Job(ctypes.Structure):
        _fields_ = [("v", ctypes.c_void_p), ("n", ctypes.c_int64), ("out", ctypes.c_void_p)]
    torch.manual_seed(0)
    dev = torch.device("cuda:0")
    vecs = [torch.randn(n, device=dev) for n in (2400, 1, 0, 70000) + tuple(range(5, 22))]
    outs = torch.full((len(vecs),), float("nan"), device=dev)
    jobs = (Job * len(vecs))(*[Job(v.data_ptr() if v.numel() else None, v.numel(), outs[i:].data_ptr())
                               for i, v in enumerate(vecs)])
    nv.call("esc_reduce_sum_jobs", ctypes.cast(jobs, ctypes.c_void_p), len(vecs), nv.stream())
    want = torch.tensor([float(v.double().sum()) for v in vecs])
    assert torch.allclose(outs.cpu().double(), want.double(), rtol=1e-6, atol=1e-6)


# ---- building blocks of the ZINC / OGB step engines (csrc/embed.hip, bag.hip) -------------------------------------------
@pytest.mark.parametrize("M,rows,C", [(6400, 100, 32), (2400, 28, 32), (20000, 5, 300), (256, 1, 300), (3, 7, 8), (17000, 3, 64), (5000, 9, 12), (9000, 4, 256)])
def test_small_table_embedding_kernels(E, M, rows, C):
    """esc_embed_fwd / esc_embed_bwd (type-embedding lookups of zinc_models.py:581,591) against index_select / index_add_
    in fp64; the gradient is bitwise reproducible; an out-of-range index yields a zero row and raises the flag."""
    from esc_gnn_amd import _native as nv
    dev = torch.device("cuda:0")
    g0 = torch.Generator().manual_seed(M + rows)
    table = torch.randn(rows, C, generator=g0)
    idx = torch.randint(0, rows, (M,), generator=g0)
    if M > 10:
        idx[: M // 2] = idx[0]                                   # one dominant type, like carbon
    td, idd = table.to(dev), idx.to(dev)
    ld = C + 4
    out = torch.zeros(M, ld, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    nv.call("esc_embed_fwd", nv.ptr(td), rows, C, nv.ptr(idd), M, nv.ptr(out), ld, nv.ptr(bad), nv.stream())
    assert torch.equal(out[:, :C].cpu(), table[idx]) and int(bad.item()) == 0 and float(out[:, C:].abs().max()) == 0
    gr = torch.randn(M, ld, generator=g0)
    grd = gr.to(dev)
    dts = []
    for _ in range(2):
        dt = torch.full((rows, C), float("nan"), device=dev)
        nv.call("esc_embed_bwd", nv.ptr(grd), ld, nv.ptr(idd), M, rows, C, nv.ptr(dt), nv.stream())
        dts.append(dt.cpu())
    want = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, idx, gr[:, :C].double())
    assert torch.equal(dts[0], dts[1])
    assert torch.allclose(dts[0].double(), want, rtol=1e-5, atol=1e-5 * max(1.0, float(want.abs().max())))
    idd2 = idd.clone(); idd2[M // 2] = rows
    nv.call("esc_embed_fwd", nv.ptr(td), rows, C, nv.ptr(idd2), M, nv.ptr(out), ld, nv.ptr(bad), nv.stream())
    assert int(bad.item()) == 1 and float(out[M // 2].abs().max()) == 0


@pytest.mark.parametrize("M,C,p", [(20000, 300, 0.65), (6500, 300, 0.5), (256, 300, 0.0), (1000, 64, 0.1)])
def test_dropout_kernels(E, M, C, p):
    """esc_dropout_fwd / _bwd: keep rate 1-p, kept values scaled by 1/(1-p), the optional residual added after the
    dropout, backward = the same mask; a different seed draws a different mask, the same seed the same one."""
    from esc_gnn_amd import _native as nv
    dev = torch.device("cuda:0")
    x = torch.randn(M, C, device=dev) + 3.0
    res = torch.randn(M, C, device=dev)
    y, y2, y3 = (torch.empty(M, C, device=dev) for _ in range(3))
    m1, m2, m3 = (torch.zeros(M * C, dtype=torch.uint8, device=dev) for _ in range(3))
    nv.call("esc_dropout_fwd", nv.ptr(x), C, M, C, p, 1234, nv.ptr(res), C, nv.ptr(y), C, nv.ptr(m1), nv.stream())
    nv.call("esc_dropout_fwd", nv.ptr(x), C, M, C, p, 1234, None, 0, nv.ptr(y2), C, nv.ptr(m2), nv.stream())
    nv.call("esc_dropout_fwd", nv.ptr(x), C, M, C, p, 99, None, 0, nv.ptr(y3), C, nv.ptr(m3), nv.stream())
    if p == 0:
        assert torch.equal(y, x + res) and torch.equal(y2, x)
        return
    keep = m1.view(M, C).bool()
    assert torch.equal(m1, m2) and not torch.equal(m1, m3)
    rate = float(keep.float().mean())
    assert abs(rate - (1 - p)) < 4 * (p * (1 - p) / (M * C)) ** 0.5 + 1e-3
    scale = float(np.float32(1.0 / (1.0 - float(np.float32(p)))))
    assert torch.equal(y2, torch.where(keep, x * scale, torch.zeros_like(x)))
    assert torch.equal(y, y2 + res)
    col_rate = keep.float().mean(0)                              # no column or row structure in the mask
    assert float(col_rate.min()) > (1 - p) - 0.05 and float(col_rate.max()) < (1 - p) + 0.05
    dy = torch.randn(M, C, device=dev)
    dx = torch.empty(M, C, device=dev)
    nv.call("esc_dropout_bwd", nv.ptr(dy), C, M, C, p, nv.ptr(m1), nv.ptr(res), C, nv.ptr(dx), C, nv.stream())
    assert torch.equal(dx, torch.where(keep, dy * scale, torch.zeros_like(dy)) + res)


@pytest.mark.parametrize("M,C,p,act", [(6500, 300, 0.65, 1), (6500, 300, 0.5, 0), (256, 300, 0.0, 1), (1000, 64, 0.1, 1)])
def test_affine_act_dropout_is_the_two_kernels_in_one(E, M, C, p, act):
    """esc_affine_act_dropout_fwd == esc_affine_act followed by esc_dropout_fwd, bit for bit (values and keep mask)"""
    from esc_gnn_amd import _native as nv
    dev = torch.device("cuda:0")
    x = torch.randn(M, C, device=dev)
    sc, sh = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    res = torch.randn(M, C, device=dev)
    mid, want, got = (torch.empty(M, C, device=dev) for _ in range(3))
    m_want, m_got = (torch.zeros(M * C, dtype=torch.uint8, device=dev) for _ in range(2))
    nv.call("esc_affine_act", nv.ptr(x), C, M, C, nv.ptr(sc), nv.ptr(sh), act, nv.ptr(mid), C, nv.stream())
    nv.call("esc_dropout_fwd", nv.ptr(mid), C, M, C, p, 77, nv.ptr(res), C, nv.ptr(want), C, nv.ptr(m_want), nv.stream())
    nv.call("esc_affine_act_dropout_fwd", nv.ptr(x), C, M, C, nv.ptr(sc), nv.ptr(sh), act, p, 77, nv.ptr(res), C, nv.ptr(got), C,
            nv.ptr(m_got), nv.stream())
    assert torch.equal(got, want) and torch.equal(m_got, m_want)
    if act == 1 and p == 0:
        assert torch.equal(got, torch.relu(torch.addcmul(sh, x, sc)) + res) or torch.allclose(got, torch.relu(x * sc + sh) + res, atol=1e-6)


@pytest.mark.parametrize("M,C,p,relu,on_output", [(6500, 300, 0.65, 1, 0), (6500, 300, 0.5, 0, 0), (20000, 300, 0.65, 1, 1),
                                                  (256, 600, 0.3, 1, 0), (1000, 64, 0.1, 1, 1)])
def test_bn_backward_with_dropout_folded_in(E, M, C, p, relu, on_output):
    """esc_bn_bwd_dropout == esc_dropout_bwd -> esc_bn_bwd (mask on the incoming gradient) or esc_bn_bwd -> esc_dropout_bwd
    (mask on the result), bit for bit: dX, dgamma, dbeta"""
    from esc_gnn_amd import _native as nv
    dev = torch.device("cuda:0")
    torch.manual_seed(M + C)
    x = torch.randn(M, C, device=dev) * 2 + 0.5
    dy = torch.randn(M, C, device=dev)
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.3
    mean, var = x.mean(0).contiguous(), x.var(0, unbiased=False)
    invstd = (1.0 / torch.sqrt(var + 1e-5)).contiguous()
    mask = (torch.rand(M * C, device=dev) >= p).to(torch.uint8)
    scratch = torch.empty(nv.lib().esc_bn_scratch(C), device=dev)
    assert nv.lib().esc_bn_bwd_dropout_ok(C, C, C, C)

    def run(fused):
        dx, dg, db = torch.empty(M, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
        if fused:
            nv.call("esc_bn_bwd_dropout", nv.ptr(x), C, nv.ptr(dy), C, M, C, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta),
                    relu, nv.ptr(mask), p, on_output, nv.ptr(dx), C, nv.ptr(dg), nv.ptr(db), nv.ptr(scratch), nv.stream())
        elif on_output:
            nv.call("esc_bn_bwd", nv.ptr(x), C, None, 0, nv.ptr(dy), C, M, C, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta),
                    relu, nv.ptr(dx), C, nv.ptr(dg), nv.ptr(db), nv.ptr(scratch), nv.stream())
            nv.call("esc_dropout_bwd", nv.ptr(dx), C, M, C, p, nv.ptr(mask), None, 0, nv.ptr(dx), C, nv.stream())
        else:
            t = torch.empty(M, C, device=dev)
            nv.call("esc_dropout_bwd", nv.ptr(dy), C, M, C, p, nv.ptr(mask), None, 0, nv.ptr(t), C, nv.stream())
            nv.call("esc_bn_bwd", nv.ptr(x), C, None, 0, nv.ptr(t), C, M, C, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta),
                    relu, nv.ptr(dx), C, nv.ptr(dg), nv.ptr(db), nv.ptr(scratch), nv.stream())
        return dx, dg, db

    got, want = run(True), run(False)
    for a, b, name in zip(got, want, ("dX", "dgamma", "dbeta")):
        # (the two-step form may take the node-sized one-workgroup-finalize route: same sums, possibly another order)
        assert torch.equal(a, b) or torch.allclose(a, b, rtol=2e-6, atol=2e-6 * float(b.abs().max())), name
    keep = mask.view(M, C).bool()
    if on_output:
        assert float(got[0][~keep].abs().max()) == 0


def test_broadcast_add_table_pack_and_accumulating_bag(E):
    """esc_segment_broadcast_add (h + vn[batch]), esc_table_pack / _unpack_grad and esc_bag_fwd_acc against torch"""
    import ctypes
    from esc_gnn_amd import _native as nv
    from esc_gnn_amd.engine import _TableList
    dev = torch.device("cuda:0")
    g0 = torch.Generator().manual_seed(5)
    sizes = torch.randint(1, 40, (300,), generator=g0)
    sizes[7] = 0 if False else sizes[7]
    ptr = torch.zeros(301, dtype=torch.int32); ptr[1:] = torch.cumsum(sizes, 0)
    N, G, C = int(ptr[-1]), 300, 300
    x, rows = torch.randn(N, C, generator=g0), torch.randn(G, C, generator=g0)
    batch = torch.repeat_interleave(torch.arange(G), sizes)
    out = torch.empty(N, C, device=dev)
    xd, rd, pd = x.to(dev), rows.to(dev), ptr.to(dev)
    nv.call("esc_segment_broadcast_add", nv.ptr(xd), C, nv.ptr(rd), C, nv.ptr(pd), G, N, C, nv.ptr(out), C, nv.stream())
    assert torch.equal(out.cpu(), x + rows[batch])
    nv.call("esc_segment_broadcast_add", None, 0, nv.ptr(rd), C, nv.ptr(pd), G, N, C, nv.ptr(out), C, nv.stream())
    assert torch.equal(out.cpu(), rows[batch])
    # tables
    dims = (119, 5, 12, 2)
    tabs = [torch.randn(d, C, generator=g0).to(dev) for d in dims]
    grads = [torch.zeros(d, C, device=dev) for d in dims]
    tl = _TableList()
    tl.count = len(dims)
    for j, (t, gr) in enumerate(zip(tabs, grads)):
        tl.rows[j], tl.w[j], tl.dw[j] = t.size(0), t.data_ptr(), gr.data_ptr()
    cat = torch.empty(sum(dims), C, device=dev)
    nv.call("esc_table_pack", ctypes.byref(tl), C, nv.ptr(cat), nv.stream())
    assert torch.equal(cat, torch.cat(tabs))
    dcat = torch.randn(sum(dims), C, device=dev)
    nv.call("esc_table_unpack_grad", ctypes.byref(tl), C, nv.ptr(dcat), nv.stream())
    assert torch.equal(torch.cat(grads), dcat)
    # bag that adds onto its output
    n = 500
    index = torch.stack([torch.randint(0, d, (n,), generator=g0) for d in dims], 1).to(dev)
    plan = E.ops.embed_plan(index, dims)
    base = torch.randn(n, C, device=dev)
    acc = base.clone()
    nv.call("esc_bag_fwd_acc", nv.ptr(cat), C, nv.ptr(plan["row_ptr"]), nv.ptr(plan["idx32"]), nv.ptr(plan["ones"]), n, nv.ptr(acc), C,
            nv.stream())
    want = base.clone()
    offs = [0, 119, 124, 136]
    for j in range(len(dims)):
        want = want + cat[index[:, j] + offs[j]]
    assert torch.equal(acc, want)


@pytest.mark.parametrize("n,dims", [(6500, (119, 4, 12, 12, 10, 6, 6, 2, 2)), (20181, (5, 6, 2)), (1, (3,)), (0, (7, 2)),
                                    (333, (100,)), (5000, (300, 70000))])
def test_embed_plan_arrays(E, n, dims):
    """esc_embed_plan (ops.embed_plan): every array of the plan against a numpy restatement — flat keys, row pointers,
    stable grouping by table row (CSC) — bit-exact; an id outside its table raises unless the caller vouched for the range"""
    dev = torch.device("cuda:0")
    g0 = torch.Generator().manual_seed(n + len(dims))
    k = len(dims)
    index = torch.stack([torch.randint(0, d, (n,), generator=g0) for d in dims], 1).to(dev) if n else torch.zeros(0, k, dtype=torch.int64, device=dev)
    plan = E.ops.embed_plan(index, dims)
    offs = np.concatenate([[0], np.cumsum(dims)[:-1]])
    flat = (index.cpu().numpy() + offs[None, :]).reshape(-1)
    rows = int(sum(dims))
    order = np.argsort(flat, kind="stable")
    assert plan["entries"] == n * k and plan["rows"] == rows
    assert np.array_equal(plan["idx32"].cpu().numpy(), flat.astype(np.int32))
    assert np.array_equal(plan["row_ptr"].cpu().numpy(), np.arange(0, n * k + 1, k, dtype=np.int32))
    assert np.array_equal(plan["ones"].cpu().numpy(), np.ones(n * k, dtype=np.int32))
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=rows))]).astype(np.int32)
    assert np.array_equal(plan["col_ptr"].cpu().numpy(), want_ptr)
    assert np.array_equal(plan["c_row"].cpu().numpy(), (order // k).astype(np.int32))
    assert np.array_equal(plan["c_col"].cpu().numpy(), flat[order].astype(np.int32))
    assert E.ops.embed_plan(index, dims) is plan                     # cached on the index tensor
    if n > 1:
        bad = index.clone()
        bad[n // 2, k - 1] = dims[-1]
        with pytest.raises(IndexError):
            E.ops.embed_plan(bad, dims)
        neg = index.clone()
        neg[0, 0] = -1
        with pytest.raises(IndexError):
            E.ops.embed_plan(neg, dims)
    with pytest.raises(ValueError):
        E.ops.embed_plan(torch.zeros(4, k + 1, dtype=torch.int64, device=dev), dims)


def test_scatter_add_execution_window_on_the_device_clock(E):
    """esc_prof_span_arm / _read: the armed launches of the scatter-add run the stamped instantiation (same result, bit for bit) and
    report a positive execution window that is no longer than the event pair of the same launch (pair = dispatch gap + kernel);
    launches beyond the armed count carry no stamps."""
    from esc_gnn_amd import _native as nv
    dev = torch.device("cuda:0")
    b = _batch()
    plan = _plan(E, b, dev)
    N, Ee, C = plan.num_nodes, plan.num_edges, 256
    g0 = torch.Generator().manual_seed(11)
    x, e = torch.randn(N, C, generator=g0).to(dev), torch.randn(Ee, C, generator=g0).to(dev)
    sc, sh = (torch.rand(C, generator=g0) + 0.5).to(dev), torch.randn(C, generator=g0).to(dev)
    eps = torch.tensor([0.3], device=dev)
    s = nv.stream()

    def run():
        out = torch.empty(N, C, device=dev)
        nv.call("esc_gine_aggregate_fwd_affine", nv.ptr(x), C, nv.ptr(sc), nv.ptr(sh), nv.ptr(e), C, nv.ptr(plan.in_ptr), nv.ptr(plan.in_edge),
                nv.ptr(plan.in_src), nv.ptr(eps), N, C, nv.ptr(out), C, s)
        return out
    want = run()
    nv.prof_reset("agg_fwd")
    nv.prof_span_arm("agg_fwd", 2)
    nv.prof_enable("agg_fwd", True)
    try:
        outs = [run() for _ in range(3)]
        torch.cuda.synchronize()
    finally:
        nv.prof_enable("agg_fwd", False)
    for o in outs:
        assert torch.equal(o, want)
    spans = nv.prof_span_read("agg_fwd")
    pairs = [1e3 * ms for ms in nv.prof_read_all("agg_fwd")]
    assert len(spans) == 2 and len(pairs) == 3                 # the third launch was not armed
    for sp, pr in zip(spans, pairs):
        assert 0.0 < sp <= pr + 0.5, (sp, pr)
    nv.prof_reset("agg_fwd")


def test_aggregate_with_on_the_fly_batchnorm_relu_matches_the_materialised_path(E):
    """esc_gine_aggregate_fwd_affine / _bwd_affine (the layer input given as pre-BatchNorm rows + (scale, shift)) against
    esc_affine_act followed by the plain aggregate kernels: forward BIT-identical (same fmaf + max, same summation order),
    backward d_e / dx / deps identical"""
    from esc_gnn_amd import _native as nv
    dev = torch.device("cuda:0")
    b = _batch()
    plan = _plan(E, b, dev)
    N, Ee, C = plan.num_nodes, plan.num_edges, 256
    g0 = torch.Generator().manual_seed(9)
    ld = C + 8
    x = torch.randn(N, ld, generator=g0).to(dev)
    e = torch.randn(Ee, C, generator=g0).to(dev)
    sc, sh = (torch.rand(C, generator=g0) + 0.5).to(dev), torch.randn(C, generator=g0).to(dev)
    eps = torch.tensor([0.3], device=dev)
    s = nv.stream()
    xa = torch.empty(N, C, device=dev)
    nv.call("esc_affine_act", nv.ptr(x), ld, N, C, nv.ptr(sc), nv.ptr(sh), 1, nv.ptr(xa), C, s)
    want, got = torch.empty(N, C, device=dev), torch.empty(N, C, device=dev)
    nv.call("esc_gine_aggregate_fwd", nv.ptr(xa), C, nv.ptr(e), C, nv.ptr(plan.in_ptr), nv.ptr(plan.in_edge), nv.ptr(plan.in_src),
            nv.ptr(eps), N, C, nv.ptr(want), C, s)
    nv.call("esc_gine_aggregate_fwd_affine", nv.ptr(x), ld, nv.ptr(sc), nv.ptr(sh), nv.ptr(e), C, nv.ptr(plan.in_ptr), nv.ptr(plan.in_edge),
            nv.ptr(plan.in_src), nv.ptr(eps), N, C, nv.ptr(got), C, s)
    assert torch.equal(got, want)
    g = torch.randn(N, C, generator=g0).to(dev)
    outs = []
    for affine in (False, True):
        de = torch.empty(Ee, C, device=dev)
        dx = torch.full((N, C), 0.25, device=dev)            # accumulate_dx = 1: added onto what is there
        dp = torch.empty(N * int(nv.lib().esc_gine_aggregate_bwd_deps_slots(C)), device=dev)
        if affine:
            nv.call("esc_gine_aggregate_bwd_affine", nv.ptr(x), ld, nv.ptr(sc), nv.ptr(sh), nv.ptr(e), C, nv.ptr(g), C, nv.ptr(plan.out_ptr),
                    nv.ptr(plan.out_edge), nv.ptr(plan.out_dst), nv.ptr(eps), N, C, nv.ptr(de), C, nv.ptr(dx), C, 1, nv.ptr(dp), s)
        else:
            nv.call("esc_gine_aggregate_bwd", nv.ptr(xa), C, nv.ptr(e), C, nv.ptr(g), C, nv.ptr(plan.out_ptr), nv.ptr(plan.out_edge),
                    nv.ptr(plan.out_dst), nv.ptr(eps), N, C, nv.ptr(de), C, nv.ptr(dx), C, 1, nv.ptr(dp), s)
        outs.append((de, dx, dp))
    for a, c in zip(outs[0], outs[1]):
        assert torch.equal(a, c)
    with pytest.raises(RuntimeError):                        # narrow rows have no affine variant
        nv.call("esc_gine_aggregate_fwd_affine", nv.ptr(x), ld, nv.ptr(sc), nv.ptr(sh), nv.ptr(e), C, nv.ptr(plan.in_ptr), nv.ptr(plan.in_edge),
                nv.ptr(plan.in_src), nv.ptr(eps), N, 32, nv.ptr(got), C, s)
    # ... and the variant that leaves the column sums of the BatchNorm backward in front of it (r03): same d_e / dx / deps bits,
    # partials that finalize to what esc_bn_bwd_coef computes from (x, dx)
    mean = (-sh / sc).contiguous()                           # any per-column statistics will do for the sums
    invstd = (torch.rand(C, generator=g0) + 0.5).to(dev)
    slots = int(nv.lib().esc_gine_aggregate_bwd_stats_slots(N))
    part = torch.full((slots, C, 2), float("nan"), device=dev)
    de2, dx2 = torch.empty(Ee, C, device=dev), torch.full((N, C), 0.25, device=dev)
    dp2 = torch.empty(N * int(nv.lib().esc_gine_aggregate_bwd_deps_slots(C)), device=dev)
    nv.call("esc_gine_aggregate_bwd_affine_stats", nv.ptr(x), ld, nv.ptr(sc), nv.ptr(sh), nv.ptr(mean), nv.ptr(invstd), nv.ptr(e), C, nv.ptr(g), C,
            nv.ptr(plan.out_ptr), nv.ptr(plan.out_edge), nv.ptr(plan.out_dst), nv.ptr(eps), N, C, nv.ptr(de2), C, nv.ptr(dx2), C, 1, nv.ptr(dp2),
            nv.ptr(part), s)
    assert torch.equal(de2, outs[1][0]) and torch.equal(dx2, outs[1][1]) and torch.equal(dp2, outs[1][2])
    assert not bool(torch.isnan(part).any())
    xs = x[:, :C].double().cpu()
    pre = xs * sc.double().cpu() + sh.double().cpu()
    gm = torch.where(pre > 0, dx2.double().cpu(), torch.zeros((), dtype=torch.float64))
    xh = (xs - mean.double().cpu()) * invstd.double().cpu()
    _chk(part[:, :, 0].sum(0), gm.sum(0), "sum g from the aggregate backward")
    _chk(part[:, :, 1].sum(0), (gm * xh).sum(0), "sum g*xhat from the aggregate backward")


@pytest.mark.parametrize("M,N,K,relu,pro,acc,nxt", [
    (2400, 256, 256, 1, True, 0, True),      # GINEConv.nn.4 backward: BatchNorm1 apply in front, BatchNorm0 sums behind
    (2400, 256, 256, 1, False, 1, False),    # ... accumulating dX
    (2400, 256, 1024, 1, True, 0, False),    # readout lin1, the edge stream's column block
    (2400, 256, 10, 1, False, 0, False),     # conv1.nn.0 / x_embedding.0: the narrow-input kernels
    (77, 64, 96, 0, False, 0, True),         # ragged rows, no activation
    (1500, 300, 600, 1, True, 0, True),      # widths that are not multiples of the 32-wide K-step
    (333, 128, 16, 1, True, 0, False),
    (2400, 256, 256, 2, False, 0, True),     # ELU behind both BatchNorms (zinc_models.py:513-522), materialised hidden activation
    (3100, 256, 44, 2, False, 0, False),
    (15200, 256, 256, 1, False, 0, True),    # z_embedding.3 backward (edge rows: the 128x128 tile), both BatchNorms of the tail
    (9000, 256, 256, 1, True, 1, False),
])
def test_linear_backward_with_batchnorm_backward_folded_in(E, M, N, K, relu, pro, acc, nxt):
    """esc_linear_bwd_both_bn == esc_bn_bwd_apply -> esc_linear_bwd_both (run_graphcount.py:65-73,78-87,183-186 backward):
    the BatchNorm backward is applied to the dY operand as the GEMM stages it; with `next` the dX tiles leave the column
    sums of the next BatchNorm backward.  Checked against the unfused C-ABI sequence and an fp64 autograd reference."""
    import ctypes
    nv = E._native
    dev = torch.device("cuda:0")
    torch.manual_seed(M * 7 + N + K)
    xb = (torch.randn(M, N) * 1.5 + 0.3).to(dev)                 # what the BatchNorm normalised
    gamma, beta = (torch.rand(N) + 0.5).to(dev), (torch.randn(N) * 0.3).to(dev)
    dOut = torch.randn(M, N).to(dev)
    ldx = K + 8                                                  # a slice of a wider buffer, like the concat slices
    Xw = torch.randn(M, ldx).to(dev)
    X = Xw[:, :K]
    W = (torch.randn(N, K) / K ** 0.5).to(dev)
    isc, ish = ((torch.rand(K) + 0.5).to(dev), (torch.randn(K) * 0.2).to(dev)) if pro else (None, None)
    scratch = torch.empty(nv.lib().esc_bn_scratch(max(N, K)), device=dev)

    def stats(x, C, ga, be):       # the library's own statistics / forward coefficients (what the engine hands on)
        out = [torch.empty(C, device=dev) for _ in range(4)]
        nv.call("esc_bn_stats", nv.ptr(x), C, M, C, 1e-5, 0.1, nv.ptr(out[0]), nv.ptr(out[1]), None, None, nv.ptr(ga), nv.ptr(be),
                nv.ptr(out[2]), nv.ptr(out[3]), nv.ptr(scratch), nv.stream())
        return out
    mean, invstd, scale, shift = stats(xb, N, gamma, beta)
    coef, dg, db_bn = torch.empty(N, 2, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    nv.call("esc_bn_bwd_coef", nv.ptr(xb), N, None, 0, nv.ptr(dOut), N, M, N, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta),
            relu, nv.ptr(coef), nv.ptr(dg), nv.ptr(db_bn), nv.ptr(scratch), nv.stream())
    dx0 = torch.randn(M, K).to(dev) if acc else torch.zeros(M, K, device=dev)
    x2 = (torch.randn(M, K) * 0.8 - 0.2).to(dev)                 # input rows of the NEXT BatchNorm (over dX's K channels)
    g2, b2 = (torch.rand(K) + 0.5).to(dev), (torch.randn(K) * 0.3).to(dev)
    mean2, invstd2, scale2, shift2 = stats(x2, K, g2, b2)
    slab_n = int(nv.lib().esc_linear_bwd_weight_scratch(M, N, K))

    def unfused():
        dY = torch.empty(M, N, device=dev)
        nv.call("esc_bn_bwd_apply", nv.ptr(xb), N, None, 0, nv.ptr(dOut), N, M, N, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta),
                relu, nv.ptr(coef), nv.ptr(dY), N, nv.stream())
        dX, dW, db = dx0.clone(), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        slabs = torch.empty(slab_n, device=dev)
        nv.call("esc_linear_bwd_both", nv.ptr(dY), N, nv.ptr(X), ldx, nv.ptr(isc), nv.ptr(ish), nv.ptr(W), K, M, N, K, nv.ptr(dX), K, acc,
                nv.ptr(dW), K, nv.ptr(db), nv.ptr(slabs), nv.stream())
        return dX, dW, db, dY

    f = nv.BnBwdFused()
    f.x, f.ld_x, f.mean, f.invstd, f.scale, f.shift, f.coef, f.relu = xb.data_ptr(), N, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), coef.data_ptr(), relu
    f.beta = beta.data_ptr()                                     # read when relu == 2: the ELU derivative's centred pre-activation
    nx = None
    if nxt:
        rows = int(nv.lib().esc_linear_bwd_bn_block_rows(M, N, K))
        slots = -(-M // rows)
        partial = torch.full((slots, K, 2), float("nan"), device=dev)
        nx = nv.BnBwdNext()
        nx.partial, nx.x, nx.ld_x, nx.mean, nx.invstd, nx.scale, nx.shift, nx.relu = partial.data_ptr(), x2.data_ptr(), K, mean2.data_ptr(), invstd2.data_ptr(), scale2.data_ptr(), shift2.data_ptr(), (relu or 1)
        nx.beta = b2.data_ptr()
    slabs = torch.empty(slab_n, device=dev)
    dX, dW, db = dx0.clone(), torch.full((N, K), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)
    assert nv.lib().esc_linear_bwd_both_bn_ok(nv.ptr(dOut), N, ctypes.byref(f), nv.ptr(X), ldx, nv.ptr(W), K, M, N, K, nv.ptr(dX), K, nv.ptr(slabs),
                                              ctypes.byref(nx) if nx is not None else None) == 1
    nv.call("esc_linear_bwd_both_bn", nv.ptr(dOut), N, ctypes.byref(f), nv.ptr(X), ldx, nv.ptr(isc), nv.ptr(ish), nv.ptr(W), K, M, N, K,
            nv.ptr(dX), K, acc, nv.ptr(dW), K, nv.ptr(db), nv.ptr(slabs), None, ctypes.byref(nx) if nx is not None else None, nv.stream())
    uX, uW, ub, dY = unfused()
    scale_of = lambda t: max(1.0, float(t.abs().max()))
    for a, b, name in ((dX, uX, "dX"), (dW, uW, "dW")):
        assert float((a - b).abs().max()) <= 2e-5 * scale_of(b), (name, float((a - b).abs().max()), scale_of(b))
    # the bias gradient of a Linear in front of a BatchNorm is zero up to rounding (column sums of a BatchNorm backward)
    assert float((db - ub).abs().max()) <= 1e-3 and float(db.abs().max()) <= 1e-2 * scale_of(dY) * M ** 0.5
    # fp64 reference of the whole chain
    xb64, ga64, be64 = xb.double().cpu().requires_grad_(True), gamma.double().cpu().requires_grad_(True), beta.double().cpu().requires_grad_(True)
    X64 = X.double().cpu()
    Xa = (torch.relu(X64 * isc.double().cpu() + ish.double().cpu()) if pro else X64).requires_grad_(True)
    W64 = W.double().cpu().requires_grad_(True)
    # (Linear in front of the BatchNorm is irrelevant here: treat the BatchNorm input as a leaf and chain by hand)
    y = torch.nn.functional.batch_norm(xb64, None, None, ga64, be64, True, 0.1, 1e-5)
    y = y.relu() if relu == 1 else (torch.nn.functional.elu(y) if relu == 2 else y)
    y.backward(dOut.double().cpu())
    dY64 = xb64.grad
    _chk(dY, dY64, "unfused dY")
    _chk(dg, ga64.grad, "dgamma")
    _chk(db_bn, be64.grad, "dbeta")
    want_dX = dY64 @ W64.detach() + (dx0.double().cpu() if acc else 0)
    want_dW = dY64.t() @ Xa.detach()
    _chk(dX, want_dX, "fused dX vs fp64")
    _chk(dW, want_dW, "fused dW vs fp64", tol=2e-5)
    if nxt:
        c2, dg2, db2 = torch.empty(K, 2, device=dev), torch.empty(K, device=dev), torch.empty(K, device=dev)
        nv.call("esc_bn_bwd_coef_from_partials", nv.ptr(partial), slots, M, K, nv.ptr(c2), nv.ptr(dg2), nv.ptr(db2), nv.stream())
        r2, rg2, rb2 = torch.empty(K, 2, device=dev), torch.empty(K, device=dev), torch.empty(K, device=dev)
        nv.call("esc_bn_bwd_coef", nv.ptr(x2), K, None, 0, nv.ptr(dX), K, M, K, nv.ptr(mean2), nv.ptr(invstd2), nv.ptr(g2), nv.ptr(b2),
                (relu or 1), nv.ptr(r2), nv.ptr(rg2), nv.ptr(rb2), nv.ptr(scratch), nv.stream())
        assert not bool(torch.isnan(partial).any())
        for a, b, name in ((c2, r2, "coef"), (dg2, rg2, "dgamma"), (db2, rb2, "dbeta")):
            assert float((a - b).abs().max()) <= 1e-5 * scale_of(b) * max(1.0, M ** 0.5 / 10), (name, float((a - b).abs().max()))


def test_linear_backward_leaves_the_next_batchnorm_sums_without_a_fused_apply(E):
    """esc_linear_bwd_both_bn(bn=NULL, next): a plain dY, only the column sums of the NEXT BatchNorm backward ride in the dX
    epilogue — dX / dW bit-identical to esc_linear_bwd_both, the sums equal to esc_bn_bwd_coef's"""
    import ctypes
    nv = E._native
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    M, N, K = 2400, 256, 256
    dY, X, W = torch.randn(M, N).to(dev), torch.randn(M, K).to(dev), (torch.randn(N, K) / 16).to(dev)
    x2 = (torch.randn(M, K) * 0.8 - 0.2).to(dev)
    g2, b2 = (torch.rand(K) + 0.5).to(dev), (torch.randn(K) * 0.3).to(dev)
    scratch = torch.empty(nv.lib().esc_bn_scratch(K), device=dev)
    st = [torch.empty(K, device=dev) for _ in range(4)]
    nv.call("esc_bn_stats", nv.ptr(x2), K, M, K, 1e-5, 0.1, nv.ptr(st[0]), nv.ptr(st[1]), None, None, nv.ptr(g2), nv.ptr(b2), nv.ptr(st[2]), nv.ptr(st[3]),
            nv.ptr(scratch), nv.stream())
    slab_n = int(nv.lib().esc_linear_bwd_weight_scratch(M, N, K))
    out = []
    for fused in (False, True):
        dX, dW, db = torch.empty(M, K, device=dev), torch.empty(N, K, device=dev), torch.empty(N, device=dev)
        slabs = torch.empty(slab_n, device=dev)
        if fused:
            slots = -(-M // int(nv.lib().esc_linear_bwd_bn_block_rows(M, N, K)))
            partial = torch.full((slots, K, 2), float("nan"), device=dev)
            nx = nv.BnBwdNext()
            nx.partial, nx.x, nx.ld_x, nx.mean, nx.invstd, nx.scale, nx.shift, nx.relu = partial.data_ptr(), x2.data_ptr(), K, st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(), st[3].data_ptr(), 1
            nv.call("esc_linear_bwd_both_bn", nv.ptr(dY), N, None, nv.ptr(X), K, None, None, nv.ptr(W), K, M, N, K, nv.ptr(dX), K, 0, nv.ptr(dW), K,
                    nv.ptr(db), nv.ptr(slabs), None, ctypes.byref(nx), nv.stream())
        else:
            nv.call("esc_linear_bwd_both", nv.ptr(dY), N, nv.ptr(X), K, None, None, nv.ptr(W), K, M, N, K, nv.ptr(dX), K, 0, nv.ptr(dW), K, nv.ptr(db),
                    nv.ptr(slabs), nv.stream())
        out.append((dX, dW, db))
    for a, b, name in zip(out[0], out[1], ("dX", "dW", "db")):
        assert torch.equal(a, b), name
    c2, dg2, db2 = torch.empty(K, 2, device=dev), torch.empty(K, device=dev), torch.empty(K, device=dev)
    nv.call("esc_bn_bwd_coef_from_partials", nv.ptr(partial), slots, M, K, nv.ptr(c2), nv.ptr(dg2), nv.ptr(db2), nv.stream())
    r2, rg2, rb2 = torch.empty(K, 2, device=dev), torch.empty(K, device=dev), torch.empty(K, device=dev)
    nv.call("esc_bn_bwd_coef", nv.ptr(x2), K, None, 0, nv.ptr(out[1][0]), K, M, K, nv.ptr(st[0]), nv.ptr(st[1]), nv.ptr(g2), nv.ptr(b2), 1, nv.ptr(r2),
            nv.ptr(rg2), nv.ptr(rb2), nv.ptr(scratch), nv.stream())
    for a, b, name in ((c2, r2, "coef"), (dg2, rg2, "dgamma"), (db2, rb2, "dbeta")):
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), name


@pytest.mark.parametrize("H,spread", [(256, False), (300, False), (64, False), (256, True)])
def test_bag_forward_with_lds_staged_table_slices(E, H, spread):
    """esc_bag_fwd_rows (r03: a workgroup stages the table rows its 128 edges use in LDS) against the wave-per-row kernel and the
    sequential CPU scatter — bit for bit, plain and accumulating; `spread` draws the bins uniformly over all 1800 rows so that
    a workgroup needs more rows than it can stage and takes the global-memory branch; the statistics epilogue against
    esc_bn_stats (run_graphcount.py:155-156: bag -> BatchNorm)."""
    nv = E._native
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(H + int(spread))
    Ee, rows = 3000, 1800
    cnt = torch.randint(20, 60, (Ee,), generator=g)
    cnt[7] = 0                                                     # an edge without entries
    row_ptr = torch.zeros(Ee + 1, dtype=torch.int64); row_ptr[1:] = torch.cumsum(cnt, 0)
    Z = int(row_ptr[-1])
    seg = torch.repeat_interleave(torch.arange(Ee), cnt)
    if spread:
        idx = torch.randint(0, rows, (Z,), generator=g)
    else:                                                          # like real batches: the edges of a graph share ~100 bins
        base = (seg // 120) * 37 % 1500
        idx = base + torch.randint(0, 100, (Z,), generator=g)
    val = torch.randint(1, 9, (Z,), generator=g)
    W = torch.randn(rows, H, generator=g)
    torch.set_num_threads(1)
    ref = torch.zeros(Ee, H).index_add_(0, seg, W[idx] * val.view(-1, 1).float())
    rp, ix, vl, Wd = row_ptr.to(torch.int32).to(dev), idx.to(torch.int32).to(dev), val.to(torch.int32).to(dev), W.to(dev)
    old, new = torch.empty(Ee, H, device=dev), torch.empty(Ee, H, device=dev)
    nv.call("esc_bag_fwd", nv.ptr(Wd), H, nv.ptr(rp), nv.ptr(ix), nv.ptr(vl), Ee, nv.ptr(old), H, nv.stream())
    block = int(nv.lib().esc_bag_fwd_stats_block_rows(nv.ptr(Wd), rows, H, nv.ptr(new), H, Ee))
    if block == 0:                                                 # the tiled kernel is off by default (ESC_BAG_TILED=1 enables it):
        nv.call("esc_bag_fwd_rows", nv.ptr(Wd), rows, H, nv.ptr(rp), nv.ptr(ix), nv.ptr(vl), Ee, nv.ptr(new), H, 0, None, nv.stream())
        assert torch.equal(old.cpu(), ref) and torch.equal(new, old)     # the entry point then runs the wave-per-row kernel
        with pytest.raises(RuntimeError):
            nv.call("esc_bag_fwd_rows", nv.ptr(Wd), rows, H, nv.ptr(rp), nv.ptr(ix), nv.ptr(vl), Ee, nv.ptr(new), H, 0, nv.ptr(old), nv.stream())
        return
    assert block == 128
    stats = torch.full((-(-Ee // block), H, 2), float("nan"), device=dev)
    nv.call("esc_bag_fwd_rows", nv.ptr(Wd), rows, H, nv.ptr(rp), nv.ptr(ix), nv.ptr(vl), Ee, nv.ptr(new), H, 0, nv.ptr(stats), nv.stream())
    assert torch.equal(old.cpu(), ref) and torch.equal(new, old)
    acc0 = torch.randn(Ee, H, generator=g)
    a1, a2 = acc0.to(dev), acc0.to(dev)
    nv.call("esc_bag_fwd_acc", nv.ptr(Wd), H, nv.ptr(rp), nv.ptr(ix), nv.ptr(vl), Ee, nv.ptr(a1), H, nv.stream())
    nv.call("esc_bag_fwd_rows", nv.ptr(Wd), rows, H, nv.ptr(rp), nv.ptr(ix), nv.ptr(vl), Ee, nv.ptr(a2), H, 1, None, nv.stream())
    assert torch.equal(a1, a2)
    # the epilogue's partials -> the same statistics as a pass over the output
    mean, invstd, sc, sh = (torch.empty(H, device=dev) for _ in range(4))
    nv.call("esc_bn_stats_from_partials_rows", nv.ptr(stats), Ee, H, block, 1e-5, 0.1, nv.ptr(mean), nv.ptr(invstd), None, None, None, None,
            nv.ptr(sc), nv.ptr(sh), nv.stream())
    assert not bool(torch.isnan(stats).any())
    _chk(mean, ref.double().mean(0), "mean from the bag epilogue")
    _chk(invstd, 1.0 / torch.sqrt(ref.double().var(0, unbiased=False) + 1e-5), "invstd from the bag epilogue")
    with pytest.raises(RuntimeError):                              # fewer edges than the tiled kernel serves: no statistics
        nv.call("esc_bag_fwd_rows", nv.ptr(Wd), rows, H, nv.ptr(rp), nv.ptr(ix), nv.ptr(vl), 100, nv.ptr(new), H, 0, nv.ptr(stats), nv.stream())


def _one_row(v, dev):
    """(leaf [C, 1], its transpose): ONE row of C columns whose stride(0) is 1, below its width - what PyTorch hands on for a
    transposed column.  The backward of an op must read it with the leading dimension its forward used (ops._rows)."""
    leaf = v.reshape(-1, 1).to(dev).requires_grad_(True)
    row = leaf.t()
    assert tuple(row.shape) == (1, v.numel()) and row.stride(0) == 1
    return leaf, row


@pytest.mark.parametrize("K,N", [(4, 3), (256, 256)])          # 256 x 256: the matrix-core branch
def test_one_row_operand_linear(E, K, N):
    torch.manual_seed(K)
    dev = torch.device("cuda:0")
    x, w, bias = torch.randn(1, K), torch.randn(N, K) / K ** 0.5, torch.randn(N)
    leaf, row = _one_row(x, dev)
    wd, bd = (t.to(dev).requires_grad_(True) for t in (w, bias))
    y = E.ops.linear(row, wd, bd)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, bias))
    r = x64 @ w64.t() + b64
    assert torch.allclose(y.cpu().double(), r, **TOL)
    g = torch.randn(1, N)
    y.backward(g.to(dev))
    r.backward(g.double())
    assert torch.allclose(leaf.grad.t().cpu().double(), x64.grad, **TOL)
    scale = max(1.0, float(w64.grad.abs().max()))
    assert torch.allclose(wd.grad.cpu().double() / scale, w64.grad / scale, **TOL)
    assert torch.allclose(bd.grad.cpu().double() / scale, b64.grad / scale, **TOL)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C", [10, 256])
def test_one_row_operand_bn_eval_act(E, C, act):
    torch.manual_seed(C + act)
    dev = torch.device("cuda:0")
    x = torch.randn(1, C) * 3 + 5
    gamma, beta, rm0, rv0 = torch.rand(C) + 0.5, torch.randn(C), torch.randn(C) + 5, torch.rand(C) * 9 + 0.5
    leaf, row = _one_row(x, dev)
    gd, bd = (t.to(dev).requires_grad_(True) for t in (gamma, beta))
    y = E.ops.bn_eval_act(row, gd, bd, rm0.to(dev), rv0.to(dev), 1e-5, act)
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    r = (x64 - rm0.double()) / torch.sqrt(rv0.double() + 1e-5) * g64 + b64
    r = r.relu() if act else r
    assert torch.allclose(y.cpu().double(), r, **TOL)
    g = torch.randn(1, C)
    y.backward(g.to(dev))
    r.backward(g.double())
    _chk(leaf.grad.t(), x64.grad, "dx")
    _chk(gd.grad, g64.grad, "dgamma")
    _chk(bd.grad, b64.grad, "dbeta")


@pytest.mark.parametrize("C", [10, 64])
def test_one_row_operand_gine_aggregate(E, C):
    """one node with one self-loop: out = relu(x + e) + (1 + eps) x"""
    torch.manual_seed(C)
    dev = torch.device("cuda:0")
    plan = E.BatchPlan.from_tensors(torch.zeros(2, 1, dtype=torch.long, device=dev), 1)
    x, e, eps = torch.randn(1, C), torch.randn(1, C), torch.tensor([0.3])
    xl, xrow = _one_row(x, dev)
    el, erow = _one_row(e, dev)
    epsd = eps.to(dev).requires_grad_(True)
    out = E.ops.gine_aggregate(xrow, erow, epsd, plan)
    x64, e64, eps64 = (t.double().requires_grad_(True) for t in (x, e, eps))
    r = (x64 + e64).relu() + (1 + eps64) * x64
    assert torch.allclose(out.cpu().double(), r, **TOL)
    g = torch.randn(1, C)
    out.backward(g.to(dev))
    r.backward(g.double())
    assert torch.allclose(xl.grad.t().cpu().double(), x64.grad, **TOL)
    assert torch.allclose(el.grad.t().cpu().double(), e64.grad, **TOL)
    assert torch.allclose(epsd.grad.cpu().double(), eps64.grad, rtol=1e-5, atol=1e-4)
