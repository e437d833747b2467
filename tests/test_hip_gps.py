"""The graph transformer on the GPU: the ragged multi-head attention kernels (csrc/attention.hip) against the fp64 oracle of
tests/gps_oracle.py through the op and through the C ABI, dropout with the kernel's own mask fed to the oracle, bit stability,
a saturated softmax, the limits, GraphMultiheadAttention / GPSModel against the oracle model, AdamW + gradient clipping through
FlatAdam, and the driver.

Error measure: max |got - want| over the largest |want| of the tensor, bound 1e-5 (the README's bound on predictions).  torch's
own fp32 evaluation of the same expression on the CPU is printed next to every figure: on unit-variance inputs it is about 3e-7
from fp64, so the bound leaves about 40x over what fp32 arithmetic alone costs."""
import math
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import gps_oracle as go
import loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-5
BASE = [1, 2, 37, 64, 65, 130, 3]
BATCHES = {"base": BASE, "empty-middle": [1, 2, 37, 0, 64, 65, 130, 3], "empty-end": BASE + [0], "one-node": [1], "256-nodes": [256]}
HEADS = [(1, 4), (4, 16), (8, 8), (2, 64)]


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()) / float(want.abs().max()) if want.numel() else 0.0


def graph_ptr(sizes):
    return torch.tensor(go.graph_ptr_of(sizes), dtype=torch.int32, device=DEV)


_REFS = {}


def reference(tag, sizes, heads, d, keep=None, p=0.0, scale=1.0):
    """inputs (fp32, unit variance times `scale`), upstream gradient cos(arange), and the oracle's out / lse / d_qkv in fp64 and in
    fp32 on the CPU: computed once per case, shared, never modified"""
    key = (tag, heads, d, p, scale)
    if key not in _REFS:
        N, H = sum(sizes), heads * d
        gen = torch.Generator().manual_seed(lc.seed_of("gps-%s-%d-%d" % (tag.split("/")[0], heads, d)))
        qkv = torch.randn((N, 3 * H), generator=gen) * scale
        gy = torch.cos(torch.arange(N * H, dtype=torch.float64)).reshape(N, H).float()
        res = []
        for dtype in (torch.float64, torch.float32):
            x = qkv.clone().to(dtype).requires_grad_(True)             # (a copy: .to(float32) alone would hand qkv itself back)
            out, lse = go.ragged_attention(x, sizes, heads, keep, p)
            out.backward(gy.to(dtype))
            res.append((out.detach(), lse.detach(), x.grad))
        _REFS[key] = (qkv, gy) + tuple(res)
    return _REFS[key]


def check(what, got, want64, want32):
    e, e32 = rel(got, want64), rel(want32, want64)
    print("%-40s kernel %.3g   torch fp32 on the CPU %.3g" % (what, e, e32))
    assert e <= BOUND, "%s: %.3g of the largest value, bound %g (torch fp32: %.3g)" % (what, e, BOUND, e32)


def run_op(E, qkv_dev, sizes, heads, **kw):
    x = qkv_dev.detach().requires_grad_(True)
    res = E.ops.graph_attention(x, graph_ptr(sizes), heads, max_nodes=max(sizes), return_aux=True, **kw)
    return x, res


# ---- 1. forward and backward against the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,d", HEADS)
@pytest.mark.parametrize("tag", list(BATCHES))
def test_forward_and_backward_against_the_oracle(E, tag, heads, d):
    sizes = BATCHES[tag]
    qkv, gy, (o64, l64, g64), (o32, l32, g32) = reference(tag, sizes, heads, d)
    x, (out, lse, mask) = run_op(E, qkv.to(DEV), sizes, heads)
    assert mask is None
    out.backward(gy.to(DEV))
    name = "%s %dx%d " % (tag, heads, d)
    check(name + "out", out, o64, o32)
    check(name + "lse", lse, l64, l32)
    check(name + "d_qkv", x.grad, g64, g32)
    assert bool(torch.isfinite(x.grad).all())


def test_column_slices_of_wider_buffers(E):
    """qkv a column slice of wider rows (leading dimension != 3H), the upstream gradient likewise; and `out` written into a
    slice of a wider buffer through the C ABI"""
    heads, d, sizes = 4, 16, BASE
    H, N = heads * d, sum(BASE)
    qkv, gy, (o64, l64, g64), (o32, l32, g32) = reference("base", sizes, heads, d)
    wide = torch.full((N, 3 * H + 12), float("nan"), device=DEV)
    wide[:, 4:4 + 3 * H] = qkv.to(DEV)
    x = wide.requires_grad_(True)
    out = E.ops.graph_attention(x[:, 4:4 + 3 * H], graph_ptr(sizes), heads, max_nodes=max(sizes))
    gwide = torch.full((N, H + 8), float("nan"), device=DEV)
    gwide[:, 8:] = gy.to(DEV)
    out.backward(gwide[:, 8:])
    check("slice out", out, o64, o32)
    check("slice d_qkv", x.grad[:, 4:4 + 3 * H], g64, g32)
    assert not bool(x.grad[:, :4].any()) and not bool(x.grad[:, 4 + 3 * H:].any())
    nv, gp = E._native, graph_ptr(sizes)
    pp = E.ops._pair_ptr(gp)
    owide = torch.full((N, H + 20), -7.0, device=DEV)
    lse = torch.empty((heads, N), device=DEV)
    o = owide[:, 16:16 + H]
    nv.call("esc_graph_attention_fwd", wide[:, 4:].data_ptr(), wide.stride(0), nv.ptr(gp), nv.ptr(pp), len(sizes), N, 0, max(sizes),
            heads, d, 0.0, 0, o.data_ptr(), owide.stride(0), nv.ptr(lse), None, nv.stream())
    assert torch.equal(o, out.detach()) and torch.equal(lse, E.ops.graph_attention(x[:, 4:4 + 3 * H], gp, heads, max_nodes=max(sizes), return_aux=True)[1])
    assert bool((owide[:, :16] == -7.0).all()) and bool((owide[:, 16 + H:] == -7.0).all())


def test_nothing_to_do_is_legal(E):
    """G == 0, N == 0 and a batch of empty graphs only write nothing and return empty results"""
    for sizes in ([], [0], [0, 0, 0]):
        x = torch.zeros((0, 3 * 64), device=DEV, requires_grad=True)
        out = E.ops.graph_attention(x, graph_ptr(sizes), 4, max_nodes=0)
        out.sum().backward()
        assert out.shape == (0, 64) and x.grad.shape == (0, 192)


# ---- 2. dropout ------------------------------------------------------------------------------------------------------------------
DROP_SIZES, DROP_P = [37, 64, 65], 0.5


def test_dropout_with_the_kernels_own_mask(E):
    heads, d = 4, 16
    total = sum(n * n for n in DROP_SIZES)
    qkv = reference("drop", DROP_SIZES, heads, d)[0]
    x, (out, lse, mask) = run_op(E, qkv.to(DEV), DROP_SIZES, heads, p=DROP_P, training=True, seed=1234)
    keep = go.unpack_mask(mask.cpu(), DROP_SIZES, heads)
    qkv, gy, (o64, l64, g64), (o32, l32, g32) = reference("drop/1234", DROP_SIZES, heads, d, keep=keep, p=DROP_P)
    out.backward(gy.to(DEV))
    check("dropout out", out, o64, o32)
    check("dropout lse", lse, l64, l32)
    check("dropout d_qkv", x.grad, g64, g32)
    live = mask[:heads * total]
    assert bool((live <= 1).all())
    kept, n = int(live.sum()), heads * total
    sd = math.sqrt(n * DROP_P * (1 - DROP_P))
    print("kept %d of %d: %.2f standard deviations from %g" % (kept, n, (kept - n * (1 - DROP_P)) / sd, 1 - DROP_P))
    assert abs(kept - n * (1 - DROP_P)) <= 5 * sd
    again = run_op(E, qkv.to(DEV), DROP_SIZES, heads, p=DROP_P, training=True, seed=1234)[1]
    assert torch.equal(again[2][:n], live) and torch.equal(again[0], out)
    other = run_op(E, qkv.to(DEV), DROP_SIZES, heads, p=DROP_P, training=True, seed=1235)[1]
    assert not torch.equal(other[2][:n], live)
    plain = run_op(E, qkv.to(DEV), DROP_SIZES, heads, p=DROP_P, training=False)[1]     # eval mode: no dropout, no mask
    assert plain[2] is None


def test_backward_reads_the_mask_it_is_given(E):
    """the mask entries of one query row zeroed by hand between forward and backward: that row's d_q is exactly 0 in every
    column of that head (and only there); p = 0 with a NULL mask equals the op's result"""
    heads, d, sizes = 4, 16, DROP_SIZES
    H, N, G = heads * d, sum(sizes), len(sizes)
    total = sum(n * n for n in sizes)
    nv, gp = E._native, graph_ptr(sizes)
    pp = E.ops._pair_ptr(gp)
    qkv, gy = (t.to(DEV) for t in reference("drop", sizes, heads, d)[:2])
    room = N * max(sizes)

    def fwd(p, mask):
        out, lse = torch.empty((N, H), device=DEV), torch.empty((heads, N), device=DEV)
        nv.call("esc_graph_attention_fwd", nv.ptr(qkv), 3 * H, nv.ptr(gp), nv.ptr(pp), G, N, room, max(sizes), heads, d, p, 99,
                nv.ptr(out), H, nv.ptr(lse), nv.ptr(mask), nv.stream())
        return out, lse

    def bwd(p, lse, mask):
        dq = torch.full((N, 3 * H), float("nan"), device=DEV)
        nv.call("esc_graph_attention_bwd", nv.ptr(qkv), 3 * H, nv.ptr(gy), H, nv.ptr(lse), nv.ptr(mask), nv.ptr(gp), nv.ptr(pp), G, N,
                room, max(sizes), heads, d, p, nv.ptr(dq), nv.stream())
        return dq

    mask = torch.full((heads * room,), 7, dtype=torch.uint8, device=DEV)
    out, lse = fwd(DROP_P, mask)
    assert bool((mask[heads * total:] == 7).all()), "bytes behind heads * pair_ptr[G] were written"
    before = bwd(DROP_P, lse, mask)
    g, a, i = 1, 2, 5                                       # graph 1 (64 nodes, rows 37..100), head 2, its query row 5
    n, row = sizes[g], sizes[0] + i
    at = a * total + sizes[0] ** 2 + i * n
    mask[at:at + n] = 0
    after = bwd(DROP_P, lse, mask)
    cols = slice(a * d, (a + 1) * d)
    assert bool(before[row, cols].any()) and not bool(after[row, cols].any()), "d_q of a fully dropped row must be exactly 0"
    same = torch.ones((N, 3 * H), dtype=torch.bool)
    same[row, cols] = False
    same[sizes[0]:sizes[0] + n, H + a * d:H + (a + 1) * d] = False          # d_k and d_v of that graph and head see the row go
    same[sizes[0]:sizes[0] + n, 2 * H + a * d:2 * H + (a + 1) * d] = False
    assert torch.equal(before.cpu()[same], after.cpu()[same]) and bool(torch.isfinite(after).all())
    out0, lse0 = fwd(0.0, None)                             # p == 0: NULL mask, nothing read or written
    x, (out_op, lse_op, _) = run_op(E, qkv, sizes, heads)
    out_op.backward(gy)
    assert torch.equal(out0, out_op) and torch.equal(lse0, lse_op) and torch.equal(bwd(0.0, lse0, None), x.grad)


# ---- 3. bit stability ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_results_are_bit_identical_run_to_run(E, p):
    heads, d = 4, 16
    qkv, gy = (t.to(DEV) for t in reference("base", BASE, heads, d)[:2])
    runs = []
    for _ in range(2):
        x, (out, lse, mask) = run_op(E, qkv, BASE, heads, p=p, training=True, seed=5)
        out.backward(gy)
        runs.append((out.detach(), lse, x.grad))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- 4. a saturated softmax ------------------------------------------------------------------------------------------------------
def test_sharp_softmax_stays_finite_and_convex(E):
    """inputs scaled by 1e3: the logits reach 1e7 and the softmax is one-hot up to ties; outputs and gradients are finite and
    every output row is a convex combination of its graph's V rows (no fp64 comparison: the logits themselves carry about 0.06
    of fp32 rounding)"""
    heads, d = 4, 16
    H = heads * d
    qkv = reference("base", BASE, heads, d)[0] * 1e3
    x, (out, lse, _) = run_op(E, qkv.to(DEV), BASE, heads)
    out.backward(reference("base", BASE, heads, d)[1].to(DEV))
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(x.grad).all())
    o, v, at = out.detach().cpu(), qkv[:, 2 * H:], 0
    for n in BASE:
        lo, hi = v[at:at + n].min(0).values, v[at:at + n].max(0).values
        slack = 4e-7 * torch.maximum(lo.abs(), hi.abs())          # the weights sum to 1 within a few roundings
        assert bool((o[at:at + n] >= lo - slack).all()) and bool((o[at:at + n] <= hi + slack).all())
        at += n


# ---- 5. limits -------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host(E):
    limit = E.ops.attention_max_nodes(16)
    assert limit >= 256 and E.ops.attention_max_nodes(32) >= 256 and E.ops.attention_max_nodes(64) >= 256
    assert E.ops.attention_max_nodes(6) == 0 and E.ops.attention_max_nodes(68) == 0
    n = limit + 1
    with pytest.raises(RuntimeError, match=r"exceeds the limit of %d nodes" % limit):
        E.ops.graph_attention(torch.zeros((n, 3 * 64), device=DEV), graph_ptr([n]), 4, max_nodes=n)
    with pytest.raises(RuntimeError, match=r"exceeds the limit of %d nodes" % limit):           # ... also when the op has to look itself
        E.ops.graph_attention(torch.zeros((n, 3 * 64), device=DEV), graph_ptr([n]), 4)
    with pytest.raises(RuntimeError, match="multiple of 4 and at most 64"):
        E.ops.graph_attention(torch.zeros((5, 3 * 12), device=DEV), graph_ptr([5]), 2)           # head_dim 6
    with pytest.raises(RuntimeError, match=r"heads \* head_dim == H"):
        E.ops.graph_attention(torch.zeros((5, 3 * 64 + 3), device=DEV), graph_ptr([5]), 4)
    nv, gp = E._native, graph_ptr([n])
    buf = torch.zeros((n, 3 * 64), device=DEV)
    with pytest.raises(RuntimeError, match=r"limit of %d nodes" % limit):                        # the C entry points check for themselves
        nv.call("esc_graph_attention_fwd", nv.ptr(buf), 192, nv.ptr(gp), nv.ptr(E.ops._pair_ptr(gp)), 1, n, 0, n, 4, 16, 0.0, 0,
                nv.ptr(buf), 64, nv.ptr(buf), None, nv.stream())
    with pytest.raises(RuntimeError, match="multiple of 4 and at most 64"):
        nv.call("esc_graph_attention_bwd", nv.ptr(buf), 192, nv.ptr(buf), 64, nv.ptr(buf), None, nv.ptr(gp), nv.ptr(E.ops._pair_ptr(gp)), 1,
                n, 0, 8, 4, 6, 0.0, nv.ptr(buf), nv.stream())
    heads, d = 4, 16                                         # a valid call after the refusals is correct
    qkv, gy, (o64, l64, g64), (o32, l32, g32) = reference("base", BASE, heads, d)
    x, (out, lse, _) = run_op(E, qkv.to(DEV), BASE, heads)
    out.backward(gy.to(DEV))
    check("after the refusals out", out, o64, o32)
    check("after the refusals d_qkv", x.grad, g64, g32)


# ---- 6. layer and model ----------------------------------------------------------------------------------------------------------
def _close(a, b, what, tol):
    """the measure of test_hip_multihop's network test: max error over max(1, largest value)"""
    a, b = a.detach().cpu().double(), b.detach().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    print("%-48s max scaled error %.3g" % (what, err))
    assert a.shape == b.shape and err <= tol, "%s: max scaled error %.3g > %g" % (what, err, tol)


def test_attention_layer_against_torch_multihead_attention(E):
    """GraphMultiheadAttention loads a torch.nn.MultiheadAttention state_dict and computes what that layer computes on the padded
    batch (fp64, key_padding_mask)"""
    torch.manual_seed(11)
    ref = torch.nn.MultiheadAttention(64, 4, batch_first=True)
    torch.nn.init.normal_(ref.in_proj_bias)
    torch.nn.init.normal_(ref.out_proj.bias)
    mine = E.nn.GraphMultiheadAttention(64, 4)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(DEV)
    x = torch.randn(sum(BASE), 64)
    want = go.padded_attention(ref.double(), x.double(), BASE)
    got = mine(x.to(DEV), graph_ptr(BASE), max(BASE))
    e = rel(got, want)
    print("GraphMultiheadAttention vs padded MultiheadAttention: %.3g" % e)
    assert e <= BOUND


def test_model_against_the_oracle_model(E):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
    from esc_gnn_amd.gps_models import GPSModel
    graphs = build_feature_dataset(synthetic_zinc_graphs(0, 3), 3, use_rd=True, self_loop=True)
    torch.manual_seed(7)
    oracle = go.GPSModel(layers=2, dim_hidden=64, n_heads=4)
    for m in oracle.modules():                             # weights that make every term count: biases and BatchNorm affine off their defaults
        if isinstance(m, torch.nn.BatchNorm1d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, std=0.1)
        if isinstance(m, torch.nn.MultiheadAttention):
            torch.nn.init.normal_(m.in_proj_bias, std=0.1)
            torch.nn.init.normal_(m.out_proj.bias, std=0.1)
    mine = GPSModel(layers=2, dim_hidden=64, n_heads=4, dropout=0.0, attn_dropout=0.0)
    mine.load_state_dict(oracle.state_dict())
    mine = mine.to(DEV)
    oracle = oracle.double()
    batch = E.Batch.from_data_list([g for g in graphs])
    cpu = {k: batch[k].cpu() for k in ("x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
    y = torch.tensor([0.3, -1.1, 0.7], dtype=torch.float64).view(-1, 1)
    for mode in ("train", "eval"):
        getattr(oracle, mode)()
        getattr(mine, mode)()
        oracle.zero_grad()
        mine.zero_grad()
        want = oracle(cpu)
        (want - y).abs().mean().backward()
        got = mine(batch.to(DEV))
        E.ops.l1_loss(got, y.float().to(DEV)).backward()
        _close(got, want, mode + " prediction", 1e-5)
        ref_p, ref_b = dict(oracle.named_parameters()), dict(oracle.named_buffers())
        unused = 0
        for n, p in mine.named_parameters():
            if ref_p[n].grad is None:                      # edge_attn_emb / edge_attn_linear: in the state_dict, not in the forward
                assert "edge_attn" in n and p.grad is None, n
                unused += 1
                continue
            _close(p.grad, ref_p[n].grad, mode + " grad " + n, 1e-4)
        assert unused == 2 * 7
        for n, b in mine.named_buffers():
            _close(b, ref_b[n], mode + " buffer " + n, 1e-4)


# ---- 7. optimiser pieces ---------------------------------------------------------------------------------------------------------
WD, MAX_NORM = 1e-2, 1.0
ADAMW = lc.Adam("adamw-4099-s3-plain", 4099, 3, 0, (lc.LR,) * 3, lc.DEFAULT_BETAS, lc.DEFAULT_EPS, "plain", None, "one")


def adamw_ref64(case, data):
    """AdamW + clip_grad_norm_ in fp64 with the first-order error bounds of an fp32 evaluation, per element: the recursion of
    loss_cases.adam_ref64 (same statements, same charges, same doubling) with the two pieces this test adds written in -
    the gradient is divided by den = max((|g| + 1e-6) / max_norm, 1), whose fp32 value is charged 16 u (a tree sum of 4 099
    squares, the root, the sum, the quotient: 12 + 4 roundings) on top of the quotient's own u, and the parameter is scaled by
    1 - lr * wd first (the factor's cast and the product: 2 u |p|)."""
    b1, b2 = case.betas
    eps, u = case.eps, lc.U
    p, m, v = data.p0.astype(np.float64), data.m0.astype(np.float64), data.v0.astype(np.float64)
    Bp, Bm, Bv = np.zeros(case.n), np.zeros(case.n), np.zeros(case.n)
    for k in range(case.steps):
        t, lr = case.step0 + k + 1, case.lrs[k]
        g = data.grads[k].astype(np.float64)
        den = max((np.sqrt((g * g).sum()) + 1e-6) / MAX_NORM, 1.0)
        g = g / den
        p = p * (1 - lr * WD)
        Bp = Bp * (1 - lr * WD) + 2 * u * np.abs(p)
        m_prev, v_prev = m, v
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr * (m / (1 - b1 ** t)) / (np.sqrt(v / (1 - b2 ** t)) + eps)
        dg = 17 * u * np.abs(g)
        Bm = b1 * Bm + (1 - b1) * dg + 3 * u * (1 - b1) * np.abs(g - m_prev) + u * np.abs(m)
        Bv = b2 * Bv + u * (2 * b2 * v_prev + 3 * (1 - b2) * g * g + v) + 2 * (1 - b2) * np.abs(g) * dg
        bc2s, ns = np.sqrt(1 - b2 ** t), lr / (1 - b1 ** t)
        s = np.sqrt(v)
        q = s / bc2s
        dn = q + eps
        with np.errstate(divide="ignore", invalid="ignore"):
            Bs = np.where(v > 0, Bv / (2 * s), 0.0) + u * s
        Bden = Bs / bc2s + 2 * u * q + u * eps + u * dn
        r = np.abs(m) / dn
        Br = Bm / dn + r * Bden / dn + u * r
        Bp = Bp + ns * Br + 2 * u * ns * r + u * np.abs(p)
    return p, m, v, lc.SAFETY * Bp, lc.SAFETY * Bm, lc.SAFETY * Bv


def test_adamw_with_clipping_through_flat_adam(E):
    case, data = ADAMW, lc.AdamData(ADAMW)
    assert max(float(np.sqrt((g.astype(np.float64) ** 2).sum())) for g in data.grads) > MAX_NORM, "the case must clip"
    pt = torch.nn.Parameter(torch.from_numpy(data.p0.copy()).double())                     # the reference: torch's own classes in fp64
    ref = torch.optim.AdamW([pt], lr=lc.LR, betas=case.betas, eps=case.eps, weight_decay=WD)
    for k in range(case.steps):
        pt.grad = torch.from_numpy(data.grads[k].copy()).double()
        torch.nn.utils.clip_grad_norm_([pt], MAX_NORM)
        ref.step()
    p64, m64, v64, Bp, Bm, Bv = adamw_ref64(case, data)
    assert np.abs(p64 - pt.detach().numpy()).max() <= 1e-12 and np.abs(m64 - ref.state[pt]["exp_avg"].numpy()).max() <= 1e-12

    def run(**kw):
        p = torch.nn.Parameter(torch.from_numpy(data.p0.copy()).to(DEV))
        opt = E.optim.FlatAdam([p], lr=lc.LR, betas=case.betas, eps=case.eps, **kw)
        for k in range(case.steps):
            opt.zero_grad()
            p.grad.copy_(torch.from_numpy(data.grads[k]).to(DEV))
            scale = opt.clip_scale(MAX_NORM)
            assert scale.is_cuda and scale.shape == (1,) and scale.dtype == torch.float32
            opt.step(grad_denom=scale)
        return tuple(b[:case.n].cpu().numpy() for b in (opt.flat_param, opt.exp_avg, opt.exp_avg_sq))

    got = run(weight_decay=WD)
    for mine, want, bound, what in zip(got, (pt.detach().numpy(), m64, v64), (Bp, Bm, Bv), ("flat_param", "exp_avg", "exp_avg_sq")):
        ratio, err = lc.worst_ratio(mine, want, bound)
        print("%-24s %-10s %.3f of its bound (%.3g)" % (case.name, what, ratio, err))
        assert ratio <= 1.0, "%s: %s is %.3g from fp64, %.3f of its bound" % (case.name, what, err, ratio)
    plain, zero = run(), run(weight_decay=0.0)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(plain, zero)), "weight_decay=0 must change no bit"
    assert not np.array_equal(plain[0], got[0])


# ---- 8. driver -------------------------------------------------------------------------------------------------------------------
def test_driver_trains_checkpoints_and_evaluates(tmp_path, monkeypatch, capsys):
    require_gpu()
    import esc_gnn_amd.run_zinc_gps as rg
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rg.main("--synthetic_graphs 48 --epochs 2 --layers 2 --batch_size 16 --num_warmup_epochs 1 --save_appendix _t".split())
    out = capsys.readouterr().out
    lines = re.findall(r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)", out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    res = tmp_path / "results" / "zinc_GPS_t"
    assert (res / "log.txt").exists() and (res / "model_checkpoint2.pth").exists()
    rg.main(("--synthetic_graphs 48 --layers 2 --batch_size 16 --eval 1 --save_appendix _t --load_model %s" % (res / "model_checkpoint2.pth")).split())
    m = re.search(r"Test MAE: (\S+)", capsys.readouterr().out)
    assert m and math.isfinite(float(m.group(1)))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="data parallelism is out of scope"):
        rg.main("--synthetic_graphs 48 --epochs 1".split())
