"""The GatedGCN gate kernels (csrc/gatedgcn.hip), ops.gated_gcn_aggregate, nn.GatedGCNLayer, the CustomGatedGCN variants of
GPSLayer / GPSModel and the driver's --gt_layer_type on the GPU, against tests/gatedgcn_oracle.py evaluated in fp64 on the CPU.
Error measure, bound 1e-5 and the oracle's fp32 figure printed beside every kernel figure: tests/gps_cases.py.  Two tensors
are measured over the scale of the terms that cancel in them instead of their own largest value, each derived where it stands:
the edge gradients of the four cases where they are a pure cancellation residue (the oracle's CANCELLING, held to the same cap
by tests/test_gatedgcn_cpu.py) and the bias gradients of the layer and model tests (_compare_models).  References are computed
once per case and shared."""
import math
import re

import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import gatedgcn_oracle as gg
import gps_cases as gc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
OPERANDS = ("Ax", "Bx", "Dx", "Ex", "Ce")
SAT_SCALE = 12.0                          # unit-variance operands times 12: |e_ij| reaches 40 (the CPU test asserts it)


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


_PLANS = {}


def plan_of(E, name):
    """the plan of a case from a stable argsort on the CPU: the two views exactly as the header describes them"""
    if name not in _PLANS:
        n, src, dst = gg.edges_of(name)
        kw = dict(num_nodes=n, num_edges=src.numel(), nnz=0)
        for view, key, other in (("in", dst, src), ("out", src, dst)):
            perm = torch.sort(key, stable=True).indices
            ptr = torch.zeros(n + 1, dtype=torch.int64)
            ptr[1:] = torch.cumsum(torch.bincount(key, minlength=n), 0)[:n] if n else ptr[1:]
            kw[view + "_ptr"] = ptr.to(torch.int32).to(DEV)
            kw[view + "_edge"] = perm.to(torch.int32).to(DEV)
            kw[view + ("_src" if view == "in" else "_dst")] = other[perm].to(torch.int32).to(DEV)
        _PLANS[name] = E.BatchPlan(**kw)
    return _PLANS[name]


def check(what, got, want64, want32, floor=0.0):
    e, e32 = gg.rel(got, want64, floor), gg.rel(want32, want64, floor)
    print("%-44s kernel %.3g   torch fp32 on the CPU %.3g" % (what, e, e32))
    assert e <= gc.BOUND, "%s: %.3g of the largest value, bound %g (torch fp32: %.3g)" % (what, e, gc.BOUND, e32)


def run_op(E, name, C, with_ge, scale=1.0):
    ops, g_out, g_e = gg.inputs_of(name, C, scale)
    x = [t.to(DEV).requires_grad_(True) for t in ops]
    out, e_out = E.ops.gated_gcn_aggregate(*x, plan_of(E, name))
    loss = (out * g_out.to(DEV)).sum()
    if with_ge:
        loss = loss + (e_out * g_e.to(DEV)).sum()
    loss.backward()
    return out, e_out, x


# ---- 1. forward and backward against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ge", [True, False], ids=["g_e", "no-g_e"])
@pytest.mark.parametrize("C", gg.WIDTHS)
def test_op_against_the_oracle(E, C, with_ge):
    for name in gg.CASES:
        ref = gg.reference(name, C, with_ge)
        out, e_out, x = run_op(E, name, C, with_ge)
        got = dict(out=out, e_out=e_out)
        for k, t in zip(OPERANDS, x):
            assert t.grad is not None and t.grad.shape == t.shape, (name, k)
            got["d_" + k] = t.grad
        for k, v in got.items():
            check("%s C=%d %s" % (name, C, k), v, ref[F64][k], ref[F32][k], gg.scale_floor(name, C, with_ge, k))


def raw_call(E, name, C, ops, g_out, g_e, plan, ld_extra=0, sentinel=None):
    """esc_gated_gcn_fwd and _bwd through the C ABI; every operand and output a column slice of a buffer ld_extra wider"""
    nv = E._native
    n, m = plan.num_nodes, plan.num_edges

    def wide(t):
        buf = torch.full((t.size(0), C + ld_extra), float("nan") if sentinel is None else sentinel, device=DEV)
        buf[:, 4:4 + C] = t.to(DEV)
        return buf, buf[:, 4:4 + C]

    def blank(rows):
        buf = torch.full((rows, C + ld_extra), 0.0 if sentinel is None else sentinel, device=DEV)
        return buf, buf[:, (4 if ld_extra else 0):(4 if ld_extra else 0) + C]

    if not ld_extra:
        wide = lambda t: (t.to(DEV).contiguous(),) * 2          # noqa: E731
    ld = C + ld_extra
    (_, Ax), (_, Bx), (_, Dx), (_, Ex), (_, Ce) = (wide(t) for t in ops)
    (_, go_), (_, ge_) = wide(g_out), (wide(g_e) if g_e is not None else (None, None))
    bufs = {k: blank(n if k in ("out", "d_Dx", "d_Ex", "d_Bx") else m) for k in ("out", "e_out", "d_Ce", "d_Dx", "d_Ex", "d_Bx")}
    den = torch.empty((n, C), device=DEV)
    v = {k: b[1] for k, b in bufs.items()}
    edge = (lambda t: nv.ptr(t)) if m else (lambda t: None)
    nv.call("esc_gated_gcn_fwd", nv.ptr(Ax), ld, nv.ptr(Bx), ld, nv.ptr(Dx), ld, nv.ptr(Ex), ld, edge(Ce), ld, nv.ptr(plan.in_ptr),
            edge(plan.in_edge), edge(plan.in_src), n, m, C, nv.ptr(v["out"]), ld, edge(v["e_out"]), ld, nv.ptr(den), nv.stream())
    nv.call("esc_gated_gcn_bwd", nv.ptr(go_), ld, edge(ge_) if ge_ is not None else None, ld, edge(v["e_out"]), ld, nv.ptr(den),
            nv.ptr(v["out"]), ld, nv.ptr(Ax), ld, nv.ptr(Bx), ld, nv.ptr(plan.in_ptr), edge(plan.in_edge), edge(plan.in_src),
            nv.ptr(plan.out_ptr), edge(plan.out_edge), edge(plan.out_dst), n, m, C, edge(v["d_Ce"]), ld, nv.ptr(v["d_Dx"]), ld,
            nv.ptr(v["d_Ex"]), ld, nv.ptr(v["d_Bx"]), ld, nv.stream())
    torch.cuda.synchronize()
    return v, den, {k: b[0] for k, b in bufs.items()}


def test_raw_abi_against_the_oracle(E):
    """once through the C ABI itself: the batch at C = 64 with g_e, den included, and the same call with g_e NULL"""
    name, C = "batch", 64
    ops, g_out, g_e = gg.inputs_of(name, C)
    for with_ge in (True, False):
        ref = gg.reference(name, C, with_ge)
        v, den, _ = raw_call(E, name, C, ops, g_out, g_e if with_ge else None, plan_of(E, name))
        for k, got in dict(v, den=den).items():
            check("raw %s %s" % ("g_e" if with_ge else "NULL g_e", k), got, ref[F64][k], ref[F32][k])
    zero_in = [a for a in range(gg.CASES[name][0]) if a not in set(gg.CASES[name][2])]
    assert zero_in and torch.equal(den[zero_in].cpu(), torch.zeros(len(zero_in), C))
    assert torch.equal(v["out"][zero_in].cpu(), ops[0][zero_in])                   # out = Ax exactly: 0 / 1e-6


@pytest.mark.parametrize("name,C", [("degree-ladder", C) for C in gg.WIDTHS + (gg.LADDER_WIDTH,)] + [("molecule-30", gg.LADDER_WIDTH)])
def test_every_tail_length_and_the_second_column_pass(E, name, C):
    """the degree ladder (in- and out-degrees 0 .. 17: every tail of the batched walk) and width 260 (the first at which a group
    of 64 lanes runs its column loop twice, with one live lane), through the op and through the C ABI, with and without g_e"""
    ops, g_out, g_e = gg.inputs_of(name, C)
    for with_ge in (True, False):
        ref = gg.reference(name, C, with_ge)
        out, e_out, x = run_op(E, name, C, with_ge)
        got = dict(out=out, e_out=e_out, **{"d_" + k: t.grad for k, t in zip(OPERANDS, x)})
        v, den, _ = raw_call(E, name, C, ops, g_out, g_e if with_ge else None, plan_of(E, name))
        for how, tensors in (("op", got), ("raw", dict(v, den=den))):
            for k, t in tensors.items():
                check("%s %s C=%d %s %s" % (how, name, C, "g_e" if with_ge else "no-g_e", k), t, ref[F64][k], ref[F32][k],
                      gg.scale_floor(name, C, with_ge, k))
        for k in v:                                              # (d_Ax is g_out, formed by the op: the C ABI has no such output)
            assert torch.equal(got[k], v[k]), "%s: the op and the C ABI differ" % k


# ---- 2. column slices -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 68])
def test_column_slices_of_wider_buffers(E, C):
    name, SENT = "batch", -777.0
    ops, g_out, g_e = gg.inputs_of(name, C)
    ref = gg.reference(name, C, True)
    v, den, whole = raw_call(E, name, C, ops, g_out, g_e, plan_of(E, name), ld_extra=8, sentinel=SENT)
    for k, got in v.items():
        check("sliced C=%d %s" % (C, k), got, ref[F64][k], ref[F32][k])
        outside = torch.cat([whole[k][:, :4], whole[k][:, 4 + C:]], 1)
        assert bool((outside == SENT).all()), "%s: a column outside the slice was written" % k
    plain, _, _ = raw_call(E, name, C, ops, g_out, g_e, plan_of(E, name))
    for k in v:
        assert torch.equal(v[k], plain[k]), "%s: the slice changes the bits" % k
    # ... and through the op: operands that are column slices are taken in place and give the same bits
    x = [torch.nn.functional.pad(t, (4, 4)).to(DEV)[:, 4:4 + C].requires_grad_(True) for t in ops]
    out, e_out = E.ops.gated_gcn_aggregate(*x, plan_of(E, name))
    assert torch.equal(out, plain["out"]) and torch.equal(e_out, plain["e_out"])


# ---- 3. bit equality --------------------------------------------------------------------------------------------------------------
def _bits(E, name, C, ops, g_out, g_e, plan):
    v, den, _ = raw_call(E, name, C, ops, g_out, g_e, plan)
    return dict(v, den=den)


@pytest.mark.parametrize("C", [64, 256])
def test_bits_run_to_run_and_alone_against_inside_the_batch(E, C):
    ops, g_out, g_e = gg.inputs_of("batch", C)
    first = _bits(E, "batch", C, ops, g_out, g_e, plan_of(E, "batch"))
    again = _bits(E, "batch", C, ops, g_out, g_e, plan_of(E, "batch"))
    for k in first:
        assert torch.equal(first[k], again[k]), "%s differs run to run" % k
    for name, (n0, n1, e0, e1) in gg.WHERE.items():
        part = [t[n0:n1] for t in ops[:4]] + [ops[4][e0:e1]]
        alone = _bits(E, name, C, part, g_out[n0:n1], g_e[e0:e1], plan_of(E, name))
        for k, t in alone.items():
            lo, hi = (e0, e1) if k in ("e_out", "d_Ce") else (n0, n1)
            assert torch.equal(t, first[k][lo:hi]), "%s: %s alone differs from its rows inside the batch" % (name, k)


def test_bits_survive_a_relabelling_that_keeps_the_edge_order(E):
    """the reversed star with its nodes renamed by a permutation: every node's in- and out-edges keep their order, so every
    row has the bits of the row it was renamed from"""
    name, C = "star-out-300", 64
    n, src, dst = gg.edges_of(name)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))              # new name of node a: perm[a]
    gg.CASES["star-out-300/renamed"] = (n, perm[src].tolist(), perm[dst].tolist())
    try:
        ops, g_out, g_e = gg.inputs_of(name, C)
        base = _bits(E, name, C, ops, g_out, g_e, plan_of(E, name))
        inv = torch.argsort(perm)                                                       # renamed row b holds old row inv[b]
        moved = [t[inv] for t in ops[:4]] + [ops[4]]
        got = _bits(E, "star-out-300/renamed", C, moved, g_out[inv], g_e, plan_of(E, "star-out-300/renamed"))
    finally:
        del gg.CASES["star-out-300/renamed"]
    for k in base:
        want = base[k] if k in ("e_out", "d_Ce") else base[k][inv.to(DEV)]
        assert torch.equal(got[k], want), k


# ---- 4. saturated gates -------------------------------------------------------------------------------------------------------------
def test_saturated_gates_stay_finite_and_sub_convex(E):
    """aggr_i = sum_k w_k Bx_j with w_k = s_k / (den + 1e-6) >= 0 and sum_k w_k < 1: a sub-convex combination, so it lies in
    the hull of the neighbours' Bx AND zero - between min(0, min Bx_j) and max(0, max Bx_j).  (Without the zero the statement
    fails for the oracle itself: one neighbour gives aggr = Bx_j * s / (s + 1e-6), strictly inside (0, Bx_j).)  out - Ax is
    formed in fp64 from fp32 values, so it carries out's rounding: half an ulp of |out| on either side."""
    name, C = "batch", 64
    ref = gg.reference(name, C, False, SAT_SCALE)
    out, e_out, x = run_op(E, name, C, False, SAT_SCALE)
    assert float(ref[F64]["e_out"].abs().max()) >= 40.0
    for t in (out, e_out) + tuple(v.grad for v in x):
        assert bool(torch.isfinite(t).all())
    for k, got in (("out", out), ("e_out", e_out)):
        check("saturated " + k, got, ref[F64][k], ref[F32][k])
    n, src, dst = gg.edges_of(name)
    Ax, Bx = (gg.inputs_of(name, C, SAT_SCALE)[0][i].double() for i in (0, 1))
    lo = torch.zeros(n, C, dtype=F64).scatter_reduce_(0, dst.view(-1, 1).expand(-1, C), Bx[src], "amin", include_self=True)
    hi = torch.zeros(n, C, dtype=F64).scatter_reduce_(0, dst.view(-1, 1).expand(-1, C), Bx[src], "amax", include_self=True)
    aggr = out.detach().cpu().double() - Ax
    slack = out.detach().cpu().double().abs() * 2.0 ** -24
    assert bool((aggr >= lo - slack).all()) and bool((aggr <= hi + slack).all())


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host(E):
    nv = E._native
    plan = plan_of(E, "pair")
    assert E.ops.gated_gcn_max_channels() == 1024
    for C in (6, 1028):
        x = [torch.zeros(2, C, device=DEV) for _ in range(4)] + [torch.zeros(1, C, device=DEV)]
        with pytest.raises(ValueError, match="multiple of 4 with 4 <= C <= 1024"):
            E.ops.gated_gcn_aggregate(*x, plan)
        buf = torch.zeros(2, 1032, device=DEV)
        args = [nv.ptr(buf), 1032] * 5 + [nv.ptr(plan.in_ptr), nv.ptr(plan.in_edge), nv.ptr(plan.in_src), 2, 1, C, nv.ptr(buf), 1032,
                                          nv.ptr(buf), 1032, nv.ptr(buf), nv.stream()]
        with pytest.raises(RuntimeError, match=r"multiple of 4 with 4 <= C <= 1024 \(esc_gated_gcn_max_channels\)"):
            nv.call("esc_gated_gcn_fwd", *args)
    buf, sent = torch.zeros(2, 64, device=DEV), torch.full((2, 64), 5.0, device=DEV)
    args = [nv.ptr(buf), 64] * 4 + [nv.ptr(buf), 60, nv.ptr(plan.in_ptr), nv.ptr(plan.in_edge), nv.ptr(plan.in_src), 2, 1, 64,
                                    nv.ptr(sent), 64, nv.ptr(sent), 64, nv.ptr(sent), nv.stream()]
    with pytest.raises(RuntimeError, match="leading dimension ld_ce=60.*>= C=64"):
        nv.call("esc_gated_gcn_fwd", *args)
    bwd = [nv.ptr(buf), 64, None, 0, nv.ptr(buf), 64, nv.ptr(buf), nv.ptr(buf), 64, nv.ptr(buf), 64, nv.ptr(buf), 62] \
        + [nv.ptr(getattr(plan, f)) for f in ("in_ptr", "in_edge", "in_src", "out_ptr", "out_edge", "out_dst")] \
        + [2, 1, 64] + [nv.ptr(sent), 64] * 4 + [nv.stream()]
    with pytest.raises(RuntimeError, match="leading dimension ld_bx=62"):
        nv.call("esc_gated_gcn_bwd", *bwd)
    bwd[0] = nv.ptr(buf) + 4
    bwd[12] = 64
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        nv.call("esc_gated_gcn_bwd", *bwd)
    torch.cuda.synchronize()
    assert bool((sent == 5.0).all())                                               # nothing was launched
    x = [torch.zeros(2, 64, device=DEV) for _ in range(4)]
    with pytest.raises(ValueError, match="Ce has 3 rows, the batch has 1 edges"):
        E.ops.gated_gcn_aggregate(*x, torch.zeros(3, 64, device=DEV), plan)
    with pytest.raises(ValueError, match="share one width"):
        E.ops.gated_gcn_aggregate(x[0], x[1][:, :32], x[2], x[3], torch.zeros(1, 64, device=DEV), plan)


# ---- 6. the layer -------------------------------------------------------------------------------------------------------------------
def _perturb(module):
    for m in module.modules():                                # BatchNorm affine off its defaults: every term counts
        if isinstance(m, torch.nn.BatchNorm1d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, std=0.1)


def _compare_models(what, mine, oracle64, oracle32, run_mine, run_oracle):
    outs = {}
    for tag, model, run in (("mine", mine, run_mine), ("f64", oracle64, run_oracle), ("f32", oracle32, run_oracle)):
        model.zero_grad()
        outs[tag] = run(model)
    p64, p32 = dict(oracle64.named_parameters()), dict(oracle32.named_parameters())
    for k in outs["f64"]:
        check("%s %s" % (what, k), outs["mine"][k], outs["f64"][k], outs["f32"][k])
    for n, p in mine.named_parameters():
        if p64[n].grad is None:
            # in the state_dict, not in the forward: the attn_bias modules, the last layer's edge BatchNorm (nothing reads the
            # edge attributes that leave the last layer - the op's backward then runs with g_e absent) and, without a global
            # model, norm1_attn
            assert ("edge_attn" in n or n.startswith("layers.1.local_model.bn_edge_e.") or (mine.has_attention is False and ".norm1_attn." in n)) \
                and p.grad is None, n
            continue
        # A bias gradient (Linear or BatchNorm) is a column sum over the rows of the very terms whose products with unit-scale
        # inputs make the weight gradient of the same module, and behind a training-mode BatchNorm that sum cancels: to zero in
        # exact arithmetic where the Linear feeds the BatchNorm directly (A, ff_linear2, out_proj, z_embedding.3: 1e-16 in fp64,
        # 1e-7 in any fp32), to the gate's 1e-6 for B, by two or three orders for a BatchNorm bias whose constant the next
        # layer's BatchNorms remove again (norm2.bias of layer 0: torch's own fp32 is 9.6e-6 of its largest value).  What bounds
        # the rounding error of a sum is the size of its terms, not of its result, so a bias gradient is measured over the
        # larger of its own largest value and its weight gradient's.  Every other tensor: the project's measure unchanged.
        floor, weight = 0.0, p64.get(n[:-len("bias")] + "weight") if n.endswith(".bias") else None
        if weight is not None and weight.grad is not None:
            floor = float(weight.grad.abs().max())
        check("%s grad %s" % (what, n), p.grad, p64[n].grad, p32[n].grad, floor)


def test_layer_against_the_oracle_layer(E):
    import copy
    name, W = "molecule-30", 16
    n, src, dst = gg.edges_of(name)
    gen = torch.Generator().manual_seed(16)
    x, e = torch.randn(n, W, generator=gen), torch.randn(src.numel(), W, generator=gen)
    gx, ge = torch.randn(n, W, generator=gen), torch.randn(src.numel(), W, generator=gen)
    torch.manual_seed(6)
    oracle32 = gg.GatedGCNLayer(W, W)
    _perturb(oracle32)
    oracle64 = copy.deepcopy(oracle32).double()
    mine = E.nn.GatedGCNLayer(W, W, 0.0, True)
    mine.load_state_dict(oracle32.state_dict())
    mine = mine.to(DEV)
    plan, ei = plan_of(E, name), torch.stack([src, dst])

    def run_mine(m):
        h, e2 = m(x.to(DEV), e.to(DEV), plan)
        if m.training:
            ((h * gx.to(DEV)).sum() + (e2 * ge.to(DEV)).sum()).backward()
        return dict(x=h.detach(), e=e2.detach())

    def run_oracle(m):
        dt = next(m.parameters()).dtype
        h, e2 = m(x.to(dt), e.to(dt), ei)
        if m.training:
            ((h * gx.to(dt)).sum() + (e2 * ge.to(dt)).sum()).backward()
        return dict(x=h.detach(), e=e2.detach())

    _compare_models("layer train", mine, oracle64, oracle32, run_mine, run_oracle)          # ... which also moved the running statistics
    for (k, b), (_, b64) in zip(mine.named_buffers(), oracle64.named_buffers()):
        check("layer buffer " + k, b, b64, dict(oracle32.named_buffers())[k])
    for m in (mine, oracle64, oracle32):
        m.eval()
    with torch.no_grad():
        got, want, want32 = run_mine(mine), run_oracle(oracle64), run_oracle(oracle32)
    for k in want:
        check("layer eval " + k, got[k], want[k], want32[k])


# ---- 7. the model -------------------------------------------------------------------------------------------------------------------
_MOLS = {}


def molecules(E):
    if not _MOLS:
        from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
        graphs = build_feature_dataset(synthetic_zinc_graphs(0, 5), 3, use_rd=True, self_loop=True)
        batch = E.Batch.from_data_list([g for g in graphs])
        _MOLS["cpu"] = {k: batch[k].cpu() for k in ("x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
        _MOLS["graphs"] = graphs
    return _MOLS


@pytest.mark.parametrize("global_model_type", ["Transformer", "None"])
def test_model_against_the_oracle_model(E, global_model_type):
    import copy
    from esc_gnn_amd.gps_models import GPSModel
    mol = molecules(E)
    kw = dict(layers=2, dim_hidden=16, n_heads=2, local_gnn_type="CustomGatedGCN", global_model_type=global_model_type)
    torch.manual_seed(7)
    oracle32 = gg.GPSModel(**kw)
    _perturb(oracle32)
    for m in oracle32.modules():
        if isinstance(m, torch.nn.MultiheadAttention):
            torch.nn.init.normal_(m.in_proj_bias, std=0.1)
            torch.nn.init.normal_(m.out_proj.bias, std=0.1)
    oracle64 = copy.deepcopy(oracle32).double()
    mine = GPSModel(dropout=0.0, attn_dropout=0.0, **kw)
    mine.load_state_dict(oracle32.state_dict())
    mine = mine.to(DEV).train()
    y = torch.tensor([0.3, -1.1, 0.7, 0.2, -0.4], dtype=F64).view(-1, 1)

    def run_mine(m):
        pred = m(E.Batch.from_data_list([g for g in mol["graphs"]]).to(DEV))
        E.ops.l1_loss(pred, y.float().to(DEV)).backward()
        return dict(prediction=pred.detach())

    def run_oracle(m):
        pred = m(mol["cpu"])
        (pred - y.to(pred.dtype)).abs().mean().backward()
        return dict(prediction=pred.detach())

    _compare_models("CustomGatedGCN+" + global_model_type, mine, oracle64.train(), oracle32.train(), run_mine, run_oracle)


# ---- 8. the default is untouched ------------------------------------------------------------------------------------------------------
def test_default_model_is_bit_identical_to_the_spelled_out_default(E):
    from esc_gnn_amd.gps_models import GPSModel
    mol = molecules(E)
    kw = dict(layers=2, dim_hidden=16, n_heads=2, dropout=0.0, attn_dropout=0.0)
    torch.manual_seed(8)
    a = GPSModel(**kw)
    torch.manual_seed(8)
    b = GPSModel(local_gnn_type="GINE", global_model_type="Transformer", **kw)
    assert list(a.state_dict()) == list(b.state_dict()) and all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    preds = [m.to(DEV).train()(E.Batch.from_data_list([g for g in mol["graphs"]]).to(DEV)) for m in (a, b)]
    assert torch.equal(preds[0], preds[1])


# ---- 9. the driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_trains_checkpoints_evaluates_and_refuses_the_other_layout(E, tmp_path, monkeypatch, capsys):
    import esc_gnn_amd.run_zinc_gps as rg
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = "--synthetic_graphs 24 --layers 2 --batch_size 8 --save_appendix _g"
    rg.main(("--gt_layer_type CustomGatedGCN+Transformer --epochs 1 " + common).split())
    out = capsys.readouterr().out
    lines = re.findall(r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)", out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    ckpt = tmp_path / "results" / "zinc_GPS_g" / "model_checkpoint1.pth"
    assert ckpt.exists()
    assert any(k.endswith("local_model.bn_edge_e.running_var") for k in torch.load(ckpt, map_location="cpu"))
    rg.main(("--gt_layer_type CustomGatedGCN+Transformer --eval 1 --load_model %s " % ckpt + common).split())
    m = re.search(r"Test MAE: (\S+)", capsys.readouterr().out)
    assert m and abs(float(m.group(1)) - float(lines[-1][4].rstrip(","))) <= 2e-7          # both are printed to 7 decimals
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        rg.main(("--eval 1 --load_model %s " % ckpt + common).split())
