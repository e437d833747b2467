"""The PNA aggregate kernels (csrc/pna.hip), ops.pna_aggregate, nn.PNAConv, the PNA variants of GPSLayer / GPSModel and the
driver's two new --gt_layer_type names on the GPU, against tests/pna_oracle.py evaluated in fp64 on the CPU.  Error measure and
bound 1e-5 are the project's (tests/gps_cases.py), the oracle's own fp32 figure is printed beside every kernel figure, and arg -
the edge position of every maximum - is held exactly: tests/test_pna_cpu.py holds the condition under which fp32 and fp64 agree
on it.  A bias gradient that a following training-mode BatchNorm cancels is measured as tests/test_hip_gatedgcn.py measures it.
References are computed once per case and shared."""
import copy
import math
import re

import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import gps_cases as gc
import pna_oracle as po

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64, F32 = torch.float64, torch.float32
FLOATS = ("agg", "d_P", "d_Q", "d_R")
MODEL_GAP = 1e-5                          # of a layer's largest |message|: ten times what fp32 GEMM rounding can move a message


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


_PLANS = {}


def make_plan(E, n, src, dst):
    """the plan of an edge list from a stable argsort on the CPU: the two views exactly as the header describes them"""
    kw = dict(num_nodes=n, num_edges=src.numel(), nnz=0)
    for view, key, other in (("in", dst, src), ("out", src, dst)):
        perm = torch.sort(key, stable=True).indices
        ptr = torch.zeros(n + 1, dtype=torch.int64)
        if n:
            ptr[1:] = torch.cumsum(torch.bincount(key, minlength=n), 0)[:n]
        kw[view + "_ptr"] = ptr.to(torch.int32).to(DEV)
        kw[view + "_edge"] = perm.to(torch.int32).to(DEV)
        kw[view + ("_src" if view == "in" else "_dst")] = other[perm].to(torch.int32).to(DEV)
    return E.BatchPlan(**kw)


def plan_of(E, name):
    if name not in _PLANS:
        _PLANS[name] = make_plan(E, *po.edges_of(name))
    return _PLANS[name]


def check(what, got, want64, want32, floor=0.0):
    e, e32 = po.rel(got, want64, floor), po.rel(want32, want64, floor)
    print("%-44s kernel %.3g   torch fp32 on the CPU %.3g" % (what, e, e32))
    assert e <= gc.BOUND, "%s: %.3g of the largest value, bound %g (torch fp32: %.3g)" % (what, e, gc.BOUND, e32)


def run_op(E, ops, g, plan):
    """dict(agg, arg, d_P, d_Q, d_R) through ops.pna_aggregate; arg is what the Function keeps for its backward"""
    x = [t.to(DEV).requires_grad_(True) for t in ops]
    agg = E.ops.pna_aggregate(*x, plan)
    arg, = agg.grad_fn.saved_tensors
    (agg * g.to(DEV)).sum().backward()
    return dict(agg=agg.detach(), arg=arg, **{"d_" + k: t.grad for k, t in zip("PQR", x)})


def raw_call(E, C, ops, g, plan, sliced=False, sentinel=-777.0):
    """esc_pna_aggregate_fwd and _bwd through the C ABI.  sliced: every operand a column slice of a buffer 8 wider with NaN
    around it, every output inside a buffer with a sentinel row above and below and sentinel columns left and right - agg in
    the columns C .. 4C of an [N, 4C] buffer, as the layer's post-layer operand would hold it.  Returns (views, whole buffers)."""
    nv = E._native
    n, m = plan.num_nodes, plan.num_edges

    def operand(t):
        if not sliced:
            return t.to(DEV).contiguous()
        buf = torch.full((t.size(0), t.size(1) + 8), float("nan"), device=DEV)
        buf[:, 4:4 + t.size(1)] = t.to(DEV)
        return buf[:, 4:4 + t.size(1)]

    def output(rows, width, left, total, dtype=F32):
        buf = torch.full((rows + 2, total if sliced else width), sentinel, device=DEV, dtype=dtype)
        return buf, buf[1:rows + 1, (left if sliced else 0):(left if sliced else 0) + width]

    P, Q, R, g_ = (operand(t) for t in (*ops, g))
    whole, v = {}, {}
    for k, (rows, width, left, total, dtype) in dict(agg=(n, 3 * C, C, 4 * C, F32), arg=(n, C, 0, C, torch.int32), d_R=(m, C, 4, C + 8, F32),
                                                      d_P=(n, C, 4, C + 8, F32), d_Q=(n, C, 4, C + 8, F32)).items():
        whole[k], v[k] = output(rows, width, left, total, dtype)
    ld = lambda t: t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1))          # noqa: E731
    edge = (lambda t: nv.ptr(t)) if m else (lambda t: None)
    nv.call("esc_pna_aggregate_fwd", nv.ptr(P), ld(P), nv.ptr(Q), ld(Q), edge(R), ld(R), nv.ptr(plan.in_ptr), edge(plan.in_edge),
            edge(plan.in_src), n, m, C, nv.ptr(v["agg"]), ld(v["agg"]), nv.ptr(v["arg"]), nv.stream())
    nv.call("esc_pna_aggregate_bwd", nv.ptr(g_), ld(g_), nv.ptr(v["arg"]), nv.ptr(plan.in_ptr), edge(plan.in_edge), edge(plan.in_src),
            nv.ptr(plan.out_ptr), edge(plan.out_edge), edge(plan.out_dst), n, m, C, edge(v["d_R"]), ld(v["d_R"]), nv.ptr(v["d_P"]),
            ld(v["d_P"]), nv.ptr(v["d_Q"]), ld(v["d_Q"]), nv.stream())
    torch.cuda.synchronize()
    return v, whole


def against_the_oracle(what, got, ref):
    assert torch.equal(got["arg"].cpu().long(), ref[F64]["arg"]), "%s: arg differs from the oracle's" % what
    for k in FLOATS:
        assert got[k].shape == ref[F64][k].shape, (what, k)
        check("%s %s" % (what, k), got[k], ref[F64][k], ref[F32][k])


# ---- 1. forward and backward against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C", po.WIDTHS)
def test_op_against_the_oracle(E, C):
    for name in po.CASES:
        ops, g = po.inputs_of(name, C)
        against_the_oracle("%s C=%d" % (name, C), run_op(E, ops, g, plan_of(E, name)), po.reference(name, C))


@pytest.mark.parametrize("C", po.WIDTHS)
def test_raw_abi_against_the_oracle(E, C):
    for name in po.CASES:
        ops, g = po.inputs_of(name, C)
        v, _ = raw_call(E, C, ops, g, plan_of(E, name))
        against_the_oracle("raw %s C=%d" % (name, C), v, po.reference(name, C))
    n, _, dst = po.edges_of("batch")
    zero_in = [a for a in range(n) if a not in set(dst.tolist())]
    assert zero_in and bool((v["arg"][zero_in] == -1).all()) and bool((v["agg"][zero_in] == 0).all())


# ---- 2. ties and signs --------------------------------------------------------------------------------------------------------------
def _integers(n, m, C, seed, degree_lcm):
    """operands from the integers -2 .. 2 and an upstream gradient from multiples of degree_lcm: every message, sum, quotient
    g_mean / deg and gradient is a small integer, exact in fp32 in any order"""
    gen = torch.Generator().manual_seed(seed)
    mk = lambda rows, cols: torch.randint(-2, 3, (rows, cols), generator=gen).float()       # noqa: E731
    return [mk(n, C), mk(n, C), mk(m, C)], mk(n, 3 * C) * degree_lcm


def _tie_counts(ops, src, dst, n, C):
    m = po.messages(*[t.double() for t in ops], src, dst)
    top = po.aggregate_messages(m, dst, n)[0][:, C:2 * C]
    return torch.zeros(n, C, dtype=F64).index_add_(0, dst, (m == top[dst]).double())


@pytest.mark.parametrize("name", ["repeated-edge", "molecule-30"])
def test_ties_go_to_the_lowest_edge_position_bit_for_bit(E, name):
    C = 8
    n, src, dst = po.edges_of(name)
    ops, g = _integers(n, src.numel(), C, 0, 12)                          # in-degrees 1 .. 4
    assert int(torch.bincount(dst).max()) <= 4
    if name == "repeated-edge":
        ops[2][1] = ops[2][0]                                             # the two edges 0 -> 1 carry equal rows: a tie in every column
    held = _tie_counts(ops, src, dst, n, C)
    if name == "repeated-edge":
        assert bool((held[1] == 2).all())
    else:
        assert int((held == 2).sum()) >= 10 and int((held == 3).sum()) >= 1, "the case has lost its two- and three-way ties"
    want = po.run(ops, g, src, dst, F64)
    for what, got in (("op", run_op(E, ops, g, plan_of(E, name))), ("raw", raw_call(E, C, ops, g, plan_of(E, name))[0])):
        assert torch.equal(got["arg"].cpu().long(), want["arg"]), what
        for k in ("d_P", "d_Q", "d_R"):
            assert torch.equal(got[k].cpu(), want[k].float()), "%s %s is not the oracle's rule bit for bit" % (what, k)
        agg = got["agg"].cpu()
        assert torch.equal(agg[:, C:], want["agg"][:, C:].float())       # max and sum are integers
        deg = torch.bincount(dst, minlength=n).clamp(min=1).float().view(-1, 1)
        assert torch.equal(agg[:, :C], agg[:, 2 * C:] / deg)             # the mean is the IEEE quotient of the exact sum


def test_all_negative_messages_up_to_1e30_keep_a_negative_finite_maximum(E):
    name, C = "batch", 64
    ops, g = po.inputs_of(name, C)
    n, src, dst = po.edges_of(name)
    scale = 10.0 ** torch.linspace(-3, 30, C).view(1, -1)                 # per column; the hub's sum of 300 stays below 1e33
    ops = [-(t.abs() + 0.01) * scale for t in ops]
    want = po.run(ops, g, src, dst, F32)                                  # the same fp32 additions in the same order: equal bits
    got = run_op(E, ops, g, plan_of(E, name))
    has = torch.bincount(dst, minlength=n) > 0
    top = got["agg"][:, C:2 * C].cpu()
    assert bool(torch.isfinite(got["agg"]).all()) and bool((top[has] < 0).all()) and float(top[has].abs().max()) > 1e29
    assert bool((top[~has] == 0).all())
    assert torch.equal(got["arg"].cpu().long(), want["arg"]) and torch.equal(top, want["agg"][:, C:2 * C])
    for k in ("d_P", "d_Q", "d_R"):
        assert bool(torch.isfinite(got[k]).all()), k


# ---- 3. layouts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 68])
def test_column_slices_of_wider_buffers(E, C):
    name, SENT = "batch", -777.0
    ops, g = po.inputs_of(name, C)
    v, whole = raw_call(E, C, ops, g, plan_of(E, name), sliced=True, sentinel=SENT)
    against_the_oracle("sliced C=%d" % C, v, po.reference(name, C))
    assert v["agg"].stride(0) == 4 * C and v["agg"].storage_offset() == 4 * C + C        # columns C .. 4C of the [N, 4C] buffer
    for k, buf in whole.items():
        inside = torch.zeros_like(buf, dtype=torch.bool)
        left = {"agg": C, "arg": 0}.get(k, 4)
        inside[1:-1, left:left + v[k].size(1)] = True
        assert bool((buf[~inside] == (int(SENT) if k == "arg" else SENT)).all()), "%s: an element outside the slice was written" % k
    plain, _ = raw_call(E, C, ops, g, plan_of(E, name))
    for k in v:
        assert torch.equal(v[k], plain[k]), "%s: the slice changes the bits" % k
    # ... and through the op: operands that are column slices are taken in place and give the same bits, as does a gradient
    # that arrives as the columns C .. 4C of a wider one (what the layer's cat hands back)
    x = [torch.nn.functional.pad(t, (4, 4)).to(DEV)[:, 4:4 + C].requires_grad_(True) for t in ops]
    agg = E.ops.pna_aggregate(*x, plan_of(E, name))
    wide = torch.cat([torch.zeros(agg.size(0), C, device=DEV), agg], 1)
    (wide * torch.nn.functional.pad(g, (C, 0)).to(DEV)).sum().backward()
    assert torch.equal(agg.detach(), plain["agg"])
    for k, t in zip("PQR", x):
        assert torch.equal(t.grad, plain["d_" + k]), k


# ---- 4. bit equality ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 256])
def test_bits_run_to_run_and_alone_against_inside_the_batch(E, C):
    ops, g = po.inputs_of("batch", C)
    first, _ = raw_call(E, C, ops, g, plan_of(E, "batch"))
    again, _ = raw_call(E, C, ops, g, plan_of(E, "batch"))
    for k in first:
        assert torch.equal(first[k], again[k]), "%s differs run to run" % k
    for name, (n0, n1, e0, e1) in po.WHERE.items():
        part = [ops[0][n0:n1], ops[1][n0:n1], ops[2][e0:e1]]
        alone, _ = raw_call(E, C, part, g[n0:n1], plan_of(E, name))
        for k, t in alone.items():
            lo, hi = (e0, e1) if k == "d_R" else (n0, n1)
            want = first[k][lo:hi]
            if k == "arg":                                             # edge positions count from the graph's first edge
                want = torch.where(want >= 0, want - e0, want)
            assert torch.equal(t, want), "%s: %s alone differs from its rows inside the batch" % (name, k)


def test_bits_survive_a_relabelling_that_keeps_the_edge_order(E):
    """the molecule with its nodes renamed by a permutation: the edge positions stay, so every node's in- and out-edges keep
    their order and every row has the bits of the row it was renamed from"""
    name, C = "molecule-30", 64
    n, src, dst = po.edges_of(name)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))              # new name of node a: perm[a]
    ops, g = po.inputs_of(name, C)
    base, _ = raw_call(E, C, ops, g, plan_of(E, name))
    inv = torch.argsort(perm)                                                       # renamed row b holds old row inv[b]
    got, _ = raw_call(E, C, [ops[0][inv], ops[1][inv], ops[2]], g[inv], make_plan(E, n, perm[src], perm[dst]))
    for k in base:
        want = base[k] if k == "d_R" else base[k][inv.to(DEV)]
        assert torch.equal(got[k], want), k


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host(E):
    nv = E._native
    plan = plan_of(E, "pair")
    views = [nv.ptr(getattr(plan, f)) for f in ("in_ptr", "in_edge", "in_src", "out_ptr", "out_edge", "out_dst")]
    assert E.ops.pna_max_channels() == 1024
    sent = torch.full((2, 4096), 5.0, device=DEV)
    isent = torch.full((2, 1024), 5, device=DEV, dtype=torch.int32)
    buf = torch.zeros(2, 4096, device=DEV)

    def fwd(C=64, ld=(64, 64, 64), ld_agg=192, shift=0):
        return [nv.ptr(buf) + shift, ld[0], nv.ptr(buf), ld[1], nv.ptr(buf), ld[2]] + views[:3] + [2, 1, C, nv.ptr(sent), ld_agg, nv.ptr(isent),
                                                                                                  nv.stream()]

    def bwd(C=64, ld_g=192, ld=(64, 64, 64), shift=0):
        return [nv.ptr(buf), ld_g, nv.ptr(isent) + shift] + views + [2, 1, C, nv.ptr(sent), ld[0], nv.ptr(sent), ld[1], nv.ptr(sent), ld[2],
                                                                     nv.stream()]

    for C in (0, 6, 1028):
        x = [torch.zeros(2, C, device=DEV), torch.zeros(2, C, device=DEV), torch.zeros(1, C, device=DEV)]
        with pytest.raises(ValueError, match="multiple of 4 with 4 <= C <= 1024"):
            E.ops.pna_aggregate(*x, plan)
        for fn, args in (("esc_pna_aggregate_fwd", fwd(C, (1032,) * 3, 3096)), ("esc_pna_aggregate_bwd", bwd(C, 3096, (1032,) * 3))):
            with pytest.raises(RuntimeError, match=r"multiple of 4 with 4 <= C <= 1024 \(esc_pna_max_channels\)"):
                nv.call(fn, *args)
    for fn, args, word in (("esc_pna_aggregate_fwd", fwd(ld=(60, 64, 64)), "ld_p=60"), ("esc_pna_aggregate_fwd", fwd(ld=(64, 66, 64)), "ld_q=66"),
                           ("esc_pna_aggregate_fwd", fwd(ld=(64, 64, 32)), "ld_r=32"), ("esc_pna_aggregate_fwd", fwd(ld_agg=188), "ld_agg=188"),
                           ("esc_pna_aggregate_bwd", bwd(ld_g=64), "ld_g=64"), ("esc_pna_aggregate_bwd", bwd(ld=(62, 64, 64)), "ld_dr=62"),
                           ("esc_pna_aggregate_bwd", bwd(ld=(64, 60, 64)), "ld_dp=60"), ("esc_pna_aggregate_bwd", bwd(ld=(64, 64, 70)), "ld_dq=70")):
        with pytest.raises(RuntimeError, match="leading dimension %s.*row width" % word):
            nv.call(fn, *args)
    for fn, args in (("esc_pna_aggregate_fwd", fwd(shift=4)), ("esc_pna_aggregate_bwd", bwd(shift=8))):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            nv.call(fn, *args)
    torch.cuda.synchronize()
    assert bool((sent == 5.0).all()) and bool((isent == 5).all())                  # nothing was launched
    x = [torch.zeros(2, 64, device=DEV), torch.zeros(2, 64, device=DEV)]
    with pytest.raises(ValueError, match="R has 3 rows, the batch has 1 edges"):
        E.ops.pna_aggregate(*x, torch.zeros(3, 64, device=DEV), plan)
    with pytest.raises(ValueError, match="share one width"):
        E.ops.pna_aggregate(x[0], x[1][:, :32], torch.zeros(1, 64, device=DEV), plan)
    with pytest.raises(ValueError, match="share one width"):
        E.ops.pna_aggregate(x[0], x[1], torch.zeros(1, 32, device=DEV), plan)


def test_no_edges_and_no_nodes(E):
    """E == 0 with N > 0 takes NULL edge arrays and writes zeros and -1; N == 0 writes nothing"""
    C = 64
    for name in ("no-edge-3", "one-node", "empty"):
        ops, g = po.inputs_of(name, C)
        v, whole = raw_call(E, C, ops, g, plan_of(E, name), sliced=True)
        n = po.CASES[name][0]
        assert bool((v["agg"] == 0).all()) and bool((v["arg"] == -1).all()) and bool((v["d_P"] == 0).all()) and bool((v["d_Q"] == 0).all())
        assert v["agg"].shape == (n, 3 * C) and v["d_R"].shape == (0, C)
        if n == 0:
            assert all(bool((b == (-777 if k == "arg" else -777.0)).all()) for k, b in whole.items())
        got = run_op(E, ops, g, plan_of(E, name))
        assert got["d_R"].shape == (0, C) and bool((got["d_P"] == 0).all()) and got["agg"].shape == (n, 3 * C)


# ---- 6. the layer ---------------------------------------------------------------------------------------------------------------------
def _perturb(module):
    for m in module.modules():                                # BatchNorm affine off its defaults: every term counts
        if isinstance(m, torch.nn.BatchNorm1d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, std=0.1)
        if isinstance(m, torch.nn.MultiheadAttention):
            torch.nn.init.normal_(m.in_proj_bias, std=0.1)
            torch.nn.init.normal_(m.out_proj.bias, std=0.1)


def _compare_models(what, mine, oracle64, oracle32, run_mine, run_oracle, gap_of, unused=()):
    outs = {}
    for tag, model, run in (("mine", mine, run_mine), ("f64", oracle64, run_oracle), ("f32", oracle32, run_oracle)):
        model.zero_grad()
        outs[tag] = run(model)
    worst = gap_of(oracle64)
    print("%s: smallest top-two gap of a layer's messages %.3g of its largest (condition %g)" % (what, worst, MODEL_GAP))
    assert worst >= MODEL_GAP, "%s: the seed no longer keeps the two largest messages apart; pick another on the CPU" % what
    p64, p32 = dict(oracle64.named_parameters()), dict(oracle32.named_parameters())
    for k in outs["f64"]:
        check("%s %s" % (what, k), outs["mine"][k], outs["f64"][k], outs["f32"][k])
    for n, p in mine.named_parameters():
        if p64[n].grad is None:                               # in the state_dict, not in the forward
            assert any(u in n for u in unused) and p.grad is None, n
            continue
        # a bias gradient is a column sum that a following training-mode BatchNorm cancels (lin and post_nns of the layer feed
        # norm1_local through a residual add: to zero in exact arithmetic), so it is measured over the larger of its own largest
        # value and its weight gradient's - the scale of the terms of the sum; tests/test_hip_gatedgcn.py derives the measure
        floor, weight = 0.0, p64.get(n[:-len("bias")] + "weight") if n.endswith(".bias") else None
        if weight is not None and weight.grad is not None:
            floor = float(weight.grad.abs().max())
        check("%s grad %s" % (what, n), p.grad, p64[n].grad, p32[n].grad, floor)


def test_layer_against_the_oracle_layer(E):
    name, W = "molecule-30", 16
    n, src, dst = po.edges_of(name)
    gen = torch.Generator().manual_seed(16)
    x, e, gx = torch.randn(n, W, generator=gen), torch.randn(src.numel(), W, generator=gen), torch.randn(n, W, generator=gen)
    torch.manual_seed(20)                                     # chosen on the CPU: the oracle's gap is 1.2e-3
    oracle32 = po.PNAConv(W)
    oracle64 = copy.deepcopy(oracle32).double()
    mine = E.nn.PNAConv(W, W, edge_dim=W)
    mine.load_state_dict(oracle32.state_dict())
    mine = mine.to(DEV)
    plan, ei = plan_of(E, name), torch.stack([src, dst])

    def run_mine(m):
        xs, es = x.to(DEV).requires_grad_(True), e.to(DEV).requires_grad_(True)
        h = m(xs, ei.to(DEV), es, plan)
        (h * gx.to(DEV)).sum().backward()
        return dict(out=h.detach(), d_x=xs.grad, d_e=es.grad)

    def run_oracle(m):
        dt = next(m.parameters()).dtype
        xs, es = x.to(dt).requires_grad_(True), e.to(dt).requires_grad_(True)
        h = m(xs, ei, es)
        (h * gx.to(dt)).sum().backward()
        return dict(out=h.detach(), d_x=xs.grad, d_e=es.grad)

    def gap_of(m):
        gap, top = po.top_two_gap(*m.last, n)
        return gap / top

    _compare_models("PNAConv", mine, oracle64, oracle32, run_mine, run_oracle, gap_of)


# ---- 7. GPSLayer and GPSModel -------------------------------------------------------------------------------------------------------------
_MOLS = {}
MODEL_SEED = 14       # chosen on the CPU from the oracle alone: gaps 2.1e-4 (PNA+Transformer), 1.1e-4 (PNA+None), 2.2e-4 (GPSLayer)


def molecules(E):
    if not _MOLS:
        from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
        graphs = build_feature_dataset(synthetic_zinc_graphs(0, 6), 3, use_rd=True, self_loop=True)
        batch = E.Batch.from_data_list([g for g in graphs])
        _MOLS["cpu"] = {k: batch[k].cpu() for k in ("x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
        _MOLS["graphs"] = graphs
    return _MOLS


@pytest.mark.parametrize("global_model_type", ["Transformer", "None"])
def test_model_against_the_oracle_model(E, global_model_type):
    from esc_gnn_amd.gps_models import GPSModel
    mol = molecules(E)
    kw = dict(layers=2, dim_hidden=16, n_heads=2, local_gnn_type="PNA", global_model_type=global_model_type)
    torch.manual_seed(MODEL_SEED)
    oracle32 = po.GPSModel(**kw)
    _perturb(oracle32)
    oracle64 = copy.deepcopy(oracle32).double()
    mine = GPSModel(dropout=0.0, attn_dropout=0.0, **kw)
    mine.load_state_dict(oracle32.state_dict())
    mine = mine.to(DEV).train()
    y = torch.tensor([0.3, -1.1, 0.7, 0.2, -0.4, 0.9], dtype=F64).view(-1, 1)

    def run_mine(m):
        pred = m(E.Batch.from_data_list([g for g in mol["graphs"]]).to(DEV))
        E.ops.l1_loss(pred, y.float().to(DEV)).backward()
        return dict(prediction=pred.detach())

    def run_oracle(m):
        pred = m(mol["cpu"])
        (pred - y.to(pred.dtype)).abs().mean().backward()
        return dict(prediction=pred.detach())

    unused = ("edge_attn",) + ((".norm1_attn.",) if global_model_type == "None" else ())
    _compare_models("PNA+" + global_model_type, mine, oracle64.train(), oracle32.train(), run_mine, run_oracle,
                    lambda m: m.worst_gap(), unused)


def test_gps_layer_against_the_oracle_layer(E):
    """one GPSLayer('PNA') on its own: node states and edge attributes in, both out - the edge attributes leave with this
    layer's ESC term added and otherwise untouched"""
    from esc_gnn_amd.gps_models import GPSLayer
    from esc_gnn_amd.nested import Z_TABLE_ROWS
    from esc_gnn_amd.plan import graph_ptr_of, plan_of as batch_plan_of
    mol = molecules(E)
    b, W = mol["cpu"], 16
    N, M = b["x"].size(0), b["edge_index"].size(1)
    gen = torch.Generator().manual_seed(11)
    h, ea, gh = torch.randn(N, W, generator=gen), torch.randn(M, W, generator=gen), torch.randn(N, W, generator=gen)
    torch.manual_seed(MODEL_SEED)
    oracle32 = po.GPSLayer(W, 2)
    _perturb(oracle32)
    oracle64 = copy.deepcopy(oracle32).double()
    mine = GPSLayer(W, 2, dropout=0.0, attn_dropout=0.0, local_gnn_type="PNA")
    mine.load_state_dict(oracle32.state_dict())
    mine = mine.to(DEV).train()
    sizes = torch.bincount(b["batch"]).tolist()

    def run_mine(m):
        data = E.Batch.from_data_list([g for g in mol["graphs"]]).to(DEV)
        plan = batch_plan_of(data, Z_TABLE_ROWS)
        graph_ptr, _ = graph_ptr_of(data, plan)
        out, e2 = m(h.to(DEV), ea.to(DEV), data, plan, graph_ptr, None)
        ((out * gh.to(DEV)).sum() + e2.sum()).backward()
        return dict(h=out.detach(), edge_attr=e2.detach())

    def run_oracle(m):
        dt = next(m.parameters()).dtype
        out, e2 = m(h.to(dt), ea.to(dt), b, sizes)
        ((out * gh.to(dt)).sum() + e2.sum()).backward()
        return dict(h=out.detach(), edge_attr=e2.detach())

    def gap_of(m):
        gap, top = po.top_two_gap(*m.local_model.last, N)
        return gap / top

    _compare_models("GPSLayer PNA", mine, oracle64.train(), oracle32.train(), run_mine, run_oracle, gap_of, ("edge_attn",))


# ---- 8. the driver ------------------------------------------------------------------------------------------------------------------------
def test_driver_trains_checkpoints_and_evaluates(E, tmp_path, monkeypatch, capsys):
    import esc_gnn_amd.run_zinc_gps as rg
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = "--synthetic_graphs 24 --layers 2 --batch_size 8 --save_appendix _p"
    rg.main(("--gt_layer_type PNA+Transformer --epochs 1 " + common).split())
    out = capsys.readouterr().out
    lines = re.findall(r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)", out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    ckpt = tmp_path / "results" / "zinc_GPS_p" / "model_checkpoint1.pth"
    assert ckpt.exists()
    keys = list(torch.load(ckpt, map_location="cpu"))
    assert "layers.1.local_model.pre_nns.0.0.weight" in keys and "layers.0.self_attn.in_proj_weight" in keys
    rg.main(("--gt_layer_type PNA+Transformer --eval 1 --load_model %s " % ckpt + common).split())
    m = re.search(r"Test MAE: (\S+)", capsys.readouterr().out)
    assert m and abs(float(m.group(1)) - float(lines[-1][4].rstrip(","))) <= 2e-7          # both are printed to 7 decimals
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        rg.main(("--eval 1 --load_model %s " % ckpt + common).split())


def test_driver_trains_without_the_attention_branch(E, tmp_path, monkeypatch, capsys):
    import esc_gnn_amd.run_zinc_gps as rg
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    rg.main(("--gt_layer_type PNA+None --epochs 1 --synthetic_graphs 24 --layers 2 --batch_size 8 --save_appendix _pn").split())
    out = capsys.readouterr().out
    lines = re.findall(r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)", out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    keys = list(torch.load(tmp_path / "results" / "zinc_GPS_pn" / "model_checkpoint1.pth", map_location="cpu"))
    assert "layers.1.local_model.lin.bias" in keys and not any(".self_attn." in k for k in keys)
