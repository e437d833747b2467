"""The per-graph LayerNorm on the GPU: esc_graph_layer_norm_fwd / _bwd against the fp64 oracle of tests/layernorm_oracle.py on
every width class, graph size and conditioning of its case list (y, stats, d_x, d_weight, d_bias), the folded residual bit for
bit against an add beforehand, column slices, bit stability run to run and between a graph alone and inside other batches, the
skip contract over sentinel-filled outputs, the host limits, nn.GraphLayerNorm, GPSModel with the two normalisation switches
against the oracle model for every local type, and the driver.

Error measure: max |got - want| over the largest |want| of the tensor.  Bound, for y, stats, d_x, d_weight and d_bias alike:
max(1e-5, 4 x the distance of torch's fp32 evaluation of the same oracle on the CPU from fp64), measured per case and tensor
(the rule of tests/test_hip_spd.py; the factor 4 covers another summation order); both figures are printed.  The model
comparison uses the measure and the tolerances of tests/test_hip_gps.py (1e-5 predictions, 1e-4 gradients and buffers)."""
import contextlib
import copy
import io
import math
import os
import re

import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import layernorm_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-5
FILL = -777.25
KEYS = ("y", "stats", "d_x", "d_weight", "d_bias")


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def graph_ptr(sizes):
    return torch.tensor(lo.go.graph_ptr_of(sizes), dtype=torch.int32, device=DEV)


def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if not want.numel():
        return 0.0
    top, err = float(want.abs().max()), float((got - want).abs().max())
    return err / top if top > 0 else (0.0 if err == 0 else float("inf"))


def run_op(E, x, sizes, weight, bias, gy, residual=None):
    """the op and its backward on copies of the inputs: y, stats, d_x, d_weight, d_bias (and d_residual)"""
    xs = x.to(DEV).detach().clone().requires_grad_(True)
    rs = None if residual is None else residual.to(DEV).detach().clone().requires_grad_(True)
    w = None if weight is None else weight.to(DEV).detach().clone().requires_grad_(True)
    b = None if bias is None else bias.to(DEV).detach().clone().requires_grad_(True)
    y, stats = E.ops.graph_layer_norm(xs, graph_ptr(sizes), w, b, lo.EPS, residual=rs, return_stats=True)
    y.backward(gy.to(DEV))
    out = dict(y=y.detach(), stats=stats.detach(), d_x=xs.grad, d_weight=None if w is None else w.grad, d_bias=None if b is None else b.grad)
    if rs is not None:
        out["d_residual"] = rs.grad
    return out


# ---- 1. the kernels against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("name", list(lo.CASES))
def test_kernels_against_the_oracle(E, name, residual):
    (x, r, weight, bias, gy), r64, r32 = lo.reference(name, residual)
    sizes, C, _, constant = lo.CASES[name]
    got = run_op(E, x, sizes, weight, bias, gy, r if residual else None)
    for key in KEYS:
        e, e32 = rel(got[key], r64[key]), rel(r32[key], r64[key])
        bound = max(BOUND, 4.0 * e32)
        print("%-28s %-9s %-9s kernel %.3g   torch fp32 on the CPU %.3g   bound %.3g" % (name, "residual" if residual else "plain", key, e, e32, bound))
        assert e <= bound, "%s %s: %.3g of the largest value, bound %g (torch fp32: %.3g)" % (name, key, e, bound, e32)
    for g, n in enumerate(sizes):
        if n == 0:
            assert not bool(got["stats"][g].any()), "an empty graph: stats (0, 0)"
    if residual:
        assert torch.equal(got["d_x"], got["d_residual"]), "d_x is the residual's gradient"
    if constant is not None:                                   # var = 0: c is exactly zero, y the bias
        o, n = sum(sizes[:constant]), sizes[constant]
        assert torch.equal(got["y"][o:o + n].cpu(), bias.expand(n, C))
        assert float(got["stats"][constant, 0]) == lo.CONSTANT, "every partial sum of the constant is exact: so is the mean"


def test_without_an_affine(E):
    (x, r, _, _, gy), _, _ = lo.reference("ragged-12")
    sizes = lo.CASES["ragged-12"][0]
    got = run_op(E, x, sizes, None, None, gy, r)
    xs = x.double().requires_grad_(True)
    want = lo.segment_layer_norm(xs, sizes, residual=r.double())
    want.backward(gy.double())
    assert rel(got["y"], want) <= BOUND and rel(got["d_x"], xs.grad) <= BOUND and got["d_weight"] is None
    ones = run_op(E, x, sizes, torch.ones(12), torch.zeros(12), gy, r)
    assert torch.equal(ones["y"], got["y"]) and torch.equal(ones["d_x"], got["d_x"]), "weight 1, bias 0: the same bits"


# ---- 2. the residual, slices, bit stability -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ragged-12", "ragged-64", "ragged-300", "one-graph-260x64", "offset-100-64"])
def test_folded_residual_is_bit_equal_to_an_add_beforehand(E, name):
    (x, r, weight, bias, gy), _, _ = lo.reference(name)
    sizes = lo.CASES[name][0]
    folded = run_op(E, x, sizes, weight, bias, gy, r)
    before = run_op(E, (x.to(DEV) + r.to(DEV)), sizes, weight, bias, gy)
    for key in KEYS:
        assert torch.equal(folded[key], before[key]), key
    assert torch.equal(folded["d_residual"], before["d_x"])


@pytest.mark.parametrize("C", [12, 64, 300])
def test_column_slices_are_read_and_written_in_place(E, C):
    """the op on column slices of wider rows (x, residual and the upstream gradient), and the entry points with every leading
    dimension - y's and d_x's too - above C: the same bits as on contiguous operands"""
    from esc_gnn_amd import _native as nv
    name = "ragged-%d" % C
    (x, r, weight, bias, gy), _, _ = lo.reference(name)
    sizes = lo.CASES[name][0]
    N, G = x.size(0), len(sizes)
    want = run_op(E, x, sizes, weight, bias, gy, r)

    def wide(t, pad):
        buf = torch.full((N, C + 2 * pad), FILL, device=DEV)
        buf[:, pad:pad + C] = t.to(DEV)
        return buf, buf[:, pad:pad + C]

    (_, xs), (_, rs), (_, gs) = wide(x, 4), wide(r, 8), wide(gy, 12)
    xs.requires_grad_(True)
    w, b = weight.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    y, stats = E.ops.graph_layer_norm(xs, graph_ptr(sizes), w, b, lo.EPS, residual=rs, return_stats=True)
    y.backward(gs)
    for key, t in (("y", y.detach()), ("stats", stats), ("d_x", xs.grad), ("d_weight", w.grad), ("d_bias", b.grad)):
        assert torch.equal(t, want[key]), key
    # the entry points themselves, outputs as slices as well
    (ybuf, ys), (dbuf, ds) = wide(torch.zeros(N, C), 4), wide(torch.zeros(N, C), 16)
    ybuf.fill_(FILL)
    dbuf.fill_(FILL)
    st, gp = torch.full((G, 2), FILL, device=DEV), graph_ptr(sizes)
    dw, db, partial = (torch.full(s, FILL, device=DEV) for s in ((C,), (C,), (G, 2, C)))
    xs, wd, bd = xs.detach(), w.detach(), b.detach()
    nv.call("esc_graph_layer_norm_fwd", xs.data_ptr(), xs.stride(0), rs.data_ptr(), rs.stride(0), gp.data_ptr(), G, N, C, wd.data_ptr(), bd.data_ptr(),
            lo.EPS, ys.data_ptr(), ys.stride(0), st.data_ptr(), nv.stream())
    nv.call("esc_graph_layer_norm_bwd", xs.data_ptr(), xs.stride(0), rs.data_ptr(), rs.stride(0), st.data_ptr(), gs.data_ptr(), gs.stride(0), gp.data_ptr(),
            G, N, C, wd.data_ptr(), ds.data_ptr(), ds.stride(0), dw.data_ptr(), db.data_ptr(), partial.data_ptr(), nv.stream())
    assert torch.equal(ys, want["y"]) and torch.equal(st, want["stats"]) and torch.equal(ds, want["d_x"])
    assert torch.equal(dw, want["d_weight"]) and torch.equal(db, want["d_bias"])
    for buf, pad in ((ybuf, 4), (dbuf, 16)):                   # the columns beside the slice are left alone
        assert bool((buf[:, :pad] == FILL).all()) and bool((buf[:, pad + C:] == FILL).all())


@pytest.mark.parametrize("name", ["ragged-64", "ragged-300", "130-one-node-graphs-12", "one-graph-260x64"])
def test_two_runs_give_equal_bits(E, name):
    (x, r, weight, bias, gy), _, _ = lo.reference(name)
    sizes = lo.CASES[name][0]
    a, b = run_op(E, x, sizes, weight, bias, gy, r), run_op(E, x, sizes, weight, bias, gy, r)
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("C,n", [(4, 37), (12, 37), (64, 37), (64, 100), (128, 37), (300, 37), (300, 70)])
def test_a_graph_has_the_same_bits_alone_and_inside_two_batches(E, C, n):
    gen = torch.Generator().manual_seed(1000 * C + n)
    mine, g_mine = torch.randn((n, C), generator=gen), torch.randn((n, C), generator=gen)
    weight, bias = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    res = []
    for before, after in (([], []), ([23, 1, 30, 0, 9], [2]), ([260], [1, 0])):
        sizes = before + [n] + after
        parts = [torch.randn((sum(before), C), generator=gen), mine, torch.randn((sum(after), C), generator=gen)]
        grads = [torch.randn((sum(before), C), generator=gen), g_mine, torch.randn((sum(after), C), generator=gen)]
        out = run_op(E, torch.cat(parts, 0), sizes, weight, bias, torch.cat(grads, 0))
        o = sum(before)
        res.append((out["y"][o:o + n], out["stats"][len(before)], out["d_x"][o:o + n]))
    for other in res[1:]:
        for a, b, key in zip(res[0], other, ("y", "stats", "d_x")):
            assert torch.equal(a, b), key


# ---- 3. the skip contract -----------------------------------------------------------------------------------------------------------
def _raw(E, x, gy, ptr, G, N, C, weight, bias):
    """both entry points over sentinel-filled outputs: y, stats, d_x, partial, d_weight, d_bias"""
    from esc_gnn_amd import _native as nv
    rows = x.size(0)
    y, d_x = torch.full((rows, C), FILL, device=DEV), torch.full((rows, C), FILL, device=DEV)
    stats, partial = torch.full((max(G, 1), 2), FILL, device=DEV), torch.full((max(G, 1), 2, C), FILL, device=DEV)
    dw, db = torch.full((C,), FILL, device=DEV), torch.full((C,), FILL, device=DEV)
    gp = torch.tensor(ptr, dtype=torch.int32, device=DEV)
    nv.call("esc_graph_layer_norm_fwd", x.data_ptr(), C, None, C, gp.data_ptr(), G, N, C, weight.data_ptr(), bias.data_ptr(), lo.EPS, y.data_ptr(), C,
            stats.data_ptr(), nv.stream())
    nv.call("esc_graph_layer_norm_bwd", x.data_ptr(), C, None, C, stats.data_ptr(), gy.data_ptr(), C, gp.data_ptr(), G, N, C, weight.data_ptr(),
            d_x.data_ptr(), C, dw.data_ptr(), db.data_ptr(), partial.data_ptr(), nv.stream())
    torch.cuda.synchronize()
    return dict(y=y, stats=stats, d_x=d_x, partial=partial, d_weight=dw, d_bias=db)


def test_skip_contract_clause_by_clause(E):
    C, N = 8, 20
    gen = torch.Generator().manual_seed(5)
    x, gy = torch.randn((N, C), generator=gen).to(DEV), torch.randn((N, C), generator=gen).to(DEV)
    weight, bias = (torch.rand(C, generator=gen) + 0.5).to(DEV), torch.randn(C, generator=gen).to(DEV)
    clean = run_op(E, x[:9], [4, 0, 5], weight, bias, gy[:9])

    def untouched(t):
        return bool((t == FILL).all())

    # graph 1 is empty, graph 3's range is unordered, graph 4's leaves [0, N]: rows 0..8 are graphs 0 and 2, nothing else is written
    got = _raw(E, x, gy, [0, 4, 4, 9, 7, 25], 5, N, C, weight, bias)
    for key in ("y", "d_x"):
        assert torch.equal(got[key][:9], clean[key]) and untouched(got[key][9:]), key
    assert torch.equal(got["stats"][:3], clean["stats"]) and not bool(got["stats"][1].any()), "an empty graph: stats (0, 0)"
    assert untouched(got["stats"][3:]), "a skipped graph's stats stay unwritten"
    assert not bool(got["partial"][[1, 3, 4]].any()), "empty and skipped graphs: a zero partial"
    assert bool(got["partial"][0].any()) and bool(got["partial"][2].any())
    assert torch.equal(got["d_weight"], clean["d_weight"]) and torch.equal(got["d_bias"], clean["d_bias"])
    # a range that starts below 0
    got = _raw(E, x, gy, [-3, 4, 9], 2, N, C, weight, bias)
    assert untouched(got["y"][:4]) and untouched(got["y"][9:]) and untouched(got["d_x"][:4]) and untouched(got["stats"][0])
    assert torch.equal(got["y"][4:9], clean["y"][4:]) and torch.equal(got["d_x"][4:9], clean["d_x"][4:])
    assert not bool(got["partial"][0].any())
    # G == 0 and N == 0: nothing but d_weight and d_bias, which become zeros
    for ptr, G, n_rows in (([0], 0, N), ([0, 0, 0, 0], 3, 0)):
        got = _raw(E, x, gy, ptr, G, n_rows, C, weight, bias)
        assert all(untouched(got[k]) for k in ("y", "stats", "d_x", "partial")), (G, n_rows)
        assert not bool(got["d_weight"].any()) and not bool(got["d_bias"].any())
    # the op on a batch without rows and on no graphs
    empty = run_op(E, x[:0], [0, 0], weight, bias, gy[:0])
    assert empty["y"].shape == (0, C) and not bool(empty["d_weight"].any()) and not bool(empty["d_bias"].any())


# ---- 4. the host limits -------------------------------------------------------------------------------------------------------------
def test_each_host_limit_raises_with_its_message(E):
    from esc_gnn_amd import _native as nv
    N, G = 6, 2
    buf = torch.zeros((N + 1) * 1100, device=DEV)
    gp, st = graph_ptr([2, 4]), torch.zeros((G, 2), device=DEV)
    p = buf.data_ptr()

    def fwd(C=8, ld_x=8, ld_r=8, ld_y=8, x=p, r=p, w=p, b=p, y=p, G=G, N=N):
        nv.call("esc_graph_layer_norm_fwd", x, ld_x, r, ld_r, gp.data_ptr(), G, N, C, w, b, lo.EPS, y, ld_y, st.data_ptr(), nv.stream())

    def bwd(C=8, ld_x=8, ld_g=8, ld_dx=8, g=p, w=p, dw=p, db=p, part=p, d_x=p):
        nv.call("esc_graph_layer_norm_bwd", p, ld_x, None, 8, st.data_ptr(), g, ld_g, gp.data_ptr(), G, N, C, w, d_x, ld_dx, dw, db, part, nv.stream())

    width = r"the width must be a multiple of 4 with 4 <= C <= 1024 \(esc_graph_layer_norm_max_channels\)"
    for C in (0, 6, 1028):
        with pytest.raises(RuntimeError, match=width):
            fwd(C=C, ld_x=1100, ld_r=1100, ld_y=1100)
        with pytest.raises(RuntimeError, match=width):
            bwd(C=C, ld_x=1100, ld_g=1100, ld_dx=1100)
    for kw, name in ((dict(ld_x=4), "ld_x=4"), (dict(ld_r=10), "ld_r=10"), (dict(ld_y=4), "ld_y=4")):
        with pytest.raises(RuntimeError, match=r"leading dimension %s: every leading dimension must be >= C=8 and a multiple of 4" % name):
            fwd(**kw)
    for kw, name in ((dict(ld_g=6), "ld_g=6"), (dict(ld_dx=4), "ld_dx=4"), (dict(ld_x=9), "ld_x=9")):
        with pytest.raises(RuntimeError, match=r"leading dimension %s: every leading dimension must be >= C=8 and a multiple of 4" % name):
            bwd(**kw)
    for kw in (dict(x=p + 4), dict(r=p + 8), dict(w=p + 4), dict(b=p + 12), dict(y=p + 4)):
        with pytest.raises(RuntimeError, match="esc_graph_layer_norm_fwd: every pointer must be 16-byte aligned"):
            fwd(**kw)
    for kw in (dict(g=p + 4), dict(d_x=p + 8), dict(dw=p + 4), dict(db=p + 4), dict(part=p + 4)):
        with pytest.raises(RuntimeError, match="esc_graph_layer_norm_bwd: every pointer must be 16-byte aligned"):
            bwd(**kw)
    with pytest.raises(RuntimeError, match="bad sizes"):
        fwd(N=(1 << 31) // 64)
    with pytest.raises(RuntimeError, match="bad sizes"):
        fwd(G=(1 << 31) - 1)
    with pytest.raises(RuntimeError, match="weight and bias come together"):
        fwd(b=None)
    with pytest.raises(RuntimeError, match="weight, d_weight, d_bias and partial come together"):
        bwd(dw=None)
    # the op refuses a width before the library is asked, and operands that do not fit
    x = torch.zeros((N, 8), device=DEV)
    for C in (6, 1028):
        with pytest.raises(ValueError, match="graph_layer_norm: width %d: the kernels take a multiple of 4 with 4 <= C <= 1024" % C):
            E.ops.graph_layer_norm(torch.zeros((N, C), device=DEV), gp, None, None)
    with pytest.raises(ValueError, match="come together"):
        E.ops.graph_layer_norm(x, gp, torch.ones(8, device=DEV), None)
    with pytest.raises(ValueError, match="must have the shape of x"):
        E.ops.graph_layer_norm(x, gp, None, None, residual=torch.zeros((N, 12), device=DEV))
    with pytest.raises(TypeError, match="int32"):
        E.ops.graph_layer_norm(x, gp.long(), None, None)
    torch.cuda.synchronize()
    assert not bool(buf.any()) and not bool(st.any()), "a refused call launches nothing"


# ---- 5. the module ------------------------------------------------------------------------------------------------------------------
def test_graph_layer_norm_module_train_and_eval_give_equal_bits(E):
    (x, r, weight, bias, _), r64, _ = lo.reference("ragged-64", True)
    sizes = lo.CASES["ragged-64"][0]
    m = E.nn.GraphLayerNorm(64)
    m.load_state_dict(dict(weight=weight, bias=bias))
    m = m.to(DEV)
    gp = graph_ptr(sizes)
    a = m.train()(x.to(DEV), gp, residual=r.to(DEV))
    b = m.eval()(x.to(DEV), gp, residual=r.to(DEV))
    with torch.no_grad():
        c = m(x.to(DEV), gp, residual=r.to(DEV))
    assert torch.equal(a, b) and torch.equal(a, c) and rel(a, r64["y"]) <= BOUND
    assert list(m.state_dict()) == ["weight", "bias"]


# ---- 6. the model -------------------------------------------------------------------------------------------------------------------
_MOLS = {}


def molecules(E):
    if not _MOLS:
        from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
        graphs = build_feature_dataset(synthetic_zinc_graphs(0, 6), 3, use_rd=True, self_loop=True)
        batch = E.Batch.from_data_list([g for g in graphs])
        _MOLS["cpu"] = {k: batch[k].cpu() for k in ("x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
        _MOLS["graphs"] = graphs
    return _MOLS


def _close(a, b, what, tol):
    """the measure of tests/test_hip_gps.py's model test: max error over max(1, largest value)"""
    a, b = a.detach().cpu().double(), b.detach().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    print("%-64s max scaled error %.3g" % (what, err))
    assert a.shape == b.shape and err <= tol, "%s: max scaled error %.3g > %g" % (what, err, tol)


def _model_against_the_oracle(E, what, **kw):
    from esc_gnn_amd.gps_models import GPSModel
    mol = molecules(E)
    torch.manual_seed(7)
    oracle = lo.GPSModel(layers=2, dim_hidden=16, n_heads=2, **kw)
    for m in oracle.modules():                                 # weights that make every term count: every affine and bias off its default
        if isinstance(m, (torch.nn.BatchNorm1d, lo.LayerNorm)):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, std=0.1)
        if isinstance(m, torch.nn.MultiheadAttention):
            torch.nn.init.normal_(m.in_proj_bias, std=0.1)
            torch.nn.init.normal_(m.out_proj.bias, std=0.1)
    mine = GPSModel(layers=2, dim_hidden=16, n_heads=2, dropout=0.0, attn_dropout=0.0, **kw)
    mine.load_state_dict(oracle.state_dict())
    mine = mine.to(DEV)
    oracle = copy.deepcopy(oracle).double()
    y = torch.tensor([0.3, -1.1, 0.7, 0.2, -0.4, 0.9], dtype=torch.float64).view(-1, 1)
    for mode in ("train", "eval"):
        getattr(oracle, mode)()
        getattr(mine, mode)()
        oracle.zero_grad()
        mine.zero_grad()
        want = oracle(mol["cpu"])
        (want - y).abs().mean().backward()
        got = mine(E.Batch.from_data_list([g for g in mol["graphs"]]).to(DEV))
        E.ops.l1_loss(got, y.float().to(DEV)).backward()
        _close(got, want, "%s %s prediction" % (what, mode), 1e-5)
        ref_p, ref_b = dict(oracle.named_parameters()), dict(oracle.named_buffers())
        unused = []
        for n, p in mine.named_parameters():
            if ref_p[n].grad is None:                          # edge_attn_*: never in the forward; norm1_attn: not without attention
                assert p.grad is None, n
                unused.append(n)
                continue
            assert p.grad is not None, n
            _close(p.grad, ref_p[n].grad, "%s %s grad %s" % (what, mode, n), 1e-4)
        # ... and the last GatedGCN layer's edge branch: nothing reads the edge attributes it returns
        assert all("edge_attn" in n or (".norm1_attn." in n and kw.get("global_model_type") == "None")
                   or (n.startswith("layers.1.local_model.") and kw.get("local_gnn_type") == "CustomGatedGCN") for n in unused), unused
        assert not any(".norm1_local." in n or ".norm2." in n for n in unused)
        for n, b in mine.named_buffers():
            _close(b, ref_b[n], "%s %s buffer %s" % (what, mode, n), 1e-4)
    return mine


@pytest.mark.parametrize("global_model_type", ["Transformer", "None"])
@pytest.mark.parametrize("local_gnn_type", ["GINE", "CustomGatedGCN", "PNA"])
def test_layer_norm_model_against_the_oracle_model(E, local_gnn_type, global_model_type):
    mine = _model_against_the_oracle(E, "%s+%s layer_norm" % (local_gnn_type, global_model_type), local_gnn_type=local_gnn_type,
                                     global_model_type=global_model_type, layer_norm=True, batch_norm=False)
    assert all(isinstance(getattr(layer, n), E.nn.GraphLayerNorm) for layer in mine.layers for n in ("norm1_local", "norm1_attn", "norm2"))
    assert any(p.grad is not None and bool(p.grad.any()) for n, p in mine.named_parameters() if n.endswith("norm2.weight"))


@pytest.mark.parametrize("local_gnn_type,global_model_type", [("GINE", "Transformer"), ("CustomGatedGCN", "None")])
def test_model_without_norms_against_the_oracle_model(E, local_gnn_type, global_model_type):
    _model_against_the_oracle(E, "%s+%s no norm" % (local_gnn_type, global_model_type), local_gnn_type=local_gnn_type,
                              global_model_type=global_model_type, layer_norm=False, batch_norm=False)


def test_layer_norm_model_gives_a_graph_the_same_prediction_alone_and_in_a_batch(E):
    """what the norm is for: in evaluation nothing in the model looks across graphs any more"""
    from esc_gnn_amd.gps_models import GPSModel
    mol = molecules(E)
    torch.manual_seed(3)
    model = GPSModel(layers=2, dim_hidden=16, n_heads=2, dropout=0.0, attn_dropout=0.0, layer_norm=True, batch_norm=False).to(DEV).eval()
    with torch.no_grad():
        whole = model(E.Batch.from_data_list([g for g in mol["graphs"]]).to(DEV))
        alone = model(E.Batch.from_data_list([mol["graphs"][2]]).to(DEV))
    _close(alone[0], whole[2].cpu(), "graph 2 alone against inside the batch", 1e-5)


# ---- 7. the driver ------------------------------------------------------------------------------------------------------------------
def test_driver_trains_with_layer_norm(tmp_path, monkeypatch):
    require_gpu()
    import esc_gnn_amd.run_zinc_gps as rg
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rg.main("--gt_layer_norm 1 --gt_batch_norm 0 --synthetic_graphs 12 --epochs 1 --layers 2 --batch_size 4 --num_warmup_epochs 1 "
                "--save_appendix _ln".split())
    out = buf.getvalue()
    lines = re.findall(r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)", out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    keys = list(torch.load(tmp_path / "results" / "zinc_GPS_ln" / "model_checkpoint1.pth", map_location="cpu"))
    assert "layers.0.norm1_local.weight" in keys and "layers.1.norm2.bias" in keys
    assert not any(".norm" in k and "running" in k for k in keys)
    assert os.path.exists(tmp_path / "results" / "zinc_GPS_ln" / "log.txt")
