"""The per-graph LayerNorm without a GPU: the segment form of tests/layernorm_oracle.py (what include/escgnn_layernorm.h states)
against the PyG form spelled out in torch ops and against torch.nn.functional.layer_norm over each graph's flattened block
(fp64, 1e-12: outputs and all four gradients), the binding of the header, and the model's and the driver's two switches:
state_dict layouts, the refusals, the parser defaults."""
import ctypes
import os

import pytest
import torch

import layernorm_oracle as lo

TOL = 1e-12                      # tests/test_gps_cpu.py's fp64 tolerance
F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = [23, 1, 30, 9, 37, 2]    # no empty graph here: PyG's batch vector cannot name one in the middle without batch_size


def _inputs(sizes, C, seed, offset=0.0):
    gen = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    x = (torch.randn((N, C), generator=gen, dtype=F64) + offset).requires_grad_(True)
    r = torch.randn((N, C), generator=gen, dtype=F64).requires_grad_(True)
    w = (torch.rand(C, generator=gen, dtype=F64) + 0.5).requires_grad_(True)
    b = torch.randn(C, generator=gen, dtype=F64).requires_grad_(True)
    gy = torch.randn((N, C), generator=gen, dtype=F64)
    return x, r, w, b, gy


def _grads(y, gy, leaves):
    for t in leaves:
        t.grad = None
    y.backward(gy)
    return [t.grad.clone() for t in leaves]


def _same(a, b, what):
    err = float((a - b).abs().max()) / max(1.0, float(b.abs().max())) if b.numel() else 0.0
    assert a.shape == b.shape and err <= TOL, "%s: %.3g" % (what, err)


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def _want():
    p, i64, i, f = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float
    return {
        "esc_graph_layer_norm_max_channels": ([], i64),
        "esc_graph_layer_norm_fwd": ([p, i64, p, i64, p, i64, i64, i64, p, p, f, p, i64, p, p], i),
        "esc_graph_layer_norm_bwd": ([p, i64, p, i64, p, p, i64, p, i64, i64, i64, p, p, i64, p, p, p, p], i),
    }


def test_header_declares_exactly_the_three_entry_points():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.LAYERNORM_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    want = _want()
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.LAYERNORM_SIGNATURES) == set(want)
    others = (nv.SIGNATURES, nv.EXTENSION_SIGNATURES, nv.I2GNN_SIGNATURES, nv.GINEPLUS_SIGNATURES, nv.GPS_SIGNATURES, nv.LAPPE_SIGNATURES,
              nv.RWSE_SIGNATURES, nv.STEP_SIGNATURES, nv.GATEDGCN_SIGNATURES, nv.PNA_SIGNATURES, nv.SPD_SIGNATURES)
    assert not any(set(want) & set(o) for o in others)
    assert nv.ABI_VERSION == nv.const("ESC_ABI_VERSION")


def test_every_declared_symbol_is_exported_and_the_width_limit_is_1024():
    from esc_gnn_amd import _native as nv
    h = ctypes.CDLL(nv.LIB_PATH)
    for name in _want():
        assert hasattr(h, name), name
    h.esc_graph_layer_norm_max_channels.restype = ctypes.c_int64
    assert h.esc_graph_layer_norm_max_channels() == 1024


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 12, 64, 300])
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "residual"])
def test_segment_form_equals_the_pyg_form(C, residual):
    x, r, w, b, gy = _inputs(SIZES, C, 3 + C)
    leaves = [x, r, w, b] if residual else [x, w, b]
    want = lo.pyg_layer_norm(x + r if residual else x, lo.batch_of(SIZES), w, b)
    g_want = _grads(want, gy, leaves)
    got = lo.segment_layer_norm(x, SIZES, w, b, residual=r if residual else None)
    g_got = _grads(got, gy, leaves)
    _same(got.detach(), want.detach(), "y")
    for name, a, c in zip(("d_x", "d_residual", "d_weight", "d_bias") if residual else ("d_x", "d_weight", "d_bias"), g_got, g_want):
        _same(a, c, name)
    if residual:
        assert torch.equal(g_got[0], g_got[1]), "the residual's gradient is d_x"


def test_an_empty_graph_in_the_middle_and_at_the_end():
    """PyG's form with batch_size given (an empty graph has degree 0, clamped to 1, and no rows): the same rows as without it"""
    sizes = [5, 0, 3, 0]
    x, _, w, b, _ = _inputs(sizes, 8, 9)
    batch = lo.batch_of(sizes)
    assert batch.tolist() == [0] * 5 + [2] * 3
    y, stats = lo.segment_layer_norm(x, sizes, w, b, return_stats=True)
    _same(y.detach(), lo.pyg_layer_norm(x, batch, w, b, batch_size=4).detach(), "y")
    assert stats.shape == (4, 2) and not stats[1].any() and not stats[3].any() and bool(stats[0, 1] > 0)


@pytest.mark.parametrize("offset", [0.0, 100.0])
def test_every_graph_equals_functional_layer_norm_over_its_flattened_block(offset):
    C = 12
    x, _, w, b, gy = _inputs(SIZES, C, 21, offset)
    got = lo.segment_layer_norm(x, SIZES, w, b)
    g_got = _grads(got, gy, [x, w, b])
    blocks, o = [], 0
    for n in SIZES:
        flat = torch.nn.functional.layer_norm(x[o:o + n].reshape(-1), (n * C,), eps=lo.EPS)
        blocks.append(flat.reshape(n, C) * w + b)              # the affine is per channel, applied afterwards
        o += n
    want = torch.cat(blocks, 0)
    g_want = _grads(want, gy, [x, w, b])
    _same(got.detach(), want.detach(), "y")
    for name, a, c in zip(("d_x", "d_weight", "d_bias"), g_got, g_want):
        _same(a, c, name)


def test_a_graph_has_the_same_output_alone_and_inside_a_batch():
    """what BatchNorm cannot say, and why the recipe uses this norm for inference one graph at a time"""
    x, _, w, b, _ = _inputs(SIZES, 8, 5)
    whole = lo.segment_layer_norm(x, SIZES, w, b).detach()
    o = sum(SIZES[:2])
    alone = lo.segment_layer_norm(x[o:o + SIZES[2]], [SIZES[2]], w, b).detach()
    assert torch.equal(whole[o:o + SIZES[2]], alone)


def test_the_one_pass_variance_fails_where_the_centred_one_holds():
    """at 100 + randn in fp32, E[h^2] - mean^2 loses the variance to cancellation; the centred second pass keeps it: the reason
    the header insists on it, and the case tests/test_hip_layernorm.py holds the kernels to"""
    (x, _, w, b, _), r64, r32 = lo.reference("offset-100-64")
    sizes, C = lo.CASES["offset-100-64"][:2]
    top = float(r64["y"].abs().max())
    assert float((r32["y"].double() - r64["y"]).abs().max()) / top < 1e-5
    out, o = [], 0
    for n in sizes:
        rows = x[o:o + n]
        o += n
        if n:
            mean = rows.mean()
            var = (rows * rows).mean() - mean * mean
            out.append((rows - mean) / torch.sqrt(var + lo.EPS) * w + b)
    one_pass = torch.cat(out, 0)
    assert float((one_pass.double() - r64["y"]).abs().max()) / top > 1e-4


def test_the_constant_graph_of_the_gpu_cases_is_exact_in_every_summation_order():
    """1.5 x k is exact in fp32 for every k the case can form, so the mean is 1.5 whatever the order and y == bias"""
    sizes, C, _, which = lo.CASES["constant-graph-64"]
    assert sizes[which] * C * lo.CONSTANT < 2 ** 24 and (lo.CONSTANT * 2).is_integer()
    (x, r, w, b, _), r64, r32 = lo.reference("constant-graph-64", residual=True)
    o = sum(sizes[:which])
    assert torch.equal(r32["y"][o:o + sizes[which]], b.expand(sizes[which], C))
    assert torch.equal(r64["y"][o:o + sizes[which]], b.double().expand(sizes[which], C))


# ---- the model and the driver ---------------------------------------------------------------------------------------------------------
def _golden():
    with open(os.path.join(GOLDEN, "gps_layernorm_state_keys.txt")) as fh:
        lines = [line.strip() for line in fh if line.strip()]
    assert lines[0].startswith("#") and "reading" in lines[0]
    return lines[1:]


def test_layer_norm_state_dict_keys_are_the_reference_layout():
    from esc_gnn_amd.gps_models import GPSModel
    kw = dict(layers=1, dim_hidden=16, n_heads=2, layer_norm=True, batch_norm=False)
    mine, oracle = GPSModel(**kw), lo.GPSModel(**kw)
    keys = list(mine.state_dict())
    assert keys == list(oracle.state_dict()) == _golden()
    assert {k: tuple(v.shape) for k, v in mine.state_dict().items()} == {k: tuple(v.shape) for k, v in oracle.state_dict().items()}
    norms = [k for k in keys if ".norm" in k]
    assert norms == ["layers.0.%s.%s" % (m, p) for m in ("norm1_local", "norm1_attn", "norm2") for p in ("weight", "bias")]
    sd = mine.state_dict()
    assert all(bool((sd[k] == (1.0 if k.endswith("weight") else 0.0)).all()) for k in norms)       # ones and zeros
    # GatedGCN's own BatchNorms and z_embedding's keep their running statistics
    gated = list(GPSModel(local_gnn_type="CustomGatedGCN", global_model_type="None", **kw).state_dict())
    assert gated == list(lo.GPSModel(local_gnn_type="CustomGatedGCN", global_model_type="None", **kw).state_dict())
    assert "layers.0.local_model.bn_node_x.running_mean" in gated and "layers.0.z_embedding.1.running_var" in gated
    assert "layers.0.norm1_attn.weight" in gated and not any(".norm" in k and "running" in k for k in gated)


@pytest.mark.parametrize("local_gnn_type", ["GINE", "CustomGatedGCN", "PNA"])
def test_without_norms_the_layer_has_no_norm_module(local_gnn_type):
    from esc_gnn_amd.gps_models import GPSModel
    kw = dict(layers=2, dim_hidden=16, n_heads=2, local_gnn_type=local_gnn_type, layer_norm=False, batch_norm=False)
    mine = GPSModel(**kw)
    keys = list(mine.state_dict())
    assert keys == list(lo.GPSModel(**kw).state_dict())
    assert not any(".norm" in k for k in keys)
    assert not any(hasattr(layer, n) for layer in mine.layers for n in ("norm1_local", "norm1_attn", "norm2"))


def test_the_defaults_are_the_batch_norm_layout():
    from esc_gnn_amd.gps_models import GPSModel
    from esc_gnn_amd.nn import BatchNorm1d, GraphLayerNorm
    kw = dict(layers=1, dim_hidden=16, n_heads=2)
    torch.manual_seed(3)
    a = GPSModel(**kw)
    torch.manual_seed(3)
    b = GPSModel(layer_norm=False, batch_norm=True, **kw)
    assert list(a.state_dict()) == list(b.state_dict()) == list(lo.GPSModel(**kw).state_dict())
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    assert isinstance(a.layers[0].norm2, BatchNorm1d) and "layers.0.norm2.running_mean" in a.state_dict()
    assert isinstance(GPSModel(layer_norm=True, batch_norm=False, **kw).layers[0].norm2, GraphLayerNorm)


def test_graph_layer_norm_module_has_pygs_parameters():
    from esc_gnn_amd.nn import GraphLayerNorm
    m = GraphLayerNorm(12)
    assert list(m.state_dict()) == ["weight", "bias"] == list(lo.LayerNorm(12).state_dict())
    assert bool((m.weight == 1).all()) and bool((m.bias == 0).all()) and m.eps == 1e-5
    assert list(GraphLayerNorm(12, affine=False).state_dict()) == []


def test_both_normalisations_together_are_refused():
    from esc_gnn_amd import run_zinc_gps as rg
    from esc_gnn_amd.gps_models import GPSLayer, GPSModel
    for make in (lambda: GPSLayer(16, 2, layer_norm=True, batch_norm=True), lambda: GPSModel(layers=1, dim_hidden=16, n_heads=2, layer_norm=True),
                 lambda: GPSModel(layers=0, dim_hidden=16, n_heads=2, layer_norm=True, batch_norm=True),
                 lambda: lo.GPSLayer(16, 2, layer_norm=True, batch_norm=True)):
        with pytest.raises(ValueError, match="^Cannot apply two types of normalization together$"):
            make()
    with pytest.raises(SystemExit) as exc:
        rg.main("--gt_layer_norm 1 --synthetic_graphs 12".split())
    assert "--gt_layer_norm" in str(exc.value) and "--gt_batch_norm" in str(exc.value)
    with pytest.raises(SystemExit) as exc:
        rg.main("--gt_layer_norm 1 --gt_batch_norm 1 --gt_layer_type PNA+None".split())
    assert "--gt_layer_norm" in str(exc.value) and "--gt_batch_norm" in str(exc.value)


def test_parser_defaults_and_the_flags_combine_with_every_layer_type():
    from esc_gnn_amd import run_zinc_gps as rg
    args = rg.build_parser().parse_args([])
    assert (args.gt_layer_norm, args.gt_batch_norm, args.gt_layer_type) == (0, 1, "GINE+Transformer")
    assert rg.norm_flags_of(args) == (False, True)
    for name in rg.LAYER_TYPES + rg.BIASED_LAYER_TYPES:
        args = rg.build_parser().parse_args(["--gt_layer_type", name, "--gt_layer_norm", "1", "--gt_batch_norm", "0"])
        assert rg.norm_flags_of(args) == (True, False) and rg.layer_type_of(args.gt_layer_type) == tuple(name.split("+"))
    assert rg.norm_flags_of(rg.build_parser().parse_args(["--gt_batch_norm", "0"])) == (False, False)
    with pytest.raises(SystemExit):
        rg.build_parser().parse_args(["--gt_layer_norm", "2"])


def test_a_checkpoint_of_one_normalisation_is_refused_by_the_others():
    from esc_gnn_amd.gps_models import GPSModel
    kw = dict(layers=1, dim_hidden=16, n_heads=2)
    models = [GPSModel(**kw), GPSModel(layer_norm=True, batch_norm=False, **kw), GPSModel(layer_norm=False, batch_norm=False, **kw)]
    for i, a in enumerate(models):
        for j, b in enumerate(models):
            if i != j:
                with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
                    b.load_state_dict(a.state_dict())
    models[1].load_state_dict(lo.GPSModel(layer_norm=True, batch_norm=False, **kw).state_dict())      # ... and the oracle's loads


def test_the_op_refuses_a_cpu_tensor():
    from esc_gnn_amd import ops
    gp = torch.tensor([0, 2], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.graph_layer_norm(torch.zeros(2, 8), gp, None, None)
