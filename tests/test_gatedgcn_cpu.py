"""The GatedGCN local layer without a GPU: the binding of include/escgnn_gatedgcn.h, the oracle (tests/gatedgcn_oracle.py) against
closed forms and torch.autograd.gradcheck, the conditioning of every case tests/test_hip_gatedgcn.py asserts, the state_dict
layouts, the construction order, the driver's --gt_layer_type and the documented ValueErrors."""
import ctypes
import os

import pytest
import torch

import gatedgcn_oracle as gg
import gps_cases as gc
import gps_oracle as go
from conftest import GOLDEN


def test_header_declares_the_entry_points_and_the_binding_holds_exactly_them():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.GATEDGCN_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    want = {
        "esc_gated_gcn_max_channels": ([], i64),
        "esc_gated_gcn_fwd": ([p, i64] * 5 + [p, p, p, i64, i64, i64, p, i64, p, i64, p, p], i),
        "esc_gated_gcn_bwd": ([p, i64] * 3 + [p] + [p, i64] * 3 + [p] * 6 + [i64] * 3 + [p, i64] * 4 + [p], i),
    }
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.GATEDGCN_SIGNATURES) == set(want)
    others = (nv.SIGNATURES, nv.EXTENSION_SIGNATURES, nv.I2GNN_SIGNATURES, nv.GINEPLUS_SIGNATURES, nv.GPS_SIGNATURES,
              nv.LAPPE_SIGNATURES, nv.RWSE_SIGNATURES, nv.STEP_SIGNATURES)
    assert not any(set(want) & set(o) for o in others)


# ---- the oracle against closed forms ------------------------------------------------------------------------------------------------
def _rand(*shape, seed=0):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def test_one_edge_closed_form():
    Ax, Bx, Dx, Ex, Ce = [_rand(2, 4, seed=s) for s in range(4)] + [_rand(1, 4, seed=9)]
    out, e, den = gg.gate(Ax, Bx, Dx, Ex, Ce, torch.tensor([0]), torch.tensor([1]))
    s = torch.sigmoid(Dx[1] + Ex[0] + Ce[0])
    assert torch.equal(e[0], Dx[1] + Ex[0] + Ce[0]) and torch.equal(den[1], s)
    assert torch.allclose(out[1], Ax[1] + s * Bx[0] / (s + 1e-6), rtol=0, atol=1e-15)
    assert torch.equal(out[0], Ax[0]) and torch.equal(den[0], torch.zeros(4, dtype=torch.float64))


def test_equal_gates_give_the_mean_of_the_neighbours():
    """Dx, Ex, Ce constant per column -> every in-edge of a node has the same gate: aggr = mean(Bx_j) * den / (den + 1e-6)"""
    n, src, dst = gg.edges_of("molecule-30")
    Ax, Bx = _rand(n, 4, seed=1), _rand(n, 4, seed=2)
    col = _rand(1, 4, seed=3)
    out, _, den = gg.gate(Ax, Bx, col.expand(n, 4), col.expand(n, 4), col.expand(src.numel(), 4), src, dst)
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, torch.ones(src.numel(), dtype=torch.float64))
    mean = torch.zeros_like(Bx).index_add_(0, dst, Bx[src]) / deg.view(-1, 1)
    assert float((out - Ax - mean * den / (den + 1e-6)).abs().max()) <= 1e-14


def test_an_isolated_node_keeps_ax_and_gets_no_gradient():
    n, src, dst = gg.edges_of("star-in-300")            # nodes 308 and 309 touch no edge
    x = [_rand(n, 4, seed=s).requires_grad_(True) for s in range(4)] + [_rand(src.numel(), 4, seed=5).requires_grad_(True)]
    out, e, _ = gg.gate(*x, src, dst)
    assert torch.equal(out[308:], x[0][308:].detach())
    (out.sum() + e.sum()).backward()
    for t in x[1:4]:
        assert torch.equal(t.grad[308:], torch.zeros(2, 4, dtype=torch.float64))
    assert torch.equal(x[0].grad, torch.ones(n, 4, dtype=torch.float64))


def test_oracle_agrees_with_gradcheck():
    """5 nodes, a self-loop (2 -> 2) and a repeated edge (0 -> 1 twice)"""
    src, dst = torch.tensor([0, 0, 2, 3, 4, 1, 1]), torch.tensor([1, 1, 2, 2, 3, 4, 0])
    x = [_rand(5, 3, seed=s).requires_grad_(True) for s in range(4)] + [_rand(7, 3, seed=7).requires_grad_(True)]
    assert torch.autograd.gradcheck(lambda *t: gg.gate(*t, src, dst), x, eps=1e-6, atol=1e-7)


# ---- conditioning of what the GPU tests assert -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", gg.WIDTHS + (gg.LADDER_WIDTH,))
def test_every_asserted_case_is_within_the_conditioning_cap(C):
    worst = 0.0
    for name in (list(gg.CASES) + list(gg.LADDER) if C in gg.WIDTHS else ["degree-ladder", "molecule-30"]):
        for with_ge in (True, False):
            ref = gg.reference(name, C, with_ge)
            for k, want in ref[torch.float64].items():
                floor = gg.scale_floor(name, C, with_ge, k)          # 0 except for the cancelling cases' edge gradients without g_e
                e = gg.rel(ref[torch.float32][k], want, floor)
                assert floor > 0 or e == gc.rel(ref[torch.float32][k], want)
                worst = max(worst, e)
                assert e <= gc.CAP, "%s C=%d %s: the oracle's fp32 is %.3g from its fp64, cap %g" % (name, C, k, e, gc.CAP)
    print("C=%d: worst fp32-vs-fp64 figure of the oracle %.3g (cap %g)" % (C, worst, gc.CAP))


def test_the_saturated_case_reaches_gates_of_40_and_is_conditioned_forward():
    ref = gg.reference("batch", 64, False, gg_scale())
    assert float(ref[torch.float64]["e_out"].abs().max()) >= 40.0
    for k in ("out", "e_out", "den"):
        assert gc.rel(ref[torch.float32][k], ref[torch.float64][k]) <= gc.CAP, k


def gg_scale():
    return 12.0


# ---- layouts, construction order, driver ---------------------------------------------------------------------------------------------
def _golden_keys():
    with open(os.path.join(GOLDEN, "gps_gatedgcn_state_keys.txt")) as fh:
        return [line.strip() for line in fh if line.strip()]


@pytest.mark.parametrize("global_model_type", ["Transformer", "None"])
def test_state_dict_keys_are_the_reference_layout(global_model_type):
    """the golden list is a one-layer CustomGatedGCN+Transformer model, written down from the reference classes; with the global
    model None the self_attn keys are absent and nothing else moves"""
    from esc_gnn_amd.gps_models import GPSModel
    want = [k for k in _golden_keys() if global_model_type == "Transformer" or ".self_attn." not in k]
    mine = GPSModel(layers=1, dim_hidden=16, n_heads=2, local_gnn_type="CustomGatedGCN", global_model_type=global_model_type)
    assert list(mine.state_dict().keys()) == want
    oracle = gg.GPSModel(layers=1, dim_hidden=16, n_heads=2, local_gnn_type="CustomGatedGCN", global_model_type=global_model_type)
    assert [(k, tuple(v.shape)) for k, v in mine.state_dict().items()] == [(k, tuple(v.shape)) for k, v in oracle.state_dict().items()]
    mine.load_state_dict(oracle.state_dict())


def test_default_model_keeps_todays_layout():
    from esc_gnn_amd.gps_models import GPSModel
    mine = GPSModel(layers=2, attn_dropout=0.0).state_dict()
    want = go.GPSModel(layers=2).state_dict()
    assert [(k, tuple(v.shape), v.dtype) for k, v in mine.items()] == [(k, tuple(v.shape), v.dtype) for k, v in want.items()]
    spelled = GPSModel(layers=2, attn_dropout=0.0, local_gnn_type="GINE", global_model_type="Transformer").state_dict()
    assert list(spelled) == list(mine)


def test_equal_seeds_give_equal_weights():
    from esc_gnn_amd.gps_models import GPSModel
    kw = dict(layers=2, dim_hidden=16, n_heads=2, local_gnn_type="CustomGatedGCN")
    torch.manual_seed(5)
    a = GPSModel(**kw).state_dict()
    torch.manual_seed(5)
    b = GPSModel(**kw).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    torch.manual_seed(5)                                 # ... and the layer draws A, B, C, D, E in the reference's order
    from esc_gnn_amd.nn import GatedGCNLayer
    mine = GatedGCNLayer(8, 8, 0.0, True).state_dict()
    torch.manual_seed(5)
    ref = gg.GatedGCNLayer(8, 8).state_dict()
    assert list(mine) == list(ref) and all(torch.equal(mine[k], ref[k]) for k in ref)


def test_driver_accepts_four_layer_types_and_refuses_a_fifth():
    from esc_gnn_amd import run_zinc_gps as rg
    assert build_default(rg) == "GINE+Transformer"
    want = {"GINE+Transformer": ("GINE", "Transformer"), "CustomGatedGCN+Transformer": ("CustomGatedGCN", "Transformer"),
            "GINE+None": ("GINE", "None"), "CustomGatedGCN+None": ("CustomGatedGCN", "None")}
    for name, halves in want.items():
        a = rg.build_parser().parse_args(["--gt_layer_type", name])
        assert rg.layer_type_of(a.gt_layer_type) == halves
    for bad in ("GINE+Performer", "GatedGCN+Transformer", "GINE"):
        with pytest.raises(SystemExit) as exc:
            rg.main(["--gt_layer_type", bad, "--synthetic_graphs", "12"])
        assert all(name in str(exc.value) for name in want), str(exc.value)


def build_default(rg):
    return rg.build_parser().parse_args([]).gt_layer_type


def test_documented_value_errors():
    from esc_gnn_amd.gps_models import GPSLayer, GPSModel
    from esc_gnn_amd.nn import GatedGCNLayer
    with pytest.raises(ValueError, match="equivstable_pe"):
        GatedGCNLayer(8, 8, 0.0, True, equivstable_pe=True)
    with pytest.raises(ValueError, match="relu"):
        GatedGCNLayer(8, 8, 0.0, True, act="gelu")
    with pytest.raises(ValueError, match="in_dim == out_dim"):
        GatedGCNLayer(8, 12, 0.0, True)
    GatedGCNLayer(8, 12, 0.0, False)
    with pytest.raises(ValueError, match="Unsupported local GNN model: GAT"):
        GPSLayer(16, 2, local_gnn_type="GAT")
    with pytest.raises(ValueError, match="Unsupported global x-former model: Performer"):
        GPSModel(layers=1, dim_hidden=16, n_heads=2, global_model_type="Performer")
    none = GPSLayer(16, 2, local_gnn_type="CustomGatedGCN", global_model_type="None")
    assert none.self_attn is None and isinstance(none.norm1_attn, torch.nn.BatchNorm1d)


def test_a_checkpoint_of_one_layout_is_refused_by_another():
    from esc_gnn_amd.gps_models import GPSModel
    gated = GPSModel(layers=1, dim_hidden=16, n_heads=2, local_gnn_type="CustomGatedGCN")
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        GPSModel(layers=1, dim_hidden=16, n_heads=2).load_state_dict(gated.state_dict())
    with pytest.raises(RuntimeError, match="Unexpected key"):
        GPSModel(layers=1, dim_hidden=16, n_heads=2, local_gnn_type="CustomGatedGCN", global_model_type="None").load_state_dict(gated.state_dict())
