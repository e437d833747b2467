"""The PNA local layer without a GPU: the binding of include/escgnn_pna.h, the oracle (tests/pna_oracle.py) against closed forms
and torch.autograd.gradcheck, the conditioning of every case tests/test_hip_pna.py asserts (as a condition on the top-two gap of
the messages, not as a measurement), the state_dict layout, the construction order, the driver's two new --gt_layer_type names
and the documented ValueErrors."""
import ctypes
import os

import pytest
import torch

import gatedgcn_oracle as gg
import pna_oracle as po
from conftest import GOLDEN

F64, F32 = torch.float64, torch.float32
GAP = 1e-6            # of the case's largest |m|; a message is two fp32 additions: its rounding error is below 1.2e-7 of that


def test_header_declares_the_entry_points_and_the_binding_holds_exactly_them():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.PNA_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    want = {
        "esc_pna_max_channels": ([], i64),
        "esc_pna_aggregate_fwd": ([p, i64] * 3 + [p, p, p, i64, i64, i64, p, i64, p, p], i),
        "esc_pna_aggregate_bwd": ([p, i64, p] + [p] * 6 + [i64] * 3 + [p, i64] * 3 + [p], i),
    }
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.PNA_SIGNATURES) == set(want)
    others = (nv.SIGNATURES, nv.EXTENSION_SIGNATURES, nv.I2GNN_SIGNATURES, nv.GINEPLUS_SIGNATURES, nv.GPS_SIGNATURES,
              nv.LAPPE_SIGNATURES, nv.RWSE_SIGNATURES, nv.STEP_SIGNATURES, nv.GATEDGCN_SIGNATURES)
    assert not any(set(want) & set(o) for o in others)


# ---- the oracle against closed forms ------------------------------------------------------------------------------------------------
def _rand(*shape, seed=0):
    return torch.randn(shape, dtype=F64, generator=torch.Generator().manual_seed(seed))


def test_one_edge_closed_form():
    P, Q, R = _rand(2, 4, seed=1), _rand(2, 4, seed=2), _rand(1, 4, seed=3)
    agg, arg = po.aggregate(P, Q, R, torch.tensor([0]), torch.tensor([1]))
    m = P[1] + Q[0] + R[0]
    assert torch.equal(agg[1], torch.cat([m, m, m])) and torch.equal(arg[1], torch.zeros(4, dtype=torch.int64))
    assert torch.equal(agg[0], torch.zeros(12, dtype=F64)) and torch.equal(arg[0], torch.full((4,), -1))


def test_two_equal_messages_the_lower_edge_position_takes_the_whole_gradient():
    """the repeated edge 0 -> 1 with equal R rows: mean = max = m, sum = 2 m, arg = the first of the two, and the gradient of
    the maximum reaches that edge alone (an even split between the ties would give 0.5 and 0.5)"""
    n, src, dst = po.edges_of("repeated-edge")                # edges 0 and 1 are 0 -> 1, edge 2 is 1 -> 0
    P, Q = _rand(n, 3, seed=4).requires_grad_(True), _rand(n, 3, seed=5).requires_grad_(True)
    row = _rand(1, 3, seed=6)
    R = torch.cat([row, row, _rand(1, 3, seed=7)]).requires_grad_(True)
    agg, arg = po.aggregate(P, Q, R, src, dst)
    m = (P[1] + Q[0] + R[0]).detach()
    assert torch.equal(agg[1].detach(), torch.cat([m, m, 2 * m])) and arg[1].tolist() == [0, 0, 0] and arg[0].tolist() == [2, 2, 2]
    agg[:, 3:6].sum().backward()                              # the loss is the sum of the maxima
    assert torch.equal(R.grad, torch.tensor([[1.0] * 3, [0.0] * 3, [1.0] * 3], dtype=F64))
    assert torch.equal(P.grad, torch.ones(2, 3, dtype=F64)) and torch.equal(Q.grad, torch.ones(2, 3, dtype=F64))


def test_an_isolated_node_gets_zeros_and_no_gradient():
    n, src, dst = po.edges_of("star-in-300")                  # nodes 308 and 309 touch no edge
    x = [_rand(n, 4, seed=1).requires_grad_(True), _rand(n, 4, seed=2).requires_grad_(True),
         _rand(src.numel(), 4, seed=3).requires_grad_(True)]
    agg, arg = po.aggregate(*x, src, dst)
    assert torch.equal(agg[308:].detach(), torch.zeros(2, 12, dtype=F64)) and bool((arg[308:] == -1).all())
    agg.sum().backward()
    assert torch.equal(x[0].grad[308:], torch.zeros(2, 4, dtype=F64)) and torch.equal(x[1].grad[308:], torch.zeros(2, 4, dtype=F64))
    deg = torch.bincount(dst, minlength=n)
    assert float((agg[:, 8:].detach() - agg[:, :4].detach() * deg.clamp(min=1).view(-1, 1)).abs().max()) <= 1e-12   # sum = deg * mean


def test_all_negative_messages_keep_a_negative_maximum():
    """the maximum starts from the first message, not from 0"""
    n, src, dst = po.edges_of("molecule-30")
    P, Q, R = -_rand(n, 4, seed=1).abs() - 1, -_rand(n, 4, seed=2).abs(), -_rand(src.numel(), 4, seed=3).abs()
    agg, arg = po.aggregate(P, Q, R, src, dst)
    m = po.messages(P, Q, R, src, dst)
    assert bool((agg[:, 4:8] < 0).all()) and bool((arg >= 0).all())
    for i in range(n):
        assert torch.equal(agg[i, 4:8], m[dst == i].max(0).values)


def test_oracle_agrees_with_gradcheck():
    """5 nodes, a self-loop (2 -> 2) and a repeated edge (0 -> 1 twice) whose R rows differ: no tie"""
    src, dst = torch.tensor([0, 0, 2, 3, 4, 1, 1]), torch.tensor([1, 1, 2, 2, 3, 4, 0])
    x = [_rand(5, 3, seed=1).requires_grad_(True), _rand(5, 3, seed=2).requires_grad_(True), _rand(7, 3, seed=7).requires_grad_(True)]
    gap, top = po.top_two_gap(po.messages(*x, src, dst), dst, 5)
    assert gap > 1e-3 * top                                   # far from a tie against the 1e-6 step
    assert torch.autograd.gradcheck(lambda *t: po.aggregate(*t, src, dst)[0], x, eps=1e-6, atol=1e-7)


# ---- conditioning of what the GPU tests assert, as a condition ------------------------------------------------------------------------
@pytest.mark.parametrize("C", po.WIDTHS)
def test_every_asserted_case_keeps_its_two_largest_messages_apart(C):
    """the smallest top-two gap of every case is at least 1e-6 of the case's largest |m|, eight times what the two fp32 additions
    of a message can move it: the fp32 and the fp64 arg agree at every node and column"""
    worst = float("inf")
    for name in po.CASES:
        ops, _ = po.inputs_of(name, C)
        n, src, dst = po.edges_of(name)
        gap, top = po.top_two_gap(po.messages(*[t.double() for t in ops], src, dst), dst, n)
        if gap != float("inf"):
            worst = min(worst, gap / top)
            assert gap >= GAP * top, "%s C=%d: the two largest messages of a node are %.3g apart, the largest |m| is %.3g" % (name, C, gap, top)
        ref = po.reference(name, C)
        assert torch.equal(ref[F64]["arg"], ref[F32]["arg"]), (name, C)
    print("C=%d: smallest top-two gap %.3g of the largest |m| (condition %g)" % (C, worst, GAP))


# ---- layouts, construction order, driver ---------------------------------------------------------------------------------------------
def _golden_keys():
    with open(os.path.join(GOLDEN, "gps_pna_state_keys.txt")) as fh:
        return [line.strip() for line in fh if line.strip()]


@pytest.mark.parametrize("global_model_type", ["Transformer", "None"])
def test_state_dict_keys_are_the_reference_layout(global_model_type):
    """the golden list is a one-layer PNA+Transformer model, written down from the definition: edge_encoder, pre_nns.0.0,
    post_nns.0.0, lin and no buffer of the degree histogram; with the global model None the self_attn keys are absent"""
    from esc_gnn_amd.gps_models import GPSModel
    want = [k for k in _golden_keys() if global_model_type == "Transformer" or ".self_attn." not in k]
    mine = GPSModel(layers=1, dim_hidden=16, n_heads=2, local_gnn_type="PNA", global_model_type=global_model_type)
    assert list(mine.state_dict().keys()) == want
    local = {k: tuple(v.shape) for k, v in mine.state_dict().items() if ".local_model." in k and k.endswith("weight")}
    assert local == {"layers.0.local_model.edge_encoder.weight": (16, 16), "layers.0.local_model.pre_nns.0.0.weight": (16, 48),
                     "layers.0.local_model.post_nns.0.0.weight": (16, 64), "layers.0.local_model.lin.weight": (16, 16)}
    oracle = po.GPSModel(layers=1, dim_hidden=16, n_heads=2, global_model_type=global_model_type)
    assert [(k, tuple(v.shape)) for k, v in mine.state_dict().items()] == [(k, tuple(v.shape)) for k, v in oracle.state_dict().items()]
    mine.load_state_dict(oracle.state_dict())


def test_equal_seeds_give_equal_weights():
    from esc_gnn_amd.gps_models import GPSModel
    kw = dict(layers=2, dim_hidden=16, n_heads=2, local_gnn_type="PNA")
    torch.manual_seed(5)
    a = GPSModel(**kw).state_dict()
    torch.manual_seed(5)
    b = GPSModel(**kw).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    torch.manual_seed(5)                                 # ... and the layer draws edge_encoder, pre_nns, post_nns, lin in this order
    from esc_gnn_amd.nn import PNAConv
    mine = PNAConv(8, 8, edge_dim=8).state_dict()
    torch.manual_seed(5)
    ref = po.PNAConv(8).state_dict()
    assert list(mine) == list(ref) and all(torch.equal(mine[k], ref[k]) for k in ref)


def test_driver_accepts_the_two_pna_layer_types():
    from esc_gnn_amd import run_zinc_gps as rg
    assert rg.build_parser().parse_args([]).gt_layer_type == "GINE+Transformer"
    for name, halves in {"PNA+Transformer": ("PNA", "Transformer"), "PNA+None": ("PNA", "None")}.items():
        a = rg.build_parser().parse_args(["--gt_layer_type", name])
        assert rg.layer_type_of(a.gt_layer_type) == halves
    with pytest.raises(SystemExit) as exc:
        rg.main(["--gt_layer_type", "PNA+Performer", "--synthetic_graphs", "12"])
    assert all(name in str(exc.value) for name in rg.LAYER_TYPES) and len(rg.LAYER_TYPES) == 6, str(exc.value)


def test_documented_value_errors():
    from esc_gnn_amd.gps_models import GPSLayer, GPSModel
    from esc_gnn_amd.nn import PNAConv
    for kw, word in ((dict(aggregators=["mean", "min", "max", "std"]), "aggregators"), (dict(aggregators=["max", "mean", "sum"]), "aggregators"),
                     (dict(scalers=["identity", "amplification"]), "scalers"), (dict(towers=2), "towers"),
                     (dict(pre_layers=2), "pre_layers"), (dict(post_layers=2), "post_layers")):
        with pytest.raises(ValueError, match=word):
            PNAConv(8, 8, **dict(dict(edge_dim=8), **kw))
    with pytest.raises(ValueError, match="edge_dim"):
        PNAConv(8, 8)
    with pytest.raises(ValueError, match="in_channels.*out_channels"):
        PNAConv(8, 12, edge_dim=8)
    PNAConv(8, 8, aggregators=["mean", "max", "sum"], scalers=["identity"], deg=torch.tensor([0, 3, 5]), edge_dim=8, towers=1,
            pre_layers=1, post_layers=1, divide_input=False)
    with pytest.raises(ValueError, match="dim_h <= 128"):
        GPSLayer(132, 4, local_gnn_type="PNA")
    GPSLayer(128, 4, local_gnn_type="PNA")
    with pytest.raises(ValueError, match="Unsupported global x-former model: Performer"):
        GPSModel(layers=1, dim_hidden=16, n_heads=2, local_gnn_type="PNA", global_model_type="Performer")
    none = GPSLayer(16, 2, local_gnn_type="PNA", global_model_type="None")
    assert none.self_attn is None and not list(none.local_model.buffers())


def test_a_checkpoint_of_the_pna_layout_is_refused_by_the_gine_layout():
    from esc_gnn_amd.gps_models import GPSModel
    pna = GPSModel(layers=1, dim_hidden=16, n_heads=2, local_gnn_type="PNA")
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        GPSModel(layers=1, dim_hidden=16, n_heads=2).load_state_dict(pna.state_dict())
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        pna.load_state_dict(GPSModel(layers=1, dim_hidden=16, n_heads=2).state_dict())


def test_the_oracle_layer_is_the_split_into_three_products():
    """what the package computes: with W_pre = [W_i | W_j | W_e] cut by input columns, the message of the concatenation is
    (P[i] + Q[j]) + R[k] with P = x W_i^T + b, Q = x W_j^T, R = edge_encoder(e) W_e^T"""
    n, src, dst = po.edges_of("molecule-30")
    torch.manual_seed(3)
    conv = po.PNAConv(8).double()
    x, e = _rand(n, 8, seed=1), _rand(src.numel(), 8, seed=2)
    want = conv(x, torch.stack([src, dst]), e)
    W, b = conv.pre_nns[0][0].weight, conv.pre_nns[0][0].bias
    P, Q, R = x @ W[:, :8].t() + b, x @ W[:, 8:16].t(), conv.edge_encoder(e) @ W[:, 16:].t()
    assert float((po.messages(P, Q, R, src, dst) - conv.last[0]).detach().abs().max()) <= 1e-14
    agg, _ = po.aggregate(P, Q, R, src, dst)
    assert float((conv.lin(conv.post_nns[0](torch.cat([x, agg], 1))) - want).detach().abs().max()) <= 1e-13
    assert gg.CASES is po.CASES
