"""The graph transformer without a GPU: the oracle's ragged attention against torch.nn.MultiheadAttention on the padded batch,
the binding of include/escgnn_gps.h, the cosine schedule against torch's LambdaLR, the driver's defaults against the reference's
configuration file, and the state_dict layout of GPSModel against the oracle model's."""
import ctypes
import os

import pytest
import torch

import gps_oracle as go
from conftest import GOLDEN

SIZES = [1, 2, 37, 64, 65, 130, 3]


def test_ragged_attention_is_padded_multihead_attention():
    """p = 0: the ragged form equals to_dense_batch + MultiheadAttention(key_padding_mask) + gather, in fp64 to 1e-12"""
    torch.manual_seed(0)
    mha = torch.nn.MultiheadAttention(64, 4, batch_first=True).double()
    torch.nn.init.normal_(mha.in_proj_bias)
    torch.nn.init.normal_(mha.out_proj.bias)
    x = torch.randn(sum(SIZES), 64, dtype=torch.float64)
    want = go.padded_attention(mha, x, SIZES)
    got = go.ragged_mha(mha, x, SIZES)
    err = float((got - want).detach().abs().max())
    print("ragged vs padded MultiheadAttention: max |diff| %.3g" % err)
    assert got.shape == want.shape and err <= 1e-12


def test_header_declares_the_three_entry_points():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.GPS_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    p, i64, i, f, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64
    want = {
        "esc_graph_attention_max_nodes": ([i], i64),
        "esc_graph_attention_fwd": ([p, i64, p, p, i64, i64, i64, i64, i, i, f, u64, p, i64, p, p, p], i),
        "esc_graph_attention_bwd": ([p, i64, p, i64, p, p, p, p, i64, i64, i64, i64, i, i, f, p, p], i),
    }
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.GPS_SIGNATURES) == set(want)
    assert not set(want) & (set(nv.SIGNATURES) | set(nv.EXTENSION_SIGNATURES) | set(nv.I2GNN_SIGNATURES) | set(nv.GINEPLUS_SIGNATURES))


def test_cosine_with_warmup_is_torchs_lambda_lr():
    from esc_gnn_amd.optim import CosineWithWarmup

    class Groups(object):
        def __init__(self):
            self.param_groups = [dict(lr=1e-3), dict(lr=0.25)]

    mine = Groups()
    sched = CosineWithWarmup(mine, 5, 50)
    ps = [torch.nn.Parameter(torch.zeros(1)), torch.nn.Parameter(torch.zeros(1))]
    ref = torch.optim.SGD([dict(params=[ps[0]], lr=1e-3), dict(params=[ps[1]], lr=0.25)])
    ref_sched = torch.optim.lr_scheduler.LambdaLR(ref, go.cosine_lambda(5, 50))
    for epoch in range(61):
        assert [g["lr"] for g in mine.param_groups] == [g["lr"] for g in ref.param_groups], epoch
        ref.step()
        ref_sched.step()
        sched.step(0.123)                      # a metric is accepted and ignored


def test_driver_defaults_are_the_reference_configuration():
    import yaml
    from esc_gnn_amd.run_zinc_gps import build_parser
    with open(os.path.join(GOLDEN, "zinc_gps_config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    a = build_parser().parse_args([])
    gt, optim, ds = cfg["gt"], cfg["optim"], cfg["dataset"]
    assert gt["layer_type"].startswith("GINE+Transformer") and gt["batch_norm"] is True and gt["layer_norm"] is False
    assert (a.layers, a.n_heads, a.dim_hidden) == (gt["layers"], gt["n_heads"], gt["dim_hidden"])
    assert (a.dropout, a.attn_dropout) == (gt["dropout"], gt["attn_dropout"])
    assert a.batch_size == cfg["train"]["batch_size"]
    assert a.lr == float(optim["base_lr"]) and a.weight_decay == float(optim["weight_decay"])
    assert (a.epochs, a.num_warmup_epochs) == (optim["max_epoch"], optim["num_warmup_epochs"])
    assert bool(a.clip_grad_norm) is optim["clip_grad_norm"] and a.clip_grad_norm_value == 1.0
    assert (a.node_encoder_num_types, a.edge_encoder_num_types) == (ds["node_encoder_num_types"], ds["edge_encoder_num_types"])


def test_state_dict_layout_is_the_oracle_models():
    from esc_gnn_amd.gps_models import GPSModel
    mine = GPSModel(layers=2, attn_dropout=0.0).state_dict()
    want = go.GPSModel(layers=2).state_dict()
    assert [(k, tuple(v.shape), v.dtype) for k, v in mine.items()] == [(k, tuple(v.shape), v.dtype) for k, v in want.items()]
    for k in ("layers.1.self_attn.in_proj_weight", "layers.0.edge_attn_emb.weight", "layers.0.local_model.eps",
              "layers.1.z_embedding.3.weight", "encoder.node_encoder.encoder.weight", "post_mp.FC_layers.2.bias"):
        assert k in mine, k


def test_attention_layer_loads_a_multihead_attention_state_dict():
    from esc_gnn_amd.nn import GraphMultiheadAttention
    torch.manual_seed(3)
    ref = torch.nn.MultiheadAttention(64, 4, dropout=0.5, batch_first=True)
    torch.manual_seed(3)
    mine = GraphMultiheadAttention(64, 4, dropout=0.5)
    for (k, a), (k2, b) in zip(mine.state_dict().items(), ref.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k                 # same keys, and the same values from the same stream
    mine.load_state_dict(ref.state_dict())
