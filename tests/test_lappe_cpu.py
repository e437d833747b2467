"""The Laplacian positional encoding without a GPU: the binding of include/escgnn_lappe.h, the oracle's decomposition against
numpy.linalg.eigh under the sign- and basis-free comparison (and the conditioning of the test graphs that comparison relies on),
the state_dict layout and initial weights of the TypeDictNode+LapPE encoder against the oracle built the reference's way, the
driver's new defaults against the reference's configuration file, and the oracle encoder against a step-by-step evaluation."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gps_oracle as go
import lappe_oracle as lo
from conftest import GOLDEN


def test_header_declares_exactly_the_new_entry_points():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.LAPPE_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    want = {
        "esc_laplacian_eig_max_nodes": ([], i64),
        "esc_laplacian_eig_lds_nodes": ([], i64),
        "esc_laplacian_eig_scratch_bytes": ([i64, i64], i64),
        "esc_laplacian_eig": ([p, p, i64, p, p, i64, i64, i, i, i64, p, i64, p, p, p], i),
        "esc_lappe_gather": ([p, p, p, i64, i64, p, p, i64, i64, i, p, p, p], i),
        "esc_lappe_encode_fwd": ([p, p, p, p, p, p, p, i64, i, i, p, i64, p], i),
        "esc_lappe_encode_block_rows": ([], i64),
        "esc_lappe_encode_scratch_floats": ([i64, i], i64),
        "esc_lappe_encode_bwd": ([p, p, p, p, p, p, p, p, i64, i64, i, i, p, i64, p, p, p, p, p], i),
    }
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.LAPPE_SIGNATURES) == set(want)
    others = set(nv.SIGNATURES) | set(nv.EXTENSION_SIGNATURES) | set(nv.I2GNN_SIGNATURES) | set(nv.GINEPLUS_SIGNATURES) | set(nv.GPS_SIGNATURES)
    assert not set(want) & others


def test_the_list_of_graphs_is_the_one_the_comparison_needs():
    names = [g[0] for g in lo.GRAPHS]
    assert len(set(names)) == len(names) == 16
    by = {g[0]: g for g in lo.GRAPHS}
    assert by["one-node"][1] < lo.K_DEFAULT and by["molecule-37"][1] == 37
    assert (by["random-lds-limit"][1], by["random-over-lds"][1], by["random-256"][1]) == (lo.LDS_NODES, lo.LDS_NODES + 1, lo.MAX_NODES)
    for name, n, e, _ in lo.GRAPHS:
        assert e.dtype == np.int64 and e.shape[0] == 2 and (e.size == 0 or (0 <= e.min() and e.max() < n)), name
    w = np.linalg.eigh(lo.laplacian(12, by["cycle-12"][2]))[0]
    assert abs(w[7] - w[8]) < 1e-12 and w[8] - w[6] > 0.5, "K = 8 must cut an eigenspace of C12"
    w = np.linalg.eigh(lo.laplacian(10, by["petersen"][2]))[0]
    assert abs(w[5] - w[1]) < 1e-12 and w[6] - w[5] > 1, "eigenvalue 2 of the Petersen graph is five-fold; K = 8 cuts the next one"
    assert np.array_equal(lo.laplacian(7, by["triangle+path"][2]), lo.laplacian(7, by["triangle+path-directed"][2]))
    assert np.array_equal(lo.laplacian(7, by["triangle+path"][2]), lo.laplacian(7, by["triangle+path-self-loop"][2]))
    assert (by["triangle+path-self-loop"][2][0] == by["triangle+path-self-loop"][2][1]).any()
    d = by["triangle+path-directed"][2]
    assert not {(a, b) for a, b in d.T} & {(b, a) for a, b in d.T}


@pytest.mark.parametrize("name,n,edges,why", lo.GRAPHS, ids=[g[0] for g in lo.GRAPHS])
def test_oracle_decomposition_against_eigh(name, n, edges, why):
    """(i)-(vi) for the oracle itself, and the conditioning every comparison of the device's fp32 output relies on: among the
    first K+1 eigenvalues distinct clusters lie at least 1e-3 apart"""
    vals, vecs = lo.lap_pe(n, edges)
    assert vals.shape == (n, lo.K_DEFAULT, 1) and vecs.shape == (n, lo.K_DEFAULT)
    lo.compare(name, n, edges, vals, vecs, bound=1e-12)
    gap = lo.smallest_gap(n, edges)
    print("%s: smallest gap between clusters of the first K+1 eigenvalues %.4g" % (name, gap))
    assert gap >= lo.GAP


def test_comparison_rejects_what_it_should():
    """a wrong eigenvalue, a vector from outside the eigenspace, a lost NaN and a scaled column all fail"""
    name, n, edges, _ = lo.GRAPHS[5]                       # cycle-12
    vals, vecs = lo.lap_pe(n, edges)
    for spoil in ("value", "vector", "nan", "norm"):
        a, b = vals.copy(), vecs.copy()
        if spoil == "value":
            a[:, 3] += 1e-3
        elif spoil == "vector":
            b[:, 1] = np.roll(b[:, 1], 1) * 0.5 + b[:, 5] * 0.5
        elif spoil == "nan":
            b[2, 0] = np.nan
        else:
            b[:, 2] *= 1.001
        with pytest.raises(AssertionError):
            lo.compare(name, n, edges, a, b)


def test_state_dict_layout_with_lap_pe_is_the_oracle_models():
    from esc_gnn_amd.gps_models import GPSModel
    mine = GPSModel(layers=2, attn_dropout=0.0, lap_pe=True).state_dict()
    want = lo.GPSModel(layers=2).state_dict()
    assert [(k, tuple(v.shape), v.dtype) for k, v in mine.items()] == [(k, tuple(v.shape), v.dtype) for k, v in want.items()]
    pre = "encoder.node_encoder."
    assert tuple(mine[pre + "encoder1.encoder.weight"].shape) == (28, 56)
    shapes = {"encoder2.linear_A.weight": (16, 2), "encoder2.linear_A.bias": (16,), "encoder2.pe_encoder.1.weight": (8, 16),
              "encoder2.pe_encoder.1.bias": (8,)}
    for k, shape in shapes.items():
        assert tuple(mine[pre + k].shape) == shape, k
    assert pre + "encoder.weight" not in mine


def test_default_layout_is_unchanged():
    from esc_gnn_amd.gps_models import GPSModel
    torch.manual_seed(5)
    mine = GPSModel(layers=2, attn_dropout=0.0)
    torch.manual_seed(5)
    off = GPSModel(layers=2, attn_dropout=0.0, lap_pe=False, dim_pe=8, max_freqs=8)
    want = go.GPSModel(layers=2).state_dict()
    for sd in (mine.state_dict(), off.state_dict()):
        assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == [(k, tuple(v.shape), v.dtype) for k, v in want.items()]
    assert all(torch.equal(a, b) for a, b in zip(mine.state_dict().values(), off.state_dict().values()))
    assert "encoder.node_encoder.encoder.weight" in mine.state_dict() and not any("encoder2" in k for k in mine.state_dict())


@pytest.mark.parametrize("dim_pe", [8, 4, 16])
def test_encoder_initial_weights_equal_the_oracles(dim_pe):
    """the reference constructs Linear(2, dim_pe) and replaces it by Linear(2, 2 dim_pe): the generator is consumed twice"""
    from esc_gnn_amd.nn import LapPENodeEncoder
    torch.manual_seed(21)
    want = lo.LapPEEncoder(dim_pe).state_dict()
    torch.manual_seed(21)
    mine = LapPENodeEncoder(dim_pe).state_dict()
    assert list(mine) == list(want) == ["linear_A.weight", "linear_A.bias", "pe_encoder.1.weight", "pe_encoder.1.bias"]
    for k in want:
        assert torch.equal(mine[k], want[k]), k
    torch.manual_seed(21)
    once = torch.nn.Linear(2, 2 * dim_pe)                  # drawn once only, the weights differ
    assert not torch.equal(once.weight, want["linear_A.weight"])


def test_encoder_refuses_what_it_does_not_implement():
    from esc_gnn_amd.nn import LapPENodeEncoder
    for kw in (dict(model="Transformer"), dict(layers=1), dict(layers=3), dict(post_layers=1), dict(raw_norm_type="batchnorm")):
        with pytest.raises(ValueError, match="DeepSet.*layers 2.*post_layers 0.*raw_norm_type 'none'"):
            LapPENodeEncoder(**kw)
    enc = LapPENodeEncoder()
    assert enc.signs_override is None

    class NoKeys(object):
        pass
    with pytest.raises(ValueError, match="Precomputed eigen values and vectors are required"):
        enc(NoKeys())


def test_driver_defaults_are_the_reference_configuration():
    import yaml
    from esc_gnn_amd.run_zinc_gps import build_parser
    with open(os.path.join(GOLDEN, "zinc_gps_config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    pe = cfg["posenc_LapPE"]
    assert cfg["dataset"]["node_encoder_name"] == "TypeDictNode+LapPE" and pe["enable"] is True
    assert pe["eigen"] == dict(laplacian_norm="none", eigvec_norm="L2", max_freqs=8)
    a = build_parser().parse_args([])
    assert a.posenc_LapPE == 0, "opt-in: the default run is today's"
    assert (a.posenc_LapPE_max_freqs, a.posenc_LapPE_dim_pe) == (pe["eigen"]["max_freqs"], pe["dim_pe"])
    assert (pe["layers"], pe["model"], pe["raw_norm_type"]) == (2, "DeepSet", "none")      # what nn.LapPENodeEncoder's defaults implement
    from esc_gnn_amd.nn import LapPENodeEncoder
    enc = LapPENodeEncoder()
    assert (enc.dim_pe, enc.max_freqs) == (pe["dim_pe"], pe["eigen"]["max_freqs"])
    on = build_parser().parse_args(["--posenc_LapPE", "1"])
    assert on.posenc_LapPE == 1


def test_oracle_encoder_equals_the_stepwise_forward():
    """on a batch with NaN padding (graphs of 1, 3 and 5 nodes at K = 8, and a row that is NaN throughout), with and without
    signs, in fp64 to 1e-12 - values and parameter gradients"""
    torch.manual_seed(2)
    enc = lo.LapPEEncoder(8).double()
    vals, vecs = [], []
    for n in (1, 3, 5):
        a, b = lo.lap_pe(n, lo._both(lo._path(n)))
        vals.append(torch.from_numpy(a))
        vecs.append(torch.from_numpy(b))
    vals, vecs = torch.cat(vals), torch.cat(vecs)
    vecs[4, :] = float("nan")
    assert bool(torch.isnan(vecs).any()) and not bool(torch.isnan(vecs[:, 0]).all())
    signs = torch.tensor([1.0, -1, -1, 1, 1, -1, 1, -1], dtype=torch.float64)
    for s in (None, signs):
        grads = []
        for fn in (enc, lambda v, l, sg: lo.stepwise_forward(enc, v, l, sg)):
            enc.zero_grad()
            out = fn(vecs, vals, s)
            (out * torch.cos(torch.arange(out.numel(), dtype=torch.float64)).view_as(out)).sum().backward()
            grads.append((out.detach(), [p.grad.clone() for p in enc.parameters()]))
        (o1, g1), (o2, g2) = grads
        assert o1.shape == (9, 8) and float((o1 - o2).abs().max()) <= 1e-12
        assert all(float((a - b).abs().max()) <= 1e-12 for a, b in zip(g1, g2))
        assert not bool(o1[4].any()), "a row whose entries are all NaN encodes to exact zeros"
