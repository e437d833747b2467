"""The random-walk structural encoding without a GPU: the binding of include/escgnn_rwse.h, the oracle against closed forms and
against an independent matrix power, the reference's own fp32 expression against the fp64 oracle (how far the reference itself
lies from the exact value), the step-list validation of ops.rw_landing, the state_dict layouts and initial weights of the RWSE
encoder and of the TypeDictNode+RWSE / TypeDictNode+LapPE+RWSE models against the oracle built the reference's way, and the
driver's new flags."""
import ctypes

import numpy as np
import pytest
import torch

import gps_oracle as go
import lappe_oracle as lo
import rwse_oracle as ro


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def _want():
    p, i64, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    return {
        "esc_rw_landing_max_nodes": ([], i64),
        "esc_rw_landing_max_edges": ([], i64),
        "esc_rw_landing": ([p, p, i64, p, p, i64, i64, i, i64, i64, i64, p, i64, p], i),
        "esc_rwse_gather": ([p, p, i64, i64, p, p, i64, i64, i, p, i64, p], i),
    }


def test_header_declares_exactly_the_new_entry_points():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.RWSE_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    want = _want()
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.RWSE_SIGNATURES) == set(want)
    others = [nv.SIGNATURES, nv.EXTENSION_SIGNATURES, nv.I2GNN_SIGNATURES, nv.GINEPLUS_SIGNATURES, nv.GPS_SIGNATURES, nv.LAPPE_SIGNATURES]
    assert not any(set(want) & set(o) for o in others)
    assert nv.ABI_VERSION == nv.const("ESC_ABI_VERSION")


def test_every_declared_symbol_is_exported_by_the_built_library():
    from esc_gnn_amd import _native as nv
    h = ctypes.CDLL(nv.LIB_PATH)
    for name in _want():
        assert hasattr(h, name), name
    assert (h.esc_rw_landing_max_nodes(), h.esc_rw_landing_max_edges()) == (ro.MAX_NODES, ro.MAX_EDGES)
    assert ro.MAX_NODES >= 256 and ro.MAX_EDGES >= 4096


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def test_the_list_of_graphs_is_the_one_the_comparison_needs():
    assert len(set(ro.NAMES)) == len(ro.NAMES) == 17
    by = {g[0]: g for g in ro.GRAPHS}
    for name, n, e, why in ro.GRAPHS:
        assert why and e.dtype == np.int64 and e.shape[0] == 2 and (e.size == 0 or (0 <= e.min() and e.max() < n)), name
        assert n <= ro.MAX_NODES and e.shape[1] <= ro.MAX_EDGES, name
    assert by["random-256"][1] == ro.MAX_NODES and by["multigraph-edge-limit"][2].shape[1] == ro.MAX_EDGES
    assert by["random-65"][1] == 65 and by["molecule-37"][1] == 37
    mol = by["molecule-37"][2]
    assert np.array_equal(mol[:, -37:], np.arange(37)[None, :].repeat(2, 0)), "the self-loops come last, as create_subgraphs appends them"
    d = by["triangle+path-directed"][2]
    assert not {(a, b) for a, b in d.T} & {(b, a) for a, b in d.T} and 6 not in d[0] and 7 not in d
    assert (by["triangle+path-self-loop"][2][0] == by["triangle+path-self-loop"][2][1]).sum() == 1
    dup = by["triangle+path-duplicate"][2]
    assert len({(a, b) for a, b in dup.T}) == dup.shape[1] - 1
    src = by["descending-sources"][2][0]
    assert (np.diff(src) <= 0).all() and src[0] > src[-1]
    mg = by["multigraph-edge-limit"][2]
    assert (mg[0] == mg[1]).any() and len({(a, b) for a, b in mg.T}) < mg.shape[1]


def test_oracle_against_closed_forms_exactly():
    by = {g[0]: g for g in ro.GRAPHS}
    k20 = ro.KSTEPS

    def rw(name, ks=k20):
        _, n, e, _ = by[name]
        return ro.rw_landing64(n, e, ks)
    assert rw("one-node").shape == (1, 20) and not rw("one-node").any()
    two = rw("two-node-edge")
    assert (two[:, 0::2] == 0.0).all() and (two[:, 1::2] == 1.0).all()            # columns 0, 2, ...: steps 1, 3, ...
    assert np.array_equal(rw("triangle", [1, 2, 3]), np.tile([0.0, 0.5, 0.25], (3, 1)))
    c12 = rw("cycle-12")
    assert (c12[:, 0::2] == 0.0).all() and (c12[:, 1] == 0.5).all()
    star = rw("star-6")
    assert (star[:, 0::2] == 0.0).all() and star[0, 1] == 1.0
    assert (rw("K5", [1, 2])[:, 1] == 0.25).all() and (rw("K5", [1, 2])[:, 0] == 0.0).all()
    pet = rw("petersen", [1, 2, 3, 4, 5])
    assert (pet[:, [0, 2]] == 0.0).all() and (pet[:, 4] > 0).all() and np.allclose(pet[:, 1], 1.0 / 3.0, rtol=1e-15, atol=0)
    p3 = rw("path-3", [2, 4])
    assert (p3[1] == 1.0).all() and (p3[0] == 0.5).all()
    iso = rw("triangle+path-isolated")
    assert not iso[7].any()
    d = rw("triangle+path-directed")
    assert not d[3:].any(), "a walk along the directed path never returns, and the sink's row of P is zero"
    assert (d[:3, 2] == 1.0).all() and (d[:3, 0] == 0.0).all(), "the directed triangle returns at every third step"
    loop = rw("triangle+path-self-loop", [1])
    assert loop[2, 0] == 1.0 / 3.0 and not np.delete(loop[:, 0], 2).any()
    # the duplicated edge 4 -> 5: deg[4] = 3 with P[4, 3] = 1/3 and P[4, 5] = 2/3, so (P^2)[3, 3] = 1 * 1/3 where the simple graph has 1/2
    dup, plain = rw("triangle+path-duplicate", [2]), rw("triangle+path-isolated", [2])
    assert dup[3, 0] == 1.0 / 3.0 and plain[3, 0] == 0.5
    assert abs(dup[4, 0] - 2.0 / 3.0) <= 2.0 ** -52 and plain[4, 0] == 0.75 and np.array_equal(dup[:3], plain[:3])


@pytest.mark.parametrize("name,n,edges,why", ro.GRAPHS, ids=ro.NAMES)
def test_oracle_trace_against_an_independent_matrix_power(name, n, edges, why):
    """the rows of the oracle sum to the trace of P^k, P^k by numpy.linalg.matrix_power (repeated squaring: another order)"""
    ks = [1, 2, 3, 7, 20] if n > 200 else ro.GAPPED + [20]
    ks = sorted(set(ks))
    P = ro.transition(n, edges)
    deg_zero = ~P.any(1)
    assert np.allclose(P.sum(1)[~deg_zero], 1.0, rtol=1e-14) and (P >= 0).all()
    got = ro.rw_landing64(n, edges, ks)
    for c, k in enumerate(ks):
        want = np.trace(np.linalg.matrix_power(P, k))
        assert abs(got[:, c].sum() - want) <= 1e-12 * max(1.0, abs(want)), (name, k)
    assert (got >= 0).all() and (got <= 1.0 + 1e-14).all()


@pytest.mark.parametrize("name,n,edges,why", ro.GRAPHS, ids=ro.NAMES)
def test_reference_fp32_expression_against_the_fp64_oracle(name, n, edges, why):
    """how far the reference's own fp32 result lies from the fp64 value: printed per graph.  fp32 products of n terms over 20
    steps: a relative error of a few times 20 * n * 2^-24 of the largest entry bounds it loosely"""
    want = ro.rw_landing64(n, edges, ro.KSTEPS)
    got = ro.rw_landing_ref32(n, edges, ro.KSTEPS).numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    dist = float(np.abs(got - want).max())
    print("%-28s n %3d  reference fp32 against fp64: largest distance %.3g" % (name, n, dist))
    assert dist <= 20 * max(n, 8) * 2.0 ** -24
    assert (got[want == 0.0] == 0.0).all(), "sums of non-negative terms: an exact zero stays one in any precision"


@pytest.mark.parametrize("name", ["triangle", "petersen", "triangle+path-directed", "molecule-37", "random-65"])
def test_consecutive_and_matrix_power_branches_agree(name):
    _, n, edges, _ = ro.GRAPHS[ro.NAMES.index(name)]
    cons = ro.rw_landing_ref32(n, edges, list(range(1, 9))).numpy()
    for ks in ([1, 2, 4, 8], [3], [2, 3, 5, 7]):
        gapped = ro.rw_landing_ref32(n, edges, ks).numpy()
        assert gapped.shape == (n, len(ks))
        assert np.abs(gapped - cons[:, [k - 1 for k in ks]]).max() <= 8 * n * 2.0 ** -24
        want = ro.rw_landing64(n, edges, ks)
        assert np.abs(gapped - want).max() <= 8 * n * 2.0 ** -24
    from_two = ro.rw_landing_ref32(n, edges, [2, 3, 4]).numpy()        # consecutive, not from 1: matrix_power(min) first
    assert np.abs(from_two - cons[:, 1:4]).max() <= 8 * n * 2.0 ** -24


# ---- ops.rw_landing's step list -----------------------------------------------------------------------------------------------------
def test_step_list_validation():
    from esc_gnn_amd import ops
    ei = torch.zeros((2, 0), dtype=torch.int64)
    ptr = torch.zeros(2, dtype=torch.int64)
    for bad, what in (([], "non-empty"), ([1, 1, 2], "repeated"), ([0, 1], r"outside 1\.\.63"), ([1, 64], r"outside 1\.\.63"),
                      ([-3], r"outside 1\.\.63"), ([2, 1], "ascending"), ([1, 3, 2], "ascending"), ([1.5], "list of ints"),
                      (None, "list of ints")):
        with pytest.raises(ValueError, match=what):
            ops.rw_landing(ei, ptr, ptr, bad)
        with pytest.raises(ValueError, match=what):
            ops.rw_step_mask(bad)
    assert ops.rw_step_mask([1]) == 1 and ops.rw_step_mask([63]) == 1 << 62 and ops.rw_step_mask(range(1, 21)) == (1 << 20) - 1
    assert ops.rw_step_mask(ro.GAPPED) == sum(1 << (k - 1) for k in ro.GAPPED) and 0 < ops.rw_step_mask(range(1, 64)) < 1 << 63
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # a valid list reaches the device check: nothing runs on the host
        ops.rw_landing(ei, ptr, ptr, [1, 2])


# ---- encoder and model layouts ----------------------------------------------------------------------------------------------------
ENCODERS = [("linear", 1, "batchnorm"), ("linear", 1, "none"), ("mlp", 1, "batchnorm"), ("mlp", 2, "batchnorm"), ("mlp", 3, "batchnorm"),
            ("mlp", 3, "none")]


def _same(mine, want):
    assert [(k, tuple(v.shape), v.dtype) for k, v in mine.items()] == [(k, tuple(v.shape), v.dtype) for k, v in want.items()]
    for k in want:
        assert torch.equal(mine[k], want[k]), k


@pytest.mark.parametrize("model,layers,raw_norm", ENCODERS)
def test_encoder_layout_and_initial_weights_equal_the_oracles(model, layers, raw_norm):
    from esc_gnn_amd import nn as enn
    for dim_pe, steps in ((28, 20), (5, 3)):
        torch.manual_seed(31)
        want = ro.RWSEEncoder(dim_pe, steps, model, layers, raw_norm)
        torch.manual_seed(31)
        mine = enn.RWSENodeEncoder(dim_pe, steps, model=model, layers=layers, raw_norm=raw_norm)
        _same(mine.state_dict(), want.state_dict())
        keys = list(mine.state_dict())
        assert ("raw_norm.weight" in keys) == (raw_norm == "batchnorm")
        if model == "linear":
            assert keys[-2:] == ["pe_encoder.weight", "pe_encoder.bias"] and isinstance(mine.pe_encoder, enn.Linear)
        else:
            n_lin = max(layers, 1) if layers == 1 else layers
            assert [k for k in keys if k.startswith("pe_encoder")] == ["pe_encoder.%d.%s" % (2 * j, w) for j in range(n_lin) for w in ("weight", "bias")]
            assert all(isinstance(m, (enn.Linear, enn.ReLU)) for m in mine.pe_encoder), "the library's kernels, not torch's"
        assert mine.raw_norm is None or isinstance(mine.raw_norm, enn.BatchNorm1d)


def test_encoder_refuses_what_it_does_not_implement():
    from esc_gnn_amd.nn import RWSENodeEncoder
    with pytest.raises(ValueError, match="RWSENodeEncoder: Does not support 'transformer' encoder model."):
        RWSENodeEncoder(28, 20, model="Transformer")
    for kw in (dict(expand_x=True), dict(pass_as_var=True)):
        with pytest.raises(ValueError, match="expand_x and pass_as_var"):
            RWSENodeEncoder(28, 20, **kw)

    class NoKeys(object):
        pass
    with pytest.raises(ValueError, match="Precomputed 'pestat_RWSE' variable is required for RWSENodeEncoder; set config "
                                         "'posenc_RWSE.enable' to True, and also set 'posenc.kernel.times' values"):
        RWSENodeEncoder(28, 20)(NoKeys())


@pytest.mark.parametrize("model,layers,raw_norm", ENCODERS)
@pytest.mark.parametrize("lap_pe", [False, True], ids=["Concat2", "Concat3"])
def test_model_layout_and_initial_weights_equal_the_oracle_models(lap_pe, model, layers, raw_norm):
    from esc_gnn_amd.gps_models import GPSModel
    kw = dict(rwse_dim_pe=28, rwse_steps=20, rwse_model=model, rwse_layers=layers, rwse_raw_norm=raw_norm)
    torch.manual_seed(9)
    want = ro.GPSModel(layers=1, lap_pe=lap_pe, **kw).state_dict()
    torch.manual_seed(9)
    mine = GPSModel(layers=1, attn_dropout=0.0, lap_pe=lap_pe, rwse=True, **kw).state_dict()
    _same(mine, want)
    pre = "encoder.node_encoder."
    assert tuple(mine[pre + "encoder1.encoder.weight"].shape) == (28, 64 - 28 - (8 if lap_pe else 0))
    rw = pre + ("encoder3." if lap_pe else "encoder2.")
    assert any(k.startswith(rw + "pe_encoder") for k in mine) and (rw + "raw_norm.running_mean" in mine) == (raw_norm == "batchnorm")
    assert (pre + "encoder2.linear_A.weight" in mine) == lap_pe and (pre + "encoder3.pe_encoder.weight" in mine) == (lap_pe and model == "linear")
    assert pre + "encoder.weight" not in mine


def test_a_width_that_leaves_nothing_for_the_type_embedding_is_refused():
    from esc_gnn_amd.gps_models import GPSModel
    with pytest.raises(ValueError, match="RWSE size 64 is too large for desired embedding size of 64"):
        GPSModel(layers=1, rwse=True, rwse_dim_pe=64)
    with pytest.raises(ValueError, match=r"LapPE\+RWSE size 8\+56 is too large for desired embedding size of 64"):
        GPSModel(layers=1, lap_pe=True, rwse=True, rwse_dim_pe=56)
    GPSModel(layers=1, lap_pe=True, rwse=True, rwse_dim_pe=55)


def test_lap_pe_only_and_plain_layouts_are_unchanged():
    from esc_gnn_amd.gps_models import GPSModel
    off = dict(rwse=False, rwse_dim_pe=28, rwse_steps=20, rwse_model="linear", rwse_layers=1, rwse_raw_norm="batchnorm")
    for lap_pe, oracle in ((False, go.GPSModel), (True, lo.GPSModel)):
        torch.manual_seed(5)
        a = GPSModel(layers=2, attn_dropout=0.0, lap_pe=lap_pe).state_dict()
        torch.manual_seed(5)
        b = GPSModel(layers=2, attn_dropout=0.0, lap_pe=lap_pe, **off).state_dict()
        torch.manual_seed(5)
        want = oracle(layers=2).state_dict()
        _same(a, want)
        _same(b, want)
        assert not any("encoder3" in k or "raw_norm" in k for k in a)
    plain = GPSModel(layers=1).state_dict()
    assert "encoder.node_encoder.encoder.weight" in plain and not any("encoder1" in k for k in plain)


# ---- the driver's flags -----------------------------------------------------------------------------------------------------------
def test_parser_defaults_and_flags():
    from esc_gnn_amd.run_zinc_gps import build_parser
    a = build_parser().parse_args([])
    assert a.posenc_RWSE == 0, "opt-in: the default run is today's"
    assert (a.posenc_RWSE_ksteps, a.posenc_RWSE_dim_pe, a.posenc_RWSE_model, a.posenc_RWSE_layers, a.posenc_RWSE_raw_norm_type) == \
        (20, 28, "linear", 1, "BatchNorm")
    assert a.posenc_LapPE == 0
    on = build_parser().parse_args(["--posenc_RWSE", "1"])
    assert on.posenc_RWSE == 1 and on.posenc_LapPE == 0
    both = build_parser().parse_args("--posenc_RWSE 1 --posenc_LapPE 1 --posenc_RWSE_ksteps 16 --posenc_RWSE_model mlp --posenc_RWSE_layers 2".split())
    assert (both.posenc_RWSE, both.posenc_LapPE, both.posenc_RWSE_ksteps, both.posenc_RWSE_model, both.posenc_RWSE_layers) == (1, 1, 16, "mlp", 2)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--posenc_RWSE", "2"])
    helps = build_parser().format_help()
    assert "upstream" in helps and "posenc_RWSE_raw_norm_type" in helps
