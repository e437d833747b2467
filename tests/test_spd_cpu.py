"""The shortest-path attention bias without a GPU: the binding of include/escgnn_spd.h, the distance oracle against networkx
(the reference's path) and against closed forms, the ragged biased attention oracle against torch.nn.MultiheadAttention on the
padded batch with the float attn_mask built the reference's way (fp64, 1e-12: outputs and every gradient, row 100 of the
embedding exactly zero, the table form equal to the per-pair form), and the driver's and the model's new layer types."""
import ctypes

import numpy as np
import pytest
import torch

import gps_oracle as go
import spd_oracle as so

TOL = 1e-12                      # tests/test_gps_cpu.py's fp64 tolerance


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def _want():
    p, i64, i, f, u64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_uint64
    return {
        "esc_graph_spd_max_nodes": ([], i64),
        "esc_graph_spd": ([p, p, i64, p, p, p, i64, i64, i64, i, i64, p, p], i),
        "esc_spd_gather": ([p, p, p, i64, i64, p, p, p, i64, i64, p, p], i),
        "esc_graph_attention_bias_max_nodes": ([i], i64),
        "esc_graph_attention_bias_scratch_floats": ([i64, i], i64),
        "esc_graph_attention_bias_fwd": ([p, i64, p, p, p, i64, p, i64, i64, i64, i64, i, i, f, u64, p, i64, p, p, p], i),
        "esc_graph_attention_bias_bwd": ([p, i64, p, i64, p, p, p, p, p, i64, p, i64, i64, i64, i64, i, i, f, p, p, i64, p, p], i),
    }


def test_header_declares_exactly_the_new_entry_points():
    from esc_gnn_amd import _abi, _native as nv
    abi = _abi.load(nv.SPD_HEADER)
    assert not abi.structs and not abi.constants and not abi.callbacks
    want = _want()
    assert {k: (list(a), r) for k, (a, r) in abi.functions.items()} == want
    assert set(nv.SPD_SIGNATURES) == set(want)
    others = (nv.SIGNATURES, nv.EXTENSION_SIGNATURES, nv.I2GNN_SIGNATURES, nv.GINEPLUS_SIGNATURES, nv.GPS_SIGNATURES, nv.LAPPE_SIGNATURES,
              nv.RWSE_SIGNATURES, nv.STEP_SIGNATURES, nv.GATEDGCN_SIGNATURES, nv.PNA_SIGNATURES)
    assert not any(set(want) & set(o) for o in others)
    assert sorted(nv.GPS_SIGNATURES) == ["esc_graph_attention_bwd", "esc_graph_attention_fwd", "esc_graph_attention_max_nodes"]
    assert nv.ABI_VERSION == nv.const("ESC_ABI_VERSION")


def test_every_declared_symbol_is_exported_and_the_limits_hold():
    from esc_gnn_amd import _native as nv
    h = ctypes.CDLL(nv.LIB_PATH)
    for name in _want():
        assert hasattr(h, name), name
    for fn in (h.esc_graph_spd_max_nodes, h.esc_graph_attention_bias_max_nodes, h.esc_graph_attention_max_nodes):
        fn.restype = ctypes.c_int64
    assert h.esc_graph_spd_max_nodes() == so.MAX_NODES >= 256
    limits = {d: h.esc_graph_attention_bias_max_nodes(d) for d in (4, 8, 12, 16, 32, 64)}
    assert all(64 <= v <= h.esc_graph_attention_max_nodes(d) and v % 4 == 0 for d, v in limits.items()), limits
    assert limits[16] >= 222 and limits[12] == limits[16]
    # the header's formula: (2 DP + 2) floats per node beside 104 floats of table and 101 x 256 floats of bins in 160 KiB
    for d, dp in ((4, 4), (8, 8), (16, 16), (32, 32), (64, 64)):
        fit = ((160 * 1024 - 4 * (104 + 101 * 256)) // (4 * (2 * dp + 2))) // 4 * 4
        assert limits[d] == min(fit, h.esc_graph_attention_max_nodes(d)), d
    assert h.esc_graph_attention_bias_max_nodes(6) == 0 and h.esc_graph_attention_bias_max_nodes(68) == 0


# ---- the distance oracle ----------------------------------------------------------------------------------------------------------
def test_the_list_of_graphs_is_the_one_the_comparison_needs():
    by = {g[0]: g for g in so.GRAPHS + so.DEVICE_GRAPHS}
    assert so.NAMES == ["one-node", "two-isolated", "path-5", "cycle-6-chord", "two-components-7", "loops-and-duplicates",
                        "one-direction-only", "path-104"]
    for name, n, e in by.values():
        assert e.dtype == np.int64 and e.shape[0] == 2 and (e.size == 0 or (0 <= e.min() and e.max() < n)) and n <= so.MAX_NODES, name
    dup = by["loops-and-duplicates"][2]
    assert (dup[0] == dup[1]).sum() == 3 and len({(a, b) for a, b in dup.T}) < dup.shape[1]
    one = by["one-direction-only"][2]
    assert not {(a, b) for a, b in one.T} & {(b, a) for a, b in one.T}
    assert [by[k][1] for k in ("random-64", "random-65", "random-129", "random-256")] == [64, 65, 129, so.MAX_NODES]
    for k in ("random-64", "random-65", "random-129", "random-256"):
        d = so.spd_bfs(by[k][1], by[k][2])
        assert (d == so.NO_PATH).any() and 3 < d[d < so.NO_PATH].max() < so.NO_PATH, k      # several components, and long paths


@pytest.mark.parametrize("name,n,edges", so.GRAPHS + so.DEVICE_GRAPHS, ids=[g[0] for g in so.GRAPHS + so.DEVICE_GRAPHS])
def test_bfs_equals_networkx_with_the_references_fill(name, n, edges):
    want = so.spd_networkx(n, edges)
    got = so.spd_bfs(n, edges)
    assert got.dtype == np.uint8 and got.shape == (n, n)
    assert np.array_equal(got.astype(np.int64), np.minimum(want, so.NO_PATH))
    assert np.array_equal(got, got.T) and not got.diagonal().any()


def test_oracle_against_closed_forms():
    by = {g[0]: g for g in so.GRAPHS}
    d = lambda name: so.spd_bfs(by[name][1], by[name][2]).astype(np.int64)      # noqa: E731
    assert d("one-node").tolist() == [[0]]
    assert d("two-isolated").tolist() == [[0, 100], [100, 0]]
    i = np.arange(5)
    assert np.array_equal(d("path-5"), np.abs(i[:, None] - i[None, :]))
    c = d("cycle-6-chord")
    assert c[0, 3] == 1 and c[1, 4] == 3 and c[0, 2] == 2 and c[2, 5] == 3 and c.max() == 3
    t = d("two-components-7")
    assert (t[:3, 3:] == 100).all() and (t[3:, :3] == 100).all() and t[3, 6] == 3 and t[0, 2] == 1
    ld = d("loops-and-duplicates")
    assert np.array_equal(ld[:3, :3], np.abs(i[:3, None] - i[None, :3])) and (ld[3, :3] == 100).all() and (ld[4] == [100, 100, 100, 100, 0]).all()
    od = d("one-direction-only")
    assert np.array_equal(od[:5, :5], np.abs(i[:, None] - i[None, :])) and (od[5, :5] == 100).all()
    long = d("path-104")
    j = np.arange(104)
    assert np.array_equal(long, np.minimum(np.abs(j[:, None] - j[None, :]), 100)) and long[0, 103] == 100 and long[0, 99] == 99
    assert (so.spd_networkx(104, by["path-104"][2]) > 100).any(), "the clamp is exercised: the reference's lookup would raise here"


# ---- the biased attention oracle ----------------------------------------------------------------------------------------------------
def _case(sizes_graphs, heads, d, seed):
    _, sizes, flat = so.collate(sizes_graphs)
    spds = so.split_spd(flat, sizes)
    torch.manual_seed(seed)
    H = heads * d
    mha = torch.nn.MultiheadAttention(H, heads, batch_first=True).double()
    torch.nn.init.normal_(mha.in_proj_bias)
    torch.nn.init.normal_(mha.out_proj.bias)
    emb, mlp = so.make_bias_modules(heads)
    x = torch.randn(sum(sizes), H, dtype=torch.float64)
    return sizes, spds, mha, emb, mlp, x


def _params(mha, emb, mlp):
    return [("mha." + n, p) for n, p in mha.named_parameters()] + [("emb." + n, p) for n, p in emb.named_parameters()] + \
        [("mlp." + n, p) for n, p in mlp.named_parameters()]


@pytest.mark.parametrize("heads,d", [(1, 4), (4, 16), (2, 12)])
def test_ragged_oracle_equals_padded_multihead_attention_with_the_references_mask(heads, d):
    by = {g[0]: g for g in so.GRAPHS}
    graphs = [by[k] for k in ("one-node", "two-isolated", "path-5", "two-components-7", "cycle-6-chord", "loops-and-duplicates")]
    sizes, spds, mha, emb, mlp, x = _case(graphs, heads, d, 3)
    gy = torch.cos(torch.arange(x.numel(), dtype=torch.float64)).reshape(x.shape)
    res = []
    for fn in (so.padded_biased_attention, so.ragged_biased_mha):
        for _, p in _params(mha, emb, mlp):
            p.grad = None
        xi = x.clone().requires_grad_(True)
        out = fn(mha, emb, mlp, xi, sizes, spds)
        out.backward(gy)
        res.append((out.detach(), xi.grad, {n: p.grad.clone() for n, p in _params(mha, emb, mlp)}))
    (o_ref, gx_ref, gp_ref), (o_mine, gx_mine, gp_mine) = res
    assert float((o_ref - o_mine).abs().max()) <= TOL and float((gx_ref - gx_mine).abs().max()) <= TOL
    for n in gp_ref:
        assert float((gp_ref[n] - gp_mine[n]).abs().max()) <= TOL * max(1.0, float(gp_ref[n].abs().max())), n
    for gp in (gp_ref, gp_mine):
        assert not gp["emb.weight"][so.NO_PATH].any(), "padding_idx: row 100 takes no gradient"
        assert gp["mlp.4.bias"].abs().max() > 0
        assert heads == 1 or gp["emb.weight"][:4].abs().max() > 0      # (one head: a width-1 ReLU MLP may be dead at this seed)
        assert not gp["emb.weight"][7:so.NO_PATH].any(), "no pair of these graphs lies that far apart"


def test_table_form_equals_per_pair_form_with_mask_and_q_k_v_gradients():
    heads, d, p = 4, 16, 0.5
    by = {g[0]: g for g in so.GRAPHS}
    _, sizes, flat = so.collate([by["path-5"], by["two-components-7"], by["path-104"]])
    spds = so.split_spd(flat, sizes)
    torch.manual_seed(5)
    emb, mlp = so.make_bias_modules(heads)
    qkv = torch.randn(sum(sizes), 3 * heads * d, dtype=torch.float64)
    keep = [(torch.rand(heads, n, n) >= p) for n in sizes]
    gy = torch.sin(torch.arange(sum(sizes) * heads * d, dtype=torch.float64)).reshape(sum(sizes), heads * d)
    res = []
    for form in ("pair", "table"):
        emb.zero_grad()
        mlp.zero_grad()
        x = qkv.clone().requires_grad_(True)
        bias = [so.pair_bias(emb, mlp, s) for s in spds] if form == "pair" else so.table_bias(so.bias_table(emb, mlp), spds)
        out, lse = so.ragged_biased_attention(x, sizes, heads, bias, keep, p)
        out.backward(gy)
        res.append((out.detach(), lse.detach(), x.grad, emb.weight.grad.clone(), [q.grad.clone() for q in mlp.parameters()]))
    a, b = res
    assert float((a[0] - b[0]).abs().max()) <= TOL and float((a[1] - b[1]).abs().max()) <= TOL and float((a[2] - b[2]).abs().max()) <= TOL
    assert float((a[3] - b[3]).abs().max()) <= TOL * max(1.0, float(a[3].abs().max()))
    for ga, gb in zip(a[4], b[4]):
        assert float((ga - gb).abs().max()) <= TOL * max(1.0, float(ga.abs().max()))
    assert not a[3][so.NO_PATH].any() and not b[3][so.NO_PATH].any()
    assert a[3][99].abs().max() > 0, "path-104 reaches distance 99"
    # a zero table is the unbiased attention
    zero = so.table_bias(torch.zeros(so.ROWS, heads, dtype=torch.float64), spds)
    assert torch.equal(so.ragged_biased_attention(qkv, sizes, heads, zero)[0], go.ragged_attention(qkv, sizes, heads)[0])
    # bytes above 100 read row 100
    over = [s.clone() for s in spds]
    over[1][over[1] == so.NO_PATH] = 255
    t = so.bias_table(emb, mlp).detach()
    assert torch.equal(so.ragged_biased_attention(qkv, sizes, heads, so.table_bias(t, over))[0],
                       so.ragged_biased_attention(qkv, sizes, heads, so.table_bias(t, spds))[0])


# ---- driver and model -------------------------------------------------------------------------------------------------------------
def test_driver_accepts_the_biased_types_and_refuses_the_rest():
    import esc_gnn_amd.run_zinc_gps as rg
    assert len(rg.LAYER_TYPES) == 6
    assert rg.BIASED_LAYER_TYPES == ("GINE+BiasedTransformer", "CustomGatedGCN+BiasedTransformer", "PNA+BiasedTransformer")
    assert not set(rg.LAYER_TYPES) & set(rg.BIASED_LAYER_TYPES)
    for name in rg.BIASED_LAYER_TYPES:
        assert rg.layer_type_of(name) == (name.split("+")[0], "BiasedTransformer")
        assert rg.build_parser().parse_args(["--gt_layer_type", name]).gt_layer_type == name
        assert name in rg.build_parser().format_help().replace("\n", " ").replace("  ", " ") or name.split("+")[0] in rg.build_parser().format_help()
    for name in rg.LAYER_TYPES:
        assert rg.layer_type_of(name) == tuple(name.split("+"))
    with pytest.raises(SystemExit) as err:
        rg.layer_type_of("GINE+Performer")
    assert all(name in str(err.value) for name in rg.LAYER_TYPES + rg.BIASED_LAYER_TYPES) and "GINE+Performer" in str(err.value)
    with pytest.raises(SystemExit):
        rg.layer_type_of("GINE+BigBird")
    assert rg.build_parser().parse_args([]).gt_layer_type == "GINE+Transformer"


@pytest.mark.parametrize("local", ["GINE", "CustomGatedGCN", "PNA"])
def test_biased_model_has_the_transformer_state_dict(local):
    from esc_gnn_amd.gps_models import GPSLayer, GPSModel
    torch.manual_seed(2)
    plain = GPSModel(layers=2, dim_hidden=16, n_heads=2, local_gnn_type=local, global_model_type="Transformer").state_dict()
    torch.manual_seed(2)
    model = GPSModel(layers=2, dim_hidden=16, n_heads=2, local_gnn_type=local, global_model_type="BiasedTransformer")
    biased = model.state_dict()
    assert list(plain) == list(biased) and all(torch.equal(plain[k], biased[k]) for k in plain)
    assert model.has_attention and all(layer.global_model_type == "BiasedTransformer" for layer in model.layers)
    layer = model.layers[0]
    table = layer.bias_table()
    assert tuple(table.shape) == (so.ROWS, 2)
    want = so.bias_table(layer.edge_attn_emb, layer.edge_attn_linear)
    assert torch.equal(table, want)
    table.sum().backward()
    assert not layer.edge_attn_emb.weight.grad[so.NO_PATH].any() and layer.edge_attn_emb.weight.grad[:so.NO_PATH].abs().min() >= 0
    assert layer.edge_attn_linear[4].bias.grad.abs().max() > 0
    with pytest.raises(ValueError, match="Unsupported global x-former model: Performer"):
        GPSLayer(16, 2, global_model_type="Performer")


def test_biased_layer_names_the_missing_key():
    from esc_gnn_amd.gps_models import GPSLayer

    class NoKeys(object):
        def __contains__(self, key):
            return False
    class Local(torch.nn.Module):
        def forward(self, h, edge_index, edge_attr, plan):
            return torch.zeros_like(h)
    layer = GPSLayer(16, 2, global_model_type="BiasedTransformer")
    layer.local_model = Local()
    layer.norm1_local = torch.nn.Identity()
    NoKeys.edge_index = None
    with pytest.raises(ValueError, match=r"spd\.add_spd.*SPDTable"):
        layer(torch.zeros(3, 16), torch.zeros(0, 16), NoKeys(), None, None, None)


def test_ops_refuse_before_any_launch():
    from esc_gnn_amd import ops
    ei = torch.zeros((2, 0), dtype=torch.int64)
    ptr = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.graph_spd(ei, ptr, ptr)
    with pytest.raises(TypeError, match="int64 \\[2, E\\]"):
        ops.graph_spd(ei.int(), ptr, ptr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spd_gather(torch.zeros(4, dtype=torch.uint8), ptr, ptr, [0], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(TypeError, match="uint8"):
        ops.spd_gather(torch.zeros(4), ptr, ptr, [0], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.graph_attention(torch.zeros(1, 12), torch.zeros(2, dtype=torch.int32), 1, spd=torch.zeros(1, dtype=torch.uint8),
                            bias_table=torch.zeros(101, 1))
