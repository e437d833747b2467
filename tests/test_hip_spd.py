"""The shortest-path attention bias on the GPU: esc_graph_spd byte for byte against the oracle of tests/spd_oracle.py (alone, in a
batch, graph-local and batch ids, the word-count boundaries and the node limit), its skip contract, SPDTable against add_spd; the
biased ragged attention against the fp64 oracle (forward, lse, d_qkv and the table's gradient; dropout with the kernel's own
mask, column slices, an asymmetric byte matrix, bytes above 100, a saturated softmax, bit stability, a zero table against the
unbiased op); GPSModel('BiasedTransformer') against the oracle model; the driver.

Error measure of out / lse / d_qkv: max |got - want| over the largest |want|, bound 1e-5 (tests/test_hip_gps.py's).  The table's
gradient sums up to G n^2 terms per bin: its bound is max(1e-5, 4 x the distance of torch's fp32 evaluation of the same oracle on
the CPU from fp64), measured per case (the factor 4 covers another summation order); both figures are printed."""
import contextlib
import io
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import gps_oracle as go
import loss_cases as lc
import spd_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 1e-5
FILL = 0xAB
ALL = so.GRAPHS + so.DEVICE_GRAPHS
BY = {g[0]: g for g in ALL}


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def ranges(graphs):
    node_ptr = np.cumsum([0] + [g[1] for g in graphs]).astype(np.int64)
    edge_ptr = np.cumsum([0] + [g[2].shape[1] for g in graphs]).astype(np.int64)
    return node_ptr, edge_ptr


def run_spd(E, graphs, local=False, **kw):
    ei, sizes, want = so.collate(graphs)
    if local:
        ei = np.concatenate([g[2] for g in graphs], 1) if graphs else ei
    node_ptr, edge_ptr = ranges(graphs)
    got = E.ops.graph_spd(dev(ei, torch.int64), dev(node_ptr), dev(edge_ptr), edges_local=local, **kw)
    return got.cpu().numpy(), want


# ---- 1. distances -------------------------------------------------------------------------------------------------------------------
def test_limits(E):
    assert E.ops.graph_spd_limits() == (so.MAX_NODES, None)
    assert E.ops.attention_bias_max_nodes(16) >= 222 and all(E.ops.attention_bias_max_nodes(d) >= 64 for d in range(4, 65, 4))


@pytest.mark.parametrize("name", [g[0] for g in ALL])
def test_distances_of_every_graph_alone(E, name):
    for local in (False, True):
        got, want = run_spd(E, [BY[name]], local=local)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, local)
    got, want = run_spd(E, [BY[name]], max_nodes=BY[name][1], num_nodes=BY[name][1], num_pairs=BY[name][1] ** 2)      # nothing read back
    assert np.array_equal(got, want)


def test_the_list_as_one_batch_in_either_id_space(E):
    order = [ALL[i] for i in (11, 0, 8, 1, 2, 9, 3, 4, 10, 5, 6, 7)]          # 256 first, every word count mixed in one launch
    for local in (False, True):
        got, want = run_spd(E, order, local=local)
        assert np.array_equal(got, want), local
    got32, _ = run_spd(E, ALL[:8], max_nodes=104)                            # the two-word kernel on graphs of one word and two
    assert np.array_equal(got32, so.collate(ALL[:8])[2])
    # int32 offsets are taken too
    ei, sizes, want = so.collate(ALL[:5])
    node_ptr, edge_ptr = ranges(ALL[:5])
    got = E.ops.graph_spd(dev(ei), dev(node_ptr, torch.int32), dev(edge_ptr, torch.int32))
    assert np.array_equal(got.cpu().numpy(), want)


def test_nothing_to_do_and_graphs_without_edges_are_legal(E):
    empty = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    for ptr in ([0], [0, 0], [0, 0, 0, 0]):
        assert E.ops.graph_spd(empty, dev(ptr, torch.int64), dev(ptr, torch.int64), max_nodes=0, num_nodes=0, num_pairs=0).shape == (0,)
        assert E.ops.graph_spd(empty, dev(ptr, torch.int32), dev(ptr, torch.int32)).shape == (0,)
    nv = E._native
    nv.call("esc_graph_spd", None, None, 0, None, None, None, 0, 0, 0, 0, 0, None, nv.stream())
    got = E.ops.graph_spd(empty, dev([0, 3, 3, 5], torch.int64), dev([0, 0, 0, 0], torch.int64)).cpu().numpy()      # E == 0, an empty graph between
    want = np.concatenate([(100 * (1 - np.eye(3))).reshape(-1), (100 * (1 - np.eye(2))).reshape(-1)]).astype(np.uint8)
    assert np.array_equal(got, want)


def raw_spd(E, ei, node_ptr, edge_ptr, sizes, max_nodes, pairs=None, local=0):
    nv = E._native
    pair_ptr = np.cumsum([0] + [n * n for n in sizes]).astype(np.int64)
    total = int(pair_ptr[-1])
    out = torch.full((total + 64,), FILL, dtype=torch.uint8, device=DEV)
    src, dst = dev(ei[0].copy(), torch.int64), dev(ei[1].copy(), torch.int64)        # (every operand held until the result is back)
    np_d, ep_d, pp_d = dev(node_ptr, torch.int64), dev(edge_ptr, torch.int64), dev(pair_ptr)
    nv.call("esc_graph_spd", nv.ptr(src), nv.ptr(dst), src.numel(), nv.ptr(np_d), nv.ptr(ep_d), nv.ptr(pp_d), len(sizes), int(sum(sizes)),
            total if pairs is None else pairs, local, max_nodes, nv.ptr(out), nv.stream())
    res = out.cpu().numpy()
    assert (res[total:] == FILL).all(), "bytes behind the buffer's stated room were written"
    return res[:total]


def test_a_graph_that_contradicts_the_host_is_skipped_and_the_limit_is_refused(E):
    pick = [BY["path-5"], BY["random-65"], BY["two-components-7"]]
    ei, sizes, want = so.collate(pick)
    node_ptr, edge_ptr = ranges(pick)
    lo, hi = 25, 25 + 65 * 65

    def check(out, skipped, what):
        for g, (a, b) in enumerate(((0, lo), (lo, hi), (hi, hi + 49))):
            if g == skipped:
                assert (out[a:b] == FILL).all(), "%s: the skipped graph was written" % what
            else:
                assert np.array_equal(out[a:b], want[a:b]), "%s: graph %d beside it" % (what, g)
    check(raw_spd(E, ei, node_ptr, edge_ptr, sizes, 65), None, "nothing wrong")
    check(raw_spd(E, ei, node_ptr, edge_ptr, sizes, 64), 1, "more nodes than max_nodes")            # 65 nodes, the host said 64
    check(raw_spd(E, ei, node_ptr, edge_ptr, sizes, 7), 1, "more nodes than max_nodes")
    bad = ei.copy()
    bad[1, int(edge_ptr[2]) + 1] = 2                                                                 # an edge of the last graph ends in the first
    check(raw_spd(E, bad, node_ptr, edge_ptr, sizes, 65), 2, "an edge end outside the graph")
    check(raw_spd(E, ei, node_ptr, edge_ptr, sizes, 65, pairs=hi + 20), 2, "pair bytes beyond the buffer's room")
    nv = E._native
    limit = so.MAX_NODES
    big = ("path-257", limit + 1, so._both(so._path(limit + 1)))
    with pytest.raises(RuntimeError, match="exceeds the limit of %d nodes per graph" % limit):
        run_spd(E, [big])
    with pytest.raises(RuntimeError, match=r"esc_graph_spd: a graph of 257 nodes exceeds the limit of 256 nodes per graph \(esc_graph_spd_max_nodes\)"):
        nv.call("esc_graph_spd", None, None, 0, None, None, None, 1, limit + 1, (limit + 1) ** 2, 0, limit + 1, None, nv.stream())
    got, want1 = run_spd(E, [BY["random-256"]])                                                      # a valid call after the refusals
    assert np.array_equal(got, want1)


def test_table_attach_equals_add_spd_on_the_collated_batch(E):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
    from esc_gnn_amd.spd import SPDTable, add_spd
    graphs = build_feature_dataset(synthetic_zinc_graphs(0, 12), 3, use_rd=True, self_loop=True)
    store = E.DeviceGraphStore(graphs, DEV)
    table = SPDTable(store)
    n = (store.h_node_ptr[1:] - store.h_node_ptr[:-1]).tolist()
    assert table.spd.dtype == torch.uint8 and table.spd.shape == (sum(v * v for v in n),)
    for ids in (torch.arange(0, 6), torch.tensor([11, 4, 4, 7, 0, 9])):
        batch = table.attach(store.collate(ids), ids)
        other = add_spd(store.collate(ids))
        assert batch.attn_bias.dtype == torch.uint8 and torch.equal(batch.attn_bias, other.attn_bias)
        want = np.concatenate([so.spd_bfs(n[g], graphs[g].edge_index.numpy()).reshape(-1) for g in ids.tolist()])
        assert np.array_equal(batch.attn_bias.cpu().numpy(), want)
    single = add_spd(E.Data(x=graphs[2].x.to(DEV), edge_index=graphs[2].edge_index.to(DEV)))
    assert np.array_equal(single.attn_bias.cpu().numpy(), so.spd_bfs(n[2], graphs[2].edge_index.numpy()).reshape(-1))
    ids = torch.tensor([11, 4, 4, 7, 0, 9])
    for wrong in ([11, 4, 4, 7, 0, 12], [11, -1, 4, 7, 0, 9]):
        with pytest.raises(IndexError, match="graph id out of range"):
            table.attach(store.collate(ids), torch.tensor(wrong))
    with pytest.raises(ValueError, match="graph ids for a batch of"):
        table.attach(store.collate(ids), ids[:3])


# ---- 2. biased attention against the oracle -------------------------------------------------------------------------------------------
HEADS = [(1, 4), (4, 16), (2, 12), (1, 64)]
ZINC = [("zinc-%d" % n, n, so._random_sparse(n, 40 + n, 3)) for n in (23, 30, 37)]
BATCHES = {"one-node": [BY["one-node"]], "small": [BY["one-node"], BY["two-isolated"], BY["path-5"], BY["two-components-7"]], "zinc": ZINC,
           "64-65": [BY["random-64"], BY["random-65"]]}


def large_graph(E, d):
    """one graph above 256 nodes where the biased limit at this head_dim allows it, else one graph at the limit"""
    limit = E.ops.attention_bias_max_nodes(d)
    n = 260 if limit > 256 else limit
    return ("large-%d" % n, n, so._random_sparse(n, 77, 16))


def graph_ptr(sizes):
    return torch.tensor(go.graph_ptr_of(sizes), dtype=torch.int32, device=DEV)


def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    top = float(want.abs().max()) if want.numel() else 0.0
    if top == 0.0:
        return 0.0 if not bool(got.any()) else float("inf")
    return float((got - want).abs().max()) / top


_REFS = {}


def reference(tag, graphs, heads, d, keep=None, p=0.0, spd=None, table=None):
    """inputs (fp32: unit-variance qkv, a table of standard deviation 1, upstream gradient cos(arange)) and the oracle's out / lse /
    d_qkv / d_table in fp64 and in fp32 on the CPU: computed once per case, shared, never modified"""
    key = (tag, heads, d, p)
    if key not in _REFS:
        _, sizes, flat = so.collate(graphs)
        flat = flat if spd is None else spd
        spds = so.split_spd(flat, sizes)
        N, H = sum(sizes), heads * d
        gen = torch.Generator().manual_seed(lc.seed_of("spd-%s-%d-%d" % (tag.split("/")[0], heads, d)))
        qkv = torch.randn((N, 3 * H), generator=gen)
        tab = torch.randn((so.ROWS, heads), generator=gen) if table is None else table
        gy = torch.cos(torch.arange(N * H, dtype=torch.float64)).reshape(N, H).float()
        res = []
        for dtype in (torch.float64, torch.float32):
            x = qkv.clone().to(dtype).requires_grad_(True)
            t = tab.clone().to(dtype).requires_grad_(True)
            out, lse = so.ragged_biased_attention(x, sizes, heads, so.table_bias(t, spds), keep, p)
            out.backward(gy.to(dtype))
            res.append((out.detach(), lse.detach(), x.grad, t.grad))
        _REFS[key] = (qkv, tab, gy, sizes, torch.as_tensor(flat)) + tuple(res)
    return _REFS[key]


def check(what, got, want64, want32, table=False):
    e, e32 = rel(got, want64), rel(want32, want64)
    bound = max(BOUND, 4.0 * e32) if table else BOUND
    print("%-44s kernel %.3g   torch fp32 on the CPU %.3g   bound %.3g" % (what, e, e32, bound))
    assert e <= bound, "%s: %.3g of the largest value, bound %g (torch fp32: %.3g)" % (what, e, bound, e32)


def run_op(E, qkv, tab, flat, sizes, heads, **kw):
    x = qkv.to(DEV).detach().requires_grad_(True)
    t = tab.to(DEV).detach().requires_grad_(True)
    res = E.ops.graph_attention(x, graph_ptr(sizes), heads, max_nodes=max(sizes), return_aux=True, spd=flat.to(DEV), bias_table=t, **kw)
    return x, t, res


def compare(E, name, ref, heads, **kw):
    qkv, tab, gy, sizes, flat, (o64, l64, g64, t64), (o32, l32, g32, t32) = ref
    x, t, (out, lse, mask) = run_op(E, qkv, tab, flat, sizes, heads, **kw)
    out.backward(gy.to(DEV))
    check(name + " out", out, o64, o32)
    check(name + " lse", lse, l64, l32)
    check(name + " d_qkv", x.grad, g64, g32)
    check(name + " d_table", t.grad, t64, t32, table=True)
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(t.grad).all()) and t.grad.shape == (so.ROWS, heads)
    return out, x.grad, t.grad, mask


@pytest.mark.parametrize("heads,d", HEADS)
@pytest.mark.parametrize("tag", list(BATCHES) + ["large"])
def test_forward_and_backward_against_the_oracle(E, tag, heads, d):
    graphs = [large_graph(E, d)] if tag == "large" else BATCHES[tag]
    ref = reference(tag, graphs, heads, d)
    _, _, d_table, mask = compare(E, "%s %dx%d" % (tag, heads, d), ref, heads)
    assert mask is None
    seen = torch.zeros(so.ROWS, dtype=torch.bool)
    seen[ref[4].long().clamp(max=100).unique()] = True
    assert not bool(d_table.cpu()[~seen].any()), "a distance no pair has takes no gradient"


def test_dropout_with_the_kernels_own_mask(E):
    heads, d, p = 4, 16, 0.5
    graphs = BATCHES["zinc"] + BATCHES["64-65"]
    qkv, tab, gy, sizes, flat = reference("drop/inputs", graphs, heads, d)[:5]
    x, t, (out, lse, mask) = run_op(E, qkv, tab, flat, sizes, heads, p=p, training=True, seed=1234)
    keep = go.unpack_mask(mask.cpu(), sizes, heads)
    frac = float(torch.cat([k.reshape(-1) for k in keep]).float().mean())
    assert abs(frac - 0.5) < 0.02, frac
    ref = reference("drop/masked", graphs, heads, d, keep=keep, p=p)
    out.backward(gy.to(DEV))
    for what, got, i in (("out", out, 0), ("lse", lse, 1), ("d_qkv", x.grad, 2)):
        check("dropout " + what, got, ref[5][i], ref[6][i])
    check("dropout d_table", t.grad, ref[5][3], ref[6][3], table=True)
    x2, t2, (out2, _, mask2) = run_op(E, qkv, tab, flat, sizes, heads, p=p, training=True, seed=1234)
    out2.backward(gy.to(DEV))
    used = heads * sum(n * n for n in sizes)                                       # (the buffer has room for N * max_nodes pairs per head)
    assert torch.equal(mask[:used], mask2[:used]) and torch.equal(out, out2) and torch.equal(x.grad, x2.grad) and torch.equal(t.grad, t2.grad)
    # the same seed draws the unbiased op's mask: the bias moves no index
    plain = E.ops.graph_attention(qkv.to(DEV), graph_ptr(sizes), heads, p=p, training=True, seed=1234, max_nodes=max(sizes), return_aux=True)
    assert torch.equal(plain[2][:used], mask[:used])


def test_column_slices_of_wider_buffers(E):
    heads, d = 4, 16
    qkv, tab, gy, sizes, flat, (o64, l64, g64, t64), (o32, l32, g32, t32) = reference("zinc", BATCHES["zinc"], heads, d)
    H, N = heads * d, sum(sizes)
    wide = torch.full((N, 3 * H + 12), float("nan"), device=DEV)
    wide[:, 4:4 + 3 * H] = qkv.to(DEV)
    x = wide.requires_grad_(True)
    t = tab.to(DEV).requires_grad_(True)
    out = E.ops.graph_attention(x[:, 4:4 + 3 * H], graph_ptr(sizes), heads, max_nodes=max(sizes), spd=flat.to(DEV), bias_table=t)
    gwide = torch.full((N, H + 8), float("nan"), device=DEV)
    gwide[:, 8:] = gy.to(DEV)
    out.backward(gwide[:, 8:])
    check("slice out", out, o64, o32)
    check("slice d_qkv", x.grad[:, 4:4 + 3 * H], g64, g32)
    check("slice d_table", t.grad, t64, t32, table=True)
    assert not bool(x.grad[:, :4].any()) and not bool(x.grad[:, 4 + 3 * H:].any())


def test_a_zero_table_is_the_unbiased_op_bit_for_bit(E):
    for (heads, d), tag in (((4, 16), "zinc"), ((2, 12), "64-65"), ((1, 64), "small")):
        qkv, _, gy, sizes, flat = reference(tag, BATCHES[tag], heads, d)[:5]
        x, t, (out, lse, _) = run_op(E, qkv, torch.zeros(so.ROWS, heads), flat, sizes, heads)
        out.backward(gy.to(DEV))
        y = qkv.to(DEV).requires_grad_(True)
        out0, lse0, _ = E.ops.graph_attention(y, graph_ptr(sizes), heads, max_nodes=max(sizes), return_aux=True)
        out0.backward(gy.to(DEV))
        assert torch.equal(out, out0) and torch.equal(lse, lse0) and torch.equal(x.grad, y.grad), (heads, d)


def test_an_asymmetric_byte_matrix_and_bytes_above_100(E):
    heads, d = 4, 16
    _, sizes, flat = so.collate(BATCHES["zinc"])
    rng = np.random.RandomState(5)
    asym = rng.randint(0, 12, size=flat.shape).astype(np.uint8)                     # any byte matrix: no symmetry, no zero diagonal
    at, n = 23 * 23, 30
    m = asym[at:at + n * n].reshape(n, n)
    assert not np.array_equal(m, m.T)
    compare(E, "asymmetric spd", reference("asym", BATCHES["zinc"], heads, d, spd=asym), heads)
    over = flat.copy()
    sel = rng.rand(over.size) < 0.3
    over[sel] = rng.randint(101, 256, size=int(sel.sum())).astype(np.uint8)
    as100 = over.copy()
    as100[sel] = 100
    ref = reference("over-100", BATCHES["zinc"], heads, d, spd=as100)
    qkv, tab, gy, _, _ = ref[:5]
    out, gx, gt, _ = compare(E, "bytes above 100 as 100", ref[:4] + (torch.as_tensor(over),) + ref[5:], heads)
    x, t, (out100, _, _) = run_op(E, qkv, tab, torch.as_tensor(as100), sizes, heads)
    out100.backward(gy.to(DEV))
    assert torch.equal(out, out100) and torch.equal(gx, x.grad) and torch.equal(gt, t.grad)
    assert bool(gt[100].any())


def test_a_huge_table_entry_saturates_and_stays_finite(E):
    heads, d = 4, 16
    table = torch.zeros(so.ROWS, heads)
    table[1] = torch.tensor([3e4, -3e4, 1e3, 0.0])                                 # neighbours take everything / nothing
    qkv, _, gy, sizes, flat = reference("zinc", BATCHES["zinc"], heads, d)[:5]
    x, t, (out, lse, _) = run_op(E, qkv, table, flat, sizes, heads)
    out.backward(gy.to(DEV))
    assert all(bool(torch.isfinite(v).all()) for v in (out, lse, x.grad, t.grad))
    # a node with a neighbour: head 0's row is carried by its pairs at distance 1, head 1's has lost them.  (No comparison with the
    # oracle here: at a score of 3e4 one fp32 ulp is 2e-3, and torch's own fp32 evaluation lies 3e-4 from fp64.)
    has = torch.cat([(s == 1).any(1) for s in so.split_spd(flat, sizes)]).to(DEV)
    assert bool(has.any()) and bool(((lse[0][has] - 3e4).abs() < 60).all()) and bool((lse[0][~has] < 100).all()) and bool((lse[1] < 100).all())


def test_two_runs_give_identical_bits(E):
    for (heads, d), tag in (((4, 16), "zinc"), ((1, 64), "64-65")):
        qkv, tab, gy, sizes, flat = reference(tag, BATCHES[tag], heads, d)[:5]
        runs = []
        for _ in range(2):
            x, t, (out, lse, _) = run_op(E, qkv, tab, flat, sizes, heads)
            out.backward(gy.to(DEV))
            runs.append((out.detach(), lse, x.grad, t.grad))
        assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_limits_are_refused_on_the_host(E):
    heads, d = 1, 64
    limit = E.ops.attention_bias_max_nodes(d)
    n = limit + 1
    assert n <= E.ops.attention_max_nodes(d)
    x = torch.zeros((n, 3 * d), device=DEV)
    spd = torch.zeros(n * n, dtype=torch.uint8, device=DEV)
    tab = torch.zeros((so.ROWS, heads), device=DEV)
    with pytest.raises(RuntimeError, match="exceeds the limit of %d nodes per graph at head_dim 64 with the shortest-path bias" % limit):
        E.ops.graph_attention(x, graph_ptr([n]), heads, max_nodes=n, spd=spd, bias_table=tab)
    E.ops.graph_attention(x, graph_ptr([n]), heads, max_nodes=n)                   # the unbiased op still takes it
    nv, gp = E._native, graph_ptr([n])
    with pytest.raises(RuntimeError, match=r"esc_graph_attention_bias_fwd: a graph of %d nodes exceeds the limit of %d nodes per graph at "
                                           r"head_dim 64 \(esc_graph_attention_bias_max_nodes\)" % (n, limit)):
        nv.call("esc_graph_attention_bias_fwd", nv.ptr(x), 3 * d, nv.ptr(gp), nv.ptr(E.ops._pair_ptr(gp)), nv.ptr(spd), n * n, nv.ptr(tab), 1, n,
                0, n, heads, d, 0.0, 0, nv.ptr(x), d, nv.ptr(x), None, nv.stream())
    with pytest.raises(ValueError, match="come together"):
        E.ops.graph_attention(x, gp, heads, max_nodes=n, spd=spd)
    with pytest.raises(ValueError, match=r"bias_table must be \[101, heads = 1\]"):
        E.ops.graph_attention(x, gp, heads, max_nodes=n, spd=spd, bias_table=torch.zeros((100, 1), device=DEV))
    with pytest.raises(TypeError, match="uint8"):
        E.ops.graph_attention(x, gp, heads, max_nodes=n, spd=spd.int(), bias_table=tab)


def test_nothing_to_do_is_legal(E):
    for sizes in ([], [0], [0, 0, 0]):
        x = torch.zeros((0, 3 * 64), device=DEV, requires_grad=True)
        t = torch.ones((so.ROWS, 4), device=DEV, requires_grad=True)
        out = E.ops.graph_attention(x, graph_ptr(sizes), 4, max_nodes=0, spd=torch.zeros(0, dtype=torch.uint8, device=DEV), bias_table=t)
        out.sum().backward()
        assert out.shape == (0, 64) and x.grad.shape == (0, 192) and t.grad.shape == (so.ROWS, 4) and not bool(t.grad.any())


# ---- 3. layer and model ---------------------------------------------------------------------------------------------------------------
def _close(a, b, what, tol):
    """tests/test_hip_gps.py's measure: max error over max(1, largest value)"""
    a, b = a.detach().cpu().double(), b.detach().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    print("%-48s max scaled error %.3g" % (what, err))
    assert a.shape == b.shape and err <= tol, "%s: max scaled error %.3g > %g" % (what, err, tol)


def test_model_against_the_oracle_model(E):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
    from esc_gnn_amd.gps_models import GPSModel
    from esc_gnn_amd.spd import add_spd
    graphs = build_feature_dataset(synthetic_zinc_graphs(0, 3), 3, use_rd=True, self_loop=True)
    torch.manual_seed(7)
    oracle = so.GPSModel(layers=2, dim_hidden=16, n_heads=2)
    for m in oracle.modules():                             # weights that make every term count
        if isinstance(m, torch.nn.BatchNorm1d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, std=0.1)
        if isinstance(m, torch.nn.MultiheadAttention):
            torch.nn.init.normal_(m.in_proj_bias, std=0.1)
            torch.nn.init.normal_(m.out_proj.bias, std=0.1)
    for layer in oracle.layers:                            # ... the bias MLP's ReLUs alive at every distance
        for lin in (layer.edge_attn_linear[0], layer.edge_attn_linear[2]):
            torch.nn.init.uniform_(lin.bias, 0.5, 1.0)
    mine = GPSModel(layers=2, dim_hidden=16, n_heads=2, dropout=0.0, attn_dropout=0.0, global_model_type="BiasedTransformer")
    mine.load_state_dict(oracle.state_dict())
    plain = GPSModel(layers=2, dim_hidden=16, n_heads=2, dropout=0.0, attn_dropout=0.0, global_model_type="Transformer")
    plain.load_state_dict(oracle.state_dict())
    mine, plain = mine.to(DEV), plain.to(DEV)
    oracle = oracle.double()
    batch = E.Batch.from_data_list([g for g in graphs])
    cpu = {k: batch[k].cpu() for k in ("x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
    cpu["attn_bias"] = torch.as_tensor(np.concatenate([so.spd_bfs(g.x.size(0), g.edge_index.numpy()).reshape(-1) for g in graphs]))
    y = torch.tensor([0.3, -1.1, 0.7], dtype=torch.float64).view(-1, 1)
    for mode in ("train", "eval"):
        getattr(oracle, mode)()
        getattr(mine, mode)()
        oracle.zero_grad()
        mine.zero_grad()
        want = oracle(cpu)
        (want - y).abs().mean().backward()
        data = add_spd(batch.to(DEV))
        assert torch.equal(data.attn_bias.cpu(), cpu["attn_bias"])
        got = mine(data)
        E.ops.l1_loss(got, y.float().to(DEV)).backward()
        _close(got, want, mode + " prediction", 1e-5)
        ref_p, ref_b = dict(oracle.named_parameters()), dict(oracle.named_buffers())
        biased = 0
        for n, p in mine.named_parameters():
            assert ref_p[n].grad is not None and p.grad is not None, n
            _close(p.grad, ref_p[n].grad, mode + " grad " + n, 1e-4)
            if "edge_attn" in n:
                biased += 1
                assert bool(p.grad.any()), n
            if n.endswith("edge_attn_emb.weight"):
                assert not bool(p.grad[so.NO_PATH].any()) and not bool(ref_p[n].grad[so.NO_PATH].any()), "padding_idx: row 100 takes no gradient"
        assert biased == 2 * 7
        for n, b in mine.named_buffers():
            _close(b, ref_b[n], mode + " buffer " + n, 1e-4)
    with pytest.raises(ValueError, match=r"spd\.add_spd"):                           # (eval: the layers before the check move no statistic)
        mine.eval()(E.Batch.from_data_list([g for g in graphs]).to(DEV))
    plain.train()
    E.ops.l1_loss(plain(add_spd(E.Batch.from_data_list([g for g in graphs]).to(DEV))), y.float().to(DEV)).backward()
    unused = [n for n, p in plain.named_parameters() if p.grad is None]
    assert len(unused) == 2 * 7 and all("edge_attn" in n for n in unused), "under Transformer the two modules stay gradient-free"


# ---- 4. driver --------------------------------------------------------------------------------------------------------------------
def test_driver_runs_with_the_biased_transformer(tmp_path, monkeypatch):
    require_gpu()
    import esc_gnn_amd.run_zinc_gps as rg
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rg.main("--gt_layer_type GINE+BiasedTransformer --synthetic_graphs 24 --epochs 1 --layers 2 --batch_size 8 --num_warmup_epochs 1 "
                "--save_appendix _spd".split())
    out = buf.getvalue()
    lines = re.findall(r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)", out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    assert re.search(r"SPD table build time cost: [\d.eE+-]+s", out), out
    keys = set(torch.load(tmp_path / "results" / "zinc_GPS_spd" / "model_checkpoint1.pth", map_location="cpu"))
    assert "layers.0.edge_attn_emb.weight" in keys and "layers.1.edge_attn_linear.4.bias" in keys
    assert os.path.exists(tmp_path / "results" / "zinc_GPS_spd" / "log.txt")
