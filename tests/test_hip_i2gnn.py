"""The I2GNN baseline on the MI355X: the second-root expansion kernels (csrc/subgraphs.hip, esc_subgraph2_*) against the
reference goldens and the numpy oracle, rd against scipy's pseudo-inverse, the collated batch of the reference, the pooling and
gate kernels (csrc/i2pool.hip) against torch, zinc_cycle_models.I2GNN against the reference golden and an fp64 oracle, the
error paths and the run_zinc_cycle driver."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from conftest import require_gpu
import i2gnn_oracle as io
from test_i2gnn_cpu import INT_FIELDS, i2gnn_golden_runs, load_collate_i2gnn3, subgraph2_golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PTRS = ("sub_node_ptr", "sub_edge_ptr", "sub2_ptr", "s2_node_ptr")


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _graph(E, n, ei, x=None, edge_attr=None, y=None):
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64).reshape(2, -1)
    return E.Data(x=torch.arange(n) if x is None else torch.as_tensor(x), edge_index=ei,
                  edge_attr=torch.arange(ei.size(1)) % 4 if edge_attr is None else torch.as_tensor(edge_attr),
                  y=torch.zeros(n, 4) if y is None else torch.as_tensor(y), num_nodes=n)


def _sym(pairs):
    return np.array([[a for a, b in pairs] + [b for a, b in pairs], [b for a, b in pairs] + [a for a, b in pairs]], dtype=np.int64).reshape(2, -1)


def _ring(rng, n, chords):
    pairs = [(i, (i + 1) % n) for i in range(n)] if n > 2 else ([(0, 1)] if n == 2 else [])
    pairs += [(int(a), int(b)) for a, b in rng.randint(0, n, (chords, 2)) if a != b]
    return _sym(pairs)


def _expand(E, graphs, h, **kw):
    from esc_gnn_amd.subgraphs2 import collate_graphs, expand_subgraphs2
    return expand_subgraphs2(collate_graphs(graphs, DEV), h, **kw)


def _check_integers(sub, want, what=""):
    """every integer output of expand_subgraphs2 against the oracle's expansion of the same batch"""
    for k in INT_FIELDS + PTRS + ("batch", "subgraph_to_graph"):
        got = sub[k].cpu().numpy()
        assert got.dtype == np.int64 and got.shape == want[k].shape and np.array_equal(got, want[k]), (what, k)
    assert np.array_equal(sub.node_to_original_node.cpu().numpy(), want["orig_node"]), what
    assert sub.num_subgraphs == want["sub_node_ptr"].shape[0] - 1 and sub.num_subgraphs2 == want["center_idx"].shape[0]
    assert int(sub.status.abs().sum()) == 0, what


def _rd_close(got, ref, atol):
    """the rule of test_hip_ngnn.test_rd_against_scipy_pinv: |got - ref| <= 2^-23 |ref| + atol"""
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    err, bound = np.abs(got - ref), 2.0 ** -23 * np.abs(ref) + atol
    assert got.shape == ref.shape and bool((err <= bound).all()), (float((err - bound).max()), int(np.argmax(err - bound)))
    return float((err / bound).max())


# ---- 1. expansion ----------------------------------------------------------------------------------------------------------
def test_expansion_against_reference_golden(E):
    """every integer field exact; rd within 2^-23 |ref| + atol, atol = 10 x the largest fp64 difference between rd from
    numpy.linalg.pinv and from scipy.linalg.pinv (the reference's call) over these very subgraphs, measured here"""
    cases = list(subgraph2_golden_cases())
    diff = 0.0
    for name, n, ei, h, want in cases:
        a, b = io.expand_graph2(n, ei[0], ei[1], h, True), io.expand_graph2(n, ei[0], ei[1], h, True, pinv=np.linalg.pinv)
        diff = max(diff, float(np.abs(a["rd64"] - b["rd64"]).max()))
    atol = 10.0 * diff
    print("rd: numpy-vs-scipy fp64 difference %.3g -> atol %.3g" % (diff, atol))
    assert 0 < atol < 1e-9
    worst = 0.0
    for name, n, ei, h, want in cases:
        sub = _expand(E, [_graph(E, n, ei)], h, use_rd=True)
        for k in INT_FIELDS:
            got = sub[k].cpu().numpy()
            assert got.shape == want[k].shape and np.array_equal(got, want[k]), (name, k)
        assert np.array_equal(sub.x.cpu().numpy(), want["orig_node"])             # x = arange(n): the original ids
        assert np.array_equal(sub.node_to_original_node.cpu().numpy(), want["orig_node"])
        rd = sub.rd.cpu().numpy()
        assert rd.dtype == np.float32
        worst = max(worst, _rd_close(rd, want["rd"], atol))
        ci = want["center_idx"]
        assert bool((rd[ci[:, 0], 0] == 0).all()) and bool((rd[ci[:, 1], 1] == 0).all()), name      # R(a, a) is exactly 0
        assert int(sub.status.abs().sum()) == 0
    print("rd: worst error / bound %.3g over %d cases" % (worst, len(cases)))
    assert len(cases) >= 12


@pytest.fixture(scope="module")
def fresh_graphs(E):
    """directed graphs (asymmetric reach), an isolated root (K = 0) first and last, a self loop at a root, a repeated edge from
    a root, graphs smaller than h (h above the diameter), a one-node graph, n in {63, 64, 65, 130} (wavefront boundaries, more
    than two ballot chunks of nodes and of edges), and 30 molecules so that the batch has more than 1024 roots (the scan's chunk)"""
    from esc_gnn_amd.datasets import synthetic_zinc_graphs
    rng = np.random.RandomState(17)
    gs = [(5, np.zeros((2, 0), dtype=np.int64)), (1, np.zeros((2, 0), dtype=np.int64)), (1, np.array([[0], [0]], dtype=np.int64))]
    for n in (2, 3, 63, 64, 65, 130):
        gs.append((n, _ring(rng, n, n // 8)))
    gs.append((10, _sym([(1, 3), (3, 7)])))                                                    # isolated nodes
    gs.append((30, np.stack([rng.randint(0, 30, 60), rng.randint(0, 30, 60)]).astype(np.int64)))     # directed
    gs.append((66, np.stack([rng.randint(0, 66, 140), rng.randint(0, 66, 140)]).astype(np.int64)))   # directed, three edge chunks
    loops = np.concatenate([_sym([(0, 1), (1, 2), (2, 0), (2, 3), (4, 5)]), np.array([[0, 3, 1, 1, 7], [0, 3, 2, 2, 7]])], axis=1)
    gs.append((8, loops))                                                                    # self loops, a repeated edge
    gs += [(int(d.num_nodes), d.edge_index.numpy()) for d in synthetic_zinc_graphs(100, 30)]
    gs.append((3, np.zeros((2, 0), dtype=np.int64)))
    assert sum(n for n, _ in gs) > 1024 + 64
    return gs


@pytest.mark.parametrize("h", [1, 2, 3], ids=lambda h: "h%d" % h)
def test_expansion_fresh_sweep_against_oracle(E, fresh_graphs, h):
    from esc_gnn_amd.subgraphs2 import subgraph2_sizes
    gs = fresh_graphs
    want = io.expand_batch2([n for n, _ in gs], [ei for _, ei in gs], h)
    graphs = [_graph(E, n, ei) for n, ei in gs]
    sub = _expand(E, graphs, h)
    _check_integers(sub, want, what="h=%d" % h)
    sizes, largest = subgraph2_sizes(graphs, h, with_largest=True)
    node_ptr = np.cumsum([0] + [n for n, _ in gs])
    assert sizes.dtype == torch.int64 and sizes.device.type == "cpu" and sizes.shape == (len(gs), 3)
    for col, k in enumerate(("sub_node_ptr", "sub_edge_ptr", "sub2_ptr")):
        assert np.array_equal(sizes[:, col].numpy(), np.diff(want[k][node_ptr])), k
    per_root = np.diff(want["sub_node_ptr"]) // np.diff(want["sub2_ptr"])
    assert largest == int(per_root.max())
    again = _expand(E, graphs, h, sizes=sizes)                                 # the store's path: totals from the host
    assert torch.equal(again.z, sub.z) and torch.equal(again.edge_index, sub.edge_index) and torch.equal(again.center_idx, sub.center_idx)


def test_labels_reach_2h_plus_5_and_no_further_on_a_directed_chain(E):
    """The largest label at the largest h.  A second-root label cannot pass 2h + 5 on any graph, directed ones included: the
    sub-edge root -> j puts the root one step from j, and every node of the subgraph reaches the root inside it within h steps
    (so there is no graph whose label reaches 100, and no status for it).  A directed chain of 47 nodes into node 0, which
    shares a 2-cycle with node 1, meets the bound at h = 47: the chain's far end is 47 steps behind root 0 and 48 steps behind
    its neighbour 1.  Graphs on both sides check the offsets."""
    h = 47
    pairs = [(0, 1), (1, 0), (2, 0)] + [(k + 1, k) for k in range(2, 48)]
    ei = np.array([[a for a, b in pairs], [b for a, b in pairs]], dtype=np.int64)
    side = _sym([(0, 1), (1, 2)])
    want = io.expand_batch2([4, 49, 4], [side, ei, side], h)
    sub = _expand(E, [_graph(E, 4, side), _graph(E, 49, ei), _graph(E, 4, side)], h)
    _check_integers(sub, want, "chain")
    assert int(sub.z.max()) == 2 * h + 5 == 99 and sub.status.cpu().tolist() == [0, 0, 0]


# ---- 2. rd on large subgraphs ----------------------------------------------------------------------------------------------
def test_rd_both_columns_up_to_96_nodes(E):
    rng = np.random.RandomState(9)
    gs = [(m, _ring(rng, m, m // 6)) for m in (33, 64, 96)]                      # h = m: every subgraph is the whole graph
    gs.append((24, np.stack([rng.randint(0, 24, 60), rng.randint(0, 24, 60)]).astype(np.int64)))
    h = 47
    counts, lists = [n for n, _ in gs], [ei for _, ei in gs]
    want = io.expand_batch2(counts, lists, h, use_rd=True)
    other = io.expand_batch2(counts, lists, h, use_rd=True, pinv=np.linalg.pinv)
    atol = 10.0 * float(np.abs(want["rd64"] - other["rd64"]).max())
    print("rd: numpy-vs-scipy fp64 difference %.3g -> atol %.3g; largest |rd| %.3g" % (atol / 10, atol, float(np.abs(want["rd64"]).max())))
    assert 0 < atol < 1e-9
    sub = _expand(E, [_graph(E, n, ei) for n, ei in gs], h, use_rd=True)
    _check_integers(sub, want, "rd graphs")
    assert 96 in set(int(v) for v in np.diff(want["sub_node_ptr"]) // np.diff(want["sub2_ptr"]))
    print("rd: worst error / bound %.3g" % _rd_close(sub.rd.cpu().numpy(), want["rd"], atol))


# ---- 3. the collated batch -------------------------------------------------------------------------------------------------
def test_collate_i2gnn3_equals_the_reference_batch_without_a_host_copy(E):
    from esc_gnn_amd.subgraphs2 import I2GraphStore, collate_graphs, expand_subgraphs2, subgraph2_sizes
    raws, want, h = load_collate_i2gnn3()
    graphs = [_graph(E, r["x"].shape[0], r["edge_index"], r["x"], r["edge_attr"], r["y"]) for r in raws]
    sizes = subgraph2_sizes(graphs, h)                                       # once, at dataset build
    assert sizes.sum(dim=0).tolist() == [want["x"].shape[0], want["edge_index"].shape[1], want["center_idx"].shape[0]]
    batch = collate_graphs(graphs, DEV)
    store = I2GraphStore(graphs, h, True, DEV)
    sbatch = store.collate([0, 1, 2])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                  # any device-to-host copy that waits now raises
    try:
        sub = expand_subgraphs2(batch, h, True, sizes)
        sub2 = store.expand(sbatch)
        with pytest.raises(RuntimeError):                                    # the probe is live: without `sizes` the totals are read back
            expand_subgraphs2(batch, h, True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in ("x", "z", "node_to_subgraph2", "subgraph2_to_subgraph", "center_idx", "edge_index", "edge_attr", "subgraph_to_graph",
              "batch", "node_to_original_node", "orig_node", "orig_edge", "y"):
        got = sub[k].cpu().numpy()
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), k
        assert torch.equal(sub2[k], sub[k]), k
    ref = io.expand_batch2([r["x"].shape[0] for r in raws], [r["edge_index"] for r in raws], h, use_rd=True)
    other = io.expand_batch2([r["x"].shape[0] for r in raws], [r["edge_index"] for r in raws], h, use_rd=True, pinv=np.linalg.pinv)
    atol = 10.0 * float(np.abs(ref["rd64"] - other["rd64"]).max())
    _rd_close(sub.rd.cpu().numpy(), want["rd"], atol)
    for k in PTRS:
        assert np.array_equal(sub[k].cpu().numpy(), ref[k]), k
    assert int(sub.status.abs().sum()) == 0 and sub.num_subgraphs2 == 154
    # the pre-filled pooling caches are the pointers themselves
    assert torch.equal(E.ops._seg_ptr(sub.node_to_subgraph2, 154).long(), sub.s2_node_ptr)
    assert torch.equal(E.ops._seg_ptr(sub.subgraph2_to_subgraph, sub.num_subgraphs).long(), sub.sub2_ptr)


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------
def test_rd_above_96_nodes_raises_at_store_build_and_names_the_limit(E):
    from esc_gnn_amd.subgraphs2 import I2GraphStore
    g = _graph(E, 97, _sym([(0, k) for k in range(1, 97)]))                   # a star: at h = 2 every subgraph is all 97 nodes
    with pytest.raises(ValueError, match="at most 96 nodes"):
        I2GraphStore([g], 2, True, DEV)                                       # at build, not inside a step
    with pytest.raises(ValueError, match="use_rd, a subgraph of more than 96 nodes") as err:
        _expand(E, [g], 2, use_rd=True)
    assert "node id" not in str(err.value)
    store = I2GraphStore([g], 2, False, DEV)                                  # without rd the same subgraphs are fine
    # the hub has 96 neighbours, every leaf one: 192 copies of 97 nodes and 192 sub-edges
    assert store.largest_subgraph == 97 and store.sizes.tolist() == [[192 * 97, 192 * 192, 192]]
    assert store.expand(store.collate([0])).z.shape == (192 * 97, 4)


@pytest.mark.parametrize("h", [0, 48])
def test_h_outside_1_to_47(E, h):
    from esc_gnn_amd import _native as nv
    g = _graph(E, 4, _sym([(0, 1), (1, 2)]))
    with pytest.raises(ValueError, match="1..47"):
        _expand(E, [g], h)
    ptrs = torch.tensor([0, 4], device=DEV)
    ei = g.edge_index.to(DEV)
    out = torch.zeros(5, dtype=torch.int64, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"outside 1\.\.47"):                # the entry point itself
        nv.call("esc_subgraph2_count", nv.ptr(ptrs), nv.ptr(ptrs), nv.ptr(ei[0].contiguous()), nv.ptr(ei[1].contiguous()), 1, 4, 4, 4,
                h, nv.ptr(out), nv.ptr(out), nv.ptr(out), nv.ptr(st), nv.stream())


def test_bad_node_id_is_erange_and_writes_nothing_for_that_graph(E):
    from esc_gnn_amd import _native as nv
    from esc_gnn_amd.subgraphs2 import collate_graphs, expand_subgraphs2
    rng = np.random.RandomState(4)
    graphs = [_graph(E, 6, _ring(rng, 6, 2)), _graph(E, 7, _ring(rng, 7, 2)), _graph(E, 5, _ring(rng, 5, 1))]
    batch = collate_graphs(graphs, DEV)
    e_bad = int(graphs[0].edge_index.size(1)) + 3
    batch.edge_index[1, e_bad] = 13                                           # the first node of the NEXT graph
    with pytest.raises(ValueError, match="graph 1 .*node id outside the graph"):
        expand_subgraphs2(batch, 2)
    sub = expand_subgraphs2(batch, 2, check=False)
    assert sub.status.cpu().tolist() == [0, nv.ESC_ERANGE, 0]
    for k in ("sub_node_ptr", "sub_edge_ptr", "sub2_ptr"):
        assert bool((np.diff(sub[k].cpu().numpy())[6:13] == 0).all()), k
    good = io.expand_batch2([6, 5], [graphs[0].edge_index.numpy(), graphs[2].edge_index.numpy()], 2)
    total, s2 = int(sub.sub_node_ptr[-1]), int(sub.sub2_ptr[-1])
    assert total == good["orig_node"].shape[0] and s2 == good["center_idx"].shape[0]      # nothing of graph 1 among the rows
    got = sub.orig_node[:total].cpu().numpy()
    assert np.array_equal(got, np.where(good["orig_node"] >= 6, good["orig_node"] + 7, good["orig_node"]))
    assert np.array_equal(sub.z[:total].cpu().numpy(), good["z"]) and np.array_equal(sub.center_idx[:s2].cpu().numpy(), good["center_idx"])
    assert np.array_equal(sub.s2_node_ptr[:s2 + 1].cpu().numpy(), good["s2_node_ptr"])


def test_unsupported_arguments_raise_and_name_themselves(E):
    g = _graph(E, 4, _sym([(0, 1), (1, 2)]))
    for kw, name in ((dict(self_loop=True), "self_loop"), (dict(node_label="drnl"), "node_label"),
                     (dict(max_nodes_per_hop=3), "max_nodes_per_hop"), (dict(subgraph_pretransform=lambda d: d), "subgraph_pretransform")):
        with pytest.raises((NotImplementedError, ValueError), match=name):
            _expand(E, [g], 2, **kw)
    from esc_gnn_amd.engine import zinc_engine_supports
    from esc_gnn_amd.zinc_cycle_models import I2GNN
    assert zinc_engine_supports(I2GNN(None, num_layers=2).to(DEV)) is False


# ---- 5. pooling and gate kernels ---------------------------------------------------------------------------------------------
LENS = [1, 3, 0, 5, 2, 67]
CENTER_SIDE = [(0, 0), (0, 2), None, (1, 1), (0, 1), (3, 66)]     # local rows: length 1; side = last row; empty; centre == side


def _segments():
    ptr = np.cumsum([0] + LENS)
    ci = np.array([[ptr[s] + cs[0], ptr[s] + cs[1]] if cs is not None else [0, 0] for s, cs in enumerate(CENTER_SIDE)], dtype=np.int64)
    seg = np.repeat(np.arange(len(LENS)), LENS)
    return torch.tensor(ptr, dtype=torch.int64), torch.tensor(ci), torch.tensor(seg, dtype=torch.int64)


@pytest.mark.parametrize("C", [1, 3, 64, 65])
@pytest.mark.parametrize("pad", [0, 3], ids=["dense", "strided"])
def test_pool_mean_center_side(E, C, pad):
    """Forward: centre and side parts are copies (bit-equal); the mean is a sequential fp32 sum of len terms and one division,
    so |got - fp64| <= len * 2^-23 * mean|x| (each of the len - 1 additions and the division rounds once, relative to a partial
    sum of at most sum|x|).  Backward against torch autograd in fp64: a row that is neither centre nor side holds the single
    term dout_mean / len, one fp32 division — bit-equal to torch's fp32 quotient; the others add up to two terms (two more
    roundings).  ld > C on both inputs is the `strided` case."""
    ptr, ci, seg = _segments()
    N, S = int(ptr[-1]), len(LENS)
    g = torch.Generator().manual_seed(100 * C + pad)
    xw = torch.randn(N, C + pad, generator=g) * 3
    x = xw[:, :C]
    xd = xw.to(DEV)[:, :C].requires_grad_(True)
    assert pad == 0 or not xd.is_contiguous()
    out = E.ops.pool_mean_center_side(xd, ptr.to(DEV), ci.to(DEV), seg.to(DEV))
    assert out.shape == (S, 3 * C)
    got = out.detach().cpu()
    x64 = x.double().requires_grad_(True)
    parts = []
    for s in range(S):
        a, b = int(ptr[s]), int(ptr[s + 1])
        if a == b:
            parts.append(torch.zeros(3 * C, dtype=torch.float64))
        else:
            parts.append(torch.cat([x64[a:b].mean(dim=0), x64[ci[s, 0]], x64[ci[s, 1]]]))
    ref = torch.stack(parts)
    nonempty = torch.tensor([n > 0 for n in LENS])
    assert torch.equal(got[nonempty][:, C:2 * C], x[ci[nonempty][:, 0]]) and torch.equal(got[nonempty][:, 2 * C:], x[ci[nonempty][:, 1]])
    assert bool((got[~nonempty] == 0).all())
    for s in range(S):
        if LENS[s]:
            a, b = int(ptr[s]), int(ptr[s + 1])
            bound = LENS[s] * 2.0 ** -23 * x[a:b].abs().double().mean(dim=0)
            assert bool(((got[s, :C].double() - ref[s, :C].detach()).abs() <= bound).all()), s
    dw = torch.randn(S, 3 * C + pad, generator=g)
    dout = dw[:, :3 * C]
    out.backward(dw.to(DEV)[:, :3 * C])
    ref.backward(dout.double())
    dx, dx64 = xd.grad.cpu(), x64.grad
    single = torch.ones(N, dtype=torch.bool)
    single[ci[nonempty].reshape(-1)] = False
    lens_row = torch.tensor(LENS, dtype=torch.float32)[seg]
    assert bool(single.any()) and torch.equal(dx[single], dout[seg][single][:, :C] / lens_row[single].view(-1, 1))
    terms = (dout[seg][:, :C] / lens_row.view(-1, 1)).abs() + dout[seg][:, C:2 * C].abs() + dout[seg][:, 2 * C:].abs()
    assert bool(((dx.double() - dx64).abs() <= 3 * 2.0 ** -24 * terms.double()).all())
    # centre == side receives BOTH terms (segments 0 and 3), and every row is written: raw call on a NaN-filled buffer
    for s in (0, 3):
        r = int(ci[s, 0])
        assert int(ci[s, 1]) == r
        want = (dout[s, :C] / LENS[s] + dout[s, C:2 * C]) + dout[s, 2 * C:]
        assert torch.equal(dx[r], want), s
    from esc_gnn_amd import _native as nv
    raw = torch.full((N, C + pad), float("nan"), device=DEV)
    dd, pd, cd, sd = dw.to(DEV), ptr.to(DEV), ci.to(DEV), seg.to(DEV)
    nv.call("esc_pool_mean_center_side_bwd", nv.ptr(dd), 3 * C + pad, nv.ptr(pd), cd.data_ptr(), cd.data_ptr() + 8, 2, nv.ptr(sd), N, C,
            nv.ptr(raw), C + pad, nv.stream())
    assert torch.equal(raw.cpu()[:, :C], dx) and (pad == 0 or bool(torch.isnan(raw.cpu()[:, C:]).all()))


@pytest.mark.parametrize("M,C,pad", [(1, 1, 0), (7, 3, 2), (33, 64, 0), (130, 65, 1)])
def test_sigmoid_mul(E, M, C, pad):
    """y = sigmoid(a) * x and both gradients against fp64 at the bound tests/test_hip_csl.py holds the ELU kernel to,
    |error| <= 1e-6 |ref| + 1e-7; a = +-100 (exp(100) overflows fp32) and x = 0 included; nothing is NaN or inf."""
    g = torch.Generator().manual_seed(M * 1000 + C)
    aw, xw = torch.randn(M, C + pad, generator=g) * 4, torch.randn(M, C + pad, generator=g) * 3
    specials = [(100.0, 2.5), (-100.0, 2.5), (100.0, 0.0), (-100.0, 0.0), (0.0, 0.0), (0.0, -1.5), (15.0, 3.0), (-15.0, 3.0), (88.0, 1.0), (-88.0, 1.0)]
    for k, (av, xv) in enumerate(specials):
        r, c = divmod((k * 7919) % (M * C), C)
        aw[r, c], xw[r, c] = av, xv                     # M * C = 1 keeps the last one: every special is covered by a larger shape
    a, x = aw[:, :C], xw[:, :C]
    ad, xd = aw.to(DEV)[:, :C].requires_grad_(True), xw.to(DEV)[:, :C].requires_grad_(True)
    y = E.ops.sigmoid_mul(ad, xd)
    dy = torch.randn(M, C, generator=g)
    y.backward(dy.to(DEV))
    a64, x64 = a.double().requires_grad_(True), x.double().requires_grad_(True)
    y64 = torch.sigmoid(a64) * x64
    y64.backward(dy.double())
    for what, mine, ref in (("forward", y.detach().cpu(), y64.detach()), ("da", ad.grad.cpu(), a64.grad), ("dx", xd.grad.cpu(), x64.grad)):
        assert bool(torch.isfinite(mine).all()), what
        err, bound = (mine.double() - ref).abs(), 1e-6 * ref.abs() + 1e-7
        print("sigmoid_mul %s M=%d C=%d: worst error / bound %.3g" % (what, M, C, float((err / bound).max())))
        assert bool((err <= bound).all()), (what, float((err / bound).max()))
    if M * C > len(specials):
        assert float(y.detach().cpu()[a == 100.0][0]) == 2.5           # sigmoid(100) is 1 in fp32


def test_group_mean_and_gather_over_an_unsorted_index(E):
    """the context mean and the gather back over node_to_original_node: one grouping, both directions"""
    g = torch.Generator().manual_seed(3)
    idx = torch.randint(0, 37, (500,), generator=g)
    idx[:37] = torch.randperm(37, generator=g)                                  # every key occurs
    x = torch.randn(500, 64, generator=g)
    xd, idxd = x.to(DEV).requires_grad_(True), idx.to(DEV)
    plan = E.ops.group_plan(idxd, 37)
    assert E.ops.group_plan(idxd, 37) is plan                                   # built once per index tensor
    mean = E.ops.group_mean(xd, plan)
    back = E.ops.gather_rows(mean, plan)
    x64 = x.double().requires_grad_(True)
    m64 = torch.zeros(37, 64, dtype=torch.float64).index_add_(0, idx, x64) / torch.bincount(idx, minlength=37).double().view(-1, 1)
    b64 = m64[idx]
    assert float((mean.detach().cpu().double() - m64.detach()).abs().max()) <= 1e-5
    assert torch.equal(back.detach().cpu(), mean.detach().cpu()[idx])           # the gather is a copy
    w = torch.randn(500, 64, generator=g)
    (back * w.to(DEV)).sum().backward()
    (b64 * w.double()).sum().backward()
    assert float((xd.grad.cpu().double() - x64.grad).abs().max()) <= 1e-5 * max(1.0, float(x64.grad.abs().max()))
    assert int(plan["bad"].item()) == 0


# ---- 6. model ----------------------------------------------------------------------------------------------------------------
def _model_batch(E, b):
    keys = ("x", "edge_index", "edge_attr", "z", "rd", "node_to_subgraph2", "subgraph2_to_subgraph", "subgraph_to_graph", "center_idx",
            "node_to_original_node")
    d = E.Data(**{k: b[k].to(DEV) for k in keys})
    first = np.unique(b["node_to_subgraph2"].numpy(), return_index=True)[1]
    d.s2_node_ptr = torch.tensor(np.r_[first, b["x"].shape[0]], dtype=torch.int64, device=DEV)
    return d


@pytest.mark.parametrize("tag,split", [(t, True) for t in io.CONFIGS] + [("default", False)],
                         ids=lambda v: v if isinstance(v, str) else ("split" if v else "cat"))
def test_i2gnn_against_reference_golden_and_fp64_oracle(E, tag, split):
    """split: the first Linear of double_nns as x W_x + (P W_p)[idx] (the default) or as Linear(cat[x, P[idx]]); both are held
    to the same bounds"""
    from esc_gnn_amd.zinc_cycle_models import I2GNN
    from test_hip_model import _close
    from test_hip_zinc_cycle import _grad_errors
    torch.set_num_threads(1)
    z, b, _ = next(r for r in i2gnn_golden_runs() if r[2] == tag)
    ref = io.i2gnn_from_recipe(z["seed"], z["layers"], tag)
    m = I2GNN(None, num_layers=int(z["layers"]), **io.CONFIGS[tag])
    m.load_state_dict(ref.state_dict())
    m.split_double_linear = split
    m = m.to(DEV).train()
    y = torch.tensor(z["y"])
    out = m(_model_batch(E, b))
    assert out.shape == (int(b["subgraph_to_graph"].numel()), 1)                       # one row per original node
    loss = E.ops.l1_loss(out, y.to(DEV))
    loss.backward()
    _close(out, torch.tensor(z[tag + "/pred"]), "i2gnn predictions " + tag)
    assert abs(float(loss.detach()) - float(z[tag + "/loss"])) <= 1e-5
    ref.train()
    torch.nn.functional.l1_loss(ref(b), y).backward()
    ref64 = copy.deepcopy(ref).double(); ref64.zero_grad()
    p64 = ref64(b)
    l64 = torch.nn.functional.l1_loss(p64, y.double()); l64.backward()
    _close(out, p64, "i2gnn predictions vs fp64 " + tag)
    assert abs(float(loss.detach()) - float(l64.detach())) <= 1e-5 * max(1.0, abs(float(l64.detach())))
    g32 = {n: p.grad for n, p in ref.named_parameters()}
    g64 = {n: p.grad for n, p in ref64.named_parameters()}
    unused = sorted(n for n, g in g64.items() if g is None)
    assert unused == sorted(n for n, p in m.named_parameters() if p.grad is None), unused     # the same parameters are never read
    errs = _grad_errors([(n, p) for n, p in m.named_parameters() if p.grad is not None], g32, g64)
    print("i2gnn %s: worst gradient error vs fp64 %.3g (fp32 oracle %.3g) over %d parameters" % (
        tag, max(e[0] for e in errs.values()), max(e[1] for e in errs.values()), len(errs)))
    bad = {n: e for n, e in errs.items() if e[0] > max(1e-5, 3 * e[1])}
    assert not bad, bad


@pytest.mark.parametrize("p1,p2", [("mean", "add"), ("add", "center"), ("mean-context", "mean")])
def test_i2gnn_remaining_poolings_against_fp64_oracle(E, p1, p2):
    """the pooling modes no recorded configuration uses (the gate on for 'mean'), predictions against the fp64 oracle"""
    from esc_gnn_amd.zinc_cycle_models import I2GNN
    from test_hip_model import _close
    _, b, _ = next(i2gnn_golden_runs())
    kw = dict(subgraph_pooling=p1, subgraph2_pooling=p2, use_pooling_nn=False, use_rd=True, double_pooling=True, gate=True)
    torch.manual_seed(5)
    ref = io.no.perturb(io.I2GNNRef(2, **kw)).train()
    m = I2GNN(None, num_layers=2, **kw)
    m.load_state_dict(ref.state_dict())
    out = m.to(DEV).train()(_model_batch(E, b))
    _close(out, copy.deepcopy(ref).double()(b), "i2gnn %s / %s vs fp64" % (p1, p2))


def test_i2gnn_eval_mode_one_graph_batch(E):
    from esc_gnn_amd.zinc_cycle_models import I2GNN
    from test_hip_model import _close
    z, _, tag = next(i2gnn_golden_runs())                                            # the driver's defaults
    raws, _, h = load_collate_i2gnn3()
    r = raws[1]
    ref = io.i2gnn_from_recipe(z["seed"], z["layers"], tag).eval()
    m = I2GNN(None, num_layers=int(z["layers"]), **io.CONFIGS[tag])
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    sub = _expand(E, [_graph(E, r["x"].shape[0], r["edge_index"], r["x"], r["edge_attr"], r["y"])], h, use_rd=True)
    keys = ("x", "z", "rd", "edge_index", "edge_attr", "node_to_subgraph2", "subgraph2_to_subgraph", "subgraph_to_graph", "center_idx",
            "node_to_original_node")
    with torch.no_grad():
        got = m(sub)
        want = ref({k: sub[k].cpu() for k in keys})
    assert got.shape == (r["x"].shape[0], 1)                                       # one row per original node
    _close(got, want, "one-graph eval")


# ---- 7. driver ---------------------------------------------------------------------------------------------------------------
def test_run_zinc_cycle_i2gnn_two_epochs_and_eval(E, tmp_path, monkeypatch, capsys):
    import esc_gnn_amd.run_zinc_cycle as rc
    monkeypatch.chdir(tmp_path)
    common = "--model I2GNN --synthetic_graphs 48 --epochs 2 --batch_size 16 --layers 2 --h 2 --save_appendix _t".split()
    rc.main(common)
    out = capsys.readouterr().out
    assert "Using I2GNN model" in out and "Epoch: 001" in out and "Validation MAE" in out      # (later epochs are logged when validation improves)
    nums = [float(v) for line in out.splitlines() if line.startswith("Epoch:") for v in re.findall(r"[-+]?\d+\.\d+(?:e[-+]?\d+)?", line)]
    assert nums and all(np.isfinite(v) for v in nums), out
    res = os.path.join(tmp_path, "results", "zinc_I2GNN_t")
    assert "model_checkpoint2.pth" in os.listdir(res) and "log.txt" in os.listdir(res)
    assert "Epoch: 001" in open(os.path.join(res, "log.txt")).read()             # the checkpoint's name counts the epochs run: 2
    sd = torch.load(os.path.join(res, "model_checkpoint2.pth"), map_location="cpu")
    assert sd["rd_projection_list.0.weight"].shape == (9, 2) and sd["double_nns.0.0.weight"].shape == (128, 320)
    assert sd["subgraph_gate.2.0.weight"].shape == (64, 64) and sd["fc1.weight"].shape == (32, 256)
    rc.main(common + ["--eval", "1", "--load_model", os.path.join(res, "model_checkpoint2.pth")])
    out = capsys.readouterr().out
    m = re.search(r"Test MAE: ([-+0-9.e]+)", out)
    assert m and np.isfinite(float(m.group(1))), out
