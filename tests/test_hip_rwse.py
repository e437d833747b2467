"""The random-walk structural encoding on the GPU (csrc/rwse.hip): esc_rw_landing through the op and the C ABI on every graph of
rwse_oracle.GRAPHS, alone and as one ragged batch, against the dense fp64 oracle; bit stability, the leading dimension, limits
and the skip contract clause by clause; RWSETable against add_rwse and the gather's guards; nn.RWSENodeEncoder's forward and
backward against the fp64 oracle module; GPSModel with rwse alone and with lap_pe + rwse against the oracle model; the driver.

Bound of the statistic: |out - fp32(oracle)| <= numpy.spacing(fp32(oracle)) elementwise, one fp32 unit in the last place, and
exact zeros where the oracle is exactly 0.  Derived, not measured: the kernel's fp64 sums differ from the oracle's only in order,
by a few 2^-53 relative, which can move the single fp32 rounding by at most one unit.
Bound of the encoder: 1e-5 of the tensor's largest value (tests/test_hip_lappe.py's measure); of the model: 1e-5 under the
measure tests/test_hip_gps.py holds this model to (the error over max(1, the tensor's largest value)), for the prediction, every
parameter gradient and every buffer."""
import contextlib
import io
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import lappe_oracle as lo
import rwse_oracle as ro

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP_LISTS = {"1..20": ro.KSTEPS, "gapped": ro.GAPPED, "single": ro.SINGLE}
FILL = -7.0


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def mask_of(ks):
    return sum(1 << (k - 1) for k in ks)


_ORACLE, _ALONE = {}, {}


def oracle(i, which):
    """fp64 [n, K] of graph i: computed once, shared, never modified"""
    if (i, which) not in _ORACLE:
        _, n, edges, _ = ro.GRAPHS[i]
        _ORACLE[(i, which)] = ro.rw_landing64(n, edges, STEP_LISTS[which])
    return _ORACLE[(i, which)]


def alone(E, i, which):
    """pestat [n, K] of graph i computed in a launch of its own: once, shared, never modified"""
    if (i, which) not in _ALONE:
        _, n, edges, _ = ro.GRAPHS[i]
        ks = STEP_LISTS[which]
        out = E.ops.rw_landing(dev(edges), dev([0, n], torch.int64), dev([0, edges.shape[1]], torch.int64), ks, max_nodes=n,
                               max_edges=edges.shape[1], num_nodes=n)
        assert out.shape == (n, len(ks)) and out.dtype == torch.float32 and out.is_contiguous()
        _ALONE[(i, which)] = out
    return _ALONE[(i, which)]


def raw_rw(E, edges, node_ptr, edge_ptr, N, max_nodes, max_edges, ks, local=0, ld=None, fill=FILL):
    """the C entry point on a pre-filled output [N, ld]"""
    nv = E._native
    src, dst = dev(edges[0]), dev(edges[1])
    gp, ep = dev(node_ptr, torch.int64), dev(edge_ptr, torch.int64)
    ld = len(ks) if ld is None else ld
    out = torch.full((N, ld), fill, device=DEV)
    nv.call("esc_rw_landing", nv.ptr(src), nv.ptr(dst), src.numel(), nv.ptr(gp), nv.ptr(ep), gp.numel() - 1, N, local, mask_of(ks), max_nodes,
            max_edges, nv.ptr(out), ld, nv.stream())
    return out


def within(name, got, want64):
    ok, worst = ro.within_one_ulp(got.cpu().numpy(), want64)
    print("%-40s largest distance %.3g units in the last place (bound 1)" % (name, worst))
    assert ok, "%s: %.3g units in the last place, or a zero of the oracle that is not exactly 0.0" % (name, worst)


# ---- 1. the statistic -------------------------------------------------------------------------------------------------------------
def test_limits_are_the_ones_the_oracle_assumes(E):
    assert E.ops.rw_landing_limits() == (ro.MAX_NODES, ro.MAX_EDGES)
    assert ro.MAX_NODES >= 256 and ro.MAX_EDGES >= 4096


@pytest.mark.parametrize("which", list(STEP_LISTS))
@pytest.mark.parametrize("i", range(len(ro.GRAPHS)), ids=ro.NAMES)
def test_landing_probabilities_of_every_graph(E, i, which):
    name, n, edges, _ = ro.GRAPHS[i]
    ks = STEP_LISTS[which]
    out = alone(E, i, which)
    within("%s %s" % (name, which), out, oracle(i, which))
    again = E.ops.rw_landing(dev(edges), dev([0, n], torch.int32), dev([0, edges.shape[1]], torch.int32), ks)     # int32 ranges, sizes read back
    assert torch.equal(bits(again), bits(out)), "not bit-identical run to run"
    for local in (0, 1):                                       # one graph from row 0: local and batch ids coincide
        raw = raw_rw(E, edges, [0, n], [0, edges.shape[1]], n, n, edges.shape[1], ks, local=local)
        assert torch.equal(bits(raw), bits(out)), "the C entry point and the op differ"


@pytest.mark.parametrize("which", list(STEP_LISTS))
def test_the_list_as_one_ragged_batch(E, which):
    """every graph inside the batch (an empty graph in the middle and at the end) is within the bound and bit-equal to the same
    graph alone; through the op with batch rows as edge ends and through the C ABI with graph-local ids"""
    ks = STEP_LISTS[which]
    last = len(ro.GRAPHS) - 1
    ei, gp, ep, sizes = ro.batch_of(ro.GRAPHS, empty_after=(7, last))
    assert sizes.count(0) == 2 and sizes[-1] == 0 and sizes[8] == 0
    N = int(gp[-1])
    out = E.ops.rw_landing(dev(ei), dev(gp), dev(ep), ks, max_nodes=ro.MAX_NODES, max_edges=ro.MAX_EDGES, num_nodes=N)
    looked = E.ops.rw_landing(dev(ei), dev(gp), dev(ep), ks)                    # the sizes read back
    assert torch.equal(bits(looked), bits(out))
    local = np.concatenate([g[2] for g in ro.GRAPHS], 1)
    loc = raw_rw(E, local, gp, ep, N, ro.MAX_NODES, ro.MAX_EDGES, ks, local=1)
    at, g = 0, 0
    for n in sizes:
        if n == 0:
            continue
        name = ro.NAMES[g]
        within("batch/%s %s" % (name, which), out[at:at + n], oracle(g, which))
        a = alone(E, g, which)
        assert torch.equal(bits(out[at:at + n]), bits(a)), name + ": alone and inside the batch differ"
        assert torch.equal(bits(loc[at:at + n]), bits(a)), name + " (local ids)"
        at, g = at + n, g + 1
    assert at == N and g == len(ro.GRAPHS)


def test_leading_dimension_leaves_the_other_columns_untouched(E):
    pick = [ro.GRAPHS[ro.NAMES.index(n)] for n in ("petersen", "random-65", "triangle+path-directed")]
    ei, gp, ep, _ = ro.batch_of(pick)
    N = int(gp[-1])
    ks = ro.GAPPED
    me = int(np.diff(ep).max())
    tight = raw_rw(E, ei, gp, ep, N, 65, me, ks)
    wide = raw_rw(E, ei, gp, ep, N, 65, me, ks, ld=len(ks) + 5)
    assert torch.equal(bits(wide[:, :len(ks)]), bits(tight)) and bool((wide[:, len(ks):] == FILL).all())
    nv = E._native
    buf = torch.full((N, 3 + len(ks)), FILL, device=DEV)       # a column slice of a wider buffer
    src, dst, gp_d, ep_d = dev(ei[0]), dev(ei[1]), dev(gp, torch.int64), dev(ep, torch.int64)
    nv.call("esc_rw_landing", nv.ptr(src), nv.ptr(dst), ei.shape[1], nv.ptr(gp_d), nv.ptr(ep_d), 3, N, 0, mask_of(ks), 65, me, buf[:, 3:].data_ptr(),
            buf.stride(0), nv.stream())
    assert torch.equal(bits(buf[:, 3:]), bits(tight)) and bool((buf[:, :3] == FILL).all())
    with pytest.raises(RuntimeError, match="leading dimension of out 5 below the 6 steps"):
        raw_rw(E, ei, gp, ep, N, 65, me, ks, ld=5)


# ---- 2. limits and robustness -----------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host(E):
    n = ro.MAX_NODES + 1
    edges = lo._both(lo._path(n))
    gp, ep = dev([0, n], torch.int64), dev([0, edges.shape[1]], torch.int64)
    ks = ro.KSTEPS
    with pytest.raises(RuntimeError, match="exceeds the limit of %d nodes" % ro.MAX_NODES):
        E.ops.rw_landing(dev(edges), gp, ep, ks, max_nodes=n, max_edges=edges.shape[1], num_nodes=n)
    with pytest.raises(RuntimeError, match="exceeds the limit of %d nodes" % ro.MAX_NODES):     # ... also when the op has to look itself
        E.ops.rw_landing(dev(edges), gp, ep, ks)
    with pytest.raises(RuntimeError, match=r"limit of %d nodes per graph \(esc_rw_landing_max_nodes\)" % ro.MAX_NODES):
        raw_rw(E, edges, [0, n], [0, edges.shape[1]], n, n, edges.shape[1], ks)
    many = ro.random_multigraph(64, ro.MAX_EDGES + 1, 8)
    mp, me = dev([0, 64], torch.int64), dev([0, many.shape[1]], torch.int64)
    with pytest.raises(RuntimeError, match="exceeds the limit of %d edges" % ro.MAX_EDGES):
        E.ops.rw_landing(dev(many), mp, me, ks, max_nodes=64, max_edges=many.shape[1], num_nodes=64)
    with pytest.raises(RuntimeError, match="exceeds the limit of %d edges" % ro.MAX_EDGES):
        E.ops.rw_landing(dev(many), mp, me, ks)
    with pytest.raises(RuntimeError, match=r"limit of %d edges per graph \(esc_rw_landing_max_edges\)" % ro.MAX_EDGES):
        raw_rw(E, many, [0, 64], [0, many.shape[1]], 64, 64, many.shape[1], ks)
    small = lo._both(lo._path(9))
    sp, se = dev([0, 9], torch.int64), dev([0, 16], torch.int64)
    nv = E._native
    out = torch.full((9, 4), FILL, device=DEV)
    s_src, s_dst = dev(small[0]), dev(small[1])
    for mask in (0, -1, -(1 << 63)):
        with pytest.raises(RuntimeError, match="selects no step"):
            nv.call("esc_rw_landing", nv.ptr(s_src), nv.ptr(s_dst), 16, nv.ptr(sp), nv.ptr(se), 1, 9, 0, mask, 9, 16, nv.ptr(out), 4, nv.stream())
    assert bool((out == FILL).all())
    with pytest.raises(TypeError, match="int64"):
        E.ops.rw_landing(dev(small).to(torch.int32), sp, se, ks, max_nodes=9, max_edges=16, num_nodes=9)
    with pytest.raises(TypeError, match="int32 or int64"):
        E.ops.rw_landing(dev(small), sp.float(), se, ks, max_nodes=9, max_edges=16, num_nodes=9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ops.rw_landing(torch.as_tensor(small), sp, se, ks, max_nodes=9, max_edges=16, num_nodes=9)
    got = E.ops.rw_landing(dev(small), sp, se, ks, max_nodes=9, max_edges=16, num_nodes=9)      # a valid call after the refusals is correct
    within("after the refusals", got, ro.rw_landing64(9, small, ks))


def test_a_graph_that_contradicts_the_host_is_skipped(E):
    """clause by clause on a sentinel-filled output: that graph's rows keep the sentinel, its neighbours' rows are right"""
    ks = ro.KSTEPS
    pick = [ro.GRAPHS[ro.NAMES.index(n)] for n in ("triangle", "petersen", "K5")]       # (3, 6), (10, 30), (5, 20) nodes and edges
    ei, gp, ep, _ = ro.batch_of(pick)
    N, Etot = int(gp[-1]), ei.shape[1]
    want = [ro.rw_landing64(n, e, ks) for _, n, e, _ in pick]

    def check(out, skipped, what):
        assert out.shape == (N, len(ks))
        at = 0
        for g, (name, n, _, _) in enumerate(pick):
            if g == skipped:
                assert bool((out[at:at + n] == FILL).all()), "%s: %s was written" % (what, name)
            else:
                within("%s / beside it: %s" % (what, name), out[at:at + n], want[g])
            at += n
    check(raw_rw(E, ei, gp, ep, N, 5, 30, ks), 1, "more nodes than max_nodes")           # petersen has 10 nodes, the host said 5
    check(raw_rw(E, ei, gp, ep, N, 10, 20, ks), 1, "more edges than max_edges")          # ... and 30 edges, the host said 20
    for row in (0, 1):
        bad = ei.copy()
        bad[row, int(ep[2]) + 3] = 1                                                     # an edge of K5 starts / ends in the triangle
        check(raw_rw(E, bad, gp, ep, N, 10, 30, ks), 2, "an edge end outside the graph (row %d)" % row)
    bad = ei.copy()
    bad[1, int(ep[1]) + 7] = N + 1000                                                    # ... and far outside the batch
    check(raw_rw(E, bad, gp, ep, N, 10, 30, ks), 1, "an edge end outside the batch")
    gp2 = gp.copy()
    gp2[3] = gp[2] - 1                                                                   # K5's node range runs backwards
    check(raw_rw(E, ei, gp2, ep, N, 10, 30, ks), 2, "a decreasing node_ptr")
    gp3 = gp.copy()
    gp3[3] = N + 2                                                                       # ... or leaves [0, N)
    check(raw_rw(E, ei, gp3, ep, N, 10, 30, ks), 2, "a node range beyond N")
    ep2 = ep.copy()
    ep2[3] = Etot + 5                                                                    # K5's edge range leaves the list
    check(raw_rw(E, ei, gp, ep2, N, 10, 30, ks), 2, "an edge_ptr beyond E")
    ep3 = ep.copy()
    ep3[3] = ep[2] - 2                                                                   # ... or runs backwards
    check(raw_rw(E, ei, gp, ep3, N, 10, 30, ks), 2, "a decreasing edge_ptr")
    check(raw_rw(E, ei, gp, ep, N, 10, 30, ks), None, "nothing wrong")


def test_nothing_to_do_and_graphs_without_edges_are_legal(E):
    empty = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    ks = ro.KSTEPS
    for ptr in ([0], [0, 0], [0, 0, 0, 0]):
        out = E.ops.rw_landing(empty, dev(ptr, torch.int64), dev(ptr, torch.int64), ks, max_nodes=0, max_edges=0, num_nodes=0)
        assert out.shape == (0, 20)
        assert E.ops.rw_landing(empty, dev(ptr, torch.int32), dev(ptr, torch.int32), ks).shape == (0, 20)
    nv = E._native
    nv.call("esc_rw_landing", None, None, 0, None, None, 0, 0, 0, 1, 0, 0, None, 1, nv.stream())
    out = raw_rw(E, np.zeros((2, 0), dtype=np.int64), [0, 4, 4, 5], [0, 0, 0, 0], 5, 4, 0, ks)      # E == 0: nodes without edges write zeros
    assert bool((out == 0.0).all())
    tri = ro.GRAPHS[ro.NAMES.index("triangle")][2]
    out = raw_rw(E, tri + 2, [0, 2, 5, 9], [0, 0, 6, 6], 9, 4, 6, ks)                               # edgeless graphs around a triangle
    assert bool((out[:2] == 0.0).all()) and bool((out[5:] == 0.0).all())
    within("a triangle between edgeless graphs", out[2:5], ro.rw_landing64(3, tri, ks))


# ---- 3. the resident table and its gather --------------------------------------------------------------------------------------------
def test_table_attach_equals_add_rwse_on_the_collated_batch(E):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
    from esc_gnn_amd.rwse import RWSETable, add_rwse
    graphs = build_feature_dataset(synthetic_zinc_graphs(0, 40), 3, use_rd=True, self_loop=True)
    store = E.DeviceGraphStore(graphs, DEV)
    ks = ro.KSTEPS
    table = RWSETable(store, ks)
    n_all = int(store.h_node_ptr[-1])
    assert table.pestat.shape == (n_all, 20) and table.pestat.dtype == torch.float32
    assert table.max_nodes == int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    assert table.max_edges == int((store.h_edge_ptr[1:] - store.h_edge_ptr[:-1]).max())
    for ids in (torch.arange(0, 8), torch.arange(32, 40), torch.tensor([39, 4, 4, 17, 0, 4, 21])):      # in order, and repeated and permuted
        batch = table.attach(store.collate(ids), ids)
        other = add_rwse(store.collate(ids), ks)
        assert batch.pestat_RWSE.shape == (batch.x.size(0), 20)
        assert torch.equal(bits(batch.pestat_RWSE), bits(other.pestat_RWSE))
        at = 0
        for g in ids.tolist():
            a, b = int(store.h_node_ptr[g]), int(store.h_node_ptr[g + 1])
            assert torch.equal(bits(batch.pestat_RWSE[at:at + b - a]), bits(table.pestat[a:b]))
            at += b - a
        assert at == batch.x.size(0)
    ids = torch.tensor([39, 4, 4, 17, 0, 4, 21])
    batch, at = table.attach(store.collate(ids), ids), 0
    for g in ids.tolist():                                             # ... and it is the statistic of those graphs, self-loops included
        n, edges = graphs[g].x.size(0), graphs[g].edge_index.numpy()
        assert (edges[0] == edges[1]).sum() == n, "the stored edge list carries the appended self-loops"
        within("store graph %d" % g, batch.pestat_RWSE[at:at + n], ro.rw_landing64(n, edges, ks))
        at += n
    single = add_rwse(E.Data(x=graphs[2].x.to(DEV), edge_index=graphs[2].edge_index.to(DEV)), ks)      # one graph, no batch vector
    a, b = int(store.h_node_ptr[2]), int(store.h_node_ptr[3])
    assert torch.equal(bits(single.pestat_RWSE), bits(table.pestat[a:b]))
    for wrong in ([39, 4, 4, 17, 0, 4, 40], [39, 4, -1, 17, 0, 4, 21]):
        with pytest.raises(IndexError, match="graph id out of range"):
            table.attach(store.collate(ids), torch.tensor(wrong))
    with pytest.raises(ValueError, match="graph ids for a batch of"):
        table.attach(store.collate(ids), ids[:3])


def test_gather_guards(E):
    """through the C ABI, past the host's id check: an id out of range, two ranges of different length and ranges that leave
    their arrays each copy nothing for that graph; the other graphs' rows arrive; a leading dimension leaves the rest alone"""
    nv = E._native
    K, sizes = 5, [3, 10, 5]
    n_all = sum(sizes)
    table = torch.rand((n_all, K), device=DEV)
    ptr_all = np.concatenate([[0], np.cumsum(sizes)])

    def gather(ids, graph_ptr, N, node_ptr_all=ptr_all, N_all=n_all, ld=K):
        out = torch.full((N, ld), FILL, device=DEV)
        np_d, ids_d, gp_d = dev(node_ptr_all, torch.int64), dev(ids, torch.int64), dev(graph_ptr, torch.int32)
        nv.call("esc_rwse_gather", nv.ptr(table), nv.ptr(np_d), len(node_ptr_all) - 1, N_all, nv.ptr(ids_d), nv.ptr(gp_d), len(ids), N, K, nv.ptr(out),
                ld, nv.stream())
        return out
    good = gather([2, 0, 1], [0, 5, 8, 18], 18)
    assert torch.equal(good, torch.cat([table[13:18], table[0:3], table[3:13]]))
    wide = gather([2, 0, 1], [0, 5, 8, 18], 18, ld=K + 3)
    assert torch.equal(wide[:, :K], good) and bool((wide[:, K:] == FILL).all())
    for bad_id in (3, -1, 1 << 40):
        out = gather([2, bad_id, 1], [0, 5, 8, 18], 18)
        assert torch.equal(out[:5], good[:5]) and torch.equal(out[8:], good[8:]) and bool((out[5:8] == FILL).all())
    out = gather([2, 0, 1], [0, 5, 9, 18], 18)                          # graph 0 has 3 rows, the batch says 4 - and graph 1 then 9 for 10
    assert torch.equal(out[:5], good[:5]) and bool((out[5:] == FILL).all())
    out = gather([2, 0, 1], [0, 5, 8, 18], 18, node_ptr_all=np.array([0, 3, 13, 19]))       # graph 2's source range: 6 rows for 5
    assert bool((out[:5] == FILL).all()) and torch.equal(out[5:], good[5:])
    out = gather([2, 0, 1], [0, 5, 8, 18], 18, N_all=17)                # graph 2's source rows leave a table of 17 rows
    assert bool((out[:5] == FILL).all()) and torch.equal(out[5:], good[5:])
    out = gather([2, 0, 1], [0, 5, 8, 18], 17)                          # graph 1's target rows leave an output of 17 rows
    assert torch.equal(out[:8], good[:8]) and bool((out[8:] == FILL).all())
    out = gather([2, 0, 1], [-1, 4, 7, 17], 18)                         # a negative target row
    assert bool((out[:4] == FILL).all()) and torch.equal(out[4:17], good[5:]) and bool((out[17:] == FILL).all())
    with pytest.raises(RuntimeError, match=r"steps outside 1\.\.63"):
        gather_k64 = (dev(ptr_all, torch.int64), dev([0], torch.int64), dev([0, 3], torch.int32))
        nv.call("esc_rwse_gather", nv.ptr(table), nv.ptr(gather_k64[0]), 3, n_all, nv.ptr(gather_k64[1]), nv.ptr(gather_k64[2]), 1, 3, 64, nv.ptr(table),
                64, nv.stream())
    with pytest.raises(RuntimeError, match="leading dimension of out 4 below the 5 steps"):
        gather([0], [0, 3], 3, ld=4)
    nv.call("esc_rwse_gather", None, None, 0, 0, None, None, 0, 0, K, None, K, nv.stream())


@pytest.mark.parametrize("k", [1, 63])
def test_gather_of_one_table_in_any_order_and_at_a_leading_dimension(E, k):
    """the shared gather kernel with one table: graphs of 1, 2 and 3 nodes whose rows hold their own flat index, gathered in
    reversed order with a repeat; through the op (ld_out = K) and through the C ABI into a wider, sentinel-filled output"""
    nv = E._native
    table = torch.arange(6 * k, dtype=torch.float32, device=DEV).view(6, k)
    ptr_all, ids, graph_ptr = dev([0, 1, 3, 6], torch.int64), [2, 0, 2], dev([0, 3, 4, 7], torch.int32)
    want = table[torch.tensor([3, 4, 5, 0, 3, 4, 5], device=DEV)]
    out = E.ops.rwse_gather(table, ptr_all, ids, graph_ptr, 7)
    assert out.shape == (7, k) and torch.equal(out, want)
    wide = torch.full((7, k + 3), FILL, device=DEV)
    ids_d = dev(ids, torch.int64)
    nv.call("esc_rwse_gather", nv.ptr(table), nv.ptr(ptr_all), 3, 6, nv.ptr(ids_d), nv.ptr(graph_ptr), 3, 7, k, nv.ptr(wide), k + 3, nv.stream())
    assert torch.equal(wide[:, :k], want) and bool((wide[:, k:] == FILL).all())


# ---- 4. the encoder ---------------------------------------------------------------------------------------------------------------
def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    return err / scale if scale > 0 else (0.0 if err == 0 else math.inf)


def check(what, got, want64, bound=1e-5):
    e = rel(got, want64)
    print("%-60s %.3g of the largest value (bound %g)" % (what, e, bound))
    assert e <= bound, "%s: %.3g of the largest value, bound %g" % (what, e, bound)


SHAPES = [(20, 28), (16, 16), (5, 4), (1, 8)]


@pytest.mark.parametrize("model,layers,raw_norm", [("linear", 1, "batchnorm"), ("linear", 1, "none"), ("mlp", 1, "batchnorm"),
                                                   ("mlp", 2, "batchnorm"), ("mlp", 3, "none")])
@pytest.mark.parametrize("steps,dim_pe", SHAPES)
def test_encoder_forward_and_backward_against_the_oracle(E, steps, dim_pe, model, layers, raw_norm):
    """landing probabilities of real graphs with appended self-loops, the run's shape, as the input (70 rows: petersen, random-65
    cut to its first 60 rows), weights off their defaults, forward and parameter gradients in training and in evaluation mode, the running statistics too"""
    from esc_gnn_amd.nn import RWSENodeEncoder
    ks = list(range(1, steps + 1))
    rows = [ro.rw_landing64(n, ro.with_self_loops(n, e), ks) for _, n, e, _ in (ro.GRAPHS[ro.NAMES.index("petersen")], ro.GRAPHS[ro.NAMES.index("random-65")])]
    pestat = torch.from_numpy(np.concatenate([rows[0], rows[1][:60]])).float()
    torch.manual_seed(100 * steps + dim_pe + layers)
    want = ro.RWSEEncoder(dim_pe, steps, model, layers, raw_norm)
    for q in want.parameters():
        torch.nn.init.normal_(q, std=0.6)
    mine = RWSENodeEncoder(dim_pe, steps, model=model, layers=layers, raw_norm=raw_norm)
    mine.load_state_dict(want.state_dict())
    mine, want = mine.to(DEV), want.double()
    gy = torch.cos(torch.arange(70 * dim_pe, dtype=torch.float64)).reshape(70, dim_pe)
    name = "K %d P %d %s/%d/%s " % (steps, dim_pe, model, layers, raw_norm)
    for mode in ("train", "eval"):
        getattr(mine, mode)()
        getattr(want, mode)()
        mine.zero_grad()
        want.zero_grad()
        o = want(pestat.double())
        o.backward(gy)
        got = mine(E.Data(x=pestat.to(DEV), pestat_RWSE=pestat.to(DEV)))
        got.backward(gy.float().to(DEV))
        assert got.shape == (70, dim_pe)
        check(name + mode + " out", got, o)
        ref = dict(want.named_parameters())
        for k, q in mine.named_parameters():
            check(name + mode + " d " + k, q.grad, ref[k].grad)
        refb = dict(want.named_buffers())
        for k, b in mine.named_buffers():
            if b.dtype.is_floating_point:
                check(name + mode + " " + k, b, refb[k])


# ---- 5. the model -----------------------------------------------------------------------------------------------------------------
def _close(a, b, what, tol):
    """the measure of test_hip_gps's model test: max error over max(1, largest value)"""
    a, b = a.detach().cpu().double(), b.detach().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    print("%-64s max scaled error %.3g" % (what, err))
    assert a.shape == b.shape and err <= tol, "%s: max scaled error %.3g > %g" % (what, err, tol)


@pytest.mark.parametrize("lap_pe", [False, True], ids=["rwse", "lap_pe+rwse"])
def test_model_with_rwse_against_the_oracle_model(E, lap_pe):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
    from esc_gnn_amd.gps_models import GPSModel
    from esc_gnn_amd.lappe import add_lap_pe
    from esc_gnn_amd.rwse import add_rwse
    graphs = build_feature_dataset(synthetic_zinc_graphs(0, 6), 3, use_rd=True, self_loop=True)
    torch.manual_seed(7)
    oracle_m = ro.GPSModel(layers=2, dim_hidden=64, n_heads=4, lap_pe=lap_pe)
    for m in oracle_m.modules():                           # weights that make every term count: biases and BatchNorm affine off their defaults
        if isinstance(m, torch.nn.BatchNorm1d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, std=0.1)
        if isinstance(m, torch.nn.MultiheadAttention):
            torch.nn.init.normal_(m.in_proj_bias, std=0.1)
            torch.nn.init.normal_(m.out_proj.bias, std=0.1)
    mine = GPSModel(layers=2, dim_hidden=64, n_heads=4, dropout=0.0, attn_dropout=0.0, lap_pe=lap_pe, rwse=True)
    mine.load_state_dict(oracle_m.state_dict())
    mine = mine.to(DEV)
    oracle_m = oracle_m.double()
    batch = add_rwse(E.Batch.from_data_list([g for g in graphs]).to(DEV), ro.KSTEPS)
    keys = ["x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch", "pestat_RWSE"]
    signs = None
    if lap_pe:
        batch = add_lap_pe(batch)
        keys += ["EigVecs", "EigVals"]
        signs = torch.tensor([1.0, -1, -1, 1, -1, 1, 1, -1])
        mine.encoder.node_encoder.encoder2.signs_override = signs
    cpu = {k: batch[k].cpu() for k in keys}
    at = 0
    for g in graphs:                                       # the statistics the oracle is fed are the device's own - and they are right
        n = g.x.size(0)
        within("model batch", batch.pestat_RWSE[at:at + n], ro.rw_landing64(n, g.edge_index.numpy(), ro.KSTEPS))
        at += n
    y = torch.tensor([0.3, -1.1, 0.7, 0.2, -0.4, 1.3], dtype=torch.float64).view(-1, 1)
    rw = "encoder.node_encoder.encoder%d." % (3 if lap_pe else 2)
    for mode in ("train", "eval"):
        getattr(oracle_m, mode)()
        getattr(mine, mode)()
        oracle_m.zero_grad()
        mine.zero_grad()
        want = oracle_m(cpu, signs)
        (want - y).abs().mean().backward()
        got = mine(batch)
        E.ops.l1_loss(got, y.float().to(DEV)).backward()
        _close(got, want, mode + " prediction", 1e-5)
        ref_p, ref_b = dict(oracle_m.named_parameters()), dict(oracle_m.named_buffers())
        unused = 0
        for n, p in mine.named_parameters():
            if ref_p[n].grad is None:                      # edge_attn_emb / edge_attn_linear: in the state_dict, not in the forward
                assert "edge_attn" in n and p.grad is None, n
                unused += 1
                continue
            _close(p.grad, ref_p[n].grad, mode + " grad " + n, 1e-5)
        assert unused == 2 * 7
        named = dict(mine.named_parameters())
        assert float(named[rw + "pe_encoder.weight"].grad.abs().max()) > 0 and float(named[rw + "raw_norm.weight"].grad.abs().max()) > 0
        for n, b in mine.named_buffers():
            _close(b, ref_b[n], mode + " buffer " + n, 1e-5)
    bare = E.Batch.from_data_list([g for g in graphs]).to(DEV)
    if lap_pe:
        bare = add_lap_pe(bare)
    with pytest.raises(ValueError, match="Precomputed 'pestat_RWSE' variable is required"):
        mine(bare)


# ---- 6. the driver ----------------------------------------------------------------------------------------------------------------
COMMON = "--synthetic_graphs 48 --epochs 1 --batch_size 8 --layers 2"
LINE = r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)"


def _run(argv):
    import esc_gnn_amd.run_zinc_gps as rg
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rg.main(argv.split())
    return buf.getvalue()


@pytest.fixture(scope="module")
def driver_dir(tmp_path_factory):
    require_gpu()
    here = os.getcwd()
    d = tmp_path_factory.mktemp("rwse_driver")
    os.chdir(d)
    world = os.environ.pop("WORLD_SIZE", None)
    yield d
    os.chdir(here)
    if world is not None:
        os.environ["WORLD_SIZE"] = world


def _result_line(out):
    lines = re.findall(LINE, out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    assert re.search(r"RWSE table build time cost: [\d.eE+-]+s", out), out


def test_driver_runs_with_rwse(driver_dir):
    out = _run("--posenc_RWSE 1 " + COMMON + " --save_appendix _rw")
    _result_line(out)
    assert "LapPE table build" not in out
    keys = set(torch.load(driver_dir / "results" / "zinc_GPS_rw" / "model_checkpoint1.pth", map_location="cpu"))
    pre = "encoder.node_encoder."
    assert {pre + "encoder1.encoder.weight", pre + "encoder2.raw_norm.running_mean", pre + "encoder2.pe_encoder.weight"} <= keys
    assert pre + "encoder.weight" not in keys and not any("encoder3" in k for k in keys)


def test_driver_runs_with_lap_pe_and_rwse(driver_dir):
    out = _run("--posenc_RWSE 1 --posenc_LapPE 1 " + COMMON + " --save_appendix _both")
    _result_line(out)
    assert re.search(r"LapPE table build time cost: [\d.eE+-]+s", out), out
    keys = set(torch.load(driver_dir / "results" / "zinc_GPS_both" / "model_checkpoint1.pth", map_location="cpu"))
    pre = "encoder.node_encoder."
    assert {pre + "encoder1.encoder.weight", pre + "encoder2.linear_A.weight", pre + "encoder3.raw_norm.running_mean",
            pre + "encoder3.pe_encoder.weight"} <= keys


def test_a_checkpoint_of_one_layout_is_refused_by_another(driver_dir):
    rw = driver_dir / "results" / "zinc_GPS_rw" / "model_checkpoint1.pth"
    both = driver_dir / "results" / "zinc_GPS_both" / "model_checkpoint1.pth"
    if not rw.exists():
        _run("--posenc_RWSE 1 " + COMMON + " --save_appendix _rw")
    if not both.exists():
        _run("--posenc_RWSE 1 --posenc_LapPE 1 " + COMMON + " --save_appendix _both")
    with pytest.raises(RuntimeError, match="encoder.node_encoder.encoder3"):             # load_state_dict's own error
        _run("--posenc_RWSE 1 --posenc_LapPE 1 --eval 1 " + COMMON + " --save_appendix _x --load_model %s" % rw)
    with pytest.raises(RuntimeError, match="(Unexpected|Missing) key.*encoder.node_encoder"):
        _run("--posenc_RWSE 1 --eval 1 " + COMMON + " --save_appendix _y --load_model %s" % both)
    with pytest.raises(RuntimeError, match="(Unexpected|Missing) key.*encoder.node_encoder"):
        _run(COMMON + " --eval 1 --save_appendix _z --load_model %s" % rw)
    m = re.search(r"Test MAE: (\S+)", _run("--posenc_RWSE 1 --eval 1 " + COMMON + " --save_appendix _rw --load_model %s" % rw))
    assert m and math.isfinite(float(m.group(1)))
