"""The multi-hop cases of tests/gineplus_cases.py have the properties they exist for, and their sequential loop specification
agrees with two independent evaluations of the same formula: multihop_oracle.aggregate64 in fp64 (the project's measure, 1e-5
of max(1, largest value)) and plain torch fp32 index_add_ on one thread, bit for bit - which is what makes the GPU assertions
against the loops meaningful.  Runs without a GPU."""
import numpy as np
import pytest
import torch

import gineplus_cases as gp
import graph_cases as gc
import multihop_oracle as mo

LOOP_CASES = ["degrees", "ties", "hub", "segments", "edgeless_9", "no_d1", "rows_9", "rows_264"]


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_every_case_is_a_valid_batch():
    assert len(set(gp.CASE_NAMES)) == len(gp.CASE_NAMES)
    for name in gp.CASE_NAMES:
        c = gp.case(name)
        n, pairs, dist = c["num_nodes"], c["pairs"], c["distance"]
        assert c["name"] == name and pairs.dtype == np.int64 and dist.dtype == np.int64 and pairs.shape == (2, len(dist))
        assert pairs.size == 0 or (0 <= pairs.min() and pairs.max() < n and dist.min() >= 0)
        b = c["batch"]
        assert len(b) == n and bool((np.diff(b) >= 0).all())
        assert 1 <= c["k"] <= 4 and gp.ks_of(name)[-1] == c["k"]
        if c["source"] == "expand":
            assert sum(m for m, _ in c["graphs"]) == n and max(m for m, _ in c["graphs"]) <= 4096
            order = np.lexsort((pairs[1], pairs[0]))
            assert np.array_equal(order, np.arange(len(dist))), "an expansion comes in (row, col) order"
            assert dist.size == 0 or dist.max() <= c["k"]
            assert bool((b[pairs[0]] == b[pairs[1]]).all()), "no pair crosses two graphs"


def test_degrees_case():
    c = gp.case("degrees")
    n, dist = c["num_nodes"], c["distance"]
    din, dout = gp.pair_degrees(c)
    assert 17 <= n <= 23, "about 20 nodes"
    assert sorted(din[1:n - 1]) == sorted(gp.DEGREE_SET) and sorted(dout[1:n - 1]) == sorted(gp.DEGREE_SET)
    assert set(gp.DEGREES_REQUIRED) == {0, 1} | {b * m + o for b in (gp.BWD_BATCH, gp.FWD_BATCH) for m in (1, 2) for o in (-1, 0, 1)}
    assert set(gp.DEGREES_REQUIRED) <= set(din.tolist()) and set(gp.DEGREES_REQUIRED) <= set(dout.tolist())
    assert din[0] == dout[0] == din[n - 1] == dout[n - 1] == 0, "the first and the last node are isolated"
    for d in gp.DEGREE_SET:                                       # a degree sits on different nodes on the two sides
        assert not set(np.flatnonzero(din == d)) & set(np.flatnonzero(dout == d)) - {0, n - 1}
    assert sorted(set(dist.tolist())) == [1, 2, 3, 4, 5] and c["beyond_k"] == 5 > c["k"] == 4, "one class beyond every k"
    assert all(int((dist == d).sum()) >= 8 for d in (1, 2, 3, 4)) and int((dist == 5).sum()) >= 4
    row, col = c["pairs"]
    far = c["far"]
    touch = (row == far) | (col == far)
    assert int(touch.sum()) >= 4 and int(dist[touch].min()) >= 2, "a node with pairs of distance >= 2 only"
    # the input order is scrambled, so the rank has to follow the input order of the distance-1 pairs
    assert not bool((np.diff(row) >= 0).all()) and not bool((np.diff(col) >= 0).all())
    rank, out_order, in_order = gp.grouping(c)
    d1 = np.flatnonzero(dist == 1)
    assert np.array_equal(rank[d1], np.arange(len(d1))) and bool((rank[dist != 1] == -1).all())
    assert not np.array_equal(rank[out_order][dist[out_order] == 1], np.arange(len(d1))), "rank by (row, col) would be another"
    p, q = c["repeat"]
    assert p != q and row[p] == row[q] and col[p] == col[q] and dist[p] == dist[q] == 1 and rank[q] > rank[p] >= 0
    xs, e, eps, g = gp.operands("degrees", 1, 4)
    assert not torch.equal(e[rank[p]], e[rank[q]]), "the repeated pair has two different rows of e"
    # the two groupings are stable: (row, col) / (col, row) ascending, equal keys in input order
    for order, major, minor in ((out_order, row, col), (in_order, col, row)):
        key = major[order] * n + minor[order]
        assert bool((np.diff(key) >= 0).all()) and bool((np.diff(order)[np.diff(key) == 0] > 0).all())


def test_hub_case():
    c, h = gp.case("hub"), gc.case("hub")
    row, col = c["pairs"]
    dist = c["distance"]
    into = col == h["hub_in"]
    assert int((into & (dist == 1)).sum()) == 1000, "in-degree 1000 at distance 1 on one node"
    # every two-step walk from the out-hub ends on the in-hub, and a multi-hop pair is recorded once: one pair at distance 2
    assert int((into & (dist == 2)).sum()) == 1 and int(row[into & (dist == 2)][0]) == h["hub_out"]
    out = row == h["hub_out"]
    assert int((out & (dist == 1)).sum()) == 1000 and int(out.sum()) == 1002
    assert int(into.sum()) // gp.FWD_BATCH > 100 and int(out.sum()) // gp.BWD_BATCH > 200, "the batch loops of the hub rows run long"
    assert c["num_nodes"] == 1003 and c["k"] == 2 and int((dist == 0).sum()) == 1003


def test_rows_cases():
    assert [gp.bwd_blocks(n) for n in gp.ROWS_N] == list(gp.ROWS_BLOCKS)
    assert [-(-n // (gp.BWD_WAVES * gp.bwd_blocks(n))) for n in gp.ROWS_N] == list(gp.ROWS_PER_WAVE)
    assert gp.ROWS_N[-2] - 4096 == 1 and gp.ROWS_N[-1] - 2 * 4096 == 3, "one wave gets a second row; three waves get a third"
    assert sorted(set(-(-p // 4) for p in gp.ROWS_BLOCKS)) == [1, 8, 9, 128], "rows per group of gp_deps_reduce: trips 1, 1, 2, 16"
    for n, name in zip(gp.ROWS_N, gp.ROWS_CASES):
        c = gp.case(name)
        assert c["num_nodes"] == n and c["k"] == 2 and c["source"] == "expand"
        cnt = np.bincount(c["distance"], minlength=3)
        paths = len(c["graphs"])
        assert cnt[0] == n and cnt[1] == n - paths and cnt[2] >= n - 2 * paths
        depth = gp.deps_depth(c, 2)
        P, R = gp.bwd_blocks(n), -(-n // (8 * gp.bwd_blocks(n)))
        tail = 7 + (-(-P // 4) - 1) + min(3, P - 1)
        assert depth == [R + tail, 1 + R + tail, R + tail], "a path has one pair per source and distance"
        if R > 1:                                                  # the waves that take R rows: every one of their rows has pairs
            W = gp.BWD_WAVES * P
            for d in (1, 2):
                src = set(c["pairs"][0][c["distance"] == d].tolist())
                assert all(node in src for w in range(n - (R - 1) * W) for node in range(w, n, W)), (n, d)


def test_segments_case():
    c = gp.case("segments")
    sizes = [n for n, _ in c["graphs"]]
    assert tuple(sizes) == gp.SEGMENT_SIZES == (1, 3, 5, 1, 40, 2, 1)
    edges = [ei.shape[1] for _, ei in c["graphs"]]
    assert edges[0] == edges[1] == edges[3] == edges[-1] == 0 and edges[4] == 90, "one-node and edgeless graphs first and last"
    assert len(set(map(tuple, c["graphs"][4][1].T.tolist()))) == 90 and bool((c["graphs"][4][1][0] != c["graphs"][4][1][1]).all())
    assert tuple(np.bincount(c["batch"], minlength=len(sizes))) == gp.SEGMENT_SIZES
    row, col = c["pairs"]
    dist = c["distance"]
    rank = gp.grouping(c)[0]
    assert sorted(set(dist.tolist())) == [0, 1, 2, 3, 4]
    for g, ((n0, n1), (r0, r1)) in enumerate(zip(c["node_ranges"], c["d1_ranges"])):
        assert n1 - n0 == sizes[g] and r1 - r0 == len(set(map(tuple, c["graphs"][g][1].T.tolist())) - {(i, i) for i in range(sizes[g])})
        mine = (row >= n0) & (row < n1)
        assert bool(((col[mine] >= n0) & (col[mine] < n1)).all())
        assert sorted(rank[mine & (dist == 1)].tolist()) == list(range(r0, r1))
        # the graph alone expands to the same pairs, shifted (an edgeless graph alone has none; inside it keeps its diagonal)
        a_pairs, a_dist = mo.multihop_batch([sizes[g]], [c["graphs"][g][1]], c["k"])
        if edges[g]:
            assert np.array_equal(a_pairs + n0, c["pairs"][:, mine]) and np.array_equal(a_dist, dist[mine])
        else:
            assert a_dist.size == 0 and bool((dist[mine] == 0).all()) and int(mine.sum()) == sizes[g]
    assert c["node_ranges"][0][0] == 0 and c["node_ranges"][-1][1] == c["num_nodes"] == 53
    assert c["d1_ranges"][0][0] == 0 and c["d1_ranges"][-1][1] == gp.num_d1(c)


def test_edgeless_and_no_d1_cases():
    c = gp.case("edgeless_9")
    assert c["num_nodes"] == 9 and c["pairs"].shape == (2, 0) and gp.num_d1(c) == 0
    c = gp.case("no_d1")
    assert sorted(set(c["distance"].tolist())) == [2, 3] and gp.num_d1(c) == 0 and c["pairs"].shape[1] == 30
    xs, e, eps, g = gp.operands("no_d1", 3, 4)
    assert tuple(e.shape) == (0, 4), "M1 = 0: the edge term has no row"
    assert bool((gp.grouping(c)[0] == -1).all())


def test_ties_case():
    c, base = gp.case("ties"), gp.case("degrees")
    assert np.array_equal(c["pairs"], base["pairs"]) and np.array_equal(c["distance"], base["distance"]), "the `degrees` structure"
    row, col = c["pairs"]
    dist = c["distance"]
    rank = gp.grouping(c)[0]
    k, C = 4, 7
    xs, e, eps, g = gp.operands("ties", k, C)
    s0 = c["negzero_source"]
    assert bool((xs[0][s0] == 0).all()) and bool(torch.signbit(xs[0][s0]).all()), "x_0[s0] = -0.0"
    assert len(c["cancel_pairs"]) == 4 and len(set(c["cancel_pairs"]) | set(c["negzero_pairs"])) == 6
    for p in c["cancel_pairs"] + c["negzero_pairs"]:
        assert dist[p] == 1
        msg = xs[0][row[p]] + e[rank[p]]                          # fp32, one rounding
        assert msg.dtype == torch.float32 and bool((msg == 0).all()), "msg == 0 exactly"
    for p in c["cancel_pairs"]:
        assert row[p] != s0 and bool((xs[0][row[p]] != 0).all()) and not bool(torch.signbit(xs[0][row[p]] + e[rank[p]]).any())
    p, q = c["negzero_pairs"]
    assert row[p] == row[q] == s0
    assert not bool(torch.signbit(xs[0][s0] + e[rank[p]]).any()) and bool(torch.signbit(xs[0][s0] + e[rank[q]]).all()), "+0 and -0"
    seen = set()
    for t in (1, 2, 3):
        nodes = c["dead_sources"][t]
        assert len(nodes) == 3
        for (node, v), sign, zero in zip(nodes, (False, True, True), (True, True, False)):
            assert node not in seen and int(((row == node) & (dist == t + 1)).sum()) >= 1, "a source of pairs at that distance"
            seen.add(node)
            r = xs[t][node]
            assert bool((torch.signbit(r) == sign).all()) and bool(((r == 0) == zero).all()) and bool((r <= 0).all())
            if not zero:
                assert bool((r.abs() < torch.finfo(torch.float32).tiny).all()) and bool((r != 0).all()), "a negative subnormal"
    # at a smaller k only the rows that exist are edited
    assert len(gp.operands("ties", 2, C)[0]) == 2


def _fp64(c, k, xs, e, eps, g):
    xs = [x.double().requires_grad_(True) for x in xs]
    e, eps = e.double().requires_grad_(True), eps.double().requires_grad_(True)
    out = mo.aggregate64(xs, e, eps, torch.from_numpy(c["pairs"]), torch.from_numpy(c["distance"]), k)
    out.backward(g.double())
    zero = lambda t, like: t if t is not None else torch.zeros_like(like)
    return out.detach(), [zero(x.grad, x) for x in xs], zero(e.grad, e), eps.grad


def _near(got, want, what, tol=1e-5):
    got, want = got.double(), want.double()
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) / scale if want.numel() else 0.0
    assert got.shape == want.shape and err <= tol, "%s: max error %.3g of scale %.3g > %g" % (what, err, scale, tol)


@pytest.mark.parametrize("name", LOOP_CASES)
def test_loops_against_fp64_and_index_add(name):
    """the sequential specification against multihop_oracle.aggregate64 with fp64 autograd (which reads the pairs in the order
    given, with e by input rank) and, bit for bit, against torch fp32 index_add_ with autograd on one thread"""
    c = gp.case(name)
    for k in gp.ks_of(name):
        for C in (4, 7):
            r = gp.reference(name, k, C)
            xs, e, eps, g = r["xs"], r["e"], r["eps"], r["g"]
            w_out, w_dx, w_de, w_deps = _fp64(c, k, xs, e, eps, g)
            tag = "%s k=%d C=%d " % (name, k, C)
            _near(r["out"], w_out, tag + "forward")
            for t in range(k):
                _near(r["dx"][t], w_dx[t], tag + "dx_%d" % t)
            _near(r["d_e"], w_de, tag + "d_e")
            _near(r["d_eps"], w_deps, tag + "d_eps", tol=1e-12)
            out, lx, le, leps = gp.aggregate_torch(c, k, xs, e, eps, torch.float32)
            out.backward(g)
            assert torch.equal(out.detach(), r["out"]), tag + "forward"
            for t in range(k):
                got = lx[t].grad if lx[t].grad is not None else torch.zeros_like(xs[t])
                assert torch.equal(got, r["dx"][t]), tag + "dx_%d" % t
            assert torch.equal(le.grad if le.grad is not None else torch.zeros_like(e), r["d_e"]), tag + "d_e"


def test_loop_ignores_what_it_must():
    """distance 0, the class beyond k and a masked pair add nothing; the restricted case keeps the order of what is left"""
    c = gp.case("degrees")
    r = gp.reference("degrees", 3, 7)
    sub = gp.restricted(c, 3)
    assert sub["pairs"].shape[1] == int(((c["distance"] >= 1) & (c["distance"] <= 3)).sum()) and gp.num_d1(sub) == gp.num_d1(c)
    assert torch.equal(gp.forward_loop(sub, 3, r["xs"], r["e"], r["eps"]), r["out"])
    dx, d_e = gp.backward_loop(sub, 3, r["xs"], r["e"], r["eps"], r["g"])
    assert all(torch.equal(a, b) for a, b in zip(dx, r["dx"])) and torch.equal(d_e, r["d_e"])
    keep = c["distance"] != 2
    got = gp.forward_loop(c, 3, r["xs"], r["e"], r["eps"], keep=keep)
    assert not torch.equal(got, r["out"]) and torch.equal(got, gp.forward_loop(gp.restricted(c, 3), 3, r["xs"], r["e"], r["eps"], keep=sub["distance"] != 2))
