"""The structural cases of tests/graph_cases.py have the properties they exist for, and their sequential loop references
agree with single-threaded torch.index_add_ bit for bit (which is what makes the GPU assertions against them meaningful).
Runs without a GPU."""
import numpy as np
import pytest
import torch

import graph_cases as gc


@pytest.fixture(autouse=True)
def _one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_every_case_is_a_valid_batch():
    names = [c["name"] for c in gc.CASES]
    assert len(set(names)) == len(names)
    for want in ("degrees", "hub", "no_edges", "bag_edges", "bag_borders", "bag_tiny", "bag_local", "bag_local_skew"):
        assert want in gc.BY_NAME
    for c in gc.CASES:
        ei, n = c["edge_index"], c["num_nodes"]
        assert ei.dtype == torch.int64 and ei.shape[0] == 2 and ei.dim() == 2
        assert ei.numel() == 0 or (0 <= int(ei.min()) and int(ei.max()) < n)
        b = c["batch"]
        assert b.dtype == torch.int64 and b.numel() == n and bool((b[1:] >= b[:-1]).all())
        assert n == 0 or int(b[-1]) < c["num_graphs"]
        if "pos_batch" in c:
            pe, pi, pb = c["pos_enc"], c["pos_index"], c["pos_batch"]
            assert pe.numel() == pi.numel() == pb.numel() > 0
            assert bool((pb[1:] >= pb[:-1]).all()), "BatchPlan.from_tensors demands a non-decreasing pos_batch"
            assert 0 <= int(pb.min()) and int(pb.max()) < ei.shape[1]
            assert 0 <= int(pi.min()) and int(pi.max()) < c["n_cols"] == 1800
            assert int(pe.min()) >= 1


def test_degrees_case():
    c = gc.case("degrees")
    din, dout = gc.degrees(c)
    n = c["num_nodes"]
    assert sorted(din[1:n - 1]) == sorted(gc.DEGREE_SET) and sorted(dout[1:n - 1]) == sorted(gc.DEGREE_SET)
    assert din[0] == dout[0] == din[n - 1] == dout[n - 1] == 0, "the first and the last node are isolated"
    for d in gc.DEGREE_SET:                                      # a degree sits on different nodes on the two sides
        assert not set(np.flatnonzero(din == d)) & set(np.flatnonzero(dout == d)) - {0, n - 1}
    src, dst = c["edge_index"].numpy()
    assert int((src == dst).sum()) >= 1, "self loops"
    pairs = src * n + dst
    assert len(np.unique(pairs)) < len(pairs), "parallel edges"
    rev = set((dst * n + src).tolist())
    assert any(p not in rev for p in pairs.tolist()), "not symmetric"
    # the edges of a node are scattered: neither endpoint list is sorted
    assert not bool((np.diff(dst) >= 0).all()) and not bool((np.diff(src) >= 0).all())


def test_hub_case():
    c = gc.case("hub")
    din, dout = gc.degrees(c)
    assert din[c["hub_in"]] == 1000 and dout[c["hub_out"]] == 1000
    assert din[c["hub_in"]] // 8 > 100, "the batch loop of the hub row runs more than 100 times"
    rest = np.ones(c["num_nodes"], dtype=bool)
    rest[[c["hub_in"], c["hub_out"]]] = False
    assert (din + dout)[rest].max() <= 2 and (din + dout)[rest].min() == 0
    assert dout[c["hub_in"]] == 0 and din[c["hub_out"]] == 0


def test_tiny_and_empty_cases():
    assert sorted(gc.case(t)["num_nodes"] % 4 for t in gc.TINY_CASES) == [0, 1, 1, 2, 3]
    for t, n in zip(gc.TINY_CASES, (1, 2, 3, 4, 5)):
        c = gc.case(t)
        assert c["num_nodes"] == n and 3 <= c["edge_index"].shape[1] <= 8
    c = gc.case("no_edges")
    assert c["num_nodes"] == 6 and tuple(c["edge_index"].shape) == (2, 0)


def test_segment_cases():
    assert [gc.case(s)["num_graphs"] for s in gc.SEGMENT_CASES] == [1, 5, 9]
    sizes = [s for name in gc.SEGMENT_CASES for s in gc.case(name)["sizes"]]
    assert 0 in sizes and 1 in sizes and max(sizes) >= 297
    for name in gc.SEGMENT_CASES:
        c = gc.case(name)
        counts = np.bincount(c["batch"].numpy(), minlength=c["num_graphs"])
        assert tuple(counts) == c["sizes"]
    for name in ("segments_G5", "segments_G9"):
        s = gc.case(name)["sizes"]
        assert s[-1] == 0, "an unused graph id at the end"
        assert any(s[i] == 0 and any(s[i + 1:]) for i in range(1, len(s) - 1)), "an unused graph id in the middle"
    assert [g % 4 for g in (1, 5, 9)] == [1, 1, 1] and 9 > 2 * 4, "G is never a multiple of the 4 graphs of a workgroup; three workgroups"


def test_bag_edges_case():
    c = gc.case("bag_edges")
    ln = gc.bag_lengths(c)
    assert tuple(ln) == c["lengths"]
    assert ln[0] == 0 and ln[-1] == 0 and 0 in ln[1:-1] and 1 in ln and ln.max() >= 200
    # the lengths the forward's 8 / 4 / 1 unrolling distinguishes
    assert {1, 4, 7, 8, 9, 12} <= set(ln.tolist())
    pe = c["pos_enc"]
    assert int(pe.min()) == 1 and int(pe.max()) >= 50000
    assert int(pe[c["pos_batch"] == 1][0]) == 1


def _columns(c):
    """[(column, first sorted entry, one past the last)] of the non-empty columns and every column's length"""
    ln = gc.column_lengths(c)
    ptr = np.concatenate([[0], np.cumsum(ln)])
    return ln, ptr


def test_bag_borders_case():
    c = gc.case("bag_borders")
    ln, ptr = _columns(c)
    assert tuple(ln[list(gc.BORDER_COLUMNS)]) == gc.BORDER_LENGTHS and int(ln.sum()) == sum(gc.BORDER_LENGTHS)
    assert tuple(gc.BORDER_LENGTHS[:8]) == (64, 1, 63, 320, 0, 0, 64 + 1, 127)
    Z, CH = int(ln.sum()), gc.BAG_CH
    assert Z % CH != 0
    span = {col: (int(ptr[col]), int(ptr[col + 1])) for col in gc.BORDER_COLUMNS}
    chunks = lambda col: (span[col][1] - 1) // CH - span[col][0] // CH + 1
    assert span[0] == (0, CH), "a column that is exactly one chunk"
    assert span[2][1] % CH == 0 and span[2][0] % CH != 0 and chunks(2) == 1, "ends on a chunk border"
    assert span[3][0] % CH == 0 and span[3][1] % CH == 0 and chunks(3) == 5, "starts on a border, spans five chunks"
    assert ln[4] == ln[5] == 0 and ln[3] >= CH and ln[6] >= CH, "empty columns between two long ones"
    assert span[6][0] % CH == 0 and chunks(6) == 2, "starts on a border and runs one entry into the next chunk"
    assert span[7][1] % CH == 0 and chunks(7) == 2, "starts inside a chunk, ends on a border"
    assert span[902][0] % CH != 0 and span[902][1] % CH != 0 and chunks(902) == 6, "a long column aligned to nothing"
    assert ln[1799] > 0 and ln[0] > 0, "the first and the last table row are used"
    # pos_batch is sorted by edge, and inside a column the stable sort leaves the entries in ascending edge order
    _, perm = gc.stable_csr(c["pos_index"].numpy(), c["n_cols"])
    rows = c["pos_batch"].numpy()[perm]
    for col in gc.BORDER_COLUMNS:
        a, b = span[col]
        assert bool((np.diff(rows[a:b]) > 0).all())


def test_bag_tiny_and_local_cases():
    assert gc.case("bag_tiny")["pos_batch"].numel() == 5 < gc.BAG_CH
    for name in ("bag_local", "bag_local_skew"):
        c = gc.case(name)
        E, Z, H = c["edge_index"].shape[1], c["pos_batch"].numel(), gc.LOCAL_H
        assert E == 4200 and H == 256 and Z >= 4096 + 37
        # the two inequalities of bag_local_schedule (csrc/bag.hip), restated
        assert E * H * 4 > 4 * 1024 * 1024
        assert (Z + 63) // 64 >= 64
        assert gc.bag_local_schedule(Z, H, E) and not gc.bag_local_schedule(Z, H, 0) and not gc.bag_local_schedule(Z, 10, E)
        assert Z % gc.BAG_CH != 0
    c = gc.case("bag_local")
    ln = gc.bag_lengths(c)
    assert ln.max() - ln.min() <= 1, "entries spread evenly over the edges"
    assert len(set(gc.chunk_buckets(c, 4200).tolist())) == 8, "every bucket of the local schedule gets chunks"
    c = gc.case("bag_local_skew")
    E = c["edge_index"].shape[1]
    assert int(c["pos_batch"].max()) < E // 8
    assert int((gc.bag_lengths(c)[E // 8:] != 0).sum()) == 0, "every other edge has an empty bag"
    b = gc.chunk_buckets(c, E)
    assert set(b.tolist()) == {0}, "every chunk lands in bucket 0"
    # ... which is more than the launch's waves of one group hold at once: the strided loop of bag_bwd_pass1_local must run
    chunks = len(b)
    per_group = -(-(-(-chunks // 8) * 5 // 4 + 4) // 4)
    assert chunks > per_group * 4


def _inputs(c, C, seed):
    g0 = torch.Generator().manual_seed(seed)
    N, E = c["num_nodes"], c["edge_index"].shape[1]
    return torch.randn(N, C, generator=g0), torch.randn(E, C, generator=g0), torch.tensor([0.3])


@pytest.mark.parametrize("name", gc.GRAPH_CASES)
def test_aggregate_loop_is_index_add(name):
    c = gc.case(name)
    ei = c["edge_index"]
    for C in (5, 64):
        x, e, eps = _inputs(c, C, 3)
        for use_e in (True, False):
            for use_eps in (True, False):
                msg = (x.index_select(0, ei[0]) + e).relu() if use_e else x.index_select(0, ei[0]).relu()
                want = torch.zeros_like(x).index_add_(0, ei[1], msg)
                if use_eps:
                    want = want + (1 + eps) * x
                got = gc.aggregate_loop(x, e if use_e else None, eps if use_eps else None, ei)
                assert torch.equal(got, want), (name, C, use_e, use_eps)
        # the fp32 sequential backward against fp64 autograd (a yardstick, not bit-exact against anything)
        g = torch.randn(c["num_nodes"], C, generator=torch.Generator().manual_seed(4))
        x64, e64 = x.double().requires_grad_(True), e.double()
        (torch.zeros_like(x64).index_add(0, ei[1], (x64.index_select(0, ei[0]) + e64).relu()) + (1 + eps.double()) * x64).backward(g.double())
        dx = gc.aggregate_dx_loop(x, e, eps, g, ei)
        assert torch.allclose(dx.double(), x64.grad, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("name", gc.BAG_CASES)
def test_bag_loop_is_index_add(name):
    c = gc.case(name)
    E = c["edge_index"].shape[1]
    W = torch.randn(c["n_cols"], 12, generator=torch.Generator().manual_seed(5))
    prod = W[c["pos_index"]] * c["pos_enc"].to(torch.float32).view(-1, 1)
    want = torch.zeros(E, 12).index_add_(0, c["pos_batch"], prod)
    got = gc.bag_loop(W, c["pos_enc"], c["pos_index"], c["pos_batch"], E)
    assert torch.equal(got, want)
    empty = torch.tensor(gc.bag_lengths(c) == 0)
    assert not bool(torch.signbit(got[empty]).any()) and float(got[empty].abs().sum()) == 0.0
    base = torch.randn(E, 12, generator=torch.Generator().manual_seed(6))
    assert torch.equal(gc.bag_loop(W, c["pos_enc"], c["pos_index"], c["pos_batch"], E, base=base),
                       base.clone().index_add_(0, c["pos_batch"], prod))


@pytest.mark.parametrize("name", gc.SEGMENT_CASES)
def test_segment_loop_is_index_add(name):
    c = gc.case(name)
    x = torch.randn(c["num_nodes"], 9, generator=torch.Generator().manual_seed(7))
    want = torch.zeros(c["num_graphs"], 9).index_add_(0, c["batch"], x)
    got = gc.segment_sum_loop(x, c["batch"], c["num_graphs"])
    assert torch.equal(got, want)
    for g, s in enumerate(c["sizes"]):
        if s == 0:
            assert float(got[g].abs().sum()) == 0.0


def test_stable_csr_is_a_stable_grouping():
    c = gc.case("degrees")
    dst = c["edge_index"][1].numpy()
    ptr, perm = gc.stable_csr(dst, c["num_nodes"])
    assert ptr[0] == 0 and ptr[-1] == len(dst)
    for i in range(c["num_nodes"]):
        seg = perm[ptr[i]:ptr[i + 1]]
        assert bool((dst[seg] == i).all()) and bool((np.diff(seg) > 0).all())
