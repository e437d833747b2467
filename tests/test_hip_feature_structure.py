"""HIP feature builder (csrc/features.hip) on the case table of tests/feature_cases.py: ego-net sizes on either side of every
rd bucket limit, more rd classes than a launch has workgroups, batches of more than 2048 graphs with edgeless graphs in the
middle, the all-edgeless batch, multi-edges, the sub-degree limit.  All six outputs of encode_edge_lists - `in_edge_of_out`
among them - bit for bit against the oracle (against a golden recorded from the reference for the multi-edge graphs).  That the
rd bins are a fair bit-exact target on these cases is what tests/test_feature_cases_cpu.py asserts."""
import numpy as np
import pytest
import torch

from conftest import FeatureCases, require_gpu
import feature_cases as fc

pytestmark = pytest.mark.gpu

KEYS = ("out_src", "out_dst", "in_edge_of_out", "pos_enc", "pos_index", "pos_batch")


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _encode(graphs, h, use_rd, self_loop):
    from esc_gnn_amd.utils_edge_efficient import encode_edge_lists
    encs = encode_edge_lists([g[0] for g in graphs], [torch.tensor(np.stack([g[1], g[2]])) for g in graphs], h, use_rd, self_loop)
    assert len(encs) == len(graphs)
    out = []
    for ei, in_of_out, pe, pi, pb in encs:
        assert ei.dtype == in_of_out.dtype == pe.dtype == pi.dtype == pb.dtype == torch.int64
        assert ei.dim() == 2 and ei.size(0) == 2 and in_of_out.dim() == pe.dim() == pi.dim() == pb.dim() == 1
        out.append(dict(out_src=ei[0].numpy(), out_dst=ei[1].numpy(), in_edge_of_out=in_of_out.numpy(),
                        pos_enc=pe.numpy(), pos_index=pi.numpy(), pos_batch=pb.numpy()))
    return out


def _same(got, want, name):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for key in KEYS:
            if not np.array_equal(a[key], b[key]):
                pytest.fail("%s: graph %d of %d, %s differs (%d entries against %d)"
                            % (name, i, len(got), key, a[key].shape[0], b[key].shape[0]))


def _run_case(name):
    c = fc.case(name)
    got = _encode(c["graphs"], c["h"], c["use_rd"], c["self_loop"])
    assert sum(g["out_src"].shape[0] for g in got) == c["out_edges"]
    _same(got, fc.expected_batch(c), name)
    return got


@pytest.mark.parametrize("name", ["hub32", "hub33", "hub64", "hub65", "hub96", "hub97"])
def test_one_class_on_each_side_of_every_bucket_limit(E, name):
    """m == n == max_nodes at 32 | 33, 64 | 65, 96 | 97: the device's `m <= 32 / 64 / 96` and the host's comparisons of max_nodes
    have to agree.  Slips it fails under: `m < 32` in place of `m <= 32` in feat_class_mark_kernel, or `m < 96` (the class of hub32 /
    hub96 goes to a launch the host does not make for that max_nodes, its rd bins stay zero); a `break` one too eager
    (`max_nodes <= 33`, `<= 65`, or the two limits swapped: hub33 / hub65 lose their launch); the slab only from
    `max_nodes > 97` (hub97's class is never inverted)."""
    _run_case(name)


@pytest.mark.parametrize("name", ["buckets_mixed", "big_graph_small_egonets", "big_graph_small_egonets_second"])
def test_buckets_in_one_call_and_idle_launches(E, name):
    """All four size buckets filled by one batch with the largest graph first, and a graph of more than 96 nodes whose ego-nets
    have 3 or 4: the ld = 64, ld = 96 and slab launches run on empty class lists, bucket 0 runs with ld = 32 and n_cap = 120.
    Slips: bucket 0's LDS sized from max_nodes instead of min(m_even, 32); `memb` / `loc` sized by ld instead of n_cap (node ids up
    to 119 index them); a launch that does not come back from an empty class list."""
    _run_case(name)


@pytest.mark.parametrize("name", ["many_classes_ld64", "many_classes_ld96", "many_classes_huge"])
def test_more_classes_than_workgroups(E, name):
    """633 classes for the 512 workgroups of the ld = 64 launch, 472 for the 256 of ld = 96, 314 for the 64 slabs: every workgroup
    takes a second class (the slab ones a fifth) on LDS arrays / a slab the first one used, with another m and, in the LDS cases,
    another graph.  Slips: the loop over classes not strided by gridDim.x (the classes beyond the grid keep zero rd rows); Gm / Vm
    not reset to 0 / I, or `memb` / `loc` / `bad_s` not rewritten, between two classes of a workgroup; the leading __syncthreads
    of the class loop dropped."""
    _run_case(name)


@pytest.mark.parametrize("name", ["many_tiny_graphs_loops", "many_tiny_graphs_plain"])
def test_scan_carries_over_2100_graphs(E, name):
    """2100 graphs of 1 to 6 nodes in one call: scan_counts_kernel over e_out and feat_sq_scan_kernel over n^2 run three
    1024-wide rounds, and every per-root and per-edge kernel finds its graph by find_segment in their results.  Without self loops
    a quarter of the graphs have no output edge (out_edge_ptr repeats mid-batch, next to both round boundaries) and one-node
    graphs sit between the others.  Slips: the carry dropped or not updated in either scan (every graph from 1024 on reads the
    hop table / writes the edges of another); `carry_s` read after thread 1023 rewrote it; find_segment returning the first of
    equal pointers instead of the last; out[n] missing the last round."""
    _run_case(name)


@pytest.mark.parametrize("name", ["all_edgeless_rd", "all_edgeless_plain"])
def test_batch_without_any_edge(E, name):
    """No input edge and no self loop to add: esc_features_count returns after the edge scan (`cap_edges == 0`) and
    esc_features_fill at once.  Every graph gets empty int64 outputs of the right rank.  Slips: nnz_ptr[0] left unset on that
    return, or the host reading nnz_ptr[Eout] of a zero-length buffer; the scan skipped so that out_edge_ptr is read unset."""
    got = _run_case(name)
    assert len(got) == 3
    for g in got:
        for key in KEYS:
            assert g[key].shape == (0,) and g[key].dtype == np.int64
    # and as the chunk of a larger list: the edgeless chunk between two that have edges
    tri = dict(fc.TINY_POOL)["triangle"]
    c = fc.case(name)
    datas = [E.Data(x=torch.ones(n, 1), edge_index=torch.tensor(np.stack([s, t])), y=torch.zeros(1))
             for n, s, t in [tri] + c["graphs"] + [tri]]
    outs = E.create_subgraphs_many(datas, c["h"], use_rd=c["use_rd"], self_loop=False, chunk=1)
    outs3 = E.create_subgraphs_many(datas[1:4], c["h"], use_rd=c["use_rd"], self_loop=False)
    want = fc.expected(tri, c["h"], c["use_rd"], False)
    for o in (outs[0], outs[4]):
        assert np.array_equal(o.edge_index.numpy(), np.stack([want["out_src"], want["out_dst"]]))
        assert np.array_equal(o.pos_enc.numpy(), want["pos_enc"]) and np.array_equal(o.pos_index.numpy(), want["pos_index"])
    for o in outs[1:4] + outs3:
        assert tuple(o.edge_index.shape) == (2, 0) and o.pos_enc.numel() == o.pos_index.numel() == o.pos_batch.numel() == 0
        assert o.edge_index.dtype == o.pos_enc.dtype == o.pos_index.dtype == o.pos_batch.dtype == torch.int64


@pytest.mark.parametrize("cfg", fc.MULTI_EDGE_CONFIGS, ids=lambda c: "h%d_rd%d_sl%d" % (c[0], int(c[1]), int(c[2])))
def test_multi_edges_against_the_reference(E, cfg):
    """Repeated (s, t) entries (one three times), reversed repeats and pre-existing self loops (one twice), four graphs as one
    batch; the expectation is the reference's own output (tests/golden/features_structure.npz).  Every listed copy counts: in the
    sub-degree, in the edge-code bins and in the Laplacian (L[s][t] -= 1, L[t][t] += 1 per entry).  Slips: the Laplacian built
    with `=` instead of one atomicAdd per listed edge, or from a de-duplicated list; a pre-existing loop counted into the
    Laplacian's diagonal; with self loops on, a dropped loop still taking a slot so that in_edge_of_out shifts."""
    gold = FeatureCases(fc.GOLDEN_FILE)
    by_name = {gold.names[i]: gold.case(i) for i in range(len(gold))}
    h, rd, sl = cfg
    got = _encode(fc.MULTI_EDGE_GRAPHS, h, rd, sl)
    want = []
    for gi, (n, s, t) in enumerate(fc.MULTI_EDGE_GRAPHS):
        w = dict(by_name[fc.multi_edge_name(gi, cfg)])
        assert np.array_equal(w["in_src"], s) and np.array_equal(w["in_dst"], t)
        w["in_edge_of_out"] = fc.in_edge_of_out(n, s, t, sl)
        want.append(w)
    _same(got, want, "multi_edges")


def _tiny40():
    c = fc.case("many_tiny_graphs_plain")
    return dict(name="tiny40", graphs=c["graphs"][5:45], h=2, use_rd=True, self_loop=False)


@pytest.mark.parametrize("name", ["buckets_mixed", "tiny40"])
def test_order_independence(E, name):
    """A graph's result does not depend on its place in the batch: as given, reversed, and one graph per call.  Slips: anything
    indexed by the position in the batch where the graph's own offset is meant - `in_edge_of_out` returned as `w_in` without
    `edge_ptr[g]` or made local with the wrong graph's offset, pos_batch holding the batch-wide edge id, a class list or slab
    addressed by the first graph's n."""
    c = fc.case(name) if name != "tiny40" else _tiny40()
    cfg = (c["h"], c["use_rd"], c["self_loop"])
    fwd = _encode(c["graphs"], *cfg)
    rev = _encode(c["graphs"][::-1], *cfg)[::-1]
    single = [_encode([g], *cfg)[0] for g in c["graphs"]]
    _same(rev, fwd, name + " reversed")
    _same(single, fwd, name + " one at a time")
    _same(fwd, [fc.expected(g, *cfg) for g in c["graphs"]], name)


def test_edge_attr_rows_follow_in_edge_of_out(E):
    """create_subgraphs_many with a three-column integer edge_attr on six graphs that all have self loops to drop: graph g's
    surviving rows are its own rows `kept`, in order, then n rows of ones - whatever the chunking.  Slips: `in_edge_of_out` as
    `w_in` without `edge_ptr[g]` (the host's subtraction turns every row index of graphs 1.. negative) or with it and no
    subtraction on the host (rows of the previous graphs); the fill rows taken from the dropped loops."""
    pool = dict(fc.TINY_POOL)
    graphs = list(fc.MULTI_EDGE_GRAPHS) + [pool["only_loop"], pool["tri_loop_isolated"]]
    assert len(graphs) >= 4 and all(bool((s == t).any()) for _, s, t in graphs[1:])
    attrs, datas = [], []
    for g, (n, s, t) in enumerate(graphs):
        j = np.arange(s.shape[0], dtype=np.int64)
        ea = np.stack([1000 * (g + 1) + j, 7 * j + g + 2, (13 * j + g) % 5 + 2], axis=1)        # no entry is 1
        attrs.append(ea)
        datas.append(E.Data(x=torch.ones(n, 2), edge_index=torch.tensor(np.stack([s, t])), edge_attr=torch.tensor(ea),
                            y=torch.zeros(1)))
    runs = [E.create_subgraphs_many(datas, 2, use_rd=True, self_loop=True, **kw) for kw in ({}, dict(chunk=1), dict(chunk=3))]
    for (n, s, t), ea, outs in zip(graphs, attrs, zip(*runs)):
        want = fc.expected((n, s, t), 2, True, True)
        want_attr = np.concatenate([ea[s != t], np.ones((n, 3), np.int64)])
        for o in outs:
            assert o.edge_attr.dtype == torch.int64 and np.array_equal(o.edge_attr.numpy(), want_attr)
            assert np.array_equal(o.edge_index.numpy(), np.stack([want["out_src"], want["out_dst"]]))
            for key in ("pos_enc", "pos_index", "pos_batch"):
                assert np.array_equal(o[key].numpy(), want[key]), key
    # without self-loop normalisation the rows stay as they are
    plain = E.create_subgraphs_many(datas, 2, use_rd=False, self_loop=False, chunk=3)
    for ea, d, o in zip(attrs, datas, plain):
        assert np.array_equal(o.edge_attr.numpy(), ea) and torch.equal(o.edge_index, d.edge_index)


@pytest.mark.parametrize("n,self_loop,degree,encodes", fc.STAR_CASES)
def test_sub_degree_limit(E, n, self_loop, degree, encodes):
    """The hub of a star has sub-degree n - 1, plus one for its self loop: 199 encodes (bin 199 of the degree one-hot), 200 is
    refused like the reference's one_hot(num_classes=200).  Slips: `dg > 200` in place of `dg >= 200`; the self loop left out
    of the out-degree (the 200-node star with loops would encode); the limit applied to the graph's degree before sub-edges."""
    g = fc.star(n)
    if encodes:
        got = _encode([g], 1, False, self_loop)
        _same(got, [fc.expected(g, 1, False, self_loop)], "star%d" % n)
        assert degree in got[0]["pos_index"][got[0]["pos_batch"] == 0].tolist()
    else:
        with pytest.raises(RuntimeError, match="graph 0 cannot be encoded"):
            _encode([g], 1, False, self_loop)


def test_refused_graph_in_a_batch_is_named_and_leaves_nothing_behind(E):
    """A graph over the degree limit as the third of five: the error names graph 2, and the next call on the four good graphs is
    correct.  Slips: the status written at the edge's batch-wide index or at graph 0; a status that outlives the call."""
    pool = dict(fc.TINY_POOL)
    good = [pool["triangle"], pool["path4"], pool["star5"], pool["cycle6"]]
    graphs = good[:2] + [fc.star(200)] + good[2:]
    with pytest.raises(RuntimeError, match=r"graph 2 cannot be encoded \(status"):
        _encode(graphs, 1, False, True)
    for rd in (False, True):
        _same(_encode(good, 1, rd, True), [fc.expected(g, 1, rd, True) for g in good], "after the refusal")
