"""The cases of tests/feature_cases.py have the properties they exist for, and the bit-exact comparison of the rd bins that
tests/test_hip_feature_structure.py makes with them is a fair one: no fp64 resistance distance of the oracle is balanced on an
integer, and no Laplacian has a singular value where scipy's cutoff and the kernel's could part.  Runs without a GPU, on the
oracle (oracle/ref_features.py) and numpy / scipy alone."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, FeatureCases
import feature_cases as fc
import ref_features as orc

EPS = np.finfo(np.float64).eps
RD_CASES = [c["name"] for c in fc.CASES if c["use_rd"]]

_STRUCT = {}


def structure(graph, h, self_loop):
    """From the oracle's hop table: the output edges of a graph, the ego-net size |S_u ∪ S_v| of each, and its rd classes (the
    distinct unordered pairs of reach sets {S_u, S_v}) counted per size bucket."""
    n, s, t = graph
    key = (n, s.tobytes(), t.tobytes(), h, self_loop)
    if key in _STRUCT:
        return _STRUCT[key]
    if self_loop:
        s, t, _ = orc.normalise_self_loops(s, t, n)
    reach = orc.hop_table(s, t, n, h) <= h
    first = {}
    canon = np.array([first.setdefault(reach[r].tobytes(), r) for r in range(n)], dtype=np.int64)
    sizes = (reach[s] | reach[t]).sum(axis=1) if s.size else np.zeros(0, np.int64)
    lo, hi = np.minimum(canon[s], canon[t]), np.maximum(canon[s], canon[t])
    per_class = {}
    for a, b, m in zip(lo.tolist(), hi.tolist(), sizes.tolist()):
        assert per_class.setdefault((a, b), m) == m
    buckets = [0, 0, 0, 0]
    for m in per_class.values():
        buckets[fc.bucket_of(m)] += 1
    _STRUCT[key] = dict(out_edges=int(s.size), sizes=sizes, classes=tuple(buckets), class_sizes=sorted(per_class.values()))
    return _STRUCT[key]


def batch_structure(c):
    per = [structure(g, c["h"], c["self_loop"]) for g in c["graphs"]]
    sizes = np.concatenate([p["sizes"] for p in per])
    return dict(per=per, out_edges=sum(p["out_edges"] for p in per),
                classes=tuple(int(x) for x in np.sum([p["classes"] for p in per], axis=0)),
                m_range=(int(sizes.min()), int(sizes.max())) if sizes.size else None,
                class_sizes=sorted(m for p in per for m in p["class_sizes"]))


def test_table_is_complete():
    names = [c["name"] for c in fc.CASES]
    assert len(set(names)) == len(names)
    for want in ("hub32", "hub33", "hub64", "hub65", "hub96", "hub97", "buckets_mixed", "big_graph_small_egonets",
                 "big_graph_small_egonets_second", "many_classes_ld64", "many_classes_ld96", "many_classes_huge",
                 "many_tiny_graphs_loops", "many_tiny_graphs_plain", "all_edgeless_rd", "all_edgeless_plain"):
        assert want in fc.BY_NAME
    assert sorted((c["h"], c["use_rd"], c["self_loop"]) for c in fc.CASES if c.get("golden")) == sorted(fc.MULTI_EDGE_CONFIGS)
    for c in fc.CASES:
        for n, s, t in c["graphs"]:
            assert s.dtype == t.dtype == np.int64 and s.shape == t.shape and s.ndim == 1 and n >= 1
            assert s.size == 0 or (0 <= min(s.min(), t.min()) and max(s.max(), t.max()) < n)
        assert 1 <= c["h"] <= 4


@pytest.mark.parametrize("name", [c["name"] for c in fc.CASES])
def test_structural_claims(name):
    c = fc.case(name)
    st = batch_structure(c)
    print(name, "out_edges", st["out_edges"], "classes", st["classes"], "m_range", st["m_range"])
    assert max(g[0] for g in c["graphs"]) == c["max_nodes"]
    assert st["out_edges"] == c["out_edges"]
    assert st["out_edges"] == sum(e["out_src"].shape[0] for e in fc.expected_batch(c, record=True))
    if c["use_rd"] and not c.get("golden"):
        assert st["classes"] == c["classes"] and st["m_range"] == c["m_range"]


def test_hub_cases_sit_on_the_bucket_limits():
    for n, bucket in ((32, 0), (33, 1), (64, 1), (65, 2), (96, 2), (97, 3)):
        c = fc.case("hub%d" % n)
        st = batch_structure(c)
        assert c["h"] == 2 and c["use_rd"] and c["self_loop"] and len(c["graphs"]) == 1
        assert bool((st["per"][0]["sizes"] == n).all()), "every ego-net is the whole graph"
        assert st["class_sizes"] == [n] and fc.bucket_of(n) == bucket and c["max_nodes"] == n
        assert c["graphs"][0][1].shape[0] == 4 * (n - 1) and 124 <= 4 * (n - 1) <= 384
    # what the host compares max_nodes with (esc_features_count): the ld of bucket 0, the two breaks, the slab
    assert [n for n in (32, 33, 64, 65, 96, 97) if n <= 32] == [32] and [n for n in (33, 64, 65) if n <= 64] == [33, 64]
    assert (97 + 1) & ~1 == 98, "the slab's leading dimension is rounded to even"


def test_buckets_mixed_and_big_graph_cases():
    c = fc.case("buckets_mixed")
    assert [g[0] for g in c["graphs"]] == [97, 32, 20, 64, 33] and c["h"] == 2
    assert all(k > 0 for k in (c["classes"][0], c["classes"][1], c["classes"][3])), "LDS buckets and the slab in one call"
    per = batch_structure(c)["per"]
    assert [p["classes"] for p in per][:2] == [(0, 0, 0, 1), (1, 0, 0, 0)] and per[3]["classes"] == per[4]["classes"] == (0, 1, 0, 0)
    # ld = 96 is launched (max_nodes > 64) although no class of this batch lands there: an empty list for that launch
    assert c["classes"][2] == 0
    for name in ("big_graph_small_egonets", "big_graph_small_egonets_second"):
        c = fc.case(name)
        assert c["graphs"][-1][0] >= 97 and c["h"] == 1 and c["use_rd"]
        assert c["classes"][3] == 0 and c["max_nodes"] > 96, "the slab kernel is launched and finds nothing"
        assert batch_structure(c)["per"][-1]["classes"][1:] == (0, 0, 0)
    assert fc.case("big_graph_small_egonets_second")["graphs"][0][0] == 33


def test_many_classes_cases_outnumber_their_launches():
    c = fc.case("many_classes_ld64")
    assert len(c["graphs"]) == 4 and c["h"] == 3 and not c["self_loop"]
    assert c["classes"][1] > fc.LDS_GRIDS[1] == 512
    c = fc.case("many_classes_ld96")
    assert len(c["graphs"]) == 2 and c["h"] == 3 and c["max_nodes"] == 96
    assert c["classes"][2] > fc.LDS_GRIDS[2] == 256
    c = fc.case("many_classes_huge")
    assert len(c["graphs"]) == 1 and c["h"] == 4 and c["self_loop"]
    assert c["classes"][3] > fc.HUGE_SLABS == 64
    # the grids, restated from esc_features_count: 256 * min(16, 160 KB / class_lds_bytes(ld, n_cap))
    lds = lambda ld, n_cap: ((2 * ld + 8) * 8 + 400 + 3 * n_cap + 2 * ld * ld * 8 + 15) & ~15
    assert 256 * min(16, 160 * 1024 // lds(64, 80)) == 512 and 256 * min(16, 160 * 1024 // lds(96, 96)) == 256
    # and of the slab launch: min(64, 1 GiB / (2 * ld^2 * 8))
    assert min(64, (1 << 30) // (2 * 130 * 130 * 8)) == 64


def test_many_tiny_graphs_cross_the_scan_rounds():
    pool = [g for _, g in fc.TINY_POOL]
    assert 10 <= len(pool) <= 14 and {g[0] for g in pool} == {1, 2, 3, 4, 5, 6}
    assert len({name for name, _ in fc.TINY_POOL}) == len(pool)
    for sl in (True, False):
        c = fc.case("many_tiny_graphs_loops" if sl else "many_tiny_graphs_plain")
        G = len(c["graphs"])
        assert G == fc.TINY_G == 2100 > 2048 and c["h"] == 2 and c["use_rd"] and c["self_loop"] == sl
        e_out = np.array([structure(g, 2, sl)["out_edges"] for g in c["graphs"]])
        sq = np.array([g[0] ** 2 for g in c["graphs"]])
        # the carries of scan_counts_kernel (e_out) and feat_sq_scan_kernel (n^2) after each 1024-wide round are not zero and differ
        assert 0 < e_out[:1024].sum() < e_out[:2048].sum() < e_out.sum() == c["out_edges"]
        assert 0 < sq[:1024].sum() < sq[:2048].sum() < sq.sum()
        assert len(set(e_out[:len(pool)].tolist())) >= 6 and len(set(sq[:len(pool)].tolist())) == 6
        zero = np.flatnonzero(e_out == 0)
        if sl:
            assert zero.size == 0
        else:
            assert c["zero_edge_middle"] and zero.size > 300 and 0 < zero[1] and zero[-2] < G - 1
            one_node_mid = [i for i in range(1, G - 1) if c["graphs"][i][0] == 1]
            assert len(one_node_mid) > 300
            # find_segment: repeated out_edge_ptr entries next to a boundary of the scan rounds
            assert any(1000 <= z <= 1048 for z in zero.tolist()) and any(2024 <= z <= 2072 for z in zero.tolist())
    kinds = dict(fc.TINY_POOL)
    assert kinds["node"][0] == 1 and kinds["node"][1].size == 0 and kinds["edgeless3"][0] == 3 and kinds["edgeless3"][1].size == 0
    assert kinds["arc"][1].tolist() == [0] and kinds["arc"][2].tolist() == [1]
    assert kinds["only_loop"][0] == 1 and kinds["only_loop"][1].tolist() == kinds["only_loop"][2].tolist() == [0]
    s, t = kinds["dicycle_dup"][1:]
    assert len(set(zip(s.tolist(), t.tolist()))) == 3 < s.size


def test_many_tiny_graphs_tiling_is_the_oracle_per_graph():
    for name in ("many_tiny_graphs_loops", "many_tiny_graphs_plain"):
        c = fc.case(name)
        tiled = fc.expected_batch(c, record=True)
        assert len(fc._MEMO) < 200, "one oracle call per pool shape and configuration, not one per graph"
        for (n, s, t), e in list(zip(c["graphs"], tiled))[:30]:
            w = orc.encode_graph(s, t, n, c["h"], c["use_rd"], c["self_loop"])
            for key, got in (("out_src", w["edge_src"]), ("out_dst", w["edge_dst"]), ("pos_enc", w["pos_enc"]),
                             ("pos_index", w["pos_index"]), ("pos_batch", w["pos_batch"])):
                assert np.array_equal(e[key], got) and e[key].dtype == np.int64
            kept = w["kept"]
            want_in = np.concatenate([np.flatnonzero(kept), np.full(n, -1)]) if c["self_loop"] else np.arange(s.size)
            assert np.array_equal(e["in_edge_of_out"], want_in)


def test_all_edgeless_cases():
    for name in ("all_edgeless_rd", "all_edgeless_plain"):
        c = fc.case(name)
        assert [g[0] for g in c["graphs"]] == [3, 1, 5] and not c["self_loop"]
        assert sum(g[1].size for g in c["graphs"]) == 0, "total_in_edges + 0 self loops: the cap_edges == 0 return"
        for e in fc.expected_batch(c, record=True):
            assert all(v.size == 0 and v.dtype == np.int64 for v in e.values())
    assert fc.case("all_edgeless_rd")["use_rd"] and not fc.case("all_edgeless_plain")["use_rd"]


def test_star_cases_sit_on_the_degree_limit():
    assert [(n, sl) for n, sl, _, _ in fc.STAR_CASES] == [(199, True), (200, False), (200, True), (201, False)]
    for n, sl, degree, encodes in fc.STAR_CASES:
        g = fc.star(n)
        s = g[1]
        assert int(np.bincount(s).max()) + int(sl) == degree and encodes == (degree < 200)
        if encodes:
            e = fc.expected(g, 1, False, sl)
            hub_edge = e["pos_batch"] == 0                      # edge 0 is (0, 1): the hub is in its ego-net
            assert degree in e["pos_index"][hub_edge].tolist(), "the hub's degree bin"
        else:
            with pytest.raises(RuntimeError, match="sub-degree"):
                orc.encode_graph(g[1], g[2], n, 1, False, sl)


def test_multi_edge_graphs_and_golden():
    for n, s, t in fc.MULTI_EDGE_GRAPHS:
        assert 7 <= n <= 10
        pairs = list(zip(s.tolist(), t.tolist()))
        non_loop = [p for p in pairs if p[0] != p[1]]
        loops = [p for p in pairs if p[0] == p[1]]
        counts = {p: pairs.count(p) for p in set(pairs)}
        assert max(counts[p] for p in non_loop) >= 3 and sum(1 for p in set(non_loop) if counts[p] >= 2) >= 2, "repeated (s, t)"
        assert any((b, a) in counts for a, b in non_loop), "reversed repeats"
        assert len(set(loops)) >= 2 and len(loops) > len(set(loops)), "pre-existing self loops, one of them twice"
        assert any((b, a) not in counts for a, b in non_loop), "not symmetric"
    gold = FeatureCases(fc.GOLDEN_FILE)
    assert os.path.getsize(os.path.join(GOLDEN, fc.GOLDEN_FILE)) < 64 * 1024
    assert len(gold) == len(fc.MULTI_EDGE_GRAPHS) * len(fc.MULTI_EDGE_CONFIGS) == 16
    by_name = {gold.names[i]: gold.case(i) for i in range(len(gold))}
    for cfg in fc.MULTI_EDGE_CONFIGS:
        for gi, g in enumerate(fc.MULTI_EDGE_GRAPHS):
            want = by_name[fc.multi_edge_name(gi, cfg)]
            assert (want["n"], want["h"], want["use_rd"], want["self_loop"]) == (g[0],) + cfg
            assert np.array_equal(want["in_src"], g[1]) and np.array_equal(want["in_dst"], g[2])
            e = fc.expected(g, *cfg, record=True)
            for key in ("out_src", "out_dst", "pos_enc", "pos_index", "pos_batch"):
                assert np.array_equal(e[key], want[key]), (gi, cfg, key)


# ---- conditioning of the bit-exact rd comparison ---------------------------------------------------------------------------------
# (a) an fp64 rd value is either within NEAR of an integer or at least FAR from every integer.  The fp32 cast snaps anything
#     within half an fp32 ulp onto the integer: at most 2.4e-7 below 8, where every undirected case stays, and 4.8e-7 below 16,
#     where the directed multi-edge graphs stay (asserted: no |rd| reaches 16).  So 1e-6 is clear of the snap zone and 1e-9 far
#     inside it, and far above the 1e-13 or so that two fp64 pseudo-inverses of these matrices differ by.
# (b) a singular value of a Laplacian, relative to the largest, is either below a quarter of scipy's cutoff m * eps or above 1e-8:
#     the kernel drops directions below 2 * m * eps * |L|_F, at most 2 * m^1.5 * eps < 1e-12 of the largest at m <= 131.
NEAR, FAR, SV_FLOOR, SV_NULL = 1e-9, 1e-6, 1e-8, 0.25


@pytest.mark.parametrize("name", RD_CASES)
def test_rd_comparison_is_well_conditioned(name):
    c = fc.case(name)
    worst = dict(rd_far=np.inf, rd_near=0.0, sv_low=0.0, sv_high=np.inf, rd_max=0.0, count=0)
    for g in c["graphs"]:
        fc.expected(g, c["h"], True, c["self_loop"], record=True)
        r = fc.margins(g, c["h"], c["self_loop"])
        worst["rd_far"], worst["sv_high"] = min(worst["rd_far"], r.rd_far), min(worst["sv_high"], r.sv_high)
        worst["rd_near"], worst["sv_low"] = max(worst["rd_near"], r.rd_near), max(worst["sv_low"], r.sv_low)
        worst["rd_max"], worst["count"] = max(worst["rd_max"], r.rd_max), worst["count"] + r.count
    print("%s: nearest non-integer rd %.3g from an integer, snapped ones within %.3g, largest rd %.3f; smallest kept singular "
          "value %.3g of the largest, largest dropped %.3g of m*eps" % (name, worst["rd_far"], worst["rd_near"], worst["rd_max"],
                                                                       worst["sv_high"], worst["sv_low"]))
    if fc.case(name)["out_edges"]:
        assert worst["count"] > 0
    assert worst["rd_max"] < (16.0 if c.get("golden") else 8.0)
    assert worst["rd_near"] <= NEAR and worst["rd_far"] >= FAR
    assert worst["sv_low"] < SV_NULL and worst["sv_high"] > SV_FLOOR
    assert 2 * 131 ** 1.5 * EPS < 1e-12 and max(g[0] for g in c["graphs"]) <= 130
