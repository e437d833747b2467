"""The NGNN baseline on the MI355X: the rooted-subgraph expansion kernels (csrc/subgraphs.hip) against the reference goldens
and the numpy oracle, rd against scipy's pseudo-inverse, the collated batch of the reference, ops.segment_first against torch
indexing, zinc_models.NGNN against the reference golden and an fp64 oracle, the error paths and the run_zinc driver."""
import copy
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, require_gpu
import ngnn_oracle as no
from test_ngnn_cpu import load_collate_ngnn3, ngnn_golden_runs, subgraph_golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _graph(E, n, ei, x=None, edge_attr=None, y=None):
    ei = torch.as_tensor(np.asarray(ei), dtype=torch.int64).reshape(2, -1)
    return E.Data(x=torch.arange(n) if x is None else torch.as_tensor(x), edge_index=ei,
                  edge_attr=torch.arange(ei.size(1)) % 4 if edge_attr is None else torch.as_tensor(edge_attr),
                  y=torch.zeros(1) if y is None else torch.as_tensor(y), num_nodes=n)


def _sym(pairs):
    return np.array([[a for a, b in pairs] + [b for a, b in pairs], [b for a, b in pairs] + [a for a, b in pairs]], dtype=np.int64).reshape(2, -1)


def _ring(rng, n, chords):
    pairs = [(i, (i + 1) % n) for i in range(n)] if n > 2 else ([(0, 1)] if n == 2 else [])
    pairs += [(int(a), int(b)) for a, b in rng.randint(0, n, (chords, 2)) if a != b]
    return _sym(pairs)


def _check_integers(sub, want, h, node_label="spd", what=""):
    """every integer output of expand_subgraphs against the oracle's expansion of the same batch"""
    for k in ("orig_node", "orig_edge", "node_to_subgraph", "edge_index", "batch", "sub_node_ptr", "sub_edge_ptr"):
        got = sub[k].cpu().numpy()
        assert got.dtype == np.int64 and got.shape == want[k].shape and np.array_equal(got, want[k]), (what, k)
    assert np.array_equal(sub.z.cpu().numpy(), no.labels(want["z"], want["paths"], h, node_label)), (what, "z")
    assert sub.num_subgraphs == want["sub_node_ptr"].shape[0] - 1


def _expand(E, graphs, h, **kw):
    from esc_gnn_amd.subgraphs import collate_graphs, expand_subgraphs
    return expand_subgraphs(collate_graphs(graphs, DEV), h, **kw)


# ---- 1. expansion ----------------------------------------------------------------------------------------------------------
def test_expansion_against_reference_golden(E):
    from esc_gnn_amd.utils import create_subgraphs
    seen = 0
    for name, n, ei, h, want in subgraph_golden_cases():
        for label in ("spd", "drnl"):
            sub = _expand(E, [_graph(E, n, ei)], h, node_label=label)
            for k in ("orig_node", "orig_edge", "node_to_subgraph", "edge_index"):
                assert np.array_equal(sub[k].cpu().numpy(), want[k]), (name, k)
            assert np.array_equal(sub.z.cpu().numpy(), want["z_" + label].reshape(sub.z.shape)), (name, label)
            assert np.array_equal(sub.x.cpu().numpy(), want["orig_node"])             # x = arange(n): the original ids
        one = create_subgraphs(_graph(E, n, ei), h, node_label="spd", use_rd=True)     # the reference's entry point, CPU tensors
        assert one.edge_index.device.type == "cpu" and np.array_equal(one.edge_index.numpy(), want["edge_index"])
        assert sorted(one.keys) == sorted(["x", "edge_index", "edge_attr", "z", "rd", "node_to_subgraph", "subgraph_to_graph",
                                           "num_subgraphs", "node_id", "original_edge_index", "original_edge_attr",
                                           "original_num_nodes", "y"]), one.keys
        assert one.num_subgraphs == n and np.array_equal(one.node_id.numpy(), np.flatnonzero(np.r_[True, np.diff(want["node_to_subgraph"]) != 0]))
        seen += 1
    assert seen >= 10


@pytest.fixture(scope="module")
def fresh_graphs(E):
    """n in {1, 2, 63, 64, 65, 130} (wavefront boundaries, more than two ballot chunks), a graph with no edges first and last,
    isolated nodes, directed graphs (asymmetric reach), self loops and repeated edges, and 40 molecules so that the batch has
    more than 1024 roots (the scan's chunk)"""
    from esc_gnn_amd.datasets import synthetic_zinc_graphs
    rng = np.random.RandomState(5)
    gs = [(5, np.zeros((2, 0), dtype=np.int64))]
    for n in (1, 2, 63, 64, 65, 130):
        gs.append((n, _ring(rng, n, n // 8)))
    gs.append((10, _sym([(1, 3), (3, 7)])))                                                    # isolated nodes
    gs.append((30, np.stack([rng.randint(0, 30, 60), rng.randint(0, 30, 60)]).astype(np.int64)))     # directed
    gs.append((66, np.stack([rng.randint(0, 66, 90), rng.randint(0, 66, 90)]).astype(np.int64)))     # directed, two chunks
    loops = np.concatenate([_sym([(0, 1), (1, 2), (2, 0), (2, 3), (4, 5)]), np.array([[0, 3, 1, 1, 7], [0, 3, 2, 2, 7]])], axis=1)
    gs.append((8, loops))                                                                    # self loops, a repeated edge
    gs += [(int(d.num_nodes), d.edge_index.numpy()) for d in synthetic_zinc_graphs(100, 40)]
    gs.append((3, np.zeros((2, 0), dtype=np.int64)))
    assert sum(n for n, _ in gs) > 1024 + 64
    return gs


@pytest.mark.parametrize("h", [1, 2, 3, 98], ids=lambda h: "h%d" % h)
def test_expansion_fresh_sweep_against_oracle(E, fresh_graphs, h):
    from esc_gnn_amd.subgraphs import subgraph_sizes
    gs = fresh_graphs if h != 98 else fresh_graphs[:12]            # h above every diameter (the ring of 130 has 65): the whole graph
    want = no.expand_batch([n for n, _ in gs], [ei for _, ei in gs], h)
    graphs = [_graph(E, n, ei) for n, ei in gs]
    sub = _expand(E, graphs, h)
    _check_integers(sub, want, h, what="h=%d" % h)
    sizes = subgraph_sizes(graphs, h)
    node_ptr = np.cumsum([0] + [n for n, _ in gs])
    assert sizes.dtype == torch.int64 and sizes.device.type == "cpu"
    assert np.array_equal(sizes[:, 0].numpy(), np.diff(want["sub_node_ptr"][node_ptr]))
    assert np.array_equal(sizes[:, 1].numpy(), np.diff(want["sub_edge_ptr"][node_ptr]))
    if h == 98:
        comp = sub.sub_node_ptr.cpu().numpy()
        assert int(comp[node_ptr[7]] - comp[node_ptr[6]]) == 130 * 130          # every root of the ring sees all of it


# ---- 2. rd -----------------------------------------------------------------------------------------------------------------
RD_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 95, 96)


@pytest.fixture(scope="module")
def rd_graphs():
    """connected graphs of m nodes expanded with h = m: every one of the m subgraphs is the whole graph (m x m Laplacian), plus
    a directed graph and the loops / repeats graph"""
    rng = np.random.RandomState(9)
    gs = [(m, _ring(rng, m, m // 6)) for m in RD_SIZES]
    gs.append((24, np.stack([rng.randint(0, 24, 60), rng.randint(0, 24, 60)]).astype(np.int64)))
    gs.append((4, np.concatenate([_sym([(0, 1), (1, 2), (2, 0), (2, 3)]), np.array([[0, 2, 1, 1], [0, 2, 2, 2]])], axis=1)))
    return gs


def _rd_reference(node_counts, edge_lists, h):
    """the oracle's expansion with rd from scipy.linalg.pinv, and atol = 10 x the largest fp64 difference to rd from
    numpy.linalg.pinv over the same subgraphs"""
    want = no.expand_batch(node_counts, edge_lists, h, use_rd=True)
    other = no.expand_batch(node_counts, edge_lists, h, use_rd=True, pinv=np.linalg.pinv)
    return want, 10.0 * float(np.abs(want["rd64"] - other["rd64"]).max())


def test_rd_against_scipy_pinv(E, rd_graphs):
    """|got - ref| <= 2^-23 |ref| + atol: both sides round an fp64 value to fp32 (one ulp), and atol = 10 x the largest
    difference between rd from numpy.linalg.pinv and from scipy.linalg.pinv (the reference's call) over these very subgraphs,
    computed here on the CPU in fp64 — what two correct fp64 pseudo-inverses disagree by near zero.  Measured on the test's
    subgraphs: the numpy / scipy difference is at most 8.9e-15 (atol 8.9e-14), on values up to 32.8.  The goldens' rd
    (directed graphs included) are held to the same bound.  The root's value is exactly 0."""
    h = 96
    want, atol = _rd_reference([n for n, _ in rd_graphs], [ei for _, ei in rd_graphs], h)
    sizes = np.diff(want["sub_node_ptr"])
    assert set(RD_SIZES) <= set(int(s) for s in sizes)
    print("rd: numpy-vs-scipy fp64 difference %.3g -> atol %.3g; largest |rd| %.3g" % (atol / 10, atol, float(np.abs(want["rd64"]).max())))
    assert 0 < atol < 1e-9
    sub = _expand(E, [_graph(E, n, ei) for n, ei in rd_graphs], h, use_rd=True)
    _check_integers(sub, want, h, what="rd graphs")
    got = sub.rd.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (want["rd"].shape[0], 1)
    got = got.reshape(-1).astype(np.float64)
    ref = want["rd"].astype(np.float64)
    err = np.abs(got - ref)
    bound = 2.0 ** -23 * np.abs(ref) + atol
    print("rd: worst error / bound %.3g" % float((err / bound).max()))
    assert bool((err <= bound).all()), (float((err - bound).max()), int(np.argmax(err - bound)))
    assert bool((got[want["sub_node_ptr"][:-1]] == 0.0).all())
    for name, n, ei, hh, gold in subgraph_golden_cases():
        g = _expand(E, [_graph(E, n, ei)], hh, use_rd=True).rd.cpu().numpy().reshape(-1).astype(np.float64)
        r = gold["rd"].astype(np.float64)
        assert bool((np.abs(g - r) <= 2.0 ** -23 * np.abs(r) + atol).all()), (name, float(np.abs(g - r).max()))


def test_rd_above_96_nodes_raises_and_names_the_limit(E):
    rng = np.random.RandomState(2)
    g = _graph(E, 97, _ring(rng, 97, 0))
    with pytest.raises(ValueError, match="use_rd, a subgraph of more than 96 nodes") as err:
        _expand(E, [g], 98, use_rd=True)
    assert "node id" not in str(err.value)                                    # the message names the limit that was hit
    from esc_gnn_amd.subgraphs import PlainGraphStore
    store = PlainGraphStore([g], 98, DEV)                                     # the driver's path: refused on the host, at no step's cost
    assert store.largest_subgraph == 97
    with pytest.raises(ValueError, match="at most 96 nodes"):
        store.expand(store.collate([0]), "spd", True)
    assert store.expand(store.collate([0]), "spd", False).z.size(0) == 97 * 97
    sub = _expand(E, [g], 98, use_rd=False)                                  # without rd the same subgraphs are fine
    assert sub.z.size(0) == 97 * 97


# ---- 3. the collated batch -------------------------------------------------------------------------------------------------
def test_collate_ngnn3_equals_the_reference_batch_without_a_host_copy(E):
    from esc_gnn_amd.subgraphs import collate_graphs, expand_subgraphs, subgraph_sizes
    raws, want, h = load_collate_ngnn3()
    graphs = [_graph(E, r["x"].shape[0], r["edge_index"], r["x"], r["edge_attr"], r["y"]) for r in raws]
    sizes = subgraph_sizes(graphs, h)                                        # once, at dataset build
    assert sizes[:, 0].sum() == want["x"].shape[0] and sizes[:, 1].sum() == want["edge_index"].shape[1]
    batch = collate_graphs(graphs, DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                  # any device-to-host copy that waits now raises
    try:
        sub = expand_subgraphs(batch, h, "spd", True, sizes)
        with pytest.raises(RuntimeError):                                    # the probe is live: without `sizes` the totals are read back
            expand_subgraphs(batch, h, "spd", True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for k in ("x", "z", "node_to_subgraph", "edge_index", "edge_attr", "subgraph_to_graph", "batch", "orig_node", "orig_edge"):
        got = sub[k].cpu().numpy()
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), k
    assert np.array_equal(sub.y.cpu().numpy().reshape(-1), want["y"].reshape(-1)) and sub.num_subgraphs == sum(r["x"].shape[0] for r in raws)
    got, ref = sub.rd.cpu().numpy().astype(np.float64), want["rd"].astype(np.float64)
    _, atol = _rd_reference([r["x"].shape[0] for r in raws], [r["edge_index"] for r in raws], h)      # as test_rd_against_scipy_pinv
    assert got.shape == ref.shape and bool((np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref) + atol).all()), float(np.abs(got - ref).max())
    assert int(sub.status.abs().sum()) == 0
    # a batch without the collate's pointers (any Batch with x / edge_index / batch): the same expansion
    plain = E.Batch.from_data_list(graphs).to(DEV)
    for kw in (dict(), dict(max_nodes=max(r["x"].shape[0] for r in raws))):   # the LDS tables sized by a bound from `sizes`, or exactly
        again = expand_subgraphs(plain, h, "spd", True, sizes, **kw)
        assert torch.equal(again.edge_index, sub.edge_index) and torch.equal(again.z, sub.z)
        assert bool(((again.rd - sub.rd).abs() <= 2.0 ** -23 * sub.rd.abs()).all())


# ---- 4. segment_first --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 64, 130])
def test_segment_first_forward_backward_bit_equal(E, C):
    lens = [1, 2, 65, 1, 65, 2, 1]
    ptr = torch.tensor(np.cumsum([0] + lens), dtype=torch.int64)
    seg = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens))
    g = torch.Generator().manual_seed(C)
    x = torch.randn(int(ptr[-1]), C, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    out = E.ops.segment_first(xd, ptr.to(DEV), seg.to(DEV))
    assert torch.equal(out.detach().cpu(), x[ptr[:-1]])
    dout = torch.randn(len(lens), C, generator=g)
    out.backward(dout.to(DEV))
    want = torch.zeros_like(x)
    want[ptr[:-1]] = dout
    assert torch.equal(xd.grad.cpu(), want)
    # every row is written, rows off the segment starts exactly zero: raw call on a buffer pre-filled with NaN
    from esc_gnn_amd import _native as nv
    dx = torch.full((x.size(0), C), float("nan"), device=DEV)
    dd, pd, sd = dout.to(DEV), ptr.to(DEV), seg.to(DEV)
    nv.call("esc_segment_first_bwd", nv.ptr(dd), C, nv.ptr(pd), nv.ptr(sd), x.size(0), C, nv.ptr(dx), nv.stream())
    assert torch.equal(dx.cpu(), want)
    off = torch.ones(x.size(0), dtype=torch.bool)
    off[ptr[:-1]] = False
    assert bool((dx.cpu()[off] == 0).all())


# ---- 5. model ----------------------------------------------------------------------------------------------------------------
def _model_batch(E, b):
    d = E.Data(x=b["x"].to(DEV), edge_index=b["edge_index"].to(DEV), edge_attr=b["edge_attr"].to(DEV), z=b["z"].to(DEV),
               rd=b["rd"].to(DEV), node_to_subgraph=b["node_to_subgraph"].to(DEV), subgraph_to_graph=b["subgraph_to_graph"].to(DEV))
    first = np.unique(b["node_to_subgraph"].numpy(), return_index=True)[1]
    d.sub_node_ptr = torch.tensor(np.r_[first, b["x"].shape[0]], dtype=torch.int64, device=DEV)
    return d


@pytest.mark.parametrize("pooling,use_rd", [("mean", False), ("mean", True), ("center", False), ("center", True)])
def test_ngnn_against_reference_golden_and_fp64_oracle(E, pooling, use_rd):
    from esc_gnn_amd.zinc_models import NGNN
    from test_hip_model import _close
    from test_hip_zinc_cycle import _grad_errors
    torch.set_num_threads(1)
    z, b, _, _, tag = next(r for r in ngnn_golden_runs() if (r[2], r[3]) == (pooling, use_rd))
    ref = no.ngnn_from_recipe(z["seed"], z["layers"], pooling, use_rd)
    m = NGNN(None, num_layers=int(z["layers"]), subgraph_pooling=pooling, use_rd=use_rd)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in z[tag + "/keys"]]
    assert ["x".join(map(str, v.shape)) or "scalar" for v in sd.values()] == [str(s) for s in z[tag + "/shapes"]]
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).train()
    y = torch.tensor(z["y"])
    out = m(_model_batch(E, b))
    loss = E.ops.l1_loss(out, y.to(DEV))
    loss.backward()
    _close(out, torch.tensor(z[tag + "/pred"]), "ngnn predictions " + tag)
    assert abs(float(loss.detach()) - float(z[tag + "/loss"])) <= 1e-5
    ref.train()
    args = no.model_args(b)
    torch.nn.functional.l1_loss(ref(*args), y).backward()
    ref64 = copy.deepcopy(ref).double(); ref64.zero_grad()
    p64 = ref64(*args)
    l64 = torch.nn.functional.l1_loss(p64, y.double()); l64.backward()
    _close(out, p64, "ngnn predictions vs fp64 " + tag)
    assert abs(float(loss.detach()) - float(l64.detach())) <= 1e-5 * max(1.0, abs(float(l64.detach())))
    g32 = {n: p.grad for n, p in ref.named_parameters()}
    g64 = {n: p.grad for n, p in ref64.named_parameters()}
    errs = _grad_errors(m.named_parameters(), g32, g64)
    print("ngnn %s: worst gradient error vs fp64 %.3g (fp32 oracle %.3g)" % (tag, max(e[0] for e in errs.values()),
                                                                             max(e[1] for e in errs.values())))
    bad = {n: e for n, e in errs.items() if e[0] > max(1e-5, 3 * e[1])}
    assert not bad, bad


def test_ngnn_eval_mode_one_graph_batch(E):
    from esc_gnn_amd.subgraphs import collate_graphs, expand_subgraphs
    from esc_gnn_amd.zinc_models import NGNN
    from test_hip_model import _close
    z, _, pooling, use_rd, tag = [r for r in ngnn_golden_runs()][1]                    # mean pooling with rd
    raws, _, h = load_collate_ngnn3()
    r = raws[1]
    ref = no.ngnn_from_recipe(z["seed"], z["layers"], pooling, use_rd).eval()
    m = NGNN(None, num_layers=int(z["layers"]), subgraph_pooling=pooling, use_rd=use_rd)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    sub = expand_subgraphs(collate_graphs([_graph(E, r["x"].shape[0], r["edge_index"], r["x"], r["edge_attr"], r["y"])], DEV), h, "spd", True)
    with torch.no_grad():
        got = m(sub)
        want = ref(sub.x.cpu(), sub.z.cpu(), sub.rd.cpu(), sub.edge_index.cpu(), sub.edge_attr.cpu(), sub.node_to_subgraph.cpu(),
                   sub.subgraph_to_graph.cpu())
    assert got.shape == (1, 1)
    _close(got, want, "one-graph eval")


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------
def test_bad_node_id_is_erange_and_writes_nothing_for_that_graph(E):
    from esc_gnn_amd import _native as nv
    from esc_gnn_amd.subgraphs import collate_graphs, expand_subgraphs
    rng = np.random.RandomState(4)
    graphs = [_graph(E, 6, _ring(rng, 6, 2)), _graph(E, 7, _ring(rng, 7, 2)), _graph(E, 5, _ring(rng, 5, 1))]
    batch = collate_graphs(graphs, DEV)
    e_bad = int(graphs[0].edge_index.size(1)) + 3
    batch.edge_index[1, e_bad] = 13                                           # the first node of the NEXT graph
    with pytest.raises(ValueError, match="graph 1 .*node id outside the graph") as err:
        expand_subgraphs(batch, 2)
    assert "use_rd" not in str(err.value)
    sub = expand_subgraphs(batch, 2, check=False)
    assert sub.status.cpu().tolist() == [0, nv.ESC_ERANGE, 0]
    ptr = sub.sub_node_ptr.cpu().numpy()
    assert bool((np.diff(ptr)[6:13] == 0).all()) and bool((np.diff(sub.sub_edge_ptr.cpu().numpy())[6:13] == 0).all())
    good = no.expand_batch([6, 5], [graphs[0].edge_index.numpy(), graphs[2].edge_index.numpy()], 2)
    total = int(ptr[-1])
    assert total == good["orig_node"].shape[0]                                # nothing of graph 1 among the rows
    got = sub.orig_node[:total].cpu().numpy()
    assert np.array_equal(got, np.where(good["orig_node"] >= 6, good["orig_node"] + 7, good["orig_node"]))
    assert not bool(((got >= 6) & (got < 13)).any())


@pytest.mark.parametrize("h", [0, 99])
def test_h_outside_1_to_98(E, h):
    from esc_gnn_amd import _native as nv
    g = _graph(E, 4, _sym([(0, 1), (1, 2)]))
    with pytest.raises(ValueError, match="1..98"):
        _expand(E, [g], h)
    ptrs = torch.tensor([0, 4], device=DEV)
    ei = g.edge_index.to(DEV)
    out = torch.zeros(5, dtype=torch.int64, device=DEV)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match=r"outside 1\.\.98"):                # the entry point itself
        nv.call("esc_subgraph_count", nv.ptr(ptrs), nv.ptr(ptrs), nv.ptr(ei[0].contiguous()), nv.ptr(ei[1].contiguous()), 1, 4, 4, 4,
                h, nv.ptr(out), nv.ptr(out), nv.ptr(st), nv.stream())


def test_node_label_hop_and_unsupported_arguments_raise(E):
    from esc_gnn_amd.utils import create_subgraphs
    g = _graph(E, 4, _sym([(0, 1), (1, 2)]))
    with pytest.raises(ValueError, match="hop"):
        _expand(E, [g], 2, node_label="hop")
    with pytest.raises(ValueError, match="hop"):
        create_subgraphs(g, 2)                                                # the reference's default label
    with pytest.raises(NotImplementedError):
        _expand(E, [g], 2, max_nodes_per_hop=3)
    with pytest.raises(NotImplementedError):
        _expand(E, [g], 2, subgraph_pretransform=lambda d: d)
    from esc_gnn_amd.zinc_models import NGNN
    for kw in (dict(use_pos=True), dict(RNI=True)):
        with pytest.raises(NotImplementedError):
            NGNN(None, **kw)
    from esc_gnn_amd.engine import zinc_engine_supports
    assert zinc_engine_supports(NGNN(None, num_layers=2).to(DEV)) is False


# ---- 7. driver ---------------------------------------------------------------------------------------------------------------
def test_run_zinc_ngnn_two_epochs(E, tmp_path, monkeypatch, capsys):
    import re
    import esc_gnn_amd.run_zinc as rz
    monkeypatch.chdir(tmp_path)
    rz.main("--model NGNN --h 2 --layers 2 --epochs 2 --synthetic_graphs 48 --batch_size 16 --save_appendix _t".split())
    out = capsys.readouterr().out
    assert "Using NGNN model" in out and "Epoch: 001" in out and "Validation MAE" in out      # (later epochs are logged when validation improves)
    nums = [float(v) for line in out.splitlines() if line.startswith("Epoch:") for v in re.findall(r"[-+]?\d+\.\d+(?:e[-+]?\d+)?", line)]
    assert nums and all(np.isfinite(v) for v in nums), out
    res = os.path.join(tmp_path, "results", "zinc_NGNN_t")
    assert "model_checkpoint2.pth" in os.listdir(res) and "log.txt" in os.listdir(res)
    sd = torch.load(os.path.join(res, "model_checkpoint2.pth"), map_location="cpu")
    assert sd["node_type_embedding.weight"].shape == (100, 8) and sd["convs.1.mlp.0.weight"].shape == (256, 128)
    assert sd["rd_projection_list.0.weight"].shape == (9, 1)                  # use_rd is on by default, as in the reference
