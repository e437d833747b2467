"""The GINE+ baseline on the device: the multi-hop expansion (csrc/multihop.hip) against the reference's recorded output and the
numpy BFS, the one-launch aggregate (csrc/gineplus.hip) against an fp64 restatement and against the per-distance path it
replaces, ClassifierNetwork against the reference's record, and `run_ogb_mol --gnn gine+` end to end."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, require_gpu
import gineplus_cases as gp
import multihop_oracle as mo
from test_multihop_cpu import edge_cases, edge_golden, molecule_batch, net_golden, net_molecules, refnet_run, split_graphs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _graph(E, n, ei, x=None, edge_attr=None, y=None):
    return E.Data(x=torch.zeros(n, dtype=torch.int64) if x is None else torch.as_tensor(x), edge_index=torch.as_tensor(ei).reshape(2, -1),
                  edge_attr=None if edge_attr is None else torch.as_tensor(edge_attr), y=None if y is None else torch.as_tensor(y),
                  num_nodes=n)


def _expand(E, graphs, k):
    from esc_gnn_amd.multihop import make_multihop_edges
    from esc_gnn_amd.subgraphs import collate_graphs
    out = make_multihop_edges(collate_graphs(graphs, DEV), k)
    return out.multihop_edge_index, out.distance


# ---- expansion -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in mo.hand_cases()])
def test_expansion_equals_reference_and_oracle(E, name):
    z = edge_golden()
    rng = np.random.RandomState(len(name))
    done = 0
    for nm, ns, es, ei, k, mei, dist in edge_cases(z):
        if nm != name:
            continue
        locs = split_graphs(ns, es, ei)
        got_mei, got_dist = _expand(E, [_graph(E, n, e) for n, e in zip(ns, locs)], k)
        assert got_mei.dtype == torch.int64 and got_dist.dtype == torch.int64
        assert np.array_equal(got_mei.cpu().numpy(), mei) and np.array_equal(got_dist.cpu().numpy(), dist), (name, k)
        want = mo.multihop_batch(ns, locs, k)
        assert np.array_equal(got_mei.cpu().numpy(), want[0]) and np.array_equal(got_dist.cpu().numpy(), want[1]), (name, k)
        shuffled = [e[:, rng.permutation(e.shape[1])] for e in locs]         # the order of a graph's edges does not matter
        s_mei, s_dist = _expand(E, [_graph(E, n, e) for n, e in zip(ns, shuffled)], k)
        assert torch.equal(s_mei, got_mei) and torch.equal(s_dist, got_dist), (name, k, "shuffled")
        done += 1
    assert done == (1 if name == "star200" else 4)


def test_batch_without_edges_gives_empty_tensors(E):
    none = np.zeros((2, 0), dtype=np.int64)
    mei, dist = _expand(E, [_graph(E, 3, none), _graph(E, 1, none)], 3)
    assert tuple(mei.shape) == (2, 0) and tuple(dist.shape) == (0,) and mei.dtype == torch.int64 and dist.dtype == torch.int64


def test_expansion_of_more_than_1024_roots_against_oracle(E):
    """a batch shaped like the fresh sweeps of test_hip_ngnn.py and test_hip_i2gnn.py: a graph without edges first and last, a
    one-node graph, rings of 63, 64, 65 and 130 nodes (wavefront boundaries, more than two ballot chunks), a directed graph and 30
    molecules, so that the batch has more than 1024 + 64 roots and the two-array scan of esc_multihop_count carries"""
    from esc_gnn_amd.datasets import synthetic_zinc_graphs
    rng = np.random.RandomState(23)
    none = np.zeros((2, 0), dtype=np.int64)
    gs = [(5, none), (1, none)]
    for n in (63, 64, 65, 130):
        chords = [(int(a), int(b)) for a, b in rng.randint(0, n, (n // 8, 2)) if a != b]
        gs.append((n, mo._und([(i, (i + 1) % n) for i in range(n)] + chords)))
    gs.append((66, np.stack([rng.randint(0, 66, 140), rng.randint(0, 66, 140)]).astype(np.int64)))    # directed, three edge chunks
    gs += [(int(d.num_nodes), d.edge_index.numpy()) for d in synthetic_zinc_graphs(100, 30)]
    gs.append((3, none))
    assert sum(n for n, _ in gs) > 1024 + 64
    k = 2
    got_mei, got_dist = _expand(E, [_graph(E, n, ei) for n, ei in gs], k)
    want = mo.multihop_batch([n for n, _ in gs], [ei for _, ei in gs], k)
    assert got_mei.dtype == torch.int64 and got_dist.dtype == torch.int64
    assert np.array_equal(got_mei.cpu().numpy(), want[0]) and np.array_equal(got_dist.cpu().numpy(), want[1])
    plan = got_mei._esc_multihop_plan
    assert int(plan.status.abs().sum()) == 0
    # the two scanned arrays themselves: the pair ranges of the roots, and the ranks of the distance-1 pairs
    assert np.array_equal(plan.out_ptr.cpu().numpy(), np.searchsorted(want[0][0], np.arange(plan.num_nodes + 1)))
    meta, d1 = plan.meta.cpu().numpy(), want[1] == 1
    assert np.array_equal(meta[d1, 3], np.arange(d1.sum())) and (meta[~d1, 3] == -1).all()


def _molecule_graphs(E, raws):
    return [_graph(E, r["x"].shape[0], r["edge_index"], r["x"], r["edge_attr"], r["y"]) for r in raws]


def test_store_expands_the_molecule_batch_without_reading_back(E):
    from esc_gnn_amd.multihop import MultihopGraphStore, make_multihop_edges, multihop_sizes
    from esc_gnn_amd.subgraphs import collate_graphs
    raws, k, mei, dist = molecule_batch(edge_golden())
    graphs = _molecule_graphs(E, raws)
    sizes = multihop_sizes(graphs, k)                                        # once, at dataset build
    assert tuple(sizes.shape) == (3, k + 1) and sizes[:, 0].tolist() == [r["x"].shape[0] for r in raws]
    assert sizes.sum(dim=0).tolist() == np.bincount(dist, minlength=k + 1).tolist()
    store = MultihopGraphStore(graphs, k, DEV)
    sbatch = store.collate([0, 1, 2])
    plain = collate_graphs(graphs, DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                  # any device-to-host copy that waits now raises
    try:
        out = store.expand(sbatch)
        with pytest.raises(RuntimeError):                                    # the probe is live: without sizes the total is read back
            make_multihop_edges(plain, k)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert np.array_equal(out.multihop_edge_index.cpu().numpy(), mei) and np.array_equal(out.distance.cpu().numpy(), dist)
    plan = out.multihop_edge_index._esc_multihop_plan
    assert plan.counts == np.bincount(dist, minlength=k + 1).tolist() and plan.num_d1 == sum(r["edge_index"].shape[1] for r in raws)
    meta = plan.meta.cpu().numpy()
    assert np.array_equal(meta[:, 0], mei[0]) and np.array_equal(meta[:, 1], mei[1]) and np.array_equal(meta[:, 2], dist)
    d1 = dist == 1
    assert np.array_equal(meta[d1, 3], np.arange(d1.sum())) and (meta[~d1, 3] == -1).all()
    assert np.array_equal(plan.out_ptr.cpu().numpy(), np.searchsorted(mei[0], np.arange(plan.num_nodes + 1)))
    order = np.lexsort((mei[0], mei[1]))                                     # by destination, ascending source inside
    assert np.array_equal(plan.in_meta.cpu().numpy(), meta[order])
    assert np.array_equal(plan.in_ptr.cpu().numpy(), np.searchsorted(mei[1][order], np.arange(plan.num_nodes + 1)))
    assert int(plan.status.abs().sum()) == 0
    # a sub-batch in another order: the sizes follow the ids
    sub = store.expand(store.collate([2, 0]))
    want = mo.multihop_batch([raws[2]["x"].shape[0], raws[0]["x"].shape[0]], [raws[2]["edge_index"], raws[0]["edge_index"]], k)
    assert np.array_equal(sub.multihop_edge_index.cpu().numpy(), want[0]) and np.array_equal(sub.distance.cpu().numpy(), want[1])


def test_expansion_limits_raise_value_errors(E):
    from esc_gnn_amd.multihop import MAX_NODES, make_multihop_edges
    from esc_gnn_amd.subgraphs import collate_graphs
    tri = np.array([[0, 1, 2], [1, 2, 0]], dtype=np.int64)
    batch = collate_graphs([_graph(E, 3, tri), _graph(E, 3, tri)], DEV)
    with pytest.raises(ValueError, match="k=0"):
        make_multihop_edges(batch, 0)
    with pytest.raises(ValueError, match="k=9"):
        make_multihop_edges(batch, 9)
    big = collate_graphs([_graph(E, MAX_NODES + 1, np.array([[0], [1]], dtype=np.int64))], DEV)
    with pytest.raises(ValueError, match="%d nodes exceeds the limit of %d" % (MAX_NODES + 1, MAX_NODES)):
        make_multihop_edges(big, 2)
    bad = collate_graphs([_graph(E, 3, tri), _graph(E, 3, np.array([[0, 1], [1, 5]], dtype=np.int64))], DEV)
    with pytest.raises(ValueError, match="graph 1 cannot be expanded"):
        make_multihop_edges(bad, 2)


# ---- aggregate -------------------------------------------------------------------------------------------------------------
def _directed_graph():
    """40 nodes, 90 directed edges without loops or repeats, sorted by (row, col); nodes 36..39 isolated: the in-lists and the
    out-lists differ"""
    rng = np.random.RandomState(11)
    pairs = set()
    while len(pairs) < 90:
        a, b = (int(v) for v in rng.randint(0, 36, size=2))
        if a != b:
            pairs.add((a, b))
    return 40, np.array(sorted(pairs), dtype=np.int64).T


AGG_GRAPHS = {"star": lambda: (201, mo.hand_cases()[8][1][0][1]), "directed": _directed_graph,
              "single_node": lambda: (1, np.zeros((2, 0), dtype=np.int64))}
_agg_cache = {}


def _agg_plan(E, gname, k):
    """expansion of one of the three graphs at k (shared by the cases; never modified)"""
    if (gname, k) not in _agg_cache:
        n, ei = AGG_GRAPHS[gname]()
        mei, dist = _expand(E, [_graph(E, n, ei)], k)
        _agg_cache[(gname, k)] = (n, mei, dist, mei._esc_multihop_plan)
    return _agg_cache[(gname, k)]


def _agg_inputs(n, m1, k, C, seed):
    """x_t, e ~ N(0, 1); the output gradient g ~ N(0, 1 / n), the size a mean readout over n rows hands down"""
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, C, generator=gen) for _ in range(k)]
    return xs, torch.randn(m1, C, generator=gen), 0.3 * torch.randn(k + 1, C, generator=gen), torch.randn(n, C, generator=gen) / float(np.sqrt(n))


def _on_device(t, wide):
    """wide: the tensor becomes a column slice of a device tensor of 2C + 4 columns, 16 bytes in: leading dimension > C"""
    if not wide:
        return t.to(DEV)
    base = torch.zeros((t.size(0), 2 * t.size(1) + 4), device=DEV)
    view = base[:, 4:4 + t.size(1)]
    view.copy_(t)
    assert view.stride(0) == 2 * t.size(1) + 4 or t.size(0) <= 1
    return view.detach()


def _run_fused(E, plan, xs, e, eps, g, wide=False):
    xs = [_on_device(x, wide).requires_grad_(True) for x in xs]
    e, eps = _on_device(e, wide).requires_grad_(True), eps.to(DEV).requires_grad_(True)
    out = E.ops.gineplus_aggregate(xs, e, eps, plan)
    out.backward(_on_device(g, wide))
    return out.detach(), [x.grad for x in xs], e.grad, eps.grad


def _run_per_distance(E, mei, dist, k, xs, e, eps, g):
    """today's path: GINEPLUS on a plain pair of tensors (a clone carries no plan)"""
    from esc_gnn_amd.modules.gine_operations import GINEPLUS
    conv = GINEPLUS(torch.nn.Identity(), xs[0].size(1), k=k).to(DEV)
    with torch.no_grad():
        conv.eps.copy_(eps.to(DEV))
    xs = [x.to(DEV).requires_grad_(True) for x in xs]
    e = e.to(DEV).requires_grad_(True)
    out = conv(list(xs), mei.clone(), dist.clone(), e)[0]
    out.backward(g.to(DEV))
    return out.detach(), [x.grad for x in xs], e.grad, conv.eps.grad


def _run_fp64(mei, dist, k, xs, e, eps, g):
    xs = [x.double().requires_grad_(True) for x in xs]
    e, eps = e.double().requires_grad_(True), eps.double().requires_grad_(True)
    out = mo.aggregate64(xs, e, eps, mei.cpu(), dist.cpu(), k)
    out.backward(g.double())
    return out.detach(), [x.grad for x in xs], e.grad if e.grad is not None else torch.zeros_like(e), eps.grad


def _chk(got, want, what, tol=1e-5):
    got, want = got.detach().cpu().double(), want.detach().double()
    scale = max(1.0, float(want.abs().max())) if want.numel() else 1.0
    err = float((got - want).abs().max()) / scale if want.numel() else 0.0
    print("%s: max error %.3g of scale %.3g" % (what, err, scale))
    assert got.shape == want.shape and err <= tol, "%s: max error %.3g of scale %.3g > %g" % (what, err, scale, tol)


def _check_case(E, gname, k, C, wide=False):
    n, mei, dist, plan = _agg_plan(E, gname, k)
    xs, e, eps, g = _agg_inputs(n, plan.num_d1, k, C, 1000 * k + C)
    f_out, f_dx, f_de, f_deps = _run_fused(E, plan, xs, e, eps, g, wide)
    r_out, r_dx, r_de, r_deps = _run_fp64(mei, dist, k, xs, e, eps, g)
    tag = "%s k=%d C=%d " % (gname, k, C)
    _chk(f_out, r_out, tag + "forward")
    for t in range(k):
        _chk(f_dx[t], r_dx[t], tag + "dX_%d" % t)
    _chk(f_de, r_de, tag + "d_e")
    # d_eps: the bound of the kernels' own summation order (gineplus_cases.deps_depth; these shapes have at most 26 workgroups)
    c = dict(num_nodes=n, pairs=mei.cpu().numpy(), distance=dist.cpu().numpy())
    w_deps, mag = gp.deps64(c, k, xs, e, g)
    assert torch.allclose(w_deps, r_deps, rtol=1e-12, atol=1e-12)
    err, bound = (f_deps.cpu().double() - w_deps).abs(), gp.deps_bound(c, k, mag)
    assert bool((err <= bound).all()), tag + "d_eps: %.3g x its bound of depth %s" % (float((err / bound.clamp(min=1e-300)).max()), gp.deps_depth(c, k))
    p_out, p_dx, p_de, p_deps = _run_per_distance(E, mei, dist, k, xs, e, eps, g)
    assert torch.equal(f_out, p_out), tag + "forward must equal the per-distance path bit for bit"
    for t in range(k):
        assert torch.equal(f_dx[t], p_dx[t]), tag + "dX_%d must equal the per-distance path bit for bit" % t
    assert torch.equal(f_de, p_de), tag + "d_e must equal the per-distance path bit for bit"
    assert torch.allclose(p_deps.cpu().double(), r_deps, rtol=1e-5, atol=1e-4)
    _, dx2, de2, deps2 = _run_fused(E, plan, xs, e, eps, g, wide)                 # bit-stable from run to run
    assert all(torch.equal(a, b) for a, b in zip(f_dx, dx2)) and torch.equal(f_de, de2) and torch.equal(f_deps, deps2)


@pytest.mark.parametrize("C", [300, 64, 4, 7])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("gname", ["star", "directed", "single_node"])
def test_fused_aggregate_against_fp64_and_per_distance_path(E, gname, k, C):
    _check_case(E, gname, k, C)


@pytest.mark.parametrize("C", [300, 7])
def test_fused_aggregate_on_column_slices(E, C):
    """leading dimension 2C + 4: the vector path for C = 300 (slices start 16 bytes in), the scalar path for C = 7"""
    _check_case(E, "directed", 3, C, wide=True)


def test_fused_aggregate_with_one_tensor_for_every_distance(E):
    """NAIVEGINEPLUS: x_t = x for every t; autograd adds the k gradients, so dx is compared with fp64 only (its sum of three or
    more terms has no fixed order on either path)"""
    k, C = 3, 64
    n, mei, dist, plan = _agg_plan(E, "directed", k)
    xs, e, eps, g = _agg_inputs(n, plan.num_d1, k, C, 5)
    x = xs[0].to(DEV).requires_grad_(True)
    ed, epsd = e.to(DEV).requires_grad_(True), eps.to(DEV).requires_grad_(True)
    out = E.ops.gineplus_aggregate([x] * k, ed, epsd, plan)
    out.backward(g.to(DEV))
    x64, e64, eps64 = x.detach().cpu().double().requires_grad_(True), e.double().requires_grad_(True), eps.double().requires_grad_(True)
    r = mo.aggregate64([x64] * k, e64, eps64, mei.cpu(), dist.cpu(), k)
    r.backward(g.double())
    _chk(out, r, "naive forward")
    _chk(x.grad, x64.grad, "naive dx")
    _chk(ed.grad, e64.grad, "naive d_e")
    assert torch.allclose(epsd.grad.cpu().double(), eps64.grad, rtol=1e-5, atol=1e-4)


def _close(a, b, what, tol=1e-5):
    a, b = a.detach().cpu().double(), b.detach().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    print("%s: max scaled error %.3g" % (what, err))
    assert err <= tol, "%s: max scaled error %.3g > %g" % (what, err, tol)


@pytest.mark.parametrize("which", ["naive", "plus"])
def test_recorded_gineplus_case_through_the_fused_op(E, which):
    """tests/golden/model_gineplus.npz (the reference's own class bodies on random multi-hop pairs, one distance class beyond k)
    through MultihopPlan.from_tensors and the fused op, at the tolerances of test_gineplus_against_reference_class_golden"""
    from esc_gnn_amd.modules.gine_operations import GINEPLUS, NAIVEGINEPLUS
    from esc_gnn_amd.multihop import MultihopPlan
    g = np.load(os.path.join(GOLDEN, "model_gineplus.npz"))
    k = int(g["k"])
    dim = g[which + "_x0"].shape[1]
    fun = torch.nn.Sequential(E.Linear(dim, dim), torch.nn.ReLU(), E.Linear(dim, dim))
    conv = (NAIVEGINEPLUS if which == "naive" else GINEPLUS)(fun, dim, k=k).to(DEV)
    with torch.no_grad():
        for n, p in conv.named_parameters():
            p.copy_(torch.tensor(g["%s_param_%s" % (which, n)]))
    mei, dist = torch.tensor(g["multihop_edge_index"]).to(DEV), torch.tensor(g["distance"]).to(DEV)
    plan = MultihopPlan.from_tensors(mei, dist, g[which + "_x0"].shape[0], k)
    assert mei._esc_multihop_plan is plan and plan.num_d1 == g[which + "_edge_attr"].shape[0]
    ea = torch.tensor(g[which + "_edge_attr"]).to(DEV).requires_grad_(True)
    nx = 1 if which == "naive" else k + 1
    xs = [torch.tensor(g["%s_x%d" % (which, i)]).to(DEV).requires_grad_(True) for i in range(nx)]
    calls = []
    real = E.ops.gineplus_aggregate
    E.ops.gineplus_aggregate = lambda *a: calls.append(1) or real(*a)
    try:
        out = conv(xs[0], mei, dist, ea) if which == "naive" else conv(list(xs), mei, dist, ea)[0]
    finally:
        E.ops.gineplus_aggregate = real
    assert calls == [1], "a pair of tensors that carries a plan takes the fused op"
    (out * torch.tensor(g[which + "_w"]).to(DEV)).sum().backward()
    _close(out, torch.tensor(g[which + "_out"]), which + " forward")
    _close(ea.grad, torch.tensor(g[which + "_d_edge_attr"]), which + " d edge_attr")
    for i, x in enumerate(xs):
        got = x.grad if x.grad is not None else torch.zeros_like(x)
        _close(got, torch.tensor(g["%s_dx%d" % (which, i)]), "%s dx%d" % (which, i))
    for n, p in conv.named_parameters():
        _close(p.grad, torch.tensor(g["%s_grad_%s" % (which, n)]), "%s grad %s" % (which, n), tol=2e-5)


def test_edge_term_row_count_must_match_the_distance_1_pairs(E):
    n, mei, dist, plan = _agg_plan(E, "directed", 2)
    xs, e, eps, g = _agg_inputs(n, plan.num_d1 + 1, 2, 8, 3)
    with pytest.raises(ValueError, match="distance-1 pairs"):
        E.ops.gineplus_aggregate([x.to(DEV) for x in xs], e.to(DEV), eps.to(DEV), plan)
    with pytest.raises(ValueError, match="outside 1..4"):
        E.ops.gineplus_aggregate([xs[0].to(DEV)] * 5, e.to(DEV), eps.to(DEV), plan)


def test_k5_takes_the_per_distance_path_and_agrees_with_fp64(E):
    from esc_gnn_amd.modules.gine_operations import GINEPLUS
    k, C = 5, 12
    n, ei = _directed_graph()
    mei, dist = _expand(E, [_graph(E, n, ei)], k)
    plan = mei._esc_multihop_plan
    xs, e, eps, g = _agg_inputs(n, plan.num_d1, k, C, 77)
    conv = GINEPLUS(torch.nn.Identity(), C, k=k).to(DEV)
    with torch.no_grad():
        conv.eps.copy_(eps.to(DEV))
    xd = [x.to(DEV).requires_grad_(True) for x in xs]
    ed = e.to(DEV).requires_grad_(True)
    real = E.ops.gineplus_aggregate
    E.ops.gineplus_aggregate = None                                           # the fused op must not be reached
    try:
        out = conv(list(xd), mei, dist, ed)[0]
    finally:
        E.ops.gineplus_aggregate = real
    out.backward(g.to(DEV))
    r_out, r_dx, r_de, r_deps = _run_fp64(mei, dist, k, xs, e, eps, g)
    _chk(out, r_out, "k=5 forward")
    for t in range(k):
        _chk(xd[t].grad, r_dx[t], "k=5 dX_%d" % t)
    _chk(ed.grad, r_de, "k=5 d_e")
    assert torch.allclose(conv.eps.grad.cpu().double(), r_deps, rtol=1e-5, atol=1e-4)


# ---- model and driver -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,vn", mo.CONFIGS)
def test_classifier_network_against_the_reference_record(E, layers, vn):
    """HIP ClassifierNetwork on the recorded batch of 8 molecules: eval and train forward (dropout 0) within 1e-5 of scale of the
    reference's recorded predictions; every parameter gradient and BatchNorm buffer within 1e-4 of the restated network (which the
    recording held bit-equal to the reference's classes, tests/test_multihop_cpu.py pins it to the record); the same results with
    the plan made by the store and with make_multihop_edges called in forward"""
    from esc_gnn_amd.modules.gine_operations import ClassifierNetwork
    from esc_gnn_amd.multihop import MultihopGraphStore
    from esc_gnn_amd.subgraphs import collate_graphs
    rec = net_golden()
    tag = "L%d_vn%d" % (layers, int(vn))
    raws, k = net_molecules(rec), int(rec["k"])
    ref, ref_eval, ref_train, ref_loss = refnet_run(layers, vn, rec)
    graphs = _molecule_graphs(E, raws)
    ids = list(range(len(graphs)))
    store = MultihopGraphStore(graphs, k, DEV)
    w = mo.loss_weights(len(graphs), mo.OUT_DIM).to(DEV)
    results = []
    for source in ("store", "forward"):
        m = ClassifierNetwork(hidden=mo.HIDDEN, out_dim=mo.OUT_DIM, layers=layers, dropout=0.0, virtual_node=vn, k=k, conv_type="gin+")
        m.load_state_dict(mo.fill_params(mo.RefNet(mo.HIDDEN, mo.OUT_DIM, layers, vn, k, "gin+")).state_dict())
        m = m.to(DEV)
        batch = (lambda: store.expand(store.collate(ids))) if source == "store" else (lambda: collate_graphs(graphs, DEV))
        m.eval()
        with torch.no_grad():
            ev = m(batch())
        m.train()
        pred = m(batch())
        (pred * w).sum().backward()
        results.append((m, ev, pred.detach()))
        _close(ev, torch.tensor(rec[tag + "/eval"]), tag + " eval forward (" + source + ")")
        _close(pred, torch.tensor(rec[tag + "/train"]), tag + " train forward (" + source + ")")
        refp, refb = dict(ref.named_parameters()), dict(ref.named_buffers())
        for n, p in m.named_parameters():
            assert p.grad is not None, n
            _close(p.grad, refp[n].grad, "grad " + n, tol=1e-4)
        for n, b in m.named_buffers():
            _close(b, refb[n], "buffer " + n, tol=1e-4)
    (m1, e1, p1), (m2, e2, p2) = results
    assert torch.equal(e1, e2) and torch.equal(p1, p2), "the store's plan and make_multihop_edges in forward give equal results"
    for (n, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a.grad, b.grad), n


def test_classifier_network_refuses_rooted_subgraphs(E):
    from esc_gnn_amd.modules.gine_operations import ClassifierNetwork
    from esc_gnn_amd.subgraphs import collate_graphs
    raws, k, _, _ = molecule_batch(edge_golden())
    batch = collate_graphs(_molecule_graphs(E, raws), DEV)
    batch.node_to_subgraph = batch.batch
    m = ClassifierNetwork(hidden=8, out_dim=1, layers=1, k=k, conv_type="gin+").to(DEV)
    with pytest.raises(NotImplementedError, match="node_to_subgraph"):
        m(batch)


@pytest.mark.parametrize("dataset", ["ogbg-molhiv", "ogbg-molpcba"])
def test_run_ogb_mol_gineplus_trains_and_checkpoints(E, dataset, tmp_path, monkeypatch):
    """two epochs of `run_ogb_mol --gnn gine+` on 64 stand-in molecules: finite logged losses, best-model and checkpoint files;
    ogbg-molpcba has 128 tasks with NaN (unlabelled) targets"""
    import re
    import esc_gnn_amd.run_ogb_mol as ro
    monkeypatch.chdir(tmp_path)
    ro.main(["--gnn", "gine+", "--dataset", dataset, "--runs", "1", "--epochs", "2", "--synthetic_graphs", "64", "--batch_size", "16",
             "--emb_dim", "32", "--num_layer", "3", "--log_steps", "1", "--save_appendix", "_t"])
    rdir = tmp_path / "results" / (dataset + "_t")
    rows = re.findall(r"'Epoch': (\d+), 'Loss': ([^,]+),", open(rdir / "log.txt").read())
    assert [int(r[0]) for r in rows] == [1, 2] and all(np.isfinite(float(r[1])) for r in rows), rows
    for f in ("run1_best_model.pth", "run1_model_checkpoint1.pth", "run1_model_checkpoint2.pth", "run1_optimizer_checkpoint2.pth"):
        assert (rdir / f).exists(), f
    sd = torch.load(rdir / "run1_best_model.pth", map_location="cpu")
    assert "main.1.conv.eps" in sd and tuple(sd["main.3.conv.eps"].shape) == (4, 32)
