"""QM9 on the MI355X: the geometry kernels (csrc/geometry.hip: esc_edge_distance, esc_node_input_fwd / _bwd, esc_mse_loss)
against the reference goldens and torch, the per-op NestedGIN_eff (qm9_models) against the reference golden and an fp64
oracle, the device store / loader with the QM9 keys against the host collate, and the run_qm9 driver end to end."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_collate, require_gpu
import qm9_oracle as qo
from test_qm9_cpu import distance_golden_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ESC_EINVAL = -1


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


class DS(object):
    num_features = qo.NUM_FEATURES


# ---- Distance ----------------------------------------------------------------------------------------------------------
def _torch_distance(pos, ei, ea, norm=True, max_value=None, cat=True, relative_pos=False, squared=False):
    """the reference formula (distance.py:29-47) in torch fp32 on the host"""
    row, col = ei[0], ei[1]
    rel = pos[col] - pos[row]
    dist = ((rel ** 2).sum(1) if squared else torch.norm(rel, p=2, dim=-1)).view(-1, 1)
    if norm and dist.numel() > 0:
        dist = dist / (dist.max() if max_value is None else max_value)
    out = torch.cat([ea, dist], dim=-1) if (ea is not None and cat) else dist
    return torch.cat([out, rel], dim=-1) if relative_pos else out


def _check_distance(got, want, n_attr, relative_pos, what):
    """bond columns and relative positions bit-exact, the distance column within rtol 1e-6 (atol 0), NaN where the
    reference has NaN.  Three squares, two adds and a square root put each side within 2^-23 of the exact value and the
    normalising division doubles that: 4.8e-7; 1e-6 is twice it."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got[:, :n_attr], want[:, :n_attr]), what
    if relative_pos:
        assert torch.equal(got[:, n_attr + 1:], want[:, n_attr + 1:]), what
    d, w = got[:, n_attr].double(), want[:, n_attr].double()
    assert torch.equal(torch.isnan(d), torch.isnan(w)), what
    ok = ~torch.isnan(w)
    err = (d[ok] - w[ok]).abs()
    assert bool((err <= 1e-6 * w[ok].abs()).all()), (what, float((err / w[ok].abs().clamp(min=1e-30)).max()))


def test_distance_against_reference_golden(E):
    from esc_gnn_amd.geometry import Distance, edge_distance_many
    datas, wants, metas = [], [], []
    for name, pos, ei, ea, flags, want in distance_golden_cases():
        d = E.Data(pos=torch.tensor(pos), edge_index=torch.tensor(ei), edge_attr=None if ea is None else torch.tensor(ea))
        got = Distance(**flags)(d).edge_attr                               # one graph, the reference's signature
        n_attr = ea.shape[1] if (ea is not None and flags["cat"]) else 0
        _check_distance(got, torch.tensor(want), n_attr, flags["relative_pos"], name)
        if name == "self_loops_only":
            assert bool(torch.isnan(got[:, n_attr]).all())
        if flags == dict(norm=True, squared=False, relative_pos=False, cat=True, max_value=None) and ea is not None:
            datas.append(E.Data(pos=torch.tensor(pos), edge_index=torch.tensor(ei), edge_attr=torch.tensor(ea)))
            wants.append(torch.tensor(want)); metas.append((name, n_attr))
    assert len(datas) >= 3
    for d, want, (name, n_attr) in zip(edge_distance_many(datas), wants, metas):   # the same graphs in ONE launch
        _check_distance(d.edge_attr, want, n_attr, False, name + " (many)")


def _random_graph(rng, n, m, scale=1.3, offset=0.0):
    pos = torch.tensor(rng.randn(n, 3).astype(np.float32) * scale + offset)
    ei = torch.tensor(np.stack([rng.randint(0, n, size=m), rng.randint(0, n, size=m)]).astype(np.int64))
    ea = torch.zeros(m, 4)
    ea[torch.arange(m), torch.tensor(rng.randint(0, 4, size=m))] = 1.0
    return pos, ei, ea


@pytest.fixture(scope="module")
def fresh_graphs():
    """edge counts 0, 1, 2, 63, 64, 65, 257, 1100 (wavefront and workgroup boundaries), first and last graph empty, the
    maximum on the last edge, tied maxima, |pos| ~ 1e3, and uneven graphs up to about 300 in all"""
    rng = np.random.RandomState(3)
    graphs = [_random_graph(rng, 5, 0)]
    for m in (1, 2, 63, 64, 65, 257, 1100):
        graphs.append(_random_graph(rng, 4 + m % 37, m))
    pos, ei, ea = _random_graph(rng, 9, 70)                                # the maximum on the last edge
    pos = torch.cat([pos, torch.tensor([[50.0, -40.0, 30.0]])])
    ei = torch.cat([ei, torch.tensor([[0], [9]])], dim=1)
    graphs.append((pos, ei, torch.cat([ea, ea[:1]])))
    pos = torch.tensor([[0., 0., 0.], [3., 4., 0.], [-3., -4., 0.], [1., 1., 1.]])      # tied maxima (5, 5, and twins)
    ei = torch.tensor([[0, 1, 0, 2, 0, 3], [1, 0, 2, 0, 3, 0]])
    graphs.append((pos, ei, torch.eye(4)[[0, 0, 1, 1, 2, 2]]))
    graphs.append(_random_graph(rng, 20, 90, scale=1.0, offset=1000.0))    # |pos| ~ 1e3
    graphs.append(_random_graph(rng, 20, 90, scale=1000.0))
    while len(graphs) < 299:
        graphs.append(_random_graph(rng, int(rng.randint(1, 40)), int(rng.randint(0, 140))))
    graphs.append(_random_graph(rng, 3, 0))
    return graphs


FLAG_SETS = [dict(), dict(squared=True), dict(norm=False), dict(relative_pos=True), dict(max_value=2.5), dict(cat=False),
             dict(norm=False, squared=True, relative_pos=True), dict(cat=False, relative_pos=True, max_value=0.5)]


@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "-".join("%s=%s" % kv for kv in sorted(f.items())) or "default")
def test_distance_fresh_graphs_one_launch(E, fresh_graphs, flags):
    from esc_gnn_amd.geometry import edge_distance_many
    assert [g[1].size(1) for g in fresh_graphs[:8]] == [0, 1, 2, 63, 64, 65, 257, 1100] and fresh_graphs[-1][1].size(1) == 0
    datas = [E.Data(pos=p.clone(), edge_index=e.clone(), edge_attr=a.clone()) for p, e, a in fresh_graphs]
    out = edge_distance_many(datas, **flags)
    assert len(out) == len(fresh_graphs) >= 300
    rel = bool(flags.get("relative_pos"))
    n_attr = 4 if flags.get("cat", True) else 0
    for g, (d, (p, e, a)) in enumerate(zip(out, fresh_graphs)):
        _check_distance(d.edge_attr, _torch_distance(p, e, a, **flags), n_attr, rel, "graph %d" % g)
    if not flags:
        last = out[8].edge_attr[:, 4]
        assert float(last[-1]) == 1.0 and float(last[:-1].max()) < 1.0     # the maximum sits on the last edge
        assert out[9].edge_attr[:, 4].tolist() == [1.0, 1.0, 1.0, 1.0] + [float(out[9].edge_attr[4, 4])] * 2


def test_distance_bad_node_id_is_an_error_and_writes_nothing(E):
    from esc_gnn_amd import _native as nv
    from esc_gnn_amd.geometry import edge_distance_arrays
    rng = np.random.RandomState(5)
    parts = [_random_graph(rng, 6, 10), _random_graph(rng, 6, 70), _random_graph(rng, 6, 10)]
    parts[1][1][1, 69] = 6                                                  # one past the graph's last node
    pos = torch.cat([p[0] for p in parts]).to(DEV)
    ei = torch.cat([p[1] for p in parts], dim=1).to(DEV)
    node_ptr = torch.tensor([0, 6, 12, 18], device=DEV)
    edge_ptr = torch.tensor([0, 10, 80, 90], device=DEV)
    with pytest.raises(ValueError, match="graph 1"):
        edge_distance_arrays(pos, ei[0].contiguous(), ei[1].contiguous(), node_ptr, edge_ptr)
    out = torch.full((90, 4), -7.0, device=DEV)
    status = torch.zeros(3, dtype=torch.int32, device=DEV)
    src, dst = ei[0].contiguous(), ei[1].contiguous()
    nv.call("esc_edge_distance", nv.ptr(pos), 3, nv.ptr(src), nv.ptr(dst), nv.ptr(node_ptr), nv.ptr(edge_ptr), 3, 18, 90,
            1, 0, 1, 0, 0.0, nv.ptr(out), 4, 0, nv.ptr(status), nv.stream())
    assert status.tolist() == [0, ESC_EINVAL, 0]
    out = out.cpu()
    assert bool((out[10:80] == -7.0).all())                                # nothing of the bad graph was written
    assert bool((out[:10] != -7.0).all()) and bool((out[80:] != -7.0).all())
    neg = ei.clone(); neg[0, 3] = -1
    with pytest.raises(ValueError, match="graph 0"):
        edge_distance_arrays(pos, neg[0].contiguous(), neg[1].contiguous(), node_ptr, edge_ptr)


# ---- node input --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 8, 13])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 300])
def test_node_input_forward_backward(E, N, F):
    g = torch.Generator().manual_seed(100 * N + F)
    wide_x, wide_p = torch.randn(N, F + 5, generator=g), torch.randn(N, 6, generator=g)
    table = torch.randn(5, F + 3, generator=g)
    types = torch.tensor([0, 2, 4])[torch.randint(0, 3, (N,), generator=g)]         # rows 1 and 3 are never hit
    want = torch.cat([wide_x[:, 2:2 + F], wide_p[:, 1:4]], 1) + table[types]
    td = table.to(DEV).requires_grad_(True)
    xd, pd = wide_x.to(DEV), wide_p.to(DEV)
    for x, p in ((xd[:, 2:2 + F], pd[:, 1:4]),                                       # views with a leading dimension
                 (xd[:, 2:2 + F].contiguous(), pd[:, 1:4].contiguous())):
        out = E.ops.node_input(x, p, types.to(DEV), td)
        assert torch.equal(out.detach().cpu(), want)                                 # one fp32 add per element
    grad = torch.randn(N, F + 3, generator=g)
    out.backward(grad.to(DEV))
    truth = torch.zeros(5, F + 3, dtype=torch.float64).index_add_(0, types, grad.double())
    mass = torch.zeros(5, F + 3, dtype=torch.float64).index_add_(0, types, grad.double().abs())
    hits = torch.bincount(types, minlength=5).double().view(-1, 1)
    bound = (hits - 1).clamp(min=0) * 2.0 ** -24 * mass
    got = td.grad.cpu().double()
    assert bool(((got - truth).abs() <= bound).all()), float(((got - truth).abs() - bound).max())
    assert bool((td.grad.cpu()[[1, 3]] == 0).all())                                  # rows never hit: exactly 0
    assert bool((td.grad.cpu()[hits.view(-1) == 0] == 0).all())


def test_node_input_bad_type_raises(E):
    x, p, t = torch.randn(7, 8, device=DEV), torch.randn(7, 3, device=DEV), torch.randn(5, 11, device=DEV)
    for bad in (5, -1):
        types = torch.tensor([0, 1, 2, bad, 4, 0, 1], device=DEV)
        with pytest.raises(IndexError):
            E.ops.node_input(x, p, types, t)


# ---- MSE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,denom", [(1, None), (2, None), (64, None), (65, None), (1000, None), (65, 7), (1000, 4096)])
def test_mse_loss(E, M, denom):
    from esc_gnn_amd import _native as nv
    g = torch.Generator().manual_seed(M)
    pred, y = torch.randn(M, generator=g) * 3, torch.randn(M, generator=g)
    d = denom or M
    p_ref = pred.clone().requires_grad_(True)
    (l_ref := torch.nn.functional.mse_loss(p_ref, y, reduction="sum") / d).backward()
    truth = float(((pred.double() - y.double()) ** 2).sum() / d)
    pd = pred.to(DEV).requires_grad_(True)
    loss = E.ops.mse_loss(pd, y.to(DEV), denom)
    loss.backward()
    assert loss.shape == () and abs(float(loss.detach()) - truth) <= 2.0 ** -23 * abs(truth)
    got, want = pd.grad.cpu().double(), p_ref.grad.double()
    assert bool(((got - want).abs() <= 1e-6 * want.abs()).all())                     # at most three fp32 roundings, 1.8e-7
    only = torch.empty(1, device=DEV)                                                # dpred = NULL is accepted
    yd = y.to(DEV)
    nv.call("esc_mse_loss", nv.ptr(pd.detach()), nv.ptr(yd), M, d, 1.0, nv.ptr(only), None, nv.stream())
    assert float(only) == float(loss.detach())
    p2 = pred.view(-1, 1).to(DEV).requires_grad_(True)                               # the gradient keeps the input's shape
    E.ops.mse_loss(p2, yd.view(-1, 1), denom).backward()
    assert p2.grad.shape == (M, 1) and torch.equal(p2.grad.view(-1), pd.grad)


# ---- the model ---------------------------------------------------------------------------------------------------------
def _golden_batch(z):
    _, b, G = load_collate("zinc3")
    b = {k: torch.tensor(v) for k, v in b.items()}
    b.update({k: torch.tensor(z["in/" + k]) for k in ("x", "pos", "node_type", "edge_attr", "y")})
    return b, G


def _data(E, b):
    keys = ("x", "pos", "node_type", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch", "y")
    return E.Data(**{k: b[k].clone() for k in keys})


def test_qm9_model_against_reference_golden(E):
    from esc_gnn_amd.qm9_models import NestedGIN_eff as Qm9Model
    from test_hip_model import _close, _close_grad
    torch.set_num_threads(1)
    z = np.load(os.path.join(GOLDEN, "model_qm9.npz"))
    ref = qo.qm9_oracle_from_recipe(z)
    m = Qm9Model(DS, int(z["layers"]))
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in z["keys"]]
    assert ["x".join(map(str, v.shape)) or "scalar" for v in sd.values()] == [str(s) for s in z["shapes"]]
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).train()
    b, G = _golden_batch(z)
    out = m(_data(E, b))
    assert out.shape == (G,)
    loss = E.ops.mse_loss(out, b["y"].to(DEV))
    loss.backward()
    _close(out, torch.tensor(z["pred"]), "qm9 predictions")
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5
    ref.train()
    args = qo.model_args(b)
    torch.nn.functional.mse_loss(ref(*args), b["y"]).backward()
    ref64 = copy.deepcopy(ref).double(); ref64.zero_grad()
    a64 = tuple(t.double() if t.is_floating_point() else t for t in args)
    torch.nn.functional.mse_loss(ref64(*a64), b["y"].double()).backward()
    rp, rp64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    for n, p in m.named_parameters():
        _close_grad(n, p.grad, rp[n].grad, rp64[n].grad)


def test_qm9_model_single_graph_eval_skips_bn_lin1(E):
    from esc_gnn_amd.qm9_models import NestedGIN_eff as Qm9Model
    from test_hip_model import _close
    z = np.load(os.path.join(GOLDEN, "model_qm9.npz"))
    ref = qo.qm9_oracle_from_recipe(z)
    with torch.no_grad():                                   # running statistics that differ from the identity
        for mod in ref.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(0, 0.1); mod.running_var.uniform_(0.5, 1.5)
        ref.bn_lin1.running_mean.fill_(100.0)               # ... and would wreck the output if bn_lin1 were applied
    m = Qm9Model(DS, int(z["layers"]))
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval(); ref.eval()
    b, _ = _golden_batch(z)
    n0 = int((b["batch"] == 0).sum()); e0 = int((b["edge_index"][0] < n0).sum()); z0 = int((b["pos_batch"] < e0).sum())
    one = dict(x=b["x"][:n0], pos=b["pos"][:n0], node_type=b["node_type"][:n0], edge_index=b["edge_index"][:, :e0],
               edge_attr=b["edge_attr"][:e0], pos_enc=b["pos_enc"][:z0], pos_index=b["pos_index"][:z0],
               pos_batch=b["pos_batch"][:z0], batch=b["batch"][:n0], y=b["y"][:1])
    assert int(one["edge_index"].max()) < n0 and int(one["pos_batch"].max()) == e0 - 1
    with torch.no_grad():
        got, want = m(_data(E, one)), ref(*qo.model_args(one))
    assert got.shape == (1,)
    _close(got, want, "single-graph eval")


def test_qm9_train_step_on_synthetic_molecules(E):
    from esc_gnn_amd.datasets import build_qm9_dataset, synthetic_qm9_graphs
    from esc_gnn_amd.qm9_models import NestedGIN_eff as Qm9Model
    from test_hip_zinc_cycle import _grad_errors
    L = 2
    graphs = build_qm9_dataset(synthetic_qm9_graphs(0, 8), 3, target=2)
    store = E.DeviceGraphStore(graphs, DEV)
    b = store.collate(torch.arange(8))
    assert b.edge_attr.shape[1] == 5 and b.y.shape == (8,)
    torch.manual_seed(46)
    ref = qo.perturb(qo.NestedGINEffQm9Ref(L))
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    mine = Qm9Model(DS, L)
    mine.load_state_dict(sd)
    mine = mine.to(DEV).train()
    cpu = {k: b[k].cpu() for k in ("x", "pos", "node_type", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
    args, yc = qo.model_args(cpu), b.y.cpu()
    ref.train()
    torch.nn.functional.mse_loss(ref(*args), yc).backward()
    ref64 = copy.deepcopy(ref).double(); ref64.zero_grad()
    p64 = ref64(*tuple(t.double() if t.is_floating_point() else t for t in args))
    l64 = torch.nn.functional.mse_loss(p64, yc.double()); l64.backward()
    g32 = {n: p.grad for n, p in ref.named_parameters()}
    g64 = {n: p.grad for n, p in ref64.named_parameters()}
    out = mine(b)
    assert out.shape == (8,)
    loss = E.ops.mse_loss(out, b.y)
    loss.backward()
    scale = max(1.0, float(p64.abs().max()))
    assert float((out.detach().cpu().double() - p64.detach()).abs().max()) / scale <= 1e-5
    assert abs(float(loss.detach()) - float(l64.detach())) <= 1e-5 * max(1.0, abs(float(l64.detach())))
    errs = _grad_errors(mine.named_parameters(), g32, g64)
    bad = {n: e for n, e in errs.items() if e[0] > max(1e-5, 3 * e[1])}
    print("qm9 8 molecules L %d: worst gradient error vs fp64 %.3g (fp32 oracle %.3g)" % (
        L, max(e[0] for e in errs.values()), max(e[1] for e in errs.values())))
    assert not bad, bad


# ---- store and loader --------------------------------------------------------------------------------------------------
BATCH_KEYS = ("x", "pos", "node_type", "edge_attr", "y", "batch", "edge_index", "pos_enc", "pos_index", "pos_batch")


def _same_batch(dev_b, host_b, what):
    assert sorted(dev_b.keys) == sorted(host_b.keys), what
    for k in BATCH_KEYS:
        a, h = dev_b[k], host_b[k]
        assert a.is_cuda and a.dtype == h.dtype and tuple(a.shape) == tuple(h.shape), (what, k, a.dtype, tuple(a.shape))
        assert torch.equal(a.cpu(), h), (what, k)
    assert list(dev_b.name) == list(host_b.name), what
    assert dev_b.num_graphs == host_b.num_graphs


@pytest.fixture(scope="module")
def qm9_graphs(E):
    from esc_gnn_amd.datasets import build_qm9_dataset, synthetic_qm9_graphs
    return build_qm9_dataset(synthetic_qm9_graphs(0, 12), 3, target=0)


@pytest.mark.parametrize("bs", [1, 5])
def test_loader_pins_qm9_graphs_and_equals_host_collate(E, qm9_graphs, bs):
    dev_loader = E.DataLoader(qm9_graphs, batch_size=bs, shuffle=True, generator=torch.Generator().manual_seed(11))
    host_loader = E.DataLoader(qm9_graphs, batch_size=bs, shuffle=True, generator=torch.Generator().manual_seed(11),
                               device=None)
    dev_batches, host_batches = list(dev_loader), list(host_loader)
    assert dev_loader._esc_store is not False and dev_loader._esc_store is not None
    assert host_loader._esc_store is False
    assert len(dev_batches) == len(host_batches) == (12 + bs - 1) // bs
    for i, (a, h) in enumerate(zip(dev_batches, host_batches)):
        _same_batch(a, h, "bs %d batch %d" % (bs, i))
    if bs == 5:
        assert dev_batches[-1].num_graphs == 2                              # the ragged last batch
        back = dev_batches[0].to_data_list()                                # ... and the way back
        assert len(back) == 5 and back[1].name == dev_batches[0].name[1]
        assert torch.equal(back[1].pos.cpu(), host_batches[0].to_data_list()[1].pos)


def test_store_reproduces_reference_qm9_collate(E):
    from esc_gnn_amd.datasets import build_qm9_dataset
    graphs, batch, G = load_collate("qm9_3")
    datas = [E.Data(**{k: (str(v) if k == "name" else torch.tensor(v)) for k, v in g.items()}) for g in graphs]
    b = E.DeviceGraphStore(datas, DEV).collate([0, 1, 2])
    for k in BATCH_KEYS:
        want = torch.tensor(batch[k])
        assert b[k].dtype == want.dtype and tuple(b[k].shape) == tuple(want.shape), k
        assert torch.equal(b[k].cpu(), want), k
    assert list(b.name) == [str(s) for s in batch["name"]]
    # the same three graphs through the device feature build and the distance kernel
    z = np.load(os.path.join(GOLDEN, "collate_qm9_3.npz"))
    raw = [E.Data(**{k: torch.tensor(z["raw%d_%s" % (j, k)]) for k in ("x", "edge_index", "edge_attr", "y", "pos", "node_type")},
                  name=str(graphs[j]["name"])) for j in range(3)]
    for d, g in zip(build_qm9_dataset(raw, 3, target=0), graphs):
        for k in ("x", "pos", "node_type", "edge_index", "pos_enc", "pos_index", "pos_batch", "y"):
            assert torch.equal(d[k], torch.tensor(g[k])), k
        _check_distance(d.edge_attr, torch.tensor(g["edge_attr"]), 4, False, "feature-built " + d.name)


# ---- the driver --------------------------------------------------------------------------------------------------------
LOG = re.compile(r"^Epoch: \d{3}, LR: [\d.]+, Loss: ([\d.einf+-]+|nan), Validation MAE: ([\d.einf+-]+|nan), "
                 r"Test MAE: ([\d.einf+-]+|nan), Test MAE norm: ([\d.einf+-]+|nan), Test MAE convert: ([\d.einf+-]+|nan)$")


def _run_driver(tmp_path, tag, convert):
    import esc_gnn_amd.run_qm9 as rq
    res = tmp_path / tag
    rq.main(["--data_size", "96", "--epochs", "2", "--layers", "2", "--batch_size", "16", "--target", "7", "--convert", convert,
             "--res_dir", str(res)])
    lines = (res / "log.txt").read_text().splitlines()
    assert lines
    for line in lines:
        m = LOG.match(line)
        assert m, line
        assert all(np.isfinite(float(v)) for v in m.groups()), line
    return res, lines


def test_run_qm9_driver(E, tmp_path):
    import esc_gnn_amd.run_qm9 as rq
    from esc_gnn_amd.qm9_models import NestedGIN_eff as Qm9Model
    res, post = _run_driver(tmp_path, "post", "post")
    conv = float(LOG.match(post[-1]).group(5)); mae = float(LOG.match(post[-1]).group(3))
    assert abs(conv - mae / rq.CONVERSION[7]) <= 1e-6 * max(1.0, mae)
    fresh = Qm9Model(DS, 2)
    fresh.load_state_dict(torch.load(str(res / "model_checkpoint2.pth"), map_location="cpu"))
    _, again = _run_driver(tmp_path, "again", "post")
    assert again == post                                                    # the same seed: the same log
    _, pre = _run_driver(tmp_path, "pre", "pre")
    assert float(LOG.match(pre[-1]).group(5)) == 0.0
    with pytest.raises(NotImplementedError, match="k1_GNN"):
        rq.main(["--model", "k1_GNN", "--res_dir", str(tmp_path / "no")])
    for extra in (["--RNI"], ["--max_nodes_per_hop", "10"]):
        with pytest.raises(NotImplementedError):
            rq.main(extra + ["--res_dir", str(tmp_path / "no")])
    assert not (tmp_path / "no").exists()
