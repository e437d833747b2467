"""ZINC cycle counting on the MI355X: the cycle-label kernel (csrc/cycles.hip) bit-exact against networkx, the node-level
NestedGIN_eff (zinc_cycle_models, esc_zinc_* with node_readout = 1) against the reference golden and an fp64 oracle at
the driver's shape (bs 256, 6 layers: the two-stream edge pipeline) and at a one-stream size, the graph-sharded
SyncBN step on two ranks, and the run_zinc_cycle driver end to end."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLDEN, ROOT, load_collate, require_gpu
import zinc_cycle_oracle as zco

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def _kernel(node_counts, edge_lists):
    from esc_gnn_amd.cycles import cycle_counts_edge_lists
    return [t.numpy() for t in cycle_counts_edge_lists(node_counts, [torch.as_tensor(e) for e in edge_lists])]


def _check_against_networkx(node_counts, edge_lists):
    got = _kernel(node_counts, edge_lists)
    for g, (n, ei) in enumerate(zip(node_counts, edge_lists)):
        assert np.array_equal(got[g], zco.cycle_labels(n, ei)), g
    return got


# ---- the label kernel --------------------------------------------------------------------------------------------------
def test_cycle_kernel_hand_cases(E):
    from test_zinc_cycle_cpu import hand_cases
    cases = hand_cases()
    got = _check_against_networkx([c[1] for c in cases], [c[2] for c in cases])
    for (name, n, ei, want), g in zip(cases, got):
        assert np.array_equal(g, want), name


def test_cycle_kernel_collate_graphs(E):
    ns, eis = [], []
    for tag in ("zinc3", "molhiv4"):
        gs, _, _ = load_collate(tag)
        ns += [int(g["x"].shape[0]) for g in gs]
        eis += [g["edge_index"] for g in gs]
    got = _check_against_networkx(ns, eis)
    assert sum(float(g.sum()) for g in got) > 0


def test_cycle_kernel_synthetic_molecules(E):
    from esc_gnn_amd.datasets import _ring_closing_edges, synthetic_zinc_cycle_graphs
    ns, eis = [], []
    for g in range(2000):
        n, ei, _ = _ring_closing_edges(90000 + g)
        ns.append(n)
        eis.append(ei)
    got = _check_against_networkx(ns, eis)
    allc = np.concatenate(got)
    assert ((allc > 0).sum(axis=0) > 0).all()                  # every ring size occurs
    again = _kernel(ns, eis)                                   # deterministic
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    ds = synthetic_zinc_cycle_graphs(0, 40)                    # the dataset's y is the kernel's labels
    for g, d in enumerate(ds):
        assert d.y.dtype == torch.float32 and np.array_equal(d.y.numpy(), got[g])


def test_cycle_kernel_count_shaped_regular_graphs(E):
    from esc_gnn_amd.datasets import count_shape_adjacency
    ns, eis = [], []
    for g in range(200):
        A = count_shape_adjacency(g)
        ns.append(A.shape[0])
        eis.append(np.stack(np.where(A == 1.0)).astype(np.int64))
    _check_against_networkx(ns, eis)


def test_cycle_kernel_size_limit(E):
    import networkx as nx
    G64 = nx.random_regular_graph(3, 64, seed=11)
    ei64 = _und_edges(G64.edges())
    ring = np.array([[i for i in range(64)], [(i + 1) % 64 for i in range(64)]], dtype=np.int64)
    small = np.array([[0, 1, 2], [1, 2, 0]], dtype=np.int64)
    _check_against_networkx([64, 64, 3], [ei64, ring, small])
    ei65 = np.array([[i for i in range(65)], [(i + 1) % 65 for i in range(65)]], dtype=np.int64)
    with pytest.raises(ValueError, match="65 nodes"):
        _kernel([3, 65], [small, ei65])
    with pytest.raises(ValueError, match="outside"):
        _kernel([3], [np.array([[0, 1], [1, 3]], dtype=np.int64)])
    none = np.zeros((2, 0), dtype=np.int64)
    got = _kernel([4, 3], [none, small])                       # an edgeless graph, beside one with edges
    assert got[0].shape == (4, 4) and not got[0].any() and np.array_equal(got[1], zco.cycle_labels(3, small))
    got = _kernel([5], [none])                                 # no edge at all in the call
    assert got[0].shape == (5, 4) and not got[0].any()
    assert _kernel([], []) == []


def _und_edges(pairs):
    s = {(int(a), int(b)) for a, b in pairs}
    return np.array(sorted(s | {(b, a) for a, b in s}), dtype=np.int64).T


# ---- the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step_engine", [False, True], ids=["per_op", "engine"])
def test_zinc_cycle_model_against_reference_golden(E, step_engine):
    from esc_gnn_amd.zinc_cycle_models import NestedGIN_eff as CycleModel
    from test_hip_model import _close, _close_grad
    torch.set_num_threads(1)
    z = np.load(os.path.join(GOLDEN, "model_zinc_cycle.npz"))
    ref = zco.zinc_cycle_oracle_from_recipe(z)
    m = CycleModel(None, int(z["layers"]))
    assert list(m.state_dict().keys()) == [str(k) for k in z["keys"]]
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).train()
    m.step_engine = step_engine
    _, b, _ = load_collate("zinc3")
    bt = {k: torch.tensor(v) for k, v in b.items()}
    y = torch.tensor(z["labels"][:, int(z["target"])])
    out = m(E.Data(**{k: v.clone() for k, v in bt.items()}))
    assert out.shape == (bt["x"].numel(), 1)
    assert (type(out.grad_fn).__name__ == "_EngineNodeBackward") == step_engine
    loss = E.ops.l1_loss(out, y.to(DEV))
    loss.backward()
    _close(out, torch.tensor(z["pred"]), "zinc cycle predictions")
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-5
    ref.train()
    args = (bt["x"], bt["edge_index"], bt["edge_attr"], bt["pos_enc"], bt["pos_index"], bt["pos_batch"], bt["batch"])
    torch.nn.functional.l1_loss(ref(*args), y.view(-1, 1)).backward()
    ref64 = copy.deepcopy(ref).double(); ref64.zero_grad()
    torch.nn.functional.l1_loss(ref64(*args), y.double().view(-1, 1)).backward()
    rp, rp64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    for n, p in m.named_parameters():
        _close_grad(n, p.grad, rp[n].grad, rp64[n].grad)


def _grad_errors(named, g32, g64):
    """per parameter: (error of its .grad vs fp64, fp32-oracle error vs fp64), both relative to max(1, |fp64|max)"""
    out = {}
    for n, p in named:
        g, truth = p.grad, g64[n]
        sc = max(1.0, float(truth.abs().max()))
        out[n] = (float((g.detach().cpu().double() - truth).abs().max()) / sc, float((g32[n].double() - truth).abs().max()) / sc)
    return out


@pytest.mark.parametrize("bs,L", [(256, 6), (16, 3)], ids=["bs256_L6_two_stream", "bs16_L3_one_stream"])
def test_zinc_cycle_full_size_step(E, bs, L):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_cycle_graphs
    from esc_gnn_amd.engine import ZincStepEngine
    from esc_gnn_amd.zinc_cycle_models import NestedGIN_eff as CycleModel
    target = 1
    graphs = build_feature_dataset(synthetic_zinc_cycle_graphs(0, bs), 3, use_rd=True, self_loop=False)
    store = E.DeviceGraphStore(graphs, DEV)
    b = store.collate(torch.arange(bs))
    assert (b.edge_index.size(1) >= 12000) == (bs == 256)        # the engine's two-stream threshold
    y = b.y[:, target].contiguous()
    assert float(y.abs().sum()) > 0
    torch.manual_seed(46)
    ref = zco.NestedGINEffZincCycleRef(L)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            if p.dim() == 1 and "bias" not in n:
                p.add_(0.1 * torch.randn_like(p))
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    mine = CycleModel(None, L)
    mine.load_state_dict(sd)
    mine = mine.to(DEV).train()
    cpu = {k: b[k].cpu() for k in ("x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch")}
    args = (cpu["x"], cpu["edge_index"], cpu["edge_attr"], cpu["pos_enc"], cpu["pos_index"], cpu["pos_batch"], cpu["batch"])
    yc = y.cpu().view(-1, 1)
    ref.train()
    torch.nn.functional.l1_loss(ref(*args), yc).backward()
    ref64 = copy.deepcopy(ref).double(); ref64.zero_grad()
    p64 = ref64(*args)
    l64 = torch.nn.functional.l1_loss(p64, yc.double()); l64.backward()
    g32 = {n: p.grad for n, p in ref.named_parameters()}
    g64 = {n: p.grad for n, p in ref64.named_parameters()}
    # the training step through the engine node: predictions, loss, every gradient as accurate as the fp32 oracle
    out = mine(b)
    assert type(out.grad_fn).__name__ == "_EngineNodeBackward" and out.shape == (b.x.numel(), 1)
    loss = E.ops.l1_loss(out, y)
    loss.backward()
    scale = max(1.0, float(p64.abs().max()))
    assert float((out.detach().cpu().double() - p64.detach()).abs().max()) / scale <= 1e-5
    assert abs(float(loss.detach()) - float(l64.detach())) <= 1e-5 * max(1.0, abs(float(l64.detach())))
    errs = _grad_errors(mine.named_parameters(), g32, g64)
    bad = {n: e for n, e in errs.items() if e[0] > max(1e-5, 3 * e[1])}
    print("bs %d L %d: worst gradient error vs fp64 %.3g (fp32 oracle %.3g)" % (
        bs, L, max(e[0] for e in errs.values()), max(e[1] for e in errs.values())))
    assert not bad, bad
    # ZincStepEngine.train_step (the driver's path) equals the per-op autograd step
    per_op = CycleModel(None, L); per_op.load_state_dict(sd); per_op = per_op.to(DEV).train()
    per_op.step_engine = False
    lp = E.ops.l1_loss(per_op(b), y); lp.backward()
    eng_m = CycleModel(None, L); eng_m.load_state_dict(sd); eng_m = eng_m.to(DEV).train()
    le, pe = ZincStepEngine(eng_m).train_step(b, y=y, return_pred=True)
    assert pe.shape == (b.x.numel(), 1)
    assert abs(float(le) - float(lp.detach())) <= 1e-5 * max(1.0, abs(float(lp.detach())))
    for (n, pa), (_, pb) in zip(per_op.named_parameters(), eng_m.named_parameters()):
        sc = max(1.0, float(g64[n].abs().max()))
        d = float((pa.grad - pb.grad).abs().max()) / sc
        assert d <= max(1e-5, 6 * errs[n][1]), (n, d, errs[n][1])
    for (n, ba), (_, bb) in zip(per_op.named_buffers(), eng_m.named_buffers()):
        assert torch.allclose(ba.float(), bb.float(), rtol=1e-5, atol=1e-6), n
    # eval on the module's running statistics vs the fp64 oracle on the same buffers: 1e-5
    mine.eval()
    ev64 = copy.deepcopy(ref).double()
    ev64.load_state_dict({k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
                          for k, v in mine.state_dict().items()})
    ev64.eval()
    with torch.no_grad():
        e_m = mine(store.collate(torch.arange(bs)))
        e_r = ev64(*args)
    assert e_m.shape == (b.x.numel(), 1)
    assert float((e_m.cpu().double() - e_r).abs().max()) <= 1e-5 * max(1.0, float(e_r.abs().max()))


# ---- graph-sharded data parallelism with SyncBN: node-count denominators -----------------------------------------------
def _dp_setup(E):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_cycle_graphs
    from esc_gnn_amd.zinc_cycle_models import NestedGIN_eff as CycleModel
    graphs = build_feature_dataset(synthetic_zinc_cycle_graphs(0, 10), 2, use_rd=True, self_loop=False)
    store = E.DeviceGraphStore(graphs, DEV)
    torch.manual_seed(9)
    return store, CycleModel(None, 2).to(DEV).train()


def _dp_worker(rank, world, port, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import esc_gnn_amd as E
    from esc_gnn_amd.engine import ZincStepEngine
    store, model = _dp_setup(E)
    E.nn.BatchNorm1d.convert_sync(model)                        # run_zinc_cycle --sync_bn
    opt = E.optim.FlatAdam(model.parameters(), lr=1e-3)
    lo, hi = E.parallel.shard_slice(len(store), rank, world)
    b = store.collate(torch.arange(len(store))[lo:hi])
    y = b.y[:, 2].contiguous()
    s = ZincStepEngine(model).train_step(b, loss_denom=1, y=y)  # sum form, exactly as the driver
    n_all = opt.all_reduce_sum(y.numel())
    grad = (opt.flat_grad / n_all).clone()
    tot = s.detach().reshape(1).clone()
    dist.all_reduce(tot)
    torch.cuda.synchronize()
    q.put((rank, grad.cpu().numpy(), float(tot) / float(n_all), float(n_all)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_syncbn_node_level_step_equals_single_device(E):
    from esc_gnn_amd.engine import ZincStepEngine
    world, port = 2, 29400 + os.getpid() % 300
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    store, model = _dp_setup(E)
    opt = E.optim.FlatAdam(model.parameters(), lr=1e-3)
    b = store.collate(torch.arange(len(store)))
    y = b.y[:, 2].contiguous()
    loss = ZincStepEngine(model).train_step(b, y=y)             # default denominator: the N nodes of the batch
    want = opt.flat_grad.cpu().numpy()
    assert res[0][3] == float(b.x.numel())                       # the global NODE count
    assert abs(res[0][2] - float(loss)) <= 1e-6 * max(1.0, abs(float(loss)))
    for r in range(world):
        err = np.abs(res[r][1] - want).max()
        assert err <= 1e-5 * max(1.0, np.abs(want).max()), (r, err)


# ---- the driver --------------------------------------------------------------------------------------------------------
def test_run_zinc_cycle_driver_two_epochs(E, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "esc_gnn_amd.run_zinc_cycle", "--epochs", "2", "--synthetic_graphs", "600",
           "--batch_size", "64", "--save_appendix", "_t"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Mean = " in r.stdout and "Epoch: 001" in r.stdout
    res = tmp_path / "results" / "zinc_NestedGIN_eff_t"
    log = (res / "log.txt").read_text()
    loss = float(log.splitlines()[0].split("Loss: ")[1].split(",")[0])
    assert np.isfinite(loss)
    assert (res / "model_checkpoint2.pth").exists()
