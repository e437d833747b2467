"""ms per training step of run_zinc_cycle's two models on the same synthetic split, measured the way the driver runs them:
`--model I2GNN` (host collate of the plain batch -> device expansion into one copy of every rooted subgraph per neighbour of
its root, with rd -> per-op forward, L1 over the nodes, backward, FlatAdam) and `--model NestedGIN_eff` (device collate ->
ZincStepEngine.train_step -> FlatAdam), both with the driver's default flags.  The two are alternated in one process, each
window ends in a device synchronise; the expansion (count + fill) and the pooling kernels are timed alone as well.  Writes
profiles-style text to the path given with --out (default: stdout only).

    python tools/measure/i2gnn_vs_esc.py --h 3 --layers 6 --batch_size 256 [--out out.txt]
"""
import argparse
import os
import sys
import time

import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]      # the repo root
import esc_gnn_amd as E  # noqa: E402
from esc_gnn_amd import ops  # noqa: E402
from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_cycle_graphs  # noqa: E402
from esc_gnn_amd.engine import ZincStepEngine  # noqa: E402
from esc_gnn_amd.subgraphs2 import I2GraphStore, expand_subgraphs2  # noqa: E402
from esc_gnn_amd.zinc_cycle_models import I2GNN, NestedGIN_eff  # noqa: E402

DEV, WARM, ROUNDS, TARGET = "cuda:0", 5, 3, 0
STEPS = {"i2": 30, "eff": 300, "expand": 200, "kernel": 200}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def window(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=3)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--batch_size", type=int, default=256)
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.manual_seed(1)
    H, BS, G = a.h, a.batch_size, a.graphs
    raw = synthetic_zinc_cycle_graphs(0, G)
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(G // BS)]
    t0 = time.time()
    plain = I2GraphStore(raw, H, True, DEV)
    t_sizes = time.time() - t0
    t0 = time.time()
    esc = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_cycle_graphs(0, G), H, use_rd=True, self_loop=False), DEV)
    t_feat = time.time() - t0

    i2 = I2GNN(None, num_layers=a.layers, subgraph_pooling="mean-context", subgraph2_pooling="mean-center-side", use_rd=True,
               double_pooling=True, gate=True).to(DEV).train()                     # the driver's defaults
    opt_i = E.optim.FlatAdam(i2.parameters(), lr=1e-3)

    def step_i2(i, split=True):
        i2.split_double_linear = split
        data = plain.expand(plain.collate(ids[i % len(ids)]))
        opt_i.zero_grad()
        loss = ops.l1_loss(i2(data), data.y[:, TARGET].contiguous().view(-1, 1))
        loss.backward()
        opt_i.step()

    def expand_with_collate(i):
        plain.expand(plain.collate(ids[i % len(ids)]))

    fixed = plain.collate(ids[0])
    sizes0 = plain.sizes[ids[0]]

    def expand_only(use_rd):
        return lambda i: expand_subgraphs2(fixed, H, use_rd, sizes0)

    eff = NestedGIN_eff(None, num_layers=a.layers, use_rd=True).to(DEV).train()
    opt_e = E.optim.FlatAdam(eff.parameters(), lr=1e-3)
    eng = ZincStepEngine(eff)

    def step_eff(i):
        data = esc.collate(ids[i % len(ids)])
        eng.train_step(data, y=data.y[:, TARGET].contiguous())
        opt_e.step()

    say("run_zinc_cycle on %d synthetic ring-closed molecules, --h %d --layers %d --batch_size %d --target %d, the driver's default "
        "flags (gate, double pooling, mean-context / mean-center-side, use_rd); %d warm-up steps, windows of %d (I2GNN) / %d "
        "(NestedGIN_eff) / %d (expansion, kernels alone) steps, %d alternations; host clock around a window that ends in a device "
        "synchronise" % (G, H, a.layers, BS, TARGET, WARM, STEPS["i2"], STEPS["eff"], STEPS["expand"], ROUNDS))
    say("one-off per split: I2GNN subgraph2 sizes (one count pass) %.2f s; NestedGIN_eff ESC feature build %.2f s" % (t_sizes, t_feat))
    for k, i in enumerate(ids):
        b = plain.collate(i)
        d = plain.expand(b)
        e = esc.collate(i)
        say("batch %d: %d nodes, %d edges -> I2GNN %d sub-nodes, %d sub-edges, %d subgraph2s (%.1fx, %.1fx, %.2f per node); "
            "NestedGIN_eff %d nodes, %d edges, %d bag entries"
            % (k, b.x.size(0), b.edge_index.size(1), d.z.size(0), d.edge_index.size(1), d.num_subgraphs2, d.z.size(0) / b.x.size(0),
               d.edge_index.size(1) / b.edge_index.size(1), d.num_subgraphs2 / b.x.size(0), e.x.size(0), e.edge_index.size(1),
               e.pos_enc.numel()))
    # the pooling kernels alone, on the first batch's shapes at 64 columns
    d = plain.expand(fixed)
    Ns, S2, N = d.z.size(0), d.num_subgraphs2, d.num_subgraphs
    x = torch.randn(Ns, 64, device=DEV, requires_grad=True)
    av = torch.randn(Ns, 64, device=DEV, requires_grad=True)
    gp = ops.group_plan(d.node_to_original_node, N)
    ctx_rows = torch.randn(N, 256, device=DEV, requires_grad=True)
    g3, g1, gN, gB = (torch.randn(S2, 192, device=DEV), torch.randn(Ns, 64, device=DEV), torch.randn(N, 64, device=DEV),
                      torch.randn(Ns, 256, device=DEV))

    def fb(fn, inputs, grad):
        def run(i):
            out = fn()
            torch.autograd.grad(out, inputs, grad)
        return run
    kernels = [
        ("pool_mean_center_side fwd+bwd [%d x 64 -> %d x 192]" % (Ns, S2),
         fb(lambda: ops.pool_mean_center_side(x, d.s2_node_ptr, d.center_idx, d.node_to_subgraph2), [x], g3)),
        ("sigmoid_mul fwd+bwd [%d x 64]" % Ns, fb(lambda: ops.sigmoid_mul(av, x), [av, x], g1)),
        ("context mean over node_to_original_node fwd+bwd (esc_plan_csr grouping + esc_bag_fwd, unit counts) [%d x 64 -> %d x 64]" % (Ns, N),
         fb(lambda: ops.group_mean(x, gp), [x], gN)),
        ("gather back [node_to_original_node] fwd+bwd (the same grouping) [%d x 256 -> %d x 256]" % (N, Ns),
         fb(lambda: ops.gather_rows(ctx_rows, gp), [ctx_rows], gB)),
    ]
    window(step_i2, WARM), window(step_eff, WARM), window(expand_with_collate, WARM)
    window(lambda i: step_i2(i, False), WARM)
    res = {"i2": [], "i2_cat": [], "eff": [], "expand": [], "fill_rd": [], "fill_nord": []}
    for _ in range(ROUNDS):
        res["i2"].append(window(step_i2, STEPS["i2"]))
        res["i2_cat"].append(window(lambda i: step_i2(i, False), STEPS["i2"]))
        res["eff"].append(window(step_eff, STEPS["eff"]))
        res["expand"].append(window(expand_with_collate, STEPS["expand"]))
        res["fill_rd"].append(window(expand_only(True), STEPS["expand"]))
        res["fill_nord"].append(window(expand_only(False), STEPS["expand"]))
    fmt = lambda v: ", ".join("%.3f" % x for x in v)  # noqa: E731
    med = lambda v: sorted(v)[ROUNDS // 2]  # noqa: E731
    say("--model I2GNN           ms/step: %s  (median %.3f)" % (fmt(res["i2"]), med(res["i2"])))
    say("   with double_nns as Linear(cat[x, P[idx]]) on the expanded rows (split_double_linear = False): %s  (median %.3f)"
        % (fmt(res["i2_cat"]), med(res["i2_cat"])))
    say("   of which host collate + count + fill with rd, alone: %s" % fmt(res["expand"]))
    say("   count + fill with rd on a collated batch (no read-back):    %s" % fmt(res["fill_rd"]))
    say("   count + fill without rd on a collated batch:                %s" % fmt(res["fill_nord"]))
    say("--model NestedGIN_eff   ms/step: %s  (median %.3f)" % (fmt(res["eff"]), med(res["eff"])))
    say("ratio I2GNN / NestedGIN_eff (medians): %.2f" % (med(res["i2"]) / med(res["eff"])))
    for name, run in kernels:
        window(run, WARM)
        say("%s: %s ms" % (name, fmt([window(run, STEPS["kernel"]) for _ in range(ROUNDS)])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
