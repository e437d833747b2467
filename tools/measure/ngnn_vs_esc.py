"""ms per training step of run_zinc's two models on the same synthetic split, measured the way the driver runs them:
`--model NGNN` (host collate of the plain batch -> device expansion into rooted subgraphs with rd -> per-op forward, L1,
backward, FlatAdam) and `--model NestedGIN_eff` (device collate -> ZincStepEngine.train_step -> FlatAdam).  --h 3 --layers 5
--batch_size 256, both with use_rd.  The two are alternated in one process, each window lasts about a second and ends in
a device synchronise, and the expansion alone is timed as well.  Writes profiles-style text to the path given as argv[1] (default: stdout only).

    python tools/measure/ngnn_vs_esc.py [out.txt]
"""
import os
import sys
import time

import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]      # the repo root
import esc_gnn_amd as E  # noqa: E402
from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs  # noqa: E402
from esc_gnn_amd.engine import ZincStepEngine  # noqa: E402
from esc_gnn_amd.subgraphs import PlainGraphStore  # noqa: E402
from esc_gnn_amd.zinc_models import NGNN, NestedGIN_eff  # noqa: E402

DEV, H, LAYERS, BS, GRAPHS, WARM, ROUNDS = "cuda:0", 3, 5, 256, 1024, 8, 3
STEPS = {"ngnn": 100, "eff": 400, "expand": 400}          # every window lasts about a second or more
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
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.manual_seed(1)
    raw = synthetic_zinc_graphs(0, GRAPHS)
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(GRAPHS // BS)]
    t0 = time.time()
    plain = PlainGraphStore(raw, H, DEV)
    t_sizes = time.time() - t0
    t0 = time.time()
    esc = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, GRAPHS), H, use_rd=True, self_loop=False), DEV)
    t_feat = time.time() - t0

    ngnn = NGNN(None, num_layers=LAYERS, subgraph_pooling="mean", use_rd=True).to(DEV).train()
    opt_n = E.optim.FlatAdam(ngnn.parameters(), lr=1e-3)

    def step_ngnn(i):
        data = plain.expand(plain.collate(ids[i % len(ids)]), "spd", True)
        opt_n.zero_grad()
        loss = E.ops.l1_loss(ngnn(data), data.y.view(-1, 1))
        loss.backward()
        opt_n.step()

    def expand_only(i):
        plain.expand(plain.collate(ids[i % len(ids)]), "spd", True)

    eff = NestedGIN_eff(None, num_layers=LAYERS, use_rd=True).to(DEV).train()
    opt_e = E.optim.FlatAdam(eff.parameters(), lr=1e-3)
    eng = ZincStepEngine(eff)

    def step_eff(i):
        eng.train_step(esc.collate(ids[i % len(ids)]))
        opt_e.step()

    say("run_zinc on %d synthetic molecules, --h %d --layers %d --batch_size %d, use_rd on both; %d warm-up steps, windows of %d "
        "(NGNN) / %d (NestedGIN_eff, expansion alone) steps, %d alternations; host clock around a window that ends in a device "
        "synchronise" % (GRAPHS, H, LAYERS, BS, WARM, STEPS["ngnn"], STEPS["eff"], ROUNDS))
    say("one-off per split: NGNN subgraph sizes (one count pass) %.2f s; NestedGIN_eff ESC feature build %.2f s" % (t_sizes, t_feat))
    for k, i in enumerate(ids):
        b = plain.collate(i)
        d = plain.expand(b, "spd", True)
        e = esc.collate(i)
        say("batch %d: %d nodes, %d edges -> NGNN %d sub-nodes, %d sub-edges (%.1fx, %.1fx); NestedGIN_eff %d nodes, %d edges, %d bag entries"
            % (k, b.x.size(0), b.edge_index.size(1), d.z.size(0), d.edge_index.size(1), d.z.size(0) / b.x.size(0),
               d.edge_index.size(1) / b.edge_index.size(1), e.x.size(0), e.edge_index.size(1), e.pos_enc.numel()))
    window(step_ngnn, WARM), window(step_eff, WARM), window(expand_only, WARM)
    res = {"ngnn": [], "eff": [], "expand": []}
    for _ in range(ROUNDS):
        res["ngnn"].append(window(step_ngnn, STEPS["ngnn"]))
        res["eff"].append(window(step_eff, STEPS["eff"]))
        res["expand"].append(window(expand_only, STEPS["expand"]))
    fmt = lambda v: ", ".join("%.3f" % x for x in v)  # noqa: E731
    say("--model NGNN            ms/step: %s  (median %.3f)" % (fmt(res["ngnn"]), sorted(res["ngnn"])[ROUNDS // 2]))
    say("   of which host collate + device expansion with rd, alone: %s" % fmt(res["expand"]))
    say("--model NestedGIN_eff   ms/step: %s  (median %.3f)" % (fmt(res["eff"]), sorted(res["eff"])[ROUNDS // 2]))
    say("ratio NGNN / NestedGIN_eff (medians): %.2f" % (sorted(res["ngnn"])[ROUNDS // 2] / sorted(res["eff"])[ROUNDS // 2]))
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
