"""Expressiveness runs (run_exp / run_sr defaults: 8 layers x 64, h 3, batches of 20) on the two data fixtures: the per-op
EXP training step, the SR25 evaluation, and the classification head alone (the fused esc_log_softmax_nll launch against
torch's log_softmax + nll_loss + backward on the same logits).  Device-event clock after warm-up, one JSON line per
measurement; alternated repeats show the spread.

    python tools/measure/expressive_time.py [step|sr|head|all] [--steps K] [--warmup W]

`step` alone is the loop kept under `rocprofv3 --kernel-trace`: the launch count per step is the difference of the
dispatch counts of two such runs with different --steps (and --warmup 0), divided by the difference of the step counts."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) / steps


def exp_step(args, repeats):
    import esc_gnn_amd as E
    from esc_gnn_amd.datasets import build_expressive_dataset, load_exp_txt
    from esc_gnn_amd.expressive_models import NestedGIN
    graphs = build_expressive_dataset(load_exp_txt(os.path.join(GOLDEN, "exp_first40.txt"), 20), 3)
    b = E.DeviceGraphStore(graphs, DEV).collate(torch.arange(20))
    y = b.y.view(-1).long()
    torch.manual_seed(0)
    m = NestedGIN(2, args.layers, args.width)
    m.reset_parameters()
    m = m.to(DEV).train()
    opt = E.optim.FlatAdam(m.parameters(), lr=1e-3)

    def step():
        opt.zero_grad()
        E.ops.log_softmax_nll(m.logits(b), y).backward()
        opt.step()
    for _ in range(repeats):
        ms = _time(step, args.steps, args.warmup)
        print(json.dumps(dict(what="exp_train_step", mode="per_op", graphs=20, layers=args.layers, width=args.width,
                              nodes=int(b.x.size(0)), edges=int(b.edge_index.size(1)), bag_entries=int(b.pos_index.numel()),
                              ms_per_step=round(ms, 4))), flush=True)


def sr_eval(args, repeats):
    import esc_gnn_amd as E
    from esc_gnn_amd.datasets import build_expressive_dataset, load_sr25
    from esc_gnn_amd.expressive_models import NestedGIN
    graphs = build_expressive_dataset(load_sr25(os.path.join(GOLDEN, "sr251256.g6")), 3)
    with_y = [E.Data(x=g.x, edge_index=g.edge_index, y=torch.zeros(1), pos_enc=g.pos_enc, pos_index=g.pos_index,
                     pos_batch=g.pos_batch) for g in graphs]
    b = E.DeviceGraphStore(with_y, DEV).collate(torch.arange(15))
    torch.manual_seed(1)
    m = NestedGIN(1, args.layers, args.width)
    m.reset_parameters()
    m = m.to(DEV).eval()
    res = {}

    def run():
        with torch.no_grad():
            res["wrong"] = E.ops.pdist(m(b), 1e-2)[1]          # forward of all 15 graphs + distances + count (one read-back)
    for _ in range(repeats):
        ms = _time(run, args.steps, args.warmup)
        print(json.dumps(dict(what="sr25_eval", graphs=15, nodes=int(b.x.size(0)), edges=int(b.edge_index.size(1)),
                              bag_entries=int(b.pos_index.numel()), wrong=res["wrong"], ms_per_eval=round(ms, 4))), flush=True)


def head(args, repeats):
    import esc_gnn_amd as E
    from esc_gnn_amd.ops import _head_raw
    for M in (20, 1014):
        g = torch.Generator().manual_seed(M)
        x = (torch.randn(M, 64, generator=g) * 10).to(DEV)
        t = torch.randint(0, 64, (M,), generator=g).to(DEV)

        def fused_raw():                                        # ONE launch: loss, logp, d loss / d logits (+ one read-back of the flag pair)
            _head_raw(x, t, 0, True)

        def fused_autograd():
            a = x.detach().requires_grad_(True)
            E.ops.log_softmax_nll(a, t).backward()

        def torch_ops():
            a = x.detach().requires_grad_(True)
            F.nll_loss(F.log_softmax(a, dim=1), t).backward()
        for _ in range(repeats):
            for name, fn in (("fused_one_launch", fused_raw), ("fused_autograd", fused_autograd), ("torch", torch_ops)):
                us = _time(fn, args.steps * 10, args.warmup * 10) * 1e3
                print(json.dumps(dict(what="classification_head", mode=name, M=M, C=64, us_per_call=round(us, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=("step", "sr", "head", "all"))
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.what in ("step", "all"):
        exp_step(args, args.repeats)
    if args.what in ("sr", "all"):
        sr_eval(args, args.repeats)
    if args.what in ("head", "all"):
        head(args, args.repeats)


if __name__ == "__main__":
    main()
