"""ZINC cycle counting (run_zinc_cycle's defaults: bs 256, 6 layers, h 3): step time of the node-level engine
(ZincStepEngine.train_step + FlatAdam) against the per-op autograd path, and the cycle-label build for 12 000 molecules on
the device against networkx on a pool of host processes.  One JSON line per measurement.

    python tools/measure/zinc_cycle_time.py [steps|engine|labels] [--steps K] [--warmup W] [--procs P]

`engine` runs only the engine loop (the loop kept under `rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def _batch(bs, h, target):
    import esc_gnn_amd as E
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_cycle_graphs
    graphs = build_feature_dataset(synthetic_zinc_cycle_graphs(0, bs), h, use_rd=True, self_loop=False)
    store = E.DeviceGraphStore(graphs, "cuda:0")
    b = store.collate(torch.arange(bs))
    return E, b, b.y[:, target].contiguous()


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


def step_times(args, modes):
    from esc_gnn_amd.engine import ZincStepEngine
    from esc_gnn_amd.zinc_cycle_models import NestedGIN_eff
    E, b, y = _batch(args.bs, args.h, args.target)
    torch.manual_seed(0)
    for mode in modes:
        m = NestedGIN_eff(None, args.layers).to("cuda:0").train()
        opt = E.optim.FlatAdam(m.parameters(), lr=1e-4)
        if mode == "engine":
            eng = ZincStepEngine(m)

            def step():
                eng.train_step(b, y=y)
                opt.step()
        else:
            m.step_engine = False

            def step():
                opt.zero_grad()
                E.ops.l1_loss(m(b), y).backward()
                opt.step()
        ms = _time(step, args.steps, args.warmup)
        print(json.dumps(dict(what="zinc_cycle_step", mode=mode, bs=args.bs, layers=args.layers, nodes=int(b.x.numel()),
                              edges=int(b.edge_index.size(1)), ms_per_step=round(ms, 4))), flush=True)


def _nx_labels(item):
    import zinc_cycle_oracle as zco
    n, ei = item
    return zco.cycle_labels(n, ei)


def label_times(args):
    from multiprocessing import get_context
    from esc_gnn_amd.cycles import cycle_counts_edge_lists
    from esc_gnn_amd.datasets import _ring_closing_edges
    items = [_ring_closing_edges(90000 + g)[:2] for g in range(args.graphs)]
    eis = [torch.from_numpy(ei) for _, ei in items]
    ns = [n for n, _ in items]
    cycle_counts_edge_lists(ns[:64], eis[:64])                    # warm-up: code object load, allocator
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = cycle_counts_edge_lists(ns, eis)                    # host lists in, host tensors out (copies included)
        reps.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    with get_context("spawn").Pool(args.procs) as pool:
        want = pool.map(_nx_labels, items, chunksize=64)
    nx_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    print(json.dumps(dict(what="zinc_cycle_labels", graphs=args.graphs, device_ms_median=round(float(np.median(reps)), 3),
                          device_ms_all=[round(r, 3) for r in reps], networkx_ms=round(nx_ms, 1), networkx_procs=args.procs,
                          identical=same)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="steps", choices=("steps", "engine", "labels"))
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--h", type=int, default=3)
    ap.add_argument("--target", type=int, default=0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--graphs", type=int, default=12000)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    if args.what == "labels":
        label_times(args)
    elif args.what == "engine":
        step_times(args, ["engine"])
    else:
        step_times(args, ["engine", "per_op", "engine", "per_op"])   # alternated: the spread shows in the repeat


if __name__ == "__main__":
    main()
