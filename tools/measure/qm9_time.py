"""QM9 (run_qm9's defaults: bs 64, 5 layers, h 3): per-step time of the per-op training loop with the device collate
included, the kernel launches per step, and the time of the Distance transform (esc_edge_distance) over the whole
synthetic set.  One JSON line per measurement.  There is no earlier counterpart to compare with: the numbers are recorded
for what they are.

    python tools/measure/qm9_time.py [steps|launches|distance] [--steps K] [--warmup W] [--graphs G]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]


class _Features(object):
    num_features = 8


def _setup(args):
    import esc_gnn_amd as E
    from esc_gnn_amd.datasets import build_qm9_dataset, synthetic_qm9_graphs
    from esc_gnn_amd.qm9_models import NestedGIN_eff
    graphs = build_qm9_dataset(synthetic_qm9_graphs(0, args.train_graphs), args.h, target=0)
    store = E.DeviceGraphStore(graphs, "cuda:0")
    torch.manual_seed(0)
    model = NestedGIN_eff(_Features, args.layers).to("cuda:0").train()
    opt = E.optim.FlatAdam(model.parameters(), lr=1e-4)
    gen = torch.Generator().manual_seed(1)

    def batches():
        while True:
            for b in E.DeviceLoader(store, args.bs, shuffle=True, generator=gen):
                if b.num_graphs == args.bs:
                    yield b
    it = batches()

    def step():
        b = next(it)                                         # the device collate is part of the step
        opt.zero_grad()
        E.ops.mse_loss(model(b), b.y).backward()
        opt.step()
    return step, store


def step_time(args):
    step, store = _setup(args)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    for _ in range(args.steps):
        step()
    z.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    print(json.dumps(dict(what="qm9_train_step_per_op_with_device_collate", bs=args.bs, layers=args.layers, h=args.h,
                          graphs=len(store), steps=args.steps, warmup=args.warmup,
                          ms_per_step_events=round(a.elapsed_time(z) / args.steps, 4), ms_per_step_wall=round(wall, 4))),
          flush=True)


def launch_count(args):
    """device kernels per step from torch's profiler (every launch of the stream: HIP library kernels and torch's own)"""
    from torch.profiler import ProfilerActivity, profile
    step, _ = _setup(args)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    n = 10
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            step()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower()]
    copies = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and
              ("memcpy" in e.name.lower() or "memset" in e.name.lower())]
    print(json.dumps(dict(what="qm9_launches_per_step", bs=args.bs, layers=args.layers, steps=n,
                          kernels_per_step=round(len(kernels) / n, 1), copies_per_step=round(len(copies) / n, 1))), flush=True)


def distance_time(args):
    from esc_gnn_amd.datasets import synthetic_qm9_graphs
    from esc_gnn_amd.geometry import edge_distance_arrays, edge_distance_many
    from esc_gnn_amd.utils_edge_efficient import create_subgraphs_many
    done = create_subgraphs_many(synthetic_qm9_graphs(0, args.graphs), args.h, use_rd=True, self_loop=True)
    dev = "cuda:0"
    G = len(done)
    node_ptr, edge_ptr = torch.zeros(G + 1, dtype=torch.int64), torch.zeros(G + 1, dtype=torch.int64)
    node_ptr[1:] = torch.cumsum(torch.tensor([d.pos.size(0) for d in done]), 0)
    edge_ptr[1:] = torch.cumsum(torch.tensor([d.edge_index.size(1) for d in done]), 0)
    pos = torch.cat([d.pos for d in done]).to(dev)
    ei = torch.cat([d.edge_index for d in done], dim=1).to(dev)
    attr = torch.cat([d.edge_attr for d in done]).to(dev)
    src, dst, node_ptr, edge_ptr = ei[0].contiguous(), ei[1].contiguous(), node_ptr.to(dev), edge_ptr.to(dev)
    edge_distance_arrays(pos, src, dst, node_ptr, edge_ptr, attr)        # warm-up
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):                                                   # the call on device arrays: attribute copy, kernel, status
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        edge_distance_arrays(pos, src, dst, node_ptr, edge_ptr, attr)
        z.record()
        torch.cuda.synchronize()
        reps.append(a.elapsed_time(z))
    t0 = time.perf_counter()
    edge_distance_many(done)                                             # host lists in, host tensors out (copies included)
    host_ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(what="qm9_edge_distance_whole_set", graphs=G, edges=int(src.numel()),
                          device_call_ms_median=round(sorted(reps)[2], 4), device_call_ms_all=[round(r, 4) for r in reps],
                          data_list_wall_ms=round(host_ms, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="steps", choices=("steps", "launches", "distance"))
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--h", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--train_graphs", type=int, default=1280, help="graphs resident for the step loop")
    ap.add_argument("--graphs", type=int, default=12000, help="the synthetic set of the distance measurement")
    args = ap.parse_args()
    dict(steps=step_time, launches=launch_count, distance=distance_time)[args.what](args)


if __name__ == "__main__":
    main()
