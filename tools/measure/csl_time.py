"""CSL (run_csl's defaults: bs 64, 5 layers x 128, h 4): per-step time of the per-op training loop with the device collate
included, the kernel launches per step split into library and torch kernels, and the bare activation kernels
(esc_act_fwd / esc_act_bwd, ELU) against torch.nn.functional.elu and its backward at the two row counts of a batch of 64
CSL graphs (2 624 node rows, 13 120 edge rows) x 128 columns.  One JSON line per measurement.

Times are device events around a window of many calls after a warm-up of the same calls; the two sides of a comparison
alternate inside one process, and every figure is repeated so that the spread is visible.

    python tools/measure/csl_time.py [steps|launches|act|all] [--steps K] [--warmup W] [--repeats R]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT]
DEV = "cuda:0"


def _setup(args):
    import esc_gnn_amd as E
    from esc_gnn_amd.csl_models import NestedGIN
    from esc_gnn_amd.datasets import build_csl_dataset, csl_graphs
    from esc_gnn_amd.run_exp import labels_of
    graphs = build_csl_dataset(csl_graphs(copies=args.copies), args.h)
    store = E.DeviceGraphStore(graphs, DEV)
    torch.manual_seed(0)
    torch.cuda.manual_seed_all(0)
    model = NestedGIN(args.layers, args.width).to(DEV).train()
    opt = E.optim.FlatAdam(model.parameters(), lr=1e-3)
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
        E.ops.log_softmax_nll(model.logits(b), labels_of(b)).backward()
        opt.step()
    b0 = next(it)
    shape = dict(bs=args.bs, layers=args.layers, width=args.width, h=args.h, graphs=len(store), nodes=int(b0.x.size(0)),
                 edges=int(b0.edge_index.size(1)), bag_entries=int(b0.pos_index.numel()))
    return step, shape


def step_time(args):
    step, shape = _setup(args)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        for _ in range(args.steps):
            step()
        z.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / args.steps
        print(json.dumps(dict(what="csl_train_step_per_op_with_device_collate", steps=args.steps, warmup=args.warmup,
                              ms_per_step_events=round(a.elapsed_time(z) / args.steps, 4), ms_per_step_wall=round(wall, 4),
                              **shape)), flush=True)


def launch_count(args):
    """device kernels per step from torch's profiler: names inside the library's `esc` namespace against everything else"""
    from torch.profiler import ProfilerActivity, profile
    step, shape = _setup(args)
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    n = 10
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            step()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = [e for e in dev if "memcpy" in e.name.lower() or "memset" in e.name.lower() or "copybuffer" in e.name.lower()]
    kernels = [e for e in dev if e not in copies]
    lib = [e for e in kernels if "esc::" in e.name]
    act = [e for e in lib if "act_fwd_kernel" in e.name or "act_bwd_kernel" in e.name]
    print(json.dumps(dict(what="csl_launches_per_step", steps=n, kernels_per_step=round(len(kernels) / n, 1),
                          library_per_step=round(len(lib) / n, 1), torch_per_step=round((len(kernels) - len(lib)) / n, 1),
                          activation_per_step=round(len(act) / n, 1), copies_per_step=round(len(copies) / n, 1), **shape)),
          flush=True)


def act_time(args):
    """esc_act_fwd / esc_act_bwd (ELU, contiguous rows) against torch's elu / elu_backward kernels, output buffers
    preallocated on both sides (out= / the C ABI), alternating"""
    import esc_gnn_amd as E
    lib, nv = E._native.lib(), E._native
    calls = args.act_calls
    for M in (2624, 13120):
        C = 128
        g = torch.Generator().manual_seed(M)
        x = torch.randn(M, C, generator=g).to(DEV)
        dy = torch.randn(M, C, generator=g).to(DEV)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        s = nv.stream()
        elu_bwd = torch.ops.aten.elu_backward.grad_input
        sides = {
            "fwd": {"library": lambda: lib.esc_act_fwd(x.data_ptr(), C, M, C, 2, y.data_ptr(), C, s),
                    "torch": lambda: torch.nn.functional.elu(x) if args.act_alloc else torch.ops.aten.elu.out(x, out=y)},
            "bwd": {"library": lambda: lib.esc_act_bwd(y.data_ptr(), C, dy.data_ptr(), C, M, C, 2, dx.data_ptr(), C, s),
                    "torch": lambda: elu_bwd(dy, 1.0, 1.0, 1.0, True, y, grad_input=dx)},
        }
        lib.esc_act_fwd(x.data_ptr(), C, M, C, 2, y.data_ptr(), C, s)
        for direction, pair in sides.items():
            for f in pair.values():
                for _ in range(args.warmup):
                    f()
            torch.cuda.synchronize()
            for _ in range(args.repeats):
                for side, f in pair.items():
                    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(calls):
                        f()
                    z.record()
                    torch.cuda.synchronize()
                    us = a.elapsed_time(z) * 1e3 / calls
                    moved = (2 if direction == "fwd" else 3) * M * C * 4        # bytes the algorithm needs
                    print(json.dumps(dict(what="elu_" + direction, side=side, M=M, C=C, calls=calls,
                                          us_per_call=round(us, 3), gb_per_s=round(moved / us / 1e3, 1))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=("steps", "launches", "act", "all"))
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--layers", type=int, default=5)
    ap.add_argument("--width", type=int, default=128)
    ap.add_argument("--h", type=int, default=4)
    ap.add_argument("--copies", type=int, default=15, help="graphs per class resident for the step loop")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--act_calls", type=int, default=2000, help="calls per timed window of the activation comparison")
    ap.add_argument("--act_alloc", action="store_true", help="torch's forward allocates its output (F.elu) instead of out=")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("csl_time: needs a HIP device (no time is measured without one)")
    for what in (("act", "steps", "launches") if args.what == "all" else (args.what,)):
        dict(steps=step_time, launches=launch_count, act=act_time)[what](args)


if __name__ == "__main__":
    main()
