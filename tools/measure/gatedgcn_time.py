"""What the GatedGCN local layer costs on the GPU, measured the way tools/measure/rwse_time.py and gps_time.py measure theirs:

  1. the fused gate, ops.gated_gcn_aggregate forward + backward (one launch + two), against the same expression written as
     torch ops - index_select, sigmoid, index_add_ (tests/gatedgcn_oracle.gate on the device) - at C = 64 on the ZINC batch of
     DESIGN 6k (32 stand-in molecules with their self-loops) and on a molhiv-shaped batch (256 graphs, mean about 25 nodes, the
     largest 222: chains with ring closures, every bond both ways, self-loops), with the device launches of one call from
     torch's profiler;
  2. the training step of run_zinc_gps and its launches with --gt_layer_type CustomGatedGCN+Transformer against
     GINE+Transformer - the parent's step, whose code path this change leaves untouched - in the same process.

The forms are alternated after a warm-up of each; every window is bracketed by device events; medians over five windows.

    python tools/measure/gatedgcn_time.py --out profiles/gatedgcn_measurements.txt
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import esc_gnn_amd as E  # noqa: E402
from esc_gnn_amd import ops  # noqa: E402
from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs  # noqa: E402
from esc_gnn_amd.gps_models import GPSModel  # noqa: E402
from gps_time import cnt, fmt, launches, lines, med, say, window  # noqa: E402  (the helpers of the attention's measurement)

DEV, WARM, ROUNDS, C = "cuda:0", 20, 5, 64
CALLS = 1000                    # per window of the gate alone: 0.1 - 0.4 s, not a few milliseconds


def molhiv_edges():
    gen = torch.Generator().manual_seed(0)
    sizes = torch.randint(10, 46, (255,), generator=gen).tolist() + [222]
    src, dst, base = [], [], 0
    for n in sizes:
        bonds = [(a, a + 1) for a in range(n - 1)]
        for _ in range(max(1, n // 10)):                                  # ring closures
            a = int(torch.randint(0, n - 3, (1,), generator=gen))
            bonds.append((a, min(n - 1, a + int(torch.randint(3, 7, (1,), generator=gen)))))
        for a, b in bonds:
            src += [base + a, base + b]
            dst += [base + b, base + a]
        src += range(base, base + n)
        dst += range(base, base + n)
        base += n
    return torch.tensor([src, dst]), base


def gate_alone(name, edge_index, N):
    import gatedgcn_oracle as gg
    edge_index = edge_index.to(DEV)
    plan = E.BatchPlan.from_tensors(edge_index, N)
    Em = edge_index.size(1)
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = [torch.randn(N, C, device=DEV, generator=gen).requires_grad_(True) for _ in range(4)]
    x.append(torch.randn(Em, C, device=DEV, generator=gen).requires_grad_(True))
    g_out, g_e = torch.randn(N, C, device=DEV, generator=gen), torch.randn(Em, C, device=DEV, generator=gen)
    src, dst = edge_index[0], edge_index[1]

    def fused(i):
        out, e = ops.gated_gcn_aggregate(*x, plan)
        torch.autograd.backward([out, e], [g_out, g_e], inputs=x)

    def composed(i):
        out, e, _ = gg.gate(*x, src, dst)
        torch.autograd.backward([out, e], [g_out, g_e], inputs=x)

    forms = (fused, composed)
    for f in forms:
        window(f, WARM)
    res = [[] for _ in forms]
    for _ in range(ROUNDS):
        for r, f in zip(res, forms):
            r.append(window(f, CALLS))
    n = [launches(f) for f in forms]
    say("")
    say("the gate alone, forward + backward, C = %d, %s: %d nodes, %d edges; ms per call, %d calls per window, the two forms "
        "alternated (the gradient accumulation into .grad is part of both):" % (C, name, N, Em, CALLS))
    say("   ops.gated_gcn_aggregate (csrc/gatedgcn.hip)          (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   torch ops: index_select, sigmoid, index_add_         (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   ratio torch ops / fused (medians): %.2f" % (med(res[1]) / med(res[0])))


def training_steps(graphs):
    store = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, graphs), 3, use_rd=True, self_loop=True), DEV)
    widest = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    BS = 32
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(graphs // BS)]
    steps = []
    for local in ("GINE", "CustomGatedGCN"):
        torch.manual_seed(1)
        model = GPSModel(local_gnn_type=local).to(DEV).train()
        opt = E.optim.FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)

        def step(i, model=model, opt=opt):
            data = store.collate(ids[i % len(ids)])
            data._esc_max_nodes = widest
            opt.zero_grad()
            loss = ops.l1_loss(model(data), data.y.view(-1, 1))
            loss.backward()
            opt.step(grad_denom=opt.clip_scale(1.0))
        steps.append(step)
    for step in steps:
        window(step, WARM)
    res = [[] for _ in steps]
    for _ in range(ROUNDS):
        for r, step in zip(res, steps):
            r.append(window(step, 40))
    n = [launches(step) for step in steps]
    say("")
    say("training step of run_zinc_gps, GPSModel 10 layers x 64, 4 heads, attn_dropout 0.5, batch %d, AdamW + clipping; ms per step, "
        "40 steps per window, the two forms alternated:" % BS)
    say("   GINE+Transformer (the parent's step)     (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   CustomGatedGCN+Transformer               (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   CustomGatedGCN costs %+.4f ms per step against GINE (medians)" % (med(res[1]) - med(res[0])))
    return store, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("GatedGCN on stand-in molecules; %d warm-up calls of every form, then %d alternations of windows, each between two device "
        "events" % (WARM, ROUNDS))
    store, ids = training_steps(a.graphs)
    b = store.collate(ids[0])
    gate_alone("the ZINC batch of 32 graphs", b.edge_index, b.x.size(0))
    gate_alone("a molhiv-shaped batch of 256 graphs", *molhiv_edges())
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
