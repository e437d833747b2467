"""What the PNA local layer costs on the GPU, measured the way tools/measure/gatedgcn_time.py measures GatedGCN:

  1. the fused aggregate, ops.pna_aggregate forward + backward (one launch + two), against the same aggregate written as torch
     ops - index_select, index_add_, scatter_reduce('amax') and a division by the degree - at C = 64 on the ZINC batch of
     DESIGN 6k (32 stand-in molecules with their self-loops) and on gatedgcn_time's molhiv-shaped batch (256 graphs), with the
     device launches of one call from torch's profiler.  (The torch form splits the gradient of a tied maximum evenly where
     the fused one routes it to the lowest edge position; with random operands there is no tie, and the cost is the same.);
  2. the training step of run_zinc_gps and its launches with --gt_layer_type PNA+Transformer against GINE+Transformer - the
     parent's step, whose code path this change leaves untouched - in the same process.

The forms are alternated after a warm-up of each; every window is bracketed by device events; medians over five windows.

    python tools/measure/pna_time.py --out profiles/pna_measurements.txt
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
from gatedgcn_time import molhiv_edges  # noqa: E402  (the molhiv-shaped batch of the GatedGCN measurement)
from gps_time import cnt, fmt, launches, lines, med, say, window  # noqa: E402  (the helpers of the attention's measurement)

DEV, WARM, ROUNDS, C = "cuda:0", 20, 5, 64
CALLS = 1000                    # per window of the aggregate alone: 0.1 - 0.4 s, not a few milliseconds


def torch_aggregate(P, Q, R, src, dst, inv_deg):
    """mean | max | sum as torch ops; a node without in-edges gets 0 (include_self=False leaves the zero it starts from)"""
    m = P.index_select(0, dst) + Q.index_select(0, src) + R
    total = torch.zeros_like(P).index_add_(0, dst, m)
    top = torch.zeros_like(P).scatter_reduce(0, dst.view(-1, 1).expand(-1, P.size(1)), m, "amax", include_self=False)
    return torch.cat([total * inv_deg, top, total], 1)


def aggregate_alone(name, edge_index, N):
    edge_index = edge_index.to(DEV)
    plan = E.BatchPlan.from_tensors(edge_index, N)
    Em = edge_index.size(1)
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = [torch.randn(N, C, device=DEV, generator=gen).requires_grad_(True) for _ in range(2)]
    x.append(torch.randn(Em, C, device=DEV, generator=gen).requires_grad_(True))
    g = torch.randn(N, 3 * C, device=DEV, generator=gen)
    src, dst = edge_index[0], edge_index[1]
    inv_deg = (1.0 / torch.bincount(dst, minlength=N).clamp(min=1).float()).view(-1, 1)
    want, got = torch_aggregate(*x, src, dst, inv_deg), ops.pna_aggregate(*x, plan)
    say("")
    say("the aggregate alone, forward + backward, C = %d, %s: %d nodes, %d edges; the two forms agree to %.2g of the largest value"
        % (C, name, N, Em, float(((want - got).abs().max() / want.abs().max()).detach())))

    def fused(i):
        torch.autograd.backward([ops.pna_aggregate(*x, plan)], [g], inputs=x)

    def composed(i):
        torch.autograd.backward([torch_aggregate(*x, src, dst, inv_deg)], [g], inputs=x)

    forms = (fused, composed)
    for f in forms:
        window(f, WARM)
    res = [[] for _ in forms]
    for _ in range(ROUNDS):
        for r, f in zip(res, forms):
            r.append(window(f, CALLS))
    n = [launches(f) for f in forms]
    say("ms per call, %d calls per window, the two forms alternated (the gradient accumulation into .grad is part of both):" % CALLS)
    say("   ops.pna_aggregate (csrc/pna.hip)                              (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   torch ops: index_select, index_add_, scatter_reduce('amax')   (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    ratio = med(res[1]) / med(res[0])
    say("   ratio torch ops / fused (medians): %.2f%s" % (ratio, "" if ratio >= 1 else "   THE FUSED FORM IS SLOWER AT THIS SHAPE"))


def training_steps(graphs):
    store = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, graphs), 3, use_rd=True, self_loop=True), DEV)
    widest = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    BS = 32
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(graphs // BS)]
    steps = []
    for local in ("GINE", "PNA"):
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
    say("   PNA+Transformer                          (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   PNA costs %+.4f ms per step against GINE (medians)" % (med(res[1]) - med(res[0])))
    return store, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("PNA on stand-in molecules; %d warm-up calls of every form, then %d alternations of windows, each between two device "
        "events" % (WARM, ROUNDS))
    store, ids = training_steps(a.graphs)
    b = store.collate(ids[0])
    aggregate_alone("the ZINC batch of 32 graphs", b.edge_index, b.x.size(0))
    aggregate_alone("a molhiv-shaped batch of 256 graphs", *molhiv_edges())
    say("")
    say("not measured: a kernel trace of the three kernels alone (the figures are event windows with launch overhead), widths other "
        "than 64, and any real-data accuracy")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
