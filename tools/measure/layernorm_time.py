"""What the per-graph LayerNorm costs on the GPU, measured the way tools/measure/pna_time.py measures the PNA aggregate:

  1. ops.graph_layer_norm forward + backward (one launch + two) against PyG's norm.LayerNorm.forward(x, batch) written as the
     torch ops it is - a degree count, two index_add scatters, two gathers and the elementwise ops between them - on the ZINC
     batch of DESIGN 6k (32 stand-in molecules, C = 64) and on gatedgcn_time's molhiv-shaped batch (256 graphs, the largest
     222 nodes) at C = 64 and C = 300, with the device launches of one call from torch's profiler;
  2. the residual add folded into the launch against a torch add in front of it;
  3. the training step of run_zinc_gps and its launches, GINE+Transformer, with gt.layer_norm against gt.batch_norm - the
     parent's step, whose code path this change leaves untouched - in the same process.

The forms are alternated after a warm-up of each; every window is bracketed by device events; medians over five windows.

    python tools/measure/layernorm_time.py --out profiles/layernorm_measurements.txt
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

DEV, WARM, ROUNDS = "cuda:0", 20, 5
CALLS = 200                     # per window of the op alone
EPS = 1e-5


def pyg_layer_norm(x, batch, weight, bias, batch_size):
    """torch_geometric.nn.norm.LayerNorm.forward(x, batch), statement by statement (tests/layernorm_oracle.py, on the device)"""
    norm = torch.zeros(batch_size, dtype=x.dtype, device=x.device).index_add_(0, batch, torch.ones_like(batch, dtype=x.dtype)).clamp_(min=1)
    norm = norm.mul_(x.size(-1)).view(-1, 1)
    mean = torch.zeros((batch_size, x.size(1)), dtype=x.dtype, device=x.device).index_add(0, batch, x).sum(dim=-1, keepdim=True) / norm
    x = x - mean.index_select(0, batch)
    var = torch.zeros((batch_size, x.size(1)), dtype=x.dtype, device=x.device).index_add(0, batch, x * x).sum(dim=-1, keepdim=True)
    var = var / norm
    return x / (var + EPS).sqrt().index_select(0, batch) * weight + bias


def alternate(forms, calls):
    for f in forms:
        window(f, WARM)
    res = [[] for _ in forms]
    for _ in range(ROUNDS):
        for r, f in zip(res, forms):
            r.append(window(f, calls))
    return res, [launches(f) for f in forms]


def op_alone(name, sizes, C):
    sizes = torch.as_tensor(sizes, dtype=torch.int64)
    G, N = sizes.numel(), int(sizes.sum())
    graph_ptr = torch.zeros(G + 1, dtype=torch.int32)
    graph_ptr[1:] = torch.cumsum(sizes, 0)
    graph_ptr = graph_ptr.to(DEV)
    batch = torch.repeat_interleave(torch.arange(G), sizes).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    x, r = (torch.randn(N, C, device=DEV, generator=gen).requires_grad_(True) for _ in range(2))
    w = (torch.rand(C, device=DEV, generator=gen) + 0.5).requires_grad_(True)
    b = torch.randn(C, device=DEV, generator=gen).requires_grad_(True)
    g = torch.randn(N, C, device=DEV, generator=gen)
    want, got = pyg_layer_norm(x, batch, w, b, G), ops.graph_layer_norm(x, graph_ptr, w, b, EPS)
    say("")
    say("the op alone, forward + backward, C = %d, %s: %d graphs, %d nodes, the largest %d; the two forms agree to %.2g of the largest "
        "value" % (C, name, G, N, int(sizes.max()), float(((want - got).abs().max() / want.abs().max()).detach())))

    def fused(i):
        torch.autograd.backward([ops.graph_layer_norm(x, graph_ptr, w, b, EPS)], [g], inputs=[x, w, b])

    def composed(i):
        torch.autograd.backward([pyg_layer_norm(x, batch, w, b, G)], [g], inputs=[x, w, b])

    def folded(i):
        torch.autograd.backward([ops.graph_layer_norm(x, graph_ptr, w, b, EPS, residual=r)], [g], inputs=[x, r, w, b])

    def added(i):
        torch.autograd.backward([ops.graph_layer_norm(x + r, graph_ptr, w, b, EPS)], [g], inputs=[x, r, w, b])

    res, n = alternate((fused, composed), CALLS)
    say("ms per call, %d calls per window, the two forms alternated (the gradient accumulation into .grad is part of both):" % CALLS)
    say("   ops.graph_layer_norm (csrc/layernorm.hip)                     (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   torch ops: PyG's LayerNorm.forward(x, batch) spelled out      (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    ratio = med(res[1]) / med(res[0])
    say("   ratio torch ops / fused (medians): %.2f%s" % (ratio, "" if ratio >= 1 else "   THE FUSED FORM IS SLOWER AT THIS SHAPE"))
    res, n = alternate((folded, added), CALLS)
    say("with a residual in front of the norm, gradients for both:")
    say("   the add folded into the launch                                (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   a torch add, then the op                                      (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   the separate add costs %+.4f ms per call (medians)" % (med(res[1]) - med(res[0])))


def training_steps(graphs):
    store = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, graphs), 3, use_rd=True, self_loop=True), DEV)
    widest = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    BS = 32
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(graphs // BS)]
    steps = []
    for kw in (dict(), dict(layer_norm=True, batch_norm=False), dict(layer_norm=False, batch_norm=False)):
        torch.manual_seed(1)
        model = GPSModel(**kw).to(DEV).train()
        opt = E.optim.FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)

        def step(i, model=model, opt=opt):
            data = store.collate(ids[i % len(ids)])
            data._esc_max_nodes = widest
            opt.zero_grad()
            loss = ops.l1_loss(model(data), data.y.view(-1, 1))
            loss.backward()
            opt.step(grad_denom=opt.clip_scale(1.0))
        steps.append(step)
    res, n = alternate(steps, 40)
    say("")
    say("training step of run_zinc_gps, GPSModel 10 layers x 64, 4 heads, GINE+Transformer, attn_dropout 0.5, batch %d, AdamW + clipping; "
        "ms per step, 40 steps per window, the three forms alternated:" % BS)
    say("   batch_norm (the default: the parent's step)  (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   layer_norm                                   (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   neither                                      (%s launches): %s" % (cnt(n[2]), fmt(res[2])))
    say("   layer_norm costs %+.4f ms per step against batch_norm (medians)" % (med(res[1]) - med(res[0])))
    return store, ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("the per-graph LayerNorm on stand-in molecules; %d warm-up calls of every form, then %d alternations of windows, each between "
        "two device events" % (WARM, ROUNDS))
    store, ids = training_steps(a.graphs)
    per_graph = store.h_node_ptr[1:] - store.h_node_ptr[:-1]
    sizes = [int(per_graph[int(i)]) for i in ids[0]]
    op_alone("the ZINC batch of 32 graphs", sizes, 64)
    gen = torch.Generator().manual_seed(0)
    molhiv = torch.randint(10, 46, (255,), generator=gen).tolist() + [222]        # the graph sizes of gatedgcn_time.molhiv_edges
    assert sum(molhiv) == molhiv_edges()[1]
    for C in (64, 300):
        op_alone("a molhiv-shaped batch of 256 graphs", molhiv, C)
    say("")
    say("not measured: a kernel trace of the three kernels alone (the figures are event windows with launch overhead), and any "
        "real-data accuracy")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
