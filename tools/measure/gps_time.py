"""ms per training step of `run_zinc_gps` at the configuration of the reference's zinc-GPS.yaml (10 layers x 64, 4 heads, batch 32,
attn_dropout 0.5) measured the way the driver runs it — device collate, per-op forward, L1, backward, clipping scale, flat AdamW —
with the device launches of one step; and the attention alone at ZINC's shape and at molhiv's (256 graphs, the largest 222 nodes):
the two kernels (forward; forward + backward), the whole GraphMultiheadAttention layer, and what a user would run without the
kernels on the same GPU — pad (to_dense_batch), torch.nn.MultiheadAttention with key_padding_mask, gather — with the pad's index
and mask built once outside the timed window (in the reference every layer rebuilds them).  The forms are alternated in one process
after a warm-up of every shape; every window is bracketed by device events and the spread of the repeats is printed.

    python tools/measure/gps_time.py --out profiles/gps_measurements.txt
"""
import argparse
import os
import sys

import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]      # the repo root
import esc_gnn_amd as E  # noqa: E402
from esc_gnn_amd import ops  # noqa: E402
from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs  # noqa: E402
from esc_gnn_amd.gps_models import GPSModel  # noqa: E402
from esc_gnn_amd.nn import GraphMultiheadAttention  # noqa: E402

DEV, WARM, ROUNDS, HEADS, HIDDEN, P = "cuda:0", 5, 5, 4, 64, 0.5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def window(step, n):
    """ms per call over n calls, between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(n):
        step(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def fmt(v):
    s = sorted(v)
    return "%s  (median %.4f, min %.4f, max %.4f)" % (", ".join("%.4f" % x for x in v), s[len(s) // 2], s[0], s[-1])


def med(v):
    return sorted(v)[len(v) // 2]


def launches(step, n=3):
    """device kernels per call, from torch's profiler (None when it reports no device activity)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for i in range(n):
                step(i)
            torch.cuda.synchronize()
        cnt = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "mem" not in e.name.lower())
        return cnt / n if cnt else None
    except Exception:                                     # noqa: BLE001 — a measurement aid, not a product path
        return None


def cnt(v):
    return "n/a" if v is None else "%.0f" % v


def train_step(graphs):
    store = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, graphs), 3, use_rd=True, self_loop=True), DEV)
    widest = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    BS = 32
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(graphs // BS)]
    torch.manual_seed(1)
    model = GPSModel().to(DEV).train()
    opt = E.optim.FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)

    def step(i):
        data = store.collate(ids[i % len(ids)])
        data._esc_max_nodes = widest
        opt.zero_grad()
        loss = ops.l1_loss(model(data), data.y.view(-1, 1))
        loss.backward()
        opt.step(grad_denom=opt.clip_scale(1.0))

    window(step, WARM)
    res = [window(step, 40) for _ in range(ROUNDS)]
    b = store.collate(ids[0])
    say("training step, GPSModel 10 layers x %d, %d heads, attn_dropout %g, batch %d (first batch: %d nodes, %d edges, largest graph of "
        "the store %d nodes), AdamW + clipping:" % (HIDDEN, HEADS, P, BS, b.x.size(0), b.edge_index.size(1), widest))
    say("   ms/step: %s" % fmt(res))
    say("   device launches per step: %s" % cnt(launches(step)))
    sizes = (store.h_node_ptr[1:] - store.h_node_ptr[:-1])[ids[0]].tolist()
    return sizes


def attention_alone(tag, sizes):
    N, G, n_max = sum(sizes), len(sizes), max(sizes)
    gp = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    torch.manual_seed(2)
    x = torch.randn(N, HIDDEN, device=DEV, requires_grad=True)
    qkv = torch.randn(N, 3 * HIDDEN, device=DEV, requires_grad=True)
    g = torch.randn(N, HIDDEN, device=DEV)
    mine = GraphMultiheadAttention(HIDDEN, HEADS, dropout=P).to(DEV).train()
    ref = torch.nn.MultiheadAttention(HIDDEN, HEADS, dropout=P, batch_first=True).to(DEV).train()
    ref.load_state_dict(mine.state_dict())
    flat = torch.cat([torch.arange(n) + i * n_max for i, n in enumerate(sizes)]).to(DEV)       # to_dense_batch's index, built once
    valid = torch.zeros(G * n_max, dtype=torch.bool, device=DEV)
    valid[flat] = True
    pad_mask = ~valid.view(G, n_max)

    def kernel_fwd(i):
        with torch.no_grad():
            ops.graph_attention(qkv, gp, HEADS, p=P, training=True, max_nodes=n_max, seed=i + 1)

    def kernel_both(i):
        torch.autograd.grad(ops.graph_attention(qkv, gp, HEADS, p=P, training=True, max_nodes=n_max, seed=i + 1), qkv, g)

    def layer_mine(i):
        torch.autograd.grad(mine(x, gp, n_max), [x] + list(mine.parameters()), g)

    def layer_torch(i):
        dense = x.new_zeros((G * n_max, HIDDEN)).index_copy(0, flat, x).view(G, n_max, HIDDEN)
        out = ref(dense, dense, dense, attn_mask=None, key_padding_mask=pad_mask, need_weights=False)[0].reshape(G * n_max, HIDDEN)[flat]
        torch.autograd.grad(out, [x] + list(ref.parameters()), g)

    fns = (kernel_fwd, kernel_both, layer_mine, layer_torch)
    for fn in fns:
        window(fn, WARM)
    res = [[] for _ in fns]
    for _ in range(ROUNDS):
        for r, fn in zip(res, fns):
            r.append(window(fn, 200))
    n = [launches(fn) for fn in fns]
    pairs = sum(s * s for s in sizes)
    say("")
    say("attention alone, %s: %d graphs, %d nodes, largest %d, %d heads x %d, dropout %g; ms per call, 200 calls per window"
        % (tag, G, N, n_max, HEADS, HIDDEN // HEADS, P))
    say("   memory the ragged form keeps for the backward: mask %d B + lse %d B; the padded form's score tensor alone: %d B"
        % (HEADS * pairs, 4 * HEADS * N, 4 * HEADS * G * n_max * n_max))
    say("   esc_graph_attention_fwd alone                      (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   esc_graph_attention_fwd + _bwd                     (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   GraphMultiheadAttention layer, forward + backward  (%s launches): %s" % (cnt(n[2]), fmt(res[2])))
    say("   pad + torch.nn.MultiheadAttention + gather, f + b  (%s launches): %s" % (cnt(n[3]), fmt(res[3])))
    say("   ratio torch / ragged layer (medians): %.2f" % (med(res[3]) / med(res[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("run_zinc_gps on %d stand-in ZINC molecules; %d warm-up calls of every form, then %d alternations of windows, each between "
        "two device events" % (a.graphs, WARM, ROUNDS))
    zinc_sizes = train_step(a.graphs)
    attention_alone("ZINC's shape (one batch of the driver)", zinc_sizes)
    gen = torch.Generator().manual_seed(3)
    molhiv = torch.randint(10, 46, (255,), generator=gen).tolist() + [222]                        # molhiv: mean about 25 nodes, largest 222
    attention_alone("molhiv's shape (stand-in sizes)", molhiv)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
