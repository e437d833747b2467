"""ms per training step of `run_zinc_gps` at the configuration of the reference's zinc-GPS.yaml (10 layers x 64, 4 heads, batch 32,
attn_dropout 0.5) measured the way the driver runs it — device collate, per-op forward, L1, backward, clipping scale, flat AdamW —
with the device launches of one step; and the attention alone at ZINC's shape and at molhiv's (256 graphs, the largest 222 nodes):
the two kernels (forward; forward + backward), the whole GraphMultiheadAttention layer, and what a user would run without the
kernels on the same GPU — pad (to_dense_batch), torch.nn.MultiheadAttention with key_padding_mask, gather — with the pad's index
and mask built once outside the timed window (in the reference every layer rebuilds them).  The forms are alternated in one process
after a warm-up of every shape; every window is bracketed by device events and the spread of the repeats is printed.

    python tools/measure/gps_time.py --out profiles/gps_measurements.txt

--spd 1 measures the shortest-path attention bias instead: the build of a 10 000-graph distance table in one launch
against the reference's path, the host loop over networkx; the biased attention, forward + backward, against the unbiased ragged
op in the same process and against pad + torch.nn.MultiheadAttention with the dense float attn_mask built the reference's way
(embedding, MLP over [B, n, n, heads], permute, reshape), with the launches of each; and the GINE+BiasedTransformer training step
against GINE+Transformer.  --unbiased_only 1 prints the unbiased op's two figures alone: run it against two checkouts in one job
to compare a commit with its parent.

    python tools/measure/gps_time.py --spd 1 --out profiles/spd_bias_measurements.txt
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


def train_step(graphs, global_model_type="Transformer", store=None):
    if store is None:
        store = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, graphs), 3, use_rd=True, self_loop=True), DEV)
    widest = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    BS = 32
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(graphs // BS)]
    torch.manual_seed(1)
    model = (GPSModel() if global_model_type == "Transformer" else GPSModel(global_model_type=global_model_type)).to(DEV).train()
    opt = E.optim.FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    table = None
    if global_model_type == "BiasedTransformer":
        from esc_gnn_amd.spd import SPDTable
        table = SPDTable(store)

    def step(i):
        data = store.collate(ids[i % len(ids)])
        if table is not None:
            table.attach(data, ids[i % len(ids)])
        data._esc_max_nodes = widest
        opt.zero_grad()
        loss = ops.l1_loss(model(data), data.y.view(-1, 1))
        loss.backward()
        opt.step(grad_denom=opt.clip_scale(1.0))

    window(step, WARM)
    res = [window(step, 40) for _ in range(ROUNDS)]
    b = store.collate(ids[0])
    say("training step, GPSModel GINE+%s 10 layers x %d, %d heads, attn_dropout %g, batch %d (first batch: %d nodes, %d edges, largest "
        "graph of the store %d nodes), AdamW + clipping:" % (global_model_type, HIDDEN, HEADS, P, BS, b.x.size(0), b.edge_index.size(1), widest))
    say("   ms/step: %s" % fmt(res))
    say("   device launches per step: %s" % cnt(launches(step)))
    sizes = (store.h_node_ptr[1:] - store.h_node_ptr[:-1])[ids[0]].tolist()
    return sizes, store


def unbiased_alone(tag, sizes):
    """the unbiased ragged op alone, the figures two checkouts are compared by"""
    N, n_max = sum(sizes), max(sizes)
    gp = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    torch.manual_seed(2)
    qkv = torch.randn(N, 3 * HIDDEN, device=DEV, requires_grad=True)
    g = torch.randn(N, HIDDEN, device=DEV)

    def fwd(i):
        with torch.no_grad():
            ops.graph_attention(qkv, gp, HEADS, p=P, training=True, max_nodes=n_max, seed=i + 1)

    def both(i):
        torch.autograd.grad(ops.graph_attention(qkv, gp, HEADS, p=P, training=True, max_nodes=n_max, seed=i + 1), qkv, g)

    for fn in (fwd, both):
        window(fn, WARM)
    res = [[], []]
    for _ in range(ROUNDS):
        for r, fn in zip(res, (fwd, both)):
            r.append(window(fn, 200))
    say("unbiased ragged attention, %s (%d graphs, %d nodes, largest %d); ms per call, 200 calls per window" % (tag, len(sizes), N, n_max))
    say("   esc_graph_attention_fwd alone   : %s" % fmt(res[0]))
    say("   esc_graph_attention_fwd + _bwd  : %s" % fmt(res[1]))


def spd_table_build(graphs):
    """a split's distance table in one launch against the reference's host loop (networkx per graph, utils_escgnn.py:29-38)"""
    import time
    data = synthetic_zinc_graphs(0, graphs)
    n = torch.tensor([int(d.num_nodes) for d in data], dtype=torch.int64)
    m = torch.tensor([d.edge_index.size(1) for d in data], dtype=torch.int64)
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)])
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), m.cumsum(0)])
    pair_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), (n * n).cumsum(0)])
    ei = torch.cat([d.edge_index for d in data], 1).to(DEV)
    node_ptr_d, edge_ptr_d, pair_ptr_d = node_ptr.to(DEV), edge_ptr.to(DEV), pair_ptr.to(DEV)
    kw = dict(max_nodes=int(n.max()), edges_local=True, num_nodes=int(node_ptr[-1]), num_pairs=int(pair_ptr[-1]), pair_ptr=pair_ptr_d)

    def build(i):
        ops.graph_spd(ei, node_ptr_d, edge_ptr_d, **kw)

    window(build, WARM)
    res = [window(build, 20) for _ in range(ROUNDS)]
    say("")
    say("distance table of %d stand-in ZINC molecules (%d nodes, %d listed edges, largest graph %d nodes, %d bytes), esc_graph_spd in ONE "
        "launch; ms per build, 20 builds per window:" % (graphs, int(node_ptr[-1]), int(edge_ptr[-1]), int(n.max()), int(pair_ptr[-1])))
    say("   %s" % fmt(res))
    try:
        import networkx as nx
    except ImportError:
        say("   networkx is not installed: no host comparison")
        return
    part = data[:1000]                                    # the host loop is timed on the first 1000 graphs and scaled
    t0 = time.time()
    for d in part:
        G = nx.Graph()
        G.add_nodes_from(range(int(d.num_nodes)))
        G.add_edges_from(d.edge_index.t().tolist())
        SPT = dict(nx.all_pairs_shortest_path_length(G))
        k = int(d.num_nodes)
        bias = torch.zeros(k, k, dtype=torch.long)
        for i in range(k):
            for j in range(k):
                bias[i][j] = SPT[i][j] if j in SPT[i] else 100
    host = (time.time() - t0) * graphs / len(part)
    say("   the reference's host loop (networkx all_pairs_shortest_path_length and its fill loop, one CPU core; timed on the first %d "
        "graphs, scaled to %d): %.1f s, %.0f x the median build" % (len(part), graphs, host, host * 1e3 / med(res)))


def biased_attention(tag, sizes):
    N, G, n_max = sum(sizes), len(sizes), max(sizes)
    gp = torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
    torch.manual_seed(2)
    x = torch.randn(N, HIDDEN, device=DEV, requires_grad=True)
    qkv = torch.randn(N, 3 * HIDDEN, device=DEV, requires_grad=True)
    g = torch.randn(N, HIDDEN, device=DEV)
    gen = torch.Generator().manual_seed(4)
    spds = [torch.randint(0, 12, (n, n), generator=gen, dtype=torch.uint8) for n in sizes]            # stand-in distances: any bytes cost the same
    spd = torch.cat([s.reshape(-1) for s in spds]).to(DEV)
    emb = torch.nn.Embedding(101, HEADS, padding_idx=100).to(DEV)
    mlp = torch.nn.Sequential(torch.nn.Linear(HEADS, HEADS), torch.nn.ReLU(), torch.nn.Linear(HEADS, HEADS), torch.nn.ReLU(),
                              torch.nn.Linear(HEADS, HEADS)).to(DEV)
    bias_params = list(emb.parameters()) + list(mlp.parameters())
    index = torch.arange(101, device=DEV)
    ref = torch.nn.MultiheadAttention(HIDDEN, HEADS, dropout=P, batch_first=True).to(DEV).train()
    flat = torch.cat([torch.arange(n) + i * n_max for i, n in enumerate(sizes)]).to(DEV)
    valid = torch.zeros(G * n_max, dtype=torch.bool, device=DEV)
    valid[flat] = True
    pad_mask = ~valid.view(G, n_max)
    dense_bias = torch.full((G, n_max, n_max), 100, dtype=torch.long)                                # the padded attn_bias the reference's collate
    for i, s in enumerate(spds):                                                                     # would hand over, built once outside
        dense_bias[i, :s.size(0), :s.size(0)] = s.long()
    dense_bias = dense_bias.to(DEV)
    key_pad = torch.zeros((G, n_max), device=DEV).masked_fill(pad_mask, float("-inf"))               # float, like the attn_mask

    def biased_both(i):
        table = mlp(emb(index))
        out = ops.graph_attention(qkv, gp, HEADS, p=P, training=True, max_nodes=n_max, seed=i + 1, spd=spd, bias_table=table)
        torch.autograd.grad(out, [qkv] + bias_params, g)

    def biased_kernels(i):
        out = ops.graph_attention(qkv, gp, HEADS, p=P, training=True, max_nodes=n_max, seed=i + 1, spd=spd, bias_table=tab)
        torch.autograd.grad(out, [qkv, tab], g)

    def unbiased_both(i):
        torch.autograd.grad(ops.graph_attention(qkv, gp, HEADS, p=P, training=True, max_nodes=n_max, seed=i + 1), qkv, g)

    def layer_torch(i):
        dense = x.new_zeros((G * n_max, HIDDEN)).index_copy(0, flat, x).view(G, n_max, HIDDEN)
        attn_mask = mlp(emb(dense_bias)).permute(0, 3, 1, 2).reshape(-1, n_max, n_max)               # gps_layer.py:273-278
        out = ref(dense, dense, dense, attn_mask=attn_mask, key_padding_mask=key_pad, need_weights=False)[0].reshape(G * n_max, HIDDEN)[flat]
        torch.autograd.grad(out, [x] + list(ref.parameters()) + bias_params, g)

    tab = torch.randn(101, HEADS, device=DEV, requires_grad=True)
    fns = (biased_kernels, biased_both, unbiased_both, layer_torch)
    for fn in fns:
        window(fn, WARM)
    res = [[] for _ in fns]
    for _ in range(ROUNDS):
        for r, fn in zip(res, fns):
            r.append(window(fn, 100))
    n = [launches(fn) for fn in fns]
    say("")
    say("biased attention, %s: %d graphs, %d nodes, largest %d, %d heads x %d, dropout %g; forward + backward, ms per call, 100 calls per "
        "window" % (tag, G, N, n_max, HEADS, HIDDEN // HEADS, P))
    say("   memory of the bias: ragged %d B of distances + a %d B table; the padded form's float attn_mask alone: %d B (and its MLP "
        "activations over [B, n, n, heads] as many again per Linear)" % (spd.numel(), 4 * 101 * HEADS, 4 * HEADS * G * n_max * n_max))
    say("   esc_graph_attention_bias_fwd + _bwd, table given           (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   ... with the table's 101 x heads MLP and its backward       (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   esc_graph_attention_fwd + _bwd (unbiased)                  (%s launches): %s" % (cnt(n[2]), fmt(res[2])))
    say("   pad + dense attn_mask + torch.nn.MultiheadAttention, f + b (%s launches): %s" % (cnt(n[3]), fmt(res[3])))
    say("   biased / unbiased kernels (medians): %.2f;  torch dense / biased with its MLP (medians): %.2f"
        % (med(res[0]) / med(res[2]), med(res[3]) / med(res[1])))


def spd_measurements(a):
    say("shortest-path attention bias; %d warm-up calls of every form, then %d alternations of windows, each between two device events"
        % (WARM, ROUNDS))
    spd_table_build(10000)
    say("")
    zinc_sizes, store = train_step(a.graphs)
    say("")
    train_step(a.graphs, "BiasedTransformer", store)
    biased_attention("ZINC's shape (one batch of the driver)", zinc_sizes)
    gen = torch.Generator().manual_seed(3)
    molhiv = torch.randint(10, 46, (255,), generator=gen).tolist() + [222]
    biased_attention("molhiv's shape (stand-in sizes)", molhiv)


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
    ap.add_argument("--spd", type=int, default=0, help="1: the shortest-path bias's measurements instead")
    ap.add_argument("--unbiased_only", type=int, default=0, help="1: the unbiased ragged op's figures alone (to compare two checkouts)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    if a.spd or a.unbiased_only:
        if a.spd:
            spd_measurements(a)
        else:
            gen = torch.Generator().manual_seed(3)
            unbiased_alone("ZINC-like sizes", torch.randint(12, 38, (32,), generator=gen).tolist())
            unbiased_alone("molhiv-like sizes", torch.randint(10, 46, (255,), generator=gen).tolist() + [222])
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    say("run_zinc_gps on %d stand-in ZINC molecules; %d warm-up calls of every form, then %d alternations of windows, each between "
        "two device events" % (a.graphs, WARM, ROUNDS))
    zinc_sizes, _ = train_step(a.graphs)
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
