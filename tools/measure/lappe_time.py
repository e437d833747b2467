"""What the Laplacian positional encoding costs on the GPU, measured the way tools/measure/gps_time.py measures the attention:

  1. the PE table of a 10 000-graph training split (stand-in ZINC molecules): ONE esc_laplacian_eig launch over the split's flat
     edge arrays, against the host loop the reference runs at dataset load - numpy.linalg.eigh per graph plus the statistics
     (tests/lappe_oracle.lap_pe restates it);
  2. esc_lappe_encode_fwd + _bwd at the ZINC batch (32 graphs, about 750 nodes, K = 8, dim_pe 8), against the same expression as
     torch ops on the device (cat, isnan mask, Linear, ReLU, Linear, ReLU, masked_fill, sum, and autograd's backward);
  3. the training step of run_zinc_gps and its device launches with the TypeDictNode+LapPE encoder (table attach included),
     against the step without it - the parent configuration, whose code path this change leaves untouched - in the same process.

The forms are alternated after a warm-up of each; every window is bracketed by device events; medians over the windows.

    python tools/measure/lappe_time.py --out profiles/lappe_measurements.txt
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import esc_gnn_amd as E  # noqa: E402
from esc_gnn_amd import ops  # noqa: E402
from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs  # noqa: E402
from esc_gnn_amd.gps_models import GPSModel  # noqa: E402
from esc_gnn_amd.lappe import LapPETable  # noqa: E402
from gps_time import cnt, fmt, launches, lines, med, say, window  # noqa: E402  (the helpers of the attention's measurement)

DEV, WARM, ROUNDS, K, P = "cuda:0", 5, 5, 8, 8


def table_build(graphs):
    import lappe_oracle as lo
    raw = synthetic_zinc_graphs(0, graphs)
    n = torch.tensor([g.x.size(0) for g in raw])
    e = torch.tensor([g.edge_index.size(1) for g in raw])
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)]).to(DEV)
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), e.cumsum(0)]).to(DEV)
    ei = torch.cat([g.edge_index for g in raw], 1).to(torch.int64).to(DEV)
    N, widest = int(n.sum()), int(n.max())

    def build(i):
        ops.laplacian_eig(ei, node_ptr, edge_ptr, K, max_nodes=widest, edges_local=True, num_nodes=N)

    window(build, 2)
    res = [window(build, 3) for _ in range(ROUNDS)]
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for g in raw:
            lo.lap_pe(g.x.size(0), g.edge_index.numpy(), K)
        host.append((time.perf_counter() - t0) * 1e3)
    say("PE table of %d graphs (%d nodes, %d edges, largest graph %d nodes), K = %d:" % (graphs, N, int(e.sum()), widest, K))
    say("   esc_laplacian_eig, one launch, ms: %s" % fmt(res))
    say("   host loop of numpy.linalg.eigh + statistics over the same graphs, ms: %s" % fmt(host))
    say("   ratio host / device (medians): %.0f;  the table holds %d bytes" % (med(host) / med(res), 2 * N * K * 4))


def encoder_alone(vecs, vals):
    N = vecs.size(0)
    torch.manual_seed(2)
    enc = E.nn.LapPENodeEncoder(P, K).to(DEV)
    params = [enc.linear_A.weight, enc.linear_A.bias, enc.pe_encoder[1].weight, enc.pe_encoder[1].bias]
    g = torch.randn(N, P, device=DEV)
    signs = torch.where(torch.rand(K, device=DEV) >= 0.5, 1.0, -1.0)

    def fused_fwd(i):
        with torch.no_grad():
            ops.lappe_encode(vecs, vals, signs, *params)

    def fused_both(i):
        torch.autograd.grad(ops.lappe_encode(vecs, vals, signs, *params), params, g)

    def torch_chain(i):
        pe = torch.cat(((vecs * signs.unsqueeze(0)).unsqueeze(2), vals), dim=2)
        mask = torch.isnan(pe)
        pe = pe.masked_fill(mask, 0.0)
        pe = enc.pe_encoder(enc.linear_A(pe))
        pe = pe.masked_fill(mask[:, :, 0].unsqueeze(2), 0.0)
        torch.autograd.grad(torch.sum(pe, 1), params, g)

    fns = (fused_fwd, fused_both, torch_chain)
    for fn in fns:
        window(fn, WARM)
    res = [[] for _ in fns]
    for _ in range(ROUNDS):
        for r, fn in zip(res, fns):
            r.append(window(fn, 200))
    n = [launches(fn) for fn in fns]
    say("")
    say("LapPE encoder alone at one ZINC batch: %d nodes, K = %d, dim_pe %d; ms per call, 200 calls per window" % (N, K, P))
    say("   esc_lappe_encode_fwd alone                    (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   esc_lappe_encode_fwd + _bwd                   (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   the same expression as torch ops, f + b       (%s launches): %s" % (cnt(n[2]), fmt(res[2])))
    say("   ratio torch / fused, forward + backward (medians): %.2f" % (med(res[2]) / med(res[1])))


def training_steps(graphs):
    store = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, graphs), 3, use_rd=True, self_loop=True), DEV)
    widest = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    table = LapPETable(store, K)
    BS = 32
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(graphs // BS)]
    steps = []
    for lap_pe in (False, True):
        torch.manual_seed(1)
        model = GPSModel(lap_pe=lap_pe, dim_pe=P, max_freqs=K).to(DEV).train()
        opt = E.optim.FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)

        def step(i, model=model, opt=opt, lap_pe=lap_pe):
            data = store.collate(ids[i % len(ids)])
            if lap_pe:
                table.attach(data, ids[i % len(ids)])
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
    say("   TypeDictNode (the parent's step)              (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   TypeDictNode+LapPE, table attach included     (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   LapPE adds %.4f ms per step (medians)" % (med(res[1]) - med(res[0])))
    batch = table.attach(store.collate(ids[0]), ids[0])
    return batch.EigVecs, batch.EigVals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table_graphs", type=int, default=10000)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("LapPE on stand-in ZINC molecules; %d warm-up calls of every form, then %d alternations of windows, each between two device "
        "events" % (WARM, ROUNDS))
    table_build(a.table_graphs)
    vecs, vals = training_steps(a.graphs)
    encoder_alone(vecs, vals)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
