"""What the random-walk structural encoding costs on the GPU, measured the way tools/measure/lappe_time.py measures LapPE:

  1. the RWSE table of a 10 000-graph training split (stand-in ZINC molecules with the appended self-loops the run's stores
     carry, 20 steps): ONE esc_rw_landing launch over the split's flat edge arrays, against the host loop the reference runs at
     dataset load - get_rw_landing_probs per graph, dense n x n products in fp32 torch (tests/rwse_oracle.rw_landing_ref32
     restates it);
  2. the training step of run_zinc_gps and its device launches with the TypeDictNode+RWSE encoder (table attach included),
     against the step without it - the parent configuration, whose code path this change leaves untouched - in the same process.

The forms are alternated after a warm-up of each; every window is bracketed by device events; medians over the windows.

    python tools/measure/rwse_time.py --out profiles/rwse_measurements.txt
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
from esc_gnn_amd.rwse import RWSETable  # noqa: E402
from gps_time import cnt, fmt, launches, lines, med, say, window  # noqa: E402  (the helpers of the attention's measurement)

DEV, WARM, ROUNDS = "cuda:0", 5, 5
KSTEPS = list(range(1, 21))


def table_build(graphs):
    import rwse_oracle as ro
    raw = synthetic_zinc_graphs(0, graphs)
    edges = [ro.with_self_loops(g.x.size(0), g.edge_index.numpy()) for g in raw]      # what create_subgraphs(self_loop=True) stores
    n = torch.tensor([g.x.size(0) for g in raw])
    e = torch.tensor([a.shape[1] for a in edges])
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), n.cumsum(0)]).to(DEV)
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), e.cumsum(0)]).to(DEV)
    ei = torch.cat([torch.from_numpy(a) for a in edges], 1).to(DEV)
    N, widest, most = int(n.sum()), int(n.max()), int(e.max())

    def build(i):
        ops.rw_landing(ei, node_ptr, edge_ptr, KSTEPS, max_nodes=widest, max_edges=most, edges_local=True, num_nodes=N)

    window(build, 2)
    res = [window(build, 3) for _ in range(ROUNDS)]
    host = []
    for _ in range(2):
        t0 = time.perf_counter()
        for g, a in zip(raw, edges):
            ro.rw_landing_ref32(g.x.size(0), a, KSTEPS)
        host.append((time.perf_counter() - t0) * 1e3)
    say("RWSE table of %d graphs (%d nodes, %d edges with the self-loops, largest graph %d nodes / %d edges), %d steps:"
        % (graphs, N, int(e.sum()), widest, most, len(KSTEPS)))
    say("   esc_rw_landing, one launch, ms: %s" % fmt(res))
    say("   host loop of the reference's dense matrix powers (fp32 torch) over the same graphs, ms: %s" % fmt(host))
    say("   ratio host / device (medians): %.0f;  the table holds %d bytes" % (med(host) / med(res), N * len(KSTEPS) * 4))


def training_steps(graphs):
    store = E.DeviceGraphStore(build_feature_dataset(synthetic_zinc_graphs(0, graphs), 3, use_rd=True, self_loop=True), DEV)
    widest = int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    table = RWSETable(store, KSTEPS)
    BS = 32
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(graphs // BS)]
    steps = []
    for rwse in (False, True):
        torch.manual_seed(1)
        model = GPSModel(rwse=rwse).to(DEV).train()
        opt = E.optim.FlatAdam(model.parameters(), lr=1e-3, weight_decay=1e-5)

        def step(i, model=model, opt=opt, rwse=rwse):
            data = store.collate(ids[i % len(ids)])
            if rwse:
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
    say("   TypeDictNode (the parent's step)                          (%s launches): %s" % (cnt(n[0]), fmt(res[0])))
    say("   TypeDictNode+RWSE (20 steps, dim_pe 28, linear, BatchNorm), attach included (%s launches): %s" % (cnt(n[1]), fmt(res[1])))
    say("   RWSE adds %.4f ms per step (medians)" % (med(res[1]) - med(res[0])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table_graphs", type=int, default=10000)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("RWSE on stand-in ZINC molecules; %d warm-up calls of every form, then %d alternations of windows, each between two device "
        "events" % (WARM, ROUNDS))
    table_build(a.table_graphs)
    training_steps(a.graphs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
