"""ms per training step of `run_ogb_mol --gnn gine+` (5 layers x 300, k = 3, virtual node, the driver's defaults) on the stand-in
molhiv, measured the way the driver runs it: host collate of the plain batch -> device multi-hop expansion
(MultihopGraphStore.expand) -> per-op forward, masked BCE, backward, FlatAdam.  Also: the device launches of one step, the
expansion's share, the one-launch aggregate (csrc/gineplus.hip) against the per-distance path it replaces — inside the step and
alone — and the `--gnn gin_eff` step (OgbStepEngine) on the same molecules.  The two aggregate forms are alternated in one
process after a warm-up of every shape; every window is bracketed by device events and the spread of the repeats is printed.

    python tools/measure/gineplus_time.py --out profiles/gineplus_measurements.txt
"""
import argparse
import os
import sys

import torch

sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))]      # the repo root
import esc_gnn_amd as E  # noqa: E402
from esc_gnn_amd import multihop, ops  # noqa: E402
from esc_gnn_amd.datasets import build_feature_dataset, synthetic_ogbmol_graphs  # noqa: E402
from esc_gnn_amd.modules.gine_operations import GINEPLUS, ClassifierNetwork  # noqa: E402
from esc_gnn_amd.multihop import MultihopGraphStore, expand_multihop  # noqa: E402

DEV, WARM, ROUNDS, K, LAYERS, HIDDEN, H_EFF = "cuda:0", 5, 5, 3, 5, 300, 4
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
    return "%s  (median %.3f, min %.3f, max %.3f)" % (", ".join("%.3f" % x for x in v), s[len(s) // 2], s[0], s[-1])


def med(v):
    return sorted(v)[len(v) // 2]


def launches(step, n=3):
    """device kernels per step, from torch's profiler (None when it reports no device activity)"""
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


def measure(raw, esc_store, BS, steps):
    G = len(raw)
    ids = [torch.arange(i * BS, (i + 1) * BS) for i in range(G // BS)]
    store = MultihopGraphStore(raw, K, DEV)
    torch.manual_seed(1)
    model = ClassifierNetwork(hidden=HIDDEN, out_dim=1, layers=LAYERS, dropout=0.65, virtual_node=True, k=K, conv_type="gin+").to(DEV).train()
    opt = E.optim.FlatAdam(model.parameters(), lr=2e-4)

    def step(i):
        data = store.expand(store.collate(ids[i % len(ids)]))
        opt.zero_grad()
        loss = ops.bce_with_logits_loss(model(data), data.y.view(-1, 1))
        loss.backward()
        opt.step()

    def step_per_distance(i):
        multihop.FUSED_K_MAX = 0                            # GINEPLUS then takes the per-distance path (masks, k plans per batch)
        try:
            step(i)
        finally:
            multihop.FUSED_K_MAX = 4

    def expand_with_collate(i):
        store.expand(store.collate(ids[i % len(ids)]))

    fixed = store.collate(ids[0])
    sizes0 = store.sizes[ids[0]]

    def expand_only(i):
        expand_multihop(fixed, K, sizes0)

    from esc_gnn_amd.engine import OgbStepEngine
    from esc_gnn_amd.ogb_mol_gnn import GNN
    eff = GNN("ogbg-molhiv", 1, gnn_type="gin_eff", num_layer=LAYERS, emb_dim=HIDDEN, drop_ratio=0.65, virtual_node=True, residual=True,
              use_rd=True).to(DEV).train()
    opt_e = E.optim.FlatAdam(eff.parameters(), lr=2e-4)
    eng = OgbStepEngine(eff)
    eng.refresh()

    def step_eff(i):
        eng.train_step(esc_store.collate(ids[i % len(ids)]))
        opt_e.step()

    b = store.expand(store.collate(ids[0]))
    plan = b.multihop_edge_index._esc_multihop_plan
    say("")
    say("batch_size %d: first batch %d nodes, %d edges -> %d multi-hop pairs at k = %d (per distance 0..k: %s)"
        % (BS, b.x.size(0), b.edge_index.size(1), plan.num_pairs, K, plan.counts))
    # the aggregate alone on this batch: C = 300, k = 3, forward + backward, all gradients
    N, M1 = b.x.size(0), plan.num_d1
    xs = [torch.randn(N, HIDDEN, device=DEV, requires_grad=True) for _ in range(K)]
    e = torch.randn(M1, HIDDEN, device=DEV, requires_grad=True)
    g = torch.randn(N, HIDDEN, device=DEV)
    conv = GINEPLUS(torch.nn.Identity(), HIDDEN, k=K).to(DEV)
    mei_plain, dist_plain = b.multihop_edge_index.clone(), b.distance.clone()        # clones carry no plan: today's path

    def agg_fused(i):
        torch.autograd.grad(ops.gineplus_aggregate(xs, e, conv.eps, plan), xs + [e, conv.eps], g)

    def agg_per_distance(i):
        torch.autograd.grad(conv(list(xs), mei_plain, dist_plain, e)[0], xs + [e, conv.eps], g)

    for fn in (step, step_per_distance, step_eff, expand_with_collate, expand_only, agg_fused, agg_per_distance):
        window(fn, WARM)
    res = {k: [] for k in ("fused", "perd", "eff", "expand", "fill", "agg_f", "agg_p")}
    for _ in range(ROUNDS):
        res["fused"].append(window(step, steps))
        res["perd"].append(window(step_per_distance, steps))
        res["eff"].append(window(step_eff, steps))
        res["expand"].append(window(expand_with_collate, steps))
        res["fill"].append(window(expand_only, steps))
        res["agg_f"].append(window(agg_fused, 100))
        res["agg_p"].append(window(agg_per_distance, 100))
    n_f, n_p, n_af, n_ap = launches(step), launches(step_per_distance), launches(agg_fused), launches(agg_per_distance)
    cnt = lambda v: "n/a" if v is None else "%.0f" % v  # noqa: E731
    say("--gnn gine+  ms/step, one-launch aggregate:   %s" % fmt(res["fused"]))
    say("--gnn gine+  ms/step, per-distance aggregate: %s" % fmt(res["perd"]))
    say("   device launches per step: %s (one-launch aggregate), %s (per-distance aggregate)" % (cnt(n_f), cnt(n_p)))
    say("   host collate + count + fill + grouping by destination, alone: %s" % fmt(res["expand"]))
    say("   count + fill + grouping on a collated batch (no read-back):  %s" % fmt(res["fill"]))
    say("   expansion's share of the step (medians, with the host collate): %.1f %%" % (100.0 * med(res["expand"]) / med(res["fused"])))
    say("aggregate alone, forward + backward [%d x %d, k = %d, %d pairs]:" % (N, HIDDEN, K, plan.num_pairs))
    say("   one launch per direction (%s launches): %s" % (cnt(n_af), fmt(res["agg_f"])))
    say("   per-distance path        (%s launches): %s" % (cnt(n_ap), fmt(res["agg_p"])))
    say("   ratio per-distance / one-launch (medians): %.2f alone, %.3f for the whole step"
        % (med(res["agg_p"]) / med(res["agg_f"]), med(res["perd"]) / med(res["fused"])))
    say("--gnn gin_eff --h %d (OgbStepEngine) ms/step: %s" % (H_EFF, fmt(res["eff"])))
    say("ratio gine+ / gin_eff (medians): %.2f" % (med(res["fused"]) / med(res["eff"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    raw = synthetic_ogbmol_graphs(0, a.graphs, 1, 0.0)
    esc_store = E.DeviceGraphStore(build_feature_dataset(synthetic_ogbmol_graphs(0, a.graphs, 1, 0.0), H_EFF, use_rd=True, self_loop=True), DEV)
    say("run_ogb_mol on %d stand-in ogbg-molhiv molecules, %d layers x %d, drop_ratio 0.65, virtual node; gine+ at k = %d; %d warm-up "
        "calls of every form, then %d alternations of windows (steps: 60 at batch 32, 30 at batch 256; aggregate alone: 100), each "
        "between two device events" % (a.graphs, LAYERS, HIDDEN, K, WARM, ROUNDS))
    measure(raw, esc_store, 32, 60)
    measure(raw, esc_store, 256, 30)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
