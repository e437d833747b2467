"""OGB molecule driver on the ESC hot path — the MI355X-native twin of /root/reference/run_ogb_mol.py for
`--gnn gin_eff --edge_nest True --efficient True` (BASELINE config 5): flags (:196-281), feature settings
(:321-331), criterion with NaN-label masking (:65-72), evaluation (:77-149), repeated runs, best-model /
periodic model+optimizer checkpoints, `--continue_from`, checkpoint ensembling and the final mean ± std summary
(:394-562).

`PygGraphPropPredDataset` downloads by name and needs ogb + rdkit (absent, no network), so the data are seeded
molecule-shaped graphs with the ogbg-mol feature layout (datasets.synthetic_ogbmol_graphs; ogbg-molpcba gets 128
tasks with NaN labels) and `metrics.Evaluator` stands in for ogb's.  Dataset resident in HBM; forward, loss,
backward and Adam through libescgnn_hip.so; graph-sharded under torchrun.

`--gnn gine+` (reference :419-427, modules/gine_operations.py) trains the multi-hop GINE+ baseline on the same molecules, loop,
evaluator and checkpoints: the splits hold the raw graphs (no feature build), and every batch gets its multi-hop edges on the
device (multihop.MultihopGraphStore, csrc/multihop.hip) before the per-op forward / masked BCE / backward / Adam.

    python -m esc_gnn_amd.run_ogb_mol --h 4 --gnn gin_eff --edge_nest True --efficient True --self_loop True
    python -m esc_gnn_amd.run_ogb_mol --gnn gine+
"""
import numpy as np
import torch

from . import ops
from .harness import Context, default_appendix, expanded_batches, open_result_dir, parser_from, prefetched, sharded_batches
from .ogb_mol_gnn import GNN

_FLAGS = [  # same names, types and defaults as the reference CLI (its `type=bool` flags included: any non-empty
    # string is True, run_ogb_mol.py:238-245)
    ("--dataset", dict(type=str, default="ogbg-molhiv")),
    ("--runs", dict(type=int, default=10)),
    ("--gnn", dict(type=str, default="gin", help="gin_eff is the ESC path; gin / gcn / ppgn / gine+ are baselines")),
    ("--virtual_node", dict(type=bool, default=True)),
    ("--residual", dict(action="store_true", default=True)),
    ("--RNI", dict(action="store_true", default=False)),
    ("--adj_dropout", dict(type=float, default=0)),
    ("--drop_ratio", dict(type=float, default=0.65)),
    ("--num_layer", dict(type=int, default=5)),
    ("--emb_dim", dict(type=int, default=300)),
    ("--h", dict(type=int, default=None)),
    ("--subgraph_pooling", dict(type=str, default="mean")),
    ("--graph_pooling", dict(type=str, default="mean")),
    ("--node_label", dict(type=str, default="spd")),
    ("--use_rd", dict(action="store_true", default=True)),
    ("--use_rp", dict(type=int, default=None)),
    ("--use_id", dict(type=str, default=None)),
    ("--edge_nest", dict(type=bool, default=False)),
    ("--self_loop", dict(type=bool, default=False)),
    ("--use_deg", dict(type=bool, default=False)),
    ("--efficient", dict(type=bool, default=False)),
    ("--batch_size", dict(type=int, default=32)),
    ("--epochs", dict(type=int, default=100)),
    ("--lr", dict(type=float, default=2e-4)),
    ("--lr_decay_factor", dict(type=float, default=0.5)),
    ("--num_workers", dict(type=int, default=2)),
    ("--ensemble", dict(action="store_true", default=False)),
    ("--ensemble_lookback", dict(type=int, default=70)),
    ("--ensemble_interval", dict(type=int, default=10)),
    ("--scheduler", dict(action="store_true", default=False)),
    ("--save_appendix", dict(type=str, default="_h4_l6_spd_rd_gin_edge_eff")),
    ("--log_steps", dict(type=int, default=10)),
    ("--continue_from", dict(type=int, default=None)),
    ("--run_from", dict(type=int, default=1)),
    ("--visualize_all", dict(action="store_true", default=False)),
    ("--visualize_test", dict(action="store_true", default=False)),
    ("--pre_visualize", dict(action="store_true", default=False)),
    # additions (not in the reference): size of the synthetic stand-in dataset
    ("--synthetic_graphs", dict(type=int, default=4000, help="molecules; split 80/10/10 by index")),
    ("--prefetch", dict(action="store_true", default=False,
                        help="collate the next batch on a side stream (harness.prefetched): 4.21 vs 4.31 ms/step on MI355X at "
                             "config 5 (bs=256, emb 300), see DESIGN.md 4")),
]

TASKS = {"ogbg-molhiv": (1, 0.0), "ogbg-molpcba": (128, 0.6)}     # (num_tasks, NaN-label ratio of the stand-in)


def build_parser():
    return parser_from(_FLAGS, "ESC-GNN for OGB molecular graphs (MI355X hot path).")


class StepLR(object):
    """torch.optim.lr_scheduler.StepLR(optimizer, step_size, gamma) (reference :415-417) over `param_groups`."""

    def __init__(self, optimizer, step_size, gamma):
        self.optimizer, self.step_size, self.gamma, self.epoch = optimizer, step_size, gamma, 0
        self.base = [g["lr"] for g in optimizer.param_groups]

    def step(self):
        self.epoch += 1
        for g, b in zip(self.optimizer.param_groups, self.base):
            g["lr"] = b * self.gamma ** (self.epoch // self.step_size)


def main(argv=None):
    import os
    import sys
    import time

    from .datasets import build_feature_dataset, synthetic_ogbmol_graphs
    from .metrics import Evaluator
    from .optim import FlatAdam
    from .parallel import broadcast_buffers, broadcast_parameters
    from .store import DeviceGraphStore

    args = build_parser().parse_args(argv)
    gineplus = args.gnn == "gine+"
    if gineplus and args.h is not None:
        raise NotImplementedError("`--gnn gine+` with --h (GINE+ on rooted subgraphs, h=%d) is out of scope: leave --h unset" % args.h)
    if not gineplus and (args.gnn != "gin_eff" or not (args.edge_nest and args.efficient) or args.h is None):
        raise NotImplementedError("only `--gnn gin_eff --edge_nest True --efficient True --h H` is the ESC hot path; "
                                  "the other --gnn types are the reference's baselines")
    if args.use_rp is not None or args.use_deg or args.use_id is not None or args.RNI:
        raise NotImplementedError("use_rp / use_deg / use_id / RNI are outside the ESC hot path")
    if args.visualize_all or args.visualize_test or args.pre_visualize:
        raise NotImplementedError("visualisation is outside the ESC hot path")
    ctx = Context()
    args.save_appendix = default_appendix(args.save_appendix)
    args.res_dir = "results/{}{}".format(args.dataset, args.save_appendix)
    cmd_input = open_result_dir(ctx, args.res_dir, ("run_ogb_mol.py", "ogb_mol_gnn.py", "utils_edge_efficient.py"))
    log_file = os.path.join(args.res_dir, "log.txt")

    def log(text):
        if ctx.rank == 0:
            with open(log_file, "a") as fh:
                print(text, file=fh)
    log("\n" + cmd_input)

    num_tasks, nan_ratio = TASKS.get(args.dataset, (1, 0.0))
    t1 = time.time()
    raw = synthetic_ogbmol_graphs(0, args.synthetic_graphs, num_tasks, nan_ratio)
    GINEPLUS_K = 3                                          # reference :421
    if gineplus:                                            # raw molecules: the multi-hop edges are built per batch on the device
        done = raw
    else:
        done = build_feature_dataset(raw, args.h, use_rd=args.use_rd, self_loop=args.self_loop)     # reference :321-326
    t2 = time.time()
    G = len(done)
    n_tr, n_va = (G * 8) // 10, G // 10
    parts = (done[:n_tr], done[n_tr:n_tr + n_va], done[n_tr + n_va:])
    if gineplus:                                            # per-graph pair counts: one count pass per split, no read-back per step
        from .multihop import MultihopGraphStore
        stores = [MultihopGraphStore(p, GINEPLUS_K, ctx.device) for p in parts]
    else:
        stores = [DeviceGraphStore(p, ctx.device) for p in parts]
    evaluator = Evaluator(args.dataset)
    eval_metric = evaluator.eval_metric
    kwargs = dict(num_layer=args.num_layer, residual=args.residual, use_rd=args.use_rd, use_rp=args.use_rp,
                  adj_dropout=args.adj_dropout, subgraph_pooling=args.subgraph_pooling, graph_pooling=args.graph_pooling)

    def train(model, optimizer, gen):
        from .engine import OgbStepEngine, ogb_engine_ready, ogb_engine_supports
        model.train()
        engine = model.__dict__.get("_esc_step_engine")
        if engine is None and not gineplus and ogb_engine_supports(model):      # (gine+ has no whole-step engine: per-op branch)
            engine = model.__dict__["_esc_step_engine"] = OgbStepEngine(model)    # forward + masked BCE + backward in ONE call
        if engine is not None:
            engine.refresh()                                # (the optimiser owns the gradient buffers: re-read the addresses)
        total = torch.zeros((), device=ctx.device)
        warm = (lambda item: engine.prepare(item[0]) if ogb_engine_ready(model, item[0]) else None) if engine is not None else None
        batches = sharded_batches(stores[0], args.batch_size, ctx, True, gen)
        if args.prefetch:         # the next batch is collated (and its embedding plans built) on a side stream while this one trains
            batches = prefetched(batches, ctx.device, warm)
        if gineplus:              # every plain batch gets multihop_edge_index / distance and the aggregate's plan, on the device
            batches = expanded_batches(stores[0], batches)
        for data, _ in batches:
            y = data.y.view(-1, num_tasks)
            if engine is not None and ogb_engine_ready(model, data):
                if ctx.world > 1:                           # sum-form gradients, ONE all-reduce of grad ++ [labeled targets]
                    n_lab = int((y == y).sum())
                    loss_sum = engine.train_step(data, loss_denom=1)
                    denom = optimizer.all_reduce_sum(n_lab)
                    optimizer.step(grad_denom=denom)
                    total += loss_sum / max(n_lab, 1) * y.shape[0]
                else:
                    total += engine.train_step(data) * y.shape[0]
                    optimizer.step()
                continue
            optimizer.zero_grad()
            pred = model(data)
            loss = ops.bce_with_logits_loss(pred, y)      # NaN (unlabelled) targets ignored, reference :65-70
            loss.backward()
            n_lab = int((y == y).sum())
            if ctx.world > 1:
                optimizer.all_reduce_weighted(n_lab)
            optimizer.step()
            total += loss.detach() * y.shape[0]
        return float(ctx.all_reduce(total)) / len(parts[0])

    @torch.no_grad()
    def evaluate(model, store, checkpoints=(None,)):
        broadcast_buffers(model, 0)                        # rank-local BatchNorm running statistics -> rank 0's everywhere
        model.eval()
        preds = []
        for ckpt in checkpoints:                           # checkpoint ensembling: mean of the predictions (:84-138)
            if ckpt:
                model.load_state_dict(torch.load(ckpt, map_location=ctx.device))
            y_true, y_pred = [], []
            batches = sharded_batches(store, args.batch_size, ctx, False)
            for data, _ in (expanded_batches(store, batches) if gineplus else batches):
                pred = model(data)
                y_true.append(data.y.view(pred.shape))
                y_pred.append(pred)
            y_true, y_pred = torch.cat(y_true), torch.cat(y_pred)
            if ctx.world > 1:                              # shards are contiguous per batch; metrics are order-free
                import torch.distributed as dist
                sizes = [None] * ctx.world
                dist.all_gather_object(sizes, int(y_true.size(0)))
                gt = [torch.empty((s, num_tasks), device=ctx.device) for s in sizes]
                gp = [torch.empty((s, num_tasks), device=ctx.device) for s in sizes]
                dist.all_gather(gt, y_true.contiguous())
                dist.all_gather(gp, y_pred.contiguous())
                y_true, y_pred = torch.cat(gt), torch.cat(gp)
            preds.append(y_pred.cpu().numpy())
        return evaluator.eval({"y_true": y_true.cpu().numpy(), "y_pred": np.stack(preds).mean(0)})

    valid_perfs, test_perfs = [], []
    start_run = args.run_from - 1
    for run in range(start_run, start_run + args.runs - args.run_from + 1):
        torch.manual_seed(run)                             # the reference leaves runs unseeded; seeded here for replay
        gen = torch.Generator().manual_seed(run)           # the shuffle order every rank shards identically
        if gineplus:                                       # reference :419-427
            from .modules.gine_operations import ClassifierNetwork
            model = ClassifierNetwork(hidden=args.emb_dim, out_dim=num_tasks, layers=args.num_layer, dropout=args.drop_ratio,
                                      virtual_node=args.virtual_node, k=GINEPLUS_K, conv_type="gin+", nested=False).to(ctx.device)
        else:
            model = GNN(args.dataset, num_tasks, gnn_type="gin_eff", emb_dim=args.emb_dim, drop_ratio=args.drop_ratio,
                        virtual_node=args.virtual_node, RNI=args.RNI, deg_graph=None, deg_sub=None, **kwargs).to(ctx.device)
        broadcast_parameters(model, 0)
        optimizer = FlatAdam(model.parameters(), lr=args.lr)
        scheduler = StepLR(optimizer, 20, args.lr_decay_factor) if args.scheduler else None
        start_epoch, epochs = 1, args.epochs
        if args.continue_from is not None:
            model.load_state_dict(torch.load(os.path.join(
                args.res_dir, "run{}_model_checkpoint{}.pth".format(run + 1, args.continue_from)), map_location=ctx.device))
            optimizer.load_state_dict(torch.load(os.path.join(
                args.res_dir, "run{}_optimizer_checkpoint{}.pth".format(run + 1, args.continue_from)),
                map_location=ctx.device))
            start_epoch, epochs = args.continue_from + 1, epochs - args.continue_from
        best_valid_perf, best_test_perf = -1e6, None       # classification: higher is better
        t3 = time.time()
        for epoch in range(start_epoch, start_epoch + epochs):
            ctx.say(f"=====Run {run + 1}, epoch {epoch}, {args.save_appendix}")
            ctx.say("Training...")
            loss = train(model, optimizer, gen)
            ctx.say("Evaluating...")
            valid_perf = evaluate(model, stores[1])[eval_metric]
            if valid_perf > best_valid_perf:
                best_valid_perf = valid_perf
                best_test_perf = evaluate(model, stores[2])[eval_metric]
                if ctx.rank == 0:
                    torch.save(model.state_dict(), os.path.join(args.res_dir, f"run{run + 1}_best_model.pth"))
            if scheduler is not None:
                scheduler.step()
            res = {"Epoch": epoch, "Loss": loss, "Cur Val": valid_perf, "Best Val": best_valid_perf,
                   "Best Test": best_test_perf}
            ctx.say(res)
            log(res)
            if epoch % args.log_steps == 0 and ctx.rank == 0:
                torch.save(model.state_dict(),
                           os.path.join(args.res_dir, "run{}_model_checkpoint{}.pth".format(run + 1, epoch)))
                torch.save(optimizer.state_dict(),
                           os.path.join(args.res_dir, "run{}_optimizer_checkpoint{}.pth".format(run + 1, epoch)))
        t4 = time.time()
        final_res = "Run {}\nBest validation score: {}\nTest score: {}\nPreprocessing time: {}\nTraining time: {}\n".format(
            run + 1, best_valid_perf, best_test_perf, t2 - t1, t4 - t3)
        ctx.say("Finished training!")
        ctx.say("python " + " ".join(sys.argv))
        ctx.say(final_res)
        log(final_res)
        if args.ensemble:
            ctx.say("Start ensemble testing...")
            lo, hi = args.epochs - args.ensemble_lookback, args.epochs
            ckpts = [os.path.join(args.res_dir, "run{}_model_checkpoint{}.pth".format(run + 1, x))
                     for x in range(lo, hi + 1, args.ensemble_interval)]
            if ctx.world > 1:
                import torch.distributed as dist
                dist.barrier()                             # rank 0 wrote the checkpoints
            ens_valid = evaluate(model, stores[1], ckpts)[eval_metric]
            ens_test = evaluate(model, stores[2], ckpts)[eval_metric]
            ens = "Run {}\nEnsemble validation score: {}\nEnsemble test score: {}\n".format(run + 1, ens_valid, ens_test)
            ctx.say(ens)
            log(ens)
            valid_perfs.append(ens_valid)
            test_perfs.append(ens_test)
        else:
            valid_perfs.append(best_valid_perf)
            test_perfs.append(best_test_perf)

    valid_perfs, test_perfs = torch.tensor(valid_perfs), torch.tensor(test_perfs)
    ctx.say("===========================")
    ctx.say(cmd_input)
    for name, v in (("Valid", valid_perfs), ("Test", test_perfs)):
        line = f"Final {name}: {v.mean():.4f} ± {v.std():.4f}"
        ctx.say(line)
        log(line)
    ctx.say(valid_perfs.tolist())
    ctx.say(test_perfs.tolist())
    ctx.close()


if __name__ == "__main__":
    main()
