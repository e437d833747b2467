"""ZINC cycle counting on the ESC hot path — the MI355X-native twin of the reference's run_zinc_cycle.py for
`--model NestedGIN_eff` and the subgraph baseline `--model I2GNN`: flags (:20-85), feature settings (`create_subgraphs_eff(g, h, use_rd, self_loop)` :140-146),
targets y = data.y[:, target] without normalisation (:205-215: the normalising lines are commented out there, the
Mean / Std are printed and Std scales the reported MAE), L1 over the NODES, and "test when validation improves or every 10
epochs" logging (:282-325).  test() returns sum |y_hat - y| over the nodes / the number of GRAPHS * std (:292-306).

The raw ZINC.pkl of the reference (a DGL pickle) is absent, so the data are seeded ring-closed molecules whose node labels
(3- to 6-cycles through each node, dataset_zinc_cycle.py:45-61) are counted on the device (datasets.
synthetic_zinc_cycle_graphs, csrc/cycles.hip).  The whole dataset lives in HBM (DeviceGraphStore); forward, loss,
backward and Adam run through libescgnn_hip.so (esc_zinc_* with node_readout = 1); under torchrun the global batch is
sharded by graph and every loss / gradient denominator is the global NODE count.

Deviation: the reference's `--eval` branch unpacks six values from a test() that returns one, so it cannot run; here it
prints `Test MAE` as run_zinc does.

`--model I2GNN` (reference :159-161, zinc_cycle_models.py:116-307, the reference's default model) trains the subgraph GNN
that counts cycles on the same molecules and labels: the split holds the plain graphs (subgraphs2.I2GraphStore), and every
step expands the batch into one copy of every rooted subgraph per neighbour of its root on the device
(subgraphs2.expand_subgraphs2, csrc/subgraphs.hip) before the per-op forward / L1 / backward / Adam.

    python -m esc_gnn_amd.run_zinc_cycle --model NestedGIN_eff --h 3 --target 0
    python -m esc_gnn_amd.run_zinc_cycle --model I2GNN --h 3 --target 0
"""
import torch

from . import ops
from .harness import (Context, default_appendix, expanded_batches, fit_regression, open_result_dir, parser_from, prefetched,
                      seed_everything, sharded_batches)
from .zinc_cycle_models import I2GNN, NestedGIN_eff

_FLAGS = [  # same names, types and defaults as the reference CLI
    ("--target", dict(default=0, type=int, help="cycle length - 3: column of the [n, 4] node labels")),
    ("--filter", dict(action="store_true", default=False)),
    ("--convert", dict(type=str, default="post")),
    ("--model", dict(type=str, default="NestedGIN_eff", help="NestedGIN_eff | I2GNN (GNN / NGNN baselines: out of scope)")),
    ("--layers", dict(type=int, default=6)),
    ("--h", dict(type=int, default=3)),
    ("--max_nodes_per_hop", dict(type=int, default=None)),
    ("--node_label", dict(type=str, default="spd")),
    ("--use_rd", dict(action="store_true", default=True)),
    ("--subgraph2_pooling", dict(default="mean-center-side")),
    ("--subgraph_pooling", dict(default="mean-context")),
    ("--use_pooling_nn", dict(action="store_true", default=False)),
    ("--virtual_node", dict(action="store_true", default=False)),
    ("--double_pooling", dict(action="store_true", default=True)),
    ("--gate", dict(action="store_true", default=True)),
    ("--epochs", dict(type=int, default=1000)),
    ("--batch_size", dict(type=int, default=256)),
    ("--lr", dict(type=float, default=1e-3)),
    ("--lr_decay_factor", dict(type=float, default=0.95)),
    ("--patience", dict(type=int, default=10)),
    ("--drop_ratio", dict(type=float, default=0.0)),
    ("--normalize_x", dict(action="store_true", default=False)),
    ("--squared_dist", dict(action="store_true", default=False)),
    ("--not_normalize_dist", dict(action="store_true", default=False)),
    ("--use_max_dist", dict(action="store_true", default=False)),
    ("--use_pos", dict(action="store_true", default=False)),
    ("--RNI", dict(action="store_true", default=False)),
    ("--use_relative_pos", dict(action="store_true", default=False)),
    ("--self_loop", dict(action="store_true", default=False)),
    ("--seed", dict(type=int, default=1)),
    ("--save_appendix", dict(default="")),
    ("--keep_old", dict(action="store_true", default=False)),
    ("--dataset", dict(default="zinc")),
    ("--load_model", dict(default=None)),
    ("--eval", dict(default=0, type=int)),
    ("--train_only", dict(default=0, type=int)),
    # additions (not in the reference): size of the synthetic stand-in for the absent ZINC.pkl
    ("--synthetic_graphs", dict(type=int, default=12000, help="train+val+test ring-closed molecules (10:1:1 like ZINC-12k)")),
    ("--prefetch", dict(action="store_true", default=False,
                        help="collate the next batch on a side stream (harness.prefetched); slower on MI355X at config 4 "
                             "(1.20 vs 1.11 ms/step: the step is a chain of small launches), see DESIGN.md 4 (measured on run_zinc)")),
    ("--sync_bn", dict(action="store_true", default=False,
                       help="data parallel only: BatchNorm statistics over all ranks (single-device-equivalent numerics)")),
]


def build_parser():
    return parser_from(_FLAGS, "ESC-GNN for ZINC cycle counting (MI355X hot path).")


def _load_splits(args):
    from .datasets import build_feature_dataset, synthetic_zinc_cycle_graphs
    G = args.synthetic_graphs
    raw = synthetic_zinc_cycle_graphs(0, G)
    if args.model == "I2GNN":                             # plain molecules: the subgraph2s are expanded per batch
        done = raw
    else:
        done = build_feature_dataset(raw, args.h, use_rd=args.use_rd, self_loop=args.self_loop)     # reference :140-146
    n_tr, n_va = (G * 10) // 12, G // 12
    return done[:n_tr], done[n_tr:n_tr + n_va], done[n_tr + n_va:]


def main(argv=None):
    import time

    from .optim import FlatAdam, ReduceLROnPlateau
    from .parallel import broadcast_buffers, broadcast_parameters
    from .store import DeviceGraphStore

    args = build_parser().parse_args(argv)
    if args.model not in ("NestedGIN_eff", "I2GNN"):
        print("Error: no such model!")                    # reference :166-168 (GNN / NGNN: out of scope)
        raise SystemExit(1)
    i2gnn = args.model == "I2GNN"
    if i2gnn:                                             # what the expansion has no path for: refused before anything is built
        from .subgraphs2 import check_args
        check_args(args.h, args.node_label, args.max_nodes_per_hop, None, args.self_loop)
    if args.max_nodes_per_hop is not None:
        raise NotImplementedError("max_nodes_per_hop: random neighbour sampling is outside the ESC hot path")
    if not 0 <= args.target < 4:
        raise ValueError("--target %d: the labels are the 3-, 4-, 5- and 6-cycles (columns 0..3)" % args.target)
    ctx = Context()
    seed_everything(args.seed)
    args.save_appendix = default_appendix(args.save_appendix)
    args.res_dir = "results/" + args.dataset + "_" + args.model + args.save_appendix
    cmd_input = open_result_dir(ctx, args.res_dir, ("run_zinc_cycle.py", "utils_edge_efficient.py", "zinc_cycle_models.py"))

    t11 = time.time()
    tr, va, te = _load_splits(args)
    ctx.say("Preprocessing time cost: {}s,".format(time.time() - t11))
    target = args.target
    y_train_val = torch.cat([d.y[:, target] for d in tr + va], dim=0)       # reference :209-215 (not applied)
    mean, std = y_train_val.mean(dim=0), y_train_val.std(dim=0)
    ctx.say("Mean = %.3f, Std = %.3f" % (float(mean), float(std)))
    if i2gnn:                                             # per-graph sizes and both limits: one count pass per split
        from .subgraphs2 import I2GraphStore
        stores = [I2GraphStore(part, args.h, args.use_rd, ctx.device) for part in (tr, va, te)]
    else:
        stores = [DeviceGraphStore(part, ctx.device) for part in (tr, va, te)]
    n_train = len(tr)

    if i2gnn:
        model = I2GNN(None, num_layers=args.layers, subgraph_pooling=args.subgraph_pooling,
                      subgraph2_pooling=args.subgraph2_pooling, use_pos=args.use_pos, edge_attr_dim=5,
                      use_max_dist=args.use_max_dist, use_rd=args.use_rd, RNI=args.RNI, drop_ratio=args.drop_ratio,
                      use_pooling_nn=args.use_pooling_nn, use_virtual_node=args.virtual_node,
                      double_pooling=args.double_pooling, gate=args.gate)               # reference :241-255
    else:
        model = NestedGIN_eff(None, num_layers=args.layers, use_rd=args.use_rd, RNI=args.RNI, drop_ratio=args.drop_ratio,
                              edge_attr_dim=5, use_pos=args.use_pos, use_max_dist=args.use_max_dist)
    if args.load_model is not None:
        model.load_state_dict(torch.load(args.load_model, map_location="cpu"))
    ctx.say("Using " + model.__class__.__name__ + " model")
    model = model.to(ctx.device)
    if args.sync_bn and ctx.world > 1:
        from .nn import BatchNorm1d
        BatchNorm1d.convert_sync(model)
    broadcast_parameters(model, 0)
    optimizer = FlatAdam(model.parameters(), lr=args.lr)
    scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=args.lr_decay_factor, patience=args.patience,
                                  min_lr=0.00001)
    gen = torch.Generator().manual_seed(args.seed)

    from .engine import ZincStepEngine, zinc_engine_ready, zinc_engine_supports
    engine = ZincStepEngine(model) if zinc_engine_supports(model) else None     # forward + L1 + backward in ONE call

    def train(epoch):
        # loss_all: sum over batches of (node-mean L1) * (graphs in the global batch), reference :272-284
        model.train()
        loss_all = torch.zeros((), device=ctx.device)
        batches = sharded_batches(stores[0], args.batch_size, ctx, True, gen)
        if args.prefetch:         # the next batch is collated on a side stream while this one trains
            batches = prefetched(batches, ctx.device)
        if i2gnn:                 # every plain batch becomes the disconnected graph of its subgraph2s, on the device
            batches = expanded_batches(stores[0], batches)
        for data, n_graphs in batches:
            y = data.y[:, target].contiguous()
            n_loc = y.numel()
            if engine is not None and zinc_engine_ready(model, data):
                if ctx.world > 1:                          # sums, one all-reduce of grad ++ [nodes], division inside Adam
                    s = engine.train_step(data, loss_denom=1, y=y)
                    n_all = optimizer.all_reduce_sum(n_loc)
                    loss_all += s / n_all[0] * n_graphs
                    optimizer.step(grad_denom=n_all)
                else:
                    loss_all += engine.train_step(data, y=y) * n_graphs
                    optimizer.step()
                continue
            optimizer.zero_grad()
            y = y.view(-1, 1)
            if ctx.world > 1 and args.sync_bn:            # one objective shared by the ranks: sum form, divided once
                loss = ops.l1_loss(model(data), y, denom=1)
                loss.backward()
                n_all = optimizer.all_reduce_sum(n_loc)
                loss_all += loss.detach() / n_all[0] * n_graphs
                optimizer.step(grad_denom=n_all)
                continue
            loss = ops.l1_loss(model(data), y)            # torch.nn.L1Loss over the nodes (reference :277-279)
            loss.backward()
            n_all = float(optimizer.all_reduce_weighted(n_loc)) if ctx.world > 1 else n_loc
            loss_all += loss.detach() * (n_loc / n_all) * n_graphs
            optimizer.step()
        return float(ctx.all_reduce(loss_all)) / n_train

    def test(store):
        broadcast_buffers(model, 0)                        # rank-local BatchNorm running statistics -> rank 0's everywhere
        model.eval()
        err = torch.zeros(1, device=ctx.device)
        with torch.no_grad():
            batches = sharded_batches(store, args.batch_size, ctx, False)
            for data, _ in (expanded_batches(store, batches) if i2gnn else batches):
                y_hat = model(data)[:, 0]
                err += torch.sum(torch.abs(y_hat - data.y[:, target]))
        ctx.all_reduce(err)
        return float(err) / len(store) * float(std)       # reference :292-306: divided by the number of GRAPHS

    if args.eval:
        print("Test MAE: %.7f" % test(stores[2]))         # (the reference's branch cannot run: see the module docstring)
        ctx.close()
        return
    fit_regression(ctx, args, model, optimizer, scheduler, train, test, stores[1], stores[2], std, cmd_input)
    ctx.close()


if __name__ == "__main__":
    main()
