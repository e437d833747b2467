"""QM9 property regression on the ESC hot path — the MI355X-native twin of the reference's run_qm9.py for
`--model NestedGIN_eff`: flags (:80-131), features `create_subgraphs(g, h, 'hop', use_rd=True, self_loop=True)` (:202-205),
y = data.y[:, target] (MyTransform :67-75) and the Distance transform (:222-224), shuffle, targets normalised by the mean /
std of dataset[10%:] (:293-296), test / validation / train = first 10 % / next 10 % / rest (:307-309), Adam +
ReduceLROnPlateau on the validation MAE (:329-331), F.mse_loss training (:348), MAE * std evaluation (:366-368) and the log
line of :385-393.  The checkpoint is written after the last epoch (:397-398).

The QM9 download is absent, so the data are seeded molecule-shaped graphs with positions (datasets.synthetic_qm9_graphs;
`--data_size`).  The dataset lives in HBM (DeviceGraphStore: node rows packed as [x | pos | node_type]); every batch is
collated on the device and the model runs per-op through libescgnn_hip.so (no whole-step engine: the widths 11 and 261
are no multiples of 4).  The evaluation error is accumulated on the device and read back once per loader.

Out of scope (NotImplementedError): the k-GNN / PPGN baseline models, --max_nodes_per_hop, --RNI.  The reference class
ignores --use_pos and --use_max_dist; they are accepted and ignored here too.

    python -m esc_gnn_amd.run_qm9 --target 0
"""
import torch

from . import ops
from .harness import Context, default_appendix, open_result_dir, parser_from, seed_everything, sharded_batches
from .qm9_models import NestedGIN_eff

# unit conversion of the 12 regression targets (reference :24-31): PyG's QM9 units back to the original ones
HAR2EV = 27.2113825435
KCALMOL2EV = 0.04336414
CONVERSION = (1., 1., HAR2EV, HAR2EV, HAR2EV, 1., HAR2EV, HAR2EV, HAR2EV, HAR2EV, HAR2EV, 1.)

_FLAGS = [  # same names and defaults as the reference CLI
    ("--target", dict(default=11, type=int)),
    ("--filter", dict(action="store_true", default=False, help="filter graphs with less than 7 nodes")),
    ("--convert", dict(type=str, default="post", help='"post": convert units after optimisation; "pre": before')),
    ("--model", dict(type=str, default="NestedGIN_eff", help="NestedGIN_eff (k-GNN / PPGN baselines: out of scope)")),
    ("--layers", dict(type=int, default=5)),
    ("--h", dict(type=int, default=3)),
    ("--max_nodes_per_hop", dict(type=int, default=None)),
    ("--node_label", dict(type=str, default="spd")),
    ("--use_rd", dict(action="store_true", default=False)),
    ("--subgraph_pooling", dict(default="mean")),
    ("--epochs", dict(type=int, default=200)),
    ("--batch_size", dict(type=int, default=64)),
    ("--lr", dict(type=float, default=1e-3)),
    ("--lr_decay_factor", dict(type=float, default=0.7)),
    ("--patience", dict(type=int, default=5)),
    ("--normalize_x", dict(action="store_true", default=False, help="normalise the non-binary node features (columns 5..)")),
    ("--squared_dist", dict(action="store_true", default=False)),
    ("--not_normalize_dist", dict(action="store_true", default=False)),
    ("--use_max_dist", dict(action="store_true", default=False)),
    ("--use_pos", dict(action="store_true", default=False)),
    ("--RNI", dict(action="store_true", default=False)),
    ("--use_relative_pos", dict(action="store_true", default=False)),
    ("--seed", dict(type=int, default=1)),
    ("--save_appendix", dict(default="")),
    ("--keep_old", dict(action="store_true", default=False)),
    # additions (not in the reference)
    ("--data_size", dict(type=int, default=12000, help="number of synthetic molecules (test 10 % / validation 10 % / train 80 %)")),
    ("--res_dir", dict(default=None, help="result directory (default results/QM9_<target><save_appendix>)")),
]
REFERENCE_FLAGS = tuple(name for name, _ in _FLAGS[:-2])


def build_parser():
    return parser_from(_FLAGS, "ESC-GNN for QM9 graphs (MI355X hot path).")


class _Features(object):
    """what the model's constructor reads from its `dataset` argument (reference qm9_models.py:53)"""

    def __init__(self, num_features):
        self.num_features = num_features


def _load_dataset(args):
    """shuffled, feature-built, distance-augmented graphs with normalised targets -> (graphs, std of the target)"""
    from .datasets import build_qm9_dataset, synthetic_qm9_graphs
    raw = synthetic_qm9_graphs(0, args.data_size)
    if args.filter:
        raw = [d for d in raw if d.x.size(0) > 6]                                  # MyFilter, reference :34-36
    done = build_qm9_dataset(raw, args.h, args.target, norm=not args.not_normalize_dist, relative_pos=args.use_relative_pos,
                             squared=args.squared_dist)
    order = torch.randperm(len(done), generator=torch.Generator().manual_seed(args.seed)).tolist()
    done = [done[i] for i in order]                                                 # dataset.shuffle(), :243
    ten = int(len(done) * 0.1)
    y = torch.cat([d.y for d in done])
    mean, std = y[ten:].mean(dim=0), y[ten:].std(dim=0)                             # :293-296
    for d in done:
        d.y = (d.y - mean) / std
        if args.convert == "pre":                                                   # MyTransform(pre_convert), applied at access
            d.y = d.y / CONVERSION[args.target]
    if args.normalize_x:                                                            # :300-305
        x = torch.cat([d.x[:, 5:] for d in done[2 * ten:]])
        x_mean, x_std = x.mean(dim=0), x.std(dim=0)
        for d in done:
            d.x = torch.cat([d.x[:, :5], (d.x[:, 5:] - x_mean) / x_std], 1)
    return done, ten, float(std)


def main(argv=None):
    import os
    import time

    from .optim import FlatAdam, ReduceLROnPlateau
    from .store import DeviceGraphStore

    args = build_parser().parse_args(argv)
    if args.model != "NestedGIN_eff":
        raise NotImplementedError("--model %s: only NestedGIN_eff runs on the ESC hot path (the k-GNN and PPGN baselines "
                                  "are out of scope)" % args.model)
    if args.max_nodes_per_hop is not None:
        raise NotImplementedError("max_nodes_per_hop: random neighbour sampling is outside the ESC hot path")
    if args.RNI:
        raise NotImplementedError("--RNI: random node initialisation belongs to the baseline models (the reference's "
                                  "NestedGIN_eff ignores it)")
    if not 0 <= args.target < 12:
        raise ValueError("--target %d: the regression targets are 0..11" % args.target)
    if args.convert not in ("post", "pre"):
        raise ValueError("--convert %r: 'post' or 'pre'" % args.convert)
    ctx = Context()
    if ctx.world > 1:
        raise NotImplementedError("run_qm9 runs on one device")
    seed_everything(args.seed)
    args.save_appendix = default_appendix(args.save_appendix)
    if args.res_dir is None:
        args.res_dir = "results/QM9_{}{}".format(args.target, args.save_appendix)  # reference :145
    cmd_input = open_result_dir(ctx, args.res_dir, ("run_qm9.py", "utils_edge_efficient.py", "qm9_models.py"))

    t0 = time.time()
    graphs, ten, std = _load_dataset(args)
    print("Preprocessing time cost: {}s,".format(time.time() - t0))
    test_store, val_store, train_store = (DeviceGraphStore(part, ctx.device) for part in
                                          (graphs[:ten], graphs[ten:2 * ten], graphs[2 * ten:]))
    n_train = len(train_store)

    model = NestedGIN_eff(_Features(graphs[0].x.size(1)), num_layers=args.layers, subgraph_pooling=args.subgraph_pooling,
                          use_pos=args.use_pos, edge_attr_dim=8 if args.use_relative_pos else 5,
                          use_max_dist=args.use_max_dist, use_rd=args.use_rd, RNI=args.RNI)
    print("Using " + model.__class__.__name__ + " model")
    model = model.to(ctx.device)
    optimizer = FlatAdam(model.parameters(), lr=args.lr)
    scheduler = ReduceLROnPlateau(optimizer, factor=args.lr_decay_factor, patience=args.patience, min_lr=0.00001)
    gen = torch.Generator().manual_seed(args.seed)

    def train(epoch):
        model.train()
        loss_all = torch.zeros((), device=ctx.device)
        for data, n_graphs in sharded_batches(train_store, args.batch_size, ctx, True, gen):
            optimizer.zero_grad()
            loss = ops.mse_loss(model(data), data.y)       # F.mse_loss, reference :348
            loss.backward()
            loss_all += loss.detach() * n_graphs
            optimizer.step()
        return float(loss_all) / n_train

    def test(store):
        model.eval()
        err = torch.zeros((), device=ctx.device)           # on the device: one read-back per loader
        with torch.no_grad():
            for data, _ in sharded_batches(store, args.batch_size, ctx, False):
                err += (model(data) * std - data.y * std).abs().sum()
        return float(err) / len(store)

    t1 = time.time()
    best_val_error, log = None, ""
    for epoch in range(1, args.epochs + 1):
        lr = optimizer.param_groups[0]["lr"]
        loss = train(epoch)
        val_error = test(val_store)
        scheduler.step(val_error)
        if best_val_error is None:
            best_val_error = val_error
        if val_error <= best_val_error:
            test_error = test(test_store)
            best_val_error = val_error
            log = ("Epoch: {:03d}, LR: {:7f}, Loss: {:.7f}, Validation MAE: {:.7f}, "
                   "Test MAE: {:.7f}, Test MAE norm: {:.7f}, Test MAE convert: {:.7f}").format(
                epoch, lr, loss, val_error, test_error, test_error / std,
                test_error / CONVERSION[args.target] if args.convert == "post" else 0)
            print(log)
            with open(os.path.join(args.res_dir, "log.txt"), "a") as fh:
                fh.write(log + "\n")
    torch.save(model.state_dict(), os.path.join(args.res_dir, "model_checkpoint{}.pth".format(args.epochs)))
    print("Training time cost: {}s".format(time.time() - t1))
    print(cmd_input[:-1])
    print(log)
    ctx.close()


if __name__ == "__main__":
    main()
