"""NestedGIN_eff for the substructure-counting benchmark + its training harness — the MI355X-native
twin of /root/reference/run_graphcount.py (model :39-194, CLI :315-358, data wiring :393-455,
train/test/loop :483-613).

Same constructor, forward contract and state_dict key layout as the reference class, so a
checkpoint written by either loads into the other (`--load_model`, reference :472-474).
All device arithmetic of forward/backward goes through libescgnn_hip.so.
"""
import torch
import torch.nn.functional as F

from . import engine, nested
from .harness import (Context, default_appendix, fit_regression, open_result_dir, parser_from, seed_everything,
                      sharded_batches, sharded_ids)
from .nested import Z_TABLE_ROWS  # noqa: F401  (bench.py and the package root read it from here)
from .nn import BatchNorm1d, GINEConv, Linear, global_mean_pool
from .plan import plan_of


class NestedGIN_eff(torch.nn.Module):
    def __init__(self, dataset, num_layers, hidden, use_z=False, use_rd=False, use_cycle=False, graph_pred=True,
                 use_id=None, dropout=0.2, multi_layer=False, edge_nest=False):
        super().__init__()
        if use_id is not None:
            raise NotImplementedError("use_id: the identity-aware baseline is outside the ESC hot path")
        # stored-but-unused flags are kept for interface parity (reference :43-50)
        self.use_rd, self.use_z, self.graph_pred, self.use_cycle = use_rd, True, graph_pred, use_cycle
        self.use_id, self.dropout, self.multi_layer, self.edge_nest = use_id, dropout, multi_layer, edge_nest
        input_dim = 10
        self.z_initial = torch.nn.Embedding(Z_TABLE_ROWS, hidden)
        self.z_embedding = nested.z_embedding(hidden, dropout=dropout)
        self.x_embedding = nested.mlp(input_dim, hidden, dropout)
        self.conv1 = GINEConv(nested.mlp(input_dim, hidden, dropout), train_eps=True, edge_dim=hidden)
        self.convs = torch.nn.ModuleList(
            GINEConv(nested.mlp(hidden, hidden, dropout), train_eps=True, edge_dim=hidden)
            for _ in range(num_layers - 1))
        self.lin1 = Linear(num_layers * hidden + hidden, hidden)
        self.bn_lin1 = BatchNorm1d(hidden, eps=1e-5, momentum=0.1, fuse_relu=True)
        self.lin2 = Linear(hidden, 1 if use_cycle else dataset.num_classes)
        self.engine_forward = True       # training-mode forward through the whole-step engine when it covers the config

    def reset_parameters(self):
        nested.reset_parameters(self, "z_embedding", "conv1", "convs", "lin1", "bn_lin1", "lin2")

    def forward(self, data, return_embeddings=False):
        data.to(self.lin1.weight.device)
        x, edge_index, batch = data.x, data.edge_index, data.batch
        if (self.training == torch.is_grad_enabled() and not return_embeddings and self.engine_forward
                and "edge_pos" not in data and x.is_floating_point() and x.dim() == 2 and x.size(0) >= 2
                and edge_index.size(1) >= 2 and "pos_batch" in data       # the engine's own preconditions (esc::check)
                and x.size(1) == self.x_embedding[0].in_features):
            if self.training:
                cache = (engine._node_cache(self, engine.COUNTING) if self.lin1.weight.device.type == "cuda"
                         and 1 + len(self.convs) <= engine.MAX_LAYERS else None)
                if engine.engine_supports(self, cache):
                    return engine.engine_forward(self, data, cache)       # the whole step as one autograd node (engine.hip)
            elif engine.engine_supports(self):
                return engine.engine_predict(self, data)       # eval-mode forward as one call (esc_engine_predict)
        plan = plan_of(data, Z_TABLE_ROWS)
        z = self.z_embedding(nested.edge_term(self.z_initial, data, plan))
        cat = torch.cat(nested.conv_stack(self, x, edge_index, z, plan, skip=self.x_embedding), dim=1)
        if self.graph_pred:
            cat = global_mean_pool(cat, batch)
        o = self.lin1(cat)
        o = self.bn_lin1(o) if o.size(0) > 1 else F.relu(o)      # bn_lin1 carries the ReLU of reference :186
        o = F.dropout(o, p=self.dropout, training=self.training)
        o = self.lin2(o)
        if not self.use_cycle:
            o = F.log_softmax(o, dim=-1)
        return (o, cat) if return_embeddings else o


# =====================================================================================================
# Training harness — `python -m esc_gnn_amd.run_graphcount ...` (flags of reference :315-358)
# =====================================================================================================
_FLAGS = [  # (name, kwargs) — same names, types and defaults as the reference CLI
    ("--model", dict(default="NestedGIN_eff", type=str, help="NestedGIN_eff (PPGN_eff: dense 3-WL baseline, out of scope)")),
    ("--target", dict(default=3, type=int)),
    ("--ab", dict(action="store_true", default=False)),
    ("--layers", dict(type=int, default=5)),
    ("--h", dict(type=int, default=3, help="hop of enclosing subgraph")),
    ("--max_nodes_per_hop", dict(type=int, default=None)),
    ("--node_label", dict(type=str, default="hop")),
    ("--epochs", dict(type=int, default=2000)),
    ("--batch_size", dict(type=int, default=256)),
    ("--lr", dict(type=float, default=1e-3)),
    ("--lr_decay_factor", dict(type=float, default=0.9)),
    ("--patience", dict(type=int, default=10)),
    ("--normalize_x", dict(action="store_true", default=False)),
    ("--not_normalize_dist", dict(action="store_true", default=False)),
    ("--RNI", dict(action="store_true", default=False)),
    ("--use_relative_pos", dict(action="store_true", default=False)),
    ("--seed", dict(type=int, default=0)),
    ("--save_appendix", dict(default="")),
    ("--keep_old", dict(action="store_true", default=False)),
    ("--dataset", dict(default="count_cycle", help="count_cycle/count_graphlet")),
    ("--load_model", dict(default=None)),
    ("--eval", dict(default=0, type=int)),
    ("--train_only", dict(default=0, type=int)),
    # additions (not in the reference): synthetic data when data/<dataset>/raw/data.mat is absent
    ("--synthetic_graphs", dict(type=int, default=5000, help="size of the synthetic count_cycle-shaped dataset")),
    ("--data_root", dict(default="data")),
    ("--synthetic_labels", dict(default="triangle", choices=("triangle", "task"),
                                help="labels of the synthetic dataset: the per-node triangle count whatever --dataset and "
                                     "--target say, or the task's own (count_cycle: 3..6-cycles, count_graphlet: the five "
                                     "graphlets, column --target), counted on the device; ignored with a real data.mat")),
    ("--graphlet_orbit", dict(type=int, default=-1,
                              help="with --synthetic_labels task on count_graphlet: count only the copies that hold the "
                                   "node at the K-th orbit of the pattern (-1: at any position)")),
]


def build_parser():
    return parser_from(_FLAGS, "NestedGNN for counting experiments (MI355X hot path).")


def _mat_path(args):
    import os
    return os.path.join(args.data_root, args.dataset, "raw", "data.mat")


def task_label_column(dataset, target, orbit=-1):
    """(labels, column) of `--synthetic_labels task`: the `labels` kind of datasets.synthetic_count_graphs and the column
    of its y that --dataset / --target / --graphlet_orbit select.  ValueError for a name or an index outside the task."""
    from .graphlets import GRAPHLET_NAMES, GRAPHLET_ORBITS
    if dataset == "count_cycle":
        if not 0 <= target <= 3:
            raise ValueError("--target %d: count_cycle has targets 0..3 (the 3-, 4-, 5- and 6-cycles)" % target)
        if not -1 <= orbit <= 0:
            raise ValueError("--graphlet_orbit %d: a cycle has one orbit, valid values are -1..0" % orbit)
        return "cycles", target
    if dataset == "count_graphlet":
        if not 0 <= target <= 4:
            raise ValueError("--target %d: count_graphlet has targets 0..4 (%s)" % (target, ", ".join(GRAPHLET_NAMES)))
        cols = GRAPHLET_ORBITS[target]
        if not -1 <= orbit < len(cols):
            raise ValueError("--graphlet_orbit %d: the %s of --target %d has orbits 0..%d (-1: any position)"
                             % (orbit, GRAPHLET_NAMES[target], target, len(cols) - 1))
        return ("graphlets", target) if orbit < 0 else ("graphlet_orbits", cols[orbit])
    raise ValueError("--dataset %s: --synthetic_labels task knows count_cycle and count_graphlet" % dataset)


def _load_splits(args, labels="triangle"):
    """train/val/test lists of pre-transformed Data (reference :404-430)."""
    import os
    from .datasets import build_count_dataset, load_count_mat
    from .utils_edge_efficient import create_subgraphs_many
    mat = _mat_path(args)
    if os.path.exists(mat):
        splits = []
        for name in ("train", "val", "test"):
            raw = load_count_mat(mat, name)
            splits.append(create_subgraphs_many(raw, args.h, use_rd=True, self_loop=True))
        return splits, True
    G = args.synthetic_graphs
    n_tr, n_val = int(0.3 * G), int(0.2 * G)              # 30/20/50 split by index
    alld = build_count_dataset(0, G, h=args.h, use_rd=True, self_loop=True, labels=labels)
    return [alld[:n_tr], alld[n_tr:n_tr + n_val], alld[n_tr + n_val:]], False


def main(argv=None):
    import os

    from .optim import FlatAdam, ReduceLROnPlateau
    from .parallel import broadcast_buffers, broadcast_parameters, edge_pipeline_parameters
    from .store import DeviceGraphStore

    args = build_parser().parse_args(argv)
    if args.model != "NestedGIN_eff":
        print("Model not implemented")
        raise NotImplementedError
    # the task's own labels on the synthetic dataset (a real data.mat carries its own): checked before anything is built
    task = None
    if args.synthetic_labels == "task" and not os.path.exists(_mat_path(args)):
        task = task_label_column(args.dataset, int(args.target), int(args.graphlet_orbit))
    ctx = Context()
    world, device = ctx.world, ctx.device
    seed_everything(args.seed)                            # reference :361-366
    args.save_appendix = default_appendix(args.save_appendix)
    args.res_dir = "results/" + args.dataset + "_" + args.save_appendix
    cmd_input = open_result_dir(ctx, args.res_dir, ("run_graphcount.py", "utils_edge_efficient.py"))   # reference :381-383
    target = int(args.target)
    ctx.say("---- Target: {} ----".format(target))

    (tr, va, te), real = _load_splits(args, "triangle" if task is None else task[0])

    def column(d):                                        # MyTransform (reference :35-37)
        y = d.y
        if task is not None and not real:
            return y[:, task[1]]
        return y[:, target] if (real and y.dim() == 2) else y.reshape(-1)
    for part in (tr, va, te):
        for d in part:
            d.y = column(d).float()
    y_train_val = torch.cat([d.y for d in tr + va])       # reference :441-447
    mean, std = y_train_val.mean(), y_train_val.std()
    if task is not None and not float(std) > 0:
        raise ValueError("--dataset %s --target %d: the label is constant over the train and validation graphs "
                         "(std %s), there is nothing to fit" % (args.dataset, target, float(std)))
    for part in (tr, va, te):
        for d in part:
            d.y = (d.y - mean) / std
    ctx.say("Mean = %.3f, Std = %.3f" % (float(mean), float(std)))
    stores = [DeviceGraphStore(part, device) for part in (tr, va, te)]
    n_train_targets = sum(d.y.numel() for d in tr)

    model = NestedGIN_eff(None, args.layers, 256, use_rd=True, graph_pred=False, dropout=0, edge_nest=True,
                          use_cycle=True)                # reference :465
    if args.load_model is not None:
        model.load_state_dict(torch.load(args.load_model, map_location="cpu"))
    ctx.say("Using " + model.__class__.__name__ + " model")
    model = model.to(device)
    broadcast_parameters(model, 0)
    # world > 1: two gradient buckets — node-pipeline parameters first, the edge pipeline's (whose gradients are final only
    # after the backward tail) behind them
    optimizer = FlatAdam(model.parameters(), lr=args.lr, late=edge_pipeline_parameters(model))
    scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=args.lr_decay_factor, patience=args.patience,
                                  min_lr=0.00001)
    step = engine.StepEngine(model)         # one native call per step; same parameters / .grad slots / BN buffers
    gen = torch.Generator().manual_seed(args.seed)

    def train(epoch):
        model.train()
        loss_all = torch.zeros((), device=device)
        todo = sharded_ids(stores[0], args.batch_size, ctx, True, gen)
        first = next(todo, None)
        data = None if first is None else stores[0].collate(first[0])
        while data is not None:
            n_local = data.y.size(0)
            # forward + L1Loss + backward (reference :494-503); the next batch is collated between the two halves of
            # the step, while the edge pipeline finishes.  world > 1: sum-gradients, one all-reduce of grad ++ [n_local],
            # division inside the Adam launch
            loss = step.begin_step(data, loss_denom=1 if world > 1 else None)
            ids = next(todo, None)
            upcoming = None if ids is None else stores[0].collate(ids[0])
            if world > 1:
                optimizer.all_reduce_early()        # overlaps the edge pipeline's backward tail
            step.end_step()
            if world > 1:
                loss_all += loss
                optimizer.step(grad_denom=optimizer.all_reduce_late(n_local))
            else:
                loss_all += loss * n_local
                optimizer.step()
            data = upcoming
        return float(ctx.all_reduce(loss_all)) / n_train_targets

    def test(store):
        # BatchNorm running statistics were updated from rank-local shards: evaluate (and later checkpoint) rank 0's on
        # every rank, so that the logged MAE is the one the saved model reproduces
        broadcast_buffers(model, 0)
        model.eval()
        err, num = torch.zeros((), device=device), 0
        with torch.no_grad():
            for data, _ in sharded_batches(store, args.batch_size, ctx, False):
                y_hat = step.predict(data)[:, 0]
                err += torch.sum(torch.abs(y_hat - data.y))
                num += data.y.size(0)
        tot = torch.stack([err, torch.tensor(float(num), device=device)])
        ctx.all_reduce(tot)
        return float(tot[0] / tot[1]) * float(std)

    if args.eval:
        print("Test MAE: %.7f" % test(stores[2]))
        return
    log = fit_regression(ctx, args, model, optimizer, scheduler, train, test, stores[1], stores[2], std, cmd_input,
                         timed=False)                    # reference :585-613 prints no training time ...
    if ctx.rank == 0:
        with open(os.path.join(args.res_dir, "log.txt"), "a") as fh:
            fh.write(log + "\n")                          # ... and writes the last line a second time
    ctx.close()


if __name__ == "__main__":
    main()
