"""ZINC driver of ESC-GNN inside a graph transformer — the MI355X-native twin of the reference's GraphGPS fork run with
GraphGPS/configs/GPS/zinc-GPS.yaml: GPSModel (gps_models.py) with ten `GINE+Transformer` layers of width 64 and 4 heads, AdamW
with weight decay 1e-5, gradient-norm clipping at 1.0 (graphgps/config/optimizers_config.py), the cosine schedule with 50
warm-up epochs, L1 loss on the raw targets (GraphGPS does not normalise y), batch 32.  Every flag's default is that file's value.

Data are what run_zinc uses: seeded ZINC-shaped molecules (datasets.synthetic_zinc_graphs; data/zinc/raw/ZINC.pkl is absent),
then the ESC features of create_subgraphs_eff(h, use_rd=True, self_loop=True) (GraphGPS/graphgps/loader/master_loader.py:32-33),
the whole dataset resident in HBM (DeviceGraphStore).  The loop is run_zinc's per-op branch: forward, ops.l1_loss, backward, one
flat AdamW launch whose gradient divisor is the clipping scale (no read-back), driven by harness.fit_regression.
The attention of every layer runs straight off the batch's graph_ptr (csrc/attention.hip); the largest graph of the store is
known on the host and travels on the batch, so nothing is read back for it.

--posenc_LapPE 1 selects the yaml's node encoder, TypeDictNode+LapPE (posenc_LapPE: laplacian_norm none, eigvec_norm L2,
max_freqs 8, DeepSet, dim_pe 8, 2 layers): one lappe.LapPETable per split is computed on the device after the stores (one launch
each), every batch gets its rows with one gather launch, and checkpoints carry the reference's key layout
(encoder.node_encoder.encoder1.* / encoder2.*).  The default, 0, is TypeDictNode at full width.

--posenc_RWSE 1 adds the random-walk structural encoding GraphGPS is normally run with on ZINC (node encoder TypeDictNode+RWSE,
or TypeDictNode+LapPE+RWSE with --posenc_LapPE 1 as well): one rwse.RWSETable per split - the landing probabilities of
--posenc_RWSE_ksteps steps, one launch each - and one more gather launch per batch.  The reference ships no yaml that enables
RWSE: the posenc_RWSE_* defaults (20 steps, dim_pe 28, linear, BatchNorm on the raw statistics) are upstream GraphGPS's usual
ZINC values, this project's choice.

--gt_layer_type picks the two halves of every layer as the yaml's gt.layer_type does: the local GNN is GINE (the yaml's),
CustomGatedGCN (nn.GatedGCNLayer on the fused gate kernel, csrc/gatedgcn.hip; it also updates the edge attributes from layer to
layer, so the ESC term of layer l is carried and re-gated) or PNA (nn.PNAConv on the fused mean | max | sum aggregate,
csrc/pna.hip; the edge attributes pass through as with GINE), the global model Transformer, BiasedTransformer or None (no
attention branch).  A checkpoint of one layout is refused by another (load_state_dict's own error).

<local GNN>+BiasedTransformer adds Graphormer's spatial encoding to the attention as the reference's fork defines it
(gps_layer.py:237-239,273-278): every layer's edge_attn_emb / edge_attn_linear turn the shortest-path distance of a pair into a
per-head bias on its score.  One spd.SPDTable per split - the all-pairs distances of every graph, one launch each
(csrc/spd.hip) - and one more gather launch per batch; the attention reads the bytes in place.  Same state_dict as Transformer.

--gt_layer_norm 1 --gt_batch_norm 0 is the yaml's other normalisation (gt.layer_norm): the three norms of every layer become PyG's
graph-mode LayerNorm - one mean and one variance over all nodes and channels of each graph, one launch forward and two backward
with the residual add folded in (csrc/layernorm.hip) - the GPS recipe's choice for small batches and for inference one graph
at a time.  Both 0 runs without the three norms; both 1 is refused, as the reference refuses it.  Either combines with every
--gt_layer_type; a checkpoint of one normalisation is refused by another.

Out of scope: Performer and BigBird, Graphormer's own encoders, log_attn_weights, edge-feature biases, the local GNN types GCN / GIN / GENConv / GAT, PNA's other
aggregators, degree scalers (pna_degrees) and towers, the EquivStableLapPE gate of GINE and GatedGCN, the other positional
encodings (SignNet, EquivStableLapPE, HKdiagSE, ElstaticSE), graphgym's config system and wandb, a whole-step engine, and data
parallelism (WORLD_SIZE > 1 is refused).

    python -m esc_gnn_amd.run_zinc_gps --h 3 --epochs 2000 --posenc_LapPE 1
"""
import os

import torch

from . import ops
from .gps_models import GPSModel
from .harness import Context, default_appendix, fit_regression, open_result_dir, parser_from, seed_everything, sharded_batches, sharded_ids

_FLAGS = [  # defaults: GraphGPS/configs/GPS/zinc-GPS.yaml (gt.*, train.batch_size, optim.*, dataset.*_num_types)
    ("--layers", dict(type=int, default=10)),
    ("--n_heads", dict(type=int, default=4)),
    ("--dim_hidden", dict(type=int, default=64)),
    ("--dropout", dict(type=float, default=0.0)),
    ("--attn_dropout", dict(type=float, default=0.5)),
    ("--batch_size", dict(type=int, default=32)),
    ("--lr", dict(type=float, default=1e-3)),
    ("--weight_decay", dict(type=float, default=1e-5)),
    ("--epochs", dict(type=int, default=2000)),
    ("--num_warmup_epochs", dict(type=int, default=50)),
    ("--clip_grad_norm", dict(type=int, default=1, help="1: clip the gradient norm (optim.clip_grad_norm: True), 0: do not")),
    ("--clip_grad_norm_value", dict(type=float, default=1.0, help="the largest norm (graphgps/config/optimizers_config.py)")),
    ("--node_encoder_num_types", dict(type=int, default=28)),
    ("--edge_encoder_num_types", dict(type=int, default=4)),
    ("--h", dict(type=int, default=3)),
    ("--seed", dict(type=int, default=0)),
    ("--save_appendix", dict(default="")),
    ("--load_model", dict(default=None)),
    ("--eval", dict(default=0, type=int)),
    ("--synthetic_graphs", dict(type=int, default=12000, help="train+val+test molecules (10:1:1 like ZINC-12k)")),
    ("--gt_layer_type", dict(default="GINE+Transformer", help="gt.layer_type, <local GNN>+<global model>: " + ", ".join(
        ("GINE+Transformer", "CustomGatedGCN+Transformer", "GINE+None", "CustomGatedGCN+None", "PNA+Transformer", "PNA+None",
         "GINE+BiasedTransformer", "CustomGatedGCN+BiasedTransformer", "PNA+BiasedTransformer")))),
    ("--gt_layer_norm", dict(type=int, default=0, choices=(0, 1), help="gt.layer_norm: 1: per-graph LayerNorm as the layers' three norms "
                                                                       "(with --gt_batch_norm 0)")),
    ("--gt_batch_norm", dict(type=int, default=1, choices=(0, 1), help="gt.batch_norm: 1: BatchNorm as the layers' three norms (the yaml's)")),
    ("--posenc_LapPE", dict(type=int, default=0, help="1: node encoder TypeDictNode+LapPE (the reference yaml), 0: TypeDictNode")),
    ("--posenc_LapPE_max_freqs", dict(type=int, default=8, help="posenc_LapPE.eigen.max_freqs")),
    ("--posenc_LapPE_dim_pe", dict(type=int, default=8, help="posenc_LapPE.dim_pe (model DeepSet, layers 2)")),
    # the reference ships no yaml that enables RWSE: these defaults are upstream GraphGPS's usual ZINC values, this project's choice
    ("--posenc_RWSE", dict(type=int, default=0, choices=(0, 1), help="1: add the random-walk structural encoding to the node encoder "
                                                                      "(TypeDictNode+RWSE, with --posenc_LapPE 1 TypeDictNode+LapPE+RWSE)")),
    ("--posenc_RWSE_ksteps", dict(type=int, default=20, help="posenc_RWSE.kernel.times = range(1, ksteps + 1); default: upstream "
                                                             "GraphGPS's usual ZINC value, not a file of the reference")),
    ("--posenc_RWSE_dim_pe", dict(type=int, default=28, help="posenc_RWSE.dim_pe (default: upstream GraphGPS's usual ZINC value)")),
    ("--posenc_RWSE_model", dict(default="linear", help="posenc_RWSE.model: linear or mlp (default: upstream's usual ZINC value)")),
    ("--posenc_RWSE_layers", dict(type=int, default=1, help="posenc_RWSE.layers, for model mlp")),
    ("--posenc_RWSE_raw_norm_type", dict(default="BatchNorm", help="posenc_RWSE.raw_norm_type: BatchNorm or none")),
]


LAYER_TYPES = ("GINE+Transformer", "CustomGatedGCN+Transformer", "GINE+None", "CustomGatedGCN+None", "PNA+Transformer", "PNA+None")
BIASED_LAYER_TYPES = ("GINE+BiasedTransformer", "CustomGatedGCN+BiasedTransformer", "PNA+BiasedTransformer")    # + the shortest-path bias


def build_parser():
    return parser_from(_FLAGS, "ESC-GNN inside a GraphGPS transformer for ZINC graphs (MI355X hot path).")


def layer_type_of(name):
    """gt.layer_type -> (local_gnn_type, global_model_type), split at '+' as graphgps/network/gps_model.py:72-76 does"""
    if name not in LAYER_TYPES + BIASED_LAYER_TYPES:
        raise SystemExit("run_zinc_gps: --gt_layer_type %r is not supported; accepted: %s" % (name, ", ".join(LAYER_TYPES + BIASED_LAYER_TYPES)))
    local_gnn_type, global_model_type = name.split("+")
    return local_gnn_type, global_model_type


def norm_flags_of(args):
    """(gt.layer_norm, gt.batch_norm); the two together are refused before anything is built (gps_layer.py:139-140)"""
    if args.gt_layer_norm and args.gt_batch_norm:
        raise SystemExit("run_zinc_gps: --gt_layer_norm 1 and --gt_batch_norm 1 cannot be applied together: "
                         "pass --gt_batch_norm 0 with --gt_layer_norm 1")
    return bool(args.gt_layer_norm), bool(args.gt_batch_norm)


def _load_splits(args):
    from .datasets import build_feature_dataset, synthetic_zinc_graphs
    G = args.synthetic_graphs
    done = build_feature_dataset(synthetic_zinc_graphs(0, G), args.h, use_rd=True, self_loop=True)     # master_loader.py:32-33
    n_tr, n_va = (G * 10) // 12, G // 12
    return done[:n_tr], done[n_tr:n_tr + n_va], done[n_tr + n_va:]


def main(argv=None):
    import time

    from .optim import CosineWithWarmup, FlatAdam
    from .store import DeviceGraphStore

    args = build_parser().parse_args(argv)
    local_gnn_type, global_model_type = layer_type_of(args.gt_layer_type)
    norm_flags_of(args)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("run_zinc_gps: data parallelism is out of scope for the graph transformer (WORLD_SIZE must be 1)")
    ctx = Context()
    seed_everything(args.seed)
    args.save_appendix = default_appendix(args.save_appendix)
    args.res_dir = "results/zinc_GPS" + args.save_appendix
    cmd_input = open_result_dir(ctx, args.res_dir, ("run_zinc_gps.py", "gps_models.py"))

    t11 = time.time()
    tr, va, te = _load_splits(args)
    ctx.say("Preprocessing time cost: {}s,".format(time.time() - t11))
    stores = [DeviceGraphStore(part, ctx.device) for part in (tr, va, te)]
    widest = [int((s.h_node_ptr[1:] - s.h_node_ptr[:-1]).max()) for s in stores]      # the largest graph of each store: host data
    n_train = len(tr)
    tables = [[] for _ in stores]                   # the resident encoding tables of every split, attached to each of its batches in order

    def lap_pe_limits():
        limit = ops.laplacian_eig_limits()[0]
        if max(widest) > limit:
            raise SystemExit("run_zinc_gps: the largest graph has %d nodes, the Laplacian eigen-solver takes at most %d" % (max(widest), limit))

    def rwse_limits():
        node_limit, edge_limit = ops.rw_landing_limits()
        most_edges = max(int((s.h_edge_ptr[1:] - s.h_edge_ptr[:-1]).max()) for s in stores)
        if max(widest) > node_limit or most_edges > edge_limit:
            raise SystemExit("run_zinc_gps: the largest graph has %d nodes and %d edges, the random-walk kernel takes at most %d nodes "
                             "and %d edges per graph" % (max(widest), most_edges, node_limit, edge_limit))
        if not 1 <= args.posenc_RWSE_ksteps <= 63:
            raise SystemExit("run_zinc_gps: --posenc_RWSE_ksteps %d outside 1..63" % args.posenc_RWSE_ksteps)

    def spd_limits():
        head_dim = args.dim_hidden // args.n_heads
        node_limit, attn_limit = ops.graph_spd_limits()[0], ops.attention_bias_max_nodes(head_dim)
        if max(widest) > min(node_limit, attn_limit):
            raise SystemExit("run_zinc_gps: the largest graph has %d nodes, the shortest-path kernel takes at most %d nodes per graph and "
                             "the biased attention kernels at most %d at head_dim %d" % (max(widest), node_limit, attn_limit, head_dim))

    from .lappe import LapPETable
    from .rwse import RWSETable
    from .spd import SPDTable
    for name, on, cls, what, check in (("LapPE", args.posenc_LapPE, LapPETable, (args.posenc_LapPE_max_freqs,), lap_pe_limits),
                                       ("RWSE", args.posenc_RWSE, RWSETable, (list(range(1, args.posenc_RWSE_ksteps + 1)),), rwse_limits),
                                       ("SPD", global_model_type == "BiasedTransformer", SPDTable, (), spd_limits)):
        if not on:
            continue
        check()
        t12 = time.time()
        for t, s in zip(tables, stores):
            t.append(cls(s, *what))
        torch.cuda.synchronize()
        ctx.say("{} table build time cost: {}s,".format(name, time.time() - t12))

    model = GPSModel(layers=args.layers, dim_hidden=args.dim_hidden, n_heads=args.n_heads, dropout=args.dropout,
                     attn_dropout=args.attn_dropout, node_types=args.node_encoder_num_types, edge_types=args.edge_encoder_num_types,
                     lap_pe=bool(args.posenc_LapPE), dim_pe=args.posenc_LapPE_dim_pe, max_freqs=args.posenc_LapPE_max_freqs,
                     rwse=bool(args.posenc_RWSE), rwse_dim_pe=args.posenc_RWSE_dim_pe, rwse_steps=args.posenc_RWSE_ksteps,
                     rwse_model=args.posenc_RWSE_model, rwse_layers=args.posenc_RWSE_layers, rwse_raw_norm=args.posenc_RWSE_raw_norm_type,
                     local_gnn_type=local_gnn_type, global_model_type=global_model_type, layer_norm=bool(args.gt_layer_norm),
                     batch_norm=bool(args.gt_batch_norm))
    limit = ops.attention_max_nodes(args.dim_hidden // args.n_heads)
    if global_model_type != "None" and max(widest) > limit:
        raise SystemExit("run_zinc_gps: the largest graph has %d nodes, the attention kernels take at most %d at head_dim %d"
                         % (max(widest), limit, args.dim_hidden // args.n_heads))
    if args.load_model is not None:
        model.load_state_dict(torch.load(args.load_model, map_location="cpu"))
    ctx.say("Using " + model.__class__.__name__ + " model")
    model = model.to(ctx.device)
    optimizer = FlatAdam(model.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    scheduler = CosineWithWarmup(optimizer, args.num_warmup_epochs, args.epochs)
    gen = torch.Generator().manual_seed(args.seed)

    def batches(which, shuffle):
        if not tables[which]:
            for data, _ in sharded_batches(stores[which], args.batch_size, ctx, shuffle, gen if shuffle else None):
                data._esc_max_nodes = widest[which]        # an upper bound of this batch's largest graph, known without a read-back
                yield data
            return
        for ids, _ in sharded_ids(stores[which], args.batch_size, ctx, shuffle, gen if shuffle else None):
            data = stores[which].collate(ids)              # sharded_batches' collate, plus the batch's PE rows
            for table in tables[which]:
                table.attach(data, ids)
            data._esc_max_nodes = widest[which]
            yield data

    def train(epoch):
        model.train()
        loss_all = torch.zeros((), device=ctx.device)
        for data in batches(0, True):
            optimizer.zero_grad()
            y = data.y.view(-1, 1)
            loss = ops.l1_loss(model(data), y)             # graphgps/loss/l1.py
            loss.backward()
            loss_all += loss.detach() * y.size(0)
            optimizer.step(grad_denom=optimizer.clip_scale(args.clip_grad_norm_value) if args.clip_grad_norm else None)
        return float(loss_all) / n_train

    def test(store):
        which = next(i for i, s in enumerate(stores) if s is store)
        model.eval()
        tot = torch.zeros(2, device=ctx.device)
        with torch.no_grad():
            for data in batches(which, False):
                y_hat = model(data)[:, 0]
                tot[0] += torch.sum(torch.abs(y_hat - data.y.view(-1)))
                tot[1] += y_hat.numel()
        return float(tot[0] / tot[1])

    if args.eval:
        print("Test MAE: %.7f" % test(stores[2]))
        ctx.close()
        return
    fit_regression(ctx, args, model, optimizer, scheduler, train, test, stores[1], stores[2], 1.0, cmd_input)
    ctx.close()


if __name__ == "__main__":
    main()
