"""SR25 expressiveness run on the ESC hot path — the MI355X-native twin of the reference's run_sr.py: the 15 strongly
regular graphs srg(25, 12, 5, 6) of data/sr25/raw/sr251256.g6 go through an UNTRAINED NestedGIN (expressive_models) in
eval mode, and two graphs count as told apart when their outputs differ by at least 1e-2 in L2 (run_sr.py:232-250).
Flags and defaults are the reference's (:25-34); `--data_root` and `--seed` are additions.  Features (h-hop ESC
encodings, `use_rd=False, self_loop=True`, :76-78) are built by the HIP feature builder, the forward runs through
libescgnn_hip.so, and the pairwise distances and the below-threshold count are one esc_pdist launch.

    python -m esc_gnn_amd.run_sr --data_root data/sr25
"""
import torch

from . import ops
from .harness import BATCH, Context, find_data_file, parser_from, seed_everything

_FLAGS = [  # same names, types and defaults as the reference CLI
    ("--model", dict(type=str, default="GIN")),
    ("--h", dict(type=int, default=3, help="largest height of rooted subgraphs to simulate")),
    ("--layers", dict(type=int, default=8)),
    ("--width", dict(type=int, default=64)),
    ("--epochs", dict(type=int, default=500)),
    ("--dataset", dict(type=str, default="EXP")),
    ("--learnRate", dict(type=float, default=0.001)),
    # additions (not in the reference)
    ("--data_root", dict(type=str, default="data/sr25", help="directory that holds raw/sr251256.g6 (or the file itself)")),
    ("--seed", dict(type=int, default=None, help="seed torch before the model is built (default: unseeded, as the reference)")),
]
THRESHOLD = 1e-2


def build_parser():
    return parser_from(_FLAGS, "Nested GNN on SR25 (MI355X hot path).")


def predictions(model, dataset, device):
    """eval-mode outputs of every graph, in dataset order (run_sr.py:232-240)"""
    from .dataloader import DataLoader
    model.eval()
    out = []
    with torch.no_grad():
        for data in DataLoader(dataset, batch_size=BATCH):      # y = None: the loader collates these on the host
            out.append(model(data.to(device)))
    return torch.cat(out, dim=0)


def main(argv=None):
    from .datasets import build_expressive_dataset, load_sr25
    from .expressive_models import NestedGIN

    args = build_parser().parse_args(argv)
    if args.model != "GIN":
        raise NotImplementedError("model type not supported")       # reference :218-221
    path = find_data_file(args.data_root, ("sr251256.g6",))
    if path is None:
        raise SystemExit("run_sr: no sr251256.g6 under %s (the reference ships it as data/sr25/raw/sr251256.g6)" % args.data_root)
    ctx = Context()
    if args.seed is not None:
        seed_everything(args.seed)
    dataset = build_expressive_dataset(load_sr25(path), args.h)
    model = NestedGIN(dataset[0].num_features, args.layers, args.width)
    model.reset_parameters()
    model = model.to(ctx.device)
    pred = predictions(model, dataset, ctx.device)
    mm, wrong = ops.pdist(pred, THRESHOLD)
    test_score = 1 - (wrong / mm.shape[0])
    print("---------------- Final Result ----------------")
    print("Acc: {}".format(test_score))
    ctx.close()


if __name__ == "__main__":
    main()
