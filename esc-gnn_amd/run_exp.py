"""EXP / CEXP expressiveness run on the ESC hot path — the MI355X-native twin of the reference's run_exp.py: 1 200 planar
SAT graphs in 600 non-isomorphic, 1-WL-equivalent pairs with opposite labels, 10-fold protocol of :276-342 (fold i tests
on the i-th tenth, split into the `Lrn` (index % 4 <= 1) and `Exp` halves, validates on the i-th tenth of the rest), a
freshly initialised NestedGIN (expressive_models) per fold, Adam + ReduceLROnPlateau(factor 0.7, patience 5,
min_lr = lr), batches of 20.  Flags and defaults are the reference's (:24-33); `--data_root`, `--seed`, `--splits` (how
many of the ten folds to run) and `--limit` (read only the first graphs of the file) are additions.

The training head is one launch (ops.log_softmax_nll: log-softmax, NLL loss, accuracy count and the gradient of the
logits); every batch is collated on the device from an HBM-resident store (DataLoader).  The text file GRAPHSAT.txt
(CEXP.txt for `--dataset CEXP`) is not part of this repository: put it under --data_root.

    python -m esc_gnn_amd.run_exp --data_root data/EXP
"""
import torch

from . import ops
from .harness import (BATCH, Context, classify_test, classify_train, find_data_file, labels_of, parser_from,
                      print_final_result, seed_everything)

_FLAGS = [  # same names, types and defaults as the reference CLI
    ("--model", dict(type=str, default="GIN")),
    ("--h", dict(type=int, default=3, help="largest height of rooted subgraphs to simulate")),
    ("--layers", dict(type=int, default=8)),
    ("--width", dict(type=int, default=64)),
    ("--epochs", dict(type=int, default=500)),
    ("--dataset", dict(type=str, default="EXP")),
    ("--learnRate", dict(type=float, default=0.001)),
    # additions (not in the reference)
    ("--data_root", dict(type=str, default=None, help="directory that holds GRAPHSAT.txt / CEXP.txt, or the file itself "
                                                       "(default: data/<dataset>)")),
    ("--seed", dict(type=int, default=None, help="seed torch before the model is built (default: unseeded, as the reference)")),
    ("--splits", dict(type=int, default=10, help="run the first SPLITS of the ten folds")),
    ("--limit", dict(type=int, default=None, help="read only the first LIMIT graphs of the file")),
]
FOLDS = 10
EPOCH_LINE = ("Epoch: {:03d}, LR: {:7f}, Train Loss: {:.7f}, Val Loss: {:.7f}, Test Acc: {:.7f}, Exp Acc: {:.7f}, "
              "Lrn Acc: {:.7f}, Train Acc: {:.7f}")


def build_parser():
    return parser_from(_FLAGS, "Nested GNN for EXP/CEXP datasets (MI355X hot path).")


def main(argv=None):
    from .dataloader import DataLoader
    from .datasets import build_expressive_dataset, exp_split, load_exp_txt
    from .expressive_models import NestedGIN
    from .optim import FlatAdam, ReduceLROnPlateau

    args = build_parser().parse_args(argv)
    if args.model != "GIN":
        raise NotImplementedError("model type not supported")       # reference :222-225
    root = args.data_root if args.data_root is not None else "data/" + args.dataset
    name = "GRAPHSAT.txt" if args.dataset == "EXP" else args.dataset + ".txt"
    path = find_data_file(root, (name,))
    if path is None:
        raise SystemExit("run_exp: no %s under %s (the reference ships it as data/EXP/%s; supply it with --data_root)"
                         % (name, root, name))
    if not 1 <= args.splits <= FOLDS:
        raise SystemExit("run_exp: --splits must lie in 1..%d" % FOLDS)
    ctx = Context()
    if args.seed is not None:
        seed_everything(args.seed)
    dataset = build_expressive_dataset(load_exp_txt(path, args.limit), args.h)
    device = ctx.device
    model = NestedGIN(dataset[0].num_features, args.layers, args.width).to(device)

    def val(loader):
        model.eval()
        loss_all = 0
        with torch.no_grad():
            for data in loader:
                data = data.to(device)
                loss_all += ops.log_softmax_nll(model.logits(data), labels_of(data), reduction="sum").item()
        return loss_all / len(loader.dataset)

    acc, tr_acc = [], []
    for i in range(args.splits):
        model.reset_parameters()
        optimizer = FlatAdam(model.parameters(), lr=args.learnRate)
        scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=0.7, patience=5, min_lr=args.learnRate)
        parts = exp_split(len(dataset), i, FOLDS)
        if not parts["train"] or not parts["val"] or not parts["test"]:
            raise SystemExit("run_exp: %d graphs are too few for the %d-fold protocol" % (len(dataset), FOLDS))
        sub = {k: [dataset[j] for j in v] for k, v in parts.items()}
        val_loader = DataLoader(sub["val"], batch_size=BATCH)
        test_loader = DataLoader(sub["test"], batch_size=BATCH)
        test_exp_loader = DataLoader(sub["exp"], batch_size=BATCH)
        test_lrn_loader = DataLoader(sub["lrn"], batch_size=BATCH)
        train_loader = DataLoader(sub["train"], batch_size=BATCH, shuffle=True)
        print("---------------- Split {} ----------------".format(i))
        best_val_loss, test_acc, train_acc = 100, 0, 0
        for epoch in range(args.epochs):
            lr = optimizer.param_groups[0]["lr"]
            train_loss = classify_train(model, train_loader, optimizer, device)     # F.nll_loss(model(data), data.y)
            val_loss = val(val_loader)
            scheduler.step(val_loss)
            if best_val_loss >= val_loss:
                best_val_loss = val_loss
            train_acc = classify_test(model, train_loader, device)
            test_acc = classify_test(model, test_loader, device)
            test_exp_acc = classify_test(model, test_exp_loader, device) if sub["exp"] else float("nan")
            test_lrn_acc = classify_test(model, test_lrn_loader, device) if sub["lrn"] else float("nan")
            print(EPOCH_LINE.format(epoch + 1, lr, train_loss, val_loss, test_acc, test_exp_acc, test_lrn_acc, train_acc))
        acc.append(test_acc)
        tr_acc.append(train_acc)
    print_final_result(acc, tr_acc)
    ctx.close()


if __name__ == "__main__":
    main()
