"""CSL expressiveness run on the ESC hot path — the MI355X-native twin of the reference's run_csl.py: 150 circular-skip-link
graphs (41 nodes, 10 skip lengths = 10 classes of 15 relabelled copies, all 4-regular and 1-WL-equivalent), ESC features
with h = 4 and resistance distance, the stratified 10-fold protocol of kernel/train_eval.py:225-240 (datasets.csl_k_fold), a
NestedGIN (csl_models) reset for every split, Adam + ReduceLROnPlateau(factor 0.7, patience 5, min_lr = lr), batches of 64,
cross-entropy on raw logits.  Flags and defaults are the reference's (:26-35); `--seed`, `--splits` (how many of the ten
folds to run), `--copies` (graphs per class) and `--data_seed` (the relabelling permutations) are additions.

The dataset is generated (datasets.csl_graphs), not read from the benchmark's downloaded pickle: CSL is a defined graph
family, so the classes are the reference's while the relabellings are this project's.  The training head is one launch
(ops.log_softmax_nll: cross-entropy, accuracy count and the gradient of the logits); every batch is collated on the device
from an HBM-resident store (DataLoader).  Nothing is written to a log file.

    python -m esc_gnn_amd.run_csl
"""
import torch

from . import ops
from .harness import (Context, classify_test, classify_train, labels_of, parser_from, print_final_result,
                      seed_everything)

_FLAGS = [  # same names, types and defaults as the reference CLI
    ("--model", dict(type=str, default="GIN")),
    ("--h", dict(type=int, default=4, help="largest height of rooted subgraphs to simulate")),
    ("--layers", dict(type=int, default=5)),
    ("--width", dict(type=int, default=128)),
    ("--epochs", dict(type=int, default=500)),
    ("--dataset", dict(type=str, default="CSL")),
    ("--learnRate", dict(type=float, default=1E-3)),
    # additions (not in the reference)
    ("--seed", dict(type=int, default=None, help="seed torch before the model is built (default: unseeded, as the reference)")),
    ("--splits", dict(type=int, default=10, help="run the first SPLITS of the ten folds")),
    ("--copies", dict(type=int, default=15, help="graphs per class (the benchmark has 15)")),
    ("--data_seed", dict(type=int, default=0, help="seed of the relabelling permutations")),
]
BATCH = 64
FOLDS = 10
EPOCH_LINE = ("Epoch: {:03d}, LR: {:7f}, Train Loss: {:.7f}, Val Loss: {:.7f}, Val Acc: {:.7f}, Test Loss: {:.7f}, "
              "Test Acc: {:.7f}, Train Acc: {:.7f}")


def build_parser():
    return parser_from(_FLAGS, "Nested GNN for CSL datasets (MI355X hot path).")


def main(argv=None):
    from .csl_models import NestedGIN
    from .dataloader import DataLoader
    from .datasets import build_csl_dataset, csl_graphs, csl_k_fold
    from .optim import FlatAdam, ReduceLROnPlateau

    args = build_parser().parse_args(argv)
    if args.model != "GIN":
        raise NotImplementedError("model type not supported")       # reference :229-232
    if args.dataset != "CSL":
        raise SystemExit("run_csl: --dataset %s: only CSL is generated here" % args.dataset)
    if not 1 <= args.splits <= FOLDS:
        raise SystemExit("run_csl: --splits must lie in 1..%d" % FOLDS)
    if args.copies < FOLDS:
        raise SystemExit("run_csl: the %d-fold protocol needs --copies >= %d" % (FOLDS, FOLDS))
    ctx = Context()
    if args.seed is not None:
        seed_everything(args.seed)
    dataset = build_csl_dataset(csl_graphs(copies=args.copies, seed=args.data_seed), args.h)
    device = ctx.device
    model = NestedGIN(args.layers, args.width).to(device)

    def val(loader):
        model.eval()
        total_loss = 0
        with torch.no_grad():
            for data in loader:
                num_graphs = data.num_graphs
                data = data.to(device)
                total_loss += ops.log_softmax_nll(model.logits(data), labels_of(data)).item() * num_graphs
        return total_loss / len(loader.dataset)

    acc, tr_acc = [], []
    folds = csl_k_fold([int(d.y) for d in dataset], FOLDS)
    for i, (train_idx, test_idx, val_idx) in enumerate(zip(*folds)):
        if i >= args.splits:
            break
        model.reset_parameters()
        optimizer = FlatAdam(model.parameters(), lr=args.learnRate)
        scheduler = ReduceLROnPlateau(optimizer, mode="min", factor=0.7, patience=5, min_lr=args.learnRate)
        val_loader = DataLoader([dataset[j] for j in val_idx], batch_size=BATCH)
        test_loader = DataLoader([dataset[j] for j in test_idx], batch_size=BATCH)
        train_loader = DataLoader([dataset[j] for j in train_idx], batch_size=BATCH, shuffle=True)
        print("---------------- Split {} ----------------".format(i))
        best_val_loss, test_acc, train_acc = 100, 0, 0
        for epoch in range(args.epochs):
            lr = optimizer.param_groups[0]["lr"]
            train_loss = classify_train(model, train_loader, optimizer, device)     # F.cross_entropy(out, y)
            val_loss = val(val_loader)
            scheduler.step(val_loss)
            if best_val_loss >= val_loss:
                best_val_loss = val_loss
            train_acc = classify_test(model, train_loader, device)
            val_acc = classify_test(model, val_loader, device)
            test_loss = val(test_loader)
            test_acc = classify_test(model, test_loader, device)
            print(EPOCH_LINE.format(epoch + 1, lr, train_loss, val_loss, val_acc, test_loss, test_acc, train_acc))
        acc.append(test_acc)
        tr_acc.append(train_acc)
    print_final_result(acc, tr_acc)
    ctx.close()


if __name__ == "__main__":
    main()
