"""Pieces shared by the training drivers (run_*.py): the argument parser, device + process-group set-up, seeding, result
directory bookkeeping, graph-sharded batch iteration (rank r takes a contiguous slice of every global batch;
the only collective of a step is the weighted all-reduce of the flat gradient bucket), the epoch loop of the regression
drivers and the passes of the classification drivers.  No driver imports from another driver."""
import argparse
import os
import random
import shutil
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .parallel import shard_slice

BATCH = 20       # graphs per batch of the expressiveness runs (reference run_sr.py:236, run_exp.py:296-300)


def parser_from(flags, description):
    """argparse parser of a driver's _FLAGS: (name, add_argument keywords) pairs"""
    ap = argparse.ArgumentParser(description=description)
    for name, kw in flags:
        ap.add_argument(name, **kw)
    return ap


class Context(object):
    def __init__(self):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        if not torch.cuda.is_available():
            raise RuntimeError("needs a HIP device (the hot path has no CPU fallback)")
        local %= torch.cuda.device_count()
        torch.cuda.set_device(local)
        self.device = torch.device("cuda", local)
        if self.world > 1 and not dist.is_initialized():
            backend = os.environ.get("ESC_DIST_BACKEND", "nccl")      # gloo only to rehearse N>1 on one GPU
            dist.init_process_group(backend, **({"device_id": self.device} if backend == "nccl" else {}))

    def say(self, *a, **kw):
        if self.rank == 0:
            print(*a, **kw)

    def all_reduce(self, t):
        if self.world > 1:
            dist.all_reduce(t)
        return t

    def close(self):
        if self.world > 1 and dist.is_initialized():
            dist.destroy_process_group()


def seed_everything(seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    random.seed(seed)
    np.random.seed(seed)


def open_result_dir(ctx, res_dir, sources):
    """results/<...> with the driver sources and the command line saved next to the logs (reference drivers do the
    same, e.g. run_zinc.py:100-113)."""
    cmd_input = "python " + " ".join(sys.argv) + "\n"
    if ctx.rank == 0:
        print("Results will be saved in " + res_dir)
        os.makedirs(res_dir, exist_ok=True)
        here = os.path.dirname(os.path.abspath(__file__))
        for f in sources:
            shutil.copy(os.path.join(here, f), res_dir)
        with open(os.path.join(res_dir, "cmd_input.txt"), "a") as fh:
            fh.write(cmd_input)
        print("Command line input: " + cmd_input + " is saved.")
    return cmd_input


def default_appendix(appendix):
    return appendix if appendix != "" else "_" + time.strftime("%Y%m%d%H%M%S")


def sharded_ids(store, batch_size, ctx, shuffle, generator=None):
    """(this rank's graph ids, size of the global batch) for every global batch of `batch_size` graphs in loader order:
    rank r takes a contiguous slice.  Only len(store) is read; nothing touches the device."""
    G = len(store)
    if shuffle and ctx.world > 1 and generator is None:
        # the global CPU RNG would give every rank the same permutation only while all ranks consume it identically;
        # any rank-dependent draw would silently shard DIFFERENT orders (graphs duplicated / dropped, no error anywhere)
        raise ValueError("sharded_batches(shuffle=True) on %d ranks needs a dedicated, identically seeded torch.Generator" % ctx.world)
    order = torch.randperm(G, generator=generator) if shuffle else torch.arange(G)
    for i in range(0, G, batch_size):
        ids = order[i:i + batch_size]
        if ids.numel() < ctx.world:
            # a remainder smaller than the rank count would leave some ranks without data while the others enter the
            # step's collectives: training drops it (every rank alike), evaluation hands it to rank 0
            if shuffle or ctx.rank != 0:
                continue
            yield ids, ids.numel()
            continue
        lo, hi = shard_slice(ids.numel(), ctx.rank, ctx.world)
        yield ids[lo:hi], ids.numel()


def sharded_batches(store, batch_size, ctx, shuffle, generator=None):
    """Global batches of `batch_size` graphs in loader order; this rank collates its contiguous share."""
    for ids, n_global in sharded_ids(store, batch_size, ctx, shuffle, generator):
        yield store.collate(ids), n_global


def expanded_batches(store, batches, *extra):
    """The device-expanding baselines (NGNN, I2GNN, GINE+): every plain batch of `batches` through `store.expand(data, *extra)`
    (expansion.GraphStore), on the device"""
    for data, n_global in batches:
        yield store.expand(data, *extra), n_global


_prefetch_streams = {}


def prefetched(batches, device, warm=None):
    """Iterates `batches` (a generator that collates device batches: sharded_batches, DeviceLoader) ONE ITEM AHEAD on a
    side HIP stream: batch i+1 is collated — and `warm(item)` builds whatever per-batch index plans the step engine will
    ask for — while the caller trains on batch i.  This is the role of the reference's DataLoader worker processes
    (run_ogb_mol.py:229-234, num_workers) with the dataset resident in HBM: the ~60 small gather / counting-sort launches
    of a molecule batch leave the step's critical path.
    Ordering: the side stream first waits for everything the caller's stream has been given so far (all of step i-1), so
    the caching allocator may hand it the blocks of batches that are already dropped; the caller's stream waits for the
    side stream's event before it touches the batch.  Tensors live in the side stream's pool but are only ever reused
    behind such a wait."""
    device = torch.device(device)
    if device.type != "cuda":
        for item in batches:
            if warm is not None:
                warm(item)
            yield item
        return
    side = _prefetch_streams.get(device)
    if side is None:
        side = _prefetch_streams[device] = torch.cuda.Stream(device)
    it = iter(batches)

    def issue():
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            try:
                item = next(it)
            except StopIteration:
                return None
            if warm is not None:
                warm(item)
            ready = torch.cuda.Event()
            ready.record(side)
        return item, ready

    ahead = issue()
    while ahead is not None:
        item, ready = ahead
        torch.cuda.current_stream(device).wait_event(ready)
        ahead = issue()                                    # queued BEFORE the caller enqueues step i: overlaps it
        yield item


EPOCH_LINE = "Epoch: {:03d}, LR: {:7f}, Loss: {:.7f}, Validation MAE: {:.7f}, Test MAE: {:.7f}, Test MAE norm: {:.7f}"


def fit_regression(ctx, args, model, optimizer, scheduler, train, test, val_store, test_store, std, cmd_input, timed=True):
    """Epoch loop of the MAE regression drivers (reference run_zinc.py:309-339, run_graphcount.py:585-613): train, validate,
    step the plateau scheduler, test when validation improves or at the 10th epoch since the last test, append the line to
    log.txt, checkpoint after the last epoch and print the closing lines.  `timed`: with "Training time cost".  Returns
    the last log line."""
    t1 = time.time()
    best_val_error, count, log = None, 0, ""
    for epoch in range(1, args.epochs + 1):
        lr = optimizer.param_groups[0]["lr"]
        loss = train(epoch)
        val_error = test(val_store)
        scheduler.step(val_error)
        count += 1
        if best_val_error is None:
            best_val_error = val_error
        if val_error <= best_val_error or count == 10:
            count = 0
            test_error = test(test_store)
            best_val_error = val_error
            log = EPOCH_LINE.format(epoch, lr, loss, val_error, test_error, test_error / float(std))
            if ctx.rank == 0:
                print("\n" + log + "\n")
                with open(os.path.join(args.res_dir, "log.txt"), "a") as fh:
                    fh.write(log + "\n")
    if ctx.rank == 0:
        torch.save(model.state_dict(), os.path.join(args.res_dir, "model_checkpoint{}.pth".format(args.epochs)))
        if timed:
            print("Training time cost: {}s".format(time.time() - t1))
        print(cmd_input[:-1])
        print(log)
    return log


# ---- classification runs (run_exp / run_csl; run_sr for find_data_file and the batch size) ----------------------------
def find_data_file(root, names):
    """`root` itself when it is a file, else the first of root/<name>, root/raw/<name> that exists; None otherwise"""
    if os.path.isfile(root):
        return root
    for name in names:
        for p in (os.path.join(root, name), os.path.join(root, "raw", name)):
            if os.path.isfile(p):
                return p
    return None


def labels_of(data):
    """int64 class labels of a batch.  The device store keeps y as float32; 0 / 1 survive that exactly — checked."""
    y = data.y.view(-1)
    if y.dtype == torch.int64:
        return y
    yl = y.long()
    assert torch.equal(yl.to(y.dtype), y), "graph labels are not integers"
    return yl


def classify_train(model, loader, optimizer, device):
    """one epoch of F.nll_loss(log_softmax(logits), y) / F.cross_entropy(logits, y) -> mean loss per graph"""
    model.train()
    loss_all = 0
    for data in loader:
        optimizer.zero_grad()
        data = data.to(device)
        loss = ops.log_softmax_nll(model.logits(data), labels_of(data))
        loss.backward()
        loss_all += data.num_graphs * loss.item()
        optimizer.step()
    return loss_all / len(loader.dataset)


def classify_test(model, loader, device):
    """accuracy over the loader's graphs; the correct predictions are counted by the loss launch"""
    model.eval()
    correct = 0
    with torch.no_grad():
        for data in loader:
            data = data.to(device)
            correct += ops.log_softmax_nll(model.logits(data), labels_of(data), return_aux=True)[2]
    return correct / len(loader.dataset)


def print_final_result(acc, tr_acc):
    """mean and standard deviation over the splits of the test and the train accuracy"""
    acc, tr_acc = torch.tensor(acc, dtype=torch.float64), torch.tensor(tr_acc, dtype=torch.float64)
    std = (lambda t: float(t.std()) if t.numel() > 1 else float("nan"))
    print("---------------- Final Result ----------------")
    print("Mean: {:7f}, Std: {:7f}".format(float(acc.mean()), std(acc)))
    print("Tr Mean: {:7f}, Std: {:7f}".format(float(tr_acc.mean()), std(tr_acc)))
