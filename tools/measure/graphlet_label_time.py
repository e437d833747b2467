"""Graphlet labels of the synthetic counting dataset: host-to-host time of graphlets.graphlet_orbit_counts for the first
`--graphs` count-shaped graphs (copies included, median of 5 after one warm-up call), and the networkx oracle
(tests/graphlet_oracle.py) on the first `--oracle_graphs` of them on a pool of host processes.  One JSON line.

    python tools/measure/graphlet_label_time.py [--graphs 5000] [--oracle_graphs 320] [--procs 16]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _oracle(item):
    import graphlet_oracle as go
    n, ei = item
    return go.orbit_labels(n, ei)


def main():
    from multiprocessing import get_context
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=5000)
    ap.add_argument("--oracle_graphs", type=int, default=320)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    from esc_gnn_amd.datasets import synthetic_count_graphs
    from esc_gnn_amd.graphlets import graphlet_orbit_counts
    data = synthetic_count_graphs(0, args.graphs)
    graphlet_orbit_counts(data[:64])                              # warm-up: code object load, allocator
    torch.cuda.synchronize()
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        got = graphlet_orbit_counts(data)                         # host Data in, host tensors out
        reps.append((time.perf_counter() - t0) * 1e3)
    k = min(args.oracle_graphs, args.graphs)
    items = [(int(d.x.size(0)), d.edge_index.numpy()) for d in data[:k]]
    t0 = time.perf_counter()
    with get_context("spawn").Pool(args.procs) as pool:
        want = pool.map(_oracle, items, chunksize=4)
    nx_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    print(json.dumps(dict(what="graphlet_labels", graphs=args.graphs, nodes=int(sum(d.x.size(0) for d in data)),
                          device_ms_median=round(float(np.median(reps)), 3), device_ms_all=[round(r, 3) for r in reps],
                          oracle_graphs=k, oracle_ms=round(nx_ms, 1), oracle_procs=args.procs, identical=same)), flush=True)


if __name__ == "__main__":
    main()
