"""Multi-hop batches whose STRUCTURE is the test, for the one-launch GINE+ aggregate (csrc/gineplus.hip) and the MultihopPlan
that feeds it (multihop.py): degree tails around the 4- and 8-pair batches, a 1000-pair hub, the row schedules of the backward
(1 to 512 workgroups, one to three rows per wave), a batch of graphs with one-node and edgeless graphs at both ends, no pair at
all, no distance-1 pair, and operands that sit exactly on the ReLU gate.  Generated deterministically: no fixture file, no
reference project.

A case is a dict: name, num_nodes, pairs (int64 [2, M]), distance (int64 [M]), k (the largest k it is run at, the k its plan is
built for), batch (int64 [N], non-decreasing) and source: "tensors" (the pairs are handed to MultihopPlan.from_tensors in the
order given) or "expand" (graphs = [(n, edge_index)] go through expand_multihop, and pairs / distance are what the numpy BFS of
multihop_oracle says it must return, already in (row, col) order).

The *_loop functions are the SEQUENTIAL specification, the contract the header comment of csrc/gineplus.hip promises: explicit
loops, one separately rounded fp32 operation at a time (numpy float32), over the pairs and distances alone - never a
MultihopPlan.  The CPU test ties them to fp64 and to single-threaded torch.index_add_; the GPU test holds the kernels to them
bit for bit.  d_eps has no bit contract: deps64 is its fp64 value with the sum of the terms' magnitudes, deps_depth the number
of roundings on the longest path of the kernels' fixed summation order.
"""
import functools

import numpy as np
import torch

import graph_cases as gc
import multihop_oracle as mo

FWD_BATCH, BWD_BATCH = 8, 4                  # pairs in flight per wave (GP_FWD_BATCH, GP_BWD_BATCH)
BWD_WAVES, BWD_MAX_BLOCKS = 8, 512           # GP_BWD_WAVES, GP_BWD_MAX_BLOCKS
# b - 1, b, b + 1, 2b - 1, 2b, 2b + 1 for b = 4 and b = 8, with 0 and 1: the degrees the tail clamp distinguishes ...
DEGREES_REQUIRED = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17)
DEGREE_SET = DEGREES_REQUIRED + (2, 6, 12, 24, 25, 33)       # ... and a few more, which bring the case to 19 nodes
ROWS_N = (8, 9, 24, 25, 256, 264, 4096, 4097, 8195)
ROWS_BLOCKS = (1, 2, 3, 4, 32, 33, 512, 512, 512)            # esc_gineplus_bwd_blocks of ROWS_N
ROWS_PER_WAVE = (1, 1, 1, 1, 1, 1, 1, 2, 3)
PATH_NODES = 1000                            # the directed paths of rows_N are graphs of at most this many nodes
SEGMENT_SIZES = (1, 3, 5, 1, 40, 2, 1)
NONE = np.zeros((2, 0), dtype=np.int64)


def _base(name, num_nodes, pairs, distance, k, source, batch=None, graphs=None):
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(2, -1))
    distance = np.ascontiguousarray(np.asarray(distance, dtype=np.int64).reshape(-1))
    batch = np.zeros(num_nodes, dtype=np.int64) if batch is None else np.asarray(batch, dtype=np.int64)
    return dict(name=name, num_nodes=int(num_nodes), pairs=pairs, distance=distance, k=int(k), source=source, batch=batch, graphs=graphs)


def _expanded(name, graphs, k):
    ns, eis = [n for n, _ in graphs], [ei for _, ei in graphs]
    pairs, dist = mo.multihop_batch(ns, eis, k)
    return _base(name, sum(ns), pairs, dist, k, "expand", batch=np.repeat(np.arange(len(ns), dtype=np.int64), ns), graphs=graphs)


def _degrees(name="degrees"):
    # as graph_cases._degrees: nodes 1..n carry the in-degrees of DEGREE_SET in order and the out-degrees rotated by three
    # places, nodes 0 and n + 1 are isolated, and the stubs are paired through two different permutations, so that the pairs of
    # a node are scattered over the input, (row, col) repeats and nothing is symmetric.  Degrees count every pair of the plan,
    # whatever its distance: the batch loops load them all and mask what the call does not use.
    n = len(DEGREE_SET)
    col = np.concatenate([np.full(d, 1 + i, dtype=np.int64) for i, d in enumerate(DEGREE_SET)])
    row = np.concatenate([np.full(d, 1 + (i + 3) % n, dtype=np.int64) for i, d in enumerate(DEGREE_SET)])
    m = len(col)                                             # 187 = 11 * 17
    row, col = row[gc._perm(m, 56, 7)], col[gc._perm(m, 89, 3)]
    idx = np.arange(m, dtype=np.int64)
    dist = 1 + (idx * 3) % 4                                 # 1..4 ...
    dist[idx % 23 == 5] = 5                                  # ... and one class beyond every k of the fused aggregate
    far = 1 + DEGREE_SET.index(4)                            # a node none of whose pairs, in or out, has distance 1
    near = (dist == 1) & ((row == far) | (col == far))
    dist[near] = 2 + idx[near] % 3
    first, repeat = {}, None                                 # the first (row, col) that comes twice: both at distance 1
    for p in range(m):
        key = (int(row[p]), int(col[p]))
        if far in key:
            continue
        if key in first:
            repeat = (first[key], p)
            break
        first[key] = p
    dist[list(repeat)] = 1
    c = _base(name, n + 2, np.stack([row, col]), dist, 4, "tensors")
    c["far"], c["repeat"], c["beyond_k"] = far, repeat, 5
    return c


def _ties():
    # the `degrees` structure; `operands` edits what it draws so that messages and rows sit exactly on the ReLU gate
    c = _degrees("ties")
    row, col = c["pairs"]
    dist = c["distance"]
    d1 = np.flatnonzero(dist == 1)
    by_src = {}
    for p in d1.tolist():
        by_src.setdefault(int(row[p]), []).append(p)
    s0 = min(s for s, ps in by_src.items() if len(ps) >= 2)
    c["negzero_source"] = s0                                 # x_0[s0] = -0.0: with e = +0 the message is +0, with e = -0.0 it is -0
    c["negzero_pairs"] = tuple(by_src[s0][:2])
    c["cancel_pairs"] = tuple(ps[0] for s, ps in sorted(by_src.items()) if s != s0)[:4]      # e[rank] = -x_0[src]: msg = +0
    vals = (0.0, -0.0, -1e-40)                               # +0, -0, a negative subnormal
    dead, used = {}, set()
    for t in (1, 2, 3):                                      # x_t[node] for sources of pairs at distance t + 1
        srcs = [s for s in sorted(set(row[dist == t + 1].tolist())) if s not in used][:3]
        used.update(srcs)
        dead[t] = tuple(zip(srcs, vals))
    c["dead_sources"] = dead
    return c


def _path(n, forward):
    i = np.arange(max(n - 1, 0), dtype=np.int64)
    return np.stack([i, i + 1]) if forward else np.stack([i + 1, i])


def _rows(n):
    # the first path runs from its first node on, the others from their last node down: node 0 and the last nodes of the batch,
    # which are the first and the later rows of the same waves, all have pairs of both distances
    sizes = [PATH_NODES] * (n // PATH_NODES) + ([n % PATH_NODES] if n % PATH_NODES else [])
    return _expanded("rows_%d" % n, [(s, _path(s, g == 0)) for g, s in enumerate(sizes)], 2)


def _forty():
    """40 nodes, 90 directed edges without loops or repeats among nodes 0..35; nodes 36..39 isolated"""
    seen, t = [], 0
    while len(seen) < 90:
        a, b = (t * 5 + t // 36) % 36, (t * 11 + 1) % 36
        if a != b and (a, b) not in seen:
            seen.append((a, b))
        t += 1
    return 40, np.array(seen, dtype=np.int64).T


def _segments():
    five = np.array([[0, 1, 2, 3, 4, 2], [1, 2, 3, 4, 0, 0]], dtype=np.int64)
    graphs = [(1, NONE), (3, NONE), (5, five), (1, NONE), _forty(), (2, np.array([[0, 1], [1, 0]], dtype=np.int64)), (1, NONE)]
    c = _expanded("segments", graphs, 4)
    ptr = np.concatenate([[0], np.cumsum([n for n, _ in graphs])])
    c["node_ranges"] = [(int(ptr[g]), int(ptr[g + 1])) for g in range(len(graphs))]
    rank1 = np.concatenate([[0], np.cumsum(c["distance"] == 1)])       # d = 1 pairs before pair p; the pairs are sorted by row
    first = np.searchsorted(c["pairs"][0], ptr)
    c["d1_ranges"] = [(int(rank1[first[g]]), int(rank1[first[g + 1]])) for g in range(len(graphs))]
    return c


def _no_d1():
    t = np.arange(30, dtype=np.int64)
    return _base("no_d1", 12, np.stack([(t * 5 + 1) % 12, (t * 7 + 3) % 12]), 2 + t % 2, 3, "tensors")


_BUILDERS = dict(degrees=_degrees, ties=_ties, hub=lambda: _expanded("hub", [(gc.case("hub")["num_nodes"], gc.case("hub")["edge_index"].numpy())], 2),
                 segments=_segments, edgeless_9=lambda: _expanded("edgeless_9", [(4, NONE), (5, NONE)], 2), no_d1=_no_d1)
_BUILDERS.update({"rows_%d" % n: functools.partial(_rows, n) for n in ROWS_N})
ROWS_CASES = ["rows_%d" % n for n in ROWS_N]
CASE_NAMES = ["degrees", "ties", "hub", "segments", "edgeless_9", "no_d1"] + ROWS_CASES


@functools.lru_cache(maxsize=None)
def case(name):
    """the case of that name, built once; never modified"""
    return _BUILDERS[name]()


def ks_of(name):
    """the k at which a case is run: 1..4 where it has the distances; the row schedules at their k = 2 alone"""
    c = case(name)
    return [c["k"]] if name.startswith("rows_") else list(range(1, c["k"] + 1))


# ---- structure, restated on the CPU ---------------------------------------------------------------------------------------
def bwd_blocks(n):
    """esc_gineplus_bwd_blocks: one wave per source row, 8 waves per workgroup, at most 512 workgroups"""
    return min(max(-(-n // BWD_WAVES), 1), BWD_MAX_BLOCKS)


def pair_degrees(c):
    """(in-degree, out-degree) of every node over ALL the pairs of the case"""
    n = c["num_nodes"]
    return np.bincount(c["pairs"][1], minlength=n), np.bincount(c["pairs"][0], minlength=n)


def num_d1(c):
    return int((c["distance"] == 1).sum())


def grouping(c):
    """(rank, out_order, in_order): the rank of every pair among the distance-1 pairs IN THE ORDER GIVEN (-1 off distance 1),
    the pairs in (row, col) order, and grouped by destination with ascending source inside; equal keys keep the order given"""
    row, col = c["pairs"]
    idx = np.arange(len(row))
    is1 = c["distance"] == 1
    rank = np.where(is1, np.cumsum(is1) - 1, -1)
    return rank, np.lexsort((idx, col, row)), np.lexsort((idx, row, col))


def plan_arrays(c):
    """what a MultihopPlan of the case must hold: meta, out_ptr, in_ptr, in_meta"""
    n = c["num_nodes"]
    row, col = c["pairs"]
    rank, out_order, in_order = grouping(c)
    full = np.stack([row, col, c["distance"], rank], axis=1)
    ptr = lambda key: np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n))])
    return dict(meta=full[out_order].astype(np.int32), out_ptr=ptr(row).astype(np.int64), in_ptr=ptr(col).astype(np.int32),
                in_meta=full[in_order].astype(np.int32))


def restricted(c, k):
    """the case with the pairs of distance 1..k alone, in the order they had"""
    keep = (c["distance"] >= 1) & (c["distance"] <= k)
    return _base(c["name"] + "_le%d" % k, c["num_nodes"], c["pairs"][:, keep], c["distance"][keep], k, "tensors", batch=c["batch"])


# ---- operands ---------------------------------------------------------------------------------------------------------------
def operands(name, k, C, seed=None):
    """(xs, e, eps, g) as test_hip_multihop._agg_inputs draws them: x_t, e ~ N(0, 1), eps ~ 0.3 N(0, 1), g ~ N(0, 1 / N); the
    `ties` case then puts chosen messages and rows on the gate"""
    c = case(name)
    n, m1 = c["num_nodes"], num_d1(c)
    gen = torch.Generator().manual_seed(1000 * k + C if seed is None else seed)
    xs = [torch.randn(n, C, generator=gen) for _ in range(k)]
    e, eps = torch.randn(m1, C, generator=gen), 0.3 * torch.randn(k + 1, C, generator=gen)
    g = torch.randn(n, C, generator=gen) / float(np.sqrt(n))
    if "cancel_pairs" in c:
        rank = grouping(c)[0]
        row = c["pairs"][0]
        xs[0][c["negzero_source"]] = -0.0
        p, q = c["negzero_pairs"]
        e[rank[p]] = 0.0
        e[rank[q]] = -0.0
        for p in c["cancel_pairs"]:
            e[rank[p]] = -xs[0][row[p]]
        for t, rows in c["dead_sources"].items():
            if t < k:
                for node, v in rows:
                    xs[t][node] = v
    return xs, e, eps, g


# ---- the sequential specification (numpy float32, one rounding per operation) ------------------------------------------------
_f32 = gc._f32


def forward_loop(c, k, xs, e, eps, keep=None):
    """per destination, its pairs in ascending source order: acc[d] = acc[d] + max(x_{d-1}[j] + [d = 1] e[rank], 0); then
    res = (1 + eps[0]) x_0[i], res = res + (1 + eps[d]) acc[d] for ascending d <= k.  keep: a mask of the pairs that count"""
    xs, e, eps = [_f32(x) for x in xs], _f32(e), _f32(eps)
    n, C = xs[0].shape
    row, col, dist = c["pairs"][0].tolist(), c["pairs"][1].tolist(), c["distance"].tolist()
    rank, _, order = grouping(c)
    rank, order = rank.tolist(), order.tolist()
    one, zero = np.float32(1), np.float32(0)
    ope = [one + eps[d] for d in range(k + 1)]
    out = np.empty((n, C), dtype=np.float32)
    pos, m = 0, len(order)
    for i in range(n):
        acc = [np.zeros(C, dtype=np.float32) for _ in range(k + 1)]
        while pos < m and col[order[pos]] == i:
            p = order[pos]
            pos += 1
            d = dist[p]
            if d < 1 or d > k or (keep is not None and not keep[p]):
                continue
            msg = xs[d - 1][row[p]]
            if d == 1 and e.shape[0]:
                msg = msg + e[rank[p]]
            acc[d] = acc[d] + np.maximum(msg, zero)
        res = ope[0] * xs[0][i]
        for d in range(1, k + 1):
            res = res + ope[d] * acc[d]
        out[i] = res
    assert pos == m
    return torch.from_numpy(out)


def backward_loop(c, k, xs, e, eps, g):
    """per source, its pairs in (row, col) order: the pair's own term is (1 + eps[d]) g[i] where the message is > 0, else +0;
    accS[d - 1] = accS[d - 1] + term; d_e[rank] = term; dx_0 = g (1 + eps[0]) + accS[0], dx_t = accS[t].  Returns ([dx_t], d_e)"""
    xs, e, eps, g = [_f32(x) for x in xs], _f32(e), _f32(eps), _f32(g)
    n, C = xs[0].shape
    row, col, dist = c["pairs"][0].tolist(), c["pairs"][1].tolist(), c["distance"].tolist()
    rank, order, _ = grouping(c)
    rank, order = rank.tolist(), order.tolist()
    one, zero = np.float32(1), np.float32(0)
    ope = [one + eps[d] for d in range(k + 1)]
    dx = [np.empty((n, C), dtype=np.float32) for _ in range(k)]
    d_e = np.empty_like(e)
    pos, m = 0, len(order)
    for j in range(n):
        acc = [np.zeros(C, dtype=np.float32) for _ in range(k)]
        while pos < m and row[order[pos]] == j:
            p = order[pos]
            pos += 1
            d = dist[p]
            if d < 1 or d > k:
                continue
            msg = xs[d - 1][j]
            if d == 1 and e.shape[0]:
                msg = msg + e[rank[p]]
            term = np.where(msg > zero, g[col[p]] * ope[d], zero)
            acc[d - 1] = acc[d - 1] + term
            if d == 1 and e.shape[0]:
                d_e[rank[p]] = term
        dx[0][j] = g[j] * ope[0] + acc[0]
        for t in range(1, k):
            dx[t][j] = acc[t]
    assert pos == m
    return [torch.from_numpy(a) for a in dx], torch.from_numpy(d_e)


def deps64(c, k, xs, e, g):
    """(d_eps, sum of the magnitudes of its terms), both fp64 [k + 1, C]: d_eps[0] = sum_i g[i] x_0[i], d_eps[d] = sum over the
    pairs of distance d of g[col] relu(x_{d-1}[row] + [d = 1] e[rank])"""
    xs, e, g = [_f32(x).astype(np.float64) for x in xs], _f32(e).astype(np.float64), _f32(g).astype(np.float64)
    row, col = c["pairs"]
    rank = grouping(c)[0]
    val, mag = np.zeros((k + 1, g.shape[1])), np.zeros((k + 1, g.shape[1]))
    val[0], mag[0] = (g * xs[0]).sum(axis=0), np.abs(g * xs[0]).sum(axis=0)
    for d in range(1, k + 1):
        sel = c["distance"] == d
        msg = xs[d - 1][row[sel]]
        if d == 1 and e.shape[0]:
            msg = msg + e[rank[sel]]
        t = g[col[sel]] * np.maximum(msg, 0.0)
        val[d], mag[d] = t.sum(axis=0), np.abs(t).sum(axis=0)
    return torch.from_numpy(val), torch.from_numpy(mag)


def deps_depth(c, k):
    """[k + 1] ints: the number of fp32 roundings a term of d_eps[d] can meet on its way through gp_bwd_wave and
    gp_deps_reduce (csrc/gineplus.hip), on the longest path of their fixed order.  With P = bwd_blocks(N) workgroups a wave
    takes R = ceil(N / 8P) rows at the most.

    inside the wave  d = 0: one fma per row, dep = fma(g, x_0, dep)                                      R
                     d = 1: the message x_0 + e, then one fma per distance-1 pair of the wave's rows      1 + (most such pairs
                                                                                                          on one wave)
                     d >= 2: accU = accU + g over the n pairs of the row at that distance, from +0         (n - 1 for the
                             (the first add is exact), then one fma per row, dep = fma(relu(x), accU, dep)  longest row) + R
    the workgroup    wave 0's partial meets the 7 others in LDS                                            7
    gp_deps_reduce   group 0 adds its ceil(P / 4) partial rows to +0, the first exactly                    ceil(P / 4) - 1
                     the groups that hold a row are added in order                                         min(3, P - 1)
    """
    n = c["num_nodes"]
    row, dist = c["pairs"][0], c["distance"]
    P = bwd_blocks(n)
    W = BWD_WAVES * P
    R = -(-n // W)
    tail = (BWD_WAVES - 1) + (-(-P // 4) - 1) + min(3, P - 1)
    depth = [R + tail]
    for d in range(1, k + 1):
        deg = np.bincount(row[dist == d], minlength=n)
        if d == 1:
            depth.append(1 + int(np.bincount(np.arange(n) % W, weights=deg, minlength=W).max()) + tail)
        else:
            depth.append(max(int(deg.max()) - 1, 0) + R + tail)
    return depth


def deps_bound(c, k, mag):
    """the elementwise bound on |d_eps - fp64|: depth * 2^-24 * sum |terms|, fp64 [k + 1, C]"""
    return torch.tensor(deps_depth(c, k), dtype=torch.float64).view(-1, 1) * 2.0 ** -24 * mag


def aggregate_torch(c, k, xs, e, eps, dtype):
    """the same formula by plain torch in `dtype` on the pairs put into (row, col) order first, which inside a destination is
    ascending source: index_add_ on one thread then adds in the specified order, forward and (through autograd) backward.
    Returns (out, xs, e, eps); the three are the leaves whose .grad a backward of `out` fills"""
    rank, order, _ = grouping(c)
    row, col = torch.from_numpy(c["pairs"][:, order])
    dist = torch.from_numpy(c["distance"][order])
    xs = [x.detach().to(dtype, copy=True).requires_grad_(True) for x in xs]
    e, eps = e.detach().to(dtype, copy=True).requires_grad_(True), eps.detach().to(dtype, copy=True).requires_grad_(True)
    out = (1 + eps[0]) * xs[0]
    for d in range(1, k + 1):
        sel = dist == d
        msg = xs[d - 1].index_select(0, row[sel])
        if d == 1 and e.shape[0]:
            msg = msg + e.index_select(0, torch.from_numpy(rank[order])[sel])
        out = out + (1 + eps[d]) * torch.zeros_like(xs[0]).index_add_(0, col[sel], msg.relu())
    return out, xs, e, eps


@functools.lru_cache(maxsize=None)
def reference(name, k, C):
    """operands and every CPU reference of one (case, k, width), computed once and shared by the tests; never modified"""
    c = case(name)
    xs, e, eps, g = operands(name, k, C)
    dx, d_e = backward_loop(c, k, xs, e, eps, g)
    d_eps, mag = deps64(c, k, xs, e, g)
    return dict(xs=xs, e=e, eps=eps, g=g, out=forward_loop(c, k, xs, e, eps), dx=dx, d_e=d_e, d_eps=d_eps, mag=mag)
