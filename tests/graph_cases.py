"""Small synthetic batches whose STRUCTURE is the test: degenerate and skewed graphs, bags and segments for the
index-driven kernels (csrc/aggregate.hip, bag.hip, plan.hip), generated deterministically — no fixture file, no
reference project, no random number generator whose stream could change between library versions.

CASES is a list of dicts: name, edge_index (int64 [2, E]), num_nodes, batch (int64 [N], non-decreasing), num_graphs,
and for the bag cases pos_enc / pos_index / pos_batch (int64 [Z], pos_batch non-decreasing) and n_cols.

The *_loop functions are the SEQUENTIAL references: explicit loops over edges / entries / nodes in ascending order, one
separately rounded fp32 operation at a time (numpy float32).  The loop is the specification; the CPU test checks that
single-threaded torch.index_add_ agrees with it bit for bit, the GPU tests hold the kernels to it.
"""
import numpy as np
import torch

N_COLS = 1800
BAG_CH = 64                       # entries per chunk of the table-gradient kernels (csrc/bag.hip)
DEGREE_SET = (0, 1, 7, 8, 9, 15, 16, 17, 64, 65)
# column lengths of `bag_borders` in column order (after the stable sort by column) and the table rows they sit on
BORDER_LENGTHS = (64, 1, 63, 320, 0, 0, 65, 127, 30, 0, 300, 5, 7)
BORDER_COLUMNS = (0, 1, 2, 3, 4, 5, 6, 7, 900, 901, 902, 1000, 1799)
BORDER_EDGES = 331                # prime: every stride walks all the edges before it repeats one
LOCAL_EDGES, LOCAL_ENTRIES, LOCAL_H = 4200, 4096 + 37, 256


def _perm(n, mul, add):
    """a fixed permutation of 0..n-1 (mul coprime with n)"""
    assert np.gcd(mul, n) == 1
    return (np.arange(n, dtype=np.int64) * mul + add) % n


def _case(name, src, dst, num_nodes, batch=None, num_graphs=None, **bag):
    ei = torch.tensor(np.stack([np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)]).reshape(2, -1))
    batch = torch.zeros(num_nodes, dtype=torch.int64) if batch is None else torch.as_tensor(batch, dtype=torch.int64)
    d = dict(name=name, edge_index=ei, num_nodes=int(num_nodes), batch=batch,
             num_graphs=int(num_graphs if num_graphs is not None else (int(batch[-1]) + 1 if batch.numel() else 0)))
    if bag:
        for k in ("pos_enc", "pos_index", "pos_batch"):
            d[k] = torch.as_tensor(np.asarray(bag[k], dtype=np.int64))
        d["n_cols"] = N_COLS
    return d


def _degrees():
    # nodes 1..10 carry the in-degrees of DEGREE_SET in order and the out-degrees rotated by three places, so no node has
    # the same in- and out-degree and the two nodes of degree 0 on one side have edges on the other; nodes 0 and 11 are
    # isolated.  Stubs are paired through two different permutations: parallel edges and self loops come with it, the edges
    # of a node are scattered over the edge list, and nothing is symmetric.
    n = len(DEGREE_SET)
    dst = np.concatenate([np.full(d, 1 + i) for i, d in enumerate(DEGREE_SET)])
    src = np.concatenate([np.full(d, 1 + (i + 3) % n) for i, d in enumerate(DEGREE_SET)])
    m = len(dst)                                           # 202
    return _case("degrees", src[_perm(m, 55, 7)], dst[_perm(m, 89, 3)], n + 2)


def _hub():
    # leaves -> node 5 (in-degree 1000) and node 700 -> the same leaves (out-degree 1000); the leaves have in- and
    # out-degree 1, node 1002 is isolated; edge order scattered
    n, hub_in, hub_out = 1003, 5, 700
    leaves = np.array([i for i in range(n - 1) if i not in (hub_in, hub_out)], dtype=np.int64)      # 1000 of them
    src = np.concatenate([leaves, np.full(len(leaves), hub_out)])
    dst = np.concatenate([np.full(len(leaves), hub_in), leaves])
    p = _perm(len(src), 777, 11)
    c = _case("hub", src[p], dst[p], n)
    c["hub_in"], c["hub_out"] = hub_in, hub_out
    return c


def _tiny(n):
    k = np.arange(n + 3, dtype=np.int64)
    return _case("tiny_N%d" % n, (k * 7 + 1) % n, (k * 3 + 2) % n, n)


def _segments(name, sizes):
    # graph g owns sizes[g] consecutive nodes (0: the id is unused); a directed path inside every graph
    batch = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    n = int(sum(sizes))
    src = np.array([i for i in range(n - 1) if batch[i] == batch[i + 1]], dtype=np.int64)
    c = _case(name, src, src + 1, n, batch=batch, num_graphs=len(sizes))
    c["sizes"] = tuple(int(s) for s in sizes)
    return c


def _ring_edges(e, n):
    k = np.arange(e, dtype=np.int64)
    return k % n, (k * 7 + 1) % n


def _bag_edges():
    lengths = (0, 1, 200, 0, 1, 7, 8, 9, 4, 12, 250, 0)            # first and last edge without a bag
    pb = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    z = np.arange(len(pb), dtype=np.int64)
    pi = (z * 37 + pb * 101) % N_COLS
    pe = 1 + (z * z) % 13
    pe[0] = 1                                                      # the single entry of edge 1
    pe[5] = 50000                                                  # a large count inside the 200-entry bag
    pe[-1] = 65537
    src, dst = _ring_edges(len(lengths), 5)
    c = _case("bag_edges", src, dst, 5, pos_enc=pe, pos_index=pi, pos_batch=pb)
    c["lengths"] = lengths
    return c


def _bag_borders():
    # built column by column: column BORDER_COLUMNS[i] gets BORDER_LENGTHS[i] entries on distinct edges (a stride walk over
    # the prime edge count), then the entries are put into edge order (stable), as create_subgraphs would emit them
    edge, col = [], []
    for i, (c, ln) in enumerate(zip(BORDER_COLUMNS, BORDER_LENGTHS)):
        edge.append((np.arange(ln, dtype=np.int64) * (3 + 2 * i) + 17 * i) % BORDER_EDGES)
        col.append(np.full(ln, c, dtype=np.int64))
    edge, col = np.concatenate(edge), np.concatenate(col)
    order = np.argsort(edge, kind="stable")
    pb, pi = edge[order], col[order]
    pe = 1 + (np.arange(len(pb), dtype=np.int64) * 5) % 9
    src, dst = _ring_edges(BORDER_EDGES, 40)
    return _case("bag_borders", src, dst, 40, pos_enc=pe, pos_index=pi, pos_batch=pb)


def _bag_tiny():
    src, dst = _ring_edges(3, 2)
    return _case("bag_tiny", src, dst, 2, pos_enc=[2, 1, 3, 1, 4], pos_index=[7, 1799, 7, 0, 7], pos_batch=[0, 0, 1, 2, 2])


def _bag_local(name, skew):
    z = np.arange(LOCAL_ENTRIES, dtype=np.int64)
    rows = LOCAL_EDGES // 8 - 1 if skew else LOCAL_EDGES           # skew: every entry on an edge id below E / 8
    pb = (z * rows) // LOCAL_ENTRIES
    pi = (z * 53) % 600
    pe = 1 + z % 5
    src, dst = _ring_edges(LOCAL_EDGES, 64)
    return _case(name, src, dst, 64, pos_enc=pe, pos_index=pi, pos_batch=pb)


CASES = ([_degrees(), _hub()] + [_tiny(n) for n in (1, 2, 3, 4, 5)] +
         [_case("no_edges", [], [], 6),
          _segments("segments_G1", (7,)),
          _segments("segments_G5", (1, 0, 300, 3, 0)),
          _segments("segments_G9", (2, 1, 0, 0, 297, 1, 5, 0, 0)),
          _bag_edges(), _bag_borders(), _bag_tiny(), _bag_local("bag_local", False), _bag_local("bag_local_skew", True)])
BY_NAME = {c["name"]: c for c in CASES}
BAG_CASES = [c["name"] for c in CASES if "pos_batch" in c]
GRAPH_CASES = [c["name"] for c in CASES if "pos_batch" not in c]      # the aggregate runs on these (the bag cases' graphs add nothing)
TINY_CASES = ["tiny_N%d" % n for n in (1, 2, 3, 4, 5)]
SEGMENT_CASES = ["segments_G1", "segments_G5", "segments_G9"]


def case(name):
    return BY_NAME[name]


# ---- structure, restated on the CPU -------------------------------------------------------------------------------------
def degrees(c):
    """(in-degree, out-degree) of every node"""
    ei, n = c["edge_index"].numpy(), c["num_nodes"]
    return np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)


def stable_csr(key, n_keys):
    """(ptr int32 [n_keys + 1], perm int32): positions grouped by key, ascending position inside a key"""
    key = np.asarray(key, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_keys))]).astype(np.int32)
    return ptr, np.argsort(key, kind="stable").astype(np.int32)


def column_lengths(c):
    return np.bincount(c["pos_index"].numpy(), minlength=c["n_cols"])


def bag_lengths(c):
    return np.bincount(c["pos_batch"].numpy(), minlength=c["edge_index"].shape[1])


def bag_local_schedule(Z, H, rows):
    """the condition of bag_local_schedule (csrc/bag.hip), restated: the gradient rows exceed one XCD's 4 MiB L2 and there
    are at least 64 chunks to spread over the 8 groups"""
    return rows > 0 and rows * H * 4 > (4 << 20) and -(-Z // BAG_CH) >= 64


def chunk_buckets(c, rows):
    """bucket (row eighth of the middle entry) of every 64-entry chunk of the column-sorted entries, as bag_bwd_classify
    computes it"""
    _, perm = stable_csr(c["pos_index"].numpy(), c["n_cols"])
    c_row = c["pos_batch"].numpy()[perm]
    Z = len(c_row)
    eighth = (rows + 7) // 8
    out = []
    for q in range(-(-Z // BAG_CH)):
        beg, end = q * BAG_CH, min(q * BAG_CH + BAG_CH, Z)
        out.append(min(7, int(c_row[(beg + end) >> 1]) // eighth))
    return np.array(out)


# ---- sequential references (numpy float32, one rounding per operation) -------------------------------------------------
def _f32(t):
    return None if t is None else np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)


def aggregate_loop(x, e, eps, edge_index):
    """out[i] = (sum over edges k -> i, ascending k, of relu(x[src_k] (+ e[k]))) (+ (1 + eps) * x[i]); e / eps may be None"""
    x, e = _f32(x), _f32(e)
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    out = np.zeros_like(x)
    zero = np.float32(0)
    for k in range(len(src)):
        m = x[src[k]] if e is None else x[src[k]] + e[k]
        out[dst[k]] = out[dst[k]] + np.maximum(m, zero)
    if eps is not None:
        one_eps = np.float32(1) + np.float32(float(eps))
        for i in range(x.shape[0]):
            out[i] = out[i] + one_eps * x[i]
    return torch.from_numpy(out)


def aggregate_dx_loop(x, e, eps, g, edge_index):
    """fp32 sequential form of the aggregate's input gradient: dx[i] = (sum over edges i -> j, ascending k, of
    [x[i] + e[k] > 0] * g[j]) + (1 + eps) * g[i] — the yardstick for a row with very many terms"""
    x, e, g = _f32(x), _f32(e), _f32(g)
    src, dst = edge_index[0].tolist(), edge_index[1].tolist()
    dx = np.zeros_like(x)
    zero = np.float32(0)
    for k in range(len(src)):
        m = x[src[k]] if e is None else x[src[k]] + e[k]
        dx[src[k]] = dx[src[k]] + np.where(m > zero, g[dst[k]], zero)
    if eps is not None:
        one_eps = np.float32(1) + np.float32(float(eps))
        for i in range(x.shape[0]):
            dx[i] = dx[i] + one_eps * g[i]
    return torch.from_numpy(dx)


def bag_loop(table, pos_enc, pos_index, pos_batch, num_edges, base=None):
    """out[pos_batch[z]] += table[pos_index[z]] * pos_enc[z] for z = 0, 1, ...: product rounded, then the sum; starts from
    `base` (the accumulating form) or from +0"""
    w = _f32(table)
    out = np.zeros((num_edges, w.shape[1]), dtype=np.float32) if base is None else _f32(base).copy()
    pe, pi, pb = pos_enc.tolist(), pos_index.tolist(), pos_batch.tolist()
    for z in range(len(pb)):
        out[pb[z]] = out[pb[z]] + w[pi[z]] * np.float32(pe[z])
    return torch.from_numpy(out)


def segment_sum_loop(x, batch, num_graphs):
    """out[batch[i]] += x[i] for i = 0, 1, ..."""
    x = _f32(x)
    out = np.zeros((num_graphs, x.shape[1]), dtype=np.float32)
    b = batch.tolist()
    for i in range(len(b)):
        out[b[i]] = out[b[i]] + x[i]
    return torch.from_numpy(out)
