"""Case table of the feature builder (csrc/features.hip): graphs chosen for the branch each one reaches, and what every case
claims about itself.  No GPU here: tests/test_feature_cases_cpu.py proves the claims from the oracle's hop tables and checks that
the bit-exact rd comparison is a fair one; tests/test_hip_feature_structure.py runs the table on the device.

A graph is `(n, src, dst)` with int64 arrays of graph-local node ids.  A case is a dict:
    name, graphs, h, use_rd, self_loop      what goes into encode_edge_lists, as one batch
    out_edges                               output edges of the whole batch
    max_nodes                               the largest graph (what the host picks the rd launches from)
    classes                                 rd classes per ego-net size bucket (m <= 32, <= 64, <= 96, larger), rd cases only;
                                            a class is an unordered pair of reach sets {S_u, S_v} present among a graph's edges
    m_range                                 smallest and largest ego-net size |S_u ∪ S_v| over the batch's edges (rd cases)
    zero_edge_middle                        (optional) a graph without output edges that is neither first nor last
"""
import numpy as np

import graph_sources as gs
import ref_features as orc

try:                                         # hundreds of 100 x 100 pinv calls: a BLAS thread pool only gets in its own way
    from threadpoolctl import threadpool_limits as _blas_threads
except ImportError:
    import contextlib

    def _blas_threads(limits):
        return contextlib.nullcontext()

I64 = np.int64
BUCKET_LIMITS = (32, 64, 96)                 # features.hip: m <= 32 / 64 / 96 stay in LDS, larger ones use the global slab
LDS_GRIDS = (None, 512, 256)                 # workgroups of the ld = 64 and ld = 96 launches (256 * per_cu)
HUGE_SLABS = 64                              # workgroups of the slab launch, at most


def bucket_of(m):
    return sum(1 for limit in BUCKET_LIMITS if m > limit)


def _both(pairs):
    s = np.array([a for a, b in pairs] + [b for a, b in pairs], I64)
    t = np.array([b for a, b in pairs] + [a for a, b in pairs], I64)
    return s, t


def directed(n, pairs):
    return n, np.array([a for a, b in pairs], I64), np.array([b for a, b in pairs], I64)


def edgeless(n):
    return n, np.zeros(0, I64), np.zeros(0, I64)


def hub_ring(n):
    """node 0 joined to everyone, the others on a ring: every 2-hop ego-net is the whole graph"""
    pairs = [(0, i) for i in range(1, n)] + [(i, i + 1) for i in range(1, n - 1)] + [(n - 1, 1)]
    return (n,) + _both(pairs)


def regular_like(n, seed, k=2):
    """ring + k random perfect matchings (degree <= 2 + k): many distinct 3- and 4-hop ego-nets of a good part of the graph"""
    rng = np.random.default_rng(seed)
    pairs = {(i, (i + 1) % n) for i in range(n)}
    for _ in range(k):
        p = rng.permutation(n)
        pairs |= {(int(min(a, b)), int(max(a, b))) for a, b in zip(p[0::2], p[1::2]) if a != b}
    pairs = sorted((min(a, b), max(a, b)) for a, b in pairs)
    return (n,) + _both(pairs)


def ring(n):
    return (n,) + _both([(i, (i + 1) % n) for i in range(n)])


def star(n):
    """node 0 joined to the n - 1 others, both directions: out-degree n - 1 at the hub"""
    return (n,) + _both([(0, i) for i in range(1, n)])


def multi_edge_graph(seed, n):
    """directed graph with repeated (s, t) entries (one of them three times), reversed repeats and pre-existing self loops
    (one of them twice), scattered over the edge list"""
    rng = np.random.RandomState(seed)
    m = 2 * n
    s, t = rng.randint(0, n, size=m), rng.randint(0, n, size=m)
    t = np.where(s == t, (s + 1) % n, t)
    dup = rng.choice(m, 4, replace=False)
    rev = rng.choice(m, 3, replace=False)
    loops = rng.choice(n, 3, replace=False)
    s2 = np.concatenate([s, s[dup], s[dup[:1]], t[rev], loops, loops[:1]])
    t2 = np.concatenate([t, t[dup], t[dup[:1]], s[rev], loops, loops[:1]])
    p = rng.permutation(s2.shape[0])
    return n, s2[p].astype(I64), t2[p].astype(I64)


MULTI_EDGE_GRAPHS = (multi_edge_graph(1, 7), multi_edge_graph(2, 8), multi_edge_graph(3, 9), multi_edge_graph(4, 10))
MULTI_EDGE_CONFIGS = ((2, True, True), (3, True, False), (3, False, False), (4, True, True))
GOLDEN_FILE = "features_structure.npz"


def multi_edge_name(gi, cfg):
    return "multi%d/h%d_rd%d_sl%d" % (gi, cfg[0], int(cfg[1]), int(cfg[2]))


# ---- the pool of many_tiny_graphs: 1 to 6 nodes, output-edge counts and sizes all over the place --------------------
TINY_POOL = (
    ("node", edgeless(1)),
    ("triangle", (3,) + _both([(0, 1), (1, 2), (0, 2)])),
    ("edgeless3", edgeless(3)),
    ("arc", directed(2, [(0, 1)])),
    ("path4", (4,) + _both([(0, 1), (1, 2), (2, 3)])),
    ("only_loop", directed(1, [(0, 0)])),
    ("star5", star(5)),
    ("dicycle_dup", directed(3, [(0, 1), (1, 2), (2, 0), (0, 1)])),
    ("edgeless2", edgeless(2)),
    ("cycle6", ring(6)),
    ("tri_loop_isolated", directed(5, [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0), (3, 3)])),
    ("dipath_back", directed(4, [(0, 1), (1, 2), (2, 3), (2, 1), (1, 2)])),
    ("edge", (2,) + _both([(0, 1)])),
)
TINY_G = 2100


def tiny_graphs(count=TINY_G):
    return [TINY_POOL[i % len(TINY_POOL)][1] for i in range(count)]


MOL20 = gs.molecule_like_graph(3, 20, 20)
HUGE_SEED = 6
LD64_SEEDS = (1, 2, 3, 4)
LD96_SEEDS = (5, 6)


def _case(name, graphs, h, use_rd, self_loop, **claims):
    return dict(name=name, graphs=list(graphs), h=h, use_rd=use_rd, self_loop=self_loop, **claims)


def _hub_case(n, classes):
    return _case("hub%d" % n, [hub_ring(n)], 2, True, True, out_edges=5 * n - 4, max_nodes=n, classes=classes, m_range=(n, n))


CASES = [
    # one class each, the whole graph: m == n == max_nodes on either side of every bucket limit
    _hub_case(32, (1, 0, 0, 0)), _hub_case(33, (0, 1, 0, 0)), _hub_case(64, (0, 1, 0, 0)),
    _hub_case(65, (0, 0, 1, 0)), _hub_case(96, (0, 0, 1, 0)), _hub_case(97, (0, 0, 0, 1)),
    # all four buckets in one call, the largest graph first
    _case("buckets_mixed", [hub_ring(97), hub_ring(32), MOL20, hub_ring(64), hub_ring(33)], 2, True, True,
          out_edges=1176, max_nodes=97, classes=(37, 2, 0, 1), m_range=(3, 97)),
    # a graph beyond the LDS limit whose ego-nets are tiny: the slab is allocated, the slab kernel finds an empty list
    _case("big_graph_small_egonets", [ring(120)], 1, True, True, out_edges=360, max_nodes=120, classes=(240, 0, 0, 0),
          m_range=(3, 4)),
    _case("big_graph_small_egonets_second", [hub_ring(33), ring(120)], 1, True, True, out_edges=521, max_nodes=120,
          classes=(304, 33, 0, 0), m_range=(3, 33)),
    # more classes in one bucket than its launch has workgroups: every workgroup reuses its LDS arrays / its slab
    _case("many_classes_ld64", [regular_like(80, s, k=2) for s in LD64_SEEDS], 3, True, False,
          out_edges=1266, max_nodes=80, classes=(0, 633, 0, 0), m_range=(35, 64)),
    _case("many_classes_ld96", [regular_like(96, s, k=3) for s in LD96_SEEDS], 3, True, False,
          out_edges=944, max_nodes=96, classes=(0, 0, 472, 0), m_range=(66, 94)),
    _case("many_classes_huge", [regular_like(130, HUGE_SEED, k=2)], 4, True, True,
          out_edges=644, max_nodes=130, classes=(0, 2, 71, 314), m_range=(60, 124)),
    # both scans carry over two 1024 boundaries; without self loops the edgeless shapes repeat out_edge_ptr mid-batch
    _case("many_tiny_graphs_loops", tiny_graphs(), 2, True, True, out_edges=14691, max_nodes=6, classes=(6294, 0, 0, 0),
          m_range=(1, 6)),
    _case("many_tiny_graphs_plain", tiny_graphs(), 2, True, False, out_edges=8394, max_nodes=6, classes=(3227, 0, 0, 0),
          m_range=(1, 6), zero_edge_middle=True),
    # the cap_edges == 0 return of esc_features_count
    _case("all_edgeless_rd", [edgeless(3), edgeless(1), edgeless(5)], 2, True, False, out_edges=0, max_nodes=5,
          classes=(0, 0, 0, 0), m_range=None),
    _case("all_edgeless_plain", [edgeless(3), edgeless(1), edgeless(5)], 2, False, False, out_edges=0, max_nodes=5),
]
CASES += [_case("multi_edges_h%d_rd%d_sl%d" % (h, int(rd), int(sl)), MULTI_EDGE_GRAPHS, h, rd, sl, golden=True,
                out_edges=134 if sl else 116, max_nodes=10) for h, rd, sl in MULTI_EDGE_CONFIGS]
BY_NAME = {c["name"]: c for c in CASES}

# star_degree_limit: h = 1, no rd.  (nodes, self_loop, the hub's sub-degree, encodes)
STAR_CASES = ((199, True, 199, True), (200, False, 199, True), (200, True, 200, False), (201, False, 200, False))


def case(name):
    return BY_NAME[name]


# ---- expectations: the oracle once per distinct (graph, config), whatever the number of copies in a batch ---------------
_MEMO = {}
_MARGINS = {}


def in_edge_of_out(n, src, dst, self_loop):
    """which input edge every output edge came from: the surviving ones in order, then -1 for the n appended loops"""
    if not self_loop:
        return np.arange(src.shape[0], dtype=I64)
    return np.concatenate([np.flatnonzero(src != dst).astype(I64), np.full(n, -1, I64)])


def expected(graph, h, use_rd, self_loop, record=False):
    """the six outputs of encode_edge_lists for one graph, from the oracle (do not modify the returned arrays).  With `record`
    the oracle runs under a PinvRecorder, kept for margins()."""
    n, s, t = graph
    key = (n, s.tobytes(), t.tobytes(), h, use_rd, self_loop)
    record = record and use_rd
    if key not in _MEMO or (record and key not in _MARGINS):
        with _blas_threads(1):
            if record:
                with PinvRecorder() as rec:
                    w = orc.encode_graph(s, t, n, h, use_rd, self_loop)
                _MARGINS[key] = rec
            else:
                w = orc.encode_graph(s, t, n, h, use_rd, self_loop)
        if self_loop:
            assert np.array_equal(w["kept"], s != t)
        _MEMO[key] = dict(out_src=w["edge_src"], out_dst=w["edge_dst"], in_edge_of_out=in_edge_of_out(n, s, t, self_loop),
                          pos_enc=w["pos_enc"], pos_index=w["pos_index"], pos_batch=w["pos_batch"])
    return _MEMO[key]


def margins(graph, h, self_loop):
    """the PinvRecorder of expected(graph, h, True, self_loop, record=True)"""
    n, s, t = graph
    return _MARGINS[(n, s.tobytes(), t.tobytes(), h, True, self_loop)]


def expected_batch(c, record=False):
    return [expected(g, c["h"], c["use_rd"], c["self_loop"], record) for g in c["graphs"]]


# ---- recording what the oracle's pseudo-inverse sees ------------------------------------------------------------------
class PinvRecorder(object):
    """Stands in for the scipy.linalg handle of ref_features while a case is encoded: every Laplacian handed to pinv and the
    fp64 rd vector formed from the result (rd = P00 + diag(P) - P[0, :] - P[:, 0], ref_features._pinv_rd) are reduced to
    the two margins the CPU test bounds.  ref_features itself is not edited."""

    def __init__(self):
        self.real = orc._sla
        self.count = 0
        self.rd_far = np.inf          # distance to the nearest integer, over the rd values more than SNAP away from one
        self.rd_near = 0.0            # the same, over the values within SNAP
        self.sv_low = 0.0             # largest relative singular value below the gap, in units of scipy's cutoff m * eps
        self.sv_high = np.inf         # smallest relative singular value above it
        self.rd_max = 0.0

    SNAP = 1e-7

    def pinv(self, L, *a, **kw):
        P = self.real.pinv(L, *a, **kw)
        self.count += 1
        rd = P[0, 0] + np.diag(P) - P[0, :] - P[:, 0]
        dist = np.abs(rd - np.rint(rd))
        near = dist <= self.SNAP
        if near.any():
            self.rd_near = max(self.rd_near, float(dist[near].max()))
        if (~near).any():
            self.rd_far = min(self.rd_far, float(dist[~near].min()))
        self.rd_max = max(self.rd_max, float(np.abs(rd).max()))
        sv = np.linalg.svd(L, compute_uv=False)
        if sv[0] > 0.0:
            rel = sv / sv[0]
            cut = L.shape[0] * np.finfo(np.float64).eps
            low = rel < 1e-10
            if low.any():
                self.sv_low = max(self.sv_low, float(rel[low].max()) / cut)
            self.sv_high = min(self.sv_high, float(rel[~low].min()))
        return P

    def __getattr__(self, name):
        return getattr(self.real, name)

    def __enter__(self):
        orc._sla = self
        return self

    def __exit__(self, *exc):
        orc._sla = self.real
        return False
