"""Multi-hop edges of a collated batch on the device (csrc/multihop.hip) — what feeds the GINE+ baseline.  The reference builds
them inside every forward (modules/gine_operations.py:243, make_multihop_edges :256-303: k - 1 torch_sparse SpGEMMs and a
coalesce(op='min')); here one bounded BFS per node writes the pairs already sorted by (row, col), together with what the GINE+
aggregate walks:

    multihop_edge_index [2, M], distance [M]     {(i, i) at 0} u {(i, j) at d(i -> j) : 1 <= d(i -> j) <= k}, int64
    MultihopPlan                                  the pairs grouped by source (the output order itself) and by destination
                                                  (one stable esc_plan_csr grouping of the column), with (row, col, distance,
                                                  rank among the distance-1 pairs) per pair: no per-distance mask is ever built

A batch with no edge at all has no pairs, not even the diagonal (reference :270-273).
"""
import copy

import torch

from . import _native as nv
from .expansion import (GraphStore, _below_2_31, _column_totals, _count_prologue, _known_sizes, _raise_status as _raise_for,
                        _sizes_of_list, _tagged_sizes, _wants_check)

K_MAX = 8
MAX_NODES = 4096             # one byte of LDS per node of the root's graph (csrc/multihop.hip)
FUSED_K_MAX = 4              # the one-launch aggregate (csrc/gineplus.hip) holds k accumulators per lane


def _check_k(k):
    if isinstance(k, bool) or int(k) != k:
        raise ValueError("multihop: k must be an integer (got %r)" % (k,))
    k = int(k)
    if k < 1 or k > K_MAX:
        raise ValueError("multihop: k=%d outside 1..%d" % (k, K_MAX))
    return k


class MultihopPlan(object):
    """What the GINE+ aggregate walks.  meta [M, 4] int32 = (row, col, distance, rank) per pair in (row, col) order with
    out_ptr int64 [N+1] (grouping by source); in_ptr int32 [N+1] and in_meta [M, 4] (grouping by destination, ascending source
    inside); counts[d] = pairs at distance d when the host knows them (None: unknown)."""

    def __init__(self, multihop_edge_index, distance, num_nodes, k, out_ptr, meta, in_ptr, in_meta, counts=None):
        # (the [2, M] tensor itself carries the plan as `_esc_multihop_plan`: only its rows are kept here, so that the two do
        # not hold each other)
        self.row, self.col, self.distance = multihop_edge_index[0], multihop_edge_index[1], distance
        multihop_edge_index._esc_multihop_plan = self
        self.num_nodes, self.k = int(num_nodes), int(k)
        self.out_ptr, self.meta, self.in_ptr, self.in_meta = out_ptr, meta, in_ptr, in_meta
        self.counts = None if counts is None else [int(c) for c in counts]
        self.num_pairs = int(distance.numel())

    @property
    def num_d1(self):
        """number of distance-1 pairs = rows of the edge term (read back when the plan was built without known counts)"""
        if self.counts is None:
            self.counts = torch.bincount(self.distance, minlength=self.k + 1).tolist() if self.num_pairs else [0] * (self.k + 1)
        return self.counts[1] if len(self.counts) > 1 else 0

    @staticmethod
    def _group_by_destination(meta, col, num_nodes):
        from .plan import _csr
        dev = col.device
        if col.numel() == 0:
            return torch.zeros(num_nodes + 1, dtype=torch.int32, device=dev), meta
        bad = torch.zeros(1, dtype=torch.int32, device=dev)          # the columns are node ids the expansion wrote: never read
        in_ptr, in_perm = _csr(col, num_nodes, bad=bad)
        return in_ptr, meta[in_perm.long()].contiguous()

    @staticmethod
    def from_tensors(multihop_edge_index, distance, num_nodes, k=None):
        """The plan of multi-hop edges the user supplies, in any order (the reference's forward takes them as inputs).  The
        pairs are put into (row, col) order by two stable groupings; ranges are checked with read-backs."""
        from .plan import _csr
        mei, dist = multihop_edge_index, distance
        if mei.device.type != "cuda":
            raise RuntimeError("esc_gnn_amd.multihop: the multi-hop edges must be on the HIP device; there is no CPU fallback")
        N, M = int(num_nodes), int(dist.numel())
        if mei.dim() != 2 or mei.size(0) != 2 or mei.size(1) != M:
            raise ValueError("MultihopPlan: multihop_edge_index %s does not match distance %s" % (tuple(mei.shape), tuple(dist.shape)))
        dev = mei.device
        dmax = int(dist.max()) if M else 0
        if M and (int(dist.min()) < 0 or int(mei.min()) < 0 or int(mei.max()) >= N):
            raise ValueError("MultihopPlan: a pair refers to a node outside [0, %d) or has a negative distance" % N)
        k = dmax if k is None else int(k)
        if M == 0:
            z32 = torch.zeros((0, 4), dtype=torch.int32, device=dev)
            return MultihopPlan(mei, dist, N, k, torch.zeros(N + 1, dtype=torch.int64, device=dev), z32,
                                torch.zeros(N + 1, dtype=torch.int32, device=dev), z32, [0] * (k + 1))
        # (row, col) order: stable by col, then stable by row
        _, p1 = _csr(mei[1], N)
        p1 = p1.long()
        out_ptr, p2 = _csr(mei[0][p1], N)
        order = p1[p2.long()]
        row, col, d = mei[0][order], mei[1][order], dist[order]
        # the rank among the distance-1 pairs FOLLOWS THE INPUT ORDER of those pairs: row m of edge_attr goes with the m-th
        # column of multihop_edge_index[:, distance == 1], which is what the reference's forward reads (:351)
        is1 = dist == 1
        rank_in = torch.cumsum(is1.to(torch.int64), 0) - 1
        rank = torch.where(d == 1, rank_in[order], torch.full_like(d, -1))
        meta = torch.stack([row, col, d, rank], dim=1).to(torch.int32).contiguous()
        in_ptr, in_meta = MultihopPlan._group_by_destination(meta, col, N)
        counts = torch.bincount(dist.clamp(max=k + 1), minlength=k + 2).tolist()[:k + 1]
        return MultihopPlan(mei, dist, N, k, out_ptr.to(torch.int64), meta, in_ptr, in_meta, counts)


def _count(batch, k, G_known=None, max_nodes=None):
    k = _check_k(k)
    c = _count_prologue(batch, MAX_NODES, "multihop", G_known, max_nodes)
    G, N = c["G"], c["N"]
    _below_2_31("multihop", "%d nodes / %d edges", N, c["E"])
    dev = batch.edge_index.device
    pair_ptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    d1_ptr = torch.empty(N + 1, dtype=torch.int64, device=dev)
    dist_count = torch.empty((max(G, 1), k + 1), dtype=torch.int64, device=dev)
    nv.call("esc_multihop_count", nv.ptr(c["node_ptr"]), nv.ptr(c["edge_ptr"]), nv.ptr(c["src"]), nv.ptr(c["dst"]), max(G, 1), N, c["E"],
            c["nmax"], k, nv.ptr(pair_ptr), nv.ptr(d1_ptr), nv.ptr(dist_count), nv.ptr(c["status"]), nv.stream())
    c.update(k=k, pair_ptr=pair_ptr, d1_ptr=d1_ptr, dist_count=dist_count)
    return c


def _raise_status(c, what):
    _raise_for(c, what, "a node id outside the graph, edges of one graph not contiguous, a graph of more than %d nodes (limit %d), "
               "or a pair total that is not the count pass's" % (c["nmax"], MAX_NODES))


def multihop_sizes(batch_or_list, k, chunk=4096):
    """The count pass alone: int64 [G, k+1] on the host, per graph the number of pairs at every distance 0..k."""
    if isinstance(batch_or_list, (list, tuple)):
        return _sizes_of_list(lambda b: (multihop_sizes(b, k), 0), batch_or_list, chunk, lambda: _check_k(k) + 1)[0]
    c = _count(batch_or_list, k)
    _raise_status(c, "multihop_sizes")
    return c["dist_count"][:c["G"]].cpu()


def expand_multihop(batch, k, sizes=None, check=None, max_nodes=None):
    """(multihop_edge_index [2, M], distance [M], MultihopPlan) of a collated batch on its device.
    sizes: the batch's rows of a `multihop_sizes` result (known on the host from the dataset build) — M and the number of
    distance-1 pairs are their sums and nothing is read back; without it the total is copied once.  check: read the status back
    and raise (default: only without `sizes`, where the call synchronises anyway)."""
    k = _check_k(k)
    dev = batch.edge_index.device
    N, E = int(batch.batch.numel()), int(batch.edge_index.size(1))
    if E == 0:                                               # the reference returns before it forms the diagonal (:270-273)
        mei = torch.empty((2, 0), dtype=torch.int64, device=dev)
        z32 = torch.zeros((0, 4), dtype=torch.int32, device=dev)
        dist = mei[0]
        plan = MultihopPlan(mei, dist, N, k, torch.zeros(N + 1, dtype=torch.int64, device=dev), z32,
                            torch.zeros(N + 1, dtype=torch.int32, device=dev), z32, [0] * (k + 1))
        return mei, dist, plan
    sizes, G_known, max_nodes = _known_sizes(sizes, k + 1, max_nodes)        # n_g = its distance-0 pairs
    c = _count(batch, k, G_known, max_nodes)
    # per distance from `sizes`, or the one total that `sizes` saves reading back
    totals = _column_totals("expand_multihop", c, sizes, G_known, lambda: [c["pair_ptr"][N].item()])
    M, counts = sum(totals), (None if sizes is None else totals)
    _below_2_31("expand_multihop", "%d pairs", M)
    out = torch.empty((3, M), dtype=torch.int64, device=dev)          # row | col | distance
    meta = torch.empty((M, 4), dtype=torch.int32, device=dev)
    nv.call("esc_multihop_fill", nv.ptr(c["node_ptr"]), nv.ptr(c["edge_ptr"]), nv.ptr(c["src"]), nv.ptr(c["dst"]), max(c["G"], 1), N, E,
            c["nmax"], k, nv.ptr(c["pair_ptr"]), nv.ptr(c["d1_ptr"]), M, nv.ptr(out[0]), nv.ptr(out[1]), nv.ptr(out[2]),
            nv.ptr(meta), nv.ptr(c["status"]), nv.stream())
    if _wants_check(check, sizes):
        _raise_status(c, "expand_multihop")
    in_ptr, in_meta = MultihopPlan._group_by_destination(meta, out[1], N)
    mei, dist = out[:2], out[2]
    plan = MultihopPlan(mei, dist, N, k, c["pair_ptr"], meta, in_ptr, in_meta, counts)
    plan.status = c["status"]
    return mei, dist, plan


def plan_of(multihop_edge_index, distance, num_nodes, k):
    """the MultihopPlan these tensors carry (expand_multihop, MultihopPlan.from_tensors) if it covers distances 1..k, or None:
    a pair of tensors that did not come from there, or a re-assigned `distance`, has none"""
    plan = getattr(multihop_edge_index, "_esc_multihop_plan", None)
    if plan is None or plan.k < int(k) or plan.distance is not distance or plan.num_nodes != int(num_nodes):
        return None
    return plan


def make_multihop_edges(data, k):
    """The reference's make_multihop_edges (modules/gine_operations.py:256-303): a shallow copy of `data` with
    `multihop_edge_index` and `distance`; the copy also carries the MultihopPlan.  Without known sizes the pair total is read
    back once (MultihopGraphStore.expand reads nothing back)."""
    out = copy.copy(data)
    object.__setattr__(out, "_store", dict(object.__getattribute__(data, "_store")))
    sizes = _tagged_sizes(data, "multihop", k)               # (sizes counted for another k are ignored: the total is read back)
    src = data
    if data["batch"] is None:                                # a single graph, as the reference's Data objects are
        src = copy.copy(out)
        object.__setattr__(src, "_store", dict(object.__getattribute__(out, "_store")))
        src.batch = torch.zeros(int(data.num_nodes), dtype=torch.int64, device=data.edge_index.device)
    mei, dist, plan = expand_multihop(src, k, sizes)
    out.multihop_edge_index, out.distance = mei, dist
    return out


class MultihopGraphStore(GraphStore):
    """The GINE+ run's split (expansion.GraphStore): the count pass at build time keeps, per graph, the number of pairs at every
    distance, so that `collate` + `expand` read nothing back."""
    kind = "multihop"
    _check_param = staticmethod(_check_k)
    k = property(lambda self: self.param)

    def _count_sizes(self):
        return multihop_sizes(self.graphs, self.k), None     # (no rooted subgraph, no rd limit)

    def expand(self, batch):
        """the batch with `multihop_edge_index`, `distance` and its MultihopPlan (in place: the batch is the store's own)"""
        mei, dist, plan = expand_multihop(batch, self.k, self.sizes_of(batch))
        batch.multihop_edge_index, batch.distance = mei, dist
        return batch
