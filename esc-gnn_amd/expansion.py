"""What the device-side expansions of a plain collated batch share: `subgraphs` (NGNN), `subgraphs2` (I2GNN) and
`multihop` (GINE+) each run one wave per root in a count pass and a fill pass, and keep their limits, their argument checks,
their two library calls and the assembly of their output.  Here, once: the host collate with its pointers, the count pass's
prologue, the status read-back, the sizes of a python list of graphs, what `sizes` tells the host before and after the count
pass, the pooling tag, the typed tag a store's batch carries its sizes in, and the store itself.
"""
import collections

import numpy as np
import torch

from .batch import Batch


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("esc_gnn_amd.subgraphs needs a HIP device (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _tag_segments(index, ptr, num_segments):
    """pooling over `index`, whose segment pointers are `ptr`: no rebuild, no read-back"""
    seg = ptr.to(torch.int32)
    v = index._version
    index._esc_seg = {(v, None): seg, (v, num_segments): seg}


def collate_graphs(data_list, device=None):
    """Host collate of plain graphs (x, edge_index, edge_attr, y): one concatenation per key and one copy to the device.
    The batch carries its int64 node / edge pointers (device and host) so that the expansion derives nothing."""
    dev = _device() if device is None else torch.device(device)
    G = len(data_list)
    if G == 0:
        raise ValueError("collate_graphs: empty list")
    n = np.array([int(d.num_nodes) for d in data_list], dtype=np.int64)
    e = np.array([int(d.edge_index.size(1)) for d in data_list], dtype=np.int64)
    node_ptr, edge_ptr = np.zeros(G + 1, dtype=np.int64), np.zeros(G + 1, dtype=np.int64)
    np.cumsum(n, out=node_ptr[1:])
    np.cumsum(e, out=edge_ptr[1:])
    ei = torch.cat([d.edge_index.reshape(2, -1).to(torch.int64) for d in data_list], dim=1)
    ei += torch.from_numpy(np.repeat(node_ptr[:-1], e)).view(1, -1)
    out = Batch()
    if data_list[0].x is not None:
        out.x = torch.cat([d.x for d in data_list], dim=0).to(dev)
    out.edge_index = ei.to(dev)
    if data_list[0].edge_attr is not None:
        out.edge_attr = torch.cat([d.edge_attr for d in data_list], dim=0).to(dev)
    if data_list[0].y is not None:
        out.y = torch.cat([d.y.reshape(-1) if d.y.dim() <= 1 else d.y for d in data_list], dim=0).to(dev)
    out.batch = torch.from_numpy(np.repeat(np.arange(G, dtype=np.int64), n)).to(dev)
    object.__setattr__(out, "_num_graphs", G)
    ptrs = torch.from_numpy(np.stack([node_ptr, edge_ptr])).to(dev)
    object.__setattr__(out, "_esc_sub_ptrs", (ptrs[0], ptrs[1], node_ptr, edge_ptr, int(n.max())))
    _tag_segments(out.batch, ptrs[0], G)
    return out


def _pointers(batch, G_known=None):
    """(node_ptr, edge_ptr int64 on the device, G, total_nodes, total_edges, max_nodes or None)"""
    tag = object.__getattribute__(batch, "__dict__").get("_esc_sub_ptrs")
    N, E = int(batch.batch.numel()), int(batch.edge_index.size(1))
    if tag is not None and int(tag[2][-1]) == N and int(tag[3][-1]) == E:
        return tag[0], tag[1], len(tag[2]) - 1, N, E, tag[4]
    from .plan import _csr
    b = batch.batch
    if b.device.type != "cuda":
        raise RuntimeError("esc_gnn_amd.subgraphs: the batch must be on the HIP device (batch.to(device)); there is no CPU fallback")
    G = int(G_known) if G_known is not None else (int(b[-1].item()) + 1 if N else 0)      # (a read-back without `sizes`)
    bad = torch.zeros(2, dtype=torch.int32, device=b.device)
    node_ptr = _csr(b, max(G, 1), want_perm=False, bad=bad[0:1])[0].to(torch.int64)
    edge_ptr = _csr(b[batch.edge_index[0]], max(G, 1), want_perm=False, bad=bad[1:2])[0].to(torch.int64)
    return node_ptr, edge_ptr, G, N, E, None                   # (a bad key shows up as ESC_ERANGE in the status of its graph)


def _count_prologue(batch, node_limit, who, G_known=None, max_nodes=None):
    """What every count pass starts from: the batch's pointers, the node count that sizes the LDS tables (the collate's, the
    caller's, or one read-back) refused beyond `node_limit`, the two edge rows and a cleared per-graph status."""
    node_ptr, edge_ptr, G, N, E, nmax = _pointers(batch, G_known)
    if nmax is None:
        nmax = max_nodes
    if nmax is None:
        nmax = int((node_ptr[1:] - node_ptr[:-1]).max().item()) if G else 1
    if nmax > node_limit:
        raise ValueError("%s: a graph of %d nodes exceeds the limit of %d nodes per graph" % (who, nmax, node_limit))
    ei = batch.edge_index
    return dict(node_ptr=node_ptr, edge_ptr=edge_ptr, G=G, N=N, E=E, nmax=max(int(nmax), 1), src=ei[0].contiguous(),
                dst=ei[1].contiguous(), status=torch.zeros(max(G, 1), dtype=torch.int32, device=ei.device))


def _raise_status(c, what, why_refused, why_counted=None, counted_ptr=None):
    """raise for the first graph whose status is set, naming what it hit: a graph the COUNT pass refused has zero-length
    output ranges in `counted_ptr`; one that was counted can only have failed in the fill pass"""
    st = c["status"].cpu()
    if bool((st != 0).any()):
        g = int(torch.nonzero(st)[0])
        why = why_refused
        if counted_ptr is not None:
            a, b = (int(v) for v in c["node_ptr"][g:g + 2].tolist())
            if a < b and int(counted_ptr[b]) > int(counted_ptr[a]):
                why = why_counted
        raise ValueError("%s: graph %d cannot be expanded (status %d): %s" % (what, g, int(st[g]), why))


def _sizes_of_list(per_batch, graphs, chunk, width):
    """(sizes [len(graphs), width()], largest) of a python list of graphs, collated `chunk` at a time;
    per_batch(batch) -> (sizes, largest) of one collated batch"""
    parts = [per_batch(collate_graphs(graphs[i:i + chunk])) for i in range(0, len(graphs), chunk)]
    sizes = torch.cat([p[0] for p in parts], dim=0) if parts else torch.zeros((0, width()), dtype=torch.int64)
    return sizes, max([p[1] for p in parts] or [0])


def _known_sizes(sizes, width, max_nodes, node_limit=None):
    """Before the count pass: (sizes as int64 [G, width] or None, its row count or None, max_nodes).  Column 0 bounds the node
    count of every graph (its roots' own rows are among them), which serves as `max_nodes` when the caller gave none."""
    if sizes is None:
        return None, None, max_nodes
    sizes = torch.as_tensor(sizes, dtype=torch.int64).reshape(-1, width)
    G_known = int(sizes.size(0))
    if max_nodes is None:
        max_nodes = int(sizes[:, 0].max()) if G_known else 1
        if node_limit is not None:
            max_nodes = min(node_limit, max_nodes)
    return sizes, G_known, max_nodes


def _below_2_31(what, text, *totals):
    if max(totals) >= 2 ** 31 - 1:
        raise ValueError("%s: %s: totals must stay below 2^31" % (what, text % totals))


def _column_totals(what, c, sizes, G_known, read_back):
    """After the count pass: the output totals, from the column sums of `sizes` or from the caller's one read-back"""
    if G_known is not None and G_known != c["G"]:
        raise ValueError("%s: sizes has %d rows for a batch of %d graphs" % (what, G_known, c["G"]))
    return [int(v) for v in (sizes.sum(dim=0).tolist() if sizes is not None else read_back())]


def _wants_check(check, sizes):
    """read the status back and raise?  By default only without `sizes`, where the call has synchronised anyway."""
    return sizes is None if check is None else check


# ---- the sizes a store's batch carries ---------------------------------------------------------------------------------------
SizeTag = collections.namedtuple("SizeTag", "kind param sizes")
_PARAM_OF_KIND = {"subgraph": "h", "subgraph2": "h", "multihop": "k"}


def _tagged_sizes(batch, kind, param, store=None):
    """The per-graph sizes of a store's batch when they were counted for this expansion and this h / k, else None.  For a
    `store` (its expand reads no status back) sizes counted for anything else are refused; without, they are ignored."""
    tag = object.__getattribute__(batch, "__dict__").get("_esc_sizes")
    if tag is None:
        return None
    if tag.kind == kind and tag.param == param:
        return tag.sizes
    if store is not None:
        raise ValueError("%s.expand: the batch carries the sizes of kind '%s' at %s=%d and cannot be expanded as kind '%s' at %s=%d"
                         % (type(store).__name__, tag.kind, _PARAM_OF_KIND[tag.kind], tag.param, kind, _PARAM_OF_KIND[kind], param))
    return None


class GraphStore(object):
    """A split of plain graphs for a baseline that expands on the device: host collate per batch (the device store keeps ESC
    bag tensors and does not take graphs without them) and the per-graph output sizes from ONE count pass at
    build time, so that no training step reads a size back.  A subclass names its `kind`, checks its parameter
    (`_check_param`), counts (`_count_sizes` -> sizes, largest single subgraph) and expands (`expand`)."""
    kind = None
    _check_param = staticmethod(int)

    def __init__(self, data_list, param, device=None):
        if len(data_list) == 0:
            raise ValueError("%s: empty dataset" % type(self).__name__)
        self.graphs, self.param = list(data_list), self._check_param(param)
        self.device = _device() if device is None else torch.device(device)
        self.sizes, self.largest_subgraph = self._count_sizes()

    def __len__(self):
        return len(self.graphs)

    def collate(self, graph_ids):
        ids = torch.as_tensor(graph_ids, dtype=torch.int64).reshape(-1)
        if ids.numel() == 0:
            raise ValueError("collate: empty batch")
        out = collate_graphs([self.graphs[i] for i in ids.tolist()], self.device)
        object.__setattr__(out, "_esc_sizes", SizeTag(self.kind, self.param, self.sizes[ids]))
        return out

    def sizes_of(self, batch):
        """the batch's sizes for `expand`; a batch of another store's kind or parameter is refused here, before any launch"""
        return _tagged_sizes(batch, self.kind, self.param, self)
