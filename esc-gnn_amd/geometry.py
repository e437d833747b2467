"""The `Distance` transform of the QM9 run on the device (csrc/geometry.hip, esc_edge_distance).

Restates the reference's distance.py:5-47: the Euclidean length of every edge from `pos` (row = edge_index[0],
col = edge_index[1], d = |pos[col] - pos[row]|, or the sum of squares when `squared`), divided by the graph's own maximum
(or by `max_value`), appended to the existing edge attributes (or replacing them with `cat=False`), optionally followed by
the relative position pos[col] - pos[row].  The reference applies it per graph on the CPU on every dataset access
(run_qm9.py:226-231); `edge_distance_many` does a whole list of graphs with one launch, once.
"""
import torch

from . import _native as nv


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("esc_gnn_amd.geometry needs a HIP device (MI355X); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def edge_distance_arrays(pos, src, dst, node_ptr, edge_ptr, attr=None, norm=True, squared=False, relative_pos=False,
                         max_value=None, cat=True):
    """Low-level call on device arrays: pos float32 [N, 3] (rows may be strided), src / dst int64 [E] graph-local ids,
    node_ptr / edge_ptr int64 [G+1], attr None or float32 [E, A].  Returns float32 [E, A + 1 (+3)] — [attr | d | rel] —
    raising ValueError for a node id outside its graph."""
    dev = pos.device
    if pos.dim() != 2 or pos.size(1) != 3 or pos.dtype != torch.float32:
        raise ValueError("edge_distance: pos must be float32 [N, 3], got %s %s" % (pos.dtype, tuple(pos.shape)))
    if pos.stride(1) != 1 or (pos.size(0) > 1 and pos.stride(0) < 3):
        pos = pos.contiguous()
    ld_pos = pos.stride(0) if pos.size(0) > 1 else 3
    G, N, E = node_ptr.numel() - 1, pos.size(0), src.numel()
    if attr is not None and cat:
        attr = attr.view(-1, 1) if attr.dim() == 1 else attr
        if attr.size(0) != E:
            raise ValueError("edge_distance: %d attribute rows for %d edges" % (attr.size(0), E))
    A = attr.size(1) if (attr is not None and cat) else 0
    W = A + 1 + (3 if relative_pos else 0)
    out = torch.empty((E, W), dtype=torch.float32, device=dev)
    if A:
        out[:, :A] = attr
    status = torch.zeros(max(G, 1), dtype=torch.int32, device=dev)
    nv.call("esc_edge_distance", nv.ptr(pos), ld_pos, nv.ptr(src), nv.ptr(dst), nv.ptr(node_ptr), nv.ptr(edge_ptr), G, N, E,
            int(bool(norm)), int(bool(squared)), int(bool(relative_pos)), int(max_value is not None),
            float(max_value if max_value is not None else 0.0), nv.ptr(out), W, A, nv.ptr(status), nv.stream())
    st = status.cpu()
    if bool((st != 0).any()):
        g = int(torch.nonzero(st)[0])
        raise ValueError("edge_distance: graph %d has a node id or a range outside its arrays" % g)
    return out


def _num_nodes(d):
    return int(d.pos.size(0))


def edge_distance_many(data_list, norm=True, squared=False, relative_pos=False, max_value=None, cat=True):
    """`Distance(norm, max_value, cat, relative_pos, squared)` over a list of Data with one launch: every graph's
    `edge_attr` becomes [edge_attr | d (| pos[col] - pos[row])] (the graphs are edited in place, like the reference's
    transform, and returned).  A graph without edges keeps an empty attribute of the new width."""
    dev = _device()
    G = len(data_list)
    if G == 0:
        return data_list
    for d in data_list:
        if d.pos is None:
            raise ValueError("edge_distance_many: a graph has no `pos`")
    n_t = torch.tensor([_num_nodes(d) for d in data_list], dtype=torch.int64)
    m_t = torch.tensor([int(d.edge_index.size(1)) for d in data_list], dtype=torch.int64)
    node_ptr = torch.zeros(G + 1, dtype=torch.int64)
    edge_ptr = torch.zeros(G + 1, dtype=torch.int64)
    node_ptr[1:] = torch.cumsum(n_t, 0)
    edge_ptr[1:] = torch.cumsum(m_t, 0)
    pos = torch.cat([d.pos.reshape(-1, 3).float().cpu() for d in data_list]).contiguous().to(dev)
    ei = torch.cat([d.edge_index.reshape(2, -1).to(torch.int64).cpu() for d in data_list], dim=1)
    with_attr = [d.edge_attr is not None for d in data_list]
    if cat and any(with_attr) and not all(with_attr):
        raise ValueError("edge_distance_many: some graphs carry edge_attr and some do not")
    attr = None
    if cat and all(with_attr):
        rows = [d.edge_attr.view(-1, 1) if d.edge_attr.dim() == 1 else d.edge_attr for d in data_list]
        kind = rows[0].dtype
        attr = torch.cat([r.float().cpu() for r in rows]).to(dev)
    out = edge_distance_arrays(pos, ei[0].contiguous().to(dev), ei[1].contiguous().to(dev), node_ptr.to(dev), edge_ptr.to(dev),
                               attr, norm, squared, relative_pos, max_value, cat).cpu()
    for g, d in enumerate(data_list):
        piece = out[int(edge_ptr[g]):int(edge_ptr[g + 1])].clone()
        if attr is not None and kind != torch.float32 and not relative_pos:
            piece = piece.to(kind)                     # dist.type_as(pseudo), distance.py:41
        d.edge_attr = piece.to(d.edge_index.device)
    return data_list


class Distance(object):
    """The reference's transform (same constructor), for one graph, on the device."""

    def __init__(self, norm=True, max_value=None, cat=True, relative_pos=False, squared=False):
        self.norm, self.max, self.cat, self.relative_pos, self.squared = norm, max_value, cat, relative_pos, squared

    def __call__(self, data):
        if type(data) == dict:
            return {key: self.__call__(data_) for key, data_ in data.items()}
        if "original_edge_index" in data:
            raise NotImplementedError("Distance: original_edge_index belongs to the k-GNN baselines (distance.py:49-63)")
        return edge_distance_many([data], self.norm, self.squared, self.relative_pos, self.max, self.cat)[0]

    def __repr__(self):
        return "{}(norm={}, max_value={})".format(self.__class__.__name__, self.norm, self.max)
