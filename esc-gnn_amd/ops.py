"""Autograd bindings of the HIP hot-path kernels (ctypes -> libescgnn_hip.so, C ABI in
include/escgnn_hip.h).  Each Function names the reference call site it replaces.  There is no
CPU or PyTorch fallback: a CPU tensor raises.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _native as nv


def _dev(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("esc_gnn_amd: the hot path runs on the HIP device only (got a %s tensor); "
                               "there is no CPU fallback" % t.device)
        if t.dtype != torch.float32:
            raise TypeError("esc_gnn_amd: expected float32, got %s" % t.dtype)


def _on(dev, *tensors):
    """Every pointer handed to a kernel must be a DEVICE pointer on the same GPU: an index tensor left on the host
    would be dereferenced by the GPU and fault.  Raise instead."""
    for t in tensors:
        if t is not None and t.device != dev:
            raise RuntimeError("esc_gnn_amd: tensor on %s but the kernel runs on %s — move the batch to the device "
                               "first (data.to(device))" % (t.device, dev))


def _plan_on(dev, plan, *fields):
    for f in fields:
        _on(dev, getattr(plan, f))


def _views_on(dev, plan):
    """both sorted edge views of the plan, as the aggregate kernels walk them, on the operands' device"""
    _plan_on(dev, plan, "in_ptr", "in_edge", "in_src", "out_ptr", "out_edge", "out_dst")


def _edge_ptr(E):
    """nv.ptr for what exists only where the batch has edges: a batch without any hands the kernels NULL instead"""
    return nv.ptr if E else (lambda t: None)


def _width_limit(op, C, limit):
    """the width rule of the lane-group kernels, refused before anything is launched: a multiple of 4 from 4 up to `limit`"""
    if C % 4 or not 4 <= C <= limit:
        raise ValueError("%s: width %d: the kernels take a multiple of 4 with 4 <= C <= %d" % (op, C, limit))


def _rows(t, width=None):
    """The row-operand rule, stated once: a 2-D tensor (of `width` columns when one is required) as a kernel reads it, and its
    leading dimension.  Unit inner stride with rows that do not overlap is taken in place (a column slice of wider rows keeps
    its row stride); anything else is made contiguous.  PyTorch leaves stride(0) of a tensor of at most one row arbitrary, so
    such a tensor is re-strided to (width, 1) - a view, no copy.  The tensor returned therefore has stride(0) == ld, and
    _rows of it returns it unchanged: every launch, forward and backward, takes the pair from here."""
    if width is None:
        if t.dim() != 2:
            raise ValueError("expected a 2-D tensor, got shape %s" % (tuple(t.shape),))
    elif t.dim() != 2 or t.size(1) != width:
        raise ValueError("expected a [N, %d] tensor, got shape %s" % (width, tuple(t.shape)))
    M, C = t.shape
    if t.stride(1) != 1 or (M > 1 and t.stride(0) < C):
        t = t.contiguous()
    if M <= 1 and t.stride() != (C, 1):
        t = t.as_strided((M, C), (C, 1))
    return t, t.stride(0)


def _empty(dev, *shape):
    """an uninitialised fp32 buffer on `dev`"""
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _zeros(dev, *shape):
    return torch.zeros(shape, dtype=torch.float32, device=dev)


def _cached(t, attr, key, build):
    """build() once per (tensor, its _version, key): the value rides on the tensor under `attr`, so everything that looks the
    same index tensor up again (every layer, both directions) shares it, and an in-place edit of the tensor drops it."""
    key = (t._version, key)
    hit = getattr(t, attr, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    value = build()
    setattr(t, attr, (key, value))
    return value


def _bag_rows(table, row_ptr, idx32, ones, n_out):
    """esc_bag_fwd: out[r] = sum of table[idx32[j]] * ones[j] over the entries j of row r"""
    table = table.contiguous()
    H = table.size(1)
    out = _empty(table.device, n_out, H)
    nv.call("esc_bag_fwd", nv.ptr(table), H, nv.ptr(row_ptr), nv.ptr(idx32), nv.ptr(ones), n_out, nv.ptr(out), H, nv.stream())
    return out


def _bag_table_grad(g, H, col_ptr, c_row, c_val, c_col, nnz, rows, bag_rows=None):
    """The table gradient [rows, H] of a bag launch from the CSC grouping of its nnz entries (deterministic segmented sum) with
    its scratch: esc_bag_bwd_table, or esc_bag_bwd_table_rows when the plan's bag row count is given."""
    g, ld = _rows(g)
    dtable = _empty(g.device, rows, H)
    scratch = _empty(g.device, max(1, nv.lib().esc_bag_bwd_scratch(nnz, H)))
    tail = (rows,) if bag_rows is None else (rows, bag_rows, 0)
    nv.call("esc_bag_bwd_table" if bag_rows is None else "esc_bag_bwd_table_rows", nv.ptr(g), ld, H, nv.ptr(col_ptr), nv.ptr(c_row),
            nv.ptr(c_val), nv.ptr(c_col), nnz, *tail, nv.ptr(dtable), nv.ptr(scratch), nv.stream())
    return dtable


class _Bag(Function):
    """z_emb = global_add_pool(z_initial.weight[pos_index] * pos_enc[:,None], pos_batch)
    (run_graphcount.py:155) as a CSR SpMM; backward = deterministic CSC segmented sum."""

    @staticmethod
    def forward(ctx, table, plan):
        _dev(table)
        table = table.contiguous()
        if plan.row_ptr is None:
            raise ValueError("batch has no pos_enc/pos_index/pos_batch")
        _plan_on(table.device, plan, "row_ptr", "bag_idx", "bag_val", "col_ptr", "col_row", "col_val", "col_col")
        E, H = plan.num_edges, table.size(1)
        out = _empty(table.device, E, H)
        nv.call("esc_bag_fwd_rows", nv.ptr(table), table.size(0), H, nv.ptr(plan.row_ptr), nv.ptr(plan.bag_idx),
                nv.ptr(plan.bag_val), E, nv.ptr(out), H, 0, None, nv.stream())
        ctx.plan, ctx.shape = plan, tuple(table.shape)
        return out

    @staticmethod
    def backward(ctx, dz):
        plan = ctx.plan
        rows, H = ctx.shape
        return _bag_table_grad(dz, H, plan.col_ptr, plan.col_row, plan.col_val, plan.col_col, plan.nnz, rows, plan.num_edges), None


def esc_bag(table, plan):
    return _Bag.apply(table, plan)


class _Aggregate(Function):
    """out = sum_{k: dst_k=i} relu(x[src_k] (+ e_k)) (+ (1+eps) x_i).  With e and eps it is PyG GINEConv propagate + self term
    (run_graphcount.py:161,169; gine_conv_layer.py:56-84); with eps None and e optional, the per-distance message sum of
    GINEPLUS / NAIVEGINEPLUS (modules/gine_operations.py:306-362).  `gine` selects the shape check of the first."""

    @staticmethod
    def forward(ctx, x, e, eps, plan, gine):
        _dev(x, e, eps)
        _on(x.device, e, eps)
        _views_on(x.device, plan)
        x, ldx = _rows(x)
        e, lde = _rows(e) if (gine or e is not None) else (None, 0)
        N, C = x.shape
        if gine and (e.shape != (plan.num_edges, C) or N != plan.num_nodes):
            raise ValueError("aggregate: x %s / e %s do not match the batch (N=%d, E=%d)"
                             % (tuple(x.shape), tuple(e.shape), plan.num_nodes, plan.num_edges))
        if not gine and e is not None and e.shape != (plan.num_edges, C):
            raise ValueError("neighbour_sum: edge term %s does not match %d edges x %d" % (tuple(e.shape), plan.num_edges, C))
        out = _empty(x.device, N, C)
        nv.call("esc_gine_aggregate_fwd", nv.ptr(x), ldx, nv.ptr(e), lde, nv.ptr(plan.in_ptr),
                nv.ptr(plan.in_edge), nv.ptr(plan.in_src), nv.ptr(eps), N, C, nv.ptr(out), C, nv.stream())
        ctx.save_for_backward(x, e, eps)
        ctx.plan = plan
        return out

    @staticmethod
    def backward(ctx, g):
        x, e, eps = ctx.saved_tensors
        plan = ctx.plan
        x, ldx = _rows(x)
        e, lde = _rows(e) if e is not None else (None, 0)
        g, ldg = _rows(g)
        N, C = x.shape
        need_dx, need_de, need_eps = ctx.needs_input_grad[:3]
        d_e = _empty(x.device, *e.shape) if e is not None else None
        dx = _empty(x.device, N, C) if need_dx else None
        slots = int(nv.lib().esc_gine_aggregate_bwd_deps_slots(C)) if need_eps else 0    # partial dot products per row (see the header)
        part = _empty(x.device, N * slots) if need_eps else None
        nv.call("esc_gine_aggregate_bwd", nv.ptr(x), ldx, nv.ptr(e), lde, nv.ptr(g), ldg,
                nv.ptr(plan.out_ptr), nv.ptr(plan.out_edge), nv.ptr(plan.out_dst), nv.ptr(eps), N, C,
                nv.ptr(d_e), C if d_e is not None else 0, nv.ptr(dx), C, 0, nv.ptr(part), nv.stream())
        deps = None
        if need_eps:
            deps = _empty(x.device, 1)
            nv.call("esc_reduce_sum", nv.ptr(part), N * slots, nv.ptr(deps), nv.stream())
        return dx, (d_e if need_de else None), deps, None, None


def gine_aggregate(x, e, eps, plan):
    return _Aggregate.apply(x, e, eps, plan, True)


def neighbour_sum(x, e, plan):
    return _Aggregate.apply(x, e, None, plan, False)


def gated_gcn_max_channels():
    """the widest row esc_gated_gcn_fwd / _bwd take (a multiple of 4 from 4 up to this)"""
    return int(nv.lib().esc_gated_gcn_max_channels())


class _GatedGCN(Function):
    """e_ij = Dx_i + Ex_j + Ce_k, out_i = Ax_i + sum_k sigmoid(e_ij) Bx_j / (sum_k sigmoid(e_ij) + 1e-6) and e_ij itself: message,
    aggregate and update of the reference's GatedGCNLayer (GraphGPS/graphgps/layer/gatedgcn_layer.py:67-70,90-136) in one
    launch, their backward in two (csrc/gatedgcn.hip).  Kept for the backward: e_out and out (outputs anyway), den, Ax, Bx."""

    @staticmethod
    def forward(ctx, Ax, Bx, Dx, Ex, Ce, plan):
        _dev(Ax, Bx, Dx, Ex, Ce)
        _on(Ax.device, Bx, Dx, Ex, Ce)
        _views_on(Ax.device, plan)
        (Ax, lda), (Bx, ldb), (Dx, ldd), (Ex, lde), (Ce, ldc) = (_rows(t) for t in (Ax, Bx, Dx, Ex, Ce))
        N, C = Ax.shape
        E = plan.num_edges
        _width_limit("gated_gcn_aggregate", C, gated_gcn_max_channels())
        if any(tuple(t.shape) != (N, C) for t in (Bx, Dx, Ex)) or Ce.size(1) != C or N != plan.num_nodes:
            raise ValueError("gated_gcn_aggregate: Ax %s, Bx %s, Dx %s, Ex %s, Ce %s must share one width and the batch's %d nodes"
                             % (tuple(Ax.shape), tuple(Bx.shape), tuple(Dx.shape), tuple(Ex.shape), tuple(Ce.shape), plan.num_nodes))
        if Ce.size(0) != E:
            raise ValueError("gated_gcn_aggregate: Ce has %d rows, the batch has %d edges" % (Ce.size(0), E))
        dev = Ax.device
        out, e_out, den = _empty(dev, N, C), _empty(dev, E, C), _empty(dev, N, C)
        edge = _edge_ptr(E)
        nv.call("esc_gated_gcn_fwd", nv.ptr(Ax), lda, nv.ptr(Bx), ldb, nv.ptr(Dx), ldd, nv.ptr(Ex), lde, edge(Ce), ldc,
                nv.ptr(plan.in_ptr), edge(plan.in_edge), edge(plan.in_src), N, E, C, nv.ptr(out), C, edge(e_out), C, nv.ptr(den),
                nv.stream())
        ctx.save_for_backward(Ax, Bx, out, e_out, den)
        ctx.plan = plan
        ctx.set_materialize_grads(False)         # an unused output's gradient arrives as None: g_e NULL, no zero rows are made
        return out, e_out

    @staticmethod
    def backward(ctx, g_out, g_e):
        Ax, Bx, out, e_out, den = ctx.saved_tensors
        plan = ctx.plan
        N, C = Ax.shape
        E, dev = plan.num_edges, Ax.device
        (Ax, lda), (Bx, ldb) = _rows(Ax), _rows(Bx)
        g_out, ldg = _rows(g_out if g_out is not None else _zeros(dev, N, C))
        g_e, ldge = _rows(g_e) if g_e is not None else (None, 0)
        d_Ce, d_Dx, d_Ex, d_Bx = _empty(dev, E, C), _empty(dev, N, C), _empty(dev, N, C), _empty(dev, N, C)
        edge = _edge_ptr(E)
        nv.call("esc_gated_gcn_bwd", nv.ptr(g_out), ldg, edge(g_e), ldge, edge(e_out), C, nv.ptr(den), nv.ptr(out), C, nv.ptr(Ax), lda,
                nv.ptr(Bx), ldb, nv.ptr(plan.in_ptr), edge(plan.in_edge), edge(plan.in_src), nv.ptr(plan.out_ptr),
                edge(plan.out_edge), edge(plan.out_dst), N, E, C, edge(d_Ce), C, nv.ptr(d_Dx), C, nv.ptr(d_Ex), C, nv.ptr(d_Bx), C,
                nv.stream())
        return g_out, d_Bx, d_Dx, d_Ex, d_Ce, None


def gated_gcn_aggregate(Ax, Bx, Dx, Ex, Ce, plan):
    """(out [N, C], e_out [E, C]) of the GatedGCN gate over the batch's plan; differentiable in all five operands and through
    both outputs.  ValueError: a width outside the kernels' limits, operands of different widths, Ce rows != plan.num_edges."""
    return _GatedGCN.apply(Ax, Bx, Dx, Ex, Ce, plan)


def pna_max_channels():
    """the widest row esc_pna_aggregate_fwd / _bwd take (a multiple of 4 from 4 up to this)"""
    return int(nv.lib().esc_pna_max_channels())


class _PNAAggregate(Function):
    """m_k = (P[i] + Q[j]) + R[k] over the edges k = (j -> i), and mean | max | sum of the messages of every node's in-edges in
    one [N, 3C] tensor: message and aggregate of PyG's PNAConv with aggregators mean / max / sum and the identity scaler in
    one launch, their backward in two (csrc/pna.hip).  Kept for the backward: arg [N, C] int32, the edge position of every
    maximum - nothing of size [E, C]."""

    @staticmethod
    def forward(ctx, P, Q, R, plan):
        _dev(P, Q, R)
        _on(P.device, Q, R)
        _views_on(P.device, plan)
        (P, ldp), (Q, ldq), (R, ldr) = (_rows(t) for t in (P, Q, R))
        N, C = P.shape
        E = plan.num_edges
        _width_limit("pna_aggregate", C, pna_max_channels())
        if tuple(Q.shape) != (N, C) or R.size(1) != C or N != plan.num_nodes:
            raise ValueError("pna_aggregate: P %s, Q %s, R %s must share one width and the batch's %d nodes"
                             % (tuple(P.shape), tuple(Q.shape), tuple(R.shape), plan.num_nodes))
        if R.size(0) != E:
            raise ValueError("pna_aggregate: R has %d rows, the batch has %d edges" % (R.size(0), E))
        dev = P.device
        agg, arg = _empty(dev, N, 3 * C), torch.empty((N, C), dtype=torch.int32, device=dev)
        edge = _edge_ptr(E)
        nv.call("esc_pna_aggregate_fwd", nv.ptr(P), ldp, nv.ptr(Q), ldq, edge(R), ldr, nv.ptr(plan.in_ptr), edge(plan.in_edge),
                edge(plan.in_src), N, E, C, nv.ptr(agg), 3 * C, nv.ptr(arg), nv.stream())
        ctx.save_for_backward(arg)
        ctx.plan = plan
        return agg

    @staticmethod
    def backward(ctx, g):
        arg, = ctx.saved_tensors
        plan = ctx.plan
        N, C = arg.shape
        E, dev = plan.num_edges, arg.device
        g, ldg = _rows(g)
        d_R, d_P, d_Q = _empty(dev, E, C), _empty(dev, N, C), _empty(dev, N, C)
        edge = _edge_ptr(E)
        nv.call("esc_pna_aggregate_bwd", nv.ptr(g), ldg, nv.ptr(arg), nv.ptr(plan.in_ptr), edge(plan.in_edge), edge(plan.in_src),
                nv.ptr(plan.out_ptr), edge(plan.out_edge), edge(plan.out_dst), N, E, C, edge(d_R), C, nv.ptr(d_P), C, nv.ptr(d_Q), C,
                nv.stream())
        return d_P, d_Q, d_R, None


def pna_aggregate(P, Q, R, plan):
    """agg [N, 3C] = mean | max | sum of the messages (P[i] + Q[j]) + R[k] over every node's in-edges, in this column order: one
    tensor, so the layer joins it to x with one cat and never cats the aggregates.  Differentiable in all three operands; the
    gradient of a maximum goes to the lowest edge position that holds it.  ValueError: a width outside the kernels' limits,
    operands of different widths, R rows != plan.num_edges."""
    return _PNAAggregate.apply(P, Q, R, plan)


class _Linear(Function):
    """torch.nn.Linear on the fp32 matrix cores (every Linear of run_graphcount.py:54-121,183-189)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _dev(x, weight, bias)
        _on(x.device, weight, bias)
        x, ldx = _rows(x)
        weight = weight.contiguous()
        M, K = x.shape
        N = weight.size(0)
        if weight.size(1) != K:
            raise ValueError("linear: x %s vs weight %s" % (tuple(x.shape), tuple(weight.shape)))
        y = _empty(x.device, M, N)
        nv.call("esc_linear_fwd", nv.ptr(x), ldx, nv.ptr(weight), K, nv.ptr(bias), None, None, M, N, K,
                nv.ptr(y), N, None, nv.stream())
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        x, ldx = _rows(x)
        dy, ldy = _rows(dy)
        M, K = x.shape
        N, dev = weight.size(0), x.device
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _empty(dev, M, K)
            nv.call("esc_linear_bwd_input", nv.ptr(dy), ldy, nv.ptr(weight), K, M, N, K, nv.ptr(dx), K, 0,
                    nv.stream())
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dw = _empty(dev, N, K)
            db = _empty(dev, N) if ctx.has_bias else None
            if M == 0:
                dw.zero_()
                if db is not None:
                    db.zero_()
            else:
                slabs = _empty(dev, nv.lib().esc_linear_bwd_weight_scratch(M, N, K))
                nv.call("esc_linear_bwd_weight", nv.ptr(dy), ldy, nv.ptr(x), ldx, None, None, M, N, K,
                        nv.ptr(dw), K, nv.ptr(db), nv.ptr(slabs), nv.stream())
        return dx, dw, db


def linear(x, weight, bias=None):
    return _Linear.apply(x, weight, bias)


def _bn_stats(x, ldx, eps, momentum, running_mean, running_var, s, launch=True):
    """esc_bn_stats with its buffers -> (mean, invstd, scratch); the launch also updates the running statistics it is given"""
    M, C = x.shape
    mean, invstd, scratch = _empty(x.device, C), _empty(x.device, C), _empty(x.device, nv.lib().esc_bn_scratch(C))
    if launch:
        nv.call("esc_bn_stats", nv.ptr(x), ldx, M, C, float(eps), float(momentum), nv.ptr(mean), nv.ptr(invstd),
                nv.ptr(running_mean), nv.ptr(running_var), None, None, None, None, nv.ptr(scratch), s)
    return mean, invstd, scratch


def _bn_apply(x, ldx, mean, invstd, gamma, beta, act, s):
    """esc_bn_apply -> y [M, C] (nothing is launched for no rows)"""
    M, C = x.shape
    y = _empty(x.device, M, C)
    if M > 0:
        nv.call("esc_bn_apply", nv.ptr(x), ldx, M, C, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta),
                int(act), nv.ptr(y), C, s)
    return y


def _bn_bwd_operands(x, y, dy, mean, invstd, gamma, beta, act):
    """The thirteen leading arguments that esc_bn_bwd, esc_bn_bwd_sums and esc_bn_bwd_apply share, and the row operands they
    point into (the caller holds these until the launches are queued): (x, dy, arguments)."""
    x, ldx = _rows(x)
    dy, ldg = _rows(dy)
    M, C = x.shape
    return x, dy, (nv.ptr(x), ldx, nv.ptr(y), C, nv.ptr(dy), ldg, M, C, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta),
                   int(act))          # act: 0 none, 1 relu, 2 elu


def _bn_bwd_sums(x, head, sums, scratch, s):
    """esc_bn_bwd_sums into `sums` [2C] -> (dgamma, dbeta), which stay zero for no rows"""
    M, C = x.shape
    dgamma, dbeta = _zeros(x.device, C), _zeros(x.device, C)
    if M > 0:
        nv.call("esc_bn_bwd_sums", *head, nv.ptr(sums), nv.ptr(dgamma), nv.ptr(dbeta), nv.ptr(scratch), s)
    return dgamma, dbeta


def _bn_bwd_apply(x, head, coef, s):
    """esc_bn_bwd_apply with the batch terms `coef` [2C] -> dx [M, C]"""
    M, C = x.shape
    dx = _empty(x.device, M, C)
    if M > 0:
        nv.call("esc_bn_bwd_apply", *head, nv.ptr(coef), nv.ptr(dx), C, s)
    return dx


class _BatchNormAct(Function):
    """Training-mode BatchNorm1d (+ optional fused ReLU): batch statistics, running-stat update and
    normalisation (run_graphcount.py:55-60,66-72,80-87,115)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu):
        _dev(x, gamma, beta)
        _on(x.device, gamma, beta, running_mean, running_var)
        x, ldx = _rows(x)
        if x.size(0) <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(x.shape),))
        s = nv.stream()
        mean, invstd, scratch = _bn_stats(x, ldx, eps, momentum, running_mean, running_var, s)
        y = _bn_apply(x, ldx, mean, invstd, gamma, beta, relu, s)
        ctx.save_for_backward(x, y if relu else None, gamma, mean, invstd)
        ctx.relu, ctx.scratch = int(relu), scratch        # 0 none, 1 relu, 2 elu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, mean, invstd = ctx.saved_tensors
        x, dy, head = _bn_bwd_operands(x, y, dy, mean, invstd, gamma, None, ctx.relu)
        M, C = x.shape
        dx, dgamma, dbeta = _empty(x.device, M, C), _empty(x.device, C), _empty(x.device, C)
        nv.call("esc_bn_bwd", *head, nv.ptr(dx), C, nv.ptr(dgamma), nv.ptr(dbeta), nv.ptr(ctx.scratch), nv.stream())
        return dx, (dgamma if gamma is not None else None), (dbeta if gamma is not None else None), None, None, None, None, None


def batch_norm_act(x, gamma, beta, running_mean, running_var, eps, momentum, relu):
    return _BatchNormAct.apply(x, gamma, beta, running_mean, running_var, eps, momentum, relu)


class _SyncBatchNormAct(Function):
    """BatchNorm1d(train) whose batch statistics span all ranks of a process group (what makes graph-sharded
    data parallelism reproduce the single-device forward).  Forward: local (n, mean, M2) from esc_bn_stats, one
    all_gather of 2C+1 doubles, Chan merge, esc_bn_apply with the global statistics.  Backward: local column sums
    (esc_bn_bwd_sums), one all-reduce of 2C floats, esc_bn_bwd_apply with sums / N_global.  The incoming gradient must
    belong to ONE objective shared by the ranks (sum-form loss, `l1_loss(..., denom=1)` + `FlatBucket.all_reduce_sum`)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, relu, group):
        import torch.distributed as dist
        _dev(x, gamma, beta)
        _on(x.device, gamma, beta, running_mean, running_var)
        x, ldx = _rows(x)
        M, C = x.shape
        s = nv.stream()
        pack = torch.zeros(2 * C + 1, dtype=torch.float64, device=x.device)
        pack[0] = M
        mean, invstd, scratch = _bn_stats(x, ldx, eps, momentum, None, None, s, launch=M > 1)     # the local statistics
        if M > 1:
            pack[1:C + 1] = mean.double()
            pack[C + 1:] = (1.0 / invstd.double().pow(2) - float(eps)).clamp_min(0.0) * M        # M2 = var * n
        elif M == 1:
            pack[1:C + 1] = x[0].double()
        world = dist.get_world_size(group)
        gathered = [torch.empty_like(pack) for _ in range(world)]
        dist.all_gather(gathered, pack, group=group)
        n, mu, m2 = gathered[0][0].clone(), gathered[0][1:C + 1].clone(), gathered[0][C + 1:].clone()
        for g in gathered[1:]:                                   # Chan merge in rank order (identical on every rank)
            nb, mub, m2b = g[0], g[1:C + 1], g[C + 1:]
            tot = n + nb
            delta = mub - mu
            mu = mu + delta * (nb / tot)
            m2 = m2 + m2b + delta * delta * (n * nb / tot)
            n = tot
        if float(n) <= 1:
            raise ValueError("Expected more than 1 value per channel when training (over all ranks)")
        var = m2 / n
        mean = mu.float()
        invstd = torch.rsqrt(var + float(eps)).float()
        if running_mean is not None:
            running_mean.mul_(1.0 - momentum).add_(mean, alpha=momentum)
            running_var.mul_(1.0 - momentum).add_((m2 / (n - 1)).float(), alpha=momentum)
        y = _bn_apply(x, ldx, mean, invstd, gamma, beta, relu, s)
        ctx.save_for_backward(x, y if relu else None, gamma, mean, invstd)
        ctx.relu, ctx.scratch, ctx.group, ctx.n_global = int(relu), scratch, group, float(n)
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        x, y, gamma, mean, invstd = ctx.saved_tensors
        x, dy, head = _bn_bwd_operands(x, y, dy, mean, invstd, gamma, None, ctx.relu)
        s = nv.stream()
        sums = _zeros(x.device, 2 * x.size(1))
        dgamma, dbeta = _bn_bwd_sums(x, head, sums, ctx.scratch, s)
        dist.all_reduce(sums, group=ctx.group)
        dx = _bn_bwd_apply(x, head, sums / ctx.n_global, s)
        return dx, dgamma, dbeta, None, None, None, None, None, None


def sync_batch_norm_act(x, gamma, beta, running_mean, running_var, eps, momentum, relu, group=None):
    return _SyncBatchNormAct.apply(x, gamma, beta, running_mean, running_var, eps, momentum, relu, group)


class _BnEvalAct(Function):
    """Inference-mode BatchNorm (+ fused activation) on the RUNNING statistics, differentiable: y = act(x*scale + shift)
    with scale = gamma / sqrt(running_var + eps), shift = beta - running_mean*scale (model.eval() with gradients enabled:
    fine-tuning with frozen statistics, input-gradient probes).  Backward on the BatchNorm kernels with the batch terms
    switched off: column sums give d(gamma), d(beta); dx = scale * dy * act'(.)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, relu):
        _dev(x)
        _on(x.device, gamma, beta, running_mean, running_var)
        x, ldx = _rows(x)
        M, C = x.shape
        dev = x.device
        scale, shift = _empty(dev, C), _empty(dev, C)
        s = nv.stream()
        nv.call("esc_bn_eval_coef", nv.ptr(running_mean), nv.ptr(running_var), nv.ptr(gamma), nv.ptr(beta), float(eps), C,
                nv.ptr(scale), nv.ptr(shift), s)
        y = _empty(dev, M, C)
        if M > 0:
            nv.call("esc_affine_act", nv.ptr(x), ldx, M, C, nv.ptr(scale), nv.ptr(shift), int(relu), nv.ptr(y), C, s)
        ctx.save_for_backward(x, y if relu else None, gamma, beta, running_mean, running_var)
        ctx.relu, ctx.eps = int(relu), float(eps)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, beta, rm, rv = ctx.saved_tensors
        dev, C = x.device, x.size(1)
        s = nv.stream()
        invstd, unused = _empty(dev, C), _empty(dev, C)
        nv.call("esc_bn_eval_coef", nv.ptr(rm), nv.ptr(rv), None, None, ctx.eps, C, nv.ptr(invstd), nv.ptr(unused), s)
        x, dy, head = _bn_bwd_operands(x, y, dy, rm, invstd, gamma, beta, ctx.relu)
        dgamma, dbeta = _bn_bwd_sums(x, head, _empty(dev, 2 * C), _empty(dev, nv.lib().esc_bn_scratch(C)), s)
        dx = _bn_bwd_apply(x, head, _zeros(dev, 2 * C), s)                  # no batch-statistics terms in eval mode
        return dx, (dgamma if gamma is not None else None), (dbeta if beta is not None else None), None, None, None, None


def bn_eval_act(x, gamma, beta, running_mean, running_var, eps, relu):
    """Inference-mode BatchNorm (+activation) with running statistics; differentiable (see _BnEvalAct)."""
    return _BnEvalAct.apply(x, gamma, beta, running_mean, running_var, eps, relu)


# name -> (entry point, the divisor is M unless `denom` is given (else the entry point counts: 0), arguments between the divisor
# and the outputs, targets cast with .float())
_LOSS_HEADS = {"l1_loss": ("esc_l1_loss", True, (1.0,), False),
               "mse_loss": ("esc_mse_loss", True, (1.0,), False),
               "bce_with_logits_loss": ("esc_bce_logits_loss", False, (), True)}


class _ElementwiseLoss(Function):
    """The three elementwise loss heads: one launch leaves the loss and d loss / d pred, the backward scales the latter and
    returns it in pred's shape.  `denom` overrides the divisor (the global count under graph-sharded data parallelism).
      l1_loss: torch.nn.L1Loss()(pred, y) (run_graphcount.py:500-501)
      mse_loss: F.mse_loss(pred, y) (reference run_qm9.py:348), squares summed in fp64 by esc_mse_loss
      bce_with_logits_loss: BCEWithLogitsLoss()(pred[is_labeled], y[is_labeled]), is_labeled = (y == y) (run_ogb_mol.py:65-72)"""

    @staticmethod
    def forward(ctx, pred, y, denom, name):
        kernel, over_m, scale, cast = _LOSS_HEADS[name]
        _dev(pred, y)
        _on(pred.device, y)
        ctx.shape = pred.shape
        pred = pred.contiguous().view(-1)
        y = y.contiguous().view(-1)
        if cast:
            y = y.float()
        if pred.numel() != y.numel():
            raise ValueError("%s: %d predictions vs %d targets" % (name, pred.numel(), y.numel()))
        M = pred.numel()
        loss, dpred = _empty(pred.device, 1), _empty(pred.device, M)
        nv.call(kernel, nv.ptr(pred), nv.ptr(y), M, int(denom or (M if over_m else 0)), *scale, nv.ptr(loss), nv.ptr(dpred),
                nv.stream())
        ctx.save_for_backward(dpred)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return (dpred * g).view(ctx.shape), None, None, None


def l1_loss(pred, y, denom=None):
    return _ElementwiseLoss.apply(pred, y, denom, "l1_loss")


def mse_loss(pred, y, denom=None):
    return _ElementwiseLoss.apply(pred, y, denom, "mse_loss")


def bce_with_logits_loss(pred, y, denom=None):
    return _ElementwiseLoss.apply(pred, y, denom, "bce_with_logits_loss")


class _NodeInput(Function):
    """cat([x, pos], 1) + table[node_type] (reference qm9_models.py:106-107) in one launch; x and pos are data (no
    gradient), the table's gradient is the small-table segmented sum of esc_embed_bwd."""

    @staticmethod
    def forward(ctx, x, pos, node_type, table):
        _dev(x, pos, table)
        _on(table.device, x, pos, node_type)
        if node_type.dtype != torch.int64:
            raise TypeError("node_input: node_type must be int64, got %s" % node_type.dtype)
        N, F = x.size(0), x.size(1) if x.dim() == 2 else -1
        if F < 1 or table.dim() != 2 or table.size(1) != F + 3:
            raise ValueError("node_input: x %s and pos %s need a table of %d columns, got %s"
                             % (tuple(x.shape), tuple(pos.shape), F + 3, tuple(table.shape)))
        x, ldx = _rows(x, F)              # a column slice of wider rows is taken as it is
        pos, ldp = _rows(pos, 3)
        node_type = node_type.reshape(-1).contiguous()
        if pos.size(0) != N or node_type.numel() != N:
            raise ValueError("node_input: %d rows of x, %d of pos, %d node types" % (N, pos.size(0), node_type.numel()))
        table = table.contiguous()
        out = _empty(table.device, N, F + 3)
        bad = torch.zeros(1, dtype=torch.int32, device=table.device)
        nv.call("esc_node_input_fwd", nv.ptr(x), ldx, nv.ptr(pos), ldp, nv.ptr(node_type), nv.ptr(table), table.size(0), F, N,
                nv.ptr(out), F + 3, nv.ptr(bad), nv.stream())
        known = getattr(node_type, "_esc_known_range", None)      # a batch of the device store: the range was checked once
        if not (known is not None and known[1] == node_type._version and known[0][0] >= 0 and known[0][1] < table.size(0)):
            if int(bad.item()):
                raise IndexError("node_input: node_type outside the %d-row table" % table.size(0))
        ctx.save_for_backward(node_type)
        ctx.rows, ctx.F = table.size(0), F
        return out

    @staticmethod
    def backward(ctx, g):
        (node_type,) = ctx.saved_tensors
        g, ld = _rows(g)
        dtable = _empty(g.device, ctx.rows, ctx.F + 3)
        nv.call("esc_node_input_bwd", nv.ptr(g), ld, nv.ptr(node_type), node_type.numel(), ctx.rows, ctx.F, nv.ptr(dtable),
                nv.stream())
        return None, None, None, dtable


def node_input(x, pos, node_type, table):
    return _NodeInput.apply(x, pos, node_type, table)


ACT_CODES = {"relu": 1, "elu": 2}


class _RowMap(Function):
    """y = f(x) on [M, C] rows by the entry points `kernel`_fwd / `kernel`_bwd (with the extra arguments `code`); only the output
    is saved: the backward reads the derivative off Y.
      esc_act: a bare ReLU / ELU(alpha = 1) (reference run_csl.py:152-169,219: no BatchNorm in front to fuse it behind)
      esc_log_softmax: F.log_softmax(x, dim=1) (run_sr.py:211, run_exp.py:215): one wave per row, maximum taken off first"""

    @staticmethod
    def forward(ctx, x, kernel, *code):
        _dev(x)
        x, ldx = _rows(x)
        M, C = x.shape
        y = _empty(x.device, M, C)
        nv.call(kernel + "_fwd", nv.ptr(x), ldx, M, C, *code, nv.ptr(y), C, nv.stream())
        ctx.save_for_backward(y)
        ctx.kernel, ctx.code = kernel, code
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        _dev(dy)
        dy, ldg = _rows(dy)
        M, C = y.shape
        dx = _empty(y.device, M, C)
        nv.call(ctx.kernel + "_bwd", nv.ptr(y), C, nv.ptr(dy), ldg, M, C, *ctx.code, nv.ptr(dx), C, nv.stream())
        return (dx, None) + (None,) * len(ctx.code)


def act(x, kind):
    """kind: 'relu' | 'elu' on a [M, C] tensor; a view with unit inner stride (a column slice of wider rows) is read in
    place through its row stride, any other layout is made contiguous first"""
    if kind not in ACT_CODES:
        raise ValueError("act: kind must be 'relu' or 'elu', got %r" % (kind,))
    return _RowMap.apply(x, "esc_act", ACT_CODES[kind])


def elu(x):
    return act(x, "elu")


def relu(x):
    return act(x, "relu")


def _segment_rows(spread, x, seg_ptr, G, n, mean):
    """The two segment kernels over G sorted segments of n rows, each the transpose of the other: esc_segment_pool_fwd sums (or
    averages) the rows of every segment, [n, C] -> [G, C]; `spread`, esc_segment_pool_bwd copies row g (over the segment's size
    for a mean) to the rows of segment g, [G, C] -> [n, C], G being the rows it is given."""
    x, ld = _rows(x)
    G, C = (x.size(0) if spread else G), x.size(1)
    out = _empty(x.device, n if spread else G, C)
    nv.call("esc_segment_pool_bwd" if spread else "esc_segment_pool_fwd", nv.ptr(x), ld, nv.ptr(seg_ptr), G, C, int(mean),
            nv.ptr(out), C, nv.stream())
    return out


class _SegmentPool(Function):
    """global_add_pool / global_mean_pool (run_graphcount.py:179, zinc_models.py:602) over a sorted batch vector."""

    @staticmethod
    def forward(ctx, x, seg_ptr, mean):
        _dev(x)
        _on(x.device, seg_ptr)
        out = _segment_rows(False, x, seg_ptr, seg_ptr.numel() - 1, None, mean)
        ctx.seg_ptr, ctx.mean, ctx.n = seg_ptr, bool(mean), x.size(0)
        return out

    @staticmethod
    def backward(ctx, g):
        return _segment_rows(True, g, ctx.seg_ptr, None, ctx.n, ctx.mean), None, None


def _seg_ptr(batch, size=None):
    """int32 [G+1] segment pointers of a non-decreasing batch vector (esc_plan_csr: integer histogram + scan), built
    once per batch tensor and cached on it (the device collate pre-fills the cache: it knows the node ranges)"""
    from .plan import _csr
    cache = getattr(batch, "_esc_seg", None)
    key = (batch._version, size)
    if cache is not None and key in cache:
        return cache[key]
    n_seg = int(batch[-1].item()) + 1 if (size is None and batch.numel()) else int(size or 0)
    if batch.numel() > 1 and not bool((batch[1:] >= batch[:-1]).all()):
        raise ValueError("segment_pool: batch vector must be sorted")
    seg_ptr = _csr(batch, max(n_seg, 1), want_perm=False)[0][:n_seg + 1]
    batch._esc_seg = {key: seg_ptr}
    return seg_ptr


def segment_pool(x, batch, size=None, mean=False):
    """`batch` must be non-decreasing (Batch.from_data_list / the device collate produce it that way)."""
    _dev(x)
    _on(x.device, batch)
    return _SegmentPool.apply(x, _seg_ptr(batch, size), mean)


class _Embedding(Function):
    """weight[index] via esc_bag_fwd with unit counts (exact: 0 + w*1); gradient via the CSC segmented sum."""

    @staticmethod
    def forward(ctx, weight, index):
        _dev(weight)
        _on(weight.device, index)
        weight = weight.contiguous()
        idx = index.reshape(-1)
        n, H = idx.numel(), weight.size(1)
        if n and (int(idx.min()) < 0 or int(idx.max()) >= weight.size(0)):
            raise IndexError("embedding index out of range")
        dev = weight.device
        row_ptr = torch.arange(n + 1, dtype=torch.int32, device=dev)
        idx32 = idx.to(torch.int32)
        ones = torch.ones(n, dtype=torch.int32, device=dev)
        out = _bag_rows(weight, row_ptr, idx32, ones, n)
        ctx.save_for_backward(idx)
        ctx.rows, ctx.H = weight.size(0), H
        return out.view(*index.shape, H)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        n = idx.numel()
        from .plan import _csr
        col_ptr, c_row = _csr(idx, ctx.rows)                 # stable grouping of the positions by table row (csrc/plan.hip)
        c_val = torch.ones(n, dtype=torch.int32, device=g.device)
        c_col = idx[c_row.long()].to(torch.int32)
        return _bag_table_grad(g.reshape(-1, ctx.H), ctx.H, col_ptr, c_row, c_val, c_col, n, ctx.rows), None


def embedding(weight, index):
    return _Embedding.apply(weight, index)


def embed_plan(index, dims, known_range=None):
    """bag plan of a sum-of-embeddings lookup over the concatenated tables: CSR by output row (idx32, row_ptr, ones) and
    CSC by table row (col_ptr, c_row, c_col); depends only on the index tensor — built once (esc_plan_csr) and cached
    on it (the bond features of a batch are looked up by every layer).
    known_range = (per-column minima, per-column maxima) of the DATASET the rows were gathered from (the device store
    computes them once): when they lie inside `dims` the per-batch range check — a device read-back that drains the
    stream — is skipped."""
    return _cached(index, "_esc_embed", dims, lambda: _build_embed_plan(index, dims, known_range))


def _build_embed_plan(index, dims, known_range):
    if index.device.type != "cuda":
        raise RuntimeError("esc_gnn_amd: embedding plans are built on the GPU (got a %s tensor)" % index.device.type)
    n, k = index.shape
    dev = index.device
    if k != len(dims) or k > nv.const("ESC_MAX_EMBED_COLS"):
        raise ValueError("embed_plan: index has %d columns for %d tables (at most %d)" % (k, len(dims), nv.const("ESC_MAX_EMBED_COLS")))
    if known_range is None:                              # the device store leaves the dataset-wide range on the tensors it collates
        tag = getattr(index, "_esc_known_range", None)
        if tag is not None and tag[1] == index._version:
            known_range = tag[0]
    trusted = (known_range is not None and len(known_range[0]) == k == len(dims) and
               all(lo >= 0 and hi < d for lo, hi, d in zip(known_range[0], known_range[1], dims)))
    idx = index if (index.dtype == torch.int64 and index.is_contiguous()) else index.to(torch.int64).contiguous()
    rows, total = int(sum(dims)), n * k
    # ONE int32 slab: idx32 | ones | c_row | c_col | row_ptr | col_ptr | flag | scratch (8-byte aligned start)
    sizes = [total, total, total, total, n + 1, rows + 1, 2]
    pad = (-sum(sizes)) % 2
    need = int(nv.lib().esc_embed_plan_scratch(n, k, rows))
    slab = torch.empty(sum(sizes) + pad + need, dtype=torch.int32, device=dev)
    parts, o = [], 0
    for sz in sizes:
        parts.append(slab[o:o + sz])
        o += sz
    idx32, ones, c_row, c_col, row_ptr, col_ptr, flag = parts
    scratch = slab[o + pad:]
    dims_h = (ctypes.c_int64 * k)(*[int(d) for d in dims])
    if total == 0:                                       # nothing to look up: empty entry arrays, all-zero pointers
        row_ptr.zero_()
        col_ptr.zero_()
        flag.zero_()
    else:
        nv.call("esc_embed_plan", nv.ptr(idx), n, k, ctypes.addressof(dims_h), nv.ptr(idx32), nv.ptr(ones), nv.ptr(row_ptr),
                nv.ptr(col_ptr), nv.ptr(c_row), nv.ptr(c_col), nv.ptr(scratch), nv.ptr(flag), nv.stream())
    if not trusted and total and int(flag[0].item()):    # one check per index tensor, not per lookup (ids known in range: no read-back)
        raise IndexError("embedding index out of range")
    return dict(idx32=idx32, row_ptr=row_ptr, ones=ones, col_ptr=col_ptr, c_row=c_row, c_col=c_col, entries=total, rows=rows,
                _slab=slab)


class _EmbeddingSum(Function):
    """out[r] = sum_j table[index[r, j] + offset_j]: the sum-of-embeddings encoders of the OGB models (AtomEncoder,
    BondEncoder: ogb_mol_gnn.py:264-282 and ogb's BondEncoder) as ONE bag launch over the concatenated tables instead
    of one lookup per feature column.  Entries of a row are added in column order starting from 0, i.e. exactly the
    reference's `out = 0; for i: out = out + emb_i(x[:, i])`.  The CSC plan of the gradient depends only on the index
    tensor: it is built once and cached on it (the bond features of a batch are looked up by every layer)."""

    @staticmethod
    def forward(ctx, table, index, dims):
        _dev(table)
        _on(table.device, index)
        table = table.contiguous()
        n, k = index.shape
        H, dev = table.size(1), table.device
        plan = embed_plan(index, dims)
        out = _empty(dev, n, H)
        nv.call("esc_bag_fwd_rows", nv.ptr(table), table.size(0), H, nv.ptr(plan["row_ptr"]), nv.ptr(plan["idx32"]), nv.ptr(plan["ones"]), n,
                nv.ptr(out), H, 0, None, nv.stream())
        ctx.plan, ctx.rows, ctx.H, ctx.nk = plan, table.size(0), H, n * k
        return out

    @staticmethod
    def backward(ctx, g):
        p = ctx.plan
        return _bag_table_grad(g.reshape(-1, ctx.H), ctx.H, p["col_ptr"], p["c_row"], p["ones"], p["c_col"], ctx.nk, ctx.rows), None, None


def embedding_sum(weights, index):
    """sum_j weights[j][index[:, j]] (index: LongTensor [n, len(weights)])."""
    if index.dim() != 2 or index.size(1) != len(weights):
        raise ValueError("embedding_sum: index must be [n, %d]" % len(weights))
    dims = tuple(int(w.size(0)) for w in weights)
    return _EmbeddingSum.apply(torch.cat(list(weights), dim=0), index, dims)


def _four_rows(rows):
    """the four (pointer, leading dimension) slots of the GINE+ entry points from k <= 4 row operands, the rest NULL"""
    return [a for x, ld in rows + [(None, 0)] * (4 - len(rows)) for a in (nv.ptr(x), ld)]


class _GinePlusAggregate(Function):
    """(1+eps[0]) x_0 + sum_{d=1..k} (1+eps[d]) sum_{j: d(j->i)=d} relu(x_{d-1}[j] + [d=1] e) — everything GINEPLUS /
    NAIVEGINEPLUS compute before self.nn (modules/gine_operations.py:306-362) in one launch per direction over the two
    groupings of a MultihopPlan (csrc/gineplus.hip), k <= 4."""

    @staticmethod
    def forward(ctx, plan, e, eps, *xs):
        k = len(xs)
        _dev(e, eps, *xs)
        dev = xs[0].device
        _on(dev, e, eps, plan.in_ptr, plan.in_meta, plan.out_ptr, plan.meta, *xs)
        rows = [_rows(x) for x in xs]
        N, C = rows[0][0].shape
        for x, _ in rows:
            if tuple(x.shape) != (N, C):
                raise ValueError("gineplus_aggregate: rows of %s and %s" % (tuple(x.shape), (N, C)))
        if N != plan.num_nodes:
            raise ValueError("gineplus_aggregate: %d rows for a plan of %d nodes" % (N, plan.num_nodes))
        eps = eps.contiguous()
        if tuple(eps.shape) != (k + 1, C):
            raise ValueError("gineplus_aggregate: eps %s, expected %s" % (tuple(eps.shape), (k + 1, C)))
        M1 = plan.num_d1
        e, lde = _rows(e)
        if tuple(e.shape) != (M1, C):
            raise ValueError("gineplus_aggregate: edge term %s does not match %d distance-1 pairs x %d" % (tuple(e.shape), M1, C))
        out = _empty(dev, N, C)
        nv.call("esc_gineplus_aggregate_fwd", *_four_rows(rows), nv.ptr(e) if M1 else None, lde, nv.ptr(plan.in_ptr),
                nv.ptr(plan.in_meta) if plan.num_pairs else None, nv.ptr(eps), N, C, k, M1, nv.ptr(out), C, nv.stream())
        ctx.save_for_backward(e, eps, *[x for x, _ in rows])
        ctx.plan, ctx.k = plan, k
        return out

    @staticmethod
    def backward(ctx, g):
        e, eps = ctx.saved_tensors[:2]
        rows = [_rows(x) for x in ctx.saved_tensors[2:]]
        plan, k = ctx.plan, ctx.k
        e, lde = _rows(e)
        g, ldg = _rows(g)
        N, C = rows[0][0].shape
        M1, dev = e.size(0), g.device
        need_e, need_eps = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = _empty(dev, k, N, C)
        d_e = _empty(dev, M1, C) if need_e else None
        part = d_eps = None
        if need_eps:
            part = _empty(dev, int(nv.lib().esc_gineplus_bwd_blocks(N)), (k + 1) * C)
            d_eps = _empty(dev, k + 1, C)
        nv.call("esc_gineplus_aggregate_bwd", *_four_rows(rows), nv.ptr(e) if M1 else None, lde, nv.ptr(g), ldg, nv.ptr(plan.out_ptr),
                nv.ptr(plan.meta) if plan.num_pairs else None, nv.ptr(eps), N, C, k, M1, nv.ptr(dx), nv.ptr(d_e) if M1 else None,
                nv.ptr(part), nv.ptr(d_eps), nv.stream())
        return (None, d_e, d_eps) + tuple(dx[t] for t in range(k))


def gineplus_aggregate(xs, e, eps, plan):
    """xs: the k rows X_0..X_{k-1} (GINEPLUS: the k latest layer outputs; NAIVEGINEPLUS: k times the same tensor), e [M1, C]
    the edge term of the distance-1 pairs in (row, col) order, eps [k+1, C], plan a multihop.MultihopPlan."""
    xs = list(xs)
    if not 1 <= len(xs) <= 4:
        raise ValueError("gineplus_aggregate: k=%d outside 1..4 (larger k takes the per-distance path)" % len(xs))
    return _GinePlusAggregate.apply(plan, e, eps, *xs)


class _SegmentBroadcast(Function):
    """rows[batch] for a sorted batch vector (virtual-node embedding -> nodes, ogb_mol_gnn.py:744): the transpose of
    global_add_pool, run by the segment-pool kernels."""

    @staticmethod
    def forward(ctx, rows, seg_ptr, n):
        _dev(rows)
        _on(rows.device, seg_ptr)
        out = _segment_rows(True, rows, seg_ptr, None, n, False)
        ctx.seg_ptr, ctx.G = seg_ptr, rows.size(0)
        return out

    @staticmethod
    def backward(ctx, g):
        return _segment_rows(False, g, ctx.seg_ptr, ctx.G, None, False), None, None


def segment_broadcast(rows, batch, size=None):
    size = rows.size(0) if size is None else int(size)
    return _SegmentBroadcast.apply(rows, _seg_ptr(batch, size), batch.numel())


# ---- classification head (csrc/classify.hip) -------------------------------------------------------------------------
def log_softmax(x):
    """row-wise log-softmax of a [M, C] tensor"""
    return _RowMap.apply(x, "esc_log_softmax")


def _targets(target, M, dev):
    if target.dtype != torch.int64:
        raise TypeError("esc_gnn_amd: class targets must be int64, got %s" % target.dtype)
    _on(dev, target)
    target = target.contiguous().view(-1)
    if target.numel() != M:
        raise ValueError("%d targets for %d rows" % (target.numel(), M))
    return target


def _denom(reduction, denom):
    if denom is not None:
        return int(denom)
    if reduction not in ("mean", "sum"):
        raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
    return 0 if reduction == "mean" else 1


def _head_info(info, C):
    """one read-back of the head's int32 pair (bad-target flag, correct count): raises on a target outside [0, C)"""
    bad, correct = info.tolist()
    if bad:
        raise RuntimeError("Target out of bounds: class targets must lie in [0, %d)" % C)
    return correct


def _head_raw(x, target, denom, want_grad, fused=True):
    """One launch of the classification head on [M, C] rows: esc_log_softmax_nll on logits (`fused`: also leaves logp), or
    esc_nll_loss on log-probabilities.  Returns (loss, logp or None, d loss / d x or None, correct): targets, the info pair,
    the row scratch and the one read-back are the same for both."""
    x, ld = _rows(x)
    M, C = x.shape
    dev = x.device
    target = _targets(target, M, dev)
    loss = _empty(dev, 1)
    info = torch.empty(2, dtype=torch.int32, device=dev)
    logp = _empty(dev, M, C) if fused else None
    dx = _empty(dev, M, C) if want_grad else None
    rows = _empty(dev, 2 * M)
    outs = (nv.ptr(logp), C, nv.ptr(loss)) if fused else (nv.ptr(loss),)
    nv.call("esc_log_softmax_nll" if fused else "esc_nll_loss", nv.ptr(x), ld, nv.ptr(target), M, C, denom, 1.0, *outs,
            nv.ptr(dx), C, info[1:].data_ptr(), info.data_ptr(), nv.ptr(rows), nv.stream())
    return loss.view(()), logp, dx, _head_info(info, C)


class _HeadLoss(Function):
    """F.nll_loss(logp, target, reduction=...) (run_exp.py:235,248), deterministic; the accuracy count of run_exp.py:261-264
    rides on the same launch.  `fused`: nll_loss(log_softmax(logits), target) with its gradient (softmax - onehot) / denom in
    ONE launch; logp and the loss equal the two-op composition bit for bit."""

    @staticmethod
    def forward(ctx, x, target, denom, fused):
        _dev(x)
        loss, logp, dx, ctx.correct = _head_raw(x, target, denom, True, fused)
        ctx.save_for_backward(dx)
        if not fused:
            return loss
        ctx.mark_non_differentiable(logp)
        return loss, logp

    @staticmethod
    def backward(ctx, g, _glogp=None):
        (dx,) = ctx.saved_tensors
        return dx * g, None, None, None


def _head_loss(fused, x, target, reduction, denom):
    """(loss, logp or None, correct) through autograd when x asks for a gradient, else by the bare launch"""
    denom = _denom(reduction, denom)
    if torch.is_grad_enabled() and x.requires_grad:
        res = _HeadLoss.apply(x, target, denom, fused)
        loss, logp = res if fused else (res, None)
        return loss, logp, loss.grad_fn.correct
    _dev(x)
    loss, logp, _, correct = _head_raw(x, target, denom, False, fused)
    return loss, logp, correct


def nll_loss(logp, target, reduction="mean", denom=None, return_correct=False):
    """-sum_i logp[i, target_i] / denom; `denom` overrides the divisor that `reduction` implies.  A target outside
    [0, C) raises RuntimeError.  return_correct: also the number of rows whose argmax equals the target."""
    loss, _, correct = _head_loss(False, logp, target, reduction, denom)
    return (loss, correct) if return_correct else loss


def log_softmax_nll(logits, target, reduction="mean", denom=None, return_aux=False):
    """The fused classification head: loss = nll_loss(log_softmax(logits), target).  return_aux: (loss, logp, correct)
    with logp the (non-differentiable) log-probabilities and correct the number of rows whose argmax is the target."""
    loss, logp, correct = _head_loss(True, logits, target, reduction, denom)
    return (loss, logp, correct) if return_aux else loss


def pdist(x, threshold=None):
    """torch.pdist(x, p=2) in the difference form (fp64 inside): [M*(M-1)/2] distances in row-major upper-triangle order.
    With a threshold: (distances, number of entries < threshold) — the SR25 criterion of run_sr.py:241-242.  Not
    differentiable (the drivers use it under no_grad)."""
    _dev(x)
    x, ldx = _rows(x.detach())
    M, C = x.shape
    if C == 0:
        raise ValueError("pdist: rows have no columns")
    out = _empty(x.device, M * (M - 1) // 2)
    below = torch.empty(1, dtype=torch.int32, device=x.device) if threshold is not None else None
    nv.call("esc_pdist", nv.ptr(x), ldx, M, C, nv.ptr(out), float(threshold if threshold is not None else 0.0),
            nv.ptr(below), nv.stream())
    return out if threshold is None else (out, int(below.item()))


class _SegmentFirst(Function):
    """x[first row of every segment]: the reference's `x[center_indices]` (zinc_models.py:388-392, the root is the first node
    of its subgraph) without the host round trip of np.unique; the gradient writes every row once (no memset, no atomics)."""

    @staticmethod
    def forward(ctx, x, ptr, node_to_segment):
        _dev(x)
        _on(x.device, ptr, node_to_segment)
        if ptr.dtype != torch.int64 or node_to_segment.dtype != torch.int64:
            raise TypeError("segment_first: ptr and node_to_segment must be int64")
        x, ldx = _rows(x)
        ptr, node_to_segment = ptr.contiguous(), node_to_segment.contiguous()
        S, C = ptr.numel() - 1, x.size(1)
        if node_to_segment.numel() != x.size(0):
            raise ValueError("segment_first: %d rows but %d segment ids" % (x.size(0), node_to_segment.numel()))
        out = _empty(x.device, S, C)
        nv.call("esc_segment_first_fwd", nv.ptr(x), ldx, nv.ptr(ptr), S, C, nv.ptr(out), nv.stream())
        ctx.ptr, ctx.seg, ctx.n = ptr, node_to_segment, x.size(0)
        return out

    @staticmethod
    def backward(ctx, g):
        g, ldg = _rows(g)
        C = g.size(1)
        dx = _empty(g.device, ctx.n, C)
        nv.call("esc_segment_first_bwd", nv.ptr(g), ldg, nv.ptr(ctx.ptr), nv.ptr(ctx.seg), ctx.n, C, nv.ptr(dx), nv.stream())
        return dx, None, None


def segment_first(x, ptr, node_to_segment):
    """out[s] = x[ptr[s]]; ptr: int64 [S+1] segment pointers, node_to_segment: int64 [N] (non-decreasing)."""
    return _SegmentFirst.apply(x, ptr, node_to_segment)


class _PoolMeanCenterSide(Function):
    """cat([global_mean_pool(x, node_to_subgraph2), x[center_idx[:, 0]], x[center_idx[:, 1]]], -1) of the reference's I2GNN
    (zinc_cycle_models.py:218-222) in one pass over x (csrc/i2pool.hip); the gradient writes every row once — a centre that is
    also the side row (a root without neighbours, a self loop) receives both terms."""

    @staticmethod
    def forward(ctx, x, ptr, center_idx, node_to_segment):
        _dev(x)
        _on(x.device, ptr, center_idx, node_to_segment)
        if ptr.dtype != torch.int64 or center_idx.dtype != torch.int64 or node_to_segment.dtype != torch.int64:
            raise TypeError("pool_mean_center_side: ptr, center_idx and node_to_segment must be int64")
        x, ldx = _rows(x)
        ptr, center_idx, node_to_segment = ptr.contiguous(), center_idx.contiguous(), node_to_segment.contiguous()
        S, C = ptr.numel() - 1, x.size(1)
        if center_idx.shape != (S, 2):
            raise ValueError("pool_mean_center_side: center_idx %s for %d segments" % (tuple(center_idx.shape), S))
        if node_to_segment.numel() != x.size(0):
            raise ValueError("pool_mean_center_side: %d rows but %d segment ids" % (x.size(0), node_to_segment.numel()))
        out = _empty(x.device, S, 3 * C)
        nv.call("esc_pool_mean_center_side_fwd", nv.ptr(x), ldx, nv.ptr(ptr), center_idx.data_ptr(), center_idx.data_ptr() + 8, 2,
                S, C, nv.ptr(out), 3 * C, nv.stream())
        ctx.ptr, ctx.ci, ctx.seg, ctx.n = ptr, center_idx, node_to_segment, x.size(0)
        return out

    @staticmethod
    def backward(ctx, g):
        g, ldg = _rows(g)
        C = g.size(1) // 3
        dx = _empty(g.device, ctx.n, C)
        nv.call("esc_pool_mean_center_side_bwd", nv.ptr(g), ldg, nv.ptr(ctx.ptr), ctx.ci.data_ptr(), ctx.ci.data_ptr() + 8, 2,
                nv.ptr(ctx.seg), ctx.n, C, nv.ptr(dx), C, nv.stream())
        return dx, None, None, None


def pool_mean_center_side(x, ptr, center_idx, node_to_segment):
    """out[s] = [mean of x[ptr[s]:ptr[s+1]] | x[center_idx[s, 0]] | x[center_idx[s, 1]]]; ptr: int64 [S+1], center_idx: int64
    [S, 2] (rows inside segment s), node_to_segment: int64 [N] (non-decreasing)."""
    return _PoolMeanCenterSide.apply(x, ptr, center_idx, node_to_segment)


class _SigmoidMul(Function):
    """sigmoid(a) * x: the gate `subgraph_gate[layer](z_emb) * x` of the reference's I2GNN (zinc_cycle_models.py:205-206,
    219-220; the Sigmoid of the Sequential moves into this kernel), finite for every finite a."""

    @staticmethod
    def forward(ctx, a, x):
        _dev(a, x)
        _on(a.device, x)
        a, lda = _rows(a)
        x, ldx = _rows(x)
        if a.shape != x.shape:
            raise ValueError("sigmoid_mul: shapes %s and %s differ" % (tuple(a.shape), tuple(x.shape)))
        M, C = a.shape
        y = _empty(a.device, M, C)
        nv.call("esc_sigmoid_mul_fwd", nv.ptr(a), lda, nv.ptr(x), ldx, M, C, nv.ptr(y), C, nv.stream())
        ctx.save_for_backward(a, x)
        return y

    @staticmethod
    def backward(ctx, g):
        (a, lda), (x, ldx), (g, ldg) = (_rows(t) for t in ctx.saved_tensors + (g,))
        M, C = a.shape
        da = _empty(g.device, M, C) if ctx.needs_input_grad[0] else None
        dx = _empty(g.device, M, C) if ctx.needs_input_grad[1] else None
        if da is not None or dx is not None:
            nv.call("esc_sigmoid_mul_bwd", nv.ptr(a), lda, nv.ptr(x), ldx, nv.ptr(g), ldg, M, C, nv.ptr(da), nv.ptr(dx), nv.stream())
        return da, dx


def sigmoid_mul(a, x):
    return _SigmoidMul.apply(a, x)


def group_plan(index, n_keys):
    """The stable grouping of the positions of an UNSORTED index vector by key (esc_plan_csr), with what the two transposed
    bag launches below need: built once per index tensor and cached on it, shared by every layer and both directions (I2GNN's
    node_to_original_node: the context mean and the gather back).  No read-back: the keys come from the expansion kernel, and a
    key outside [0, n_keys) only sets `bad`."""
    def build():
        from .plan import _csr
        dev, n = index.device, index.numel()
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        col_ptr, c_row = _csr(index, int(n_keys), bad=bad)
        counts = (col_ptr[1:] - col_ptr[:-1]).clamp(min=1).to(torch.float32)
        return dict(n=n, n_keys=int(n_keys), idx32=index.to(torch.int32), row_ptr=torch.arange(n + 1, dtype=torch.int32, device=dev),
                    ones=torch.ones(n, dtype=torch.int32, device=dev), col_ptr=col_ptr, c_row=c_row, bad=bad,
                    inv_count=(1.0 / counts).view(-1, 1))
    return _cached(index, "_esc_group", int(n_keys), build)


class _GatherRows(Function):
    """table[index] for an unsorted index with repeats (`...[data.node_to_original_node]`, zinc_cycle_models.py:276): the bag
    kernel with one unit entry per row; its gradient is the group sum below — each the transpose of the other, both
    deterministic (entry order) and without atomics."""

    @staticmethod
    def forward(ctx, table, plan):
        _dev(table)
        ctx.plan = plan
        return _bag_rows(table, plan["row_ptr"], plan["idx32"], plan["ones"], plan["n"])

    @staticmethod
    def backward(ctx, g):
        p = ctx.plan
        return _bag_rows(g, p["col_ptr"], p["c_row"], p["ones"], p["n_keys"]), None


class _GroupSum(Function):
    """out[k] = sum of the rows whose key is k, in position order (scatter-add over an unsorted index); gradient = gather."""

    @staticmethod
    def forward(ctx, x, plan):
        _dev(x)
        ctx.plan = plan
        return _bag_rows(x, plan["col_ptr"], plan["c_row"], plan["ones"], plan["n_keys"])

    @staticmethod
    def backward(ctx, g):
        p = ctx.plan
        return _bag_rows(g, p["row_ptr"], p["idx32"], p["ones"], p["n"]), None


def gather_rows(table, plan):
    return _GatherRows.apply(table, plan)


def group_mean(x, plan):
    """global_mean_pool(x, index) for the unsorted index the plan was built from"""
    if x.size(0) != plan["n"]:
        raise ValueError("group_mean: %d rows for a plan of %d" % (x.size(0), plan["n"]))
    return _GroupSum.apply(x, plan) * plan["inv_count"]


# ---- graph transformer (csrc/attention.hip, include/escgnn_gps.h) -----------------------------------------------------------
def _pair_ptr(graph_ptr):
    """int64 [G+1] exclusive scan of n_g^2 on the device (torch plumbing, no read-back), cached on the graph_ptr tensor the way
    _seg_ptr caches segment pointers: the ten attention layers of a step share it"""
    def build():
        n = (graph_ptr[1:] - graph_ptr[:-1]).to(torch.int64)
        pair_ptr = torch.zeros(graph_ptr.numel(), dtype=torch.int64, device=graph_ptr.device)
        torch.cumsum(n * n, 0, out=pair_ptr[1:])
        return pair_ptr
    return _cached(graph_ptr, "_esc_pairs", None, build)


def attention_max_nodes(head_dim):
    """the largest graph esc_graph_attention_* take at this head_dim (0: no kernel for that head_dim)"""
    return int(nv.lib().esc_graph_attention_max_nodes(int(head_dim)))


class _GraphAttention(Function):
    """softmax(Q K^T / sqrt(d)) V per head over the nodes of each graph, with dropout on the attention weights: the reference's
    to_dense_batch -> torch.nn.MultiheadAttention(key_padding_mask) -> [mask] between the two projections
    (GraphGPS/graphgps/layer/gps_layer.py:234-236), one launch per direction off graph_ptr.  Saves qkv, the row log-sum-exp and
    the keep mask; the probabilities are recomputed by the backward."""

    @staticmethod
    def forward(ctx, qkv, graph_ptr, pair_ptr, heads, head_dim, p, seed, max_nodes):
        qkv, ld = _rows(qkv)
        N, H = qkv.size(0), heads * head_dim
        G, dev = graph_ptr.numel() - 1, qkv.device
        out = _empty(dev, N, H)
        lse = _empty(dev, heads, N)
        mask_pairs = N * max_nodes if p > 0.0 else 0           # >= sum n_g^2, known without reading graph_ptr back
        mask = torch.empty(heads * mask_pairs, dtype=torch.uint8, device=dev) if p > 0.0 else None
        nv.call("esc_graph_attention_fwd", nv.ptr(qkv), ld, nv.ptr(graph_ptr), nv.ptr(pair_ptr), G, N, mask_pairs, max_nodes,
                heads, head_dim, float(p), int(seed), nv.ptr(out), H, nv.ptr(lse), nv.ptr(mask), nv.stream())
        ctx.save_for_backward(qkv, lse, mask)
        ctx.args = (graph_ptr, pair_ptr, G, N, mask_pairs, max_nodes, heads, head_dim, float(p))
        ctx.mark_non_differentiable(lse)
        ctx.set_materialize_grads(False)                       # no zero-filled gradients of lse and mask: two launches per backward
        return (out, lse) if mask is None else (out, lse, mask)

    @staticmethod
    def backward(ctx, d_out, *unused):
        if d_out is None:
            return (None,) * 8
        qkv, lse, mask = ctx.saved_tensors
        graph_ptr, pair_ptr, G, N, mask_pairs, max_nodes, heads, head_dim, p = ctx.args
        _dev(d_out)
        qkv, ld = _rows(qkv)
        d_out, ldg = _rows(d_out)
        d_qkv = _empty(qkv.device, N, 3 * heads * head_dim)
        nv.call("esc_graph_attention_bwd", nv.ptr(qkv), ld, nv.ptr(d_out), ldg, nv.ptr(lse),
                nv.ptr(mask), nv.ptr(graph_ptr), nv.ptr(pair_ptr), G, N, mask_pairs, max_nodes, heads, head_dim, p, nv.ptr(d_qkv),
                nv.stream())
        return d_qkv, None, None, None, None, None, None, None


def attention_bias_max_nodes(head_dim):
    """the largest graph esc_graph_attention_bias_* take at this head_dim (0: no kernel for that head_dim): the unbiased limit
    cut by the LDS the bias gradient's bins take (include/escgnn_spd.h states the formula)"""
    return int(nv.lib().esc_graph_attention_bias_max_nodes(int(head_dim)))


BIAS_ROWS = 101                   # rows of the bias table: distances 0..99, and 100 = no path (the reference's padding row)


class _GraphAttentionBias(Function):
    """_GraphAttention with table[min(spd_ij, 100), head] added to the scores: the reference's `BiasedTransformer`
    (gps_layer.py:237-239,273-278), whose dense float attn_mask [B * heads, n_max, n_max] is never formed.  One launch forward,
    two backward (the attention's, and the sum of the bias gradient's per-graph partials).  Gradients: qkv and the table; spd is
    data."""

    @staticmethod
    def forward(ctx, qkv, table, spd, graph_ptr, pair_ptr, heads, head_dim, p, seed, max_nodes):
        qkv, ld = _rows(qkv)
        N, H = qkv.size(0), heads * head_dim
        G, dev = graph_ptr.numel() - 1, qkv.device
        out = _empty(dev, N, H)
        lse = _empty(dev, heads, N)
        mask_pairs = N * max_nodes if p > 0.0 else 0
        mask = torch.empty(heads * mask_pairs, dtype=torch.uint8, device=dev) if p > 0.0 else None
        nv.call("esc_graph_attention_bias_fwd", nv.ptr(qkv), ld, nv.ptr(graph_ptr), nv.ptr(pair_ptr), nv.ptr(spd), spd.numel(), nv.ptr(table),
                G, N, mask_pairs, max_nodes, heads, head_dim, float(p), int(seed), nv.ptr(out), H, nv.ptr(lse), nv.ptr(mask), nv.stream())
        ctx.save_for_backward(qkv, table, spd, lse, mask)
        ctx.args = (graph_ptr, pair_ptr, G, N, mask_pairs, max_nodes, heads, head_dim, float(p))
        ctx.mark_non_differentiable(lse)
        ctx.set_materialize_grads(False)
        return (out, lse) if mask is None else (out, lse, mask)

    @staticmethod
    def backward(ctx, d_out, *unused):
        if d_out is None:
            return (None,) * 10
        qkv, table, spd, lse, mask = ctx.saved_tensors
        graph_ptr, pair_ptr, G, N, mask_pairs, max_nodes, heads, head_dim, p = ctx.args
        _dev(d_out)
        qkv, ld = _rows(qkv)
        d_out, ldg = _rows(d_out)
        d_qkv = _empty(qkv.device, N, 3 * heads * head_dim)
        d_table = _empty(qkv.device, BIAS_ROWS, heads)
        need = int(nv.lib().esc_graph_attention_bias_scratch_floats(G, heads))
        partial = _empty(qkv.device, max(need, 1))
        nv.call("esc_graph_attention_bias_bwd", nv.ptr(qkv), ld, nv.ptr(d_out), ldg, nv.ptr(lse), nv.ptr(mask), nv.ptr(graph_ptr),
                nv.ptr(pair_ptr), nv.ptr(spd), spd.numel(), nv.ptr(table), G, N, mask_pairs, max_nodes, heads, head_dim, p, nv.ptr(d_qkv),
                nv.ptr(partial), need, nv.ptr(d_table), nv.stream())
        return d_qkv, d_table, None, None, None, None, None, None, None, None


def graph_attention(qkv, graph_ptr, heads, p=0.0, training=False, max_nodes=None, seed=None, return_aux=False, spd=None, bias_table=None):
    """Multi-head self-attention inside every graph of a ragged batch.  qkv: [N, 3H] rows [q | k | v] (a column slice of wider
    rows is read in place), graph_ptr: int32 [G+1] node ranges on the device, H = heads * head_dim.  Dropout with rate p on the
    attention weights when `training` (counter-based masks: `seed`, drawn from torch's generator when None).
    max_nodes: the largest graph of the batch as the HOST knows it (the device store's h_node_ptr) - given, nothing is read back;
    None costs one read-back of graph_ptr, cached on it.  Limits: head_dim a multiple of 4 and at most 64, max_nodes at most
    attention_max_nodes(head_dim); beyond them RuntimeError, raised before anything is launched.
    return_aux: also (lse [heads, N], keep mask bytes or None; the mask's layout: include/escgnn_gps.h).
    spd, bias_table (both or neither): the shortest-path bias of the reference's BiasedTransformer - spd uint8, byte (i, j) of
    graph g at pair_ptr[g] + i n + j (graph_spd, spd_gather; any byte matrix is legal, above 100 counts as 100), bias_table fp32
    [101, heads], differentiable; the scores gain bias_table[min(spd_ij, 100), head] and lse includes it.  The node limit is then
    attention_bias_max_nodes(head_dim).  Without them nothing changes."""
    _dev(qkv)
    if (spd is None) != (bias_table is None):
        raise ValueError("graph_attention: spd and bias_table come together (got %s)" % ("spd alone" if bias_table is None else "bias_table alone"))
    if spd is not None:
        _dev(bias_table)
        _on(qkv.device, spd, bias_table)
        if spd.dtype != torch.uint8 or spd.dim() != 1:
            raise TypeError("graph_attention: spd must be a 1-D uint8 tensor (the graphs' flattened n x n distance matrices)")
        if tuple(bias_table.shape) != (BIAS_ROWS, int(heads)):
            raise ValueError("graph_attention: bias_table must be [%d, heads = %d], got %s" % (BIAS_ROWS, int(heads), tuple(bias_table.shape)))
    _on(qkv.device, graph_ptr)
    if graph_ptr.dtype != torch.int32 or graph_ptr.dim() != 1 or graph_ptr.numel() < 1:
        raise TypeError("graph_attention: graph_ptr must be a 1-D int32 tensor of G+1 node offsets")
    heads = int(heads)
    if qkv.dim() != 2 or heads < 1 or qkv.size(1) % (3 * heads):
        raise RuntimeError("graph_attention: qkv %s is not [N, 3 * H] with heads * head_dim == H for %d heads"
                           % (tuple(qkv.shape), heads))
    head_dim = qkv.size(1) // (3 * heads)
    limit = attention_max_nodes(head_dim) if spd is None else attention_bias_max_nodes(head_dim)
    if limit == 0:
        raise RuntimeError("graph_attention: head_dim %d must be a multiple of 4 and at most 64" % head_dim)
    graph_ptr = graph_ptr.contiguous()
    if max_nodes is None:
        max_nodes = _cached(graph_ptr, "_esc_max_nodes", None,
                            lambda: int((graph_ptr[1:] - graph_ptr[:-1]).max()) if graph_ptr.numel() > 1 else 0)
    max_nodes = int(max_nodes)
    if max_nodes > limit:
        raise RuntimeError("graph_attention: a graph of %d nodes exceeds the limit of %d nodes per graph at head_dim %d%s"
                           % (max_nodes, limit, head_dim, "" if spd is None else " with the shortest-path bias"))
    p = float(p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError("graph_attention: dropout rate %g outside [0, 1)" % p)
    if p > 0.0 and seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())      # host generator: seeded runs repeat, nothing waits for the device
    if spd is None:
        res = _GraphAttention.apply(qkv, graph_ptr, _pair_ptr(graph_ptr), heads, head_dim, p, seed or 0, max_nodes)
    else:
        res = _GraphAttentionBias.apply(qkv, bias_table.contiguous(), spd.contiguous(), graph_ptr, _pair_ptr(graph_ptr), heads, head_dim, p,
                                        seed or 0, max_nodes)
    return (res[0], res[1], res[2] if len(res) > 2 else None) if return_aux else res[0]


# ---- Laplacian positional encoding (csrc/lappe.hip, include/escgnn_lappe.h) -------------------------------------------------
def laplacian_eig_limits():
    """(largest graph esc_laplacian_eig takes, largest graph whose matrices stay in LDS)"""
    h = nv.lib()
    return int(h.esc_laplacian_eig_max_nodes()), int(h.esc_laplacian_eig_lds_nodes())


def _index_vector(t, what, dtype):
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 1 or t.numel() < 1:
        raise TypeError("%s must be a 1-D %s tensor" % (what, str(dtype).replace("torch.", "")))
    return t.contiguous()


def _ragged_graphs(who, node_limit, edge_index, graph_ptr, edge_ptr, max_nodes, num_nodes):
    """A ragged set of graphs as a per-graph kernel takes it (laplacian_eig, rw_landing; csrc/ragged_graphs.h): a device
    edge_index [2, E] and the two offset vectors of its G graphs, checked; G, N and the largest graph resolved - max_nodes or
    num_nodes None costs one read-back of graph_ptr each - and the largest graph held against node_limit, the kernel's.  Returns
    (src, dst, node_ptr, edge_ptr, G, N, max_nodes), the four vectors contiguous int64."""
    if not torch.is_tensor(edge_index) or edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise TypeError("%s: edge_index must be an int64 [2, E] tensor" % who)
    if not edge_index.is_cuda:
        raise RuntimeError("esc_gnn_amd: the hot path runs on the HIP device only (got a %s tensor); there is no CPU fallback"
                           % edge_index.device)
    for name, t in (("graph_ptr", graph_ptr), ("edge_ptr", edge_ptr)):
        if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64) or t.dim() != 1 or t.numel() < 1:
            raise TypeError("%s: %s must be a 1-D int32 or int64 tensor of G+1 offsets" % (who, name))
    _on(edge_index.device, graph_ptr, edge_ptr)
    if graph_ptr.numel() != edge_ptr.numel():
        raise ValueError("%s: graph_ptr has %d entries, edge_ptr %d" % (who, graph_ptr.numel(), edge_ptr.numel()))
    G = graph_ptr.numel() - 1
    if max_nodes is None:
        max_nodes = int((graph_ptr[1:] - graph_ptr[:-1]).max()) if G else 0
    max_nodes = int(max_nodes)
    if max_nodes > node_limit:
        raise RuntimeError("%s: a graph of %d nodes exceeds the limit of %d nodes per graph" % (who, max_nodes, node_limit))
    if num_nodes is None:
        num_nodes = int(graph_ptr[-1])
    return (edge_index[0].contiguous(), edge_index[1].contiguous(), graph_ptr.to(torch.int64).contiguous(),
            edge_ptr.to(torch.int64).contiguous(), G, int(num_nodes), max_nodes)


def _checked_gather(who, tables, table_rule, node_ptr_all, graph_ids, graph_ptr, num_nodes):
    """What lappe_gather and rwse_gather share: the resident tables (fp32, contiguous [N_all, K], one shape) and the index
    vectors checked, graph_ids checked on the HOST (count, range) and uploaded, one output [N, K] per table.  Returns
    (node_ptr_all, ids_d, graph_ptr, (G_all, N_all, B, N, K), outputs)."""
    _dev(*tables)
    dev = tables[0].device
    if any(t.dim() != 2 or t.shape != tables[0].shape or not t.is_contiguous() for t in tables):
        raise ValueError("%s: %s" % (who, table_rule))
    node_ptr_all = _index_vector(node_ptr_all, "%s: node_ptr_all" % who, torch.int64)
    graph_ptr = _index_vector(graph_ptr, "%s: graph_ptr" % who, torch.int32)
    _on(dev, node_ptr_all, graph_ptr)
    G_all, B = node_ptr_all.numel() - 1, graph_ptr.numel() - 1
    if torch.is_tensor(graph_ids) and graph_ids.is_cuda:
        raise RuntimeError("%s: graph_ids must live on the host (they are checked there, without a read-back)" % who)
    ids_h = torch.as_tensor(graph_ids, dtype=torch.int64).reshape(-1)
    if ids_h.numel() != B:
        raise ValueError("%s: %d graph ids for a batch of %d graphs" % (who, ids_h.numel(), B))
    if B and (int(ids_h.min()) < 0 or int(ids_h.max()) >= G_all):
        raise IndexError("%s: graph id out of range (the table holds %d graphs)" % (who, G_all))
    N, K = int(num_nodes), tables[0].size(1)
    ids_d = ids_h.to(dev, non_blocking=True)
    outs = [_empty(dev, N, K) for _ in tables]
    return node_ptr_all, ids_d, graph_ptr, (G_all, tables[0].size(0), B, N, K), outs


def laplacian_eig(edge_index, graph_ptr, edge_ptr, max_freqs, max_nodes=None, edges_local=False, num_nodes=None):
    """The max_freqs smallest eigenpairs of L = D - A of every graph of a ragged set, one workgroup per graph, one launch: the
    reference's compute_posenc_stats for pe_types ['LapPE'] with laplacian_norm none and eigvec_norm L2
    (GraphGPS/graphgps/transform/posenc_stats.py:40-73,149-182).  edge_index int64 [2, E] on the device; graph_ptr, edge_ptr
    [G+1] node and edge range of every graph (int32 or int64; edges contiguous per graph); edges_local: the edge ends are
    graph-local ids (a store's flat arrays) instead of batch rows.  Returns (EigVals [N, K, 1], EigVecs [N, K]) fp32, NaN in the
    columns j >= n of a graph with n < K nodes.
    max_nodes: the largest graph as the HOST knows it, num_nodes: N likewise; None costs one read-back of graph_ptr each.
    Limits: laplacian_eig_limits()[0] = 256 nodes per graph, max_freqs <= 32; beyond them RuntimeError, raised before anything
    is launched."""
    K = int(max_freqs)
    if not 1 <= K <= 32:
        raise RuntimeError("laplacian_eig: max_freqs %d outside 1..32" % K)
    src, dst, node_ptr, edge_ptr, G, N, max_nodes = _ragged_graphs("laplacian_eig", laplacian_eig_limits()[0], edge_index, graph_ptr,
                                                                   edge_ptr, max_nodes, num_nodes)
    dev = src.device
    vecs = _empty(dev, N, K)
    vals = _empty(dev, N, K)
    need = int(nv.lib().esc_laplacian_eig_scratch_bytes(N, max_nodes))
    scratch = torch.empty(need // 8, dtype=torch.float64, device=dev) if need else None
    nv.call("esc_laplacian_eig", nv.ptr(src), nv.ptr(dst), src.numel(), nv.ptr(node_ptr), nv.ptr(edge_ptr), G, N, int(bool(edges_local)), K,
            max_nodes, nv.ptr(scratch), need, nv.ptr(vecs), nv.ptr(vals), nv.stream())
    return vals.view(N, K, 1), vecs


def lappe_gather(vecs_all, vals_all, node_ptr_all, graph_ids, graph_ptr, num_nodes):
    """The batch's rows of a split's resident PE tables (what the reference's collate does to the EigVecs / EigVals keys), one
    launch.  vecs_all, vals_all [N_all, K] fp32; node_ptr_all int64 [G_all+1] (device); graph_ids: the batch's graphs in batch
    order, a HOST int64 tensor or list - checked here, an id out of range raises IndexError before anything is launched;
    graph_ptr int32 [B+1]: the batch's node ranges; num_nodes: the batch's N.  Returns (vals [N, K, 1], vecs [N, K])."""
    node_ptr_all, ids_d, graph_ptr, (G_all, N_all, B, N, K), (vecs, vals) = _checked_gather(
        "lappe_gather", (vecs_all, vals_all), "the two tables must be contiguous [N_all, K] tensors of one shape", node_ptr_all, graph_ids,
        graph_ptr, num_nodes)
    nv.call("esc_lappe_gather", nv.ptr(vecs_all), nv.ptr(vals_all), nv.ptr(node_ptr_all), G_all, N_all, nv.ptr(ids_d), nv.ptr(graph_ptr), B, N, K,
            nv.ptr(vecs), nv.ptr(vals), nv.stream())
    return vals.view(N, K, 1), vecs


def lappe_encode_block_rows():
    """rows per workgroup of esc_lappe_encode_bwd: its fixed row partition"""
    return int(nv.lib().esc_lappe_encode_block_rows())


class _LapPEEncode(Function):
    """sum_j ReLU(W1 ReLU(WA [v_ij s_j, l_ij] + bA) + b1) over the frequencies whose eigenvector entry is not NaN: the reference's
    LapPENodeEncoder.forward for the DeepSet model with 2 layers (graphgps/encoder/laplace_pos_encoder.py:94-132: cat, isnan
    mask, linear_A, pe_encoder, masked_fill_, sum), one launch forward and two backward.  Saves only its inputs."""

    @staticmethod
    def forward(ctx, eigvecs, eigvals, signs, wA, bA, w1, b1):
        N, K = eigvecs.shape
        P = w1.size(0)
        out = _empty(eigvecs.device, N, P)
        nv.call("esc_lappe_encode_fwd", nv.ptr(eigvecs), nv.ptr(eigvals), nv.ptr(signs), nv.ptr(wA), nv.ptr(bA), nv.ptr(w1), nv.ptr(b1),
                N, K, P, nv.ptr(out), P, nv.stream())
        ctx.save_for_backward(eigvecs, eigvals, signs, wA, bA, w1, b1)
        return out

    @staticmethod
    def backward(ctx, d_out):
        eigvecs, eigvals, signs, wA, bA, w1, b1 = ctx.saved_tensors
        N, K = eigvecs.shape
        P = w1.size(0)
        _dev(d_out)
        d_out, ldg = _rows(d_out)
        need = int(nv.lib().esc_lappe_encode_scratch_floats(N, P))
        scratch = _empty(eigvecs.device, max(need, 1))
        flat = _empty(eigvecs.device, 2 * P * P + 7 * P)
        d_wA, d_bA, d_w1, d_b1 = flat[:4 * P].view(2 * P, 2), flat[4 * P:6 * P], flat[6 * P:6 * P + 2 * P * P].view(P, 2 * P), flat[6 * P + 2 * P * P:]
        nv.call("esc_lappe_encode_bwd", nv.ptr(eigvecs), nv.ptr(eigvals), nv.ptr(signs), nv.ptr(wA), nv.ptr(bA), nv.ptr(w1), nv.ptr(b1),
                nv.ptr(d_out), ldg, N, K, P, nv.ptr(scratch), need, nv.ptr(d_wA), nv.ptr(d_bA), nv.ptr(d_w1), nv.ptr(d_b1), nv.stream())
        return None, None, None, d_wA, d_bA, d_w1, d_b1


def lappe_encode(eigvecs, eigvals, signs, wA, bA, w1, b1):
    """The DeepSet LapPE encoder.  eigvecs [N, K], eigvals [N, K] or [N, K, 1] (NaN-padded, not differentiable), signs [K] of +-1
    or None, wA [2P, 2], bA [2P], w1 [P, 2P], b1 [P] -> [N, P] (the C entry point also writes a column slice of a wider buffer:
    ld_out).  Limits: P a multiple of 4 and at most 32, K <= 32; beyond them RuntimeError before any launch."""
    _dev(eigvecs, eigvals, signs, wA, bA, w1, b1)
    dev = eigvecs.device
    _on(dev, eigvals, signs, wA, bA, w1, b1)
    if eigvecs.dim() != 2:
        raise ValueError("lappe_encode: eigvecs must be [N, K], got %s" % (tuple(eigvecs.shape),))
    N, K = eigvecs.shape
    if eigvals.dim() == 3 and eigvals.size(2) == 1:
        eigvals = eigvals.view(eigvals.size(0), eigvals.size(1))
    if eigvals.shape != eigvecs.shape:
        raise ValueError("lappe_encode: eigvals %s does not match eigvecs %s" % (tuple(eigvals.shape), tuple(eigvecs.shape)))
    if w1.dim() != 2:
        raise ValueError("lappe_encode: w1 must be [P, 2P]")
    P = w1.size(0)
    if P % 4 or not 0 < P <= 32:
        raise RuntimeError("lappe_encode: dim_pe %d must be a multiple of 4 and at most 32" % P)
    if not 1 <= K <= 32:
        raise RuntimeError("lappe_encode: max_freqs %d outside 1..32" % K)
    if tuple(wA.shape) != (2 * P, 2) or tuple(bA.shape) != (2 * P,) or tuple(w1.shape) != (P, 2 * P) or tuple(b1.shape) != (P,):
        raise ValueError("lappe_encode: expected wA [%d, 2], bA [%d], w1 [%d, %d], b1 [%d]" % (2 * P, 2 * P, P, 2 * P, P))
    if signs is not None and tuple(signs.shape) != (K,):
        raise ValueError("lappe_encode: signs must be [%d]" % K)
    cont = [t.contiguous() for t in (eigvecs.detach(), eigvals.detach(), wA, bA, w1, b1)]
    return _LapPEEncode.apply(cont[0], cont[1], None if signs is None else signs.detach().contiguous(), cont[2], cont[3], cont[4], cont[5])


# ---- random-walk structural encoding (csrc/rwse.hip, include/escgnn_rwse.h) ------------------------------------------------------
def rw_landing_limits():
    """(most nodes, most edges) of one graph esc_rw_landing takes"""
    h = nv.lib()
    return int(h.esc_rw_landing_max_nodes()), int(h.esc_rw_landing_max_edges())


def rw_step_mask(ksteps):
    """the step list as esc_rw_landing takes it: bit k - 1 set for every step k.  ValueError for an empty list, a step outside
    1..63, a repeat or a list that is not ascending (the columns come out in ascending order: the list must say so itself)."""
    try:
        steps = [int(k) for k in ksteps]
        whole = all(k == s for k, s in zip(ksteps, steps))
    except (TypeError, ValueError):
        steps, whole = [], False
    if not steps or not whole:
        raise ValueError("rw_landing: ksteps must be a non-empty list of ints, got %r" % (ksteps,))
    if min(steps) < 1 or max(steps) > 63:
        raise ValueError("rw_landing: steps outside 1..63 in %r" % (steps,))
    if len(set(steps)) != len(steps):
        raise ValueError("rw_landing: a step is repeated in %r" % (steps,))
    if steps != sorted(steps):
        raise ValueError("rw_landing: the steps must be ascending, got %r" % (steps,))
    return sum(1 << (k - 1) for k in steps)


def rw_landing(edge_index, graph_ptr, edge_ptr, ksteps, max_nodes=None, max_edges=None, edges_local=False, num_nodes=None):
    """The landing probabilities (P^k)[i, i], P = D^-1 A, of the k-step random walk for every node of a ragged set of graphs and
    every k of `ksteps` (a list of ascending ints in 1..63), one workgroup per graph, one launch: the reference's
    get_rw_landing_probs with edge_weight None and space_dim 0 (GraphGPS/graphgps/transform/posenc_stats.py:185-231).  The edge
    list is directed and counts as listed: self-loops are kept, duplicates add up, a node without out-edges has a zero row.
    edge_index, graph_ptr, edge_ptr, edges_local: as in laplacian_eig.  Returns pestat_RWSE [N, K] fp32 - fp64 arithmetic
    rounded once.  Not differentiable: the statistics are data.
    max_nodes, max_edges: the largest graph as the HOST knows it, num_nodes: N likewise; None costs one read-back each.
    Limits: rw_landing_limits() = (256, 7678) nodes and edges per graph; beyond them RuntimeError, raised before anything is
    launched."""
    mask = rw_step_mask(ksteps)
    node_limit, edge_limit = rw_landing_limits()
    src, dst, node_ptr, edge_ptr, G, N, max_nodes = _ragged_graphs("rw_landing", node_limit, edge_index, graph_ptr, edge_ptr, max_nodes, num_nodes)
    if max_edges is None:
        max_edges = int((edge_ptr[1:] - edge_ptr[:-1]).max()) if G else 0
    max_edges = int(max_edges)
    if max_edges > edge_limit:
        raise RuntimeError("rw_landing: a graph of %d edges exceeds the limit of %d edges per graph" % (max_edges, edge_limit))
    K = bin(mask).count("1")
    out = _empty(src.device, N, K)
    nv.call("esc_rw_landing", nv.ptr(src), nv.ptr(dst), src.numel(), nv.ptr(node_ptr), nv.ptr(edge_ptr), G, N, int(bool(edges_local)), mask,
            max(max_nodes, 0), max(max_edges, 0), nv.ptr(out), K, nv.stream())
    return out


def rwse_gather(table, node_ptr_all, graph_ids, graph_ptr, num_nodes):
    """The batch's rows of a split's resident pestat_RWSE table (what the reference's collate does to that key), one launch.
    table [N_all, K] fp32; node_ptr_all int64 [G_all+1] (device); graph_ids: the batch's graphs in batch order, a HOST int64
    tensor or list - checked here, an id out of range raises IndexError before anything is launched; graph_ptr int32 [B+1]: the
    batch's node ranges; num_nodes: the batch's N.  Returns [N, K]."""
    node_ptr_all, ids_d, graph_ptr, (G_all, N_all, B, N, K), (out,) = _checked_gather(
        "rwse_gather", (table,), "the table must be a contiguous fp32 [N_all, K] tensor", node_ptr_all, graph_ids, graph_ptr, num_nodes)
    nv.call("esc_rwse_gather", nv.ptr(table), nv.ptr(node_ptr_all), G_all, N_all, nv.ptr(ids_d), nv.ptr(graph_ptr), B, N, K, nv.ptr(out), K,
            nv.stream())
    return out


# ---- shortest-path distances of the attention bias (csrc/spd.hip, include/escgnn_spd.h) ------------------------------------------
def graph_spd_limits():
    """(most nodes, most edges) of one graph esc_graph_spd takes, in the shape of rw_landing_limits(); the edges are not limited:
    None"""
    return int(nv.lib().esc_graph_spd_max_nodes()), None


def _pairs_vector(pair_ptr, like, who):
    pair_ptr = _index_vector(pair_ptr, "%s: pair_ptr" % who, torch.int64)
    if pair_ptr.numel() != like.numel():
        raise ValueError("%s: pair_ptr has %d entries, graph_ptr %d" % (who, pair_ptr.numel(), like.numel()))
    return pair_ptr


def graph_spd(edge_index, graph_ptr, edge_ptr, max_nodes=None, edges_local=False, num_nodes=None, num_pairs=None, pair_ptr=None):
    """The all-pairs shortest-path distances of every graph of a ragged set, one workgroup per graph, one launch: the reference's
    attn_bias key (GraphGPS/graphgps/loader/utils_escgnn.py:29-38: networkx on the undirected graph, 100 where there is no path).
    edge_index, graph_ptr, edge_ptr, edges_local: as in laplacian_eig.  An edge listed in either direction connects both ends;
    self-loops and duplicates change nothing.  Returns uint8 [sum n^2]: entry (i, j) of graph g at pair_ptr[g] + i n + j, the value
    min(d, 100) - a true distance of 100 aliases "no path" as in the reference, and beyond 100 (where the reference's embedding
    lookup raises) the pair reads the same row.  Not differentiable: the distances are data.
    max_nodes, num_nodes, num_pairs (= sum n^2): as the HOST knows them; None costs one read-back each.  pair_ptr: the int64
    scan of n^2 when the caller has it (default: the one cached on graph_ptr, which ops.graph_attention shares).
    Limit: graph_spd_limits()[0] = 256 nodes per graph; beyond it RuntimeError, raised before anything is launched."""
    src, dst, node_ptr, edge_ptr_, G, N, max_nodes = _ragged_graphs("graph_spd", graph_spd_limits()[0], edge_index, graph_ptr, edge_ptr,
                                                                    max_nodes, num_nodes)
    pair_ptr = _pair_ptr(graph_ptr) if pair_ptr is None else _pairs_vector(pair_ptr, graph_ptr, "graph_spd")
    _on(src.device, pair_ptr)
    if num_pairs is None:
        num_pairs = int(pair_ptr[-1])
    num_pairs = int(num_pairs)
    out = torch.empty(max(num_pairs, 0), dtype=torch.uint8, device=src.device)
    nv.call("esc_graph_spd", nv.ptr(src), nv.ptr(dst), src.numel(), nv.ptr(node_ptr), nv.ptr(edge_ptr_), nv.ptr(pair_ptr), G, N, num_pairs,
            int(bool(edges_local)), max(max_nodes, 0), nv.ptr(out), nv.stream())
    return out


def spd_gather(table, pair_ptr_all, node_ptr_all, graph_ids, graph_ptr, num_pairs=None):
    """The batch's bytes of a split's resident distance table (what the reference's collate would do to the attn_bias key), one
    launch.  table uint8 [pairs_all] in pair_ptr_all's layout; pair_ptr_all, node_ptr_all int64 [G_all+1] (device); graph_ids: the
    batch's graphs in batch order, a HOST int64 tensor or list - checked here, an id out of range raises IndexError before
    anything is launched; graph_ptr int32 [B+1]: the batch's node ranges (its pair_ptr is the one cached on it); num_pairs: the
    batch's sum of n^2 as the host knows it (None: one read-back).  Returns uint8 [num_pairs]."""
    who = "spd_gather"
    if not torch.is_tensor(table) or table.dtype != torch.uint8 or table.dim() != 1 or not table.is_contiguous():
        raise TypeError("%s: the table must be a contiguous 1-D uint8 tensor" % who)
    if not table.is_cuda:
        raise RuntimeError("esc_gnn_amd: the hot path runs on the HIP device only (got a %s tensor); there is no CPU fallback" % table.device)
    dev = table.device
    node_ptr_all = _index_vector(node_ptr_all, "%s: node_ptr_all" % who, torch.int64)
    pair_ptr_all = _pairs_vector(pair_ptr_all, node_ptr_all, who)
    graph_ptr = _index_vector(graph_ptr, "%s: graph_ptr" % who, torch.int32)
    _on(dev, node_ptr_all, pair_ptr_all, graph_ptr)
    G_all, B = node_ptr_all.numel() - 1, graph_ptr.numel() - 1
    if torch.is_tensor(graph_ids) and graph_ids.is_cuda:
        raise RuntimeError("%s: graph_ids must live on the host (they are checked there, without a read-back)" % who)
    ids_h = torch.as_tensor(graph_ids, dtype=torch.int64).reshape(-1)
    if ids_h.numel() != B:
        raise ValueError("%s: %d graph ids for a batch of %d graphs" % (who, ids_h.numel(), B))
    if B and (int(ids_h.min()) < 0 or int(ids_h.max()) >= G_all):
        raise IndexError("%s: graph id out of range (the table holds %d graphs)" % (who, G_all))
    pair_ptr = _pair_ptr(graph_ptr)
    if num_pairs is None:
        num_pairs = int(pair_ptr[-1])
    num_pairs = int(num_pairs)
    ids_d = ids_h.to(dev, non_blocking=True)
    out = torch.empty(max(num_pairs, 0), dtype=torch.uint8, device=dev)
    nv.call("esc_spd_gather", nv.ptr(table), nv.ptr(pair_ptr_all), nv.ptr(node_ptr_all), G_all, table.numel(), nv.ptr(ids_d), nv.ptr(graph_ptr),
            nv.ptr(pair_ptr), B, num_pairs, nv.ptr(out), nv.stream())
    return out


# ---- per-graph LayerNorm (csrc/layernorm.hip, include/escgnn_layernorm.h) ----------------------------------------------------------
def graph_layer_norm_max_channels():
    """the widest row esc_graph_layer_norm_fwd / _bwd take (a multiple of 4 from 4 up to this)"""
    return int(nv.lib().esc_graph_layer_norm_max_channels())


class _GraphLayerNorm(Function):
    """PyG's norm.LayerNorm in graph mode (the reference's gt.layer_norm, gps_layer.py:143-145,161,226-227,249-250,261-262: one mean
    and one variance over all nodes and channels of each graph) on x, or on x + residual with the add folded in: one launch
    forward, two backward (one without an affine).  Saves x, the residual and stats [G, 2] = (mean, rstd); the backward
    recomputes xhat from them.  d_x is also the residual's gradient: written once, returned for both."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, graph_ptr, eps):
        x, ldx = _rows(x)
        N, C = x.shape
        G, dev = graph_ptr.numel() - 1, x.device
        ldr = C
        if residual is not None:
            residual, ldr = _rows(residual, C)
        y, stats = _empty(dev, N, C), _empty(dev, G, 2)
        nv.call("esc_graph_layer_norm_fwd", nv.ptr(x), ldx, nv.ptr(residual), ldr, nv.ptr(graph_ptr), G, N, C, nv.ptr(weight), nv.ptr(bias),
                float(eps), nv.ptr(y), C, nv.ptr(stats), nv.stream())
        ctx.save_for_backward(x, residual, weight, stats)
        ctx.graph_ptr = graph_ptr
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)                       # no zero-filled gradient of stats: two launches per backward
        return y, stats

    @staticmethod
    def backward(ctx, g, _unused):
        if g is None:
            return (None,) * 6
        x, residual, weight, stats = ctx.saved_tensors
        graph_ptr = ctx.graph_ptr
        _dev(g)
        x, ldx = _rows(x)
        N, C = x.shape
        G, dev = graph_ptr.numel() - 1, x.device
        ldr = C
        if residual is not None:
            residual, ldr = _rows(residual, C)
        g, ldg = _rows(g)
        d_x = _empty(dev, N, C)
        affine = weight is not None
        d_weight, d_bias, partial = (_empty(dev, C), _empty(dev, C), _empty(dev, max(G, 1), 2, C)) if affine else (None, None, None)
        nv.call("esc_graph_layer_norm_bwd", nv.ptr(x), ldx, nv.ptr(residual), ldr, nv.ptr(stats), nv.ptr(g), ldg, nv.ptr(graph_ptr), G, N, C,
                nv.ptr(weight), nv.ptr(d_x), C, nv.ptr(d_weight), nv.ptr(d_bias), nv.ptr(partial), nv.stream())
        return d_x, (d_x if residual is not None else None), d_weight, d_bias, None, None


def graph_layer_norm(x, graph_ptr, weight, bias, eps=1e-5, residual=None, return_stats=False):
    """y = LayerNorm over all nodes and channels of each graph (PyG norm.LayerNorm(C)(h, batch)) of h = x, or of h = x + residual
    with the add folded into the launch (one fp32 addition per element: the same bits as adding beforehand).  x, residual: [N, C]
    rows (a column slice of wider rows is read in place); graph_ptr: int32 [G+1] node ranges on the device; weight, bias: [C],
    both or neither (None: no affine).  The variance is the centred second pass.  A graph's rows have the same bits alone and
    inside any batch; an empty graph writes nothing.  Differentiable in x, residual, weight and bias.
    return_stats: also stats [G, 2] = (mean, rstd) of every graph, what the backward reads.
    Limits: C a multiple of 4 from 4 up to graph_layer_norm_max_channels() - ValueError before anything is launched; there is
    no limit on the nodes of a graph."""
    _dev(x, residual, weight, bias)
    _on(x.device, residual, weight, bias, graph_ptr)
    if x.dim() != 2:
        raise ValueError("graph_layer_norm: expected a 2-D tensor, got shape %s" % (tuple(x.shape),))
    C = x.size(1)
    _width_limit("graph_layer_norm", C, graph_layer_norm_max_channels())
    if residual is not None and tuple(residual.shape) != tuple(x.shape):
        raise ValueError("graph_layer_norm: residual %s must have the shape of x %s" % (tuple(residual.shape), tuple(x.shape)))
    if (weight is None) != (bias is None):
        raise ValueError("graph_layer_norm: weight and bias come together (got %s)" % ("weight alone" if bias is None else "bias alone"))
    if weight is not None and (tuple(weight.shape) != (C,) or tuple(bias.shape) != (C,)):
        raise ValueError("graph_layer_norm: weight %s and bias %s must be [%d]" % (tuple(weight.shape), tuple(bias.shape), C))
    if graph_ptr.dtype != torch.int32 or graph_ptr.dim() != 1 or graph_ptr.numel() < 1:
        raise TypeError("graph_layer_norm: graph_ptr must be a 1-D int32 tensor of G+1 node offsets")
    if weight is not None:
        weight, bias = weight.contiguous(), bias.contiguous()
    y, stats = _GraphLayerNorm.apply(x, residual, weight, bias, graph_ptr.contiguous(), eps)
    return (y, stats) if return_stats else y
