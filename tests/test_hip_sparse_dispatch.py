"""One run per kernel family of the index-driven row kernels (csrc/aggregate.hip, bag.hip, embed.hip, gineplus.hip, gatedgcn.hip).

The cases come from tests/sparse_cases.py: for every member of FAMILIES the first table case that reaches it and has a structure to
run on, so that tests/test_sparse_plan_cpu.py (which holds csrc/sparse_plan.h to the table's family_of) proves which family a run
reaches.  Results are held to the references the structure tests use: the sequential loops of tests/graph_cases.py bit for bit
(aggregate forward, bag forward, segment pool; d_e of the aggregate is a masked copy: exact), fp64 at the suite's 1e-5 where a kernel
sums in its own fixed order (dx, deps, the table gradients), gineplus_cases' loops and bound, gatedgcn_oracle at its bound.  The query
entries are held to sparse_cases on the same cases.  Operands are laid out as the case says (leading dimension, base offset); what
lies outside them must stay untouched.  Families behind ESC_AGG_SPLIT_BWD / ESC_BAG_TILED run in a fresh child process, because the
switches are read once."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, require_gpu
import gatedgcn_oracle as gg
import graph_cases as gc
import sparse_cases as sc
from sparse_cases import cdiv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 777.25                                     # what lies around an operand before a kernel runs
NAN = float("nan")
TOL = 1e-5                                        # the suite's bound on sums the kernels order themselves (test_hip_sparse_structure.py)
GPU_CASES = [c for c in (sc.gpu_case_of(f) for f in sc.FAMILIES) if c is not None]
HERE = [c.name for c in GPU_CASES if sc._knobs(c) == sc.KNOB_DEFAULTS]
SWITCHED = sorted({tuple(sorted(c.knobs.items())) for c in GPU_CASES if sc._knobs(c) != sc.KNOB_DEFAULTS})
ENV = {"agg_split": "ESC_AGG_SPLIT", "agg_split_bwd": "ESC_AGG_SPLIT_BWD", "bag_tiled": "ESC_BAG_TILED"}


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    torch.set_num_threads(1)
    return esc_gnn_amd


# ---- operands laid out as a case says --------------------------------------------------------------------------------------
def _place(t, lay, fill=None):
    """(buffer, view): a [rows, C] device view with leading dimension lay[0] whose base lies lay[1] floats past a 16-byte boundary,
    holding t (or `fill`), inside a buffer that holds SENT everywhere else"""
    rows, C = t.shape
    ld, off = lay
    buf = torch.full((rows * ld + off + 8,), SENT, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = torch.as_strided(buf, (rows, C), (ld, 1), off)
    if fill is None:
        view.copy_(t)
    else:
        view.fill_(fill)
    return buf, view


def _untouched(buf, view, what):
    outside = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(outside, tuple(view.shape), tuple(view.stride()), view.storage_offset()).fill_(False)
    assert bool((buf[outside] == SENT).all()), "%s: the kernel wrote outside its rows" % what


def _ld(lay, op):
    return lay[op][0] if lay[op] is not None else 0


def _close(got, want64, what, tol=TOL):
    """max |got - want| over the largest |want| (at least 1): test_hip_sparse_structure._chk"""
    got, want64 = got.detach().cpu().double(), want64.detach().double()
    scale = max(1.0, float(want64.abs().max())) if want64.numel() else 1.0
    err = float((got - want64).abs().max()) / scale if want64.numel() else 0.0
    assert err <= tol, "%s: max error %.3g of scale %.3g > %g" % (what, err, scale, tol)


_PLANS = {}


def _plan(E, name):
    if name not in _PLANS:
        c = gc.case(name)
        bag = [c[k].to(DEV) for k in ("pos_enc", "pos_index", "pos_batch")] if "pos_batch" in c else [None, None, None]
        _PLANS[name] = E.BatchPlan.from_tensors(c["edge_index"].to(DEV), c["num_nodes"], *bag)
    return _PLANS[name]


def _launches(nv, kind, fn):
    """fn() with the launches of a kernel family counted"""
    nv.prof_reset(kind)
    nv.prof_enable(kind, True)
    try:
        fn()
        torch.cuda.synchronize()
        return nv.prof_read(kind)[0]
    finally:
        nv.prof_enable(kind, False)
        nv.prof_reset(kind)


# ---- GINE aggregate ------------------------------------------------------------------------------------------------------------
def _run_aggregate(E, c, fam, want):
    nv, lib, s = E._native, E._native.lib(), E._native.stream()
    g, plan, lay, k = gc.case(c.graph), _plan(E, c.graph), sc.layout_of(c), sc._knobs(c)
    ei = g["edge_index"]
    N, Ne, C = c.N, ei.shape[1], c.C
    assert N == g["num_nodes"]
    gen = torch.Generator().manual_seed(3000 + C)
    x, e, gr = torch.randn(N, C, generator=gen), torch.randn(Ne, C, generator=gen), torch.randn(N, C, generator=gen)
    scale, shift = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen)
    mean, invstd = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
    eps = torch.tensor([0.3])
    scd, shd, meand, invd, epsd = (t.to(DEV) for t in (scale, shift, mean, invstd, eps))
    affine = c.entry not in ("agg_fwd", "agg_bwd")
    xa = x                                               # the rows the plain kernels would be given
    if affine:                                           # relu(x * scale + shift) by the elementwise kernel the step would have run
        xad = torch.empty(N, C, device=DEV)
        nv.call("esc_affine_act", nv.ptr(x.to(DEV)), C, N, C, nv.ptr(scd), nv.ptr(shd), 1, nv.ptr(xad), C, s)
        xa = xad.cpu()
    use_e = lay["e"] is not None
    xv = _place(x, lay["x"])[1]
    ev = _place(e, lay["e"])[1] if use_e else None
    aff = (nv.ptr(scd), nv.ptr(shd)) if affine else ()
    if c.entry in ("agg_fwd", "agg_fwd_affine"):
        ob, ov = _place(x, lay["out"], fill=NAN)
        call = lambda: nv.call("esc_gine_aggregate_fwd" + ("_affine" if affine else ""), nv.ptr(xv), _ld(lay, "x"), *aff, nv.ptr(ev), _ld(lay, "e"),
                               nv.ptr(plan.in_ptr), nv.ptr(plan.in_edge), nv.ptr(plan.in_src), nv.ptr(epsd), N, C, nv.ptr(ov), _ld(lay, "out"), s)
        if "span" in c.flags:                            # the stamped instantiation alone writes an execution window
            nv.prof_reset("agg_fwd")
            nv.prof_span_arm("agg_fwd", 1)
            assert _launches_keep(nv, "agg_fwd", call) == 1
            spans = nv.prof_span_read("agg_fwd")
            nv.prof_reset("agg_fwd")
            assert (len(spans) == 1 and spans[0] > 0.0) == fam.endswith("+span"), (fam, spans)
        else:
            call()
        assert torch.equal(ov.cpu(), gc.aggregate_loop(xa, e if use_e else None, eps, ei)), c.name
        _untouched(ob, ov, c.name)
        return
    slots = int(lib.esc_gine_aggregate_bwd_deps_slots(C))
    assert slots == sc.deps_slots(C, k) and int(lib.esc_gine_aggregate_bwd_stats_slots(N)) == cdiv(N, 4)
    gv = _place(gr, lay["g"])[1]
    deb, dev_ = _place(e, lay["d_e"], fill=NAN) if lay["d_e"] is not None else (None, None)
    dxb, dxv = _place(x, lay["dx"], fill=NAN) if lay["dx"] is not None else (None, None)
    part = torch.full((N * slots,), NAN, device=DEV)
    stats = torch.full((want["slots"], C, 2), NAN, device=DEV) if c.entry == "agg_bwd_stats" else None
    bn = (nv.ptr(meand), nv.ptr(invd)) if stats is not None else ()
    tail = (nv.ptr(stats),) if stats is not None else ()
    nv.call("esc_gine_aggregate_bwd" + {"agg_bwd": "", "agg_bwd_affine": "_affine", "agg_bwd_stats": "_affine_stats"}[c.entry], nv.ptr(xv), _ld(lay, "x"),
            *aff, *bn, nv.ptr(ev), _ld(lay, "e"), nv.ptr(gv), _ld(lay, "g"), nv.ptr(plan.out_ptr), nv.ptr(plan.out_edge), nv.ptr(plan.out_dst), nv.ptr(epsd),
            N, C, nv.ptr(dev_), _ld(lay, "d_e"), nv.ptr(dxv), _ld(lay, "dx"), 0, nv.ptr(part), *tail, s)
    x64, eps64 = xa.double().requires_grad_(True), eps.double().requires_grad_(True)
    msg = x64.index_select(0, ei[0]) + e.double() if use_e else x64.index_select(0, ei[0])
    (torch.zeros_like(x64).index_add(0, ei[1], msg.relu()) + (1 + eps64) * x64).backward(gr.double())
    if dev_ is not None:                                 # a masked copy: exact
        pre = xa.index_select(0, ei[0]) + e
        assert torch.equal(dev_.cpu(), torch.where(pre > 0, gr.index_select(0, ei[1]), torch.zeros(()))), c.name + ": d_e"
        _untouched(deb, dev_, c.name + " d_e")
    if dxv is not None:
        err = (dxv.cpu().double() - x64.grad).abs()
        assert bool((err <= TOL + TOL * x64.grad.abs()).all()), "%s: dx misses fp64 by %.3g" % (c.name, float(err.max()))
        _untouched(dxb, dxv, c.name + " dx")
    written = part[:N * want["split"]]                   # wave w writes deps_part[w]: `split` waves per row, inside the N * slots promised
    assert want["split"] <= slots and not bool(torch.isnan(written).any()), c.name + ": a deps slot was not written"
    assert bool(torch.isnan(part[N * want["split"]:]).all()), c.name + ": deps_part written past the waves of the launch"
    assert torch.allclose(written.double().sum().cpu().view(1), eps64.grad, rtol=1e-5, atol=1e-4), c.name + ": deps"
    if stats is not None:                                # every partial slot written, their column sums against fp64
        assert not bool(torch.isnan(stats).any()), c.name + ": a BatchNorm partial slot was not written"
        pre = x.double() * scale.double() + shift.double()
        gm = torch.where(pre > 0, dxv.cpu().double(), torch.zeros((), dtype=torch.float64))
        _close(stats[:, :, 0].double().sum(0), gm.sum(0), c.name + ": sum g")
        _close(stats[:, :, 1].double().sum(0), (gm * ((x.double() - mean.double()) * invstd.double())).sum(0), c.name + ": sum g*xhat")


def _launches_keep(nv, kind, fn):
    """as _launches, without resetting the family's records (the spans are read afterwards)"""
    nv.prof_enable(kind, True)
    try:
        fn()
        torch.cuda.synchronize()
        return nv.prof_read(kind)[0]
    finally:
        nv.prof_enable(kind, False)


def _run_pool(E, c, fam, want):
    nv, s = E._native, E._native.stream()
    g, lay, C = gc.case(c.graph), sc.layout_of(c), c.C
    G, batch, n = g["num_graphs"], g["batch"], g["num_nodes"]
    assert c.N == G
    seg = torch.tensor(np.concatenate([[0], np.cumsum(np.bincount(batch.numpy(), minlength=G))]), dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(4000 + C)
    x, gr = torch.randn(n, C, generator=gen), torch.randn(G, C, generator=gen)
    xv = _place(x, lay["x"])[1]
    ob, ov = _place(gr, lay["out"], fill=NAN)
    nv.call("esc_segment_pool_fwd", nv.ptr(xv), _ld(lay, "x"), nv.ptr(seg), G, C, 0, nv.ptr(ov), _ld(lay, "out"), s)
    assert torch.equal(ov.cpu(), gc.segment_sum_loop(x, batch, G)), c.name
    _untouched(ob, ov, c.name)
    gv = _place(gr, lay["out"])[1]                       # the backward in the mirrored layout: the same family
    dxb, dxv = _place(x, lay["x"], fill=NAN)
    nv.call("esc_segment_pool_bwd", nv.ptr(gv), _ld(lay, "out"), nv.ptr(seg), G, C, 0, nv.ptr(dxv), _ld(lay, "x"), s)
    assert torch.equal(dxv.cpu(), gr[batch]), c.name + " backward"
    _untouched(dxb, dxv, c.name + " backward")


# ---- the ESC bag ---------------------------------------------------------------------------------------------------------------
def _run_bag_fwd(E, c, fam, want):
    """the statistics epilogue leaves (mean, M2) of every 128 output rows per column.  Bound: a Welford step is four fp32 roundings of
    quantities no larger than the running mean / M2, the merge of the 16 lane groups as many per group: 4 * 128 * 2^-24 of the largest
    value of each, to first order"""
    nv, lib, s = E._native, E._native.lib(), E._native.stream()
    g, plan, lay, H = gc.case(c.graph), _plan(E, c.graph), sc.layout_of(c), c.C
    Ne = plan.num_edges
    assert (c.N, c.Z) == (Ne, plan.nnz) and lay["table"] == (H, 0)
    gen = torch.Generator().manual_seed(5000 + H)
    W, base = torch.randn(g["n_cols"], H, generator=gen), torch.randn(Ne, H, generator=gen)
    Wd = W.to(DEV)
    acc = c.entry == "bag_fwd_acc" or "acc" in c.flags
    ob, ov = _place(base, lay["out"], fill=None if acc else NAN)
    bag = (nv.ptr(plan.row_ptr), nv.ptr(plan.bag_idx), nv.ptr(plan.bag_val), Ne, nv.ptr(ov), _ld(lay, "out"))
    stats = None
    if c.entry != "bag_fwd_rows":
        nv.call("esc_" + c.entry, nv.ptr(Wd), H, *bag, s)
    else:
        assert c.rows == g["n_cols"]
        block = int(lib.esc_bag_fwd_stats_block_rows(nv.ptr(Wd), c.rows, H, nv.ptr(ov), _ld(lay, "out"), Ne))
        assert block == (sc.BAG_EB if sc.tiled_ok(c, lay, sc._knobs(c)) else 0)
        stats = torch.full((cdiv(Ne, sc.BAG_EB), H, 2), NAN, device=DEV) if "stats" in c.flags else None
        call = lambda: nv.call("esc_bag_fwd_rows", nv.ptr(Wd), c.rows, H, *bag, int(acc), nv.ptr(stats), s)
        if want["refused"]:                              # an error, never a silent other path
            with pytest.raises(RuntimeError):
                call()
            torch.cuda.synchronize()
            assert bool(torch.isnan(ov).all()) and bool(torch.isnan(stats).all())
            return
        call()
    out = gc.bag_loop(W, g["pos_enc"], g["pos_index"], g["pos_batch"], Ne, base=base if acc else None)
    assert torch.equal(ov.cpu(), out), c.name
    _untouched(ob, ov, c.name)
    if stats is not None:
        assert want["slots"] == sc.BAG_EB and not bool(torch.isnan(stats).any()), c.name
        blocks = out.double().split(sc.BAG_EB)
        mean = torch.stack([b.mean(0) for b in blocks])
        m2 = torch.stack([((b - b.mean(0)) ** 2).sum(0) for b in blocks])
        bound = 4 * sc.BAG_EB * 2.0 ** -24
        assert float((stats[:, :, 0].cpu().double() - mean).abs().max()) <= bound * float(out.abs().max()), c.name + ": mean"
        assert float((stats[:, :, 1].cpu().double() - m2).abs().max()) <= bound * float(m2.max()), c.name + ": M2"


def _bag_bwd_operands(E, c):
    """(plan arrays, Z, edges, n_cols, the structure or None): the `no_entries` structure is an all-empty column pointer"""
    if c.graph == "no_entries":
        return (torch.zeros(sc.N_COLS + 1, dtype=torch.int32, device=DEV), None, None, None), 0, c.N, sc.N_COLS, None
    plan = _plan(E, c.graph)
    return (plan.col_ptr, plan.col_row, plan.col_val, plan.col_col), plan.nnz, plan.num_edges, plan.n_cols, gc.case(c.graph)


def _run_bag_bwd(E, c, fam, want):
    nv, lib, s = E._native, E._native.lib(), E._native.stream()
    (col_ptr, col_row, col_val, col_col), Z, Ne, n_cols, g = _bag_bwd_operands(E, c)
    lay, H = sc.layout_of(c), c.C
    assert (c.N, c.Z, n_cols) == (Ne, Z, sc.N_COLS) and lay["dtable"] == (H, 0) and lay["partials"] == (H, 0)
    floats = int(lib.esc_bag_bwd_scratch(Z, H))
    assert floats == sc.scratch_floats(Z, H)
    dz = torch.randn(Ne, H, generator=torch.Generator().manual_seed(6000 + H))
    dzv = _place(dz, lay["dz"])[1]
    head = (nv.ptr(dzv), _ld(lay, "dz"), H, nv.ptr(col_ptr), nv.ptr(col_row), nv.ptr(col_val), nv.ptr(col_col), Z, n_cols)

    def run(entry, classified):
        dtable = torch.full((n_cols, H), NAN, device=DEV)
        scratch = torch.full((max(1, floats),), NAN, device=DEV)
        if classified:
            nv.call("esc_bag_bwd_classify", nv.ptr(col_row), Z, H, c.rows, nv.ptr(scratch), s)
        mid = (c.rows, int(classified)) if entry == "esc_bag_bwd_table_rows" else ()
        n = _launches(nv, "bag_bwd", lambda: nv.call(entry, *head, *mid, nv.ptr(dtable), nv.ptr(scratch), s))
        return dtable, n
    got, n = run("esc_bag_bwd_table" if c.entry == "bag_bwd" else "esc_bag_bwd_table_rows", "classified" in c.flags)
    assert n == len(want["grids"]), (c.name, n, want["grids"])               # [classify,] pass 1, pass 2: which schedule ran
    assert not bool(torch.isnan(got).any()), c.name + ": a table row was not written"
    if g is None:
        assert float(got.abs().sum()) == 0.0 and not bool(torch.signbit(got).any()), c.name
        return
    pe, pi, pb = g["pos_enc"], g["pos_index"], g["pos_batch"]
    _close(got, torch.zeros(n_cols, H, dtype=torch.float64).index_add_(0, pi, dz.double()[pb] * pe.double().view(-1, 1)), c.name)
    assert float(got.cpu()[torch.tensor(gc.column_lengths(g) == 0)].abs().sum()) == 0.0, c.name + ": a column without entries is not zero"
    plain, n_plain = run("esc_bag_bwd_table", False)                         # placement affects speed only
    assert n_plain == 2 and torch.equal(plain, got), c.name + ": the schedule changed the sums"


def _run_classify(E, c, fam, want):
    nv, s = E._native, E._native.stream()
    g, plan, H = gc.case(c.graph), _plan(E, c.graph), c.C
    Z = plan.nnz
    assert (c.N, c.Z) == (plan.num_edges, Z)
    chunks = cdiv(Z, sc.BAG_CH)
    scratch = torch.full((sc.scratch_floats(Z, H),), NAN, device=DEV)
    n = _launches(nv, "bag_bwd", lambda: nv.call("esc_bag_bwd_classify", nv.ptr(plan.col_row), Z, H, c.rows, nv.ptr(scratch), s))
    assert n == len(want["grids"]), (c.name, n)
    if not want["grids"]:
        assert bool(torch.isnan(scratch).all()), c.name + ": nothing to build, yet the scratch was written"
        return
    words = scratch.view(torch.int32).cpu().numpy()                          # order [8][chunks], then bucket_cnt [8], behind the partials
    order, count = words[2 * chunks * H:2 * chunks * H + 8 * chunks].reshape(8, chunks), words[2 * chunks * H + 8 * chunks:][:8]
    buckets = gc.chunk_buckets(g, c.rows)
    assert np.array_equal(count, np.bincount(buckets, minlength=8)) and int(count.sum()) == chunks, c.name
    for b in range(8):
        assert sorted(order[b, :count[b]].tolist()) == np.flatnonzero(buckets == b).tolist(), (c.name, b)
    assert bool(torch.isnan(scratch[:2 * chunks * H]).all()), c.name + ": the chunk partials are not the classify launch's to write"


def _run_embed(E, c, fam, want):
    nv, s = E._native, E._native.stream()
    lay, M, rows, C = sc.layout_of(c), c.N, c.rows, c.C
    assert lay["dtable"] == (C, 0)
    idx = (torch.arange(M, dtype=torch.int64) * 7 + 3) % rows
    gr = torch.randn(M, C, generator=torch.Generator().manual_seed(7000 + C))
    gv = _place(gr, lay["g"])[1]
    dtable = torch.full((rows, C), NAN, device=DEV)
    nv.call("esc_embed_bwd", nv.ptr(gv), _ld(lay, "g"), nv.ptr(idx.to(DEV)), M, rows, C, nv.ptr(dtable), s)
    assert not bool(torch.isnan(dtable).any()), c.name
    _close(dtable, torch.zeros(rows, C, dtype=torch.float64).index_add_(0, idx, gr.double()), c.name)


# ---- GINE+ and GatedGCN: through their ops, against their own oracles ------------------------------------------------------------
def _run_gineplus(E, c, fam, want):
    import gineplus_cases as gp
    import test_hip_gineplus_structure as tg
    assert c.layout == "" and not c.absent and c.N == gp.case(c.graph)["num_nodes"]
    assert int(E._native.lib().esc_gineplus_bwd_blocks(c.N)) == sc.gp_bwd_blocks(c.N)
    r = gp.reference(c.graph, c.k, c.C)
    out, dx, d_e, d_eps = tg._gpu(E, c.graph, c.k, c.C)
    if c.entry == "gp_fwd":
        tg._same(out, r["out"], c.name + " out")
        return
    for t in range(c.k):
        tg._same(dx[t], r["dx"][t], c.name + " dx_%d" % t)
    tg._same(d_e, r["d_e"], c.name + " d_e")
    ratio = tg._deps_ratios(c.graph, c.k, c.C, d_eps)[0]
    assert tuple(d_eps.shape) == (c.k + 1, c.C) and ratio <= 1.0, "%s: d_eps %.3g x the bound of its summation order" % (c.name, ratio)


def _run_gated(E, c, fam, want):
    import test_hip_gatedgcn as tgat
    assert c.N == gg.CASES[c.graph][0]
    ref = gg.reference(c.graph, c.C, True)
    out, e_out, x = tgat.run_op(E, c.graph, c.C, True)
    got = dict(out=out, e_out=e_out) if c.entry == "gated_fwd" else {"d_" + k: t.grad for k, t in zip(tgat.OPERANDS, x)}
    for k, v in got.items():
        tgat.check("%s %s" % (c.name, k), v, ref[torch.float64][k], ref[torch.float32][k], gg.scale_floor(c.graph, c.C, True, k))


RUNNERS = {"agg_fwd": _run_aggregate, "agg_bwd": _run_aggregate, "pool": _run_pool, "bag_fwd": _run_bag_fwd, "bag_bwd": _run_bag_bwd,
           "classify": _run_classify, "embed_bwd": _run_embed, "gp_fwd": _run_gineplus, "gp_bwd": _run_gineplus, "gated_fwd": _run_gated,
           "gated_bwd": _run_gated}


def run_case(E, c):
    """one table case on the device, under the switches the library was loaded with (the caller sees to it that they are the case's)"""
    fam = sc.family_of(c.entry, c)
    assert fam in sc.FAMILIES
    RUNNERS[fam.split(":")[0]](E, c, fam, sc.expected(c))
    torch.cuda.synchronize()


def test_every_family_has_its_run():
    ran = {sc.family_of(c.entry, c) for c in GPU_CASES}
    assert ran == set(sc.FAMILIES) - {"classify:launch"}                     # the counters-only launch is the step engine's (see the CPU test)
    assert len(HERE) + sum(len(_names(k)) for k in SWITCHED) == len(GPU_CASES)


@pytest.mark.parametrize("name", HERE)
def test_family_at_the_default_switches(E, name):
    run_case(E, sc.BY_NAME[name])


CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import esc_gnn_amd
import sparse_cases as sc
import test_hip_sparse_dispatch as t
for name in %r:
    t.run_case(esc_gnn_amd, sc.BY_NAME[name])
    print("ran", name, sc.family_of(sc.BY_NAME[name].entry, sc.BY_NAME[name]))
print("switched families ok")
"""


def _names(knobs):
    return [c.name for c in GPU_CASES if tuple(sorted(c.knobs.items())) == knobs]


@pytest.mark.parametrize("knobs", SWITCHED, ids=lambda k: ",".join("%s=%d" % kv for kv in k))
def test_switched_families_in_a_child_process(knobs):
    require_gpu()
    env = dict(os.environ, **{ENV[k]: str(v) for k, v in knobs})
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), _names(knobs))], env=env, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "switched families ok" in r.stdout, r.stdout[-3000:]
