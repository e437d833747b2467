"""The dense-layer entry points (csrc/linear_mfma.hip, gemm_dma.h, linear_small.h) on every dispatch branch, operand layout
and scratch plan of tests/linear_cases.py.

Every operand is a view into a larger allocation whose padding columns and guard rows hold NaN (inputs) or a sentinel bit
pattern (outputs); the reference is fp64 on the CPU from the live regions only, the bound is the project's 1e-5 of
max(1, max |reference|).  A kernel that depends on the floats between `width` and `ld`, reads a row past M, or skips the
mask of a partial last K-step turns NaN; one that writes outside its output trips the sentinel.  The weight-gradient
scratch is exactly esc_linear_bwd_weight_scratch() floats followed by a guard as large as the densest plan (one slab per
32 rows), so a mis-sized plan lands in memory the test owns and is reported.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, require_gpu
import linear_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
EPS = 1e-5


class ReduceJob(ctypes.Structure):
    """mirror of `esc_reduce_job` (include/escgnn_hip.h)"""
    _fields_ = [("slabs", ctypes.c_void_p), ("n", ctypes.c_int64), ("splits", ctypes.c_int32), ("cols", ctypes.c_int64),
                ("dw", ctypes.c_void_p), ("ld_dw", ctypes.c_int64), ("db_part", ctypes.c_void_p), ("rows", ctypes.c_int64),
                ("db", ctypes.c_void_p)]


@pytest.fixture(scope="module")
def nv():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd._native


def _err(got, want):
    want = want.double()
    return float((got.double() - want).abs().max()) / max(1.0, float(want.abs().max()))


def _ptr(ops, name):
    b = ops.inputs.get(name) or ops.outputs.get(name)
    return None if b is None else b.ptr()


def _block_rows(nv, ops):
    c = ops.case
    return int(nv.lib().esc_linear_stats_block_rows(_ptr(ops, "X"), ops.lay["X"][0], _ptr(ops, "W"), ops.lay["W"][0], c.M, c.N, c.K))


def _launch(nv, case, promised=None, slabs_ptr=None, job=None, entry=None):
    """build the guarded operands of `case` on the GPU and make the one library call; returns the Operands"""
    lib, e = nv.lib(), entry or case.entry
    c = case._replace(entry=e)
    M, N, K = c.M, c.N, c.K
    if e in ("bwd_weight", "bwd_both") and promised is None and slabs_ptr is None:
        promised = int(lib.esc_linear_bwd_weight_scratch(M, N, K))
    ops = lc.Operands(c, DEV, promised)
    ld = lambda op: ops.lay[op][0]
    p = lambda name: _ptr(ops, name)
    slabs = slabs_ptr if slabs_ptr is not None else p("slabs")
    s = nv.stream()
    if e == "fwd":
        if N > 32:
            ops.block_rows = _block_rows(nv, ops)
            # guard rows for the finest partition any kernel writes (32-row blocks), should the library's answer be wrong
            ops.outputs["stats"] = lc.output(lc.cdiv(M, ops.block_rows), 2 * N, 2 * N, 0, guard_rows=lc.cdiv(M, 32) + 2, device=DEV)
        nv.call("esc_linear_fwd", p("X"), ld("X"), p("W"), ld("W"), p("B"), p("scale"), p("shift"), M, N, K, p("Y"), ld("Y"),
                p("stats"), s)
    elif e == "bwd_input":
        nv.call("esc_linear_bwd_input", p("Y"), ld("Y"), p("W"), ld("W"), M, N, K, p("dX"), ld("dX"), c.accumulate, s)
    elif e == "bwd_weight":
        nv.call("esc_linear_bwd_weight", p("Y"), ld("Y"), p("X"), ld("X"), p("scale"), p("shift"), M, N, K, p("dW"), ld("dW"),
                p("db"), slabs, s)
    elif job is None:
        nv.call("esc_linear_bwd_both", p("Y"), ld("Y"), p("X"), ld("X"), p("scale"), p("shift"), p("W"), ld("W"), M, N, K,
                p("dX"), ld("dX"), c.accumulate, p("dW"), ld("dW"), p("db"), slabs, s)
    else:
        nv.call("esc_linear_bwd_both_deferred", p("Y"), ld("Y"), p("X"), ld("X"), p("scale"), p("shift"), p("W"), ld("W"), M, N, K,
                p("dX"), ld("dX"), c.accumulate, p("dW"), ld("dW"), p("db"), slabs, ctypes.addressof(job), s)
    torch.cuda.synchronize()
    return ops


def _check(nv, ops):
    """fp64 parity of every output, no NaN left in a live region, sentinels bit-identical, inputs untouched"""
    c, ref, bad = ops.case, ops.reference(), []
    for name, want in ref.items():
        got = ops.outputs[name].result()
        if bool(torch.isnan(got).any()):
            bad.append("%s: %d NaN in the live region" % (name, int(torch.isnan(got).sum())))
            continue
        err = _err(got, want)
        print("%s %s: error %.3g of scale" % (c.name, name, err))
        if err > TOL:
            bad.append("%s: max error %.3g of scale > %g" % (name, err, TOL))
    for name, b in ops.outputs.items():
        n = b.outside_changed()
        if n:
            bad.append("%s: %d floats outside the live region were written" % (name, n))
    for name, b in ops.inputs.items():
        if not b.untouched():
            bad.append("%s: an input was modified" % name)
    if "stats" in ops.outputs:
        bad += _check_stats(nv, ops, ref["Y"])
    assert not bad, "%s [%s]: %s" % (c.name, c.family, "; ".join(bad))


def _check_stats(nv, ops, y):
    c, bad = ops.case, []
    part = ops.outputs["stats"].result().view(-1, c.N, 2)
    if bool(torch.isnan(part).any()):
        return ["col_stats: %d NaN partials at block height %d" % (int(torch.isnan(part).sum()), ops.block_rows)]
    if c.M == 1:                                  # the finalize wants more than one row: a one-row block is (y, 0)
        if _err(part[0, :, 0], y[0]) > TOL or float(part[0, :, 1].abs().max()) != 0.0:
            bad.append("col_stats of one row must be (y, 0)")
        return bad
    mean, invstd = lc.output(1, c.N, c.N, 0, device=DEV), lc.output(1, c.N, c.N, 0, device=DEV)
    nv.call("esc_bn_stats_from_partials_rows", ops.outputs["stats"].ptr(), c.M, c.N, ops.block_rows, EPS, 0.1, mean.ptr(),
            invstd.ptr(), None, None, None, None, None, None, nv.stream())
    torch.cuda.synchronize()
    want_invstd = (y.var(0, unbiased=False) + EPS).rsqrt()
    for name, got, want in (("mean", mean, y.mean(0)), ("invstd", invstd, want_invstd)):
        err = _err(got.result()[0], want)
        if not err <= TOL:
            bad.append("BatchNorm %s from col_stats at block height %d: error %.3g of scale" % (name, ops.block_rows, err))
    return bad


def _ids(cases):
    return [c.name for c in cases]


# ---- 1. forward ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.cases("fwd"), ids=_ids(lc.cases("fwd")))
def test_forward(nv, case):
    ops = _launch(nv, case)
    if case.N > 32:                      # the anchor of the table: the library names the family's row-block height
        assert ops.block_rows == lc.stats_block_rows(case), \
            "%s is meant for %s (%d-row partials), the library answers %d" % (case.name, case.family, lc.stats_block_rows(case),
                                                                            ops.block_rows)
    _check(nv, ops)


# ---- 2. the gradients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.cases("bwd_input"), ids=_ids(lc.cases("bwd_input")))
def test_bwd_input(nv, case):
    _check(nv, _launch(nv, case))


def _same_bits(a, b, names):
    return [n for n in names if n in a.outputs and not torch.equal(a.outputs[n].result().view(torch.int32), b.outputs[n].result().view(torch.int32))]


@pytest.mark.parametrize("case", lc.cases("bwd_weight"), ids=_ids(lc.cases("bwd_weight")))
def test_bwd_weight(nv, case):
    ops = _launch(nv, case)
    _check(nv, ops)
    again = _launch(nv, case)
    assert not _same_bits(ops, again, ("dW", "db")), "dW / db of a second identical call differ (promised bitwise reproducible)"


@pytest.mark.parametrize("case", lc.cases("bwd_both"), ids=_ids(lc.cases("bwd_both")))
def test_bwd_both(nv, case):
    ops = _launch(nv, case)
    _check(nv, ops)
    again = _launch(nv, case)
    assert not _same_bits(ops, again, ("dW", "db")), "dW / db of a second identical call differ (promised bitwise reproducible)"
    # ... and the two separate calls give the same gradients
    w = _launch(nv, case, entry="bwd_weight")
    for n in ("dW", "db"):
        if n in ops.outputs:
            assert _err(ops.outputs[n].result(), w.outputs[n].result()) <= TOL, n
    if case.dx:
        x = _launch(nv, case, entry="bwd_input")
        assert _err(ops.outputs["dX"].result(), x.outputs["dX"].result()) <= TOL


def test_scratch_contract_of_the_narrow_both_kernel(nv):
    """N <= 4 and K <= 16 (a hidden width <= 16 in front of the H -> 1 head): the narrow both-kernel cuts the rows into 32-row
    slabs, so esc_linear_bwd_weight_scratch must promise that plan.  With a promise of (cdiv(M, 128) + 1) * (N*K + N) floats
    these shapes wrote 544 floats into 153 promised (1000 x 1 x 16); the control (100, 4, 256) was always inside."""
    for M, N, K in lc.SCRATCH_BUG_CLASS + (lc.SCRATCH_CONTROL,):
        case = lc.BY_NAME["bwd_both-narrow_both-%dx%dx%d" % (M, N, K)]
        promised = int(nv.lib().esc_linear_bwd_weight_scratch(M, N, K))
        assert lc.scratch_needed("bwd_both", case) <= promised, (case.name, lc.scratch_needed("bwd_both", case), promised)
        ops = _launch(nv, case)
        over = ops.outputs["slabs"].outside_changed()
        print("%s: promised %d, plan %d, %d floats written past the promise" % (case.name, promised, lc.scratch_needed("bwd_both", case), over))
        assert over == 0, "%s: %d floats written past the %d promised" % (case.name, over, promised)


# ---- 3. the deferred form and the multi-job reduce -----------------------------------------------------------------------------------
DEFERRED = ("bwd_both-narrow_both-131x4x100", "bwd_both-split-131x72x10-a", "bwd_both-dma64_dual-131x72x100",
            "bwd_both-r01_dual-131x70x100", "bwd_both-narrow_both-200x4x8", "bwd_both-split-131x72x100-x")


def test_deferred_reduce_jobs(nv):
    """four families (and the two special shapes: the narrow scratch class, dX == NULL) write their slabs into disjoint regions
    of ONE buffer, one esc_slab_reduce_jobs call sums them all: bit-equal to the immediate form, guards between regions intact"""
    lib = nv.lib()
    cases = [lc.BY_NAME[n] for n in DEFERRED]
    assert [c.family for c in cases[:4]] == ["narrow_both", "split", "dma64_dual", "r01_dual"]
    sizes = [(int(lib.esc_linear_bwd_weight_scratch(c.M, c.N, c.K)), lc.scratch_guard(c)) for c in cases]
    starts, at = [], 64
    for promised, guard in sizes:
        starts.append(at)
        at = lc.cdiv(at + promised + guard, 64) * 64
    raw = torch.empty(at + 4, dtype=torch.float32, device=DEV)
    skew = (-(raw.data_ptr() // 4)) % 4
    buf = raw[skew:skew + at]
    buf.fill_(lc.sentinel())
    live = torch.zeros(at, dtype=torch.bool)
    for st, (promised, _) in zip(starts, sizes):
        buf[st:st + promised] = float("nan")
        live[st:st + promised] = True
    jobs = (ReduceJob * len(cases))()
    deferred = [_launch(nv, c, slabs_ptr=buf.data_ptr() + 4 * st, job=jobs[i]) for i, (c, st) in enumerate(zip(cases, starts))]
    for c, j in zip(cases, jobs):
        assert j.n == c.N * c.K and j.cols == c.K and j.rows == c.N and j.splits >= 1, c.name
    nv.call("esc_slab_reduce_jobs", ctypes.addressof(jobs), len(cases), nv.stream())
    torch.cuda.synchronize()
    bits = buf.cpu().view(torch.int32)
    assert int(((bits != lc.SENTINEL_BITS) & ~live).sum()) == 0, "a deferred call wrote outside its slab region"
    for c, ops in zip(cases, deferred):
        _check(nv, ops)
        now = _launch(nv, c)
        assert not _same_bits(ops, now, ("dW", "db", "dX")), "%s: deferred and immediate forms differ" % c.name


# ---- 4. the knobs ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def knobs(nv):
    def set_(knob, value):
        nv.call("esc_tune_set", knob, value)
    try:
        yield set_
    finally:
        nv.call("esc_tune_set", 11, lc.USE_DMA_DEFAULT)
        for k, v in enumerate(lc.KNOB_DEFAULTS):
            nv.call("esc_tune_set", k, v)


def _knob_case(entry, M, N, K, flags=""):
    return lc.Case("knob-%s-%dx%dx%d%s" % (entry, M, N, K, flags), entry, M, N, K, "", "p" in flags, True, int("a" in flags), "r01", True)


KNOB_SHAPES = ((131, 70, 100), (128, 128, 64))


@pytest.mark.parametrize("M,N,K", KNOB_SHAPES)
def test_r01_forward_tiles(nv, knobs, M, N, K):
    knobs(11, 0)
    assert nv.lib().esc_linear_fold_available() == 0
    for tile in range(11):
        knobs(1, tile)
        for flags in ("", "p"):
            ops = _launch(nv, _knob_case("fwd", M, N, K, flags)._replace(name="fwd tile %d %s %dx%dx%d" % (tile, flags, M, N, K)))
            assert ops.block_rows == 32
            _check(nv, ops)


@pytest.mark.parametrize("M,N,K", KNOB_SHAPES)
def test_r01_input_gradient_tiles(nv, knobs, M, N, K):
    knobs(11, 0)
    for tile in range(11):
        knobs(3, tile)
        for flags in ("", "a"):
            _check(nv, _launch(nv, _knob_case("bwd_input", M, N, K, flags)._replace(name="dX tile %d %s %dx%dx%d" % (tile, flags, M, N, K))))


def _r01_splits(M, N, K, tile, blocks):
    bm, bn, bk = lc.R01_TILE_DIMS.get(tile, (64, 64, 32))
    return lc._r01_wgrad_splits(M, N, K, bm, bn, bk, knobs=lc.KNOB_DEFAULTS[:5] + (blocks,) + lc.KNOB_DEFAULTS[6:])


@pytest.mark.parametrize("M,N,K", KNOB_SHAPES)
def test_r01_weight_gradient_tiles(nv, knobs, M, N, K):
    knobs(11, 0)
    promised = int(nv.lib().esc_linear_bwd_weight_scratch(M, N, K))
    for tile in range(8):
        knobs(4, tile)
        for blocks in (1, 512, 4096):
            knobs(5, blocks)
            assert _r01_splits(M, N, K, tile, blocks) * (N * K + N) <= promised
            for flags in ("", "p"):
                _check(nv, _launch(nv, _knob_case("bwd_weight", M, N, K, flags)._replace(
                    name="dW tile %d blocks %d %s %dx%dx%d" % (tile, blocks, flags, M, N, K))))


@pytest.mark.parametrize("M,N,K", KNOB_SHAPES)
def test_r01_dual_launch_tiles(nv, knobs, M, N, K):
    knobs(11, 0)
    for small_tile in (0, 1, 2):
        knobs(7, small_tile)
        for flags in ("", "p", "a"):
            _check(nv, _launch(nv, _knob_case("bwd_both", M, N, K, flags)._replace(
                name="dual knob7=%d %s %dx%dx%d" % (small_tile, flags, M, N, K))))


def test_each_family_bit_moves_only_its_family(nv, knobs):
    """knob 11: bit 0 the LDS-DMA forward, bit 1 its gradients, bit 2 the tiny-dimension kernels, bit 3 the 64x32 tile.
    esc_linear_stats_block_rows / esc_linear_fold_available tell which forward family a mask leaves on; a case per family
    is computed under every single bit (and checked against fp64, whichever kernel serves it)."""
    probes = ("fwd-dma64-131x70x100", "fwd-smallk-131x70x16", "fwd-dma64x32-131x5x100", "fwd-dma128-8193x128x32",
              "bwd_input-dma64_dx-131x72x100", "bwd_input-smalln_dx-131x72x10", "bwd_weight-dma64_dw-131x72x100",
              "bwd_weight-small_dw-131x70x16", "bwd_both-dma64_dual-131x72x100")
    for mask in (1, 2, 4, 8):
        knobs(11, mask)
        assert nv.lib().esc_linear_fold_available() == (1 if mask & 1 else 0)
        for name in probes:
            case = lc.BY_NAME[name]
            ops = _launch(nv, case)
            if case.entry == "fwd" and case.N > 32:
                fam = lc.family_of("fwd", case, use_dma=mask)
                assert fam == (case.family if mask & {"dma64": 1, "dma128": 1, "smallk": 4}[case.family] else "r01")
                assert ops.block_rows == lc.stats_block_rows(case, use_dma=mask) == lc.stats_block_rows_of(fam), (name, mask, ops.block_rows)
            _check(nv, ops)


# ---- 5. the predicates refuse on the host -----------------------------------------------------------------------------------------------
def test_misaligned_operands_are_refused_before_any_launch(nv):
    """one operand misaligned or with ld % 4 != 0: the *_ok predicates answer 0 and the calls return ESC_EINVAL with a message;
    they return before any launch, so the output still holds what it held"""
    lib = nv.lib()
    M, N, K = 131, 72, 100
    s = nv.stream()
    for edit in ("X+1", "X@1", "W+1", "W@1"):
        case = lc.Case("refuse-" + edit, "fwd", M, N, K, edit, False, True, 0, "r01", True)
        ops = lc.Operands(case, DEV)
        y0 = lc.operand(M, N, N, 0, seed=11, device=DEV)
        ld, p = (lambda op: ops.lay[op][0]), (lambda n: _ptr(ops, n))
        assert lib.esc_linear_fwd_from_ok(p("X"), ld("X"), p("W"), ld("W"), M, N, K, 0) == 0, edit
        rc = lib.esc_linear_fwd_from(y0.ptr(), N, p("X"), ld("X"), p("W"), ld("W"), p("B"), None, None, M, N, K, p("Y"), ld("Y"), None, s)
        assert rc == -1 and lib.esc_last_error(), edit
        # the folding forward (MFMA form: N > 32)
        part = torch.zeros(lc.cdiv(M, 64) * K * 2, device=DEV)
        mean, invstd = torch.zeros(K, device=DEV), torch.zeros(K, device=DEV)
        fold = nv.BnFold(partials=part.data_ptr(), rows=M, block_rows=64, C=K, eps=EPS, momentum=0.1, gamma=None, beta=None,
                         mean=mean.data_ptr(), invstd=invstd.data_ptr(), scale=None, shift=None, running_mean=None, running_var=None)
        rc = lib.esc_linear_fwd_fold(p("X"), ld("X"), p("W"), ld("W"), p("B"), ctypes.byref(fold), M, N, K, p("Y"), ld("Y"), None, s)
        assert rc == -1 and lib.esc_last_error(), edit
        torch.cuda.synchronize()
        assert ops.outputs["Y"].untouched() and float(mean.abs().max()) == 0.0, edit
    # the H -> 1 head: X, w or the prologue vectors misaligned
    for edit in ("X+1", "X@1", "W@1", "P@1"):
        case = lc.Case("refuse-l1-" + edit, "fwd", M, 1, K, edit, True, True, 0, "r01", True)
        ops = lc.Operands(case, DEV)
        ld, p = (lambda op: ops.lay[op][0]), (lambda n: _ptr(ops, n))
        target, dpred = lc.operand(1, M, M, 0, seed=5, device=DEV), lc.output(1, M, M, 0, device=DEV)
        assert lib.esc_linear_fwd_l1_ok(p("X"), ld("X"), p("W"), K, p("scale"), p("shift")) == 0, edit
        rc = lib.esc_linear_fwd_l1(p("X"), ld("X"), p("W"), p("B"), p("scale"), p("shift"), M, K, target.ptr(), M, 1.0, p("Y"), dpred.ptr(), s)
        assert rc == -1 and lib.esc_last_error(), edit
        torch.cuda.synchronize()
        assert ops.outputs["Y"].untouched() and dpred.untouched(), edit
    # the Linear backward with the BatchNorm backward folded in
    for edit in ("Y+1", "Y@1", "X+1", "X@1", "W+1", "W@1", "dX+1", "dX@1", "bn"):
        case = lc.Case("refuse-bn-" + edit, "bwd_both", M, N, K, "" if edit == "bn" else edit, False, True, 0, "r01_dual", True)
        ops = lc.Operands(case, DEV, int(lib.esc_linear_bwd_weight_scratch(M, N, K)))
        ld, p = (lambda op: ops.lay[op][0]), (lambda n: _ptr(ops, n))
        bnx = lc.operand(M, N, N + (1 if edit == "bn" else 0), 0, seed=3, device=DEV)
        vec = [lc.operand(1, 2 * N, 2 * N, 0, seed=20 + i, device=DEV) for i in range(5)]
        bn = nv.BnBwdFused(x=bnx.ptr(), ld_x=bnx.ld, mean=vec[0].ptr(), invstd=vec[1].ptr(), scale=vec[2].ptr(), shift=vec[3].ptr(),
                           coef=vec[4].ptr(), relu=1)
        args = (p("Y"), ld("Y"), ctypes.byref(bn), p("X"), ld("X"))
        assert lib.esc_linear_bwd_both_bn_ok(*args, p("W"), ld("W"), M, N, K, p("dX"), ld("dX"), p("slabs"), None) == 0, edit
        rc = lib.esc_linear_bwd_both_bn(*args, None, None, p("W"), ld("W"), M, N, K, p("dX"), ld("dX"), 0, p("dW"), ld("dW"), p("db"),
                                        p("slabs"), None, None, s)
        assert rc == -1 and lib.esc_last_error(), edit
        torch.cuda.synchronize()
        assert all(ops.outputs[n].untouched() for n in ("dX", "dW", "db", "slabs")), edit


# ---- 6. the 128x160 tile (off unless ESC_TILE160=1 is in the environment when the library first dispatches) --------------------------------
TILE160_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
import esc_gnn_amd
import linear_cases as lc
import test_hip_dense_dispatch as t
nv = esc_gnn_amd._native
for M, N, K in ((129, 300, 64), (257, 600, 300)):
    fwd = lc.Case("tile160-fwd-%%dx%%dx%%d" %% (M, N, K), "fwd", M, N, K, "", False, True, 0, "dma128", True)
    ops = t._launch(nv, fwd)
    assert ops.block_rows == 128, ops.block_rows
    t._check(nv, ops)
    t._check(nv, t._launch(nv, fwd._replace(name=fwd.name + "-p", prologue=True)))
    # the gradients tile the K columns: K = 300 / 600 takes the 160-wide tile
    for flags in ("", "a", "p"):
        g = lc.Case("tile160-%%s-%%dx%%dx%%d" %% (flags, M, K, N), "bwd_input", M, K, N, "", "p" in flags, True, int("a" in flags), "", True)
        if flags != "p":
            t._check(nv, t._launch(nv, g))
        t._check(nv, t._launch(nv, g._replace(entry="bwd_both")))
print("tile160 ok")
"""


def test_tile160_in_a_child_process(nv):
    env = dict(os.environ, ESC_TILE160="1", ESC_TILE160_MIN_WGS="1")
    r = subprocess.run([sys.executable, "-c", TILE160_CHILD % (ROOT, os.path.join(ROOT, "tests"))], env=env, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "tile160 ok" in r.stdout, r.stdout[-3000:]
