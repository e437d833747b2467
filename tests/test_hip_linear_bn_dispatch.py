"""esc_linear_bwd_both_bn (csrc/linear_mfma.hip; linear_small.h and the 64x64 / 128x128 tiles of gemm_dma.h) on every record of
tests/bnb_cases.py, through the C ABI.

Every operand is a view into a larger allocation whose padding columns, guard rows and vector surroundings hold NaN (inputs) or a
sentinel bit pattern (outputs); `slabs` is exactly esc_linear_bwd_weight_scratch floats, `next.partial` exactly the promised slots,
each followed by a guard.  The reference is fp64 on the CPU from the entry's own fp32 inputs; dX, dW and the `next` sums (summed, and
slot by slot) hold 1e-5 of max(1, max |reference|), db the depth bound of bnb_cases.Data.  The table is anchored to the library
through esc_linear_bwd_both_bn_ok, esc_linear_bwd_bn_block_rows and the launch count of esc_prof_read.  Refused records answer 0,
return -1 and leave every output as it was."""
import ctypes

import pytest
import torch

from conftest import require_gpu
import bnb_cases as bc
import linear_cases as lc
import norm_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB_TWO_LAUNCHES = 14
WORST = {}                                  # (family, output) -> (error / bound, case): printed when the module is done


@pytest.fixture(scope="module")
def nv():
    require_gpu()
    import esc_gnn_amd
    yield esc_gnn_amd._native
    for (fam, out), (e, name) in sorted(WORST.items()):
        print("worst %-10s %-8s %.3g of its bound (%s)" % (fam, out, e, name))


def _structs(nv, case, ops):
    lay, p = ops.lay, ops.ptr
    bn = nxt = None
    if case.bn:
        bn = nv.BnBwdFused(x=p("bx"), ld_x=lay["bx"][0], mean=p("mean"), invstd=p("invstd"), scale=p("scale"), shift=p("shift"), coef=p("coef"),
                           relu=case.bn_act, beta=p("beta"))
    if case.next:
        nxt = nv.BnBwdNext(partial=p("npartial"), x=p("nx"), ld_x=lay["nx"][0], mean=p("nmean"), invstd=p("ninvstd"), scale=p("nscale"),
                           shift=p("nshift"), relu=case.next_act, beta=p("nbeta"))
    return bn, nxt


class Run(object):
    """the guarded operands of a case on the GPU and the one library call: .ok (the predicate), .rc, .launches"""

    def __init__(self, nv, case, job=None, slabs_ptr=None):
        lib, lay = nv.lib(), bc.layout_of(case)
        M, N, K = case.M, case.N, case.K
        self.case, self.data = case, bc.data_of(case)
        promised = int(lib.esc_linear_bwd_weight_scratch(M, N, K))
        assert promised == bc.scratch_promised(case), (case.name, promised)
        self.slot_rows = int(lib.esc_linear_bwd_bn_block_rows(M, N, K))
        # guard for the finest partition any kernel writes, should the library's slot height be wrong: the buffer holds what it promises
        self.ops = ops = bc.Operands(case, self.data, DEV, promised, lc.cdiv(M, self.slot_rows))
        p = ops.ptr
        self.bn, self.nxt = _structs(nv, case, ops)
        ref = lambda s: None if s is None else ctypes.byref(s)
        slabs = p("slabs") if slabs_ptr is None else slabs_ptr
        self.ok = int(lib.esc_linear_bwd_both_bn_ok(p("dOut"), lay["dOut"][0], ref(self.bn), p("X"), lay["X"][0], p("W"), lay["W"][0], M, N, K,
                                                    p("dX"), lay["dX"][0], slabs, ref(self.nxt)))
        nv.prof_enable("linear", True)
        try:
            nv.prof_reset("linear")
            self.rc = int(lib.esc_linear_bwd_both_bn(p("dOut"), lay["dOut"][0], ref(self.bn), p("X"), lay["X"][0], p("in_scale"), p("in_shift"),
                                                     p("W"), lay["W"][0], M, N, K, p("dX"), lay["dX"][0], case.acc, p("dW"), lay["dW"][0],
                                                     p("db"), slabs, None if job is None else ctypes.addressof(job), ref(self.nxt), nv.stream()))
            torch.cuda.synchronize()
            self.launches = nv.prof_read("linear")[0]
        finally:
            nv.prof_enable("linear", False)
        self.error = lib.esc_last_error().decode() if self.rc else ""

    def bits(self, names=("dX", "dW", "db", "npartial")):
        return {n: self.ops.outputs[n].result().view(torch.int32).clone() for n in names if n in self.ops.outputs}


def check(run, record=True):
    """every output inside its bound, no NaN left in a live region or a promised slot, sentinels bit-identical, inputs untouched"""
    c, d, ops, bad = run.case, run.data, run.ops, []
    got = ops.results()
    for n, t in got.items():
        if bool(torch.isnan(t).any()):
            bad.append("%s: %d NaN left" % (n, int(torch.isnan(t).sum())))
    for n, e in d.excess(got).items():
        print("%s %s: %.3g of its bound" % (c.name, n, e))
        if record:
            WORST[(c.family, n)] = max(WORST.get((c.family, n), (0.0, "")), (e, c.name))
        if not e <= 1.0:
            rule = n in bc.FP32_ORACLE_RULE.get(c.name, ())
            if rule:                                        # at most 3x the error of the same formulas in fp32 on the CPU
                oracle = d.excess(d.replay_fp32("centred"))[n]
                rule = e <= 3 * oracle
            if not rule:
                bad.append("%s: %.3g of its bound" % (n, e))
    for n, b in ops.outputs.items():                         # (slabs and npartial: nothing behind the promised floats)
        if b.outside_changed():
            bad.append("%s: %d floats outside the live region were written" % (n, b.outside_changed()))
    for n, b in ops.inputs.items():
        if not b.untouched():
            bad.append("%s: an input was modified" % n)
    assert not bad, "%s [%s]: %s" % (c.name, c.family, "; ".join(bad))


def _ids(cases):
    return [c.name for c in cases]


# ---- 1. every served record ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.served(), ids=_ids(bc.served()))
def test_served(nv, case):
    run = Run(nv, case)
    # the anchors of the table: served, the slot height of the family, the launches of the family
    assert run.ok == 1 and run.rc == 0, "%s is meant for %s, the library refuses it: %s" % (case.name, case.family, run.error)
    assert run.slot_rows == bc.block_rows(case), (case.name, run.slot_rows)
    assert run.launches == bc.launches_of(case), "%s is meant for %s (%d launches), the library made %d" % (
        case.name, case.family, bc.launches_of(case), run.launches)
    check(run)
    first = run.bits()
    del run
    again = Run(nv, case).bits()
    diff = [n for n in first if not torch.equal(first[n], again[n])]
    assert not diff, "%s: %s of a second identical call on fresh buffers differ" % (case.name, diff)


# ---- 2. every refused record ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.refused(), ids=_ids(bc.refused()))
def test_refused(nv, case):
    run = Run(nv, case)
    assert run.ok == 0, "%s: the predicate serves what the plan refuses" % case.name
    assert run.rc == -1 and run.error, (case.name, run.rc)
    assert run.launches == 0, (case.name, run.launches)
    touched = [n for n, b in run.ops.outputs.items() if not b.untouched()]
    assert not touched, "%s: refused, but %s changed" % (case.name, touched)


# ---- 3. chained: statistics and coef from the library, the `next` partials through esc_bn_bwd_coef_from_partials -----------------------
def _dev(t):
    return t.float().to(DEV).contiguous()


def _bn_stats(nv, x, gamma, beta, scratch):
    M, C = x.shape
    out = [torch.empty(C, device=DEV) for _ in range(4)]                  # mean, invstd, scale, shift
    nv.call("esc_bn_stats", nv.ptr(x), C, M, C, nc.EPS, nc.MOMENTUM, nv.ptr(out[0]), nv.ptr(out[1]), None, None, nv.ptr(gamma), nv.ptr(beta),
            nv.ptr(out[2]), nv.ptr(out[3]), nv.ptr(scratch), nv.stream())
    return out


def _within(got, want, what, bad, scale=None):
    want = want.double()
    got = got.detach().cpu().double().view(want.shape)
    e = float((got - want).abs().max()) / (1e-5 * max(1.0, float(want.abs().max()) if scale is None else scale))
    print("chained %s: %.3g of its bound" % (what, e))
    if not e <= 1.0:
        bad.append("%s: %.3g of its bound" % (what, e))


@pytest.mark.parametrize("name", bc.CHAINED)
def test_chained_with_the_librarys_own_statistics(nv, name):
    """what the step engines do: esc_bn_stats -> esc_bn_bwd_coef -> the fused call -> esc_bn_bwd_coef_from_partials.  The fused call and
    the unfused sequence (esc_bn_bwd_apply, esc_linear_bwd_both) are held to the SAME fp64 reference and bars — the reference takes the
    library's fp32 mean / invstd / scale as given and everything behind them in fp64; the two are not compared with each other."""
    case, lib = bc.BY_NAME[name], nv.lib()
    M, N, K, i = case.M, case.N, case.K, bc.data_of(case).inputs
    cpu = lambda t: t.detach().cpu().double()
    dOut, X, W, bx, gamma, beta = (_dev(i[n]) for n in ("dOut", "X", "W", "bx", "gamma", "beta"))
    scratch = torch.empty(int(lib.esc_bn_scratch(max(N, K))), device=DEV)
    mean, invstd, scale, shift = _bn_stats(nv, bx, gamma, beta, scratch)
    coef, dg, dbeta = torch.empty(N, 2, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    nv.call("esc_bn_bwd_coef", nv.ptr(bx), N, None, 0, nv.ptr(dOut), N, M, N, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta), case.bn_act,
            nv.ptr(coef), nv.ptr(dg), nv.ptr(dbeta), nv.ptr(scratch), nv.stream())
    isc, ish = (_dev(i["in_scale"]), _dev(i["in_shift"])) if case.pro else (None, None)
    dx0 = _dev(i["dX0"]) if case.acc else None
    # fp64 from the library's statistics
    xh = (i["bx"] - cpu(mean)) * cpu(invstd)
    g = i["dOut"] * nc.act_grad(i["gamma"] * xh + i["beta"], case.bn_act)
    k1, k2 = g.sum(0) / M, (g * xh).sum(0) / M
    dy = cpu(scale) * (g - k1 - xh * k2)
    act_x = torch.clamp(i["X"] * i["in_scale"] + i["in_shift"], min=0) if case.pro else i["X"]
    want = {"dX": dy @ i["W"] + (i["dX0"] if case.acc else 0.0), "dW": dy.t() @ act_x, "coef": torch.stack((k1, k2), 1), "dgamma": k2 * M, "dbeta": k1 * M}
    bad = []
    for n, t in (("coef", coef), ("dgamma", dg), ("dbeta", dbeta)):
        _within(t, want[n], "%s %s" % (name, n), bad)
    f = nv.BnBwdFused(x=bx.data_ptr(), ld_x=N, mean=mean.data_ptr(), invstd=invstd.data_ptr(), scale=scale.data_ptr(), shift=shift.data_ptr(),
                      coef=coef.data_ptr(), relu=case.bn_act, beta=beta.data_ptr())
    nxt = None
    if case.next:
        nx, g2, b2 = _dev(i["nx"]), _dev(i["ngamma"]), _dev(i["nbeta"])
        st2 = _bn_stats(nv, nx, g2, b2, scratch)
        slots = lc.cdiv(M, int(lib.esc_linear_bwd_bn_block_rows(M, N, K)))
        partial = torch.full((slots, K, 2), float("nan"), device=DEV)
        nxt = nv.BnBwdNext(partial=partial.data_ptr(), x=nx.data_ptr(), ld_x=K, mean=st2[0].data_ptr(), invstd=st2[1].data_ptr(), scale=st2[2].data_ptr(),
                           shift=st2[3].data_ptr(), relu=case.next_act, beta=b2.data_ptr())
    slab_n = int(lib.esc_linear_bwd_weight_scratch(M, N, K))
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)
    dX, dW, db, slabs = (dx0.clone() if case.acc else new(M, K)), new(N, K), new(N), new(slab_n)
    nv.call("esc_linear_bwd_both_bn", nv.ptr(dOut), N, ctypes.byref(f), nv.ptr(X), K, nv.ptr(isc), nv.ptr(ish), nv.ptr(W), K, M, N, K,
            nv.ptr(dX) if case.dx else None, K, case.acc, nv.ptr(dW), K, nv.ptr(db), nv.ptr(slabs), None, ctypes.byref(nxt) if nxt is not None else None,
            nv.stream())
    # the unfused sequence of the same layer
    dY = new(M, N)
    nv.call("esc_bn_bwd_apply", nv.ptr(bx), N, None, 0, nv.ptr(dOut), N, M, N, nv.ptr(mean), nv.ptr(invstd), nv.ptr(gamma), nv.ptr(beta), case.bn_act,
            nv.ptr(coef), nv.ptr(dY), N, nv.stream())
    uX, uW, ub, slabs2 = (dx0.clone() if case.acc else new(M, K)), new(N, K), new(N), new(slab_n)
    nv.call("esc_linear_bwd_both", nv.ptr(dY), N, nv.ptr(X), K, nv.ptr(isc), nv.ptr(ish), nv.ptr(W), K, M, N, K, nv.ptr(uX) if case.dx else None, K,
            case.acc, nv.ptr(uW), K, nv.ptr(ub), nv.ptr(slabs2), nv.stream())
    torch.cuda.synchronize()
    for tag, x_, w_ in (("fused", dX, dW), ("unfused", uX, uW)):
        if case.dx:
            _within(x_, want["dX"], "%s %s dX" % (name, tag), bad)
        _within(w_, want["dW"], "%s %s dW" % (name, tag), bad)
    if case.next:
        assert not bool(torch.isnan(partial).any()), name
        c2, dg2, db2 = torch.empty(K, 2, device=DEV), torch.empty(K, device=DEV), torch.empty(K, device=DEV)
        nv.call("esc_bn_bwd_coef_from_partials", nv.ptr(partial), slots, M, K, nv.ptr(c2), nv.ptr(dg2), nv.ptr(db2), nv.stream())
        torch.cuda.synchronize()
        xh2 = (i["nx"] - cpu(st2[0])) * cpu(st2[1])
        gg = want["dX"] * nc.act_grad(i["ngamma"] * xh2 + i["nbeta"], case.next_act)
        s1, s2 = gg.sum(0), (gg * xh2).sum(0)
        # dgamma and dbeta ARE the summed partials: one bar over the pair, as for the sums of the table (without an activation on
        # either side dbeta is a column sum of a BatchNorm backward times W, about zero: a bar relative to itself means nothing)
        both = float(torch.stack((s1, s2)).abs().max())
        for n, t, w, sc in (("coef", c2, torch.stack((s1, s2), 1) / M, None), ("dgamma", dg2, s2, both), ("dbeta", db2, s1, both)):
            _within(t, w, "%s next %s" % (name, n), bad, sc)
    assert not bad, "%s: %s" % (name, "; ".join(bad))


# ---- 4. the deferred slab reduce and the two-launch form: the same bits ------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.DEFERRED)
def test_deferred_reduce_equals_the_immediate_call_bitwise(nv, name):
    case = bc.BY_NAME[name]
    now = Run(nv, case)
    job = nv.struct("esc_reduce_job")()
    later = Run(nv, case, job=job)
    assert later.rc == 0 and later.launches == bc.launches_of(case, deferred=True), (name, later.rc, later.launches)
    assert job.n == case.N * case.K and job.cols == case.K and job.rows == case.N and job.splits == bc.splits_of(case)[0], name
    assert bool(torch.isnan(later.ops.outputs["dW"].result()).all()), "%s: dW written before the reduce" % name
    nv.call("esc_slab_reduce_jobs", ctypes.addressof(job), 1, nv.stream())
    torch.cuda.synchronize()
    check(later, record=False)
    a, b = now.bits(), later.bits()
    diff = [n for n in a if not torch.equal(a[n], b[n])]
    assert not diff, "%s: deferred and immediate forms differ in %s" % (name, diff)


@pytest.mark.parametrize("name", bc.TWO_LAUNCHES)
def test_two_launches_equal_the_one_launch_bitwise(nv, name):
    case = bc.BY_NAME[name]
    one = Run(nv, case)
    try:
        nv.call("esc_tune_set", KNOB_TWO_LAUNCHES, 1)
        two = Run(nv, case)
    finally:
        nv.call("esc_tune_set", KNOB_TWO_LAUNCHES, 0)
    assert two.rc == 0 and two.launches == bc.launches_of(case, two_launches=True), (name, two.rc, two.launches)
    check(two, record=False)
    a, b = one.bits(), two.bits()
    diff = [n for n in a if not torch.equal(a[n], b[n])]
    assert not diff, "%s: two launches and one differ in %s" % (name, diff)
