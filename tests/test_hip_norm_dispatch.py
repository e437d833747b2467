"""The BatchNorm entry points (csrc/norm.hip, bn_fold_column / grid_last_block in common.h) on every dispatch branch, operand
layout, knob setting and data regime of tests/norm_cases.py.

Every operand is a view into a larger allocation whose padding columns and guard rows hold NaN (inputs) or a sentinel bit
pattern (outputs); the scratch is exactly esc_bn_scratch(C) floats of NaN followed by a sentinel guard as large again; the
dropout mask sits between sentinel bytes.  The reference is fp64 on the CPU from the live regions only, written out as the plain
formulas (norm_cases.ref_*), and every output is compared per column with the bounds DESIGN.md derives.  Each call is repeated
on fresh buffers and must give the same bits (three times where a ticket or barrier counter has to be re-zeroed), in-place
results must equal the out-of-place ones bit for bit, and every knob is restored afterwards.

A backward output that misses 1e-5 of max(1, |ref|) falls under the project's standing rule (three times the error of the same
formula in fp32 on the CPU); one case needs it, bwd-fused_last_block+rows-4096x1280-a1y-k8=1 (dbeta 1.87e-5 of scale against
1.30e-5 of the CPU formula, dgamma 1.15e-5 against 1.53e-5).  Each line printed is `case  output  error / bound`.
"""
import ctypes
import os

import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import linear_cases as lc
import norm_cases as nc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
KNOB_RESTORE = dict(nc.KNOB_DEFAULTS)
KNOB_RESTORE[13] = int(os.environ.get("ESC_BN_BWD_ONE", "0") or 0)
WORST = {}                                  # entry -> (ratio, case, output): printed by the last test of the module


@pytest.fixture(scope="module")
def nv():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd._native


@pytest.fixture
def knobs(nv):
    def set_(pairs):
        for k, v in pairs:
            nv.call("esc_tune_set", k, v)
    try:
        yield set_
    finally:
        for k, v in KNOB_RESTORE.items():
            nv.call("esc_tune_set", k, v)


_DATA = {}


def data_of(case):
    """the operands and fp64 references of a case: computed once, shared by every test and repeat, never modified"""
    key = (nc.seed_of(case), case.entry, case.M, case.C, case.act, case.has_Y, case.affine, case.running, case.fused, case.regime, case.extra)
    if key not in _DATA:
        if len(_DATA) > 8:
            _DATA.clear()
        _DATA[key] = nc.Data(case)
    return _DATA[key]


class Run(object):
    """the guarded device buffers of a case and the argument list of its one library call"""

    def __init__(self, case, data):
        self.case, self.data, self.lay = case, data, nc.layout_of(case)
        self.inputs, self.outputs, self.keep = {}, {}, []
        self.fn, self.args = getattr(self, "_" + case.entry)()

    # -- buffers
    def _mat(self, name, op):
        c, (ld, off) = self.case, self.lay[op]
        live = self.data.inputs[name].float() if c.M > 0 else torch.full((1, c.C), NAN)
        b = lc.Buf(max(c.M, 1), c.C, ld, off, live, NAN, 2 * ld + 64, 2 * ld + 64, DEV)
        self.inputs[name] = b
        return b

    def _vec(self, name, op=None, optional=False):
        if name not in self.data.inputs:
            assert optional, name
            return None
        live = self.data.inputs[name].float().reshape(1, -1)
        w = live.shape[1]
        b = lc.Buf(1, w, w, self.lay[op][1] if op else 0, live, NAN, 64, 64, DEV)
        self.inputs[name] = b
        return b

    def _rows(self, name):
        live = self.data.inputs[name].float()
        b = lc.Buf(live.shape[0], live.shape[1], live.shape[1], 0, live, NAN, 64, 64, DEV)
        self.inputs[name] = b
        return b

    def _out(self, name, width=None, wanted=True):
        if not wanted:
            return None
        w = width or self.case.C
        b = lc.output(1, w, w, 0, device=DEV)
        self.outputs[name] = b
        return b

    def _inout(self, name):
        """running statistics: live values in, sentinel around"""
        if not self.case.running:
            return None
        live = self.data.inputs[name].float().reshape(1, -1)
        b = lc.Buf(1, live.shape[1], live.shape[1], 0, live, lc.sentinel(), 64, 64, DEV)
        self.outputs[name] = b
        return b

    def _mat_out(self, name, op):
        c, (ld, off) = self.case, self.lay[op]
        b = lc.output(max(c.M, 1), c.C, ld, off, device=DEV)
        self.outputs[name] = b
        return b

    def _scratch(self):
        n = nc.scratch_floats(self.case.C)
        b = lc.Buf(1, n, n, self.lay["S"][1], torch.full((1, n), NAN), lc.sentinel(), 0, n + 64, DEV)
        self.outputs["scratch"] = b
        return b

    @staticmethod
    def _p(b):
        return None if b is None else b.ptr()

    # -- one builder per entry point: (function name, [(argument name, value), ...])
    def _stat_outputs(self):
        c = self.case
        return [("mean", self._p(self._out("mean"))), ("invstd", self._p(self._out("invstd"))), ("rm", self._p(self._inout("rm"))),
                ("rv", self._p(self._inout("rv"))), ("gamma", self._p(self._vec("gamma", "gamma", True))),
                ("beta", self._p(self._vec("beta", "gamma", True))), ("scale", self._p(self._out("scale", wanted=c.fused))),
                ("shift", self._p(self._out("shift", wanted=c.fused)))]

    def _stats(self):
        c = self.case
        return "esc_bn_stats", ([("X", self._mat("X", "X").ptr()), ("ld_x", self.lay["X"][0]), ("M", c.M), ("C", c.C), ("eps", nc.EPS),
                                 ("momentum", nc.MOMENTUM)] + self._stat_outputs() + [("S", self._scratch().ptr())])

    def _stats_partials(self):
        c = self.case
        return "esc_bn_stats_from_partials", ([("partials", self._rows("partials").ptr()), ("M", c.M), ("C", c.C), ("eps", nc.EPS),
                                               ("momentum", nc.MOMENTUM)] + self._stat_outputs())

    def _stats_partials_rows(self):
        c = self.case
        return "esc_bn_stats_from_partials_rows", ([("partials", self._rows("partials").ptr()), ("M", c.M), ("C", c.C), ("block_rows", c.extra),
                                                    ("eps", nc.EPS), ("momentum", nc.MOMENTUM)] + self._stat_outputs())

    def _affine_fold(self):
        c = self.case
        st = dict(self._stat_outputs())
        self.bn = self.nv_BnFold(partials=self._rows("partials").ptr(), rows=c.M, block_rows=c.extra, C=c.C, eps=nc.EPS, momentum=nc.MOMENTUM,
                                 gamma=st["gamma"], beta=st["beta"], mean=st["mean"], invstd=st["invstd"], scale=st["scale"], shift=st["shift"],
                                 running_mean=st["rm"], running_var=st["rv"])
        return "esc_affine_act_fold", [("X", self._mat("X", "X").ptr()), ("ld_x", self.lay["X"][0]), ("M", c.M), ("C", c.C),
                                       ("bn", ctypes.byref(self.bn)), ("relu", c.act), ("Y", self._mat_out("Y", "Y").ptr()),
                                       ("ld_y", self.lay["Y"][0])]

    def _apply(self):
        c = self.case
        return "esc_bn_apply", [("X", self._mat("X", "X").ptr()), ("ld_x", self.lay["X"][0]), ("M", c.M), ("C", c.C),
                                ("mean", self._vec("mean", "mean").ptr()), ("invstd", self._vec("invstd", "mean").ptr()),
                                ("gamma", self._p(self._vec("gamma", "gamma", True))), ("beta", self._p(self._vec("beta", "gamma", True))),
                                ("relu", c.act), ("Y", self._mat_out("Y", "Y").ptr()), ("ld_y", self.lay["Y"][0])]

    def _affine(self):
        c = self.case
        return "esc_affine_act", [("X", self._mat("X", "X").ptr()), ("ld_x", self.lay["X"][0]), ("M", c.M), ("C", c.C),
                                  ("scale", self._vec("scale", "P").ptr()), ("shift", self._vec("shift", "P").ptr()), ("relu", c.act),
                                  ("Y", self._mat_out("Y", "Y").ptr()), ("ld_y", self.lay["Y"][0])]

    def _eval_coef(self):
        c = self.case
        return "esc_bn_eval_coef", [("rm", self._vec("rm").ptr()), ("rv", self._vec("rv").ptr()), ("gamma", self._p(self._vec("gamma", "gamma", True))),
                                    ("beta", self._p(self._vec("beta", "gamma", True))), ("eps", nc.EPS), ("C", c.C),
                                    ("scale", self._out("scale").ptr()), ("shift", self._out("shift").ptr())]

    def _bwd_head(self):
        c = self.case
        y = self._mat("Y", "Y") if c.has_Y else None
        return [("X", self._mat("X", "X").ptr()), ("ld_x", self.lay["X"][0]), ("Y", self._p(y)), ("ld_y", self.lay["Y"][0] if y else 0),
                ("dY", self._mat("dY", "dY").ptr()), ("ld_dy", self.lay["dY"][0]), ("M", c.M), ("C", c.C),
                ("mean", self._vec("mean", "mean").ptr()), ("invstd", self._vec("invstd", "mean").ptr()),
                ("gamma", self._p(self._vec("gamma", "gamma", True))), ("beta", self._p(self._vec("beta", "gamma", True))), ("relu", c.act)]

    def _dx(self):
        if self.case.in_place:
            self.outputs["dX"] = self.inputs.pop("dY")
            return self.outputs["dX"]
        return self._mat_out("dX", "dX")

    def _bwd(self):
        g = self.case.extra != "nograd"
        head = self._bwd_head()
        return "esc_bn_bwd", head + [("dX", self._dx().ptr()), ("ld_dx", self.lay["dX"][0]), ("dgamma", self._p(self._out("dgamma", wanted=g))),
                                     ("dbeta", self._p(self._out("dbeta", wanted=g))), ("S", self._scratch().ptr())]

    def _bwd_sums(self):
        return "esc_bn_bwd_sums", self._bwd_head() + [("sums", self._out("sums", 2 * self.case.C).ptr()), ("dgamma", self._out("dgamma").ptr()),
                                                      ("dbeta", self._out("dbeta").ptr()), ("S", self._scratch().ptr())]

    def _bwd_coef(self):
        return "esc_bn_bwd_coef", self._bwd_head() + [("coef", self._out("coef", 2 * self.case.C).ptr()), ("dgamma", self._out("dgamma").ptr()),
                                                      ("dbeta", self._out("dbeta").ptr()), ("S", self._scratch().ptr())]

    def _bwd_apply(self):
        head = self._bwd_head()
        return "esc_bn_bwd_apply", head + [("coef", self._vec("coef", "S").ptr()), ("dX", self._dx().ptr()), ("ld_dx", self.lay["dX"][0])]

    def _coef_partials(self):
        c = self.case
        return "esc_bn_bwd_coef_from_partials", [("partial", self._rows("partial").ptr()), ("slots", c.extra), ("M", c.M), ("C", c.C),
                                                 ("coef", self._out("coef", 2 * c.C).ptr()), ("dgamma", self._out("dgamma").ptr()),
                                                 ("dbeta", self._out("dbeta").ptr())]

    def _bwd_dropout(self):
        c = self.case
        self.mask = lc.ByteBuf(self.data.inputs["mask"], 4 * c.C + 64, DEV)
        return "esc_bn_bwd_dropout", [("X", self._mat("X", "X").ptr()), ("ld_x", self.lay["X"][0]), ("dY", self._mat("dY", "dY").ptr()),
                                      ("ld_dy", self.lay["dY"][0]), ("M", c.M), ("C", c.C), ("mean", self._vec("mean", "mean").ptr()),
                                      ("invstd", self._vec("invstd", "mean").ptr()), ("gamma", self._p(self._vec("gamma", "gamma", True))),
                                      ("beta", self._p(self._vec("beta", "gamma", True))), ("relu", c.act), ("mask", self.mask.ptr()),
                                      ("p", c.extra[1]), ("mask_on_output", c.extra[0]), ("dX", self._dx().ptr()), ("ld_dx", self.lay["dX"][0]),
                                      ("dgamma", self._out("dgamma").ptr()), ("dbeta", self._out("dbeta").ptr()), ("S", self._scratch().ptr())]

    nv_BnFold = None

    def call(self, nv, **override):
        """make the call (arguments replaced by name through `override`); returns the library's status"""
        unknown = set(override) - {n for n, _ in self.args}
        assert not unknown, unknown
        rc = getattr(nv.lib(), self.fn)(*[override.get(n, v) for n, v in self.args], nv.stream())
        torch.cuda.synchronize()
        return rc

    def bits(self):
        return {n: b.result().view(torch.int32).clone() for n, b in self.outputs.items() if n != "scratch"}


def launch(nv, case, data=None):
    Run.nv_BnFold = nv.BnFold
    run = Run(case, data or data_of(case))
    nv.prof_enable("norm", True)
    try:
        nv.prof_reset("norm")
        rc = run.call(nv)
        run.launches = nv.prof_read("norm")[0]
    finally:
        nv.prof_enable("norm", False)
    assert rc == 0, "%s: %s failed (%d): %s" % (case.name, run.fn, rc, nv.lib().esc_last_error().decode())
    return run


def check(run):
    """fp64 parity per column, no NaN in a live region, sentinels and guards bit-identical, inputs untouched"""
    c, d, bad = run.case, run.data, []
    for name, want in d.ref.items():
        got = run.outputs[name].result().double()
        if c.M == 0 and want.dim() == 2:
            continue
        got = got.reshape(want.shape)
        if not bool(torch.isfinite(got).all()):
            bad.append("%s: %d non-finite values in the live region" % (name, int((~torch.isfinite(got)).sum())))
            continue
        err, bound = (got - want).abs(), d.bound[name]
        if want.dim() == 2 and bound.dim() == 1:
            err = nc.colmax(err)
        ratio = err / bound
        worst = passed = float(ratio.max()) if ratio.numel() else 0.0
        note = ""
        if worst > 1.0 and name in nc.FP32_ORACLE_RULE.get(c.name, ()):
            # the project's standing rule: as accurate as the same formula in fp32 on the CPU, three times over
            e32 = d.fp32_error()[name]
            e32 = nc.colmax(e32) if (e32.dim() == 2 and bound.dim() == 1) else e32
            passed = float((err / torch.maximum(bound, 3 * e32)).max())
            note = "  FALLBACK: the fp32 CPU formula is at %.3g of the bound, the kernel at %.3g of the allowance" % (float((e32 / bound).max()), passed)
        print("%s  %s  %.3g%s" % (c.name, name, worst, note))
        if worst > WORST.get(c.entry, (0.0,))[0]:
            WORST[c.entry] = (worst, c.name, name)
        if passed > 1.0:
            bad.append("%s: error %.3g of its bound (worst at flat index %d)%s" % (name, worst, int(ratio.reshape(-1).argmax()), note))
    const = nc.constant_columns(c.C, c.regime)
    if "mean" in d.ref and bool(const.any()) and "mean" in run.outputs:
        x0 = d.inputs["X"][0].float()
        if not torch.equal(run.outputs["mean"].result()[0][const], x0[const]):
            bad.append("mean of a constant column is not the constant")
    for name, b in run.outputs.items():
        n = b.outside_changed()
        if n:
            bad.append("%s: %d floats outside the live region were written" % (name, n))
    for name, b in run.inputs.items():
        if not b.untouched():
            bad.append("%s: an input was modified" % name)
    if hasattr(run, "mask") and not run.mask.untouched():
        bad.append("the mask or the bytes around it were modified")
    if c.M == 0:
        bad += ["%s: written although M = 0" % n for n, b in run.outputs.items() if not b.untouched()]
    assert not bad, "%s [%s]: %s" % (c.name, c.family, "; ".join(bad))


def same_bits(a, b):
    return [n for n, v in a.items() if not torch.equal(v, b[n])]


def run_case(nv, knobs, case):
    knobs(case.knobs)
    k = dict(case.knobs)
    first = launch(nv, case)
    # the anchor of the table: the library made the launches of the family the case is meant for (3: partial + finalize + apply,
    # 2: last-block or folded finalize, 1: one launch)
    assert first.launches == nc.launches_of(case), "%s is meant for %s (%d launches), the library made %d" % (
        case.name, case.family, nc.launches_of(case), first.launches)
    check(first)
    bits = first.bits()
    del first
    for _ in range(2 if (k.get(8) or k.get(13)) else 1):
        again = launch(nv, case)
        diff = same_bits(bits, again.bits())
        assert not diff, "%s: %s of a repeated identical call differ (promised fixed-order)" % (case.name, diff)
        assert again.outputs.get("scratch") is None or again.outputs["scratch"].outside_changed() == 0
        del again
    if case.in_place:
        apart = launch(nv, case._replace(in_place=False))
        assert torch.equal(apart.outputs["dX"].result().view(torch.int32), bits["dX"]), "%s: in-place dX differs from out-of-place" % case.name
        assert not same_bits({n: v for n, v in bits.items() if n != "dX"}, apart.bits())


def _ids(cases):
    return [c.name for c in cases]


def _param(*entries, **kw):
    cs = [c for e in entries for c in nc.cases(e, **kw)]
    return pytest.mark.parametrize("case", cs, ids=_ids(cs))


def test_scratch_promise(nv):
    for C in (1, 4, 300, 1280):
        assert int(nv.lib().esc_bn_scratch(C)) == nc.scratch_floats(C)


@_param("stats")
def test_statistics(nv, knobs, case):
    run_case(nv, knobs, case)


@_param("stats_partials", "stats_partials_rows")
def test_statistics_from_partials(nv, knobs, case):
    run_case(nv, knobs, case)


@_param("affine_fold")
def test_affine_act_fold(nv, knobs, case):
    run_case(nv, knobs, case)


@_param("apply", "affine", "eval_coef")
def test_forward_elementwise(nv, knobs, case):
    run_case(nv, knobs, case)


@_param("bwd")
def test_backward(nv, knobs, case):
    run_case(nv, knobs, case)


@_param("bwd_sums", "bwd_coef", "bwd_apply", "coef_partials")
def test_backward_halves(nv, knobs, case):
    run_case(nv, knobs, case)


@_param("bwd_dropout")
def test_backward_dropout(nv, knobs, case):
    run_case(nv, knobs, case)


@_param("bwd", node=True)
def test_backward_one_launch(nv, knobs, case):
    """knob 13: at most 256 x 2 small workgroups, far inside residency; the spin is bounded in the kernel"""
    run_case(nv, knobs, case)


def test_split_backward_equals_whole(nv, knobs):
    """esc_bn_bwd_coef + esc_bn_bwd_apply are esc_bn_bwd's steps: the same bits"""
    for name in ("bwd-v4+rows-131x12-a1y-mixed", "bwd-scalar+flat1-131x10-a2-mixed"):
        case = nc.BY_NAME[name]
        whole = launch(nv, case)
        d = data_of(case)
        half = launch(nv, case._replace(entry="bwd_coef", name=case.name), nc.Data(case._replace(entry="bwd_coef", name=case.name)))
        coef = half.outputs["coef"].result().double().view(case.C, 2)
        d2 = nc.Data(case._replace(entry="bwd_apply", name=case.name))
        d2.inputs["coef"] = coef
        d2.ref["dX"] = nc.ref_backward(d.inputs["X"], d.inputs["dY"], d.inputs["mean"], d.inputs["invstd"], d.inputs["gamma"], d.inputs["beta"],
                                       case.act, coef=coef)["dX"]
        ap = launch(nv, case._replace(entry="bwd_apply", name=case.name), d2)
        check(ap)
        assert torch.equal(ap.outputs["dX"].result().view(torch.int32), whole.outputs["dX"].result().view(torch.int32)), name
        for n in ("dgamma", "dbeta"):
            assert torch.equal(half.outputs[n].result().view(torch.int32), whole.outputs[n].result().view(torch.int32)), (name, n)


# ---- the SyncBN trio in one process ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,C,n_local", nc.SYNC_CASES, ids=[s[0] for s in nc.SYNC_CASES])
def test_syncbn_single_process(nv, name, C, n_local):
    world, N = len(n_local), sum(n_local)
    x = nc.sync_rows(C, n_local, 7 + C)
    gamma, beta = nc.gamma_beta(C)
    vec = lambda t, outside=NAN: lc.Buf(1, t.numel(), t.numel(), 0, t.float().reshape(1, -1), outside, 64, 64, DEV)
    packed, at = [], 0
    for r, n in enumerate(n_local):
        mean, _, invstd, _ = nc.ref_stats(x[at:at + n])
        at += n
        m, s = vec(mean), vec(invstd)
        buf = lc.Buf(1, world * 3 * C, world * 3 * C, 0, torch.zeros(1, world * 3 * C), lc.sentinel(), 64, 64, DEV)
        nv.call("esc_bn_sync_pack", m.ptr(), s.ptr(), n, nc.EPS, C, r, world, buf.ptr(), nv.stream())
        torch.cuda.synchronize()
        assert buf.outside_changed() == 0 and m.untouched() and s.untouched(), (name, r)
        got = buf.result().view(world, 3, C)
        assert float(got[torch.arange(world) != r].abs().max() if world > 1 else 0.0) == 0.0, "rank %d wrote into another rank's slot" % r
        assert torch.equal(got[r, 0], torch.full((C,), float(n))) and torch.equal(got[r, 1], mean.float())
        packed.append(buf)
    total = packed[0].view().clone()
    for b in packed[1:]:
        total = total + b.view()                             # the all-reduce
    summed = vec(total)
    rm0, rv0 = nc.uniform((C,), 3, 2.0), nc.uniform((C,), 4, 0.5) + 1.0
    out = {n: lc.output(1, C, C, 0, device=DEV) for n in ("mean", "invstd", "scale", "shift")}
    out["rm"], out["rv"] = vec(rm0, lc.sentinel()), vec(rv0, lc.sentinel())
    out["n"] = lc.output(1, 1, 1, 0, device=DEV)
    g, b = vec(gamma), vec(beta)
    nv.call("esc_bn_sync_finalize", summed.ptr(), world, C, nc.EPS, nc.MOMENTUM, out["mean"].ptr(), out["invstd"].ptr(), out["rm"].ptr(),
            out["rv"].ptr(), g.ptr(), b.ptr(), out["scale"].ptr(), out["shift"].ptr(), out["n"].ptr(), nv.stream())
    torch.cuda.synchronize()
    mean, var, invstd, unbiased = nc.ref_stats(x)
    rm, rv = nc.ref_running(rm0, rv0, mean, unbiased)
    ref = {"mean": mean, "invstd": invstd, "scale": gamma * invstd, "shift": beta - mean * gamma * invstd, "rm": rm, "rv": rv}
    bound = {"mean": nc.bound_mean(mean), "invstd": nc.bound_invstd(mean, invstd), "scale": nc.bound_scale(mean, invstd, gamma),
             "shift": nc.bound_shift(mean, invstd, gamma, beta), "rm": nc.bound_running_mean(rm, rm0, mean),
             "rv": nc.bound_running_var(rv, mean, invstd, unbiased)}
    bad = []
    for n, want in ref.items():
        got = out[n].result()[0].double()
        ratio = (got - want).abs() / bound[n]
        worst = float(ratio.max()) if bool(torch.isfinite(got).all()) else float("inf")
        print("%s  %s  %.3g   (constant column %.3g, variance-1e-8 column %.3g)" % (name, n, worst, float(ratio[0]), float(ratio[1])))
        if worst > WORST.get("sync", (0.0,))[0]:
            WORST["sync"] = (worst, name, n)
        if not worst <= 1.0:
            bad.append("%s: error %.3g of its bound at column %d" % (n, worst, int(ratio.argmax())))
    assert float(out["n"].result()[0, 0]) == float(N)
    assert float(out["mean"].result()[0, 0]) == 0.75, "mean of the constant column"
    bad += ["%s: written outside" % n for n, o in out.items() if o.outside_changed()]
    assert summed.untouched() and g.untouched() and b.untouched()
    # the backward's coefficient: all-reduced sums / global row count
    sums = nc.uniform((C, 2), 9, 50.0)
    coef = lc.Buf(1, 2 * C, 2 * C, 0, sums.float().reshape(1, -1), lc.sentinel(), 64, 64, DEV)
    nv.call("esc_bn_sync_coef", coef.ptr(), C, out["n"].ptr(), nv.stream())
    torch.cuda.synchronize()
    err = (coef.result()[0].double().view(C, 2) - sums / N).abs() / (4 * nc.U * (sums / N).abs() + 1e-30)
    print("%s  coef  %.3g" % (name, float(err.max())))
    if float(err.max()) > 1.0 or coef.outside_changed():
        bad.append("coef: %.3g of 4 ulp" % float(err.max()))
    assert not bad, "%s: %s" % (name, "; ".join(bad))


# ---- the argument checks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,what", nc.REFUSALS, ids=["%s-%s" % r for r in nc.REFUSALS])
def test_refusals_leave_the_outputs_alone(nv, entry, what):
    """every ESC_REQUIRE of the family answers ESC_EINVAL with a message before any launch: sentinels AND live NaNs intact"""
    Run.nv_BnFold = nv.BnFold
    case = nc.BY_NAME[nc.REFUSAL_BASE[entry]]
    case = case._replace(fused=True) if what == "scale_without_shift" and entry != "affine_fold" else case
    if what == "scale_without_shift" and entry == "affine_fold":
        case = case._replace(fused=True, running=True)
    if what == "C%4":
        case = case._replace(C=10, layout="X+2,dY+2,dX+2,Y+2")
    elif what == "ld%4":
        case = case._replace(layout="X+1")
    elif what == "base@1":
        case = case._replace(layout="X@1")
    run = Run(case, nc.Data(case))
    over = {}
    if what.startswith("M="):
        over["M"] = int(what[2:])
    elif what == "ld<C":
        over["ld_x"] = case.C - 1
    elif what.startswith("null:"):
        over[what[5:]] = None
    elif what.startswith("relu="):
        over["relu"] = int(what[5:])
    elif what.startswith("p="):
        over["p"] = float(what[2:])
    elif what in ("block_rows=0", "slots=0", "C=0"):
        over[what.split("=")[0]] = 0
    elif what == "scale_without_shift":
        if entry == "affine_fold":
            run.bn.shift = None
        else:
            over["shift"] = None
    if entry == "affine_fold":
        if what == "M=1":
            run.bn.rows = 1
        if what == "null:partials":
            run.bn.partials, over = None, {}
    rc = run.call(nv, **over)
    assert rc == -1 and nv.lib().esc_last_error(), "%s %s: accepted (status %d)" % (entry, what, rc)
    for n, b in run.outputs.items():
        assert b.untouched(), "%s %s: %s was written by a refused call" % (entry, what, n)
    # ... and the same call without the fault is accepted
    if what not in ("C%4", "ld%4", "base@1"):
        ok = Run(case, run.data)
        assert ok.call(nv) == 0, nv.lib().esc_last_error()


SYNC_FN = {"pack": "esc_bn_sync_pack", "finalize": "esc_bn_sync_finalize", "coef": "esc_bn_sync_coef"}


@pytest.mark.parametrize("entry,what", nc.SYNC_REFUSALS, ids=["sync_%s-%s" % r for r in nc.SYNC_REFUSALS])
def test_syncbn_refusals_leave_the_outputs_alone(nv, entry, what):
    """the ESC_REQUIREs of the SyncBN trio: ESC_EINVAL with a message before any launch, every buffer as it was"""
    C, world, n = 12, 3, 37
    vec = lambda t, outside=NAN: lc.Buf(1, t.numel(), t.numel(), 0, t.float().reshape(1, -1), outside, 64, 64, DEV)
    ins = {k: vec(nc.uniform((C,), i, 1.0).abs() + 0.5) for i, k in enumerate(("m_in", "is_in", "gamma", "beta"))}
    ins["summed"] = vec(torch.cat([torch.full((C,), float(n)), nc.uniform((C,), 7), nc.uniform((C,), 8).abs()] * world))
    ins["n_total"] = vec(torch.tensor([float(n * world)]))
    outs = {k: lc.output(1, C, C, 0, device=DEV) for k in ("mean", "invstd", "scale", "shift", "rm", "rv")}
    outs["packed"] = lc.output(1, world * 3 * C, world * 3 * C, 0, device=DEV)
    outs["n_out"] = lc.output(1, 1, 1, 0, device=DEV)
    outs["coef"] = vec(nc.uniform((2 * C,), 9), lc.sentinel())
    p = lambda k: (ins.get(k) or outs[k]).ptr()
    args = {"pack": [("mean", p("m_in")), ("invstd", p("is_in")), ("n_local", n), ("eps", nc.EPS), ("C", C), ("rank", 1), ("world", world),
                     ("buf", p("packed"))],
            "finalize": [("buf", p("summed")), ("world", world), ("C", C), ("eps", nc.EPS), ("momentum", nc.MOMENTUM), ("mean", p("mean")),
                         ("invstd", p("invstd")), ("rm", p("rm")), ("rv", p("rv")), ("gamma", p("gamma")), ("beta", p("beta")),
                         ("scale", p("scale")), ("shift", p("shift")), ("n_total", p("n_out"))],
            "coef": [("coef", p("coef")), ("C", C), ("n_total", p("n_total"))]}[entry]
    over = {"rank=world": {"rank": world}, "scale_without_shift": {"shift": None}, "shift_without_scale": {"scale": None}}.get(what)
    if over is None:
        over = {what[5:]: None} if what.startswith("null:") else {what.split("=")[0]: int(what.split("=")[1])}
    assert set(over) <= {k for k, _ in args}, over
    rc = getattr(nv.lib(), SYNC_FN[entry])(*[over.get(k, v) for k, v in args], nv.stream())
    torch.cuda.synchronize()
    assert rc == -1 and nv.lib().esc_last_error(), "%s %s: accepted (status %d)" % (entry, what, rc)
    for k, b in list(ins.items()) + list(outs.items()):
        assert b.untouched(), "%s %s: %s was written by a refused call" % (entry, what, k)


def test_default_knobs_and_worst_ratios(nv, knobs):
    """runs last.  The library has no getter for knobs 8 / 9 / 12 / 13, so their state is read from what a call does: with the
    defaults (runtime.hip: 0, 256, 0, and ESC_BN_BWD_ONE or 0) esc_bn_bwd at 131 rows makes three launches (knob 8 or 12: two,
    knob 13: one) and at 8200 rows writes 256 partial slots (knob 9 caps them).  Every test above sets knobs only through the
    `knobs` fixture, whose `finally` puts these defaults back; tests/test_hip_ops.py run behind this module in one process is the
    end-to-end confirmation.  Then the worst error / bound per entry point is printed (DESIGN.md quotes them)."""
    small = launch(nv, nc.BY_NAME["bwd-v4+rows-131x12-a1y"])
    assert small.launches == (1 if KNOB_RESTORE[13] else 3), "knob 8, 12 or 13 was left changed (%d launches)" % small.launches
    tall = launch(nv, nc.BY_NAME["bwd-v4+rows-8200x8-a1y-k9=512-mixed"]._replace(knobs=()))
    C = tall.case.C
    slots = tall.outputs["scratch"].result()[0, :nc.NORM_ROWBLOCKS * 4 * C * 2].view(-1, 2 * C)
    written = int((~torch.isnan(slots)).all(1).sum())
    assert written == nc.KNOB_DEFAULTS[9] and int((~torch.isnan(slots)).any(1).sum()) == written, "knob 9 was left changed (%d slots)" % written
    for entry, (ratio, name, out) in sorted(WORST.items()):
        print("WORST %-20s %.3g  %s %s" % (entry, ratio, name, out))
