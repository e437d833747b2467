"""The case table of esc_linear_bwd_both_bn, the Linear backward with the BatchNorm backward folded in: one record per (shape,
operand layout, argument combination, activation codes, data regime) chosen so that every branch of plan::plan_both_bn
(csrc/linear_plan.h) and of the three kernel families behind it (linear_small.h, the 64x64 and 128x128 tiles of gemm_dma.h) is
reached by name.  No GPU is needed to import or check this module (tests/test_bnb_cases_cpu.py);
tests/test_hip_linear_bn_dispatch.py runs the table against the library.  The guarded buffers are those of tests/linear_cases.py,
the data regimes those of tests/norm_cases.py.

A case is Case(name, M, N, K, layout, bn, next, bn_act, next_act, pro, acc, dx, regime, nregime, beta, family):
  layout    comma-separated edits of the plain layout (16-byte aligned base, ld == width):
              "X+4"  operand X has ld = width + 4        "X@4"  its base lies 4 floats into the allocation
              "X+1"  ld = width + 1 (demoting)           "X@1"  base 4 bytes past a 16-byte boundary (matrices: ld rounded up to 4)
            matrices: dOut [M,N], bx (bn.x) [M,N], X [M,K], W [N,K], dX [M,K], nx (next.x) [M,K], dW [N,K]
            vectors:  mean invstd scale shift coef beta (bn), npartial nmean ninvstd nscale nshift nbeta (next), slabs, P (in_scale / in_shift)
  bn, next  the structure is given                       bn_act, next_act   0 none, 1 ReLU, 2 ELU behind that BatchNorm
  pro       act(X) = relu(X * in_scale + in_shift)       acc   dX += ...          dx   False passes dX == NULL
  regime    data regime of bn.x, nregime of next.x (norm_cases.regime_x: plain | offset | tiny | constant | outlier | mixed)
  beta      (bn.beta given, next.beta given)             family   the kernel family the case is MEANT to reach ("none": refused)

family_of(), block_rows(), splits_of() transcribe plan_both_bn; tests/test_bnb_cases_cpu.py compiles linear_plan.h into
tests/bnb_plan_host.cpp and compares.  The fp64 reference takes the entry's fp32 inputs (mean, invstd, scale, shift, coef, beta)
as given; the bounds are derived in DESIGN.md ("Dispatch coverage of the fused BatchNorm backward"), never measured.
"""
import collections
import functools

import torch

import linear_cases as lc
import norm_cases as nc
from linear_cases import cdiv

Case = collections.namedtuple("Case", "name M N K layout bn next bn_act next_act pro acc dx regime nregime beta family")

SMALL_MAX, SMALLN_DX_MAX_N, ROWS_WGRAD, BNB_MAX_N, EDGE_ROWS, PRO_MAX_K = 16, 848, 32, 640, 8192, 1280      # csrc/linear_plan.h
U = nc.U
MATRICES = ("dOut", "bx", "X", "W", "dX", "nx", "dW")
BN_VECTORS = ("mean", "invstd", "scale", "shift", "coef", "beta")
NEXT_VECTORS = ("npartial", "nmean", "ninvstd", "nscale", "nshift", "nbeta")
VECTORS = BN_VECTORS + NEXT_VECTORS + ("slabs", "P")
FAMILIES = ("small_bn", "dma64_bn", "dma128_bn")


def shape_of(case, op):
    M, N, K = case.M, case.N, case.K
    return {"dOut": (M, N), "bx": (M, N), "X": (M, K), "W": (N, K), "dX": (M, K), "nx": (M, K), "dW": (N, K)}[op]


def layout_of(case):
    """{matrix: (ld, offset_floats)} and {vector: (0, offset_floats)}"""
    out = {op: (shape_of(case, op)[1], 0) for op in MATRICES}
    out.update({v: (0, 0) for v in VECTORS})
    for edit in filter(None, case.layout.split(",")):
        if "+" in edit:
            op, pad = edit.split("+")
            out[op] = (out[op][0] + int(pad), out[op][1])
        else:
            op, off = edit.split("@")
            ld = out[op][0]
            out[op] = ((cdiv(ld, 4) * 4) if (op in MATRICES and int(off) % 4) else ld, int(off))
    return out


def build_of(case):
    """which of the three instantiations of a tile family a call takes"""
    return "bn+next" if (case.bn and case.next) else ("bn" if case.bn else "next")


def is_big(case):
    return case.M >= EDGE_ROWS and lc.tile128_ok(case.N) and lc.tile128_ok(case.K)


def family_of(case, use_dma=lc.USE_DMA_DEFAULT):
    """the family plan_both_bn picks, "none" when it refuses"""
    M, N, K, lay = case.M, case.N, case.K, layout_of(case)
    al = lambda *ops: all(lay[o][1] % 4 == 0 for o in ops)
    vec = lambda op: lay[op][1] % 4 == 0 and lay[op][0] % 4 == 0
    if M <= 1 or N <= 0 or K <= 0 or not (case.bn or case.next):
        return "none"
    big = is_big(case)
    if M >= EDGE_ROWS and not (big and case.bn and N <= BNB_MAX_N):
        return "none"
    if case.bn:
        elu_ok = case.bn_act != 2 or (case.beta[0] and al("beta"))
        if not (0 <= case.bn_act <= 2 and lay["bx"][0] >= N and vec("bx") and al("mean", "invstd", "scale", "shift", "coef") and elu_ok):
            return "none"
    if case.bn and (use_dma & 4) and K <= SMALL_MAX and N > SMALL_MAX and N % 4 == 0 and N <= SMALLN_DX_MAX_N:
        # X, W, dX and the prologue vectors are read as scalars by these kernels: only dOut and bn's operands must be aligned
        return "none" if (case.next or not vec("dOut")) else "small_bn"
    if not case.dx or N > BNB_MAX_N:
        return "none"
    if not ((use_dma & 2) and N > 32 and K > 32 and N % 4 == 0 and K % 4 == 0 and vec("dOut") and vec("W") and vec("dX") and vec("X")
            and al("slabs")):
        return "none"
    if case.next:
        elu_ok = case.next_act != 2 or (case.beta[1] and al("nbeta"))
        if not (lay["nx"][0] >= K and vec("nx") and al("npartial", "nmean", "ninvstd", "nscale", "nshift") and 0 <= case.next_act <= 2 and elu_ok):
            return "none"
    return "dma128_bn" if big else "dma64_bn"


def block_rows(case):
    """esc_linear_bwd_bn_block_rows: rows per `next` partial slot"""
    return 128 if is_big(case) else 64


def splits_of(case):
    """(slabs, reduction rows per slab) of a served case"""
    fam = family_of(case)
    if fam == "small_bn":
        return cdiv(case.M, ROWS_WGRAD), ROWS_WGRAD
    bm = 128 if fam == "dma128_bn" else 64
    sp = max(1, min(cdiv(256, cdiv(case.N, bm) * cdiv(case.K, bm)), cdiv(case.M, 128)))
    per = max(128, cdiv(cdiv(case.M, sp), 32) * 32)
    return cdiv(case.M, per), per


def scratch_promised(case):
    """esc_linear_bwd_weight_scratch(M, N, K)"""
    M, N, K = case.M, case.N, case.K
    fine = (K <= SMALL_MAX) != (N <= SMALL_MAX) or (N <= 4 and K <= 256)
    return (cdiv(M, 32 if fine else 128) + 1) * (N * K + N)


def launches_of(case, deferred=False, two_launches=False):
    """kernel launches of a served call (esc_prof_read counts them): the narrow-input family makes one for the slabs, one for dX when it is
    wanted and the slab reduce; the tiles one (two under knob 14) and the reduce"""
    n = (2 + int(case.dx)) if family_of(case) == "small_bn" else (3 if two_launches else 2)
    return n - int(deferred)


# ---- named branches ----------------------------------------------------------------------------------------------------------------
def _acts(fam):
    return ["%s:bn_act%d:%s" % (fam, a, r) for a in (0, 1, 2) for r in ("plain", "mixed")]


BRANCHES = frozenset(
    ["small_bn", "dma64_bn:bn", "dma64_bn:bn+next", "dma64_bn:next", "dma128_bn:bn", "dma128_bn:bn+next"]
    + _acts("small_bn") + _acts("dma64_bn") + _acts("dma128_bn")
    + ["%s:next_act%d:%s" % (f, a, r) for f in ("dma64_bn", "dma128_bn") for a in (0, 1, 2) for r in ("plain", "mixed")]
    + ["dma64_bn:acts%d%d" % (a, b) for a in (0, 1, 2) for b in (0, 1, 2)]
    + ["dma64_bn:next_only_act%d" % a for a in (0, 1, 2)]
    + ["small_bn:M=%d" % m for m in (2, 31, 32, 33, 100)] + ["small_bn:K=%d" % k for k in (1, 3, 4, 10, 16)]
    + ["small_bn:N=%d" % n for n in (20, 64, 68, 848)]
    + ["small_bn:dx_null", "small_bn:dx_null+elu", "small_bn:acc", "small_bn:pro", "small_bn:scalar_operand"]
    + ["dma64_bn:%s:M=%d" % (b, m) for b in ("bn", "bn+next", "next") for m in (2, 63, 64, 65, 129, 130, 257)]
    + ["dma64_bn:N=%d" % n for n in (36, 64, 68, 636, 640)] + ["dma64_bn:K=%d" % k for k in (36, 64, 68, 260, 1280, 1284)]
    + ["dma64_bn:kstep_ragged_N", "dma64_bn:kstep_ragged_K", "dma64_bn:two_slabs", "dma64_bn:acc", "dma64_bn:pro", "dma64_bn:acc+next"]
    + ["dma128_bn:M=8192", "dma128_bn:M=8321", "dma128_bn:128x128", "dma128_bn:120x236", "dma128_bn:640x128", "dma128_bn:pro", "dma128_bn:acc"]
    + ["%s:rows<77" % f for f in ("small_bn", "dma64_bn")]
    + ["%s:%s%s" % (f, op, e) for f in FAMILIES for op in ("dOut", "bx", "X", "W", "dX", "dW") for e in ("+4", "+8", "@4", "@12")]
    + ["%s:nx%s" % (f, e) for f in ("dma64_bn", "dma128_bn") for e in ("+4", "+8", "@4", "@12")]
    + ["refuse:" + r for r in ("N=852", "N=16", "N%4:small", "small+next", "M=1", "N=644", "K=17", "N=20", "N=32", "K=20", "K=32", "no_bn_no_next",
                               "dma64:dx_null", "big:bn_null", "big:tile128_N", "big:tile128_K", "elu:bn_beta_null", "elu:next_beta_null")]
    + ["refuse:%s:%s%s" % (f, op, e) for f in ("dma64_bn", "dma128_bn") for op in ("dOut", "bx", "X", "W", "dX", "nx") for e in ("+1", "@1")]
    + ["refuse:small_bn:%s%s" % (op, e) for op in ("dOut", "bx") for e in ("+1", "@1")]
    + ["refuse:%s:%s@1" % (f, v) for f in FAMILIES for v in BN_VECTORS]
    + ["refuse:%s:%s@1" % (f, v) for f in ("dma64_bn", "dma128_bn") for v in NEXT_VECTORS + ("slabs",)]
    + ["refuse:dma64_bn:nx+2"])


def branches_of(case):
    """the members of BRANCHES a case reaches (by its own transcription: family_of)"""
    fam, M, N, K, out = family_of(case), case.M, case.N, case.K, set()
    edits = [e for e in case.layout.split(",") if e]
    if fam == "none":
        if case.family != "none":
            return out
        meant = case.name.split("-")[1]                     # the family whose neighbour the refusal is
        one = edits[0] if len(edits) == 1 else None
        if one and (one.endswith("+1") or one.endswith("@1") or one == "nx+2"):
            out.add("refuse:%s:%s" % (meant, one))
        tags = {"N=852": meant == "small_bn" and N == 852, "N=16": meant == "small_bn" and N == 16, "N%4:small": meant == "small_bn" and N % 4 != 0,
                "small+next": meant == "small_bn" and case.next and K <= 16, "M=1": M == 1, "N=644": N == 644, "K=17": K == 17,
                "N=20": meant == "dma64_bn" and N == 20, "N=32": meant == "dma64_bn" and N == 32, "K=20": K == 20, "K=32": K == 32,
                "no_bn_no_next": not case.bn and not case.next, "dma64:dx_null": meant == "dma64_bn" and not case.dx,
                "big:bn_null": M >= EDGE_ROWS and not case.bn, "big:tile128_N": M >= EDGE_ROWS and not lc.tile128_ok(N),
                "big:tile128_K": M >= EDGE_ROWS and not lc.tile128_ok(K), "elu:bn_beta_null": case.bn and case.bn_act == 2 and not case.beta[0],
                "elu:next_beta_null": case.next and case.next_act == 2 and not case.beta[1]}
        if not one:
            out |= {"refuse:" + t for t, on in tags.items() if on}
        return out
    build = build_of(case)
    out.add(fam if fam == "small_bn" else "%s:%s" % (fam, build))
    if case.bn:
        out.add("%s:bn_act%d:%s" % (fam, case.bn_act, case.regime))
    if case.next:
        out.add("%s:next_act%d:%s" % (fam, case.next_act, case.nregime))
    for e in edits:
        op = e.replace("+", "@").split("@")[0]
        if e[len(op):] in ("+4", "+8", "@4", "@12"):
            out.add("%s:%s" % (fam, e))
        elif fam == "small_bn" and op in ("X", "W", "dX", "dW", "P"):
            out.add("small_bn:scalar_operand")
    if M < 77:
        out.add("%s:rows<77" % fam)
    if fam == "small_bn":
        out |= {"small_bn:M=%d" % M, "small_bn:K=%d" % K, "small_bn:N=%d" % N}
        out |= {t for t, on in (("small_bn:dx_null", not case.dx), ("small_bn:dx_null+elu", not case.dx and case.bn_act == 2),
                                ("small_bn:acc", case.acc and case.dx), ("small_bn:pro", case.pro)) if on}
    elif fam == "dma64_bn":
        out |= {"dma64_bn:%s:M=%d" % (build, M), "dma64_bn:N=%d" % N, "dma64_bn:K=%d" % K}
        if case.bn and case.next:
            out.add("dma64_bn:acts%d%d" % (case.bn_act, case.next_act))
        if build == "next":
            out.add("dma64_bn:next_only_act%d" % case.next_act)
        out |= {t for t, on in (("dma64_bn:kstep_ragged_N", N % 32 != 0), ("dma64_bn:kstep_ragged_K", K % 32 != 0),
                                ("dma64_bn:two_slabs", splits_of(case)[0] >= 2), ("dma64_bn:acc", case.acc), ("dma64_bn:pro", case.pro),
                                ("dma64_bn:acc+next", case.acc and case.next)) if on}
    else:
        out |= {"dma128_bn:M=%d" % M, "dma128_bn:%dx%d" % (N, K)}
        out |= {t for t, on in (("dma128_bn:pro", case.pro), ("dma128_bn:acc", case.acc)) if on}
    return out & BRANCHES | {b for b in out if b.startswith("refuse:")}


# ---- data, reference, bounds -----------------------------------------------------------------------------------------------------
def _f32(t):
    return t.float().double()


def _side(x, act, seed):
    """the fp32 inputs a BatchNorm side hands the entry (as fp64 tensors holding fp32 values) and its fp64 pre-activation"""
    C = x.shape[1]
    mean, _, invstd, _ = nc.ref_stats(x)
    mean, invstd = _f32(mean), _f32(invstd)
    gamma, beta = nc.gamma_beta(C + 2)
    gamma, beta = gamma[2:] if seed % 2 else gamma[:C], beta[2:] if seed % 2 else beta[:C]
    if act == 1:
        x = nc.nudge_relu(x, mean, invstd, gamma, beta, seed)
    scale = _f32(gamma * invstd)
    return dict(x=x, mean=mean, invstd=invstd, gamma=gamma, beta=beta, scale=scale, shift=_f32(beta - mean * scale),
                xh=(x - mean) * invstd, pre=gamma * ((x - mean) * invstd) + beta)


class Data(object):
    """the live fp32 values of every operand of a case, the fp64 reference of every output and its bound.
    inputs: {name: fp64 tensor of fp32 values}; ref / bound: {output: tensor / float or per-column tensor}"""

    def __init__(self, case):
        M, N, K, seed = case.M, case.N, case.K, nc.seed_of(case)
        self.case, i, self.ref, self.bound, self.pre = case, {}, {}, {}, {}
        self.inputs = i
        i["dOut"] = nc.uniform((M, N), seed + 4) * (1 + 0.5 * (torch.arange(N) % 3))
        i["X"], i["W"] = nc.uniform((M, K), seed + 1), nc.uniform((N, K), seed + 2, K ** -0.5)
        if case.bn:
            b = _side(nc.regime_x(M, N, case.regime, seed), case.bn_act, seed)
            g = i["dOut"] * nc.act_grad(b["pre"], case.bn_act)
            coef = _f32(torch.stack((g.sum(0), (g * b["xh"]).sum(0)), 1) / M)
            dy = b["scale"] * (g - coef[:, 0] - b["xh"] * coef[:, 1])
            terms = b["scale"].abs() * (g.abs() + coef[:, 0].abs() + (b["xh"] * coef[:, 1]).abs())
            i.update(bx=b["x"], mean=b["mean"], invstd=b["invstd"], scale=b["scale"], shift=b["shift"], coef=coef, beta=b["beta"], gamma=b["gamma"])
            self.pre["bn"] = b["pre"]
        else:
            dy, terms = i["dOut"], i["dOut"].abs()
        act_x = i["X"]
        if case.pro:
            i["in_scale"], i["in_shift"] = nc.uniform((K,), seed + 5, 0.5) + 1.0, nc.uniform((K,), seed + 6, 0.5)
            act_x = torch.clamp(i["X"] * i["in_scale"] + i["in_shift"], min=0)
        self.dy = dy
        if case.dx:
            if case.acc:
                i["dX0"] = nc.uniform((M, K), seed + 7)
            self.ref["dX"] = dy @ i["W"] + (i["dX0"] if case.acc else 0.0)
        self.ref["dW"] = dy.t() @ act_x
        self.ref["db"] = dy.sum(0)
        for n in ("dX", "dW"):
            if n in self.ref:
                self.bound[n] = 1e-5 * max(1.0, float(self.ref[n].abs().max()))
        # db is a column sum of a BatchNorm backward: about zero, so it is bounded through the terms that cancel.  Any summation
        # order whose longest chain has d additions errs by at most d u sum|t|; the kernels sum a slab's rows, then the slabs in
        # order, so d <= rows per slab + slabs.  Each term carries a few roundings of its own (the fmaf, the product with scale, exp).
        if family_of(case) != "none":
            sp, per = splits_of(case)
            self.bound["db"] = (per + sp + 8) * U * terms.sum(0)
        if case.next and case.dx:
            n = _side(nc.regime_x(M, K, case.nregime, seed + 9), case.next_act, seed + 9)
            i.update(nx=n["x"], nmean=n["mean"], ninvstd=n["invstd"], nscale=n["scale"], nshift=n["shift"], nbeta=n["beta"], ngamma=n["gamma"])
            self.pre["next"] = n["pre"]
            g2 = self.ref["dX"] * nc.act_grad(n["pre"], case.next_act)
            br = block_rows(case)
            both = torch.stack((g2, g2 * n["xh"]), 2)                                      # [M, K, 2]
            self.ref["partial"] = torch.stack([both[r0:r0 + br].sum(0) for r0 in range(0, M, br)])
            self.ref["sums"] = both.sum(0)
            self.bound["sums"] = 1e-5 * max(1.0, float(self.ref["sums"].abs().max()))
            self.bound["partial"] = 1e-5 * torch.clamp(self.ref["partial"].abs().amax((1, 2)), min=1)    # per slot

    def relu_margin(self):
        """the smallest |fp64 pre-activation| over the ReLU sides of the case (inf when it has none)"""
        c, low = self.case, float("inf")
        if c.bn and c.bn_act == 1:
            low = min(low, float(self.pre["bn"].abs().min()))
        if c.next and c.next_act == 1 and "next" in self.pre:
            low = min(low, float(self.pre["next"].abs().min()))
        return low

    def replay_fp32(self, form="centred"):
        """the entry's formulas in fp32 with torch on the CPU, one rounding per operation: form "centred" takes the ELU derivative at
        (x - mean) * scale + beta (what the kernels do), "fused" at x * scale + shift (what they did).  {output: fp32 tensor}"""
        c, i = self.case, self.inputs
        f = lambda n: i[n].float()

        def dact(x, mean, scale, shift, beta, act):
            if act == 0:
                return torch.ones_like(x)
            if act == 1:
                return (x * scale + shift > 0).float()
            v = ((x - mean) * scale + beta) if form == "centred" else (x * scale + shift)
            return torch.where(v > 0, torch.ones_like(v), torch.exp(v))
        out = {}
        if c.bn:
            g = f("dOut") * dact(f("bx"), f("mean"), f("scale"), f("shift"), f("beta"), c.bn_act)
            k1, k2 = f("coef")[:, 0], f("invstd") * f("coef")[:, 1]
            dy = f("scale") * ((f("mean") - f("bx")) * k2 + (g - k1))
        else:
            dy = f("dOut")
        act_x = torch.clamp(f("X") * f("in_scale") + f("in_shift"), min=0) if c.pro else f("X")
        if c.dx:
            out["dX"] = dy @ f("W") + (f("dX0") if c.acc else 0.0)
        out["dW"], out["db"] = dy.t() @ act_x, dy.sum(0)
        if c.next and c.dx:
            g2 = out["dX"] * dact(f("nx"), f("nmean"), f("nscale"), f("nshift"), f("nbeta"), c.next_act)
            both = torch.stack((g2, g2 * ((f("nx") - f("nmean")) * f("ninvstd"))), 2)
            br = block_rows(c)
            out["partial"] = torch.stack([both[r0:r0 + br].sum(0) for r0 in range(0, c.M, br)])
            out["sums"] = out["partial"].double().sum(0).float()
        return out

    def excess(self, got):
        """{output: max over its elements of |got - ref| / bound}"""
        out = {}
        for n, want in self.ref.items():
            if n not in got or n not in self.bound:
                continue
            b = self.bound[n]
            if n == "partial":
                b = b.view(-1, 1, 1)
            d = (got[n].double() - want).abs()
            r = d / b
            r = torch.where(d == 0, torch.zeros_like(r), r)             # (a column whose terms all vanish has bound 0: exact or wrong)
            out[n] = (float("nan") if bool(torch.isnan(r).any()) else float(r.max())) if d.numel() else 0.0
        return out


@functools.lru_cache(maxsize=8)
def data_of(case):
    return Data(case)


# outputs that pass by the fp32-CPU-oracle rule (at most 3x the error of replay_fp32("centred")) instead of their bar, by case name
# (DESIGN.md names them with both errors); any other output over its bar fails
FP32_ORACLE_RULE = {}


# ---- guarded operands on a device --------------------------------------------------------------------------------------------------
def _buf(live, ld, off, outside, device, guard_rows=2):
    rows, width = live.shape
    g = guard_rows * ld + 64
    return lc.Buf(rows, width, ld, off % 4, live.float(), outside, g + (off - off % 4), g, device)


class Operands(object):
    """every buffer of a call: inputs with NaN in padding columns, guard rows and around the per-channel vectors (which are exactly
    N or K floats); outputs pre-filled with NaN inside and the sentinel pattern outside.  `slabs` is exactly the promised floats
    followed by a guard, `npartial` exactly slots * K * 2 floats of NaN followed by a sentinel guard of the same size."""

    def __init__(self, case, data, device, promised=None, slots=None):
        lay, M, N, K, i = layout_of(case), case.M, case.N, case.K, data.inputs
        nan, sen = float("nan"), lc.sentinel()
        self.case, self.lay, self.inputs, self.outputs = case, lay, {}, {}
        mat = lambda op, t: _buf(t, lay[op][0], lay[op][1], nan, device)
        vecs = lambda name, t: _buf(t.reshape(1, -1), t.numel(), lay[name][1], nan, device, guard_rows=0)
        self.inputs.update(dOut=mat("dOut", i["dOut"]), X=mat("X", i["X"]), W=mat("W", i["W"]))
        if case.bn:
            self.inputs["bx"] = mat("bx", i["bx"])
            for v in BN_VECTORS:
                if v != "beta" or case.beta[0]:
                    self.inputs[v] = vecs(v, i[v])
        if case.pro:
            for v in ("in_scale", "in_shift"):
                self.inputs[v] = _buf(i[v].reshape(1, -1), K, lay["P"][1], nan, device, guard_rows=0)
        if case.next:
            nx = i["nx"] if "nx" in i else nc.uniform((M, K), 3)
            self.inputs["nx"] = mat("nx", nx)
            for v in NEXT_VECTORS[1:]:
                if v != "nbeta" or case.beta[1]:
                    self.inputs[v] = vecs(v, i[v] if v in i else nc.uniform((K,), 5) + 2.0)
            slots = cdiv(M, block_rows(case)) if slots is None else slots
            n = slots * K * 2
            self.outputs["npartial"] = lc.Buf(1, n, n, lay["npartial"][1], torch.full((1, n), nan), sen, 64, n + 64, device)
        if case.dx:
            live = i["dX0"] if case.acc else torch.full((M, K), nan)
            self.outputs["dX"] = _buf(live, lay["dX"][0], lay["dX"][1], sen, device)
        self.outputs["dW"] = _buf(torch.full((N, K), nan), lay["dW"][0], lay["dW"][1], sen, device)
        self.outputs["db"] = _buf(torch.full((1, N), nan), N, 0, sen, device, guard_rows=0)
        promised = scratch_promised(case) if promised is None else promised
        self.outputs["slabs"] = lc.Buf(1, promised, promised, lay["slabs"][1], torch.full((1, promised), nan), sen, 64,
                                       cdiv(M, 32) * (N * K + N) + 64, device)

    def ptr(self, name):
        b = self.inputs.get(name) or self.outputs.get(name)
        return None if b is None else b.ptr()

    def results(self):
        """{output: CPU tensor} in the shapes of Data.ref"""
        c, out = self.case, {"dW": self.outputs["dW"].result(), "db": self.outputs["db"].result()[0]}
        if c.dx:
            out["dX"] = self.outputs["dX"].result()
        if c.next:
            out["partial"] = self.outputs["npartial"].result().view(-1, c.K, 2)
            out["sums"] = out["partial"].double().sum(0)
        return out


# ---- the table --------------------------------------------------------------------------------------------------------------------
CASES = []


def _add(family, M, N, K, layout="", build="bn", acts=(1, 1), flags="", regime="plain", nregime=None, beta=(True, True), meant=None):
    """flags: p (prologue), a (accumulate), x (dX == NULL).  meant: for a refused case, the family whose neighbour it is"""
    bn, nxt = build in ("bn", "bn+next"), build in ("bn+next", "next")
    bits = [meant or family, family if meant else "", "%dx%dx%d" % (M, N, K), build, "a%d%d" % acts, flags, layout,
            regime if regime != "plain" else "", ("n" + nregime) if nregime not in (None, "plain") else "",
            "" if beta == (True, True) else "beta%d%d" % (int(beta[0]), int(beta[1]))]
    name = "bnb-" + "-".join(b for b in bits if b)
    CASES.append(Case(name, M, N, K, layout, bn, nxt, acts[0], acts[1], "p" in flags, int("a" in flags), "x" not in flags, regime,
                      nregime or "plain", beta, family))


KEEP_EDITS = ("+4", "+8", "@4", "@12")


def _table():
    S, D, B = "small_bn", "dma64_bn", "dma128_bn"
    # ---- the narrow-input kernels (linear_small.h): K <= 16, 16 < N <= 848, N % 4 == 0, no `next`
    for j, M in enumerate((2, 31, 32, 33, 100)):
        _add(S, M, 20, 10, acts=(j % 3, 1), regime="mixed" if j % 2 else "plain")
    for j, K in enumerate((1, 3, 4, 10, 16)):
        _add(S, 33, 64, K, acts=((j + 2) % 3, 1), flags="pa"[j % 2:j % 2 + 1], regime="plain" if j % 2 else "mixed")
    for N in (20, 64, 68):
        _add(S, 100, N, 16, acts=(2, 1), regime="mixed")
    _add(S, 33, 848, 16, acts=(2, 1), regime="mixed", flags="a")
    for a in (0, 1, 2):
        for reg in ("plain", "mixed", "offset", "tiny"):
            _add(S, 100, 68, 10, acts=(a, 1), regime=reg)
    for flags, a in (("x", 1), ("x", 2), ("xp", 0), ("a", 2), ("p", 2), ("pa", 1)):
        _add(S, 33, 64, 10, acts=(a, 1), flags=flags, regime="mixed")
    for op in ("dOut", "bx", "X", "W", "dX", "dW"):
        for e in KEEP_EDITS:
            _add(S, 33, 68, 10, op + e, acts=(2, 1), regime="mixed", flags="a" if op == "dX" else "")
    for e in ("X+1", "X@1", "W+1", "W@1", "dX+1", "dX@1", "dW+1", "dW@1", "P@1"):          # scalar reads and writes: served
        _add(S, 33, 68, 10, e, acts=(1, 1), regime="mixed", flags="p" if e == "P@1" else "")
    for e in ("dOut+1", "dOut@1", "bx+1", "bx@1") + tuple(v + "@1" for v in BN_VECTORS):
        _add("none", 33, 68, 10, e, acts=(2, 1), meant=S)
    _add("none", 33, 852, 16, meant=S)
    _add("none", 33, 16, 10, meant=S)
    _add("none", 33, 18, 10, meant=S)
    _add("none", 33, 68, 10, build="bn+next", meant=S)
    _add("none", 33, 68, 10, acts=(2, 1), beta=(False, True), meant=S)
    # ---- the 64x64 tile in its three builds
    for build in ("bn", "bn+next", "next"):
        for j, M in enumerate((2, 63, 64, 65, 129, 130, 257)):
            _add(D, M, 36 if j % 2 else 68, 36, build=build, acts=(j % 3, (j + 1) % 3), regime="mixed" if j % 2 else "plain",
                 nregime="plain" if j % 2 else "mixed")
    for N in (36, 64, 68, 636, 640):
        _add(D, 65, N, 36, build="bn+next", acts=(2, 2), regime="mixed", nregime="mixed")
    for K in (36, 64, 68, 260):
        _add(D, 65, 36, K, build="bn+next", acts=(2, 1), regime="mixed", nregime="mixed", flags="p")
    _add(D, 65, 36, 1280, acts=(2, 1), regime="mixed", flags="p")
    _add(D, 65, 36, 1284, acts=(1, 1), flags="p")          # the prologue of the dW job is per column: no PRO_MAX_K limit here
    for a in (0, 1, 2):
        for b in (0, 1, 2):
            for reg in ("plain", "mixed"):
                _add(D, 130, 68, 36, build="bn+next", acts=(a, b), regime=reg, nregime=reg)
        for reg in ("plain", "mixed", "offset", "tiny"):
            _add(D, 130, 68, 36, build="bn", acts=(a, 1), regime=reg)
            _add(D, 130, 68, 36, build="next", acts=(1, a), nregime=reg)
    for reg in ("offset", "tiny"):
        _add(D, 130, 64, 36, build="bn+next", acts=(2, 2), regime=reg, nregime=reg)
    for flags in ("a", "p", "pa"):
        _add(D, 130, 68, 36, build="bn+next", acts=(2, 2), flags=flags, regime="mixed", nregime="mixed")
        _add(D, 130, 68, 36, build="next", acts=(1, 2), flags=flags, nregime="mixed")
    for op in ("dOut", "bx", "X", "W", "dX", "nx", "dW"):
        for e in KEEP_EDITS:
            _add(D, 130, 68, 36, op + e, build="bn+next", acts=(2, 2), regime="mixed", nregime="mixed", flags="a" if op == "dX" else "")
    _add(D, 130, 68, 36, "dW+1", acts=(1, 1))
    _add(D, 130, 68, 36, "P@1", acts=(1, 1), flags="p")
    for op in ("dOut", "bx", "X", "W", "dX", "nx"):
        for e in ("+1", "@1"):
            _add("none", 130, 68, 36, op + e, build="bn+next", acts=(2, 2), meant=D)
    _add("none", 130, 68, 36, "nx+2", build="bn+next", meant=D)
    for v in BN_VECTORS + NEXT_VECTORS + ("slabs",):
        _add("none", 130, 68, 36, v + "@1", build="bn+next", acts=(2, 2), meant=D)
    for M, N, K in ((1, 68, 36), (130, 644, 36), (130, 36, 17), (130, 20, 36), (130, 32, 36), (130, 36, 20), (130, 36, 32)):
        _add("none", M, N, K, build="bn+next", meant=D)
    _add("none", 130, 68, 36, build="none", meant=D)
    _add("none", 130, 68, 36, flags="x", meant=D)
    _add("none", 130, 68, 36, acts=(2, 1), beta=(False, True), meant=D)
    _add("none", 130, 68, 36, build="bn+next", acts=(1, 2), beta=(True, False), meant=D)
    # ---- the 128x128 tile: edge-sized rows, N and K pass tile128_ok, bn given
    _add(B, 8192, 128, 128, acts=(1, 1))
    _add(B, 8321, 128, 128, build="bn+next", acts=(2, 2), regime="mixed", nregime="mixed", flags="p")
    _add(B, 8192, 120, 236, build="bn+next", acts=(1, 0), nregime="mixed")
    _add(B, 8192, 120, 236, build="bn+next", acts=(0, 1), flags="a")
    _add(B, 8321, 120, 236, acts=(2, 1), regime="mixed", flags="pa")
    _add(B, 8192, 640, 128, acts=(0, 1), regime="mixed")
    _add(B, 8321, 640, 128, "dOut+4,bx+8,X+4,W+4,dX+8,nx+4,dW+4", build="bn+next", acts=(2, 1), nregime="mixed")
    _add(B, 8321, 128, 128, "dOut@4,bx@12,X@4,W@12,dX@4,nx@12,dW@4", build="bn+next", acts=(1, 2), regime="mixed", flags="a")
    _add(B, 8192, 128, 128, "dOut+8,bx+4,X+8,W+8,dX+4,nx+8,dW+8", build="bn+next", acts=(0, 2), nregime="mixed")
    _add(B, 8192, 128, 128, "dOut@12,bx@4,X@12,W@4,dX@12,nx@4,dW@12", build="bn+next", acts=(2, 0), regime="plain")
    for reg in ("offset", "tiny"):
        _add(B, 8192, 128, 128, build="bn+next", acts=(2, 2), regime=reg, nregime=reg)
    _add("none", 8192, 128, 128, build="next", meant=B)
    _add("none", 8192, 100, 128, meant=B)
    _add("none", 8192, 128, 300, meant=B)
    for op in ("dOut", "bx", "X", "W", "dX", "nx"):
        for e in ("+1", "@1"):
            _add("none", 8192, 128, 128, op + e, build="bn+next", acts=(2, 2), meant=B)
    for v in BN_VECTORS + NEXT_VECTORS + ("slabs",):
        _add("none", 8192, 128, 128, v + "@1", build="bn+next", acts=(2, 2), meant=B)


_table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES), "duplicate case names"


def served():
    return [c for c in CASES if c.family != "none"]


def refused():
    return [c for c in CASES if c.family == "none"]


# one case per family and activation whose statistics and coef come from the library (esc_bn_stats, esc_bn_bwd_coef) and whose
# `next` partials go on through esc_bn_bwd_coef_from_partials: what the step engines do
CHAINED = ("bnb-small_bn-100x68x10-bn-a01-mixed", "bnb-small_bn-100x68x10-bn-a11-mixed", "bnb-small_bn-100x68x10-bn-a21-mixed",
           "bnb-dma64_bn-130x68x36-bn+next-a00-mixed-nmixed", "bnb-dma64_bn-130x68x36-bn+next-a11-mixed-nmixed",
           "bnb-dma64_bn-130x68x36-bn+next-a22-mixed-nmixed", "bnb-dma128_bn-8192x640x128-bn-a01-mixed",
           "bnb-dma128_bn-8321x128x128-bn+next-a12-a-dOut@4,bx@12,X@4,W@12,dX@4,nx@12,dW@4-mixed",
           "bnb-dma128_bn-8321x128x128-bn+next-a22-p-mixed-nmixed")
# the deferred slab reduce and the two-launch form (knob 14), once per family
DEFERRED = ("bnb-small_bn-100x68x10-bn-a21-mixed", "bnb-dma64_bn-130x68x36-bn+next-a22-mixed-nmixed", "bnb-dma128_bn-8192x128x128-bn-a11")
TWO_LAUNCHES = DEFERRED[1:]
# where the ELU derivative's pre-activation is ill-conditioned: with the fused form fmaf(x, scale, shift) these fail
ELU_ILL_CONDITIONED = tuple(c.name for c in CASES if c.family != "none" and ((c.bn and c.bn_act == 2 and c.regime in ("offset", "tiny", "mixed"))
                                                                             or (c.next and c.next_act == 2 and c.nregime in ("offset", "tiny", "mixed"))))
