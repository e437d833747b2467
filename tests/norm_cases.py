"""The BatchNorm case table: one record per (entry point, shape, operand layout, argument combination, knob setting, data
regime) chosen so that every branch of the host predicates in csrc/norm_plan.h (and bn_fold_column in common.h) is reached by
name.  No GPU is needed to import or check this module (tests/test_norm_cases_cpu.py); tests/test_hip_norm_dispatch.py runs
the table against the library, and tests/test_norm_plan_cpu.py holds the header the library decides with to family_of, which
stays an independent transcription.  The guarded buffers are those of tests/linear_cases.py.

A case is Case(name, entry, M, C, layout, act, has_Y, affine, running, fused, in_place, knobs, regime, extra, family):
  entry     stats | stats_partials | stats_partials_rows | affine_fold | apply | affine | eval_coef | bwd | bwd_sums | bwd_coef |
            bwd_apply | coef_partials | bwd_dropout          (esc_bn_* / esc_affine_act*; the SyncBN trio has its own list)
  layout    comma-separated edits of the plain layout (16-byte aligned base, ld == C):
              "X+1"    matrix X has ld = C + 1             "X@1"  its base is 1 float past a 16-byte boundary (ld rounded up to 4)
              matrices: X, Y, dY, dX; vectors: mean (mean and invstd), gamma (gamma and beta), P (scale and shift), S (scratch)
  act       0 none, 1 ReLU, 2 ELU                has_Y     the backward is given the forward output
  affine    gamma / beta given (else NULL)       running   running_mean / running_var given
  fused     scale / shift wanted                 in_place  dX is dY
  knobs     ((knob, value), ...) set through esc_tune_set around the call
  regime    plain | offset | tiny | constant | ones | outlier | mixed   (regime_x)
  extra     entry-specific: block_rows (stats_partials_rows, affine_fold), slots (coef_partials), (mask_on_output, p)
            (bwd_dropout), "nograd" (bwd: dgamma = dbeta = NULL)
  family    the kernel family the case is MEANT to reach; family_of() transcribes the predicates and must agree

References are fp64 and written out as the plain formulas; bounds are derived in DESIGN.md ("Dispatch coverage of the
BatchNorm kernels"), never measured.
"""
import collections

import torch

from linear_cases import cdiv

Case = collections.namedtuple("Case", "name entry M C layout act has_Y affine running fused in_place knobs regime extra family")

EPS = 1e-5
MOMENTUM = 0.1
U = 2.0 ** -24                                        # unit roundoff of fp32
NORM_ROWBLOCKS = 512
KNOB_DEFAULTS = {8: 0, 9: 256, 12: 0, 13: 0}
MATRICES, VECTORS = ("X", "Y", "dY", "dX"), ("mean", "gamma", "P", "S")
REGIMES = ("plain", "offset", "tiny", "constant", "ones", "outlier", "mixed")
RELU_MARGIN = 1e-3
BACKWARD_ENTRIES = ("bwd", "bwd_sums", "bwd_coef", "bwd_apply", "bwd_dropout")


def scratch_floats(C):
    """esc_bn_scratch(C)"""
    return NORM_ROWBLOCKS * 4 * C * 2 + 2 * C


def layout_of(case):
    out = {op: (case.C, 0) for op in MATRICES}
    out.update({v: (case.C, 0) for v in VECTORS})
    for edit in filter(None, case.layout.split(",")):
        if "+" in edit:
            op, pad = edit.split("+")
            out[op] = (out[op][0] + int(pad), out[op][1])
        else:
            op, off = edit.split("@")
            out[op] = ((cdiv(out[op][0], 4) * 4) if op in MATRICES else out[op][0], int(off))
    if case.in_place:
        out["dX"] = out["dY"]
    return out


def _knobs(case, knobs=None):
    k = dict(KNOB_DEFAULTS)
    k.update(dict(case.knobs) if knobs is None else dict(knobs))
    return k


def _al(lay, *ops):
    return all(lay[o][1] % 4 == 0 for o in ops)


def _ld4(lay, *ops):
    return all(lay[o][0] % 4 == 0 for o in ops)


def rowblocks(M, wide, backward, cap):
    return max(1, min(cdiv(M, 16), cap if (wide and backward) else 64))


def reduce_family(case, lay, k, allow_fuse, divisor_is_M):
    """bn_bwd_reduce: v4 | scalar | fused_last_block"""
    mats = ("X", "dY") + (("Y",) if case.has_Y else ())
    wide = (case.C % 4 == 0 and _ld4(lay, *mats) and _al(lay, *mats) and _al(lay, "mean", "S")
            and (not case.affine or _al(lay, "gamma")))
    if allow_fuse and wide and case.M <= 4096 and divisor_is_M and k[8]:
        return "fused_last_block"
    return "v4" if wide else "scalar"


def apply_family(case, lay):
    """bn_bwd_apply_impl: rows | flat4 | flat1"""
    mats = ("X", "dY", "dX") + (("Y",) if case.has_Y else ())
    vec = case.C % 4 == 0 and _ld4(lay, *mats) and _al(lay, *mats) and (not case.affine or _al(lay, "gamma"))
    if vec and _al(lay, "mean", "S") and (not case.affine or _al(lay, "gamma")):
        return "rows"               # S: coef lives behind the partials of the same scratch (esc_bn_bwd) or is the coef operand itself
    return "flat4" if vec else "flat1"


def family_of(entry, case, knobs=None):
    """the kernel family the host code of esc_bn_* / esc_affine_act* picks for `case` under `knobs`"""
    lay, k, M, C = layout_of(case), _knobs(case, knobs), case.M, case.C
    if entry == "stats":
        return "stats:v4" if (C % 4 == 0 and _ld4(lay, "X") and _al(lay, "X", "S")) else "stats:scalar"
    if entry == "apply":
        return "apply:flat4" if (C % 4 == 0 and _ld4(lay, "X", "Y") and _al(lay, "X", "Y")) else "apply:flat1"
    if entry == "affine":          # affine_act_kernel<4> needs M >= 2^31
        return "affine:rows" if (C % 4 == 0 and _ld4(lay, "X", "Y") and _al(lay, "X", "Y", "P")) else "affine:flat1"
    if entry == "bwd":
        mats = ("X", "dY", "dX") + (("Y",) if case.has_Y else ())
        node_sized = (64 <= M <= 4096 and C % 4 == 0 and _ld4(lay, *mats) and _al(lay, *mats) and _al(lay, "mean", "S")
                      and (not case.affine or _al(lay, "gamma")))
        if k[13] and node_sized:
            return "bwd:node"
        if k[12] and node_sized and not k[8]:
            return "bwd:fold"
        return "bwd:%s+%s" % (reduce_family(case, lay, k, True, True), apply_family(case, lay))
    if entry == "bwd_sums":
        return "sums:" + reduce_family(case, lay, k, False, False)
    if entry == "bwd_coef":
        return "coef:" + reduce_family(case, lay, k, True, True)
    if entry == "bwd_apply":
        return "bwd_apply:" + apply_family(case, lay)
    if entry == "bwd_dropout":
        return "dropout:out" if case.extra[0] else "dropout:in"
    return {"stats_partials": "partials:32", "stats_partials_rows": "partials:rows", "affine_fold": "fold", "eval_coef": "eval_coef",
            "coef_partials": "coef_partials"}[entry]


FAMILIES = ("stats:v4", "stats:scalar", "partials:32", "partials:rows", "fold", "apply:flat4", "apply:flat1", "affine:rows",
            "affine:flat1", "eval_coef", "bwd:v4+rows", "bwd:v4+flat1", "bwd:scalar+flat4", "bwd:scalar+flat1",
            "bwd:fused_last_block+rows", "bwd:fold", "bwd:node", "sums:v4", "sums:scalar", "coef:v4", "coef:scalar",
            "coef:fused_last_block", "bwd_apply:rows", "bwd_apply:flat4", "bwd_apply:flat1", "coef_partials", "dropout:in",
            "dropout:out")
STAT_FAMILIES = ("stats:v4", "stats:scalar", "partials:32", "partials:rows", "fold")
BWD_FAMILIES = tuple(f for f in FAMILIES if f.split(":")[0] in ("bwd", "sums", "coef", "bwd_apply", "dropout"))
BOUNDARIES = (
    "cols:second_block", "cols:one_live_lane", "cols:five_blocks", "cols:scalar_second_block",
    "stats:idle_slots", "stats:rb_exact", "stats:rb_cap", "stats:second_trip",
    "bwd:one_row", "bwd:rb_exact", "bwd:rb_cap", "bwd:one_block", "bwd:cap512",
    "fused:one_block", "fused:rb_cap", "fused:fallthrough", "fused:not_for_sums",
    "fold:fallthrough_lo", "fold:fallthrough_hi", "fold:rb_cap", "fold:no_dgamma",
    "node:fallthrough_lo", "node:fallthrough_hi", "node:ragged", "rows:ycap",
    "flat:second_trip:apply4", "flat:second_trip:apply1", "flat:second_trip:affine1", "flat:second_trip:bwd_apply1",
    "flat:second_trip:bwd_apply4", "rows:zero", "rows:one",
    "demote:ld+1", "demote:ld+2", "demote:base@1", "demote:mean@1", "demote:gamma@1", "demote:S@1", "demote:P@1", "keep:ld+4",
    "in_place", "null_gamma_beta", "Y:null+elu", "Y:null+relu", "Y:given+elu", "Y:given+relu",
    "partials:lane_takes_two", "partials:one_row_block", "partials:ragged_tail",
    "foldcol:no_full_block", "foldcol:one_chunk", "foldcol:chunk_exact", "foldcol:second_chunk", "foldcol:third_chunk",
    "foldcol:ragged", "foldcol:no_ragged", "fold:no_scale_shift", "fold:no_running", "fold:ld+4",
    "coef_partials:one", "coef_partials:63", "coef_partials:64", "coef_partials:65", "coef_partials:300",
    "dropout:ld+4", "dropout:relu", "dropout:one_row", "dropout:rb_cap")
BRANCHES = frozenset(FAMILIES + BOUNDARIES)


def branches_of(case):
    """the members of BRANCHES a case reaches"""
    fam, k, M, C, lay = family_of(case.entry, case), _knobs(case), case.M, case.C, layout_of(case)
    out = {fam}
    v4 = not ("scalar" in fam or fam.endswith("flat1") or fam in ("eval_coef", "coef_partials", "partials:32", "partials:rows"))
    if v4 and C > 256:
        out.add("cols:second_block")
    if v4 and C == 260:
        out.add("cols:one_live_lane")
    if v4 and C == 1280:
        out.add("cols:five_blocks")
    if "scalar" in fam and C > 64:
        out.add("cols:scalar_second_block")
    for edit in filter(None, case.layout.split(",")):
        op = edit.replace("+", "@").split("@")[0]
        if edit.endswith("+4"):
            out.add("keep:ld+4")
        elif edit.endswith("+1") or edit.endswith("+2"):
            out.add("demote:ld" + edit[-2:])
        elif op in MATRICES:
            out.add("demote:base@1")
        else:
            out.add("demote:%s@1" % op)
    if case.entry == "stats":
        rb = rowblocks(M, v4, False, 0)
        out |= {t for t, on in (("stats:idle_slots", rb * 4 > M), ("stats:rb_exact", M % 16 == 0 and M // 16 <= 64),
                                ("stats:rb_cap", cdiv(M, 16) > 64), ("stats:second_trip", M > 256)) if on}
    if case.entry in ("bwd", "bwd_sums", "bwd_coef", "bwd_dropout") and fam not in ("bwd:node", "bwd:fold"):
        red = fam.split(":")[1].split("+")[0]
        if red in ("v4", "in", "out"):
            out |= {t for t, on in (("bwd:one_row", M == 1), ("bwd:rb_exact", M == 16 or M == 16 * k[9]),
                                    ("bwd:rb_cap", cdiv(M, 16) > k[9]), ("bwd:one_block", k[9] == 1 and M > 16),
                                    ("bwd:cap512", k[9] == 512 and cdiv(M, 16) > 512)) if on}
        if red == "fused_last_block":
            out |= {t for t, on in (("fused:one_block", M <= 32), ("fused:rb_cap", cdiv(M, 32) > 64)) if on}
        if k[8] and M > 4096 and case.entry != "bwd_sums":
            out.add("fused:fallthrough")
        if k[8] and case.entry == "bwd_sums":
            out.add("fused:not_for_sums")
    if case.entry == "bwd":
        if k[12] and not k[8] and fam != "bwd:fold":
            out.add("fold:fallthrough_lo" if M < 64 else "fold:fallthrough_hi")
        if fam == "bwd:fold":
            out |= {t for t, on in (("fold:rb_cap", cdiv(M, 32) > 32), ("fold:no_dgamma", case.extra == "nograd")) if on}
        if k[13] and fam != "bwd:node":
            out.add("node:fallthrough_lo" if M < 64 else "node:fallthrough_hi")
        if fam == "bwd:node" and M % 16:
            out.add("node:ragged")
    rows_form = fam in ("affine:rows", "bwd_apply:rows", "dropout:in", "dropout:out", "bwd:fold") or fam.endswith("+rows")
    if rows_form and cdiv(M, 16) > 2048:
        out.add("rows:ycap")
    flat = {"apply:flat4": ("apply4", 4), "apply:flat1": ("apply1", 1), "affine:flat1": ("affine1", 1), "bwd_apply:flat1": ("bwd_apply1", 1),
            "bwd_apply:flat4": ("bwd_apply4", 4)}.get(fam)
    if flat and M * (C // flat[1]) > 4096 * 256:
        out.add("flat:second_trip:" + flat[0])
    if case.entry in ("apply", "affine") and M <= 1:
        out.add("rows:zero" if M == 0 else "rows:one")
    if case.in_place:
        out.add("in_place")
    if not case.affine and case.entry != "eval_coef":
        out.add("null_gamma_beta")
    if case.entry in ("bwd", "bwd_sums", "bwd_coef", "bwd_apply") and case.act:
        out.add("Y:%s+%s" % ("given" if case.has_Y else "null", "relu" if case.act == 1 else "elu"))
    if case.entry in ("stats_partials", "stats_partials_rows"):
        br = 32 if case.entry == "stats_partials" else case.extra
        out |= {t for t, on in (("partials:lane_takes_two", cdiv(M, br) > 64), ("partials:one_row_block", M % br == 1),
                                ("partials:ragged_tail", M % br > 1)) if on}
    if case.entry == "affine_fold":
        full = M // case.extra
        out |= {t for t, on in (("foldcol:no_full_block", full == 0), ("foldcol:one_chunk", 0 < full < 40), ("foldcol:chunk_exact", full == 40),
                                ("foldcol:second_chunk", 40 < full <= 80), ("foldcol:third_chunk", full > 80), ("foldcol:ragged", M % case.extra),
                                ("foldcol:no_ragged", M % case.extra == 0), ("fold:no_scale_shift", not case.fused),
                                ("fold:no_running", not case.running), ("fold:ld+4", "Y+4" in case.layout)) if on}
    if case.entry == "coef_partials":
        out.add("coef_partials:" + {1: "one"}.get(case.extra, str(case.extra)))
    if case.entry == "bwd_dropout":
        out |= {t for t, on in (("dropout:ld+4", "+4" in case.layout), ("dropout:relu", case.act == 1), ("dropout:one_row", M == 1),
                                ("dropout:rb_cap", cdiv(M, 16) > k[9])) if on}
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------------
def seed_of(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % 100003


KINDS = ("plain", "off100", "off1000", "tiny", "const", "outlier")


def column_kinds(C, regime):
    c = torch.arange(C)
    if regime == "mixed":                      # period 6: every kind meets every position of a column quad
        return c % 6
    if regime == "offset":
        return 1 + c % 2
    return torch.full((C,), {"plain": 0, "tiny": 3, "constant": 4, "ones": 4, "outlier": 5}[regime])


def regime_x(M, C, regime, seed):
    """[M, C] fp64 whose columns each have their own offset and spread:
    plain N(5 + .5j, 3(1 + .1k)); off100 / off1000 |mean| / sigma = 1e2 / 1e3; tiny mean 1, sigma 1e-3; const sigma = 0
    (every column its own constant; `ones`: all 1); outlier N(0, 1) with one row at 1e4"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, C, generator=g, dtype=torch.float64)
    c = torch.arange(C, dtype=torch.float64)
    kind = column_kinds(C, regime)
    sig = 1 + 0.25 * (c % 3)
    sign = 1 - 2 * ((c // 2) % 2)
    cols = [(5 + 0.5 * (c % 7)) + 3 * (1 + 0.1 * (c % 5)) * z,
            sign * 1e2 * sig + sig * z,
            sign * 1e3 * sig + sig * z,
            (1 + 0.125 * (c % 3)) + 1e-3 * z,
            (torch.ones(C, dtype=torch.float64) if regime == "ones" else (0.25 * (c % 9) - 1.25 + (c % 9 == 5) * 0.25)) + 0 * z,
            z.clone()]
    rows = (torch.arange(C) * 7919 + 3) % M
    cols[5][rows, torch.arange(C)] = 1e4
    x = torch.zeros(M, C, dtype=torch.float64)
    for i, col in enumerate(cols):
        x = torch.where((kind == i).unsqueeze(0), col, x)
    return x.float().double()                  # the fp32 values the kernel sees


def constant_columns(C, regime):
    return column_kinds(C, regime) == 4


def gamma_beta(C):
    """every column its own gamma (|gamma| in .5 .. 1.5, every third negative) and beta (|beta| in .1 .. 1, alternating sign)"""
    c = torch.arange(C, dtype=torch.float64)
    gamma = (0.5 + 0.25 * (c % 5)) * (1 - 2 * (c % 3 == 2).double())
    beta = (0.1 + 0.15 * (c % 7)) * (1 - 2 * (c % 2))
    return gamma.float().double(), beta.float().double()


def uniform(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().double()


# ---- the references: plain formulas, any dtype ------------------------------------------------------------------------------------
def act(v, code):
    if code == 1:
        return torch.clamp(v, min=0)
    if code == 2:
        return torch.where(v > 0, v, torch.expm1(v))
    return v


def act_grad(v, code):
    if code == 1:
        return (v > 0).to(v.dtype)
    if code == 2:
        return torch.where(v > 0, torch.ones_like(v), torch.exp(v))
    return torch.ones_like(v)


def ref_stats(x, eps=EPS):
    """mean, biased variance, invstd, unbiased variance of the columns of x"""
    M = x.shape[0]
    mean = x.sum(0) / M
    var = ((x - mean) ** 2).sum(0) / M
    return mean, var, 1 / torch.sqrt(var + eps), var * M / max(M - 1, 1)


def ref_running(rm, rv, mean, unbiased, momentum=MOMENTUM):
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unbiased


def ref_forward(x, mean, invstd, gamma, beta, code):
    return act(gamma * ((x - mean) * invstd) + beta, code)


def ref_backward(x, dy, mean, invstd, gamma, beta, code, keep_in=None, keep_out=None, p=0.0, coef=None):
    """g = dY act'(pre); dbeta = sum g; dgamma = sum g xhat; dX = gamma invstd (g - sum g / M - xhat sum g xhat / M).
    keep_in: dY is the gradient of dropout(act(bn(x))); keep_out: x was dropout(input).  coef given: it replaces the two means."""
    M = x.shape[0]
    xh = (x - mean) * invstd
    g = dy if keep_in is None else dy * keep_in / (1 - p)
    g = g * act_grad(gamma * xh + beta, code)
    dbeta, dgamma = g.sum(0), (g * xh).sum(0)
    k1, k2 = (dbeta / M, dgamma / M) if coef is None else (coef[:, 0], coef[:, 1])
    dx = gamma * invstd * (g - k1 - xh * k2)
    if keep_out is not None:
        dx = dx * keep_out / (1 - p)
    return {"dX": dx, "dgamma": dgamma, "dbeta": dbeta, "sums": torch.stack((dbeta, dgamma), 1), "coef": torch.stack((dbeta, dgamma), 1) / M}


def nudge_relu(x, mean, invstd, gamma, beta, seed):
    """move every x whose pre-activation lies within RELU_MARGIN of zero to 4 RELU_MARGIN on a side fixed by (row, column, seed)"""
    r = torch.arange(x.shape[0]).unsqueeze(1)
    c = torch.arange(x.shape[1]).unsqueeze(0)
    side = (((r * 31 + c * 17 + seed) % 2) * 2 - 1).double()
    for _ in range(4):
        pre = gamma * ((x - mean) * invstd) + beta
        bad = pre.abs() < 2 * RELU_MARGIN
        if not bool(bad.any()):
            break
        x = torch.where(bad, mean + (side * 4 * RELU_MARGIN - beta) / (gamma * invstd), x).float().double()
    low = float((gamma * ((x - mean) * invstd) + beta).abs().min()) if x.numel() else RELU_MARGIN
    assert low >= RELU_MARGIN, "nudge_relu left a pre-activation %.3g from the kink" % low
    return x


# ---- bounds (per column; DESIGN.md derives them) -------------------------------------------------------------------------------------
def colmax(t):
    if t.dim() == 2:
        return t.abs().max(0).values if t.shape[0] > 0 else torch.zeros(t.shape[1], dtype=t.dtype)
    return t.abs()


def bound_mean(mean):
    return 1e-5 * torch.clamp(mean.abs(), min=1)


def rel_invstd(mean, invstd):
    return 1e-5 + 2 * U * mean.abs() * invstd


def bound_invstd(mean, invstd):
    return rel_invstd(mean, invstd) * invstd


def bound_running_mean(rm_ref, rm0, mean, momentum=MOMENTUM):
    return momentum * bound_mean(mean) + 4 * U * ((1 - momentum) * rm0.abs() + momentum * mean.abs())


def bound_running_var(rv_ref, mean, invstd, unbiased, momentum=MOMENTUM):
    return momentum * 2 * rel_invstd(mean, invstd) * (unbiased + EPS) + 4 * U * rv_ref.abs()


def bound_scale(mean, invstd, gamma):
    return gamma.abs() * bound_invstd(mean, invstd) + 2 * U * (gamma * invstd).abs()


def bound_shift(mean, invstd, gamma, beta):
    sc = (gamma * invstd).abs()
    return sc * bound_mean(mean) + mean.abs() * bound_scale(mean, invstd, gamma) + 2 * U * (beta.abs() + mean.abs() * sc)


def bound_y(y_ref, x, mean, invstd, gamma):
    return 1e-5 * torch.clamp(colmax(y_ref), min=1) + 4 * U * gamma.abs() * invstd * torch.maximum(mean.abs(), colmax(x))


def bound_grad(ref):
    return 1e-5 * torch.clamp(colmax(ref), min=1)


class Data(object):
    """the live fp32 values of every operand of a case (as fp64 tensors holding fp32 values), its fp64 references and bounds.
    inputs / outputs: {name: [rows, width] tensor}; ref / bound: {output name: tensor}"""

    def __init__(self, case):
        M, C, e, seed = case.M, case.C, case.entry, seed_of(case)
        self.case, self.inputs, self.ref, self.bound, self.pre = case, {}, {}, {}, None
        i, f32 = self.inputs, (lambda t: t.float().double())
        gamma, beta = gamma_beta(C) if case.affine else (torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64))
        if case.affine:
            i["gamma"], i["beta"] = gamma, beta
        if e == "eval_coef":
            i["rm"], i["rv"] = uniform((C,), seed, 3.0), uniform((C,), seed + 1, 1.0).abs() + 1e-3
            sc = gamma / torch.sqrt(i["rv"] + EPS)
            self.ref = {"scale": sc, "shift": beta - i["rm"] * sc}
            self.bound = {"scale": 8 * U * sc.abs(), "shift": 8 * U * (beta.abs() + (i["rm"] * sc).abs())}
            return
        if e == "coef_partials":
            part = uniform((case.extra, C, 2), seed, 2.0)
            i["partial"] = part.view(case.extra, 2 * C)
            s = part.sum(0)
            self.ref = {"coef": s / M, "dgamma": s[:, 1], "dbeta": s[:, 0]}
            self.bound = {n: bound_grad(v) if v.dim() == 1 else 1e-5 * torch.clamp(v.abs(), min=1) for n, v in self.ref.items()}
            return
        x = regime_x(max(M, 1), C, case.regime, seed)[:M]
        if e in ("stats", "stats_partials", "stats_partials_rows", "affine_fold"):
            mean, var, invstd, unbiased = ref_stats(x)
            self.ref.update(mean=mean, invstd=invstd)
            self.bound.update(mean=bound_mean(mean), invstd=bound_invstd(mean, invstd))
            if case.running:
                i["rm"], i["rv"] = uniform((C,), seed + 2, 2.0), uniform((C,), seed + 3, 0.5) + 1.0
                self.ref["rm"], self.ref["rv"] = ref_running(i["rm"], i["rv"], mean, unbiased)
                self.bound["rm"] = bound_running_mean(self.ref["rm"], i["rm"], mean)
                self.bound["rv"] = bound_running_var(self.ref["rv"], mean, invstd, unbiased)
            if case.fused:
                self.ref["scale"] = gamma * invstd
                self.ref["shift"] = beta - mean * self.ref["scale"]
                self.bound["scale"], self.bound["shift"] = bound_scale(mean, invstd, gamma), bound_shift(mean, invstd, gamma, beta)
            if e != "stats":
                br = {"stats_partials": 32}.get(e, case.extra)
                blocks = [x[r0:r0 + br] for r0 in range(0, M, br)]
                i["partials"] = f32(torch.stack([torch.stack((b.mean(0), ((b - b.mean(0)) ** 2).sum(0)), 1) for b in blocks])).view(len(blocks), 2 * C)
            if e != "affine_fold":
                i["X"] = x
            else:
                i["X"] = x
                self.ref["Y"] = ref_forward(x, mean, invstd, gamma, beta, case.act)
                self.bound["Y"] = bound_y(self.ref["Y"], x, mean, invstd, gamma)
            return
        mean, var, invstd, _ = ref_stats(x) if M > 0 else (torch.zeros(C, dtype=torch.float64),) * 4
        if M == 1:
            invstd = torch.full((C,), 1.0, dtype=torch.float64) / (1 + 0.25 * (torch.arange(C) % 3))
        mean, invstd = f32(mean), f32(invstd)                     # inputs of these entry points: the reference uses the same values
        if e == "apply":
            i.update(X=x, mean=mean, invstd=invstd)
            self.ref["Y"] = ref_forward(x, mean, invstd, gamma, beta, case.act)
            self.bound["Y"] = bound_y(self.ref["Y"], x, mean, invstd, gamma)
            return
        if e == "affine":
            sc = f32(gamma * invstd)
            sh = f32(beta - mean * sc)
            i.update(X=x, scale=sc, shift=sh)
            self.ref["Y"] = act(x * sc + sh, case.act)
            self.bound["Y"] = 1e-5 * torch.clamp(colmax(self.ref["Y"]), min=1) + 4 * U * torch.maximum(sh.abs(), sc.abs() * colmax(x))
            return
        assert e in BACKWARD_ENTRIES, e
        if case.act == 1:
            x = nudge_relu(x, mean, invstd, gamma, beta, seed)
        self.pre = gamma * ((x - mean) * invstd) + beta
        # the condition every ReLU case carries, on the CPU and on the GPU: no fp64 pre-activation within RELU_MARGIN of the kink
        assert case.act != 1 or float(self.pre.abs().min()) >= RELU_MARGIN, (case.name, float(self.pre.abs().min()))
        dy = uniform((M, C), seed + 4) * (1 + 0.5 * (torch.arange(C) % 3))
        i.update(X=x, dY=dy, mean=mean, invstd=invstd)
        if case.has_Y:
            i["Y"] = f32(act(self.pre, case.act))
        keep_in = keep_out = None
        p = 0.0
        if e == "bwd_dropout":
            on_output, p = case.extra
            g = torch.Generator().manual_seed(seed + 5)
            keep = (torch.rand(M, C, generator=g) >= p)
            i["mask"] = keep.to(torch.uint8)
            keep_in, keep_out = (None, keep.double()) if on_output else (keep.double(), None)
            p = float(torch.tensor(p, dtype=torch.float32))
        full = ref_backward(x, dy, mean, invstd, gamma, beta, case.act, keep_in, keep_out, p)
        if e == "bwd_apply":
            i["coef"] = f32(full["coef"])
            full = ref_backward(x, dy, mean, invstd, gamma, beta, case.act, coef=i["coef"])
        want = {"bwd": ("dX", "dgamma", "dbeta"), "bwd_dropout": ("dX", "dgamma", "dbeta"), "bwd_sums": ("sums", "dgamma", "dbeta"),
                "bwd_coef": ("coef", "dgamma", "dbeta"), "bwd_apply": ("dX",)}[e]
        if case.extra == "nograd":
            want = ("dX",)
        for n in want:
            self.ref[n] = full[n]
            self.bound[n] = bound_grad(full[n]) if n in ("dX", "dgamma", "dbeta") else 1e-5 * torch.clamp(full[n].abs(), min=1)

    def fp32_error(self):
        """the error of the same backward formulas evaluated in fp32 with torch on the CPU, per output, against the fp64 reference
        (the project's fallback bar: DESIGN.md 'as accurate as the fp32 CPU oracle')"""
        c, i = self.case, self.inputs
        f = lambda n: i[n].float() if n in i else None
        C = c.C
        gamma = f("gamma") if c.affine else torch.ones(C)
        beta = f("beta") if c.affine else torch.zeros(C)
        keep_in = keep_out = None
        p = 0.0
        if c.entry == "bwd_dropout":
            p = float(torch.tensor(c.extra[1], dtype=torch.float32))
            keep_in, keep_out = (None, i["mask"].float()) if c.extra[0] else (i["mask"].float(), None)
        got = ref_backward(f("X"), f("dY"), f("mean"), f("invstd"), gamma, beta, c.act, keep_in, keep_out, p, coef=f("coef"))
        return {n: (got[n].double() - r).abs() for n, r in self.ref.items()}


# ---- the table --------------------------------------------------------------------------------------------------------------------
CASES = []


def _add(entry, family, M, C, layout="", act=0, Y=False, affine=True, running=False, fused=False, in_place=False, knobs=(),
         regime="plain", extra=None):
    knobs = tuple(sorted(knobs))
    bits = [entry, family.split(":")[-1], "%dx%d" % (M, C)]
    if layout:
        bits.append(layout)
    flags = "a%d" % act + ("y" if Y else "") + ("" if affine else "n") + ("r" if running else "") + ("f" if fused else "") + ("i" if in_place else "")
    bits.append(flags)
    if knobs:
        bits.append("k" + "_".join("%d=%d" % kv for kv in knobs))
    if regime != "plain":
        bits.append(regime)
    if extra is not None:
        bits.append("x" + str(extra).replace(" ", "").replace("(", "").replace(")", "").replace(",", "_"))
    CASES.append(Case("-".join(bits), entry, M, C, layout, act, Y, affine, running, fused, in_place, knobs, regime, extra, family))


def _table():
    V4_WIDTHS, SC_WIDTHS = (4, 64, 256, 260, 300, 1280), (1, 10, 63, 65, 66)
    THREE = ("plain", "mixed", "constant")
    # ---- forward statistics
    for C in V4_WIDTHS:
        _add("stats", "stats:v4", 37, C, running=True, fused=True, regime="mixed")
    for C in SC_WIDTHS:
        _add("stats", "stats:scalar", 37, C, running=True, fused=True, regime="mixed")
    for M in (2, 3, 5, 16, 17, 1024, 1025, 4097):
        _add("stats", "stats:v4", M, 8, running=True, fused=True, regime="mixed")
        _add("stats", "stats:scalar", M, 7, running=True, fused=True, regime="mixed")
    for reg in REGIMES:
        _add("stats", "stats:v4", 1025, 12, running=True, fused=True, regime=reg)
        _add("stats", "stats:scalar", 1025, 10, running=True, fused=True, regime=reg)
    _add("stats", "stats:v4", 4097, 12, running=True, regime="offset")
    _add("stats", "stats:v4", 37, 300, affine=False, fused=True)
    _add("stats", "stats:v4", 37, 300)
    for C in (256, 300):
        _add("stats", "stats:v4", 37, C, "X+4", regime="mixed")
        for edit in ("X+1", "X+2", "X@1", "S@1"):
            _add("stats", "stats:scalar", 37, C, edit, running=True, fused=True, regime="mixed")
    # ---- the partial forms
    for M in (2, 32, 33, 2049):
        for reg in THREE + ("offset",):
            _add("stats_partials", "partials:32", M, 10, running=True, fused=True, regime=reg)
    for br, M in ((64, 64 * 3 + 17), (128, 128 * 2 + 1), (128, 128 * 66 + 100), (64, 128)):
        for reg in THREE:
            _add("stats_partials_rows", "partials:rows", M, 12, running=True, fused=(reg != "plain"), regime=reg, extra=br)
    for full in (0, 1, 40, 41, 85):
        for ragged in (False, True):
            if full == 0 and not ragged:
                continue
            M = 32 * full + (20 if ragged else 0)
            for C, reg in ((4, "mixed"), (300, "plain"), (1280, "mixed")):
                if C == 1280 and full not in (1, 41):
                    continue
                _add("affine_fold", "fold", M, C, act=1, running=True, fused=True, regime=reg, extra=32)
    _add("affine_fold", "fold", 84, 300, "Y+4", act=2, running=False, fused=False, regime="constant", extra=32)
    _add("affine_fold", "fold", 84, 300, "X+4,Y+4", act=0, affine=False, running=True, fused=True, regime="offset", extra=64)
    _add("affine_fold", "fold", 128 * 3 + 5, 8, act=1, running=True, regime="ones", extra=128)
    # ---- the forward elementwise passes
    for ent, v, s, v_big in (("apply", "apply:flat4", "apply:flat1", (4100, 1280)), ("affine", "affine:rows", "affine:flat1", (32784, 4))):
        for C in V4_WIDTHS:
            _add(ent, v, 37, C, act=1, regime="mixed")
        for C in SC_WIDTHS:
            _add(ent, s, 37, C, act=2, regime="mixed")
        for a in (0, 1, 2):
            _add(ent, v, 131, 12, act=a, regime="constant")
            _add(ent, s, 131, 10, act=a, regime="offset")
        for M in (0, 1):
            _add(ent, v, M, 8, act=1)
            _add(ent, s, M, 7, act=1)
        _add(ent, v, v_big[0], v_big[1], act=1)
        _add(ent, s, 4100, 257, act=1)
        for C in (256, 300):
            _add(ent, v, 37, C, "X+4,Y+4", act=1)
            for edit in ("X+1", "Y+2", "X@1", "Y@1"):
                _add(ent, s, 37, C, edit, act=1)
    _add("apply", "apply:flat4", 37, 300, "mean@1,gamma@1", act=1)           # the flat kernel reads its vectors as scalars
    _add("apply", "apply:flat4", 37, 300, act=1, affine=False)
    _add("affine", "affine:flat1", 37, 300, "P@1", act=1)
    for C in (1, 255, 256, 257):
        for aff in (True, False):
            _add("eval_coef", "eval_coef", 2, C, affine=aff)
    # ---- the backward: every family x act x Y
    FAM = (("bwd:v4+rows", 12, "", ()), ("bwd:v4+flat1", 12, "dX+1", ()), ("bwd:scalar+flat4", 12, "mean@1", ()),
           ("bwd:scalar+flat1", 10, "", ()), ("bwd:fused_last_block+rows", 12, "", ((8, 1),)), ("bwd:fold", 12, "", ((12, 1),)))
    for fam, C, lay, kn in FAM:
        for a, y in ((0, False), (1, True), (1, False), (2, True), (2, False)):
            _add("bwd", fam, 131, C, lay, act=a, Y=y, knobs=kn)
        for reg in ("mixed", "constant", "offset", "outlier", "tiny", "ones"):
            _add("bwd", fam, 131, C, lay, act=1, Y=True, knobs=kn, regime=reg)
        _add("bwd", fam, 131, C, lay, act=2, Y=False, knobs=kn, regime="mixed")
        _add("bwd", fam, 131, C, lay, act=1, Y=False, knobs=kn, affine=False, regime="offset")     # (no beta: a constant column would sit ON the kink)
    for C in V4_WIDTHS:
        _add("bwd", "bwd:v4+rows", 37, C, act=1, Y=True, regime="mixed")
        _add("bwd", "bwd:v4+rows", 37, C, "X+4,Y+4,dY+4,dX+4", act=1, Y=True)
    for C in SC_WIDTHS:
        _add("bwd", "bwd:scalar+flat1", 37, C, act=1, Y=True, regime="mixed")
    for C in (256, 300):
        for edit in ("X+1", "dY+2", "X@1", "Y@1"):
            _add("bwd", "bwd:scalar+flat1", 37, C, edit, act=1, Y=True)
        _add("bwd", "bwd:v4+flat1", 37, C, "dX@1", act=1, Y=True)
        _add("bwd", "bwd:scalar+flat1", 37, C, "gamma@1", act=1, Y=False)
        _add("bwd", "bwd:scalar+flat4", 37, C, "S@1", act=1, Y=True)
        _add("bwd", "bwd:scalar+flat4", 37, C, "mean@1", act=2, Y=False)
    for M in (1, 15, 16, 17, 4096, 4097):
        _add("bwd", "bwd:v4+rows", M, 8, act=1, Y=True, regime="mixed")
        _add("bwd", "bwd:scalar+flat1", M, 7, act=1, Y=False, regime="mixed")
    _add("bwd", "bwd:v4+rows", 700, 8, act=1, Y=True, knobs=((9, 1),), regime="mixed")
    _add("bwd", "bwd:v4+rows", 8200, 8, act=1, Y=True, knobs=((9, 512),), regime="mixed")
    _add("bwd", "bwd:v4+rows", 32784, 4, act=1, Y=False)
    for C in (300, 1280):
        for M in (1, 31, 32, 33, 2048, 2049, 4096):
            _add("bwd", "bwd:fused_last_block+rows", M, C, act=1, Y=(M % 2 == 0), knobs=((8, 1),), regime="mixed" if C == 300 else "plain")
        _add("bwd", "bwd:v4+rows", 4097, C, act=1, Y=True, knobs=((8, 1),))
    for M in (64, 1024, 1025, 4096):
        _add("bwd", "bwd:fold", M, 300, act=1, Y=(M % 2 == 0), knobs=((12, 1),), regime="mixed")
    _add("bwd", "bwd:v4+rows", 63, 300, act=1, Y=True, knobs=((12, 1),))
    _add("bwd", "bwd:v4+rows", 4097, 300, act=1, Y=True, knobs=((12, 1),))
    _add("bwd", "bwd:fold", 1025, 300, act=1, Y=True, knobs=((12, 1),), extra="nograd")
    _add("bwd", "bwd:fused_last_block+rows", 1025, 300, act=1, Y=True, knobs=((8, 1), (12, 1)))      # knob 8 wins over knob 12
    # in place: dX over dY
    _add("bwd", "bwd:v4+rows", 131, 300, act=1, Y=True, in_place=True, regime="mixed")
    _add("bwd", "bwd:scalar+flat1", 131, 65, act=2, Y=False, in_place=True, regime="mixed")
    _add("bwd", "bwd:fused_last_block+rows", 131, 300, act=1, Y=True, in_place=True, knobs=((8, 1),), regime="mixed")
    _add("bwd", "bwd:fold", 131, 300, act=1, Y=False, in_place=True, knobs=((12, 1),), regime="mixed")
    for fam, lay in (("bwd_apply:rows", ""), ("bwd_apply:flat4", "mean@1"), ("bwd_apply:flat1", "X+1")):
        for a, y in ((0, False), (1, True), (1, False), (2, True), (2, False)):
            _add("bwd_apply", fam, 131, 300, lay, act=a, Y=y, regime="mixed" if a == 1 else "plain")
        _add("bwd_apply", fam, 131, 300, lay, act=1, Y=True, regime="constant")
        _add("bwd_apply", fam, 131, 300, lay, act=1, Y=True, in_place=True, regime="mixed")
        _add("bwd_apply", fam, 131, 300, lay, act=2, Y=False, affine=False)
    _add("bwd_apply", "bwd_apply:flat4", 37, 300, "S@1", act=1, Y=True)                 # a misaligned coef
    _add("bwd_apply", "bwd_apply:flat1", 4100, 257, act=1, Y=True)
    _add("bwd_apply", "bwd_apply:flat4", 4100, 1280, "mean@1", act=1, Y=False)
    _add("bwd_apply", "bwd_apply:rows", 32784, 4, act=1, Y=True)
    for ent, fams in (("bwd_sums", ("sums:v4", "sums:scalar")), ("bwd_coef", ("coef:v4", "coef:scalar", "coef:fused_last_block"))):
        for fam in fams:
            C, kn = (10 if "scalar" in fam else 300), (((8, 1),) if "fused" in fam else ())
            for a, y in ((0, False), (1, True), (1, False), (2, True), (2, False)):
                _add(ent, fam, 131, C, act=a, Y=y, knobs=kn)
            for reg in ("mixed", "constant"):
                _add(ent, fam, 131, C, act=1, Y=True, knobs=kn, regime=reg)
            _add(ent, fam, 4096 if "fused" in fam else 4097, C, act=1, Y=True, knobs=kn, regime="mixed")
    _add("bwd_sums", "sums:v4", 131, 300, act=1, Y=True, knobs=((8, 1),), regime="mixed")     # must not fuse: the divisor is 1
    _add("bwd_coef", "coef:v4", 4097, 300, act=1, Y=True, knobs=((8, 1),))                   # above the last-block limit
    for slots in (1, 63, 64, 65, 300):
        _add("coef_partials", "coef_partials", 777, 10, extra=slots)
    for on_out in (0, 1):
        for relu in (0, 1):
            for lay in ("", "X+4,dY+4,dX+4"):
                for M in (1, 37, 4097):
                    _add("bwd_dropout", "dropout:out" if on_out else "dropout:in", M, 12 if M > 37 else 300, lay, act=relu,
                         regime="mixed" if M == 37 else "plain", extra=(on_out, 0.25))
        _add("bwd_dropout", "dropout:out" if on_out else "dropout:in", 37, 300, act=1, regime="constant", extra=(on_out, 0.5))
    # ---- the one-launch backward (knob 13): its own test function
    for C in (4, 300):
        for M in (64, 65, 100, 4096):
            for a, y in ((1, True), (2, False)):
                _add("bwd", "bwd:node", M, C, act=a, Y=y, knobs=((13, 1),), regime="mixed")
    for a, y in ((0, False), (1, False), (2, True)):
        _add("bwd", "bwd:node", 100, 300, act=a, Y=y, knobs=((13, 1),))
    _add("bwd", "bwd:node", 100, 300, act=1, Y=True, knobs=((13, 1),), regime="constant")
    _add("bwd", "bwd:node", 100, 300, act=1, Y=True, knobs=((13, 1),), in_place=True, regime="mixed")
    _add("bwd", "bwd:node", 100, 300, act=1, Y=True, knobs=((13, 1),), affine=False)
    _add("bwd", "bwd:v4+rows", 63, 300, act=1, Y=True, knobs=((13, 1),))
    _add("bwd", "bwd:v4+rows", 4097, 4, act=1, Y=True, knobs=((13, 1),))


_table()
BY_NAME = {c.name: c for c in CASES}


def cases(entry=None, node=False):
    """the cases of an entry point; those that turn knob 13 on are listed only with node=True"""
    return [c for c in CASES if (entry is None or c.entry == entry) and (dict(c.knobs).get(13, 0) == 1) == node]


# ---- the SyncBN trio, single process: (name, C, rows per simulated rank) ---------------------------------------------------------------
SYNC_CASES = (("sync-w1", 300, (37,)), ("sync-w3", 300, (2, 37, 130)), ("sync-w3-narrow", 7, (64, 2, 33)))
SYNC_TINY_VAR = 1e-8                                     # column 1: variance far below eps; column 0: constant


def sync_rows(C, n_local, seed):
    x = regime_x(sum(n_local), C, "mixed", seed)
    g = torch.Generator().manual_seed(seed + 1)
    x[:, 0] = 0.75
    x[:, 1] = (1.0 + (SYNC_TINY_VAR ** 0.5) * torch.randn(sum(n_local), generator=g, dtype=torch.float64))
    return x.float().double()


# their refusals: (entry point, what is wrong) on a valid C = 12, world = 3 call
SYNC_REFUSALS = (("pack", "rank=world"), ("pack", "rank=-1"), ("pack", "n_local=0"), ("pack", "world=0"), ("pack", "C=0"), ("pack", "null:mean"),
                 ("pack", "null:invstd"), ("pack", "null:buf"),
                 ("finalize", "world=0"), ("finalize", "C=0"), ("finalize", "null:buf"), ("finalize", "null:mean"), ("finalize", "null:invstd"),
                 ("finalize", "scale_without_shift"), ("finalize", "shift_without_scale"),
                 ("coef", "C=0"), ("coef", "null:coef"), ("coef", "null:n_total"))

# the backward outputs that pass by the fp32-CPU-oracle rule instead of the 1e-5 bar (DESIGN.md names them with both errors); any
# other output that exceeds its bound fails
FP32_ORACLE_RULE = {"bwd-fused_last_block+rows-4096x1280-a1y-k8=1": ("dgamma", "dbeta")}


def launches_of(case):
    """kernel launches the call of a case makes (esc_prof_read counts them): what tells the reduction families apart"""
    fam = family_of(case.entry, case)
    if case.entry in ("apply", "affine") and case.M == 0:
        return 0
    if fam.startswith("stats:"):
        return 2
    if fam.startswith("bwd:"):
        return {"bwd:node": 1, "bwd:fold": 2, "bwd:fused_last_block+rows": 2}.get(fam, 3)
    if fam.startswith(("sums:", "coef:")):
        return 1 if fam.endswith("fused_last_block") else 2
    return 3 if fam.startswith("dropout:") else 1


# ---- the refusals: (name, entry, what is wrong) — the GPU test builds a valid call of the entry and breaks this one thing -----------------
REFUSALS = tuple((e, w) for e, ws in (
    ("stats", ("M=1", "ld<C", "scale_without_shift", "null:X", "null:mean", "null:S")),
    ("stats_partials", ("M=1", "scale_without_shift", "null:partials")),
    ("stats_partials_rows", ("M=1", "block_rows=0", "scale_without_shift", "null:partials")),
    ("affine_fold", ("M=1", "C%4", "ld<C", "ld%4", "base@1", "scale_without_shift", "null:partials", "relu=3", "relu=-1")),
    ("apply", ("ld<C", "null:mean", "relu=3", "relu=-1")),
    ("affine", ("ld<C", "null:scale", "relu=3")),
    ("bwd", ("M=0", "ld<C", "null:S", "null:dX", "relu=3", "relu=-1")),
    ("bwd_sums", ("M=0", "ld<C", "null:sums", "relu=3")),
    ("bwd_coef", ("M=0", "ld<C", "null:coef", "relu=3")),
    ("bwd_apply", ("M=0", "ld<C", "null:coef", "relu=3")),
    ("coef_partials", ("slots=0", "null:partial")),
    ("bwd_dropout", ("C%4", "base@1", "p=0", "p=1", "relu=2", "null:mask", "ld<C")),
    ("eval_coef", ("null:rm", "C=0")),
) for w in ws)

# the valid call each refusal starts from
REFUSAL_BASE = {"stats": "stats-v4-37x300-a0rf-mixed", "stats_partials": "stats_partials-32-33x10-a0rf",
                "stats_partials_rows": "stats_partials_rows-rows-209x12-a0rf-mixed-x64", "affine_fold": "affine_fold-fold-84x300-Y+4-a2-constant-x32",
                "apply": "apply-flat4-37x300-a1-mixed", "affine": "affine-rows-37x300-a1-mixed", "bwd": "bwd-v4+rows-131x12-a1y",
                "bwd_sums": "bwd_sums-v4-131x300-a1y", "bwd_coef": "bwd_coef-v4-131x300-a1y", "bwd_apply": "bwd_apply-rows-131x300-a1y-mixed",
                "coef_partials": "coef_partials-coef_partials-777x10-a0-x63", "bwd_dropout": "bwd_dropout-in-37x300-a1-mixed-x0_0.25",
                "eval_coef": "eval_coef-eval_coef-2x255-a0"}
