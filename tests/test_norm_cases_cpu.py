"""The BatchNorm case table (tests/norm_cases.py) checked without a GPU: it reaches every branch it names, its written-out
fp64 references are torch's batch_norm + autograd, its guards trip, and its error bounds are neither vacuous nor hiding
anything — a numpy fp32 replay of the shipped statistics algorithm stays under half of each bound on every data regime while
the naive E[x^2] - E[x]^2 variance breaks the invstd bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_cases as lc
import norm_cases as nc


def test_every_branch_is_reached_and_names_are_unique():
    names = [c.name for c in nc.CASES]
    assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)
    reached = {}
    for c in nc.CASES:
        assert nc.family_of(c.entry, c) == c.family, "%s: meant for %s, the predicates say %s" % (c.name, c.family, nc.family_of(c.entry, c))
        found = nc.branches_of(c)
        assert found <= nc.BRANCHES, (c.name, sorted(found - nc.BRANCHES))
        for b in found:
            reached.setdefault(b, []).append(c.name)
    for b in sorted(nc.BRANCHES):
        print("%-32s %3d  %s" % (b, len(reached.get(b, ())), ", ".join(reached.get(b, ())[:3])))
    assert not nc.BRANCHES - set(reached), "no case reaches %s" % sorted(nc.BRANCHES - set(reached))
    for name in nc.REFUSAL_BASE.values():
        assert name in nc.BY_NAME, name
    assert set(nc.REFUSAL_BASE) == {e for e, _ in nc.REFUSALS}


def test_every_family_sees_the_three_regimes_and_every_activation():
    seen, acts = {}, {}
    for c in nc.CASES:
        seen.setdefault(c.family, set()).add("constant" if c.regime == "ones" else c.regime)
        acts.setdefault(c.family, set()).add((c.act, c.has_Y))
    for fam in nc.STAT_FAMILIES + nc.BWD_FAMILIES:
        assert {"plain", "mixed", "constant"} <= seen[fam], (fam, seen[fam])
    for fam in nc.BWD_FAMILIES:
        want = {(0, False), (1, False)} if fam.startswith("dropout") else {(0, False), (1, True), (1, False), (2, True), (2, False)}
        assert want <= acts[fam], (fam, sorted(want - acts[fam]))
    # the knob-13 cases stay in a test function of their own, on the shapes that keep its barrier far inside residency
    for c in nc.cases("bwd", node=True):
        assert c.C in (4, 300) and (c.family != "bwd:node" or 64 <= c.M <= 4096), c.name
        assert nc.cdiv(c.C, 256) * nc.cdiv(c.M, 16) <= 512, c.name
    assert not [c.name for c in nc.cases() if dict(c.knobs).get(13)]


def test_no_case_is_large():
    """what the GPU run allocates per buffer, guards included: a matrix stays under 32 MiB; the scratch buffer is the promise plus
    a guard as large again, so its size is fixed by the widest column count of the table (42 MB at C = 1280)"""
    for c in nc.CASES:
        lay = nc.layout_of(c)
        matrix = max((max(c.M, 1) + 4) * lay[op][0] + 128 + 8 for op in nc.MATRICES) * 4
        scratch = (2 * nc.scratch_floats(c.C) + 64 + 8) * 4
        assert matrix <= 32 * 2 ** 20, (c.name, matrix)
        assert c.C <= 1280 and scratch <= 42.1e6, (c.name, scratch)


def test_every_relu_case_keeps_its_distance_from_the_kink():
    """every one: nc.Data asserts the margin itself (so the GPU run carries the condition too); here it is read back for each case"""
    n = 0
    for c in nc.CASES:
        if c.entry in nc.BACKWARD_ENTRIES and c.act == 1:
            d = nc.Data(c)
            assert float(d.pre.abs().min()) >= nc.RELU_MARGIN, (c.name, float(d.pre.abs().min()))
            if c.has_Y:                  # the forward output handed to the kernel agrees with the fp64 mask
                assert torch.equal(d.inputs["Y"] > 0, d.pre > 0), c.name
            const = nc.constant_columns(c.C, c.regime)
            if bool(const.any()):        # a nudge must not break a constant column
                assert float((d.inputs["X"][:, const] - d.inputs["X"][0, const]).abs().max()) == 0.0, c.name
            n += 1
    assert n == sum(1 for c in nc.CASES if c.entry in nc.BACKWARD_ENTRIES and c.act == 1) and n > 150, n


def test_the_oracle_rule_names_existing_cases():
    for name, outs in nc.FP32_ORACLE_RULE.items():
        assert nc.BY_NAME[name].entry in nc.BACKWARD_ENTRIES and set(outs) <= {"dX", "dgamma", "dbeta", "coef", "sums"}
    for c in nc.CASES:
        assert 0 <= nc.launches_of(c) <= 3


# ---- the references against torch ----------------------------------------------------------------------------------------------------------
def _torch_forward(x, gamma, beta, act, rm=None, rv=None):
    y = F.batch_norm(x, rm, rv, gamma, beta, training=True, momentum=nc.MOMENTUM, eps=nc.EPS)
    return F.relu(y) if act == 1 else (F.elu(y) if act == 2 else y)


@pytest.mark.parametrize("regime", nc.REGIMES)
@pytest.mark.parametrize("act", (0, 1, 2))
def test_references_are_torch_batch_norm_and_autograd(regime, act):
    M, C = 37, 12
    x = nc.regime_x(M, C, regime, 5)
    gamma, beta = nc.gamma_beta(C)
    mean, var, invstd, unbiased = nc.ref_stats(x)
    if act == 1:
        x = nc.nudge_relu(x, mean, invstd, gamma, beta, 5)
        mean, var, invstd, unbiased = nc.ref_stats(x)
    rm0, rv0 = nc.uniform((C,), 1, 2.0), nc.uniform((C,), 2, 0.5) + 1.0
    rm, rv = rm0.clone(), rv0.clone()
    xt, gt, bt = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = _torch_forward(xt, gt, bt, act, rm, rv)
    dy = nc.uniform((M, C), 3)
    y.backward(dy)
    rel = lambda a, b: float((a - b).abs().max() / max(1.0, float(b.abs().max())))
    assert rel(nc.ref_forward(x, mean, invstd, gamma, beta, act), y.detach()) <= 1e-12
    want_rm, want_rv = nc.ref_running(rm0, rv0, mean, unbiased)
    assert rel(want_rm, rm) <= 1e-12 and rel(want_rv, rv) <= 1e-12
    got = nc.ref_backward(x, dy, mean, invstd, gamma, beta, act)
    # the zero-variance columns amplify fp64 rounding by invstd^2 = 1e5 in autograd's own chain; 1e-12 still holds of the scale
    assert rel(got["dX"], xt.grad) <= 1e-12, rel(got["dX"], xt.grad)
    assert rel(got["dgamma"], gt.grad) <= 1e-12 and rel(got["dbeta"], bt.grad) <= 1e-12
    assert rel(got["coef"] * M, got["sums"]) <= 1e-15
    # the dropout variants: explicit masks around the same composition
    p = 0.25
    keep = (torch.rand(M, C, generator=torch.Generator().manual_seed(9)) >= p).double()
    if act != 2:
        xt = x.clone().requires_grad_()
        (_torch_forward(xt, gamma, beta, act) * keep / (1 - p)).backward(dy)                 # dropout behind the activation
        assert rel(nc.ref_backward(x, dy, mean, invstd, gamma, beta, act, keep_in=keep, p=p)["dX"], xt.grad) <= 1e-12
        raw = x.clone().requires_grad_()                                                     # x itself was dropout(raw)
        xin = raw * keep / (1 - p)
        m2, _, is2, _ = nc.ref_stats(xin.detach())
        _torch_forward(xin, gamma, beta, act).backward(dy)
        if act == 0 or float((gamma * ((xin.detach() - m2) * is2) + beta).abs().min()) > 1e-9:
            assert rel(nc.ref_backward(xin.detach(), dy, m2, is2, gamma, beta, act, keep_out=keep, p=p)["dX"], raw.grad) <= 1e-12


# ---- the guards ------------------------------------------------------------------------------------------------------------------------------
def test_a_wrong_kernel_trips_the_guards():
    M, C, ld = 5, 6, 8
    x = lc.operand(M, C, ld, 1, seed=1)
    y = lc.output(M, C, ld, 0)
    X, Y = x.dev.numpy(), y.dev.numpy()                        # the "device" is the CPU here: numpy views of the same memory

    def kernel(width, rows):
        for r in range(rows):
            Y[y.base + r * ld:y.base + r * ld + width] = 2 * X[x.base + r * ld:x.base + r * ld + width]
    kernel(C, M)
    assert y.outside_changed() == 0 and not bool(torch.isnan(y.result()).any()) and x.untouched()
    kernel(C + 1, M)                                           # one column too many: reads padding (NaN), writes padding (sentinel)
    assert y.outside_changed() == M
    kernel(C, M + 1)                                           # one row too many
    assert y.outside_changed() > M
    y2 = lc.output(M, C, ld, 0)
    Y2 = y2.dev.numpy()
    for r in range(M):                                         # reads the padding column into a live element
        Y2[y2.base + r * ld:y2.base + r * ld + C] = X[x.base + r * ld + 1:x.base + r * ld + C + 1]
    assert y2.outside_changed() == 0 and bool(torch.isnan(y2.result()).any())
    s = lc.Buf(1, 16, 16, 0, torch.full((1, 16), float("nan")), lc.sentinel(), 0, 16, "cpu")
    s.dev.numpy()[16] = 0.0                                    # one float past the promised scratch
    assert s.outside_changed() == 1
    m = lc.ByteBuf(torch.ones(3, 8, dtype=torch.uint8), 32, "cpu")
    assert m.untouched() and m.ptr() % 16 == 0
    m.dev.numpy()[m.base + 24] = 1                             # one byte behind the mask
    assert not m.untouched()


# ---- the bounds: a replay of the shipped algorithm in numpy fp32 ---------------------------------------------------------------------------------
def replay_stats(x, gamma, beta):
    """bn_partial_kernel + bn_finalize_kernel: every slot sums around its first row in fp32, its (mean, M2) is stored as
    float, the slots are Chan-merged in fp64, mean / invstd are stored as float; then both output forms"""
    f32 = np.float32
    M, C = x.shape
    P = min(nc.cdiv(M, 16), 64) * 4
    n, mu, m2 = 0.0, np.zeros(C), np.zeros(C)
    for p in range(min(P, M)):
        rows = x[p::P].astype(f32)
        d = (rows - rows[0]).astype(f32)
        s1 = np.add.accumulate(d, axis=0, dtype=f32)[-1]
        s2 = np.add.accumulate((d * d).astype(f32), axis=0, dtype=f32)[-1]
        k = rows.shape[0]
        m = s1.astype(np.float64) / k
        pm = (rows[0].astype(np.float64) + m).astype(f32).astype(np.float64)
        pm2 = np.maximum(s2.astype(np.float64) - s1.astype(np.float64) * m, 0.0).astype(f32).astype(np.float64)
        tot = n + k
        delta = pm - mu
        mu = mu + delta * k / tot
        m2 = m2 + pm2 + delta * delta * n * k / tot
        n = tot
    mean = mu.astype(f32)
    invstd = (1.0 / np.sqrt(m2 / M + nc.EPS)).astype(f32)
    g, b, xf = gamma.astype(f32), beta.astype(f32), x.astype(f32)
    y_apply = ((xf - mean) * invstd).astype(f32) * g + b                     # bn_apply_kernel
    scale = (g * invstd).astype(f32)
    shift = (b - (mean * scale).astype(f32)).astype(f32)
    y_affine = (xf * scale).astype(f32) + shift                                # affine_act_rows (without the fused rounding of fmaf)
    return dict(mean=mean, invstd=invstd, rv=m2 / (M - 1), scale=scale, shift=shift, y_apply=y_apply.astype(f32), y_affine=y_affine.astype(f32))


@pytest.mark.parametrize("M", (37, 1025, 4097))
@pytest.mark.parametrize("regime", nc.REGIMES)
def test_the_replayed_algorithm_uses_at_most_half_of_each_bound(M, regime):
    C = 12
    x = nc.regime_x(M, C, regime, 11)
    gamma, beta = nc.gamma_beta(C)
    mean, var, invstd, unbiased = nc.ref_stats(x)
    got = {k: torch.from_numpy(np.asarray(v, dtype=np.float64)) for k, v in replay_stats(x.numpy(), gamma.numpy(), beta.numpy()).items()}
    y = nc.ref_forward(x, mean, invstd, gamma, beta, 0)
    by = nc.bound_y(y, x, mean, invstd, gamma)
    ratios = {
        "mean": (got["mean"] - mean).abs() / nc.bound_mean(mean),
        "invstd": (got["invstd"] - invstd).abs() / nc.bound_invstd(mean, invstd),
        "running_var": (got["rv"] - unbiased).abs() / (2 * nc.rel_invstd(mean, invstd) * (unbiased + nc.EPS)),
        "scale": (got["scale"] - gamma * invstd).abs() / nc.bound_scale(mean, invstd, gamma),
        "shift": (got["shift"] - (beta - mean * gamma * invstd)).abs() / nc.bound_shift(mean, invstd, gamma, beta),
        "Y (apply form)": nc.colmax(got["y_apply"] - y) / by,
        "Y (affine form)": nc.colmax(got["y_affine"] - y) / by,
    }
    for k, r in ratios.items():
        print("M=%d %-8s %-16s worst error / bound %.3g" % (M, regime, k, float(r.max())))
        assert float(r.max()) <= 0.5, (k, float(r.max()), int(r.argmax()))
    const = nc.constant_columns(C, regime)
    assert torch.equal(got["mean"][const], x[0][const])               # the mean of a constant column is the constant, exactly


@pytest.mark.parametrize("M", (37, 1025, 4097))
def test_the_naive_variance_breaks_the_invstd_bound_on_offset_columns(M):
    x = nc.regime_x(M, 12, "offset", 11)
    mean, var, invstd, _ = nc.ref_stats(x)
    xf = x.numpy().astype(np.float32)
    e1 = np.add.accumulate(xf, axis=0, dtype=np.float32)[-1] / np.float32(M)
    e2 = np.add.accumulate(xf * xf, axis=0, dtype=np.float32)[-1] / np.float32(M)
    naive = 1.0 / np.sqrt(np.maximum((e2 - e1 * e1).astype(np.float64), 0.0) + nc.EPS)
    ratio = (torch.from_numpy(naive) - invstd).abs() / nc.bound_invstd(mean, invstd)
    print("M=%d naive invstd error / bound per column: %s" % (M, ["%.3g" % r for r in ratio.tolist()]))
    big = nc.column_kinds(12, "offset") == 2                           # |mean| / sigma = 1e3
    assert float(ratio[big].min()) > 1.0, ratio
