"""The case table of the loss heads and the optimiser (tests/loss_cases.py) checked without a GPU: every size, regime and flag
it promises occurs, its written-out fp64 formulas are torch's (functional losses + autograd, torch.optim.Adam in fp64, the
changing learning rate and a resumed state included), and its bounds are neither vacuous nor hiding anything — two numpy fp32
replays of adam_kernel's statements (uncontracted and FMA-contracted) stay under half of each bound while each of five
deliberate mistakes in the update, and three in the losses, breaks a bound on a case the table names."""
import numpy as np
import pytest
import torch

import loss_cases as lc


def test_names_are_unique_and_everything_promised_occurs():
    for table in (lc.LOSS_CASES, lc.ADAM_CASES):
        names = [c.name for c in table]
        assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)
    for entry, regimes in (("l1", lc.L1_REGIMES), ("mse", lc.L1_REGIMES), ("bce", lc.BCE_REGIMES)):
        cs = lc.loss_cases(entry)
        assert {c.G * c.T for c in cs} >= set(lc.LOSS_SIZES), entry
        assert {c.regime for c in cs} == set(regimes), entry
        assert {None, 1} <= {c.denom for c in cs} and any(c.denom and c.denom > c.G * c.T for c in cs), entry
        assert {c.want_dpred for c in cs} == {True, False} and {c.upstream for c in cs} == {1.0, 3.0}, entry
        assert {c.grad_scale for c in cs} == ({1.0} if entry == "bce" else {1.0, 0.25}), entry
        assert all(c.T == 1 for c in cs) or entry == "bce"
        for c in cs:                                    # a NULL dpred is compared with the same case with it: that case exists
            if not c.want_dpred:
                assert c.upstream == 1.0 and c.grad_scale == 1.0, c.name
    bce = lc.loss_cases("bce")
    assert {(g, 1) for g in (1, 2, 63, 64, 1023, 2049)} <= {(c.G, c.T) for c in bce}                 # G x 1
    assert any(c.G * c.T == lc.MULTIPASS and c.G * c.T > 37 * lc.WORKGROUP for c in bce)
    assert any(c.regime == "none_labelled" and c.denom for c in bce) and any(c.regime == "none_labelled" and not c.denom for c in bce)
    ad = lc.ADAM_CASES
    assert {c.n for c in ad} >= set(lc.ADAM_SIZES) and lc.ADAM_SIZES[-3:] == (524288, 524289, 2 * 524288 + 3)
    assert {c.regime for c in ad} == set(lc.ADAM_REGIMES)
    assert {c.step0 for c in ad} == {0, 20000} and {c.layout for c in ad} == {"one", "padded", "late"}
    assert {(c.betas, c.eps) for c in ad} == {(lc.DEFAULT_BETAS, lc.DEFAULT_EPS), (lc.OTHER_BETAS, lc.OTHER_EPS)}
    assert any(len(set(c.lrs)) > 1 for c in ad) and {c.grad_denom for c in ad} == {None, lc.GRAD_DENOM}
    long_ = [c for c in ad if c.steps > 5]
    assert len(long_) == 1 and long_[0].steps == 20 and long_[0].n <= 4096
    assert any(c.grad_denom and c.n == 2 * lc.ADAM_CAP + 3 for c in ad)
    for c in ad:
        assert len(c.lrs) == c.steps
        if c.layout == "late":                          # every late= case has its twin without
            twin = c.name[:-len("late")] + "padded"
            assert twin in lc.ADAM_BY_NAME and lc.ADAM_BY_NAME[twin]._replace(name=c.name, layout="late") == c
            assert lc.flat_layout(c)[0] != lc.flat_layout(lc.ADAM_BY_NAME[twin])[0]
        if c.layout != "one":
            sizes = lc.tensor_sizes(c)
            assert sum(sizes) == c.n and sizes.count(1) == 2 and min(sizes) >= 1, (c.name, sizes)
            idx = lc.flat_index(c)
            assert len(set(idx.tolist())) == c.n and idx.max() < lc.flat_layout(c)[2] and lc.flat_layout(c)[2] > c.n


def test_no_buffer_is_large():
    for c in lc.LOSS_CASES:
        assert (2 * c.G * c.T + 256) * 4 <= lc.MAX_BUFFER_BYTES, c.name        # the widest: the matrix `slice` is cut from
    for c in lc.ADAM_CASES:
        assert (lc.flat_layout(c)[2] + 256) * 4 <= lc.MAX_BUFFER_BYTES, c.name
    assert max(lc.flat_layout(c)[2] for c in lc.ADAM_CASES) * 4 <= 4.01 * 2 ** 20


def test_the_regimes_are_what_they_say():
    for c in lc.LOSS_CASES:
        pred, y = lc.loss_data(c)
        M = c.G * c.T
        assert pred.shape == y.shape == (c.G, c.T) and pred.dtype == y.dtype == torch.float32
        assert bool(torch.isfinite(pred).all())
        again = lc.loss_data(c)
        assert torch.equal(pred, again[0]) and torch.equal(y.view(torch.int32), again[1].view(torch.int32))
        lab = lc.labelled(y)
        if c.regime == "ties":
            tie = pred == y
            assert int(tie.sum()) >= (M + 2) // 3 and (M < 16 or bool((pred[tie] == 0).any())), c.name
            if M >= 16:                                 # both orders of a signed-zero tie
                z = (pred == 0) & (y == 0)
                assert bool((torch.signbit(pred[z]) != torch.signbit(y[z])).any()), c.name
        if c.regime == "offset":
            assert float(y.abs().min()) >= 1e3 and float((pred - y).abs().max()) < 10
        if c.regime == "one_sided":
            assert bool((pred > y).all())
        if c.entry == "bce":
            n = int(lab.sum())
            want = {"all_labelled": M, "none_labelled": 0, "one_labelled": 1, "soft": M}.get(c.regime)
            assert want is None or n == want, (c.name, n)
            if c.regime in ("plain", "saturated") and M >= 64:
                assert 0.15 * M < M - n < 0.45 * M, (c.name, n)
            if c.regime == "saturated":
                v = set(pred.abs().reshape(-1).tolist())
                assert ({20.0, 100.0, 1e4} <= v) if M >= 12 else (1e4 in v), c.name
                assert float(pred.reshape(-1)[0]) == -1e4 and float(y.reshape(-1)[0]) == 0.0
                assert M < 12 or (float(pred.reshape(-1)[-1]) == 1e4 and float(y.reshape(-1)[-1]) == 1.0)
            if c.regime == "soft":
                assert 0 < float(y.min()) and float(y.max()) < 1
    for c in lc.ADAM_CASES:
        d = lc.adam_data(c)
        g = np.stack(d.grads)
        assert g.dtype == np.float32 and g.shape == (c.steps, c.n) and bool(np.isfinite(g).all())
        if c.regime == "all_zero":
            assert not g.any()
        if c.regime == "sparse" and c.n >= 256:
            assert 0.04 < (np.abs(g).max(0) > 0).mean() < 0.2, c.name
        if c.regime == "flip":
            assert bool((np.sign(g[1:]) == -np.sign(g[:-1])).all())
        if c.regime == "mixed" and c.n >= 256:
            mag = np.abs(g).max(0) / (c.grad_denom or 1.0)
            assert mag.min() < 1e-4 and mag.max() > 1e2, c.name
        if c.regime in ("large", "tiny"):
            assert (np.abs(g).max() / (c.grad_denom or 1.0) > 1e3) == (c.regime == "large")
        assert bool(d.m0.any()) == bool(d.v0.any()) == bool(c.step0 and c.regime != "all_zero")


def test_written_out_losses_are_torch_in_fp64():
    """values to 1e-12 of their scale; bce on the labelled entries, reduction='sum' / the case's divisor.  Without a label
    torch's own mean is NaN: the table pins 0."""
    for c in lc.LOSS_CASES:
        pred, y = lc.loss_data(c)
        loss, grad = lc.loss_ref64(c, pred, y)
        tl, tg = lc.loss_torch(c, pred, y, torch.float64)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all()), c.name
        assert abs(float(loss - tl)) <= 1e-12 * max(1.0, abs(float(tl))), (c.name, float(loss), float(tl))
        assert float((grad - tg).abs().max()) <= 1e-12 * max(float(tg.abs().max()), 1e-300), c.name
        if c.entry == "bce":
            assert bool((grad[~lc.labelled(y).reshape(-1)] == 0).all()), c.name
        if c.regime == "none_labelled":
            assert float(loss) == 0.0 and not bool(grad.any())
            if not c.denom:
                x = pred.double().reshape(-1)[:0]
                assert bool(torch.isnan(torch.nn.functional.binary_cross_entropy_with_logits(x, x)))
        if c.regime == "ties" and c.entry == "l1":
            assert bool((grad[(pred == y).reshape(-1)] == 0).all()), c.name
        if c.regime == "saturated" and c.upstream == 1.0:
            assert float(grad[0]) == 0.0 and (c.G * c.T < 12 or float(grad[-1]) == 0.0), c.name


def test_loss_mistakes_break_the_criterion():
    """the criterion of the GPU test is not vacuous: each mistake, made in fp64, fails it on a case of the table"""
    wanted = {"divide_by_M": [], "count_nan": [], "tie_sign": []}
    for c in lc.LOSS_CASES:
        pred, y = lc.loss_data(c)
        loss, grad = lc.loss_ref64(c, pred, y)
        l32, g32 = lc.loss_torch(c, pred, y, torch.float32)
        fl, fg = lc.loss_floors(c, pred, y, loss, grad)
        assert not lc.breaks(loss, l32, loss, fl) and not lc.breaks(grad, g32, grad, fg)
        for mistake in wanted:
            ml, mg = lc.loss_ref64(c, pred, y, mistake=mistake)
            if lc.breaks(ml, l32, loss, fl) or lc.breaks(mg, g32, grad, fg):
                wanted[mistake].append(c.name)
    for mistake, caught in sorted(wanted.items()):
        print("%-12s caught by %3d cases: %s" % (mistake, len(caught), ", ".join(caught[:4])))
    assert all(wanted.values()), wanted
    for e in ("l1", "mse", "bce"):                      # every entry with a `denom` argument has a case that holds it to it
        assert any(n.startswith(e) for n in wanted["divide_by_M"]), e
    assert all(n.startswith("bce") for n in wanted["count_nan"]) and all(n.startswith("l1") for n in wanted["tie_sign"])


SMALL = [c for c in lc.ADAM_CASES if c.n <= 4096]


def test_written_out_adam_is_torch_in_fp64():
    sets = set()
    for c in SMALL:
        d = lc.adam_data(c)
        for mine, theirs, what in zip(lc.adam_ref64(c, d, bounds=False), lc.adam_torch64(c, d), ("p", "exp_avg", "exp_avg_sq")):
            scale = max(float(np.abs(theirs).max()), 1e-300)
            assert float(np.abs(mine - theirs).max()) <= 1e-12 * scale, (c.name, what)
        sets.add((c.betas, c.eps, len(set(c.lrs)) > 1, c.step0))
    assert {(s[0], s[1]) for s in sets} == {(lc.DEFAULT_BETAS, lc.DEFAULT_EPS), (lc.OTHER_BETAS, lc.OTHER_EPS)}
    assert any(s[2] for s in sets) and any(s[3] for s in sets) and any(s[2] and s[3] for s in sets)


def test_fp32_replays_stay_under_half_of_each_bound():
    """per case: the worst |error| / bound over the elements, for p, exp_avg and exp_avg_sq, of the uncontracted replay, the
    fused replay and torch's fp32 Adam; next to it the bound itself in units of u = 2^-24 (its largest element)"""
    print("%-44s %-4s %10s %8s %8s %8s" % ("case", "", "bound / u", "plain", "fused", "torch"))
    for c in SMALL:
        d = lc.adam_data(c)
        p, m, v, Bp, Bm, Bv = lc.adam_ref64(c, d)
        runs = [lc.adam_replay32(c, d, False), lc.adam_replay32(c, d, True), lc.adam_torch32(c, d)]
        for i, (ref, bound, what) in enumerate(((p, Bp, "p"), (m, Bm, "m"), (v, Bv, "v"))):
            ratios = [lc.worst_ratio(r[i], ref, bound)[0] for r in runs]
            print("%-44s %-4s %10.3g %8.3f %8.3f %8.3f" % (c.name, what, float(bound.max()) / lc.U, ratios[0], ratios[1], ratios[2]))
            assert ratios[0] <= 0.5 and ratios[1] <= 0.5, (c.name, what, ratios)
            assert ratios[2] <= 1.0, (c.name, what, ratios)
        if c.regime == "all_zero":
            for r in runs[:2]:
                assert np.array_equal(r[0].view(np.int32), d.p0.view(np.int32)) and not r[1].any() and not r[2].any()


def test_adam_mistakes_break_a_bound():
    """each deliberate mistake, made in the fp64 formulas, leaves at least one of the three bounds on at least one case"""
    caught = {k: [] for k in lc.MISTAKES}
    for c in SMALL:
        d = lc.adam_data(c)
        p, m, v, Bp, Bm, Bv = lc.adam_ref64(c, d)
        for mistake in lc.MISTAKES:
            wrong = lc.adam_ref64(c, d, mistake=mistake, bounds=False)
            broken = [what for got, ref, bound, what in zip(wrong, (p, m, v), (Bp, Bm, Bv), ("p", "m", "v"))
                      if lc.worst_ratio(got, ref, bound)[0] > 1.0]
            if broken:
                caught[mistake].append("%s (%s)" % (c.name, ",".join(broken)))
    for mistake in lc.MISTAKES:
        print("%-28s caught by %3d cases: %s" % (mistake, len(caught[mistake]), "; ".join(caught[mistake][:3])))
    assert all(caught.values()), {k: len(v) for k, v in caught.items()}
    # eps inside the root passes a check of p on ordinary gradients; the tiny and mixed regimes are what catches it
    eps_cases = {n.split(" ")[0] for n in caught["eps_inside_sqrt"]}
    assert any(lc.ADAM_BY_NAME[n].regime in ("tiny", "mixed") for n in eps_cases)
    assert all(lc.ADAM_BY_NAME[n.split(" ")[0]].grad_denom for n in caught["denom_after_square"])


def test_guarded_buffers_trip():
    """the guards the GPU run relies on (tests/linear_cases.py) notice a write one float before and one behind a vector"""
    import linear_cases as lin
    for where in (-1, 7):
        b = lin.Buf(1, 7, 7, 0, torch.zeros(1, 7), lin.sentinel(), 64, 64, "cpu")
        assert b.outside_changed() == 0
        b.dev[b.base + where] = 1.0
        assert b.outside_changed() == 1
