"""The case table of the Linear backward with the BatchNorm backward folded in (tests/bnb_cases.py), checked without a GPU:
every named branch is reached, family_of agrees with plan::plan_both_bn (tests/bnb_plan_host.cpp: csrc/linear_plan.h compiled with
the host compiler under AddressSanitizer and UBSan), the ReLU cases keep their margin from the kink, the fp64 reference differentiates
what it says it does (torch autograd), an fp32 replay of the kernels' formulas holds every bound — and the replay of the ELU
derivative at the forward's fused pre-activation fmaf(x, scale, shift), the form the kernels had, breaks the dX and the
summed-partials bars on ill-conditioned columns while the centred form stays under half of them: the table discriminates."""
import os
import subprocess

import pytest
import torch

import bnb_cases as bc
import linear_cases as lc
import norm_cases as nc
from test_linear_plan_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "esc-gnn_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bnb_plan") / "bnb_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "bnb_plan_host.cpp"), "-o", exe], check=True)
    return exe


def describe(case, request=0):
    lay = bc.layout_of(case)
    head = [case.M, case.N, case.K, int(case.bn), int(case.next), case.bn_act, case.next_act, int(not case.dx), int(case.beta[0]), int(case.beta[1]),
            request]
    mats = [v for op in ("dOut", "bx", "X", "W", "dX", "nx") for v in lay[op]]
    vecs = [lay[v][1] for v in bc.BN_VECTORS + bc.NEXT_VECTORS + ("slabs",)]
    return " ".join(str(v) for v in head + mats + vecs) + "\n"


def ask(exe, cases, request=0):
    out = subprocess.run([exe], input="".join(describe(c, request) for c in cases), stdout=subprocess.PIPE, universal_newlines=True,
                         check=True).stdout.split("\n")
    out = [o.split() for o in out if o]
    assert len(out) == len(cases)
    return [(o[0],) + tuple(int(v) for v in o[1:]) for o in out]


def test_the_transcription_agrees_with_the_plan_header(program):
    """family, tile, slot height, slabs and launches of every record, served or refused"""
    for case, a in zip(bc.CASES, ask(program, bc.CASES)):
        fam = bc.family_of(case)
        assert a[0] == fam == case.family, (case.name, a[0], fam, case.family)
        if fam == "none":
            continue
        sp, per = bc.splits_of(case)
        promised = bc.scratch_promised(case)
        assert a[1:] == ({"small_bn": 0, "dma64_bn": 64, "dma128_bn": 128}[fam], bc.block_rows(case), sp, per, sp * (case.N * case.K + case.N),
                         promised, 1), (case.name, a)
        assert a[5] <= promised, case.name
    tiles = [c for c in bc.served() if c.family != "small_bn"]
    for case, a in zip(tiles, ask(program, tiles, request=1)):           # knob 14: the same plan as two launches
        assert a[0] == case.family and a[7] == 2, (case.name, a)


def test_every_named_branch_is_reached_by_a_case():
    reached, by = set(), {}
    for c in bc.CASES:
        for b in bc.branches_of(c):
            reached.add(b)
            by.setdefault(b, c.name)
    missing = sorted(bc.BRANCHES - reached)
    assert not missing, "no case reaches: %s" % ", ".join(missing)
    # the three families, each on plain and mixed data under each activation code; every demoting edit refuses on the tiles
    for c in bc.refused():
        assert bc.branches_of(c), "%s is refused for no named reason" % c.name
    for name in bc.CHAINED + bc.DEFERRED + bc.TWO_LAUNCHES + bc.ELU_ILL_CONDITIONED:
        assert bc.BY_NAME[name].family != "none"
    for fam in bc.FAMILIES:
        ill = [bc.BY_NAME[n] for n in bc.ELU_ILL_CONDITIONED if bc.BY_NAME[n].family == fam]
        assert any(c.bn and c.bn_act == 2 for c in ill), fam
        assert fam == "small_bn" or any(c.next and c.next_act == 2 for c in ill), fam


def test_relu_cases_keep_their_margin_and_the_reference_is_the_derivative():
    """the condition every ReLU case carries (bn side and next side), and on the small shapes: the fp64 dY the reference multiplies
    into the GEMMs is torch autograd's gradient of act(BatchNorm(x)) once coef is the exact pair of means"""
    for c in bc.served():
        d = bc.data_of(c)
        assert d.relu_margin() >= nc.RELU_MARGIN, (c.name, d.relu_margin())
        if not c.bn or c.M > 300 or c.regime not in ("plain",):
            continue
        i = d.inputs
        x = i["bx"].clone().requires_grad_(True)
        xh = (x - i["mean"]) * i["invstd"]
        y = nc.act(i["gamma"] * xh + i["beta"], c.bn_act)
        g = i["dOut"] * nc.act_grad((i["gamma"] * xh + i["beta"]).detach(), c.bn_act)
        # the straight-through part: d/dx of act(gamma xhat + beta) with mean / invstd held fixed is scale * g
        (y * i["dOut"]).sum().backward()
        assert float((x.grad - i["gamma"] * i["invstd"] * g).abs().max()) <= 1e-12 * max(1.0, float(x.grad.abs().max())), c.name
        k = torch.stack((g.sum(0), (g * xh.detach()).sum(0)), 1) / c.M
        assert float((k.float().double() - i["coef"]).abs().max()) == 0.0, c.name


def test_an_fp32_replay_of_the_centred_formulas_holds_every_bound():
    """torch fp32 on the CPU, one rounding per operation, no library: every output of every served case inside its bound — so a kernel
    outside it is wrong and not merely fp32.  Prints the outputs listed under the fp32-oracle rule (none are needed on the CPU)."""
    print("fp32-oracle rule: %s" % (bc.FP32_ORACLE_RULE or "no case needs it"))
    worst = {}
    for c in bc.served():
        d = bc.data_of(c)
        for n, e in d.excess(d.replay_fp32("centred")).items():
            worst[n] = max(worst.get(n, (0.0, "")), (e, c.name))
            assert e <= 1.0 or n in bc.FP32_ORACLE_RULE.get(c.name, ()), "%s %s: fp32 replay at %.3g of its bound" % (c.name, n, e)
    for n, (e, name) in sorted(worst.items()):
        print("replay worst %-8s %.3g of its bound (%s)" % (n, e, name))
    for name in bc.FP32_ORACLE_RULE:
        assert bc.BY_NAME[name].family != "none"


def _probe(kinds, seed):
    """130 x 64 x 36, bn + next, ELU on both sides, columns of the given norm_cases kinds interleaved"""
    regime = {(2,): "offset1000", (3,): "tiny", (2, 3): "both"}[kinds]
    case = bc.Case("probe-%s-%d" % (regime, seed), 130, 64, 36, "", True, True, 2, 2, False, 0, True, "mixed", "mixed", (True, True), "dma64_bn")
    keep = nc.column_kinds
    try:
        nc.column_kinds = lambda C, reg: torch.tensor(kinds)[torch.arange(C) % len(kinds)]
        return bc.Data(case)
    finally:
        nc.column_kinds = keep


def test_the_table_discriminates_the_fused_elu_pre_activation():
    """offset-1000 (|mean| / sigma = 1e3) and sigma = 1e-3 ELU columns, four seeds: the centred form stays under half of the dX, dW and
    summed-partials bars; the fused form fmaf(x, scale, shift) exceeds the dX bar and the summed-partials bar"""
    for kinds in ((2,), (3,), (2, 3)):
        worst_c, worst_f = {}, {}
        for seed in range(4):
            d = _probe(kinds, seed)
            for worst, form in ((worst_c, "centred"), (worst_f, "fused")):
                for n, e in d.excess(d.replay_fp32(form)).items():
                    worst[n] = max(worst.get(n, 0.0), e)
        print("kinds %s: centred %s" % (kinds, {n: "%.3g" % e for n, e in worst_c.items()}))
        print("kinds %s: fused   %s" % (kinds, {n: "%.3g" % e for n, e in worst_f.items()}))
        for n in ("dX", "dW", "sums", "partial"):
            assert worst_c[n] < 0.5, (kinds, n, worst_c[n])
        assert worst_f["dX"] > 1.0 and worst_f["sums"] > 1.0, (kinds, worst_f)
        assert worst_f["dX"] > 10 * worst_c["dX"] and worst_f["sums"] > 10 * worst_c["sums"], (kinds, worst_f, worst_c)


def test_the_promised_scratch_covers_every_plan():
    for c in bc.served():
        sp, _ = bc.splits_of(c)
        assert sp * (c.N * c.K + c.N) <= bc.scratch_promised(c), c.name
        assert bc.launches_of(c) in (2, 3) and bc.launches_of(c, deferred=True) == bc.launches_of(c) - 1
    assert lc.PRO_MAX_K == bc.PRO_MAX_K and lc.SMALLN_DX_MAX_N == bc.SMALLN_DX_MAX_N
