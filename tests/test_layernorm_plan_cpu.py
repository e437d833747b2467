"""The work-split rule of the per-graph LayerNorm (esc-gnn_amd/csrc/layernorm_plan.h, host-only C++) against its transcription
below: tests/layernorm_plan_host.cpp is compiled once with the host compiler under AddressSanitizer and UBSan and asked for the
workgroup size, the row and column lanes and the grids of the forward and the backward at every width at which the rule flips.
Runs no library code and needs no GPU."""
import os
import subprocess

import pytest

from test_linear_plan_cpu import CSRC, HERE, _host_compiler

FLIP_WIDTHS = (4, 64, 68, 128, 132)
WIDTHS = FLIP_WIDTHS + (12, 256, 300, 1020, 1024)
GRAPHS = (0, 1, 7, 32, 130, 256)
CHAINS, MAX_C = 64, 1024


def block_threads(C):
    """256 threads up to C = 64, 512 up to 128, 1024 beyond"""
    return 256 if C <= 64 else 512 if C <= 128 else 1024


def expected(G, C, backward, affine):
    block, lanes = block_threads(C), C // 4
    two = bool(backward and affine)
    return (block, lanes, block // lanes, 2 if two else 1, G, 2 * lanes if two else 0, CHAINS, MAX_C)


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("layernorm_plan") / "layernorm_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "layernorm_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, calls):
    text = "".join("%d %d %d %d\n" % c for c in calls)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [tuple(int(v) for v in o.split()) for o in out if o]
    assert len(out) == len(calls)
    return out


def test_block_size_at_the_widths_where_the_rule_flips(plan_program):
    got = _ask(plan_program, [(32, C, 0, 1) for C in FLIP_WIDTHS])
    assert [g[0] for g in got] == [256, 256, 512, 512, 1024] == [block_threads(C) for C in FLIP_WIDTHS]
    assert [g[2] for g in got] == [256, 16, 30, 16, 31]


def test_plans_against_the_transcription(plan_program):
    calls = [(G, C, b, a) for G in GRAPHS for C in WIDTHS for b in (0, 1) for a in (0, 1)]
    for call, got in zip(calls, _ask(plan_program, calls)):
        G, C, b, a = call
        assert got == expected(G, C, b, a), (call, got)
        block, lanes, rows, launches, g0, g1 = got[:6]
        assert block % 64 == 0 and lanes * 4 == C                               # whole waves; the column lanes cover a row exactly
        assert rows >= 1 and rows * lanes <= block < (rows + 1) * lanes         # as many row lanes as fit; fewer than `lanes` threads idle
        assert g0 == G                                                          # one workgroup per graph, whatever the batch
        assert launches == 1 + (g1 > 0) and (g1 > 0) == bool(b and a)           # the second launch: the affine's gradient alone
        assert g1 in (0, 2 * lanes)                                             # ... one wave per float4 of d_weight | d_bias


def test_the_cut_does_not_see_the_batch(plan_program):
    """block, lanes and rows are functions of C alone: a graph is cut the same way alone and beside any number of others"""
    for C in WIDTHS:
        cuts = {g[:3] for g in _ask(plan_program, [(G, C, b, 1) for G in GRAPHS for b in (0, 1)])}
        assert len(cuts) == 1, (C, cuts)
