"""The dispatch rule of the PNA aggregate (esc-gnn_amd/csrc/pna_plan.h, host-only C++) against its transcription below:
tests/pna_plan_host.cpp is compiled once with the host compiler under AddressSanitizer and UBSan and asked for the lanes per
node and the grids of the forward and the backward at every width at which the rule flips.  Runs no library code and needs no
GPU."""
import os
import subprocess

import pytest

from test_linear_plan_cpu import CSRC, HERE, _host_compiler

FLIP_WIDTHS = (4, 64, 68, 128, 132)
NODES = (0, 1, 3, 4, 5, 16, 17, 796, 7112)
BLOCK, MAX_C = 256, 1024


def lanes_per_node(C):
    """float4 lanes that cover a row: 16 up to C = 64, 32 up to 128, a whole wave beyond (it loops over wider rows)"""
    return 16 if C <= 64 else 32 if C <= 128 else 64


def expected(N, C, backward):
    lanes = lanes_per_node(C)
    grid = -(-N * lanes // BLOCK)
    return (lanes, 64 // lanes, 2 if backward else 1, grid, grid if backward else 0, BLOCK, MAX_C)


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pna_plan") / "pna_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "pna_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, calls):
    text = "".join("%d %d %d\n" % c for c in calls)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [tuple(int(v) for v in o.split()) for o in out if o]
    assert len(out) == len(calls)
    return out


def test_lanes_per_node_at_the_widths_where_the_rule_flips(plan_program):
    got = _ask(plan_program, [(796, C, 0) for C in FLIP_WIDTHS])
    assert [g[0] for g in got] == [16, 16, 32, 32, 64] == [lanes_per_node(C) for C in FLIP_WIDTHS]
    assert [g[1] for g in got] == [4, 4, 2, 2, 1]


def test_grids_against_the_transcription(plan_program):
    calls = [(N, C, b) for N in NODES for C in FLIP_WIDTHS + (256, 1024) for b in (0, 1)]
    for call, got in zip(calls, _ask(plan_program, calls)):
        N, C, b = call
        assert got == expected(N, C, b), (call, got)
        lanes, per_wave, launches, g0, g1 = got[:5]
        assert lanes * per_wave == 64 and lanes * 4 >= min(C, 256)              # a full row in one pass up to C = 256
        assert g0 * BLOCK >= N * lanes and (g0 == 0) == (N == 0)                # every node has a group; nothing for no nodes
        assert (g0 - 1) * BLOCK < N * lanes or N == 0                           # ... and no workgroup without one
        assert launches == sum(1 for g in (g0, g1) if g) or N == 0
