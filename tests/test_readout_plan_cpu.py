"""plan_both_bn (esc-gnn_amd/csrc/linear_plan.h) with PlanKnobs::dual_split off and on: tests/readout_plan_host.cpp is compiled
with the host compiler under AddressSanitizer and UBSan and asked for the readout Linear's edge-stream column blocks
(2400 x 256 x 256 l, l = 1..4) and for shapes the fused LDS-DMA tiles do not serve.  Off: today's plan, one launch.  On: the same
family, tile and slabs (so the same bits) as two launches, the dX launch with the LDS request of the knob, inside the promised
scratch.  Shapes served by other kernels keep their plan.  Runs no library code and needs no GPU."""
import os
import subprocess

import pytest

from test_linear_plan_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "esc-gnn_amd", "csrc")
LDS = 160 * 1024


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("readout_plan") / "readout_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "readout_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, calls):
    """calls: (M, N, K, ldX, offX, next, request) -> (family, bm, splits, per_split, written, promised, launches, dx_lds)"""
    text = "".join("%d %d %d %d %d %d %d\n" % c for c in calls)
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [o.split() for o in out if o]
    assert len(out) == len(calls)
    return [(o[0],) + tuple(int(v) for v in o[1:]) for o in out]


def _cdiv(a, b):
    return -(-a // b)


def _splits(M, N, K, tile):
    """dma_wgrad_splits: about one workgroup per CU, slabs at least 128 rows deep, a multiple of 32"""
    sp = max(1, min(_cdiv(256, _cdiv(N, tile) * _cdiv(K, tile)), _cdiv(M, 128)))
    per = max(128, _cdiv(_cdiv(M, sp), 32) * 32)
    return _cdiv(M, per), per


K0_SHAPES = [(2400, 256, 256 * l) for l in range(1, 5)]
SMALL = [(96, 128, 128), (128, 128, 384), (130, 128, 128), (300, 128, 384)]


def test_request_off_keeps_todays_plan(program):
    shapes = K0_SHAPES + SMALL
    for (M, N, K), a in zip(shapes, _ask(program, [(M, N, K, K + 136, 128, 0, 0) for M, N, K in shapes])):
        splits, per = _splits(M, N, K, 64)
        assert a == ("dma64_bn", 64, splits, per, splits * (N * K + N), (_cdiv(M, 128) + 1) * (N * K + N), 1, 0), (K, a)
    assert _splits(2400, 256, 1024, 64) == (4, 608)          # the flagship's block: 608 dX tiles + 64 dW tiles x 4 slabs


@pytest.mark.parametrize("request_,dx_lds", [(1, 0), (84 * 1024, 84 * 1024), (LDS, LDS), (LDS + 4, LDS), (1 << 30, LDS)])
def test_request_on_is_the_same_plan_in_two_launches(program, request_, dx_lds):
    shapes = K0_SHAPES + SMALL + [(15200, 256, 256)]
    off = _ask(program, [(M, N, K, K + 136, 128, nxt, 0) for M, N, K in shapes for nxt in (0, 1)])
    on = _ask(program, [(M, N, K, K + 136, 128, nxt, request_) for M, N, K in shapes for nxt in (0, 1)])
    for a, b in zip(off, on):
        assert a[0] in ("dma64_bn", "dma128_bn")
        assert b[:6] == a[:6], (a, b)                     # family, tile, slab boundaries, floats written: every element keeps its sums
        assert b[4] <= b[5], b                            # ... inside esc_linear_bwd_weight_scratch
        assert a[6:] == (1, 0) and b[6:] == (2, dx_lds), (a, b)


def test_shapes_the_fused_tiles_do_not_serve_keep_their_plan(program):
    calls = [(2400, 256, 256, 393, 0, 0),       # leading dimension not a multiple of 4: not served at all
             (2400, 256, 256, 392, 1, 0),       # X not 16-byte aligned: not served at all
             (2400, 256, 10, 16, 0, 0),         # the tiny-K kernels: their own two launches, no request
             (2400, 700, 256, 256, 0, 0),       # more BatchNorm channels than the tiles keep in LDS
             (15200, 256, 300, 308, 0, 0)]      # edge rows the big tile does not serve
    off = _ask(program, [c + (0,) for c in calls])
    on = _ask(program, [c + (84 * 1024,) for c in calls])
    assert on == off
    assert [a[0] for a in off] == ["none", "none", "small_bn", "none", "none"]
    assert all(a[6:] == (1, 0) for a in off)
