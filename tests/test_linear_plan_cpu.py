"""The Linear dispatch plan of the library (esc-gnn_amd/csrc/linear_plan.h, host-only C++) against its transcription in
tests/linear_cases.py: tests/linear_plan_host.cpp is compiled once with the host compiler under AddressSanitizer and UBSan, fed
every record of the case table under every family mask and the knob sweeps of the r01 tile tests, and its answers are compared
with family_of / stats_block_rows / scratch_needed.  Runs no library code and needs no GPU."""
import glob
import os
import shutil
import subprocess

import pytest

import linear_cases as lc

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "esc-gnn_amd", "csrc")
MASKS = (15, 1, 2, 4, 8, 0)
KNOB_SHAPES = ((131, 70, 100), (128, 128, 64))          # tests/test_hip_dense_dispatch.py
Answer = lc.collections.namedtuple("Answer", "family block_rows promised_rows splits written promised")


def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [shutil.which("g++")] + sorted(glob.glob(os.path.join(rocm, "llvm", "bin", "clang++"))) + sorted(glob.glob(os.path.join(rocm, "lib", "llvm", "bin", "clang++")))
    found = [c for c in found if c]
    assert found, "no host C++ compiler (g++ or ROCm's clang++)"
    return found[0]


@pytest.fixture(scope="session")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("linear_plan") / "linear_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "linear_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _line(case, use_dma=lc.USE_DMA_DEFAULT, knobs=lc.KNOB_DEFAULTS):
    lay = lc.layout_of(case)
    ops = " ".join("%d %d" % lay[op] for op in ("X", "W", "Y", "dX", "dW"))
    stats = case.entry == "fwd" and case.N > 32
    return "%s %d %d %d %s %d %d %d %d %s %d" % (case.entry, case.M, case.N, case.K, ops, lay["P"][1], case.prologue, stats, case.dx,
                                                  " ".join(str(k) for k in knobs), use_dma)


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [o.split() for o in out if o]
    assert len(out) == len(lines)
    return [Answer(o[0], *(int(v) for v in o[1:])) for o in out]


def _expected_family(case, mask):
    fam = lc.family_of(case.entry, case, use_dma=mask)
    if case.entry == "fwd" and case.N > 32 and fam == "r01" and lc.stats_block_rows(case, use_dma=mask) != 32:
        return "r01_rowstats"           # the r01 tiles compute Y, the partials are delivered at the promised height
    return fam


def test_the_case_table_under_every_family_mask(plan_program):
    asked = [(c, m) for m in MASKS for c in lc.CASES]
    answers = _ask(plan_program, [_line(c, use_dma=m) for c, m in asked])
    for (c, m), a in zip(asked, answers):
        what = (c.name, m, a)
        assert a.family == _expected_family(c, m), what
        if c.entry == "fwd" and c.N > 32:
            assert a.block_rows == a.promised_rows == lc.stats_block_rows(c, use_dma=m), what
        if c.entry in ("bwd_weight", "bwd_both"):
            assert a.splits >= 1 and a.written == a.splits * (c.N * c.K + c.N), what
            if m == lc.USE_DMA_DEFAULT:
                assert a.written == lc.scratch_needed(c.entry, c), what
        else:
            assert a.splits == 0 and a.written == 0, what
        assert a.written <= a.promised, what


def _knob_case(entry, M, N, K, flags=""):
    return lc.Case("knob-%s-%dx%dx%d%s" % (entry, M, N, K, flags), entry, M, N, K, "", "p" in flags, True, int("a" in flags), "r01", True)


def _with(knob, value, knobs=lc.KNOB_DEFAULTS):
    return knobs[:knob] + (value,) + knobs[knob + 1:]


def test_the_knob_sweeps_of_the_r01_tiles(plan_program):
    asked = []          # (case, knobs, expected family, expected splits or None)
    dual_tile = {0: (64, 64, 64), 1: (32, 64, 32), 2: (64, 64, 32)}
    for M, N, K in KNOB_SHAPES:
        for tile in range(11):
            for flags in ("", "p"):
                asked.append((_knob_case("fwd", M, N, K, flags), _with(1, tile), "r01", None))
            for flags in ("", "a"):
                asked.append((_knob_case("bwd_input", M, N, K, flags), _with(3, tile), "r01_dx", None))
            for blocks in (1, 512, 4096):
                knobs = _with(5, blocks, _with(4, tile))
                bm, bn, bk = lc.R01_TILE_DIMS.get(tile, (64, 64, 32))
                for flags in ("", "p"):
                    asked.append((_knob_case("bwd_weight", M, N, K, flags), knobs, "r01_dw", lc._r01_wgrad_splits(M, N, K, bm, bn, bk, knobs=knobs)))
        for small_tile in (0, 1, 2):
            for flags in ("", "p", "a"):
                asked.append((_knob_case("bwd_both", M, N, K, flags), _with(7, small_tile), "r01_dual",
                              lc._r01_wgrad_splits(M, N, K, *dual_tile[small_tile])))
    answers = _ask(plan_program, [_line(c, use_dma=0, knobs=k) for c, k, _, _ in asked])
    for (c, k, family, splits), a in zip(asked, answers):
        what = (c.name, k, a)
        assert a.family == family, what
        if c.entry == "fwd":
            assert a.block_rows == a.promised_rows == 32, what
        if splits is not None:
            assert a.splits == splits and a.written == splits * (c.N * c.K + c.N), what
        assert a.written <= a.promised, what
