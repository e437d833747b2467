"""The BatchNorm dispatch plan of the library (esc-gnn_amd/csrc/norm_plan.h, host-only C++) against its transcription in
tests/norm_cases.py: tests/norm_plan_host.cpp is compiled once with the host compiler under AddressSanitizer and UBSan, fed every
record of the case table under its own knobs and under the full cross product of knobs 8, 9, 12 and 13, and its answers are
compared with family_of / launches_of / rowblocks and the caps the table states.  Runs no library code and needs no GPU."""
import collections
import itertools
import os
import subprocess

import pytest

import norm_cases as nc
from linear_cases import cdiv
from test_linear_plan_cpu import CSRC, HERE, _host_compiler

Answer = collections.namedtuple("Answer", "family launches slots grids scratch")
ROWS_YCAP, FOLD_FWD_YCAP, LAST_BLOCK_YCAP, FOLD_BWD_YCAP, FLAT_CAP = 2048, 1024, 64, 32, 4096       # the caps norm_cases.branches_of states
KNOB_CROSS = [dict(zip((8, 12, 13, 9), v)) for v in itertools.product((0, 1), (0, 1), (0, 1), (1, 256, 512))]


@pytest.fixture(scope="session")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("norm_plan") / "norm_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "norm_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _line(case, knobs):
    lay = nc.layout_of(case)
    mats = " ".join("%d %d" % lay[op] for op in nc.MATRICES)
    vecs = " ".join(str(lay[v][1]) for v in nc.VECTORS)
    extra = case.extra[0] if case.entry == "bwd_dropout" else 0
    return "%s %d %d %s %s %d %d %d %d %d %d %d %d" % (case.entry, case.M, case.C, mats, vecs, case.has_Y, case.affine, case.extra == "nograd", extra,
                                                      knobs[8], knobs[9], knobs[12], knobs[13])


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [o.split() for o in out if o]
    assert len(out) == len(lines)
    return [Answer(o[0], int(o[1]), int(o[2]), [(int(o[3 + 2 * i]), int(o[4 + 2 * i])) for i in range(3)], int(o[9])) for o in out]


def _rows(M, C, rows_per_wg=16, cap=ROWS_YCAP):
    return (cdiv(C, 256), min(cdiv(M, rows_per_wg), cap))


def _flat(M, C, vec):
    return (min(cdiv(M * (C // vec), 256), FLAT_CAP), 1)


def expected(case, fam, k):
    """(grids, slots) of family `fam`: norm_cases.rowblocks and the caps above, per column block of 256 (float4) or 64 (scalar) columns"""
    M, C, fin = case.M, case.C, (cdiv(case.C, 4), 1)
    head, _, leaf = fam.partition(":")
    apply_grid = {"rows": _rows(M, C), "flat4": _flat(M, C, 4), "flat1": _flat(M, C, 1)}
    if fam in ("bwd:node", "bwd:fold"):
        first = (cdiv(C, 256), cdiv(M, 16)) if fam == "bwd:node" else _rows(M, C, 32, FOLD_BWD_YCAP)
        return [first] + ([_rows(M, C)] if fam == "bwd:fold" else []), first[1]
    if head in ("stats", "bwd", "sums", "coef", "dropout"):
        red = {"in": "v4", "out": "v4"}.get(leaf, leaf.split("+")[0])
        wide = red != "scalar"
        rb = min(cdiv(M, 32), LAST_BLOCK_YCAP) if red == "fused_last_block" else nc.rowblocks(M, wide, head != "stats", k[9])
        grids = [(cdiv(C, 256 if wide else 64), rb)] + ([] if red == "fused_last_block" else [fin])
        if head in ("bwd", "dropout"):
            grids.append(apply_grid[leaf.split("+")[1] if head == "bwd" else "rows"])
        return grids, rb * (1 if wide and head != "stats" else 4)
    if M == 0:
        return [], 0
    if head in ("apply", "affine", "bwd_apply"):
        return [apply_grid[leaf]], 0
    return [{"fold": _rows(M, C, 32, FOLD_FWD_YCAP), "eval_coef": (cdiv(C, 256), 1)}.get(fam, fin)], 0


def _check_scratch(case, a, what):
    assert a.scratch == nc.scratch_floats(case.C), what
    assert a.slots * 2 * case.C + 2 * case.C <= a.scratch, what


def test_the_case_table_under_its_own_knobs(plan_program):
    answers = _ask(plan_program, [_line(c, nc._knobs(c)) for c in nc.CASES])
    assert {a.family for a in answers} == set(nc.FAMILIES)
    for c, a in zip(nc.CASES, answers):
        what = (c.name, a)
        assert a.family == c.family == nc.family_of(c.entry, c), what
        assert a.launches == nc.launches_of(c), what
        grids, slots = expected(c, a.family, nc._knobs(c))
        assert a.grids == grids + [(0, 0)] * (3 - len(grids)) and len(grids) == a.launches and a.slots == slots, (what, grids, slots)
        _check_scratch(c, a, what)
        leaf = a.family.split(":")[-1].split("+")[-1]              # the elementwise launch is the call's last
        if a.launches and (leaf == "rows" or a.family in ("dropout:in", "dropout:out", "bwd:fold")):
            gx, gy = a.grids[a.launches - 1]
            assert 1 <= gx * gy <= cdiv(c.C, 256) * ROWS_YCAP, what
        if a.launches and leaf in ("flat4", "flat1"):
            gx, gy = a.grids[a.launches - 1]
            assert 1 <= gx * gy <= FLAT_CAP, what


def test_the_knob_cross_product(plan_program):
    asked = [(c, k) for k in KNOB_CROSS for c in nc.CASES]
    answers = _ask(plan_program, [_line(c, k) for c, k in asked])
    for (c, k), a in zip(asked, answers):
        what = (c.name, k, a)
        assert a.family == nc.family_of(c.entry, c, knobs=k), what
        _check_scratch(c, a, what)
        assert a.launches == sum(1 for g in a.grids if g != (0, 0)), what


def test_two_billion_rows_take_the_flat_float4_affine(plan_program):
    """esc_affine_act: the rows kernel indexes rows with an int, so M >= 2^31 falls to affine_act_kernel<4> (no table case can hold it)"""
    base = nc.BY_NAME["affine-rows-37x4-a1-mixed"]
    small, huge = _ask(plan_program, [_line(base._replace(M=m), nc.KNOB_DEFAULTS) for m in (2 ** 31 - 1, 2 ** 31)])
    assert small.family == "affine:rows" and small.grids[0] == (1, ROWS_YCAP), small
    assert huge.family == "affine:flat4" and huge.grids[0] == (FLAT_CAP, 1) and huge.launches == 1, huge
