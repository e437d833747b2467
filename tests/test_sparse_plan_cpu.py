"""The dispatch plan of the index-driven row kernels (esc-gnn_amd/csrc/sparse_plan.h, host-only C++) against its transcription in
tests/sparse_cases.py: tests/sparse_plan_host.cpp is compiled once with the host compiler under AddressSanitizer and UBSan, fed
every record of the case table under its own switches and under the full cross product of ESC_AGG_SPLIT, ESC_AGG_SPLIT_BWD and
ESC_BAG_TILED, and its answers are compared with family_of / expected and the query formulas.  The promises the callers size their
buffers by are held as inequalities.  Runs no library code and needs no GPU."""
import collections
import itertools
import os
import subprocess

import pytest

import sparse_cases as sc
from sparse_cases import cdiv
from test_linear_plan_cpu import CSRC, HERE, _host_compiler

Answer = collections.namedtuple("Answer", "family launches grids lds slots split cw refused chunks order_offset bucket_offset scratch deps_slots stats_slots "
                                          "block_rows gp_blocks")
KNOB_CROSS = [dict(zip(("agg_split", "agg_split_bwd", "bag_tiled"), v)) for v in itertools.product((1, 2), (1, 2), (0, 1))]


@pytest.fixture(scope="session")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sparse_plan") / "sparse_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "sparse_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _line(case, knobs):
    lay = sc.layout_of(case)
    # (an operand that is not given comes with a leading dimension that would rule float4 access out, did it count)
    slots = ["1 %d %d" % lay[op] if lay[op] is not None else "0 %d 0" % (case.C + 1) for op in sc.OPERANDS[case.entry]]
    slots += ["0 0 0"] * (9 - len(slots))
    flag = lambda f: int(f in case.flags)
    return "%s %d %d %d %d %d %d %d %d %d %d %d %s %d %d %d" % (case.entry, case.N, case.C, case.Z, case.rows, case.k, sc.N_COLS, flag("span"), flag("acc"),
                                                              flag("classified"), 3 * flag("counters"), flag("deps"), " ".join(slots),
                                                              knobs["agg_split"], knobs["agg_split_bwd"], knobs["bag_tiled"])


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [o.split() for o in out if o]
    assert len(out) == len(lines)
    return [Answer(o[0], int(o[1]), [(int(o[2 + 2 * i]), int(o[3 + 2 * i])) for i in range(3)], *(int(v) for v in o[8:])) for o in out]


def _check(c, k, a):
    """family, grids, LDS, slots, scratch and the queries of one answer against the transcription; then the promises"""
    what = (c.name, k, a)
    want = sc.expected(c, k)
    assert a.family == sc.family_of(c.entry, c, k), what
    assert a.grids == want["grids"] + [(0, 0)] * (3 - len(want["grids"])) and a.launches == len(want["grids"]), (what, want)
    assert (a.lds, a.slots, a.split, bool(a.refused)) == (want["lds"], want["slots"], want["split"], want["refused"]), (what, want)
    assert a.scratch == sc.scratch_floats(c.Z, c.C) and a.deps_slots == sc.deps_slots(c.C, k) and a.stats_slots == cdiv(c.N, 4), what
    assert a.gp_blocks == sc.gp_bwd_blocks(c.N) and 1 <= a.gp_blocks <= sc.GP_BWD_MAX_BLOCKS, what
    kind = a.family.split(":")[0]
    if kind == "agg_bwd":
        # deps slots x N covers every wave that writes deps_part (wave w writes deps_part[w], split waves per row)
        assert a.split * c.N <= a.deps_slots * c.N, what
        if a.family.endswith("+stats"):                         # one BatchNorm partial per workgroup; [4 waves][C] float2 of LDS
            assert a.slots == a.grids[0][0] == a.stats_slots and a.split == 1 and a.lds == 4 * c.C * 8, what
    if kind == "bag_fwd":
        if c.entry == "bag_fwd_rows":      # esc_bag_fwd_stats_block_rows != 0 exactly where the tiled kernel serves the shape; statistics need it
            assert a.block_rows == (sc.BAG_EB if sc.tiled_ok(c, sc.layout_of(c), k) else 0), what
            assert not (a.family == "bag_fwd:tiled:stats" and a.block_rows == 0) and ("stats" in c.flags or not a.refused), what
        if a.family.startswith("bag_fwd:tiled"):
            assert a.lds <= 160 * 1024 and c.rows <= sc.BAG_MAXROWS and a.grids[0][1] * sc.BAG_EB >= c.N, what
    if kind in ("bag_bwd", "classify"):
        chunks = cdiv(c.Z, sc.BAG_CH)
        if "local" in a.family or a.family.endswith("+classify"):
            # scratch_floats(Z, H) covers the chunk partials [chunks][2][H], then order [8][chunks], then bucket_cnt [8]
            assert a.chunks == chunks and a.order_offset == 2 * chunks * c.C and a.bucket_offset == a.order_offset + 8 * chunks, what
            assert a.bucket_offset + 8 <= a.scratch, what
        else:
            assert 2 * chunks * c.C <= a.scratch, what
    if kind == "bag_bwd":
        # the pass-2 LDS stays <= 64 KiB exactly where the entry does not refuse, and pass 2 is the launch that is dropped
        assert a.lds == 3 * c.C * 4 and bool(a.refused) == (a.lds > 64 * 1024), what
        assert (a.grids[a.launches - 1] == (sc.N_COLS, 1)) == (not a.refused), what
        if "local" in a.family:                                 # every chunk of every bucket has a wave even when one bucket holds them all
            assert a.grids[a.launches - 2][0] % 8 == 0 and a.grids[a.launches - 2][0] // 8 * 4 >= cdiv(chunks, 8), what
    if kind == "embed_bwd" and a.family.endswith("generic"):
        assert a.cw == sc.embed_cw(c.C) and a.cw <= 256 and (a.cw >= c.C or a.cw == 256) and a.cw & (a.cw - 1) == 0, what
    if kind == "gp_bwd":
        assert a.slots == a.gp_blocks == a.grids[0][0] and a.slots * sc.GP_BWD_WAVES >= min(c.N, 1), what
    if kind.startswith("gated"):
        assert a.cw == int(a.family.split(":")[1]) and a.grids[0][0] * 256 >= c.N * a.cw and a.cw * 4 >= min(c.C, 256), what


def test_the_case_table_under_its_own_knobs(plan_program):
    answers = _ask(plan_program, [_line(c, sc._knobs(c)) for c in sc.CASES])
    assert {a.family for a in answers} == set(sc.FAMILIES)
    for c, a in zip(sc.CASES, answers):
        _check(c, sc._knobs(c), a)


def test_every_family_that_can_run_has_a_case_to_run_on():
    """tests/test_hip_sparse_dispatch.py takes its cases from here: all but the counters-only classify launch, which only the step
    engine can ask for (the training-step tests run it)"""
    assert [f for f in sc.FAMILIES if sc.gpu_case_of(f) is None] == ["classify:launch"]


def test_the_knob_cross_product(plan_program):
    asked = [(c, k) for k in KNOB_CROSS for c in sc.CASES]
    answers = _ask(plan_program, [_line(c, k) for c, k in asked])
    for (c, k), a in zip(asked, answers):
        _check(c, k, a)
        assert a.launches == sum(1 for g in a.grids if g != (0, 0)), (c.name, k, a)


def test_the_edges_at_which_a_rule_flips():
    """the table's edge cases answer as their names say (read off the table by name, under the cases' own switches)"""
    fam = lambda name: sc.family_of(sc.BY_NAME[name].entry, sc.BY_NAME[name])
    assert [fam("agg_fwd-C%d" % C) for C in (4, 60, 63, 64, 66, 68, 252, 256, 260)] == ["agg_fwd:" + f for f in (
        "elem", "elem", "elem", "wave4", "wave1", "wave4", "wave4", "wave2", "wave4")]
    assert [fam("agg_bwd-C%d" % C) for C in (4, 60, 63, 64, 66, 68, 252, 256, 260)] == ["agg_bwd:" + f for f in (
        "wave4", "wave4", "wave1", "wave4", "wave1", "wave4", "wave4", "wave4", "wave4")]
    assert fam("agg_fwd_affine-C256-span") == "agg_fwd:wave2+affine+span" and fam("agg_fwd_affine-C256-span-split1") == "agg_fwd:wave4+affine"
    assert fam("agg_fwd-C256-ld_x+1") == "agg_fwd:wave1" and fam("agg_fwd-C256-ld_all+4") == "agg_fwd:wave2" and fam("agg_fwd-C64-e@1") == "agg_fwd:wave1"
    assert fam("agg_fwd-C64-no_e") == "agg_fwd:wave4" and fam("agg_bwd-C64-no_dx") == "agg_bwd:wave4" and fam("agg_bwd-C256-no_e") == "agg_bwd:wave2"
    assert (fam("bag_rows-tiled-E511"), fam("bag_rows-tiled-E512")) == ("bag_fwd:row4", "bag_fwd:tiled")
    assert (fam("bag_rows-tiled-maxrows"), fam("bag_rows-tiled-maxrows+1")) == ("bag_fwd:tiled", "bag_fwd:row4")
    assert (fam("bag_bwd-63chunks"), fam("bag_bwd-64chunks")) == ("bag_bwd:flat:v4", "bag_bwd:local:v4+classify")
    assert (fam("bag_bwd-4MiB"), fam("bag_bwd-4MiB+1row")) == ("bag_bwd:flat:v4", "bag_bwd:local:v4+classify")
    assert fam("bag_bwd-rows0") == fam("bag_bwd-local-plain_entry") == "bag_bwd:flat:v4" and fam("bag_bwd-Z0") == "bag_bwd:none:v4"
    assert [sc.expected(sc.BY_NAME[n])["refused"] for n in ("bag_bwd-H5461", "bag_bwd-H5462-refused")] == [False, True]
    assert (fam("embed-v4-C256"), fam("embed-C260"), fam("embed-one_row")) == ("embed_bwd:v4", "embed_bwd:generic", "embed_bwd:one_row")
    assert [sc.embed_cw(C) for C in (1, 30, 257, 260)] == [1, 32, 256, 256]
    assert [sc.gp_bwd_blocks(N) for N in (1, 8, 9, 8 * 512, 8 * 512 + 1)] == [1, 1, 2, 512, 512]
    assert [fam("gated_fwd-C%d" % C) for C in (4, 64, 68, 128, 132)] == ["gated_fwd:%d" % g for g in (16, 16, 32, 32, 64)]
    assert fam("gp_fwd-C64-x3+1-beyond_k") == "gp_fwd:v4" and fam("gp_fwd-C64-x2+1") == "gp_fwd:v1" and fam("gp_fwd-C64-eps@1") == "gp_fwd:v1"
