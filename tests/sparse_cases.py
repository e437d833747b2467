"""The case table of the index-driven row kernels (csrc/aggregate.hip, bag.hip, embed.hip, gineplus.hip, gatedgcn.hip): one
record per (entry point, width, operand layout, optional operand, switch) chosen so that every kernel family the host rules of
csrc/sparse_plan.h can pick is reached by name, at the edges where a rule flips.  No GPU is needed to import this module:
tests/test_sparse_plan_cpu.py holds the header to family_of / expected, which stay an independent transcription, and
tests/test_hip_sparse_dispatch.py runs one case per family against the library.

A case is Case(name, entry, N, C, Z, rows, k, layout, absent, flags, knobs, graph):
  entry     agg_fwd | agg_fwd_affine | agg_bwd | agg_bwd_affine | agg_bwd_stats | pool | bag_fwd | bag_fwd_acc | bag_fwd_rows |
            bag_bwd | bag_bwd_rows | classify | embed_bwd | gp_fwd | gp_bwd | gated_fwd | gated_bwd
  N         rows of the call: nodes (aggregate, GINE+, GatedGCN), graphs (pool), edges E (bag forward), index count M (embed)
  C         row width (H of the bag)        Z   bag entries          rows  table height (bag, embed); 0: not given
  k         GINE+ hops
  layout    comma-separated edits of the plain layout (16-byte aligned base, ld == C): "x+1" operand x has ld = C + 1,
            "e@1" its base is 1 float (4 bytes) past a 16-byte boundary
  absent    optional operands not given (NULL)
  flags     span (an armed esc_prof_span), acc (accumulate), stats (the statistics operand given), classified, counters (the step
            engine's BatchNorm counters ride on the classify launch), deps (d_eps wanted)
  knobs     {"agg_split": .., "agg_split_bwd": .., "bag_tiled": ..} the case is MEANT for (ESC_AGG_SPLIT, ESC_AGG_SPLIT_BWD, ESC_BAG_TILED)
  graph     the structure a GPU run uses: a case of tests/graph_cases.py (GINE+: of gineplus_cases.py, GatedGCN: of gatedgcn_oracle.py;
            "embed": M indices drawn over the table's rows, "no_entries": a bag without entries); None: CPU only
"""
import collections

Case = collections.namedtuple("Case", "name entry N C Z rows k layout absent flags knobs graph")

KNOB_DEFAULTS = {"agg_split": 2, "agg_split_bwd": 1, "bag_tiled": 0}
BAG_CH, BAG_EB, BAG_CAP, BAG_ENT, BAG_MAXROWS = 64, 128, 192, 6144, 4096
N_COLS = 1800                                             # graph_cases.N_COLS: the bag's table height in the structure tests
GP_BWD_WAVES, GP_BWD_MAX_BLOCKS = 8, 512

OPERANDS = {
    "agg_fwd": ("x", "e", "out"), "agg_fwd_affine": ("x", "e", "out"),
    "agg_bwd": ("x", "e", "g", "d_e", "dx"), "agg_bwd_affine": ("x", "e", "g", "d_e", "dx"), "agg_bwd_stats": ("x", "e", "g", "d_e", "dx"),
    "pool": ("x", "out"),
    "bag_fwd": ("table", "out", "stats"), "bag_fwd_acc": ("table", "out", "stats"), "bag_fwd_rows": ("table", "out", "stats"),
    "bag_bwd": ("dz", "dtable", "partials"), "bag_bwd_rows": ("dz", "dtable", "partials"),
    "classify": (), "embed_bwd": ("g", "dtable"),
    "gp_fwd": ("x0", "x1", "x2", "x3", "e", "out", "eps"),
    "gp_bwd": ("x0", "x1", "x2", "x3", "e", "g", "dx", "d_e", "eps"),
    "gated_fwd": (), "gated_bwd": (),
}
VECTORS = ("eps", "stats")                                # no leading dimension
DENSE = {"table", "dtable", "partials"}                   # always ld = C; so are dx and d_e of gp_bwd


def cdiv(a, b):
    return -(-a // b)


def _knobs(case, knobs=None):
    k = dict(KNOB_DEFAULTS)
    k.update(case.knobs if knobs is None else knobs)
    return k


def layout_of(case):
    """operand -> (ld, offset in floats) or None where the operand is not given"""
    out = {}
    for op in OPERANDS[case.entry]:
        given = op not in case.absent and (op != "stats" or "stats" in case.flags)
        if case.entry in ("gp_fwd", "gp_bwd") and op in ("x1", "x2", "x3") and int(op[1]) >= case.k:
            given = False                                 # filled below: the kernels are handed x0 again
        out[op] = (0 if op in VECTORS else case.C, 0) if given else None
    for edit in filter(None, case.layout.split(",")):
        op, pad, off = (edit.split("+") + [0]) if "+" in edit else (edit.split("@")[0], 0, edit.split("@")[1])
        assert not int(pad) or (op not in DENSE and op not in VECTORS and not (case.entry == "gp_bwd" and op in ("dx", "d_e")))
        if out[op] is not None:                           # (an operand that is not given has no layout)
            out[op] = (out[op][0] + int(pad), out[op][1] + int(off))
    if case.entry in ("gp_fwd", "gp_bwd"):
        for d in (1, 2, 3):
            if d >= case.k:
                out["x%d" % d] = out["x0"]
    return out


def _vec(case, lay, ops):
    """sparse::rows_vec: C, every given leading dimension a multiple of 4, every given base 16-byte aligned"""
    return case.C % 4 == 0 and all(lay[o] is None or (lay[o][0] % 4 == 0 and lay[o][1] % 4 == 0) for o in ops)


def local_schedule(Z, H, rows):
    return rows > 0 and rows * H * 4 > (4 << 20) and cdiv(Z, BAG_CH) >= 64


def tiled_ok(case, lay, k):
    return bool(k["bag_tiled"]) and 0 < case.rows <= BAG_MAXROWS and _vec(case, lay, ("table", "out")) and case.N >= 4 * BAG_EB and cdiv(case.C, 64) <= 65535


def family_of(entry, case, knobs=None):
    """the kernel family the host code of the entry picks for `case` under `knobs`"""
    lay, k, C = layout_of(case), _knobs(case, knobs), case.C
    if entry in ("agg_fwd", "agg_fwd_affine"):
        if C < 64:
            return "agg_fwd:elem"
        vec = _vec(case, lay, ("x", "e", "out"))
        split = vec and k["agg_split"] == 2 and C == 256
        fam = "agg_fwd:" + ("wave2" if split else "wave4" if vec else "wave1")
        if entry == "agg_fwd_affine":       # an armed span is honoured only together with split 2
            fam += "+affine" + ("+span" if (split and "span" in case.flags) else "")
        return fam
    if entry in ("agg_bwd", "agg_bwd_affine", "agg_bwd_stats"):
        vec = _vec(case, lay, ("x", "e", "g", "d_e", "dx"))
        split = vec and entry != "agg_bwd_stats" and k["agg_split_bwd"] == 2 and C == 256
        return "agg_bwd:" + ("wave2" if split else "wave4" if vec else "wave1") + {"agg_bwd": "", "agg_bwd_affine": "+affine", "agg_bwd_stats": "+affine+stats"}[entry]
    if entry == "pool":
        return "pool:v4" if _vec(case, lay, ("x", "out")) else "pool:v1"
    if entry in ("bag_fwd", "bag_fwd_acc", "bag_fwd_rows"):
        acc = entry == "bag_fwd_acc" or "acc" in case.flags
        tiled = entry == "bag_fwd_rows" and tiled_ok(case, lay, k)
        if lay["stats"] is not None and not (tiled and not acc and lay["stats"][1] % 4 == 0):
            return "bag_fwd:none"
        if tiled:
            return "bag_fwd:tiled" + (":acc" if acc else ":stats" if lay["stats"] is not None else "")
        return "bag_fwd:" + ("row4" if _vec(case, lay, ("table", "out")) else "row1") + ("+acc" if acc else "")
    if entry in ("bag_bwd", "bag_bwd_rows"):
        local = case.Z > 0 and entry == "bag_bwd_rows" and local_schedule(case.Z, C, case.rows)
        fam = "bag_bwd:" + ("none" if case.Z == 0 else "local" if local else "flat") + (":v4" if _vec(case, lay, ("dz", "dtable", "partials")) else ":scalar")
        return fam + ("+classify" if local and "classified" not in case.flags else "")
    if entry == "classify":
        sched = local_schedule(case.Z, C, case.rows)
        return "classify:launch+classify" if sched else "classify:launch" if "counters" in case.flags else "classify:none"
    if entry == "embed_bwd":
        if case.rows == 1:
            return "embed_bwd:one_row"
        return "embed_bwd:v4" if (C <= 256 and _vec(case, lay, ("g", "dtable"))) else "embed_bwd:generic"
    if entry == "gp_fwd":
        return "gp_fwd:v4" if _vec(case, lay, OPERANDS["gp_fwd"]) else "gp_fwd:v1"
    if entry == "gp_bwd":
        return "gp_bwd:v4" if _vec(case, lay, OPERANDS["gp_bwd"]) else "gp_bwd:v1"
    assert entry in ("gated_fwd", "gated_bwd")
    return "%s:%d" % (entry, 16 if C <= 64 else 32 if C <= 128 else 64)


def scratch_floats(Z, H):
    """esc_bag_bwd_scratch"""
    return 2 * cdiv(Z, BAG_CH) * H + 8 * cdiv(Z, BAG_CH) + 64


def deps_slots(C, k):
    """esc_gine_aggregate_bwd_deps_slots"""
    return 2 if (k["agg_split_bwd"] == 2 and C == 256) else 1


def gp_bwd_blocks(N):
    """esc_gineplus_bwd_blocks"""
    return max(1, min(cdiv(N, GP_BWD_WAVES), GP_BWD_MAX_BLOCKS))


def embed_cw(C):
    cw = 1
    while cw < C and cw < 256:
        cw <<= 1
    return cw


def expected(case, knobs=None):
    """what the plan promises besides the family: grids (in launch order), dynamic LDS bytes, slots, waves per row, refusal"""
    fam, k, N, C = family_of(case.entry, case, knobs), _knobs(case, knobs), case.N, case.C
    kind, _, leaf = fam.partition(":")
    out = dict(grids=[], lds=0, slots=0, split=1, refused=False)
    if kind in ("agg_fwd", "agg_bwd"):
        out["split"] = 2 if leaf.startswith("wave2") else 1
        out["grids"] = [(cdiv(N * C, 256), 1)] if leaf == "elem" else [(cdiv(out["split"] * N, 4), 1)]
        if kind == "agg_bwd":
            out["slots"] = cdiv(N, 4) if leaf.endswith("+stats") else deps_slots(C, k)
            out["lds"] = 4 * C * 8 if leaf.endswith("+stats") else 0
    elif kind == "pool":
        out["grids"] = [(cdiv(N, 4), 1)]
    elif kind == "bag_fwd":
        out["refused"] = leaf == "none"
        if leaf.startswith("tiled"):
            out["grids"] = [(cdiv(C, 64), cdiv(N, BAG_EB))]
            out["lds"] = BAG_CAP * 256 + BAG_ENT * 4 + ((case.rows + 7) // 8 * 8) * 2 + BAG_CAP * 2 + 64
            out["slots"] = BAG_EB
        elif leaf != "none" and N > 0:
            out["grids"] = [(cdiv(N, 4), 1)]
    elif kind == "bag_bwd":
        chunks = cdiv(case.Z, BAG_CH)
        if leaf.startswith("local"):
            if leaf.endswith("+classify"):
                out["grids"].append((cdiv(chunks, 256), 1))
            out["grids"].append((cdiv(cdiv(chunks, 8) * 5 // 4 + 4, 4) * 8, 1))
        elif leaf.startswith("flat"):
            out["grids"].append((cdiv(chunks, 4), 1))
        out["lds"] = 3 * C * 4
        out["refused"] = out["lds"] > 64 * 1024
        if not out["refused"]:
            out["grids"].append((N_COLS, 1))
    elif kind == "classify":
        if leaf != "none":
            out["grids"] = [(cdiv(cdiv(case.Z, BAG_CH), 256) if leaf.endswith("+classify") else 1, 1)]
    elif kind == "embed_bwd":
        out["grids"] = [(cdiv(C, 64) if leaf == "one_row" else case.rows, 1)]
    elif kind == "gp_fwd":
        out["grids"] = [(cdiv(N, 4), 1)]
    elif kind == "gp_bwd":
        out["slots"] = gp_bwd_blocks(N)
        out["grids"] = [(out["slots"], 1)] + ([(cdiv((case.k + 1) * C, 64), 1)] if "deps" in case.flags else [])
    else:
        g = (cdiv(N * int(leaf), 256), 1)
        out["grids"] = [g, g] if kind == "gated_bwd" else [g]
    return out


# ---- the table -----------------------------------------------------------------------------------------------------------
def _c(name, entry, N, C, Z=0, rows=0, k=0, layout="", absent=(), flags=(), knobs=None, graph=None):
    return Case(name, entry, N, C, Z, rows, k, layout, tuple(absent), tuple(flags), dict(knobs or {}), graph)


def _aggregate():
    out = []
    for C in (4, 60, 63, 64, 66, 68, 252, 256, 260):                   # tiny_N5: 5 nodes, 8 edges
        out.append(_c("agg_fwd-C%d" % C, "agg_fwd", 5, C, graph="tiny_N5"))
        out.append(_c("agg_bwd-C%d" % C, "agg_bwd", 5, C, graph="tiny_N5"))
        if C >= 64 and C % 4 == 0:                                      # the affine entries refuse the rest
            out.append(_c("agg_fwd_affine-C%d" % C, "agg_fwd_affine", 5, C, graph="tiny_N5"))
            out.append(_c("agg_bwd_affine-C%d" % C, "agg_bwd_affine", 5, C, graph="tiny_N5"))
            out.append(_c("agg_bwd_stats-C%d" % C, "agg_bwd_stats", 5, C, graph="tiny_N5"))
    out += [
        _c("agg_fwd-C256-split1", "agg_fwd", 5, 256, knobs={"agg_split": 1}, graph="tiny_N5"),
        _c("agg_fwd_affine-C256-split1", "agg_fwd_affine", 5, 256, knobs={"agg_split": 1}, graph="tiny_N5"),
        _c("agg_fwd_affine-C256-span", "agg_fwd_affine", 5, 256, flags=("span",), graph="tiny_N5"),
        _c("agg_fwd_affine-C256-span-split1", "agg_fwd_affine", 5, 256, flags=("span",), knobs={"agg_split": 1}, graph="tiny_N5"),
        _c("agg_fwd_affine-C68-span", "agg_fwd_affine", 5, 68, flags=("span",), graph="tiny_N5"),
        _c("agg_bwd-C256-split2", "agg_bwd", 5, 256, knobs={"agg_split_bwd": 2}, graph="tiny_N5"),
        _c("agg_bwd_affine-C256-split2", "agg_bwd_affine", 5, 256, knobs={"agg_split_bwd": 2}, graph="tiny_N5"),
        _c("agg_bwd_stats-C256-split2", "agg_bwd_stats", 5, 256, knobs={"agg_split_bwd": 2}, graph="tiny_N5"),
        # a leading dimension that is no multiple of 4, a base 4 bytes past its boundary: the scalar wave kernel even at C = 256
        _c("agg_fwd-C256-ld_x+1", "agg_fwd", 5, 256, layout="x+1", graph="tiny_N5"),
        _c("agg_fwd-C256-ld_all+4", "agg_fwd", 5, 256, layout="x+4,e+4,out+4", graph="tiny_N5"),
        _c("agg_fwd-C64-out@1", "agg_fwd", 5, 64, layout="out@1", graph="tiny_N5"),
        _c("agg_fwd-C64-e@1", "agg_fwd", 5, 64, layout="e@1", graph="tiny_N5"),
        _c("agg_bwd-C256-ld_g+1", "agg_bwd", 5, 256, layout="g+1", knobs={"agg_split_bwd": 2}, graph="tiny_N5"),
        _c("agg_bwd-C68-dx@1", "agg_bwd", 5, 68, layout="dx@1", graph="tiny_N5"),
        _c("agg_bwd-C68-d_e+2", "agg_bwd", 5, 68, layout="d_e+2", graph="tiny_N5"),
        # each optional operand absent: what it would have ruled out no longer counts
        _c("agg_fwd-C64-no_e", "agg_fwd", 5, 64, absent=("e",), graph="tiny_N5"),
        _c("agg_fwd_affine-C256-no_e", "agg_fwd_affine", 5, 256, absent=("e",), graph="tiny_N5"),
        _c("agg_bwd-C256-no_e", "agg_bwd", 5, 256, absent=("e", "d_e"), knobs={"agg_split_bwd": 2}, graph="tiny_N5"),
        _c("agg_bwd-C64-no_d_e", "agg_bwd", 5, 64, absent=("d_e",), graph="tiny_N5"),
        _c("agg_bwd-C64-no_dx", "agg_bwd", 5, 64, absent=("dx",), graph="tiny_N5"),
        _c("agg_bwd_affine-C64-no_dx-no_d_e", "agg_bwd_affine", 5, 64, absent=("dx", "d_e"), graph="tiny_N5"),
        _c("agg_bwd_stats-C64-no_d_e", "agg_bwd_stats", 5, 64, absent=("d_e",), graph="tiny_N5"),
        _c("agg_fwd-N1-C256", "agg_fwd", 1, 256, graph="tiny_N1"),
        _c("agg_bwd_stats-N1-C64", "agg_bwd_stats", 1, 64, graph="tiny_N1"),
        _c("pool-C256", "pool", 5, 256, graph="segments_G5"),
        _c("pool-C10", "pool", 5, 10, graph="segments_G5"),
        _c("pool-C64-ld+1", "pool", 1, 64, layout="x+1", graph="segments_G1"),
        _c("pool-C64-out@1", "pool", 9, 64, layout="out@1", graph="segments_G9"),
    ]
    return out


def _bag():
    tiled = {"bag_tiled": 1}
    E_LOCAL, Z_LOCAL = 4200, 4096 + 37                                 # graph_cases.bag_local: 65 chunks, 4200 x 256 floats > 4 MiB
    return [
        _c("bag_fwd-H256", "bag_fwd", 3, 256, Z=5, graph="bag_tiny"),
        _c("bag_fwd-H10", "bag_fwd", 3, 10, Z=5, graph="bag_tiny"),
        _c("bag_fwd-H256-out+1", "bag_fwd", 3, 256, Z=5, layout="out+1", graph="bag_tiny"),
        _c("bag_fwd-H256-table@1", "bag_fwd", 3, 256, Z=5, layout="table@1"),
        _c("bag_fwd_acc-H256", "bag_fwd_acc", 3, 256, Z=5, graph="bag_tiny"),
        _c("bag_fwd_acc-H10", "bag_fwd_acc", 3, 10, Z=5, graph="bag_tiny"),
        _c("bag_fwd-E0", "bag_fwd", 0, 64),
        # esc_bag_fwd_rows: the switch, the table height, E against 4 * BAG_EB, float4 access
        _c("bag_rows-off", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, graph="bag_local"),
        _c("bag_rows-off-acc", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, flags=("acc",), graph="bag_local"),
        _c("bag_rows-off-stats-refused", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, flags=("stats",), graph="bag_local"),
        _c("bag_rows-tiled", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, knobs=tiled, graph="bag_local"),
        _c("bag_rows-tiled-acc", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, flags=("acc",), knobs=tiled, graph="bag_local"),
        _c("bag_rows-tiled-stats", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, flags=("stats",), knobs=tiled, graph="bag_local"),
        _c("bag_rows-tiled-stats+acc-refused", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, flags=("stats", "acc"), knobs=tiled),
        _c("bag_rows-tiled-stats@1-refused", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, layout="stats@1", flags=("stats",), knobs=tiled),
        _c("bag_rows-tiled-E511", "bag_fwd_rows", 4 * BAG_EB - 1, 64, Z=600, rows=N_COLS, knobs=tiled),
        _c("bag_rows-tiled-E512", "bag_fwd_rows", 4 * BAG_EB, 64, Z=600, rows=N_COLS, knobs=tiled),
        _c("bag_rows-tiled-E0", "bag_fwd_rows", 0, 64, rows=N_COLS, knobs=tiled),
        _c("bag_rows-tiled-maxrows", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=BAG_MAXROWS, knobs=tiled),
        _c("bag_rows-tiled-maxrows+1", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=BAG_MAXROWS + 1, knobs=tiled),
        _c("bag_rows-tiled-rows1801", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS + 1, knobs=tiled),
        _c("bag_rows-tiled-H66", "bag_fwd_rows", E_LOCAL, 66, Z=Z_LOCAL, rows=N_COLS, knobs=tiled),
        _c("bag_rows-tiled-out+1", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, layout="out+1", knobs=tiled),
        _c("bag_rows-tiled-out+4", "bag_fwd_rows", E_LOCAL, 64, Z=Z_LOCAL, rows=N_COLS, layout="out+4", knobs=tiled),
        # the table gradient: Z = 0, 64 chunks, 4 MiB of gradient rows, classified or not, rows not given
        _c("bag_bwd-Z0", "bag_bwd_rows", 3, 256, Z=0, rows=3, graph="no_entries"),
        _c("bag_bwd-Z0-H10", "bag_bwd", 3, 10, Z=0, graph="no_entries"),
        _c("bag_bwd-tiny", "bag_bwd_rows", 3, 256, Z=5, rows=3, graph="bag_tiny"),
        _c("bag_bwd-tiny-H10", "bag_bwd_rows", 3, 10, Z=5, rows=3, graph="bag_tiny"),
        _c("bag_bwd-tiny-dz+1", "bag_bwd_rows", 3, 256, Z=5, rows=3, layout="dz+1", graph="bag_tiny"),
        _c("bag_bwd-tiny-partials@1", "bag_bwd_rows", 3, 256, Z=5, rows=3, layout="partials@1"),
        _c("bag_bwd-local", "bag_bwd_rows", E_LOCAL, 256, Z=Z_LOCAL, rows=E_LOCAL, graph="bag_local"),
        _c("bag_bwd-local-classified", "bag_bwd_rows", E_LOCAL, 256, Z=Z_LOCAL, rows=E_LOCAL, flags=("classified",), graph="bag_local"),
        _c("bag_bwd-local-dz+1", "bag_bwd_rows", E_LOCAL, 256, Z=Z_LOCAL, rows=E_LOCAL, layout="dz+1", graph="bag_local"),
        _c("bag_bwd-local-dz+1-classified", "bag_bwd_rows", E_LOCAL, 256, Z=Z_LOCAL, rows=E_LOCAL, layout="dz+1", flags=("classified",), graph="bag_local"),
        _c("bag_bwd-local-plain_entry", "bag_bwd", E_LOCAL, 256, Z=Z_LOCAL, graph="bag_local"),
        _c("bag_bwd-63chunks", "bag_bwd_rows", E_LOCAL, 256, Z=63 * BAG_CH, rows=E_LOCAL),
        _c("bag_bwd-64chunks", "bag_bwd_rows", E_LOCAL, 256, Z=63 * BAG_CH + 1, rows=E_LOCAL),
        _c("bag_bwd-4MiB", "bag_bwd_rows", 4096, 256, Z=Z_LOCAL, rows=4096),            # rows * H * 4 == 4 MiB: not larger
        _c("bag_bwd-4MiB+1row", "bag_bwd_rows", 4097, 256, Z=Z_LOCAL, rows=4097),
        _c("bag_bwd-rows0", "bag_bwd_rows", E_LOCAL, 256, Z=Z_LOCAL, rows=0),
        _c("bag_bwd-H5461", "bag_bwd", 3, 5461, Z=5),                                   # 3 * H * 4 = 65 532 <= 64 KiB
        _c("bag_bwd-H5462-refused", "bag_bwd", 3, 5462, Z=5),
        _c("classify-tiny", "classify", 3, 256, Z=5, rows=3, graph="bag_tiny"),
        _c("classify-tiny-counters", "classify", 3, 256, Z=5, rows=3, flags=("counters",)),
        _c("classify-local", "classify", E_LOCAL, 256, Z=Z_LOCAL, rows=E_LOCAL, graph="bag_local"),
        _c("classify-local-counters", "classify", E_LOCAL, 256, Z=Z_LOCAL, rows=E_LOCAL, flags=("counters",)),
        _c("classify-rows0", "classify", E_LOCAL, 256, Z=Z_LOCAL, rows=0),
    ]


def _embed():
    return [
        _c("embed-one_row", "embed_bwd", 37, 300, rows=1, graph="embed"),
        _c("embed-one_row-C64", "embed_bwd", 37, 64, rows=1),
        _c("embed-v4-C32", "embed_bwd", 37, 32, rows=5, graph="embed"),
        _c("embed-v4-C256", "embed_bwd", 37, 256, rows=5),
        _c("embed-C260", "embed_bwd", 37, 260, rows=5, graph="embed"),
        _c("embed-C30", "embed_bwd", 37, 30, rows=5),                   # CW = 32
        _c("embed-C1", "embed_bwd", 37, 1, rows=5),
        _c("embed-C257", "embed_bwd", 37, 257, rows=2),                 # CW capped at 256
        _c("embed-C32-g+1", "embed_bwd", 37, 32, rows=5, layout="g+1"),
        _c("embed-C32-dtable@1", "embed_bwd", 37, 32, rows=5, layout="dtable@1"),
        _c("embed-rows4096", "embed_bwd", 37, 32, rows=4096),
    ]


def _gineplus():
    out = []
    for N in (1, 8, 9, 8 * 512 + 1):
        for k in (1, 4):
            out.append(_c("gp_fwd-N%d-k%d" % (N, k), "gp_fwd", N, 64, k=k))
            out.append(_c("gp_bwd-N%d-k%d" % (N, k), "gp_bwd", N, 64, k=k, flags=("deps",)))
    out += [
        _c("gp_fwd-C64", "gp_fwd", 53, 64, k=3, graph="segments"),
        _c("gp_fwd-C66", "gp_fwd", 53, 66, k=3, graph="segments"),
        _c("gp_fwd-C64-x2+1", "gp_fwd", 9, 64, k=3, layout="x2+1"),
        _c("gp_fwd-C64-x3+1-beyond_k", "gp_fwd", 9, 64, k=3, layout="x3+1"),     # x3 is not read at k = 3: it constrains nothing
        _c("gp_fwd-C64-eps@1", "gp_fwd", 9, 64, k=2, layout="eps@1"),
        _c("gp_fwd-C64-no_e", "gp_fwd", 9, 64, k=2, absent=("e",)),
        _c("gp_bwd-C64", "gp_bwd", 53, 64, k=3, flags=("deps",), graph="segments"),
        _c("gp_bwd-C66", "gp_bwd", 53, 66, k=3, flags=("deps",), graph="segments"),
        _c("gp_bwd-C64-no_deps", "gp_bwd", 9, 64, k=3),
        _c("gp_bwd-C64-no_dx-no_d_e", "gp_bwd", 9, 64, k=3, absent=("dx", "d_e"), flags=("deps",)),
        _c("gp_bwd-C64-g+1", "gp_bwd", 9, 64, k=3, layout="g+1", flags=("deps",)),
        _c("gp_bwd-C64-d_e@1", "gp_bwd", 9, 64, k=3, layout="d_e@1", flags=("deps",)),
    ]
    return out


def _gated():
    return [_c("%s-C%d" % (e, C), e, 30, C, graph="molecule-30") for e in ("gated_fwd", "gated_bwd") for C in (4, 64, 68, 128, 132)]


CASES = _aggregate() + _bag() + _embed() + _gineplus() + _gated()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

FAMILIES = (
    "agg_fwd:wave2", "agg_fwd:wave4", "agg_fwd:wave1", "agg_fwd:elem", "agg_fwd:wave2+affine", "agg_fwd:wave4+affine", "agg_fwd:wave2+affine+span",
    "agg_bwd:wave2", "agg_bwd:wave4", "agg_bwd:wave1", "agg_bwd:wave2+affine", "agg_bwd:wave4+affine", "agg_bwd:wave4+affine+stats",
    "pool:v4", "pool:v1",
    "bag_fwd:row4", "bag_fwd:row1", "bag_fwd:row4+acc", "bag_fwd:row1+acc", "bag_fwd:tiled", "bag_fwd:tiled:acc", "bag_fwd:tiled:stats", "bag_fwd:none",
    "bag_bwd:none:v4", "bag_bwd:none:scalar", "bag_bwd:flat:v4", "bag_bwd:flat:scalar", "bag_bwd:local:v4", "bag_bwd:local:scalar",
    "bag_bwd:local:v4+classify", "bag_bwd:local:scalar+classify",
    "classify:none", "classify:launch", "classify:launch+classify",
    "embed_bwd:one_row", "embed_bwd:v4", "embed_bwd:generic",
    "gp_fwd:v4", "gp_fwd:v1", "gp_bwd:v4", "gp_bwd:v1",
    "gated_fwd:16", "gated_fwd:32", "gated_fwd:64", "gated_bwd:16", "gated_bwd:32", "gated_bwd:64",
)


def gpu_case_of(family):
    """the first table case with a structure to run on that reaches `family` under its own knobs (None: reached on the CPU only)"""
    for c in CASES:
        if c.graph is not None and family_of(c.entry, c) == family:
            return c
    return None
