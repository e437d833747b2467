"""The step engines' schedule (esc-gnn_amd/csrc/engine_plan.h, host-only C++): tests/engine_schedule_host.cpp is compiled once with
the host compiler under AddressSanitizer and UBSan and asked, per (family, model sizes, batch sizes, run mode), for every decision
of the call.  The answers are held to the transcription in tests/engine_schedule_cases.py, and to properties that no table states:
the sums a producer leaves are consumed and fit bst_part, a Linear marked fused has a plan that serves it, the aggregate's stats
form is chosen only where its entry serves it, predict and SyncBN calls fuse nothing, the slab probe's position does not matter,
and the models the GPU suite runs reach every value the table reaches.  Runs no library code and needs no GPU."""
import json
import os
import subprocess

import pytest

import engine_cases as ec
import engine_schedule_cases as sc
from test_engine_plan_cpu import _host_compiler, _line

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "esc-gnn_amd", "csrc")


@pytest.fixture(scope="module")
def schedule_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("engine_schedule") / "engine_schedule_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "engine_schedule_host.cpp"), "-o", exe], check=True)
    return exe


def _bench_batches():
    """(N, E, G, Z) of one benchmark batch per family: bench.py's own setup (128 random regular graphs, h = 3) and its ZINC / OGB
    twins, as tests/golden/engine_workspace.json recorded them"""
    with open(os.path.join(HERE, "golden", "engine_workspace.json")) as fh:
        recs = json.load(fh)
    big = {r["family"]: (r["N"], r["E"], r["G"], r["Z"]) for r in recs if r["N"] > 1000}
    assert sorted(big) == ["count", "ogb", "zinc"] and big["count"][:2] == (2432, 15232)
    return big


def _batches(family):
    kind = "loops" if ec.SELF_LOOP[family] else "plain"
    out = [(ec.CLAIMS[c]["N"], ec.CLAIMS[c][kind][0], ec.CLAIMS[c]["G"], None) for c in sc.CASE_BATCHES]
    return out + [_bench_batches()[family]]


def _request(family, model, batch, mode, slab_off=0, misalign=0, agg_split_bwd=1):
    N, E, G, Z = batch
    if family == "count":
        L, H, C0 = model
        head = _line("count", L, H, N, E, G, Z=Z).split()
        head[3] = str(C0)
    elif family == "zinc":
        L, H, C0, nr = model
        head = _line("zinc", L, H, N, E, G, Z=Z, node_readout=nr).split()
        head[3] = str(C0)
    else:
        L, H, drop = model
        head = _line("ogb", L, H, N, E, G, Z=Z, drop=drop).split()
    return " ".join(head + [str(int(v)) for v in mode] + [str(slab_off), str(misalign), str(agg_split_bwd)])


def _expected(family, model, batch, mode, misalign=0, agg_split_bwd=1):
    N, E, G, _ = batch
    if family == "count":
        return sc.count(model[0], model[1], model[2], N, E, mode, misalign, agg_split_bwd)
    if family == "zinc":
        return sc.zinc(model[0], model[1], model[2], model[3], N, E, G, mode)
    return sc.ogb(model[0], model[1], model[2] / 1000.0, N, E, G, mode, misalign)


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [o for o in out if o]
    assert len(out) == len(lines)
    return [{k: ([] if v == "-" else [int(x) for x in v.split(",")]) for k, v in (t.split("=") for t in o.split())} for o in out]


def _table():
    """(family, model, batch, mode, misalign, agg_split_bwd): every model on every batch in every mode; the parameter groups off
    their alignment and the aggregate backward's split on the models they can change"""
    t = []
    for family, models in (("count", sc.COUNT_MODELS), ("zinc", sc.ZINC_MODELS), ("ogb", sc.OGB_MODELS)):
        for model in models:
            for batch in _batches(family):
                for mode in sc.MODES:
                    t.append((family, model, batch, mode, 0, 1))
    train = [m for m in sc.MODES if m.train and not m.sync]
    for model in ((3, 64, 10), (4, 256, 10)):
        for mode in train:
            for mis in (1, 2, 3):
                t.append(("count", model, _batches("count")[1], mode, mis, 1))
            t.append(("count", model, _batches("count")[1], mode, 0, 2))
    for mode in sc.MODES:                                    # the ESC bag's tiled forward on, at the benchmark batch (it needs 512 edges)
        t.append(("count", (4, 256, 10), _batches("count")[-1], mode, 8, 1))
    for model in ((2, 64, 500), (5, 300, 500)):
        for mode in train:
            for mis in (2, 4):
                t.append(("ogb", model, _batches("ogb")[1], mode, mis, 1))
    return t


@pytest.fixture(scope="module")
def answers(schedule_program):
    table = _table()
    return table, _ask(schedule_program, [_request(f, m, b, mode, 0, mis, asb) for f, m, b, mode, mis, asb in table])


def test_schedule_equals_its_transcription(answers):
    table, got = answers
    print("%d requests" % len(table))
    for row, g in zip(table, got):
        want = _expected(row[0], row[1], row[2], row[3], row[4], row[5])
        for k, v in want.items():
            assert g[k] == list(v), (row, k, g[k], v)
        assert set(g) == set(want) | {"agree", "entry"}, row


def test_sums_are_consumed_and_fit(answers):
    """Capacity: wherever a producer leaves column sums, the consuming MLP backward takes the fused form and the slot count fits
    the bst_part region of that layout; the producer's own form says so too (the aggregate's stats form <-> the MLP below it reads
    aggregate slots)"""
    table, got = answers
    left = 0
    for row, g in zip(table, got):
        cap = g["cap"][0]
        if row[0] == "ogb":
            assert g["hidden_slots"][0] <= cap, row
            continue
        L = row[1][0]
        for l in range(L):
            lin1, lin0, sums, slots = g["mlp%d" % l]
            assert lin1 or not lin0, row
            if sums != sc.OWN:
                left += 1
                assert lin1 and 0 < slots <= cap, (row, l)
            else:
                assert slots == 0, (row, l)
            assert (sums == sc.FROM_AGGREGATE) == (l + 1 < L and g["agg"][l + 1] == sc.AFFINE_STATS), (row, l)
            assert sums != sc.FROM_READOUT or (l == L - 1 and g["split"][0] and g["fuse_lin1"][0] and g["node_act"][0]), (row, l)
        assert g["xemb_bwd"][2:] == [sc.OWN, 0], row
        assert g["dx_split"][0] <= g["ask"][0] <= g["split"][0], row
    assert left > 1000


def test_fused_plans_agree_and_the_stats_form_is_served(answers):
    """Plans agree: every Linear marked fused has plan_both_bn(...).ok with the operands the body passes (the host program takes
    them again, the slab probe elsewhere).  Stats form: chosen only where deps_slots(C) == 1, C <= 2048 and the alignment of
    esc_gine_aggregate_bwd_affine_stats holds."""
    table, got = answers
    for row, g in zip(table, got):
        assert g["agree"] == [1] and g["entry"] == [1], row
        if row[0] == "count" and sc.AFFINE_STATS in g["agg"]:
            assert sc.agg_stats_served(row[1][1], row[5]), row
    assert any(sc.AFFINE_STATS in g["agg"] for g in got)


def test_the_stats_form_rule(schedule_program):
    widths = (64, 256, 2048, 2052, 4096)
    got = _ask_numbers(schedule_program, ["aggstats %d %d" % (C, k) for k in (1, 2) for C in widths])
    assert got == [1, 1, 1, 0, 0, 1, 0, 1, 0, 0]
    assert got == [int(sc.agg_stats_served(C, k)) for k in (1, 2) for C in widths]


def _ask_numbers(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split()
    return [int(v) for v in out]


BACKWARD_KEYS = ("split", "fuse_lin1", "ask", "dx_split", "last_dw", "agg", "xemb_bwd", "hidden", "hidden_slots", "bonds_on_node", "drop_h", "drop_v",
                 "drop_z1", "drop_z0")
PAIR_KEYS = ("zlin", "xemb", "conv0", "conv1", "readout", "lin0", "lin1", "vlin0", "vlin1")


def test_predict_and_sync_modes(answers):
    """Predict mode has no backward decision and every pair on eval coefficients.  With sync there is no merged epilogue and no
    fused backward."""
    table, got = answers
    for row, g in zip(table, got):
        mode = row[3]
        backward = [v for k in g for v in g[k] if k in BACKWARD_KEYS or k.startswith("mlp")]
        pairs = [v for k in PAIR_KEYS if k in g for v in g[k]]
        if not mode.train:
            assert not any(backward) and set(pairs) == {sc.EVAL}, row
        if mode.sync:
            assert sc.MERGED not in pairs and g.get("bag", [0]) == [0], row
            fused = [g[k][i] for k in g if k.startswith("mlp") or k == "xemb_bwd" for i in (0, 1)]
            assert not any(fused + g.get("fuse_lin1", []) + g.get("hidden", []) + g.get("drop_h", []) + g.get("drop_z1", []) + g.get("ask", [])), row
            assert sc.AFFINE_STATS not in g.get("agg", []), row
        elif row[4] & 8 and mode.train:
            assert g["bag"] == [128], row


def test_slab_probe_position_does_not_matter(schedule_program, answers):
    """Alignment independence: the bodies used to probe the plans with the slab cursor wherever it stood; every region is a multiple
    of 64 floats, so the schedule, which probes the start of the region, answers the same from any later round64 offset"""
    table, got = answers
    rows = [(r, g) for r, g in zip(table, got) if r[3].train and r[0] != "zinc"][::7]
    for off in (64, 64 * 12345, 64 * 3 + 64 * 2 ** 20):
        again = _ask(schedule_program, [_request(f, m, b, mode, off, mis, asb) for (f, m, b, mode, mis, asb), _ in rows])
        assert again == [g for _, g in rows], off


# ---- coverage: what the GPU suite runs reaches every value the table reaches -------------------------------------------------
# The models of tests/test_hip_engine_structure.py (ec.MODELS, ec.DEEP, SCHEDULE_MODELS; the structure module itself needs the
# library) on both of its SCHEDULES, through train_step, forward_train + backward and predict, with the event and readout switches
# of tests/test_hip_step_schedule.py and tests/test_hip_readout_backward.py; and the OGB model with dropout that
# tests/test_hip_engine_families.py trains.
GPU_COUNT = ((3, 64, 10), (1, 32, 10), (14, 64, 10), (15, 64, 10), (2, 64, 10))
GPU_ZINC = ((2, 256, 32, 0), (16, 256, 32, 0))
GPU_OGB = ((2, 32, 0), (10, 64, 0), (2, 64, 0), (2, 32, 300))
MAX_REDUCE_JOBS = 48
# Two exceptions, by name: `sync` (needs a collective over more than one rank: the table's sync modes are left out of the
# comparison) and `e0_early == false` (needs in_dim > 32, and the case data is 10 wide).


def _gpu_modes(jobs):
    deferred_main = jobs <= MAX_REDUCE_JOBS
    for two in (False, True):
        for plain in (False, True):
            for one in (False, True):
                yield sc.Mode(True, two, deferred_main, False, True, plain, one)           # train_step
                yield sc.Mode(True, two, True, False, False, plain, one)                   # forward_train (its job list is never filled)
                yield sc.Mode(True, two, deferred_main, False, False, plain, one)          # backward
                yield sc.Mode(False, two, False, False, False, plain, one)                 # predict


def _reached(rows):
    """{(key, value)} over the enum / flag fields (slot counts and capacities are sizes, not decisions)"""
    seen = set()
    for family, g in rows:
        for k, vs in g.items():
            if k in ("cap", "hidden_slots", "agree", "entry", "bag"):
                continue
            key = (family, "mlp" if k.startswith("mlp") else k)
            for i, v in enumerate(vs):
                if key[1] in ("mlp", "xemb_bwd") and i == 3:
                    continue
                seen.add(key + (((i,) if key[1] in ("mlp", "xemb_bwd") else ()) + (v if key[1] != "behind" else int(v >= 0),)))
    return seen


def test_gpu_suite_reaches_every_value(schedule_program, answers):
    table, got = answers
    reached_by_table = _reached((r[0], g) for r, g in zip(table, got) if not r[3].sync and r[4] == 0 and r[5] == 1 and (r[3].train or not any(r[3][2:5])))
    lines, fams = [], []
    for family, models, jobs in (("count", GPU_COUNT, lambda m: 3 * m[0] + 6), ("zinc", GPU_ZINC, lambda m: 3 * m[0] + 3), ("ogb", GPU_OGB, lambda m: 5 * m[0])):
        for model in models:
            for batch in _batches(family)[:-1]:
                for mode in _gpu_modes(jobs(model)):
                    lines.append(_request(family, model, batch, mode))
                    fams.append(family)
    reached_by_gpu = _reached(zip(fams, _ask(schedule_program, lines)))
    missing = reached_by_table - reached_by_gpu
    allowed = {m for m in missing if m[:2] == ("count", "e0") and m[-1] == 0}          # e0_early == false: needs in_dim > 32, the case data is 10 wide
    # ... and what follows from it alone: term 0 launched on its own (behind the pack, or up front on one stream)
    allowed |= {m for m in missing if m[:2] == ("count", "up") and m[-1] == 1 and ("count", "up", 1) in reached_by_gpu}
    print("table reaches %d values, the GPU suite's models %d; unreached: %s" % (len(reached_by_table), len(reached_by_gpu), sorted(missing)))
    assert missing <= allowed, sorted(missing - allowed)
