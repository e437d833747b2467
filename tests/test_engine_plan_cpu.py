"""The step engines' host plan (esc-gnn_amd/csrc/engine_plan.h, host-only C++): tests/engine_plan_host.cpp is compiled once with the
host compiler under AddressSanitizer and UBSan and asked, per (family, model sizes, batch sizes), for the workspace totals, the
slab budget, the job count and the list of weight gradients the budget and the count derive from.  The list is held against the
nn.Linear modules of the oracle's reference model, a SlabCursor over the budget against the list, and the totals against the
parent commit's (tests/golden/engine_workspace.json: the sizes and what esc_*_workspace_floats answered before the plan header
existed, taken from that library through ctypes with descriptors that carry only the sizes).  Runs no library code and needs no
GPU."""
import collections
import glob
import json
import os
import shutil
import subprocess

import pytest
import torch

import engine_cases as ec
import ref_model as rm

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "esc-gnn_amd", "csrc")
MAX_REDUCE_JOBS = 48                                     # ESC_MAX_REDUCE_JOBS
MODELS = ec.MODELS + tuple(m[:3] for m in ec.DEEP)
COUNT_IN, ZINC_NODE, ZINC_EDGE, OGB_TASKS = 10, 32, 32, 1      # widths of the reference models (engine_cases.raw_graphs, ref_model)
Answer = collections.namedtuple("Answer", "train predict slabs jobs walked over grads")


def _host_compiler():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = [shutil.which("g++")] + sorted(glob.glob(os.path.join(rocm, "llvm", "bin", "clang++"))) + sorted(glob.glob(os.path.join(rocm, "lib", "llvm", "bin", "clang++")))
    found = [c for c in found if c]
    assert found, "no host C++ compiler (g++ or ROCm's clang++)"
    return found[0]


@pytest.fixture(scope="session")
def plan_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("engine_plan") / "engine_plan_host")
    subprocess.run([_host_compiler(), "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-I", CSRC,
                    os.path.join(HERE, "engine_plan_host.cpp"), "-o", exe], check=True)
    return exe


def _line(family, L, H, N, E, G, Z=None, drop=0, node_readout=0, atom_rows=None, bond_rows=None, atom_entries=None, bond_entries=None):
    abc = {"count": (COUNT_IN, 0, 0), "zinc": (ZINC_NODE, ZINC_EDGE, node_readout),
           "ogb": (OGB_TASKS, atom_rows or sum(rm.ATOM_FEATURE_DIMS), bond_rows or sum(rm.BOND_FEATURE_DIMS))}[family]
    return "%s %d %d %d %d %d %d  %d %d %d %d %d %d" % ((family, L, H) + abc + (drop, N, E, 12 * E if Z is None else Z, G,
                                                          9 * N if atom_entries is None else atom_entries,
                                                          3 * E if bond_entries is None else bond_entries))


def _ask(exe, lines):
    out = subprocess.run([exe], input="\n".join(lines) + "\n", stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout.split("\n")
    out = [[int(v) for v in o.split()] for o in out if o]
    assert len(out) == len(lines)
    for o in out:
        assert len(o) == 7 + 3 * o[6]
    return [Answer(*o[:6], grads=[tuple(o[7 + 3 * i:10 + 3 * i]) for i in range(o[6])]) for o in out]


def _sizes(family, case):
    c = ec.CLAIMS[case]
    return c["N"], c["loops" if ec.SELF_LOOP[family] else "plain"][0], c["G"]


@pytest.mark.parametrize("model", MODELS, ids=ec.model_id)
def test_the_list_is_the_reference_models_linears(plan_program, model):
    """(out_dim, in_dim) of the listed weight gradients = weight.shape of the nn.Linear modules of the reference model, one entry
    per module and NO module absent; the counting model's lin1 [H, (L+1)*H] counts as its column blocks [H, L*H] and [H, H].  The
    rows of every entry are the batch's nodes, edges or graphs, and the job count is the list's length."""
    family, L, H = model
    N, E, G = 61, 157, 7
    a, = _ask(plan_program, [_line(family, L, H, N, E, G)])
    want = collections.Counter()
    for name, mod in ec.reference_model(family, L, H).named_modules():
        if isinstance(mod, torch.nn.Linear):
            out_dim, in_dim = mod.weight.shape
            if family == "count" and name == "lin1":
                assert (out_dim, in_dim) == (H, (L + 1) * H)
                want[(H, L * H)] += 1
                want[(H, H)] += 1
            else:
                want[(out_dim, in_dim)] += 1
    assert collections.Counter((n, k) for _, n, k in a.grads) == want
    assert a.jobs == len(a.grads) == {"count": 3 * L + 6, "zinc": 3 * L + 3, "ogb": 5 * L}[family]
    assert all(m in (N, E, G) for m, _, _ in a.grads)
    assert sum(m == E for m, _, _ in a.grads) == L + 1                      # the edge pipeline's: one per layer and z_embedding's
    # which depths defer their reduces (one launch of at most MAX_REDUCE_JOBS jobs)
    assert (a.jobs <= MAX_REDUCE_JOBS) == {"count": L <= 14, "zinc": L <= 15, "ogb": L <= 9}[family]


def test_slab_cursor_stays_inside_the_budget(plan_program):
    """the whole list through a SlabCursor over slab_floats(list), the counting readout split and whole: never refused, every
    region 256-byte aligned and where peek() said.  The walk ends exactly at the limit, and one further take of any listed shape
    is refused and moves nothing — in the form of the counting readout that sets the budget (the larger of the two); the other
    form leaves their difference unused, and there every listed shape that does not fit that remainder is refused."""
    asked = []
    for H in (4, 8, 12, 16, 32, 64, 256, 300):
        for L in (1, 2, 3, 13, 14, 15, 16):
            for rows in (2, 31, 32, 33, 127, 128, 129, 4097):
                asked.append(_line("count", L, H, rows, 2 * rows + 1, 2))
                asked.append(_line("count", L, H, 2 * rows + 1, rows, 2))
                asked.append(_line("ogb", L, H, rows, 2 * rows + 1, max(2, rows // 9), atom_rows=174, bond_rows=13))
                asked.append(_line("zinc", L, H, rows, 2 * rows + 1, max(2, rows // 9)))
                asked.append(_line("zinc", L, H, rows, 2 * rows + 1, 2, node_readout=1))
    for line, a in zip(asked, _ask(plan_program, asked)):
        assert a.walked == 1 and a.over == 1, line
        assert a.slabs % 64 == 0 and a.slabs > 0 and a.jobs == len(a.grads), line
        assert a.predict < a.train and a.slabs < a.train, line


def test_totals_do_not_exceed_the_parents(plan_program):
    """train totals <= what esc_*_workspace_floats answered at the parent commit, predict < train: ec.MODELS and the deep models
    at the `mixed` / `minimal` sizes and one benchmark-sized batch per family"""
    with open(os.path.join(HERE, "golden", "engine_workspace.json")) as fh:
        recs = json.load(fh)
    seen = {(r["family"], r["L"], r["H"]) for r in recs}
    assert all(m in seen for m in MODELS) and len(seen) == len(MODELS) + 3
    for m in MODELS:
        for case in ("mixed", "minimal"):
            N, E, G = _sizes(m[0], case)
            assert any((r["family"], r["L"], r["H"], r["N"], r["E"], r["G"]) == m + (N, E, G) for r in recs), (m, case)
    lines = []
    for r in recs:
        if r["family"] == "count":
            assert r["in_dim"] == COUNT_IN
        elif r["family"] == "zinc":
            assert (r["node_dim"], r["edge_dim"]) == (ZINC_NODE, ZINC_EDGE)
        else:
            assert r["num_tasks"] == OGB_TASKS
        lines.append(_line(r["family"], r["L"], r["H"], r["N"], r["E"], r["G"], Z=r["Z"], node_readout=r.get("node_readout", 0),
                           atom_rows=r.get("atom_rows"), bond_rows=r.get("bond_rows"), atom_entries=r.get("atom_entries"),
                           bond_entries=r.get("bond_entries")))
    for r, a in zip(recs, _ask(plan_program, lines)):
        pad = 0 if r["family"] == "count" else 64                 # esc_zinc_ / esc_ogb_workspace_floats add 64 to the layout's total
        print("%s L%d H%d N%d E%d: train %d (parent %d), predict %d, slabs %d, %d jobs"
              % (r["family"], r["L"], r["H"], r["N"], r["E"], a.train + pad, r["parent_workspace_floats"], a.predict, a.slabs, a.jobs))
        assert a.predict < a.train, r
        assert a.train + pad <= r["parent_workspace_floats"], r
        assert a.walked == 1 and a.over == 1, r
