"""tests/engine_cases.py on the CPU: every case is what it claims to be (N, E, G, in-degrees, N % 64), and the fp32 oracle is
well conditioned on it — its own error against the fp64 oracle stays under the cap for predictions, loss, every gradient
and every BatchNorm buffer, so that the relative bound of tests/test_hip_engine_structure.py (3x that error) cannot hide a
failure.  `zero_variance` is the one case where it is not, which is why the device test holds it to less."""
import math

import numpy as np
import pytest
import torch

import engine_cases as ec

FAMILIES = ("count", "zinc", "ogb")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", ec.CASE_NAMES)
def test_structure_is_as_claimed(family, case):
    b = ec.oracle_batch(family, case)
    claim = ec.CLAIMS[case]
    kind = "loops" if ec.SELF_LOOP[family] else "plain"
    if case == "zero_variance":
        c = claim[kind]
        N, G, E, (lo, hi) = c["N"], c["G"], c["E"], c["deg"]
    else:
        N, G, (E, lo, hi) = claim["N"], claim["G"], claim[kind]
    src, dst = b["edge_index"]
    deg = torch.bincount(dst, minlength=N)
    assert (b["x"].size(0), b["num_graphs"], b["edge_index"].size(1)) == (N, G, E)
    assert (int(deg.min()), int(deg.max())) == (lo, hi)
    assert int(b["batch"][-1]) + 1 == G and bool((b["batch"][1:] >= b["batch"][:-1]).all())
    assert bool((b["batch"][src] == b["batch"][dst]).all())
    assert bool(((src == dst).sum() == (N if ec.SELF_LOOP[family] else 0)))
    assert N >= 2 and E >= 2 and G >= 2                       # what the engines state as their minimum
    # every edge owns histogram entries (the bag has no empty row), in edge order
    assert int(b["pos_batch"][-1]) == E - 1 and len(torch.unique(b["pos_batch"])) == E
    assert bool((b["pos_batch"][1:] >= b["pos_batch"][:-1]).all())
    if case.startswith("rows_"):
        want = int(case.split("_")[1])
        assert N == want and N % 64 == want % 64 and N % 4 in (0, 1)
    if case.startswith("mixed"):
        counts = torch.bincount(b["batch"]).tolist()
        per_graph_edges = torch.bincount(b["batch"][dst], minlength=G).tolist()
        assert sorted(counts) == [1, 1, 2, 5, 6, 7, 41]
        if case == "mixed_edgeless_last":
            assert counts[-1] == 6 and (ec.SELF_LOOP[family] or per_graph_edges[-1] == 0)
        if case == "mixed_hub_last":
            assert counts[-1] == 41 and int(deg.argmax()) == N - 41
    if case == "sparse_edges" and not ec.SELF_LOOP[family]:
        assert E < N
    if case == "hub65":
        assert hi > 64                                          # one more than a wave of in-edges


def test_claims_of_the_issue_table():
    """the figures the case table was specified with"""
    c = ec.CLAIMS
    assert (c["mixed"]["N"], c["mixed"]["loops"][0], c["mixed"]["plain"][0], c["mixed"]["plain"][1]) == (63, 156, 93, 0)
    assert (c["minimal"]["N"], c["minimal"]["loops"][0], c["minimal"]["plain"][0]) == (5, 11, 6)
    assert (c["hub65"]["N"], c["hub65"]["plain"][2], c["hub65"]["loops"][2]) == (71, 65, 66)
    assert (c["sparse_edges"]["N"], c["sparse_edges"]["loops"][0], c["sparse_edges"]["plain"][0]) == (70, 73, 3)
    assert [c["rows_%d" % n]["N"] for n in (64, 65, 129)] == [64, 65, 129]


@pytest.mark.parametrize("model", ec.MODELS, ids=ec.model_id)
@pytest.mark.parametrize("case", ec.CASE_NAMES)
def test_fp32_oracle_is_conditioned(model, case):
    family, L, H = model
    step = ec.oracle_step(family, case, L, H)
    e_ref = ec.reference_errors(step)
    for side in ("fp32", "fp64"):
        for n, t in ec.float_items(step[side]):
            assert bool(torch.isfinite(t).all()), (side, n)
        assert len(step[side]["grads"]) == len(step["state"]) - len(step[side]["buffers"])      # every parameter has one
        assert all(int(t) == 1 for n, t in step[side]["buffers"].items() if n.endswith("num_batches_tracked"))
    grads = {n: e for n, e in e_ref.items() if n.startswith("grad:")}
    bufs = {n: e for n, e in e_ref.items() if n.startswith("buf:")}
    worst_g, worst_b = max(grads, key=grads.get), max(bufs, key=bufs.get)
    print("%s %s: e_ref pred %.2g loss %.2g eval %.2g worst gradient %.2g (%s) worst buffer %.2g (%s)"
          % (ec.model_id(model), case, e_ref["pred"], e_ref["loss"], e_ref["eval_pred"], grads[worst_g], worst_g[5:],
             bufs[worst_b], worst_b[4:]))
    if case == "zero_variance":
        # every BatchNorm column has zero batch variance: the gradients through it are rounding noise amplified by
        # eps^-1/2 = 316, and the fp32 oracle cannot produce them
        assert grads[worst_g] > ec.CAP, (worst_g, grads[worst_g])
        return
    for n, e in e_ref.items():
        assert e <= ec.CAP, (n, e)


@pytest.mark.parametrize("deep", ec.DEEP, ids=lambda d: "%s-%s" % (ec.model_id(d[:3]), d[3]))
def test_fp32_oracle_is_conditioned_on_the_deep_models(deep):
    """ec.DEEP: the same cap for the models whose weight gradients do not fit one reduce launch (and the last one that does)"""
    family, L, H, case = deep
    step = ec.oracle_step(family, case, L, H)
    e_ref = ec.reference_errors(step)
    for side in ("fp32", "fp64"):
        assert all(bool(torch.isfinite(t).all()) for n, t in ec.float_items(step[side])), side
        assert len(step[side]["grads"]) == len(step["state"]) - len(step[side]["buffers"])
    worst = max(e_ref, key=e_ref.get)
    print("%s %s: worst e_ref %.2g (%s)" % (ec.model_id(deep[:3]), case, e_ref[worst], worst))
    for n, e in e_ref.items():
        assert e <= ec.CAP, (n, e)


# tests/test_hip_engine_structure.py SCHEDULE_MODELS x SCHEDULE_CASES (that module needs the library: the pairs are repeated here)
SCHEDULE_ON_CASE = ((("count", 2, 64), "mixed"), (("count", 2, 64), "minimal"), (("count", 2, 64), "rows_65"),
                    (("ogb", 2, 64), "mixed"), (("ogb", 2, 64), "mixed_hub_last"))


@pytest.mark.parametrize("model,case", SCHEDULE_ON_CASE, ids=["%s-%s" % (ec.model_id(m), c) for m, c in SCHEDULE_ON_CASE])
def test_fp32_oracle_is_conditioned_on_the_schedule_models(model, case):
    """the same cap for the models added for the step schedule's coverage, on the cases the device test runs them on"""
    family, L, H = model
    step = ec.oracle_step(family, case, L, H)
    e_ref = ec.reference_errors(step)
    for side in ("fp32", "fp64"):
        assert all(bool(torch.isfinite(t).all()) for n, t in ec.float_items(step[side])), side
        assert len(step[side]["grads"]) == len(step["state"]) - len(step[side]["buffers"])
    worst = max(e_ref, key=e_ref.get)
    print("%s %s: worst e_ref %.2g (%s)" % (ec.model_id(model), case, e_ref[worst], worst))
    for n, e in e_ref.items():
        assert e <= ec.CAP, (n, e)


@pytest.mark.parametrize("family", ("zinc", "ogb"))
def test_single_graph_boundary_oracle(family):
    """G = 1, one path(3): the ZINC reference skips bn_lin1 at one row and trains; the OGB reference cannot train (its
    virtual-node MLP normalises over the graphs: torch refuses one row), so the device test compares it in eval mode"""
    _, L, H = next(m for m in ec.MODELS if m[0] == family)
    b = ec.oracle_batch(family, "single_path3")
    assert (b["num_graphs"], b["x"].size(0), b["edge_index"].size(1)) == (1, 3, 7 if ec.SELF_LOOP[family] else 4)
    if family == "zinc":
        step = ec.oracle_step(family, "single_path3", L, H)
        e_ref = ec.reference_errors(step)
        print("zinc single_path3: worst e_ref %.2g" % max(e_ref.values()))
        assert max(e_ref.values()) <= ec.CAP
        # bn_lin1 was skipped: its statistics are untouched
        assert int(step["fp32"]["buffers"]["bn_lin1.num_batches_tracked"]) == 0
    else:
        ref = ec.reference_model(family, L, H).train()
        with pytest.raises(ValueError, match="more than 1 value per channel"):
            ec._forward(family, ref, b, False)
        step = ec.oracle_step(family, "single_path3", L, H, train=False)
        assert ec.reference_errors(step)["eval_pred"] <= ec.CAP


def test_error_measure_and_bound():
    t = torch.tensor([0.5, -4.0], dtype=torch.float64)
    assert ec.error(torch.tensor([0.5, -4.0]), t) == 0.0
    assert math.isclose(ec.error(torch.tensor([0.5, -3.0]), t), 0.25)          # over the largest |fp64 value|
    assert math.isclose(ec.error(torch.tensor([0.25]), torch.tensor([0.5], dtype=torch.float64)), 0.25)   # over 1 below it
    assert ec.bound(0.0) == 1e-5 and ec.bound(1e-4) == pytest.approx(3e-4)
    assert np.isfinite(ec.CAP) and ec.CAP == 1e-3
