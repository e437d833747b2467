"""The one-launch GINE+ aggregate (csrc/gineplus.hip: gp_fwd_wave, gp_bwd_wave, gp_deps_reduce) and the MultihopPlan that
feeds it (multihop.py) on every schedule, branch and edge: the cases of tests/gineplus_cases.py.

out, every dx_t and d_e have a bit contract (the header comment of gineplus.hip) and are held BIT-EXACT to the sequential numpy
loops of gineplus_cases, which read the pairs and never a plan, and which the CPU suite ties to fp64 and to single-threaded
index_add_.  d_eps is summed in the kernels' own fixed order and is held to fp64 by a bound derived from that order
(gineplus_cases.deps_depth).  One GPU run per (case, k, width) is shared by the tests that look at it."""

import numpy as np
import pytest
import torch

from conftest import require_gpu
import gineplus_cases as gp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 777.25                                     # what padding columns and rows hold before a kernel runs
WIDTHS = (4, 7)
DEGREE_WIDTHS = (1, 64, 65, 68, 256, 260, 300)    # scalar C = 1 | one vector pass less | scalar, two passes | ragged vector pass |
#                                                   exactly one vector pass | a second pass with one live lane | the model's width
RUNS = [(name, k, C) for name in gp.CASE_NAMES for k in gp.ks_of(name) for C in WIDTHS]
RUNS += [("degrees", k, C) for k in gp.ks_of("degrees") for C in DEGREE_WIDTHS]
_ids = lambda runs: ["%s-k%d-C%d" % r for r in runs]


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    torch.set_num_threads(1)
    return esc_gnn_amd


def _graph(E, n, ei):
    return E.Data(x=torch.zeros(n, dtype=torch.int64), edge_index=torch.as_tensor(ei).reshape(2, -1), num_nodes=n)


def _build(E, c, k=None):
    """(multihop_edge_index, distance, MultihopPlan) of a case on the device, by the path its `source` names"""
    from esc_gnn_amd.multihop import MultihopPlan, expand_multihop
    from esc_gnn_amd.subgraphs import collate_graphs
    k = c["k"] if k is None else k
    if c["source"] == "tensors":
        mei, dist = torch.from_numpy(c["pairs"]).to(DEV), torch.from_numpy(c["distance"]).to(DEV)
        return mei, dist, MultihopPlan.from_tensors(mei, dist, c["num_nodes"], k)
    return expand_multihop(collate_graphs([_graph(E, n, ei) for n, ei in c["graphs"]], DEV), k)


_PLANS = {}


def _plan(E, name):
    """the plan of a case at the case's k (shared; never modified)"""
    if name not in _PLANS:
        _PLANS[name] = _build(E, gp.case(name))
    return _PLANS[name][2]


def _place(t, offset):
    """offset None: contiguous on the device; else a column slice `offset` floats into rows of 2C + 8 floats"""
    if offset is None:
        return t.to(DEV)
    base = torch.full((t.size(0) + 1, 2 * t.size(1) + 8), SENT, device=DEV)
    assert base.data_ptr() % 16 == 0
    view = base[:t.size(0), offset:offset + t.size(1)]
    view.copy_(t)
    return view.detach()


def _run(E, plan, xs, e, eps, g, offset=None, grads=None):
    """the fused op forward and backward; grads: the names of the leaves that require a gradient (default: all).  Returns
    (out, [dx_t], d_e, d_eps) on the CPU, None where no gradient was asked for"""
    k = len(xs)
    names = ["x%d" % t for t in range(k)] + ["e", "eps"]
    grads = set(names) if grads is None else set(grads)
    xs = [_place(x, offset).requires_grad_("x%d" % t in grads) for t, x in enumerate(xs)]
    e, eps = _place(e, offset).requires_grad_("e" in grads), eps.to(DEV).requires_grad_("eps" in grads)
    out = E.ops.gineplus_aggregate(xs, e, eps, plan)
    out.backward(_place(g, offset))
    cpu = lambda t: None if t is None else t.cpu()
    return out.detach().cpu(), [cpu(x.grad) for x in xs], cpu(e.grad), cpu(eps.grad)


_GPU = {}


def _gpu(E, name, k, C):
    """the contiguous all-gradients run of one (case, k, width): once"""
    if (name, k, C) not in _GPU:
        r = gp.reference(name, k, C)
        _GPU[(name, k, C)] = _run(E, _plan(E, name), r["xs"], r["e"], r["eps"], r["g"])
    return _GPU[(name, k, C)]


def _same(got, want, what):
    assert got is not None and got.shape == want.shape and got.dtype == want.dtype, what
    if not torch.equal(got, want):
        bad = (got != want) | (torch.signbit(got) != torch.signbit(want))
        rows = sorted(set(bad.nonzero()[:, 0].tolist()))
        raise AssertionError("%s: %d elements in %d rows differ (first rows %s), largest difference %.3g"
                             % (what, int(bad.sum()), len(rows), rows[:8], float((got - want).abs().max())))
    assert torch.equal(torch.signbit(got), torch.signbit(want)), what + ": the sign of a zero"


def _positive_zero(t):
    return float(t.abs().sum()) == 0.0 and not bool(torch.signbit(t).any())


# ---- 1. the plan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gp.CASE_NAMES)
def test_plan_is_the_stable_grouping(E, name):
    """meta, out_ptr, in_ptr, in_meta and num_d1 of the plan against a stable CPU sort of the pairs: (row, col) order, ascending
    source inside a destination, equal pairs in input order; the rank follows the INPUT order of the distance-1 pairs for
    from_tensors, their (row, col) order for expand_multihop (where the two are one: the expansion is the input), -1 elsewhere"""
    c = gp.case(name)
    plan = _plan(E, name)
    mei, dist = _PLANS[name][0], _PLANS[name][1]
    assert mei.dtype == torch.int64 and dist.dtype == torch.int64
    assert np.array_equal(mei.cpu().numpy(), c["pairs"]) and np.array_equal(dist.cpu().numpy(), c["distance"])
    want = gp.plan_arrays(c)
    for key, arr in want.items():
        got = getattr(plan, key).cpu().numpy()
        assert got.dtype == arr.dtype and got.shape == arr.shape and np.array_equal(got, arr), "%s: plan.%s" % (name, key)
    assert plan.num_d1 == gp.num_d1(c) and plan.num_pairs == len(c["distance"]) and plan.num_nodes == c["num_nodes"] and plan.k == c["k"]
    meta, in_meta = plan.meta.cpu().numpy().astype(np.int64), plan.in_meta.cpu().numpy().astype(np.int64)
    n = c["num_nodes"]
    assert bool((np.diff(meta[:, 0] * n + meta[:, 1]) >= 0).all()), "(row, col) order"
    assert bool((np.diff(in_meta[:, 1] * n + in_meta[:, 0]) >= 0).all()), "by destination, ascending source inside"
    d1 = meta[:, 2] == 1
    assert bool((meta[~d1, 3] == -1).all()) and sorted(meta[d1, 3].tolist()) == list(range(int(d1.sum())))
    if c["source"] == "expand":
        assert np.array_equal(meta[d1, 3], np.arange(int(d1.sum()))), "rank in (row, col) order"
        assert not hasattr(plan, "status") or int(plan.status.abs().sum()) == 0
    else:
        pos = np.flatnonzero(c["distance"] == 1)                    # the m-th distance-1 pair of the input is row m of e
        assert np.array_equal(meta[d1][np.argsort(meta[d1, 3]), :2], c["pairs"][:, pos].T), "rank in input order"


def test_backward_schedule_of_the_row_cases(E):
    """the workgroup counts that the rows_N cases are there for: 1, 2, 3, 4 (groups of gp_deps_reduce left empty), 32, 33 (its
    second trip) and 512 with one, two and three rows per wave"""
    blocks = E._native.lib().esc_gineplus_bwd_blocks
    assert [int(blocks(n)) for n in gp.ROWS_N] == [1, 2, 3, 4, 32, 33, 512, 512, 512] == [gp.bwd_blocks(n) for n in gp.ROWS_N]
    assert int(blocks(0)) == 1 and int(blocks(1)) == 1


# ---- 2. bits against the specification -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k,C", RUNS, ids=_ids(RUNS))
def test_bits_against_the_sequential_specification(E, name, k, C):
    """out, every dx_t and d_e: torch.equal with the numpy loops, the sign of every zero included"""
    r = gp.reference(name, k, C)
    out, dx, d_e, d_eps = _gpu(E, name, k, C)
    tag = "%s k=%d C=%d " % (name, k, C)
    _same(out, r["out"], tag + "out")
    for t in range(k):
        _same(dx[t], r["dx"][t], tag + "dx_%d" % t)
    _same(d_e, r["d_e"], tag + "d_e")
    assert tuple(d_e.shape) == (gp.num_d1(gp.case(name)), C)
    assert bool(torch.isfinite(d_eps).all())


# ---- 3. d_eps ---------------------------------------------------------------------------------------------------------------
def _deps_ratios(name, k, C, d_eps):
    """worst |error| / bound of the kernel's d_eps and of a torch fp32 CPU evaluation, per d, and the depths"""
    c, r = gp.case(name), gp.reference(name, k, C)
    bound = gp.deps_bound(c, k, r["mag"])
    out, _, _, leps = gp.aggregate_torch(c, k, r["xs"], r["e"], r["eps"], torch.float32)
    out.backward(r["g"])

    def ratio(v):
        err = (v.double() - r["d_eps"]).abs()
        assert bool((err[bound == 0] == 0).all()), "%s k=%d C=%d: d_eps without a term must be exactly 0" % (name, k, C)
        return float((err[bound > 0] / bound[bound > 0]).max()) if bool((bound > 0).any()) else 0.0
    return ratio(d_eps), ratio(leps.grad), gp.deps_depth(c, k)


@pytest.mark.parametrize("name,k,C", RUNS, ids=_ids(RUNS))
def test_deps_within_the_bound_of_its_summation_order(E, name, k, C):
    """|d_eps - fp64| <= depth * 2^-24 * sum |terms| per column and distance, the sum of magnitudes taken from the fp64
    reference.  depth counts the fp32 roundings between a term and the result on the longest path of the kernels' fixed order;
    each rounding moves what passes through it by at most 2^-24 of its size, so a term that meets `depth` of them is off by at
    most depth * 2^-24 of itself (to first order), and the sum of the terms by that share of the sum of their magnitudes.

    The path (csrc/gineplus.hip), with P = esc_gineplus_bwd_blocks(N) workgroups of 8 waves and R = ceil(N / 8P) rows per wave:
      * roundings inside one term and along the wave's rows.  d = 0: dep = fma(g, x_0, dep), one rounding per row: R.  d = 1: the
        message x_0 + e is rounded once, then dep = fma(g, relu(msg), dep) once per distance-1 pair of the wave's rows: 1 + the
        largest number of such pairs that one wave meets.  d >= 2: accU = accU + g over the n pairs of the row at that distance,
        starting from +0, so the first add is exact: n - 1 for the longest row; then dep = fma(relu(x), accU, dep) once per
        row: R.
      * the 8 waves of a workgroup are added in LDS in wave order: wave 0's partial meets 7 adds.
      * gp_deps_reduce: group 0 adds ceil(P / 4) partial rows to +0, the first exactly: ceil(P / 4) - 1.
      * the groups are added in order; a group without a row holds +0, which adds exactly: min(3, P - 1).
    For the directed paths of rows_N at k = 2 that is [R + t, 1 + R + t, R + t] with t = 7 + ceil(P / 4) - 1 + min(3, P - 1):

        N       P     R   depth (d = 0, 1, 2)   kernel / bound   torch fp32 on the CPU / bound   (worst of C = 4 and 7, MI355X)
        8       1     1     8    9    8          0.253            0.253
        9       2     1     9   10    9          0.147            0.147
        24      3     1    10   11   10          0.114            0.110
        25      4     1    11   12   11          0.095            0.115
        256     32    1    18   19   18          0.020            0.036
        264     33    1    19   20   19          0.020            0.023
        4096    512   1   138  139  138          0.0037           0.0013
        4097    512   2   139  140  139          0.0020           0.0010
        8195    512   3   140  141  140          0.0008           0.0012

    (the bound is a worst case, the errors of a sum of N terms of mixed sign grow like sqrt(N): the ratio falls with N.  What the
    bound is there to catch is a lost or doubled term, which at N = 8195 is about ten times the bound.)
    The torch fp32 CPU figure is printed beside the kernel's: it is the yardstick for what an fp32 sum of these terms achieves,
    and were it to break the bound the derivation would be wrong, not the factor."""
    _, _, _, d_eps = _gpu(E, name, k, C)
    assert tuple(d_eps.shape) == (k + 1, C) and d_eps.dtype == torch.float32
    mine, cpu, depth = _deps_ratios(name, k, C, d_eps)
    print("%s k=%d C=%d d_eps: depth %s, worst error / bound: kernel %.4f, torch fp32 on the CPU %.4f" % (name, k, C, depth, mine, cpu))
    assert mine <= 1.0, "%s k=%d C=%d d_eps: error %.4f x the bound of depth %s (torch fp32 on the CPU: %.4f x)" % (name, k, C, mine, depth, cpu)


def test_deps_is_bit_stable_run_to_run(E):
    name, k, C = "rows_8195", 2, 7
    r = gp.reference(name, k, C)
    first = _gpu(E, name, k, C)
    for _ in range(2):
        again = _run(E, _plan(E, name), r["xs"], r["e"], r["eps"], r["g"])
        assert torch.equal(again[3], first[3]) and torch.equal(torch.signbit(again[3]), torch.signbit(first[3]))


# ---- 4. null-output branches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grads", [("x0", "x1", "x2", "eps"), ("x0", "x1", "x2", "e"), ("x0", "x1", "x2"), ("x1", "e", "eps"), ("x0",), ("x2",),
                                   ("e",), ("eps",)], ids=lambda g: "+".join(g))
def test_gradients_that_are_not_asked_for(E, grads):
    """requires_grad off for e (d_e NULL with M1 > 0), for eps (no partials: the LDS reduction and its barriers are skipped), for
    both, and for all but one operand: what is still produced has the bits of the all-on run, the rest is None"""
    name, k, C = "degrees", 3, 64
    r = gp.reference(name, k, C)
    full = _gpu(E, name, k, C)
    out, dx, d_e, d_eps = _run(E, _plan(E, name), r["xs"], r["e"], r["eps"], r["g"], grads=grads)
    _same(out, full[0], "out")
    for t in range(k):
        if "x%d" % t in grads:
            _same(dx[t], full[1][t], "dx_%d with %s" % (t, grads))
        else:
            assert dx[t] is None
    for key, got, want in (("e", d_e, full[2]), ("eps", d_eps, full[3])):
        if key in grads:
            _same(got, want, "d_%s with %s" % (key, grads))
            assert not bool(torch.isnan(got).any())
        else:
            assert got is None
    assert not bool(torch.isnan(out).any()) and not any(bool(torch.isnan(d).any()) for d in dx if d is not None)


# ---- 5. alignment, leading dimensions, padding -----------------------------------------------------------------------------
@pytest.mark.parametrize("C,offset", [(64, 4), (300, 4), (64, 1), (68, 3), (7, 4)])
def test_column_slices_of_wider_buffers(E, C, offset):
    """every row operand and the output gradient as a column slice of rows of 2C + 8 floats: 16 bytes in (offset 4, the vector
    path for C % 4 == 0) and 4 or 12 bytes in (a base that is not 16-byte aligned: the scalar kernel, although C % 4 == 0).
    All give the bits of the contiguous run"""
    name, k = "degrees", 3
    r = gp.reference(name, k, C)
    probe = _place(r["xs"][0], offset)
    assert probe.data_ptr() % 16 == (4 * offset) % 16 and probe.stride(0) == 2 * C + 8
    full = _gpu(E, name, k, C)
    out, dx, d_e, d_eps = _run(E, _plan(E, name), r["xs"], r["e"], r["eps"], r["g"], offset=offset)
    what = "C=%d, %d bytes in: " % (C, 4 * offset)
    _same(out, full[0], what + "out")
    for t in range(k):
        _same(dx[t], full[1][t], what + "dx_%d" % t)
    _same(d_e, full[2], what + "d_e")
    _same(d_eps, full[3], what + "d_eps")


@pytest.mark.parametrize("C", [64, 7])
def test_forward_into_padded_rows(E, C):
    """esc_gineplus_aggregate_fwd itself with ld_out = C + 4 into a buffer full of a sentinel: the slice has the bits, every
    padding column and the row after the last are untouched"""
    nv = E._native
    name, k = "degrees", 3
    c, r, plan = gp.case(name), gp.reference(name, k, C), _plan(E, name)
    N, M1, ld = c["num_nodes"], gp.num_d1(c), C + 4
    xs = [x.to(DEV) for x in r["xs"]]
    e, eps = r["e"].to(DEV), r["eps"].to(DEV)
    buf = torch.full((N + 1, ld), SENT, device=DEV)
    nv.call("esc_gineplus_aggregate_fwd", nv.ptr(xs[0]), C, nv.ptr(xs[1]), C, nv.ptr(xs[2]), C, None, 0, nv.ptr(e), C, nv.ptr(plan.in_ptr),
            nv.ptr(plan.in_meta), nv.ptr(eps), N, C, k, M1, nv.ptr(buf), ld, nv.stream())
    got = buf.cpu()
    _same(got[:N, :C].contiguous(), r["out"], "ld_out = C + 4, C=%d" % C)
    assert bool((got[:, C:] == SENT).all()) and bool((got[N:] == SENT).all()), "the kernel wrote outside its rows"


# ---- 6. a plan wider than the call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_plan_that_covers_more_distances_than_the_call(E, k):
    """the k = 4 plan of `degrees` (which also holds the class 5) under 1, 2 and 3 row operands against a plan of the pairs of
    distance <= k alone: the pairs keep their relative order and only their positions change, so every result has the same bits"""
    name, C = "degrees", 64
    r = gp.reference(name, k, C)
    wide = _gpu(E, name, k, C)
    sub = gp.restricted(gp.case(name), k)
    assert sub["pairs"].shape[1] < gp.case(name)["pairs"].shape[1] and gp.num_d1(sub) == gp.num_d1(gp.case(name))
    mei, dist, plan = _build(E, sub)
    assert plan.k == k < _plan(E, name).k
    out, dx, d_e, d_eps = _run(E, plan, r["xs"], r["e"], r["eps"], r["g"])
    _same(out, wide[0], "k=%d out" % k)
    for t in range(k):
        _same(dx[t], wide[1][t], "k=%d dx_%d" % (k, t))
    _same(d_e, wide[2], "k=%d d_e" % k)
    _same(d_eps, wide[3], "k=%d d_eps" % k)


# ---- 7. alone against inside the batch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
def test_graph_alone_has_the_bits_of_its_rows_in_the_batch(E, C):
    """every graph of `segments` expanded and run alone: out, dx_t and d_e are its rows of the batch's results (d_eps sums over
    the batch and is left out).  An edgeless graph alone has no pair at all; inside the batch it keeps its diagonal"""
    from esc_gnn_amd.multihop import expand_multihop
    from esc_gnn_amd.subgraphs import collate_graphs
    name = "segments"
    c = gp.case(name)
    k = c["k"]
    r = gp.reference(name, k, C)
    out, dx, d_e, _ = _gpu(E, name, k, C)
    for g, ((n0, n1), (r0, r1)) in enumerate(zip(c["node_ranges"], c["d1_ranges"])):
        n, ei = c["graphs"][g]
        mei, dist, plan = expand_multihop(collate_graphs([_graph(E, n, ei)], DEV), k)
        assert plan.num_d1 == r1 - r0 and plan.num_nodes == n1 - n0
        a_out, a_dx, a_de, _ = _run(E, plan, [x[n0:n1] for x in r["xs"]], r["e"][r0:r1], r["eps"], r["g"][n0:n1])
        what = "graph %d of %d nodes, C=%d: " % (g, n, C)
        _same(a_out, out[n0:n1], what + "out")
        for t in range(k):
            _same(a_dx[t], dx[t][n0:n1], what + "dx_%d" % t)
        _same(a_de, d_e[r0:r1], what + "d_e")


# ---- 8. ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
def test_relu_gate_is_strictly_positive(E, C):
    """`ties`: through a pair whose message is exactly +0 or -0 the gradient is exactly +0; through a source whose x_t is +0, -0
    or a negative subnormal the gradient is exactly +0; and those pairs add exactly nothing to the forward"""
    name, k = "ties", 4
    c, r = gp.case(name), gp.reference(name, k, C)
    out, dx, d_e, _ = _gpu(E, name, k, C)
    rank = gp.grouping(c)[0]
    row, dist = c["pairs"][0], c["distance"]
    keep = np.ones(len(dist), dtype=bool)
    for p in c["cancel_pairs"] + c["negzero_pairs"]:
        assert _positive_zero(d_e[rank[p]]), "d_e of pair %d, whose message is 0: %s" % (p, d_e[rank[p]].tolist())
        keep[p] = False
    for t, nodes in c["dead_sources"].items():
        for node, v in nodes:
            assert _positive_zero(dx[t][node]), "dx_%d of node %d, whose x_%d is %r: %s" % (t, node, t, v, dx[t][node].tolist())
            keep[(row == node) & (dist == t + 1)] = False
    assert int((~keep).sum()) >= 6 + 9
    _same(out, gp.forward_loop(c, k, r["xs"], r["e"], r["eps"], keep=torch.from_numpy(keep).tolist()), "the forward without the tied pairs")
