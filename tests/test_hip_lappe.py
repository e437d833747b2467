"""The Laplacian positional encoding on the GPU (csrc/lappe.hip): esc_laplacian_eig through the op and the C ABI on every graph
of lappe_oracle.GRAPHS and on the list as one ragged batch under the sign- and basis-free comparison (i)-(vi) against
numpy.linalg.eigh in fp64, bit stability, limits and robustness, LapPETable against add_lap_pe, the DeepSet encoder's forward and
backward against the fp64 oracle, GPSModel(lap_pe=True) against the oracle model fed the device's own eigen-data, and the driver.

Error measure: max |got - want| over the largest |want| of the tensor, bound 1e-5 (the README's bound on predictions); a tensor
of zeros must be matched exactly.  The fp64 Jacobi solver's own error is about 1e-13 / gap with gaps >= 1e-3 between the clusters
the comparison tells apart (test_lappe_cpu checks them), so what is measured is the fp32 rounding of the output: about 1e-7.
torch's own fp32 evaluation of the encoder on the CPU is printed next to the kernel's figure."""
import math
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import lappe_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = lo.BOUND
K = lo.K_DEFAULT
NAMES = [g[0] for g in lo.GRAPHS]


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


_ALONE = {}


def alone(E, i):
    """(EigVals [n, K], EigVecs [n, K]) of graph i computed in a launch of its own: once, shared, never modified"""
    if i not in _ALONE:
        name, n, edges, _ = lo.GRAPHS[i]
        vals, vecs = E.ops.laplacian_eig(dev(edges), dev([0, n], torch.int64), dev([0, edges.shape[1]], torch.int64), K, max_nodes=n, num_nodes=n)
        assert vals.shape == (n, K, 1) and vecs.shape == (n, K) and vals.dtype == vecs.dtype == torch.float32
        _ALONE[i] = (vals.view(n, K), vecs)
    return _ALONE[i]


def raw_eig(E, edges, node_ptr, edge_ptr, N, max_nodes, k=K, local=0, fill=-7.0):
    """the C entry point on pre-filled outputs"""
    nv = E._native
    src, dst = dev(edges[0]), dev(edges[1])
    gp, ep = dev(node_ptr, torch.int64), dev(edge_ptr, torch.int64)
    vecs, vals = torch.full((N, k), fill, device=DEV), torch.full((N, k), fill, device=DEV)
    need = int(nv.lib().esc_laplacian_eig_scratch_bytes(N, max_nodes))
    scratch = torch.empty(max(need // 8, 1), dtype=torch.float64, device=DEV)
    nv.call("esc_laplacian_eig", nv.ptr(src), nv.ptr(dst), src.numel(), nv.ptr(gp), nv.ptr(ep), gp.numel() - 1, N, local, k, max_nodes,
            nv.ptr(scratch), need, nv.ptr(vecs), nv.ptr(vals), nv.stream())
    return vals, vecs


# ---- 1. the decomposition ---------------------------------------------------------------------------------------------------------
def test_limits_are_the_ones_the_oracle_assumes(E):
    assert E.ops.laplacian_eig_limits() == (lo.MAX_NODES, lo.LDS_NODES)
    h = E._native.lib()
    assert h.esc_laplacian_eig_scratch_bytes(1000, lo.LDS_NODES) == 0 and h.esc_laplacian_eig_scratch_bytes(1000, lo.LDS_NODES + 1) > 0


@pytest.mark.parametrize("i", range(len(lo.GRAPHS)), ids=NAMES)
def test_eigen_decomposition_of_every_graph(E, i):
    name, n, edges, _ = lo.GRAPHS[i]
    vals, vecs = alone(E, i)
    lo.compare(name, n, edges, vals.cpu().numpy(), vecs.cpu().numpy())
    again = E.ops.laplacian_eig(dev(edges), dev([0, n], torch.int32), dev([0, edges.shape[1]], torch.int32), K)     # int32 ranges, sizes read back
    assert torch.equal(bits(again[0].view(n, K)), bits(vals)) and torch.equal(bits(again[1]), bits(vecs)), "not bit-identical run to run"
    rv, rc = raw_eig(E, edges, [0, n], [0, edges.shape[1]], n, n)
    assert torch.equal(bits(rv), bits(vals)) and torch.equal(bits(rc), bits(vecs)), "the C entry point and the op differ"


def test_the_list_as_one_ragged_batch(E):
    """every graph inside the batch (an empty graph in the middle and at the end) is bit-equal to the same graph alone, on both
    storage paths; through the op and through the C ABI with graph-local edge ids"""
    last = len(lo.GRAPHS) - 1
    ei, gp, ep, sizes = lo.batch_of(lo.GRAPHS, empty_after=(6, last))
    assert sizes.count(0) == 2 and sizes[-1] == 0 and sizes[7] == 0
    N = int(gp[-1])
    vals, vecs = E.ops.laplacian_eig(dev(ei), dev(gp), dev(ep), K, max_nodes=lo.MAX_NODES, num_nodes=N)
    local = np.concatenate([g[2] for g in lo.GRAPHS], 1)
    lv, lc = raw_eig(E, local, gp, ep, N, lo.MAX_NODES, local=1)
    at, g = 0, 0
    for n in sizes:
        if n == 0:
            continue
        name, _, edges, _ = lo.GRAPHS[g]
        a_vals, a_vecs = alone(E, g)
        lo.compare("batch/" + name, n, edges, vals[at:at + n].cpu().numpy(), vecs[at:at + n].cpu().numpy())
        assert torch.equal(bits(vals[at:at + n].view(n, K)), bits(a_vals)) and torch.equal(bits(vecs[at:at + n]), bits(a_vecs)), name
        assert torch.equal(bits(lv[at:at + n]), bits(a_vals)) and torch.equal(bits(lc[at:at + n]), bits(a_vecs)), name + " (local ids)"
        at, g = at + n, g + 1
    assert at == N and g == len(lo.GRAPHS)


def test_other_numbers_of_frequencies(E):
    """K = 1, 3 and 32 on the Petersen graph and the molecule: more columns than nodes, and cuts at other places"""
    for gi in (NAMES.index("petersen"), NAMES.index("molecule-37")):
        name, n, edges, _ = lo.GRAPHS[gi]
        for k in (1, 3, 32):
            vals, vecs = E.ops.laplacian_eig(dev(edges), dev([0, n], torch.int64), dev([0, edges.shape[1]], torch.int64), k, max_nodes=n, num_nodes=n)
            lo.compare("%s K=%d" % (name, k), n, edges, vals.cpu().numpy(), vecs.cpu().numpy(), K=k)


# ---- 2. limits and robustness -----------------------------------------------------------------------------------------------------
def test_limits_are_refused_on_the_host(E):
    nv = E._native
    n = lo.MAX_NODES + 1
    edges = lo._both(lo._path(n))
    gp, ep = dev([0, n], torch.int64), dev([0, edges.shape[1]], torch.int64)
    with pytest.raises(RuntimeError, match="exceeds the limit of %d nodes" % lo.MAX_NODES):
        E.ops.laplacian_eig(dev(edges), gp, ep, K, max_nodes=n, num_nodes=n)
    with pytest.raises(RuntimeError, match="exceeds the limit of %d nodes" % lo.MAX_NODES):     # ... also when the op has to look itself
        E.ops.laplacian_eig(dev(edges), gp, ep, K)
    with pytest.raises(RuntimeError, match="limit of %d nodes" % lo.MAX_NODES):                 # the C entry point checks for itself
        raw_eig(E, edges, [0, n], [0, edges.shape[1]], n, n)
    small = lo._both(lo._path(9))
    sp, se = dev([0, 9], torch.int64), dev([0, 16], torch.int64)
    with pytest.raises(RuntimeError, match=r"max_freqs 33 outside 1\.\.32"):
        E.ops.laplacian_eig(dev(small), sp, se, 33, max_nodes=9, num_nodes=9)
    with pytest.raises(RuntimeError, match=r"max_freqs 33 outside 1\.\.32"):
        raw_eig(E, small, [0, 9], [0, 16], 9, 9, k=33)
    with pytest.raises(TypeError, match="int64"):
        E.ops.laplacian_eig(dev(small).to(torch.int32), sp, se, K, max_nodes=9, num_nodes=9)
    with pytest.raises(TypeError, match="int32 or int64"):
        E.ops.laplacian_eig(dev(small), sp.float(), se, K, max_nodes=9, num_nodes=9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.ops.laplacian_eig(torch.as_tensor(small), sp, se, K, max_nodes=9, num_nodes=9)
    big = lo.GRAPHS[NAMES.index("random-over-lds")]
    src = dev(big[2][0])
    with pytest.raises(RuntimeError, match="bytes of scratch"):                                  # too little scratch for the global path
        out = torch.empty((big[1], K), device=DEV)
        nv.call("esc_laplacian_eig", nv.ptr(src), nv.ptr(src), src.numel(), nv.ptr(dev([0, big[1]], torch.int64)),
                nv.ptr(dev([0, src.numel()], torch.int64)), 1, big[1], 0, K, big[1], None, 0, nv.ptr(out), nv.ptr(out), nv.stream())
    vals, vecs = E.ops.laplacian_eig(dev(small), sp, se, K, max_nodes=9, num_nodes=9)            # a valid call after the refusals is correct
    lo.compare("after the refusals", 9, small, vals.cpu().numpy(), vecs.cpu().numpy())


def test_a_graph_that_contradicts_the_host_is_skipped(E):
    """max_nodes understating one graph, an edge end outside its graph, and an edge range that leaves the edge list: that
    graph's rows keep the sentinel, the other graphs are correct"""
    pick = [lo.GRAPHS[NAMES.index(n)] for n in ("path-9", "cycle-12", "K5")]
    ei, gp, ep, sizes = lo.batch_of(pick)
    N = int(gp[-1])

    def check(vals, vecs, skipped):
        at = 0
        for g, (name, n, edges, _) in enumerate(pick):
            if g == skipped:
                assert bool((vals[at:at + n] == -7.0).all()) and bool((vecs[at:at + n] == -7.0).all()), name + " was written"
            else:
                lo.compare("beside a skipped graph/" + name, n, edges, vals[at:at + n].cpu().numpy(), vecs[at:at + n].cpu().numpy())
            at += n
    check(*raw_eig(E, ei, gp, ep, N, 9), skipped=1)                     # cycle-12 has 12 nodes, the host said 9
    bad = ei.copy()
    bad[1, int(ep[2]) + 3] = 2                                           # an edge of K5 ends in path-9
    check(*raw_eig(E, bad, gp, ep, N, 12), skipped=2)
    ep2 = ep.copy()
    ep2[3] = ei.shape[1] + 5                                             # K5's edge range leaves the list
    check(*raw_eig(E, ei, gp, ep2, N, 12), skipped=2)
    gp2 = gp.copy()
    gp2[1], gp2[2] = gp[2], gp[1]                                        # a negative node range (and one too wide for its edges)
    vals, vecs = raw_eig(E, ei, gp2, ep, N, 12)
    assert bool((vals[:int(gp[2])] == -7.0).all()) and bool((vecs[:int(gp[2])] == -7.0).all())


def test_nothing_to_do_is_legal(E):
    empty = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    for ptr in ([0], [0, 0], [0, 0, 0, 0]):
        vals, vecs = E.ops.laplacian_eig(empty, dev(ptr, torch.int64), dev(ptr, torch.int64), K, max_nodes=0, num_nodes=0)
        assert vals.shape == (0, K, 1) and vecs.shape == (0, K)
        vals, vecs = E.ops.laplacian_eig(empty, dev(ptr, torch.int32), dev(ptr, torch.int32), K)
        assert vals.shape == (0, K, 1) and vecs.shape == (0, K)
    nv = E._native
    nv.call("esc_laplacian_eig", None, None, 0, None, None, 0, 0, 0, K, 0, None, 0, None, None, nv.stream())


# ---- 3. the resident table --------------------------------------------------------------------------------------------------------
def test_table_attach_equals_add_lap_pe_on_the_collated_batch(E):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
    from esc_gnn_amd.lappe import LapPETable, add_lap_pe
    graphs = build_feature_dataset(synthetic_zinc_graphs(0, 6), 3, use_rd=True, self_loop=True)
    store = E.DeviceGraphStore(graphs, DEV)
    table = LapPETable(store, K)
    n_all = int(store.h_node_ptr[-1])
    assert table.eigvecs.shape == table.eigvals.shape == (n_all, K) and table.max_nodes == int((store.h_node_ptr[1:] - store.h_node_ptr[:-1]).max())
    ids = torch.tensor([4, 1, 1, 5, 0])
    batch = table.attach(store.collate(ids), ids)
    other = add_lap_pe(store.collate(ids), K)
    N = batch.x.size(0)
    assert batch.EigVals.shape == (N, K, 1) and batch.EigVecs.shape == (N, K)
    assert torch.equal(bits(batch.EigVals), bits(other.EigVals)) and torch.equal(bits(batch.EigVecs), bits(other.EigVecs))
    at = 0
    for g in ids.tolist():                                             # ... and it is the decomposition of those graphs
        n, edges = graphs[g].x.size(0), graphs[g].edge_index.numpy()
        lo.compare("store graph %d" % g, n, edges, batch.EigVals[at:at + n].cpu().numpy(), batch.EigVecs[at:at + n].cpu().numpy())
        at += n
    single = add_lap_pe(E.Data(x=graphs[2].x.to(DEV), edge_index=graphs[2].edge_index.to(DEV)), K)     # one graph, no batch vector
    a, b = int(store.h_node_ptr[2]), int(store.h_node_ptr[3])
    assert torch.equal(bits(single.EigVecs), bits(table.eigvecs[a:b])) and torch.equal(bits(single.EigVals.view(-1, K)), bits(table.eigvals[a:b]))
    for wrong in ([4, 1, 1, 5, 6], [4, 1, -1, 5, 0]):
        with pytest.raises(IndexError, match="graph id out of range"):
            table.attach(store.collate(ids), torch.tensor(wrong))
    with pytest.raises(ValueError, match="graph ids for a batch of"):
        table.attach(store.collate(ids), ids[:3])


@pytest.mark.parametrize("k", [1, 32])
def test_gather_of_two_tables_in_any_order(E, k):
    """the shared gather kernel with two tables: graphs of 1, 2 and 3 nodes whose rows hold their own flat index (the last
    graph's last row NaN, with a payload: compared as bits), gathered in reversed order with a repeat"""
    vecs_all = torch.arange(6 * k, dtype=torch.float32, device=DEV).view(6, k).clone()
    vals_all = -1.0 - vecs_all
    vecs_all.view(torch.int32)[5] = 0x7fc00123
    vals_all.view(torch.int32)[5] = 0x7fc00000
    ptr_all, ids, graph_ptr = dev([0, 1, 3, 6], torch.int64), [2, 0, 2], dev([0, 3, 4, 7], torch.int32)
    rows = torch.tensor([3, 4, 5, 0, 3, 4, 5], device=DEV)
    vals, vecs = E.ops.lappe_gather(vecs_all, vals_all, ptr_all, ids, graph_ptr, 7)
    assert vals.shape == (7, k, 1) and vecs.shape == (7, k)
    assert torch.equal(bits(vecs), bits(vecs_all[rows])) and torch.equal(bits(vals.view(7, k)), bits(vals_all[rows]))
    assert int(bits(vecs)[2, k - 1]) == 0x7fc00123 and int(bits(vecs)[6, 0]) == 0x7fc00123


# ---- 4. the encoder ---------------------------------------------------------------------------------------------------------------
_ENC = {}


def enc_case(k, p, n, signed, nan_rows=False):
    """inputs (fp32), upstream gradient cos(arange), and the oracle's output and parameter gradients in fp64 and in fp32 on the
    CPU: computed once per case, shared, never modified"""
    key = (k, p, n, signed, nan_rows)
    if key not in _ENC:
        gen = torch.Generator().manual_seed(1000 * k + 10 * p + n)
        if nan_rows:                                         # graphs of 1, 3 and 5 nodes at K = 8, then a row that is NaN throughout
            parts = [lo.lap_pe(m, lo._both(lo._path(m)), k) for m in (1, 3, 5)]
            vals = torch.cat([torch.from_numpy(a).float().view(-1, k) for a, _ in parts] + [torch.full((1, k), float("nan"))])
            vecs = torch.cat([torch.from_numpy(b).float() for _, b in parts] + [torch.full((1, k), float("nan"))])
            vals[1, 2] = float("nan")                        # an eigenvalue alone NaN: read as 0, the term stays
        else:
            vecs = torch.randn((n, k), generator=gen) * 0.3
            vals = torch.rand((n, k), generator=gen) * 4.0
        signs = (torch.where(torch.rand(k, generator=gen) >= 0.5, 1.0, -1.0) if signed else None)
        torch.manual_seed(77 + p)
        enc = lo.LapPEEncoder(p)
        for q in enc.parameters():
            torch.nn.init.normal_(q, std=0.7)
        gy = torch.cos(torch.arange(vecs.size(0) * p, dtype=torch.float64)).reshape(-1, p).float()
        res = []
        for dtype in (torch.float64, torch.float32):
            e = lo.LapPEEncoder(p).to(dtype)
            e.load_state_dict({a: b.to(dtype) for a, b in enc.state_dict().items()})
            out = e(vecs.to(dtype), vals.to(dtype), None if signs is None else signs.to(dtype))
            out.backward(gy.to(dtype))
            res.append((out.detach(), [q.grad for q in e.parameters()]))
        _ENC[key] = (vecs, vals, signs, [q.detach() for q in enc.parameters()], gy) + tuple(res)
    return _ENC[key]


def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    return err / scale if scale > 0 else (0.0 if err == 0 else math.inf)


def check(what, got, want64, want32):
    e, e32 = rel(got, want64), rel(want32, want64)
    print("%-44s kernel %.3g   torch fp32 on the CPU %.3g" % (what, e, e32))
    assert e <= BOUND, "%s: %.3g of the largest value, bound %g (torch fp32: %.3g)" % (what, e, BOUND, e32)


def run_encoder(E, case):
    vecs, vals, signs, params, gy = case[:5]
    ps = [q.to(DEV).requires_grad_(True) for q in params]
    out = E.ops.lappe_encode(vecs.to(DEV), vals.to(DEV), None if signs is None else signs.to(DEV), *ps)
    out.backward(gy.to(DEV))
    return out.detach(), [q.grad for q in ps]


PARAMS = ("linear_A.weight", "linear_A.bias", "pe_encoder.1.weight", "pe_encoder.1.bias")


@pytest.mark.parametrize("k,p", [(8, 8), (4, 4), (16, 16), (32, 32), (8, 12)])
def test_encoder_forward_and_backward_against_the_oracle(E, k, p):
    rows = E.ops.lappe_encode_block_rows()
    assert int(E._native.lib().esc_lappe_encode_scratch_floats(2 * rows + 1, p)) == 3 * (2 * p * p + 7 * p), "three backward partials"
    for n in (1, 3, 64, 65, 2 * rows + 1):
        for signed in (False, True):
            case = enc_case(k, p, n, signed)
            (o64, g64), (o32, g32) = case[5:]
            out, grads = run_encoder(E, case)
            name = "K %d P %d N %d %s " % (k, p, n, "signs" if signed else "plain")
            check(name + "out", out, o64, o32)
            for what, g, a, b in zip(PARAMS, grads, g64, g32):
                check(name + "d " + what, g, a, b)
            out2, grads2 = run_encoder(E, case)
            assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2)), "not bit-identical run to run"


def test_encoder_on_nan_padded_rows(E):
    """graphs of 1, 3 and 5 nodes at K = 8 (columns j >= n NaN) and a row that is NaN throughout: that row's output is exactly
    zero and it adds exactly nothing to the gradients"""
    for signed in (False, True):
        case = enc_case(8, 8, 10, signed, nan_rows=True)
        (o64, g64), (o32, g32) = case[5:]
        out, grads = run_encoder(E, case)
        check("NaN-padded out", out, o64, o32)
        for what, g, a, b in zip(PARAMS, grads, g64, g32):
            check("NaN-padded d " + what, g, a, b)
        assert out.shape == (10, 8) and not bool(out[9].any()) and bool(torch.isfinite(out).all())
        vecs, vals, signs, params, gy = case[:5]
        without = (vecs[:9], vals[:9], signs, params, gy[:9])
        out9, grads9 = run_encoder(E, without)
        assert torch.equal(out9, out[:9]) and all(torch.equal(a, b) for a, b in zip(grads, grads9)), "the NaN row changed a gradient"


def test_encoder_writes_a_column_slice_and_refuses_its_limits(E):
    nv = E._native
    case = enc_case(8, 8, 65, True)
    vecs, vals, signs, params, gy = (None if t is None else ([q.to(DEV) for q in t] if isinstance(t, list) else t.to(DEV)) for t in case[:5])
    out, _ = run_encoder(E, case)
    wide = torch.full((65, 8 + 20), -7.0, device=DEV)
    o = wide[:, 16:24]
    nv.call("esc_lappe_encode_fwd", nv.ptr(vecs), nv.ptr(vals), nv.ptr(signs), *[nv.ptr(q) for q in params], 65, 8, 8, o.data_ptr(),
            wide.stride(0), nv.stream())
    assert torch.equal(o, out) and bool((wide[:, :16] == -7.0).all()) and bool((wide[:, 24:] == -7.0).all())
    none = E.ops.lappe_encode(vecs[:0], vals[:0], signs, *[q.requires_grad_(True) for q in params])      # N == 0: zero gradients
    none.sum().backward()
    assert none.shape == (0, 8) and all(q.grad is not None and not bool(q.grad.any()) for q in params)
    for p in (6, 36):
        wA, bA, w1, b1 = (torch.zeros(s, device=DEV) for s in ((2 * p, 2), (2 * p,), (p, 2 * p), (p,)))
        with pytest.raises(RuntimeError, match="multiple of 4 and at most 32"):
            E.ops.lappe_encode(vecs, vals, signs, wA, bA, w1, b1)
        with pytest.raises(RuntimeError, match="multiple of 4 and at most 32"):
            nv.call("esc_lappe_encode_fwd", nv.ptr(vecs), nv.ptr(vals), None, nv.ptr(wA), nv.ptr(bA), nv.ptr(w1), nv.ptr(b1), 65, 8, p,
                    nv.ptr(wide), 28, nv.stream())
        with pytest.raises(RuntimeError, match="multiple of 4 and at most 32"):
            nv.call("esc_lappe_encode_bwd", nv.ptr(vecs), nv.ptr(vals), None, nv.ptr(wA), nv.ptr(bA), nv.ptr(w1), nv.ptr(b1), nv.ptr(wide), 28,
                    65, 8, p, nv.ptr(wide), 0, nv.ptr(wA), nv.ptr(bA), nv.ptr(w1), nv.ptr(b1), nv.stream())
    with pytest.raises(RuntimeError, match=r"max_freqs 33 outside 1\.\.32"):
        E.ops.lappe_encode(torch.zeros((4, 33), device=DEV), torch.zeros((4, 33), device=DEV), None, *params)
    with pytest.raises(RuntimeError, match="floats of scratch"):
        nv.call("esc_lappe_encode_bwd", nv.ptr(vecs), nv.ptr(vals), None, *[nv.ptr(q) for q in params], nv.ptr(gy), 8, 65, 8, 8, nv.ptr(wide), 5,
                *[nv.ptr(torch.empty_like(q)) for q in params], nv.stream())


# ---- 5. the model -----------------------------------------------------------------------------------------------------------------
def _close(a, b, what, tol):
    """the measure of test_hip_gps's model test: max error over max(1, largest value)"""
    a, b = a.detach().cpu().double(), b.detach().double()
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max()) / scale
    print("%-56s max scaled error %.3g" % (what, err))
    assert a.shape == b.shape and err <= tol, "%s: max scaled error %.3g > %g" % (what, err, tol)


def test_model_with_lap_pe_against_the_oracle_model(E):
    from esc_gnn_amd.datasets import build_feature_dataset, synthetic_zinc_graphs
    from esc_gnn_amd.gps_models import GPSModel
    from esc_gnn_amd.lappe import add_lap_pe
    graphs = build_feature_dataset(synthetic_zinc_graphs(0, 3), 3, use_rd=True, self_loop=True)
    torch.manual_seed(7)
    oracle = lo.GPSModel(layers=2, dim_hidden=64, n_heads=4)
    for m in oracle.modules():                             # weights that make every term count: biases and BatchNorm affine off their defaults
        if isinstance(m, torch.nn.BatchNorm1d):
            torch.nn.init.uniform_(m.weight, 0.5, 1.5)
            torch.nn.init.normal_(m.bias, std=0.1)
        if isinstance(m, torch.nn.MultiheadAttention):
            torch.nn.init.normal_(m.in_proj_bias, std=0.1)
            torch.nn.init.normal_(m.out_proj.bias, std=0.1)
    mine = GPSModel(layers=2, dim_hidden=64, n_heads=4, dropout=0.0, attn_dropout=0.0, lap_pe=True)
    mine.load_state_dict(oracle.state_dict())
    mine = mine.to(DEV)
    oracle = oracle.double()
    batch = add_lap_pe(E.Batch.from_data_list([g for g in graphs]).to(DEV))
    cpu = {k: batch[k].cpu() for k in ("x", "edge_index", "edge_attr", "pos_enc", "pos_index", "pos_batch", "batch", "EigVecs", "EigVals")}
    at = 0
    for g in graphs:                                       # the eigen-data the oracle is fed are the device's own - and they are right
        n = g.x.size(0)
        lo.compare("model batch", n, g.edge_index.numpy(), cpu["EigVals"][at:at + n].numpy(), cpu["EigVecs"][at:at + n].numpy())
        at += n
    signs = torch.tensor([1.0, -1, -1, 1, -1, 1, 1, -1])
    mine.encoder.node_encoder.encoder2.signs_override = signs
    y = torch.tensor([0.3, -1.1, 0.7], dtype=torch.float64).view(-1, 1)
    for mode in ("train", "eval"):
        getattr(oracle, mode)()
        getattr(mine, mode)()
        oracle.zero_grad()
        mine.zero_grad()
        want = oracle(cpu, signs)
        (want - y).abs().mean().backward()
        got = mine(batch)
        E.ops.l1_loss(got, y.float().to(DEV)).backward()
        _close(got, want, mode + " prediction", 1e-5)
        ref_p, ref_b = dict(oracle.named_parameters()), dict(oracle.named_buffers())
        unused = 0
        for n, p in mine.named_parameters():
            if ref_p[n].grad is None:                      # edge_attn_emb / edge_attn_linear: in the state_dict, not in the forward
                assert "edge_attn" in n and p.grad is None, n
                unused += 1
                continue
            _close(p.grad, ref_p[n].grad, mode + " grad " + n, 1e-4)
        assert unused == 2 * 7
        assert float(dict(mine.named_parameters())["encoder.node_encoder.encoder2.linear_A.weight"].grad.abs().max()) > 0
        for n, b in mine.named_buffers():
            _close(b, ref_b[n], mode + " buffer " + n, 1e-4)
    mine.encoder.node_encoder.encoder2.signs_override = None
    torch.manual_seed(3)
    mine.train()
    with torch.no_grad():
        a, b, c = mine(batch), mine(batch), mine(batch)
    assert not (torch.equal(a, b) and torch.equal(b, c)), "training draws the signs anew for every batch"
    mine.eval()
    with torch.no_grad():
        a, b = mine(batch), mine(batch)
    assert torch.equal(a, b), "evaluation applies no signs"
    bare = E.Batch.from_data_list([g for g in graphs]).to(DEV)
    with pytest.raises(ValueError, match="Precomputed eigen values and vectors are required"):
        mine(bare)


# ---- 6. the driver ----------------------------------------------------------------------------------------------------------------
def test_driver_trains_checkpoints_and_evaluates_with_lap_pe(tmp_path, monkeypatch, capsys):
    require_gpu()
    import esc_gnn_amd.run_zinc_gps as rg
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = "--synthetic_graphs 48 --layers 2 --batch_size 16"
    rg.main((common + " --posenc_LapPE 1 --epochs 2 --num_warmup_epochs 1 --save_appendix _pe").split())
    out = capsys.readouterr().out
    assert re.search(r"LapPE table build time cost: [\d.eE+-]+s", out), out
    lines = re.findall(r"Epoch: (\d+), LR: ([\d.eE+-]+), Loss: (\S+), Validation MAE: (\S+), Test MAE: (\S+), Test MAE norm: (\S+)", out)
    assert lines and all(math.isfinite(float(v.rstrip(","))) for line in lines for v in line[2:]), out
    ckpt = tmp_path / "results" / "zinc_GPS_pe" / "model_checkpoint2.pth"
    keys = set(torch.load(ckpt, map_location="cpu"))
    assert "encoder.node_encoder.encoder2.linear_A.weight" in keys and "encoder.node_encoder.encoder1.encoder.weight" in keys
    assert "encoder.node_encoder.encoder.weight" not in keys
    rg.main((common + " --posenc_LapPE 1 --eval 1 --save_appendix _pe --load_model %s" % ckpt).split())
    m = re.search(r"Test MAE: (\S+)", capsys.readouterr().out)
    assert m and math.isfinite(float(m.group(1)))
    rg.main((common + " --epochs 1 --num_warmup_epochs 1 --save_appendix _plain").split())
    capsys.readouterr()
    plain = tmp_path / "results" / "zinc_GPS_plain" / "model_checkpoint1.pth"
    assert "encoder.node_encoder.encoder.weight" in set(torch.load(plain, map_location="cpu"))
    with pytest.raises(RuntimeError, match="Missing key.*encoder.node_encoder.encoder1"):
        rg.main((common + " --posenc_LapPE 1 --eval 1 --save_appendix _pe --load_model %s" % plain).split())
