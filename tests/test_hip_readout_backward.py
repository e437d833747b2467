"""The readout Linear's edge-stream block of the two-stream backward goes out as two launches of the fused kernel — the dX tiles
first, at one workgroup per CU, then the dW tiles — and the node chain waits for the first only (DESIGN.md *Step engine, readout
backward*).  The tiles, the slabs and every reduction are those of the one launch, so everything must agree with it bit for bit:
at op level (esc_tune_set knob 14 asks esc_linear_bwd_both_bn for the two launches) on the block's shape class at its smallest,
and over three training steps of small counting models (esc_engine_set_side_stream bit 7 keeps the one launch, bit 6 the event
records — among them the one in front of the block, which is otherwise the stop event of esc_bn_bwd_coef's last launch)."""
import ctypes

import pytest
import torch

from conftest import require_gpu
from test_hip_step_schedule import _engine_steps, _store

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = 14                                   # esc_tune_set: plan::PlanKnobs::dual_split
NEW, ONE_LAUNCH, RECORDS = 2, 2 | 128, 2 | 64          # esc_engine_set_side_stream


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


@pytest.fixture
def knobs():
    """always back to the library's defaults, whatever a test set"""
    from esc_gnn_amd import _native as nv
    yield nv
    nv.call("esc_tune_set", KNOB, 0)
    nv.call("esc_engine_set_side_stream", NEW)
    nv.call("esc_engine_set_two_stream_min_edges", 12000)


def _chk(got, want, what, tol=1e-5):
    got, want = got.detach().cpu().double(), want.detach().double()
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max()) / scale
    assert err <= tol, "%s: max error %.3g of scale %.3g > %g" % (what, err, scale, tol)


class _Call:
    """one esc_linear_bwd_both_bn call of the block's shape class: X a column slice at offset 128 of a wider buffer, the
    BatchNorm+ReLU prologue on it, ReLU behind the BatchNorm whose backward is folded in, no accumulation, no `next`"""

    def __init__(self, nv, M, N, K, off=128, pad=136):
        self.nv, self.M, self.N, self.K = nv, M, N, K
        dev = torch.device(DEV)
        torch.manual_seed(M * 7 + N + K)
        self.xb = (torch.randn(M, N) * 1.5 + 0.3).to(dev)
        self.gamma, self.beta = (torch.rand(N) + 0.5).to(dev), (torch.randn(N) * 0.3).to(dev)
        self.dOut = torch.randn(M, N).to(dev)
        self.ldx = K + pad
        self.Xw = torch.randn(M, self.ldx).to(dev)
        self.X = self.Xw[:, off:off + K]
        self.W = (torch.randn(N, K) / K ** 0.5).to(dev)
        self.isc, self.ish = (torch.rand(K) + 0.5).to(dev), (torch.randn(K) * 0.2).to(dev)
        scratch = torch.empty(nv.lib().esc_bn_scratch(max(N, K)), device=dev)
        self.st = [torch.empty(N, device=dev) for _ in range(4)]           # mean, invstd, scale, shift
        nv.call("esc_bn_stats", nv.ptr(self.xb), N, M, N, 1e-5, 0.1, nv.ptr(self.st[0]), nv.ptr(self.st[1]), None, None, nv.ptr(self.gamma),
                nv.ptr(self.beta), nv.ptr(self.st[2]), nv.ptr(self.st[3]), nv.ptr(scratch), nv.stream())
        self.coef, dg, db = torch.empty(N, 2, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
        nv.call("esc_bn_bwd_coef", nv.ptr(self.xb), N, None, 0, nv.ptr(self.dOut), N, M, N, nv.ptr(self.st[0]), nv.ptr(self.st[1]),
                nv.ptr(self.gamma), nv.ptr(self.beta), 1, nv.ptr(self.coef), nv.ptr(dg), nv.ptr(db), nv.ptr(scratch), nv.stream())
        self.f = nv.BnBwdFused()
        f = self.f
        f.x, f.ld_x, f.mean, f.invstd, f.scale, f.shift, f.coef, f.relu = (self.xb.data_ptr(), N, self.st[0].data_ptr(), self.st[1].data_ptr(),
                                                                          self.st[2].data_ptr(), self.st[3].data_ptr(), self.coef.data_ptr(), 1)
        self.slab_n = int(nv.lib().esc_linear_bwd_weight_scratch(M, N, K))

    def ok(self, X=None):
        nv, M, N, K = self.nv, self.M, self.N, self.K
        dX, slabs = torch.empty(M, K, device=DEV), torch.empty(self.slab_n, device=DEV)
        return nv.lib().esc_linear_bwd_both_bn_ok(nv.ptr(self.dOut), N, ctypes.byref(self.f), nv.ptr(self.X if X is None else X), self.ldx, nv.ptr(self.W), K,
                                                  M, N, K, nv.ptr(dX), K, nv.ptr(slabs), None)

    def run(self):
        nv, M, N, K = self.nv, self.M, self.N, self.K
        slabs = torch.full((self.slab_n,), float("nan"), device=DEV)
        dX, dW, db = (torch.full((M, K), float("nan"), device=DEV), torch.full((N, K), float("nan"), device=DEV),
                      torch.full((N,), float("nan"), device=DEV))
        nv.call("esc_linear_bwd_both_bn", nv.ptr(self.dOut), N, ctypes.byref(self.f), nv.ptr(self.X), self.ldx, nv.ptr(self.isc), nv.ptr(self.ish),
                nv.ptr(self.W), K, M, N, K, nv.ptr(dX), K, 0, nv.ptr(dW), K, nv.ptr(db), nv.ptr(slabs), None, None, nv.stream())
        torch.cuda.synchronize()
        return dX, dW, db

    def fp64(self):
        xb64 = self.xb.double().cpu().requires_grad_(True)
        y = torch.nn.functional.batch_norm(xb64, None, None, self.gamma.double().cpu(), self.beta.double().cpu(), True, 0.1, 1e-5).relu()
        y.backward(self.dOut.double().cpu())
        dY = xb64.grad
        Xa = torch.relu(self.X.double().cpu() * self.isc.double().cpu() + self.ish.double().cpu())
        return dY @ self.W.double().cpu(), dY.t() @ Xa


# rows under one 64- and one 128-row tile, exactly one, one plus a two-row remainder, several with a remainder; one and three
# column tiles of dX
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("M", [96, 128, 130, 300])
def test_two_launches_equal_the_one_launch_bitwise(E, knobs, M, K):
    nv, N = knobs, 128
    call = _Call(nv, M, N, K)
    assert call.ok() == 1
    one = call.run()
    want_dX, want_dW = call.fp64()
    scale_of = lambda t: max(1.0, float(t.abs().max()))
    for request in (1, 84 * 1024, 160 * 1024):          # two launches; the dX launch at one workgroup per CU; at the whole LDS
        try:
            nv.call("esc_tune_set", KNOB, request)
            assert call.ok() == 1
            two = call.run()
        finally:
            nv.call("esc_tune_set", KNOB, 0)
        for a, b, name in zip(two, one, ("dX", "dW", "db")):
            assert not bool(torch.isnan(a).any()), (request, name)
            assert float((a - b).abs().max()) <= 2e-5 * scale_of(b), (request, name, float((a - b).abs().max()), scale_of(b))
            assert torch.equal(a, b), (request, name, int((a != b).sum()))
        _chk(two[0], want_dX, "dX vs fp64 (request %d)" % request)
        _chk(two[1], want_dW, "dW vs fp64 (request %d)" % request, tol=2e-5)
    assert torch.equal(call.run()[0], one[0])           # the knob is back: the one launch again


def test_calls_the_fused_tiles_do_not_serve_are_not_changed_by_the_request(E, knobs):
    nv = knobs
    narrow = _Call(nv, 300, 128, 10, off=0, pad=8)           # the tiny-K kernels: served, by their own launches
    wide = _Call(nv, 300, 96, 128)                           # N = 96: the 64-wide fused tile either way
    unaligned = _Call(nv, 130, 128, 128)
    off = [c.run() for c in (narrow, wide)]
    assert unaligned.ok(unaligned.Xw[:, 129:257]) == 0       # X not 16-byte aligned: refused with and without the request
    try:
        nv.call("esc_tune_set", KNOB, 84 * 1024)
        on = [c.run() for c in (narrow, wide)]
        assert unaligned.ok(unaligned.Xw[:, 129:257]) == 0
    finally:
        nv.call("esc_tune_set", KNOB, 0)
    for a3, b3 in zip(on, off):
        for a, b in zip(a3, b3):
            assert torch.equal(a, b)
    _chk(on[1][0], wide.fp64()[0], "dX vs fp64 (N = 96)")


@pytest.mark.parametrize("L,bs", [(2, 6), (1, 4)], ids=["L2_H128_bs6", "L1_H128_bs4"])
@pytest.mark.parametrize("other", [ONE_LAUNCH, RECORDS], ids=["one_launch_bit7", "event_records_bit6"])
def test_three_training_steps_agree_bitwise(E, knobs, L, bs, other):
    """begin_step -> next collate -> end_step -> FlatAdam.step, three times from the same seed, two streams forced: loss, flat_grad,
    flat_param and every BatchNorm buffer are torch.equal after every step"""
    H = 128
    store = _store(E, bs, False)
    new, _ = _engine_steps(E, knobs, store, bs, L, H, NEW, 0)
    old, _ = _engine_steps(E, knobs, store, bs, L, H, other, 0)
    for i, ((lo, go, po, bo), (ln, gn, pn, bn)) in enumerate(zip(old, new)):
        assert bool(torch.isfinite(ln).all()) and bool(torch.isfinite(gn).all()), i
        assert float(gn.abs().max()) > 0.0, i
        assert torch.equal(lo, ln), (i, float(lo), float(ln))
        assert torch.equal(go, gn), (i, int((go != gn).sum()))
        assert torch.equal(po, pn), (i, int((po != pn).sum()))
        assert len(bo) == len(bn) and all(torch.equal(a, c) for a, c in zip(bo, bn)), i
