"""The expressiveness runs on the MI355X: the classification head (csrc/classify.hip: log-softmax, NLL loss with accuracy
count, the fused training head, pairwise distances) against torch in fp64, the NestedGIN of run_sr / run_exp against the
reference golden (tests/golden/model_expressive.npz) and the fp64 oracle on the two real-graph fixtures, and the two drivers.

Tolerances are measured, not constants: an output may be as far from the fp64 result as 3x the error of torch's own CPU
fp32 kernel on the same input, floored at one fp32 ulp of the largest magnitude involved."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT, require_gpu
import expressive_oracle as eo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "model_expressive.npz"))


def _ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


def _check(what, mine, ref32, ref64, floor_at):
    """|mine - ref64| <= max(3 * |ref32 - ref64|, one fp32 ulp of floor_at); every figure is printed before the assertion"""
    ref64 = ref64.detach().double()
    e_mine = float((mine.detach().cpu().double() - ref64).abs().max()) if ref64.numel() else 0.0
    e_ref = float((ref32.detach().double() - ref64).abs().max()) if ref64.numel() else 0.0
    tol = max(3.0 * e_ref, _ulp(floor_at))
    print("%s: error %.3g, torch fp32 error %.3g, tolerance %.3g" % (what, e_mine, e_ref, tol))
    assert e_mine <= tol, "%s: error %.3g vs fp64 > %.3g (torch fp32: %.3g)" % (what, e_mine, tol, e_ref)


def _case(M, C, scale, seed):
    """logits [M, C] inside a wider buffer (ld = C + 3), int64 targets; row 0 holds equal values (M > 1), the last row a
    tie of its two largest entries, the one before it (M > 2) the same tie with the target on the LATER column"""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randn(M, C + 3, generator=g) * scale
    x = buf[:, :C]
    t = torch.randint(0, C, (M,), generator=g)
    if M > 1:
        x[0] = float(scale) * 0.75
    a, b = (0, C - 1) if C < 5 else (C // 3, C // 3 + 2)
    for r, tgt in ((M - 1, a), (M - 2, b)):
        if r >= (1 if M > 1 else 0):
            top = float(x[r].abs().max()) + float(scale)
            x[r, a] = top
            x[r, b] = top
            t[r] = tgt
    return buf, t


SHAPES = [(M, C) for M in (1, 20, 1014) for C in (2, 3, 64, 300, 1000)]


@pytest.mark.parametrize("scale", [1.0, 6e5], ids=["order1", "order6e5"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_log_softmax_and_nll_against_fp64(E, M, C, scale):
    ops = E.ops
    buf, t = _case(M, C, scale, 1000 * M + C)
    x = buf[:, :C]
    xmax = float(x.abs().max())
    w = torch.randn(M, C, generator=torch.Generator().manual_seed(5))
    # ---- log_softmax forward / backward ----
    x32 = x.clone().requires_grad_(True)
    x64 = x.double().clone().requires_grad_(True)
    l32, l64 = F.log_softmax(x32, dim=1), F.log_softmax(x64, dim=1)
    (l32 * w).sum().backward()
    (l64 * w.double()).sum().backward()
    bd = buf.to(DEV)
    xd = bd[:, :C].requires_grad_(True)                               # ld = C + 3 > C
    assert xd.stride(0) == C + 3
    ld = ops.log_softmax(xd)
    (ld * w.to(DEV)).sum().backward()
    assert bool(torch.isfinite(ld).all())
    _check("log_softmax M=%d C=%d" % (M, C), ld, l32, l64, xmax)
    _check("log_softmax grad", xd.grad, x32.grad, x64.grad, float(x64.grad.abs().max()))
    # ---- nll_loss on the SAME fp32 log-probabilities (wider buffer again), both reductions ----
    lp = l32.detach()
    lpbuf = torch.zeros(M, C + 5)
    lpbuf[:, :C] = lp
    want_correct = int((torch.tensor(np.argmax(lp.numpy(), axis=1)) == t).sum())        # first maximum
    for red in ("mean", "sum"):
        p32 = lp.clone().requires_grad_(True)
        p64 = lp.double().clone().requires_grad_(True)
        n32, n64 = F.nll_loss(p32, t, reduction=red), F.nll_loss(p64, t, reduction=red)
        n32.backward(); n64.backward()
        pd = lpbuf.to(DEV)[:, :C].requires_grad_(True)
        nd, correct = ops.nll_loss(pd, t.to(DEV), reduction=red, return_correct=True)
        nd.backward()
        _check("nll_loss(%s)" % red, nd, n32, n64, float(lp.abs().max()))
        _check("nll_loss(%s) grad" % red, pd.grad, p32.grad, p64.grad, float(p64.grad.abs().max()))
        assert correct == want_correct
        with torch.no_grad():                                         # the evaluation path (no gradient buffer): same numbers
            nd2, correct2 = ops.nll_loss(pd.detach(), t.to(DEV), reduction=red, return_correct=True)
        assert torch.equal(nd2, nd.detach()) and correct2 == want_correct
    # ---- the fused head: against fp64, and bit for bit against the two-op composition ----
    want_correct = int((torch.tensor(np.argmax(x.numpy(), axis=1)) == t).sum())
    for red in ("mean", "sum"):
        a32 = x.clone().requires_grad_(True)
        a64 = x.double().clone().requires_grad_(True)
        f32, f64 = F.nll_loss(F.log_softmax(a32, dim=1), t, reduction=red), F.nll_loss(F.log_softmax(a64, dim=1), t, reduction=red)
        f32.backward(); f64.backward()
        ad = bd[:, :C].detach().requires_grad_(True)
        fd, fl, correct = ops.log_softmax_nll(ad, t.to(DEV), reduction=red, return_aux=True)
        fd.backward()
        _check("log_softmax_nll(%s) loss" % red, fd, f32, f64, xmax)
        _check("log_softmax_nll(%s) grad" % red, ad.grad, a32.grad, a64.grad, float(a64.grad.abs().max()))
        assert correct == want_correct
        two_lp = ops.log_softmax(bd[:, :C])
        two_loss = ops.nll_loss(two_lp, t.to(DEV), reduction=red)
        assert torch.equal(fl, two_lp) and torch.equal(fl, ld.detach()), "fused logp differs from esc_log_softmax_fwd"
        assert torch.equal(fd.detach(), two_loss), "fused loss differs from the two-op composition"
        with torch.no_grad():
            fe, fle, ce = ops.log_softmax_nll(bd[:, :C], t.to(DEV), reduction=red, return_aux=True)
        assert torch.equal(fe, fd.detach()) and torch.equal(fle, fl) and ce == want_correct


def test_row_of_equal_values_and_ties(E):
    """log_softmax of a constant row is -log(C) in every column; a tie resolves to the FIRST maximal column"""
    for C in (2, 64, 1000):
        x = torch.full((3, C), 6e5)
        x[1, :] = -3.0
        x[2, 0], x[2, C - 1] = 7e5, 7e5
        lp = E.ops.log_softmax(x.to(DEV)).cpu()
        assert torch.allclose(lp[:2], torch.full((2, C), -float(np.log(C))), rtol=0, atol=_ulp(np.log(C)))
        t = torch.tensor([0, 0, C - 1])
        _, correct = E.ops.nll_loss(lp.to(DEV), t.to(DEV), return_correct=True)
        assert correct == 2                                           # rows 0, 1: argmax 0; row 2: first maximum is column 0, not C-1
        _, _, correct = E.ops.log_softmax_nll(x.to(DEV), torch.tensor([0, 0, 0]).to(DEV), return_aux=True)
        assert correct == 3


@pytest.mark.parametrize("bad", [-1, 7])
def test_out_of_range_target_raises(E, bad):
    x = torch.randn(5, 7).to(DEV)
    t = torch.tensor([0, 1, bad, 3, 4]).to(DEV)
    with pytest.raises(RuntimeError, match="[Tt]arget"):
        E.ops.nll_loss(E.ops.log_softmax(x), t)
    with pytest.raises(RuntimeError, match="[Tt]arget"):
        E.ops.log_softmax_nll(x.clone().requires_grad_(True), t)
    with pytest.raises(TypeError):
        E.ops.nll_loss(E.ops.log_softmax(x), t.int())
    ok = E.ops.log_softmax_nll(x, torch.tensor([0, 1, 2, 3, 4]).to(DEV))        # the device is still fine afterwards
    assert bool(torch.isfinite(ok))


@pytest.mark.parametrize("M", [0, 1, 2, 15, 300])
def test_pdist_against_fp64(E, M):
    C = 64
    g = torch.Generator().manual_seed(40 + M)
    buf = torch.zeros(M, C + 4)
    buf[:, :C] = 1e5 * torch.randn(1, C, generator=g) + torch.randn(M, C, generator=g)      # magnitude 1e5, distances of order 1
    x = buf[:, :C]
    d32, d64 = torch.pdist(x, p=2), torch.pdist(x.double(), p=2)
    out = E.ops.pdist(buf.to(DEV)[:, :C])
    assert out.shape == (M * (M - 1) // 2,) and out.dtype == torch.float32
    if M <= 1:
        empty, below = E.ops.pdist(buf.to(DEV)[:, :C], 1e-2)
        assert empty.numel() == 0 and below == 0 and d64.numel() == 0
        return
    assert 1.0 < float(d64.mean()) < 100.0
    _check("pdist M=%d" % M, out, d32, d64, float(d64.max()))
    thr = float(out.median()) if M > 2 else float(out[0]) + 1.0
    out2, below = E.ops.pdist(buf.to(DEV)[:, :C], thr)
    assert torch.equal(out2, out) and below == int((out < thr).sum())
    assert E.ops.pdist(buf.to(DEV)[:, :C], 0.0)[1] == 0 and E.ops.pdist(buf.to(DEV)[:, :C], 1e9)[1] == out.numel()


# ---- the model on the real-graph fixtures ------------------------------------------------------------------------------
def _product_features(E, which, h):
    from esc_gnn_amd.datasets import build_expressive_dataset, load_exp_txt, load_sr25
    raw = load_sr25(eo.SR25_FILE) if which == "sr" else load_exp_txt(eo.EXP_FILE)
    return build_expressive_dataset(raw, h)


def test_sr25_end_to_end(E, golden):
    from esc_gnn_amd.expressive_models import NestedGIN
    from esc_gnn_amd.run_sr import predictions
    z = golden
    graphs = _product_features(E, "sr", int(z["h"]))
    assert np.array_equal(eo.graph_digests(graphs), z["sr_digests"])              # HIP feature build: bit-exact
    ref = eo.expressive_oracle_from_recipe(z, 1)
    m = NestedGIN(1, int(z["layers"]), int(z["hidden"]))
    assert list(m.state_dict().keys()) == [str(k) for k in z["keys"]]
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).eval()
    # the device-collated batch of all 15 graphs (the store needs a y: a dummy one; the reference's graphs have none)
    with_y = [E.Data(x=g.x, edge_index=g.edge_index, y=torch.zeros(1), pos_enc=g.pos_enc, pos_index=g.pos_index,
                     pos_batch=g.pos_batch) for g in graphs]
    store = E.DeviceGraphStore(with_y, DEV)
    with torch.no_grad():
        pred = m(store.collate(torch.arange(15)))
    assert pred.shape == (15, int(z["hidden"]))
    p64, err32 = torch.tensor(z["sr_pred64"]), float(z["sr_err32"])
    err = float((pred.cpu().double() - p64).abs().max())
    print("SR25: max|pred - pred64| %.4g, fp32 oracle %.4g (bound %.4g); max|pred| %.4g" % (err, err32, 3 * err32, float(p64.abs().max())))
    assert err <= 3 * err32
    dist, wrong = E.ops.pdist(pred, 1e-2)
    assert dist.shape == (105,) and wrong == int(z["sr_wrong"]) == 0
    assert float((dist.cpu().double() - torch.tensor(z["sr_dist64"])).abs().max()) <= 2 * int(z["hidden"]) ** 0.5 * 3 * err32
    # the driver's path: y = None graphs through the DataLoader (host collate), same model -> the same verdict
    pred2 = predictions(m, graphs, torch.device(DEV))
    assert float((pred2.cpu().double() - p64).abs().max()) <= 3 * err32
    assert E.ops.pdist(pred2, 1e-2)[1] == 0


def test_exp_training_step(E, golden):
    from esc_gnn_amd.datasets import load_exp_txt
    from esc_gnn_amd.expressive_models import NestedGIN
    from esc_gnn_amd.run_exp import labels_of
    from test_hip_model import _close_grad
    torch.set_num_threads(1)
    z = golden
    H, n = int(z["hidden"]), int(z["exp_drop"].shape[0])
    graphs = _product_features(E, "exp", int(z["h"]))
    assert np.array_equal(eo.graph_digests(graphs), z["exp_digests"])
    ref = eo.expressive_oracle_from_recipe(z, 2)
    m = NestedGIN(2, int(z["layers"]), H)
    m.load_state_dict(ref.state_dict())
    m = m.to(DEV).train()
    store = E.DeviceGraphStore(graphs, DEV)
    b = store.collate(torch.arange(n))
    y = labels_of(b)
    assert y.dtype == torch.int64 and y.cpu().tolist() == z["exp_labels"][:n].tolist()       # int64 labels round-trip exactly
    # the mask torch will draw for the head's dropout: seed, draw, reseed
    draws = []
    for _ in range(2):
        torch.manual_seed(77); torch.cuda.manual_seed_all(77)
        draws.append(F.dropout(torch.ones(n, H, device=DEV), p=0.5, training=True))
    assert torch.equal(draws[0], draws[1]) and set(draws[0].unique().tolist()) <= {0.0, 2.0}
    drop = draws[0].cpu()
    torch.manual_seed(77); torch.cuda.manual_seed_all(77)
    logits = m.logits(b)
    loss, logp, _ = E.ops.log_softmax_nll(logits, y, return_aux=True)
    loss.backward()
    args = eo.collate(eo.cpu_features(load_exp_txt(eo.EXP_FILE, n), int(z["h"])))
    yc = torch.tensor(z["exp_labels"][:n])
    ref.train()
    o32 = ref(*args, drop=drop); l32 = F.nll_loss(o32, yc); l32.backward()
    ref64 = copy.deepcopy(ref).double(); ref64.zero_grad()
    o64 = ref64(args[0].double(), *args[1:], drop=drop); l64 = F.nll_loss(o64, yc); l64.backward()
    o32, o64, l32, l64 = o32.detach(), o64.detach(), float(l32.detach()), float(l64.detach())
    sc = max(1.0, float(o64.abs().max()))
    e_out, e_ref = float((logp.cpu().double() - o64).abs().max()) / sc, float((o32.double() - o64).abs().max()) / sc
    e_loss, e_lref = abs(float(loss.detach()) - l64) / max(1.0, abs(l64)), abs(l32 - l64) / max(1.0, abs(l64))
    print("EXP step: output error %.3g (fp32 oracle %.3g), loss %.7f error %.3g (fp32 oracle %.3g)" % (e_out, e_ref, float(loss.detach()), e_loss, e_lref))
    assert e_out <= max(1e-5, 3 * e_ref) and e_loss <= max(1e-5, 3 * e_lref)
    rp, rp64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    names = [k for k, _ in m.named_parameters()]
    assert names == list(rp) and not any(k.endswith(".eps") for k in names)
    for k, p in m.named_parameters():
        sc = max(1.0, float(rp64[k].grad.abs().max()))
        print("grad %s: error %.3g, fp32 oracle %.3g" % (k, float((p.grad.cpu().double() - rp64[k].grad).abs().max()) / sc,
                                                        float((rp[k].grad.double() - rp64[k].grad).abs().max()) / sc))
    for k, p in m.named_parameters():
        _close_grad(k, p.grad, rp[k].grad, rp64[k].grad)
    for k, buf in m.named_buffers():
        if k.endswith(".eps"):
            assert not buf.requires_grad and float(buf) == 0.0


# ---- the drivers -------------------------------------------------------------------------------------------------------
def _run(module, argv, cwd, seconds):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", module] + argv, cwd=str(cwd), env=env, capture_output=True, text=True,
                       timeout=seconds)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_run_sr_driver(E, tmp_path):
    out = _run("esc_gnn_amd.run_sr", ["--data_root", GOLDEN, "--seed", "1"], tmp_path, 600)
    acc = float(re.search(r"^Acc: (\S+)$", out, re.M).group(1))
    assert 0.0 <= acc <= 1.0


def test_run_exp_driver_two_epochs(E, tmp_path):
    out = _run("esc_gnn_amd.run_exp", ["--data_root", os.path.join(GOLDEN, "exp_first40.txt"), "--limit", "40", "--splits", "1",
                                      "--epochs", "2", "--seed", "3"], tmp_path, 900)
    pat = (r"^Epoch: (\d{3}), LR: (\S+), Train Loss: (\S+), Val Loss: (\S+), Test Acc: (\S+), Exp Acc: (\S+), "
           r"Lrn Acc: (\S+), Train Acc: (\S+)$")
    lines = re.findall(pat, out, re.M)
    assert [l[0] for l in lines] == ["001", "002"]
    for l in lines:
        assert np.isfinite(float(l[2])) and np.isfinite(float(l[3])) and all(0.0 <= float(v) <= 1.0 for v in l[4:])
    assert re.search(r"^Mean: \S+, Std: +\S+$", out, re.M) and re.search(r"^Tr Mean: \S+, Std: +\S+$", out, re.M)
    assert "---------------- Split 0 ----------------" in out


def test_missing_data_file_is_a_one_line_exit(E, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for mod in ("esc_gnn_amd.run_sr", "esc_gnn_amd.run_exp"):
        r = subprocess.run([sys.executable, "-m", mod, "--data_root", str(tmp_path)], cwd=str(tmp_path), env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "Traceback" not in r.stderr and "under %s" % tmp_path in r.stderr
