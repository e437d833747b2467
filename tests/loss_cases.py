"""The case table of the loss heads and the optimiser: one record per (entry point, size, data regime, argument combination)
of esc_l1_loss, esc_mse_loss, esc_bce_logits_loss and esc_adam_step(_scaled) / FlatAdam, chosen so that every size at which the
kernels take another trip of a loop, every argument of the ABI and every state the optimiser can be resumed from is reached by
name.  No GPU is needed to import or check this module (tests/test_loss_cases_cpu.py); tests/test_hip_loss_optim.py runs the
table against the library.  The guarded buffers are those of tests/linear_cases.py.

A loss case is Loss(name, entry, G, T, regime, denom, grad_scale, want_dpred, upstream):
  entry       l1 | mse | bce                      G, T   the prediction is [G, T]; M = G * T entries (T == 1 for l1 and mse)
  regime      l1, mse: plain | ties | offset | one_sided
              bce:     plain | all_labelled | none_labelled | one_labelled | saturated | soft
  denom       None (the mean), 1 (the sum form of data parallelism) or a count larger than M (a global batch)
  grad_scale  the ABI's factor on dpred (l1, mse)  want_dpred  False: dpred = NULL, the engines' evaluation path
  upstream    the factor c of (c * loss).backward() through ops

An Adam case is Adam(name, n, steps, step0, lrs, betas, eps, regime, grad_denom, layout):
  n           live parameter elements              steps    launches checked (lrs holds one learning rate per launch)
  step0       steps already taken: 0, or 20 000 with exp_avg / exp_avg_sq given, both set through load_state_dict
  regime      plain | sparse | all_zero | large | tiny | mixed | flip
  grad_denom  None or the value of the device scalar the gradients are divided by inside the launch
  layout      one (a single tensor) | padded (five tensors, two of them 1-element) | late (the same, first two given as late=)

References are fp64 and written out as the plain formulas.  The loss criterion is that of tests/test_hip_expressive.py::_check,
|mine - ref64| <= max(3 * |torch fp32 - ref64|, one fp32 ulp of a stated floor); the floors and the Adam bounds are derived in
DESIGN.md ("Coverage of the loss heads and the optimiser"), never measured.

One behaviour is pinned that deliberately differs from torch: a batch without a single label (bce, `none_labelled`) gives loss
exactly 0 and gradient exactly 0, everything finite, where torch's mean over an empty selection is NaN.  A training step on such
a batch then changes nothing instead of poisoning every parameter.
"""
import collections
import zlib

import numpy as np
import torch
import torch.nn.functional as F

Loss = collections.namedtuple("Loss", "name entry G T regime denom grad_scale want_dpred upstream")
Adam = collections.namedtuple("Adam", "name n steps step0 lrs betas eps regime grad_denom layout")

U = 2.0 ** -24                                         # unit roundoff of fp32: the largest relative error of one rounding
WORKGROUP = 1024                                       # the loss kernels: one workgroup, one entry per thread and pass
MULTIPASS = 38400                                      # 300 x 128, ogbg-molpcba at batch 300: 37.5 passes
LOSS_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, MULTIPASS)
L1_REGIMES = ("plain", "ties", "offset", "one_sided")
BCE_REGIMES = ("plain", "all_labelled", "none_labelled", "one_labelled", "saturated", "soft")
SATURATED = (20.0, -20.0, 100.0, -100.0, 1e4, -1e4)
ADAM_CAP = 2048 * 256                                  # adam_kernel's grid: at most 2048 workgroups of 256 threads, then a stride
ADAM_SIZES = (1, 15, 16, 17, 255, 256, 257, ADAM_CAP, ADAM_CAP + 1, 2 * ADAM_CAP + 3)
ADAM_REGIMES = ("plain", "sparse", "all_zero", "large", "tiny", "mixed", "flip")
DEFAULT_BETAS, DEFAULT_EPS = (0.9, 0.999), 1e-8
OTHER_BETAS, OTHER_EPS = (0.5, 0.9), 1e-6
ALIGN = 16                                             # FlatBucket.ALIGN
MAX_BUFFER_BYTES = 16 * 2 ** 20


def seed_of(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def ulp(v):
    return float(np.spacing(np.float32(abs(float(v)))))


# ---- the loss table ---------------------------------------------------------------------------------------------------------
LOSS_CASES = []


def _loss(entry, G, T, regime, denom=None, grad_scale=1.0, want_dpred=True, upstream=1.0):
    name = "%s-%dx%d-%s" % (entry, G, T, regime)
    name += ("-d%d" % denom if denom else "") + ("-gs%g" % grad_scale if grad_scale != 1.0 else "")
    name += ("" if want_dpred else "-nodpred") + ("-up%g" % upstream if upstream != 1.0 else "")
    LOSS_CASES.append(Loss(name, entry, G, T, regime, denom, grad_scale, want_dpred, upstream))


for _e in ("l1", "mse"):
    for _M in LOSS_SIZES:
        _loss(_e, _M, 1, "plain")
    for _M in (1, 2, 65, 1025, MULTIPASS):
        _loss(_e, _M, 1, "ties")
    for _M in (63, 1024, 2049):
        _loss(_e, _M, 1, "offset")
        _loss(_e, _M, 1, "one_sided")
    _loss(_e, 2, 1, "plain", denom=1)
    _loss(_e, 1025, 1, "ties", denom=1)
    _loss(_e, MULTIPASS, 1, "plain", denom=1)
    _loss(_e, 1, 1, "plain", denom=7)
    _loss(_e, 1023, 1, "one_sided", denom=4096)
    _loss(_e, MULTIPASS, 1, "ties", denom=4 * MULTIPASS)
    _loss(_e, 64, 1, "plain", grad_scale=0.25)
    _loss(_e, 2049, 1, "ties", denom=4096, grad_scale=0.25)
    _loss(_e, 1, 1, "plain", want_dpred=False)
    _loss(_e, 1024, 1, "offset", want_dpred=False)
    _loss(_e, MULTIPASS, 1, "plain", denom=1, want_dpred=False)
    _loss(_e, 63, 1, "plain", upstream=3.0)
    _loss(_e, 1025, 1, "ties", denom=1, upstream=3.0)

BCE_SHAPES = ((1, 1), (2, 1), (63, 1), (64, 1), (13, 5), (1023, 1), (8, 128), (205, 5), (2049, 1), (300, 128))   # M = LOSS_SIZES
for _G, _T in BCE_SHAPES:
    _loss("bce", _G, _T, "plain")
for _r in BCE_REGIMES[1:]:
    for _G, _T in ((1, 1), (13, 5), (205, 5), (300, 128)):
        _loss("bce", _G, _T, _r)
_loss("bce", 37, 5, "plain")                            # the shape tests/test_hip_train_cli.py has always used
_loss("bce", 2, 1, "all_labelled", denom=1)
_loss("bce", 205, 5, "plain", denom=1)
_loss("bce", 300, 128, "plain", denom=1)
_loss("bce", 13, 5, "plain", denom=4096)
_loss("bce", 300, 128, "soft", denom=4 * MULTIPASS)
_loss("bce", 64, 1, "none_labelled", denom=100)
_loss("bce", 1023, 1, "saturated", denom=4096)
_loss("bce", 1, 1, "plain", want_dpred=False)
_loss("bce", 8, 128, "saturated", want_dpred=False)
_loss("bce", 300, 128, "plain", denom=1, want_dpred=False)
_loss("bce", 64, 1, "none_labelled", want_dpred=False)
_loss("bce", 63, 1, "plain", upstream=3.0)
_loss("bce", 205, 5, "saturated", denom=1, upstream=3.0)

LOSS_BY_NAME = {c.name: c for c in LOSS_CASES}


def loss_cases(entry=None):
    return [c for c in LOSS_CASES if entry in (None, c.entry)]


def loss_data(case):
    """(pred, y): float32 CPU tensors of shape [G, T]; a function of the case's name alone"""
    g = torch.Generator().manual_seed(seed_of("%s-%dx%d-%s" % (case.entry, case.G, case.T, case.regime)))
    G, T = case.G, case.T
    M = G * T
    pred, y = torch.randn(M, generator=g), torch.randn(M, generator=g)
    r = case.regime
    if case.entry in ("l1", "mse"):
        if r == "ties":                                 # a third of the entries: pred == y exactly, signed zeros among them
            tie = torch.arange(M) % 3 == 0
            pred[tie] = y[tie]
            for k, (a, b) in enumerate(((0.0, -0.0), (-0.0, 0.0), (-0.0, -0.0))):
                i = 3 * (2 * k + 1)
                if i < M:
                    pred[i], y[i] = a, b
        elif r == "offset":                             # targets of magnitude 1e3, differences of order 1
            y = (1.0 + 0.1 * torch.rand(M, generator=g)) * 1e3 * torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0)
            pred = y + pred
        elif r == "one_sided":
            pred = y + pred.abs() + 0.01
            assert bool((pred > y).all())
        else:
            assert r == "plain", r
    else:
        pred = pred * 3
        y = (torch.rand(M, generator=g) > 0.5).float()
        unl = torch.rand(M, generator=g) < 0.3
        if r == "plain":
            if M >= 8:
                y[unl] = float("nan")
        elif r == "none_labelled":
            y[:] = float("nan")
        elif r == "one_labelled":
            keep = y[M // 2].clone()
            y[:] = float("nan")
            y[M // 2] = keep
        elif r == "saturated":                          # +-20, +-100, +-1e4 against both labels, ordinary logits in between
            if M >= 8:
                y[unl] = float("nan")
            for k in range(min(M, 12)):
                i = (k * M) // min(M, 12)
                pred[i], y[i] = SATURATED[k % 6], float(k // 6 if M >= 12 else k % 2)
            if M >= 12:                                 # the two entries whose gradient is exactly 0
                pred[0], y[0] = -1e4, 0.0
                pred[M - 1], y[M - 1] = 1e4, 1.0
            elif M == 1:
                pred[0], y[0] = -1e4, 0.0
        elif r == "soft":
            y = torch.rand(M, generator=g) * 0.98 + 0.01
        else:
            assert r == "all_labelled", r
    return pred.view(G, T).contiguous(), y.view(G, T).contiguous()


def labelled(y):
    return y == y


def loss_divisor(case, y):
    """what the sum is divided by: `denom` when given, else M (l1, mse) or the number of labelled entries (bce)"""
    if case.denom:
        return float(case.denom)
    return float(labelled(y).sum()) if case.entry == "bce" else float(y.numel())


def loss_ref64(case, pred, y, mistake=None):
    """(loss, dloss/dpred * grad_scale * upstream) in fp64, the plain formulas.  `mistake` is one of the deliberate ones of
    tests/test_loss_cases_cpu.py: 'divide_by_M', 'count_nan', 'tie_sign'."""
    x, t = pred.double().reshape(-1), y.double().reshape(-1)
    div = loss_divisor(case, y)
    if mistake == "divide_by_M":
        div = float(x.numel())
    if mistake == "count_nan" and not case.denom:
        div = float(x.numel())
    c = float(case.grad_scale) * float(case.upstream)
    if case.entry == "l1":
        d = x - t
        sign = torch.where(d > 0, 1.0, torch.where(d < 0, -1.0, 1.0 if mistake == "tie_sign" else 0.0)).double()
        return d.abs().sum() / div, sign * (c / div)
    if case.entry == "mse":
        d = x - t
        return (d * d).sum() / div, 2.0 * d * (c / div)
    lab = labelled(t)
    if div == 0:                                        # the pinned behaviour of a batch without labels
        return torch.zeros((), dtype=torch.float64), torch.zeros_like(x)
    t0 = torch.where(lab, t, torch.zeros_like(t))
    term = torch.clamp(x, min=0) - x * t0 + torch.log1p(torch.exp(-x.abs()))
    e = torch.exp(-x.abs())
    sigmoid = torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return torch.where(lab, term, torch.zeros_like(term)).sum() / div, torch.where(lab, (sigmoid - t0) * (c / div), torch.zeros_like(x))


def loss_torch(case, pred, y, dtype):
    """the same through torch.nn.functional + autograd on the CPU in `dtype`: (loss, gradient), both as fp64 tensors.  bce is
    taken on the labelled entries, reduction='sum' divided by the case's divisor; without labels the pinned zeros stand in."""
    x = pred.to(dtype).reshape(-1).clone().requires_grad_(True)
    t = y.to(dtype).reshape(-1)
    div = loss_divisor(case, y)
    if case.entry == "bce":
        lab = labelled(t)
        if div == 0:
            return torch.zeros((), dtype=torch.float64), torch.zeros(x.numel(), dtype=torch.float64)
        loss = F.binary_cross_entropy_with_logits(x[lab], t[lab], reduction="sum") / div
    else:
        loss = (F.l1_loss if case.entry == "l1" else F.mse_loss)(x, t, reduction="sum") / div
    (loss * (float(case.grad_scale) * float(case.upstream))).backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return loss.detach().double(), grad.detach().double()


def loss_floors(case, pred, y, loss64, grad64):
    """(floor of the loss, floor of the gradient): the magnitudes whose fp32 ulp the criterion never goes below"""
    div = loss_divisor(case, y)
    c = float(case.grad_scale) * float(case.upstream)
    if case.entry == "bce":
        lab = labelled(y)
        if div == 0 or not bool(lab.any()):
            return 0.0, 0.0
        xmax = float(pred[lab].abs().max())
        return 4.0 * (xmax + 1.0) * float(lab.sum()) / div + abs(float(loss64)), 8.0 * c / div
    if case.entry == "l1":
        return 2.0 * abs(float(loss64)), 2.0 * c / div
    return abs(float(loss64)), 2.0 * float(grad64.abs().max())


def check(what, mine, ref32, ref64, floor_at):
    """tests/test_hip_expressive.py::_check: |mine - ref64| <= max(3 * |ref32 - ref64|, one fp32 ulp of floor_at), every figure
    printed before the assertion.  Returns (error, tolerance)."""
    ref64 = ref64.detach().double().reshape(-1)
    e_mine = float((mine.detach().cpu().double().reshape(-1) - ref64).abs().max()) if ref64.numel() else 0.0
    e_ref = float((ref32.detach().double().reshape(-1) - ref64).abs().max()) if ref64.numel() else 0.0
    tol = max(3.0 * e_ref, ulp(floor_at))
    print("%s: error %.3g, torch fp32 error %.3g, tolerance %.3g" % (what, e_mine, e_ref, tol))
    assert e_mine == e_mine and e_mine <= tol, "%s: error %.3g vs fp64 > %.3g (torch fp32: %.3g)" % (what, e_mine, tol, e_ref)
    return e_mine, tol


def breaks(mine, ref32, ref64, floor_at):
    """whether `mine` fails the criterion of check()"""
    ref64 = ref64.double().reshape(-1)
    e_mine = float((mine.double().reshape(-1) - ref64).abs().max())
    e_ref = float((ref32.double().reshape(-1) - ref64).abs().max())
    return not e_mine <= max(3.0 * e_ref, ulp(floor_at))


def pred_layouts(case):
    """the shapes `pred` is handed to ops in: name -> (shape, whether it is a column slice of a wider matrix)"""
    M = case.G * case.T
    out = collections.OrderedDict()
    out["[M,1]"] = ((M, 1), False)
    out["[M]"] = ((M,), False)
    G, T = (case.G, case.T) if case.T > 1 else next(((M // k, k) for k in (128, 5, 3, 2) if M % k == 0 and M > k), (1, M))
    out["[G,T]"] = ((G, T), False)
    out["slice"] = ((G, T), True)
    return out


# ---- the Adam table ---------------------------------------------------------------------------------------------------------
ADAM_CASES = []
LR = 1e-2
LR_SCHEDULE = (1e-2, 1e-2, 5e-3, 5e-3, 2.5e-3)          # what ReduceLROnPlateau does: assignments to param_groups[0]["lr"]
STEP0 = 20000
GRAD_DENOM = 2400.0


def _adam(n, steps, regime="plain", step0=0, lrs=None, hyper="default", grad_denom=None, layout="one"):
    lrs = tuple(lrs) if lrs is not None else (LR,) * steps
    assert len(lrs) == steps
    betas, eps = (DEFAULT_BETAS, DEFAULT_EPS) if hyper == "default" else (OTHER_BETAS, OTHER_EPS)
    name = "adam-%d-s%d-%s" % (n, steps, regime)
    name += ("-from%d" % step0 if step0 else "") + ("-lrsched" if len(set(lrs)) > 1 else "") + ("-b.5,.9" if hyper != "default" else "")
    name += ("-den" if grad_denom else "") + ("-" + layout if layout != "one" else "")
    ADAM_CASES.append(Adam(name, n, steps, step0, lrs, betas, eps, regime, grad_denom, layout))


for _n in ADAM_SIZES:
    _adam(_n, 3 if _n < ADAM_CAP else 2)
_adam(255, 20)
for _r in ADAM_REGIMES[1:]:
    _adam(257, 5, _r)
    _adam(256, 5, _r, hyper="other")
_adam(256, 5, hyper="other")
_adam(2 * ADAM_CAP + 3, 2, "sparse")
_adam(ADAM_CAP + 1, 2, "all_zero")
_adam(ADAM_CAP + 1, 2, "mixed", hyper="other")
_adam(257, 5, lrs=LR_SCHEDULE)
_adam(4096, 5, "mixed", lrs=LR_SCHEDULE, hyper="other")
_adam(256, 3, step0=STEP0)
_adam(257, 5, "flip", step0=STEP0, lrs=LR_SCHEDULE)
_adam(255, 3, "tiny", step0=STEP0, hyper="other")
_adam(ADAM_CAP + 1, 2, step0=STEP0)
_adam(17, 3, grad_denom=GRAD_DENOM)
_adam(257, 5, "large", grad_denom=GRAD_DENOM)
_adam(4096, 3, "mixed", grad_denom=GRAD_DENOM, hyper="other")
_adam(2 * ADAM_CAP + 3, 2, grad_denom=GRAD_DENOM)
for _lay in ("padded", "late"):
    _adam(100, 3, layout=_lay)
    _adam(257, 5, "mixed", layout=_lay, lrs=LR_SCHEDULE)
    _adam(4096, 3, "sparse", layout=_lay, step0=STEP0, grad_denom=GRAD_DENOM)
    _adam(ADAM_CAP + 1, 2, layout=_lay)

ADAM_BY_NAME = {c.name: c for c in ADAM_CASES}


def adam_cases(layout=None, max_n=None):
    return [c for c in ADAM_CASES if layout in (None, c.layout) and (max_n is None or c.n <= max_n)]


def tensor_sizes(case):
    """element counts of the parameters the case's n live elements are split into"""
    if case.layout == "one":
        return [case.n]
    a, b = case.n // 3, case.n // 2
    return [a, 1, b - a - 1, 1, case.n - b - 1]


def late_tensors(case):
    """indices (into tensor_sizes) of the parameters given as late="""
    return [0, 1] if case.layout == "late" else []


def flat_layout(case):
    """FlatBucket's arithmetic: (order of the tensors in the buffer, their offsets in that order, padded length)"""
    sizes, late = tensor_sizes(case), late_tensors(case)
    order = [i for i in range(len(sizes)) if i not in late] + late
    offsets, n = [], 0
    for i in order:
        offsets.append(n)
        n += -(-sizes[i] // ALIGN) * ALIGN
    return order, offsets, n


def flat_index(case):
    """int64 [n]: the position of live element j (tensors concatenated in the order they were handed over) in the flat buffer"""
    sizes = tensor_sizes(case)
    order, offsets, _ = flat_layout(case)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    idx = np.empty(case.n, dtype=np.int64)
    for i, off in zip(order, offsets):
        idx[starts[i]:starts[i + 1]] = off + np.arange(sizes[i])
    return idx


class AdamData(object):
    """p0 [n], grads [steps][n] (what the gradient buffer holds: sums when grad_denom is given), m0 / v0 [n] (zeros unless
    step0): float32 numpy arrays, a function of (n, steps, step0, regime, grad_denom) alone — layouts share their data"""

    def __init__(self, case):
        rng = np.random.RandomState(seed_of("adam-%d-%d-%d-%s-%s" % (case.n, case.steps, case.step0, case.regime, case.grad_denom)))
        n, f = case.n, np.float32
        self.p0 = rng.standard_normal(n).astype(f)
        scale = {"large": 1e4, "tiny": 1e-6}.get(case.regime, 1.0) * np.ones(n)
        if case.regime == "mixed":
            scale = 10.0 ** rng.uniform(-6, 4, n)
        self.touched = np.ones(n, dtype=bool)
        if case.regime == "sparse":                     # the embedding rows no batch touches: the same 90 % at every step
            self.touched = rng.uniform(size=n) < 0.1
        if case.regime == "all_zero":
            self.touched[:] = False
        base = np.abs(rng.standard_normal(n))
        self.grads = []
        for t in range(case.steps):
            if case.regime == "flip":
                g = base * (0.5 + rng.uniform(size=n)) * (-1.0) ** t
            else:
                g = rng.standard_normal(n)
            g = g * scale * self.touched * (case.grad_denom or 1.0)          # (an untouched element's zero keeps g's sign)
            self.grads.append(g.astype(f))
        self.m0, self.v0 = np.zeros(n, f), np.zeros(n, f)
        if case.step0:                                  # a state 20 000 steps of such gradients could have left
            self.m0 = np.where(self.touched, 0.3 * rng.standard_normal(n) * scale, 0.0).astype(f)
            self.v0 = np.where(self.touched, (0.5 + rng.uniform(size=n)) * scale * scale, 0.0).astype(f)


_ADAM_DATA = {}


def adam_data(case):
    key = (case.n, case.steps, case.step0, case.regime, case.grad_denom)
    if key not in _ADAM_DATA:
        if len(_ADAM_DATA) > 6:
            _ADAM_DATA.clear()
        _ADAM_DATA[key] = AdamData(case)
    return _ADAM_DATA[key]


SAFETY = 2.0        # the bounds are twice the first-order sums: the sums themselves are what the CPU replays are held to
MISTAKES = ("no_bias_correction", "step_off_by_one", "eps_inside_sqrt", "beta1_for_one_minus_beta1", "denom_after_square")


def adam_ref64(case, data, mistake=None, bounds=True):
    """fp64 Adam from the case's fp32 inputs.  Returns p, m, v after the last step and (bounds=True) the first-order running
    error bounds Bp, Bm, Bv of an fp32 evaluation of adam_kernel's statements, per element: every rounding is
    charged its full u times the magnitude it rounds, the errors of m and v are carried into p through the quotient, and the
    sum is doubled (SAFETY) for what first order leaves out and what the compiler may reorder or contract."""
    b1, b2 = case.betas
    eps, u = case.eps, U
    p, m, v = data.p0.astype(np.float64), data.m0.astype(np.float64), data.v0.astype(np.float64)
    Bp, Bm, Bv = np.zeros(case.n), np.zeros(case.n), np.zeros(case.n)
    for k in range(case.steps):
        t, lr = case.step0 + k + 1, case.lrs[k]
        if mistake == "step_off_by_one":
            t += 1
        g = data.grads[k].astype(np.float64)
        g2 = g * g
        if case.grad_denom:
            g = g / case.grad_denom
            g2 = g2 / case.grad_denom if mistake == "denom_after_square" else g * g
        m_prev, v_prev = m, v
        # ---- Adam, the five lines
        m = b1 * m + (1 - b1) * g if mistake != "beta1_for_one_minus_beta1" else (1 - b1) * m + b1 * g
        v = b2 * v + (1 - b2) * g2
        mhat = m / (1 - b1 ** t) if mistake != "no_bias_correction" else m
        vhat = v / (1 - b2 ** t) if mistake != "no_bias_correction" else v
        p = p - lr * mhat / ((np.sqrt(vhat) + eps) if mistake != "eps_inside_sqrt" else np.sqrt(vhat + eps))
        if not bounds:
            continue
        # ---- what an fp32 evaluation of the kernel's statements can be off by, to first order
        dg = u * np.abs(g) if case.grad_denom else 0.0                          # gi = g / den: one rounding
        Bm = b1 * Bm + (1 - b1) * dg + 3 * u * (1 - b1) * np.abs(g - m_prev) + u * np.abs(m)   # sub, weight's cast, mul; add
        Bv = b2 * Bv + u * (2 * b2 * v_prev + 3 * (1 - b2) * g * g + v) + 2 * (1 - b2) * np.abs(g) * dg
        bc2s, ns = np.sqrt(1 - b2 ** t), lr / (1 - b1 ** t)
        s = np.sqrt(v)
        q = s / bc2s
        den = q + eps
        with np.errstate(divide="ignore", invalid="ignore"):
            Bs = np.where(v > 0, Bv / (2 * s), 0.0) + u * s                     # sqrtf: the error of v through it + one rounding
        Bden = Bs / bc2s + 2 * u * q + u * eps + u * den                        # bc2s's cast, the quotient, eps's cast, the sum
        r = np.abs(m) / den
        Br = Bm / den + r * Bden / den + u * r                                  # mi / denom
        Bp = Bp + ns * Br + 2 * u * ns * r + u * np.abs(p)                      # neg_step's cast, the product; the sum
    return (p, m, v, SAFETY * Bp, SAFETY * Bm, SAFETY * Bv) if bounds else (p, m, v)


def _fma(a, b, c):
    """one rounding of a * b + c: the product of two fp32 numbers is exact in fp64"""
    return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def adam_replay32(case, data, fused):
    """adam_kernel's statements in numpy fp32, with the host code's casts of the hyper-parameters: uncontracted, or with every
    a * b + c fused into one rounding (the build does not pass -ffp-contract=off for optim.hip)"""
    f = np.float32
    b1, b2 = case.betas
    p, m, v = data.p0.copy(), data.m0.copy(), data.v0.copy()
    for k in range(case.steps):
        t, lr = case.step0 + k + 1, case.lrs[k]
        w1, b2f, w2 = f(1.0 - b1), f(b2), f(1.0 - b2)
        bc2s, eps, ns = f(np.sqrt(1.0 - b2 ** t)), f(case.eps), f(-lr / (1.0 - b1 ** t))
        g = data.grads[k]
        gi = g / f(case.grad_denom) if case.grad_denom else g
        if fused:
            mi = _fma(gi - m, w1, m)
            vi = _fma(w2 * gi, gi, v * b2f)
        else:
            mi = m + w1 * (gi - m)
            vi = v * b2f + w2 * gi * gi
        m, v = mi, vi
        denom = np.sqrt(vi) / bc2s + eps
        p = _fma(mi / denom, ns, p) if fused else p + ns * (mi / denom)
        assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def _torch_adam(case, data, dtype):
    p = torch.nn.Parameter(torch.from_numpy(data.p0.copy()).to(dtype))
    opt = torch.optim.Adam([p], lr=case.lrs[0], betas=case.betas, eps=case.eps, foreach=False)
    if case.step0:                                      # through torch's own state_dict
        sd = opt.state_dict()
        sd["state"] = {0: dict(step=torch.tensor(float(case.step0)), exp_avg=torch.from_numpy(data.m0.copy()).to(dtype),
                               exp_avg_sq=torch.from_numpy(data.v0.copy()).to(dtype))}
        opt.load_state_dict(sd)
    for k in range(case.steps):
        opt.param_groups[0]["lr"] = case.lrs[k]
        g = torch.from_numpy(data.grads[k].copy()).to(dtype)
        p.grad = g / case.grad_denom if case.grad_denom else g
        opt.step()
    st = opt.state[p]
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def adam_torch64(case, data):
    return _torch_adam(case, data, torch.float64)


def adam_torch32(case, data):
    """torch.optim.Adam(foreach=False) in fp32 on the CPU"""
    return _torch_adam(case, data, torch.float32)


def worst_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf), and the largest error"""
    err = np.abs(got.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return float(ratio.max()), float(err.max())
