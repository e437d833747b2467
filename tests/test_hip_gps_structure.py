"""The graph-transformer kernels (csrc/attention.hip, csrc/lappe.hip) on the case tables of tests/gps_cases.py: every compiled
head_dim width on every size set (64- and 256-thread blocks, the second row trip, the node limit and its over-64 KiB LDS request,
empty graphs), dropout with the kernel's own mask fed to the oracle, bit equality under every announced size, the skip contract of
attn_graph() through the C ABI, the exact-logit ladder, degenerate values, the layer at three more widths; every compiled dim_pe
width of the LapPE encoder with chunk cuts inside a node's terms and NaN-ragged rows; the gather and its guard.

Error measure and bound: max |got - want| over the largest |want| of the tensor, bound 1e-5; a tensor of zeros must be matched
exactly.  tests/test_gps_cases_cpu.py holds the oracle's own fp32 evaluation to 2e-6 on every asserted case; it is printed beside
every figure.  The only unasserted figures are the ladder's rungs above max |lse| 2^-23 <= 5e-6: they are run, must be finite, and
their error is printed next to the |lse| 2^-24 the design accepts."""
import math

import pytest
import torch

from conftest import ROOT, require_gpu      # noqa: F401  (ROOT: the path set-up of the suite)
import gps_cases as gc
import gps_oracle as go
import loss_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTH_IDS = [gc.width_id(w) for w in gc.WIDTHS]
DP_IDS = [gc.width_id(w) for w in gc.ONE_PER_DP]
FILL = -7.0


@pytest.fixture(scope="module")
def E():
    require_gpu()
    import esc_gnn_amd
    return esc_gnn_amd


def graph_ptr(sizes):
    return torch.tensor(go.graph_ptr_of(sizes), dtype=torch.int32, device=DEV)


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def run_op(E, qkv, gy, sizes, heads, max_nodes=None, **kw):
    """forward and backward through the op: (out, lse, d_qkv, mask)"""
    x = qkv.to(DEV).requires_grad_(True)
    out, lse, mask = E.ops.graph_attention(x, graph_ptr(sizes), heads, max_nodes=max(sizes) if max_nodes is None else max_nodes,
                                           return_aux=True, **kw)
    out.backward(gy.to(DEV))
    return out.detach(), lse, x.grad, mask


class Raw(object):
    """the two C entry points on sentinel-filled outputs; every argument the host states can be overridden"""

    def __init__(self, E, qkv, gy, sizes, heads, d):
        self.nv, self.sizes, self.heads, self.d = E._native, list(sizes), heads, d
        self.qkv, self.gy = qkv.to(DEV).contiguous(), gy.to(DEV).contiguous()
        self.N, self.H, self.G = sum(sizes), heads * d, len(sizes)
        self.gp = graph_ptr(sizes)
        self.pp = torch.tensor(go.graph_ptr_of([n * n for n in sizes]), dtype=torch.int64, device=DEV)
        self.total = int(self.pp[-1])
        self.room = self.total + 13                              # the mask buffer: 13 pairs per head more than the batch needs

    def __call__(self, p, seed=77, gp=None, pp=None, max_nodes=None, mask_pairs=None):
        nv, heads, d, H = self.nv, self.heads, self.d, self.H
        gp = self.gp if gp is None else gp
        pp = self.pp if pp is None else pp
        N = self.N
        max_nodes = max(self.sizes) if max_nodes is None else max_nodes
        mask_pairs = (self.room if p > 0 else 0) if mask_pairs is None else mask_pairs
        out = torch.full((self.N, H), FILL, device=DEV)
        lse = torch.full((heads, N), FILL, device=DEV)
        dq = torch.full((self.N, 3 * H), FILL, device=DEV)
        mask = torch.full((heads * self.room,), 7, dtype=torch.uint8, device=DEV) if p > 0 else None
        nv.call("esc_graph_attention_fwd", nv.ptr(self.qkv), 3 * H, nv.ptr(gp), nv.ptr(pp), self.G, N, mask_pairs, max_nodes, heads, d, p,
                seed, nv.ptr(out), H, nv.ptr(lse), nv.ptr(mask), nv.stream())
        nv.call("esc_graph_attention_bwd", nv.ptr(self.qkv), 3 * H, nv.ptr(self.gy), H, nv.ptr(lse), nv.ptr(mask), nv.ptr(gp), nv.ptr(pp),
                self.G, N, mask_pairs, max_nodes, heads, d, p, nv.ptr(dq), nv.stream())
        return out, lse, dq, mask


# ---- 1. every width on every size set ----------------------------------------------------------------------------------------------
def test_the_library_states_the_limits_the_cases_assume(E):
    for d in range(4, 68, 4):
        assert E.ops.attention_max_nodes(d) == gc.attn_limit(d), d
    assert E.ops.lappe_encode_block_rows() == gc.ENC_ROWS


@pytest.mark.parametrize("name", gc.SIZE_SETS)
@pytest.mark.parametrize("w", gc.WIDTHS, ids=WIDTH_IDS)
def test_every_width_on_every_size_set(E, w, name):
    heads, d = w
    sizes, qkv, gy, (o64, l64, g64), (o32, l32, g32) = gc.attention_case(name, heads, d)
    out, lse, dq, mask = run_op(E, qkv, gy, sizes, heads)
    assert mask is None
    what = "%s %s " % (gc.width_id(w), name)
    gc.check(what + "out", out, o64, o32)
    gc.check(what + "lse", lse, l64, l32)
    gc.check(what + "d_qkv", dq, g64, g32)
    assert bool(torch.isfinite(dq).all())


# ---- 2. dropout --------------------------------------------------------------------------------------------------------------------
def _dropout(E, w, name, p):
    heads, d = w
    sizes, qkv, gy = gc.attention_case(name, heads, d)[:3]
    raw = Raw(E, qkv, gy, sizes, heads, d)
    what = "%s %s p %g " % (gc.width_id(w), name, p)
    seed = lc.seed_of("gps-drop-" + what)                   # a seed per case: the kept shares are independent samples
    out, lse, dq, mask = raw(p, seed=seed)
    live, n = mask[:heads * raw.total], heads * raw.total
    assert bool((live <= 1).all())
    assert bool((mask[n:] == 7).all()), "bytes behind heads * pair_ptr[G] were written"
    keep = go.unpack_mask(mask.cpu(), sizes, heads)
    (o64, l64, g64), (o32, l32, g32) = gc.attention_oracle(qkv, gy, sizes, heads, keep, p)
    gc.check(what + "out", out, o64, o32)
    gc.check(what + "lse", lse, l64, l32)
    gc.check(what + "d_qkv", dq, g64, g32)
    assert bool(torch.isfinite(dq).all())
    kept, sd = int(live.sum()), math.sqrt(n * p * (1 - p))
    print("%skept %d of %d: %.2f standard deviations from %g" % (what, kept, n, (kept - n * (1 - p)) / sd, 1 - p))
    assert abs(kept - n * (1 - p)) <= 5 * sd
    again = raw(p, seed=seed)                                 # the same batch, the same seed: no bit differs
    assert all(torch.equal(a, b) for a, b in zip((out, lse, dq, mask), again))
    assert not torch.equal(raw(p, seed=seed + 1)[3][:n], live)


@pytest.mark.parametrize("p", gc.DROP_PS)
@pytest.mark.parametrize("name", gc.DROP_SETS)
@pytest.mark.parametrize("w", gc.WIDTHS, ids=WIDTH_IDS)
def test_dropout_with_the_kernels_own_mask(E, w, name, p):
    _dropout(E, w, name, p)


@pytest.mark.parametrize("p", gc.DROP_PS)
@pytest.mark.parametrize("w", gc.ONE_PER_DP, ids=DP_IDS)
def test_dropout_at_the_limit(E, w, p):
    _dropout(E, w, "limit", p)


# ---- 3. the announced size changes no bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("wave", "block"))
@pytest.mark.parametrize("w", gc.ONE_PER_DP, ids=DP_IDS)
def test_the_announced_size_changes_no_bit(E, w, name):
    """p = 0: the rows of every graph are the same bits alone, inside the batch announced at its largest graph, announced at the
    limit L (the over-64 KiB LDS request at DP >= 8) and, where the largest graph has 64 nodes, announced at 64 against 65 (the
    64- against the 256-thread block)"""
    heads, d = w
    L = gc.attn_limit(d)
    sizes, qkv, gy = gc.attention_case(name, heads, d)[:3]
    base = run_op(E, qkv, gy, sizes, heads)[:3]
    announced = [L] + ([64, 65] if max(sizes) <= 64 else [])
    assert name != "wave" or (gc.attn_block(64), gc.attn_block(65)) == (64, 256)
    for m in announced:
        other = run_op(E, qkv, gy, sizes, heads, max_nodes=m)[:3]
        assert all(same_bits(a, b) for a, b in zip(base, other)), "max_nodes %d changed a bit" % m
    o = 0
    for n in sizes:
        for m in (n, L):
            out, lse, dq = run_op(E, qkv[o:o + n].clone(), gy[o:o + n].clone(), [n], heads, max_nodes=m)[:3]
            assert same_bits(out, base[0][o:o + n]) and same_bits(lse, base[1][:, o:o + n]) and same_bits(dq, base[2][o:o + n]), \
                "the graph of %d nodes alone (announced %d) differs from its rows in the batch" % (n, m)
        o += n


# ---- 4. a graph that contradicts the host is skipped -------------------------------------------------------------------------------
SKIP_SIZES = [5, 70, 3, 12]


@pytest.mark.parametrize("p", (0.0, 0.5))
@pytest.mark.parametrize("w", [(3, 12), (1, 60)], ids=gc.width_id)
def test_a_graph_that_contradicts_the_host_is_skipped(E, w, p):
    """every contradiction attn_graph() is written to catch before any access: the skipped graphs' rows of out, lse, d_qkv and
    their mask bytes keep the sentinel, every other graph is bit-equal to the uncontradicted run, which is correct"""
    heads, d = w
    sizes = SKIP_SIZES
    qkv, gy = gc.attention_inputs("skip", sizes, heads, d)
    raw = Raw(E, qkv, gy, sizes, heads, d)
    ptr, pairs = go.graph_ptr_of(sizes), go.graph_ptr_of([n * n for n in sizes])
    good = raw(p)
    keep = go.unpack_mask(good[3].cpu(), sizes, heads) if p > 0 else None
    (o64, l64, g64), (o32, l32, g32) = gc.attention_oracle(qkv, gy, sizes, heads, keep, p)
    what = "%s p %g " % (gc.width_id(w), p)
    gc.check(what + "uncontradicted out", good[0], o64, o32)
    gc.check(what + "uncontradicted lse", good[1], l64, l32)
    gc.check(what + "uncontradicted d_qkv", good[2], g64, g32)

    def verify(tag, res, skipped):
        out, lse, dq, mask = res
        for g, n in enumerate(sizes):
            rows = slice(ptr[g], ptr[g + 1])
            segs = [slice(a * raw.total + pairs[g], a * raw.total + pairs[g + 1]) for a in range(heads)] if p > 0 else []
            if g in skipped:
                assert bool((out[rows] == FILL).all()) and bool((lse[:, rows] == FILL).all()) and bool((dq[rows] == FILL).all()), \
                    "%s: graph %d was written" % (tag, g)
                assert all(bool((mask[s] == 7).all()) for s in segs), "%s: mask bytes of graph %d were written" % (tag, g)
            else:
                assert same_bits(out[rows], good[0][rows]) and same_bits(lse[:, rows], good[1][:, rows]) and \
                    same_bits(dq[rows], good[2][rows]), "%s: graph %d differs from the uncontradicted run" % (tag, g)
                assert all(torch.equal(mask[s], good[3][s]) for s in segs), "%s: mask of graph %d" % (tag, g)
        if p > 0:
            assert bool((mask[heads * raw.total:] == 7).all())

    # n <= cap: 12 announced, cap = 12, the graph of 70 nodes does not fit
    verify("max_nodes understated", raw(p, max_nodes=12), {1})
    # n > 0: a range that decreases (graph 1 has -2 nodes; graph 2 then claims 75 > cap = 72 rows from row 3)
    dec = list(ptr)
    dec[2] = 3
    verify("decreasing graph_ptr", raw(p, gp=torch.tensor(dec, dtype=torch.int32, device=DEV)), {1, 2})
    # n0 <= N - n: the last range runs 4 rows past N
    past = list(ptr)
    past[4] += 4
    verify("graph_ptr past N", raw(p, gp=torch.tensor(past, dtype=torch.int32, device=DEV)), {3})
    # n0 >= 0: the first range starts before row 0
    neg = list(ptr)
    neg[0] = -2
    verify("graph_ptr before row 0", raw(p, gp=torch.tensor(neg, dtype=torch.int32, device=DEV)), {0})
    # pair_ptr[g + 1] - pair_ptr[g] == n * n: one entry off by one contradicts the graph on either side of it
    off = list(pairs)
    off[2] += 1
    verify("pair_ptr not the scan", raw(p, pp=torch.tensor(off, dtype=torch.int64, device=DEV)), {1, 2})
    # m0 >= 0: graph 0's 25 pairs start before the buffer (graph 1 then counts 4925 pairs for its 4900)
    low = list(pairs)
    low[0], low[1] = -25, 0
    verify("pair_ptr below 0", raw(p, pp=torch.tensor(low, dtype=torch.int64, device=DEV)), {0, 1})
    # m0 <= total - n * n: graph 1's 4900 pairs, counted right, end 47 behind pair_ptr[G] (its neighbours' counts are then off)
    high = list(pairs)
    high[1], high[2] = pairs[1] + 200, pairs[2] + 200
    assert high[2] - high[1] == 70 * 70 and high[2] > pairs[4]
    verify("pair range behind pair_ptr[G]", raw(p, pp=torch.tensor(high, dtype=torch.int64, device=DEV)), {0, 1, 2})
    if p > 0:
        # total <= mask_pairs: one pair of room missing - every graph is skipped and no mask byte is written
        res = raw(p, mask_pairs=raw.total - 1)
        verify("mask room below pair_ptr[G]", res, {0, 1, 2, 3})
        assert bool((res[3] == 7).all())
    after = raw(p)                                            # a valid call after these is correct
    assert all(torch.equal(a, b) for a, b in zip(after, good) if a is not None)


# ---- 5. the exact-logit ladder -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", gc.LADDER_DIMS)
def test_exact_logit_ladder(E, d):
    """logits exact in fp32 (integers over 4, 1 / sqrt(d) a power of two): the fp64 comparison means something at any sharpness.
    Rungs with max |lse| 2^-23 <= BOUND / 2 are held to the bound; the rungs above are run, must be finite, and their error is
    printed next to |lse| 2^-24, the error the design accepts in the P the backward recomputes from one fp32 lse."""
    asserted = []
    for amp in gc.LADDER_AMPS:
        qkv, gy, (o64, l64, g64), (o32, l32, g32) = gc.ladder_case(d, amp)
        out, lse, dq, _ = run_op(E, qkv, gy, gc.LADDER_SIZES, gc.LADDER_HEADS)
        assert all(bool(torch.isfinite(t).all()) for t in (out, lse, dq))
        figures = [gc.rel(a, b) for a, b in zip((out, lse, dq), (o64, l64, g64))]
        expected = gc.ladder_expected(d, amp)
        print("ladder d %2d amp %2d: max |lse| %7.4g  out %.3g  lse %.3g  d_qkv %.3g  |lse| 2^-24 = %.3g  d_qkv over it %.2f  %s"
              % (d, amp, gc.ladder_lse(d, amp), figures[0], figures[1], figures[2], expected, figures[2] / expected,
                 "asserted" if gc.ladder_asserted(d, amp) else "recorded"))
        if gc.ladder_asserted(d, amp):
            asserted.append(amp)
            what = "ladder d %d amp %d " % (d, amp)
            gc.check(what + "out", out, o64, o32)
            gc.check(what + "lse", lse, l64, l32)
            gc.check(what + "d_qkv", dq, g64, g32)
    assert asserted == [4, 16]


# ---- 6. degenerate values ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", gc.ONE_PER_DP, ids=DP_IDS)
def test_degenerate_values(E, w):
    heads, d = w
    H, sizes = heads * d, [3, 70, 1, 64]
    qkv, gy = gc.attention_inputs("degenerate", sizes, heads, d)
    ptr = go.graph_ptr_of(sizes)
    # all keys of graph 1 equal: uniform weights, out is the mean of V, d_q is exactly 0
    same = qkv.clone()
    same[ptr[1]:ptr[2], H:2 * H] = same[ptr[1], H:2 * H]
    out, lse, dq, _ = run_op(E, same, gy, sizes, heads)
    (o64, l64, g64), (o32, l32, g32) = gc.attention_oracle(same, gy, sizes, heads)
    what = "%s equal keys " % gc.width_id(w)
    gc.check(what + "out", out, o64, o32)
    gc.check(what + "d_qkv", dq, g64, g32)
    rows = slice(ptr[1], ptr[2])
    mean_v = same[rows, 2 * H:].double().mean(0, keepdim=True).expand(sizes[1], H)
    gc.check(what + "out against the mean of V", out[rows], mean_v, o32[rows])
    q = same[rows, :H].double().reshape(sizes[1], heads, d)
    k = same[ptr[1], H:2 * H].double().reshape(heads, d)
    want_lse = ((q * k).sum(2) / math.sqrt(d) + math.log(sizes[1])).T
    gc.check(what + "lse = s + log n", lse[:, rows], want_lse, l32[:, rows])
    d_q = dq[rows, :H]
    print("%sd_q: largest |value| %.3g (d_k: %.3g)" % (what, float(d_q.abs().max()), float(dq[rows, H:2 * H].abs().max())))
    assert not bool(d_q.any()), "d_q of a graph whose keys are all equal must be exactly 0"
    # a zero upstream gradient: d_qkv is all zero
    zero = run_op(E, qkv, torch.zeros_like(gy), sizes, heads)[2]
    assert zero.shape == (sum(sizes), 3 * H) and not bool(zero.any())
    # the one-node graph: out = v, lse = s, d_q = d_k = 0, d_v = the upstream gradient
    out, lse, dq, _ = run_op(E, qkv, gy, sizes, heads)
    r = ptr[2]
    assert torch.equal(out[r].cpu(), qkv[r, 2 * H:])
    s = (qkv[r, :H].double() * qkv[r, H:2 * H].double()).reshape(heads, d).sum(1) / math.sqrt(d)
    gc.check("%s one node lse = s" % gc.width_id(w), lse[:, r], s, s.float())
    assert not bool(dq[r, :2 * H].any()) and torch.equal(dq[r, 2 * H:].cpu(), gy[r])


# ---- 7. the layer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("embed,heads", [(48, 4), (64, 2), (60, 1)])
def test_attention_layer_against_torch_multihead_attention(E, embed, heads):
    """head_dim 12 (padded to 16), 32 and 60 (padded to 64) through GraphMultiheadAttention against torch.nn.MultiheadAttention
    on the padded batch in fp64"""
    sizes = [1, 2, 37, 64, 65, 130, 3]
    torch.manual_seed(100 + embed)
    ref = torch.nn.MultiheadAttention(embed, heads, batch_first=True)
    torch.nn.init.normal_(ref.in_proj_bias)
    torch.nn.init.normal_(ref.out_proj.bias)
    mine = E.nn.GraphMultiheadAttention(embed, heads)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(DEV)
    x = torch.randn(sum(sizes), embed)
    want32 = go.padded_attention(ref, x, sizes).detach()
    want = go.padded_attention(ref.double(), x.double(), sizes).detach()
    got = mine(x.to(DEV), graph_ptr(sizes), max(sizes))
    gc.check("GraphMultiheadAttention %d / %d heads" % (embed, heads), got, want, want32)


# ---- 8. the encoder ----------------------------------------------------------------------------------------------------------------
def run_encoder(E, case):
    vecs, vals, signs, params, gy = case[:5]
    ps = [q.to(DEV).requires_grad_(True) for q in params]
    out = E.ops.lappe_encode(vecs.to(DEV), vals.to(DEV), None if signs is None else signs.to(DEV), *ps)
    out.backward(gy.to(DEV))
    return out.detach(), [q.grad for q in ps]


def check_encoder(E, case, what):
    (o64, g64), (o32, g32) = case[5:]
    out, grads = run_encoder(E, case)
    gc.check(what + "out", out, o64, o32)
    for name, g, a, b in zip(gc.PARAMS, grads, g64, g32):
        gc.check(what + "d " + name, g, a, b)
    out2, grads2 = run_encoder(E, case)
    assert same_bits(out, out2) and all(same_bits(a, b) for a, b in zip(grads, grads2)), "not bit-identical run to run"
    return out, grads


@pytest.mark.parametrize("c", gc.ENC_CASES, ids=gc.enc_id)
def test_encoder_on_every_width_and_chunk_cut(E, c):
    K, P = c
    for n in gc.ENC_ROWCOUNTS:
        for signed in (False, True):
            check_encoder(E, gc.enc_case(K, P, n, signed), "K %d P %d N %d %s " % (K, P, n, "signs" if signed else "plain"))


@pytest.mark.parametrize("c", gc.NAN_CASES, ids=gc.enc_id)
def test_encoder_on_nan_ragged_rows(E, c):
    """paths of 1 .. K+2 nodes (dropped terms on either side of the chunk boundaries) and a row that is NaN throughout: that
    row's output is exactly zero and removing it changes no gradient bit"""
    K, P = c
    for signed in (False, True):
        case = gc.enc_case(K, P, 0, signed, nan_ragged=True)
        out, grads = check_encoder(E, case, "K %d P %d nan-ragged %s " % (K, P, "signs" if signed else "plain"))
        n = case[0].size(0)
        assert out.shape == (n, P) and not bool(out[n - 1].any()) and bool(torch.isfinite(out).all())
        vecs, vals, signs, params, gy = case[:5]
        out_w, grads_w = run_encoder(E, (vecs[:n - 1], vals[:n - 1], signs, params, gy[:n - 1]))
        assert same_bits(out_w, out[:n - 1]) and all(same_bits(a, b) for a, b in zip(grads, grads_w)), "the NaN row changed a gradient"


# ---- 9. the gather -----------------------------------------------------------------------------------------------------------------
def _raw_gather(E, vecs_all, vals_all, node_ptr_all, ids, gp, N, K, G_all=None, N_all=None, B=None):
    nv = E._native
    vecs, vals = torch.full((max(N, 1), K), FILL, device=DEV), torch.full((max(N, 1), K), FILL, device=DEV)
    np_all = torch.tensor(node_ptr_all, dtype=torch.int64, device=DEV)
    ids_d, gp_d = torch.tensor(ids, dtype=torch.int64, device=DEV), torch.tensor(gp, dtype=torch.int32, device=DEV)
    nv.call("esc_lappe_gather", nv.ptr(vecs_all), nv.ptr(vals_all), nv.ptr(np_all), len(node_ptr_all) - 1 if G_all is None else G_all,
            vecs_all.size(0) if N_all is None else N_all, nv.ptr(ids_d), nv.ptr(gp_d), len(ids) if B is None else B, N, K, nv.ptr(vecs),
            nv.ptr(vals), nv.stream())
    return vecs, vals


@pytest.mark.parametrize("K", gc.GATHER_KS)
def test_gather_copies_the_tables_rows_and_skips_what_contradicts_them(E, K):
    vecs_all, vals_all, ptr, gp, want_vecs, want_vals = gc.gather_case(K)
    va, la = vecs_all.to(DEV), vals_all.to(DEV)
    ids, N = gc.GATHER_IDS, gp[-1]
    vals, vecs = E.ops.lappe_gather(va, la, torch.tensor(ptr, dtype=torch.int64, device=DEV), torch.tensor(ids), graph_ptr([gp[i + 1] - gp[i] for i in range(len(ids))]), N)
    assert vals.shape == (N, K, 1) and same_bits(vecs.cpu(), want_vecs) and same_bits(vals.view(N, K).cpu(), want_vals)
    vecs, vals = _raw_gather(E, va, la, ptr, ids, gp, N, K)              # the C entry point agrees
    assert same_bits(vecs.cpu(), want_vecs) and same_bits(vals.cpu(), want_vals)

    def verify(tag, res, skipped):
        for b in range(len(ids)):
            rows = slice(gp[b], gp[b + 1])
            for got, want in zip(res, (want_vecs, want_vals)):
                if b in skipped:
                    assert bool((got[rows] == FILL).all()), "%s: graph %d of the batch was written" % (tag, b)
                else:
                    assert same_bits(got[rows].cpu(), want[rows]), "%s: graph %d of the batch" % (tag, b)

    # the batch says 36 nodes where the table's graph 2 has 37 (the next range absorbs the row: 3 nodes for the table's 2)
    bad = list(gp)
    bad[4] -= 1
    verify("node count differs", _raw_gather(E, va, la, ptr, ids, bad, N, K), {3, 4})
    # an id outside the table, on either side
    verify("id past the table", _raw_gather(E, va, la, ptr, [4, 0, 5, 2, 3, 1], gp, N, K), {2})
    verify("negative id", _raw_gather(E, va, la, ptr, [4, -1, 0, 2, 3, 1], gp, N, K), {1})
    # the batch's last range leaves the batch (N stated 2 rows short)
    verify("range past N", _raw_gather(E, va, la, ptr, ids, gp, N - 2, K)[:2], {5})
    # the table's last range leaves the table (N_all stated 3 rows short): batch graph 0 reads the table's graph 4
    verify("table range past N_all", _raw_gather(E, va, la, ptr, ids, gp, N, K, N_all=vecs_all.size(0) - 3), {0})
    # a table range that decreases
    dec = list(ptr)
    dec[3] = 2
    verify("decreasing table range", _raw_gather(E, va, la, dec, ids, gp, N, K), {3, 4})
    # a batch range that starts before row 0
    neg = list(gp)
    neg[0] = -1
    verify("batch range before row 0", _raw_gather(E, va, la, ptr, ids, neg, N, K), {0})
    # nothing to do: B == 0, G_all == 0 and N == 0 write nothing
    for kw in ({"B": 0}, {"G_all": 0}):
        res = _raw_gather(E, va, la, ptr, ids, gp, N, K, **kw)
        assert bool((res[0] == FILL).all()) and bool((res[1] == FILL).all()), kw
    res = _raw_gather(E, va, la, ptr, ids, gp, 0, K)
    assert bool((res[0] == FILL).all()) and bool((res[1] == FILL).all())
    vecs, vals = _raw_gather(E, va, la, ptr, ids, gp, N, K)              # a valid call after these is correct
    assert same_bits(vecs.cpu(), want_vecs) and same_bits(vals.cpu(), want_vals)
