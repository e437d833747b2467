"""Case tables of the graph-transformer kernels (csrc/attention.hip, csrc/lappe.hip) on every compiled width, tile edge and skip:
every head_dim instantiation DP = 4 .. 64 at a width that equals it and at a padded one, the per-width node limit, both block
sizes, the second row trip, the exact-logit ladder, every dim_pe instantiation PP = 4 .. 32 of the LapPE encoder with chunk cuts
inside a node's terms, and the gather.  No GPU here and nothing from the package: tests/test_gps_cases_cpu.py proves what every
case claims about itself and that the fp32 oracle is well conditioned on it; tests/test_hip_gps_structure.py runs the tables
through the kernels.

The constants and small functions under "what the kernels do" restate the host-side rules of the two files (padding, limit, block
size, LDS request, chunk length); the device test holds the limit to the library's own answer.

Error measure and bound are the project's: max |got - want| over the largest |want| of the tensor, bound 1e-5; a tensor of zeros
must be matched exactly.  CAP is the conditioning cap: the oracle's own fp32 evaluation stays within 2e-6 of its fp64 evaluation
on every asserted case and tensor - a fifth of the bound, so the bound cannot hide a kernel error of its own size."""
import math

import torch

import gps_oracle as go
import lappe_oracle as lo
import loss_cases as lc

BOUND = lo.BOUND
CAP = 2e-6
assert BOUND == 1e-5


# ---- the error measure -------------------------------------------------------------------------------------------------------------
def rel(got, want):
    """max |got - want| over the largest |want|; a tensor of zeros must be matched exactly"""
    got, want = got.detach().cpu().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    return err / scale if scale > 0 else (0.0 if err == 0 else math.inf)


def check(what, got, want64, want32, width=52):
    """print the kernel's figure beside the oracle's own fp32 figure, then assert the bound"""
    e, e32 = rel(got, want64), rel(want32, want64)
    print("%-*s kernel %.3g   torch fp32 on the CPU %.3g" % (width, what, e, e32))
    assert e <= BOUND, "%s: %.3g of the largest value, bound %g (torch fp32: %.3g)" % (what, e, BOUND, e32)
    return e, e32


# ---- what the kernels do: attention ------------------------------------------------------------------------------------------------
ATTN_PADS = (4, 8, 16, 32, 64)
ATTN_LDS_FLOATS, ATTN_MAX_NODES = 32768, 1024


def attn_pad(d):
    """DP: the compiled width head_dim d runs at"""
    return next(w for w in ATTN_PADS if d <= w)


def attn_limit(d):
    """esc_graph_attention_max_nodes(d): K and V of one (graph, head) inside 128 KiB of LDS, 1024 at most"""
    return min(ATTN_LDS_FLOATS // 2 // attn_pad(d), ATTN_MAX_NODES)


def attn_block(max_nodes):
    """threads per workgroup at the announced size"""
    return 64 if max_nodes <= 64 else 256


def attn_lds_bytes(d, max_nodes, backward):
    """the dynamic LDS a launch asks for: two tiles of cap rows, plus lse and delta of the rows in the backward"""
    cap = (max_nodes + 3) & ~3
    return (2 * cap * attn_pad(d) + (2 * cap if backward else 0)) * 4


# (heads, head_dim): every DP; for 16, 32 and 64 a width that equals DP and a padded one; head counts odd where above 1
WIDTHS = [(5, 4), (3, 8), (3, 12), (1, 16), (2, 20), (1, 24), (2, 28), (2, 32), (1, 36), (1, 48), (1, 60), (1, 64)]
ONE_PER_DP = [(5, 4), (3, 8), (3, 12), (2, 28), (1, 60)]         # a padded width wherever the DP has one
SIZE_SETS = ("wave", "block", "limit", "holes")
DROP_SETS = ("wave", "block")
DROP_PS = (0.25, 0.5)


def sizes_of(name, d):
    L = attn_limit(d)
    return {"wave": [2, 63, 64, 1],                              # the 64-thread block with full and partial waves
            "block": [255, 256, 257] if L >= 257 else [L - 1, L],  # the first row of the second trip
            "limit": [3, L, 1],                                  # the limit inside a batch: n0 != 0
            "holes": [0, 5, 0, 0, 70, 0]}[name]


def width_id(w):
    return "%dx%d" % w


def attention_inputs(tag, sizes, heads, d):
    """qkv (fp32, unit variance) and the upstream gradient cos(arange), drawn as test_hip_gps.reference draws them"""
    N, H = sum(sizes), heads * d
    gen = torch.Generator().manual_seed(lc.seed_of("gps-%s-%d-%d" % (tag, heads, d)))
    qkv = torch.randn((N, 3 * H), generator=gen)
    gy = torch.cos(torch.arange(N * H, dtype=torch.float64)).reshape(N, H).float()
    return qkv, gy


def attention_oracle(qkv, gy, sizes, heads, keep=None, p=0.0):
    """(out, lse, d_qkv) of the oracle in fp64 and in fp32 on the CPU"""
    res = []
    for dtype in (torch.float64, torch.float32):
        x = qkv.clone().to(dtype).requires_grad_(True)
        out, lse = go.ragged_attention(x, sizes, heads, keep, p)
        out.backward(gy.to(dtype))
        res.append((out.detach(), lse.detach(), x.grad))
    return tuple(res)


_ATT = {}


def attention_case(name, heads, d):
    """(sizes, qkv, gy, fp64 results, fp32 results) of one width on one size set at p = 0: computed once, shared, never modified"""
    key = (name, heads, d)
    if key not in _ATT:
        sizes = sizes_of(name, d)
        qkv, gy = attention_inputs(name, sizes, heads, d)
        _ATT[key] = (sizes, qkv, gy) + attention_oracle(qkv, gy, sizes, heads)
    return _ATT[key]


def standin_keep(sizes, heads, p, tag):
    """a seeded Bernoulli keep mask in the oracle's layout, for the conditioning check on the CPU (the device test feeds the
    kernel's own mask)"""
    gen = torch.Generator().manual_seed(lc.seed_of("gps-keep-" + tag))
    return [(torch.rand((heads, n, n), generator=gen) >= p).to(torch.uint8) for n in sizes]


# ---- the exact-logit ladder --------------------------------------------------------------------------------------------------------
LADDER_DIMS = (4, 16, 64)                 # 1 / sqrt(d) is a power of two
LADDER_HEADS = 2
LADDER_SIZES = [1, 2, 37, 64, 65]
LADDER_AMPS = (4, 16, 32, 64)


def ladder_inputs(d, amp):
    """qkv from the integers -amp .. amp over 4: every product is a multiple of 1/16 and every logit a sum of at most 64 of them
    times a power of two, below 2^24 units of its last place: exact in fp32 in any order"""
    assert d in LADDER_DIMS and 2.0 ** round(math.log2(d) / 2) == math.sqrt(d)
    assert d * amp * amp < 2 ** 24
    N, H = sum(LADDER_SIZES), LADDER_HEADS * d
    gen = torch.Generator().manual_seed(lc.seed_of("gps-ladder-%d-%d" % (d, amp)))
    qkv = torch.randint(-amp, amp + 1, (N, 3 * H), generator=gen).float() / 4.0
    gy = torch.cos(torch.arange(N * H, dtype=torch.float64)).reshape(N, H).float()
    return qkv, gy


_LADDER = {}


def ladder_case(d, amp):
    key = (d, amp)
    if key not in _LADDER:
        qkv, gy = ladder_inputs(d, amp)
        _LADDER[key] = (qkv, gy) + attention_oracle(qkv, gy, LADDER_SIZES, LADDER_HEADS)
    return _LADDER[key]


def ladder_lse(d, amp):
    """the oracle's largest |lse| of the rung"""
    return float(ladder_case(d, amp)[2][1].abs().max())


def ladder_asserted(d, amp):
    """a rung is held to the bound when the one fp32 lse the backward recomputes P from costs at most half of it:
    max |lse| * 2^-23 <= BOUND / 2"""
    return ladder_lse(d, amp) * 2.0 ** -23 <= BOUND / 2


def ladder_expected(d, amp):
    """the error the design accepts in the recomputed P: |lse| * 2^-24 (half an ulp of lse, relative in exp(s - lse))"""
    return ladder_lse(d, amp) * 2.0 ** -24


# ---- what the kernels do: the LapPE encoder ----------------------------------------------------------------------------------------
ENC_PADS = (4, 8, 16, 32)
ENC_ROWS = 32


def enc_pad(P):
    """PP: the compiled width dim_pe P runs at"""
    return next(w for w in ENC_PADS if P <= w)


def enc_chunk(P):
    """T: terms per chunk of the backward"""
    return min(2048 // enc_pad(P), 256)


def enc_cut(K, P):
    """(terms of a block, full chunks, terms of the partial chunk after them, chunk boundaries that fall inside a node's K terms)"""
    terms, T = ENC_ROWS * K, enc_chunk(P)
    inside = sum(1 for c0 in range(T, terms, T) if c0 % K)
    return terms, terms // T, terms % T, inside


# (K, P): the chunk cut each is there for is ENC_CUTS[(K, P)] = (terms, full chunks, partial chunk, boundaries inside a node)
ENC_CASES = [(1, 4), (3, 8), (5, 16), (7, 12), (9, 16), (31, 32), (5, 20), (3, 28), (13, 24), (32, 4), (2, 32)]
ENC_CUTS = {
    (1, 4): (32, 0, 32, 0),            # PP 4 exact; one partial chunk only, K = 1
    (3, 8): (96, 0, 96, 0),            # PP 8 exact; one partial chunk, odd K
    (5, 16): (160, 1, 32, 1),          # PP 16 exact; 160 = 128 + 32: a partial chunk after a full one, the cut inside a node
    (7, 12): (224, 1, 96, 1),          # PP 16 padded; 224 = 128 + 96
    (9, 16): (288, 2, 32, 2),          # 288 = 2 * 128 + 32
    (31, 32): (992, 15, 32, 15),       # PP 32 exact; 992 = 15 * 64 + 32: every boundary inside a node
    (5, 20): (160, 2, 32, 2),          # PP 32 padded; 160 = 2 * 64 + 32
    (3, 28): (96, 1, 32, 1),           # PP 32 padded; 96 = 64 + 32
    (13, 24): (416, 6, 32, 6),         # PP 32 padded; 416 = 6 * 64 + 32
    (32, 4): (1024, 4, 0, 0),          # the widest K at the narrowest P: four full chunks of 256, no partial one
    (2, 32): (64, 1, 0, 0),            # exactly one full chunk of 64
}
ENC_ROWCOUNTS = (1, 31, 32, 33, 97)     # the 32-row partition's edges and a fourth block of one row
NAN_CASES = [(5, 16), (9, 16), (31, 32)]
PARAMS = ("linear_A.weight", "linear_A.bias", "pe_encoder.1.weight", "pe_encoder.1.bias")


def enc_id(c):
    return "K%d-P%d" % c


def enc_weights(K, P):
    """normal with std 1 / sqrt(fan-in) for the two weight matrices (fan-in 2 and 2P) and 0.1 for the two biases: hidden and
    output activations of order 1 at every P"""
    gen = torch.Generator().manual_seed(lc.seed_of("lappe-weights-%d-%d" % (K, P)))
    return [torch.randn((2 * P, 2), generator=gen) / math.sqrt(2.0), torch.randn((2 * P,), generator=gen) * 0.1,
            torch.randn((P, 2 * P), generator=gen) / math.sqrt(2.0 * P), torch.randn((P,), generator=gen) * 0.1]


def nan_ragged_rows(K):
    """eigen-data of paths of 1 .. K+2 nodes (columns j >= n NaN: the NaN columns straddle the chunk boundaries), then one row
    that is NaN throughout"""
    parts = [lo.lap_pe(m, lo._both(lo._path(m)), K) for m in range(1, K + 3)]
    vals = torch.cat([torch.from_numpy(a).float().view(-1, K) for a, _ in parts] + [torch.full((1, K), float("nan"))])
    vecs = torch.cat([torch.from_numpy(b).float() for _, b in parts] + [torch.full((1, K), float("nan"))])
    return vecs, vals


_ENC = {}


def enc_case(K, P, n, signed, nan_ragged=False):
    """(vecs, vals, signs, params, gy, (out64, grads64), (out32, grads32)): computed once per case, shared, never modified;
    n is ignored for the nan-ragged variant (its row count follows from K).  Eigen-data as test_hip_lappe draws them; the
    upstream gradient is N(0, 1) from the case's generator, not cos(arange): at P = 32 that advances 32 = 0.58 (mod 2 pi) per
    row, a slow wave under which the partial sums of a weight gradient over the 31 non-negative terms of every row grow to
    about a hundred terms while the total stays near forty - the fp32 oracle's own sum then loses up to 1e-5 of the tensor's
    largest value, whatever the weights (test_gps_cases_cpu measured 2.4e-6 to 1e-5 at (31, 32) for every weight scale tried)."""
    key = (K, P, None if nan_ragged else n, signed, nan_ragged)
    if key not in _ENC:
        gen = torch.Generator().manual_seed(lc.seed_of("lappe-data-%d-%d-%s" % (K, P, "ragged" if nan_ragged else n)))
        if nan_ragged:
            vecs, vals = nan_ragged_rows(K)
        else:
            vecs = torch.randn((n, K), generator=gen) * 0.3
            vals = torch.rand((n, K), generator=gen) * 4.0
        signs = torch.where(torch.rand(K, generator=gen) >= 0.5, 1.0, -1.0) if signed else None
        params = enc_weights(K, P)
        gy = torch.randn((vecs.size(0), P), generator=gen)
        _ENC[key] = (vecs, vals, signs, params, gy) + enc_oracle(vecs, vals, signs, params, gy)
    return _ENC[key]


def enc_oracle(vecs, vals, signs, params, gy):
    res = []
    P = params[3].numel()
    for dtype in (torch.float64, torch.float32):
        e = lo.LapPEEncoder(P).to(dtype)
        e.load_state_dict({name: q.to(dtype) for name, q in zip(PARAMS, params)})
        out = e(vecs.to(dtype), vals.to(dtype), None if signs is None else signs.to(dtype))
        out.backward(gy.to(dtype))
        res.append((out.detach(), [q.grad for q in e.parameters()]))
    return tuple(res)


# ---- the gather --------------------------------------------------------------------------------------------------------------------
GATHER_TABLE = [1, 4, 37, 2, 9]           # nodes of the table's graphs
GATHER_IDS = [4, 0, 0, 2, 3, 1]           # the batch: a repeated id, every graph
GATHER_KS = (3, 8)


def gather_case(K):
    """(vecs_all, vals_all, node_ptr_all, batch graph_ptr, expected vecs, expected vals): distinct values everywhere"""
    n_all = sum(GATHER_TABLE)
    vecs_all = torch.arange(n_all * K, dtype=torch.float32).reshape(n_all, K) + 0.5
    vals_all = -(torch.arange(n_all * K, dtype=torch.float32).reshape(n_all, K)) - 0.25
    ptr = go.graph_ptr_of(GATHER_TABLE)
    rows = torch.cat([torch.arange(ptr[g], ptr[g + 1]) for g in GATHER_IDS])
    graph_ptr = go.graph_ptr_of([GATHER_TABLE[g] for g in GATHER_IDS])
    return vecs_all, vals_all, ptr, graph_ptr, vecs_all[rows], vals_all[rows]
