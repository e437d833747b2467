"""The step engines' schedule (esc-gnn_amd/csrc/engine_plan.h: plan_schedule, plan_schedule_zinc, plan_schedule_ogb) written down a
second time, from the rules the bodies of engine.hip applied between their launches before the schedule existed: which
Linear+BatchNorm pairs take their statistics from a GEMM epilogue, where the edge terms are issued, which backward GEMMs carry a
BatchNorm backward, who leaves whose column sums.  tests/test_engine_schedule_cpu.py holds tests/engine_schedule_host.cpp to it.

The host program's operands: the workspace is 256-byte aligned and every buffer in it starts on a 256-byte granule, so every
workspace operand is 16-byte aligned; the parameters are aligned unless a `misalign` bit moves their group (bit 0 the readout's
weights, bit 1 the node MLPs' weights, bit 2 the BatchNorms' gamma / beta).  Knobs at their defaults except `agg_split_bwd` and
the bag's `bag_tiled` (bit 3 of `misalign`)."""
import collections

EDGE_ROWS, BNB_MAX_N, SMALL_MAX, SMALLN_DX_MAX_N, NARROW_K = 8192, 640, 16, 848, 256      # linear_plan.h
READOUT_DX_LDS = 84 * 1024                                                               # engine_plan.h kReadoutDxLds
EVAL, STATS, PARTIALS, MERGED = range(4)                     # BnMode
PLAIN, AFFINE, AFFINE_STATS = range(3)                       # AggBwd
OWN, FROM_READOUT, FROM_AGGREGATE = range(3)                 # SumsFrom
Mode = collections.namedtuple("Mode", "train two_stream deferred sync l1_head plain_events readout_one_launch")


def cdiv(a, b):
    return -(-a // b)


def tile128_ok(dim):
    return cdiv(dim, 128) * 128 * 10 <= dim * 11


def big(M, N, K):
    return M >= EDGE_ROWS and tile128_ok(N) and tile128_ok(K)


def dma_ok(aligned, ld, rows):
    return aligned and ld % 4 == 0 and rows * ld * 4 < 2 ** 31


def both_bn(M, N, K, dOut_ld, X_ld, W_ld, dX_ld, w_aligned, bn_ld=None, next_ld=None, has_dx=True, dual=0):
    """esc_linear_bwd_both_bn's plan -> (served, launches).  bn_ld: leading dimension of the rows the folded BatchNorm normalised
    (None: none folded in); next_ld: of the rows of the BatchNorm whose column sums the dX epilogue leaves (None: none)"""
    no = (False, 1)
    if M <= 1 or N <= 0 or K <= 0 or (bn_ld is None and next_ld is None):
        return no
    if M >= EDGE_ROWS and not (big(M, N, K) and bn_ld is not None and N <= BNB_MAX_N):
        return no
    if bn_ld is not None and not (bn_ld >= N and dma_ok(True, bn_ld, M)):
        return no
    if bn_ld is not None and K <= SMALL_MAX and SMALL_MAX < N <= SMALLN_DX_MAX_N and N % 4 == 0:       # the in_dim-wide kernels
        if next_ld is not None or dOut_ld % 4 or dOut_ld < N or X_ld < K or W_ld < K or (has_dx and dX_ld < K):
            return no
        return (True, 1)
    if not has_dx or N > BNB_MAX_N:
        return no
    if N <= 32 or K <= 32 or N % 4 or K % 4 or not dma_ok(True, dOut_ld, M):
        return no
    if not (dma_ok(w_aligned, W_ld, N) and dma_ok(True, dX_ld, M) and dma_ok(True, X_ld, M)):
        return no
    if next_ld is not None and not (next_ld >= K and next_ld % 4 == 0 and K % 4 == 0 and dX_ld % 4 == 0):
        return no
    return (True, 2 if dual > 0 else 1)


def pair_mode(mode, M, width):
    if not mode.train:
        return EVAL
    if not (width > 32 and mode.deferred):
        return STATS
    return MERGED if (M > 1 and not mode.sync) else PARTIALS


def edge_terms(L, batched, own0, skip0, two_stream):
    up, behind = [0] * L, [-1] * L
    if batched:
        up[0] = int(own0)
        return up, behind
    ahead = 1 if two_stream else L
    for l in range(1 if skip0 else 0, min(L, ahead)):
        up[l] = 1
    for l in range(L):
        if two_stream and l + ahead < L:
            behind[l] = l + ahead
    return up, behind


def _terms(out, L, batched, own0, skip0, two_stream):
    up, behind = edge_terms(L, batched, own0, skip0, two_stream)
    out["batched"], out["up"], out["behind"] = [int(batched)], up, behind


def agg_stats_served(C, agg_split_bwd=1):
    return not (agg_split_bwd == 2 and C == 256) and C <= 2048


def count(L, H, C0, N, E, mode, misalign=0, agg_split_bwd=1):
    W = (L + 1) * H
    readout_al, mlp_al = not misalign & 1, not misalign & 2
    o = collections.OrderedDict()
    o["zlin"] = [pair_mode(mode, E, H)]
    o["xemb"] = [pair_mode(mode, N, H)] * 2
    o["conv0"] = o["conv1"] = [pair_mode(mode, N, H)] * L
    o["readout"] = [pair_mode(mode, N, H)]
    # the bag's statistics epilogue needs the tiled forward (off by default; `misalign` bit 3 switches it on): 128-edge blocks
    tiled = bool(misalign & 8) and H % 4 == 0 and E >= 4 * 128
    o["bag"] = [128 if mode.train and not mode.sync and tiled else 0]
    e0 = C0 <= 32 and L >= 1
    o["e0"] = [int(e0)]
    _terms(o, L, L >= 3, not e0, e0, mode.two_stream)
    node_act = H >= 64 and H % 4 == 0
    o["node_act"] = [int(node_act)]
    # the L1 head: the narrow forward (one output column, K <= 256) with bn_lin1's coefficients in its prologue
    o["l1"] = [int(mode.l1_head and mode.two_stream and H <= 1024 and H <= NARROW_K and H % 4 == 0 and readout_al)]
    none = [0, 0, OWN, 0]
    mlp = [list(none) for _ in range(L)]
    xemb = list(none)
    agg = [PLAIN] * L
    split = fuse_lin1 = ask = dx_split = last_dw = False
    if mode.train:
        split = mode.two_stream and mode.deferred and L >= 1

        def lin1(ncols, nxt=False, dual=0):
            return both_bn(N, H, ncols, H, W, W, W, readout_al, bn_ld=H, next_ld=W if nxt else None, dual=dual)

        fuse_lin1 = not mode.sync and ((lin1(L * H)[0] and lin1(H)[0]) if split else lin1(W)[0])

        def fuse(C, has_dx):
            if mode.sync:
                return 0, 0
            f1 = both_bn(N, H, H, W, H, H, H, mlp_al, bn_ld=W if node_act else H, next_ld=H)[0]
            f0 = f1 and both_bn(N, H, C, H, C, C, C if has_dx else 0, mlp_al, bn_ld=H, has_dx=has_dx)[0]
            return int(f1), int(f0)

        for l in range(L):
            mlp[l][0], mlp[l][1] = fuse(C0 if l == 0 else H, True)
        xemb[0], xemb[1] = fuse(C0, False)
        if split:
            ask = fuse_lin1 and not mode.readout_one_launch and not mode.plain_events
            dx_split = ask and lin1(L * H, dual=READOUT_DX_LDS)[1] == 2
            if fuse_lin1 and node_act and lin1(H, nxt=True)[0] and mlp[L - 1][0]:
                mlp[L - 1][2:] = [FROM_READOUT, cdiv(N, 128 if big(N, H, H) else 64)]
        for l in range(1, L):
            if not node_act:
                continue
            agg[l] = AFFINE
            if agg_stats_served(H, agg_split_bwd) and mlp[l - 1][0]:
                agg[l] = AFFINE_STATS
                mlp[l - 1][2:] = [FROM_AGGREGATE, cdiv(N, 4)]
        last_dw = mode.two_stream and mode.deferred
    o["split"], o["fuse_lin1"], o["ask"], o["dx_split"], o["last_dw"] = [int(split)], [int(fuse_lin1)], [int(ask)], [int(dx_split)], [int(last_dw)]
    o["agg"], o["xemb_bwd"] = agg, xemb
    for l in range(L):
        o["mlp%d" % l] = mlp[l]
    o["cap"] = [N // 4 + 2]
    return o


def zinc(L, H, C0, node_readout, N, E, G, mode):
    o = collections.OrderedDict()
    o["zlin"] = [pair_mode(mode, E, H)]
    o["xemb"] = [EVAL, EVAL]                                  # (no x_embedding MLP)
    o["conv0"] = o["conv1"] = [pair_mode(mode, N, H)] * L
    o["readout"] = [pair_mode(mode, N if node_readout else G, H)]
    o["bag"], o["e0"] = [0], [0]
    lb = 0 if C0 == H else 1
    _terms(o, L, L - lb >= 2, C0 != H, False, mode.two_stream)
    for k in ("node_act", "l1", "split", "fuse_lin1", "ask", "dx_split", "last_dw"):     # ELU, materialised activations: no fusion
        o[k] = [0]
    o["agg"], o["xemb_bwd"] = [PLAIN] * L, [0, 0, OWN, 0]
    for l in range(L):
        o["mlp%d" % l] = [0, 0, OWN, 0]
    o["cap"] = [N // 4 + 2]
    return o


def ogb(L, H, drop, N, E, G, mode, misalign=0):
    o = collections.OrderedDict()
    p = drop if mode.train else 0
    o["zlin"] = [pair_mode(mode, E, 0 if p > 0 else H)]      # (with dropout: the Linear, the dropout, then a statistics pass)
    o["lin0"] = [pair_mode(mode, N, 2 * H)] * L
    o["lin1"] = [pair_mode(mode, N, H)] * L
    o["vlin0"] = [pair_mode(mode, G, 2 * H)] * (L - 1) + [EVAL]
    o["vlin1"] = [pair_mode(mode, G, H)] * (L - 1) + [EVAL]
    _terms(o, L, False, False, False, mode.two_stream)
    hidden = drop_site = False
    if mode.train:
        hidden = not mode.sync and both_bn(N, H, 2 * H, H, 2 * H, 2 * H, 2 * H, not misalign & 2, next_ld=2 * H)[0]
        drop_site = p > 0 and not mode.sync and H % 4 == 0 and not misalign & 4
    o["hidden"] = [int(hidden)] * L
    o["hidden_slots"] = [cdiv(N, 128 if big(N, H, 2 * H) else 64) if mode.train else 0]
    o["bonds_on_node"] = [int(mode.train and mode.two_stream)]
    o["drop_h"] = [int(drop_site)] * L
    o["drop_v"] = [int(drop_site)] * (L - 1) + [0]
    o["drop_z1"] = o["drop_z0"] = [int(drop_site)]
    o["cap"] = [N // 64 + 2]
    return o


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
COUNT_MODELS = ((1, 32, 10), (2, 64, 10), (3, 64, 10), (3, 60, 10), (4, 256, 10), (3, 64, 64), (14, 64, 10), (15, 64, 10),
                (3, 64, 32))                                  # (L, H, in_dim); the last: in_dim AT the e0_early threshold
ZINC_MODELS = tuple((L, 256, C0, nr) for L in (1, 2, 3, 16) for C0 in (32, 256) for nr in (0, 1))      # node width != / == hidden, both readouts
OGB_MODELS = tuple((L, H, drop) for (L, H) in ((2, 32), (2, 64), (5, 300), (10, 64)) for drop in (0, 500))   # drop ratio in thousandths
CASE_BATCHES = ("minimal", "mixed", "rows_64", "rows_65", "rows_129")          # engine_cases.CLAIMS: (N, E) 5/11 63/156 64/190 65/193 129/385
MODES = tuple(Mode(*(bool(bits >> i & 1) for i in range(7))) for bits in range(128))
