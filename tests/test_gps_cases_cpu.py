"""tests/gps_cases.py on the CPU: every case is what it claims to be - the compiled width each head_dim and dim_pe runs at, the
node limit per width, the block size and the LDS request each size set selects, the second row trip, the chunk cut of every
encoder case - and the fp32 oracle is well conditioned on it: its own error against the fp64 oracle stays under the cap (2e-6, a
fifth of the bound) on every asserted case and tensor, so the bound of tests/test_hip_gps_structure.py cannot hide a kernel error
of the bound's own size.  The cap is a condition on the inputs: a case that misses it gets other inputs, never a looser bound."""
import math

import pytest
import torch

import gps_cases as gc

WIDTH_IDS = [gc.width_id(w) for w in gc.WIDTHS]


# ---- attention: what the cases reach ---------------------------------------------------------------------------------------------
def test_every_compiled_width_is_reached_exact_and_padded():
    pads = {w: gc.attn_pad(w[1]) for w in gc.WIDTHS}
    assert pads == {(5, 4): 4, (3, 8): 8, (3, 12): 16, (1, 16): 16, (2, 20): 32, (1, 24): 32, (2, 28): 32, (2, 32): 32, (1, 36): 64,
                    (1, 48): 64, (1, 60): 64, (1, 64): 64}
    assert set(pads.values()) == set(gc.ATTN_PADS)
    for dp in (16, 32, 64):                                   # a width that equals DP and one that is padded to it
        ds = [w[1] for w in gc.WIDTHS if pads[w] == dp]
        assert dp in ds and any(d < dp for d in ds), (dp, ds)
    assert all(h % 2 == 1 for h, d in gc.WIDTHS if h > 1 and d <= 12)       # odd head counts where the table has more than two
    assert all(d % 4 == 0 and 0 < d <= 64 for h, d in gc.WIDTHS)
    assert sorted(gc.attn_pad(d) for h, d in gc.ONE_PER_DP) == list(gc.ATTN_PADS) and set(gc.ONE_PER_DP) <= set(gc.WIDTHS)
    assert [d < gc.attn_pad(d) for h, d in gc.ONE_PER_DP] == [False, False, True, True, True]      # 4 and 8 have no padded width


def test_limit_per_width():
    assert [gc.attn_limit(d) for d in (4, 8, 12, 16, 20, 32, 36, 64)] == [1024, 1024, 1024, 1024, 512, 512, 256, 256]
    for h, d in gc.WIDTHS:
        L = gc.attn_limit(d)
        assert 2 * L * gc.attn_pad(d) <= gc.ATTN_LDS_FLOATS and L <= gc.ATTN_MAX_NODES
        assert gc.attn_lds_bytes(d, L, True) <= 160 * 1024     # the CU's LDS


@pytest.mark.parametrize("w", gc.WIDTHS, ids=WIDTH_IDS)
def test_size_sets_select_what_they_claim(w):
    heads, d = w
    L, dp = gc.attn_limit(d), gc.attn_pad(d)
    sets = {s: gc.sizes_of(s, d) for s in gc.SIZE_SETS}
    # wave: the 64-thread block, a full wave (64), partial ones (2, 63) and a single row
    assert sets["wave"] == [2, 63, 64, 1] and gc.attn_block(max(sets["wave"])) == 64
    # block: 256 threads; 257 is the first row of the second trip wherever the limit admits it
    assert gc.attn_block(max(sets["block"])) == 256
    assert sets["block"] == ([255, 256, 257] if dp <= 32 else [255, 256]) and max(sets["block"]) <= L
    # limit: the limit inside a batch, its first row not row 0
    assert sets["limit"] == [3, L, 1] and gc.attn_block(L) == 256
    second_trip = [s for s in gc.SIZE_SETS if max(sets[s]) > gc.attn_block(max(sets[s]))]
    assert second_trip == (["block", "limit"] if dp <= 32 else []), second_trip        # at DP 64 the limit is the block: no second trip exists
    # the over-64 KiB request: both directions at DP 16 .. 64, the backward alone at DP 8, never at DP 4
    big = (gc.attn_lds_bytes(d, L, False) > 65536, gc.attn_lds_bytes(d, L, True) > 65536)
    assert big == {4: (False, False), 8: (False, True), 16: (True, True), 32: (True, True), 64: (True, True)}[dp]
    assert all(gc.attn_lds_bytes(d, max(sets[s]), True) <= 65536 for s in ("wave", "holes"))
    # holes: empty graphs at the head, in the middle and at the tail; 256 threads with 70 rows
    assert sets["holes"] == [0, 5, 0, 0, 70, 0] and gc.attn_block(70) == 256
    # the block-size switch of the bit-equality test: 64 announced against 65 on the wave set
    assert gc.attn_block(64) == 64 and gc.attn_block(65) == 256


# ---- attention: the conditioning cap ---------------------------------------------------------------------------------------------
def _worst(r32, r64):
    return max(gc.rel(a, b) for a, b in zip(r32, r64))


@pytest.mark.parametrize("w", gc.WIDTHS, ids=WIDTH_IDS)
def test_fp32_oracle_is_conditioned_on_the_attention_cases(w):
    heads, d = w
    for name in gc.SIZE_SETS:
        sizes, qkv, gy, r64, r32 = gc.attention_case(name, heads, d)
        assert qkv.shape == (sum(sizes), 3 * heads * d) and all(bool(torch.isfinite(t).all()) for t in r64 + r32)
        figures = [("p 0", _worst(r32, r64))]
        if name in gc.DROP_SETS or (name == "limit" and w in gc.ONE_PER_DP):       # a stand-in mask: the device draws its own
            for p in gc.DROP_PS:
                keep = gc.standin_keep(sizes, heads, p, "%s-%d-%d-%g" % (name, heads, d, p))
                b64, b32 = gc.attention_oracle(qkv, gy, sizes, heads, keep, p)
                figures.append(("p %g" % p, _worst(b32, b64)))
        print("%-6s %-6s " % (gc.width_id(w), name) + "  ".join("%s: %.3g" % f for f in figures))
        for what, e in figures:
            assert e <= gc.CAP, (name, what, e)


@pytest.mark.parametrize("d", gc.LADDER_DIMS)
def test_ladder_logits_are_exact_and_its_rungs_sort_themselves(d):
    asserted = []
    for amp in gc.LADDER_AMPS:
        qkv, gy, r64, r32 = gc.ladder_case(d, amp)
        H = gc.LADDER_HEADS * d
        assert bool((qkv * 4 == (qkv * 4).round()).all()) and float(qkv.abs().max()) == amp / 4.0
        q, k, o = qkv[:, :d], qkv[:, H:H + d], 0                  # head 0: every logit the same number in fp32 and in fp64
        for n in gc.LADDER_SIZES:
            s32 = (q[o:o + n] / math.sqrt(d)) @ k[o:o + n].T
            s64 = (q[o:o + n].double() @ k[o:o + n].double().T) / math.sqrt(d)
            assert torch.equal(s32.double(), s64)
            o += n
        lse, e = gc.ladder_lse(d, amp), _worst(r32, r64)
        print("d %2d amp %2d: max |lse| %.4g  asserted %s  expected |lse| 2^-24 = %.3g  torch fp32 %.3g"
              % (d, amp, lse, gc.ladder_asserted(d, amp), gc.ladder_expected(d, amp), e))
        assert gc.ladder_asserted(d, amp) == (lse * 2.0 ** -23 <= gc.BOUND / 2)
        if gc.ladder_asserted(d, amp):
            asserted.append(amp)
            assert e <= gc.CAP, (d, amp, e)
    assert asserted == [4, 16], asserted                          # max |lse| about 4.4 and 22; 87 and 330 above


# ---- the encoder -----------------------------------------------------------------------------------------------------------------
def test_every_encoder_width_is_reached_exact_and_padded():
    pads = {c: gc.enc_pad(c[1]) for c in gc.ENC_CASES}
    assert set(pads.values()) == set(gc.ENC_PADS)
    assert {c[1] for c in gc.ENC_CASES if pads[c] == 32} == {32, 20, 24, 28}        # PP 32: exact and every padded P
    assert {c[1] for c in gc.ENC_CASES if pads[c] == 16} == {16, 12}
    assert [gc.enc_chunk(P) for P in (4, 8, 12, 16, 20, 32)] == [256, 256, 128, 128, 64, 64]
    assert all(K % 2 == 1 for K, P in gc.ENC_CASES if (K, P) not in ((32, 4), (2, 32)))
    assert set(gc.NAN_CASES) <= set(gc.ENC_CASES)
    assert gc.ENC_ROWCOUNTS == (1, 31, 32, 33, 97) and -(-97 // gc.ENC_ROWS) == 4 and 97 % gc.ENC_ROWS == 1


@pytest.mark.parametrize("c", gc.ENC_CASES, ids=gc.enc_id)
def test_chunk_cut_of_every_encoder_case(c):
    K, P = c
    terms, full, part, inside = gc.enc_cut(K, P)
    T = gc.enc_chunk(P)
    assert (terms, full, part, inside) == gc.ENC_CUTS[c]
    assert terms == 32 * K == full * T + part and 0 <= part < T
    assert inside == sum(1 for b in range(1, full + (1 if part else 0)) if (b * T) % K)
    if c in ((5, 16), (9, 16), (31, 32), (7, 12), (5, 20), (3, 28), (13, 24)):
        assert full >= 1 and part > 0 and inside >= 1             # a partial chunk after a full one, the cut inside a node's terms
    assert gc.ENC_CUTS[(5, 16)] == (160, 1, 32, 1) and gc.ENC_CUTS[(9, 16)] == (288, 2, 32, 2) and gc.ENC_CUTS[(31, 32)] == (992, 15, 32, 15)


def test_nan_ragged_rows_straddle_the_chunk_boundaries():
    for K, P in gc.NAN_CASES:
        vecs, vals = gc.nan_ragged_rows(K)
        n = (K + 2) * (K + 3) // 2 + 1
        assert vecs.shape == vals.shape == (n, K) and bool(torch.isnan(vecs[-1]).all()) and bool(torch.isnan(vals[-1]).all())
        live = ~torch.isnan(vecs)
        assert torch.equal(live, ~torch.isnan(vals))
        assert live[0].tolist() == [True] + [False] * (K - 1) and bool(live[-2].all())       # the path of one node, the last of K+2
        T, terms = gc.enc_chunk(P), gc.ENC_ROWS * K
        pad = (-n) % gc.ENC_ROWS                                  # rows past N read as dropped terms
        flat = torch.cat([live, torch.zeros((pad, K), dtype=torch.bool)]).reshape(-1, terms)      # [block, term]: rows x K in row order
        mixed_full = mixed_part = cut_in_ragged_row = False
        for blk in flat:
            chunks = [blk[c0:c0 + T] for c0 in range(0, terms, T)]
            assert len(chunks) >= 2 and chunks[-1].numel() == terms % T == 32
            mixed_full |= any(bool(ch.any()) and not bool(ch.all()) for ch in chunks[:-1])
            mixed_part |= bool(chunks[-1].any()) and not bool(chunks[-1].all())
            for c0 in range(T, terms, T):
                row = blk[c0 // K * K:c0 // K * K + K]
                cut_in_ragged_row |= c0 % K != 0 and bool(row.any()) and not bool(row.all())
        # dropped and live terms meet inside a full chunk and inside the partial chunk after it; at K = 9 and 31 a boundary
        # also falls inside a row that has both
        assert mixed_full and mixed_part, (K, P)
        assert cut_in_ragged_row == (K != 5), (K, P)


@pytest.mark.parametrize("c", gc.ENC_CASES, ids=gc.enc_id)
def test_fp32_oracle_is_conditioned_on_the_encoder_cases(c):
    K, P = c
    runs = [(n, s, False) for n in gc.ENC_ROWCOUNTS for s in (False, True)]
    runs += [(0, s, True) for s in (False, True)] if c in gc.NAN_CASES else []
    worst = 0.0
    for n, signed, ragged in runs:
        vecs, vals, signs, params, gy, (o64, g64), (o32, g32) = gc.enc_case(K, P, n, signed, ragged)
        assert [tuple(q.shape) for q in params] == [(2 * P, 2), (2 * P,), (P, 2 * P), (P,)] and (signs is not None) == signed
        assert float(o64.abs().max()) > 0 and all(float(g.abs().max()) > 0 for g in g64)
        figures = [gc.rel(o32, o64)] + [gc.rel(a, b) for a, b in zip(g32, g64)]
        worst = max(worst, max(figures))
        for what, e in zip(("out",) + gc.PARAMS, figures):
            assert e <= gc.CAP, (c, n, signed, ragged, what, e)
    print("%s: worst fp32 figure %.3g" % (gc.enc_id(c), worst))


# ---- the gather and the measure --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", gc.GATHER_KS)
def test_gather_case(K):
    vecs_all, vals_all, ptr, graph_ptr, vecs, vals = gc.gather_case(K)
    assert ptr == [0, 1, 5, 42, 44, 53] and graph_ptr == [0, 9, 10, 11, 48, 50, 54]
    both = torch.cat([vecs_all.reshape(-1), vals_all.reshape(-1)])
    assert len(torch.unique(both)) == both.numel()                # distinct values: a row taken from the wrong place shows
    assert vecs.shape == vals.shape == (54, K) and torch.equal(vecs[9], vecs_all[0]) and torch.equal(vals[11:48], vals_all[5:42])
    assert sorted(set(gc.GATHER_IDS)) == list(range(len(gc.GATHER_TABLE))) and gc.GATHER_IDS.count(0) == 2


def test_error_measure_and_bound():
    t = torch.tensor([0.5, -4.0], dtype=torch.float64)
    assert gc.rel(torch.tensor([0.5, -4.0]), t) == 0.0
    assert math.isclose(gc.rel(torch.tensor([0.5, -3.0]), t), 0.25)
    z = torch.zeros(3, dtype=torch.float64)
    assert gc.rel(torch.zeros(3), z) == 0.0 and gc.rel(torch.tensor([0.0, 1e-30, 0.0]), z) == math.inf
    assert gc.BOUND == 1e-5 and gc.CAP == 2e-6 and gc.CAP * 5 <= gc.BOUND * (1 + 1e-12)
    with pytest.raises(AssertionError, match="bound 1e-05"):
        gc.check("x", torch.tensor([1.0 + 2e-5]), torch.tensor([1.0], dtype=torch.float64), torch.tensor([1.0]))
