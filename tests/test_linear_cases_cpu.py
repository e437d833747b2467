"""The dense-layer case table of tests/linear_cases.py checks itself: every family of every entry point is named, the
declared family is what the transcribed dispatcher picks, the guarded buffers are what they claim to be, the fp64
references ignore the NaN padding, and every weight-gradient plan fits the scratch the library promises (the library's
sizing function is plain host code).  Runs without a GPU."""
import pytest
import torch

import linear_cases as lc


def test_names_are_unique_and_every_family_is_named():
    assert len(lc.BY_NAME) == len(lc.CASES)
    for entry in lc.ENTRIES:
        assert {c.family for c in lc.cases(entry)} == set(lc.FAMILIES[entry]), entry


def test_declared_family_is_what_the_dispatcher_picks():
    wrong = [(c.name, lc.family_of(c.entry, c)) for c in lc.CASES if lc.family_of(c.entry, c) != c.family]
    assert not wrong, wrong
    # the row-block height the library names is the family's own, except where only a prologue keeps the call off the LDS-DMA tiles
    odd = [c.name for c in lc.cases("fwd") if c.N > 32 and lc.stats_block_rows(c) != lc.stats_block_rows_of(c.family)]
    assert odd == ["fwd-r01-33x40x1284-p"], odd
    # the family bits of knob 11
    assert lc.family_of("fwd", lc.BY_NAME["fwd-dma64x32-131x5x100"], use_dma=9) == "dma64x32"
    assert lc.family_of("fwd", lc.BY_NAME["fwd-dma64x32-131x5x100"], use_dma=1) == "r01"
    for c in lc.CASES:
        fam = lc.family_of(c.entry, c, use_dma=0)
        assert fam in ("narrow", "r01", "narrow_dx", "r01_dx", "r01_dw", "narrow_both", "split", "r01_dual"), (c.name, fam)


# what a family cannot be given, by its own predicate
NO_PROLOGUE = {("fwd", "smallk"): "a prologue sends K <= 16 to the register-staged tiles",
               ("fwd", "dma128x64"): "with a prologue the M >= 8192 rows take the 128x128 tile whatever N is"}


def test_every_family_sees_every_argument_combination():
    for entry in lc.ENTRIES:
        for fam in lc.FAMILIES[entry]:
            cs = lc.cases(entry, fam)
            if entry != "bwd_input":                  # (it takes neither a bias nor a prologue)
                assert any(not c.bias for c in cs), (entry, fam, "bias / db NULL")
            if entry != "bwd_input" and (entry, fam) not in NO_PROLOGUE:
                assert any(c.prologue for c in cs), (entry, fam, "prologue")
            if entry in ("bwd_input", "bwd_both"):
                assert any(c.accumulate for c in cs) and any(not c.accumulate for c in cs), (entry, fam, "accumulate")
            for op in lc.OPERANDS[entry]:
                assert any(lc.layout_of(c)[op][0] > lc.width_of(c, op) for c in cs), (entry, fam, op, "ld > width")
    assert any(not c.dx for c in lc.cases("bwd_both", "narrow_both")) and any(not c.dx for c in lc.cases("bwd_both", "split"))
    # a misaligned prologue vector is its own case wherever the dispatch looks at it
    for entry, fam in (("fwd", "dma64x32"), ("fwd", "r01"), ("bwd_weight", "small_dw"), ("bwd_weight", "r01_dw"), ("bwd_both", "r01_dual")):
        assert any(c.prologue and lc.layout_of(c)["P"][1] for c in lc.cases(entry, fam)), (entry, fam)


def test_the_boundaries_of_the_issue_are_in_the_table():
    shapes = {e: {(c.M, c.N, c.K) for c in lc.cases(e)} for e in lc.ENTRIES}
    for e in lc.ENTRIES:
        ns, ks = {s[1] for s in shapes[e]}, {s[2] for s in shapes[e]}
        assert {1, 4, 5, 16, 17, 32, 33} <= ns, (e, sorted(ns))
        assert {4, 16, 17, 20, 31, 32, 33, 36} <= ks, (e, sorted(ks))
        assert any(s[1] == 300 or s[2] == 300 for s in shapes[e])
        assert {s[0] for s in shapes[e]} <= {1, 31, 33, 64, 65, 100, 129, 131, 200, 1000, 8193}
        assert all(s[2] <= 128 for s in shapes[e] if s[0] == 8193)
    assert {(8193, 128, 32), (8193, 136, 36), (33, 40, 1280), (33, 40, 1284)} <= shapes["fwd"]
    # the widest dY rows smalln_dx can stage (it raises its LDS limit to 160 KiB there), the next width, and 1024
    assert {(65, 848, 16), (65, 852, 16), (65, 1024, 16)} <= shapes["bwd_input"]
    assert (32 + lc.SMALL_MAX) * (lc.SMALLN_DX_MAX_N + 4) * 4 <= 160 * 1024 < (32 + lc.SMALL_MAX) * (lc.SMALLN_DX_MAX_N + 8) * 4
    for e in ("bwd_input", "bwd_weight", "bwd_both"):
        assert (8193, 128, 128) in shapes[e]
    assert set(lc.SCRATCH_BUG_CLASS) | {lc.SCRATCH_CONTROL} <= shapes["bwd_both"]
    for c in lc.CASES:                           # the six layouts: K % 4 != 0 and N % 4 != 0 are shapes, the rest edits
        assert all(e[:-2] in ("X", "W", "Y", "dX", "dW", "P", "B") for e in filter(None, c.layout.split(","))), c.name
    edits = {e[-2:] for c in lc.CASES for e in c.layout.split(",") if e}
    assert {"+4", "+1", "+2", "+3", "@1"} <= edits
    assert any(c.K in (18, 33) for c in lc.cases("fwd", "r01")) and any(c.N == 37 for c in lc.cases("bwd_input", "r01_dx"))


@pytest.mark.parametrize("rows,width,ld,off", [(5, 7, 7, 0), (5, 7, 8, 1), (3, 10, 13, 0), (1, 4, 4, 3), (4, 6, 10, 2)])
def test_guarded_buffers(rows, width, ld, off):
    a = lc.operand(rows, width, ld, off, seed=1)
    assert (a.dev.data_ptr() % 16 == 0) and a.ptr() % 16 == (4 * off) % 16 and a.ptr() == a.dev.data_ptr() + 4 * a.base
    assert a.base >= 2 * ld + 64 and a.host.numel() - (a.base + rows * ld) >= 2 * ld + 64, "guard rows in front and behind"
    m = a.live_mask()
    assert int(m.sum()) == rows * width
    assert bool(torch.isnan(a.host[~m]).all()) and not bool(torch.isnan(a.host[m]).any()), "NaN exactly outside the live region"
    assert torch.equal(a.dev.view(torch.int32), a.host.view(torch.int32)), "the CPU mirror holds the device-bound values"
    assert a.view(a.host).shape == (rows, width) and a.view(a.host).stride() == (ld, 1)
    assert a.untouched() and a.outside_changed() == 0
    o = lc.output(rows, width, ld, off)
    assert o.ptr() % 16 == (4 * off) % 16
    assert bool(torch.isnan(o.host[m]).all()) and bool((o.host.view(torch.int32)[~m] == lc.SENTINEL_BITS).all())
    assert bool(torch.isfinite(lc.sentinel()))
    o.view().fill_(1.0)                               # a kernel writing its live region leaves the guards alone
    assert o.outside_changed() == 0 and not o.untouched()
    o.dev[o.base + width] = 0.0 if ld > width else o.dev[o.base + width]
    o.dev[o.base - 1] = 2.0                           # ... one float in front of the first row does not
    assert o.outside_changed() == (2 if ld > width else 1)
    acc = lc.output(rows, width, ld, off, seed=3)
    assert bool(torch.isfinite(acc.view(acc.host)).all())
    s = lc.scratch(10, 70)
    assert s.ptr() % 16 == 0 and s.host.numel() == 80 and bool(torch.isnan(s.host[:10]).all())
    s.dev[10] = 0.0
    assert s.outside_changed() == 1


def test_references_are_finite_although_the_padding_is_nan():
    for c in lc.CASES:
        if c.M > 1000:
            continue                              # same code path; the 8193-row references are computed on the GPU box
        ops = lc.Operands(c, "cpu", promised_scratch=8 if c.entry in ("bwd_weight", "bwd_both") else None)
        ref = ops.reference()
        want = {"fwd": {"Y"}, "bwd_input": {"dX"}, "bwd_weight": {"dW"}, "bwd_both": {"dW"} | ({"dX"} if c.dx else set())}[c.entry]
        if c.entry != "fwd" and c.entry != "bwd_input" and c.bias:
            want = want | {"db"}
        assert set(ref) == want, c.name
        for name, r in ref.items():
            assert r.dtype == torch.float64 and bool(torch.isfinite(r).all()), (c.name, name)
            assert r.shape == ops.outputs[name].view().shape, (c.name, name)
        for b in ops.inputs.values():
            assert bool(torch.isnan(b.host[~b.live_mask()]).all())
        assert all(b.ptr() % 16 == 0 for n, b in ops.inputs.items() if n in ("scale", "shift")) == (ops.lay["P"][1] == 0) or not c.prologue


def test_every_plan_fits_the_promised_scratch():
    """the CPU-side witness of the narrow both-kernel's scratch overrun and of its fix: one 32-row slab per workgroup against
    a promise that used to count 128-row slabs when N and K were both <= 16"""
    import esc_gnn_amd
    lib = esc_gnn_amd._native.lib()
    short = []
    for c in lc.CASES:
        if c.entry in ("bwd_weight", "bwd_both"):
            need, promised = lc.scratch_needed(c.entry, c), int(lib.esc_linear_bwd_weight_scratch(c.M, c.N, c.K))
            assert need <= lc.scratch_guard(c), c.name
            if need > promised:
                short.append((c.name, need, promised))
    assert not short, short
    # the whole class, not only the table's members
    for M in (1, 32, 33, 64, 65, 129, 1000, 2400, 8193):
        for N in (1, 2, 3, 4, 5, 16, 17):
            for K in (4, 8, 12, 16, 20, 256, 260):
                promised = int(lib.esc_linear_bwd_weight_scratch(M, N, K))
                if N <= lc.NARROW_N and K <= lc.NARROW_K:
                    assert lc.cdiv(M, lc.NARROW_ROWS) * (N * K + N) <= promised, (M, N, K)
                assert lc.cdiv(M, 128) * (N * K + N) <= promised, (M, N, K)
