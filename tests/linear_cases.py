"""The dense-layer case table: one record per (entry point, shape, operand layout, argument combination) chosen so
that every branch of the dispatchers in csrc/linear_mfma.hip is reached by name, and the helpers that build operands
whose surroundings are poisoned.  No GPU is needed to import or check this module (tests/test_linear_cases_cpu.py);
tests/test_hip_dense_dispatch.py runs the table against the library.

A case is Case(name, entry, M, N, K, layout, prologue, bias, accumulate, family, dx):
  entry       fwd | bwd_input | bwd_weight | bwd_both   (esc_linear_<entry>)
  layout      comma-separated edits of the plain layout (16-byte aligned base, ld == width):
                "X+4"  operand X has ld = width + 4          "X@1"  its base is 1 float past a 16-byte boundary and
                                                                     ld is the width rounded up to a multiple of 4
              operands: X [M,K], W [N,K], Y [M,N] (Y of the forward, dY of the gradients), dX [M,K], dW [N,K],
              P (in_scale / in_shift), B (bias)
  prologue    act(X) = relu(X * in_scale + in_shift)
  bias        forward: bias given; gradients: db wanted
  accumulate  dX += ...
  family      the kernel family the case is MEANT to reach (family_of documents why)
  dx          bwd_both only: False passes dX == NULL

family_of(), stats_block_rows() and scratch_needed() transcribe the dispatch plan of csrc/linear_plan.h.  The transcription
is checked: tests/test_linear_plan_cpu.py compiles that header into a host program and compares its family, row-block
height and slab count with these functions for every record of the table under every family mask.  The GPU test anchors
it to the built library through esc_linear_stats_block_rows, and every result is compared with fp64.
"""
import collections

import torch

Case = collections.namedtuple("Case", "name entry M N K layout prologue bias accumulate family dx")

ENTRIES = ("fwd", "bwd_input", "bwd_weight", "bwd_both")
FAMILIES = {
    "fwd": ("narrow", "smallk", "dma64x32", "dma64", "dma128", "dma128x64", "r01"),
    "bwd_input": ("narrow_dx", "smalln_dx", "dma64_dx", "dma128_dx", "r01_dx"),
    "bwd_weight": ("small_dw", "dma64_dw", "dma128_dw", "r01_dw"),
    "bwd_both": ("narrow_both", "dma64_dual", "dma128_dual", "split", "r01_dual"),
}
OPERANDS = {"fwd": ("X", "W", "Y"), "bwd_input": ("Y", "W", "dX"), "bwd_weight": ("Y", "X", "dW"),
            "bwd_both": ("Y", "X", "W", "dX", "dW")}
# the constants of the dispatchers (csrc/linear_plan.h)
SMALL_MAX, NARROW_N, NARROW_K, NARROW_ROWS, ROWS_WGRAD, PRO_MAX_K = 16, 4, 256, 32, 32, 1280
SMALLN_DX_MAX_N = 848                                  # smalln_dx keeps [32 + 16][N + 4] floats in the 160 KiB LDS
KNOB_DEFAULTS = (1, 4, 1, 4, 4, 512, 128, 2)           # knobs 0..7
USE_DMA_DEFAULT = 15                                   # knob 11
SENTINEL_BITS = 0x4B5A3C2D                             # a finite float (1.43e7) no kernel here computes


def cdiv(a, b):
    return -(-a // b)


def tile128_ok(dim):
    return cdiv(dim, 128) * 128 * 10 <= dim * 11


def width_of(case, op):
    return case.N if op == "Y" else case.K


def rows_of(case, op):
    return case.N if op in ("W", "dW") else case.M


def layout_of(case):
    """{operand: (ld, offset_floats)} for X, W, Y, dX, dW and {P, B: (n, offset)} of a case"""
    out = {op: (width_of(case, op), 0) for op in ("X", "W", "Y", "dX", "dW")}
    out["P"], out["B"] = (case.K, 0), (case.N, 0)
    for edit in filter(None, case.layout.split(",")):
        if "+" in edit:
            op, pad = edit.split("+")
            out[op] = (out[op][0] + int(pad), out[op][1])
        else:
            op, off = edit.split("@")
            out[op] = (cdiv(out[op][0], 4) * 4, int(off))
    return out


def _vec_ok(lay, op):
    ld, off = lay[op]
    return off % 4 == 0 and ld % 4 == 0


def family_of(entry, case, use_dma=USE_DMA_DEFAULT):
    """the family the dispatcher of esc_linear_<entry> picks (default tile knobs, ESC_TILE160 unset); the forward is
    given col_stats exactly when N > 32"""
    M, N, K, lay = case.M, case.N, case.K, layout_of(case)
    pro_aligned = (not case.prologue) or lay["P"][1] % 4 == 0
    narrow_ok = N <= NARROW_N and K <= NARROW_K and K % 4 == 0 and _vec_ok(lay, "X") and _vec_ok(lay, "W") and pro_aligned
    if entry == "fwd":
        stats = N > 32
        if not stats and narrow_ok:
            return "narrow"
        if (use_dma & 4) and K <= SMALL_MAX and not case.prologue and N > 32:
            return "smallk"
        if ((use_dma & 1) and K % 4 == 0 and K >= 32 and _vec_ok(lay, "X") and _vec_ok(lay, "W")
                and not (case.prologue and cdiv(K, 32) * 32 > PRO_MAX_K) and not (N <= 32 and (not (use_dma & 8) or stats))):
            if N <= 32:
                return "dma64x32"
            if N >= 128 and M >= 8192:
                return "dma128" if (case.prologue or tile128_ok(N)) else "dma128x64"
            return "dma64"
        return "r01"
    dma_shape = (use_dma & 2) and N > 32 and K > 32 and N % 4 == 0 and K % 4 == 0 and _vec_ok(lay, "Y")
    big = M >= 8192 and tile128_ok(N) and tile128_ok(K)
    if entry == "bwd_input":
        if N <= 16 and K <= NARROW_K and K % 4 == 0 and _vec_ok(lay, "W") and _vec_ok(lay, "dX"):
            return "narrow_dx"
        if (use_dma & 4) and K <= SMALL_MAX and N % 4 == 0 and N <= SMALLN_DX_MAX_N and _vec_ok(lay, "Y"):
            return "smalln_dx"
        if dma_shape and _vec_ok(lay, "W") and _vec_ok(lay, "dX"):
            return "dma128_dx" if (M >= 8192 and tile128_ok(K)) else "dma64_dx"
        return "r01_dx"
    if entry == "bwd_weight":
        if (use_dma & 4) and (K <= SMALL_MAX) != (N <= SMALL_MAX):
            return "small_dw"
        if dma_shape and _vec_ok(lay, "X"):
            return "dma128_dw" if big else "dma64_dw"
        return "r01_dw"
    assert entry == "bwd_both"
    if (not case.dx or _vec_ok(lay, "dX")) and narrow_ok:
        return "narrow_both"
    if case.dx and dma_shape and _vec_ok(lay, "X") and _vec_ok(lay, "W") and _vec_ok(lay, "dX"):
        return "dma128_dual" if big else "dma64_dual"
    if not case.dx or N <= 32 or K <= 32:
        return "split"                      # esc_linear_bwd_weight's dispatch, then esc_linear_bwd_input's
    return "r01_dual"


def stats_block_rows_of(family):
    """rows per col_stats partial of a forward family (N > 32)"""
    return {"smallk": 32, "r01": 32, "dma64": 64, "dma128": 128, "dma128x64": 128}[family]


def stats_block_rows(case, use_dma=USE_DMA_DEFAULT):
    """what esc_linear_stats_block_rows answers for a forward case.  The function is not told whether the call has a prologue,
    so it names the family of the same call WITHOUT one; the two differ in height for one class only — a prologue past the
    LDS-DMA tiles' K limit (K > 1280) on operands they would serve: the register-staged tiles compute Y, the partials are
    delivered at the promised 64 / 128 rows (fwd-r01-33x40x1284-p)."""
    return stats_block_rows_of(family_of("fwd", case._replace(prologue=False), use_dma))


# ---- the scratch plans, transcribed (csrc/linear_plan.h: dma_wgrad_splits, r01_wgrad_splits, plan_both, plan_dw) -------------
def _dma_wgrad_splits(M, N, K, bm, bn):
    sp = max(1, min(cdiv(256, cdiv(N, bm) * cdiv(K, bn)), cdiv(M, 128)))
    per = max(128, cdiv(cdiv(M, sp), 32) * 32)
    return cdiv(M, per)


def _r01_wgrad_splits(M, N, K, bm, bn, bk, knobs=KNOB_DEFAULTS):
    want = cdiv(knobs[5], cdiv(N, bm) * cdiv(K, bn))
    sp = max(1, min(want, cdiv(M, max(128, knobs[6]))))
    per = cdiv(cdiv(M, sp), bk) * bk
    return max(1, cdiv(M, per))


R01_TILE_DIMS = {0: (128, 128, 32), 2: (128, 32, 32), 3: (128, 64, 32), 4: (64, 64, 64), 5: (32, 64, 32), 6: (32, 32, 32),
                 7: (64, 32, 32)}             # every other id: 64 x 64 x BK32


def scratch_needed(entry, case):
    """floats of `slabs` the family of a weight-gradient case writes: splits * (N*K + N)"""
    M, N, K = case.M, case.N, case.K
    fam = family_of(entry, case)
    if fam == "split":
        fam = family_of("bwd_weight", case)
    big = 128 if fam.startswith("dma128") else 64
    if fam == "narrow_both":
        splits = cdiv(M, NARROW_ROWS)
    elif fam == "small_dw":
        splits = cdiv(M, ROWS_WGRAD)
    elif fam in ("dma64_dw", "dma128_dw", "dma64_dual", "dma128_dual"):
        splits = _dma_wgrad_splits(M, N, K, big, big)
    elif fam == "r01_dw":
        splits = _r01_wgrad_splits(M, N, K, *R01_TILE_DIMS.get(KNOB_DEFAULTS[4], (64, 64, 32)))
    else:
        assert fam == "r01_dual", fam
        splits = _r01_wgrad_splits(M, N, K, 64, 64, 32)           # knob 7 = 2
    return splits * (N * K + N)


def scratch_guard(case):
    """floats of sentinel behind the promised scratch: the densest plan any kernel uses is one slab per 32 rows"""
    return cdiv(case.M, 32) * (case.N * case.K + case.N) + 64


# ---- guarded buffers ------------------------------------------------------------------------------------------------------
def sentinel():
    return torch.tensor([SENTINEL_BITS], dtype=torch.int32).view(torch.float32)[0]


class Buf(object):
    """A [rows, width] operand with leading dimension ld inside a larger allocation.

    host   flat float32 CPU tensor: the values the device buffer starts from (never modified)
    dev    the same floats on `device`, starting at a 16-byte aligned address
    base   index of element [0, 0] in both; its address is 16-byte aligned + 4 * offset_floats
    Everything outside [0:rows, 0:width] — padding columns, guard floats in front and behind — holds `outside`."""

    def __init__(self, rows, width, ld, offset_floats, live, outside, guard_before, guard_after, device):
        assert ld >= width and rows >= 1 and 0 <= offset_floats < 4
        front = cdiv(guard_before, 4) * 4
        self.rows, self.width, self.ld, self.base = rows, width, ld, front + offset_floats
        n = self.base + rows * ld + guard_after
        self.host = torch.full((n,), float(outside), dtype=torch.float32)
        self.view(self.host).copy_(live)
        raw = torch.empty(n + 4, dtype=torch.float32, device=device)
        skew = (-(raw.data_ptr() // 4)) % 4
        self.dev = raw[skew:skew + n]
        self.dev.copy_(self.host)

    def view(self, flat=None):
        flat = self.dev if flat is None else flat
        return flat[self.base:self.base + self.rows * self.ld].view(self.rows, self.ld)[:, :self.width]

    def ptr(self):
        return self.dev.data_ptr() + 4 * self.base

    def live_mask(self):
        m = torch.zeros(self.host.numel(), dtype=torch.bool)
        self.view(m).fill_(True)
        return m

    def outside_changed(self):
        """number of floats outside the live region whose bits differ from what they were given"""
        now = self.dev.cpu().view(torch.int32)
        return int(((now != self.host.view(torch.int32)) & ~self.live_mask()).sum())

    def untouched(self):
        return torch.equal(self.dev.cpu().view(torch.int32), self.host.view(torch.int32))

    def result(self):
        return self.view(self.dev.cpu())


class ByteBuf(object):
    """A dense [rows, width] uint8 operand (a dropout keep mask) with `guard` bytes of `outside` in front and behind; its first
    byte is 16-byte aligned + offset_bytes"""

    def __init__(self, live, guard, device, outside=0xA5, offset_bytes=0):
        front = cdiv(guard, 16) * 16
        self.base, self.n = front + offset_bytes, live.numel()
        self.host = torch.full((self.base + self.n + guard,), outside, dtype=torch.uint8)
        self.host[self.base:self.base + self.n] = live.reshape(-1)
        raw = torch.empty(self.host.numel() + 16, dtype=torch.uint8, device=device)
        skew = (-raw.data_ptr()) % 16
        self.dev = raw[skew:skew + self.host.numel()]
        self.dev.copy_(self.host)

    def ptr(self):
        return self.dev.data_ptr() + self.base

    def untouched(self):
        return torch.equal(self.dev.cpu(), self.host)


def _uniform(rows, width, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(rows, width, generator=g) * 2 - 1


def operand(rows, width, ld, offset_floats, guard_rows=2, seed=0, device="cpu", scale=1.0, shift=0.0):
    """an input: uniform(shift - scale, shift + scale) values, NaN in every float outside [0:rows, 0:width]"""
    g = guard_rows * ld + 64
    return Buf(rows, width, ld, offset_floats, _uniform(rows, width, seed) * scale + shift, float("nan"), g, g, device)


def output(rows, width, ld, offset_floats, guard_rows=2, seed=None, device="cpu"):
    """an output: NaN in the live region (uniform values when `seed` is given: the accumulate form), the sentinel outside"""
    g = guard_rows * ld + 64
    live = torch.full((rows, width), float("nan")) if seed is None else _uniform(rows, width, seed)
    return Buf(rows, width, ld, offset_floats, live, sentinel(), g, g, device)


def scratch(promised, guard, device="cpu"):
    """`promised` floats of NaN (a slab that is read before it is written shows), then `guard` floats of sentinel"""
    return Buf(1, promised, promised, 0, torch.full((1, promised), float("nan")), sentinel(), 0, guard, device)


class Operands(object):
    """every buffer of a case, on `device`, with the fp64 references taken from the live regions of the CPU mirrors"""

    def __init__(self, case, device="cpu", promised_scratch=None):
        lay = layout_of(case)
        M, N, K, e = case.M, case.N, case.K, case.entry
        seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % 100003
        self.case, self.lay = case, lay
        mk = lambda op, s, scale=1.0: operand(rows_of(case, op), width_of(case, op), lay[op][0], lay[op][1], seed=seed + s,
                                              device=device, scale=scale)
        out = lambda op, acc: output(rows_of(case, op), width_of(case, op), lay[op][0], lay[op][1],
                                     seed=(seed + 7) if acc else None, device=device)
        self.inputs, self.outputs = {}, {}
        if e in ("fwd", "bwd_weight", "bwd_both"):
            self.inputs["X"] = mk("X", 1)
        if e in ("fwd", "bwd_input", "bwd_both"):
            self.inputs["W"] = mk("W", 2, K ** -0.5)
        if e == "fwd":
            self.outputs["Y"] = out("Y", False)
            if case.bias:
                self.inputs["B"] = operand(1, N, N, lay["B"][1], seed=seed + 3, device=device)
        else:
            self.inputs["Y"] = mk("Y", 4)
        if e == "bwd_input" or (e == "bwd_both" and case.dx):
            self.outputs["dX"] = out("dX", case.accumulate)
        if e in ("bwd_weight", "bwd_both"):
            self.outputs["dW"] = out("dW", False)
            if case.bias:
                self.outputs["db"] = output(1, N, N, 0, device=device)
            if promised_scratch is not None:
                self.outputs["slabs"] = scratch(promised_scratch, scratch_guard(case), device)
        if case.prologue:
            self.inputs["scale"] = operand(1, K, K, lay["P"][1], seed=seed + 5, device=device, scale=0.5, shift=1.0)     # 0.5 .. 1.5
            self.inputs["shift"] = operand(1, K, K, lay["P"][1], seed=seed + 6, device=device, scale=0.5)

    def host(self, name):
        b = self.inputs.get(name) or self.outputs[name]
        return b.view(b.host).double()

    def act_x(self):
        x = self.host("X")
        return (x * self.host("scale") + self.host("shift")).relu() if self.case.prologue else x

    def reference(self):
        """{output name: fp64 tensor} from the live regions only"""
        c, ref = self.case, {}
        if c.entry == "fwd":
            ref["Y"] = self.act_x() @ self.host("W").t() + (self.host("B") if c.bias else 0.0)
            return ref
        dy = self.host("Y")
        if "dX" in self.outputs:
            ref["dX"] = dy @ self.host("W") + (self.host("dX") if c.accumulate else 0.0)
        if "dW" in self.outputs:
            ref["dW"] = dy.t() @ self.act_x()
        if "db" in self.outputs:
            ref["db"] = dy.sum(0, keepdim=True)
        return ref


# ---- the table --------------------------------------------------------------------------------------------------------------------
CASES = []


def _add(entry, family, rows):
    """rows: (M, N, K[, layout[, flags]]) with flags a string of p (prologue), n (no bias / no db), a (accumulate), x (dX == NULL)"""
    for row in rows:
        M, N, K = row[:3]
        layout = row[3] if len(row) > 3 else ""
        flags = row[4] if len(row) > 4 else ""
        name = "%s-%s-%dx%dx%d%s%s" % (entry, family, M, N, K, ("-" + layout) if layout else "", ("-" + flags) if flags else "")
        CASES.append(Case(name, entry, M, N, K, layout, "p" in flags, "n" not in flags, int("a" in flags), family, "x" not in flags))


def _turn(shape, edits, flags=""):
    return [shape + (e, flags) for e in edits]


# forward: Y[M,N] = act(X)[M,K] W[N,K]^T + b
_add("fwd", "narrow", [(33, 1, 256), (131, 4, 256, "", "p"), (31, 4, 4), (65, 1, 16, "", "n"), (1, 3, 100, "", "pn")]
     + _turn((131, 3, 100), ("X+4", "W+4", "Y+4", "Y+1", "Y+2", "Y+3", "Y@1", "B@1")))
_add("fwd", "smallk", [(33, 33, 4), (131, 70, 16), (65, 300, 10), (129, 37, 1, "", "n"), (1, 33, 16)]
     + _turn((131, 70, 10), ("X+4", "X+1", "X@1", "W+4", "W+1", "W@1", "Y+4", "Y+1", "Y@1", "B@1")))
_add("fwd", "dma64x32", [(64, 32, 32), (131, 5, 100), (33, 16, 36), (65, 17, 32), (131, 32, 100, "", "p"), (129, 1, 260),
                         (33, 4, 100, "P@1", "p"), (31, 30, 100, "", "n")]
     + _turn((131, 30, 100), ("X+4", "W+4", "Y+4", "Y+1", "Y+2", "Y+3", "Y@1", "B@1")))
_add("fwd", "dma64", [(64, 64, 32), (131, 70, 100), (131, 70, 100, "", "p"), (131, 70, 100, "", "n"), (1, 33, 32), (131, 70, 36),
                      (33, 40, 1280, "", "p"), (131, 37, 100), (65, 300, 64), (8193, 64, 32), (131, 70, 100, "P@1", "p")]
     + _turn((131, 72, 100), ("X+4", "W+4", "Y+4", "Y+1", "Y+2", "Y+3", "Y@1", "B@1")))
_add("fwd", "dma128", [(8193, 128, 32), (8193, 136, 36, "", "p"), (8193, 128, 100, "X+4,W+4,Y+4", "n"), (8193, 128, 32, "Y+1"),
                       (8193, 128, 32, "Y@1", "p")])
_add("fwd", "dma128x64", [(8193, 136, 36), (8193, 136, 36, "X+4,W+4,Y+4", "n"), (8193, 134, 36, "Y+1")])
_add("fwd", "r01", [(131, 70, 18), (131, 70, 33), (33, 33, 17), (65, 40, 20), (33, 33, 31), (33, 5, 20), (131, 17, 16), (33, 16, 17),
                    (33, 40, 1284, "", "p"), (131, 70, 18, "P@1", "p"), (131, 70, 100, "X+1", "p"), (8193, 40, 18), (131, 3, 18),
                    (131, 3, 100, "X+1"), (64, 64, 32, "X+1"), (131, 70, 33, "", "n"), (131, 70, 16, "", "p"), (131, 5, 20, "", "p")]
     + _turn((131, 70, 100), ("X+1", "X+2", "X+3", "X@1", "W+1", "W@1", "X+1,Y+4", "X+1,Y+1", "W+1,Y@1", "X@1,W+4", "X+1,B@1")))

# input gradient: dX[M,K] = dY[M,N] W[N,K] (+ dX)
_add("bwd_input", "narrow_dx", [(33, 1, 256), (33, 1, 256, "", "a"), (131, 4, 100), (131, 5, 100, "", "a"), (65, 16, 16), (31, 16, 4),
                                (1, 10, 100)]
     + _turn((131, 10, 100), ("Y+4", "Y+1", "Y@1", "W+4", "dX+4")) + _turn((131, 3, 100), ("Y+1", "dX+4"), "a"))
_add("bwd_input", "smalln_dx", [(33, 20, 4), (131, 72, 10), (131, 72, 10, "", "a"), (65, 848, 16), (131, 300, 16, "", "a"), (33, 16, 10),
                                (1, 36, 16)]
     + _turn((131, 72, 10), ("Y+4", "W+4", "W+1", "W@1", "dX+4", "dX+1", "dX@1")) + _turn((33, 8, 16), ("W+1", "dX@1"), "a"))
_add("bwd_input", "dma64_dx", [(64, 64, 64), (131, 72, 100), (131, 72, 100, "", "a"), (33, 36, 36), (1, 36, 36, "", "a"), (129, 300, 64)]
     + _turn((131, 72, 100), ("Y+4", "W+4", "dX+4")) + [(131, 72, 100, "Y+4,W+4,dX+4", "a")])
_add("bwd_input", "dma128_dx", [(8193, 128, 128), (8193, 128, 128, "Y+4,W+4,dX+4", "a")])
_add("bwd_input", "r01_dx", [(131, 70, 100), (131, 70, 100, "", "a"), (131, 37, 100), (131, 72, 33), (131, 72, 18, "", "a"), (65, 40, 20),
                             (64, 64, 32), (33, 17, 17), (33, 33, 32, "", "a"), (33, 37, 16), (8193, 38, 36), (1, 17, 33), (65, 32, 36), (33, 33, 31), (65, 1024, 16), (65, 852, 16, "", "a")]
     + _turn((131, 72, 100), ("Y+1", "Y+2", "Y+3", "Y@1", "W+1", "W@1", "dX+1", "dX@1", "Y+1,W+4,dX+4"))
     + _turn((131, 72, 100), ("Y@1", "dX+1"), "a"))

# weight gradient: dW[N,K] = dY^T act(X), db = colsum(dY)
_add("bwd_weight", "small_dw", [(33, 33, 4), (131, 70, 16), (131, 300, 10), (131, 4, 100), (65, 16, 300), (33, 1, 17), (131, 5, 33),
                                (131, 70, 16, "", "p"), (131, 4, 100, "", "p"), (131, 70, 16, "P@1", "p"), (131, 70, 16, "", "n"), (1, 40, 8)]
     + _turn((131, 70, 10), ("Y+4", "Y+1", "Y@1", "X+4", "X+1", "X@1", "dW+4", "dW+1", "dW@1")))
_add("bwd_weight", "dma64_dw", [(64, 64, 64), (131, 72, 100), (131, 72, 100, "", "p"), (131, 72, 100, "", "n"), (129, 36, 36),
                                (131, 72, 100, "P@1", "p"), (1, 36, 36), (65, 300, 36)]
     + _turn((131, 72, 100), ("Y+4", "X+4", "dW+4", "dW+1", "dW@1")))
_add("bwd_weight", "dma128_dw", [(8193, 128, 128), (8193, 128, 128, "Y+4,X+4,dW+4", "pn")])
_add("bwd_weight", "r01_dw", [(33, 16, 16), (131, 4, 8), (65, 1, 16), (131, 70, 100), (131, 72, 33), (33, 17, 17), (33, 33, 32),
                              (64, 64, 32), (131, 32, 100), (131, 70, 100, "", "p"), (131, 72, 18, "P@1", "p"), (131, 70, 100, "", "n"),
                              (8193, 40, 18), (131, 37, 36), (1, 17, 33), (33, 33, 31), (65, 40, 20)]
     + _turn((131, 72, 100), ("Y+1", "Y+2", "Y+3", "Y@1", "X+1", "X@1", "Y+1,dW+4", "X+1,dW+1", "X+1,dW@1", "Y@1,X+4"))
     + [(131, 72, 100, "X+1", "p")])

# both gradients in one call
_add("bwd_both", "narrow_both", [(33, 1, 256), (131, 4, 100), (100, 4, 256), (65, 1, 16), (1000, 1, 16), (200, 4, 8), (129, 1, 4),
                                 (131, 4, 100, "", "p"), (131, 1, 100, "", "pa"), (131, 4, 100, "", "x"), (131, 3, 100, "", "n"),
                                 (200, 4, 8, "", "pa")]
     + _turn((131, 3, 100), ("Y+4", "Y+1", "Y@1", "X+4", "W+4", "dX+4", "dW+4", "dW+1", "dW@1")))
_add("bwd_both", "dma64_dual", [(64, 64, 64), (131, 72, 100), (131, 72, 100, "", "p"), (131, 72, 100, "", "a"), (131, 72, 100, "", "n"),
                                (129, 36, 36, "", "pa"), (131, 72, 100, "P@1", "p")]
     + _turn((131, 72, 100), ("Y+4", "X+4", "W+4", "dX+4", "dW+4", "dW+1", "dW@1")))
_add("bwd_both", "dma128_dual", [(8193, 128, 128), (8193, 128, 128, "Y+4,X+4,W+4,dX+4,dW+4", "pan")])
_add("bwd_both", "split", [(131, 72, 100, "", "x"), (131, 70, 100, "", "px"), (131, 5, 100), (131, 72, 10, "", "a"), (33, 16, 16),
                           (64, 64, 32), (131, 17, 33, "", "p"), (131, 3, 100, "X+1"), (131, 3, 18, "", "a"), (131, 72, 10, "", "n"),
                           (131, 4, 100, "dX+1"), (131, 72, 16, "", "p"), (33, 33, 31), (65, 32, 36, "", "a"), (65, 40, 20), (33, 17, 17, "", "n"), (131, 300, 10), (65, 16, 300)]
     + _turn((131, 72, 10), ("Y+4", "X+4", "W+4", "dX+4", "dW+4", "X+1", "dX+1")))
_add("bwd_both", "r01_dual", [(131, 70, 100), (131, 70, 100, "", "p"), (131, 70, 100, "", "a"), (131, 70, 100, "", "n"), (131, 72, 33),
                              (131, 37, 36), (8193, 38, 36), (131, 72, 100, "X+1,P@1", "p"), (33, 33, 33, "", "pa")]
     + _turn((131, 72, 100), ("Y+1", "Y+2", "Y+3", "Y@1", "X+1", "X@1", "W+1", "W@1", "dX+1", "dX@1", "Y+1,X+4,W+4,dX+4,dW+4", "X+1,dW+1")))

BY_NAME = {c.name: c for c in CASES}
SCRATCH_BUG_CLASS = ((65, 1, 16), (1000, 1, 16), (200, 4, 8), (129, 1, 4))          # narrow both-kernel, N <= 4 and K <= 16
SCRATCH_CONTROL = (100, 4, 256)


def cases(entry, family=None):
    return [c for c in CASES if c.entry == entry and (family is None or c.family == family)]
