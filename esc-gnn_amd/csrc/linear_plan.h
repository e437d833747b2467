// linear_plan.h — which kernel family serves a Linear call, with which tile, how many slabs: decided ONCE, on the host.
//
// Host-only C++ (no HIP header: g++ compiles it alone, tests/linear_plan_host.cpp does).  Every function here is a pure
// function of operand addresses (alignment only), leading dimensions, M, N, K, the call's flags and a PlanKnobs value.
// linear_mfma.hip owns the one PlanKnobs instance, takes a plan per call and switches on its family; the query entries
// (esc_linear_stats_block_rows, esc_linear_*_ok, esc_linear_bwd_weight_scratch, ...) answer from the same functions.
// To add a family: an enum member (+ its name), a clause in the plan_* function, one `case` in the entry's switch.
#pragma once
#include <cstddef>
#include <cstdint>

namespace esc {

// ---- the constants of the dispatch ---------------------------------------------------------------------------------
namespace small {                     // the tiny-dimension kernels (linear_small.h)
constexpr int SMALL_MAX = 16;
constexpr int ROWS_FWD = 32;          // rows per workgroup = rows per BatchNorm partial (the GEMM epilogue's contract)
constexpr int SMALLN_DX_MAX_N = ((160 * 1024 / 4) / (32 + SMALL_MAX) - 4) & ~3;      // 848: smalln_dx keeps [32 + SMALL_MAX][N + 4] floats in the 160 KiB LDS
constexpr int ROWS_WGRAD = 32;        // reduction rows per slab (a slab is N*K <= 16*1280 floats: hundreds of them are cheap to sum)
}  // namespace small

constexpr int NARROW_N = 4, NARROW_K = 256;                      // measured: at N = 10 the wave reductions cost more than the padded MFMA tile
constexpr int NARROW_ROWS = 32;                                  // rows per workgroup of linear_narrow_bwd: 2 400 rows = 75 workgroups (128 left 19 on 256 CUs)
constexpr int NARROW_DX_N = 16;                                  // linear_narrow_dx: reduction N <= 16
constexpr int64_t PRO_MAX_K = 1280;                              // the LDS-DMA tiles keep the prologue's scale / shift of a whole (padded) K in LDS
constexpr int64_t BNB_MAX_N = 640;                               // ... and the fused BatchNorm backward's coefficients of N channels
constexpr int64_t FUSE_FINALIZE_MAX_ROWS = 4096;                 // esc_linear_bn_fwd: last-block finalize up to here (when knob 8 enables it)
constexpr int LDS_BYTES = 160 * 1024;                            // LDS of a CU
constexpr int64_t EDGE_ROWS = 8192;                              // "edge-sized": from here the 128-row tiles fill the chip

namespace plan {

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// tuning state (esc_tune_set knobs 0..7, 11 and 14, three environment switches): defaults chosen from gemm_bench sweeps on MI355X
enum { KNOB_FWD_BIG = 0, KNOB_FWD_SMALL = 1, KNOB_DX_BIG = 2, KNOB_DX_SMALL = 3, KNOB_DW_TILE = 4,
       KNOB_DW_BLOCKS = 5, KNOB_DW_MIN_ROWS = 6, KNOB_DUAL_SMALL = 7, KNOB_COUNT = 8 };
struct PlanKnobs {
  int knob[KNOB_COUNT] = {1, 4, 1, 4, 4, 512, 128, 2};
  // knob 11: bit 0: LDS-DMA forward, bit 1: its gradients, bit 2: the tiny-dimension kernels (linear_small.h), bit 3: 64x32
  // narrow-output tile; 0 keeps every GEMM on the r01 register-staged tiles (A/B runs in one process)
  int use_dma = 15;
  int tile160 = 0;                        // ESC_TILE160
  int64_t tile160_min_wgs = 150;          // ESC_TILE160_MIN_WGS
  int64_t big_min_wgs = 1LL << 62;        // ESC_BIG_MIN_WGS
  // knob 14, and the step engine around the readout's edge-stream block (request_dual_split, common.h): the fused LDS-DMA tiles
  // of esc_linear_bwd_both_bn go out as TWO launches of the same kernel on the same stream, the dX tiles first — whoever waits
  // for dX only need not wait for the dW slabs.  Same tiles, same slabs, same bits.  A value > 1 is also the least dynamic LDS
  // (bytes) the dX launch asks for: its workgroups per CU.  Off by default: no default plan changes.
  int dual_split = 0;
};

// ---- the r01 tile table: ids are stable (esc_tune_set) --------------------------------------------------------------
//   0: 128x128 BK32   1: 64x64 BK32   2: 128x32 BK32 (narrow outputs)   3: 128x64 BK32   4: 64x64 BK64
//   5: 32x64 BK32, 2 waves   6: 32x32 BK32, 1 wave   7: 64x32 BK32, 2 waves   (smaller workgroups: measured slower)
//   8: 32x32 tile, 4 wave groups splitting BK64   9: same with BK128   10: 64x32, 2 groups, BK64   (in-workgroup split-K)
struct Tile { int bm, bn, wm, wn, bk, kw; };
constexpr int R01_TILES = 11;
constexpr Tile R01_TILE[R01_TILES] = {
    {128, 128, 2, 2, 32, 1}, {64, 64, 2, 2, 32, 1}, {128, 32, 4, 1, 32, 1}, {128, 64, 2, 2, 32, 1}, {64, 64, 2, 2, 64, 1},
    {32, 64, 1, 2, 32, 1},   {32, 32, 1, 1, 32, 1}, {64, 32, 2, 1, 32, 1},  {32, 32, 1, 1, 64, 4},  {32, 32, 1, 1, 128, 4},
    {64, 32, 2, 1, 64, 2}};
// the table row a knob value selects: unknown ids are tile 1; the split-K tiles (8..10) have no slab-writing (`db`) form
inline int r01_tile_id(int id, bool db) { return (id < 0 || id >= R01_TILES || (db && id >= 8)) ? 1 : id; }

// ---- families ------------------------------------------------------------------------------------------------------
enum Family {
  F_NONE = 0,            // not served (the *_ok predicates; entries that have no other family refuse)
  F_NARROW, F_SMALLK, F_DMA64X32, F_DMA64, F_DMA128, F_DMA128X64, F_DMA160, F_R01,
  F_R01_ROWSTATS,        // r01 tiles compute Y, col_stats_rows_kernel delivers the partials at the promised height
  F_R01_BN,              // r01 tiles with the BatchNorm finalize in the last workgroup (esc_linear_bn_fwd, knob 8)
  F_NARROW_DX, F_SMALLN_DX, F_DMA64_DX, F_DMA128_DX, F_DMA160_DX, F_R01_DX,
  F_SMALL_DW, F_DMA64_DW, F_DMA128_DW, F_R01_DW,
  F_NARROW_BOTH, F_DMA64_DUAL, F_DMA128_DUAL, F_DMA160_DUAL,
  F_SPLIT,               // esc_linear_bwd_weight's plan, then esc_linear_bwd_input's
  F_R01_DUAL,
  F_SMALL_BN, F_DMA64_BN, F_DMA128_BN,          // esc_linear_bwd_both_bn
  F_COUNT
};
inline const char* family_name(Family f) {
  static const char* const names[F_COUNT] = {
      "none", "narrow", "smallk", "dma64x32", "dma64", "dma128", "dma128x64", "dma160", "r01", "r01_rowstats", "r01_bn",
      "narrow_dx", "smalln_dx", "dma64_dx", "dma128_dx", "dma160_dx", "r01_dx", "small_dw", "dma64_dw", "dma128_dw", "r01_dw",
      "narrow_both", "dma64_dual", "dma128_dual", "dma160_dual", "split", "r01_dual", "small_bn", "dma64_bn", "dma128_bn"};
  return (f >= 0 && f < F_COUNT) ? names[f] : "?";
}

// how esc_linear_bn_fwd finishes the statistics after the GEMM
enum BnAfter { BN_NONE = 0, BN_FROM_ROWS /* esc_bn_stats_from_partials_rows at block_rows */, BN_FROM_PARTIALS /* esc_bn_stats_from_partials */,
               BN_IN_KERNEL };

struct Plan {
  Family family = F_NONE;
  bool ok = false;                 // family != F_NONE
  int tile = 1;                    // r01 families: row of R01_TILE
  int bm = 0, bn = 0;              // the tile's output shape (LDS-DMA shape or R01_TILE[tile]); narrow kernels: bn = NMAX
  int block_rows = 32;             // forward: rows per col_stats partial block; both_bn: rows per `next` partial block
  BnAfter bn_after = BN_NONE;
  int splits = 0, per_split = 0;   // weight gradient: slabs, reduction rows per slab
  int64_t slab_floats = 0;         // floats of `slabs` written: splits * (N*K + N)
  int launches = 1;                // both_bn on the LDS-DMA tiles: 2 = the dX tiles and the dW tiles as two launches (PlanKnobs::dual_split)
  int dx_lds = 0;                  // ... and the least dynamic LDS of the dX launch, bytes (0: what the tile needs)
};

struct Op { const void* p; int64_t ld; };                  // an operand: base address (for its alignment) and leading dimension
struct Flags {
  bool pro = false;                // in_scale given (or the folded BatchNorm of the fold form)
  bool pro_aligned = true;         // in_scale / in_shift 16-byte aligned (true without a prologue)
  bool pro_paired = true;          // in_scale and in_shift come together
  bool col_stats = false;
  bool c_init = false;             // esc_linear_fwd_from
  bool fold = false;               // esc_linear_fwd_fold
  bool bn = false;                 // esc_linear_bn_fwd's bn
  bool last_block_finalize = false;      // knob 8 (runtime.hip)
};

// ---- shape tests, each written once ---------------------------------------------------------------------------------
inline bool vec_ok(Op a) { return aligned16(a.p) && a.ld % 4 == 0; }
inline bool dma_ok(Op a, int64_t rows) { return aligned16(a.p) && a.ld % 4 == 0 && rows * a.ld * 4 < (1LL << 31); }
// a 128-wide tile dimension over `dim` columns: acceptable when the padding to a multiple of 128 wastes <= 10 % of the MFMA
// work (256, 600 -> yes; 300 -> 384 is 28 % waste -> 64-wide tiles: 320)
inline bool tile128_ok(int64_t dim) { return cdiv(dim, 128) * 128 * 10 <= dim * 11; }
inline bool tile160_ok(int64_t dim) { return cdiv(dim, 160) * 160 * 10 <= dim * 11; }
inline bool edge_sized(int64_t M) { return M >= EDGE_ROWS; }
// forward GEMM on 128-row tiles (4 compute + 4 loader waves, one workgroup per CU): edge-sized inputs.  Mid-sized launches that
// would still fill the chip with them (ogbg-mol node rows: 6 500 x 600 = 51 x 5 tiles) are faster ALONE on the big tile (32.8 ->
// 27.7 us) but slower inside the two-stream step (4.87 vs 4.77 ms: a one-workgroup-per-CU tile on the node stream shuts the
// edge stream's GEMMs out) — ESC_BIG_MIN_WGS=<workgroups> enables the rule for experiments.
inline bool fwd_big(const PlanKnobs& k, int64_t M, int64_t N) {
  if (N < 128) return false;
  if (edge_sized(M)) return true;
  return cdiv(M, 128) * cdiv(N, tile128_ok(N) ? 128 : 64) >= k.big_min_wgs;
}
// the gradients' big tile: edge-sized rows and both weight dimensions 128-tileable
inline bool bwd_big(int64_t M, int64_t N, int64_t K) { return edge_sized(M) && tile128_ok(N) && tile128_ok(K); }
// 300 / 600-wide layers (ogbg-mol emb_dim 300, its 2H hidden layer): a 128-row x 160-column tile (r03) pads them by 6.7 % at 2.2x the
// arithmetic intensity of the 64x64 tile they take (128-wide tiles would pad 300 by 28 %).  Built (reduction-major tiles with
// 640-byte rows: one DMA piece per row, 40 of 64 lanes active), correct (tests/test_hip_dense_dispatch.py, in a child process) and MEASURED SLOWER
// (profiles/r03_kernel_roofline_tile160.txt): one workgroup per CU and 157 x 2 = 314 tiles for 256 CUs leave the second round of
// workgroups on 58 CUs — 20000x300x300 forward 60.1 us against 51.5 us on the 128x64 tile, dX+dW 117 against 108 us, the
// config-5 step 4.34 against 4.27 ms.  OFF by default; ESC_TILE160=1 enables it for experiments.
inline bool use160(const PlanKnobs& k, int64_t rows, int64_t cols) {
  return k.tile160 && tile160_ok(cols) && cols % 128 != 0 && cdiv(rows, 128) * cdiv(cols, 160) >= k.tile160_min_wgs;
}
inline bool narrow_ok(int64_t N, int64_t K, Op X, Op W, const Flags& f) {
  return N <= NARROW_N && K <= NARROW_K && K % 4 == 0 && vec_ok(X) && vec_ok(W) && f.pro_aligned;
}
// the operands (not yet the prologue) suit the LDS-DMA forward
inline bool dma_fwd_operands(const PlanKnobs& k, Op X, Op W, int64_t M, int64_t N, int64_t K) {
  return (k.use_dma & 1) && K % 4 == 0 && K >= 32 && dma_ok(X, M) && dma_ok(W, N);
}
inline bool pro_fits(const Flags& f, int64_t K) { return !f.pro || cdiv(K, 32) * 32 <= PRO_MAX_K; }
inline int dma_fwd_rows(const PlanKnobs& k, int64_t M, int64_t N) { return (fwd_big(k, M, N) || use160(k, M, N)) ? 128 : 64; }
// the LDS-DMA gradients: dX needs W and dX, dW needs X and the slabs
inline bool dma_bwd_ok(const PlanKnobs& k, Op dY, const Op* X, const Op* W, const Op* dX, const void* slabs, int64_t M, int64_t N, int64_t K) {
  if (!(k.use_dma & 2) || N <= 32 || K <= 32 || N % 4 != 0 || K % 4 != 0 || !dma_ok(dY, M)) return false;
  if (W && (!dma_ok(*W, N) || !dma_ok(*dX, M))) return false;      // (N % 4 == 0 checked above: partial last K-step)
  if (X && (!dma_ok(*X, M) || !aligned16(slabs))) return false;
  return true;
}

inline Plan with_family(Plan p, Family f, int bm, int bn) { p.family = f; p.ok = f != F_NONE; p.bm = bm; p.bn = bn; return p; }
inline Plan with_r01(Plan p, Family f, int id, bool db) {
  p.tile = r01_tile_id(id, db);
  return with_family(p, f, R01_TILE[p.tile].bm, R01_TILE[p.tile].bn);
}
inline Plan with_splits(Plan p, int64_t splits, int64_t per, int64_t N, int64_t K) {
  p.splits = (int)splits; p.per_split = (int)per; p.slab_floats = splits * (N * K + N);
  return p;
}
// split-M plan of the LDS-DMA weight gradient for a BMxBN output tile: ~one workgroup per CU, splits >= 128 rows deep
inline Plan dma_wgrad_splits(Plan p, int64_t M, int64_t N, int64_t K) {
  const int64_t tiles = cdiv(N, p.bm) * cdiv(K, p.bn);
  int64_t sp = cdiv(256, tiles);
  const int64_t max_sp = cdiv(M, 128);
  if (sp > max_sp) sp = max_sp;
  if (sp < 1) sp = 1;
  int64_t pr = cdiv(cdiv(M, sp), 32) * 32;
  if (pr < 128) pr = 128;
  return with_splits(p, cdiv(M, pr), pr, N, K);
}
// ... and of the r01 tiles: enough splits along M for ~KNOB_DW_BLOCKS workgroups, each >= 128 rows deep (fixed by the shape and
// the knobs only, so scratch sizing and the launch agree)
inline Plan r01_wgrad_splits(const PlanKnobs& k, Plan p, int64_t M, int64_t N, int64_t K) {
  const Tile& t = R01_TILE[p.tile];
  const int64_t tiles = cdiv(N, t.bm) * cdiv(K, t.bn);
  const int64_t want = cdiv(k.knob[KNOB_DW_BLOCKS], tiles);
  const int64_t max_splits = cdiv(M, k.knob[KNOB_DW_MIN_ROWS] < 128 ? 128 : k.knob[KNOB_DW_MIN_ROWS]);
  int64_t sp = want < 1 ? 1 : (want > max_splits ? max_splits : want);
  if (sp < 1) sp = 1;
  const int64_t per = cdiv(cdiv(M, sp), t.bk) * t.bk;
  sp = cdiv(M, per);
  if (sp < 1) sp = 1;
  return with_splits(p, sp, per, N, K);
}

// ---- forward: esc_linear_fwd, _bn_fwd (f.bn), _fwd_from (f.c_init), _fwd_fold (f.fold), _fwd_l1 (N = 1, W = {w, K}) ---------
inline Plan plan_fwd(const PlanKnobs& k, Op X, Op W, int64_t M, int64_t N, int64_t K, const Flags& f) {
  Plan p;
  const bool plain = !f.c_init && !f.fold;
  if (!f.col_stats && !f.c_init && narrow_ok(N, K, X, W, f)) return with_family(p, F_NARROW, 0, N == 1 ? 1 : 4);
  if (plain && (k.use_dma & 4) && K <= small::SMALL_MAX && !f.pro && N > 32) {     // in_dim-wide inputs: see linear_small.h
    p.block_rows = small::ROWS_FWD;
    p.bn_after = f.bn ? BN_FROM_ROWS : BN_NONE;
    return with_family(p, F_SMALLK, small::ROWS_FWD, 256);
  }
  // edge-sized BatchNorm'd outputs have hundreds of partials per column — a wide finalize launch is faster than the last workgroup
  const bool in_kernel = f.bn && M <= FUSE_FINALIZE_MAX_ROWS && f.last_block_finalize;
  const bool operands = dma_fwd_operands(k, X, W, M, N, K);
  if (!in_kernel && operands && pro_fits(f, K)) {
    p.bn_after = f.bn ? BN_FROM_ROWS : BN_NONE;
    const bool big = fwd_big(k, M, N);
    if (!plain) {                  // partial-result and fold forms: the 128x128 and 64x64 instantiations only
      if (N <= 32 || (f.c_init && big && !tile128_ok(N))) return p;
      p.block_rows = big ? 128 : 64;
      return big ? with_family(p, F_DMA128, 128, 128) : with_family(p, F_DMA64, 64, 64);
    }
    if (N <= 32) {                 // narrow outputs (GINEConv.lin 256 -> 10): a 64x32 tile, bandwidth-bound on X
      if ((k.use_dma & 8) && !f.col_stats) return with_family(p, F_DMA64X32, 64, 32);
    } else {
      p.block_rows = dma_fwd_rows(k, M, N);
      if (use160(k, M, N)) return with_family(p, F_DMA160, 128, 160);       // 300 / 600-wide outputs with enough row tiles
      if (!big) return with_family(p, F_DMA64, 64, 64);                     // node-sized: 4 compute + 2 loader waves
      if (f.pro || tile128_ok(N)) return with_family(p, F_DMA128, 128, 128);
      return with_family(p, F_DMA128X64, 128, 64);                          // N = 300: 5 x 64 instead of 3 x 128
    }
  }
  if (!plain) return p;            // LDS-DMA tiles only
  int id = (N <= 32) ? 2 : (edge_sized(M) ? k.knob[KNOB_FWD_BIG] : k.knob[KNOB_FWD_SMALL]);
  // node-sized rows with a long reduction (lin1: K = (L+1)*H): 152 workgroups would each walk 20 K-steps alone;
  // the 32x32 tile whose 4 wave groups split every K-step puts 4x the waves on the chip (42 -> 32 us)
  if (N > 32 && !edge_sized(M) && K >= 1024 && id == 4) id = 8;
  if (in_kernel) {
    if (id >= 8) id = 4;           // the fused finalize lives in the one-wave-group tiles only
    p.bn_after = BN_IN_KERNEL;
    return with_r01(p, F_R01_BN, id, false);
  }
  // operands the LDS-DMA tiles serve, but a prologue beyond their K limit: esc_linear_stats_block_rows (which is not told about
  // the prologue) has promised their row blocks, the register-staged tiles write 32-row ones — the partials are taken from Y
  if (f.col_stats && operands && N > 32) {
    p.block_rows = dma_fwd_rows(k, M, N);
    p.bn_after = f.bn ? BN_FROM_ROWS : BN_NONE;
    return with_r01(p, F_R01_ROWSTATS, id, false);
  }
  p.bn_after = f.bn ? BN_FROM_PARTIALS : BN_NONE;
  return with_r01(p, F_R01, id, false);
}
// rows per col_stats partial block of a forward: the caller is not asked about the prologue, so this is the call without one
inline int64_t stats_block_rows(const PlanKnobs& k, Op X, Op W, int64_t M, int64_t N, int64_t K) {
  Flags f;
  f.col_stats = true;
  return plan_fwd(k, X, W, M, N, K, f).block_rows;
}
inline bool fold_available(const PlanKnobs& k) { return (k.use_dma & 1) != 0; }

// ---- input gradient --------------------------------------------------------------------------------------------------
inline Plan plan_dx(const PlanKnobs& k, Op dY, Op W, Op dX, int64_t M, int64_t N, int64_t K) {
  Plan p;
  if (N <= NARROW_DX_N && K <= NARROW_K && K % 4 == 0 && vec_ok(W) && vec_ok(dX)) return with_family(p, F_NARROW_DX, 0, N <= 4 ? 4 : 16);
  if ((k.use_dma & 4) && K <= small::SMALL_MAX && N % 4 == 0 && N <= small::SMALLN_DX_MAX_N && vec_ok(dY)) return with_family(p, F_SMALLN_DX, 32, 0);
  if (dma_bwd_ok(k, dY, nullptr, &W, &dX, nullptr, M, N, K)) {
    if (use160(k, M, K)) return with_family(p, F_DMA160_DX, 128, 160);
    if (edge_sized(M) && tile128_ok(K)) return with_family(p, F_DMA128_DX, 128, 128);
    return with_family(p, F_DMA64_DX, 64, 64);
  }
  return with_r01(p, F_R01_DX, (K <= 32) ? 2 : (edge_sized(M) ? k.knob[KNOB_DX_BIG] : k.knob[KNOB_DX_SMALL]), false);
}

// ---- weight gradient -------------------------------------------------------------------------------------------------
inline Plan plan_dw(const PlanKnobs& k, Op dY, Op X, const void* slabs, int64_t M, int64_t N, int64_t K) {
  Plan p;
  if ((k.use_dma & 4) && (K <= small::SMALL_MAX) != (N <= small::SMALL_MAX))        // one tiny feature dimension: linear_small.h
    return with_splits(with_family(p, F_SMALL_DW, 0, 256), cdiv(M, small::ROWS_WGRAD), small::ROWS_WGRAD, N, K);
  if (dma_bwd_ok(k, dY, &X, nullptr, nullptr, slabs, M, N, K)) {
    const bool big = bwd_big(M, N, K);
    return dma_wgrad_splits(big ? with_family(p, F_DMA128_DW, 128, 128) : with_family(p, F_DMA64_DW, 64, 64), M, N, K);
  }
  return r01_wgrad_splits(k, with_r01(p, F_R01_DW, k.knob[KNOB_DW_TILE], true), M, N, K);
}

// ---- both gradients in one call (dX.p == nullptr: no input gradient wanted) -------------------------------------------------
inline Plan plan_both(const PlanKnobs& k, Op dY, Op X, Op W, Op dX, Op dW, const void* slabs, int64_t M, int64_t N, int64_t K,
                      const Flags& f) {
  Plan p;
  const bool want_dx = dX.p != nullptr;
  const bool rows_ok = M > 0 && M < (1LL << 31) && dW.ld >= K && f.pro_paired;
  // dX rows and the dW / db shares in one pass over X and dY (see linear_narrow_bwd)
  if (rows_ok && dY.ld >= N && (!want_dx || (vec_ok(dX) && dX.ld >= K)) && aligned16(slabs) && narrow_ok(N, K, X, W, f))
    return with_splits(with_family(p, F_NARROW_BOTH, NARROW_ROWS, N == 1 ? 1 : 4), cdiv(M, NARROW_ROWS), NARROW_ROWS, N, K);
  if (want_dx && rows_ok && dma_bwd_ok(k, dY, &X, &W, &dX, slabs, M, N, K)) {        // dX tiles + split-M dW slabs of the LDS-DMA family in ONE launch
    const bool big = bwd_big(M, N, K);
    if (use160(k, M, K))           // dX tiles 128 rows x 160 of the K columns; the dW job rides on the same tile over [N, K]
      return dma_wgrad_splits(with_family(p, F_DMA160_DUAL, 128, 160), M, N, K);
    return dma_wgrad_splits(big ? with_family(p, F_DMA128_DUAL, 128, 128) : with_family(p, F_DMA64_DUAL, 64, 64), M, N, K);
  }
  const bool sized = M > 0 && N > 0 && K > 0;            // (the entries refuse anything else; no slab plan for it)
  if (!want_dx || N <= 32 || K <= 32) {                  // other narrow shapes keep their dedicated tiles
    const Plan w = sized ? plan_dw(k, dY, X, slabs, M, N, K) : p;
    return with_splits(with_family(p, F_SPLIT, w.bm, w.bn), w.splits, w.per_split, N, K);
  }
  // edge-sized: 64x64xBK32 (4 workgroups/CU); node-sized: KNOB_DUAL_SMALL picks 64x64xBK64 (0), the 2-wave 32x64xBK32 tile (1)
  // that doubles the workgroup count of these under-filled grids, or 64x64xBK32 (2)
  const int small_tile = k.knob[KNOB_DUAL_SMALL];
  const int id = (edge_sized(M) || (small_tile != 0 && small_tile != 1)) ? 1 : (small_tile == 1 ? 5 : 4);
  p = with_r01(p, F_R01_DUAL, id, true);
  return sized ? r01_wgrad_splits(k, p, M, N, K) : p;
}

// ---- both gradients with the BatchNorm(+ReLU) backward of dOut folded in (esc_linear_bwd_both_bn) ---------------------------
// beta: read when relu == 2 (ELU: the derivative is taken at the centred pre-activation (x - mean) * scale + beta), else ignored
struct BnOps { const void* x; int64_t ld_x; const void *mean, *invstd, *scale, *shift, *coef; int relu; const void* beta; };
struct NextOps { const void* partial; const void* x; int64_t ld_x; const void *mean, *invstd, *scale, *shift; int relu; const void* beta; };
// The C structs of include/escgnn_hip.h (esc_bn_bwd_fused, esc_bn_bwd_next: templates, so that this header needs neither) as plan
// operands — the one translation, for esc_linear_bwd_both_bn (linear_mfma.hip) and for the step engines' schedule (engine_plan.h)
template <class Fused> inline BnOps bn_ops(const Fused& b) { return BnOps{b.x, b.ld_x, b.mean, b.invstd, b.scale, b.shift, b.coef, b.relu, b.beta}; }
template <class Next> inline NextOps next_ops(const Next& n) { return NextOps{n.partial, n.x, n.ld_x, n.mean, n.invstd, n.scale, n.shift, n.relu, n.beta}; }
inline bool elu_beta_ok(int relu, const void* beta) { return relu != 2 || (beta != nullptr && aligned16(beta)); }
inline bool bn_ops_ok(const BnOps& b, int64_t M, int64_t N) {
  return b.x && b.mean && b.invstd && b.scale && b.shift && b.coef && b.relu >= 0 && b.relu <= 2 && b.ld_x >= N &&
         dma_ok(Op{b.x, b.ld_x}, M) && aligned16(b.mean) && aligned16(b.invstd) && aligned16(b.scale) && aligned16(b.shift) &&
         aligned16(b.coef) && elu_beta_ok(b.relu, b.beta);
}
inline bool next_ops_ok(const NextOps& n, Op dX, int64_t K) {
  return n.partial && n.x && n.mean && n.invstd && n.scale && n.shift && n.ld_x >= K && n.ld_x % 4 == 0 && aligned16(n.x) &&
         aligned16(n.mean) && aligned16(n.invstd) && aligned16(n.scale) && aligned16(n.shift) && aligned16(n.partial) && K % 4 == 0 &&
         vec_ok(dX) && n.relu >= 0 && n.relu <= 2 && elu_beta_ok(n.relu, n.beta);
}
inline int64_t bwd_bn_block_rows(int64_t M, int64_t N, int64_t K) { return bwd_big(M, N, K) ? 128 : 64; }
// bn / next: nullptr when the call has none (at least one is needed); dX.p may be nullptr on the tiny-K kernels only
inline Plan plan_both_bn(const PlanKnobs& k, Op dOut, const BnOps* bn, Op X, Op W, Op dX, const void* slabs, const NextOps* next,
                         int64_t M, int64_t N, int64_t K) {
  Plan p;
  if (!dOut.p || !X.p || !W.p || !slabs || M <= 1 || N <= 0 || K <= 0 || (bn == nullptr && next == nullptr)) return p;
  // edge-sized rows ride on the 128x128 tile (4 compute + 4 loader waves, one workgroup per CU, three ring stages even with the
  // third operand image): only the square-ish H-wide layers it serves; everything else is node-sized
  const bool big = bwd_big(M, N, K);
  if (edge_sized(M) && !(big && bn != nullptr && N <= BNB_MAX_N)) return p;
  if (bn != nullptr && !bn_ops_ok(*bn, M, N)) return p;
  p.block_rows = (int)bwd_bn_block_rows(M, N, K);
  if (bn != nullptr && (k.use_dma & 4) && K <= small::SMALL_MAX && N > small::SMALL_MAX && N % 4 == 0 && N <= small::SMALLN_DX_MAX_N) {
    // in_dim-wide Linear (x_embedding.0, conv1.nn.0): see linear_small.h
    if (next != nullptr || !vec_ok(dOut) || dOut.ld < N || X.ld < K || W.ld < K || (dX.p != nullptr && dX.ld < K)) return p;
    return with_splits(with_family(p, F_SMALL_BN, 0, 256), cdiv(M, small::ROWS_WGRAD), small::ROWS_WGRAD, N, K);
  }
  if (dX.p == nullptr || N > BNB_MAX_N) return p;
  if (!dma_bwd_ok(k, dOut, &X, &W, &dX, slabs, M, N, K)) return p;
  if (next != nullptr && !next_ops_ok(*next, dX, K)) return p;
  if (k.dual_split > 0) { p.launches = 2; p.dx_lds = k.dual_split > 1 ? (k.dual_split < LDS_BYTES ? k.dual_split : LDS_BYTES) : 0; }
  return dma_wgrad_splits(big ? with_family(p, F_DMA128_BN, 128, 128) : with_family(p, F_DMA64_BN, 64, 64), M, N, K);
}
// ... from the entry's own arguments (b, n: the C structs, or nullptr)
template <class Fused, class Next>
inline Plan plan_both_bn(const PlanKnobs& k, Op dOut, const Fused* b, Op X, Op W, Op dX, const void* slabs, const Next* n, int64_t M,
                         int64_t N, int64_t K) {
  BnOps bo{};
  NextOps no{};
  if (b) bo = bn_ops(*b);
  if (n) no = next_ops(*n);
  return plan_both_bn(k, dOut, b ? &bo : nullptr, X, W, dX, slabs, n ? &no : nullptr, M, N, K);
}

// ---- the scratch promise: an upper bound over every plan a knob setting can produce ----------------------------------------
// at most ceil(M/128) splits on the tiles; the tiny-dimension kernels (linear_small.h) and the narrow both-kernel
// (linear_narrow_bwd: whenever N <= NARROW_N and K <= NARROW_K, K <= 16 included) cut the rows finer, their slabs are a few KB each
static_assert(NARROW_ROWS == small::ROWS_WGRAD, "one promise covers both 32-row plans");
inline int64_t bwd_weight_scratch(int64_t M, int64_t N, int64_t K) {
  const bool fine = (K <= small::SMALL_MAX) != (N <= small::SMALL_MAX) || (N <= NARROW_N && K <= NARROW_K);
  return (cdiv(M, fine ? small::ROWS_WGRAD : 128) + 1) * (N * K + N);
}

}  // namespace plan
}  // namespace esc
