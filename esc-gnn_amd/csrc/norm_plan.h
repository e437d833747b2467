// norm_plan.h — which kernels serve a BatchNorm call, on which grids, into how many partial slots: decided ONCE, on the host.
//
// Host-only C++ like linear_plan.h (g++ compiles it alone, tests/norm_plan_host.cpp does).  Every function is a pure function of
// operand addresses (alignment only), leading dimensions, M, C, which optional operands are given and a NormKnobs value that
// norm.hip fills per call from runtime.hip's getters.  norm.hip validates, takes a plan and switches on it; esc_bn_scratch and
// esc_bn_bwd_dropout_ok answer from here.  To add a family: an enum member (+ its name), a clause in the plan_* function, one
// `case` in the entry, and its transcription in tests/norm_cases.py::family_of (tests/test_norm_plan_cpu.py holds the two together).
#pragma once
#include <initializer_list>
#include <string>

#include "linear_plan.h"

namespace esc {

constexpr int NORM_ROWBLOCKS = 512;          // scratch sizing: most row blocks (= workgroups per column block) ever used

namespace norm {
using plan::aligned16;
using plan::cdiv;
using plan::Op;
using plan::vec_ok;

// ---- the constants of the dispatch ---------------------------------------------------------------------------------
constexpr int64_t ROWBLOCK_CAP = 64;                            // grid.y of the forward statistics and of the scalar reductions
constexpr int64_t NODE_MIN_ROWS = 64, NODE_MAX_ROWS = 4096;     // "node-sized": the one-launch (knob 13) and fold (knob 12) backward
constexpr int64_t LAST_BLOCK_MAX_ROWS = 4096;                   // knob 8: one workgroup cannot pull hundreds of slots quickly
constexpr int64_t ROWS_WG = 16, ROWS_WG_FAT = 32;               // rows per workgroup: 4 per wave and pass | fewer, fatter workgroups
constexpr int64_t ROWS_YCAP = 2048, FOLD_FWD_YCAP = 1024, LAST_BLOCK_YCAP = 64, FOLD_BWD_YCAP = 32;      // grid.y caps
constexpr int64_t FLAT_CAP = 4096;                              // workgroups of the flat-index (grid-stride) kernels
static_assert(NODE_MAX_ROWS / ROWS_WG <= 256, "bn_bwd_node_kernel: every workgroup of a column block must be co-resident");
// the scratch of esc_bn_stats / esc_bn_bwd*: [NORM_ROWBLOCKS * 4 slots][C] float2 partials, then coef [C] float2
inline int64_t coef_offset(int64_t C) { return (int64_t)NORM_ROWBLOCKS * 4 * C * 2; }      // in floats
inline int64_t scratch_floats(int64_t C) { return coef_offset(C) + 2 * C; }

struct NormKnobs {                           // esc_tune_set 8, 9, 12, 13 (state and defaults: runtime.hip)
  bool last_block_finalize = false;
  int rowblock_cap = 256;
  bool bwd_fold = false, bwd_one_launch = false;
};

// ---- families: the entry's part, the reduction kernel, the elementwise kernel -------------------------------------------
enum Family { F_NONE = 0 /* refused */, F_STATS, F_PARTIALS_32, F_PARTIALS_ROWS, F_FOLD, F_APPLY, F_AFFINE, F_EVAL_COEF, F_BWD, F_BWD_FOLD,
              F_BWD_NODE, F_SUMS, F_COEF, F_BWD_APPLY, F_COEF_PARTIALS, F_DROPOUT_IN, F_DROPOUT_OUT, F_COUNT };
enum Reduce { R_NONE = 0, R_V4, R_SCALAR, R_FUSED /* knob 8: the last workgroup finalizes */ };
enum Apply { A_NONE = 0, A_ROWS, A_FLAT4, A_FLAT1 };

struct Grid { unsigned x = 0, y = 0; };
struct Plan {
  Family family = F_NONE;
  Reduce reduce = R_NONE;
  Apply apply = A_NONE;
  Grid grid[3];                              // of each launch, in launch order
  int launches = 0;
  int slots = 0;                             // [slots][C] float2 partials written to the scratch
};
// "stats:v4", "bwd_apply:rows", "bwd:v4+rows", ...: the FAMILIES of tests/norm_cases.py
inline std::string family_name(const Plan& p) {
  static const char* const base[F_COUNT] = {"none", "stats", "partials:32", "partials:rows", "fold", "apply", "affine", "eval_coef", "bwd",
                                            "bwd:fold", "bwd:node", "sums", "coef", "bwd_apply", "coef_partials", "dropout:in", "dropout:out"};
  static const char* const red[] = {"", ":v4", ":scalar", ":fused_last_block"}, *const app[] = {"", "rows", "flat4", "flat1"};
  return std::string(base[p.family]) + red[p.reduce] + (p.apply == A_NONE ? "" : p.reduce == R_NONE ? ":" : "+") + app[p.apply];
}

// ---- alignment tests, each written once ------------------------------------------------------------------------------
inline Op mat(const void* p, int64_t ld) { return Op{p, p ? ld : 0}; }          // an operand that was not given constrains nothing
// float4 access to every matrix: C and the leading dimensions multiples of 4, bases 16-byte aligned
inline bool mats_vec(int64_t C, std::initializer_list<Op> ms) {
  bool ok = C % 4 == 0;
  for (const Op& m : ms) ok = ok && vec_ok(m);
  return ok;
}
inline bool vecs_aligned(std::initializer_list<const void*> vs) {               // (NULL, an optional vector not given, is aligned)
  bool ok = true;
  for (const void* v : vs) ok = ok && aligned16(v);
  return ok;
}
// the operands of a backward call: Y, dX, gamma / beta, dgamma / dbeta, partial, coef NULL where the call has none
struct BwdOps { Op X, Y, dY, dX; const void *mean, *invstd, *gamma, *beta, *partial, *coef, *dgamma, *dbeta; };
inline bool reduce_wide(const BwdOps& o, int64_t C) { return mats_vec(C, {o.X, o.dY, o.Y}) && vecs_aligned({o.mean, o.invstd, o.gamma, o.beta, o.partial}); }
inline bool apply_vec(const BwdOps& o, int64_t C) { return mats_vec(C, {o.X, o.dY, o.dX, o.Y}) && vecs_aligned({o.gamma}); }
inline bool apply_rows(const BwdOps& o, int64_t C) { return apply_vec(o, C) && vecs_aligned({o.mean, o.invstd, o.beta, o.coef}); }
inline bool node_sized(const BwdOps& o, int64_t M, int64_t C) {
  return M >= NODE_MIN_ROWS && M <= NODE_MAX_ROWS && reduce_wide(o, C) && apply_vec(o, C) && vecs_aligned({o.dgamma, o.dbeta});
}
inline bool dropout_ok(const BwdOps& o, int64_t C) { return reduce_wide(o, C) && apply_rows(o, C); }
// esc_bn_bwd / esc_bn_bwd_dropout keep coef behind the partials of the same scratch
inline BwdOps with_scratch_coef(BwdOps o, int64_t C) {
  o.coef = reinterpret_cast<const void*>(reinterpret_cast<uintptr_t>(o.partial) + 4 * (uintptr_t)coef_offset(C));
  return o;
}

// ---- grid sizing ------------------------------------------------------------------------------------------------------
inline unsigned capped(int64_t n, int64_t cap) { return (unsigned)(n < cap ? n : cap); }
// Row blocks (grid.y) of a reduction: 16 rows each, so >= 4 rows per wave slot, up to `cap`.  ROWBLOCK_CAP = 64 blocks x 4 waves =
// 256 row slots for the forward statistics and the scalar kernels (a slot per WAVE; the finalize merges them with Chan's formula
// and its cost grows with the count — edge-sized forward statistics on 256 row blocks: measured no gain inside the step, r03).
// The float4 backward sums leave one slot per BLOCK, plain sums: NormKnobs::rowblock_cap (knob 9) = 256, swept on MI355X, 35 -> 28
// us edge-sized.
inline unsigned rowblocks(int64_t M, int64_t cap) { return M < 1 ? 1u : capped(cdiv(M, ROWS_WG), cap); }
// a lane owns one column quad (256 columns per workgroup), rows are strided over the waves of grid.y workgroups
inline Grid rows_grid(int64_t M, int64_t C, int64_t rows_per_wg, int64_t ycap) { return Grid{(unsigned)cdiv(C, 256), capped(cdiv(M, rows_per_wg), ycap)}; }
inline Grid flat_grid(int64_t M, int64_t C, bool vec) { return Grid{capped(cdiv(M * (vec ? C / 4 : C), 256), FLAT_CAP), 1}; }
// per-column kernels: 4 columns per workgroup (a wave per column: the finalizes) or 256 (a thread per column)
inline Grid column_grid(int64_t C, int64_t per_wg) { return Grid{(unsigned)cdiv(C, per_wg), 1}; }
inline Grid reduce_grid(int64_t M, int64_t C, bool wide, int64_t cap) { return Grid{(unsigned)cdiv(C, wide ? 256 : 64), rowblocks(M, cap)}; }

inline Plan with_launch(Plan p, Grid g) { p.grid[p.launches++] = g; return p; }
inline Plan one_launch(Family f, Grid g) { return with_launch(Plan{f}, g); }

// ---- forward ----------------------------------------------------------------------------------------------------------
inline Plan plan_stats(Op X, const void* scratch, int64_t M, int64_t C) {
  const bool wide = mats_vec(C, {X}) && vecs_aligned({scratch});
  Plan p = with_launch(with_launch(Plan{F_STATS, wide ? R_V4 : R_SCALAR}, reduce_grid(M, C, wide, ROWBLOCK_CAP)), column_grid(C, 4));
  p.slots = (int)p.grid[0].y * 4;
  return p;
}
// esc_bn_stats_from_partials(_rows), esc_bn_eval_coef, esc_bn_bwd_coef_from_partials: one launch over the columns
inline Plan plan_columns(Family f, int64_t C) { return one_launch(f, column_grid(C, f == F_EVAL_COEF ? 256 : 4)); }
inline Plan plan_apply(Op X, Op Y, int64_t M, int64_t C) {
  const bool vec = mats_vec(C, {X, Y});
  const Plan p{F_APPLY, R_NONE, vec ? A_FLAT4 : A_FLAT1};
  return M == 0 ? p : with_launch(p, flat_grid(M, C, vec));
}
inline Plan plan_affine(Op X, Op Y, const void* scale, const void* shift, int64_t M, int64_t C) {
  const bool vec = mats_vec(C, {X, Y}) && vecs_aligned({scale, shift});
  const bool rows = vec && M < (1LL << 31);            // the rows kernels index rows with an int
  const Plan p{F_AFFINE, R_NONE, rows ? A_ROWS : vec ? A_FLAT4 : A_FLAT1};
  return M == 0 ? p : with_launch(p, rows ? rows_grid(M, C, ROWS_WG, ROWS_YCAP) : flat_grid(M, C, vec));
}
// 32 rows per workgroup: every workgroup re-reads the partials (77 KB for 2 400 rows of 256 columns), so fewer and fatter
// workgroups than the plain affine pass
inline Plan plan_affine_fold(int64_t M, int64_t C) { return one_launch(F_FOLD, rows_grid(M, C, ROWS_WG_FAT, FOLD_FWD_YCAP)); }

// ---- backward ---------------------------------------------------------------------------------------------------------
// the column sums.  divisor_is_M: coef = sums / M (the local BatchNorm); else the sums are still to be all-reduced (SyncBN)
inline Plan plan_bwd_reduce(const NormKnobs& k, const BwdOps& o, int64_t M, int64_t C, bool allow_fuse, bool divisor_is_M) {
  const bool wide = reduce_wide(o, C);
  // node-sized inputs: few fat workgroups (>= 32 rows each) whose last one folds the <= 64 slots itself (knob 8);
  // edge-sized: many workgroups + a wide finalize launch
  const bool fuse = allow_fuse && wide && M <= LAST_BLOCK_MAX_ROWS && divisor_is_M && k.last_block_finalize;
  Plan p{divisor_is_M ? F_COEF : F_SUMS, fuse ? R_FUSED : wide ? R_V4 : R_SCALAR};
  p = with_launch(p, fuse ? rows_grid(M, C, ROWS_WG_FAT, LAST_BLOCK_YCAP) : reduce_grid(M, C, wide, wide ? k.rowblock_cap : ROWBLOCK_CAP));
  p.slots = (int)p.grid[0].y * (wide ? 1 : 4);
  return fuse ? p : with_launch(p, column_grid(C, 4));
}
// dX = gamma * invstd * (g - coef.x - xhat * coef.y)
inline Plan plan_bwd_apply(const BwdOps& o, int64_t M, int64_t C) {
  const bool vec = apply_vec(o, C), rows = apply_rows(o, C);
  return with_launch(Plan{F_BWD_APPLY, R_NONE, rows ? A_ROWS : vec ? A_FLAT4 : A_FLAT1}, rows ? rows_grid(M, C, ROWS_WG, ROWS_YCAP) : flat_grid(M, C, vec));
}
inline Plan plan_bwd(const NormKnobs& k, const BwdOps& ops, int64_t M, int64_t C) {
  const BwdOps o = with_scratch_coef(ops, C);
  const bool node = node_sized(o, M, C);
  Plan p;
  if (k.bwd_one_launch && node) {              // rows per wave are fixed (4, in registers): grid.y is not capped
    p = one_launch(F_BWD_NODE, Grid{(unsigned)cdiv(C, 256), (unsigned)cdiv(M, ROWS_WG)});
    p.slots = (int)p.grid[0].y;
  } else if (k.bwd_fold && node && !k.last_block_finalize) {
    // 32 fat row blocks leave 32 partial slots and the apply kernel adds them itself — no finalize launch
    p = with_launch(one_launch(F_BWD_FOLD, rows_grid(M, C, ROWS_WG_FAT, FOLD_BWD_YCAP)), rows_grid(M, C, ROWS_WG, ROWS_YCAP));
    p.slots = (int)p.grid[0].y;
  } else {
    const Plan a = plan_bwd_apply(o, M, C);
    p = with_launch(plan_bwd_reduce(k, o, M, C, true, true), a.grid[0]);
    p.family = F_BWD;
    p.apply = a.apply;
  }
  return p;
}
// float4 kernels only: F_NONE (the entry refuses) unless the operands suit them
inline Plan plan_bwd_dropout(const NormKnobs& k, const BwdOps& ops, int64_t M, int64_t C, bool mask_on_output) {
  if (!dropout_ok(with_scratch_coef(ops, C), C)) return Plan{};
  Plan p = one_launch(mask_on_output ? F_DROPOUT_OUT : F_DROPOUT_IN, reduce_grid(M, C, true, k.rowblock_cap));
  p.slots = (int)p.grid[0].y;
  return with_launch(with_launch(p, column_grid(C, 4)), rows_grid(M, C, ROWS_WG, ROWS_YCAP));
}

}  // namespace norm
}  // namespace esc
