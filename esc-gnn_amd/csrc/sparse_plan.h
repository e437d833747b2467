// sparse_plan.h — which kernel serves a call of the index-driven row kernels (aggregate.hip, bag.hip, embed.hip, gineplus.hip,
// gatedgcn.hip), on which grid, with how much LDS, into how many slots: decided ONCE, on the host.
//
// Host-only C++ like linear_plan.h and norm_plan.h (g++ compiles it alone, tests/sparse_plan_host.cpp does).  Every function is a
// pure function of operand addresses (alignment only), leading dimensions, sizes, which optional operands are given and a
// SparseKnobs value that the .hip files fill from the environment where and when they always read it.  Nothing here allocates
// (family_name builds a string; no entry calls it).  The entries validate, take a plan and switch on its family; the query
// entries (esc_gine_aggregate_bwd_*_slots, esc_bag_fwd_stats_block_rows, esc_bag_bwd_scratch, esc_gineplus_bwd_blocks) answer
// from here.  To add a family: an enum member (+ its name), a clause in the plan_* function, one `case` in the entry, and its
// transcription plus a table case in tests/sparse_cases.py (tests/test_sparse_plan_cpu.py holds the two together).
#pragma once
#include <initializer_list>
#include <string>

#include "linear_plan.h"

namespace esc {
namespace sparse {
using plan::aligned16;
using plan::cdiv;
using plan::Op;
using plan::vec_ok;

// ---- the constants of the dispatch ---------------------------------------------------------------------------------
constexpr int64_t WAVE_MIN_C = 64;            // aggregate forward: a wave per row from here, a thread per (row, channel) below
constexpr int64_t ROWS_WG = 4;                // rows (waves) of a 256-thread workgroup of the wave-per-row kernels
constexpr int64_t SPLIT_C = 256;              // rows of exactly this width may be split over two waves (SparseKnobs::agg_split*)
constexpr int BAG_CH = 64;                    // entries per chunk of the table gradient
constexpr int BAG_EB = 128;                   // tiled forward: edges per workgroup = rows per BatchNorm partial of its statistics
constexpr int BAG_CAP = 192;                  // ... table rows a workgroup can stage (256 B each)
constexpr int BAG_ENT = 6144;                 // ... entries a workgroup can keep in LDS (4 bytes each)
constexpr int BAG_MAXROWS = 4096;             // ... table height the row map serves
constexpr int64_t LOCAL_BUCKETS = 8;          // L2-local schedule of the table gradient: one bucket per XCD,
constexpr int64_t LOCAL_MIN_BYTES = 4 << 20;  // ... taken when the gradient rows outgrow one XCD's L2
constexpr int64_t LOCAL_MIN_CHUNKS = 64;      // ... and there are enough chunks to spread over the buckets
constexpr int64_t PASS2_LDS_MAX = 64 * 1024;  // bag_bwd_pass2 keeps [3][H] floats in the default dynamic LDS
constexpr int GP_K_MAX = 4;                   // GINE+: hops
constexpr int GP_BWD_WAVES = 8;               // ... waves per workgroup of the backward: their d_eps partials are added in LDS
constexpr int GP_BWD_MAX_BLOCKS = 512;        // ... each wave takes rows wave, wave + W, ...: the partials stay a few hundred rows
constexpr int64_t GG_GROUP16_MAX_C = 64, GG_GROUP32_MAX_C = 128;      // GatedGCN: float4 lanes per node = 16 | 32 | 64
constexpr int64_t GG_MAX_C = 1024;            // ... esc_gated_gcn_max_channels
constexpr int GROUP_BLOCK = 256;              // ... threads of every workgroup of the lane-group kernels: four waves
constexpr int64_t EMBED_V4_MAX_C = 256, EMBED_MAX_ROWS = 4096;       // esc_embed_bwd: float4 form up to here | "a small table"

// ESC_AGG_SPLIT (default 2: the forward splits 256-wide rows over two waves; 1 switches it off), ESC_AGG_SPLIT_BWD (default 1;
// 2 switches the split on for the backward), ESC_BAG_TILED (default 0; 1 enables the LDS-staged bag forward)
struct SparseKnobs {
  int agg_split = 2, agg_split_bwd = 1, bag_tiled = 0;
};

// ---- families ----------------------------------------------------------------------------------------------------------
enum Kind { K_AGG_FWD = 0, K_AGG_BWD, K_POOL, K_BAG_FWD, K_BAG_BWD, K_CLASSIFY, K_EMBED_BWD, K_GP_FWD, K_GP_BWD, K_GATED_FWD, K_GATED_BWD, K_COUNT };
enum Family { F_NONE = 0 /* refused, or nothing to launch */, F_WAVE2, F_WAVE4, F_WAVE1, F_ELEM, F_V4, F_V1, F_ROW4, F_ROW1, F_TILED, F_TILED_ACC,
              F_TILED_STATS, F_FLAT, F_LOCAL, F_LAUNCH, F_ONE_ROW, F_GENERIC, F_GROUP16, F_GROUP32, F_GROUP64, F_COUNT };

struct Grid { unsigned x = 0, y = 0; };
struct Plan {
  Kind kind = K_AGG_FWD;
  Family family = F_NONE;
  bool vec = false;                          // float4 (float2 with split == 2) access to every row
  bool affine = false, span = false, stats = false, accumulate = false, classify = false;       // the kernel's other template arguments
  bool refused = false;                      // the entry returns an error (bag forward: before it launches; table gradient: before pass 2)
  Grid grid[3];                              // of each launch, in launch order
  int launches = 0;
  size_t lds = 0;                            // dynamic LDS of the one launch that asks for any, bytes
  int split = 1;                             // aggregate: waves per row
  int cw = 0;                                // embed generic: columns per pass | GatedGCN: lanes per node
  int64_t slots = 0;                         // promised: deps_part entries per row | BatchNorm partial slots (stats) | block rows | d_eps partials
  int64_t chunks = 0, order_offset = 0, bucket_offset = 0;       // table gradient: offsets in 4-byte words behind `partials`
};
// "agg_fwd:wave2+affine+span", "bag_bwd:local:v4+classify", "gated_bwd:16", ...: the FAMILIES of tests/sparse_cases.py
inline std::string family_name(const Plan& p) {
  static const char* const kind[K_COUNT] = {"agg_fwd", "agg_bwd", "pool", "bag_fwd", "bag_bwd", "classify", "embed_bwd", "gp_fwd", "gp_bwd",
                                            "gated_fwd", "gated_bwd"};
  static const char* const fam[F_COUNT] = {"none", "wave2", "wave4", "wave1", "elem", "v4", "v1", "row4", "row1", "tiled", "tiled:acc",
                                           "tiled:stats", "flat", "local", "launch", "one_row", "generic", "16", "32", "64"};
  std::string s = std::string(kind[p.kind]) + ":" + fam[p.family];
  if (p.kind == K_BAG_BWD) s += p.vec ? ":v4" : ":scalar";
  if (p.affine) s += "+affine";
  if (p.span) s += "+span";
  if (p.stats && p.kind == K_AGG_BWD) s += "+stats";
  if (p.accumulate && (p.family == F_ROW4 || p.family == F_ROW1)) s += "+acc";
  if (p.classify) s += "+classify";
  return s;
}

// ---- the one alignment test ----------------------------------------------------------------------------------------------
inline Op mat(const void* p, int64_t ld) { return Op{p, p ? ld : 0}; }          // an operand that was not given constrains nothing
// float4 access to every row: C and the leading dimensions multiples of 4, bases 16-byte aligned (a vector: ld = 0)
inline bool rows_vec(int64_t C, std::initializer_list<Op> ms) {
  bool ok = C % 4 == 0;
  for (const Op& m : ms) ok = ok && vec_ok(m);
  return ok;
}

inline Plan with_launch(Plan p, unsigned x, unsigned y = 1) { p.grid[p.launches].x = x; p.grid[p.launches++].y = y; return p; }
inline Plan start(Kind k, Family f, bool vec) { Plan p; p.kind = k; p.family = f; p.vec = vec; return p; }

// ---- GINE aggregate ------------------------------------------------------------------------------------------------------
inline int agg_split(int knob, int64_t C) { return (knob == 2 && C == SPLIT_C) ? 2 : 1; }
// esc_gine_aggregate_bwd_deps_slots: by the width alone — a call whose operands rule the float2 kernel out writes one entry per row
inline int deps_slots(const SparseKnobs& k, int64_t C) { return agg_split(k.agg_split_bwd, C); }
inline int64_t stats_slots(int64_t N) { return cdiv(N, ROWS_WG); }              // esc_gine_aggregate_bwd_stats_slots

// esc_gine_aggregate_fwd (affine = false) and _fwd_affine, which has refused C < 64 and operands without float4 access before
inline Plan plan_agg_fwd(const SparseKnobs& k, Op x, Op e, Op out, int64_t N, int64_t C, bool affine, bool span_armed) {
  if (C < WAVE_MIN_C) return with_launch(start(K_AGG_FWD, F_ELEM, false), (unsigned)cdiv(N * C, 256));
  const bool vec = rows_vec(C, {x, e, out});
  const int split = vec ? agg_split(k.agg_split, C) : 1;
  Plan p = start(K_AGG_FWD, split == 2 ? F_WAVE2 : vec ? F_WAVE4 : F_WAVE1, vec);
  p.split = split;
  p.affine = affine;
  // an armed span (esc_prof_span_arm) is honoured only together with split 2: the stamped instantiation exists for the kernel the
  // step runs, agg_fwd_wave<2, true>, alone; an armed launch of any other family runs unstamped
  p.span = affine && span_armed && split == 2;
  return with_launch(p, (unsigned)cdiv(split * N, ROWS_WG));
}
// esc_gine_aggregate_bwd, _bwd_affine and (stats) _bwd_affine_stats, which always runs the float4 kernel on one wave per row
inline Plan plan_agg_bwd(const SparseKnobs& k, Op x, Op e, Op g, Op d_e, Op dx, int64_t N, int64_t C, bool affine, bool stats) {
  const bool vec = rows_vec(C, {x, e, g, d_e, dx});
  const int split = (vec && !stats) ? deps_slots(k, C) : 1;
  Plan p = start(K_AGG_BWD, split == 2 ? F_WAVE2 : vec ? F_WAVE4 : F_WAVE1, vec);
  p.split = split;
  p.affine = affine;
  p.stats = stats;
  p.slots = stats ? stats_slots(N) : deps_slots(k, C);
  if (stats) p.lds = (size_t)ROWS_WG * C * 2 * sizeof(float);                   // [4 waves][C] float2
  return with_launch(p, (unsigned)cdiv(split * N, ROWS_WG));
}
inline Plan plan_segment_pool(Op from, Op to, int64_t G, int64_t C) {
  const bool vec = rows_vec(C, {from, to});
  return with_launch(start(K_POOL, vec ? F_V4 : F_V1, vec), (unsigned)cdiv(G, ROWS_WG));
}

// ---- the ESC bag -----------------------------------------------------------------------------------------------------------
// the LDS-staged forward: needs the switch, the table height, float4 access, at least four workgroups of edges
inline bool bag_tiled_ok(const SparseKnobs& k, const void* table, int64_t rows, int64_t H, Op out, int64_t E) {
  return k.bag_tiled && rows > 0 && rows <= BAG_MAXROWS && rows_vec(H, {Op{table, H}, out}) && E >= 4 * BAG_EB && cdiv(H, 64) <= 65535;
}
inline size_t bag_tiled_lds(int64_t rows) { return (size_t)BAG_CAP * 256 + (size_t)BAG_ENT * 4 + (size_t)((rows + 7) & ~7) * 2 + (size_t)BAG_CAP * 2 + 64; }
// esc_bag_fwd_stats_block_rows: rows per BatchNorm partial of the statistics epilogue (0: this shape is not served by it)
inline int64_t bag_stats_block_rows(const SparseKnobs& k, const void* table, int64_t rows, int64_t H, Op out, int64_t E) {
  return bag_tiled_ok(k, table, rows, H, out, E) ? BAG_EB : 0;
}
// esc_bag_fwd / _acc (rows = 0: they never tile) and esc_bag_fwd_rows, which refuses statistics without the tiled kernel
inline Plan plan_bag_fwd(const SparseKnobs& k, const void* table, int64_t rows, int64_t H, Op out, int64_t E, bool accumulate, const void* stats,
                         bool has_stats) {
  const bool tiled = bag_tiled_ok(k, table, rows, H, out, E);
  Plan p = start(K_BAG_FWD, F_NONE, rows_vec(H, {Op{table, H}, out}));
  p.accumulate = accumulate;
  p.stats = has_stats;
  if (has_stats && !(tiled && !accumulate && aligned16(stats))) { p.refused = true; return p; }
  if (!tiled) {
    p.family = p.vec ? F_ROW4 : F_ROW1;
    return E == 0 ? p : with_launch(p, (unsigned)cdiv(E, ROWS_WG));
  }
  p.family = accumulate ? F_TILED_ACC : has_stats ? F_TILED_STATS : F_TILED;
  p.lds = bag_tiled_lds(rows);
  p.slots = BAG_EB;
  return with_launch(p, (unsigned)cdiv(H, 64), (unsigned)cdiv(E, BAG_EB));
}

// the table gradient's scratch: [chunks][2][H] chunk partials, then order [8][chunks] and bucket_cnt [8] of the local schedule
inline int64_t bag_chunks(int64_t Z) { return cdiv(Z, BAG_CH); }
inline int64_t scratch_floats(int64_t Z, int64_t H) { return 2 * bag_chunks(Z) * H + LOCAL_BUCKETS * bag_chunks(Z) + 64; }      // esc_bag_bwd_scratch
// rows given, the gradient matrix larger than one XCD's L2, enough chunks to spread over 8 groups
inline bool bag_local_schedule(int64_t Z, int64_t H, int64_t rows) {
  return rows > 0 && rows * H * (int64_t)sizeof(float) > LOCAL_MIN_BYTES && bag_chunks(Z) >= LOCAL_MIN_CHUNKS;
}
inline Plan with_schedule(Plan p, int64_t Z, int64_t H) {
  p.chunks = bag_chunks(Z);
  p.order_offset = 2 * p.chunks * H;
  p.bucket_offset = p.order_offset + LOCAL_BUCKETS * p.chunks;
  return p;
}
// esc_bag_bwd_classify (counters = 0) and the step engine's counted form: with counters the launch is always made, on one
// workgroup when there is no schedule to build
inline Plan plan_bag_classify(int64_t Z, int64_t H, int64_t rows, int counters) {
  const bool sched = bag_local_schedule(Z, H, rows);
  if (!sched && counters == 0) return start(K_CLASSIFY, F_NONE, false);
  Plan p = start(K_CLASSIFY, F_LAUNCH, false);
  p.classify = sched;
  if (sched) p = with_schedule(p, Z, H);
  return with_launch(p, sched ? (unsigned)cdiv(p.chunks, 256) : 1u);
}
// esc_bag_bwd_table (rows = 0: never the local schedule) and _table_rows: [classify,] pass 1 (none when Z == 0), pass 2.  `refused`:
// pass 2 would not fit its LDS; the entry finds out behind pass 1, as it always has
inline Plan plan_bag_bwd(Op dz, const void* dtable, const void* partials, int64_t Z, int64_t H, int64_t n_cols, int64_t rows, bool classified) {
  const bool vec = rows_vec(H, {dz, Op{dtable, H}, Op{partials, H}});
  const bool local = Z > 0 && bag_local_schedule(Z, H, rows);
  Plan p = start(K_BAG_BWD, Z == 0 ? F_NONE : local ? F_LOCAL : F_FLAT, vec);
  p.chunks = bag_chunks(Z);
  if (local) {
    p = with_schedule(p, Z, H);
    p.classify = !classified;
    if (p.classify) p = with_launch(p, plan_bag_classify(Z, H, rows, 0).grid[0].x);
    const unsigned per_group = (unsigned)cdiv(cdiv(p.chunks, LOCAL_BUCKETS) * 5 / 4 + 4, 4);       // 25 % slack; the kernel strides beyond
    p = with_launch(p, per_group * (unsigned)LOCAL_BUCKETS);
  } else if (Z > 0) {
    p = with_launch(p, (unsigned)cdiv(p.chunks, ROWS_WG));
  }
  p.lds = (size_t)3 * H * sizeof(float);
  p.refused = p.lds > (size_t)PASS2_LDS_MAX;
  return p.refused ? p : with_launch(p, (unsigned)n_cols);
}

// ---- small embedding tables ------------------------------------------------------------------------------------------------
inline Plan plan_embed_bwd(Op g, const void* dtable, int64_t rows, int64_t C) {
  if (rows == 1) return with_launch(start(K_EMBED_BWD, F_ONE_ROW, false), (unsigned)cdiv(C, 64));
  if (C <= EMBED_V4_MAX_C && rows_vec(C, {g, Op{dtable, C}})) return with_launch(start(K_EMBED_BWD, F_V4, true), (unsigned)rows);
  Plan p = start(K_EMBED_BWD, F_GENERIC, false);
  p.cw = 1;                                     // columns per pass: the next power of two, at most 256
  while (p.cw < C && p.cw < 256) p.cw <<= 1;
  return with_launch(p, (unsigned)rows);
}

// ---- GINE+ -------------------------------------------------------------------------------------------------------------------
struct GpOps { Op x0, x1, x2, x3, e; const void* eps; };           // x_d for d > k: x0 again (as the kernels are handed)
inline bool gp_vec(const GpOps& o, int64_t C, std::initializer_list<Op> more) {
  return rows_vec(C, {o.x0, o.x1, o.x2, o.x3, o.e, Op{o.eps, 0}}) && rows_vec(C, more);
}
inline int64_t gp_bwd_blocks(int64_t N) {                           // esc_gineplus_bwd_blocks
  const int64_t b = cdiv(N, GP_BWD_WAVES);
  return b < 1 ? 1 : (b > GP_BWD_MAX_BLOCKS ? GP_BWD_MAX_BLOCKS : b);
}
inline Plan plan_gineplus_fwd(const GpOps& o, Op out, int64_t N, int64_t C) {
  const bool vec = gp_vec(o, C, {out});
  return with_launch(start(K_GP_FWD, vec ? F_V4 : F_V1, vec), (unsigned)cdiv(N, ROWS_WG));
}
// [gp_bwd_wave, gp_deps_reduce when d_eps is wanted]; slots = the workgroups' d_eps partials
inline Plan plan_gineplus_bwd(const GpOps& o, Op g, Op dx, Op d_e, int64_t N, int64_t C, int k, bool want_deps) {
  const bool vec = gp_vec(o, C, {g, dx, d_e});
  Plan p = start(K_GP_BWD, vec ? F_V4 : F_V1, vec);
  p.slots = gp_bwd_blocks(N);
  p = with_launch(p, (unsigned)p.slots);
  return want_deps ? with_launch(p, (unsigned)cdiv((int64_t)(k + 1) * C, 64)) : p;
}

// ---- GatedGCN ------------------------------------------------------------------------------------------------------------------
inline Plan plan_gated(int64_t N, int64_t C, bool backward) {
  Plan p = start(backward ? K_GATED_BWD : K_GATED_FWD, C <= GG_GROUP16_MAX_C ? F_GROUP16 : C <= GG_GROUP32_MAX_C ? F_GROUP32 : F_GROUP64, true);
  p.cw = p.family == F_GROUP16 ? 16 : p.family == F_GROUP32 ? 32 : 64;
  p = with_launch(p, (unsigned)cdiv(N * p.cw, GROUP_BLOCK));
  return backward ? with_launch(p, p.grid[0].x) : p;
}

}  // namespace sparse
}  // namespace esc
