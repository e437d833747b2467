// linear_mfma.hip — the dense layers of NestedGIN_eff on the gfx950 matrix cores in exact fp32.
//
//   forward      Y[M,N]  = act(X)[M,K] * W[N,K]^T + bias           (torch.nn.Linear)
//   input grad   dX[M,K] = dY[M,N] * W[N,K]
//   weight grad  dW[N,K] = dY[M,N]^T * act(X)[M,K],  db[N] = colsum(dY)
//
// Call sites replaced: every torch.nn.Linear of /root/reference/run_graphcount.py:54-121,183-189
// and GINEConv.lin (edge_dim -> in_channels), the only GEMM-shaped work on the path.
//
// This file is the dispatch table.  Which family serves a call, with which tile and how many slabs, is decided in
// linear_plan.h (host-only, checked on the CPU by tests/test_linear_plan_cpu.py); every entry below validates its arguments,
// takes the plan, switches on its family and launches.  The kernels live beside it:
//   gemm_tile.h      the register-staged MFMA tiles (r01), their dual launch, the ordered slab reduce
//   gemm_dma.h       the LDS-DMA tiles of the H-wide layers
//   linear_small.h   a tiny feature dimension (K or N <= 16)
//   linear_narrow.h  narrow outputs (N <= 4), short reductions (dX of N <= 16), col_stats of a finished Y
#include "common.h"
#include <cstdlib>
#include "linear_plan.h"
#include "gemm_tile.h"
#include "gemm_dma.h"
#include "linear_small.h"
#include "linear_narrow.h"

namespace esc {

using plan::Flags;
using plan::Op;
using plan::Plan;

// ---- the knob state: esc_tune_set (runtime.hip) writes it, the environment switches are read once at the first dispatch ------
static plan::PlanKnobs g_plan;
void set_linear_knob(int knob, int value) {
  if (knob == 11) g_plan.use_dma = value;
  else if (knob == 14) g_plan.dual_split = value;
  else g_plan.knob[knob] = value;
}
// the step engine's request for the calling thread's NEXT esc_linear_bwd_both_bn call (common.h): PlanKnobs::dual_split for that
// call only, with the events that its two launches signal
static thread_local DualSplit t_dual_split;
static thread_local bool t_dual_split_on = false;
void request_dual_split(const DualSplit& r) { t_dual_split = r; t_dual_split_on = true; }
bool take_dual_split() { const bool pending = t_dual_split_on; t_dual_split_on = false; t_dual_split = DualSplit{}; return pending; }
static const plan::PlanKnobs& knobs() {
  static const bool env_read = [] {
    if (getenv("ESC_BIG_MIN_WGS")) g_plan.big_min_wgs = atoll(getenv("ESC_BIG_MIN_WGS"));
    if (getenv("ESC_TILE160")) g_plan.tile160 = atoi(getenv("ESC_TILE160"));
    if (getenv("ESC_TILE160_MIN_WGS")) g_plan.tile160_min_wgs = atoll(getenv("ESC_TILE160_MIN_WGS"));
    return true;
  }();
  (void)env_read;
  return g_plan;
}
const plan::PlanKnobs& linear_plan_knobs() { return knobs(); }      // (the step engines' schedule plans with the same values: engine.hip)

// the plan's constants are the kernels' own
using DmaBnCfg = dma::Cfg<64, 64, 32, 2, 2, 2, 2, false, true, 4, false, false>;
static_assert(DmaBnCfg::BNB_MAXK == BNB_MAX_N && DmaBnCfg::PRO_MAXK == PRO_MAX_K, "linear_plan.h and gemm_dma.h disagree on the LDS-resident vectors");
static_assert(plan::R01_TILE[1].bm == 64 && plan::R01_TILE[1].bn == 64 && plan::R01_TILE[1].bk == 32 && plan::R01_TILE[1].kw == 1, "tile 1 is the default tile");

static Flags pro_flags(const float* in_scale, const float* in_shift) {
  Flags f;
  f.pro = in_scale != nullptr;
  f.pro_aligned = in_scale == nullptr || (aligned16(in_scale) && aligned16(in_shift));
  f.pro_paired = (in_scale == nullptr) == (in_shift == nullptr);
  return f;
}
#define ESC_TRY_(x) do { int rc__ = (x); if (rc__ != ESC_OK) return rc__; } while (0)
static inline hipError_t dma_check(hipError_t e, const char* what) {
  if (e != hipSuccess) { set_error("%s: %s", what, hipGetErrorString(e)); (void)hipGetLastError(); }     // (do not leave it for the next call's launch check)
  return e;
}

// ---- launchers: one per kernel family, instantiations picked from the plan ----------------------------------------------------
// the LDS-DMA tile shapes: BM, BN, BK, compute waves WM x WN, ring stages, loader waves
#define ESC_T64X32 64, 32, 32, 2, 1, 3, 2
#define ESC_T64 64, 64, 32, 2, 2, 3, 2
#define ESC_T128X64 128, 64, 32, 2, 2, 3, 2
#define ESC_T128 128, 128, 32, 2, 2, 3, 4
#define ESC_T160 128, 160, 32, 4, 1, 3, 4

template <bool AKC, bool BKC, bool PRO, bool DB>
static void launch_r01(int tile, const GemmArgs& g, int splits, hipStream_t s) {
#define ESC_TILE(I)                                                                                                         \
  launch_tile<plan::R01_TILE[I].bm, plan::R01_TILE[I].bn, plan::R01_TILE[I].wm, plan::R01_TILE[I].wn, plan::R01_TILE[I].bk, \
              AKC, BKC, PRO, DB, plan::R01_TILE[I].kw>(g, splits, s)
  switch (tile) {                  // (a row of plan::R01_TILE: plan::r01_tile_id has folded unknown ids into tile 1)
    case 0: ESC_TILE(0); break;
    case 2: ESC_TILE(2); break;
    case 3: ESC_TILE(3); break;
    case 4: ESC_TILE(4); break;
    case 5: ESC_TILE(5); break;
    case 6: ESC_TILE(6); break;
    case 7: ESC_TILE(7); break;
    case 8: if constexpr (!DB) ESC_TILE(8); break;          // the in-workgroup split-K tiles write no slabs
    case 9: if constexpr (!DB) ESC_TILE(9); break;
    case 10: if constexpr (!DB) ESC_TILE(10); break;
    default: ESC_TILE(1); break;
  }
#undef ESC_TILE
}

static GemmArgs r01_dx_args(const float* dY, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M, int64_t N, int64_t K, float* dX,
                            int64_t ld_dx, int accumulate) {
  GemmArgs g{};
  g.A = dY; g.lda = ld_dy; g.B = W; g.ldb = ld_w; g.C = dX; g.ldc = ld_dx; g.bias = nullptr;
  g.rowsC = (int)M; g.colsC = (int)K; g.red = (int)N; g.red_per_split = (int)N; g.accumulate = accumulate;
  g.a_vec = plan::vec_ok(Op{dY, ld_dy}); g.b_vec = plan::vec_ok(Op{W, ld_w}); g.c_slab = 0;
  return g;
}
static GemmArgs r01_dw_args(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* in_scale, const float* in_shift,
                            int64_t M, int64_t N, int64_t K, float* slabs, const Plan& p) {
  GemmArgs g{};
  g.A = dY; g.lda = ld_dy; g.B = X; g.ldb = ld_x; g.C = slabs; g.ldc = K; g.bias = nullptr;
  g.pro_scale = in_scale; g.pro_shift = in_shift;
  g.db_part = slabs + (size_t)p.splits * N * K;
  g.rowsC = (int)N; g.colsC = (int)K; g.red = (int)M; g.red_per_split = p.per_split; g.accumulate = 0;
  g.a_vec = plan::vec_ok(Op{dY, ld_dy});
  g.b_vec = plan::vec_ok(Op{X, ld_x}) && pro_flags(in_scale, in_shift).pro_aligned;
  g.c_slab = 1;
  return g;
}
static void dma_fill_dx(dma::GArgs& g, const float* dY, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M, int64_t N,
                        int64_t K, float* dX, int64_t ld_dx, int accumulate) {
  g.A = dY; g.lda = (int)ld_dy; g.B = W; g.ldb = (int)ld_w; g.C = dX; g.ldc = (int)ld_dx;
  g.M = (int)M; g.N = (int)K; g.R = (int)N; g.red_per_split = (int)N; g.accumulate = accumulate;
}
static void dma_fill_dw(dma::GArgs& g, const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* in_scale,
                        const float* in_shift, int64_t M, int64_t N, int64_t K, float* slabs, const Plan& p) {
  g.A = dY; g.lda = (int)ld_dy; g.B = X; g.ldb = (int)ld_x; g.C = slabs; g.ldc = (int)K;
  g.pro_scale = in_scale; g.pro_shift = in_shift; g.db_part = slabs + (size_t)p.splits * N * K;
  g.M = (int)N; g.N = (int)K; g.R = (int)M; g.red_per_split = p.per_split; g.accumulate = 0;
}

// the narrow forward in its three forms: plain (in_scale optional), with the BatchNorm in front still in partial form, and the
// H -> 1 head that also leaves the L1 loss gradient
enum NarrowForm { NARROW_PLAIN, NARROW_FOLD, NARROW_L1 };
static void launch_narrow_fwd(NarrowForm form, const float* X, int64_t ld_x, const float* W, int64_t ld_w, const float* bias,
                              const float* in_scale, const float* in_shift, int64_t M, int64_t N, int64_t K, float* Y, int64_t ld_y,
                              const BnFoldDev& fold, const NarrowL1& l1, hipStream_t s) {
  const unsigned blocks = (unsigned)(cdiv(M, 16) < 2048 ? cdiv(M, 16) : 2048);      // 4 rows per wave and pass
#define ESC_NARROW_FWD(...) \
  esc::launch(ESC_K_LINEAR, linear_narrow_fwd<__VA_ARGS__>, dim3(blocks), dim3(256), 0, s, X, ld_x, W, ld_w, bias, in_scale, in_shift, (int)M, (int)N, (int)K, Y, ld_y, fold, l1)
  if (form == NARROW_L1) ESC_NARROW_FWD(1, true, false, true);
  else if (form == NARROW_FOLD) { if (N == 1) ESC_NARROW_FWD(1, true, true); else ESC_NARROW_FWD(4, true, true); }
  else if (N == 1) { if (in_scale) ESC_NARROW_FWD(1, true); else ESC_NARROW_FWD(1, false); }
  else { if (in_scale) ESC_NARROW_FWD(4, true); else ESC_NARROW_FWD(4, false); }
#undef ESC_NARROW_FWD
}

// the forward on the LDS-DMA tile of a plan.  PRO: 0 none, 1 in_scale / in_shift, 3 the folded BatchNorm; c_init: the
// instantiations whose accumulators start from a partial result
static hipError_t launch_dma_fwd(const Plan& p, const dma::GArgs& g, hipStream_t s) {
  const bool pro = g.pro_scale != nullptr;
#define ESC_DMA_FWD(PRO, ...) dma::launch_gemm<__VA_ARGS__, false, false, PRO, true, false>(g, 0, s)
#define ESC_DMA_FWD_FROM(PRO, ...) dma::launch_gemm<__VA_ARGS__, false, false, PRO, true, false, true>(g, 0, s)
  const bool big = p.family == plan::F_DMA128;
  if (g.c_init != nullptr) {
    if (big) return pro ? ESC_DMA_FWD_FROM(1, ESC_T128) : ESC_DMA_FWD_FROM(0, ESC_T128);
    return pro ? ESC_DMA_FWD_FROM(1, ESC_T64) : ESC_DMA_FWD_FROM(0, ESC_T64);
  }
  if (g.fold.partials != nullptr) return big ? ESC_DMA_FWD(3, ESC_T128) : ESC_DMA_FWD(3, ESC_T64);
  switch (p.family) {
    case plan::F_DMA64X32:
      return pro ? dma::launch_gemm<ESC_T64X32, false, false, 1, false, false>(g, 0, s)
                 : dma::launch_gemm<ESC_T64X32, false, false, 0, false, false>(g, 0, s);
    case plan::F_DMA160: return pro ? ESC_DMA_FWD(1, ESC_T160) : ESC_DMA_FWD(0, ESC_T160);
    case plan::F_DMA128: return pro ? ESC_DMA_FWD(1, ESC_T128) : ESC_DMA_FWD(0, ESC_T128);
    case plan::F_DMA128X64: return ESC_DMA_FWD(0, ESC_T128X64);
    default: return pro ? ESC_DMA_FWD(1, ESC_T64) : ESC_DMA_FWD(0, ESC_T64);
  }
#undef ESC_DMA_FWD
#undef ESC_DMA_FWD_FROM
}
static dma::GArgs dma_fwd_args(const float* X, int64_t ld_x, const float* W, int64_t ld_w, const float* bias, const float* in_scale,
                               const float* in_shift, int64_t M, int64_t N, int64_t K, float* Y, int64_t ld_y, float* col_stats) {
  dma::GArgs g{};
  g.A = X; g.lda = (int)ld_x; g.B = W; g.ldb = (int)ld_w; g.C = Y; g.ldc = (int)ld_y; g.bias = bias;
  g.pro_scale = in_scale; g.pro_shift = in_shift; g.col_stats = reinterpret_cast<float2*>(col_stats);
  g.M = (int)M; g.N = (int)N; g.R = (int)K; g.red_per_split = (int)K; g.accumulate = 0;
  return g;
}

// dX[M, K <= 16] on the tiny-dimension kernel; ACT: 0 plain dY, 1 / 2 the BatchNorm + ReLU / ELU backward of dOut applied on the way
static int launch_smalln_dx(const float* dY, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M, int64_t N, int64_t K, float* dX,
                            int64_t ld_dx, int accumulate, const BnbDev& bd, int act, const char* what, hipStream_t s) {
  const size_t lds = (size_t)(32 + small::SMALL_MAX) * (N + 4) * sizeof(float);
  static size_t raised[3] = {64 * 1024, 64 * 1024, 64 * 1024};
  hipError_t e = hipSuccess;
  if (act == 0) e = dma::raise_lds(small::smalln_dx<small::SMALL_MAX>, lds, raised[0]);
  if (act != 0) e = dma::raise_lds(small::smalln_dx<small::SMALL_MAX, 1>, lds, raised[1]);
  if (e == hipSuccess && act == 2) e = dma::raise_lds(small::smalln_dx<small::SMALL_MAX, 2>, lds, raised[2]);
  if (dma_check(e, what) != hipSuccess) return ESC_ELAUNCH;
  auto kern = act == 0 ? small::smalln_dx<small::SMALL_MAX> : (act == 2 ? small::smalln_dx<small::SMALL_MAX, 2> : small::smalln_dx<small::SMALL_MAX, 1>);
  esc::launch(ESC_K_LINEAR, kern, dim3((unsigned)cdiv(M, 32)), dim3(256), lds, s, dY, ld_dy, W, ld_w, (int)M, (int)N, (int)K, dX, ld_dx, accumulate, bd);
  return ESC_OK;
}

// dW slabs on the tiny-dimension kernel (one of N, K <= 16); act as above
static void launch_wgrad_small(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* in_scale, const float* in_shift,
                               int64_t M, int64_t N, int64_t K, float* slabs, const Plan& p, const BnbDev& bd, int act, hipStream_t s) {
  float* db_part = slabs + (size_t)p.splits * N * K;
  const bool small_k = K <= small::SMALL_MAX;
  const dim3 grid((unsigned)p.splits, (unsigned)cdiv(small_k ? N : K, 256));
#define ESC_WGRAD_SMALL(...) \
  esc::launch(ESC_K_LINEAR, small::wgrad_small<small::SMALL_MAX, __VA_ARGS__>, grid, dim3(256), 0, s, dY, ld_dy, X, ld_x, in_scale, in_shift, (int)M, (int)N, (int)K, slabs, db_part, bd)
  if (act == 2)      { if (in_scale) ESC_WGRAD_SMALL(true, true, 2); else ESC_WGRAD_SMALL(true, false, 2); }
  else if (act == 1) { if (in_scale) ESC_WGRAD_SMALL(true, true, 1); else ESC_WGRAD_SMALL(true, false, 1); }
  else if (small_k)  { if (in_scale) ESC_WGRAD_SMALL(true, true); else ESC_WGRAD_SMALL(true, false); }
  else               { if (in_scale) ESC_WGRAD_SMALL(false, true); else ESC_WGRAD_SMALL(false, false); }
#undef ESC_WGRAD_SMALL
}

// the tail of every weight gradient: the ordered slab reduce of the plan's slabs at once (the one-job form of
// esc_slab_reduce_jobs, so that the immediate and the deferred form add the slabs in the same association and give the same
// bits), or its description in *defer
static int reduce_slabs(const Plan& p, const float* slabs, int64_t N, int64_t K, float* dW, int64_t ld_dw, float* db, esc_reduce_job* defer,
                        void* stream) {
  esc_reduce_job now;
  esc_reduce_job* j = defer ? defer : &now;
  j->slabs = slabs; j->n = N * K; j->splits = p.splits; j->cols = K; j->dw = dW; j->ld_dw = ld_dw;
  j->db_part = slabs + (size_t)p.splits * N * K; j->rows = N; j->db = db;
  return defer ? ESC_OK : esc_slab_reduce_jobs(j, 1, stream);
}

}  // namespace esc

using namespace esc;

extern "C" {

// resident workgroups per CU the runtime predicts for the forward kernel of a tile id (diagnostics)
int esc_debug_gemm_occupancy(int tile_id) {
  int n = -1;
#define ESC_OCC(I)                                                                                                              \
  {                                                                                                                             \
    constexpr plan::Tile t = plan::R01_TILE[I];                                                                                 \
    auto kern = gemm_tile_kernel<t.bm, t.bn, t.wm, t.wn, t.bk, true, true, false, false>;                                       \
    const size_t lds = 2 * (KContigTile<t.bm, t.bk>::FLOATS + KContigTile<t.bn, t.bk>::FLOATS) * sizeof(float);                 \
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);    \
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, 256, lds);                                                     \
  }
  switch (tile_id) {
    case 0: ESC_OCC(0) break;
    case 2: ESC_OCC(2) break;
    case 3: ESC_OCC(3) break;
    case 4: ESC_OCC(4) break;
    default: ESC_OCC(1) break;
  }
#undef ESC_OCC
  return n;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
static int linear_fwd_impl(const float* X, int64_t ld_x, const float* W, int64_t ld_w, const float* bias,
                           const float* in_scale, const float* in_shift, int64_t M, int64_t N, int64_t K,
                           float* Y, int64_t ld_y, float* col_stats, const esc_bn_fuse* bn, void* stream) {
  ESC_REQUIRE(X && W && Y, "esc_linear_fwd: null pointer");
  ESC_REQUIRE(M >= 0 && N > 0 && K > 0 && ld_x >= K && ld_w >= K && ld_y >= N, "esc_linear_fwd: bad sizes M=%ld N=%ld K=%ld", (long)M, (long)N, (long)K);
  ESC_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "esc_linear_fwd: in_scale/in_shift must come together");
  ESC_REQUIRE(col_stats == nullptr || N > 32, "esc_linear_fwd: col_stats needs N > 32");
  ESC_REQUIRE(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "esc_linear_fwd: dimension too large");
  ESC_REQUIRE(bn == nullptr || (col_stats && bn->mean && bn->invstd && M > 1), "esc_linear_bn_fwd: needs col_stats, mean, invstd and M > 1");
  ESC_REQUIRE(bn == nullptr || ((bn->scale == nullptr) == (bn->shift == nullptr)), "esc_linear_bn_fwd: scale/shift must come together");
  if (M == 0) return ESC_OK;
  hipStream_t s = (hipStream_t)stream;
  Flags f = pro_flags(in_scale, in_shift);
  f.col_stats = col_stats != nullptr; f.bn = bn != nullptr; f.last_block_finalize = last_block_finalize();
  const Plan p = plan::plan_fwd(knobs(), Op{X, ld_x}, Op{W, ld_w}, M, N, K, f);
  switch (p.family) {
    case plan::F_NARROW:
      launch_narrow_fwd(NARROW_PLAIN, X, ld_x, W, ld_w, bias, in_scale, in_shift, M, N, K, Y, ld_y, BnFoldDev{}, NarrowL1{}, s);
      ESC_CHECK_LAUNCH("esc_linear_fwd.narrow");
      break;
    case plan::F_SMALLK:
      esc::launch(ESC_K_LINEAR, small::smallk_fwd<small::SMALL_MAX>, dim3((unsigned)cdiv(M, small::ROWS_FWD), (unsigned)cdiv(N, 256)),
                  dim3(256), 0, s, X, ld_x, W, ld_w, bias, (int)M, (int)N, (int)K, Y, ld_y, reinterpret_cast<float2*>(col_stats));
      ESC_CHECK_LAUNCH("esc_linear_fwd.smallk");
      break;
    case plan::F_DMA64X32: case plan::F_DMA64: case plan::F_DMA128: case plan::F_DMA128X64: case plan::F_DMA160:
      if (dma_check(launch_dma_fwd(p, dma_fwd_args(X, ld_x, W, ld_w, bias, in_scale, in_shift, M, N, K, Y, ld_y, col_stats), s), "esc_linear_fwd") != hipSuccess)
        return ESC_ELAUNCH;
      break;
    default: {                     // F_R01, F_R01_ROWSTATS, F_R01_BN: the register-staged tiles
      GemmArgs g{};
      g.A = X; g.lda = ld_x; g.B = W; g.ldb = ld_w; g.C = Y; g.ldc = ld_y; g.bias = bias;
      g.pro_scale = in_scale; g.pro_shift = in_shift; g.db_part = nullptr;
      g.col_stats = p.family == plan::F_R01_ROWSTATS ? nullptr : reinterpret_cast<float2*>(col_stats);
      g.rowsC = (int)M; g.colsC = (int)N; g.red = (int)K; g.red_per_split = (int)K; g.accumulate = 0;
      g.a_vec = plan::vec_ok(Op{X, ld_x}) && f.pro_aligned;
      g.b_vec = plan::vec_ok(Op{W, ld_w}); g.c_slab = 0;
      if (p.family == plan::F_R01_BN) {
        g.fin.tickets = tickets((int)cdiv(N, p.bn));
        ESC_REQUIRE(g.fin.tickets != nullptr, "esc_linear_bn_fwd: no ticket counters");
        g.fin.row_tiles = (int)cdiv(M, p.bm);
        g.fin.eps = bn->eps; g.fin.momentum = bn->momentum; g.fin.mean = bn->mean; g.fin.invstd = bn->invstd;
        g.fin.running_mean = bn->running_mean; g.fin.running_var = bn->running_var; g.fin.gamma = bn->gamma;
        g.fin.beta = bn->beta; g.fin.scale = bn->scale; g.fin.shift = bn->shift;
      }
      if (in_scale) launch_r01<true, true, true, false>(p.tile, g, 1, s);
      else          launch_r01<true, true, false, false>(p.tile, g, 1, s);
      ESC_CHECK_LAUNCH("esc_linear_fwd");
      if (p.family == plan::F_R01_ROWSTATS) {
        esc::launch(ESC_K_LINEAR, col_stats_rows_kernel, dim3((unsigned)cdiv(M, p.block_rows), (unsigned)cdiv(N, 256)), dim3(256), 0, s,
                    Y, ld_y, (int)M, (int)N, p.block_rows, reinterpret_cast<float2*>(col_stats));
        ESC_CHECK_LAUNCH("esc_linear_fwd.col_stats");
      }
    }
  }
  if (p.bn_after == plan::BN_FROM_ROWS)
    return esc_bn_stats_from_partials_rows(col_stats, M, N, p.block_rows, bn->eps, bn->momentum, bn->mean, bn->invstd, bn->running_mean,
                                           bn->running_var, bn->gamma, bn->beta, bn->scale, bn->shift, stream);
  if (p.bn_after == plan::BN_FROM_PARTIALS)
    return esc_bn_stats_from_partials(col_stats, M, N, bn->eps, bn->momentum, bn->mean, bn->invstd, bn->running_mean,
                                      bn->running_var, bn->gamma, bn->beta, bn->scale, bn->shift, stream);
  return ESC_OK;
}

int esc_linear_fwd(const float* X, int64_t ld_x, const float* W, int64_t ld_w, const float* bias,
                   const float* in_scale, const float* in_shift, int64_t M, int64_t N, int64_t K,
                   float* Y, int64_t ld_y, float* col_stats, void* stream) {
  return linear_fwd_impl(X, ld_x, W, ld_w, bias, in_scale, in_shift, M, N, K, Y, ld_y, col_stats, nullptr, stream);
}

int esc_linear_bn_fwd(const float* X, int64_t ld_x, const float* W, int64_t ld_w, const float* bias,
                      const float* in_scale, const float* in_shift, int64_t M, int64_t N, int64_t K,
                      float* Y, int64_t ld_y, float* col_stats, const esc_bn_fuse* bn, void* stream) {
  ESC_REQUIRE(bn != nullptr, "esc_linear_bn_fwd: null bn");
  return linear_fwd_impl(X, ld_x, W, ld_w, bias, in_scale, in_shift, M, N, K, Y, ld_y, col_stats, bn, stream);
}

int esc_linear_fold_available(void) { return plan::fold_available(knobs()) ? 1 : 0; }

int64_t esc_linear_stats_block_rows(const float* X, int64_t ld_x, const float* W, int64_t ld_w, int64_t M, int64_t N,
                                    int64_t K) {
  return plan::stats_block_rows(knobs(), Op{X, ld_x}, Op{W, ld_w}, M, N, K);
}

int esc_linear_fwd_fold(const float* X, int64_t ld_x, const float* W, int64_t ld_w, const float* bias,
                        const esc_bn_fold* in_bn, int64_t M, int64_t N, int64_t K, float* Y, int64_t ld_y,
                        float* col_stats, void* stream) {
  ESC_REQUIRE(X && W && Y && in_bn && in_bn->partials && in_bn->mean && in_bn->invstd, "esc_linear_fwd_fold: null pointer");
  ESC_REQUIRE(M > 0 && N > 0 && K > 0 && ld_x >= K && ld_w >= K && ld_y >= N && M < (1LL << 31), "esc_linear_fwd_fold: bad sizes");
  ESC_REQUIRE(in_bn->C == K && in_bn->rows > 1 && in_bn->block_rows > 0, "esc_linear_fwd_fold: the folded BatchNorm must have K channels");
  ESC_REQUIRE((in_bn->scale == nullptr) == (in_bn->shift == nullptr), "esc_linear_fwd_fold: scale/shift must come together");
  hipStream_t s = (hipStream_t)stream;
  BnFoldDev fold{reinterpret_cast<const float2*>(in_bn->partials), (int)cdiv(in_bn->rows, in_bn->block_rows), (int)in_bn->block_rows,
                 (int)in_bn->rows, (int)in_bn->C, in_bn->eps, in_bn->momentum, in_bn->gamma, in_bn->beta, in_bn->mean, in_bn->invstd,
                 in_bn->scale, in_bn->shift, in_bn->running_mean, in_bn->running_var};
  Flags f;
  f.pro = true; f.fold = true; f.col_stats = col_stats != nullptr;
  const Plan p = plan::plan_fwd(knobs(), Op{X, ld_x}, Op{W, ld_w}, M, N, K, f);
  if (p.family == plan::F_NARROW) {
    launch_narrow_fwd(NARROW_FOLD, X, ld_x, W, ld_w, bias, nullptr, nullptr, M, N, K, Y, ld_y, fold, NarrowL1{}, s);
    ESC_CHECK_LAUNCH("esc_linear_fwd_fold.narrow");
    return ESC_OK;
  }
  ESC_REQUIRE(p.ok, "esc_linear_fwd_fold: shape not served by the folding kernels (M=%ld N=%ld K=%ld)", (long)M, (long)N, (long)K);
  dma::GArgs g = dma_fwd_args(X, ld_x, W, ld_w, bias, nullptr, nullptr, M, N, K, Y, ld_y, col_stats);
  g.fold = fold;
  return dma_check(launch_dma_fwd(p, g, s), "esc_linear_fwd_fold") == hipSuccess ? ESC_OK : ESC_ELAUNCH;
}

/* Y = Y0 + act(X) W^T + b with the BatchNorm partials of the RESULT in col_stats: the second half of a Linear whose reduction was cut
 * in two (see include/escgnn_hip.h).  LDS-DMA tiles only. */
int esc_linear_fwd_from(const float* Y0, int64_t ld_y0, const float* X, int64_t ld_x, const float* W, int64_t ld_w, const float* bias,
                        const float* in_scale, const float* in_shift, int64_t M, int64_t N, int64_t K, float* Y, int64_t ld_y,
                        float* col_stats, void* stream) {
  ESC_REQUIRE(Y0 && X && W && Y, "esc_linear_fwd_from: null pointer");
  ESC_REQUIRE(M > 0 && N > 32 && K >= 32 && ld_y0 >= N && ld_x >= K && ld_w >= K && ld_y >= N && M < (1LL << 31), "esc_linear_fwd_from: bad sizes");
  ESC_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "esc_linear_fwd_from: in_scale/in_shift must come together");
  Flags f = pro_flags(in_scale, in_shift);
  f.c_init = true; f.col_stats = col_stats != nullptr;
  const Plan p = plan::plan_fwd(knobs(), Op{X, ld_x}, Op{W, ld_w}, M, N, K, f);
  ESC_REQUIRE(p.ok, "esc_linear_fwd_from: shape not served by the LDS-DMA tiles (M=%ld N=%ld K=%ld)", (long)M, (long)N, (long)K);
  dma::GArgs g = dma_fwd_args(X, ld_x, W, ld_w, bias, in_scale, in_shift, M, N, K, Y, ld_y, col_stats);
  g.c_init = Y0; g.ld_init = (int)ld_y0;
  return dma_check(launch_dma_fwd(p, g, (hipStream_t)stream), "esc_linear_fwd_from") == hipSuccess ? ESC_OK : ESC_ELAUNCH;
}
int esc_linear_fwd_from_ok(const float* X, int64_t ld_x, const float* W, int64_t ld_w, int64_t M, int64_t N, int64_t K, int has_prologue) {
  Flags f;
  f.pro = has_prologue != 0; f.c_init = true;
  return plan::plan_fwd(knobs(), Op{X, ld_x}, Op{W, ld_w}, M, N, K, f).ok ? 1 : 0;
}

/* pred = act(X) w^T + b for ONE output column (the H -> 1 head) and, in the same launch, dpred = d(sum |pred - target| * grad_scale /
 * denom) / d pred — what esc_l1_loss would leave in its dpred (same expression, bit for bit); see include/escgnn_hip.h */
int esc_linear_fwd_l1_ok(const float* X, int64_t ld_x, const float* w, int64_t K, const float* in_scale, const float* in_shift) {
  return (in_scale && in_shift && plan::plan_fwd(knobs(), Op{X, ld_x}, Op{w, K}, 1, 1, K, pro_flags(in_scale, in_shift)).family == plan::F_NARROW) ? 1 : 0;
}
int esc_linear_fwd_l1(const float* X, int64_t ld_x, const float* w, const float* bias, const float* in_scale, const float* in_shift,
                      int64_t M, int64_t K, const float* target, int64_t denom, float grad_scale, float* pred, float* dpred, void* stream) {
  ESC_REQUIRE(X && w && target && pred && dpred, "esc_linear_fwd_l1: null pointer");
  ESC_REQUIRE(M > 0 && K > 0 && ld_x >= K && denom > 0 && M < (1LL << 31), "esc_linear_fwd_l1: bad sizes");
  ESC_REQUIRE(in_scale != nullptr && in_shift != nullptr, "esc_linear_fwd_l1: the head reads pre-BatchNorm rows (in_scale / in_shift)");
  ESC_REQUIRE(esc_linear_fwd_l1_ok(X, ld_x, w, K, in_scale, in_shift), "esc_linear_fwd_l1: shape / alignment not served (K=%ld)", (long)K);
  const NarrowL1 l1{target, (float)((double)grad_scale / (double)denom), dpred};
  launch_narrow_fwd(NARROW_L1, X, ld_x, w, K, bias, in_scale, in_shift, M, 1, K, pred, 1, BnFoldDev{}, l1, (hipStream_t)stream);
  ESC_CHECK_LAUNCH("esc_linear_fwd_l1");
  return ESC_OK;
}

// ---- input gradient -----------------------------------------------------------------------------------------------------------------
int esc_linear_bwd_input(const float* dY, int64_t ld_dy, const float* W, int64_t ld_w, int64_t M,
                         int64_t N, int64_t K, float* dX, int64_t ld_dx, int accumulate,
                         void* stream) {
  ESC_REQUIRE(dY && W && dX, "esc_linear_bwd_input: null pointer");
  ESC_REQUIRE(M >= 0 && N > 0 && K > 0 && ld_dy >= N && ld_w >= K && ld_dx >= K, "esc_linear_bwd_input: bad sizes");
  ESC_REQUIRE(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "esc_linear_bwd_input: dimension too large");
  if (M == 0) return ESC_OK;
  hipStream_t s = (hipStream_t)stream;
  const Plan p = plan::plan_dx(knobs(), Op{dY, ld_dy}, Op{W, ld_w}, Op{dX, ld_dx}, M, N, K);
  switch (p.family) {
    case plan::F_NARROW_DX: {
      const unsigned blocks = (unsigned)(cdiv(M, 16) < 4096 ? cdiv(M, 16) : 4096);
      if (p.bn == 4) esc::launch(ESC_K_LINEAR, linear_narrow_dx<4>, dim3(blocks), dim3(256), 0, s, dY, ld_dy, W, ld_w, (int)M, (int)N, (int)K, dX, ld_dx, accumulate);
      else           esc::launch(ESC_K_LINEAR, linear_narrow_dx<16>, dim3(blocks), dim3(256), 0, s, dY, ld_dy, W, ld_w, (int)M, (int)N, (int)K, dX, ld_dx, accumulate);
      ESC_CHECK_LAUNCH("esc_linear_bwd_input.narrow");
      return ESC_OK;
    }
    case plan::F_SMALLN_DX:
      ESC_TRY_(launch_smalln_dx(dY, ld_dy, W, ld_w, M, N, K, dX, ld_dx, accumulate, BnbDev{}, 0, "esc_linear_bwd_input", s));
      ESC_CHECK_LAUNCH("esc_linear_bwd_input.smalln");
      return ESC_OK;
    case plan::F_DMA160_DX: case plan::F_DMA128_DX: case plan::F_DMA64_DX: {
      dma::GArgs d{};
      dma_fill_dx(d, dY, ld_dy, W, ld_w, M, N, K, dX, ld_dx, accumulate);
      const hipError_t e = p.family == plan::F_DMA160_DX   ? dma::launch_gemm<ESC_T160, false, true, 0, false, false>(d, 0, s)
                           : p.family == plan::F_DMA128_DX ? dma::launch_gemm<ESC_T128, false, true, 0, false, false>(d, 0, s)
                                                           : dma::launch_gemm<ESC_T64, false, true, 0, false, false>(d, 0, s);
      return dma_check(e, "esc_linear_bwd_input") == hipSuccess ? ESC_OK : ESC_ELAUNCH;
    }
    default:
      launch_r01<true, false, false, false>(p.tile, r01_dx_args(dY, ld_dy, W, ld_w, M, N, K, dX, ld_dx, accumulate), 1, s);
      ESC_CHECK_LAUNCH("esc_linear_bwd_input");
      return ESC_OK;
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------
int64_t esc_linear_bwd_weight_scratch(int64_t M, int64_t N, int64_t K) { return plan::bwd_weight_scratch(M, N, K); }

static int weight_impl(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* in_scale,
                       const float* in_shift, int64_t M, int64_t N, int64_t K, float* dW, int64_t ld_dw, float* db,
                       float* slabs, esc_reduce_job* defer, void* stream) {
  ESC_REQUIRE(dY && X && dW && slabs, "esc_linear_bwd_weight: null pointer");
  ESC_REQUIRE(M > 0 && N > 0 && K > 0 && ld_dy >= N && ld_x >= K && ld_dw >= K, "esc_linear_bwd_weight: bad sizes");
  ESC_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "esc_linear_bwd_weight: in_scale/in_shift must come together");
  ESC_REQUIRE(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "esc_linear_bwd_weight: dimension too large");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = plan::plan_dw(knobs(), Op{dY, ld_dy}, Op{X, ld_x}, slabs, M, N, K);
  switch (p.family) {
    case plan::F_SMALL_DW:
      launch_wgrad_small(dY, ld_dy, X, ld_x, in_scale, in_shift, M, N, K, slabs, p, BnbDev{}, 0, s);
      ESC_CHECK_LAUNCH("esc_linear_bwd_weight.small");
      break;
    case plan::F_DMA128_DW: case plan::F_DMA64_DW: {
      dma::GArgs d{};
      dma_fill_dw(d, dY, ld_dy, X, ld_x, in_scale, in_shift, M, N, K, slabs, p);
      hipError_t e;
      if (p.family == plan::F_DMA128_DW) e = in_scale ? dma::launch_gemm<ESC_T128, true, true, 2, false, true>(d, 0, s)
                                                      : dma::launch_gemm<ESC_T128, true, true, 0, false, true>(d, 0, s);
      else                               e = in_scale ? dma::launch_gemm<ESC_T64, true, true, 2, false, true>(d, 0, s)
                                                      : dma::launch_gemm<ESC_T64, true, true, 0, false, true>(d, 0, s);
      if (dma_check(e, "esc_linear_bwd_weight") != hipSuccess) return ESC_ELAUNCH;
      break;
    }
    default: {
      const GemmArgs g = r01_dw_args(dY, ld_dy, X, ld_x, in_scale, in_shift, M, N, K, slabs, p);
      if (in_scale) launch_r01<false, false, true, true>(p.tile, g, p.splits, s);
      else          launch_r01<false, false, false, true>(p.tile, g, p.splits, s);
      ESC_CHECK_LAUNCH("esc_linear_bwd_weight.tiles");
    }
  }
  return reduce_slabs(p, slabs, N, K, dW, ld_dw, db, defer, stream);
}

int esc_linear_bwd_weight(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x,
                          const float* in_scale, const float* in_shift, int64_t M, int64_t N,
                          int64_t K, float* dW, int64_t ld_dw, float* db, float* slabs,
                          void* stream) {
  return weight_impl(dY, ld_dy, X, ld_x, in_scale, in_shift, M, N, K, dW, ld_dw, db, slabs, nullptr, stream);
}

int esc_slab_reduce_jobs(const esc_reduce_job* jobs, int count, void* stream) {
  ESC_REQUIRE(jobs && count > 0 && count <= ESC_MAX_REDUCE_JOBS, "esc_slab_reduce_jobs: 1..%d jobs", ESC_MAX_REDUCE_JOBS);
  ReduceJobs t{};
  t.count = count;
  int blocks = 0;
  for (int j = 0; j < count; ++j) {
    ESC_REQUIRE(jobs[j].slabs && jobs[j].dw && jobs[j].n > 0 && jobs[j].splits > 0, "esc_slab_reduce_jobs: bad job %d", j);
    t.job[j] = jobs[j];
    t.block_start[j] = blocks;
    const esc_reduce_job& q = jobs[j];
    const bool vec = q.n % 4 == 0 && q.cols % 4 == 0 && q.ld_dw % 4 == 0 && aligned16(q.slabs) && aligned16(q.dw);
    t.vec[j] = vec ? 1 : 0;
    blocks += (int)(cdiv(vec ? q.n / 4 : q.n, 64) + (q.db ? cdiv(q.rows, 64) : 0));
  }
  t.block_start[count] = blocks;
  esc::launch(ESC_K_LINEAR, slab_reduce_multi_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, t);
  ESC_CHECK_LAUNCH("esc_slab_reduce_jobs");
  return ESC_OK;
}

// ---- both gradients in one call -------------------------------------------------------------------------------------------------------
static int both_impl(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* in_scale,
                     const float* in_shift, const float* W, int64_t ld_w, int64_t M, int64_t N, int64_t K,
                     float* dX, int64_t ld_dx, int accumulate, float* dW, int64_t ld_dw, float* db,
                     float* slabs, esc_reduce_job* defer, void* stream) {
  ESC_REQUIRE(dY && X && W && dW && slabs, "esc_linear_bwd_both: null pointer");
  hipStream_t s = (hipStream_t)stream;
  const Plan p = plan::plan_both(knobs(), Op{dY, ld_dy}, Op{X, ld_x}, Op{W, ld_w}, Op{dX, ld_dx}, Op{dW, ld_dw}, slabs, M, N, K,
                                 pro_flags(in_scale, in_shift));
  switch (p.family) {
    case plan::F_NARROW_BOTH: {
      float* db_part = slabs + (size_t)p.splits * N * K;
#define ESC_NARROW_BWD(NM) \
      if (in_scale) esc::launch(ESC_K_LINEAR, linear_narrow_bwd<NM, true>, dim3(p.splits), dim3(256), 0, s, dY, ld_dy, X, ld_x, W, ld_w, in_scale, in_shift, (int)M, (int)N, (int)K, dX, ld_dx, accumulate, slabs, db_part); \
      else          esc::launch(ESC_K_LINEAR, linear_narrow_bwd<NM, false>, dim3(p.splits), dim3(256), 0, s, dY, ld_dy, X, ld_x, W, ld_w, in_scale, in_shift, (int)M, (int)N, (int)K, dX, ld_dx, accumulate, slabs, db_part)
      if (p.bn == 1) { ESC_NARROW_BWD(1); } else { ESC_NARROW_BWD(4); }
#undef ESC_NARROW_BWD
      ESC_CHECK_LAUNCH("esc_linear_bwd_both.narrow");
      break;
    }
    case plan::F_DMA160_DUAL: case plan::F_DMA128_DUAL: case plan::F_DMA64_DUAL: {
      dma::DualArgs a{};
      dma_fill_dx(a.dx, dY, ld_dy, W, ld_w, M, N, K, dX, ld_dx, accumulate);
      dma_fill_dw(a.dw, dY, ld_dy, X, ld_x, in_scale, in_shift, M, N, K, slabs, p);
      hipError_t e;
      if (p.family == plan::F_DMA160_DUAL)      e = in_scale ? dma::launch_dual<ESC_T160, true>(a, 0, s) : dma::launch_dual<ESC_T160, false>(a, 0, s);
      else if (p.family == plan::F_DMA128_DUAL) e = in_scale ? dma::launch_dual<ESC_T128, true>(a, 0, s) : dma::launch_dual<ESC_T128, false>(a, 0, s);
      else                                      e = in_scale ? dma::launch_dual<ESC_T64, true>(a, 0, s) : dma::launch_dual<ESC_T64, false>(a, 0, s);
      if (dma_check(e, "esc_linear_bwd_both") != hipSuccess) return ESC_ELAUNCH;
      break;
    }
    case plan::F_SPLIT: {
      const int rc = weight_impl(dY, ld_dy, X, ld_x, in_scale, in_shift, M, N, K, dW, ld_dw, db, slabs, defer, stream);
      if (rc || dX == nullptr) return rc;
      return esc_linear_bwd_input(dY, ld_dy, W, ld_w, M, N, K, dX, ld_dx, accumulate, stream);
    }
    default: {                     // F_R01_DUAL: dX tiles and dW slabs of the register-staged family in one launch
      ESC_REQUIRE(M > 0 && ld_dy >= N && ld_x >= K && ld_w >= K && ld_dx >= K && ld_dw >= K, "esc_linear_bwd_both: bad sizes");
      ESC_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "esc_linear_bwd_both: in_scale/in_shift must come together");
      ESC_REQUIRE(M < (1LL << 31) && N < (1LL << 31) && K < (1LL << 31), "esc_linear_bwd_both: dimension too large");
      DualArgs a{};
      a.dx = r01_dx_args(dY, ld_dy, W, ld_w, M, N, K, dX, ld_dx, accumulate);
      a.dw = r01_dw_args(dY, ld_dy, X, ld_x, in_scale, in_shift, M, N, K, slabs, p);
      a.dx_nx = (int)cdiv(K, p.bn); a.dx_ny = (int)cdiv(M, p.bm);
      a.dw_nx = (int)cdiv(K, p.bn); a.dw_ny = (int)cdiv(N, p.bm); a.dw_nz = p.splits;
#define ESC_DUAL(I, PRO) launch_dual<plan::R01_TILE[I].bm, plan::R01_TILE[I].bn, plan::R01_TILE[I].wm, plan::R01_TILE[I].wn, plan::R01_TILE[I].bk, PRO>(a, s)
      if (p.tile == 5)      { if (in_scale) ESC_DUAL(5, true); else ESC_DUAL(5, false); }
      else if (p.tile == 1) { if (in_scale) ESC_DUAL(1, true); else ESC_DUAL(1, false); }
      else                  { if (in_scale) ESC_DUAL(4, true); else ESC_DUAL(4, false); }
#undef ESC_DUAL
      ESC_CHECK_LAUNCH("esc_linear_bwd_both.tiles");
    }
  }
  return reduce_slabs(p, slabs, N, K, dW, ld_dw, db, defer, stream);
}

int esc_linear_bwd_both(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* in_scale,
                        const float* in_shift, const float* W, int64_t ld_w, int64_t M, int64_t N, int64_t K,
                        float* dX, int64_t ld_dx, int accumulate, float* dW, int64_t ld_dw, float* db,
                        float* slabs, void* stream) {
  return both_impl(dY, ld_dy, X, ld_x, in_scale, in_shift, W, ld_w, M, N, K, dX, ld_dx, accumulate, dW, ld_dw, db, slabs,
                   nullptr, stream);
}

/* same, but the ordered slab reduce is NOT launched: its description is returned in *job for esc_slab_reduce_jobs.
 * `slabs` must then stay untouched until that call. */
int esc_linear_bwd_both_deferred(const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* in_scale,
                                 const float* in_shift, const float* W, int64_t ld_w, int64_t M, int64_t N, int64_t K,
                                 float* dX, int64_t ld_dx, int accumulate, float* dW, int64_t ld_dw, float* db,
                                 float* slabs, esc_reduce_job* job, void* stream) {
  ESC_REQUIRE(job, "esc_linear_bwd_both_deferred: null job");
  return both_impl(dY, ld_dy, X, ld_x, in_scale, in_shift, W, ld_w, M, N, K, dX, ld_dx, accumulate, dW, ld_dw, db, slabs,
                   job, stream);
}

// ---- Linear backward with the BatchNorm(+ReLU) backward of its dY folded in (include/escgnn_hip.h, r03) ----------------
static Plan plan_both_bn(const float* dOut, int64_t ld_dout, const esc_bn_bwd_fused* b, const float* X, int64_t ld_x, const float* W,
                         int64_t ld_w, int64_t M, int64_t N, int64_t K, const float* dX, int64_t ld_dx, const float* slabs,
                         const esc_bn_bwd_next* n) {
  plan::PlanKnobs k = knobs();
  if (t_dual_split_on) k.dual_split = t_dual_split.dx_lds > 1 ? t_dual_split.dx_lds : 1;
  return plan::plan_both_bn(k, Op{dOut, ld_dout}, b, Op{X, ld_x}, Op{W, ld_w}, Op{dX, ld_dx}, slabs, n, M, N, K);
}

int esc_linear_bwd_both_bn_ok(const float* dOut, int64_t ld_dout, const esc_bn_bwd_fused* bn, const float* X, int64_t ld_x,
                              const float* W, int64_t ld_w, int64_t M, int64_t N, int64_t K, const float* dX, int64_t ld_dx,
                              const float* slabs, const esc_bn_bwd_next* next) {
  return plan_both_bn(dOut, ld_dout, bn, X, ld_x, W, ld_w, M, N, K, dX, ld_dx, slabs, next).ok ? 1 : 0;
}

int64_t esc_linear_bwd_bn_block_rows(int64_t M, int64_t N, int64_t K) { return plan::bwd_bn_block_rows(M, N, K); }

int esc_linear_bwd_both_bn(const float* dOut, int64_t ld_dout, const esc_bn_bwd_fused* bn, const float* X, int64_t ld_x,
                           const float* in_scale, const float* in_shift, const float* W, int64_t ld_w, int64_t M,
                           int64_t N, int64_t K, float* dX, int64_t ld_dx, int accumulate, float* dW, int64_t ld_dw,
                           float* db, float* slabs, esc_reduce_job* defer, const esc_bn_bwd_next* next, void* stream) {
  ESC_REQUIRE(dOut && X && W && dW && slabs, "esc_linear_bwd_both_bn: null pointer");
  ESC_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), "esc_linear_bwd_both_bn: in_scale/in_shift must come together");
  ESC_REQUIRE(ld_dw >= K, "esc_linear_bwd_both_bn: bad sizes");
  const Plan p = plan_both_bn(dOut, ld_dout, bn, X, ld_x, W, ld_w, M, N, K, dX, ld_dx, slabs, next);
  ESC_REQUIRE(p.ok, "esc_linear_bwd_both_bn: shape / alignment not served (M=%ld N=%ld K=%ld) - use esc_bn_bwd + esc_linear_bwd_both", (long)M, (long)N, (long)K);
  hipStream_t s = (hipStream_t)stream;
  // (ELU: the offset of the pre-activation is beta, on the centred rows — common.h BnbDev)
  const BnbDev bd = bn ? BnbDev{bn->x, (int)bn->ld_x, bn->mean, bn->invstd, bn->scale, bn->relu == 2 ? bn->beta : bn->shift,
                                reinterpret_cast<const float2*>(bn->coef), bn->relu}
                       : BnbDev{};
  if (p.family == plan::F_SMALL_BN) {
    const int act = bd.relu == 2 ? 2 : 1;
    launch_wgrad_small(dOut, ld_dout, X, ld_x, in_scale, in_shift, M, N, K, slabs, p, bd, act, s);
    ESC_CHECK_LAUNCH("esc_linear_bwd_both_bn.small");
    if (dX != nullptr) {
      ESC_TRY_(launch_smalln_dx(dOut, ld_dout, W, ld_w, M, N, K, dX, ld_dx, accumulate, bd, act, "esc_linear_bwd_both_bn", s));
      ESC_CHECK_LAUNCH("esc_linear_bwd_both_bn.smalln");
    }
    return reduce_slabs(p, slabs, N, K, dW, ld_dw, db, defer, stream);
  }
  dma::DualArgs a{};
  dma_fill_dx(a.dx, dOut, ld_dout, W, ld_w, M, N, K, dX, ld_dx, accumulate);
  dma_fill_dw(a.dw, dOut, ld_dout, X, ld_x, in_scale, in_shift, M, N, K, slabs, p);
  a.dx.bnb = bd; a.dw.bnb = bd;
  // two launches (plan::PlanKnobs::dual_split): the engine's request, consumed here, names the events they signal
  dma::DualEvents ev{};
  ev.split = p.launches == 2;
  ev.dx_lds = (size_t)p.dx_lds;
  if (ev.split && t_dual_split_on) { ev.dx_done = t_dual_split.dx_done; ev.dw_done = t_dual_split.dw_done; (void)take_dual_split(); }
  if (next)
    a.dx.bst = BnStatDev{reinterpret_cast<float2*>(next->partial), next->x, (int)next->ld_x, next->mean, next->invstd, next->scale,
                         next->relu == 2 ? next->beta : next->shift, next->relu};
  hipError_t e;
  // (the third operand image of the fused apply costs a ring stage: two stages keep the workgroup at 54 KB, which fits beside
  // an edge-stream GEMM on a CU; three stages — 78 KB — measured slower inside the two-stream step, and neutral (0.988 vs 0.985 ms)
  // once the backward's node workgroups keep off the edge GEMMs' CUs altogether)
#define ESC_T64_2STAGE 64, 64, 32, 2, 2, 2, 2
  if (p.family == plan::F_DMA128_BN) {
    if (next) e = in_scale ? dma::launch_dual<ESC_T128, true, true, true>(a, 0, s, ESC_K_LINEAR, nullptr, ev) : dma::launch_dual<ESC_T128, false, true, true>(a, 0, s, ESC_K_LINEAR, nullptr, ev);
    else      e = in_scale ? dma::launch_dual<ESC_T128, true, true, false>(a, 0, s, ESC_K_LINEAR, nullptr, ev) : dma::launch_dual<ESC_T128, false, true, false>(a, 0, s, ESC_K_LINEAR, nullptr, ev);
  } else {
    if (bn == nullptr) e = in_scale ? dma::launch_dual<ESC_T64, true, false, true>(a, 0, s, ESC_K_LINEAR, nullptr, ev) : dma::launch_dual<ESC_T64, false, false, true>(a, 0, s, ESC_K_LINEAR, nullptr, ev);
    else if (next)     e = in_scale ? dma::launch_dual<ESC_T64_2STAGE, true, true, true>(a, 0, s, ESC_K_LINEAR, nullptr, ev) : dma::launch_dual<ESC_T64_2STAGE, false, true, true>(a, 0, s, ESC_K_LINEAR, nullptr, ev);
    else               e = in_scale ? dma::launch_dual<ESC_T64_2STAGE, true, true, false>(a, 0, s, ESC_K_LINEAR, nullptr, ev) : dma::launch_dual<ESC_T64_2STAGE, false, true, false>(a, 0, s, ESC_K_LINEAR, nullptr, ev);
  }
#undef ESC_T64_2STAGE
  if (dma_check(e, "esc_linear_bwd_both_bn") != hipSuccess) return ESC_ELAUNCH;
  return reduce_slabs(p, slabs, N, K, dW, ld_dw, db, defer, stream);
}

}  // extern "C"
