// gemm_tile.h — the register-staged MFMA tile kernels (the "r01" family) of the dense layers, their dual-launch form, the
// ordered slab reduce and their launchers.  linear_mfma.hip decides when they run (linear_plan.h) and fills their arguments.
//
// v_mfma_f32_32x32x2_f32 (f32 in / f32 accumulate) is a k-ordered fp32 fma chain — no TF32-like
// truncation exists on gfx950 — so results stay within fp32 rounding of the CPU oracle (1e-5 bar).
// Peak 157 TFLOP/s; these shapes (M = E or N_nodes, N,K <= 1280) are short-K, so the kernel is a
// classic LDS-tiled, register-prefetched (global -> VGPR -> LDS, one barrier per 32-deep K step)
// design with 4 waves per workgroup, each owning (BM/WM) x (BN/WN) of the tile as 32x32 MFMA blocks.
//
// Operand forms.  "k-contiguous": the reduction index is the fastest-moving index in memory
// (X[M,K], W[N,K] in forward).  LDS image [row][BK+4]; a lane fetches 4 consecutive k of its row
// with one ds_read_b128 (conflict-free with the +4 pad) and feeds 4 MFMAs — lane half h owns
// k = 8c+4h+t, so the k order inside an 8-chunk is permuted identically for A and B.
// "reduction-major": the reduction index is the row index in memory (W[N,K] for dX, dY and X for
// dW).  LDS image [k][cols+4]; a lane reads single floats (ds_read_b32, consecutive lanes ->
// consecutive banks).
#pragma once
#include "common.h"
#include <type_traits>

namespace esc {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KPAD = 4;

template <int ROWS, int BK, int NTHR = 256>
struct KContigTile {            // [ROWS][BK+KPAD]
  static constexpr int LD = BK + KPAD;
  static constexpr int FLOATS = ROWS * LD;
  static constexpr int QPR = BK / 4;                           // float4 per row
  static constexpr int PER_THREAD = ROWS * QPR / NTHR;         // float4 per thread
  static_assert(ROWS * QPR % NTHR == 0 && NTHR % QPR == 0, "tile must split evenly over the workgroup");
};
template <int COLS, int BK, int NTHR = 256>
struct RedMajorTile {           // [BK][COLS+KPAD]
  static constexpr int LD = COLS + KPAD;
  static constexpr int FLOATS = BK * LD;
  static constexpr int PER_THREAD = BK * (COLS / 4) / NTHR;
  static_assert(BK * (COLS / 4) % NTHR == 0 && NTHR % (COLS / 4) == 0, "tile must split evenly over the workgroup");
};

// ---- global -> register staging ------------------------------------------------------------------
// k-contiguous: rows r0.. of `src` (ld), reduction range [k0, k0+BK); element (r, k) valid iff
// r < rows && k < kdim.  Optional per-k affine+relu (fused BatchNorm+ReLU of the producer).
template <int ROWS, int BK, int NTHR, bool PRO>
__device__ __forceinline__ bool load_kcontig(const float* __restrict__ src, int64_t ld, int r0, int rows,
                                             int k0, int kdim, bool vec_ok,
                                             const float* __restrict__ sc, const float* __restrict__ sh,
                                             float4 (&reg)[KContigTile<ROWS, BK, NTHR>::PER_THREAD]) {
  using T = KContigTile<ROWS, BK, NTHR>;
  const int tid = threadIdx.x;
  const int kq = tid % T::QPR;
  const int k = k0 + kq * 4;
  // Fast path (block-uniform condition): whole 16-B quads inside K.  Loads are UNCONDITIONAL — an
  // out-of-range row is clamped to the last valid row and zeroed by a select — so hipcc emits straight
  // global_load_dwordx4 streams instead of a branch + vmcnt(0) per load.
  if (vec_ok && k0 + BK <= kdim) {
    // RAW loads only: nothing here may depend on the loaded values, or hipcc waits for them on the spot
    // and the prefetch collapses.  The affine+ReLU prologue and the row mask run in finish_kcontig(),
    // right before the LDS store one K-step later.
#pragma unroll
    for (int p = 0; p < T::PER_THREAD; ++p) {
      const int r = r0 + tid / T::QPR + p * (NTHR / T::QPR);
      const int rc = min(r, rows - 1);
      reg[p] = *reinterpret_cast<const float4*>(src + (size_t)rc * ld + k);
    }
    return true;
  }
#pragma unroll
  for (int p = 0; p < T::PER_THREAD; ++p) {
    const int r = r0 + tid / T::QPR + p * (NTHR / T::QPR);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) {
      const float* q = src + (size_t)r * ld + k;
      if (k + 0 < kdim) v.x = q[0];
      if (k + 1 < kdim) v.y = q[1];
      if (k + 2 < kdim) v.z = q[2];
      if (k + 3 < kdim) v.w = q[3];
      if constexpr (PRO) {
        if (k + 0 < kdim) v.x = fmaxf(fmaf(v.x, sc[k + 0], sh[k + 0]), 0.f);
        if (k + 1 < kdim) v.y = fmaxf(fmaf(v.y, sc[k + 1], sh[k + 1]), 0.f);
        if (k + 2 < kdim) v.z = fmaxf(fmaf(v.z, sc[k + 2], sh[k + 2]), 0.f);
        if (k + 3 < kdim) v.w = fmaxf(fmaf(v.w, sc[k + 3], sh[k + 3]), 0.f);
      }
    }
    reg[p] = v;
  }
  return false;
}
// prologue + row mask of a RAW k-contiguous tile (see load_kcontig)
template <int ROWS, int BK, int NTHR, bool PRO>
__device__ __forceinline__ void finish_kcontig(int r0, int rows, float4 s4, float4 h4,
                                               float4 (&reg)[KContigTile<ROWS, BK, NTHR>::PER_THREAD]) {
  using T = KContigTile<ROWS, BK, NTHR>;
  if constexpr (!PRO) {
    if (r0 + ROWS <= rows) return;        // interior tile (block-uniform): nothing to mask, nothing to transform
  }
  const int tid = threadIdx.x;
#pragma unroll
  for (int p = 0; p < T::PER_THREAD; ++p) {
    const int r = r0 + tid / T::QPR + p * (NTHR / T::QPR);
    float4 v = reg[p];
    if constexpr (PRO) {
      v.x = fmaxf(fmaf(v.x, s4.x, h4.x), 0.f); v.y = fmaxf(fmaf(v.y, s4.y, h4.y), 0.f);
      v.z = fmaxf(fmaf(v.z, s4.z, h4.z), 0.f); v.w = fmaxf(fmaf(v.w, s4.w, h4.w), 0.f);
    }
    const bool ok = r < rows;
    reg[p] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
  }
}
template <int ROWS, int BK, int NTHR>
__device__ __forceinline__ void store_kcontig(float* __restrict__ lds, const float4 (&reg)[KContigTile<ROWS, BK, NTHR>::PER_THREAD]) {
  using T = KContigTile<ROWS, BK, NTHR>;
  const int tid = threadIdx.x;
#pragma unroll
  for (int p = 0; p < T::PER_THREAD; ++p) {
    const int r = tid / T::QPR + p * (NTHR / T::QPR);
    *reinterpret_cast<float4*>(lds + r * T::LD + (tid % T::QPR) * 4) = reg[p];
  }
}

// reduction-major: rows (reduction) [k0, k0+BK) of `src`, columns c0..c0+COLS; valid iff k < kdim && c < cols.
// Optional per-COLUMN affine+relu (for act(X) in the weight gradient).
template <int COLS, int BK, int NTHR, bool PRO>
__device__ __forceinline__ bool load_redmajor(const float* __restrict__ src, int64_t ld, int k0, int kdim,
                                              int c0, int cols, bool vec_ok,
                                              const float* __restrict__ sc, const float* __restrict__ sh,
                                              float4 (&reg)[RedMajorTile<COLS, BK, NTHR>::PER_THREAD]) {
  const int tid = threadIdx.x;
  constexpr int QPR = COLS / 4;  // float4 per row
  if (vec_ok && c0 + COLS <= cols) {   // block-uniform fast path: RAW unconditional loads, clamped reduction row
#pragma unroll
    for (int p = 0; p < RedMajorTile<COLS, BK, NTHR>::PER_THREAD; ++p) {
      const int f = tid + p * NTHR;
      const int kk = f / QPR, cq = f % QPR;
      const int kc = min(k0 + kk, kdim - 1);
      reg[p] = *reinterpret_cast<const float4*>(src + (size_t)kc * ld + c0 + cq * 4);
    }
    return true;
  }
#pragma unroll
  for (int p = 0; p < RedMajorTile<COLS, BK, NTHR>::PER_THREAD; ++p) {
    const int f = tid + p * NTHR;
    const int kk = f / QPR, cq = f % QPR;
    const int k = k0 + kk, c = c0 + cq * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < kdim) {
      const float* q = src + (size_t)k * ld + c;
      if (c + 0 < cols) v.x = q[0];
      if (c + 1 < cols) v.y = q[1];
      if (c + 2 < cols) v.z = q[2];
      if (c + 3 < cols) v.w = q[3];
      if constexpr (PRO) {
        if (c + 0 < cols) v.x = fmaxf(fmaf(v.x, sc[c + 0], sh[c + 0]), 0.f);
        if (c + 1 < cols) v.y = fmaxf(fmaf(v.y, sc[c + 1], sh[c + 1]), 0.f);
        if (c + 2 < cols) v.z = fmaxf(fmaf(v.z, sc[c + 2], sh[c + 2]), 0.f);
        if (c + 3 < cols) v.w = fmaxf(fmaf(v.w, sc[c + 3], sh[c + 3]), 0.f);
      }
    }
    reg[p] = v;
  }
  return false;
}
template <int COLS, int BK, int NTHR, bool PRO>
__device__ __forceinline__ void finish_redmajor(int k0, int kdim, float4 s4, float4 h4,
                                                float4 (&reg)[RedMajorTile<COLS, BK, NTHR>::PER_THREAD]) {
  const int tid = threadIdx.x;
  constexpr int QPR = COLS / 4;
  static_assert(NTHR % QPR == 0, "a thread keeps the same column quad for every pass");
  if constexpr (!PRO) {
    if (k0 + BK <= kdim) return;          // full K-step (block-uniform): nothing to mask
  }
#pragma unroll
  for (int p = 0; p < RedMajorTile<COLS, BK, NTHR>::PER_THREAD; ++p) {
    const int f = tid + p * NTHR;
    const int kk = f / QPR;
    float4 v = reg[p];
    if constexpr (PRO) {
      v.x = fmaxf(fmaf(v.x, s4.x, h4.x), 0.f); v.y = fmaxf(fmaf(v.y, s4.y, h4.y), 0.f);
      v.z = fmaxf(fmaf(v.z, s4.z, h4.z), 0.f); v.w = fmaxf(fmaf(v.w, s4.w, h4.w), 0.f);
    }
    const bool ok = k0 + kk < kdim;
    reg[p] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
  }
}
template <int COLS, int BK, int NTHR>
__device__ __forceinline__ void store_redmajor(float* __restrict__ lds, const float4 (&reg)[RedMajorTile<COLS, BK, NTHR>::PER_THREAD]) {
  const int tid = threadIdx.x;
  constexpr int QPR = COLS / 4;
#pragma unroll
  for (int p = 0; p < RedMajorTile<COLS, BK, NTHR>::PER_THREAD; ++p) {
    const int f = tid + p * NTHR;
    *reinterpret_cast<float4*>(lds + (f / QPR) * RedMajorTile<COLS, BK, NTHR>::LD + (f % QPR) * 4) = reg[p];
  }
}

// ---- fragment reads: 4 consecutive MFMA k-steps of one 32-row block -----------------------------
// returns f[t] = operand value for MFMA t of 8-chunk `c8` (k = 8*c8 + 4*h + t)
template <int ROWS, int BK>
__device__ __forceinline__ float4 frag_kcontig(const float* __restrict__ lds, int row0, int c8) {
  const int l = lane_id();
  return *reinterpret_cast<const float4*>(lds + (row0 + (l & 31)) * KContigTile<ROWS, BK>::LD + c8 * 8 + (l >> 5) * 4);
}
template <int COLS, int BK>
__device__ __forceinline__ float4 frag_redmajor(const float* __restrict__ lds, int col0, int c8) {
  const int l = lane_id();
  constexpr int LD = RedMajorTile<COLS, BK>::LD;
  const float* p = lds + (c8 * 8 + (l >> 5) * 4) * LD + col0 + (l & 31);
  return make_float4(p[0], p[LD], p[2 * LD], p[3 * LD]);
}

// =================================================================================================
// Generic tile kernel.  C[BM x BN] (+)= A_op[BM x R] * B_op[R x BN] over reduction range
// [red0, red1) (blockIdx.z selects the split for the weight gradient).
//   A_KC : A operand k-contiguous (rows = output rows)   else reduction-major (cols = output rows)
//   B_KC : B operand k-contiguous (rows = output cols)   else reduction-major (cols = output cols)
// =================================================================================================
// BatchNorm finalize fused behind the statistics epilogue: the last row-tile workgroup of every column tile
// (grid_last_block on tickets[bx]) merges that tile's partials and writes what bn_finalize_kernel would
struct BnFuse {
  unsigned* tickets;        // nullptr = off; one counter per column tile
  int row_tiles;            // workgroups sharing a counter
  float eps, momentum;
  float* mean; float* invstd; float* running_mean; float* running_var;
  const float* gamma; const float* beta; float* scale; float* shift;
};

struct GemmArgs {
  const float* A; int64_t lda;
  const float* B; int64_t ldb;
  float* C; int64_t ldc;
  const float* bias;        // per output column (forward) or nullptr
  const float* pro_scale;   // prologue affine (applies to A if A_KC: per k; to B if !B_KC && !A_KC: per col)
  const float* pro_shift;
  float* db_part;           // weight grad: per-split column sums of A' (= dY)   [splits][rowsC]
  float2* col_stats;        // forward: per 32-row block (mean, M2) of the outputs, [ceil(rowsC/32)][colsC]
  int rowsC, colsC, red;    // output rows, output cols, reduction length
  int red_per_split;
  int accumulate;
  int a_vec, b_vec, c_slab; // alignment flags; c_slab: C is a [splits][rowsC][colsC] slab buffer
  BnFuse fin;
};

// Merge the per-32-row (mean, M2) partials of columns [n0, n0+BN) — every group but possibly the last holds exactly
// 32 rows, so the merge is division-free: with d_p = mean_p - pivot,  mean = pivot + S1/G,
// M2 = sum M2_p + 32 (S2 - S1^2/G)  (fp64, shifted by the first group's mean: no cancellation), then one Chan merge
// with the ragged last group.  NTHR/BN threads share a column (contiguous slot ranges, summed in fixed order).
template <int BN, int NTHR>
__device__ __forceinline__ void bn_finalize_cols(const GemmArgs& g, int n0, float* lds) {
  static_assert(NTHR % BN == 0, "threads must tile the column block");
  constexpr int TPC = NTHR / BN;
  const int tid = threadIdx.x, cl = tid % BN, part = tid / BN;
  const int col = n0 + cl;
  const int M = g.rowsC, C = g.colsC;
  const int full = M / 32;
  double S1 = 0.0, S2 = 0.0, SM = 0.0, pivot = 0.0;
  if (col < C && full > 0) {
    pivot = (double)g.col_stats[col].x;
    const int per = (full + TPC - 1) / TPC;
    const int p0 = part * per, p1 = min(full, p0 + per);
    // the partials were written through to memory by other workgroups: every load is a long-latency miss, so
    // keep 16 of them in flight per thread
    for (int p = p0; p < p1; p += 16) {
      float2 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = g.col_stats[(size_t)min(p + u, p1 - 1) * C + col];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        if (p + u < p1) {
          const double d = (double)v[u].x - pivot;
          S1 += d;
          S2 += d * d;
          SM += (double)v[u].y;
        }
      }
    }
  }
  double* sh = reinterpret_cast<double*>(lds);      // [3][NTHR]; the staging buffers are dead by now
  sh[tid] = S1; sh[NTHR + tid] = S2; sh[2 * NTHR + tid] = SM;
  __syncthreads();
  if (part != 0 || col >= C) return;
#pragma unroll
  for (int q = 1; q < TPC; ++q) { S1 += sh[q * BN + cl]; S2 += sh[NTHR + q * BN + cl]; SM += sh[2 * NTHR + q * BN + cl]; }
  double n = 0.0, mu = 0.0, m2 = 0.0;
  if (full > 0) {
    n = 32.0 * full;
    mu = pivot + S1 / full;
    m2 = SM + 32.0 * (S2 - S1 * S1 / full);
    if (m2 < 0.0) m2 = 0.0;
  }
  if (M > 32 * full) {
    const float2 v = g.col_stats[(size_t)full * C + col];
    chan_merge(n, mu, m2, (double)(M - 32 * full), (double)v.x, (double)v.y);
  }
  const BnFuse& f = g.fin;
  const float is = (float)(1.0 / sqrt(m2 / (double)M + (double)f.eps));
  f.mean[col] = (float)mu;
  f.invstd[col] = is;
  if (f.scale) {
    const float sc = (f.gamma ? f.gamma[col] : 1.f) * is;
    f.scale[col] = sc;
    f.shift[col] = (f.beta ? f.beta[col] : 0.f) - (float)mu * sc;
  }
  if (f.running_mean) f.running_mean[col] = (1.f - f.momentum) * f.running_mean[col] + f.momentum * (float)mu;
  if (f.running_var) f.running_var[col] = (1.f - f.momentum) * f.running_var[col] + f.momentum * (float)(m2 / (double)(M - 1));
}

template <int BM, int BN, int WM, int WN, int BK, bool A_KC, bool B_KC, bool PRO, bool DB, int KW = 1>
__device__ __forceinline__ void gemm_tile_body(const GemmArgs& g, float* __restrict__ lds, int bx, int by, int bz) {
  // KW > 1: KW wave groups share ONE output tile and split every K-step between them (wave group wk owns
  // 8-chunks [wk*BK/8/KW, (wk+1)*BK/8/KW)); their accumulators are summed through LDS in group order at
  // the end.  Node-sized layers only have ~600 32x32 output blocks, i.e. 0.6 waves per SIMD — splitting K
  // in the workgroup is what puts >2 waves on every SIMD so MFMA, LDS and barrier phases overlap.
  constexpr int NTHR = WM * WN * KW * 64;
  static_assert(!DB || KW == 1, "bias-gradient column sums assume one wave group");
  static_assert((BK / 8) % KW == 0, "K-step must split evenly over the wave groups");
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int MT = TM / 32, NT = TN / 32;
  static_assert(MT >= 1 && NT >= 1, "wave tile must hold at least one 32x32 block");
  using ATile = typename std::conditional<A_KC, KContigTile<BM, BK, NTHR>, RedMajorTile<BM, BK, NTHR>>::type;
  using BTile = typename std::conditional<B_KC, KContigTile<BN, BK, NTHR>, RedMajorTile<BN, BK, NTHR>>::type;
  constexpr int STAGE = ATile::FLOATS + BTile::FLOATS;   // one K-step of A then B (LDS holds 2 stages)

  const int m0 = by * BM;
  const int n0 = bx * BN;
  const int split = bz;
  const int red0 = split * g.red_per_split;
  const int red1 = min(g.red, red0 + g.red_per_split);
  const int wave = threadIdx.x >> 6;
  const int wk = wave / (WM * WN);
  const int wm = (wave % (WM * WN)) / WN, wn = wave % WN;
  const int l = lane_id();

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // two register sets: tile kt+1 waits in one while tile kt+2 is being fetched into the other
  float4 ra0[ATile::PER_THREAD], rb0[BTile::PER_THREAD];
  float4 ra1[ATile::PER_THREAD], rb1[BTile::PER_THREAD];
  float dbsum = 0.f;

  // Prologue coefficients travel with the tile they belong to (loaded as RAW values next to it): fetching
  // them at finish time would sit behind the NEXT tile's loads in the in-order vmcnt queue and drain the
  // prefetch.  k-contiguous A: one (scale, shift) quad per K-step; reduction-major B: the thread's column
  // quad never changes, so it is loaded once.
  const float4 one4 = make_float4(1.f, 1.f, 1.f, 1.f), zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ps0 = one4, ph0 = zero4, ps1 = one4, ph1 = zero4, pcs = one4, pch = zero4;
  bool pro_vec = false;
  if constexpr (PRO) {
    pro_vec = A_KC ? (g.a_vec != 0) : (g.b_vec != 0);   // host sets *_vec only if the coefficient vectors are 16-B aligned
    if constexpr (!A_KC) {
      const int c = n0 + (threadIdx.x % (BN / 4)) * 4;
      if (pro_vec && c + 3 < g.colsC) {
        pcs = *reinterpret_cast<const float4*>(g.pro_scale + c);
        pch = *reinterpret_cast<const float4*>(g.pro_shift + c);
      }
    }
  }
  // returns bit0: A tile is RAW (needs finish), bit1: B tile is RAW
  auto gload = [&](int k0, float4 (&ra)[ATile::PER_THREAD], float4 (&rb)[BTile::PER_THREAD], float4& ps, float4& ph) -> int {
    bool rawa, rawb;
    if constexpr (PRO && A_KC) {
      const int k = k0 + (threadIdx.x % (BK / 4)) * 4;
      if (pro_vec && k0 + BK <= red1) {
        ps = *reinterpret_cast<const float4*>(g.pro_scale + k);
        ph = *reinterpret_cast<const float4*>(g.pro_shift + k);
      }
    }
    if constexpr (A_KC) rawa = load_kcontig<BM, BK, NTHR, PRO>(g.A, g.lda, m0, g.rowsC, k0, red1, g.a_vec, g.pro_scale, g.pro_shift, ra);
    else                rawa = load_redmajor<BM, BK, NTHR, false>(g.A, g.lda, k0, red1, m0, g.rowsC, g.a_vec, nullptr, nullptr, ra);
    if constexpr (B_KC) rawb = load_kcontig<BN, BK, NTHR, false>(g.B, g.ldb, n0, g.colsC, k0, red1, g.b_vec, nullptr, nullptr, rb);
    else                rawb = load_redmajor<BN, BK, NTHR, PRO && !A_KC>(g.B, g.ldb, k0, red1, n0, g.colsC, g.b_vec, g.pro_scale, g.pro_shift, rb);
    return (rawa ? 1 : 0) | (rawb ? 2 : 0);
  };
  auto lstore = [&](int buf, int k0, int raw, float4 (&ra)[ATile::PER_THREAD], float4 (&rb)[BTile::PER_THREAD], float4 ps, float4 ph) {
    if (raw & 1) {
      if constexpr (A_KC) finish_kcontig<BM, BK, NTHR, PRO>(m0, g.rowsC, ps, ph, ra);
      else                finish_redmajor<BM, BK, NTHR, false>(k0, red1, zero4, zero4, ra);
    }
    if (raw & 2) {
      if constexpr (B_KC) finish_kcontig<BN, BK, NTHR, false>(n0, g.colsC, zero4, zero4, rb);
      else                finish_redmajor<BN, BK, NTHR, PRO && !A_KC>(k0, red1, pcs, pch, rb);
    }
    float* a_w = lds + buf * STAGE;
    float* b_w = a_w + ATile::FLOATS;
    if constexpr (A_KC) store_kcontig<BM, BK, NTHR>(a_w, ra); else store_redmajor<BM, BK, NTHR>(a_w, ra);
    if constexpr (B_KC) store_kcontig<BN, BK, NTHR>(b_w, rb); else store_redmajor<BN, BK, NTHR>(b_w, rb);
  };
  auto compute = [&](int cur) {
    const float* a_l = lds + cur * STAGE;
    const float* b_l = a_l + ATile::FLOATS;
    if constexpr (DB) {   // column sums of the reduction-major A' tile (bias gradient), block column 0 only
      if (bx == 0 && threadIdx.x < BM) {
#pragma unroll 8
        for (int kk = 0; kk < BK; ++kk) dbsum += a_l[kk * ATile::LD + threadIdx.x];
      }
    }
#pragma unroll
    for (int cc = 0; cc < BK / 8 / KW; ++cc) {
      const int c8 = wk * (BK / 8 / KW) + cc;
      float4 af[MT], bf[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if constexpr (A_KC) af[i] = frag_kcontig<BM, BK>(a_l, wm * TM + i * 32, c8);
        else                af[i] = frag_redmajor<BM, BK>(a_l, wm * TM + i * 32, c8);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if constexpr (B_KC) bf[j] = frag_kcontig<BN, BK>(b_l, wn * TN + j * 32, c8);
        else                bf[j] = frag_redmajor<BN, BK>(b_l, wn * TN + j * 32, c8);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
        }
    }
  };

  const int nk = (red1 > red0) ? (red1 - red0 + BK - 1) / BK : 0;
  int raw0 = 0, raw1 = 0;
  if (nk > 0) raw0 = gload(red0, ra0, rb0, ps0, ph0);
  if (nk > 1) raw1 = gload(red0 + BK, ra1, rb1, ps1, ph1);
  if (nk > 0) lstore(0, red0, raw0, ra0, rb0, ps0, ph0);
  __syncthreads();
  // invariant at the top of iteration kt: LDS[kt&1] = tile kt; register set (kt+1)&1 = tile kt+1 (in flight)
  for (int kt = 0; kt < nk; kt += 2) {
    if (kt + 2 < nk) raw0 = gload(red0 + (kt + 2) * BK, ra0, rb0, ps0, ph0);
    compute(0);
    if (kt + 1 < nk) lstore(1, red0 + (kt + 1) * BK, raw1, ra1, rb1, ps1, ph1);
    __syncthreads();
    if (kt + 1 >= nk) break;
    if (kt + 3 < nk) raw1 = gload(red0 + (kt + 3) * BK, ra1, rb1, ps1, ph1);
    compute(1);
    if (kt + 2 < nk) lstore(0, red0 + (kt + 2) * BK, raw0, ra0, rb0, ps0, ph0);
    __syncthreads();
  }

  if constexpr (KW > 1) {      // sum the KW partial accumulators in group order (deterministic) through LDS
    constexpr int TILE_F = MT * NT * 16 * 64;                  // floats one wave holds
    __syncthreads();                                           // staging buffers are dead from here on
    float* red = lds + (size_t)(wave % (WM * WN)) * (KW - 1) * TILE_F;
    if (wk > 0) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) red[(size_t)(wk - 1) * TILE_F + ((i * NT + j) * 16 + r) * 64 + l] = acc[i][j][r];
    }
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int q = 0; q < KW - 1; ++q)
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] += red[(size_t)q * TILE_F + ((i * NT + j) * 16 + r) * 64 + l];
  }
  // ---- optional BatchNorm statistics of the OUTPUT (bias included), one (mean, M2) pair per column and per
  // 32-row block, merged later by Chan's formula (esc_bn_stats_from_partials): the following BatchNorm needs no
  // extra pass over Y.  Lane halves hold rows 4h..4h+3 (+8k): one cross-half shuffle completes a column.
  if (g.col_stats != nullptr) {
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = n0 + wn * TN + j * 32 + (l & 31);
        const int row0 = m0 + wm * TM + i * 32;
        const float bv = (g.bias && col < g.colsC) ? g.bias[col] : 0.f;
        const int nvalid = min(32, g.rowsC - row0);
        float s1 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
          if (row < g.rowsC) s1 += acc[i][j][r] + bv;
        }
        s1 += __shfl_xor(s1, 32, 64);
        const float mean = nvalid > 0 ? s1 / (float)nvalid : 0.f;
        float m2 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = row0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
          if (row < g.rowsC) { const float d = acc[i][j][r] + bv - mean; m2 = fmaf(d, d, m2); }
        }
        m2 += __shfl_xor(m2, 32, 64);
        if (l < 32 && col < g.colsC && nvalid > 0) {
          float2* dst = g.col_stats + (size_t)(row0 / 32) * g.colsC + col;
          if (g.fin.tickets != nullptr) store_agent(dst, make_float2(mean, m2));   // read by another workgroup
          else *dst = make_float2(mean, m2);
        }
      }
  }
  // ---- epilogue: C/D map of the 32x32 block: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
  float* Cbase = g.C + (g.c_slab ? (size_t)split * g.rowsC * g.ldc : 0);
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int col = n0 + wn * TN + j * 32 + (l & 31);
      if (col >= g.colsC) continue;
      const float bv = g.bias ? g.bias[col] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        if (row < g.rowsC) {
          float* p = Cbase + (size_t)row * g.ldc + col;
          float v = acc[i][j][r] + bv;
          if (g.accumulate) v += *p;
          *p = v;
        }
      }
    }
  if constexpr (DB) {
    if (bx == 0 && threadIdx.x < BM && m0 + (int)threadIdx.x < g.rowsC)
      g.db_part[(size_t)split * g.rowsC + m0 + threadIdx.x] = dbsum;
  }
  if constexpr (KW == 1 && !DB) {
    if (g.fin.tickets != nullptr) {      // uniform over the grid
      if (grid_last_block(g.fin.tickets + bx, (unsigned)g.fin.row_tiles)) bn_finalize_cols<BN, NTHR>(g, n0, lds);
    }
  }
}

template <int BM, int BN, int WM, int WN, int BK, bool A_KC, bool B_KC, bool PRO, bool DB, int KW = 1>
__global__ __launch_bounds__(WM * WN * KW * 64) void gemm_tile_kernel(GemmArgs g) {
  ESC_PRIO();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  gemm_tile_body<BM, BN, WM, WN, BK, A_KC, B_KC, PRO, DB, KW>(g, lds, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Backward of one Linear in ONE launch: the first gx workgroups compute dX = dY*W tiles, the rest the
// split-M dW = dY^T*act(X) slabs.  Both stream the same dY; fusing them removes a launch boundary and lets
// the two under-filled grids of the node-sized layers (152 + 304 workgroups) share the chip.
struct DualArgs { GemmArgs dx; GemmArgs dw; int dx_nx, dx_ny, dw_nx, dw_ny, dw_nz; };
template <int BM, int BN, int WM, int WN, int BK, bool PRO>
__global__ __launch_bounds__(WM * WN * 64) void gemm_bwd_dual_kernel(DualArgs a) {
  ESC_PRIO();
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int b = blockIdx.x;
  const int n_dx = a.dx_nx * a.dx_ny;
  if (b < n_dx) {
    gemm_tile_body<BM, BN, WM, WN, BK, true, false, false, false>(a.dx, lds, b % a.dx_nx, b / a.dx_nx, 0);
  } else {
    const int r = b - n_dx;
    const int per = a.dw_nx * a.dw_ny;
    gemm_tile_body<BM, BN, WM, WN, BK, false, false, PRO, true>(a.dw, lds, (r % per) % a.dw_nx, (r % per) / a.dw_nx, r / per);
  }
}

// every weight gradient of a training step reduced in ONE launch (the slabs are only needed by the optimiser):
// block b belongs to the job whose [block_start, block_start+blocks) range contains it
struct ReduceJobs {
  esc_reduce_job job[ESC_MAX_REDUCE_JOBS];
  int block_start[ESC_MAX_REDUCE_JOBS + 1];
  unsigned char vec[ESC_MAX_REDUCE_JOBS];     // 1: four consecutive gradient elements per thread (float4 slab reads)
  int count;
};
// One workgroup owns 64 consecutive UNITS of a job (a unit = four consecutive gradient elements when the job allows float4
// reads, one element otherwise; bias-gradient rows are further units); its four waves each add a quarter of the slabs
// in split order — batches of 8 reads in flight, a short last batch padded by clamping the slab index and masking the
// term, so that no wave ever walks a tail of dependent single loads — and wave 0 adds the four shares in wave order: a
// fixed association, bitwise reproducible.  (One thread per unit walking all 60-75 slabs left the launch latency-bound:
// 17 us for one edge-sized gradient, 20 us for the three 10-wide ones.)
template <int VEC>
__device__ __forceinline__ void slab_sum(const float* __restrict__ base, int64_t stride, int k0, int k1, int64_t off, bool live,
                                         float (&s)[VEC]) {
#pragma unroll
  for (int t = 0; t < VEC; ++t) s[t] = 0.f;
  if (!live) return;
  for (int k = k0; k < k1; k += 8) {
    float v[8][VEC];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int kk = min(k + u, k1 - 1);
      const float* p = base + (size_t)kk * stride + off;
      if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[u][0] = q.x; v[u][1] = q.y; v[u][2] = q.z; v[u][3] = q.w;
      } else {
        v[u][0] = *p;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (k + u < k1) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) s[t] += v[u][t];
      }
  }
}

__global__ __launch_bounds__(256) void slab_reduce_multi_kernel(ReduceJobs t) {
  ESC_PRIO();
  __shared__ float part[3][64][4];
  int j = 0;
  while (j + 1 < t.count && (int)blockIdx.x >= t.block_start[j + 1]) ++j;
  const esc_reduce_job& q = t.job[j];
  const int blk = (int)blockIdx.x - t.block_start[j];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int per = (q.splits + 3) / 4;
  const int k0 = min(q.splits, w * per), k1 = min(q.splits, k0 + per);
  const bool vec = t.vec[j] != 0;
  const int64_t units = vec ? q.n / 4 : q.n;
  const int64_t nblk = (units + 63) / 64;                   // blocks that cover the weight gradient; bias rows follow
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  const bool bias = blk >= nblk;
  const int64_t i = bias ? (int64_t)(blk - nblk) * 64 + lane : (int64_t)blk * 64 + lane;
  const bool live = bias ? (q.db != nullptr && i < q.rows) : i < units;
  if (bias) {
    float o[1];
    slab_sum<1>(q.db_part, q.rows, k0, k1, i, live, o);
    s[0] = o[0];
  } else if (vec) {
    slab_sum<4>(q.slabs, q.n, k0, k1, 4 * i, live, s);
  } else {
    float o[1];
    slab_sum<1>(q.slabs, q.n, k0, k1, i, live, o);
    s[0] = o[0];
  }
  if (w > 0) { part[w - 1][lane][0] = s[0]; part[w - 1][lane][1] = s[1]; part[w - 1][lane][2] = s[2]; part[w - 1][lane][3] = s[3]; }
  __syncthreads();
  if (w != 0 || !live) return;
#pragma unroll
  for (int p = 0; p < 3; ++p) { s[0] += part[p][lane][0]; s[1] += part[p][lane][1]; s[2] += part[p][lane][2]; s[3] += part[p][lane][3]; }
  if (bias) {
    q.db[i] = s[0];
  } else if (vec) {
    const int64_t e = 4 * i;
    *reinterpret_cast<float4*>(q.dw + (e / q.cols) * q.ld_dw + (e % q.cols)) = make_float4(s[0], s[1], s[2], s[3]);
  } else {
    q.dw[(i / q.cols) * q.ld_dw + (i % q.cols)] = s[0];
  }
}

template <int BM, int BN, int WM, int WN, int BK, bool A_KC, bool B_KC, bool PRO, bool DB, int KW = 1>
static void launch_tile(const GemmArgs& g, int splits, hipStream_t s) {
  constexpr int NTHR = WM * WN * KW * 64;
  using ATile = typename std::conditional<A_KC, KContigTile<BM, BK, NTHR>, RedMajorTile<BM, BK, NTHR>>::type;
  using BTile = typename std::conditional<B_KC, KContigTile<BN, BK, NTHR>, RedMajorTile<BN, BK, NTHR>>::type;
  constexpr size_t lds_stage = 2 * (ATile::FLOATS + BTile::FLOATS) * sizeof(float);
  constexpr size_t lds_red = (size_t)WM * WN * (KW - 1) * (BM / WM / 32) * (BN / WN / 32) * 16 * 64 * sizeof(float);
  constexpr size_t lds = lds_stage > lds_red ? lds_stage : lds_red;
  static_assert(lds <= 160 * 1024, "tile does not fit the 160 KiB LDS");
  auto kern = gemm_tile_kernel<BM, BN, WM, WN, BK, A_KC, B_KC, PRO, DB, KW>;
  if (lds > 64 * 1024) {
    static bool raised = false;          // per instantiation
    if (!raised) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); raised = true; }
  }
  dim3 grid((unsigned)cdiv(g.colsC, BN), (unsigned)cdiv(g.rowsC, BM), (unsigned)splits);
  const size_t floor_ = (size_t)gemm_lds_floor();
  const size_t use = lds > floor_ ? lds : floor_;
  if (use > 64 * 1024 && use > lds) {
    static size_t raised_to = 0;     // per instantiation
    if (use > raised_to) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)use); raised_to = use; }
  }
  esc::launch(ESC_K_LINEAR, kern, grid, dim3(NTHR), use, s, g);
}

template <int BM, int BN, int WM, int WN, int BK, bool PRO>
static void launch_dual(const DualArgs& a, hipStream_t s) {
  constexpr int NTHR = WM * WN * 64;
  constexpr size_t lds = 2 * (size_t)(KContigTile<BM, BK, NTHR>::FLOATS + RedMajorTile<BN, BK, NTHR>::FLOATS) * sizeof(float);
  constexpr size_t lds2 = 2 * (size_t)(RedMajorTile<BM, BK, NTHR>::FLOATS + RedMajorTile<BN, BK, NTHR>::FLOATS) * sizeof(float);
  constexpr size_t need = lds > lds2 ? lds : lds2;
  auto kern = gemm_bwd_dual_kernel<BM, BN, WM, WN, BK, PRO>;
  if (need > 64 * 1024) {
    static bool raised = false;
    if (!raised) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need); raised = true; }
  }
  const unsigned blocks = (unsigned)(a.dx_nx * a.dx_ny + a.dw_nx * a.dw_ny * a.dw_nz);
  const size_t floor_ = (size_t)gemm_lds_floor();        // occupancy cap requested by the caller (see common.h)
  const size_t use = need > floor_ ? need : floor_;
  if (use > 64 * 1024 && use > need) {
    static size_t raised_to = 0;
    if (use > raised_to) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)use); raised_to = use; }
  }
  esc::launch(ESC_K_LINEAR, kern, dim3(blocks), dim3(NTHR), use, s, a);
}

}  // namespace esc
