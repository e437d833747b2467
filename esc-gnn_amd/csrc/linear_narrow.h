// linear_narrow.h — Linear layers with a narrow output (N <= 4: the H -> 1 head) or a short reduction (dX of an N <= 16 layer),
// and the col_stats pass over a finished Y.  linear_mfma.hip decides when they run (linear_plan.h).
#pragma once
#include "common.h"
#include "linear_plan.h"

namespace esc {

// (mean, M2) of every output column over R-row blocks of a finished Y: the col_stats contract for the one shape class whose GEMM
// cannot write its partials at the block height esc_linear_stats_block_rows has promised (see linear_fwd_impl)
__global__ __launch_bounds__(256) void col_stats_rows_kernel(const float* __restrict__ Y, int64_t ldy, int M, int N, int R,
                                                             float2* __restrict__ col_stats) {
  const int n = blockIdx.y * 256 + threadIdx.x;
  if (n >= N) return;
  const int r0 = blockIdx.x * R, rows = min(R, M - r0);
  float s1 = 0.f;
  for (int r = 0; r < rows; ++r) s1 += Y[(size_t)(r0 + r) * ldy + n];
  const float mean = s1 / (float)rows;
  float m2 = 0.f;
  for (int r = 0; r < rows; ++r) { const float d = Y[(size_t)(r0 + r) * ldy + n] - mean; m2 = fmaf(d, d, m2); }
  col_stats[(size_t)blockIdx.x * N + n] = make_float2(mean, m2);
}

// =================================================================================================
// Narrow-output linears (N <= 4 output features, K <= 256): lin2 (H -> 1).  On the 128x32 MFMA tile this is 19
// workgroups that pad N to 32 and crawl (17 us forward, 19 us backward in two launches vs 5 / 8 us here); they are
// really bandwidth problems — X is read once — so: one wave per row batch, a lane owns one k-quad, the N weight
// rows sit in registers, dot products by wave reduction.  Backward: dX rows and the workgroup's share of dW / db in
// one pass; the shares are summed by the ordinary slab-reduce job (deterministic, one share per 128 rows).
// =================================================================================================

// L1: the H -> 1 prediction head of a training step — the wave that has a node's prediction also leaves d|pred - y| / d pred for it
// (the same expression as l1_loss_kernel), so the backward does not wait for the loss launch
struct NarrowL1 { const float* target; float gs; float* dpred; };
template <int NMAX, bool PRO, bool FOLD = false, bool L1 = false>
__global__ __launch_bounds__(256) void linear_narrow_fwd(const float* __restrict__ X, int64_t ldx,
                                                         const float* __restrict__ W, int64_t ldw,
                                                         const float* __restrict__ bias,
                                                         const float* __restrict__ sc, const float* __restrict__ sh,
                                                         int M, int N, int K, float* __restrict__ Y, int64_t ldy,
                                                         BnFoldDev fold, NarrowL1 l1) {
  ESC_PRIO();
  const int lane = lane_id();
  const int k = lane * 4;
  const bool valid = k < K;
  float4 w[NMAX];
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
    w[n] = (valid && n < N) ? *reinterpret_cast<const float4*>(W + (size_t)n * ldw + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ps = make_float4(1.f, 1.f, 1.f, 1.f), ph = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (PRO && FOLD) {           // the BatchNorm in front of X is still in partial form: merge it here (common.h)
    if (valid) {
      const bool writer = blockIdx.x == 0 && threadIdx.x < 64;
      bn_fold_column(fold, k + 0, writer, ps.x, ph.x); bn_fold_column(fold, k + 1, writer, ps.y, ph.y);
      bn_fold_column(fold, k + 2, writer, ps.z, ph.z); bn_fold_column(fold, k + 3, writer, ps.w, ph.w);
    }
  } else if constexpr (PRO) {
    if (valid) { ps = *reinterpret_cast<const float4*>(sc + k); ph = *reinterpret_cast<const float4*>(sh + k); }
  }
  const float bv = (bias != nullptr && lane < N) ? bias[lane] : 0.f;
  const int stride = gridDim.x * 4;
  for (int r0 = blockIdx.x * 4 + (threadIdx.x >> 6); r0 < M; r0 += 4 * stride) {
    float4 x[4];                                   // 4 rows in flight per wave
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * stride;
      x[u] = (valid && r < M) ? *reinterpret_cast<const float4*>(X + (size_t)r * ldx + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * stride;
      if (r >= M) break;                           // wave-uniform
      float4 v = x[u];
      if constexpr (PRO) {
        v = valid ? make_float4(fmaxf(fmaf(v.x, ps.x, ph.x), 0.f), fmaxf(fmaf(v.y, ps.y, ph.y), 0.f),
                                fmaxf(fmaf(v.z, ps.z, ph.z), 0.f), fmaxf(fmaf(v.w, ps.w, ph.w), 0.f))
                  : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      float mine = 0.f;
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n < N) {                               // wave-uniform
          const float p = wave_sum(v.x * w[n].x + v.y * w[n].y + v.z * w[n].z + v.w * w[n].w);
          mine = (lane == n) ? p : mine;
        }
      }
      if (lane < N) Y[(size_t)r * ldy + lane] = mine + bv;
      if constexpr (L1) {
        if (lane == 0) {
          const float d = (mine + bv) - l1.target[r];
          l1.dpred[r] = d > 0.f ? l1.gs : (d < 0.f ? -l1.gs : 0.f);
        }
      }
    }
  }
}

template <int NMAX, bool PRO>
__global__ __launch_bounds__(256) void linear_narrow_bwd(const float* __restrict__ dY, int64_t lddy,
                                                         const float* __restrict__ X, int64_t ldx,
                                                         const float* __restrict__ W, int64_t ldw,
                                                         const float* __restrict__ sc, const float* __restrict__ sh,
                                                         int M, int N, int K, float* __restrict__ dX, int64_t lddx,
                                                         int accumulate, float* __restrict__ slab,
                                                         float* __restrict__ db_part) {
  ESC_PRIO();
  __shared__ float4 red[3][64];
  __shared__ float redb[3][NMAX];
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  const int k = lane * 4;
  const bool valid = k < K;
  float4 w[NMAX], acc[NMAX];
  float dbacc[NMAX];
#pragma unroll
  for (int n = 0; n < NMAX; ++n) {
    w[n] = (valid && n < N) ? *reinterpret_cast<const float4*>(W + (size_t)n * ldw + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    acc[n] = make_float4(0.f, 0.f, 0.f, 0.f);
    dbacc[n] = 0.f;
  }
  float4 ps = make_float4(1.f, 1.f, 1.f, 1.f), ph = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (PRO) {
    if (valid) { ps = *reinterpret_cast<const float4*>(sc + k); ph = *reinterpret_cast<const float4*>(sh + k); }
  }
  const int row_end = min(M, (int)(blockIdx.x + 1) * NARROW_ROWS);
  for (int r0 = blockIdx.x * NARROW_ROWS + wave; r0 < row_end; r0 += 16) {     // 4 rows in flight per wave
    float4 x[4], old[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * 4;
      const bool live = valid && r < row_end;
      x[u] = live ? *reinterpret_cast<const float4*>(X + (size_t)r * ldx + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      old[u] = (live && dX != nullptr && accumulate) ? *reinterpret_cast<const float4*>(dX + (size_t)r * lddx + k)
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * 4;
      if (r >= row_end) break;                     // wave-uniform
      float4 v = x[u];
      if constexpr (PRO) {
        v = valid ? make_float4(fmaxf(fmaf(v.x, ps.x, ph.x), 0.f), fmaxf(fmaf(v.y, ps.y, ph.y), 0.f),
                                fmaxf(fmaf(v.z, ps.z, ph.z), 0.f), fmaxf(fmaf(v.w, ps.w, ph.w), 0.f))
                  : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      float4 d = old[u];
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n < N) {
          const float g = dY[(size_t)r * lddy + n];              // same address in every lane: one broadcast load
          d.x = fmaf(g, w[n].x, d.x); d.y = fmaf(g, w[n].y, d.y); d.z = fmaf(g, w[n].z, d.z); d.w = fmaf(g, w[n].w, d.w);
          acc[n].x = fmaf(g, v.x, acc[n].x); acc[n].y = fmaf(g, v.y, acc[n].y);
          acc[n].z = fmaf(g, v.z, acc[n].z); acc[n].w = fmaf(g, v.w, acc[n].w);
          dbacc[n] += g;
        }
      }
      if (valid && dX != nullptr) *reinterpret_cast<float4*>(dX + (size_t)r * lddx + k) = d;
    }
  }
  // the four waves' shares, added in wave order, become this workgroup's slab
  float* out = slab + (size_t)blockIdx.x * N * K;
#pragma unroll
  for (int n = 0; n < NMAX; ++n) {
    if (n >= N) break;
    if (wave > 0) red[wave - 1][lane] = acc[n];
    __syncthreads();
    if (wave == 0 && valid) {
      float4 t = acc[n];
#pragma unroll
      for (int q = 0; q < 3; ++q) { const float4 o = red[q][lane]; t.x += o.x; t.y += o.y; t.z += o.z; t.w += o.w; }
      *reinterpret_cast<float4*>(out + (size_t)n * K + k) = t;
    }
    __syncthreads();
  }
  if (wave > 0 && lane == 0) {
#pragma unroll
    for (int n = 0; n < NMAX; ++n) redb[wave - 1][n] = dbacc[n];
  }
  __syncthreads();
  if (wave == 0 && lane == 0) {
#pragma unroll
    for (int n = 0; n < NMAX; ++n)
      if (n < N) db_part[(size_t)blockIdx.x * N + n] = ((dbacc[n] + redb[0][n]) + redb[1][n]) + redb[2][n];
  }
}

// dX = dY[M,N] * W[N,K] for a short reduction (N <= 16: conv1.lin's input gradient, 15 200 x 256 from 10 features):
// an outer-product-like, purely bandwidth-bound pass — the MFMA tile pads N to a 32-deep K-step (29 us vs 8 us).
template <int NMAX>
__global__ __launch_bounds__(256) void linear_narrow_dx(const float* __restrict__ dY, int64_t lddy,
                                                        const float* __restrict__ W, int64_t ldw, int M, int N, int K,
                                                        float* __restrict__ dX, int64_t lddx, int accumulate) {
  ESC_PRIO();
  const int lane = lane_id();
  const int k = lane * 4;
  const bool valid = k < K;                                 // (every lane stays: lanes < N carry the dY values of a row)
  float4 w[NMAX];
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
    w[n] = (valid && n < N) ? *reinterpret_cast<const float4*>(W + (size_t)n * ldw + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  const int stride = gridDim.x * 4;
  for (int r0 = blockIdx.x * 4 + (threadIdx.x >> 6); r0 < M; r0 += 4 * stride) {
    float4 d[4];
    float gy[4];                                            // lane n < N holds dY[r, n] of each of the wave's four rows: ONE load per row
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * stride;
      d[u] = (valid && accumulate && r < M) ? *reinterpret_cast<const float4*>(dX + (size_t)r * lddx + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      gy[u] = (r < M && lane < N) ? dY[(size_t)r * lddy + lane] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = r0 + u * stride;
      if (r >= M) break;
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n < N) {
          const float g = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, gy[u]), n));
          d[u].x = fmaf(g, w[n].x, d[u].x); d[u].y = fmaf(g, w[n].y, d[u].y);
          d[u].z = fmaf(g, w[n].z, d[u].z); d[u].w = fmaf(g, w[n].w, d[u].w);
        }
      }
      if (valid) *reinterpret_cast<float4*>(dX + (size_t)r * lddx + k) = d[u];
    }
  }
}

}  // namespace esc
