// i2pool.hip — the two row-wise pieces of the I2GNN baseline's hierarchical pooling that nothing else in the library covers
// (reference zinc_cycle_models.py:200-250):
//   * subgraph2_pooling = 'mean-center-side': out[s] = [mean of the rows of subgraph2 s | x[center[s]] | x[side[s]]] in ONE pass
//     over x instead of a mean pool, two gathers and a concatenation; the backward writes every dx row once from the three
//     parts (no memset, no atomics: a row belongs to exactly one subgraph2 and its centre / side rows lie inside it)
//   * the gate `subgraph_gate[layer](z_emb) * x` = sigmoid(a) * x and its two gradients, sigmoid recomputed from a
// All fp32, bound by memory traffic: one thread per output element, consecutive threads on consecutive columns.
#include <math.h>

#include "common.h"
#include "../../include/escgnn_i2gnn.h"

namespace esc {

__global__ __launch_bounds__(256) void pool_mcs_fwd_kernel(const float* __restrict__ x, int64_t ld_x, const int64_t* __restrict__ ptr,
                                                           const int64_t* __restrict__ center, const int64_t* __restrict__ side,
                                                           int64_t idx_stride, int64_t S, int64_t C, float* __restrict__ out,
                                                           int64_t ld_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= S * C) return;
  const int64_t s = i / C, c = i - s * C;
  const int64_t r0 = ptr[s], r1 = ptr[s + 1];
  float* o = out + s * ld_out + c;
  if (r1 <= r0) { o[0] = 0.f; o[C] = 0.f; o[2 * C] = 0.f; return; }     // an empty segment has neither rows nor a centre
  float acc = 0.f;
  for (int64_t r = r0; r < r1; ++r) acc += x[r * ld_x + c];
  o[0] = acc / (float)(r1 - r0);
  o[C] = x[center[s * idx_stride] * ld_x + c];
  o[2 * C] = x[side[s * idx_stride] * ld_x + c];
}

// dx[row] = dout_mean[s] / len + [row == center[s]] dout_c[s] + [row == side[s]] dout_s[s]; center == side adds both
__global__ __launch_bounds__(256) void pool_mcs_bwd_kernel(const float* __restrict__ dout, int64_t ld_dout,
                                                           const int64_t* __restrict__ ptr, const int64_t* __restrict__ center,
                                                           const int64_t* __restrict__ side, int64_t idx_stride,
                                                           const int64_t* __restrict__ node_to_segment, int64_t N, int64_t C,
                                                           float* __restrict__ dx, int64_t ld_dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int64_t row = i / C, c = i - row * C;
  const int64_t s = node_to_segment[row];
  const float* g = dout + s * ld_dout + c;
  float v = g[0] / (float)(ptr[s + 1] - ptr[s]);
  if (center[s * idx_stride] == row) v += g[C];
  if (side[s * idx_stride] == row) v += g[2 * C];
  dx[row * ld_dx + c] = v;
}

// 1 / (1 + exp(-a)) without an overflowing exponential on either side
__device__ __forceinline__ float sigmoid_stable(float a) {
  const float e = expf(-fabsf(a));
  return a >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

__global__ __launch_bounds__(256) void sigmoid_mul_fwd_kernel(const float* __restrict__ a, int64_t ld_a, const float* __restrict__ x,
                                                              int64_t ld_x, int64_t M, int64_t C, float* __restrict__ y,
                                                              int64_t ld_y) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * C) return;
  const int64_t r = i / C, c = i - r * C;
  y[r * ld_y + c] = sigmoid_stable(a[r * ld_a + c]) * x[r * ld_x + c];
}

__global__ __launch_bounds__(256) void sigmoid_mul_bwd_kernel(const float* __restrict__ a, int64_t ld_a, const float* __restrict__ x,
                                                              int64_t ld_x, const float* __restrict__ dy, int64_t ld_dy, int64_t M,
                                                              int64_t C, float* __restrict__ da, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * C) return;
  const int64_t r = i / C, c = i - r * C;
  // s (1 - s) = e / (1 + e)^2 with e = exp(-|a|): 1 - s itself cancels for large a
  const float av = a[r * ld_a + c], g = dy[r * ld_dy + c];
  const float e = expf(-fabsf(av)), d = 1.f + e;
  if (dx) dx[i] = g * (av >= 0.f ? 1.f / d : e / d);
  if (da) da[i] = g * x[r * ld_x + c] * (e / (d * d));
}

}  // namespace esc

using namespace esc;

extern "C" {

int esc_pool_mean_center_side_fwd(const float* x, int64_t ld_x, const int64_t* ptr, const int64_t* center, const int64_t* side,
                                  int64_t idx_stride, int64_t S, int64_t C, float* out, int64_t ld_out, void* stream) {
  ESC_REQUIRE(S >= 0 && C >= 0 && ld_x >= C && ld_out >= 3 * C && idx_stride >= 1 && S * C < (1LL << 40),
              "esc_pool_mean_center_side_fwd: bad shape");
  if (S * C == 0) return ESC_OK;
  ESC_REQUIRE(x && ptr && center && side && out, "esc_pool_mean_center_side_fwd: null pointer");
  esc::launch(ESC_K_AGG_FWD, pool_mcs_fwd_kernel, dim3((unsigned)cdiv(S * C, 256)), dim3(256), 0, (hipStream_t)stream, x, ld_x, ptr,
              center, side, idx_stride, S, C, out, ld_out);
  ESC_CHECK_LAUNCH("esc_pool_mean_center_side_fwd");
  return ESC_OK;
}

int esc_pool_mean_center_side_bwd(const float* dout, int64_t ld_dout, const int64_t* ptr, const int64_t* center,
                                  const int64_t* side, int64_t idx_stride, const int64_t* node_to_segment, int64_t N, int64_t C,
                                  float* dx, int64_t ld_dx, void* stream) {
  ESC_REQUIRE(N >= 0 && C >= 0 && ld_dout >= 3 * C && ld_dx >= C && idx_stride >= 1 && N * C < (1LL << 40),
              "esc_pool_mean_center_side_bwd: bad shape");
  if (N * C == 0) return ESC_OK;
  ESC_REQUIRE(dout && ptr && center && side && node_to_segment && dx, "esc_pool_mean_center_side_bwd: null pointer");
  esc::launch(ESC_K_AGG_BWD, pool_mcs_bwd_kernel, dim3((unsigned)cdiv(N * C, 256)), dim3(256), 0, (hipStream_t)stream, dout, ld_dout,
              ptr, center, side, idx_stride, node_to_segment, N, C, dx, ld_dx);
  ESC_CHECK_LAUNCH("esc_pool_mean_center_side_bwd");
  return ESC_OK;
}

int esc_sigmoid_mul_fwd(const float* a, int64_t ld_a, const float* x, int64_t ld_x, int64_t M, int64_t C, float* y, int64_t ld_y,
                        void* stream) {
  ESC_REQUIRE(M >= 0 && C >= 0 && ld_a >= C && ld_x >= C && ld_y >= C && M * C < (1LL << 40), "esc_sigmoid_mul_fwd: bad shape");
  if (M * C == 0) return ESC_OK;
  ESC_REQUIRE(a && x && y, "esc_sigmoid_mul_fwd: null pointer");
  esc::launch(ESC_K_AGG_FWD, sigmoid_mul_fwd_kernel, dim3((unsigned)cdiv(M * C, 256)), dim3(256), 0, (hipStream_t)stream, a, ld_a, x,
              ld_x, M, C, y, ld_y);
  ESC_CHECK_LAUNCH("esc_sigmoid_mul_fwd");
  return ESC_OK;
}

int esc_sigmoid_mul_bwd(const float* a, int64_t ld_a, const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t M,
                        int64_t C, float* da, float* dx, void* stream) {
  ESC_REQUIRE(M >= 0 && C >= 0 && ld_a >= C && ld_x >= C && ld_dy >= C && M * C < (1LL << 40), "esc_sigmoid_mul_bwd: bad shape");
  if (M * C == 0) return ESC_OK;
  ESC_REQUIRE(a && x && dy && (da || dx), "esc_sigmoid_mul_bwd: null pointer");
  esc::launch(ESC_K_AGG_BWD, sigmoid_mul_bwd_kernel, dim3((unsigned)cdiv(M * C, 256)), dim3(256), 0, (hipStream_t)stream, a, ld_a, x,
              ld_x, dy, ld_dy, M, C, da, dx);
  ESC_CHECK_LAUNCH("esc_sigmoid_mul_bwd");
  return ESC_OK;
}

}  // extern "C"
