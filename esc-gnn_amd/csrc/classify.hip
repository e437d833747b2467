// classify.hip — the classification head of the expressiveness drivers (run_sr.py:211,241-242, run_exp.py:215,235,248,
// 261-264): row-wise log-softmax, NLL loss with accuracy count, the fused training head, and pairwise distances.
//
// Every row is handled by ONE wave: lanes stride over the C columns, the row maximum, the first argmax and the sums are
// wave reductions (__shfl_xor butterflies, a fixed order), so a result never depends on the grid shape.  The maximum is
// taken off in fp64 before anything is exponentiated ((double)x - (double)max is exact), sums are accumulated in fp64 and
// every output is rounded to fp32 once.  M is a number of graphs (20 .. ~1 200) and C a class count: these kernels are
// about exact, deterministic results in one launch, not about bandwidth.  The only atomic is the ticket of the loss
// kernels' last-workgroup reduction (common.h: grid_last_block); the sums themselves are taken in a fixed order.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace esc {

constexpr int HEAD_WAVES = 16;                 // the loss kernels: 16 waves per workgroup, one row each

// row maximum (value of the FIRST maximal column in `arg`, like tensor.max(1)[1]) and lse = log(sum exp(x - max))
__device__ __forceinline__ void row_max_lse(const float* __restrict__ x, int C, float& mx, int& arg, double& lse) {
  const int lane = lane_id();
  float m = -INFINITY;
  int a = INT_MAX;
  for (int c = lane; c < C; c += WAVE) {
    const float v = x[c];
    if (v > m || a == INT_MAX) { m = v; a = c; }          // strictly greater: the first maximum of this lane's columns
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(a, o, 64);
    if (oa != INT_MAX && (a == INT_MAX || om > m || (om == m && oa < a))) { m = om; a = oa; }
  }
  double s = 0.0;
  for (int c = lane; c < C; c += WAVE) s += exp((double)x[c] - (double)m);
  s = wave_sum(s);
  mx = m;
  arg = a;
  lse = log(s);
}

__device__ __forceinline__ float logp_of(float x, float mx, double lse) { return (float)(((double)x - (double)mx) - lse); }

// first maximal column of a row (no softmax): the accuracy count of esc_nll_loss
__device__ __forceinline__ int row_argmax(const float* __restrict__ x, int C) {
  const int lane = lane_id();
  float m = -INFINITY;
  int a = INT_MAX;
  for (int c = lane; c < C; c += WAVE) {
    const float v = x[c];
    if (v > m || a == INT_MAX) { m = v; a = c; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64);
    const int oa = __shfl_xor(a, o, 64);
    if (oa != INT_MAX && (a == INT_MAX || om > m || (om == m && oa < a))) { m = om; a = oa; }
  }
  return a;
}

__global__ __launch_bounds__(256) void log_softmax_fwd_kernel(const float* __restrict__ x, int64_t ld_x, int M, int C,
                                                              float* __restrict__ y, int64_t ld_y) {
  ESC_PRIO();
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (size_t)row * ld_x;
  float mx; int arg; double lse;
  row_max_lse(xr, C, mx, arg, lse);
  float* yr = y + (size_t)row * ld_y;
  for (int c = lane_id(); c < C; c += WAVE) yr[c] = logp_of(xr[c], mx, lse);
}

// dx = dy - exp(logp) * sum_c dy
__global__ __launch_bounds__(256) void log_softmax_bwd_kernel(const float* __restrict__ logp, int64_t ld_p,
                                                              const float* __restrict__ dy, int64_t ld_dy, int M, int C,
                                                              float* __restrict__ dx, int64_t ld_dx) {
  ESC_PRIO();
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* pr = logp + (size_t)row * ld_p;
  const float* gr = dy + (size_t)row * ld_dy;
  double s = 0.0;
  for (int c = lane_id(); c < C; c += WAVE) s += (double)gr[c];
  s = wave_sum(s);
  float* dr = dx + (size_t)row * ld_dx;
  for (int c = lane_id(); c < C; c += WAVE) dr[c] = (float)((double)gr[c] - exp((double)pr[c]) * s);
}

// The loss kernels: one wave per row (16 rows per workgroup) leaves the row's loss term and its flags in `rows`; the
// workgroup that finishes last (grid_last_block: a ticket, no spinning) adds the terms in an order that depends on M
// alone — thread (wave w, lane l) takes the rows w + 16 l + 1024 k in increasing k (fp64), the lanes are merged by the
// butterfly and the 16 wave partials are added in wave order by thread 0.  esc_nll_loss and esc_log_softmax_nll share this
// code, so the fused head's loss is the two-op loss bit for bit, whatever the grid.
__device__ __forceinline__ void head_publish(float2* __restrict__ rows, int row, float v, int hit, bool ok) {
  if (lane_id() == 0) store_agent(rows + row, make_float2(v, __int_as_float(hit | (ok ? 0 : 2))));
}

__device__ __forceinline__ void head_finish(const float2* __restrict__ rows, int M, double denom, float* __restrict__ loss,
                                            int32_t* __restrict__ correct, int32_t* __restrict__ bad_target) {
  __shared__ double s_loss[HEAD_WAVES];
  __shared__ int s_cnt[HEAD_WAVES], s_bad[HEAD_WAVES];
  const int wave = threadIdx.x >> 6, lane = lane_id();
  double acc = 0.0;
  int cnt = 0, bad = 0;
  for (int i = wave + HEAD_WAVES * lane; i < M; i += HEAD_WAVES * WAVE) {
    const float2 r = rows[i];
    const int bits = __float_as_int(r.y);
    acc += (double)r.x;
    cnt += bits & 1;
    bad |= bits >> 1;
  }
  acc = wave_sum(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); bad |= __shfl_xor(bad, o, 64); }
  if (lane == 0) { s_loss[wave] = acc; s_cnt[wave] = cnt; s_bad[wave] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    int c = 0, b = 0;
    for (int w = 0; w < HEAD_WAVES; ++w) { t += s_loss[w]; c += s_cnt[w]; b |= s_bad[w]; }
    loss[0] = (float)(t / denom);
    if (correct) correct[0] = c;
    bad_target[0] = b & 1;
  }
}

__global__ __launch_bounds__(HEAD_WAVES * 64) void nll_loss_kernel(const float* __restrict__ logp, int64_t ld_p,
                                                                   const int64_t* __restrict__ target, int M, int C, double denom,
                                                                   double grad, float* __restrict__ loss,
                                                                   float* __restrict__ dlogp, int64_t ld_d,
                                                                   int32_t* __restrict__ correct, int32_t* __restrict__ bad_target,
                                                                   float2* __restrict__ rows, unsigned* __restrict__ ticket) {
  ESC_PRIO();
  const int row = blockIdx.x * HEAD_WAVES + (threadIdx.x >> 6), lane = lane_id();
  if (row < M) {
    const float* pr = logp + (size_t)row * ld_p;
    const int64_t t = target[row];
    const bool ok = t >= 0 && t < C;
    const float v = ok ? -pr[t] : 0.f;
    int hit = 0;
    if (correct) hit = (ok && row_argmax(pr, C) == (int)t) ? 1 : 0;
    head_publish(rows, row, v, hit, ok);
    if (dlogp) {
      const float dval = (float)(-grad / denom);
      float* dr = dlogp + (size_t)row * ld_d;
      for (int c = lane; c < C; c += WAVE) dr[c] = (ok && c == (int)t) ? dval : 0.f;
    }
  }
  if (!grid_last_block(ticket, gridDim.x)) return;
  head_finish(rows, M, denom, loss, correct, bad_target);
}

// log-softmax + NLL + d loss / d logits = (softmax - onehot) * grad / denom in one launch
__global__ __launch_bounds__(HEAD_WAVES * 64) void log_softmax_nll_kernel(const float* __restrict__ x, int64_t ld_x,
                                                                          const int64_t* __restrict__ target, int M, int C,
                                                                          double denom, double grad, float* __restrict__ logp,
                                                                          int64_t ld_p, float* __restrict__ loss,
                                                                          float* __restrict__ dx, int64_t ld_dx,
                                                                          int32_t* __restrict__ correct,
                                                                          int32_t* __restrict__ bad_target,
                                                                          float2* __restrict__ rows, unsigned* __restrict__ ticket) {
  ESC_PRIO();
  const int row = blockIdx.x * HEAD_WAVES + (threadIdx.x >> 6), lane = lane_id();
  if (row < M) {
    const float* xr = x + (size_t)row * ld_x;
    float mx; int arg; double lse;
    row_max_lse(xr, C, mx, arg, lse);
    const int64_t t = target[row];
    const bool ok = t >= 0 && t < C;
    const float v = ok ? -logp_of(xr[t], mx, lse) : 0.f;          // the value esc_log_softmax_fwd stores at [row, t], negated
    head_publish(rows, row, v, (ok && arg == (int)t) ? 1 : 0, ok);
    if (logp) {
      float* pr = logp + (size_t)row * ld_p;
      for (int c = lane; c < C; c += WAVE) pr[c] = logp_of(xr[c], mx, lse);
    }
    if (dx) {
      const double scale = grad / denom;
      float* dr = dx + (size_t)row * ld_dx;
      for (int c = lane; c < C; c += WAVE) {
        const double p = exp(((double)xr[c] - (double)mx) - lse);
        dr[c] = ok ? (float)((p - (c == (int)t ? 1.0 : 0.0)) * scale) : 0.f;
      }
    }
  }
  if (!grid_last_block(ticket, gridDim.x)) return;
  head_finish(rows, M, denom, loss, correct, bad_target);
}

// ---- pairwise distances --------------------------------------------------------------------------------------------
// out[k] = |x_i - x_j|_2 for i < j in torch.pdist order, k = i*M - i*(i+1)/2 + (j - i - 1).  Difference form: the rows
// of the SR25 run have magnitude 1e5 and true distances of a few units, which |a|^2 + |b|^2 - 2ab loses entirely in fp32;
// (double)a - (double)b is exact and the squares are summed in fp64.  A workgroup takes 16 x 16 row pairs at a time (the
// tile (bi, bj), bi <= bj, of the pair matrix) and stages the two 16-row panels through LDS 64 columns at a time.
constexpr int PD_T = 16, PD_K = 64;

__global__ __launch_bounds__(PD_T * PD_T) void pdist_kernel(const float* __restrict__ x, int64_t ld_x, int M, int C,
                                                            float* __restrict__ out, float threshold, int32_t* __restrict__ below) {
  ESC_PRIO();
  __shared__ float sa[PD_T][PD_K + 1], sb[PD_T][PD_K + 1];
  __shared__ int s_cnt[PD_T * PD_T / 64];
  const int nb = (M + PD_T - 1) / PD_T;
  const int tiles = nb * (nb + 1) / 2;
  const int ti = threadIdx.x / PD_T, tj = threadIdx.x % PD_T;
  int cnt = 0;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    int bi = 0, rest = tile;                                   // tile -> (bi, bj): row bi of the upper triangle holds nb - bi tiles
    while (rest >= nb - bi) { rest -= nb - bi; ++bi; }
    const int bj = bi + rest;
    const int i = bi * PD_T + ti, j = bj * PD_T + tj;
    double acc = 0.0;
    for (int c0 = 0; c0 < C; c0 += PD_K) {
      __syncthreads();
      for (int e = threadIdx.x; e < PD_T * PD_K; e += PD_T * PD_T) {
        const int r = e / PD_K, c = e % PD_K;
        const int ra = bi * PD_T + r, rb = bj * PD_T + r;
        sa[r][c] = (ra < M && c0 + c < C) ? x[(size_t)ra * ld_x + c0 + c] : 0.f;
        sb[r][c] = (rb < M && c0 + c < C) ? x[(size_t)rb * ld_x + c0 + c] : 0.f;
      }
      __syncthreads();
#pragma unroll 8
      for (int c = 0; c < PD_K; ++c) {
        const double d = (double)sa[ti][c] - (double)sb[tj][c];
        acc += d * d;
      }
    }
    if (i < j && j < M) {
      const float d = (float)sqrt(acc);
      out[(int64_t)i * M - (int64_t)i * (i + 1) / 2 + (j - i - 1)] = d;
      cnt += d < threshold ? 1 : 0;
    }
  }
  if (below && gridDim.x == 1) {                               // the whole problem in this workgroup: count here, no second launch
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      int t = 0;
      for (int w = 0; w < PD_T * PD_T / 64; ++w) t += s_cnt[w];
      below[0] = t;
    }
  }
}

// entries of v below the threshold (integer count: any order gives the same result)
__global__ __launch_bounds__(1024) void count_below_kernel(const float* __restrict__ v, int64_t n, float threshold,
                                                           int32_t* __restrict__ below) {
  ESC_PRIO();
  __shared__ int s_cnt[16];
  int cnt = 0;
  for (int64_t k = threadIdx.x; k < n; k += blockDim.x) cnt += v[k] < threshold ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < 16; ++w) t += s_cnt[w];
    below[0] = t;
  }
}

}  // namespace esc

using namespace esc;

extern "C" {

#define ESC_CLASS_MAX_ROWS (1 << 24)
#define ESC_CLASS_MAX_COLS (1 << 20)

int esc_log_softmax_fwd(const float* logits, int64_t ld_x, int64_t M, int64_t C, float* logp, int64_t ld_p, void* stream) {
  ESC_REQUIRE(M >= 0 && M <= ESC_CLASS_MAX_ROWS && C >= 1 && C <= ESC_CLASS_MAX_COLS && ld_x >= C && ld_p >= C,
              "esc_log_softmax_fwd: bad sizes (M=%lld, C=%lld)", (long long)M, (long long)C);
  if (M == 0) return ESC_OK;
  ESC_REQUIRE(logits && logp, "esc_log_softmax_fwd: null pointer");
  esc::launch(-1, log_softmax_fwd_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, logits, ld_x, (int)M,
              (int)C, logp, ld_p);
  ESC_CHECK_LAUNCH("esc_log_softmax_fwd");
  return ESC_OK;
}

int esc_log_softmax_bwd(const float* logp, int64_t ld_p, const float* dlogp, int64_t ld_dy, int64_t M, int64_t C,
                        float* dlogits, int64_t ld_dx, void* stream) {
  ESC_REQUIRE(M >= 0 && M <= ESC_CLASS_MAX_ROWS && C >= 1 && C <= ESC_CLASS_MAX_COLS && ld_p >= C && ld_dy >= C && ld_dx >= C,
              "esc_log_softmax_bwd: bad sizes (M=%lld, C=%lld)", (long long)M, (long long)C);
  if (M == 0) return ESC_OK;
  ESC_REQUIRE(logp && dlogp && dlogits, "esc_log_softmax_bwd: null pointer");
  esc::launch(-1, log_softmax_bwd_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, logp, ld_p, dlogp,
              ld_dy, (int)M, (int)C, dlogits, ld_dx);
  ESC_CHECK_LAUNCH("esc_log_softmax_bwd");
  return ESC_OK;
}

int esc_nll_loss(const float* logp, int64_t ld_p, const int64_t* target, int64_t M, int64_t C, int64_t denom, float grad_scale,
                 float* loss, float* dlogp, int64_t ld_d, int32_t* correct, int32_t* bad_target, float* scratch, void* stream) {
  ESC_REQUIRE(logp && target && loss && bad_target && scratch && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0,
              "esc_nll_loss: null pointer (or scratch not 8-byte aligned)");
  ESC_REQUIRE(M > 0 && M <= ESC_CLASS_MAX_ROWS && C >= 1 && C <= ESC_CLASS_MAX_COLS && ld_p >= C && (!dlogp || ld_d >= C),
              "esc_nll_loss: bad sizes (M=%lld, C=%lld)", (long long)M, (long long)C);
  unsigned* ticket = esc::tickets(1);
  ESC_REQUIRE(ticket, "esc_nll_loss: no ticket counter");
  esc::launch(-1, nll_loss_kernel, dim3((unsigned)cdiv(M, HEAD_WAVES)), dim3(HEAD_WAVES * 64), 0, (hipStream_t)stream, logp, ld_p,
              target, (int)M, (int)C, (double)(denom > 0 ? denom : M), (double)grad_scale, loss, dlogp, ld_d, correct, bad_target,
              reinterpret_cast<float2*>(scratch), ticket);
  ESC_CHECK_LAUNCH("esc_nll_loss");
  return ESC_OK;
}

int esc_log_softmax_nll(const float* logits, int64_t ld_x, const int64_t* target, int64_t M, int64_t C, int64_t denom,
                        float grad_scale, float* logp, int64_t ld_p, float* loss, float* dlogits, int64_t ld_dx,
                        int32_t* correct, int32_t* bad_target, float* scratch, void* stream) {
  ESC_REQUIRE(logits && target && loss && bad_target && scratch && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0,
              "esc_log_softmax_nll: null pointer (or scratch not 8-byte aligned)");
  ESC_REQUIRE(M > 0 && M <= ESC_CLASS_MAX_ROWS && C >= 1 && C <= ESC_CLASS_MAX_COLS && ld_x >= C && (!logp || ld_p >= C) &&
                  (!dlogits || ld_dx >= C),
              "esc_log_softmax_nll: bad sizes (M=%lld, C=%lld)", (long long)M, (long long)C);
  unsigned* ticket = esc::tickets(1);
  ESC_REQUIRE(ticket, "esc_log_softmax_nll: no ticket counter");
  esc::launch(-1, log_softmax_nll_kernel, dim3((unsigned)cdiv(M, HEAD_WAVES)), dim3(HEAD_WAVES * 64), 0, (hipStream_t)stream, logits,
              ld_x, target, (int)M, (int)C, (double)(denom > 0 ? denom : M), (double)grad_scale, logp, ld_p, loss, dlogits, ld_dx,
              correct, bad_target, reinterpret_cast<float2*>(scratch), ticket);
  ESC_CHECK_LAUNCH("esc_log_softmax_nll");
  return ESC_OK;
}

int esc_pdist(const float* x, int64_t ld_x, int64_t M, int64_t C, float* out, float threshold, int32_t* below, void* stream) {
  ESC_REQUIRE(M >= 0 && M <= 32768 && C >= 1 && C <= ESC_CLASS_MAX_COLS && ld_x >= C, "esc_pdist: bad sizes (M=%lld, C=%lld)",
              (long long)M, (long long)C);
  hipStream_t s = (hipStream_t)stream;
  if (M <= 1) {                                                // no pairs: an empty result, the counter is 0
    if (below) esc::launch(-1, count_below_kernel, dim3(1), dim3(1024), 0, s, out, (int64_t)0, threshold, below);
    ESC_CHECK_LAUNCH("esc_pdist");
    return ESC_OK;
  }
  ESC_REQUIRE(x && out, "esc_pdist: null pointer");
  const int64_t nb = cdiv(M, PD_T), tiles = nb * (nb + 1) / 2;
  const bool one = tiles <= 36;                                // M <= 128: one workgroup walks every tile and counts as it goes
  esc::launch(-1, pdist_kernel, dim3(one ? 1u : (unsigned)(tiles < 4096 ? tiles : 4096)), dim3(PD_T * PD_T), 0, s, x, ld_x,
              (int)M, (int)C, out, threshold, below);
  if (below && !one)
    esc::launch(-1, count_below_kernel, dim3(1), dim3(1024), 0, s, out, M * (M - 1) / 2, threshold, below);
  ESC_CHECK_LAUNCH("esc_pdist");
  return ESC_OK;
}

}  // extern "C"
