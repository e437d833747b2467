// gineplus.hip — the GINE+ multi-hop aggregate (reference modules/gine_operations.py:306-362, what GINEPLUS / NAIVEGINEPLUS
// compute before self.nn) in ONE launch per direction, k <= 4:
//
//   forward   out[i] = (1+eps[0]) x_0[i] + sum_{d=1..k} (1+eps[d]) * sum_{j : d(j->i) = d} relu(x_{d-1}[j] + [d=1] e[rank(j,i)])
//   backward  dx_t[j] = [t=0] (1+eps[0]) g[j] + sum_{i : d(j->i) = t+1} (1+eps[t+1]) g[i] * 1[x_t[j] + [t=0] e > 0]
//             d_e[m]  = (1+eps[1]) g[dst_m] * 1[x_0[src_m] + e_m > 0]
//             d_eps[d] = sum_i g[i] * (inner sum of distance d)          (d_eps[0] = sum_i g[i] x_0[i])
//
// The per-distance path runs k esc_gine_aggregate launches (csrc/aggregate.hip) and about 2k elementwise torch kernels in each
// direction.  Here one wave owns one destination row (forward) or one source row (backward) and walks ALL its multi-hop pairs,
// which csrc/multihop.hip left grouped both ways with (row, col, distance, rank) per pair: no mask, no atomics.
//
// Bitwise contract with the per-distance path: inside a destination the pairs come in ascending source order, so the pairs of
// one distance are met in the order of that distance's own plan; every sum uses separately rounded adds and the outer sum runs
// in ascending d, as the elementwise kernels do.  The backward adds (1+eps[d]) * g[i] per pair, not (1+eps[d]) * sum g[i]: that
// is what autograd hands the per-distance aggregate.  This file is compiled with -ffp-contract=off (see Makefile).  d_eps is the
// exception: it is regrouped by SOURCE (for d >= 2 the message does not depend on the destination, so d_eps[d] = sum_j
// relu(x_{d-1}[j]) * sum_i g[i]) and reduced per workgroup and then across workgroups in a fixed order: equal up to rounding,
// bit-stable from run to run.
#include "common.h"
#include "row_walk.h"
#include "sparse_plan.h"
#include "../../include/escgnn_gineplus.h"

namespace esc {

constexpr int GP_K_MAX = 4;
constexpr int GP_FWD_BATCH = 8;         // forward: 2 row reads per pair, 16 rows in flight per wave (as AGG_BATCH)
constexpr int GP_BWD_BATCH = 4;         // ... backward: twice the live accumulators
constexpr int GP_BWD_WAVES = 8;         // waves per workgroup of the backward: their d_eps partials are added in LDS
static_assert(GP_K_MAX == sparse::GP_K_MAX && GP_BWD_WAVES == sparse::GP_BWD_WAVES, "sparse_plan.h sizes the backward's grid by these");

struct GpArgs {
  const float* x0; const float* x1; const float* x2; const float* x3;
  int64_t ld0, ld1, ld2, ld3;
  const float* e; int64_t ld_e;
  const float* g; int64_t ld_g;
  const int* in_ptr; const int64_t* out_ptr; const int* meta;
  const float* eps;
  int N, C, k;
  int64_t M1;
  float* out; int64_t ld_out;
  float* dx; float* d_e; float* deps_part;
};

// the row of x_{d-1} that a pair of distance d reads (d wave-uniform, 1..k)
__device__ __forceinline__ const float* gp_row(const GpArgs& a, int d, int s) {
  return d == 1 ? a.x0 + (size_t)s * a.ld0 : d == 2 ? a.x1 + (size_t)s * a.ld1 : d == 3 ? a.x2 + (size_t)s * a.ld2 : a.x3 + (size_t)s * a.ld3;
}

// ---- forward: one wave per destination row ---------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(256) void gp_fwd_wave(GpArgs a) {
  ESC_PRIO();
  const int node = uniform((int)((blockIdx.x * (unsigned)blockDim.x + threadIdx.x) >> 6));
  if (node >= a.N) return;
  const int lane = lane_id();
  const int beg = uniform(a.in_ptr[node]);
  const int end = uniform(a.in_ptr[node + 1]);
  const int C = a.C, k = a.k;
  for (int c = lane * VEC; c < C; c += WAVE * VEC) {
    float acc[GP_K_MAX][VEC], self[VEC];
#pragma unroll
    for (int d = 0; d < GP_K_MAX; ++d)
#pragma unroll
      for (int t = 0; t < VEC; ++t) acc[d][t] = 0.f;
    row_load<VEC>(a.x0 + (size_t)node * a.ld0 + c, self);
    float xv[GP_FWD_BATCH][VEC], ev[GP_FWD_BATCH][VEC];
    int dd[GP_FWD_BATCH];
    segment_batches<GP_FWD_BATCH, false>(beg, end, [&](int u, int jj, bool live) {
      const int4 m = *reinterpret_cast<const int4*>(a.meta + 4 * (size_t)jj);
      const int s = min(max(uniform(m.x), 0), a.N - 1);
      const int d = uniform(m.z), rk = uniform(m.w);
      dd[u] = (live && d >= 1 && d <= k) ? d : 0;           // distance 0 is the self term, read above
      const int dsel = dd[u] ? d : 1;
      row_load<VEC>(gp_row(a, dsel, s) + c, xv[u]);
      if (dd[u] == 1 && rk >= 0 && rk < a.M1) row_load<VEC>(a.e + (size_t)rk * a.ld_e + c, ev[u]);
      else {
#pragma unroll
        for (int t = 0; t < VEC; ++t) ev[u][t] = 0.f;
      }
    }, [&](int u) {
      const int d = dd[u];                                  // wave-uniform: ascending-source order is kept inside every distance
      if (d == 1) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) acc[0][t] = __fadd_rn(acc[0][t], fmaxf(__fadd_rn(xv[u][t], ev[u][t]), 0.f));
      } else if (d == 2) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) acc[1][t] = __fadd_rn(acc[1][t], fmaxf(xv[u][t], 0.f));
      } else if (d == 3) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) acc[2][t] = __fadd_rn(acc[2][t], fmaxf(xv[u][t], 0.f));
      } else if (d == 4) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) acc[3][t] = __fadd_rn(acc[3][t], fmaxf(xv[u][t], 0.f));
      }
    });
    float res[VEC], ep[VEC];
    row_load<VEC>(a.eps + c, ep);
#pragma unroll
    for (int t = 0; t < VEC; ++t) res[t] = __fmul_rn(__fadd_rn(1.0f, ep[t]), self[t]);
#pragma unroll
    for (int d = 0; d < GP_K_MAX; ++d) {
      if (d < k) {
        row_load<VEC>(a.eps + (size_t)(d + 1) * C + c, ep);
#pragma unroll
        for (int t = 0; t < VEC; ++t) res[t] = __fadd_rn(res[t], __fmul_rn(__fadd_rn(1.0f, ep[t]), acc[d][t]));
      }
    }
    row_store<VEC>(a.out + (size_t)node * a.ld_out + c, res);
  }
}

// ---- backward: one wave per SOURCE row, rows wave, wave + W, ... ---------------------------------------------------------------
// every pair has one source, so a distance-1 pair's row of d_e and every row of dx_t are written exactly once
template <int VEC>
__global__ __launch_bounds__(GP_BWD_WAVES * 64) void gp_bwd_wave(GpArgs a) {
  ESC_PRIO();
  __shared__ float red[GP_BWD_WAVES][WAVE * VEC];
  const int lane = lane_id(), w = threadIdx.x >> 6;
  const int W = gridDim.x * GP_BWD_WAVES, gw = blockIdx.x * GP_BWD_WAVES + w;
  const int C = a.C, k = a.k, N = a.N;
  const size_t plane = (size_t)N * C;
  for (int cb = 0; cb < C; cb += WAVE * VEC) {              // workgroup-uniform: the barriers below are met by every wave
    const int c = cb + lane * VEC;
    const bool on = c < C;
    float dep[GP_K_MAX + 1][VEC], ope[GP_K_MAX + 1][VEC];
#pragma unroll
    for (int d = 0; d <= GP_K_MAX; ++d)
#pragma unroll
      for (int t = 0; t < VEC; ++t) { dep[d][t] = 0.f; ope[d][t] = 0.f; }
    if (on) {
#pragma unroll
      for (int d = 0; d <= GP_K_MAX; ++d) {
        if (d <= k) {
          float ep[VEC];
          row_load<VEC>(a.eps + (size_t)d * C + c, ep);
#pragma unroll
          for (int t = 0; t < VEC; ++t) ope[d][t] = __fadd_rn(1.0f, ep[t]);
        }
      }
      for (int node = gw; node < N; node += W) {
        const int beg = uniform((int)a.out_ptr[node]);
        const int end = uniform((int)a.out_ptr[node + 1]);
        float gi[VEC], xr[GP_K_MAX][VEC], accS[GP_K_MAX][VEC], accU[GP_K_MAX][VEC];
        row_load<VEC>(a.g + (size_t)node * a.ld_g + c, gi);
#pragma unroll
        for (int d = 0; d < GP_K_MAX; ++d) {
#pragma unroll
          for (int t = 0; t < VEC; ++t) { xr[d][t] = 0.f; accS[d][t] = 0.f; accU[d][t] = 0.f; }
          if (d < k) row_load<VEC>(gp_row(a, d + 1, node) + c, xr[d]);
        }
#pragma unroll
        for (int t = 0; t < VEC; ++t) dep[0][t] = fmaf(gi[t], xr[0][t], dep[0][t]);
        float gv[GP_BWD_BATCH][VEC], ev[GP_BWD_BATCH][VEC];
        int dd[GP_BWD_BATCH], rr[GP_BWD_BATCH];
        segment_batches<GP_BWD_BATCH, false>(beg, end, [&](int u, int jj, bool live) {
          const int4 m = *reinterpret_cast<const int4*>(a.meta + 4 * (size_t)jj);
          const int i = min(max(uniform(m.y), 0), N - 1);
          const int d = uniform(m.z), rk = uniform(m.w);
          dd[u] = (live && d >= 1 && d <= k) ? d : 0;
          rr[u] = (dd[u] == 1 && rk >= 0 && rk < a.M1) ? rk : -1;
          row_load<VEC>(a.g + (size_t)i * a.ld_g + c, gv[u]);
          if (rr[u] >= 0) row_load<VEC>(a.e + (size_t)rr[u] * a.ld_e + c, ev[u]);
          else {
#pragma unroll
            for (int t = 0; t < VEC; ++t) ev[u][t] = 0.f;
          }
        }, [&](int u) {
          const int d = dd[u];
          if (d == 1) {
            float o[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
              const float msg = __fadd_rn(xr[0][t], ev[u][t]);
              o[t] = msg > 0.f ? __fmul_rn(gv[u][t], ope[1][t]) : 0.f;
              accS[0][t] = __fadd_rn(accS[0][t], o[t]);
              dep[1][t] = fmaf(gv[u][t], fmaxf(msg, 0.f), dep[1][t]);
            }
            if (a.d_e != nullptr && rr[u] >= 0) row_store<VEC>(a.d_e + (size_t)rr[u] * C + c, o);
          } else if (d == 2) {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
              accS[1][t] = __fadd_rn(accS[1][t], xr[1][t] > 0.f ? __fmul_rn(gv[u][t], ope[2][t]) : 0.f);
              accU[1][t] += gv[u][t];
            }
          } else if (d == 3) {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
              accS[2][t] = __fadd_rn(accS[2][t], xr[2][t] > 0.f ? __fmul_rn(gv[u][t], ope[3][t]) : 0.f);
              accU[2][t] += gv[u][t];
            }
          } else if (d == 4) {
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
              accS[3][t] = __fadd_rn(accS[3][t], xr[3][t] > 0.f ? __fmul_rn(gv[u][t], ope[4][t]) : 0.f);
              accU[3][t] += gv[u][t];
            }
          }
        });
        if (a.dx != nullptr) {
          float o[VEC];
#pragma unroll
          for (int t = 0; t < VEC; ++t) o[t] = __fadd_rn(__fmul_rn(gi[t], ope[0][t]), accS[0][t]);
          row_store<VEC>(a.dx + (size_t)node * C + c, o);
#pragma unroll
          for (int d = 1; d < GP_K_MAX; ++d) {
            if (d < k) row_store<VEC>(a.dx + (size_t)d * plane + (size_t)node * C + c, accS[d]);
          }
        }
#pragma unroll
        for (int d = 1; d < GP_K_MAX; ++d)
#pragma unroll
          for (int t = 0; t < VEC; ++t) dep[d + 1][t] = fmaf(fmaxf(xr[d][t], 0.f), accU[d][t], dep[d + 1][t]);
      }
    }
    if (a.deps_part != nullptr) {                           // the waves of the workgroup, added in wave order
#pragma unroll
      for (int d = 0; d <= GP_K_MAX; ++d) {
        if (d <= k) {
#pragma unroll
          for (int t = 0; t < VEC; ++t) red[w][lane * VEC + t] = dep[d][t];
          __syncthreads();
          const int col = cb + (int)threadIdx.x;
          if (threadIdx.x < WAVE * VEC && col < C) {
            float s = red[0][threadIdx.x];
#pragma unroll
            for (int v = 1; v < GP_BWD_WAVES; ++v) s += red[v][threadIdx.x];
            a.deps_part[(size_t)blockIdx.x * (k + 1) * C + (size_t)d * C + col] = s;
          }
          __syncthreads();
        }
      }
    }
  }
}

// d_eps[q] = sum over the workgroups' partials, q in [0, (k+1)*C): four groups of 64 columns take every fourth partial row in
// ascending order, then the groups are added in order: a fixed tree
__global__ __launch_bounds__(256) void gp_deps_reduce(const float* __restrict__ part, int P, int Q, float* __restrict__ d_eps) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int q = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (q < Q) {
    for (int p0 = grp; p0 < P; p0 += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int p = p0 + 4 * u; v[u] = p < P ? part[(size_t)p * Q + q] : 0.f; }
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
  }
  red[grp][lane] = s;
  __syncthreads();
  if (grp == 0 && q < Q) d_eps[q] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}

// the operands both directions share, as the kernels are handed them (x_d for d > k: x0 again)
static inline sparse::GpOps gp_ops(const GpArgs& a) {
  return sparse::GpOps{sparse::mat(a.x0, a.ld0), sparse::mat(a.x1, a.ld1), sparse::mat(a.x2, a.ld2), sparse::mat(a.x3, a.ld3), sparse::mat(a.e, a.ld_e), a.eps};
}

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_gineplus_bwd_blocks(int64_t N) { return sparse::gp_bwd_blocks(N); }

int esc_gineplus_aggregate_fwd(const float* x0, int64_t ld0, const float* x1, int64_t ld1, const float* x2, int64_t ld2,
                               const float* x3, int64_t ld3, const float* e, int64_t ld_e, const int32_t* in_ptr,
                               const int32_t* in_meta, const float* eps, int64_t N, int64_t C, int k, int64_t M1, float* out,
                               int64_t ld_out, void* stream) {
  ESC_REQUIRE(k >= 1 && k <= GP_K_MAX, "esc_gineplus_aggregate_fwd: k=%d outside 1..%d", k, GP_K_MAX);
  ESC_REQUIRE(x0 && in_ptr && eps && out, "esc_gineplus_aggregate_fwd: null pointer");
  ESC_REQUIRE((k < 2 || x1) && (k < 3 || x2) && (k < 4 || x3), "esc_gineplus_aggregate_fwd: fewer than k=%d rows of x", k);
  ESC_REQUIRE(N >= 0 && C > 0 && M1 >= 0 && ld0 >= C && (k < 2 || ld1 >= C) && (k < 3 || ld2 >= C) && (k < 4 || ld3 >= C) &&
              (M1 == 0 || (e && ld_e >= C)) && ld_out >= C, "esc_gineplus_aggregate_fwd: bad sizes N=%ld C=%ld", (long)N, (long)C);
  ESC_REQUIRE(N < (1LL << 31) / 64 && M1 < (1LL << 31), "esc_gineplus_aggregate_fwd: N too large");
  ESC_REQUIRE(in_meta == nullptr || aligned16(in_meta), "esc_gineplus_aggregate_fwd: meta must be 16-byte aligned");
  if (N == 0) return ESC_OK;
  GpArgs a{};
  a.x0 = x0; a.x1 = k >= 2 ? x1 : x0; a.x2 = k >= 3 ? x2 : x0; a.x3 = k >= 4 ? x3 : x0;
  a.ld0 = ld0; a.ld1 = k >= 2 ? ld1 : ld0; a.ld2 = k >= 3 ? ld2 : ld0; a.ld3 = k >= 4 ? ld3 : ld0;
  a.e = e; a.ld_e = ld_e; a.in_ptr = in_ptr; a.meta = in_meta; a.eps = eps; a.N = (int)N; a.C = (int)C; a.k = k; a.M1 = e ? M1 : 0;
  a.out = out; a.ld_out = ld_out;
  const sparse::Plan p = sparse::plan_gineplus_fwd(gp_ops(a), sparse::mat(out, ld_out), N, C);
  esc::launch(ESC_K_AGG_FWD, p.family == sparse::F_V4 ? gp_fwd_wave<4> : gp_fwd_wave<1>, dim3(p.grid[0].x), dim3(256), 0, (hipStream_t)stream, a);
  ESC_CHECK_LAUNCH("esc_gineplus_aggregate_fwd");
  return ESC_OK;
}

int esc_gineplus_aggregate_bwd(const float* x0, int64_t ld0, const float* x1, int64_t ld1, const float* x2, int64_t ld2,
                               const float* x3, int64_t ld3, const float* e, int64_t ld_e, const float* g, int64_t ld_g,
                               const int64_t* out_ptr, const int32_t* meta, const float* eps, int64_t N, int64_t C, int k,
                               int64_t M1, float* dx, float* d_e, float* deps_part, float* d_eps, void* stream) {
  ESC_REQUIRE(k >= 1 && k <= GP_K_MAX, "esc_gineplus_aggregate_bwd: k=%d outside 1..%d", k, GP_K_MAX);
  ESC_REQUIRE(x0 && g && out_ptr && eps, "esc_gineplus_aggregate_bwd: null pointer");
  ESC_REQUIRE((k < 2 || x1) && (k < 3 || x2) && (k < 4 || x3), "esc_gineplus_aggregate_bwd: fewer than k=%d rows of x", k);
  ESC_REQUIRE(N >= 0 && C > 0 && M1 >= 0 && ld0 >= C && (k < 2 || ld1 >= C) && (k < 3 || ld2 >= C) && (k < 4 || ld3 >= C) &&
              (M1 == 0 || (e && ld_e >= C)) && ld_g >= C, "esc_gineplus_aggregate_bwd: bad sizes N=%ld C=%ld", (long)N, (long)C);
  ESC_REQUIRE(N < (1LL << 31) / 64 && M1 < (1LL << 31), "esc_gineplus_aggregate_bwd: N too large");
  ESC_REQUIRE((deps_part == nullptr) == (d_eps == nullptr), "esc_gineplus_aggregate_bwd: deps_part and d_eps go together");
  ESC_REQUIRE(meta == nullptr || aligned16(meta), "esc_gineplus_aggregate_bwd: meta must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (N == 0) {
    if (d_eps && hipMemsetAsync(d_eps, 0, (size_t)(k + 1) * C * sizeof(float), s) != hipSuccess) {
      set_error("esc_gineplus_aggregate_bwd: memset failed");
      return ESC_ELAUNCH;
    }
    return ESC_OK;
  }
  GpArgs a{};
  a.x0 = x0; a.x1 = k >= 2 ? x1 : x0; a.x2 = k >= 3 ? x2 : x0; a.x3 = k >= 4 ? x3 : x0;
  a.ld0 = ld0; a.ld1 = k >= 2 ? ld1 : ld0; a.ld2 = k >= 3 ? ld2 : ld0; a.ld3 = k >= 4 ? ld3 : ld0;
  a.e = e; a.ld_e = ld_e; a.g = g; a.ld_g = ld_g; a.out_ptr = out_ptr; a.meta = meta; a.eps = eps; a.N = (int)N; a.C = (int)C; a.k = k;
  a.M1 = e ? M1 : 0; a.dx = dx; a.d_e = d_e; a.deps_part = deps_part;
  const sparse::Plan p = sparse::plan_gineplus_bwd(gp_ops(a), sparse::mat(g, ld_g), sparse::mat(dx, C), sparse::mat(d_e, C), N, C, k, d_eps != nullptr);
  esc::launch(ESC_K_AGG_BWD, p.family == sparse::F_V4 ? gp_bwd_wave<4> : gp_bwd_wave<1>, dim3(p.grid[0].x), dim3(GP_BWD_WAVES * 64), 0, s, a);
  ESC_CHECK_LAUNCH("esc_gineplus_aggregate_bwd");
  if (p.launches == 2) {
    esc::launch(-1, gp_deps_reduce, dim3(p.grid[1].x), dim3(256), 0, s, (const float*)deps_part, (int)p.slots, (int)((k + 1) * C), d_eps);
    ESC_CHECK_LAUNCH("esc_gineplus_aggregate_bwd.deps");
  }
  return ESC_OK;
}

}  // extern "C"
