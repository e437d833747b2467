// pna.hip — the aggregate of the PNA local layer (include/escgnn_pna.h): what PyG's PNAConv does between its
// pre- and its post-layer with aggregators ['mean', 'max', 'sum'] and the identity scaler - a gather of three rows per edge,
// two scatter-adds, a scatter-max and a degree division - as ONE segmented pass over the destination-sorted view of the plan,
// and its backward as one pass over each view.
//
//   forward   m_k = (P[i] + Q[j]) + R[k];  sum_i = sum m_k;  mean_i = sum_i / max(deg_i, 1);  max_i = max m_k, arg_i = its k
//   backward  pass 1 (destination view): d_R[k] = (g_sum_i + g_mean_i / max(deg_i, 1)) + (arg_i == k ? g_max_i : 0);  d_P[i] = sum d_R[k]
//             pass 2 (source view):      d_Q[j] = sum d_R[k]
//
// The maximum starts from the node's first message and is replaced where m > best (or where best is NaN): among equal maxima
// the lowest edge position wins, and all-negative messages keep a negative maximum.  arg replaces a recomputation of the
// messages in the backward: nothing of size [E, C] lives between the two directions.
//
// Work split: gatedgcn.hip's, for its reasons - a group of LG = 16 (C <= 64), 32 (C <= 128) or 64 float4 lanes owns
// a node (pna_plan.h), a wave owns 64 / LG nodes, the groups walk their own edge ranges and a group's sums and comparisons run
// over its node's slots in order.  Edges are consumed in batches of PNA_BATCH with every read of the batch issued before the
// first use; a short tail is padded by clamping the slot to the node's last edge and masking its contribution.
// No atomics; every output element is written once.  Built with -ffp-contract=off (Makefile).
#include "common.h"
#include "graph_wave.h"
#include "pna_plan.h"
#include "../../include/escgnn_pna.h"

namespace esc {

constexpr int PNA_BATCH = 4;              // forward: 2 float4 row reads and 2 index reads per edge, 8 rows in flight per lane

__device__ __forceinline__ void st4i(int* p, int4 v) { *reinterpret_cast<int4*>(p) = v; }
__device__ __forceinline__ int4 ld4i(const int* p) { return *reinterpret_cast<const int4*>(p); }
// the running maximum of one column: m replaces best where it is larger, or where best is a NaN
__device__ __forceinline__ void pna_take(float m, int k, float& best, int& arg) {
  if (m > best || best != best) { best = m; arg = k; }
}

template <int LG>
__global__ __launch_bounds__(256) void pna_fwd_kernel(const float* __restrict__ P, int64_t ld_p, const float* __restrict__ Q, int64_t ld_q,
                                                      const float* __restrict__ R, int64_t ld_r, const int* __restrict__ in_ptr,
                                                      const int* __restrict__ in_edge, const int* __restrict__ in_src, int N, int C,
                                                      float* __restrict__ agg, int64_t ld_agg, int* __restrict__ arg) {
  ESC_PRIO();
  int node, c0;
  if (!group_locate<LG>(N, node, c0)) return;
  const int beg = in_ptr[node], end = in_ptr[node + 1];
  const float cnt = (float)max(end - beg, 1);
  for (int c = c0; c < C; c += LG * 4) {
    const float4 pi = ld4(P + (size_t)node * ld_p + c);
    float4 sum = make_float4(0.f, 0.f, 0.f, 0.f), best = sum;
    int4 ba = make_int4(-1, -1, -1, -1);
    for (int j = beg; j < end; j += PNA_BATCH) {
      float4 q[PNA_BATCH], r[PNA_BATCH];
      int kk[PNA_BATCH];
#pragma unroll
      for (int u = 0; u < PNA_BATCH; ++u) {
        const int jj = min(j + u, end - 1);                   // tail padding: the node's last edge again, masked below
        kk[u] = in_edge[jj];
        const int s = in_src[jj];
        q[u] = ld4(Q + (size_t)s * ld_q + c);
        r[u] = ld4(R + (size_t)kk[u] * ld_r + c);
      }
#pragma unroll
      for (int u = 0; u < PNA_BATCH; ++u) {
        if (j + u < end) {                                    // uniform over the group: ascending edge position
          float4 m;
          m.x = (pi.x + q[u].x) + r[u].x; m.y = (pi.y + q[u].y) + r[u].y;
          m.z = (pi.z + q[u].z) + r[u].z; m.w = (pi.w + q[u].w) + r[u].w;
          sum.x += m.x; sum.y += m.y; sum.z += m.z; sum.w += m.w;
          if (j + u == beg) {                                 // the first message is the first maximum, whatever its sign
            best = m;
            ba = make_int4(kk[u], kk[u], kk[u], kk[u]);
          } else {
            pna_take(m.x, kk[u], best.x, ba.x); pna_take(m.y, kk[u], best.y, ba.y);
            pna_take(m.z, kk[u], best.z, ba.z); pna_take(m.w, kk[u], best.w, ba.w);
          }
        }
      }
    }
    float4 mean;
    mean.x = sum.x / cnt; mean.y = sum.y / cnt; mean.z = sum.z / cnt; mean.w = sum.w / cnt;
    float* row = agg + (size_t)node * ld_agg + c;
    st4(row, mean);
    st4(row + C, best);
    st4(row + 2 * (size_t)C, sum);
    st4i(arg + (size_t)node * C + c, ba);
  }
}

// backward, pass 1: one group per DESTINATION node; no row is gathered, the edge positions alone are read
template <int LG>
__global__ __launch_bounds__(256) void pna_bwd_dst_kernel(const float* __restrict__ g, int64_t ld_g, const int* __restrict__ arg,
                                                          const int* __restrict__ in_ptr, const int* __restrict__ in_edge, int N, int C,
                                                          float* __restrict__ d_R, int64_t ld_dr, float* __restrict__ d_P, int64_t ld_dp) {
  ESC_PRIO();
  int node, c0;
  if (!group_locate<LG>(N, node, c0)) return;
  const int beg = in_ptr[node], end = in_ptr[node + 1];
  const float cnt = (float)max(end - beg, 1);
  for (int c = c0; c < C; c += LG * 4) {
    const float* row = g + (size_t)node * ld_g + c;
    const float4 gmean = ld4(row), gmax = ld4(row + C), gsum = ld4(row + 2 * (size_t)C);
    const int4 a = ld4i(arg + (size_t)node * C + c);
    float4 base, acc = make_float4(0.f, 0.f, 0.f, 0.f);
    base.x = gsum.x + gmean.x / cnt; base.y = gsum.y + gmean.y / cnt;
    base.z = gsum.z + gmean.z / cnt; base.w = gsum.w + gmean.w / cnt;
    for (int j = beg; j < end; j += PNA_BATCH) {
      int kk[PNA_BATCH];
#pragma unroll
      for (int u = 0; u < PNA_BATCH; ++u) kk[u] = in_edge[min(j + u, end - 1)];
#pragma unroll
      for (int u = 0; u < PNA_BATCH; ++u) {
        if (j + u < end) {
          float4 d;
          d.x = base.x + (a.x == kk[u] ? gmax.x : 0.f); d.y = base.y + (a.y == kk[u] ? gmax.y : 0.f);
          d.z = base.z + (a.z == kk[u] ? gmax.z : 0.f); d.w = base.w + (a.w == kk[u] ? gmax.w : 0.f);
          acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
          st4(d_R + (size_t)kk[u] * ld_dr + c, d);
        }
      }
    }
    st4(d_P + (size_t)node * ld_dp + c, acc);
  }
}

// backward, pass 2: one group per SOURCE node; d_R is what pass 1 wrote (the launch boundary orders the two)
template <int LG>
__global__ __launch_bounds__(256) void pna_bwd_src_kernel(const float* __restrict__ d_R, int64_t ld_dr, const int* __restrict__ out_ptr,
                                                          const int* __restrict__ out_edge, int N, int C, float* __restrict__ d_Q,
                                                          int64_t ld_dq) {
  ESC_PRIO();
  int node, c0;
  if (!group_locate<LG>(N, node, c0)) return;
  const int beg = out_ptr[node], end = out_ptr[node + 1];
  for (int c = c0; c < C; c += LG * 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = beg; j < end; j += PNA_BATCH) {
      float4 d[PNA_BATCH];
#pragma unroll
      for (int u = 0; u < PNA_BATCH; ++u) d[u] = ld4(d_R + (size_t)out_edge[min(j + u, end - 1)] * ld_dr + c);
#pragma unroll
      for (int u = 0; u < PNA_BATCH; ++u) {
        if (j + u < end) { acc.x += d[u].x; acc.y += d[u].y; acc.z += d[u].z; acc.w += d[u].w; }
      }
    }
    st4(d_Q + (size_t)node * ld_dq + c, acc);
  }
}

struct PnaLd {
  const char* name;
  int64_t ld, width;
};

// what both entries check before anything is launched; 0 or an error code with the message set
static int pna_limits(const char* fn, int64_t N, int64_t E, int64_t C, const PnaLd* ld, int n_ld, const void* const* p, int n_p) {
  ESC_REQUIRE(C >= 4 && C <= pna::MAX_C && C % 4 == 0, "%s: C=%ld: the width must be a multiple of 4 with 4 <= C <= %ld "
              "(esc_pna_max_channels)", fn, (long)C, (long)pna::MAX_C);
  for (int i = 0; i < n_ld; ++i)
    ESC_REQUIRE(ld[i].ld >= ld[i].width && ld[i].ld % 4 == 0, "%s: leading dimension %s=%ld: it must be >= its row width %ld "
                "(C=%ld) and a multiple of 4", fn, ld[i].name, (long)ld[i].ld, (long)ld[i].width, (long)C);
  for (int i = 0; i < n_p; ++i) ESC_REQUIRE(aligned16(p[i]), "%s: every pointer must be 16-byte aligned", fn);
  ESC_REQUIRE(N >= 0 && E >= 0 && N < (1LL << 31) / 64 && E < (1LL << 31), "%s: bad sizes N=%ld E=%ld", fn, (long)N, (long)E);
  return ESC_OK;
}

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_pna_max_channels(void) { return pna::MAX_C; }

int esc_pna_aggregate_fwd(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const float* R, int64_t ld_r,
                          const int32_t* in_ptr, const int32_t* in_edge, const int32_t* in_src, int64_t N, int64_t E, int64_t C,
                          float* agg, int64_t ld_agg, int32_t* arg, void* stream) {
  const char* fn = "esc_pna_aggregate_fwd";
  const bool edges = E > 0;
  const PnaLd ld[] = {{"ld_p", ld_p, C}, {"ld_q", ld_q, C}, {"ld_r", edges ? ld_r : C, C}, {"ld_agg", ld_agg, 3 * C}};
  const void* const ptrs[] = {P, Q, R, agg, arg};
  if (const int rc = pna_limits(fn, N, E, C, ld, 4, ptrs, 5)) return rc;
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(P && Q && in_ptr && agg && arg, "%s: null pointer", fn);
  ESC_REQUIRE(!edges || (R && in_edge && in_src), "%s: null edge pointer with E=%ld", fn, (long)E);
  hipStream_t s = (hipStream_t)stream;
  const pna::Plan p = pna::plan_aggregate(N, C, false);
  auto* fwd = p.lanes == 16 ? pna_fwd_kernel<16> : p.lanes == 32 ? pna_fwd_kernel<32> : pna_fwd_kernel<64>;
  esc::launch(-1, fwd, dim3(p.grid[0]), dim3(pna::BLOCK), 0, s, P, ld_p, Q, ld_q, R, ld_r, in_ptr, in_edge, in_src, (int)N, (int)C, agg, ld_agg, arg);
  ESC_CHECK_LAUNCH(fn);
  return ESC_OK;
}

int esc_pna_aggregate_bwd(const float* g, int64_t ld_g, const int32_t* arg, const int32_t* in_ptr, const int32_t* in_edge,
                          const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_edge, const int32_t* out_dst,
                          int64_t N, int64_t E, int64_t C, float* d_R, int64_t ld_dr, float* d_P, int64_t ld_dp, float* d_Q,
                          int64_t ld_dq, void* stream) {
  const char* fn = "esc_pna_aggregate_bwd";
  const bool edges = E > 0;
  const PnaLd ld[] = {{"ld_g", ld_g, 3 * C}, {"ld_dr", edges ? ld_dr : C, C}, {"ld_dp", ld_dp, C}, {"ld_dq", ld_dq, C}};
  const void* const ptrs[] = {g, arg, d_R, d_P, d_Q};
  if (const int rc = pna_limits(fn, N, E, C, ld, 4, ptrs, 5)) return rc;
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(g && arg && in_ptr && out_ptr && d_P && d_Q, "%s: null pointer", fn);
  ESC_REQUIRE(!edges || (in_edge && in_src && out_edge && out_dst && d_R), "%s: null edge pointer with E=%ld", fn, (long)E);
  hipStream_t s = (hipStream_t)stream;
  const pna::Plan p = pna::plan_aggregate(N, C, true);
  auto* dst = p.lanes == 16 ? pna_bwd_dst_kernel<16> : p.lanes == 32 ? pna_bwd_dst_kernel<32> : pna_bwd_dst_kernel<64>;
  auto* src = p.lanes == 16 ? pna_bwd_src_kernel<16> : p.lanes == 32 ? pna_bwd_src_kernel<32> : pna_bwd_src_kernel<64>;
  esc::launch(-1, dst, dim3(p.grid[0]), dim3(pna::BLOCK), 0, s, g, ld_g, arg, in_ptr, in_edge, (int)N, (int)C, d_R, ld_dr, d_P, ld_dp);
  esc::launch(-1, src, dim3(p.grid[1]), dim3(pna::BLOCK), 0, s, (const float*)d_R, ld_dr, out_ptr, out_edge, (int)N, (int)C, d_Q, ld_dq);
  ESC_CHECK_LAUNCH(fn);
  return ESC_OK;
}

}  // extern "C"
