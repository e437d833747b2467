// gatedgcn.hip — the gate of the GatedGCN local layer (include/escgnn_gatedgcn.h): what the reference's
// CustomGatedGCN does in message / aggregate / update (GraphGPS/graphgps/layer/gatedgcn_layer.py:90-136) with three row
// gathers, a sigmoid, a product and two scatter-adds, as ONE segmented pass over the destination-sorted view of the plan, and
// its backward as one pass over each view.
//
//   forward   e_ij = (Dx[i] + Ex[j]) + Ce[k];  s = 1 / (1 + expf(-e_ij));  out[i] = Ax[i] + (sum s * Bx[j]) / (sum s + 1e-6)
//   backward  pass 1 (destination view): d_Ce[k] = g_e[k] + ((r_i * (Bx[j] - aggr_i)) * s) * (1 - s);  d_Dx[i] = sum d_Ce[k]
//             pass 2 (source view):      d_Ex[j] = sum d_Ce[k];  d_Bx[j] = sum s_k * r_{dst_k}
//
// Work split (HBM/L2-bound row kernels, no MFMA, as aggregate.hip): row_walk.h's lane groups (sparse_plan.h: plan_gated) - a
// row of C floats is covered by float4 lanes, so a group of LG = 16 (C <= 64), 32 (C <= 128) or 64 lanes owns one node and a
// wave owns 64 / LG nodes - at the run's C = 64 four nodes per wave, no lane idle on a full row.  A group's sums run over its
// node's slots in order: the order of every sum is a function of the edge order alone.  A hub's group runs long while its three
// neighbours wait; dealing one node's edges over several groups would need an ordered combine through LDS for a case the
// molecule batches do not have, and was not built.
// No atomics; every output element is written once.  Built with -ffp-contract=off (Makefile).
#include "common.h"
#include "row_walk.h"
#include "sparse_plan.h"
#include "../../include/escgnn_gatedgcn.h"

namespace esc {

constexpr int GG_BATCH = 4;               // 3-4 float4 row reads per edge: 12-16 loads in flight per lane
constexpr float GG_EPS = 1e-6f;

__device__ __forceinline__ float gg_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int LG>
__global__ __launch_bounds__(256) void gated_fwd_kernel(const float* __restrict__ Ax, int64_t ld_ax, const float* __restrict__ Bx,
                                                        int64_t ld_bx, const float* __restrict__ Dx, int64_t ld_dx,
                                                        const float* __restrict__ Ex, int64_t ld_ex, const float* __restrict__ Ce,
                                                        int64_t ld_ce, const int* __restrict__ in_ptr, const int* __restrict__ in_edge,
                                                        const int* __restrict__ in_src, int N, int C, float* __restrict__ out,
                                                        int64_t ld_out, float* __restrict__ e_out, int64_t ld_eo, float* __restrict__ den) {
  ESC_PRIO();
  group_columns<LG>(in_ptr, N, C, [&](int node, int c, int beg, int end) {
    float dxi[4], axi[4], num[4] = {0.f, 0.f, 0.f, 0.f}, sum[4] = {0.f, 0.f, 0.f, 0.f}, ex[GG_BATCH][4], bx[GG_BATCH][4], ce[GG_BATCH][4];
    int kk[GG_BATCH];
    row_load<4>(Dx + (size_t)node * ld_dx + c, dxi);
    row_load<4>(Ax + (size_t)node * ld_ax + c, axi);
    segment_batches<GG_BATCH>(beg, end, [&](int u, int jj, bool) {
      kk[u] = in_edge[jj];
      const int s = in_src[jj];
      row_load<4>(Ex + (size_t)s * ld_ex + c, ex[u]);
      row_load<4>(Bx + (size_t)s * ld_bx + c, bx[u]);
      row_load<4>(Ce + (size_t)kk[u] * ld_ce + c, ce[u]);
    }, [&](int u) {
      float e[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        e[t] = (dxi[t] + ex[u][t]) + ce[u][t];
        const float g = gg_sigmoid(e[t]);
        num[t] += g * bx[u][t];
        sum[t] += g;
      }
      row_store<4>(e_out + (size_t)kk[u] * ld_eo + c, e);
    });
    float o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = axi[t] + num[t] / (sum[t] + GG_EPS);
    row_store<4>(out + (size_t)node * ld_out + c, o);
    row_store<4>(den + (size_t)node * C + c, sum);
  });
}

// backward, pass 1: one group per DESTINATION node
template <int LG>
__global__ __launch_bounds__(256) void gated_bwd_dst_kernel(const float* __restrict__ g_out, int64_t ld_go, const float* __restrict__ g_e,
                                                            int64_t ld_ge, const float* __restrict__ e_out, int64_t ld_eo,
                                                            const float* __restrict__ den, const float* __restrict__ out, int64_t ld_out,
                                                            const float* __restrict__ Ax, int64_t ld_ax, const float* __restrict__ Bx,
                                                            int64_t ld_bx, const int* __restrict__ in_ptr, const int* __restrict__ in_edge,
                                                            const int* __restrict__ in_src, int N, int C, float* __restrict__ d_Ce,
                                                            int64_t ld_dce, float* __restrict__ d_Dx, int64_t ld_ddx) {
  ESC_PRIO();
  const bool has_ge = g_e != nullptr;
  group_columns<LG>(in_ptr, N, C, [&](int node, int c, int beg, int end) {
    float go[4], dn[4], oi[4], ai[4], r[4], ag[4], acc[4] = {0.f, 0.f, 0.f, 0.f}, ev[GG_BATCH][4], bx[GG_BATCH][4], ge[GG_BATCH][4];
    int kk[GG_BATCH];
    row_load<4>(g_out + (size_t)node * ld_go + c, go);
    row_load<4>(den + (size_t)node * C + c, dn);
    row_load<4>(out + (size_t)node * ld_out + c, oi);
    row_load<4>(Ax + (size_t)node * ld_ax + c, ai);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      r[t] = go[t] / (dn[t] + GG_EPS);
      ag[t] = oi[t] - ai[t];
    }
    segment_batches<GG_BATCH>(beg, end, [&](int u, int jj, bool) {
      kk[u] = in_edge[jj];
      const int s = in_src[jj];
      row_load<4>(e_out + (size_t)kk[u] * ld_eo + c, ev[u]);
      row_load<4>(Bx + (size_t)s * ld_bx + c, bx[u]);
      if (has_ge) row_load<4>(g_e + (size_t)kk[u] * ld_ge + c, ge[u]);
      else {
#pragma unroll
        for (int t = 0; t < 4; ++t) ge[u][t] = 0.f;
      }
    }, [&](int u) {
      float d[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float s = gg_sigmoid(ev[u][t]);
        d[t] = ge[u][t] + ((r[t] * (bx[u][t] - ag[t])) * s) * (1.0f - s);
        acc[t] += d[t];
      }
      row_store<4>(d_Ce + (size_t)kk[u] * ld_dce + c, d);
    });
    row_store<4>(d_Dx + (size_t)node * ld_ddx + c, acc);
  });
}

// backward, pass 2: one group per SOURCE node; d_Ce is what pass 1 wrote (the launch boundary orders the two)
template <int LG>
__global__ __launch_bounds__(256) void gated_bwd_src_kernel(const float* __restrict__ g_out, int64_t ld_go, const float* __restrict__ e_out,
                                                            int64_t ld_eo, const float* __restrict__ den, const float* __restrict__ d_Ce,
                                                            int64_t ld_dce, const int* __restrict__ out_ptr, const int* __restrict__ out_edge,
                                                            const int* __restrict__ out_dst, int N, int C, float* __restrict__ d_Ex,
                                                            int64_t ld_dex, float* __restrict__ d_Bx, int64_t ld_dbx) {
  ESC_PRIO();
  group_columns<LG>(out_ptr, N, C, [&](int node, int c, int beg, int end) {
    float ae[4] = {0.f, 0.f, 0.f, 0.f}, ab[4] = {0.f, 0.f, 0.f, 0.f}, dc[GG_BATCH][4], ev[GG_BATCH][4], go[GG_BATCH][4], dn[GG_BATCH][4];
    segment_batches<GG_BATCH>(beg, end, [&](int u, int jj, bool) {
      const int k = out_edge[jj];
      const int d = out_dst[jj];
      row_load<4>(d_Ce + (size_t)k * ld_dce + c, dc[u]);
      row_load<4>(e_out + (size_t)k * ld_eo + c, ev[u]);
      row_load<4>(g_out + (size_t)d * ld_go + c, go[u]);
      row_load<4>(den + (size_t)d * C + c, dn[u]);
    }, [&](int u) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        ae[t] += dc[u][t];
        ab[t] += gg_sigmoid(ev[u][t]) * (go[u][t] / (dn[u][t] + GG_EPS));
      }
    });
    row_store<4>(d_Ex + (size_t)node * ld_dex + c, ae);
    row_store<4>(d_Bx + (size_t)node * ld_dbx + c, ab);
  });
}

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_gated_gcn_max_channels(void) { return sparse::GG_MAX_C; }

int esc_gated_gcn_fwd(const float* Ax, int64_t ld_ax, const float* Bx, int64_t ld_bx, const float* Dx, int64_t ld_dx,
                      const float* Ex, int64_t ld_ex, const float* Ce, int64_t ld_ce, const int32_t* in_ptr,
                      const int32_t* in_edge, const int32_t* in_src, int64_t N, int64_t E, int64_t C, float* out, int64_t ld_out,
                      float* e_out, int64_t ld_eo, float* den, void* stream) {
  const char* fn = "esc_gated_gcn_fwd";
  const bool edges = E > 0;
  const RowLd ld[] = {{"ld_ax", ld_ax}, {"ld_bx", ld_bx}, {"ld_dx", ld_dx}, {"ld_ex", ld_ex}, {"ld_out", ld_out},
                      {"ld_ce", edges ? ld_ce : C}, {"ld_eo", edges ? ld_eo : C}};
  const void* const ptrs[] = {Ax, Bx, Dx, Ex, Ce, out, e_out, den};
  if (const int rc = group_limits(fn, "esc_gated_gcn_max_channels", sparse::GG_MAX_C, N, E, C, ld, ptrs)) return rc;
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(Ax && Bx && Dx && Ex && in_ptr && out && den, "%s: null pointer", fn);
  ESC_REQUIRE(!edges || (Ce && in_edge && in_src && e_out), "%s: null edge pointer with E=%ld", fn, (long)E);
  hipStream_t s = (hipStream_t)stream;
  const sparse::Plan p = sparse::plan_gated(N, C, false);
  esc::launch(-1, ESC_GROUP_KERNEL(gated_fwd_kernel, p.cw), dim3(p.grid[0].x), dim3(sparse::GROUP_BLOCK), 0, s, Ax, ld_ax, Bx, ld_bx, Dx, ld_dx, Ex, ld_ex,
              Ce, ld_ce, in_ptr, in_edge, in_src, (int)N, (int)C, out, ld_out, e_out, ld_eo, den);
  ESC_CHECK_LAUNCH(fn);
  return ESC_OK;
}

int esc_gated_gcn_bwd(const float* g_out, int64_t ld_go, const float* g_e, int64_t ld_ge, const float* e_out, int64_t ld_eo,
                      const float* den, const float* out, int64_t ld_out, const float* Ax, int64_t ld_ax, const float* Bx,
                      int64_t ld_bx, const int32_t* in_ptr, const int32_t* in_edge, const int32_t* in_src, const int32_t* out_ptr,
                      const int32_t* out_edge, const int32_t* out_dst, int64_t N, int64_t E, int64_t C, float* d_Ce, int64_t ld_dce,
                      float* d_Dx, int64_t ld_ddx, float* d_Ex, int64_t ld_dex, float* d_Bx, int64_t ld_dbx, void* stream) {
  const char* fn = "esc_gated_gcn_bwd";
  const bool edges = E > 0;
  const RowLd ld[] = {{"ld_go", ld_go}, {"ld_out", ld_out}, {"ld_ax", ld_ax}, {"ld_bx", ld_bx}, {"ld_ddx", ld_ddx},
                      {"ld_dex", ld_dex}, {"ld_dbx", ld_dbx}, {"ld_eo", edges ? ld_eo : C}, {"ld_dce", edges ? ld_dce : C},
                      {"ld_ge", (edges && g_e) ? ld_ge : C}};
  const void* const ptrs[] = {g_out, g_e, e_out, den, out, Ax, Bx, d_Ce, d_Dx, d_Ex, d_Bx};
  if (const int rc = group_limits(fn, "esc_gated_gcn_max_channels", sparse::GG_MAX_C, N, E, C, ld, ptrs)) return rc;
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(g_out && den && out && Ax && Bx && in_ptr && out_ptr && d_Dx && d_Ex && d_Bx, "%s: null pointer", fn);
  ESC_REQUIRE(!edges || (e_out && in_edge && in_src && out_edge && out_dst && d_Ce), "%s: null edge pointer with E=%ld", fn, (long)E);
  hipStream_t s = (hipStream_t)stream;
  const sparse::Plan p = sparse::plan_gated(N, C, true);
  esc::launch(-1, ESC_GROUP_KERNEL(gated_bwd_dst_kernel, p.cw), dim3(p.grid[0].x), dim3(sparse::GROUP_BLOCK), 0, s, g_out, ld_go, g_e, ld_ge, e_out, ld_eo,
              den, out, ld_out, Ax, ld_ax, Bx, ld_bx, in_ptr, in_edge, in_src, (int)N, (int)C, d_Ce, ld_dce, d_Dx, ld_ddx);
  esc::launch(-1, ESC_GROUP_KERNEL(gated_bwd_src_kernel, p.cw), dim3(p.grid[1].x), dim3(sparse::GROUP_BLOCK), 0, s, g_out, ld_go, e_out, ld_eo, den,
              (const float*)d_Ce, ld_dce, out_ptr, out_edge, out_dst, (int)N, (int)C, d_Ex, ld_dex, d_Bx, ld_dbx);
  ESC_CHECK_LAUNCH(fn);
  return ESC_OK;
}

}  // extern "C"
