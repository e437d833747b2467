// gatedgcn.hip — the gate of the GatedGCN local layer (include/escgnn_gatedgcn.h): what the reference's
// CustomGatedGCN does in message / aggregate / update (GraphGPS/graphgps/layer/gatedgcn_layer.py:90-136) with three row
// gathers, a sigmoid, a product and two scatter-adds, as ONE segmented pass over the destination-sorted view of the plan, and
// its backward as one pass over each view.
//
//   forward   e_ij = (Dx[i] + Ex[j]) + Ce[k];  s = 1 / (1 + expf(-e_ij));  out[i] = Ax[i] + (sum s * Bx[j]) / (sum s + 1e-6)
//   backward  pass 1 (destination view): d_Ce[k] = g_e[k] + ((r_i * (Bx[j] - aggr_i)) * s) * (1 - s);  d_Dx[i] = sum d_Ce[k]
//             pass 2 (source view):      d_Ex[j] = sum d_Ce[k];  d_Bx[j] = sum s_k * r_{dst_k}
//
// Work split (HBM/L2-bound row kernels, no MFMA, as aggregate.hip): a row of C floats is covered by float4 lanes, so a group of
// LG = 16 (C <= 64), 32 (C <= 128) or 64 lanes owns one node and a wave owns 64 / LG nodes - at the run's C = 64 four nodes per
// wave, no lane idle on a full row.  The groups of a wave walk their own edge ranges (the loop is divergent between groups, not
// inside one), and a group's sums run over its node's slots in order: the order of every sum is a function of the edge order
// alone, whatever else shares the wave, the workgroup or the launch.  A hub's group runs long while its three neighbours wait;
// dealing one node's edges over several groups would need an ordered combine through LDS for a case the molecule batches do
// not have, and was not built.
// Edges are consumed in batches of GG_BATCH with every row read of the batch issued before the first use (agg_fwd_wave's
// scheme: a short tail is padded by clamping the slot to the node's last edge and masking its contribution).
// No atomics; every output element is written once.  Built with -ffp-contract=off (Makefile).
#include "common.h"
#include "graph_wave.h"
#include "sparse_plan.h"
#include "../../include/escgnn_gatedgcn.h"

namespace esc {

constexpr int GG_BATCH = 4;               // 3-4 float4 row reads per edge: 12-16 loads in flight per lane
constexpr int GG_MAX_C = 1024;
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
  int node, c0;
  if (!group_locate<LG>(N, node, c0)) return;
  const int beg = in_ptr[node], end = in_ptr[node + 1];
  for (int c = c0; c < C; c += LG * 4) {
    const float4 dxi = ld4(Dx + (size_t)node * ld_dx + c);
    const float4 axi = ld4(Ax + (size_t)node * ld_ax + c);
    float4 num = make_float4(0.f, 0.f, 0.f, 0.f), sum = num;
    for (int j = beg; j < end; j += GG_BATCH) {
      float4 ex[GG_BATCH], bx[GG_BATCH], ce[GG_BATCH];
      int kk[GG_BATCH];
#pragma unroll
      for (int u = 0; u < GG_BATCH; ++u) {
        const int jj = min(j + u, end - 1);                   // tail padding: the node's last edge again, masked below
        kk[u] = in_edge[jj];
        const int s = in_src[jj];
        ex[u] = ld4(Ex + (size_t)s * ld_ex + c);
        bx[u] = ld4(Bx + (size_t)s * ld_bx + c);
        ce[u] = ld4(Ce + (size_t)kk[u] * ld_ce + c);
      }
#pragma unroll
      for (int u = 0; u < GG_BATCH; ++u) {
        if (j + u < end) {                                    // uniform over the group: ascending edge position
          float4 e, g;
          e.x = (dxi.x + ex[u].x) + ce[u].x; e.y = (dxi.y + ex[u].y) + ce[u].y;
          e.z = (dxi.z + ex[u].z) + ce[u].z; e.w = (dxi.w + ex[u].w) + ce[u].w;
          g.x = gg_sigmoid(e.x); g.y = gg_sigmoid(e.y); g.z = gg_sigmoid(e.z); g.w = gg_sigmoid(e.w);
          num.x += g.x * bx[u].x; num.y += g.y * bx[u].y; num.z += g.z * bx[u].z; num.w += g.w * bx[u].w;
          sum.x += g.x; sum.y += g.y; sum.z += g.z; sum.w += g.w;
          st4(e_out + (size_t)kk[u] * ld_eo + c, e);
        }
      }
    }
    float4 o;
    o.x = axi.x + num.x / (sum.x + GG_EPS); o.y = axi.y + num.y / (sum.y + GG_EPS);
    o.z = axi.z + num.z / (sum.z + GG_EPS); o.w = axi.w + num.w / (sum.w + GG_EPS);
    st4(out + (size_t)node * ld_out + c, o);
    st4(den + (size_t)node * C + c, sum);
  }
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
  int node, c0;
  if (!group_locate<LG>(N, node, c0)) return;
  const int beg = in_ptr[node], end = in_ptr[node + 1];
  const bool has_ge = g_e != nullptr;
  for (int c = c0; c < C; c += LG * 4) {
    const float4 go = ld4(g_out + (size_t)node * ld_go + c);
    const float4 dn = ld4(den + (size_t)node * C + c);
    const float4 oi = ld4(out + (size_t)node * ld_out + c);
    const float4 ai = ld4(Ax + (size_t)node * ld_ax + c);
    float4 r, ag, acc = make_float4(0.f, 0.f, 0.f, 0.f);
    r.x = go.x / (dn.x + GG_EPS); r.y = go.y / (dn.y + GG_EPS); r.z = go.z / (dn.z + GG_EPS); r.w = go.w / (dn.w + GG_EPS);
    ag.x = oi.x - ai.x; ag.y = oi.y - ai.y; ag.z = oi.z - ai.z; ag.w = oi.w - ai.w;
    for (int j = beg; j < end; j += GG_BATCH) {
      float4 ev[GG_BATCH], bx[GG_BATCH], ge[GG_BATCH];
      int kk[GG_BATCH];
#pragma unroll
      for (int u = 0; u < GG_BATCH; ++u) {
        const int jj = min(j + u, end - 1);
        kk[u] = in_edge[jj];
        const int s = in_src[jj];
        ev[u] = ld4(e_out + (size_t)kk[u] * ld_eo + c);
        bx[u] = ld4(Bx + (size_t)s * ld_bx + c);
        ge[u] = has_ge ? ld4(g_e + (size_t)kk[u] * ld_ge + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < GG_BATCH; ++u) {
        if (j + u < end) {
          float4 s, d;
          s.x = gg_sigmoid(ev[u].x); s.y = gg_sigmoid(ev[u].y); s.z = gg_sigmoid(ev[u].z); s.w = gg_sigmoid(ev[u].w);
          d.x = ge[u].x + ((r.x * (bx[u].x - ag.x)) * s.x) * (1.0f - s.x);
          d.y = ge[u].y + ((r.y * (bx[u].y - ag.y)) * s.y) * (1.0f - s.y);
          d.z = ge[u].z + ((r.z * (bx[u].z - ag.z)) * s.z) * (1.0f - s.z);
          d.w = ge[u].w + ((r.w * (bx[u].w - ag.w)) * s.w) * (1.0f - s.w);
          acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
          st4(d_Ce + (size_t)kk[u] * ld_dce + c, d);
        }
      }
    }
    st4(d_Dx + (size_t)node * ld_ddx + c, acc);
  }
}

// backward, pass 2: one group per SOURCE node; d_Ce is what pass 1 wrote (the launch boundary orders the two)
template <int LG>
__global__ __launch_bounds__(256) void gated_bwd_src_kernel(const float* __restrict__ g_out, int64_t ld_go, const float* __restrict__ e_out,
                                                            int64_t ld_eo, const float* __restrict__ den, const float* __restrict__ d_Ce,
                                                            int64_t ld_dce, const int* __restrict__ out_ptr, const int* __restrict__ out_edge,
                                                            const int* __restrict__ out_dst, int N, int C, float* __restrict__ d_Ex,
                                                            int64_t ld_dex, float* __restrict__ d_Bx, int64_t ld_dbx) {
  ESC_PRIO();
  int node, c0;
  if (!group_locate<LG>(N, node, c0)) return;
  const int beg = out_ptr[node], end = out_ptr[node + 1];
  for (int c = c0; c < C; c += LG * 4) {
    float4 ae = make_float4(0.f, 0.f, 0.f, 0.f), ab = ae;
    for (int j = beg; j < end; j += GG_BATCH) {
      float4 dc[GG_BATCH], ev[GG_BATCH], go[GG_BATCH], dn[GG_BATCH];
#pragma unroll
      for (int u = 0; u < GG_BATCH; ++u) {
        const int jj = min(j + u, end - 1);
        const int k = out_edge[jj];
        const int d = out_dst[jj];
        dc[u] = ld4(d_Ce + (size_t)k * ld_dce + c);
        ev[u] = ld4(e_out + (size_t)k * ld_eo + c);
        go[u] = ld4(g_out + (size_t)d * ld_go + c);
        dn[u] = ld4(den + (size_t)d * C + c);
      }
#pragma unroll
      for (int u = 0; u < GG_BATCH; ++u) {
        if (j + u < end) {
          ae.x += dc[u].x; ae.y += dc[u].y; ae.z += dc[u].z; ae.w += dc[u].w;
          ab.x += gg_sigmoid(ev[u].x) * (go[u].x / (dn[u].x + GG_EPS));
          ab.y += gg_sigmoid(ev[u].y) * (go[u].y / (dn[u].y + GG_EPS));
          ab.z += gg_sigmoid(ev[u].z) * (go[u].z / (dn[u].z + GG_EPS));
          ab.w += gg_sigmoid(ev[u].w) * (go[u].w / (dn[u].w + GG_EPS));
        }
      }
    }
    st4(d_Ex + (size_t)node * ld_dex + c, ae);
    st4(d_Bx + (size_t)node * ld_dbx + c, ab);
  }
}


// what both entries check before anything is launched; 0 or an error code with the message set
static int gg_limits(const char* fn, int64_t N, int64_t E, int64_t C, const int64_t* ld, const char* const* ld_name, int n_ld,
                     const void* const* p, int n_p) {
  ESC_REQUIRE(C >= 4 && C <= GG_MAX_C && C % 4 == 0, "%s: C=%ld: the width must be a multiple of 4 with 4 <= C <= %d "
              "(esc_gated_gcn_max_channels)", fn, (long)C, GG_MAX_C);
  for (int i = 0; i < n_ld; ++i)
    ESC_REQUIRE(ld[i] >= C && ld[i] % 4 == 0, "%s: leading dimension %s=%ld: every leading dimension must be >= C=%ld and a "
                "multiple of 4", fn, ld_name[i], (long)ld[i], (long)C);
  for (int i = 0; i < n_p; ++i) ESC_REQUIRE(aligned16(p[i]), "%s: every pointer must be 16-byte aligned", fn);
  ESC_REQUIRE(N >= 0 && E >= 0 && N < (1LL << 31) / 64 && E < (1LL << 31), "%s: bad sizes N=%ld E=%ld", fn, (long)N, (long)E);
  return ESC_OK;
}

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_gated_gcn_max_channels(void) { return GG_MAX_C; }

int esc_gated_gcn_fwd(const float* Ax, int64_t ld_ax, const float* Bx, int64_t ld_bx, const float* Dx, int64_t ld_dx,
                      const float* Ex, int64_t ld_ex, const float* Ce, int64_t ld_ce, const int32_t* in_ptr,
                      const int32_t* in_edge, const int32_t* in_src, int64_t N, int64_t E, int64_t C, float* out, int64_t ld_out,
                      float* e_out, int64_t ld_eo, float* den, void* stream) {
  const char* fn = "esc_gated_gcn_fwd";
  const bool edges = E > 0;
  const int64_t ld[] = {ld_ax, ld_bx, ld_dx, ld_ex, ld_out, edges ? ld_ce : C, edges ? ld_eo : C};
  const char* const names[] = {"ld_ax", "ld_bx", "ld_dx", "ld_ex", "ld_out", "ld_ce", "ld_eo"};
  const void* const ptrs[] = {Ax, Bx, Dx, Ex, Ce, out, e_out, den};
  if (const int rc = gg_limits(fn, N, E, C, ld, names, 7, ptrs, 8)) return rc;
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(Ax && Bx && Dx && Ex && in_ptr && out && den, "%s: null pointer", fn);
  ESC_REQUIRE(!edges || (Ce && in_edge && in_src && e_out), "%s: null edge pointer with E=%ld", fn, (long)E);
  hipStream_t s = (hipStream_t)stream;
  const sparse::Plan p = sparse::plan_gated(N, C, false);
  auto* fwd = gated_fwd_kernel<64>;
  switch (p.family) {
    case sparse::F_GROUP16: fwd = gated_fwd_kernel<16>; break;
    case sparse::F_GROUP32: fwd = gated_fwd_kernel<32>; break;
    default: break;
  }
  esc::launch(-1, fwd, dim3(p.grid[0].x), dim3(256), 0, s, Ax, ld_ax, Bx, ld_bx, Dx, ld_dx, Ex, ld_ex, Ce, ld_ce, in_ptr, in_edge, in_src, (int)N, (int)C, out,
              ld_out, e_out, ld_eo, den);
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
  const int64_t ld[] = {ld_go, ld_out, ld_ax, ld_bx, ld_ddx, ld_dex, ld_dbx, edges ? ld_eo : C, edges ? ld_dce : C, (edges && g_e) ? ld_ge : C};
  const char* const names[] = {"ld_go", "ld_out", "ld_ax", "ld_bx", "ld_ddx", "ld_dex", "ld_dbx", "ld_eo", "ld_dce", "ld_ge"};
  const void* const ptrs[] = {g_out, g_e, e_out, den, out, Ax, Bx, d_Ce, d_Dx, d_Ex, d_Bx};
  if (const int rc = gg_limits(fn, N, E, C, ld, names, 10, ptrs, 11)) return rc;
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(g_out && den && out && Ax && Bx && in_ptr && out_ptr && d_Dx && d_Ex && d_Bx, "%s: null pointer", fn);
  ESC_REQUIRE(!edges || (e_out && in_edge && in_src && out_edge && out_dst && d_Ce), "%s: null edge pointer with E=%ld", fn, (long)E);
  hipStream_t s = (hipStream_t)stream;
  const sparse::Plan p = sparse::plan_gated(N, C, true);
  auto* dst = gated_bwd_dst_kernel<64>;
  auto* src = gated_bwd_src_kernel<64>;
  switch (p.family) {
    case sparse::F_GROUP16: dst = gated_bwd_dst_kernel<16>; src = gated_bwd_src_kernel<16>; break;
    case sparse::F_GROUP32: dst = gated_bwd_dst_kernel<32>; src = gated_bwd_src_kernel<32>; break;
    default: break;
  }
  esc::launch(-1, dst, dim3(p.grid[0].x), dim3(256), 0, s, g_out, ld_go, g_e, ld_ge, e_out, ld_eo, den, out, ld_out, Ax, ld_ax, Bx, ld_bx, in_ptr, in_edge,
              in_src, (int)N, (int)C, d_Ce, ld_dce, d_Dx, ld_ddx);
  esc::launch(-1, src, dim3(p.grid[1].x), dim3(256), 0, s, g_out, ld_go, e_out, ld_eo, den, (const float*)d_Ce, ld_dce, out_ptr, out_edge, out_dst, (int)N,
              (int)C, d_Ex, ld_dex, d_Bx, ld_dbx);
  ESC_CHECK_LAUNCH(fn);
  return ESC_OK;
}

}  // extern "C"
