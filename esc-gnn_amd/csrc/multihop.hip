// multihop.hip — the multi-hop edges of a collated batch (the GINE+ baseline's make_multihop_edges) on the GPU.
//
// Replaces make_multihop_edges of the reference's modules/gine_operations.py:256-303: k - 1 torch_sparse SpGEMMs (A^2 .. A^k), a
// concatenation with the diagonal and the edge list, and coalesce(op='min'), run inside every forward.
//
// Semantics restated: the output is {(i, i) at 0} u {(i, j) at d(i -> j) : 1 <= d(i -> j) <= k}, d the directed
// shortest-path length over the edges read src -> dst; sorted by (row, col).  A^d[i, j] > 0 exactly when a walk of length d
// leads from i to j, and the minimum over d of the coalesce is the length of the shortest one: a bounded BFS from i over the
// out-edges.  The diagonal enters at 0 before the minimum, so a self loop or a 2-cycle leaves it at 0; repeated edges only
// change the values of A^d, which are dropped.
//
// One wave per root, twice, in the manner of subgraphs.hip: the count pass sizes the output (and counts, per graph, the pairs at
// every distance, which is what a dataset keeps so that no step reads a size back), the fill pass repeats the BFS and writes
// with ballot-prefix compaction in node order, which IS ascending column order: no sort.  sub_locate, sub_bfs, the validation
// and the scan are those of subgraphs.hip (graph_wave.h); sub_bfs walks target -> source, so it is handed (dst, src) to walk
// the out-edges.  LDS: one byte per node of the root's graph.  Integer work bound by LDS / L2 latency.
#include "common.h"
#include "graph_wave.h"
#include "../../include/escgnn_gineplus.h"

namespace esc {

constexpr int MH_K_MAX = 8;
constexpr int MH_MAX_NODES = 4096;      // hop[] of 4 KB: the 32 waves a CU can hold take 128 of its 160 KB, so LDS never limits residency

__global__ __launch_bounds__(64) void mh_count_kernel(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr,
                                                      const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int G,
                                                      int64_t total_nodes, int k, const int* __restrict__ status,
                                                      int64_t* __restrict__ cnt_pairs, int64_t* __restrict__ cnt_d1,
                                                      unsigned long long* __restrict__ dist_count) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const int64_t r_glob = blockIdx.x;
  if (r_glob >= total_nodes) return;
  const SubRoot q = sub_locate(node_ptr, edge_ptr, G, r_glob);
  if (status[q.g] != 0) {
    if (lane == 0) { cnt_pairs[r_glob] = 0; cnt_d1[r_glob] = 0; }
    return;
  }
  unsigned char* hop = smem;
  sub_bfs(q, dst, src, k, hop);                             // (dst, src): hop[x] = d(r -> x) over the out-edges
  int cnt[MH_K_MAX + 1];
#pragma unroll
  for (int d = 0; d <= MH_K_MAX; ++d) cnt[d] = 0;
  for (int x0 = 0; x0 < q.n; x0 += 64) {
    const int x = x0 + lane;
    const int hx = x < q.n ? (int)hop[x] : (int)GRAPH_HOP_INF;
#pragma unroll
    for (int d = 0; d <= MH_K_MAX; ++d) cnt[d] += __popcll(__ballot(hx == d));
  }
  if (lane == 0) {
    int total = 0;
#pragma unroll
    for (int d = 0; d <= MH_K_MAX; ++d) {
      if (d <= k) {
        total += cnt[d];
        if (cnt[d]) atomicAdd(&dist_count[(size_t)q.g * (k + 1) + d], (unsigned long long)cnt[d]);    // integers: order free
      }
    }
    cnt_pairs[r_glob] = total;
    cnt_d1[r_glob] = cnt[1];
  }
}

__global__ __launch_bounds__(64) void mh_fill_kernel(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr,
                                                     const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int G,
                                                     int64_t total_nodes, int k, const int64_t* __restrict__ pair_ptr,
                                                     const int64_t* __restrict__ d1_ptr, int64_t total_pairs,
                                                     int64_t* __restrict__ row, int64_t* __restrict__ col,
                                                     int64_t* __restrict__ distance, int* __restrict__ meta,
                                                     int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const int64_t r_glob = blockIdx.x;
  if (r_glob >= total_nodes) return;
  const int64_t p0 = pair_ptr[r_glob], p1 = pair_ptr[r_glob + 1];
  if (p1 == p0) return;                                     // a graph the count pass refused (a valid root holds at least itself)
  const SubRoot q = sub_locate(node_ptr, edge_ptr, G, r_glob);
  if (p0 < 0 || p1 > total_pairs) {
    if (lane == 0) status[q.g] = ESC_ERANGE;                // the caller's total is not that of the count pass: write nothing
    return;
  }
  unsigned char* hop = smem;
  sub_bfs(q, dst, src, k, hop);
  const int64_t r1 = d1_ptr[r_glob];
  int base = 0, base1 = 0;
  for (int x0 = 0; x0 < q.n; x0 += 64) {
    const int x = x0 + lane;
    const int hx = x < q.n ? (int)hop[x] : (int)GRAPH_HOP_INF;
    const bool mine = hx != (int)GRAPH_HOP_INF, one = hx == 1;
    const int slot = ballot_compact(mine, base), slot1 = ballot_compact(one, base1);
    if (mine) {
      const int64_t p = p0 + slot;
      if (p < p1) {                                         // (holds by construction: the same BFS sized the range)
        const int64_t j = q.n0 + x;
        row[p] = r_glob; col[p] = j; distance[p] = hx;
        int4 m;
        m.x = (int)r_glob; m.y = (int)j; m.z = hx; m.w = one ? (int)(r1 + slot1) : -1;
        *reinterpret_cast<int4*>(meta + 4 * p) = m;
      }
    }
  }
}

static const ExpandLimits MH_LIMITS = {"k", MH_K_MAX, MH_MAX_NODES, "", false};

}  // namespace esc

using namespace esc;

extern "C" {

int esc_multihop_count(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                       int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int k, int64_t* pair_ptr, int64_t* d1_ptr,
                       int64_t* dist_count, int32_t* status, void* stream) {
  const int rc = expand_check(MH_LIMITS, "esc_multihop_count", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, k);
  if (rc) return rc;
  ESC_REQUIRE(pair_ptr && d1_ptr && dist_count && status, "esc_multihop_count: null output");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(dist_count, 0, (size_t)G * (k + 1) * sizeof(int64_t), s) != hipSuccess) {
    set_error("esc_multihop_count: memset failed");
    return ESC_ELAUNCH;
  }
  sub_launch_validate(node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, status, s);
  ESC_CHECK_LAUNCH("esc_multihop_count.validate");
  if (total_nodes > 0) {
    const int n_cap = (int)((max_nodes + 15) & ~15LL);
    esc::launch(ESC_K_FEATURES, mh_count_kernel, dim3((unsigned)total_nodes), dim3(64), (size_t)n_cap, s, node_ptr, edge_ptr, src, dst,
                (int)G, total_nodes, k, (const int*)status, pair_ptr, d1_ptr, reinterpret_cast<unsigned long long*>(dist_count));
    ESC_CHECK_LAUNCH("esc_multihop_count.count");
  }
  sub_launch_scan(pair_ptr, d1_ptr, total_nodes, s);
  ESC_CHECK_LAUNCH("esc_multihop_count.scan");
  return ESC_OK;
}

int esc_multihop_fill(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                      int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int k, const int64_t* pair_ptr,
                      const int64_t* d1_ptr, int64_t total_pairs, int64_t* row, int64_t* col, int64_t* distance, int32_t* meta,
                      int32_t* status, void* stream) {
  const int rc = expand_check(MH_LIMITS, "esc_multihop_fill", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, k);
  if (rc) return rc;
  ESC_REQUIRE(pair_ptr && d1_ptr && status, "esc_multihop_fill: null pointer");
  if (total_pairs < 0 || total_pairs >= (1LL << 31) - 1) {
    set_error("esc_multihop_fill: %ld pairs: totals must stay below 2^31", (long)total_pairs);
    return ESC_ERANGE;
  }
  if (total_nodes == 0 || total_pairs == 0) return ESC_OK;
  ESC_REQUIRE(row && col && distance && meta, "esc_multihop_fill: null output");
  ESC_REQUIRE(esc::aligned16(meta), "esc_multihop_fill: meta must be 16-byte aligned");
  const int n_cap = (int)((max_nodes + 15) & ~15LL);
  esc::launch(ESC_K_FEATURES, mh_fill_kernel, dim3((unsigned)total_nodes), dim3(64), (size_t)n_cap, (hipStream_t)stream, node_ptr, edge_ptr,
              src, dst, (int)G, total_nodes, k, pair_ptr, d1_ptr, total_pairs, row, col, distance, meta, status);
  ESC_CHECK_LAUNCH("esc_multihop_fill.fill");
  return ESC_OK;
}

}  // extern "C"
