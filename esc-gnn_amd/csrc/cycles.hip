// cycles.hip — per-node counts of the simple 3..6-cycles of small graphs (the ZINC cycle-counting labels).
//
// Restates the reference's dataset_zinc_cycle.py:45-61 (pkl2data): self loops dropped, edges symmetrised and de-duplicated
// (to_undirected), networkx.simple_cycles over the resulting directed graph, cycles of length 3..6 kept, +1 for every node on
// each, the whole divided by two (every undirected cycle shows up once per direction).  out[v][k-3] is therefore the number of
// undirected simple k-cycles through v, an integer.
//
// One 64-lane workgroup per graph: the adjacency rows are 64-bit masks in LDS (n <= 64), and lane r counts the closed simple
// paths r -> v1 -> ... -> v_{k-1} -> r with a depth-bounded DFS whose per-depth candidate masks are loop-local registers (the
// four nested loops below).  A cycle through r is such a path in each of its two directions, so the int32 count is halved.
// The closing step needs no loop of its own: the paths of length k that close are popcount(candidates & adj[r]).
// Work per root is at most deg * (deg-1)^3 mask steps (750 at degree 6): bound by LDS latency, microseconds per launch.
#include "ragged_graphs.h"

namespace esc {

__global__ __launch_bounds__(64) void cycle_counts_kernel(const int64_t* __restrict__ node_ptr,
                                                          const int64_t* __restrict__ edge_ptr,
                                                          const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                          int64_t total_nodes, int64_t total_edges,
                                                          float* __restrict__ out, int32_t* __restrict__ status) {
  __shared__ unsigned long long adj[ADJ_MAX_NODES];
  __shared__ int bad;
  const int lane = threadIdx.x;
  int64_t n0, n;
  if (!adjacency_masks(node_ptr, edge_ptr, src, dst, total_nodes, total_edges, status, adj, bad, n0, n)) return;
  if (lane >= n) return;
  const int r = lane;
  const unsigned long long rbit = 1ull << r, close = adj[r];
  int c3 = 0, c4 = 0, c5 = 0, c6 = 0;
  unsigned long long m1 = close;
  while (m1) {
    const int v1 = __ffsll((long long)m1) - 1;
    m1 &= m1 - 1;
    const unsigned long long vis1 = rbit | (1ull << v1);
    unsigned long long m2 = adj[v1] & ~vis1;
    c3 += __popcll(m2 & close);                     // r v1 v2 r
    while (m2) {
      const int v2 = __ffsll((long long)m2) - 1;
      m2 &= m2 - 1;
      const unsigned long long vis2 = vis1 | (1ull << v2);
      unsigned long long m3 = adj[v2] & ~vis2;
      c4 += __popcll(m3 & close);                   // r v1 v2 v3 r
      while (m3) {
        const int v3 = __ffsll((long long)m3) - 1;
        m3 &= m3 - 1;
        const unsigned long long vis3 = vis2 | (1ull << v3);
        unsigned long long m4 = adj[v3] & ~vis3;
        c5 += __popcll(m4 & close);                 // r v1 .. v4 r
        while (m4) {
          const int v4 = __ffsll((long long)m4) - 1;
          m4 &= m4 - 1;
          c6 += __popcll(adj[v4] & ~(vis3 | (1ull << v4)) & close);   // r v1 .. v5 r
        }
      }
    }
  }
  const float4 o = make_float4((float)(c3 >> 1), (float)(c4 >> 1), (float)(c5 >> 1), (float)(c6 >> 1));
  reinterpret_cast<float4*>(out)[n0 + r] = o;
}

}  // namespace esc

using namespace esc;

extern "C" int esc_cycle_counts(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst,
                                int64_t G, int64_t total_nodes, int64_t total_edges, float* out, int32_t* status,
                                void* stream) {
  ESC_REQUIRE(G >= 0 && total_nodes >= 0 && total_edges >= 0, "esc_cycle_counts: negative size");
  if (G == 0) return ESC_OK;
  ESC_REQUIRE(node_ptr && edge_ptr && status, "esc_cycle_counts: null graph arrays");
  ESC_REQUIRE((src && dst) || total_edges == 0, "esc_cycle_counts: null edge arrays");
  ESC_REQUIRE(out || total_nodes == 0, "esc_cycle_counts: null output");
  ESC_REQUIRE(out == nullptr || aligned16(out), "esc_cycle_counts: out must be 16-byte aligned (float4 rows)");
  ESC_REQUIRE(G < (1LL << 31), "esc_cycle_counts: too many graphs in one call");
  hipStream_t s = (hipStream_t)stream;
  // graphs over 64 nodes report ESC_ERANGE through status[g]; an id or a range outside the arrays, ESC_EINVAL
  esc::launch(ESC_K_FEATURES, cycle_counts_kernel, dim3((unsigned)G), dim3(64), 0, s, node_ptr, edge_ptr, src, dst, total_nodes,
              total_edges, out, status);
  ESC_CHECK_LAUNCH("esc_cycle_counts");
  return ESC_OK;
}
