// ragged_graphs.h — the device side of a ragged set of small graphs, stated once for the kernels that run one workgroup per
// graph and write per-node statistics (cycles.hip, graphlets.hip, lappe.hip, rwse.hip).
//
// The contract.  A set of G graphs is four arrays: node_ptr, edge_ptr [G+1] (int64) give graph g the node rows
// [node_ptr[g], node_ptr[g+1]) of N and the edges [edge_ptr[g], edge_ptr[g+1]) of src, dst [E].  A graph is taken when its two
// ranges are ordered and lie inside [0, N] and [0, E], and when every end of its edges, minus `base`, lies in [0, n): base = 0
// where the ends are graph-local ids, base = node_ptr[g] where they are rows of the batch.  Nothing here trusts the host: a graph
// that breaks the contract is the caller's to report (the label kernels, through status[g]) or to skip (the PE kernels), and
// every verdict is uniform over the workgroup, so it leaves together.  Each kernel adds its own size limit and its own policy
// for an empty graph on top.  Index and check code only: no floating-point expression lives here.
#pragma once
#include "common.h"

namespace esc {

// ---- 1. the graph's ranges ------------------------------------------------------------------------------------------------------
struct GraphRange {
  int64_t n0, n1, e0, e1;
  bool ok;                                   // ordered and inside [0, N] / [0, E]
};

__device__ __forceinline__ GraphRange graph_range(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr, int64_t g,
                                                  int64_t N, int64_t E) {
  GraphRange r{node_ptr[g], node_ptr[g + 1], edge_ptr[g], edge_ptr[g + 1], false};
  r.ok = r.n0 >= 0 && r.n1 >= r.n0 && r.n1 <= N && r.e0 >= 0 && r.e1 >= r.e0 && r.e1 <= E;
  return r;
}

// ---- 2. the checked edge ends ---------------------------------------------------------------------------------------------------
// the graph-local ends (s, t) of edge e and whether both lie in [0, n); one read of src[e] and dst[e]
__device__ __forceinline__ bool edge_ends(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t e, int64_t base, int64_t n,
                                          int64_t& s, int64_t& t) {
  s = src[e] - base;
  t = dst[e] - base;
  return s >= 0 && s < n && t >= 0 && t < n;
}

// ---- 3. the 64-node adjacency masks ---------------------------------------------------------------------------------------------
// The prologue of the label kernels (one 64-lane workgroup per graph, graph-local ids): row v of the graph's adjacency as a
// 64-bit mask in LDS, self loops dropped, edges symmetrised, duplicates collapsed in the mask.  status[g] becomes ESC_EINVAL for
// a range or an id outside the arrays, ESC_ERANGE for a graph over 64 nodes, ESC_OK otherwise (an empty graph included).
// Returns whether the workgroup goes on - uniform: on false the whole workgroup leaves and nothing else is written.  On true
// adj[] is complete behind a barrier, rows >= n are empty, and (n0, n) are the graph's first row and size.
constexpr int ADJ_MAX_NODES = 64;

__device__ __forceinline__ bool adjacency_masks(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr,
                                                const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t total_nodes,
                                                int64_t total_edges, int32_t* __restrict__ status,
                                                unsigned long long (&adj)[ADJ_MAX_NODES], int& bad, int64_t& n0, int64_t& n) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const GraphRange r = graph_range(node_ptr, edge_ptr, g, total_nodes, total_edges);
  n0 = r.n0;
  n = r.n1 - r.n0;
  if (!r.ok || n > ADJ_MAX_NODES) {
    if (lane == 0) status[g] = r.ok ? ESC_ERANGE : ESC_EINVAL;
    return false;
  }
  adj[lane] = 0ull;
  if (lane == 0) bad = 0;
  __syncthreads();
  for (int64_t e = r.e0 + lane; e < r.e1; e += 64) {
    int64_t a, b;
    if (!edge_ends(src, dst, e, 0, n, a, b)) { bad = 1; continue; }
    if (a == b) continue;                            // remove_self_loops
    atomicOr(&adj[a], 1ull << b);                    // to_undirected: both directions, duplicates collapse in the mask
    atomicOr(&adj[b], 1ull << a);
  }
  __syncthreads();
  if (lane == 0) status[g] = bad ? ESC_EINVAL : ESC_OK;
  return !bad;
}

// ---- 4. the table gather --------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads per graph of a batch copies the graph's n x K rows of T resident tables (row stride K) to T
// outputs of row stride ld >= K; columns K.. of an output row are left alone.  The single guard: a graph id outside the table, a
// source range outside [0, N_all], a destination range outside [0, N] or the two ranges of different length copy nothing.
template <int T>
struct GatherTables {
  const float* src[T];
  float* dst[T];
};

template <int T>
__global__ __launch_bounds__(256) void table_gather_kernel(GatherTables<T> tab, const int64_t* __restrict__ node_ptr_all, int64_t G_all,
                                                           int64_t N_all, const int64_t* __restrict__ ids,
                                                           const int32_t* __restrict__ graph_ptr, int64_t N, int K, int64_t ld) {
  const int64_t id = ids[blockIdx.x];
  if (id < 0 || id >= G_all) return;
  const int64_t s0 = node_ptr_all[id], n = node_ptr_all[id + 1] - s0;
  const int64_t d0 = graph_ptr[blockIdx.x];
  if (!(n > 0 && s0 >= 0 && s0 <= N_all - n && d0 >= 0 && d0 <= N - n && (int64_t)graph_ptr[blockIdx.x + 1] - d0 == n)) return;
  for (int64_t t = threadIdx.x; t < n * K; t += blockDim.x) {
    const int64_t o = ld == K ? t : (t / K) * ld + t % K;
#pragma unroll
    for (int i = 0; i < T; ++i) tab.dst[i][d0 * ld + o] = tab.src[i][s0 * K + t];
  }
}

}  // namespace esc
