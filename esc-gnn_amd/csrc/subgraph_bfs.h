// subgraph_bfs.h — what one root's wave of csrc/subgraphs.hip knows and does, shared with csrc/multihop.hip: the graph of a
// root, the level-synchronous BFS in LDS (moved here unchanged), the argument check that every count / fill entry of both
// files opens with, and the host launchers of the per-graph validation and of the two-array scan (the kernels themselves
// live in subgraphs.hip: a kernel has one translation unit).
#pragma once
#include "common.h"

namespace esc {

constexpr unsigned char SUB_INF = 255;

// last g with ptr[g] <= i
__device__ __forceinline__ int sub_find_segment(const int64_t* __restrict__ ptr, int G, int64_t i) {
  int lo = 0, hi = G;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// what one root's wave knows about its graph
struct SubRoot {
  int g, n, r;
  int64_t n0, e0;
  int Eg;
};

__device__ __forceinline__ SubRoot sub_locate(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr, int G,
                                              int64_t r_glob) {
  SubRoot q;
  q.g = sub_find_segment(node_ptr, G, r_glob);
  q.n0 = node_ptr[q.g];
  q.n = (int)(node_ptr[q.g + 1] - q.n0);
  q.r = (int)(r_glob - q.n0);
  q.e0 = edge_ptr[q.g];
  q.Eg = (int)(edge_ptr[q.g + 1] - q.e0);
  return q;
}

// level-synchronous BFS from q.r over the graph's edge list (global ids, L2 resident); hop[x] = d(r, x) or SUB_INF beyond h.
// Every lane that reaches a node in level d writes the same d: the race is benign.
__device__ __forceinline__ void sub_bfs(const SubRoot& q, const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int h,
                                        unsigned char* hop) {
  const int lane = threadIdx.x;
  for (int x = lane; x < q.n; x += 64) hop[x] = SUB_INF;
  __syncthreads();
  if (lane == 0) hop[q.r] = 0;
  __syncthreads();
  for (int d = 1; d <= h; ++d) {
    int grew = 0;
    for (int j = lane; j < q.Eg; j += 64) {
      const int s = (int)(src[q.e0 + j] - q.n0), t = (int)(dst[q.e0 + j] - q.n0);
      if (hop[t] == d - 1 && hop[s] == SUB_INF) { hop[s] = (unsigned char)d; grew = 1; }
    }
    __syncthreads();
    if (!__any(grew)) break;
  }
}

// ---- host side: what every count / fill entry of the expansions opens with ---------------------------------------------------
struct ExpandLimits {
  const char* depth_name;               // "h" | "k"
  int depth_max, max_nodes;
  const char* why;                      // the clause behind "outside 1..depth_max", or ""
  bool ranges_first;                    // the second-root entries test their ranges before the pointers
};

inline int expand_check(const ExpandLimits& L, const char* fn, const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src,
                        const int64_t* dst, int64_t G, int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int depth) {
  for (int pass = 0; pass < 2; ++pass) {                    // the ranges and the pointers, in the order the entry has always had
    if ((pass == 0) == L.ranges_first) {
      if (depth < 1 || depth > L.depth_max) {
        set_error("%s: %s=%d outside 1..%d%s", fn, L.depth_name, depth, L.depth_max, L.why);
        return ESC_ERANGE;
      }
      if (max_nodes < 1 || max_nodes > L.max_nodes) {
        set_error("%s: max_nodes=%ld outside 1..%d", fn, (long)max_nodes, L.max_nodes);
        return ESC_ERANGE;
      }
    } else {
      ESC_REQUIRE(node_ptr && edge_ptr, "%s: null pointer", fn);
      ESC_REQUIRE((src && dst) || total_edges == 0, "%s: null edge arrays", fn);
      ESC_REQUIRE(G > 0 && G < (1LL << 31), "%s: bad graph count %ld", fn, (long)G);
    }
  }
  if (total_nodes < 0 || total_edges < 0 || total_nodes >= (1LL << 31) - 1 || total_edges >= (1LL << 31) - 1) {
    set_error("%s: %ld nodes / %ld edges: totals must stay below 2^31", fn, (long)total_nodes, (long)total_edges);
    return ESC_ERANGE;
  }
  return ESC_OK;
}

// sub_validate_kernel (one wave per graph): status[g] = ESC_ERANGE for a graph whose ranges do not tile the arrays, of more
// than max_nodes nodes, or with an edge that leaves it; 0 otherwise
void sub_launch_validate(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                         int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int* status, hipStream_t s);
// sub_scan_kernel: in-place exclusive scans of the int64 counts a0[0..n) and a1[0..n); the totals go to a0[n] and a1[n]
void sub_launch_scan(int64_t* a0, int64_t* a1, int64_t n, hipStream_t s);

}  // namespace esc
