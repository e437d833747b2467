// graph_wave.h — the wave-level primitives of the graph-structure kernels (features.hip, subgraphs.hip, multihop.hip, plan.hip;
// DESIGN.md 6o): the segment search, the float4 accessors of pna.hip's lane groups, the ballot-prefix rank, the one-workgroup
// exclusive scan, the level-synchronous BFS in LDS and what one root's wave of the rooted expansions does with it.  Every primitive is the text its callers used to carry, once.
// Below them, the host side that subgraphs.hip and multihop.hip share: the argument check that every count / fill entry opens with
// and the launchers of the per-graph validation and of the two-array scan (the kernels themselves live in subgraphs.hip: a
// kernel has one translation unit).
#pragma once
#include "common.h"
#include "row_walk.h"

namespace esc {

constexpr unsigned char GRAPH_HOP_INF = 255;    // hop[x] of a node the BFS did not reach within its bound
constexpr int GRAPH_RD_MAX = 96;                // largest node set whose two m x m fp64 matrices fit LDS (147 KB): the rd limit

// last g with ptr[g] <= i
__device__ __forceinline__ int find_segment(const int64_t* __restrict__ ptr, int G, int64_t i) {
  int lo = 0, hi = G;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- float4 rows of pna.hip's lane groups (group_locate: row_walk.h) -----------------------------------------------------------------
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// ---- stable ballot-prefix compaction ------------------------------------------------------------------------------------------
// number of set bits of a ballot below this lane: the lane's rank among the lanes that voted
__device__ __forceinline__ int lane_rank(unsigned long long mask) {
  return __popcll(mask & ((1ull << (threadIdx.x & 63)) - 1ull));
}

// the slot of this lane among the voters of pred, counted from base (meaningful where pred holds); base advances past the
// wave's voters.  Every lane of the wave calls it.
template <typename Base>
__device__ __forceinline__ Base ballot_compact(bool pred, Base& base) {
  const unsigned long long msk = __ballot(pred);
  const Base slot = base + lane_rank(msk);
  base += __popcll(msk);
  return slot;
}

// ---- exclusive scan by ONE 1024-thread workgroup: 1024-wide chunks with a carry ---------------------------------------------
// store(i, sum of load(0..i)) for i < n; returns the total in every thread.  carry_s is read by every thread before thread
// 1023 rewrites it: three barriers per chunk, none of them optional (tests/test_hip_feature_structure.py pins the carry).
template <typename T, class Load, class Store>
__device__ __forceinline__ T block_exclusive_scan(int64_t n, Load load, Store store) {
  __shared__ T wsum[16];
  __shared__ T carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const T v = (i < n) ? load(i) : 0;
    T incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const T t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    T woff = 0;
    for (int k = 0; k < w; ++k) woff += wsum[k];
    const T carry = carry_s;
    if (i < n) store(i, carry + woff + incl - v);
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = carry + woff + incl;
    __syncthreads();
  }
  return carry_s;
}

// ---- level-synchronous BFS of one wave over an edge list, hop[] in LDS ---------------------------------------------------------
// edge(j, s, t) -> bool gives the two ends of edge j (graph-local) and whether the walk may use it; the walk goes t -> s.
// Levels 1..h on top of whatever hop[] holds: hop[s] = d for every unreached s with an edge from level d - 1.  Every lane that
// reaches a node in level d writes the same d: the race is benign.
template <class Edge>
__device__ __forceinline__ void wave_bfs_levels(int n_edges, int h, unsigned char* hop, Edge edge) {
  const int lane = threadIdx.x;
  for (int d = 1; d <= h; ++d) {
    int grew = 0;
    for (int j = lane; j < n_edges; j += 64) {
      int s, t;
      if (edge(j, s, t) && hop[t] == d - 1 && hop[s] == GRAPH_HOP_INF) { hop[s] = (unsigned char)d; grew = 1; }
    }
    __syncthreads();
    if (!__any(grew)) break;
  }
}

// hop[x] = d(r, x) over the n nodes of a graph, or GRAPH_HOP_INF beyond h
template <class Edge>
__device__ __forceinline__ void wave_bfs(int n, int r, int n_edges, int h, unsigned char* hop, Edge edge) {
  const int lane = threadIdx.x;
  for (int x = lane; x < n; x += 64) hop[x] = GRAPH_HOP_INF;
  __syncthreads();
  if (lane == 0) hop[r] = 0;
  __syncthreads();
  wave_bfs_levels(n_edges, h, hop, edge);
}

// ---- one root's wave of the rooted expansions (subgraphs.hip, multihop.hip) --------------------------------------------------
// what the wave knows about its graph
struct SubRoot {
  int g, n, r;
  int64_t n0, e0;
  int Eg;
};

__device__ __forceinline__ SubRoot sub_locate(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr, int G,
                                              int64_t r_glob) {
  SubRoot q;
  q.g = find_segment(node_ptr, G, r_glob);
  q.n0 = node_ptr[q.g];
  q.n = (int)(node_ptr[q.g + 1] - q.n0);
  q.r = (int)(r_glob - q.n0);
  q.e0 = edge_ptr[q.g];
  q.Eg = (int)(edge_ptr[q.g + 1] - q.e0);
  return q;
}

// the BFS from q.r over the graph's edge list (global ids, L2 resident), walking dst -> src: multihop.hip hands it (dst, src)
__device__ __forceinline__ void sub_bfs(const SubRoot& q, const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int h,
                                        unsigned char* hop) {
  wave_bfs(q.n, q.r, q.Eg, h, hop, [&](int j, int& s, int& t) {
    s = (int)(src[q.e0 + j] - q.n0); t = (int)(dst[q.e0 + j] - q.n0);
    return true;
  });
}

// canonical positions of the reached nodes: level by level, ascending node id inside a level (the root is the only node of
// level 0).  loc[x] of an unreached node is left alone.  Returns their number.
__device__ __forceinline__ int canonical_positions(const SubRoot& q, int h, const unsigned char* hop, short* loc) {
  const int lane = threadIdx.x;
  int m = 0;
  for (int d = 0; d <= h; ++d) {
    const int before = m;
    for (int x0 = 0; x0 < q.n; x0 += 64) {
      const int x = x0 + lane;
      const bool mine = x < q.n && hop[x] == d;
      const int p = ballot_compact(mine, m);
      if (mine) loc[x] = (short)p;
    }
    if (m == before) break;                                 // an empty level ends the BFS
  }
  return m;
}

// the sub-edges (both ends reached) in their original order, relabelled: edge number p of the root's range goes to
// sub_src / sub_dst[e_at + p] as n_at + loc[.], its global id to orig_edge; kept(s, t) runs once per kept edge, in its lane
template <class Kept>
__device__ __forceinline__ void relabel_sub_edges(const SubRoot& q, const int64_t* __restrict__ src,
                                                  const int64_t* __restrict__ dst, const unsigned char* hop, const short* loc,
                                                  int64_t n_at, int64_t e_at,
                                                  int64_t* __restrict__ sub_src, int64_t* __restrict__ sub_dst,
                                                  int64_t* __restrict__ orig_edge, Kept kept) {
  const int lane = threadIdx.x;
  int base = 0;
  for (int j0 = 0; j0 < q.Eg; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false;
    int s = 0, t = 0;
    if (j < q.Eg) {
      s = (int)(src[q.e0 + j] - q.n0); t = (int)(dst[q.e0 + j] - q.n0);
      keep = hop[s] != GRAPH_HOP_INF && hop[t] != GRAPH_HOP_INF;
    }
    const int slot = ballot_compact(keep, base);
    if (keep) {
      const int64_t p = e_at + slot;
      sub_src[p] = n_at + loc[s]; sub_dst[p] = n_at + loc[t]; orig_edge[p] = q.e0 + j;
      kept(s, t);
    }
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
