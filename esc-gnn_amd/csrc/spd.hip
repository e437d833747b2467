// spd.hip — the all-pairs shortest-path distances behind the graph transformer's attention bias (include/escgnn_spd.h; DESIGN
// 6t): what the reference computes on the host per graph at dataset load with networkx
// (GraphGPS/graphgps/loader/utils_escgnn.py:29-38, all_pairs_shortest_path_length on the undirected graph, 100 where there is no
// path) and stores flattened as the key attn_bias.
//
// esc_graph_spd: one workgroup per graph, one thread per node.
//   1. the edges pass through LDS in chunks of SPD_CHUNK, checked as they are staged (read-only: nothing has been written yet);
//      the thread of node u scans every chunk (all lanes read the same address: a broadcast) and ORs the other end of each of
//      its edges, either direction, into ITS row of the adjacency, held in W = ceil(cap / 64) registers.  Duplicates collapse in
//      the mask and a self-loop sets a bit the search never follows.  No atomics, and no limit on the edges of a graph;
//   2. the rows go to LDS; the thread of source i runs a level-synchronous breadth-first search with the frontier and the seen
//      set in registers (W words each, W a template parameter: 1, 2 or 4), ORs the rows of the frontier's nodes, and stores
//      min(level, 100) for every node a level discovers, then 100 for what was never seen: every byte of the graph is written
//      exactly once, by the thread of its row.
// Integers only: a graph's bytes are a function of the graph.
// esc_spd_gather: one workgroup per graph of the batch copies its n*n bytes of the resident table to the batch's pair_ptr layout.
#include "ragged_graphs.h"
#include "../../include/escgnn_spd.h"

namespace esc {

constexpr int SPD_MAX_NODES = 256;           // 4 words per row; molhiv's largest graph has 222 nodes
constexpr int SPD_CHUNK = 2048;              // edges staged per trip: 8 KiB of 16-bit ends beside at most 8 KiB of adjacency
constexpr int SPD_NO_PATH = 100;             // the reference's fill, and the padding row of its embedding
static_assert(SPD_MAX_NODES >= 256 && SPD_MAX_NODES <= 65535, "the issue's floor; 16-bit ids");

struct SpdArgs {
  const int64_t* src; const int64_t* dst; const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* pair_ptr;
  int64_t N, E, pairs;
  int local, cap;                            // cap: max_nodes as told
  unsigned char* spd;
};

// the bits of word w that stand for nodes below n
__device__ __forceinline__ unsigned long long spd_valid(int n, int w) {
  const int c = n - 64 * w;
  return c <= 0 ? 0ull : c >= 64 ? ~0ull : (1ull << c) - 1ull;
}

template <int W>
__global__ __launch_bounds__(256) void spd_kernel(SpdArgs a) {
  __shared__ unsigned long long adj[64 * W * W];
  __shared__ uint16_t es[SPD_CHUNK], ed[SPD_CHUNK];
  __shared__ int flag;
  const int tid = threadIdx.x;
  const GraphRange r = graph_range(a.node_ptr, a.edge_ptr, blockIdx.x, a.N, a.E);
  // (all of this is uniform over the workgroup: it leaves together)
  if (!(r.ok && r.n1 > r.n0 && r.n1 - r.n0 <= a.cap && r.n1 - r.n0 <= 64 * W)) return;       // empty, or over max_nodes: skipped
  const int n = (int)(r.n1 - r.n0);
  const int64_t m = r.e1 - r.e0, p0 = a.pair_ptr[blockIdx.x];
  if (!(p0 >= 0 && a.pair_ptr[blockIdx.x + 1] - p0 == (int64_t)n * n && p0 <= a.pairs - (int64_t)n * n)) return;
  const int64_t base = a.local ? 0 : r.n0;
  if (tid == 0) flag = 0;
  __syncthreads();
  const int u = tid;                                         // the workgroup has at least 64 * W >= n threads
  unsigned long long row[W];
#pragma unroll
  for (int w = 0; w < W; ++w) row[w] = 0ull;
  for (int64_t c0 = 0; c0 < m; c0 += SPD_CHUNK) {            // 1. check and stage a chunk, then every row takes its edges from it
    const int cnt = (int)(m - c0 < SPD_CHUNK ? m - c0 : SPD_CHUNK);
    for (int e = tid; e < cnt; e += blockDim.x) {
      int64_t s, t;
      if (!edge_ends(a.src, a.dst, r.e0 + c0 + e, base, n, s, t)) flag = 1;      // (plain stores of one value)
      es[e] = (uint16_t)s;
      ed[e] = (uint16_t)t;
    }
    __syncthreads();
    if (u < n) {
      for (int e = 0; e < cnt; ++e) {
        const int s = es[e], t = ed[e];
        const int v = s == u ? t : t == u ? s : -1;          // the other end of an edge of u, either direction (a self-loop: u itself)
#pragma unroll
        for (int w = 0; w < W; ++w) row[w] |= (v >= 0 && (v >> 6) == w) ? 1ull << (v & 63) : 0ull;     // (an end the check refused is
      }                                                      //  compared here, never used as an index)
    }
    __syncthreads();
  }
  if (flag) return;
  if (u < n) {
#pragma unroll
    for (int w = 0; w < W; ++w) adj[u * W + w] = row[w];
  }
  __syncthreads();
  if (u >= n) return;
  // 2. breadth-first from u
  unsigned char* out = a.spd + p0 + (int64_t)u * n;
  unsigned long long seen[W], fr[W];
#pragma unroll
  for (int w = 0; w < W; ++w) seen[w] = fr[w] = (u >> 6) == w ? 1ull << (u & 63) : 0ull;
  out[u] = 0;
  for (int d = 1;; ++d) {
    unsigned long long nx[W];
#pragma unroll
    for (int w = 0; w < W; ++w) nx[w] = 0ull;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      unsigned long long f = fr[w];
      while (f) {
        const int v = 64 * w + __builtin_ctzll(f);
        f &= f - 1ull;
#pragma unroll
        for (int x = 0; x < W; ++x) nx[x] |= adj[v * W + x];
      }
    }
    unsigned long long any = 0ull;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      nx[w] &= ~seen[w];
      seen[w] |= nx[w];
      any |= nx[w];
      fr[w] = nx[w];
    }
    if (!any) break;
    const unsigned char val = (unsigned char)(d < SPD_NO_PATH ? d : SPD_NO_PATH);
#pragma unroll
    for (int w = 0; w < W; ++w) {
      unsigned long long f = nx[w];
      while (f) {
        out[64 * w + __builtin_ctzll(f)] = val;
        f &= f - 1ull;
      }
    }
  }
#pragma unroll
  for (int w = 0; w < W; ++w) {                              // what no level reached
    unsigned long long f = ~seen[w] & spd_valid(n, w);
    while (f) {
      out[64 * w + __builtin_ctzll(f)] = (unsigned char)SPD_NO_PATH;
      f &= f - 1ull;
    }
  }
}

__global__ __launch_bounds__(256) void spd_gather_kernel(const unsigned char* __restrict__ table, const int64_t* __restrict__ pair_ptr_all,
                                                         const int64_t* __restrict__ node_ptr_all, int64_t G_all, int64_t pairs_all,
                                                         const int64_t* __restrict__ ids, const int32_t* __restrict__ graph_ptr,
                                                         const int64_t* __restrict__ pair_ptr, int64_t pairs, unsigned char* __restrict__ out) {
  const int64_t id = ids[blockIdx.x];
  if (id < 0 || id >= G_all) return;
  const int64_t n = node_ptr_all[id + 1] - node_ptr_all[id];
  if (!(n > 0 && n < (1LL << 31) && (int64_t)graph_ptr[blockIdx.x + 1] - graph_ptr[blockIdx.x] == n)) return;
  const int64_t s0 = pair_ptr_all[id], d0 = pair_ptr[blockIdx.x], nn = n * n;
  if (!(s0 >= 0 && pair_ptr_all[id + 1] - s0 == nn && s0 <= pairs_all - nn && d0 >= 0 && pair_ptr[blockIdx.x + 1] - d0 == nn && d0 <= pairs - nn))
    return;
  for (int64_t t = threadIdx.x; t < nn; t += blockDim.x) out[d0 + t] = table[s0 + t];
}

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_graph_spd_max_nodes(void) { return SPD_MAX_NODES; }

int esc_graph_spd(const int64_t* src, const int64_t* dst, int64_t E, const int64_t* node_ptr, const int64_t* edge_ptr,
                  const int64_t* pair_ptr, int64_t G, int64_t N, int64_t pairs, int edges_local, int64_t max_nodes, uint8_t* spd,
                  void* stream) {
  ESC_REQUIRE(G >= 0 && N >= 0 && E >= 0 && G < (1LL << 31) && N < (1LL << 31) && E < (1LL << 31) && pairs >= 0 && max_nodes >= 0,
              "esc_graph_spd: bad sizes G=%ld N=%ld E=%ld pairs=%ld max_nodes=%ld", (long)G, (long)N, (long)E, (long)pairs, (long)max_nodes);
  ESC_REQUIRE(max_nodes <= SPD_MAX_NODES, "esc_graph_spd: a graph of %ld nodes exceeds the limit of %d nodes per graph "
              "(esc_graph_spd_max_nodes)", (long)max_nodes, SPD_MAX_NODES);
  if (G == 0 || N == 0 || max_nodes == 0 || pairs == 0) return ESC_OK;
  ESC_REQUIRE(node_ptr && edge_ptr && pair_ptr && spd && (E == 0 || (src && dst)), "esc_graph_spd: null pointer");
  const SpdArgs a{src, dst, node_ptr, edge_ptr, pair_ptr, N, E, pairs, edges_local ? 1 : 0, (int)max_nodes, (unsigned char*)spd};
  const dim3 grid((unsigned)G);
  if (max_nodes <= 64) esc::launch(-1, spd_kernel<1>, grid, dim3(64), 0, (hipStream_t)stream, a);
  else if (max_nodes <= 128) esc::launch(-1, spd_kernel<2>, grid, dim3(128), 0, (hipStream_t)stream, a);
  else esc::launch(-1, spd_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, a);
  ESC_CHECK_LAUNCH("esc_graph_spd");
  return ESC_OK;
}

int esc_spd_gather(const uint8_t* table, const int64_t* pair_ptr_all, const int64_t* node_ptr_all, int64_t G_all, int64_t pairs_all,
                   const int64_t* graph_ids, const int32_t* graph_ptr, const int64_t* pair_ptr, int64_t B, int64_t pairs,
                   uint8_t* out, void* stream) {
  ESC_REQUIRE(G_all >= 0 && pairs_all >= 0 && B >= 0 && pairs >= 0 && B < (1LL << 31) && G_all < (1LL << 31),
              "esc_spd_gather: bad sizes G_all=%ld pairs_all=%ld B=%ld pairs=%ld", (long)G_all, (long)pairs_all, (long)B, (long)pairs);
  if (B == 0 || pairs == 0 || G_all == 0 || pairs_all == 0) return ESC_OK;
  ESC_REQUIRE(table && pair_ptr_all && node_ptr_all && graph_ids && graph_ptr && pair_ptr && out, "esc_spd_gather: null pointer");
  esc::launch(-1, spd_gather_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, (const unsigned char*)table, pair_ptr_all, node_ptr_all,
              G_all, pairs_all, graph_ids, graph_ptr, pair_ptr, pairs, (unsigned char*)out);
  ESC_CHECK_LAUNCH("esc_spd_gather");
  return ESC_OK;
}

}  // extern "C"
