// subgraphs.hip — node-rooted h-hop subgraph expansion of a collated batch (the NGNN baseline's pre_transform) on the GPU.
//
// Replaces create_subgraphs / k_hop_subgraph of the reference's utils.py:18-132,135-229: a python loop over every node with
// a tensor-mask BFS, a relabel and a scipy pinv per root, run once per dataset on the host.  Here the expansion runs per
// batch on the device, so there is no pre-processed dataset and no host collate of subgraphs.
//
// Semantics restated:
//   * S_r = nodes within h hops of r walking target -> source (`col, row = edge_index`, :145), as feat_bfs_kernel does
//   * sub-edges = ALL edges with both endpoints in S_r, in their original order; self loops and repeats kept (:218-222)
//   * hop label z = hop + 1 (:154,:167)
//   * the label LIST of a node gets one entry per frontier edge that reaches it in its level (:163-167 test `visited`, which
//     only grows after the level), so a node with two or more such edges carries the label twice: `paths` counts them
//     (0 for the root) and the python layer forms the reference's spd / drnl columns from (z, paths)
//   * rd[i] = P[0,0] + P[i,i] - P[0,i] - P[i,0], P = pinv(D_in - A) over the non-loop sub-edges, fp64 -> fp32 (:59-74)
//
// Canonical order (the contract): the sub-nodes of r are the root, then ascending (hop, node id).  The reference's
// order inside a level is the iteration order of a CPython set; the model does not depend on it.
//
// One wave per root, twice: the count pass sizes the output, the fill pass repeats the BFS (cheaper than keeping n^2 hop
// tables between the passes) and writes with stable ballot-prefix compaction.  Integer work bound by LDS / L2 latency.
//
// The second half of the file is the I2GNN baseline's expansion (esc_subgraph2_count / _fill, include/escgnn_i2gnn.h): the same
// subgraphs, once per neighbour of their root, labelled with the distances to both.  Both halves are written on the primitives
// of graph_wave.h (BFS, canonical positions, sub-edge compaction, the scan) and of jacobi_pinv.h (the Laplacian, its
// pseudo-inverse, the resistance distance).
#include "common.h"
#include "graph_wave.h"
#include "jacobi_pinv.h"
#include "../../include/escgnn_subgraphs.h"
#include "../../include/escgnn_i2gnn.h"

namespace esc {

constexpr int SUB_MAX_NODES = 4096;     // 7 B of LDS tables per node (see sub_fill_lds)
constexpr int SUB_H_MAX = 98;           // z = hop + 1 and the model's z tables have 100 rows
// (GRAPH_HOP_INF, GRAPH_RD_MAX, SubRoot, sub_locate and sub_bfs: graph_wave.h, shared with multihop.hip)

// ---- per-graph validation (one wave per graph): ids inside the graph, graph inside the LDS tables -----------------
__global__ __launch_bounds__(64) void sub_validate_kernel(const int64_t* __restrict__ node_ptr,
                                                          const int64_t* __restrict__ edge_ptr,
                                                          const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                          int G, int64_t total_nodes, int64_t total_edges, int64_t max_nodes,
                                                          int* __restrict__ status) {
  const int g = blockIdx.x;
  if (g >= G) return;
  const int lane = threadIdx.x;
  const int64_t n0 = node_ptr[g], n1 = node_ptr[g + 1], e0 = edge_ptr[g], e1 = edge_ptr[g + 1];
  int bad = 0;
  // per graph: ordered and inside the arrays; the first and the last also pin the ends, so that together the ranges tile
  // [0, total) and every root falls inside the graph find_segment gives it (a root of a refused graph is skipped)
  const bool ends = (g > 0 || (n0 == 0 && e0 == 0)) && (g < G - 1 || (n1 == total_nodes && e1 == total_edges));
  if (!ends || n0 < 0 || n1 < n0 || n1 > total_nodes || n1 - n0 > max_nodes || e0 < 0 || e1 < e0 || e1 > total_edges) {
    bad = 1;
  } else {
    for (int64_t j = e0 + lane; j < e1; j += 64) {
      const int64_t s = src[j], d = dst[j];
      if (s < n0 || s >= n1 || d < n0 || d >= n1) bad = 1;
    }
  }
  bad = __any(bad) ? 1 : 0;
  if (lane == 0) status[g] = bad ? ESC_ERANGE : 0;
}

// ---- count pass: |S_r| and the number of sub-edges of every root, left in the pointer arrays for the scan.  SECOND (the
// I2GNN expansion, second half of the file): a root has one copy of its subgraph per neighbour, and cnt_s2 takes that number ----
template <bool SECOND>
__global__ __launch_bounds__(64) void sub_count_kernel(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ edge_ptr,
                                                       const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int G,
                                                       int64_t total_nodes, int h, const int* __restrict__ status,
                                                       int64_t* __restrict__ cnt_nodes, int64_t* __restrict__ cnt_edges,
                                                       int64_t* __restrict__ cnt_s2) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const int64_t r_glob = blockIdx.x;
  if (r_glob >= total_nodes) return;
  const SubRoot q = sub_locate(node_ptr, edge_ptr, G, r_glob);
  if (status[q.g] != 0) {
    if (lane == 0) { cnt_nodes[r_glob] = 0; cnt_edges[r_glob] = 0; if (SECOND) cnt_s2[r_glob] = 0; }
    return;
  }
  unsigned char* hop = smem;
  sub_bfs(q, src, dst, h, hop);
  int nn = 0, ne = 0, nk = 0;
  for (int x0 = 0; x0 < q.n; x0 += 64) {
    const int x = x0 + lane;
    nn += __popcll(__ballot(x < q.n && hop[x] != GRAPH_HOP_INF));
  }
  for (int j0 = 0; j0 < q.Eg; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false, nb = false;
    if (j < q.Eg) {
      const int s = (int)(src[q.e0 + j] - q.n0);
      keep = hop[s] != GRAPH_HOP_INF && hop[dst[q.e0 + j] - q.n0] != GRAPH_HOP_INF;
      nb = keep && s == q.r;
    }
    ne += __popcll(__ballot(keep));
    if (SECOND) nk += __popcll(__ballot(nb));
  }
  const int64_t mult = nk > 0 ? nk : 1;
  if (lane == 0) { cnt_nodes[r_glob] = mult * nn; cnt_edges[r_glob] = mult * ne; if (SECOND) cnt_s2[r_glob] = mult; }
}

// ---- in-place exclusive scan of int64 counts (block_exclusive_scan); blockIdx.x picks the array ------------------------------
__global__ __launch_bounds__(1024) void sub_scan_kernel(int64_t* __restrict__ a0, int64_t* __restrict__ a1, int64_t n) {
  int64_t* __restrict__ buf = blockIdx.x == 0 ? a0 : a1;
  const int64_t total = block_exclusive_scan<int64_t>(n, [&](int64_t i) { return buf[i]; }, [&](int64_t i, int64_t v) { buf[i] = v; });
  if (threadIdx.x == 0) buf[n] = total;
}

// ---- rd of both fill kernels: P = pinv(D_in - A) over the non-loop sub-edges of S_r, m nodes at their canonical positions.
// mem: Gm[ld*ld] Vm[ld*ld] inv_s2[ld] vrow[ld] red[8] doubles of LDS.  Returns P, P[i][j] at P[j*ld + i] --------------------------
__device__ __forceinline__ const double* sub_rooted_pinv(const SubRoot& q, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                         const unsigned char* hop, const short* loc, int m, int ld, unsigned char* mem) {
  double* Gm = reinterpret_cast<double*>(mem);
  double* Vm = Gm + (size_t)ld * ld;
  double* inv_s2 = Vm + (size_t)ld * ld;
  double* vrow = inv_s2 + ld;
  double* red = vrow + ld;
  laplacian_clear<64>(Gm, Vm, m, ld);
  __syncthreads();
  for (int j = threadIdx.x; j < q.Eg; j += 64) {
    const int s = (int)(src[q.e0 + j] - q.n0), t = (int)(dst[q.e0 + j] - q.n0);
    if (s == t || hop[s] == GRAPH_HOP_INF || hop[t] == GRAPH_HOP_INF) continue;
    laplacian_add_edge(Gm, ld, loc[s], loc[t]);
  }
  __syncthreads();
  const double null2 = jacobi_orthogonalise<64>(Gm, Vm, m, ld, red);
  __syncthreads();
  pinv_from_jacobi<64>(Gm, Vm, m, ld, null2, inv_s2, vrow);
  return Vm;
}

// ---- fill pass ------------------------------------------------------------------------------------------------------
struct SubFillArgs {
  const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* src; const int64_t* dst;
  const int64_t* sub_node_ptr; const int64_t* sub_edge_ptr;
  int64_t* orig_node; int64_t* hop_label; int64_t* hop_paths; int64_t* node_to_subgraph; int64_t* node_to_graph;
  int64_t* sub_src; int64_t* sub_dst; int64_t* orig_edge;
  float* rd;
  int* status;
  int64_t total_nodes, total_sub_nodes, total_sub_edges;
  int G, h, n_cap, ld;
};

// LDS: hop[n_cap] bytes | loc[n_cap] shorts | paths[n_cap] ints; (RD) Gm[ld*ld] Vm[ld*ld] inv_s2[ld] vrow[ld] red[8] doubles
// start where `paths` did — it is dead once the node rows are written (4096-node graphs with ld = 96: 158 KB of the 160)
template <bool RD>
__global__ __launch_bounds__(64) void sub_fill_kernel(SubFillArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  const int64_t r_glob = blockIdx.x;
  if (r_glob >= a.total_nodes) return;
  const SubRoot q = sub_locate(a.node_ptr, a.edge_ptr, a.G, r_glob);
  // a graph the count pass refused has zero-length ranges (a valid root holds at least itself).  `status` is not read here:
  // another root of this graph may be setting it for an rd overflow, which must not silence this one
  if (a.sub_node_ptr[r_glob + 1] == a.sub_node_ptr[r_glob]) return;
  if (a.sub_node_ptr[r_glob + 1] > a.total_sub_nodes || a.sub_edge_ptr[r_glob + 1] > a.total_sub_edges) {
    if (threadIdx.x == 0) a.status[q.g] = ESC_ERANGE;       // the caller's totals are not those of the count pass: write nothing
    return;
  }
  unsigned char* hop = smem;                                // [n_cap]
  short* loc = reinterpret_cast<short*>(hop + a.n_cap);     // [n_cap]
  int* paths = reinterpret_cast<int*>(loc + a.n_cap);       // [n_cap]
  sub_bfs(q, a.src, a.dst, a.h, hop);
  const int m = canonical_positions(q, a.h, hop, loc);
  for (int x = lane; x < q.n; x += 64) { paths[x] = 0; if (hop[x] == GRAPH_HOP_INF) loc[x] = -1; }
  __syncthreads();
  const int64_t sn0 = a.sub_node_ptr[r_glob], se0 = a.sub_edge_ptr[r_glob];
  // sub-edges in their original order, relabelled to global sub-node ids; and the frontier edges into every node
  relabel_sub_edges(q, a.src, a.dst, hop, loc, sn0, se0, a.sub_src, a.sub_dst, a.orig_edge,
                    [&](int s, int t) { if ((int)hop[t] + 1 == (int)hop[s]) atomicAdd(&paths[s], 1); });
  __syncthreads();
  for (int x = lane; x < q.n; x += 64) {
    if (hop[x] == GRAPH_HOP_INF) continue;
    const int64_t p = sn0 + loc[x];
    a.orig_node[p] = q.n0 + x; a.hop_label[p] = (int64_t)hop[x] + 1; a.hop_paths[p] = paths[x];
    a.node_to_subgraph[p] = r_glob; a.node_to_graph[p] = q.g;
  }
  if (!RD) return;
  if (m > GRAPH_RD_MAX || m > a.ld) {                       // wave-uniform
    if (lane == 0) a.status[q.g] = ESC_ERANGE;
    return;
  }
  const int ld = a.ld;
  __syncthreads();                                          // `paths` has been read: the matrices take its place
  const size_t off = ((size_t)a.n_cap * 3 + 15) & ~(size_t)15;
  const double* P = sub_rooted_pinv(q, a.src, a.dst, hop, loc, m, ld, smem + off);
  for (int i = lane; i < m; i += 64) a.rd[sn0 + i] = (float)resistance(P, ld, 0, i);   // lxx + lyy - lxy - lyx (:73), the root is local node 0: 0 there
}

// ---- subgraph_pooling = 'center': the first row of every segment ---------------------------------------------------------
__global__ __launch_bounds__(256) void segment_first_fwd_kernel(const float* __restrict__ x, int64_t ld_x,
                                                                const int64_t* __restrict__ ptr, int64_t S, int64_t C,
                                                                float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= S * C) return;
  const int64_t s = i / C, c = i - s * C;
  const int64_t first = ptr[s];
  out[i] = first < ptr[s + 1] ? x[first * ld_x + c] : 0.f;  // (an empty segment has no first row)
}

// every row of dx is written: the gradient on a segment's first row, zero elsewhere — no memset, no atomics
__global__ __launch_bounds__(256) void segment_first_bwd_kernel(const float* __restrict__ dout, int64_t ld_dout,
                                                                const int64_t* __restrict__ ptr,
                                                                const int64_t* __restrict__ node_to_segment, int64_t N,
                                                                int64_t C, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int64_t row = i / C, c = i - row * C;
  const int64_t s = node_to_segment[row];
  dx[i] = ptr[s] == row ? dout[s * ld_dout + c] : 0.f;
}

static size_t sub_fill_lds(int n_cap, int ld, bool rd) {
  const size_t plain = ((size_t)n_cap * 7 + 15) & ~(size_t)15;
  if (!rd) return plain;
  const size_t with_rd = (((size_t)n_cap * 3 + 15) & ~(size_t)15) + ((size_t)2 * ld * ld + 2 * (size_t)ld + 8) * 8;
  return with_rd > plain ? with_rd : plain;
}

static const ExpandLimits SUB_LIMITS = {"h", SUB_H_MAX, SUB_MAX_NODES, " (the model's z tables have 100 rows and z = hop + 1)", false};

// ---- what the fill entries of both rooted expansions derive from their arguments -------------------------------------------
static bool sub_totals_ok(int64_t total_sub_nodes, int64_t total_sub_edges) {
  return total_sub_nodes >= 0 && total_sub_edges >= 0 && total_sub_nodes < (1LL << 31) - 1 && total_sub_edges < (1LL << 31) - 1;
}
static int sub_n_cap(int64_t max_nodes) { return (int)((max_nodes + 3) & ~3LL); }
static int sub_rd_ld(int64_t max_nodes) {
  const int m_even = (int)((max_nodes + 1) & ~1LL);
  return m_even < GRAPH_RD_MAX ? m_even : GRAPH_RD_MAX;
}
// one wave per root; the rd variant may need more dynamic LDS than the default 64 KB
template <typename FillArgs>
static void sub_launch_fill(void (*with_rd)(FillArgs), void (*without_rd)(FillArgs), int use_rd, size_t lds, hipStream_t s, const FillArgs& a) {
  if (use_rd && lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)with_rd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  esc::launch(ESC_K_FEATURES, use_rd ? with_rd : without_rd, dim3((unsigned)a.total_nodes), dim3(64), lds, s, a);
}

// the two kernels above that multihop.hip launches as well (graph_wave.h)
void sub_launch_validate(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                         int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int* status, hipStream_t s) {
  esc::launch(ESC_K_FEATURES, sub_validate_kernel, dim3((unsigned)G), dim3(64), 0, s, node_ptr, edge_ptr, src, dst, (int)G, total_nodes,
              total_edges, max_nodes, status);
}
void sub_launch_scan(int64_t* a0, int64_t* a1, int64_t n, hipStream_t s) {
  esc::launch(ESC_K_FEATURES, sub_scan_kernel, dim3(2), dim3(1024), 0, s, a0, a1, n);
}

// ===== the I2GNN baseline: every rooted subgraph once per neighbour of its root (reference utils_edge_I2.py:132-256, 726-813;
// DESIGN.md 6i).  S_r is the subgraph above; the neighbours of r are the targets of the sub-edges whose source is r, in
// sub-edge order (repeats and a self loop kept); copy c labels every node with its distances to r and to the c-th
// neighbour j.  The distances to j come from an unbounded BFS inside S_r (find_all_spd :475-561).  A root with no
// neighbour has one copy whose second label pair and second rd column repeat the first.
constexpr int SUB2_MAX_NODES = 1536;    // 9 B of LDS tables per node beside the two 96 x 96 fp64 matrices (see sub2_fill_lds)
constexpr int SUB2_H_MAX = 47;          // the largest label is 2h + 5 and the model's z tables have 100 rows

struct Sub2FillArgs {
  const int64_t* node_ptr; const int64_t* edge_ptr; const int64_t* src; const int64_t* dst;
  const int64_t* sub_node_ptr; const int64_t* sub_edge_ptr; const int64_t* sub2_ptr;
  int64_t* orig_node; int64_t* z; int64_t* node_to_subgraph2; int64_t* node_to_graph;
  int64_t* sub_src; int64_t* sub_dst; int64_t* orig_edge;
  int64_t* subgraph2_to_subgraph; int64_t* center_idx; int64_t* s2_node_ptr;
  float* rd;
  int* status;
  int64_t total_nodes, total_sub_nodes, total_sub_edges, total_s2;
  int G, h, n_cap, ld;
};

// LDS: hop[n_cap] two[n_cap] hopj[n_cap] bytes | loc[n_cap] shorts | cnt[n_cap] ints; (RD) Gm[ld*ld] Vm[ld*ld] inv_s2[ld] vrow[ld]
// red[8] doubles behind them: the pseudo-inverse stays alive for every copy, so nothing is overlaid
template <bool RD>
__global__ __launch_bounds__(64) void sub2_fill_kernel(Sub2FillArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int jsel;
  const int lane = threadIdx.x;
  const int64_t r_glob = blockIdx.x;
  if (r_glob >= a.total_nodes) return;
  if (r_glob == 0 && lane == 0) a.s2_node_ptr[0] = 0;       // every other entry is the end of a copy, written by its root
  const SubRoot q = sub_locate(a.node_ptr, a.edge_ptr, a.G, r_glob);
  const int64_t sn0 = a.sub_node_ptr[r_glob], se0 = a.sub_edge_ptr[r_glob], s20 = a.sub2_ptr[r_glob];
  if (a.sub_node_ptr[r_glob + 1] == sn0) return;            // a graph the count pass refused (see sub_fill_kernel)
  if (a.sub_node_ptr[r_glob + 1] > a.total_sub_nodes || a.sub_edge_ptr[r_glob + 1] > a.total_sub_edges ||
      a.sub2_ptr[r_glob + 1] > a.total_s2) {
    if (lane == 0) a.status[q.g] = ESC_ERANGE;              // the caller's totals are not those of the count pass: write nothing
    return;
  }
  unsigned char* hop = smem;                                // [n_cap] distance to the root
  unsigned char* two = hop + a.n_cap;                       // [n_cap] two or more frontier edges into the node (root's BFS)
  unsigned char* hopj = two + a.n_cap;                      // [n_cap] distance to the neighbour, inside S_r
  short* loc = reinterpret_cast<short*>(hopj + a.n_cap);    // [n_cap]
  int* cnt = reinterpret_cast<int*>(loc + a.n_cap);         // [n_cap] frontier edges into the node, of the BFS at hand
  sub_bfs(q, a.src, a.dst, a.h, hop);
  const int m = canonical_positions(q, a.h, hop, loc);
  for (int x = lane; x < q.n; x += 64) { cnt[x] = 0; if (hop[x] == GRAPH_HOP_INF) loc[x] = -1; }
  __syncthreads();
  int e = 0, K = 0;
  for (int j0 = 0; j0 < q.Eg; j0 += 64) {
    const int j = j0 + lane;
    bool keep = false, nb = false;
    if (j < q.Eg) {
      const int s = (int)(a.src[q.e0 + j] - q.n0), t = (int)(a.dst[q.e0 + j] - q.n0);
      keep = hop[s] != GRAPH_HOP_INF && hop[t] != GRAPH_HOP_INF;
      nb = keep && s == q.r;
      if (keep && (int)hop[t] + 1 == (int)hop[s]) atomicAdd(&cnt[s], 1);
    }
    e += __popcll(__ballot(keep));
    K += __popcll(__ballot(nb));
  }
  __syncthreads();
  for (int x = lane; x < q.n; x += 64) two[x] = cnt[x] >= 2 ? 1 : 0;
  const int mult = K > 0 ? K : 1;
  if ((int64_t)mult * m != a.sub_node_ptr[r_glob + 1] - sn0 || (int64_t)mult * e != a.sub_edge_ptr[r_glob + 1] - se0 ||
      (int64_t)mult != a.sub2_ptr[r_glob + 1] - s20) {      // wave-uniform: pointers that the count pass did not make
    if (lane == 0) a.status[q.g] = ESC_ERANGE;
    return;
  }
  bool rd_ok = RD;
  const int ld = a.ld;
  const double* P = nullptr;                                // P[i][j] at P[j*ld + i]; the root is local node 0
  if (RD) {
    if (m > GRAPH_RD_MAX || m > ld) {                       // wave-uniform; the rd rows of this root stay unwritten
      if (lane == 0) a.status[q.g] = ESC_ERANGE;
      rd_ok = false;
    } else {
      P = sub_rooted_pinv(q, a.src, a.dst, hop, loc, m, ld, smem + (((size_t)a.n_cap * 9 + 15) & ~(size_t)15));
    }
  }
  __syncthreads();
  for (int c = 0; c < mult; ++c) {
    const int64_t n_at = sn0 + (int64_t)c * m, e_at = se0 + (int64_t)c * e;
    int jx = q.r;
    if (K > 0) {
      // the c-th neighbour: target of the c-th sub-edge that leaves the root
      int base = 0;
      for (int j0 = 0; j0 < q.Eg && base <= c; j0 += 64) {
        const int j = j0 + lane;
        bool nb = false;
        int t = 0;
        if (j < q.Eg) {
          t = (int)(a.dst[q.e0 + j] - q.n0);
          nb = (int)(a.src[q.e0 + j] - q.n0) == q.r && hop[t] != GRAPH_HOP_INF;
        }
        const int p = ballot_compact(nb, base);
        if (nb && p == c) jsel = t;
      }
      for (int x = lane; x < q.n; x += 64) { hopj[x] = GRAPH_HOP_INF; cnt[x] = 0; }
      __syncthreads();
      jx = jsel;
      if (lane == 0) hopj[jx] = 0;
      __syncthreads();
      // the reference's unbounded BFS from the neighbour over the sub-edges only, target -> source.  It ends within h + 1
      // levels on any graph: the sub-edge r -> j puts r at distance 1 of j, and every node of S_r reaches r inside S_r in
      // hop <= h steps, so d_j <= h + 1, every node of S_r is reached and the largest label is (h + 2) + (h + 3) <= 99
      wave_bfs_levels(q.Eg, a.h + 1, hopj, [&](int j, int& s, int& t) {
        s = (int)(a.src[q.e0 + j] - q.n0); t = (int)(a.dst[q.e0 + j] - q.n0);
        return hop[s] != GRAPH_HOP_INF;
      });
      for (int j = lane; j < q.Eg; j += 64) {
        const int s = (int)(a.src[q.e0 + j] - q.n0), t = (int)(a.dst[q.e0 + j] - q.n0);
        if (hop[s] != GRAPH_HOP_INF && hopj[t] != GRAPH_HOP_INF && (int)hopj[t] + 1 == (int)hopj[s]) atomicAdd(&cnt[s], 1);
      }
      __syncthreads();
    }
    const int lj = loc[jx];
    const int64_t shift = a.h + 3;
    for (int x = lane; x < q.n; x += 64) {
      if (hop[x] == GRAPH_HOP_INF) continue;
      const int k = loc[x];
      const int64_t p = n_at + k;
      const int64_t z0 = (int64_t)hop[x] + 1, z1 = two[x] ? z0 : 0;
      int64_t z2 = z0, z3 = z1;                             // no neighbour: the root's pair tiled twice
      if (K > 0) {
        const int64_t dj = hopj[x] == GRAPH_HOP_INF ? 0 : (int64_t)hopj[x] + 1;
        z2 = dj + shift; z3 = (cnt[x] >= 2 ? dj : 0) + shift;
      }
      a.orig_node[p] = q.n0 + x;
      a.z[4 * p] = z0; a.z[4 * p + 1] = z1; a.z[4 * p + 2] = z2; a.z[4 * p + 3] = z3;
      a.node_to_subgraph2[p] = s20 + c; a.node_to_graph[p] = q.g;
      if (RD && rd_ok) {
        a.rd[2 * p] = (float)resistance(P, ld, 0, k); a.rd[2 * p + 1] = (float)resistance(P, ld, lj, k);
      }
    }
    relabel_sub_edges(q, a.src, a.dst, hop, loc, n_at, e_at, a.sub_src, a.sub_dst, a.orig_edge, [](int, int) {});
    if (lane == 0) {
      a.subgraph2_to_subgraph[s20 + c] = r_glob;
      a.center_idx[2 * (s20 + c)] = n_at; a.center_idx[2 * (s20 + c) + 1] = n_at + lj;
      a.s2_node_ptr[s20 + c + 1] = n_at + m;
    }
    __syncthreads();                                        // hopj / cnt / jsel are rewritten by the next copy
  }
}

static size_t sub2_fill_lds(int n_cap, int ld, bool rd) {
  const size_t tables = ((size_t)n_cap * 9 + 15) & ~(size_t)15;
  return rd ? tables + ((size_t)2 * ld * ld + 2 * (size_t)ld + 8) * 8 : tables;
}

static const ExpandLimits SUB2_LIMITS = {"h", SUB2_H_MAX, SUB2_MAX_NODES,
                                         " (the model's z tables have 100 rows and the second root's labels reach 2h + 5)", true};

// ---- the count pass of both rooted expansions: validation, one wave per root (LDS: hop[n_cap]), the scans.  sub2_ptr: the
// second-root expansion's third count, or NULL ---------------------------------------------------------------------------------
static int sub_launched(const char* fn, const char* step) {
  const hipError_t err = hipGetLastError();
  if (err == hipSuccess) return ESC_OK;
  set_error("%s.%s: launch failed: %s", fn, step, hipGetErrorString(err));
  return ESC_ELAUNCH;
}

static int sub_count_pass(const char* fn, const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst,
                          int64_t G, int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, int64_t* sub_node_ptr,
                          int64_t* sub_edge_ptr, int64_t* sub2_ptr, int32_t* status, hipStream_t s) {
  sub_launch_validate(node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, status, s);
  if (const int rc = sub_launched(fn, "validate")) return rc;
  if (total_nodes > 0) {
    const dim3 grid((unsigned)total_nodes);
    const size_t n_cap = (size_t)sub_n_cap(max_nodes);
    esc::launch(ESC_K_FEATURES, sub2_ptr ? sub_count_kernel<true> : sub_count_kernel<false>, grid, dim3(64), n_cap, s, node_ptr, edge_ptr,
                src, dst, (int)G, total_nodes, h, (const int*)status, sub_node_ptr, sub_edge_ptr, sub2_ptr);
    if (const int rc = sub_launched(fn, "count")) return rc;
  }
  sub_launch_scan(sub_node_ptr, sub_edge_ptr, total_nodes, s);
  if (sub2_ptr) esc::launch(ESC_K_FEATURES, sub_scan_kernel, dim3(1), dim3(1024), 0, s, sub2_ptr, sub2_ptr, total_nodes);
  return sub_launched(fn, "scan");
}

}  // namespace esc

using namespace esc;

extern "C" {

int esc_subgraph_count(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                       int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, int64_t* sub_node_ptr,
                       int64_t* sub_edge_ptr, int32_t* status, void* stream) {
  const int rc = expand_check(SUB_LIMITS, "esc_subgraph_count", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, h);
  if (rc) return rc;
  ESC_REQUIRE(sub_node_ptr && sub_edge_ptr && status, "esc_subgraph_count: null output");
  return sub_count_pass("esc_subgraph_count", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, h, sub_node_ptr,
                        sub_edge_ptr, nullptr, status, (hipStream_t)stream);
}

int esc_subgraph_fill(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                      int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, const int64_t* sub_node_ptr,
                      const int64_t* sub_edge_ptr, int64_t total_sub_nodes, int64_t total_sub_edges, int use_rd,
                      int64_t* orig_node, int64_t* hop_label, int64_t* hop_paths, int64_t* node_to_subgraph,
                      int64_t* node_to_graph, int64_t* sub_src, int64_t* sub_dst, int64_t* orig_edge, float* rd,
                      int32_t* status, void* stream) {
  const int rc = expand_check(SUB_LIMITS, "esc_subgraph_fill", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, h);
  if (rc) return rc;
  ESC_REQUIRE(sub_node_ptr && sub_edge_ptr && status, "esc_subgraph_fill: null pointer");
  if (!sub_totals_ok(total_sub_nodes, total_sub_edges)) {
    set_error("esc_subgraph_fill: %ld sub-nodes / %ld sub-edges: totals must stay below 2^31", (long)total_sub_nodes,
              (long)total_sub_edges);
    return ESC_ERANGE;
  }
  if (total_nodes == 0 || total_sub_nodes == 0) return ESC_OK;
  ESC_REQUIRE(orig_node && hop_label && hop_paths && node_to_subgraph && node_to_graph, "esc_subgraph_fill: null node output");
  ESC_REQUIRE((sub_src && sub_dst && orig_edge) || total_sub_edges == 0, "esc_subgraph_fill: null edge output");
  ESC_REQUIRE(!use_rd || rd, "esc_subgraph_fill: use_rd without an rd output");
  SubFillArgs a{};
  a.node_ptr = node_ptr; a.edge_ptr = edge_ptr; a.src = src; a.dst = dst; a.sub_node_ptr = sub_node_ptr; a.sub_edge_ptr = sub_edge_ptr;
  a.orig_node = orig_node; a.hop_label = hop_label; a.hop_paths = hop_paths; a.node_to_subgraph = node_to_subgraph;
  a.node_to_graph = node_to_graph; a.sub_src = sub_src; a.sub_dst = sub_dst; a.orig_edge = orig_edge; a.rd = rd; a.status = status;
  a.total_nodes = total_nodes; a.total_sub_nodes = total_sub_nodes; a.total_sub_edges = total_sub_edges; a.G = (int)G; a.h = h;
  a.n_cap = sub_n_cap(max_nodes); a.ld = sub_rd_ld(max_nodes);
  const size_t lds = sub_fill_lds(a.n_cap, a.ld, use_rd != 0);
  ESC_REQUIRE(!use_rd || lds <= 160 * 1024, "esc_subgraph_fill: rd working set %zu B exceeds LDS", lds);
  sub_launch_fill(sub_fill_kernel<true>, sub_fill_kernel<false>, use_rd, lds, (hipStream_t)stream, a);
  ESC_CHECK_LAUNCH("esc_subgraph_fill.fill");
  return ESC_OK;
}

int esc_subgraph2_count(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                        int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, int64_t* sub_node_ptr,
                        int64_t* sub_edge_ptr, int64_t* sub2_ptr, int32_t* status, void* stream) {
  const int rc = expand_check(SUB2_LIMITS, "esc_subgraph2_count", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, h);
  if (rc) return rc;
  ESC_REQUIRE(sub_node_ptr && sub_edge_ptr && sub2_ptr && status, "esc_subgraph2_count: null output");
  return sub_count_pass("esc_subgraph2_count", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, h, sub_node_ptr,
                        sub_edge_ptr, sub2_ptr, status, (hipStream_t)stream);
}

int esc_subgraph2_fill(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                       int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, const int64_t* sub_node_ptr,
                       const int64_t* sub_edge_ptr, const int64_t* sub2_ptr, int64_t total_sub_nodes, int64_t total_sub_edges,
                       int64_t total_subgraphs2, int use_rd, int64_t* orig_node, int64_t* z, int64_t* node_to_subgraph2,
                       int64_t* node_to_graph, int64_t* sub_src, int64_t* sub_dst, int64_t* orig_edge,
                       int64_t* subgraph2_to_subgraph, int64_t* center_idx, int64_t* s2_node_ptr, float* rd, int32_t* status,
                       void* stream) {
  const int rc = expand_check(SUB2_LIMITS, "esc_subgraph2_fill", node_ptr, edge_ptr, src, dst, G, total_nodes, total_edges, max_nodes, h);
  if (rc) return rc;
  ESC_REQUIRE(sub_node_ptr && sub_edge_ptr && sub2_ptr && status && s2_node_ptr, "esc_subgraph2_fill: null pointer");
  if (!sub_totals_ok(total_sub_nodes, total_sub_edges) || total_subgraphs2 < 0 || total_subgraphs2 > total_sub_nodes) {
    set_error("esc_subgraph2_fill: %ld sub-nodes / %ld sub-edges / %ld subgraph2s: totals must stay below 2^31",
              (long)total_sub_nodes, (long)total_sub_edges, (long)total_subgraphs2);
    return ESC_ERANGE;
  }
  if (total_nodes == 0 || total_sub_nodes == 0) return ESC_OK;
  ESC_REQUIRE(orig_node && z && node_to_subgraph2 && node_to_graph && subgraph2_to_subgraph && center_idx,
              "esc_subgraph2_fill: null node output");
  ESC_REQUIRE((sub_src && sub_dst && orig_edge) || total_sub_edges == 0, "esc_subgraph2_fill: null edge output");
  ESC_REQUIRE(!use_rd || rd, "esc_subgraph2_fill: use_rd without an rd output");
  Sub2FillArgs a{};
  a.node_ptr = node_ptr; a.edge_ptr = edge_ptr; a.src = src; a.dst = dst;
  a.sub_node_ptr = sub_node_ptr; a.sub_edge_ptr = sub_edge_ptr; a.sub2_ptr = sub2_ptr;
  a.orig_node = orig_node; a.z = z; a.node_to_subgraph2 = node_to_subgraph2; a.node_to_graph = node_to_graph;
  a.sub_src = sub_src; a.sub_dst = sub_dst; a.orig_edge = orig_edge; a.subgraph2_to_subgraph = subgraph2_to_subgraph;
  a.center_idx = center_idx; a.s2_node_ptr = s2_node_ptr; a.rd = rd; a.status = status;
  a.total_nodes = total_nodes; a.total_sub_nodes = total_sub_nodes; a.total_sub_edges = total_sub_edges; a.total_s2 = total_subgraphs2;
  a.G = (int)G; a.h = h;
  a.n_cap = sub_n_cap(max_nodes); a.ld = sub_rd_ld(max_nodes);
  const size_t lds = sub2_fill_lds(a.n_cap, a.ld, use_rd != 0);
  ESC_REQUIRE(lds + 16 <= 160 * 1024, "esc_subgraph2_fill: working set %zu B exceeds LDS", lds);
  sub_launch_fill(sub2_fill_kernel<true>, sub2_fill_kernel<false>, use_rd, lds, (hipStream_t)stream, a);
  ESC_CHECK_LAUNCH("esc_subgraph2_fill.fill");
  return ESC_OK;
}

int esc_segment_first_fwd(const float* x, int64_t ld_x, const int64_t* ptr, int64_t S, int64_t C, float* out, void* stream) {
  ESC_REQUIRE(S >= 0 && C >= 0 && ld_x >= C && S * C < (1LL << 40), "esc_segment_first_fwd: bad shape");
  if (S * C == 0) return ESC_OK;
  ESC_REQUIRE(x && ptr && out, "esc_segment_first_fwd: null pointer");
  esc::launch(ESC_K_FEATURES, segment_first_fwd_kernel, dim3((unsigned)cdiv(S * C, 256)), dim3(256), 0, (hipStream_t)stream, x, ld_x,
              ptr, S, C, out);
  ESC_CHECK_LAUNCH("esc_segment_first_fwd");
  return ESC_OK;
}

int esc_segment_first_bwd(const float* dout, int64_t ld_dout, const int64_t* ptr, const int64_t* node_to_segment, int64_t N,
                          int64_t C, float* dx, void* stream) {
  ESC_REQUIRE(N >= 0 && C >= 0 && ld_dout >= C && N * C < (1LL << 40), "esc_segment_first_bwd: bad shape");
  if (N * C == 0) return ESC_OK;
  ESC_REQUIRE(dout && ptr && node_to_segment && dx, "esc_segment_first_bwd: null pointer");
  esc::launch(ESC_K_FEATURES, segment_first_bwd_kernel, dim3((unsigned)cdiv(N * C, 256)), dim3(256), 0, (hipStream_t)stream, dout,
              ld_dout, ptr, node_to_segment, N, C, dx);
  ESC_CHECK_LAUNCH("esc_segment_first_bwd");
  return ESC_OK;
}

}  // extern "C"
