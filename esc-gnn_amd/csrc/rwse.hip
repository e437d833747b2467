// rwse.hip — the random-walk structural encoding of the graph transformer (include/escgnn_rwse.h): what the
// reference computes on the host per graph at dataset load with max(k) dense n x n matrix products whose diagonals alone are
// kept (GraphGPS/graphgps/transform/posenc_stats.py:185-231, get_rw_landing_probs), and collates as the pestat_RWSE key.
//
// esc_rw_landing: one workgroup of 256 threads (4 waves) per graph.  (P^k)[i, i] = e_i^T P^k e_i, so the entry of start node i
// is entry i of y after k steps y <- P y from y = e_i, and one step is a sparse matrix-vector product over the graph's edges
// grouped by source: y'[u] = (1 / deg[u]) * sum over the out-edges (u -> j) of y[j].  No n x n storage anywhere.
//   1. a read-only pass checks every edge end and stages the graph-local ends in LDS as 16-bit ids;
//   2. the thread of row u scans the staged sources in edge order: the number below u is the row's offset (count and prefix in
//      one pass, no cross-thread sum), the number equal to u its out-degree; a second scan copies the row's targets behind the
//      offset in the order the edges are listed.  Nothing is added concurrently: the fill order is a function of the edge
//      order alone;
//   3. the start nodes are dealt to the waves in rounds of 4; a wave keeps its two fp64 vectors in LDS, its lanes over the rows
//      u, and the lane of row i stores the emitted steps rounded once to fp32.  A workgroup barrier separates the steps (every
//      wave runs every round, a wave without a start node idles through it).
// Every loop bound depends on the graph and the step mask alone (never on max_nodes, max_edges or the launch), and the file is
// built without FMA contraction, so a graph's bits are the same alone and in any batch.
// esc_rwse_gather: one workgroup per graph of the batch copies its n x K rows of the resident table (ragged_graphs.h).
#include "ragged_graphs.h"
#include "../../include/escgnn_rwse.h"

namespace esc {

constexpr int RW_NT = 256;
constexpr int RW_WAVES = RW_NT / WAVE;
constexpr int RW_MAX_STEP = 63;
// LDS of one workgroup at (cap nodes, ecap edges):
//   y      double [RW_WAVES][2][cap]   the two vectors of every wave             64 * cap bytes
//   invdeg double [cap]                1 / out-degree, 0 for a sink               8 * cap
//   rowptr int    [cap + 1]            offsets of the rows in col                 4 * (cap + 1)
//   flag   int    [1]                  the check's verdict (a workgroup-wide OR)  4
//   es, ed uint16 [ecap] each          the staged edge ends, in edge order        4 * ecap
//   col    uint16 [ecap]               the targets grouped by source              2 * ecap
constexpr int64_t rw_lds_bytes(int64_t cap, int64_t ecap) {
  return (int64_t)(2 * RW_WAVES + 1) * cap * (int64_t)sizeof(double) + (cap + 2) * (int64_t)sizeof(int) + 3 * ecap * (int64_t)sizeof(uint16_t);
}
// The limits: 256 nodes, the attention kernel's limit at head_dim 64 (ids fit 16 bits with room to spare), and the most edges
// that then fit the 64 KiB a launch may ask for without raising the kernel's dynamic-LDS attribute - two workgroups at the
// limits still share a CU's 160 KiB:  76 * 256 + 8 + 6 * ecap <= 65 536  ->  ecap = 7 678.
constexpr int RW_MAX_NODES = 256;
constexpr int RW_LDS_BUDGET = 64 * 1024;
constexpr int rw_edges_of(int64_t bytes, int cap) {
  int m = 0;
  while (rw_lds_bytes(cap, m + 1) <= bytes) ++m;
  return m;
}
constexpr int RW_MAX_EDGES = rw_edges_of(RW_LDS_BUDGET, RW_MAX_NODES);
static_assert(RW_MAX_EDGES == 7678, "the header states 7678");
static_assert(RW_MAX_EDGES >= 4096 && RW_MAX_NODES <= 65535, "the issue's floor; 16-bit ids");

struct RwArgs {
  const int64_t* src; const int64_t* dst; const int64_t* node_ptr; const int64_t* edge_ptr;
  int64_t N, E, ldo;
  unsigned long long mask;
  int local, cap, ecap;                      // cap, ecap: max_nodes and max_edges as told - they place the LDS arrays
  float* out;
};

__global__ __launch_bounds__(RW_NT) void rw_landing_kernel(RwArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const GraphRange r = graph_range(a.node_ptr, a.edge_ptr, blockIdx.x, a.N, a.E);
  const int64_t n0 = r.n0, e0 = r.e0;
  // (all of this is uniform over the workgroup: it leaves together)
  if (!(r.ok && r.n1 > n0 && r.n1 - n0 <= a.cap && r.e1 - e0 <= a.ecap)) return;     // empty, or over max_nodes / max_edges: skipped
  const int n = (int)(r.n1 - n0), m = (int)(r.e1 - e0);
  const int64_t base = a.local ? 0 : n0;
  double* y = reinterpret_cast<double*>(smem);
  double* invdeg = y + (size_t)2 * RW_WAVES * a.cap;
  int* rowptr = reinterpret_cast<int*>(invdeg + a.cap);
  int* flag = rowptr + a.cap + 1;
  uint16_t* es = reinterpret_cast<uint16_t*>(flag + 1);
  uint16_t* ed = es + a.ecap;
  uint16_t* col = ed + a.ecap;
  if (tid == 0) *flag = 0;
  __syncthreads();
  for (int e = tid; e < m; e += RW_NT) {                      // 1. read-only: check, and stage in LDS
    int64_t s, t;
    if (!edge_ends(a.src, a.dst, e0 + e, base, n, s, t)) *flag = 1;     // (plain stores of one value; nothing writes it after the barrier)
    es[e] = (uint16_t)s;
    ed[e] = (uint16_t)t;
  }
  __syncthreads();
  if (*flag) return;
  for (int u = tid; u < n; u += RW_NT) {                      // 2. group by source, in edge order
    int lt = 0, eq = 0;
    for (int e = 0; e < m; ++e) {                             // (every thread reads the same address: a broadcast)
      const int s = es[e];
      lt += s < u ? 1 : 0;
      eq += s == u ? 1 : 0;
    }
    rowptr[u] = lt;
    invdeg[u] = eq ? 1.0 / (double)eq : 0.0;
    if (eq) {
      int p = lt;
      for (int e = 0; e < m; ++e)
        if (es[e] == u) col[p++] = ed[e];
    }
  }
  if (tid == 0) rowptr[n] = m;
  __syncthreads();
  const int wave = tid / WAVE, lane = tid % WAVE;
  const int kmax = 64 - __builtin_clzll(a.mask);              // the mask is positive: 1 <= kmax <= 63
  double* cur = y + (size_t)wave * 2 * a.cap;
  double* nxt = cur + a.cap;
  for (int i0 = 0; i0 < n; i0 += RW_WAVES) {                  // 3. a round: one start node per wave
    const int i = i0 + wave;
    const bool live = i < n;
    if (live)
      for (int u = lane; u < n; u += WAVE) cur[u] = u == i ? 1.0 : 0.0;
    __syncthreads();
    int c = 0;
    for (int k = 1; k <= kmax; ++k) {
      const bool emit = (a.mask >> (k - 1)) & 1ull;
      if (live) {
        for (int u = lane; u < n; u += WAVE) {
          double s = 0.0;
          const int p1 = rowptr[u + 1];
          for (int p = rowptr[u]; p < p1; ++p) s += cur[col[p]];
          s *= invdeg[u];
          nxt[u] = s;
          if (emit && u == i) a.out[(n0 + i) * a.ldo + c] = (float)s;
        }
      }
      c += emit ? 1 : 0;
      __syncthreads();
      double* t = cur; cur = nxt; nxt = t;
    }
  }
}

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_rw_landing_max_nodes(void) { return RW_MAX_NODES; }
int64_t esc_rw_landing_max_edges(void) { return RW_MAX_EDGES; }

int esc_rw_landing(const int64_t* src, const int64_t* dst, int64_t E, const int64_t* node_ptr, const int64_t* edge_ptr,
                   int64_t G, int64_t N, int edges_local, int64_t step_mask, int64_t max_nodes, int64_t max_edges, float* out,
                   int64_t ld_out, void* stream) {
  ESC_REQUIRE(step_mask > 0, "esc_rw_landing: step_mask %ld selects no step of 1..%d (bit k - 1 = step k)", (long)step_mask, RW_MAX_STEP);
  const int K = __builtin_popcountll((unsigned long long)step_mask);
  ESC_REQUIRE(G >= 0 && N >= 0 && E >= 0 && G < (1LL << 31) && N < (1LL << 31) && E < (1LL << 31) && max_nodes >= 0 && max_edges >= 0,
              "esc_rw_landing: bad sizes G=%ld N=%ld E=%ld max_nodes=%ld max_edges=%ld", (long)G, (long)N, (long)E, (long)max_nodes,
              (long)max_edges);
  ESC_REQUIRE(max_nodes <= RW_MAX_NODES, "esc_rw_landing: a graph of %ld nodes exceeds the limit of %d nodes per graph "
              "(esc_rw_landing_max_nodes)", (long)max_nodes, RW_MAX_NODES);
  ESC_REQUIRE(max_edges <= RW_MAX_EDGES, "esc_rw_landing: a graph of %ld edges exceeds the limit of %d edges per graph "
              "(esc_rw_landing_max_edges)", (long)max_edges, RW_MAX_EDGES);
  ESC_REQUIRE(ld_out >= K, "esc_rw_landing: leading dimension of out %ld below the %d steps of step_mask", (long)ld_out, K);
  if (G == 0 || N == 0 || max_nodes == 0) return ESC_OK;
  ESC_REQUIRE(node_ptr && edge_ptr && out && (E == 0 || (src && dst)), "esc_rw_landing: null pointer");
  const RwArgs a{src, dst, node_ptr, edge_ptr, N, E, ld_out, (unsigned long long)step_mask, edges_local ? 1 : 0, (int)max_nodes,
                 (int)max_edges, out};
  esc::launch(-1, rw_landing_kernel, dim3((unsigned)G), dim3(RW_NT), (size_t)rw_lds_bytes(max_nodes, max_edges), (hipStream_t)stream, a);
  ESC_CHECK_LAUNCH("esc_rw_landing");
  return ESC_OK;
}

int esc_rwse_gather(const float* table, const int64_t* node_ptr_all, int64_t G_all, int64_t N_all, const int64_t* graph_ids,
                    const int32_t* graph_ptr, int64_t B, int64_t N, int K, float* out, int64_t ld_out, void* stream) {
  ESC_REQUIRE(K >= 1 && K <= RW_MAX_STEP, "esc_rwse_gather: %d steps outside 1..%d", K, RW_MAX_STEP);
  ESC_REQUIRE(G_all >= 0 && N_all >= 0 && B >= 0 && N >= 0 && B < (1LL << 31) && N < (1LL << 31) && N_all < (1LL << 31),
              "esc_rwse_gather: bad sizes G_all=%ld N_all=%ld B=%ld N=%ld", (long)G_all, (long)N_all, (long)B, (long)N);
  ESC_REQUIRE(ld_out >= K, "esc_rwse_gather: leading dimension of out %ld below the %d steps", (long)ld_out, K);
  if (B == 0 || N == 0 || G_all == 0) return ESC_OK;
  ESC_REQUIRE(table && node_ptr_all && graph_ids && graph_ptr && out, "esc_rwse_gather: null pointer");
  esc::launch(-1, table_gather_kernel<1>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, GatherTables<1>{{table}, {out}}, node_ptr_all,
              G_all, N_all, graph_ids, graph_ptr, N, K, ld_out);
  ESC_CHECK_LAUNCH("esc_rwse_gather");
  return ESC_OK;
}

}  // extern "C"
