// graphlets.hip — per-node, per-orbit counts of the five graphlets of the counting benchmark (count_graphlet targets 0..4)
// in small graphs: tailed triangle, chordal cycle, 4-clique, 4-path, triangle-rectangle ("house").
//
// The label definition is the project's own.  Input normalised as in cycles.hip: self loops dropped, edges
// symmetrised, duplicates collapsed.  A copy of a pattern is a subgraph isomorphic to it — not necessarily induced — and is
// counted once, not once per automorphism.  out[v][c] is the number of copies in which v sits at orbit c:
//   0 tailed triangle: the triangle node carrying the tail     6 4-path: an end
//   1                  one of the other two triangle nodes     7         an inner node
//   2                  the tail end                            8 house: the apex (triangle only)
//   3 chordal cycle:   a chord endpoint                        9        a node of the shared edge
//   4                  a non-chord node                       10        a rectangle-only node
//   5 4-clique:        any node
//
// One 64-lane workgroup per graph, as cycles.hip: the adjacency rows are 64-bit masks in LDS (n <= 64) and lane v counts
// the copies rooted at v.  With N(.) the masks, d = |N|, c(a,b) = |N(a) & N(b)| and t(a) the triangles through a (also
// kept in LDS), one pass over the neighbours u of v and, inside it, over the other neighbours w of v gives every column
// but the apex as sums of popcounts:
//   c0 = t(v)(d(v)-2)      c1 = sum_u c(v,u)(d(u)-2)       c2 = sum_u t(u) - 2t(v)      c3 = sum_u C(c(v,u), 2)
//   c4 = 1/2 sum_u sum_{w in N(v)&N(u)} (c(u,w)-1)          c5 = sum_u sum_{w in N(v)&N(u), w>u} |N(v)&N(u)&N(w) above w|
//   c6 = sum_u sum_{w in N(u)-v} (d(w)-1-[w~v])             c7 = sum_u ((d(v)-1)(d(u)-1) - c(v,u))
//   c9 (v = s1, u = s2, w = f1): F2 = N(u)&N(w) - v, C = N(v)&N(u):  |F2|(|C| - [w in C]) - |F2 & C|   (pairs f2, apex)
//   c10 (v = f1, u = s1, w = s2 in N(u)-v): F = N(v)&N(w) - u, P = N(u)&N(w) - v:  |F||P| - |F & P|     (pairs f2, apex)
// The apex column walks the adjacent pairs s1 < s2 of N(v) and the feet f1 of s1: c8 += |N(f1) & N(s2) - {v, s1}|.
// Work per node is at most d^3/2 mask steps (108 at degree 6).  Every column fits int32 at n <= 64: the largest is the
// house in K64, 14 295 960 in columns 9 and 10.  Integer arithmetic only: the output is deterministic.
#include "ragged_graphs.h"

namespace esc {

constexpr int GRAPHLET_COLS = 11;

__global__ __launch_bounds__(64) void graphlet_counts_kernel(const int64_t* __restrict__ node_ptr,
                                                             const int64_t* __restrict__ edge_ptr,
                                                             const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                             int64_t total_nodes, int64_t total_edges,
                                                             int32_t* __restrict__ out, int64_t ld_out,
                                                             int32_t* __restrict__ status) {
  __shared__ unsigned long long adj[ADJ_MAX_NODES];
  __shared__ int tri[ADJ_MAX_NODES];
  __shared__ int bad;
  const int lane = threadIdx.x;
  int64_t n0, n;
  if (!adjacency_masks(node_ptr, edge_ptr, src, dst, total_nodes, total_edges, status, adj, bad, n0, n)) return;
  const int v = lane;
  const unsigned long long vbit = 1ull << v, nv = adj[v];     // lanes >= n hold an empty row
  const int dv = __popcll(nv);
  int t2 = 0;                                        // twice the triangles through v
  for (unsigned long long m = nv; m; m &= m - 1) t2 += __popcll(adj[__ffsll((long long)m) - 1] & nv);
  const int tv = t2 >> 1;
  tri[lane] = tv;
  __syncthreads();
  if (lane >= n) return;

  int c1 = 0, c2 = -2 * tv, c3 = 0, c4 = 0, c5 = 0, c6 = 0, c7 = 0, c8 = 0, c9 = 0, c10 = 0;
  for (unsigned long long mu = nv; mu; mu &= mu - 1) {
    const int u = __ffsll((long long)mu) - 1;
    const unsigned long long ubit = 1ull << u, nu = adj[u];
    const unsigned long long com = nv & nu;          // the triangles on the edge v-u
    const int du = __popcll(nu), cvu = __popcll(com);
    c1 += cvu * (du - 2);
    c2 += tri[u];
    c3 += cvu * (cvu - 1) / 2;
    c7 += (dv - 1) * (du - 1) - cvu;
    for (unsigned long long mw = com; mw; mw &= mw - 1) {      // w closes the triangle v u w
      const int w = __ffsll((long long)mw) - 1;
      const unsigned long long nw = adj[w];
      c4 += __popcll(nu & nw) - 1;                   // both orders (u,w), (w,u): halved below
      if (w > u) {
        const unsigned long long above = ~((2ull << w) - 1ull);   // w = 63: 2ull << 63 wraps to 0, the mask is empty
        c5 += __popcll(com & nw & above);            // the clique v u w x, once: u < w < x
        // apex v, shoulders u < w: the feet f1 of u, then f2 in N(f1) & N(w)
        const unsigned long long skip = vbit | ubit;
        for (unsigned long long mf = nu & ~(vbit | (1ull << w)); mf; mf &= mf - 1)
          c8 += __popcll(adj[__ffsll((long long)mf) - 1] & nw & ~skip);
      }
    }
    for (unsigned long long mw = nu & ~vbit; mw; mw &= mw - 1) {   // w in N(u) - v
      const int w = __ffsll((long long)mw) - 1;
      const unsigned long long nw = adj[w];
      c6 += __popcll(nw) - 1 - (int)((nw >> v) & 1ull);          // path v u w x: x in N(w) - {u, v}
      const unsigned long long F = nv & nw & ~ubit, P = nu & nw & ~vbit;   // foot v, shoulders u (mine), w
      c10 += __popcll(F) * __popcll(P) - __popcll(F & P);
    }
    for (unsigned long long mw = nv & ~ubit; mw; mw &= mw - 1) {   // shoulder v, shoulder u, my foot w
      const int w = __ffsll((long long)mw) - 1;
      const unsigned long long F2 = nu & adj[w] & ~vbit;
      c9 += __popcll(F2) * (cvu - (int)((com >> w) & 1ull)) - __popcll(F2 & com);
    }
  }
  int32_t* row = out + (n0 + v) * ld_out;
  row[0] = tv * (dv - 2);
  row[1] = c1;
  row[2] = c2;
  row[3] = c3;
  row[4] = c4 >> 1;
  row[5] = c5;
  row[6] = c6;
  row[7] = c7;
  row[8] = c8;
  row[9] = c9;
  row[10] = c10;
}

}  // namespace esc

using namespace esc;

extern "C" int esc_graphlet_counts(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst,
                                   int64_t G, int64_t total_nodes, int64_t total_edges, int32_t* out, int64_t ld_out,
                                   int32_t* status, void* stream) {
  ESC_REQUIRE(G >= 0 && total_nodes >= 0 && total_edges >= 0, "esc_graphlet_counts: negative size");
  ESC_REQUIRE(ld_out >= GRAPHLET_COLS, "esc_graphlet_counts: ld_out must be at least 11");
  if (G == 0) return ESC_OK;
  ESC_REQUIRE(node_ptr && edge_ptr && status, "esc_graphlet_counts: null graph arrays");
  ESC_REQUIRE((src && dst) || total_edges == 0, "esc_graphlet_counts: null edge arrays");
  ESC_REQUIRE(out || total_nodes == 0, "esc_graphlet_counts: null output");
  ESC_REQUIRE(G < (1LL << 31), "esc_graphlet_counts: too many graphs in one call");
  hipStream_t s = (hipStream_t)stream;
  // graphs over 64 nodes report ESC_ERANGE through status[g]; an id or a range outside the arrays, ESC_EINVAL
  esc::launch(ESC_K_FEATURES, graphlet_counts_kernel, dim3((unsigned)G), dim3(64), 0, s, node_ptr, edge_ptr, src, dst,
              total_nodes, total_edges, out, ld_out, status);
  ESC_CHECK_LAUNCH("esc_graphlet_counts");
  return ESC_OK;
}
