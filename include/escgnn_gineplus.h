/* escgnn_gineplus.h - the GINE+ baseline's entry points of libescgnn_hip.so (csrc/multihop.hip, csrc/gineplus.hip), a third
 * extension header next to escgnn_hip.h, escgnn_subgraphs.h and escgnn_i2gnn.h.  Same conventions and the same grammar:
 * esc-gnn_amd/_abi.py reads THIS FILE too and derives the binding of these functions from it (esc-gnn_amd/_native.py,
 * GINEPLUS_SIGNATURES).  Functions only, no struct, no constant: ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_GINEPLUS_H
#define ESCGNN_GINEPLUS_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- multi-hop edges of a collated batch (reference modules/gine_operations.py:256-303, make_multihop_edges).
 * Inputs as esc_subgraph_count: G graphs whose nodes [node_ptr[g], node_ptr[g+1]) and edges [edge_ptr[g], edge_ptr[g+1]) are
 * contiguous, global node ids in src / dst, an edge read as src -> dst.  The pairs of root i are (i, i) at distance 0 and (i, j)
 * for every j with 1 <= d(i -> j) <= k, d the directed shortest-path length (repeated edges count once, a self loop or a
 * 2-cycle leaves (i, i) at 0); they are written in ascending j, the roots in ascending i: sorted by (row, col), no sort.
 * esc_multihop_count: pair_ptr [total_nodes+1] = exclusive scan of the pairs per root, d1_ptr [total_nodes+1] = exclusive scan
 *   of the distance-1 pairs per root, dist_count [G, k+1] = pairs of graph g at distance 0..k, status [G] = 0 or ESC_ERANGE
 *   (a node id outside its graph, ranges that do not tile the arrays, more than max_nodes nodes): such a graph has no pairs.
 * esc_multihop_fill (same inputs, the two pointer arrays and total_pairs = pair_ptr[total_nodes]): row / col / distance
 *   [total_pairs] int64, and meta [total_pairs, 4] int32 = (row, col, distance, rank), rank = the position of the pair among
 *   the distance-1 pairs in (row, col) order - the row of the edge term it reads - for distance 1, -1 otherwise.  A root whose
 *   range ends beyond total_pairs writes nothing and sets status = ESC_ERANGE.
 * Limits (error message names them): 1 <= k <= 8, max_nodes <= 4096 (one byte of LDS per node of the root's graph), every total
 * below 2^31. */
int esc_multihop_count(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                       int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int k, int64_t* pair_ptr, int64_t* d1_ptr,
                       int64_t* dist_count, int32_t* status, void* stream);
int esc_multihop_fill(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                      int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int k, const int64_t* pair_ptr,
                      const int64_t* d1_ptr, int64_t total_pairs, int64_t* row, int64_t* col, int64_t* distance, int32_t* meta,
                      int32_t* status, void* stream);

/* ---- the GINE+ aggregate in one launch per direction (csrc/gineplus.hip; reference :306-362 before self.nn), 1 <= k <= 4:
 *   out[i] = (1+eps[0]) x0[i] + sum_{d=1..k} (1+eps[d]) * sum_{j : d(j->i) = d} relu(x_{d-1}[j] + [d=1] e[rank(j,i)])
 * x0..x3: [N, C] rows with leading dimensions ld0..ld3 (x_t is read for t < k only; the same pointer may be given k times:
 * NAIVEGINEPLUS); e [M1, C]; eps [k+1, C] contiguous.  Forward: the pairs grouped by destination, in_ptr int32 [N+1] and
 * in_meta [M, 4] = the meta rows in that order (stable: ascending source inside a destination); distance-0 rows are skipped,
 * the self term is read directly.  Every inner sum runs in ascending source order with separately rounded adds, and the outer
 * sum in ascending d: bit-identical to k esc_gine_aggregate_fwd launches combined by elementwise kernels.
 * Backward: the pairs grouped by source are the output order of esc_multihop_fill, out_ptr = pair_ptr (int64) and meta.
 *   dx_t [N, C] contiguous for t < k (dx + t*N*C), d_e [M1, C] contiguous, every row written once (a distance-1 pair owns its
 *   row of d_e); deps_part [esc_gineplus_bwd_blocks(N), (k+1)*C] per-workgroup partial sums of d eps, reduced in workgroup
 *   order into d_eps [k+1, C] by a second launch (d_eps NULL: neither is touched).  No atomics: bit-stable run to run.
 * C % 4 == 0 with 16-byte aligned pointers and leading dimensions that are multiples of 4 takes 16-byte accesses, anything else a
 * scalar path. */
int esc_gineplus_aggregate_fwd(const float* x0, int64_t ld0, const float* x1, int64_t ld1, const float* x2, int64_t ld2,
                               const float* x3, int64_t ld3, const float* e, int64_t ld_e, const int32_t* in_ptr,
                               const int32_t* in_meta, const float* eps, int64_t N, int64_t C, int k, int64_t M1, float* out,
                               int64_t ld_out, void* stream);
int64_t esc_gineplus_bwd_blocks(int64_t N);
int esc_gineplus_aggregate_bwd(const float* x0, int64_t ld0, const float* x1, int64_t ld1, const float* x2, int64_t ld2,
                               const float* x3, int64_t ld3, const float* e, int64_t ld_e, const float* g, int64_t ld_g,
                               const int64_t* out_ptr, const int32_t* meta, const float* eps, int64_t N, int64_t C, int k,
                               int64_t M1, float* dx, float* d_e, float* deps_part, float* d_eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
