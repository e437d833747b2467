/* escgnn_i2gnn.h - the I2GNN baseline's entry points of libescgnn_hip.so (csrc/subgraphs.hip, csrc/i2pool.hip), a second
 * extension header next to escgnn_hip.h and escgnn_subgraphs.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py
 * reads THIS FILE too and derives the binding of these functions from it (esc-gnn_amd/_native.py, I2GNN_SIGNATURES).
 * Functions only, no struct, no constant: ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_I2GNN_H
#define ESCGNN_I2GNN_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- every node-rooted subgraph once per neighbour of its root (the I2GNN baseline, reference utils_edge_I2.py:132-256,
 * 726-813).  Inputs as esc_subgraph_count.  S_r, its canonical sub-node order and its sub-edges are those of
 * escgnn_subgraphs.h.  The neighbours of r are the targets of the sub-edges whose source is r, in sub-edge order (repeated
 * edges repeat, a self loop gives r); K_r is their number and the output holds max(K_r, 1) copies of S_r back to back, each
 * one a "subgraph2".
 * esc_subgraph2_count: sub_node_ptr / sub_edge_ptr / sub2_ptr [total_nodes+1] = exclusive scans of max(K,1)*|S_r|, of
 *   max(K,1)*(sub-edges of r) and of max(K,1); status[G] as esc_subgraph_count.
 * esc_subgraph2_fill (same inputs, the pointers of the count pass and their totals), for copy c of root r with neighbour j:
 *   orig_node / orig_edge = global ids of the batch; z [total_sub_nodes, 4] = [hop+1, hop+1 if two or more frontier edges enter
 *   the node else 0] for root r, then the same pair for root j plus h + 3, from an unbounded BFS from j over the sub-edges of
 *   S_r (a node j does not reach: [0, 0] + h + 3); node_to_subgraph2 = global subgraph2 id, node_to_graph = graph;
 *   subgraph2_to_subgraph [total_subgraphs2] = r; center_idx [total_subgraphs2, 2] = (first row of the copy, row of j);
 *   s2_node_ptr [total_subgraphs2+1] = row pointers of the subgraph2s.  K_r = 0: one copy, columns 2-3 of z repeat columns 0-1,
 *   center_idx = (first row, first row).  use_rd: rd [total_sub_nodes, 2] = [R(0,k), R(j,k)], R(a,b) = P[a,a] + P[b,b] - P[a,b]
 *   - P[b,a], P = pinv(D_in - A) of the non-loop sub-edges in fp64 (one per root), cast to fp32; K_r = 0 repeats R(0,k).
 *   status = ESC_ERANGE for a graph with a subgraph of more than 96 nodes under use_rd (rd rows unwritten).  The labels need
 *   no status: the sub-edge r -> j puts r one step from j and every node of S_r reaches r inside S_r in at most h steps, so on
 *   any graph, directed ones included, j reaches all of S_r within h + 1 steps and the largest label is 2h + 5.
 * Limits (error message names them): 1 <= h <= 47, max_nodes <= 1536, every total below 2^31. */
int esc_subgraph2_count(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                        int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, int64_t* sub_node_ptr,
                        int64_t* sub_edge_ptr, int64_t* sub2_ptr, int32_t* status, void* stream);
int esc_subgraph2_fill(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                       int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, const int64_t* sub_node_ptr,
                       const int64_t* sub_edge_ptr, const int64_t* sub2_ptr, int64_t total_sub_nodes, int64_t total_sub_edges,
                       int64_t total_subgraphs2, int use_rd, int64_t* orig_node, int64_t* z, int64_t* node_to_subgraph2,
                       int64_t* node_to_graph, int64_t* sub_src, int64_t* sub_dst, int64_t* orig_edge,
                       int64_t* subgraph2_to_subgraph, int64_t* center_idx, int64_t* s2_node_ptr, float* rd, int32_t* status,
                       void* stream);

/* ---- subgraph2_pooling = 'mean-center-side' (csrc/i2pool.hip): out[s] = [mean of x[ptr[s] .. ptr[s+1]) | x[center[s]] |
 * x[side[s]]], S rows of 3C floats from rows of C floats; ptr int64 [S+1]; center[s] / side[s] are read at center[s *
 * idx_stride] (idx_stride = 2 for the two columns of center_idx).  An empty segment gives zeros.  Backward: every row of dx
 * [N, C] is written once, dout_mean[s] / len + (row == center[s]) dout_c[s] + (row == side[s]) dout_s[s], s =
 * node_to_segment[row]; center == side adds both. */
int esc_pool_mean_center_side_fwd(const float* x, int64_t ld_x, const int64_t* ptr, const int64_t* center, const int64_t* side,
                                  int64_t idx_stride, int64_t S, int64_t C, float* out, int64_t ld_out, void* stream);
int esc_pool_mean_center_side_bwd(const float* dout, int64_t ld_dout, const int64_t* ptr, const int64_t* center,
                                  const int64_t* side, int64_t idx_stride, const int64_t* node_to_segment, int64_t N, int64_t C,
                                  float* dx, int64_t ld_dx, void* stream);
/* ---- the gate: y = sigmoid(a) * x over M rows of C floats; da = dy * x * s (1 - s), dx = dy * s (contiguous [M, C]; either
 * may be NULL), s recomputed from a, finite for every finite a. */
int esc_sigmoid_mul_fwd(const float* a, int64_t ld_a, const float* x, int64_t ld_x, int64_t M, int64_t C, float* y, int64_t ld_y,
                        void* stream);
int esc_sigmoid_mul_bwd(const float* a, int64_t ld_a, const float* x, int64_t ld_x, const float* dy, int64_t ld_dy, int64_t M,
                        int64_t C, float* da, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
