/* escgnn_subgraphs.h - the NGNN baseline's entry points of libescgnn_hip.so (csrc/subgraphs.hip), an extension header next
 * to escgnn_hip.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE too and derives the binding of
 * these functions from it (esc-gnn_amd/_native.py, EXTENSION_SIGNATURES).  They are kept apart from escgnn_hip.h because
 * tests/golden/abi_binding.json pins the binding of that header entry for entry; functions only, no struct, no constant:
 * ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_SUBGRAPHS_H
#define ESCGNN_SUBGRAPHS_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- node-rooted subgraph expansion of a collated batch (the NGNN baseline, reference utils.py:18-229; csrc/subgraphs.hip,
 * DESIGN 6h).  node_ptr / edge_ptr [G+1]; src / dst [total_edges] hold GLOBAL node ids, the edges of one graph contiguous (what
 * every collate here produces).  For every node r, S_r = the nodes within h hops walking target -> source; its sub-nodes are
 * written root first, then ascending (hop, node id); its sub-edges are all edges with both ends in S_r, in their original order,
 * relabelled to global sub-node ids.
 * esc_subgraph_count: sub_node_ptr / sub_edge_ptr [total_nodes+1] = exclusive scans of |S_r| and of the sub-edge counts;
 *   status[G] = 0, or ESC_ERANGE for a graph with a node id outside it, a range outside the arrays or more than max_nodes nodes
 *   (such a graph gets zero-length output).
 * esc_subgraph_fill (same inputs, the pointers of the count pass and their totals): orig_node / orig_edge = global ids of the
 *   batch, hop_label = hop + 1, hop_paths = number of edges from the previous BFS level into the node (0 for the root; the
 *   reference labels a node once per such edge), node_to_subgraph = r, node_to_graph = its graph.  use_rd: rd[i] = P[0,0] + P[i,i]
 *   - P[0,i] - P[i,0], P = pinv(D_in - A) of the non-loop sub-edges in fp64, cast to fp32; a subgraph of more than 96 nodes sets
 *   status = ESC_ERANGE and leaves its rd rows unwritten.
 * Limits (error message names them): 1 <= h <= 98, max_nodes <= 4096, every total below 2^31. */
int esc_subgraph_count(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                       int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, int64_t* sub_node_ptr,
                       int64_t* sub_edge_ptr, int32_t* status, void* stream);
int esc_subgraph_fill(const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* src, const int64_t* dst, int64_t G,
                      int64_t total_nodes, int64_t total_edges, int64_t max_nodes, int h, const int64_t* sub_node_ptr,
                      const int64_t* sub_edge_ptr, int64_t total_sub_nodes, int64_t total_sub_edges, int use_rd,
                      int64_t* orig_node, int64_t* hop_label, int64_t* hop_paths, int64_t* node_to_subgraph,
                      int64_t* node_to_graph, int64_t* sub_src, int64_t* sub_dst, int64_t* orig_edge, float* rd,
                      int32_t* status, void* stream);
/* out[s] = x[ptr[s]] (S rows of C floats; ptr int64 [S+1]) and its gradient: every row of dx [N, C] is written, dout[s] on the
 * first row of segment s = node_to_segment[row], zero elsewhere. */
int esc_segment_first_fwd(const float* x, int64_t ld_x, const int64_t* ptr, int64_t S, int64_t C, float* out, void* stream);
int esc_segment_first_bwd(const float* dout, int64_t ld_dout, const int64_t* ptr, const int64_t* node_to_segment, int64_t N,
                          int64_t C, float* dx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
