/* escgnn_rwse.h - the random-walk structural encoding's entry points of libescgnn_hip.so (csrc/rwse.hip): the landing
 * probabilities of the k-step random walk on every graph of a ragged set, and the row gather from a resident table; a sixth
 * extension header next to escgnn_hip.h, escgnn_subgraphs.h, escgnn_i2gnn.h, escgnn_gineplus.h, escgnn_gps.h and
 * escgnn_lappe.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE too and derives the binding of
 * these functions from it (esc-gnn_amd/_native.py, RWSE_SIGNATURES).  Functions only, no struct, no constant:
 * ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_RWSE_H
#define ESCGNN_RWSE_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- random-walk landing probabilities (reference GraphGPS/graphgps/transform/posenc_stats.py:185-231 with edge_weight None
 * and space_dim 0).  One workgroup per graph of a ragged set: a collated batch, or a store's whole split in one
 * launch.
 * src, dst, node_ptr, edge_ptr, edges_local: exactly as in esc_laplacian_eig (escgnn_lappe.h) - the two rows of edge_index,
 *           the node and edge range of every graph (edges contiguous per graph, in any order inside the range), and whether
 *           the edge ends are graph-local ids or rows of the batch.
 * A[u, j] = the number of listed edges u -> j: the list is directed, every edge counts as it stands, self-loops are kept and
 * duplicates add up (to_dense_adj).  deg[u] = sum_j A[u, j] (out-degree), P = D^-1 A with the rows of deg = 0 zero.
 *   out [N, K] fp32, leading dimension ld_out:  out[i, c] = (P^{k_c})[i, i]  for the steps k_0 < k_1 < ... of step_mask.
 * step_mask: bit k - 1 set = step k is emitted, k in 1..63; the columns are the set bits in ascending order, K = popcount.
 * Arithmetic: fp64, rounded once to fp32 on the store.  (P^k)[i, i] is entry i of y after k steps y <- P y from y = e_i; one
 * step is y'[u] = (1 / deg[u]) * sum over the out-edges (u -> j) of y[j], the edges of u in the order they are listed.  The
 * workgroup groups its graph's edges by source in LDS (a count, its prefix and a fill, each by scanning the edges in order):
 * the order of every sum is a function of the edge order alone.  No atomics of any kind, no cross-workgroup sums: a graph's
 * result depends on nothing else in the launch - bit-equal alone and inside any batch - and is bit-identical run to run.
 * max_nodes, max_edges: the largest node and edge count of one graph, told by the caller (nothing is read back); they size
 * the LDS - a launch asks for what they need, not for the limits.
 * Limits (the message names them; checked on the host before anything is launched): step_mask > 0,
 * max_nodes <= esc_rw_landing_max_nodes() = 256, max_edges <= esc_rw_landing_max_edges() = 7678, ld_out >= K.
 * A graph that contradicts what the host was told - more nodes than max_nodes, more edges than max_edges, a node or edge range
 * that is negative or leaves [0, N) / [0, E), an edge end outside the graph - is skipped by its workgroup after a read-only
 * pass: nothing is read or written out of bounds, its rows stay unwritten.  Empty graphs, G == 0, N == 0 and E == 0 are legal;
 * a graph with nodes but no edges writes zeros.
 * Launches: 1. */
int64_t esc_rw_landing_max_nodes(void);
int64_t esc_rw_landing_max_edges(void);
int esc_rw_landing(const int64_t* src, const int64_t* dst, int64_t E, const int64_t* node_ptr, const int64_t* edge_ptr,
                   int64_t G, int64_t N, int edges_local, int64_t step_mask, int64_t max_nodes, int64_t max_edges, float* out,
                   int64_t ld_out, void* stream);

/* ---- what the reference's collate does to the pestat_RWSE key, off a resident table: one launch, one workgroup per graph of
 * the batch.  table [N_all, K] (contiguous): the statistics of a whole split; node_ptr_all int64 [G_all+1]: its node ranges;
 * graph_ids int64 [B] (device): the batch's graphs in batch order; graph_ptr int32 [B+1]: the batch's node ranges.  Rows
 * [graph_ptr[b], graph_ptr[b+1]) of out [N, K] (leading dimension ld_out >= K: a column slice of a wider buffer) receive rows
 * [node_ptr_all[id], node_ptr_all[id+1]) of the table.  The ids live on the device: the caller checks them on the host
 * (ops.rwse_gather does); a workgroup whose id is out of range, or whose two ranges differ in length or leave their arrays,
 * copies nothing.  1 <= K <= 63. */
int esc_rwse_gather(const float* table, const int64_t* node_ptr_all, int64_t G_all, int64_t N_all, const int64_t* graph_ids,
                    const int32_t* graph_ptr, int64_t B, int64_t N, int K, float* out, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
