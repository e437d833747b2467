/* escgnn_spd.h - the shortest-path attention bias of the graph transformer (reference GraphGPS global_model_type
 * 'BiasedTransformer': Graphormer's spatial encoding): the all-pairs shortest-path distances of every graph of a ragged set and
 * the gather from their resident table (csrc/spd.hip), and the ragged multi-head attention with a per-(distance, head) additive
 * bias on the scores (csrc/attention.hip); a tenth extension header next to escgnn_hip.h, escgnn_subgraphs.h, escgnn_i2gnn.h,
 * escgnn_gineplus.h, escgnn_gps.h, escgnn_lappe.h, escgnn_rwse.h, escgnn_step.h, escgnn_gatedgcn.h and escgnn_pna.h.  Same
 * conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE too and derives the binding of these functions from it
 * (esc-gnn_amd/_native.py, SPD_SIGNATURES).  Functions only, no struct, no constant: ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_SPD_H
#define ESCGNN_SPD_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- all-pairs shortest-path distances (reference GraphGPS/graphgps/loader/utils_escgnn.py:29-38:
 * nx.all_pairs_shortest_path_length on to_networkx(data, to_undirected=True), 100 where there is no path, stored flattened as
 * the key attn_bias).  One workgroup per graph of a ragged set: a collated batch, or a store's whole split in one
 * launch.
 * src, dst, node_ptr, edge_ptr, edges_local: exactly as in esc_rw_landing (escgnn_rwse.h) - the two rows of edge_index, the node
 *           and edge range of every graph (edges contiguous per graph, in any order inside the range), and whether the edge ends
 *           are graph-local ids or rows of the batch.
 * pair_ptr int64 [G+1]: the exclusive scan of n*n (ops._pair_ptr; the layout of the attention's keep mask).
 *   spd uint8 [pairs]: entry (i, j) of graph g at pair_ptr[g] + i*n + j.  `pairs` is the room the buffer has, told by the host
 *   (>= pair_ptr[G], which lives on the device and is read there).
 * The graph is undirected: an edge listed in either direction connects both ends; self-loops and duplicate edges change
 * nothing.  d(i, i) = 0; a pair without a path gets 100; the stored value is min(d, 100).  A true distance of 100 therefore
 * aliases "no path", as it does in the reference (row 100 of its Embedding(101, heads, padding_idx=100) is the padding row);
 * above 100 the reference's embedding lookup raises, here such a pair reads row 100 as well.
 * The workgroup keeps the adjacency as bit rows in LDS (ceil(n / 64) 64-bit words per node, each row built by the thread of
 * its node from a scan of the staged edges: no atomics of any kind), then one thread per source node runs a breadth-first
 * search with its frontier and seen sets in registers and stores a level's distances as the level is discovered: every byte
 * is written exactly once.  Integers only: a graph's bytes depend on nothing else in the launch - identical alone and inside
 * any batch - and are identical run to run.
 * max_nodes: the largest node count of one graph, told by the caller (nothing is read back); it picks the words per row and the
 * workgroup size.  Limits (the message names them; checked on the host before anything is launched):
 * max_nodes <= esc_graph_spd_max_nodes() = 256; there is no limit on the edges of a graph.
 * A graph that contradicts what the host was told - more nodes than max_nodes, a node or edge range that is negative or leaves
 * [0, N] / [0, E], pair_ptr entries that are not the scan of n*n or leave [0, pairs], an edge end outside the graph - is skipped
 * by its workgroup after a read-only pass: nothing is read or written out of bounds, its bytes stay unwritten.  Empty graphs,
 * G == 0, N == 0 and E == 0 are legal; a graph with nodes but no edges writes 0 on its diagonal and 100 elsewhere.
 * Launches: 1. */
int64_t esc_graph_spd_max_nodes(void);
int esc_graph_spd(const int64_t* src, const int64_t* dst, int64_t E, const int64_t* node_ptr, const int64_t* edge_ptr,
                  const int64_t* pair_ptr, int64_t G, int64_t N, int64_t pairs, int edges_local, int64_t max_nodes, uint8_t* spd,
                  void* stream);

/* ---- what the reference's collate would do to the attn_bias key (its padding block is commented out, loader/batch.py:132-141),
 * off a resident table: one launch, one workgroup per graph of the batch.  table uint8 [pairs_all]: the distances of a whole
 * split in pair_ptr_all's layout; pair_ptr_all, node_ptr_all int64 [G_all+1]: its pair and node ranges; graph_ids int64 [B]
 * (device): the batch's graphs in batch order; graph_ptr int32 [B+1], pair_ptr int64 [B+1]: the batch's node and pair ranges.
 * Bytes [pair_ptr[b], pair_ptr[b+1]) of out [pairs] receive bytes [pair_ptr_all[id], pair_ptr_all[id+1]) of the table.  The ids
 * live on the device: the caller checks them on the host (ops.spd_gather does); a workgroup whose id is out of range, whose
 * node counts differ between the table and the batch, or whose pair ranges are not n*n long or leave their arrays, copies
 * nothing. */
int esc_spd_gather(const uint8_t* table, const int64_t* pair_ptr_all, const int64_t* node_ptr_all, int64_t G_all, int64_t pairs_all,
                   const int64_t* graph_ids, const int32_t* graph_ptr, const int64_t* pair_ptr, int64_t B, int64_t pairs,
                   uint8_t* out, void* stream);

/* ---- ragged multi-head self-attention with the shortest-path bias (reference gps_layer.py:237-239,273-278: the float attn_mask
 * of torch.nn.MultiheadAttention built from attn_bias by edge_attn_emb and edge_attn_linear).  esc_graph_attention_fwd / _bwd
 * (escgnn_gps.h) with three more operands; everything not said here is as there: qkv, graph_ptr, pair_ptr, max_nodes, the
 * two-pass softmax, dropout and the mask's layout, the skip contract, the launch shape (one workgroup per (graph, head), one
 * thread per row), dQ with K_0 taken off.
 *   spd        uint8 [spd_pairs]: byte (i, j) of graph g at pair_ptr[g] + i*n + j, shared by all heads; read as given at
 *              [i, j] - no symmetry is assumed, any byte matrix is legal, a byte above 100 counts as 100.  spd_pairs: the room
 *              the buffer has, told by the host; a batch whose pair_ptr[G] exceeds it is skipped like an oversized graph.
 *   bias_table fp32 [101, heads] contiguous: the reference's MLP depends on (distance, head) alone, so it collapses to this
 *              table (nn / gps_models evaluate it once per layer and forward).
 *   S_ij = q_i . k_j / sqrt(head_dim) + bias_table[min(spd_ij, 100), a];  lse includes the bias.
 * The head's 101 entries are staged in LDS; the per-pair cost is one byte read and one LDS lookup.  The forward and both
 * phases of the backward form S from the same products in the same order and the same one addition, so P agrees bit for bit
 * between them.
 * Limits: those of escgnn_gps.h with max_nodes <= esc_graph_attention_bias_max_nodes(head_dim) instead: with DP = head_dim
 * rounded up to 4, 8, 16, 32 or 64, the backward keeps (2 DP + 2) floats per node (K and V, then Q and dO; lse and delta), 104
 * floats of table and 101 * 256 floats of bins in LDS, so
 *   limit = min(esc_graph_attention_max_nodes(head_dim), floor4((163840 - 4 * (104 + 101 * 256)) / (4 * (2 DP + 2))))
 * (floor4: rounded down to a multiple of 4) = 1024 at DP 4, 832 at 8, 440 at 16, 224 at 32, 112 at 64.
 * Launches: forward 1, backward 2. */
int64_t esc_graph_attention_bias_max_nodes(int head_dim);
int esc_graph_attention_bias_fwd(const float* qkv, int64_t ld_qkv, const int32_t* graph_ptr, const int64_t* pair_ptr,
                                 const uint8_t* spd, int64_t spd_pairs, const float* bias_table, int64_t G, int64_t N,
                                 int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p, uint64_t seed, float* out,
                                 int64_t ld_out, float* lse, uint8_t* mask, void* stream);
/* The bias gradient: d_table [101, heads] contiguous, every element written,
 *   d_table[b, a] = sum over the graphs and over their pairs with min(spd_ij, 100) == b of dS_ij,  dS_ij = P_ij (dPd_ij - delta_i).
 * No float atomics, one writer per value, bit-identical run to run: in phase A the thread of query i adds dS_ij to a private
 * LDS column bins[b * blockDim + tid] (rows in ascending i, pairs in ascending j); after a barrier thread b sums its 101st of
 * the bins in a fixed order over the threads and writes one partial per (graph, head, b); a second launch sums the partials
 * over the graphs in a fixed order (64 interleaved chains in ascending g, then the 64 in ascending lane).  A skipped graph
 * writes zero partials.
 * partial: scratch of partial_floats >= esc_graph_attention_bias_scratch_floats(G, heads) = 101 * heads * G floats. */
int64_t esc_graph_attention_bias_scratch_floats(int64_t G, int heads);
int esc_graph_attention_bias_bwd(const float* qkv, int64_t ld_qkv, const float* d_out, int64_t ld_dout, const float* lse,
                                 const uint8_t* mask, const int32_t* graph_ptr, const int64_t* pair_ptr, const uint8_t* spd,
                                 int64_t spd_pairs, const float* bias_table, int64_t G, int64_t N, int64_t mask_pairs,
                                 int64_t max_nodes, int heads, int head_dim, float p, float* d_qkv, float* partial,
                                 int64_t partial_floats, float* d_table, void* stream);

#ifdef __cplusplus
}
#endif
#endif
