/* escgnn_gps.h - the graph transformer's entry points of libescgnn_hip.so (csrc/attention.hip): multi-head self-attention over
 * the nodes of every graph of a ragged batch, a fourth extension header next to escgnn_hip.h, escgnn_subgraphs.h, escgnn_i2gnn.h
 * and escgnn_gineplus.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE too and derives the binding
 * of these functions from it (esc-gnn_amd/_native.py, GPS_SIGNATURES).  Functions only, no struct, no constant: ESC_ABI_VERSION
 * is not concerned. */
#ifndef ESCGNN_GPS_H
#define ESCGNN_GPS_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ragged multi-head self-attention (reference GraphGPS/graphgps/layer/gps_layer.py:234-236,269-286: to_dense_batch,
 * torch.nn.MultiheadAttention with key_padding_mask, gather back - here without the pad, the mask tensor and the gather;
 * DESIGN 6k).
 * qkv [N, 3H] fp32 rows with leading dimension ld_qkv, H = heads * head_dim, columns [q | k | v], head a at columns
 * a*head_dim .. of each third: what one Linear with MultiheadAttention.in_proj_weight / in_proj_bias produces.
 * graph_ptr int32 [G+1]: the nodes of graph g are the rows [graph_ptr[g], graph_ptr[g+1]), n = their number.
 * pair_ptr int64 [G+1]: the exclusive scan of n*n.
 * For graph g and head a:  S = Q_a K_a^T / sqrt(head_dim);  P = row softmax of S (maximum taken off first, sums in fp32);
 * Pd = P o M / (1-p), M the keep mask;  out[:, a] = Pd V_a.
 *   out  [N, H] rows with leading dimension ld_out;
 *   lse  [heads, N]: lse[a*N + i] = log sum_j exp(S_ij), kept for the backward;
 *   mask [heads * pair_ptr[G]] bytes: M_ij of (g, a) at a*pair_ptr[G] + pair_ptr[g] + i*n + j.  Dropout follows
 *        esc_dropout_fwd: keep when the counter-based hash of (seed, that index) is >= p.  p == 0 reads and writes no mask
 *        (NULL is accepted).  pair_ptr[G] lives on the device and is read there; the host states the room the buffer has as
 *        mask_pairs (the buffer holds heads * mask_pairs bytes; N * max_nodes bounds pair_ptr[G] without a read-back), and a
 *        batch whose pair_ptr[G] exceeds it is skipped like an oversized graph.
 * max_nodes: the largest n of the batch, told by the caller (the host never reads graph_ptr back); it sizes the workgroup and
 * its LDS.  A graph with more nodes than max_nodes, or whose rows leave [0, N), is skipped by the kernels: nothing is read or
 * written out of bounds, its rows stay unwritten; so is a graph whose pair_ptr entries are not the scan of n*n.
 * Limits (the error message names them; checked on the host before anything is launched): head_dim a multiple of 4 and at most
 * 64, ld_qkv >= 3 * heads * head_dim and ld_out >= heads * head_dim (that qkv is exactly 3H wide with heads * head_dim == H is
 * the caller's to check: ops.graph_attention does), max_nodes <= esc_graph_attention_max_nodes(head_dim) = min(1024, 16384 /
 * head_dim rounded up to 4, 8, 16, 32 or 64) - 256 nodes at head_dim 64, 512 at 32, 1024 below: the K and V slices of one
 * (graph, head) stay in LDS.
 * Empty graphs, G == 0 and N == 0 are legal and write nothing.
 * Launches: forward 1, backward 1.  No atomics and no cross-workgroup sums: one workgroup owns a (graph, head) pair and one
 * thread every output row, so the results are bit-identical run to run. */
int64_t esc_graph_attention_max_nodes(int head_dim);
int esc_graph_attention_fwd(const float* qkv, int64_t ld_qkv, const int32_t* graph_ptr, const int64_t* pair_ptr, int64_t G,
                            int64_t N, int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p, uint64_t seed,
                            float* out, int64_t ld_out, float* lse, uint8_t* mask, void* stream);
/* d_qkv [N, 3H] contiguous, every element written exactly once (a skipped graph's rows excepted).  P is recomputed from lse;
 * nothing of size n*n except the mask is kept between the passes:
 *   dPd = (dO V_a^T) o M / (1-p);  delta_i = sum_j P_ij dPd_ij;  dS = P o (dPd - delta);
 *   dV = Pd^T dO;  dQ = dS K / sqrt(head_dim);  dK = dS^T Q / sqrt(head_dim).
 * delta is summed from P and the mask the call is GIVEN, not taken as dO_i . O_i: the two agree when the mask is the forward's,
 * and the summed form is the gradient of the masked expression for any mask (a query row whose mask bytes are all zero gets
 * dQ = 0 exactly) - so the forward's `out` is not an input and is not kept for the backward. */
int esc_graph_attention_bwd(const float* qkv, int64_t ld_qkv, const float* d_out, int64_t ld_dout, const float* lse,
                            const uint8_t* mask, const int32_t* graph_ptr, const int64_t* pair_ptr, int64_t G, int64_t N,
                            int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p, float* d_qkv, void* stream);

#ifdef __cplusplus
}
#endif
#endif
