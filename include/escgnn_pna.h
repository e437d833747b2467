/* escgnn_pna.h - the PNA local layer's entry points of libescgnn_hip.so (csrc/pna.hip): the gather and the segmented
 * mean | max | sum of PyG's PNAConv with aggregators ['mean', 'max', 'sum'], scaler 'identity', one tower, one pre- and one
 * post-layer (what GraphGPS/graphgps/layer/gps_layer.py:78-93 constructs), forward and backward; a ninth extension header next
 * to escgnn_hip.h, escgnn_subgraphs.h, escgnn_i2gnn.h, escgnn_gineplus.h, escgnn_gps.h, escgnn_lappe.h, escgnn_rwse.h,
 * escgnn_step.h and escgnn_gatedgcn.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE too and
 * derives the binding of these functions from it (esc-gnn_amd/_native.py, PNA_SIGNATURES).  Functions only, no struct, no
 * constant: ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_PNA_H
#define ESCGNN_PNA_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the aggregate.  The message of PNAConv is ONE Linear of cat[x_i, x_j, edge_encoder(e_k)], so it splits into
 * a destination part P [N, C] (bias included), a source part Q [N, C] and an edge part R [E, C], which the caller forms as
 * three GEMMs.  For every edge k = (j -> i) of the batch, in fp32:
 *   m_k    = (P[i] + Q[j]) + R[k]
 *   sum_i  = sum over in(i) of m_k      mean_i = sum_i / max(deg_i, 1)      max_i = max over in(i) of m_k
 * deg_i counts the in-edges of i, self-loops and repeated edges included.  P, Q, R: fp32 rows, each with its own leading
 * dimension in floats (column slices of wider buffers are fine).  in_ptr / in_edge / in_src: the destination view of the
 * batch's plan, as in esc_gine_aggregate_fwd - in_ptr int32 [N+1], and for slot p of node i's range the edge position
 * in_edge[p] and its source in_src[p], the slots of a node in ascending edge position (a stable grouping).
 *   agg [N, 3C], leading dimension ld_agg >= 3C: mean | max | sum in this column order - the columns H .. 4H of the
 *       [N, 4H] operand of PNAConv's post-layer may be handed as they are;
 *   arg [N, C] int32 contiguous: the edge position k (not the sorted slot) that holds the maximum of that node and column,
 *       -1 for a node without in-edges.  It is all the backward needs: nothing of size [E, C] is kept.
 * Sums and comparisons run in ascending edge position.  The maximum starts from the node's FIRST message - never from 0 or a
 * finite sentinel, so a node whose messages are all negative keeps a negative maximum - and a later message replaces it only
 * where m > best: among equal maxima the LOWEST edge position wins.  A node without in-edges gets zeros in all three and -1.
 * NaN: a NaN message poisons sum and mean of its node and column, and is never selected as the maximum while the node has a
 * message that is not NaN there (m > best is false for a NaN m, and a NaN best is replaced by the next message).
 * No atomics, no cross-workgroup sums, every output element written exactly once; the file is built without FMA contraction:
 * a graph's rows have the same bits alone and inside any batch, run to run.
 * E == 0 with N > 0 may pass NULL for in_edge / in_src / R; N == 0 writes nothing.
 * Limits (checked on the host before anything is launched; the message names them): C a multiple of 4 with
 * 4 <= C <= esc_pna_max_channels() = 1024, every leading dimension >= its row width (C; 3C for agg) and a multiple of 4,
 * every pointer 16-byte aligned.
 * Launches: 1. */
int64_t esc_pna_max_channels(void);
int esc_pna_aggregate_fwd(const float* P, int64_t ld_p, const float* Q, int64_t ld_q, const float* R, int64_t ld_r,
                          const int32_t* in_ptr, const int32_t* in_edge, const int32_t* in_src, int64_t N, int64_t E, int64_t C,
                          float* agg, int64_t ld_agg, int32_t* arg, void* stream);

/* ---- its backward.  g [N, 3C] (leading dimension ld_g >= 3C) is the gradient of agg, g_mean | g_max | g_sum; arg is what
 * the forward wrote.
 *   d_R[k] = (g_sum[i] + g_mean[i] / max(deg_i, 1)) + (arg[i] == k ? g_max[i] : 0)       at the edge's own position k
 *   d_P[i] = sum over in(i)  of d_R[k]
 *   d_Q[j] = sum over out(j) of d_R[k]
 * Two launches on `stream`: the first walks the destination view (in_ptr / in_edge; in_src is not read) and writes d_R and
 * d_P, the second walks the source view (out_ptr / out_edge; out_dst is not read) and writes d_Q from d_R.  Every output
 * element is written exactly once, never accumulated into; sums in ascending edge position; no atomics.  All three outputs
 * are required.  E == 0 with N > 0 may pass NULL for the edge arrays of both views and for d_R (the node outputs are zeros);
 * N == 0 writes nothing.  Limits: those of the forward (ld_g >= 3C). */
int esc_pna_aggregate_bwd(const float* g, int64_t ld_g, const int32_t* arg, const int32_t* in_ptr, const int32_t* in_edge,
                          const int32_t* in_src, const int32_t* out_ptr, const int32_t* out_edge, const int32_t* out_dst,
                          int64_t N, int64_t E, int64_t C, float* d_R, int64_t ld_dr, float* d_P, int64_t ld_dp, float* d_Q,
                          int64_t ld_dq, void* stream);

#ifdef __cplusplus
}
#endif
#endif
