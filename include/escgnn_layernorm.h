/* escgnn_layernorm.h - the per-graph LayerNorm of the GPS layer (reference GraphGPS gt.layer_norm: gps_layer.py:143-145,161 builds
 * pygnn.norm.LayerNorm(dim_h) and calls it as norm(h, batch.batch), PyG's graph mode: one mean and one variance over all nodes
 * and all channels of each graph), forward and backward (csrc/layernorm.hip); an eleventh extension header next to escgnn_hip.h,
 * escgnn_subgraphs.h, escgnn_i2gnn.h, escgnn_gineplus.h, escgnn_gps.h, escgnn_lappe.h, escgnn_rwse.h, escgnn_step.h,
 * escgnn_gatedgcn.h, escgnn_pna.h and escgnn_spd.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE
 * too and derives the binding of these functions from it (esc-gnn_amd/_native.py, LAYERNORM_SIGNATURES).  Functions only, no
 * struct, no constant: ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_LAYERNORM_H
#define ESCGNN_LAYERNORM_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- forward (PyG 2.0.4 / 2.2 LayerNorm.forward with a batch vector, restated on graph_ptr).  For graph g with the
 * rows [graph_ptr[g], graph_ptr[g+1]) of the batch, n of them, and M = n * C:
 *   h    = x              (or x + r when a residual r is given: one fp32 addition per element)
 *   mean = sum(h) / M
 *   c    = h - mean
 *   var  = sum(c * c) / M           (centred, a second pass: not E[h^2] - mean^2)
 *   rstd = 1 / sqrt(var + eps)
 *   y    = c * rstd * weight[col] + bias[col]
 * x [N, C] rows of leading dimension ld_x; r the same with ld_r, or NULL; graph_ptr int32 [G+1] on the device; weight, bias
 * fp32 [C], both given or both NULL (then y = c * rstd); y [N, C] with ld_y; stats fp32 [2 G]: (mean, rstd) of graph g at
 * stats[2 g], stats[2 g + 1], what the backward reads.
 * One workgroup per graph, threads striding over the graph's rows at fixed columns; there is no node limit per graph (nothing
 * is staged in LDS; beyond a thread's first four rows the second and third pass read the L2).  No atomics, every output element
 * written exactly once, bit-identical run to run.  The work split and every reduction order depend on n and C alone, on nothing
 * else in the batch: y, stats and - in the backward - d_x of a graph have the same bits alone and inside any batch.
 * An empty graph writes no rows and stats (0, 0).  A graph whose range is unordered or leaves [0, N] is skipped by its
 * workgroup: nothing is read or written out of bounds, its rows and its stats stay unwritten.  G == 0 or N == 0 writes nothing.
 * Limits (checked on the host before anything is launched; the message names them): C a multiple of 4 with
 * 4 <= C <= esc_graph_layer_norm_max_channels() = 1024; every leading dimension >= C and a multiple of 4; every pointer 16-byte
 * aligned; N < 2^31 / 64, G < 2^31 - 1.
 * Launches: 1. */
int64_t esc_graph_layer_norm_max_channels(void);
int esc_graph_layer_norm_fwd(const float* x, int64_t ld_x, const float* r, int64_t ld_r, const int32_t* graph_ptr, int64_t G, int64_t N,
                             int64_t C, const float* weight, const float* bias, float eps, float* y, int64_t ld_y, float* stats,
                             void* stream);

/* ---- backward.  x, r, stats, graph_ptr, weight: the forward's; g = dL/dy [N, C] with ld_g.  With gh = g * weight[col] (g without
 * an affine) and xhat = (h - mean) * rstd recomputed from x (+ r) by the same single addition as the forward:
 *   s1 = sum_graph(gh);  s2 = sum_graph(gh * xhat)
 *   d_x = rstd * (gh - s1 / M - xhat * s2 / M)      [N, C] with ld_dx: also the residual's gradient - written once, the caller
 *                                                   returns it for both
 *   partial[g] = (sum_i g * xhat per column | sum_i g per column)        fp32 [G, 2, C], scratch
 *   d_weight[col] = sum_g partial[g][0][col];  d_bias[col] = sum_g partial[g][1][col]         fp32 [C] each
 * The first launch (one workgroup per graph, the forward's split) writes d_x and partial; the second sums partial over the graphs
 * in a fixed order - 64 interleaved chains in ascending g, then the 64 in ascending lane, as the bias gradient of
 * escgnn_spd.h does - and writes every element of d_weight and d_bias.  No atomics.
 * weight, d_weight, d_bias and partial come together: all given, or all NULL (no affine: one launch, d_x alone).
 * An empty or a skipped graph writes no rows and a zero partial.  G == 0 or N == 0 writes nothing except d_weight and d_bias,
 * which become zeros.  Limits: the forward's.
 * Launches: 2 (1 without an affine). */
int esc_graph_layer_norm_bwd(const float* x, int64_t ld_x, const float* r, int64_t ld_r, const float* stats, const float* g, int64_t ld_g,
                             const int32_t* graph_ptr, int64_t G, int64_t N, int64_t C, const float* weight, float* d_x, int64_t ld_dx,
                             float* d_weight, float* d_bias, float* partial, void* stream);

#ifdef __cplusplus
}
#endif
#endif
