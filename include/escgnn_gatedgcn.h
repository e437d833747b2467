/* escgnn_gatedgcn.h - the GatedGCN local layer's entry points of libescgnn_hip.so (csrc/gatedgcn.hip): the gather / gate /
 * segmented reduce of the reference's CustomGatedGCN (GraphGPS/graphgps/layer/gatedgcn_layer.py:67-136) forward and backward;
 * an eighth extension header next to escgnn_hip.h, escgnn_subgraphs.h, escgnn_i2gnn.h, escgnn_gineplus.h, escgnn_gps.h,
 * escgnn_lappe.h, escgnn_rwse.h and escgnn_step.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py reads THIS FILE
 * too and derives the binding of these functions from it (esc-gnn_amd/_native.py, GATEDGCN_SIGNATURES).  Functions only, no
 * struct, no constant: ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_GATEDGCN_H
#define ESCGNN_GATEDGCN_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the gate.  For every edge k = (j -> i) of the batch, in fp32:
 *   e_ij   = (Dx[i] + Ex[j]) + Ce[k]                                     gatedgcn_layer.py:96
 *   sigma  = 1 / (1 + expf(-e_ij))                                       :97   (this form: the accurate expf, an IEEE division;
 *                                                                              a gate below -88 is 0, above 17 it is 1: finite)
 *   out[i] = Ax[i] + (sum_k sigma_k * Bx[j_k]) / (sum_k sigma_k + 1e-6)  :117-133
 * Ax, Bx, Dx, Ex [N, C] and Ce [E, C]: fp32 rows, each with its own leading dimension in floats (column slices of wider
 * buffers are fine).  in_ptr / in_edge / in_src: the destination view of the batch's plan, as in esc_gine_aggregate_fwd -
 * in_ptr int32 [N+1], and for slot p of node i's range the edge position in_edge[p] and its source in_src[p], the slots of a
 * node in ascending edge position (a stable grouping).
 *   out   [N, C], leading dimension ld_out;
 *   e_out [E, C], leading dimension ld_eo: e_ij at the edge's own position k (not its sorted slot) - the layer's new edge
 *         attributes before their BatchNorm;
 *   den   [N, C] contiguous: sum_k sigma_k without the 1e-6, kept for the backward.
 * Every sum over a node's in-edges runs in ascending edge position; no atomics, no cross-workgroup sums, every output element
 * written exactly once; the file is built without FMA contraction: a graph's rows have the same bits alone and inside any
 * batch, run to run.  A node without in-edges gets out = Ax exactly (0 / 1e-6) and den = 0.
 * E == 0 with N > 0 may pass NULL for in_edge / in_src / Ce / e_out; N == 0 writes nothing.
 * Limits (checked on the host before anything is launched; the message names them): C a multiple of 4 with
 * 4 <= C <= esc_gated_gcn_max_channels() = 1024, every leading dimension >= C and a multiple of 4, every pointer 16-byte aligned.
 * Launches: 1. */
int64_t esc_gated_gcn_max_channels(void);
int esc_gated_gcn_fwd(const float* Ax, int64_t ld_ax, const float* Bx, int64_t ld_bx, const float* Dx, int64_t ld_dx,
                      const float* Ex, int64_t ld_ex, const float* Ce, int64_t ld_ce, const int32_t* in_ptr,
                      const int32_t* in_edge, const int32_t* in_src, int64_t N, int64_t E, int64_t C, float* out, int64_t ld_out,
                      float* e_out, int64_t ld_eo, float* den, void* stream);

/* ---- its backward.  g_out [N, C] and g_e [E, C] are the gradients of out and e_out; g_e may be NULL: zero.  Saved from the
 * forward and read here: e_out, den, and out with Ax - the kernel forms aggr_i = out[i] - Ax[i] itself (no saved aggr, no
 * launch for the difference; the subtraction returns aggr to within one rounding of out).  With
 * r_i = g_out[i] / (den[i] + 1e-6) and s = 1 / (1 + expf(-e_out[k])):
 *   d_e[k]  = g_e[k] + ((r_i * (Bx[j] - aggr_i)) * s) * (1 - s)       -> d_Ce [E, C] at position k
 *   d_Dx[i] = sum over in(i)  of d_e[k]
 *   d_Ex[j] = sum over out(j) of d_e[k]
 *   d_Bx[j] = sum over out(j) of s_k * r_{dst_k}
 *   d_Ax    = g_out: the caller's, no kernel work.
 * Two launches on `stream`: the first walks the destination view (in_ptr / in_edge / in_src) and writes d_Ce and d_Dx, the
 * second walks the source view (out_ptr / out_edge / out_dst) and writes d_Ex and d_Bx from d_Ce, e_out, g_out and den.
 * Every output element is written exactly once, never accumulated into; sums in ascending edge position; no atomics.
 * All four outputs are required.  E == 0 with N > 0 may pass NULL for the edge arrays of both views and for g_e / e_out /
 * d_Ce (the node outputs are zeros); N == 0 writes nothing.  Limits: those of the forward. */
int esc_gated_gcn_bwd(const float* g_out, int64_t ld_go, const float* g_e, int64_t ld_ge, const float* e_out, int64_t ld_eo,
                      const float* den, const float* out, int64_t ld_out, const float* Ax, int64_t ld_ax, const float* Bx,
                      int64_t ld_bx, const int32_t* in_ptr, const int32_t* in_edge, const int32_t* in_src, const int32_t* out_ptr,
                      const int32_t* out_edge, const int32_t* out_dst, int64_t N, int64_t E, int64_t C, float* d_Ce, int64_t ld_dce,
                      float* d_Dx, int64_t ld_ddx, float* d_Ex, int64_t ld_dex, float* d_Bx, int64_t ld_dbx, void* stream);

#ifdef __cplusplus
}
#endif
#endif
