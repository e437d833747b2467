/* escgnn_step.h - the step boundary of the counting step engine (csrc/engine.hip, *Seam*; DESIGN.md section 4, *Step engine,
 * step boundary*): the optimiser step ordered on the engine's two streams, and what lets the next step start without a hop to the
 * caller's stream and back; a seventh extension header next to escgnn_hip.h, escgnn_subgraphs.h, escgnn_i2gnn.h,
 * escgnn_gineplus.h, escgnn_gps.h, escgnn_lappe.h and escgnn_rwse.h.  Same conventions and the same grammar: esc-gnn_amd/_abi.py
 * reads THIS FILE too and derives the binding of these functions from it (esc-gnn_amd/_native.py, STEP_SIGNATURES).  Functions
 * only, no struct, no constant: ESC_ABI_VERSION is not concerned. */
#ifndef ESCGNN_STEP_H
#define ESCGNN_STEP_H
#include "escgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* esc_adam_step over [0, n) of one flat buffer whose elements [n_early, n) are the optimiser's LATE bucket (FlatAdam(late=...):
 * the edge pipeline's parameters).  Called right behind esc_engine_train_step_end of a two-stream step, on that step's stream and
 * over buffers that hold that step's z_table and its gradient in their late part, it runs as two launches of the same kernel:
 * [n_early, n) on the engine's edge stream, behind that stream's last slab reduce and behind every gradient the node pipeline
 * finished, and [0, n_early) on `stream`, which then waits for the other launch.  When the call returns, every parameter is
 * complete in the order of `stream`, as after esc_adam_step, and the bits are those of esc_adam_step: the update of an element
 * depends on that element alone.  Anywhere else (no such step in front, one stream, bit 8 of esc_engine_set_side_stream set)
 * it IS esc_adam_step: one launch on `stream`.
 * The launch on the edge stream is ordered behind esc_engine_train_step_end, NOT behind what the caller has queued on `stream`
 * since: a caller that has written gradients, parameters or optimiser state there in between (clipping, scaling, accumulation)
 * calls esc_adam_step[_scaled] instead, or esc_engine_drop_fast_seam first.  FlatAdam.step() does so by itself for every torch
 * op, which it sees in the tensors' version counters; writes by raw address or through `.data` it cannot see.  Nor is the
 * launch ordered behind READS of [n_early, n) of param / exp_avg / exp_avg_sq that the caller queued on `stream` since _end:
 * such a caller drops the seam too. */
int esc_engine_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t n_early,
                         double lr, double beta1, double beta2, double eps, int64_t step, void* stream);
/* The caller states that every array of the batch it hands to the NEXT esc_engine_train_step_begin was queued on the step's
 * stream before the last esc_engine_train_step_end (the collate between the two halves) and has not been written since.  The
 * engine then launches that step's FIRST edge kernel, the ESC bag, in edge-stream order, behind its own Adam launch, without
 * waiting for the caller's stream - if the split esc_engine_adam_step was the call in front of this one, the step uses the same
 * stream and workspace, runs on two streams on one rank, and z_table lies in the late part.  That launch reads z_table and the
 * batch's row_ptr / bag_idx / bag_val and writes workspace; every later launch of the edge pipeline (the other parameters, the
 * BatchNorm running statistics it updates) is ordered behind everything queued on the caller's stream, as always: the record
 * that orders it travels while the bag runs.  Otherwise, and without this call, the whole step starts behind the caller's stream,
 * as it always did.  Any other engine entry,
 * esc_adam_step[_scaled] and esc_engine_drop_fast_seam withdraw the claim. */
int esc_engine_claim_fast_seam(void);
/* For a caller that has written gradients, parameters, optimiser state or the batch's arrays on its stream since
 * esc_engine_train_step_end by means the engine does not see: the next esc_engine_adam_step is one launch on the caller's
 * stream, and the next step starts behind everything queued there. */
int esc_engine_drop_fast_seam(void);
/* this thread's counts (diagnostics, tests): which = 0: steps that started in edge-stream order; 1: optimiser steps that ran
 * split over the two streams; anything else: -1 */
int64_t esc_engine_seam_count(int which);

#ifdef __cplusplus
}
#endif
#endif
