// engine.hip — one host call = one NestedGIN_eff training step (forward + L1 + backward) or one
// eval-mode forward.  Orchestrates the kernels of this library from C++ so that the per-op host
// overhead of the Python/autograd path disappears, and applies the cross-op fusions a per-op
// interface cannot express:
//   * BatchNorm(+ReLU) is applied by the CONSUMER: esc_bn_stats emits (scale, shift) and the next
//     GEMM applies relu(x*scale+shift) while staging its A (or, for weight gradients, B) operand.
//     z_emb (E x H) and the hidden activation of every MLP are never written to memory; the backward
//     recomputes the ReLU mask from the pre-BN value.
//   * layer outputs are materialised directly into their slice of the [N,(L+1)H] concatenation buffer
//     (reference: torch.cat(xs, dim=1), run_graphcount.py:181), and d(cat) slices are consumed in place;
//     the aggregate backward accumulates dx into the previous layer's slice.
//   * d(z_emb) = sum_l d_e_l * W_lin_l accumulates inside the dX GEMM epilogue.
// Model composition followed: /root/reference/run_graphcount.py:134-194 (graph_pred=False, dropout=0,
// use_cycle=True — the configuration run_graphcount.py:465 instantiates).
#include "common.h"
#include "engine_plan.h"

#include <map>
#include <vector>
#include <cstdlib>

namespace esc {

#define ESC_TRY(call)            \
  do {                           \
    int rc__ = (call);           \
    if (rc__ != ESC_OK) return rc__; \
  } while (0)

struct Ctx {
  const esc_nested_gin_t* m;
  const esc_batch_t* b;
  Layout y;
  void* s;
  bool train;
  std::vector<esc_reduce_job>* jobs = nullptr;   // deferred weight-gradient reduces (main chain only); null: each is reduced at once
  SlabCursor* slabs = nullptr;                   // where the next weight gradient's slab region starts (every training entry)
  bool on_edge_stream = false;
  int act = 1;                                   // 1 ReLU (counting model), 2 ELU (ZINC): materialised activations
  const float* l1_target = nullptr;              // train_step: the prediction head also leaves d L1 / d pred (forward(), train_step_impl())
  int64_t l1_denom = 0;
  bool fast_seam = false;                        // the edge pipeline starts in edge-stream order, without the z_ready chain (see Seam)
  Schedule sch;                                  // every decision of this call (engine_plan.h): set once by the entry, the bodies only read it
};
// the knob values the kernels' own plans are taken with (linear_mfma.hip, aggregate.hip, bag.hip): the schedule plans with the same
const plan::PlanKnobs& linear_plan_knobs();
const sparse::SparseKnobs& aggregate_plan_knobs();
const sparse::SparseKnobs& bag_plan_knobs();

struct LdsFloorGuard {            // occupancy cap for the GEMMs launched while it lives (edge stream only, forward and backward)
  explicit LdsFloorGuard(bool on) : on_(on && edge_lds_floor() > 0) { if (on_) set_gemm_lds_floor(edge_lds_floor()); }
  ~LdsFloorGuard() { if (on_) set_gemm_lds_floor(0); }
  bool on_;
};

// Where the node chain's GEMM workgroups land.  An edge-stream GEMM (128x128 tile, 96 KB of LDS, one workgroup per CU) leaves 64 KB
// of its CU's LDS free, so a 54-KB node workgroup co-resides with it and the two share the CU's MFMA pipe.  A node workgroup that
// ASKS for 66 KB (dynamic LDS it does not use) is only placed on CUs without an edge workgroup: in the backward — dual launches of 392
// workgroups beside 57-us edge launches of 478 — that is worth 15 us of the node chain (phase marks: node backward 477 -> 462 us,
// step 0.995 -> 0.980 ms; bench 1.048 -> 1.031 ms); 60 000 bytes (still co-resident) changes nothing, 82 000 (one node workgroup per
// CU) costs 50 us, and in the forward (152-workgroup launches) the same request costs 8 us: the backward only.
static constexpr int kNodeLdsFloorBwd = 66 * 1024;      // bytes
// (kReadoutDxLds, engine_plan.h: the readout Linear's edge-stream block as two launches.)  Bit 7 of esc_engine_set_side_stream (and bit 6,
// the schedule of event records) keeps the block one launch with a record behind it: A/B runs.
static_assert(2 * kReadoutDxLds > 160 * 1024 && kReadoutDxLds + kNodeLdsFloorBwd <= 160 * 1024, "one readout dX tile and one node tile per CU");
static int g_readout_one_launch = 0;
struct NodeFloorGuard {
  explicit NodeFloorGuard(int bytes) : on_(bytes > 0) { if (on_) set_node_lds_floor(bytes); }
  ~NodeFloorGuard() { if (on_) set_node_lds_floor(0); }
  bool on_;
};

// The slab cursor and the deferred-reduction job list of a training entry: they live in the entry's frame, the Ctx points at
// them.  The reduces are deferred when the step's `n_jobs` weight gradients fit one reduce launch (else each is reduced at once,
// out of its own region all the same); the forward_train entries only mark the main chain (statistics from the GEMM
// epilogues): n_jobs = 0.
struct StepSlabs {
  StepSlabs(Ctx& c, float* slabs, int64_t limit, int n_jobs) : cursor{slabs, 0, limit} {
    if (n_jobs > 0) jobs.reserve(ESC_MAX_REDUCE_JOBS);
    c.slabs = &cursor;
    if (n_jobs <= ESC_MAX_REDUCE_JOBS) c.jobs = &jobs;
  }
  StepSlabs(const StepSlabs&) = delete;
  SlabCursor cursor;
  std::vector<esc_reduce_job> jobs;
};
// the private slab region of the next (M rows, N x K) weight gradient and, when reduces are deferred, its job
struct Slab { float* p = nullptr; esc_reduce_job* job = nullptr; };
static int take_slab(const Ctx& c, int64_t M, int64_t N, int64_t K, Slab* s) {
  s->p = c.slabs ? c.slabs->take(M, N, K) : nullptr;
  ESC_REQUIRE(s->p != nullptr, "esc_engine: no slab region left for a weight gradient of %ld rows, %ld x %ld", (long)M, (long)N, (long)K);
  if (c.jobs) { c.jobs->emplace_back(); s->job = &c.jobs->back(); }
  return ESC_OK;
}

// dX + dW tiles now, slab reduce deferred (or immediate when the context has no job list)
static int linear_backward(const Ctx& c, const float* dY, int64_t ld_dy, const float* X, int64_t ld_x, const float* sc,
                           const float* sh, const esc_linear_t& lin, int64_t M, float* dX, int64_t ld_dx, int accumulate) {
  const LdsFloorGuard cap(c.on_edge_stream);
  const int64_t N = lin.out_dim, K = lin.in_dim;
  Slab s;
  ESC_TRY(take_slab(c, M, N, K, &s));
  if (s.job == nullptr)
    return esc_linear_bwd_both(dY, ld_dy, X, ld_x, sc, sh, lin.w, K, M, N, K, dX, ld_dx, accumulate, lin.dw, K, lin.db, s.p, c.s);
  return esc_linear_bwd_both_deferred(dY, ld_dy, X, ld_x, sc, sh, lin.w, K, M, N, K, dX, ld_dx, accumulate, lin.dw, K, lin.db,
                                      s.p, s.job, c.s);
}

// BatchNorm(+ReLU) backward folded into the Linear backward behind it (engine_plan.h: kBnBwdApplyInGemm and the schedule)
static int linear_backward_bn(const Ctx& c, const float* dOut, int64_t ld_dout, const esc_bn_bwd_fused& f, const float* X, int64_t ld_x,
                              const float* sc, const float* sh, const esc_linear_t& lin, int64_t M, float* dX, int64_t ld_dx,
                              int accumulate, const esc_bn_bwd_next* next) {
  const LdsFloorGuard cap(c.on_edge_stream);
  const int64_t N = lin.out_dim, K = lin.in_dim;
  Slab s;
  ESC_TRY(take_slab(c, M, N, K, &s));
  return esc_linear_bwd_both_bn(dOut, ld_dout, &f, X, ld_x, sc, sh, lin.w, K, M, N, K, dX, ld_dx, accumulate, lin.dw, K, lin.db, s.p,
                                s.job, next, c.s);
}

// The edge-sized conv.lin GEMMs (e_l = lin_l(z_emb) forward; dX/dW of lin_l backward) depend on the node chain only
// through e_l / d_e_l: they run on a second HIP stream and fill the CUs that the latency-bound node-sized launches
// (152 workgroups on 256 CUs) leave idle.  One event per dependency, no host synchronisation.
struct EdgeStream {
  hipStream_t stream = nullptr;
  hipEvent_t z_ready = nullptr, joined = nullptr, lin1_fork = nullptr, lin1_rest = nullptr, lin1_dw = nullptr, e_ready[ESC_MAX_LAYERS] = {}, de_ready[ESC_MAX_LAYERS] = {},
             agg_done[ESC_MAX_LAYERS] = {};
  hipEvent_t caller_done = nullptr, late_done = nullptr;     // the step boundary (see Seam)
  bool ok = false;
};
static int g_use_edge_stream = 1;     // esc_engine_set_side_stream() bit 1
static int current_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}
static EdgeStream& edge_stream() {
  static thread_local std::map<int, EdgeStream> per_device;   // streams / events belong to the device that was current when they were made
  static thread_local EdgeStream off;   // ok == false
  if (!g_use_edge_stream) return off;
  EdgeStream& es = per_device[current_device()];
  if (!es.ok && es.stream == nullptr) {
    // lowest priority: when workgroup slots free up, the latency-critical node chain is served first
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    bool good = hipStreamCreateWithPriority(&es.stream, hipStreamNonBlocking, least) == hipSuccess;
    good = good && hipEventCreateWithFlags(&es.z_ready, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&es.joined, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&es.lin1_fork, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&es.lin1_rest, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&es.lin1_dw, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&es.caller_done, hipEventDisableTiming) == hipSuccess;
    good = good && hipEventCreateWithFlags(&es.late_done, hipEventDisableTiming) == hipSuccess;
    for (int l = 0; l < ESC_MAX_LAYERS; ++l) {
      good = good && hipEventCreateWithFlags(&es.e_ready[l], hipEventDisableTiming) == hipSuccess;
      good = good && hipEventCreateWithFlags(&es.de_ready[l], hipEventDisableTiming) == hipSuccess;
      good = good && hipEventCreateWithFlags(&es.agg_done[l], hipEventDisableTiming) == hipSuccess;
    }
    es.ok = good;
  }
  return es;
}
// The engines use the second stream only when the batch has enough edges for the edge-sized kernels to matter:
// ZINC at bs=128 (6 400 edges) measured 1.24 ms on one stream and 1.35 ms on two (the events cost more than the overlap
// returns); ogbg-molhiv at bs=256 (20 000 edges, emb 300) 5.44 -> 5.18 ms.
static int64_t g_two_stream_min_edges = 12000;       // esc_engine_set_two_stream_min_edges()
static EdgeStream& edge_stream_for(int64_t edges) {
  static thread_local EdgeStream off;   // ok == false
  return edges >= g_two_stream_min_edges ? edge_stream() : off;
}
// The fork/join protocol: `ev` marks everything queued on `src` so far; `waiter` continues only behind it.  (ESC_TRACE_LAUNCH=1
// announces both, between the launches they order.)
static int record(hipEvent_t ev, hipStream_t src) {
  if (trace_launch()) fprintf(stderr, "[esc] record event %p stream %p\n", (void*)ev, (void*)src);
  if (hipEventRecord(ev, src) != hipSuccess) { set_error("esc_engine: stream event failed"); return ESC_ELAUNCH; }
  return ESC_OK;
}
static int wait(hipStream_t waiter, hipEvent_t ev) {
  if (trace_launch()) fprintf(stderr, "[esc] wait event %p stream %p\n", (void*)ev, (void*)waiter);
  if (hipStreamWaitEvent(waiter, ev, 0) != hipSuccess) { set_error("esc_engine: stream event failed"); return ESC_ELAUNCH; }
  return ESC_OK;
}
static int chain(hipEvent_t ev, hipStream_t src, hipStream_t waiter) {
  ESC_TRY(record(ev, src));
  return wait(waiter, ev);
}

// The same dependency on the ONE kernel launched while an ArmedEvent lives.  hipEventRecord queues a marker packet behind the
// kernel and the NEXT kernel of `src` waits for that marker: 6-8 us of bubble per record in the step's kernel trace, and the node
// chain — the critical path of the backward — records once per layer.  An armed event is instead the stop event of the launch
// itself (arm_launch_event, common.h): bound to the kernel's completion signal, nothing queued behind it.  chain_armed() falls back
// to the record when no launch took the event (nothing launched, a stream being captured, on == false).  Only around calls that
// launch exactly one kernel.  g_plain_events (bit 6 of esc_engine_set_side_stream) keeps every dependency a record: A/B runs.
static int g_plain_events = 0;
struct ArmedEvent {
  ArmedEvent(hipEvent_t ev, bool on) : on_(on && !g_plain_events) { if (on_) arm_launch_event(ev); }
  ~ArmedEvent() { if (on_) (void)take_launch_event(); }
  bool on_;
};
// ... and on the LAST kernel of a call that launches several (arm_last_launch_event, common.h: the callee announces its last launch)
struct ArmedLastEvent {
  ArmedLastEvent(hipEvent_t ev, bool on) : on_(on && !g_plain_events) { if (on_) arm_last_launch_event(ev); }
  ~ArmedLastEvent() { if (on_) (void)take_last_launch_event(); }
  bool bound() const { return on_ && take_last_launch_event() == nullptr; }      // once, behind the call
  bool on_;
};
static int chain_armed(hipEvent_t ev, const ArmedEvent& arm, hipStream_t src, hipStream_t waiter) {
  const bool bound = arm.on_ && take_launch_event() == nullptr;
  if (!bound) ESC_TRY(record(ev, src));
  return waiter != nullptr ? wait(waiter, ev) : ESC_OK;
}

// The schedule's edge-term walk (engine_plan.h EdgeTerms), the same in the three forwards: `term(l)` launches e_l on the edge
// pipeline and records e_ready[l].  The terms that go out before the node pipeline starts ...
template <class Term>
static int edge_terms_up_front(const EdgeTerms& t, int64_t L, Term&& term) {
  for (int l = 0; l < (int)L; ++l)
    if (t.up_front[l]) ESC_TRY(term(l));
  return ESC_OK;
}
// ... and the one queued behind layer l's aggregate on the node stream
template <class Term>
static int edge_term_behind_agg(const EdgeTerms& t, int l, EdgeStream& es, void* node_stream, Term&& term) {
  if (t.behind_agg[l] < 0) return ESC_OK;
  ESC_TRY(chain(es.agg_done[l], (hipStream_t)node_stream, es.stream));
  return term(t.behind_agg[l]);
}

static Ctx edge_ctx(const Ctx& c, hipStream_t edge) {       // same job list / slab cursor: host-side bookkeeping only
  Ctx x = c;
  x.s = edge;
  x.on_edge_stream = true;
  x.y.bn_scratch = c.y.bn_scratch_e;
  x.y.col_stats = c.y.col_stats_e;
  return x;
}

// ---- phase marks (diagnostics, ESC_PHASE_TIMING=1): timing-enabled events at fixed points of the two pipelines, kept in a
// ring and read only by esc_engine_phase_times() after the caller has synchronised — no host/device sync inside the loop.
enum { PH_START = 0, PH_EDGE_FWD_DONE, PH_NODE_FWD_DONE, PH_NODE_BWD_DONE, PH_EDGE_BWD_DONE, PH_END, PH_COUNT };
struct PhaseRing {
  static constexpr int RING = 128;
  hipEvent_t ev[RING][PH_COUNT] = {};
  int steps = 0;
  bool on = getenv("ESC_PHASE_TIMING") != nullptr;
};
static PhaseRing& phases() { static PhaseRing p; return p; }
static void mark(int which, void* stream) {
  PhaseRing& p = phases();
  if (!p.on) return;
  hipEvent_t& e = p.ev[p.steps % PhaseRing::RING][which];
  if (e == nullptr && hipEventCreate(&e) != hipSuccess) { p.on = false; return; }
  (void)hipEventRecord(e, (hipStream_t)stream);
}

// The LAST BatchNorm+ReLU of every node MLP is not materialised: the Linear writes its pre-BatchNorm rows straight into the
// concat slice and the consumers apply relu(x*scale+shift) as they read them — the next layer's aggregate (forward and
// backward, esc_gine_aggregate_*_affine) and the readout GEMM (prologue over all (L+1)*H columns).  One elementwise launch
// less per layer on the dependent node chain.  (Schedule::node_act: ReLU models, H >= 64.)

// ---- SyncBN (esc_engine_set_collective): statistics over all ranks of a graph-sharded step ----------------------------
struct Collective {
  esc_allreduce_fn fn = nullptr; void* user = nullptr;
  int rank = 0, world = 1;
  float *buf_node = nullptr, *buf_edge = nullptr; int64_t cap = 0;
};
static Collective g_coll;
static bool sync_on(const Ctx& c) { return c.train && g_coll.fn != nullptr && g_coll.world > 1; }
// what a schedule is planned from (engine_plan.h): the entry calls this once its context has its job list
static RunMode run_mode(const Ctx& c, int64_t edges, const void* x = nullptr, bool l1_head = false) {
  RunMode r;
  r.train = c.train; r.two_stream = edge_stream_for(edges).ok; r.deferred = c.jobs != nullptr; r.sync = sync_on(c);
  r.l1_head = l1_head; r.plain_events = g_plain_events != 0; r.readout_one_launch = g_readout_one_launch != 0;
  r.x = x;
  r.linear = linear_plan_knobs(); r.aggregate = aggregate_plan_knobs(); r.bag = bag_plan_knobs();
  return r;
}
static float* sync_buf(const Ctx& c) {
  EdgeStream& es = edge_stream();
  return (es.ok && c.s == (void*)es.stream) ? g_coll.buf_edge : g_coll.buf_node;
}
static int sync_allreduce(const Ctx& c, float* buf, int64_t n) {
  ESC_REQUIRE(buf != nullptr && n <= g_coll.cap, "esc_engine: SyncBN exchange buffer too small (%ld > %ld floats)", (long)n, (long)g_coll.cap);
  const int rc = g_coll.fn(buf, n, c.s, g_coll.user);
  if (rc != 0) { set_error("esc_engine: the collective provider failed (%d)", rc); return ESC_ELAUNCH; }
  return ESC_OK;
}
// w.mean / w.invstd hold THIS rank's statistics over its M rows: replace them (and the consumer-side coefficients, the
// running statistics) by the statistics over all ranks' rows
static int bn_sync_forward(const Ctx& c, int64_t M, const esc_bn_t& bn, const BnWs& w, int64_t C) {
  float* buf = sync_buf(c);
  ESC_TRY(esc_bn_sync_pack(w.mean, w.invstd, M, bn.eps, C, g_coll.rank, g_coll.world, buf, c.s));
  ESC_TRY(sync_allreduce(c, buf, (int64_t)g_coll.world * 3 * C));
  return esc_bn_sync_finalize(buf, g_coll.world, C, bn.eps, bn.momentum, w.mean, w.invstd, bn.running_mean, bn.running_var,
                              bn.gamma, bn.beta, w.scale, w.shift, w.nglob, c.s);
}
// BatchNorm(+ReLU) backward; d(gamma), d(beta) stay this rank's sums (the gradient all-reduce adds them up)
static int bn_backward(const Ctx& c, const float* X, int64_t ldx, const float* Y, int64_t ldy, const float* dY, int64_t lddy,
                       int64_t M, const BnWs& w, const esc_bn_t& bn, float* dX, int64_t lddx, float* scratch, int64_t width = 0) {
  const int64_t C = width > 0 ? width : c.y.H;
  if (!sync_on(c))
    return esc_bn_bwd(X, ldx, Y, ldy, dY, lddy, M, C, w.mean, w.invstd, bn.gamma, bn.beta, c.act, dX, lddx, bn.dgamma, bn.dbeta,
                      scratch, c.s);
  float* buf = sync_buf(c);
  ESC_TRY(esc_bn_bwd_sums(X, ldx, Y, ldy, dY, lddy, M, C, w.mean, w.invstd, bn.gamma, bn.beta, c.act, buf, bn.dgamma, bn.dbeta,
                          scratch, c.s));
  ESC_TRY(sync_allreduce(c, buf, 2 * C));
  ESC_TRY(esc_bn_sync_coef(buf, C, w.nglob, c.s));
  return esc_bn_bwd_apply(X, ldx, Y, ldy, dY, lddy, M, C, w.mean, w.invstd, bn.gamma, bn.beta, c.act, buf, dX, lddx, c.s);
}

// BatchNorm(+ReLU) backward next to a dropout: on_output == 0: dY = grad of dropout(act(bn(X))) (mask applied to dY first);
// on_output == 1: X = dropout(input) (mask applied to the result).  `fused` (OgbSchedule::drop_*): one fused sequence
// (esc_bn_bwd_dropout), else the dropout backward as its own pass.  Dense rows (leading dimension C); ReLU / no activation only.
static int bn_backward_drop(const Ctx& c, bool fused, const float* X, int64_t ldx, const float* dY, int64_t lddy, int64_t M, const BnWs& w,
                            const esc_bn_t& bn, const uint8_t* mask, float p, int on_output, float* dX, int64_t lddx,
                            float* scratch, int64_t width = 0) {
  const int64_t C = width > 0 ? width : c.y.H;
  if (p <= 0.f) return bn_backward(c, X, ldx, nullptr, 0, dY, lddy, M, w, bn, dX, lddx, scratch, width);
  if (fused)
    return esc_bn_bwd_dropout(X, ldx, dY, lddy, M, C, w.mean, w.invstd, bn.gamma, bn.beta, c.act, mask, p, on_output, dX, lddx,
                              bn.dgamma, bn.dbeta, scratch, c.s);
  if (!on_output) {
    ESC_TRY(esc_dropout_bwd(dY, lddy, M, C, p, mask, nullptr, 0, dX, lddx, c.s));
    return bn_backward(c, X, ldx, nullptr, 0, dX, lddx, M, w, bn, dX, lddx, scratch, width);
  }
  ESC_TRY(bn_backward(c, X, ldx, nullptr, 0, dY, lddy, M, w, bn, dX, lddx, scratch, width));
  return esc_dropout_bwd(dX, lddx, M, C, p, mask, nullptr, 0, dX, lddx, c.s);
}

// Y = X*W^T + b followed by BatchNorm coefficient computation, in the pair's scheduled mode (engine_plan.h BnMode)
static int linear_bn(const Ctx& c, BnMode mode, const float* X, int64_t ld_x, const esc_linear_t& lin, const float* sc, const float* sh,
                     int64_t M, float* Y, const esc_bn_t& bn, const BnWs& w, int64_t ld_y = 0) {
  const LdsFloorGuard cap(c.on_edge_stream);
  const int64_t H = lin.out_dim, K = lin.in_dim;          // (the BatchNorm is as wide as the Linear's output)
  if (ld_y <= 0) ld_y = H;
  const bool sync = sync_on(c);     // statistics over all ranks: local ones first (no running update, no coefficients), then the exchange
  // BatchNorm statistics from the producing GEMM's epilogue (no extra pass over Y)
  const bool fused = mode == BN_EPILOGUE_PARTIALS;
  if (mode == BN_EPILOGUE_MERGED) {    // ... and their merge by the GEMM's last workgroup (no bn_finalize launch)
    esc_bn_fuse f{bn.eps, bn.momentum, w.mean, w.invstd, bn.running_mean, bn.running_var, bn.gamma, bn.beta, w.scale, w.shift};
    return esc_linear_bn_fwd(X, ld_x, lin.w, K, lin.b, sc, sh, M, H, K, Y, ld_y, c.y.col_stats, &f, c.s);
  }
  ESC_TRY(esc_linear_fwd(X, ld_x, lin.w, K, lin.b, sc, sh, M, H, K, Y, ld_y, fused ? c.y.col_stats : nullptr, c.s));
  if (fused) {
    ESC_TRY(esc_bn_stats_from_partials_rows(c.y.col_stats, M, H, esc_linear_stats_block_rows(X, ld_x, lin.w, K, M, H, K), bn.eps,
                                            bn.momentum, w.mean, w.invstd, sync ? nullptr : bn.running_mean,
                                            sync ? nullptr : bn.running_var, bn.gamma, bn.beta, sync ? nullptr : w.scale,
                                            sync ? nullptr : w.shift, c.s));
    return sync ? bn_sync_forward(c, M, bn, w, H) : ESC_OK;
  }
  if (mode == BN_STATS_PASS) {
    ESC_TRY(esc_bn_stats(Y, ld_y, M, H, bn.eps, bn.momentum, w.mean, w.invstd, sync ? nullptr : bn.running_mean,
                         sync ? nullptr : bn.running_var, bn.gamma, bn.beta, sync ? nullptr : w.scale, sync ? nullptr : w.shift,
                         c.y.bn_scratch, c.s));
    return sync ? bn_sync_forward(c, M, bn, w, H) : ESC_OK;
  }
  return esc_bn_eval_coef(bn.running_mean, bn.running_var, bn.gamma, bn.beta, bn.eps, H, w.scale, w.shift, c.s);
}

static int bn_coeffs(const Ctx& c, const float* X, int64_t ld, int64_t M, const esc_bn_t& bn, const BnWs& w, int64_t width = 0) {
  const int64_t C = width > 0 ? width : c.y.H;
  if (c.train) {
    const bool sync = sync_on(c);
    ESC_TRY(esc_bn_stats(X, ld, M, C, bn.eps, bn.momentum, w.mean, w.invstd, sync ? nullptr : bn.running_mean,
                         sync ? nullptr : bn.running_var, bn.gamma, bn.beta, sync ? nullptr : w.scale, sync ? nullptr : w.shift,
                         c.y.bn_scratch, c.s));
    return sync ? bn_sync_forward(c, M, bn, w, C) : ESC_OK;
  }
  return esc_bn_eval_coef(bn.running_mean, bn.running_var, bn.gamma, bn.beta, bn.eps, C, w.scale, w.shift, c.s);
}

// Linear, BN, ReLU, Linear, BN, ReLU  (reference :65-73, :78-87) -> out (materialised, ld_out)
static int mlp_forward(const Ctx& c, const esc_mlp_t& p, const MlpWs& w, const BnMode (&mode)[2], const float* A, int64_t ld_a, int64_t M,
                       float* out, int64_t ld_out, bool pre_out = false) {
  const int64_t H = c.y.H;
  ESC_TRY(linear_bn(c, mode[0], A, ld_a, p.lin0, nullptr, nullptr, M, w.Y0, p.bn0, w.b0));
  if (pre_out)                                // `out` receives the PRE-BatchNorm rows of lin1; w.b1 holds the coefficients
    return linear_bn(c, mode[1], w.Y0, H, p.lin1, w.b0.scale, w.b0.shift, M, out, p.bn1, w.b1, ld_out);
  if (w.A1) {                                 // activation other than ReLU: the hidden activation is written once
    ESC_TRY(esc_affine_act(w.Y0, H, M, H, w.b0.scale, w.b0.shift, c.act, w.A1, H, c.s));
    ESC_TRY(linear_bn(c, mode[1], w.A1, H, p.lin1, nullptr, nullptr, M, w.Y1, p.bn1, w.b1));
    return esc_affine_act(w.Y1, H, M, H, w.b1.scale, w.b1.shift, c.act, out, ld_out, c.s);
  }
  ESC_TRY(linear_bn(c, mode[1], w.Y0, H, p.lin1, w.b0.scale, w.b0.shift, M, w.Y1, p.bn1, w.b1));
  return esc_affine_act(w.Y1, H, M, H, w.b1.scale, w.b1.shift, 1, out, ld_out, c.s);
}

// given o.dOut (grad of the MLP's output), produce parameter grads and, if o.dA != NULL, dA — in the form the schedule chose
// (engine_plan.h MlpBwd; the fused entries refuse a call their plan does not serve)
static int mlp_backward(const Ctx& c, const MlpOps& o, const MlpBwd& how) {
  const Layout& y = c.y;
  const int64_t H = y.H, M = o.M;
  const esc_mlp_t& p = *o.p;
  const MlpWs& w = *o.w;
  if (how.fuse.lin1) {
    const esc_bn_bwd_fused f1 = mlp_fused1(y, o, c.act), f0 = mlp_fused0(y, o, c.act);
    const esc_bn_bwd_next n0 = mlp_next(y, o, c.act);
    // (activation derivatives are recomputed from the pre-BatchNorm rows everywhere — Y == NULL — so that the sums and the
    // fused apply see the same values)
    if (how.sums != SUMS_OWN_PASS)
      ESC_TRY(esc_bn_bwd_coef_from_partials(y.bst_part, how.slots, M, H, w.b1.coef, p.bn1.dgamma, p.bn1.dbeta, c.s));
    else
      ESC_TRY(esc_bn_bwd_coef(f1.x, f1.ld_x, nullptr, 0, o.dOut, o.ld_dout, M, H, w.b1.mean, w.b1.invstd, p.bn1.gamma, p.bn1.beta, c.act, w.b1.coef,
                              p.bn1.dgamma, p.bn1.dbeta, y.bn_scratch, c.s));
    ESC_TRY(linear_backward_bn(c, o.dOut, o.ld_dout, f1, w.Y0, H, w.b0.scale, w.b0.shift, p.lin1, M, y.dT2, H, 0, &n0));
    ESC_TRY(esc_bn_bwd_coef_from_partials(y.bst_part, cdiv(M, plan::bwd_bn_block_rows(M, H, H)), M, H, w.b0.coef, p.bn0.dgamma, p.bn0.dbeta, c.s));
    if (how.fuse.lin0) return linear_backward_bn(c, y.dT2, H, f0, o.A, o.ld_a, nullptr, nullptr, p.lin0, M, o.dA, o.ld_da, 0, nullptr);
    // lin0's shape is not served by the fused kernels (e.g. a 32-wide input): the apply as its own pass, then the plain backward
    ESC_TRY(esc_bn_bwd_apply(w.Y0, H, nullptr, 0, y.dT2, H, M, H, w.b0.mean, w.b0.invstd, p.bn0.gamma, p.bn0.beta, c.act, w.b0.coef, y.dT2, H, c.s));
    return linear_backward(c, y.dT2, H, o.A, o.ld_a, nullptr, nullptr, p.lin0, M, o.dA, o.ld_da, 0);
  }
  if (o.pre_out) ESC_TRY(bn_backward(c, o.out, o.ld_out, nullptr, 0, o.dOut, o.ld_dout, M, w.b1, p.bn1, y.dT1, H, y.bn_scratch));   // `out` = pre-BN rows
  else           ESC_TRY(bn_backward(c, w.Y1, H, o.out, o.ld_out, o.dOut, o.ld_dout, M, w.b1, p.bn1, y.dT1, H, y.bn_scratch));
  if (w.A1) {
    ESC_TRY(linear_backward(c, y.dT1, H, w.A1, H, nullptr, nullptr, p.lin1, M, y.dT2, H, 0));
    ESC_TRY(bn_backward(c, w.Y0, H, w.A1, H, y.dT2, H, M, w.b0, p.bn0, y.dT2, H, y.bn_scratch));
    return linear_backward(c, y.dT2, H, o.A, o.ld_a, nullptr, nullptr, p.lin0, M, o.dA, o.ld_da, 0);
  }
  ESC_TRY(linear_backward(c, y.dT1, H, w.Y0, H, w.b0.scale, w.b0.shift, p.lin1, M, y.dT2, H, 0));
  ESC_TRY(bn_backward(c, w.Y0, H, nullptr, 0, y.dT2, H, M, w.b0, p.bn0, y.dT2, H, y.bn_scratch));
  return linear_backward(c, y.dT2, H, o.A, o.ld_a, nullptr, nullptr, p.lin0, M, o.dA, o.ld_da, 0);
}

static int forward(const Ctx& c) {
  const esc_nested_gin_t* m = c.m;
  const esc_batch_t* b = c.b;
  const Layout& y = c.y;
  const Schedule& sch = c.sch;
  const int64_t N = y.N, E = y.E, H = y.H, L = y.L, W = y.W;
  // ---- edge pipeline: ESC bag, z_embedding (reference :155-156) and the edge terms e_l = lin_l(z_emb) of ALL layers
  // (:161,:169 inside GINEConv).  It touches the node chain only through e_l, so it runs on the edge stream — for batches of at
  // least g_two_stream_min_edges edges: below that (the per-rank slices of a strong-scaling run: 16 graphs, 1 900 edges) the
  // edge-sized kernels are as latency-bound as the node chain and the events cost more than the overlap returns (bs 16: 0.68 ms on
  // one stream, 0.84 on two; bs 64: 0.85 / 0.89; bs 128: 1.25 / 1.04).
  EdgeStream& es = edge_stream_for(E);
  Ctx ce = c;
  if (es.ok) {
    // the batch arrays were produced on the caller's stream.  Fast seam: ONE launch, the ESC bag, goes out in edge-stream order —
    // its index arrays were queued in front of caller_done, which the edge stream has waited for ahead of its Adam launch
    // (esc_engine_adam_step), and its table was updated by that launch; it writes workspace only.  The chain follows behind it (seam_chain
    // below): everything else the edge pipeline reads or writes — the other parameters, the BatchNorm running statistics — is ordered
    // behind the caller's stream as always, and the record's way to the edge stream is hidden behind the bag's 24 us.
    if (!c.fast_seam) ESC_TRY(chain(es.z_ready, (hipStream_t)c.s, es.stream));
    ce = edge_ctx(c, es.stream);
  }
  // ESC bag (esc_bag_fwd_rows; the LDS-staged table slices are an option that is off by default); in training mode its epilogue
  // leaves the BatchNorm partials of z_embedding's first BatchNorm, so the statistics pass over the E x H output is one finalize launch
  const int64_t bag_block = sch.bag_block;
  if (bag_block > 0) {
    ESC_TRY(esc_bag_fwd_rows(m->z_table, m->z_rows, H, b->row_ptr, b->bag_idx, b->bag_val, E, y.Zb, H, 0, ce.y.col_stats, ce.s));
    if (c.fast_seam) ESC_TRY(chain(es.z_ready, (hipStream_t)c.s, es.stream));       // seam_chain
    ESC_TRY(esc_bn_stats_from_partials_rows(ce.y.col_stats, E, H, bag_block, m->zbn0.eps, m->zbn0.momentum, y.zb0.mean, y.zb0.invstd,
                                            m->zbn0.running_mean, m->zbn0.running_var, m->zbn0.gamma, m->zbn0.beta, y.zb0.scale, y.zb0.shift, ce.s));
  } else {
    ESC_TRY(esc_bag_fwd_rows(m->z_table, m->z_rows, H, b->row_ptr, b->bag_idx, b->bag_val, E, y.Zb, H, 0, nullptr, ce.s));
    if (c.fast_seam) ESC_TRY(chain(es.z_ready, (hipStream_t)c.s, es.stream));       // seam_chain
    ESC_TRY(bn_coeffs(ce, y.Zb, H, E, m->zbn0, y.zb0));
  }
  // Edge-sized activations are materialised: the affine+ReLU prologue costs the edge-row GEMMs ~25 % (VALU-bound staging), more
  // than the two extra elementwise passes that write them once; node-sized MLP activations stay fused.
  ESC_TRY(esc_affine_act(y.Zb, H, E, H, y.zb0.scale, y.zb0.shift, 1, y.A0, H, ce.s));
  ESC_TRY(linear_bn(ce, sch.zlin, y.A0, H, m->zlin, nullptr, nullptr, E, y.Yz, m->zbn1, y.zb1));       // z_emb = relu(Yz*scale+shift)
  // The first edge term is narrow (in_dim columns: a bandwidth pass over z_emb): it applies z_embedding's last BatchNorm+ReLU to
  // its operand itself and runs BEFORE the pass that materialises z_emb for the wide layers — the node chain's first
  // aggregate waits for e_0 only (same fmaf + max per element: e_0 is bit-identical either way).  It went there when node layer 0
  // was the later pipeline; since the batched launch below the two are level (layer 0 ends with the batched GEMM), and launching
  // e_0 from the node stream instead brings the GEMM forward by 10 us without moving the end of the forward (DESIGN.md *Step
  // engine, fork and join*): it stays here.
  if (sch.e0_early) {
    const LdsFloorGuard cap(ce.on_edge_stream);
    const ArmedEvent arm(es.e_ready[0], es.ok);
    ESC_TRY(esc_linear_fwd(y.Yz, H, m->conv[0].lin.w, H, m->conv[0].lin.b, y.zb1.scale, y.zb1.shift, E, y.C0, H, y.e[0], y.ld_e[0], nullptr, ce.s));
    if (es.ok) ESC_TRY(chain_armed(es.e_ready[0], arm, es.stream, nullptr));
  }
  ESC_TRY(esc_affine_act(y.Yz, H, E, H, y.zb1.scale, y.zb1.shift, 1, y.Zemb, H, ce.s));
  // Per-layer launches (L < 3): the edge terms run one layer ahead of the node chain — e_{l+1} is queued behind the aggregate of
  // layer l and overlaps that layer's MLP, so that a bandwidth-bound aggregate never shares the HBM with an edge-sized GEMM
  // (r01: 1.255 -> 1.225 ms against two layers ahead).  From L = 3 on the batched launch below takes their place.
  auto edge_term = [&](int l) -> int {
    const LdsFloorGuard cap(ce.on_edge_stream);
    const esc_conv_t& cv = m->conv[l];
    const int64_t C = l == 0 ? y.C0 : H;
    ESC_TRY(esc_linear_fwd(y.Zemb, H, cv.lin.w, H, cv.lin.b, nullptr, nullptr, E, C, H, y.e[l], y.ld_e[l], nullptr, ce.s));
    return es.ok ? record(es.e_ready[l], es.stream) : ESC_OK;
  };
  mark(PH_START, c.s);
  const bool batched = sch.terms.batched;
  ESC_TRY(edge_terms_up_front(sch.terms, L, edge_term));
  if (batched) {                                            // e_1 .. e_{L-1} in one launch over the packed weights
    esc_table_list tl{};
    tl.count = 2 * ((int)L - 1);
    for (int l = 1; l < (int)L; ++l) {
      tl.rows[l - 1] = (int32_t)H; tl.w[l - 1] = m->conv[l].lin.w;
      tl.rows[(L - 1) + l - 1] = 1; tl.w[(L - 1) + l - 1] = m->conv[l].lin.b;
    }
    ESC_TRY(esc_table_pack(&tl, H, y.w_cat, ce.s));
    {
      const LdsFloorGuard cap(ce.on_edge_stream);
      const ArmedEvent arm(es.e_ready[1], es.ok);          // the node chain's layers 1 .. L-1 start behind this launch
      ESC_TRY(esc_linear_fwd(y.Zemb, H, y.w_cat, H, y.w_cat + (L - 1) * H * H, nullptr, nullptr, E, (L - 1) * H, H, y.e_cat, (L - 1) * H, nullptr, ce.s));
      if (es.ok) ESC_TRY(chain_armed(es.e_ready[1], arm, es.stream, nullptr));
    }
    for (int l = 2; l < (int)L; ++l)
      if (es.ok) ESC_TRY(record(es.e_ready[l], es.stream));
  }
  // ---- node pipeline (first, while it would otherwise wait for the first edge term: the chunk schedule of the bag
  // gradient, which depends on the batch's index arrays only)
  if (c.train) {                                             // ... and the BatchNorm step counters, in that same launch
    BnCounters cnt;
    cnt.n = (int)m->n_counters;
    for (int i = 0; i < cnt.n; ++i) cnt.p[i] = m->counters[i];
    ESC_TRY(bag_bwd_classify_counted(b->col_row, y.Z, H, E, y.bag_scratch, cnt, c.s));
  }
  // xs[0] = x_embedding(x) (reference :166)
  ESC_TRY(mlp_forward(c, m->xemb, y.xemb, sch.xemb, b->x, y.C0, N, y.cat, W, sch.node_act));
  // GINE layers (reference :161, :167-175): xs[l+1] -> cat[:, (l+1)H : (l+2)H]
  for (int l = 0; l < L; ++l) {
    const esc_conv_t& cv = m->conv[l];
    const int64_t C = l == 0 ? y.C0 : H;
    const float* hin = l == 0 ? b->x : y.cat + (int64_t)l * H;
    const int64_t ld_h = l == 0 ? y.C0 : W;
    // (batched edge terms: e_1 .. e_{L-1} come out of one launch, the wait in front of layer 1 covers the later layers: -7 us of step time)
    if (es.ok && !(batched && l >= 2)) ESC_TRY(wait((hipStream_t)c.s, es.e_ready[l]));
    if (sch.node_act && l > 0)          // hin = pre-BatchNorm rows of the previous layer: relu(x*scale+shift) on the fly
      ESC_TRY(esc_gine_aggregate_fwd_affine(hin, ld_h, y.cat_scale + (int64_t)l * H, y.cat_shift + (int64_t)l * H, y.e[l], y.ld_e[l], b->in_ptr,
                                            b->in_edge, b->in_src, cv.eps, N, C, y.agg[l], C, c.s));
    else
      ESC_TRY(esc_gine_aggregate_fwd(hin, ld_h, y.e[l], y.ld_e[l], b->in_ptr, b->in_edge, b->in_src, cv.eps, N, C, y.agg[l], C, c.s));
    ESC_TRY(edge_term_behind_agg(sch.terms, l, es, c.s, edge_term));
    ESC_TRY(mlp_forward(c, cv.nn, y.conv[l], sch.conv[l], y.agg[l], C, N, y.cat + (int64_t)(l + 1) * H, W, sch.node_act));
  }
  if (c.train) mark(PH_EDGE_FWD_DONE, ce.s);
  // readout (reference :183-189)
  const bool fa = sch.node_act;           // cat holds pre-BatchNorm rows: the readout GEMM applies every slice's BatchNorm+ReLU itself
  ESC_TRY(linear_bn(c, sch.readout, y.cat, W, m->lin1, fa ? y.cat_scale : nullptr, fa ? y.cat_shift : nullptr, N, y.Yl, m->bn_lin1, y.bl));
  // train_step: the head's launch leaves the L1 gradient of every prediction too, so the backward starts behind it and the loss
  // launch (a single workgroup walking all predictions, 5-7 us) leaves the chain: the edge stream continues behind the head
  // (train_step_impl() puts the loss value there)
  if (sch.l1_head) {
    const ArmedEvent arm(es.lin1_fork, es.ok);
    ESC_TRY(esc_linear_fwd_l1(y.Yl, H, m->lin2.w, m->lin2.b, y.bl.scale, y.bl.shift, N, H, c.l1_target, c.l1_denom, 1.0f, y.pred, y.dpred, c.s));
    return es.ok ? chain_armed(es.lin1_fork, arm, (hipStream_t)c.s, es.stream) : ESC_OK;
  }
  return esc_linear_fwd(y.Yl, H, m->lin2.w, H, m->lin2.b, y.bl.scale, y.bl.shift, N, 1, H, y.pred, 1, nullptr, c.s);
}

// What esc_engine_train_step_begin leaves for esc_engine_train_step_end: the join with the edge stream and the
// edge-side weight-gradient reductions.  Work the caller enqueues between the two calls (the next batch's collate)
// runs on the node stream while the edge pipeline is still finishing the step.
struct Pending {
  bool open = false;
  bool join = false;
  bool halves = false;             // opened by esc_engine_train_step_begin: the caller enqueues work between the two halves
  hipStream_t stream = nullptr;
  const float* workspace = nullptr;
  const float *z_table = nullptr, *dz_table = nullptr;      // one parameter of the edge pipeline and its gradient (see Seam)
  std::vector<esc_reduce_job> edge_jobs;
};
static Pending& pending() {
  static thread_local Pending p;
  return p;
}

// ---- the step boundary (DESIGN.md *Step engine, step boundary*).  The edge stream ends a step (bag gradient, its last slab
// reduce) and begins the next one (ESC bag, z_embedding, the edge terms); between the two only the Adam update of the parameters it
// reads is NEEDED.  The seam used to cross to the caller's stream and back: joined -> [caller] reduce, Adam over every parameter ->
// z_ready -> [edge] bag, two event hops on the critical path while the GPU is close to idle.  Now the edge stream runs its last
// reduce itself (backward()), esc_engine_adam_step() puts the update of the optimiser's LATE bucket behind it on the edge stream
// (the rest beside it on the caller's stream), and a step that follows at once starts its edge pipeline in stream order, without
// the z_ready chain in front of its first launch: the FAST SEAM.  Only that launch, the ESC bag, goes out unordered against the
// caller's stream (forward()); the chain follows behind it, so the rest of the edge pipeline (the other parameters, the BatchNorm
// running statistics it updates) keeps its order against whatever the caller queued.  The late Adam launch itself is ordered
// behind _end, not behind later work of the caller: FlatAdam.step() takes esc_adam_step_scaled when a torch op has written
// gradients, parameters or state since.  The seam is taken only when the engine knows that nothing else can have touched what the
// bag reads:
//   stage 1  esc_engine_train_step_end has just closed a two-stream step that was run in two halves.  caller_done was recorded on the
//            caller's stream in front of its wait for `joined`: behind it are the node pipeline's last launch (every reader of the
//            workspace, every gradient the node stream finishes) and whatever the caller queued between the halves (the next collate).
//   stage 2  ... and esc_engine_adam_step ran next, on that stream, over buffers that hold the step's z_table / dz_table in their late part.
//   claimed  esc_engine_claim_fast_seam: the caller says that the arrays of the next batch were queued before that _end.
// Every other engine entry (enter_engine), esc_adam_step[_scaled] (seam_reset, common.h) and esc_engine_drop_fast_seam put the
// stage back to 0, and the next step takes the z_ready chain.  g_legacy_seam (bit 8 of esc_engine_set_side_stream) keeps the former
// seam altogether: A/B runs and the tests' reference.
static int g_legacy_seam = 0;
struct Seam {
  int stage = 0;
  bool claimed = false;
  hipStream_t stream = nullptr;
  const float* workspace = nullptr;
  const float *z_table = nullptr, *dz_table = nullptr;
  const float *late_lo = nullptr, *late_hi = nullptr;        // parameters the last split update wrote in edge-stream order
  int64_t taken = 0, split_steps = 0;
};
static Seam& seam() {
  static thread_local Seam s;
  return s;
}
void seam_reset() { seam().stage = 0; seam().claimed = false; }

static int finish_pending(Pending& p) {
  if (!p.open) return ESC_OK;
  p.open = false;
  EdgeStream& es = edge_stream();
  const bool edge_reduced = p.join && p.edge_jobs.empty();      // (backward(): the edge stream has run its last reduce itself)
  if (p.join && p.halves && !g_legacy_seam) ESC_TRY(record(es.caller_done, p.stream));
  if (p.join) ESC_TRY(wait(p.stream, es.joined));
  if (!p.edge_jobs.empty()) ESC_TRY(esc_slab_reduce_jobs(p.edge_jobs.data(), (int)p.edge_jobs.size(), p.stream));
  p.edge_jobs.clear();
  mark(PH_END, p.stream);
  if (phases().on) ++phases().steps;
  Seam& sm = seam();
  seam_reset();
  if (p.halves && edge_reduced && !g_legacy_seam) {
    sm.stage = 1;
    sm.stream = p.stream; sm.workspace = p.workspace; sm.z_table = p.z_table; sm.dz_table = p.dz_table;
  }
  return ESC_OK;
}
// every entry but the two that continue a seam: an open step is closed, and whatever follows starts from the z_ready chain
static int enter_engine() {
  const int rc = finish_pending(pending());
  seam_reset();
  return rc;
}

static int backward(const Ctx& c, Pending* defer) {
  EdgeStream& es = edge_stream_for(c.y.E);
  const NodeFloorGuard node_floor(es.ok ? kNodeLdsFloorBwd : 0);
  const esc_nested_gin_t* m = c.m;
  const esc_batch_t* b = c.b;
  const Layout& y = c.y;
  const int64_t N = y.N, E = y.E, H = y.H, L = y.L, W = y.W;
  // lin2 <- dpred
  ESC_TRY(linear_backward(c, y.dpred, 1, y.Yl, H, y.bl.scale, y.bl.shift, m->lin2, N, y.dAl, H, 0));
  // bn_lin1 backward: folded into lin1's backward when the fused kernels serve its column blocks (see kBnBwdApplyInGemm)
  const Schedule& sch = c.sch;
  const bool split_lin1 = sch.split_lin1, fuse_l = sch.fuse_lin1, fa_l = sch.node_act;
  const esc_bn_bwd_fused fl = readout_fused(m, y);
  bool k0_split = false;           // the edge stream's lin1 block went out as two launches: its dW slabs are ready behind lin1_dw
  bool fork_bound = false;         // lin1_fork is the stop event of the coefficient call's last launch: no record in front of the H block
  if (fuse_l) {
    const ArmedLastEvent arm(es.lin1_fork, split_lin1);
    ESC_TRY(esc_bn_bwd_coef(y.Yl, H, nullptr, 0, y.dAl, H, N, H, y.bl.mean, y.bl.invstd, m->bn_lin1.gamma, m->bn_lin1.beta, 1, y.bl.coef,
                            m->bn_lin1.dgamma, m->bn_lin1.dbeta, y.bn_scratch, c.s));
    fork_bound = arm.bound();
  } else
    ESC_TRY(bn_backward(c, y.Yl, H, nullptr, 0, y.dAl, H, N, y.bl, m->bn_lin1, y.dAl, H, y.bn_scratch));
  // lin1 backward.  The node chain needs d(cat)[:, L*H:] (the last layer's output gradient) at once and the other
  // slices only when the first aggregate backward accumulates into them ~60 us later: with an edge stream the last
  // column block (dX slice + its dW columns) is computed here and the other L blocks over there, concurrently.
  if (split_lin1) {
    const int64_t K0 = L * H;                                 // columns [0, K0) go to the edge stream
    auto part = [&](void* stream, int64_t col0, int64_t ncols, float* db, const esc_bn_bwd_next* nx) -> int {
      Slab s;
      ESC_TRY(take_slab(c, N, H, ncols, &s));
      const bool fa = fa_l;
      if (fuse_l)
        return esc_linear_bwd_both_bn(y.dAl, H, &fl, y.cat + col0, W, fa ? y.cat_scale + col0 : nullptr, fa ? y.cat_shift + col0 : nullptr, m->lin1.w + col0, W,
                                      N, H, ncols, y.dcat + col0, W, 0, m->lin1.dw + col0, W, db, s.p, s.job, nx, stream);
      return esc_linear_bwd_both_deferred(y.dAl, H, y.cat + col0, W, fa ? y.cat_scale + col0 : nullptr, fa ? y.cat_shift + col0 : nullptr, m->lin1.w + col0, W, N, H, ncols,
                                          y.dcat + col0, W, 0, m->lin1.dw + col0, W, db, s.p, s.job, stream);
    };
    if (!fork_bound) ESC_TRY(record(es.lin1_fork, (hipStream_t)c.s));
    ESC_TRY(wait(es.stream, es.lin1_fork));
    // the node chain needs this block's dX (lin1_rest, in front of the last layer's aggregate backward) long before anyone needs
    // its dW slabs (lin1_dw, in front of the node-side slab reduce): two launches, the chain waits for the first only
    {
      const LdsFloorGuard cap(true);
      if (sch.ask_dx_split) request_dual_split(DualSplit{es.lin1_rest, es.lin1_dw, kReadoutDxLds});
      const int rc = part(es.stream, 0, K0, nullptr, nullptr);
      k0_split = !take_dual_split() && sch.ask_dx_split;                       // (a pending request: the call did not split)
      ESC_TRY(rc);
      ESC_REQUIRE(k0_split == sch.dx_split, "esc_engine: the readout block's launches disagree with the schedule");
    }
    if (!k0_split) ESC_TRY(record(es.lin1_rest, es.stream));
    // (the last layer's MLP backward follows at once: it takes the sums this block's dX tiles leave)
    const esc_bn_bwd_next nl = readout_next(y);
    ESC_TRY(part(c.s, K0, H, m->lin1.db, sch.mlp[L - 1].sums == SUMS_READOUT ? &nl : nullptr));
  } else if (fuse_l) {
    ESC_TRY(linear_backward_bn(c, y.dAl, H, fl, y.cat, W, fa_l ? y.cat_scale : nullptr, fa_l ? y.cat_shift : nullptr, m->lin1, N, y.dcat, W, 0, nullptr));
  } else {
    ESC_TRY(linear_backward(c, y.dAl, H, y.cat, W, fa_l ? y.cat_scale : nullptr, fa_l ? y.cat_shift : nullptr, m->lin1, N, y.dcat, W, 0));
  }
  // GINE layers, last to first (the eps gradients are only needed by the optimiser: one reduce launch at the end)
  Ctx ce = es.ok ? edge_ctx(c, es.stream) : c;
  std::vector<esc_reduce_job> edge_jobs;     // the edge pipeline's weight gradients are reduced after the join,
  edge_jobs.reserve(ESC_MAX_REDUCE_JOBS);    // the node pipeline's while the edge tail is still running
  if (es.ok && c.jobs) ce.jobs = &edge_jobs;
  std::vector<esc_sum_job> eps_jobs;
  for (int l = (int)L - 1; l >= 0; --l) {
    const esc_conv_t& cv = m->conv[l];
    const int64_t C = l == 0 ? y.C0 : H;
    const float* hin = l == 0 ? b->x : y.cat + (int64_t)l * H;
    const int64_t ld_h = l == 0 ? y.C0 : W;
    ESC_TRY(mlp_backward(c, conv_mlp_ops(m, y, l, sch.node_act), sch.mlp[l]));
    float* dx = l == 0 ? nullptr : y.dcat + (int64_t)l * H;            // accumulate into the previous slice
    if (split_lin1 && l == (int)L - 1) ESC_TRY(wait((hipStream_t)c.s, es.lin1_rest));      // ... which the edge stream's lin1 blocks fill
    // (kBnBwdSumsFromAgg) d(cat)[:, l*H:(l+1)*H] is final once this launch has added its share: it leaves the column sums of the PREVIOUS layer's
    // last BatchNorm backward, and that layer's MLP backward starts with the finalize
    const ArmedEvent arm(es.de_ready[l], es.ok);        // d_e[l] comes out of the aggregate backward: one launch, whichever form
    if (sch.agg[l] == AGG_AFFINE_STATS) {
      ESC_TRY(esc_gine_aggregate_bwd_affine_stats(hin, ld_h, y.cat_scale + (int64_t)l * H, y.cat_shift + (int64_t)l * H, y.conv[l - 1].b1.mean,
                                                  y.conv[l - 1].b1.invstd, y.e[l], y.ld_e[l], y.dagg, C, b->out_ptr, b->out_edge, b->out_dst, cv.eps, N, C,
                                                  y.d_e[l], C, dx, W, 1, y.deps_part + (int64_t)l * 2 * N, y.bst_part, c.s));
    } else if (sch.agg[l] == AGG_AFFINE)
      ESC_TRY(esc_gine_aggregate_bwd_affine(hin, ld_h, y.cat_scale + (int64_t)l * H, y.cat_shift + (int64_t)l * H, y.e[l], y.ld_e[l], y.dagg, C,
                                            b->out_ptr, b->out_edge, b->out_dst, cv.eps, N, C, y.d_e[l], C, dx, W, 1,
                                            y.deps_part + (int64_t)l * 2 * N, c.s));
    else
      ESC_TRY(esc_gine_aggregate_bwd(hin, ld_h, y.e[l], y.ld_e[l], y.dagg, C, b->out_ptr, b->out_edge, b->out_dst, cv.eps, N, C,
                                     y.d_e[l], C, dx, W, 1, y.deps_part + (int64_t)l * 2 * N, c.s));
    eps_jobs.push_back(esc_sum_job{y.deps_part + (int64_t)l * 2 * N, N * esc_gine_aggregate_bwd_deps_slots(C), cv.deps});
    if (es.ok) ESC_TRY(chain_armed(es.de_ready[l], arm, (hipStream_t)c.s, es.stream));   // lin_l backward: edge stream
    const float* zin = y.Zemb;
    if (l == 0 && sch.last_dw_on_node) {
      // the LAST lin backward sits in the tail of the step: only its input gradient (which completes d(z_emb)) stays on
      // the edge stream; the weight gradient runs on the node stream, which has nothing left to do.  Measured neutral when it
      // went in (1.038 vs 1.031-1.044 ms by the phase marks): the node stream's own reductions then become the end of the
      // step.  Doing the same for z_embedding's Linear costs 25-30 us (DESIGN.md *Step engine, fork and join*).
      {
        const LdsFloorGuard cap(true);
        ESC_TRY(esc_linear_bwd_input(y.d_e[l], C, cv.lin.w, H, E, C, H, y.dZemb, H, l == (int)L - 1 ? 0 : 1, es.stream));
      }
      Slab s;
      ESC_TRY(take_slab(c, E, C, H, &s));
      ESC_TRY(esc_linear_bwd_both_deferred(y.d_e[l], C, zin, H, nullptr, nullptr, cv.lin.w, H, E, C, H, nullptr, 0, 0, cv.lin.dw, H, cv.lin.db,
                                           s.p, s.job, c.s));
    } else {
      ESC_TRY(linear_backward(ce, y.d_e[l], C, zin, H, nullptr, nullptr, cv.lin, E, y.dZemb, H, l == (int)L - 1 ? 0 : 1));
    }
    if (es.ok && !edge_jobs.empty() && l > 0) {      // the edge stream now idles until d_e of the next layer: reduce these slabs there
      ESC_TRY(esc_slab_reduce_jobs(edge_jobs.data(), (int)edge_jobs.size(), es.stream));   // (l == 0: the tail of the step follows at
      edge_jobs.clear();                                                                    // once — its slabs wait for the final reduce)
    }
  }
  // x_embedding backward (input x needs no gradient): only reads d(cat)[:, 0:H]
  ESC_TRY(mlp_backward(c, xemb_mlp_ops(m, y, b->x, sch.node_act), sch.xemb_bwd));
  // z_embedding + bag: the tail of the edge pipeline (d(z_emb) is complete in edge-stream order); it overlaps the
  // x_embedding backward queued above on the node stream
  // (the ReLU mask is recomputed from the pre-BN value even though the activation was materialised: one array less to read)
  Ctx ct = ce;
  ct.on_edge_stream = false;          // the tail is the critical path: its GEMM runs at full occupancy (no LdsFloorGuard cap)
  ESC_TRY(bn_backward(ce, y.Yz, H, nullptr, 0, y.dZemb, H, E, y.zb1, m->zbn1, y.dZemb, H, ce.y.bn_scratch));
  ESC_TRY(linear_backward(ct, y.dZemb, H, y.A0, H, nullptr, nullptr, m->zlin, E, y.dAz, H, 0));
  ESC_TRY(bn_backward(ce, y.Zb, H, nullptr, 0, y.dAz, H, E, y.zb0, m->zbn0, y.dAz, H, ce.y.bn_scratch));
  ESC_TRY(esc_bag_bwd_table_rows(y.dAz, H, H, b->col_ptr, b->col_row, b->col_val, b->col_col, y.Z, m->z_rows, E,
                                 1, m->dz_table, y.bag_scratch, ce.s));
  mark(PH_NODE_BWD_DONE, c.s);
  mark(PH_EDGE_BWD_DONE, ce.s);
  // node-side reductions first (with an edge stream they overlap its tail), then join, then the edge-side ones
  if (!eps_jobs.empty()) ESC_TRY(esc_reduce_sum_jobs(eps_jobs.data(), (int)eps_jobs.size(), c.s));
  if (k0_split) ESC_TRY(wait((hipStream_t)c.s, es.lin1_dw));
  if (c.jobs && !c.jobs->empty()) ESC_TRY(esc_slab_reduce_jobs(c.jobs->data(), (int)c.jobs->size(), c.s));
  if (es.ok) {
    if (!g_legacy_seam) {
      // the edge pipeline's last slabs (z_embedding's Linear) are reduced where they were made, behind the bag gradient: the caller's
      // stream waits for `joined` as before, but nothing of the step is left to do behind that wait, and what follows on the edge
      // stream (the late bucket's Adam, the next step's bag) needs no hop to the caller's stream and back.  `joined` is the stop
      // event of the reduce launch.  Same launch, same jobs: the same bits.
      const ArmedEvent arm(es.joined, !edge_jobs.empty());
      if (!edge_jobs.empty()) ESC_TRY(esc_slab_reduce_jobs(edge_jobs.data(), (int)edge_jobs.size(), es.stream));
      edge_jobs.clear();
      ESC_TRY(chain_armed(es.joined, arm, es.stream, nullptr));
    } else
      ESC_TRY(record(es.joined, es.stream));
    Pending local;
    Pending& p = defer ? *defer : local;
    p.open = true; p.join = true; p.halves = defer != nullptr; p.stream = (hipStream_t)c.s;
    p.workspace = nullptr; p.z_table = m->z_table; p.dz_table = m->dz_table;      // (train_step_impl names the workspace)
    p.edge_jobs.swap(edge_jobs);
    if (!defer) return finish_pending(p);
  }
  return ESC_OK;
}

// =====================================================================================================================
// ZINC variant (zinc_models.py:504-611): one stream, ELU, materialised activations.  Reuses the helpers above through a
// Ctx whose count-model pointers are null.
// =====================================================================================================================
struct ZincCtx {
  const esc_zinc_gin_t* m;
  const esc_mol_batch_t* b;
  Ctx c;                       // helpers' view: layout, stream, job list, act = ELU
};

static int forward_zinc(const ZincCtx& z) {
  const esc_zinc_gin_t* m = z.m;
  const esc_mol_batch_t* b = z.b;
  const Ctx& c = z.c;
  const Layout& y = c.y;
  const int64_t N = y.N, E = y.E, H = y.H, L = y.L, W = y.W, G = y.G, D = y.D, Wz = y.Wz, C0 = y.C0;
  const int act = c.act;
  // ---- edge pipeline on the second stream (as in the counting engine): bag, z_embedding, edge-term input, edge terms
  EdgeStream& es = edge_stream_for(E);
  Ctx ce = c;
  if (es.ok) {
    ESC_TRY(chain(es.z_ready, (hipStream_t)c.s, es.stream));
    ce = edge_ctx(c, es.stream);
  }
  // z_emb = z_embedding(ESC bag) (:589-590), written into the first H columns of the edge-term input; the last D
  // columns are edge_type_embedding(edge_attr) (:591)
  ESC_TRY(esc_bag_fwd_rows(m->z_table, m->z_rows, H, b->row_ptr, b->bag_idx, b->bag_val, E, y.Zb, H, 0, nullptr, ce.s));
  if (c.train) ESC_TRY(esc_bag_bwd_classify(b->col_row, y.Z, H, E, y.bag_scratch, ce.s));
  ESC_TRY(bn_coeffs(ce, y.Zb, H, E, m->zbn0, y.zb0));
  ESC_TRY(esc_affine_act(y.Zb, H, E, H, y.zb0.scale, y.zb0.shift, act, y.A0, H, ce.s));
  ESC_TRY(linear_bn(ce, c.sch.zlin, y.A0, H, m->zlin, nullptr, nullptr, E, y.Yz, m->zbn1, y.zb1));
  ESC_TRY(esc_affine_act(y.Yz, H, E, H, y.zb1.scale, y.zb1.shift, act, y.Zcat, Wz, ce.s));
  ESC_TRY(esc_embed_fwd(m->edge_emb.w, m->edge_emb.rows, D, b->edge_type, E, y.Zcat + H, Wz, nullptr, ce.s));
  auto edge_term = [&](int l) -> int {
    const LdsFloorGuard cap(ce.on_edge_stream);
    const esc_conv_t& cv = m->conv[l];
    const int64_t C = l == 0 ? C0 : H;
    ESC_TRY(esc_linear_fwd(y.Zcat, Wz, cv.lin.w, Wz, cv.lin.b, nullptr, nullptr, E, C, Wz, y.e[l], y.ld_e[l], nullptr, ce.s));
    return es.ok ? record(es.e_ready[l], es.stream) : ESC_OK;
  };
  const Schedule& sch = c.sch;
  ESC_TRY(edge_terms_up_front(sch.terms, L, edge_term));
  if (sch.terms.batched) {            // every H-wide edge term in one launch over the packed weights (rows of Wz floats) ++ biases
    const int lb = C0 == H ? 0 : 1, nb = (int)L - lb;
    // (two packs: the weight rows are Wz wide, the biases H wide)
    esc_table_list tw{}, tb{};
    tw.count = nb; tb.count = nb;
    for (int l = lb; l < (int)L; ++l) {
      tw.rows[l - lb] = (int32_t)H; tw.w[l - lb] = m->conv[l].lin.w;
      tb.rows[l - lb] = 1; tb.w[l - lb] = m->conv[l].lin.b;
    }
    ESC_TRY(esc_table_pack(&tw, Wz, y.w_cat, ce.s));
    ESC_TRY(esc_table_pack(&tb, H, y.w_cat + (int64_t)nb * H * Wz, ce.s));
    {
      const LdsFloorGuard cap(ce.on_edge_stream);
      ESC_TRY(esc_linear_fwd(y.Zcat, Wz, y.w_cat, Wz, y.w_cat + (int64_t)nb * H * Wz, nullptr, nullptr, E, nb * H, Wz, y.e_cat, nb * H, nullptr, ce.s));
    }
    for (int l = lb; l < (int)L; ++l)
      if (es.ok) ESC_TRY(record(es.e_ready[l], es.stream));
  }
  // ---- node pipeline: x = node_type_embedding(data.x) (:581)
  ESC_TRY(esc_embed_fwd(m->node_emb.w, m->node_emb.rows, C0, b->node_type, N, y.X0, C0, nullptr, c.s));
  // GINE layers (:593-598): xs[l] -> cat[:, l*H : (l+1)*H]
  for (int l = 0; l < (int)L; ++l) {
    const esc_conv_t& cv = m->conv[l];
    const int64_t C = l == 0 ? C0 : H;
    const float* hin = l == 0 ? y.X0 : y.cat + (int64_t)(l - 1) * H;
    const int64_t ld_h = l == 0 ? C0 : W;
    if (es.ok) ESC_TRY(wait((hipStream_t)c.s, es.e_ready[l]));
    ESC_TRY(esc_gine_aggregate_fwd(hin, ld_h, y.e[l], y.ld_e[l], b->in_ptr, b->in_edge, b->in_src, cv.eps, N, C, y.agg[l], C, c.s));
    ESC_TRY(edge_term_behind_agg(sch.terms, l, es, c.s, edge_term));
    ESC_TRY(mlp_forward(c, cv.nn, y.conv[l], sch.conv[l], y.agg[l], C, N, y.cat + (int64_t)l * H, W));
  }
  // readout (:601-609): global_add_pool -> lin1 -> bn_lin1 -> ELU -> lin2; node_readout: lin1 reads the N rows of cat directly
  const int64_t R = m->node_readout ? N : G;
  const float* rin = y.cat;
  if (!m->node_readout) {
    ESC_TRY(esc_segment_pool_fwd(y.cat, W, b->graph_ptr, G, W, 0, y.pooled, W, c.s));
    rin = y.pooled;
  }
  ESC_TRY(linear_bn(c, sch.readout, rin, W, m->lin1, nullptr, nullptr, R, y.Yl, m->bn_lin1, y.bl));
  ESC_TRY(esc_affine_act(y.Yl, H, R, H, y.bl.scale, y.bl.shift, act, y.Al, H, c.s));
  ESC_TRY(esc_linear_fwd(y.Al, H, m->lin2.w, H, m->lin2.b, nullptr, nullptr, R, 1, H, y.pred, 1, nullptr, c.s));
  if (es.ok) ESC_TRY(chain(es.joined, es.stream, (hipStream_t)c.s));    // forward-only calls return ordered behind the edge stream
  return ESC_OK;
}

static int backward_zinc(const ZincCtx& z) {
  const esc_zinc_gin_t* m = z.m;
  const esc_mol_batch_t* b = z.b;
  const Ctx& c = z.c;
  const Layout& y = c.y;
  const int64_t N = y.N, E = y.E, H = y.H, L = y.L, W = y.W, G = y.G, D = y.D, Wz = y.Wz, C0 = y.C0;
  EdgeStream& es = edge_stream_for(E);
  Ctx ce = es.ok ? edge_ctx(c, es.stream) : c;
  std::vector<esc_reduce_job> edge_jobs;
  edge_jobs.reserve(ESC_MAX_REDUCE_JOBS);
  if (es.ok && c.jobs) ce.jobs = &edge_jobs;
  if (es.ok) ESC_TRY(chain(es.z_ready, (hipStream_t)c.s, es.stream));
  const int64_t R = m->node_readout ? N : G;
  ESC_TRY(linear_backward(c, y.dpred, 1, y.Al, H, nullptr, nullptr, m->lin2, R, y.dAl, H, 0));
  ESC_TRY(bn_backward(c, y.Yl, H, y.Al, H, y.dAl, H, R, y.bl, m->bn_lin1, y.dAl, H, y.bn_scratch));
  if (m->node_readout) {              // lin1's dX is the whole dcat (every column block: the layers below add into it)
    ESC_TRY(linear_backward(c, y.dAl, H, y.cat, W, nullptr, nullptr, m->lin1, N, y.dcat, W, 0));
  } else {
    ESC_TRY(linear_backward(c, y.dAl, H, y.pooled, W, nullptr, nullptr, m->lin1, G, y.dpool, W, 0));
    ESC_TRY(esc_segment_pool_bwd(y.dpool, W, b->graph_ptr, G, W, 0, y.dcat, W, c.s));
  }
  std::vector<esc_sum_job> eps_jobs;
  for (int l = (int)L - 1; l >= 0; --l) {
    const esc_conv_t& cv = m->conv[l];
    const int64_t C = l == 0 ? C0 : H;
    const float* hin = l == 0 ? y.X0 : y.cat + (int64_t)(l - 1) * H;
    const int64_t ld_h = l == 0 ? C0 : W;
    ESC_TRY(mlp_backward(c, MlpOps{&cv.nn, &y.conv[l], y.agg[l], C, N, y.cat + (int64_t)l * H, W, y.dcat + (int64_t)l * H, W, y.dagg, C, false}, c.sch.mlp[l]));
    float* dx = l == 0 ? y.dX0 : y.dcat + (int64_t)(l - 1) * H;
    ESC_TRY(esc_gine_aggregate_bwd(hin, ld_h, y.e[l], y.ld_e[l], y.dagg, C, b->out_ptr, b->out_edge, b->out_dst, cv.eps, N, C,
                                   y.d_e[l], C, dx, l == 0 ? C0 : W, l == 0 ? 0 : 1, y.deps_part + (int64_t)l * 2 * N, c.s));
    eps_jobs.push_back(esc_sum_job{y.deps_part + (int64_t)l * 2 * N, N * esc_gine_aggregate_bwd_deps_slots(C), cv.deps});
    if (es.ok) ESC_TRY(chain(es.de_ready[l], (hipStream_t)c.s, es.stream));      // conv.lin backward: edge stream
    ESC_TRY(linear_backward(ce, y.d_e[l], C, y.Zcat, Wz, nullptr, nullptr, cv.lin, E, y.dZcat, Wz, l == (int)L - 1 ? 0 : 1));
  }
  ESC_TRY(esc_embed_bwd(y.dX0, C0, b->node_type, N, m->node_emb.rows, C0, m->node_emb.dw, c.s));
  // edge pipeline tail: edge-type table, z_embedding, bag
  ESC_TRY(esc_embed_bwd(y.dZcat + H, Wz, b->edge_type, E, m->edge_emb.rows, D, m->edge_emb.dw, ce.s));
  ESC_TRY(bn_backward(ce, y.Yz, H, y.Zcat, Wz, y.dZcat, Wz, E, y.zb1, m->zbn1, y.dZemb, H, ce.y.bn_scratch));
  ESC_TRY(linear_backward(ce, y.dZemb, H, y.A0, H, nullptr, nullptr, m->zlin, E, y.dAz, H, 0));
  ESC_TRY(bn_backward(ce, y.Zb, H, y.A0, H, y.dAz, H, E, y.zb0, m->zbn0, y.dAz, H, ce.y.bn_scratch));
  ESC_TRY(esc_bag_bwd_table_rows(y.dAz, H, H, b->col_ptr, b->col_row, b->col_val, b->col_col, y.Z, m->z_rows, E, 1,
                                 m->dz_table, y.bag_scratch, ce.s));
  if (es.ok && !edge_jobs.empty()) ESC_TRY(esc_slab_reduce_jobs(edge_jobs.data(), (int)edge_jobs.size(), es.stream));
  if (!eps_jobs.empty()) ESC_TRY(esc_reduce_sum_jobs(eps_jobs.data(), (int)eps_jobs.size(), c.s));
  if (c.jobs && !c.jobs->empty()) ESC_TRY(esc_slab_reduce_jobs(c.jobs->data(), (int)c.jobs->size(), c.s));
  if (es.ok) ESC_TRY(chain(es.joined, es.stream, (hipStream_t)c.s));
  return ESC_OK;
}

static int check_zinc(const esc_zinc_gin_t* m, const esc_mol_batch_t* b, const float* ws, bool train, bool need_y) {
  ESC_REQUIRE(m && b && ws, "esc_zinc: null pointer");
  ESC_REQUIRE(m->num_layers >= 1 && m->num_layers <= ESC_MAX_LAYERS, "esc_zinc: %ld layers unsupported", (long)m->num_layers);
  ESC_REQUIRE(m->hidden > 0 && m->hidden % 4 == 0, "esc_zinc: hidden must be a multiple of 4");
  ESC_REQUIRE(m->node_emb.dim > 0 && m->node_emb.dim % 4 == 0 && m->edge_emb.dim > 0 && m->edge_emb.dim % 4 == 0,
              "esc_zinc: embedding widths must be multiples of 4");
  ESC_REQUIRE(m->conv[0].lin.in_dim == m->hidden + m->edge_emb.dim && m->conv[0].lin.out_dim == m->node_emb.dim,
              "esc_zinc: conv1.lin must map hidden + edge width to the node width");
  ESC_REQUIRE(m->node_readout == 0 || m->node_readout == 1, "esc_zinc: node_readout must be 0 or 1");
  ESC_REQUIRE(b->N >= 2 && b->E >= 2 && b->Z >= 0 && b->G >= (m->node_readout ? 1 : 2),
              "esc_zinc: batch needs >= 2 nodes, edges and %s (BatchNorm statistics)", m->node_readout ? "1 graph" : "graphs");
  ESC_REQUIRE(b->node_type && b->edge_type && b->graph_ptr && b->in_ptr && b->row_ptr &&
              (!train || ((b->y || !need_y) && b->out_ptr && b->col_ptr)), "esc_zinc: null batch arrays");
  ESC_REQUIRE(aligned16(ws), "esc_zinc: workspace must be 16-byte aligned");
  return ESC_OK;
}

static ZincCtx make_zinc(const esc_zinc_gin_t* m, const esc_mol_batch_t* b, float* ws, void* stream, bool train) {
  ZincCtx z{m, b, Ctx{nullptr, nullptr, plan_layout_zinc(m, b->N, b->E, b->Z, b->G, ws, train), stream, train}};
  z.c.act = 2;
  return z;
}

// =====================================================================================================================
// OGB molecule variant (ogb_mol_gnn.py: GNN(gnn_type='gin_eff'), virtual node, JK last): one stream, ReLU,
// materialised activations, dropout with its own counter-based stream.
// =====================================================================================================================
struct OgbCtx {
  const esc_ogb_gnn_t* m;
  const esc_ogb_batch_t* b;
  OgbLayout o;
  Ctx c;                // helpers' view (H, col_stats, bn_scratch, stream, slab cursor, jobs); act = ReLU
  float p;              // dropout probability of this call (0 in eval mode)
  OgbSchedule sch;      // every decision of this call (engine_plan.h): set once by the entry
};

static uint64_t drop_seed(const OgbCtx& z, int which) { return z.b->seed * 0x2545F4914F6CDD1Dull + (uint64_t)(which + 1) * 0xD1342543DE82EF95ull; }

static int forward_ogb(const OgbCtx& z) {
  const esc_ogb_gnn_t* m = z.m;
  const esc_ogb_batch_t* b = z.b;
  const OgbLayout& y = z.o;
  const Ctx& c = z.c;
  const int64_t N = y.N, E = y.E, H = y.H, L = y.L, G = y.G, T = y.T, H2 = 2 * H;
  const float p = z.p;
  // encoders' tables in one buffer (both pipelines read it)
  ESC_TRY(esc_table_pack(&m->tables, H, y.Tcat, c.s));
  // ---- edge pipeline (second stream, like the counting engine): ESC bag, z_embedding, the edge terms of all layers
  EdgeStream& es = edge_stream_for(E);
  Ctx ce = c;
  if (es.ok) {
    ESC_TRY(chain(es.z_ready, (hipStream_t)c.s, es.stream));
    ce = edge_ctx(c, es.stream);
  }
  // z_emb = z_embedding(ESC bag): Dropout BN ReLU Linear Dropout BN ReLU (:638-645)
  ESC_TRY(esc_bag_fwd_rows(m->z_table, m->z_rows, H, b->row_ptr, b->bag_idx, b->bag_val, E, y.Zb, H, 0, nullptr, ce.s));
  if (c.train) ESC_TRY(esc_bag_bwd_classify(b->col_row, y.Z, H, E, y.bag_scratch, ce.s));
  if (p > 0.f) ESC_TRY(esc_dropout_fwd(y.Zb, H, E, H, p, drop_seed(z, 0), nullptr, 0, y.Zd, H, y.mask_z0, ce.s));
  ESC_TRY(bn_coeffs(ce, y.Zd, H, E, m->zbn0, y.zb0));
  ESC_TRY(esc_affine_act(y.Zd, H, E, H, y.zb0.scale, y.zb0.shift, 1, y.A0, H, ce.s));
  if (p > 0.f) {
    ESC_TRY(esc_linear_fwd(y.A0, H, m->zlin.w, H, m->zlin.b, nullptr, nullptr, E, H, H, y.Yz, H, nullptr, ce.s));
    ESC_TRY(esc_dropout_fwd(y.Yz, H, E, H, p, drop_seed(z, 1), nullptr, 0, y.Yzd, H, y.mask_z1, ce.s));
    ESC_TRY(bn_coeffs(ce, y.Yzd, H, E, m->zbn1, y.zb1));
  } else {
    ESC_TRY(linear_bn(ce, z.sch.zlin, y.A0, H, m->zlin, nullptr, nullptr, E, y.Yz, m->zbn1, y.zb1));
  }
  ESC_TRY(esc_affine_act(y.Yzd, H, E, H, y.zb1.scale, y.zb1.shift, 1, y.Zemb, H, ce.s));
  // edge term of layer l = BondEncoder(edge_attr) + edge_encoder_pos(z_emb) (:352)
  auto edge_term = [&](int l) -> int {
    const LdsFloorGuard cap(ce.on_edge_stream);
    const esc_ogb_layer_t& q = m->layer[l];
    ESC_TRY(esc_linear_fwd(y.Zemb, H, q.pos.w, H, q.pos.b, nullptr, nullptr, E, H, H, y.l[l].e, H, nullptr, ce.s));
    ESC_TRY(esc_bag_fwd_rows(y.Tcat + q.bond_row0 * H, m->bond_rows, H, b->bonds.row_ptr, b->bonds.idx, b->bonds.ones, E, y.l[l].e, H, 1, nullptr, ce.s));
    return es.ok ? record(es.e_ready[l], es.stream) : ESC_OK;
  };
  // (per-layer launches, one layer ahead of the node chain as in forward(); one stream: all of them up front, in layer order)
  const OgbSchedule& sch = z.sch;
  ESC_TRY(edge_terms_up_front(sch.terms, L, edge_term));
  // ---- node pipeline: h0 = AtomEncoder(x) (:264-282); vn_0 = virtualnode_embedding(0) per graph (:701)
  ESC_TRY(esc_bag_fwd_rows(y.Tcat, m->atom_rows, H, b->atoms.row_ptr, b->atoms.idx, b->atoms.ones, N, y.h0, H, 0, nullptr, c.s));
  ESC_TRY(esc_embed_fwd(m->vn_w, 1, H, b->zero_idx, G, y.l[0].vn, H, nullptr, c.s));
  for (int l = 0; l < (int)L; ++l) {
    const esc_ogb_layer_t& q = m->layer[l];
    const OgbLayer& w = y.l[l];
    ESC_TRY(esc_segment_broadcast_add(y.h[l], H, w.vn, H, b->graph_ptr, G, N, H, w.hin, H, c.s));                 // :739
    if (es.ok) ESC_TRY(wait((hipStream_t)c.s, es.e_ready[l]));
    ESC_TRY(esc_gine_aggregate_fwd(w.hin, H, w.e, H, b->in_ptr, b->in_edge, b->in_src, q.eps, N, H, w.agg, H, c.s));
    ESC_TRY(edge_term_behind_agg(sch.terms, l, es, c.s, edge_term));
    ESC_TRY(linear_bn(c, sch.lin0[l], w.agg, H, q.lin0, nullptr, nullptr, N, w.Y0, q.bn0, w.b0));
    // relu(bn(Y0)) is applied to the staged operand of lin1 (the hidden activation is never written); + batch_norms[l] statistics
    ESC_TRY(linear_bn(c, sch.lin1[l], w.Y0, H2, q.lin1, w.b0.scale, w.b0.shift, N, w.hc, q.bn, w.bn));
    // batch_norm -> ReLU (not after the last layer) -> dropout (+ residual), :744-755, as one pass over hc
    ESC_TRY(esc_affine_act_dropout_fwd(w.hc, H, N, H, w.bn.scale, w.bn.shift, l == (int)L - 1 ? 0 : 1, p, drop_seed(z, 2 + 2 * l),
                                       m->residual ? w.hin : nullptr, H, y.h[l + 1], H, w.mask_h, c.s));
    if (l < (int)L - 1) {                                                                                            // :757-783
      ESC_TRY(esc_segment_pool_fwd(w.hin, H, b->graph_ptr, G, H, 0, w.tmp, H, c.s));
      ESC_TRY(esc_dropout_fwd(w.tmp, H, G, H, 0.f, 0, w.vn, H, w.tmp, H, nullptr, c.s));                            // + vn
      ESC_TRY(linear_bn(c, sch.vlin0[l], w.tmp, H, q.vlin0, nullptr, nullptr, G, w.V0, q.vbn0, w.vb0));
      ESC_TRY(esc_affine_act(w.V0, H2, G, H2, w.vb0.scale, w.vb0.shift, 1, w.VA, H2, c.s));
      ESC_TRY(linear_bn(c, sch.vlin1[l], w.VA, H2, q.vlin1, nullptr, nullptr, G, w.V1, q.vbn1, w.vb1));
      ESC_TRY(esc_affine_act_dropout_fwd(w.V1, H, G, H, w.vb1.scale, w.vb1.shift, 1, p, drop_seed(z, 3 + 2 * l),
                                         m->residual ? w.vn : nullptr, H, y.l[l + 1].vn, H, w.mask_v, c.s));
    }
  }
  ESC_TRY(esc_segment_pool_fwd(y.hL, H, b->graph_ptr, G, H, m->mean_pool, y.pooled, H, c.s));
  ESC_TRY(esc_linear_fwd(y.pooled, H, m->head.w, H, m->head.b, nullptr, nullptr, G, T, H, y.logits, T, nullptr, c.s));
  // a forward-only call (predict / forward_train) returns with the caller's stream ordered behind the edge stream too
  if (es.ok) ESC_TRY(chain(es.joined, es.stream, (hipStream_t)c.s));
  return ESC_OK;
}

static int backward_ogb(const OgbCtx& z) {
  const esc_ogb_gnn_t* m = z.m;
  const esc_ogb_batch_t* b = z.b;
  const OgbLayout& y = z.o;
  const Ctx& c = z.c;
  const OgbSchedule& sch = z.sch;
  Ctx c0 = c; c0.act = 0;                        // the last layer's batch_norm has no ReLU
  const int64_t N = y.N, E = y.E, H = y.H, L = y.L, G = y.G, T = y.T, H2 = 2 * H;
  const float p = z.p;
  ESC_TRY(linear_backward(c, y.dlogits, T, y.pooled, H, nullptr, nullptr, m->head, G, y.dpooled, H, 0));
  float* dH = y.dHa;                             // d h_{l+1}
  float* dHin = y.dHb;                           // d (h_l + vn_l[batch]) under construction
  ESC_TRY(esc_segment_pool_bwd(y.dpooled, H, b->graph_ptr, G, H, m->mean_pool, dH, H, c.s));
  float* dvn_next = nullptr;                     // d vn_{l+1}
  float* dvn_cur = y.dvn_a;
  std::vector<esc_sum_job> eps_jobs;
  // the edge pipeline's backward (bond tables, edge_encoder_pos, z_embedding, bag) runs on the second stream behind d_e[l]
  EdgeStream& es = edge_stream_for(E);
  Ctx ce = es.ok ? edge_ctx(c, es.stream) : c;
  std::vector<esc_reduce_job> edge_jobs;
  edge_jobs.reserve(ESC_MAX_REDUCE_JOBS);
  if (es.ok && c.jobs) ce.jobs = &edge_jobs;
  if (es.ok) ESC_TRY(chain(es.z_ready, (hipStream_t)c.s, es.stream));      // (a backward called on its own: order behind the caller's stream)
  for (int l = (int)L - 1; l >= 0; --l) {
    const esc_ogb_layer_t& q = m->layer[l];
    const OgbLayer& w = y.l[l];
    const bool last = l == (int)L - 1;
    // h_{l+1} = dropout(hb) (+ hin)
    ESC_TRY(bn_backward_drop(last ? c0 : c, sch.drop_h[l], w.hc, H, dH, H, N, w.bn, q.bn, w.mask_h, p, 0, y.dT, H, y.bn_scratch));
    if (sch.hidden_from_dx[l]) {       // the hidden BatchNorm's column sums out of lin1's dX epilogue, then finalize + apply (OgbSchedule)
      const esc_bn_bwd_next n0 = ogb_hidden_next(y, l);
      Slab s;
      ESC_TRY(take_slab(c, N, H, H2, &s));
      ESC_TRY(esc_linear_bwd_both_bn(y.dT, H, nullptr, w.Y0, H2, w.b0.scale, w.b0.shift, q.lin1.w, H2, N, H, H2, y.dA1, H2, 0, q.lin1.dw, H2,
                                     q.lin1.db, s.p, s.job, &n0, c.s));
      ESC_TRY(esc_bn_bwd_coef_from_partials(y.bst_part, sch.hidden_slots, N, H2, w.b0.coef, q.bn0.dgamma, q.bn0.dbeta, c.s));
      ESC_TRY(esc_bn_bwd_apply(w.Y0, H2, nullptr, 0, y.dA1, H2, N, H2, w.b0.mean, w.b0.invstd, q.bn0.gamma, q.bn0.beta, 1, w.b0.coef, y.dA1, H2, c.s));
    } else {
      ESC_TRY(linear_backward(c, y.dT, H, w.Y0, H2, w.b0.scale, w.b0.shift, q.lin1, N, y.dA1, H2, 0));
      ESC_TRY(bn_backward(c, w.Y0, H2, nullptr, 0, y.dA1, H2, N, w.b0, q.bn0, y.dA1, H2, y.bn_scratch, H2));      // (ReLU mask from the pre-BatchNorm rows)
    }
    ESC_TRY(linear_backward(c, y.dA1, H2, w.agg, H, nullptr, nullptr, q.lin0, N, y.dagg, H, 0));
    // virtual-node update of this layer: vn_{l+1} = dropout(mlp(add_pool(hin) + vn_l)) (+ vn_l)
    bool have_dhin = false;
    if (!last) {
      ESC_TRY(bn_backward_drop(c, sch.drop_v[l], w.V1, H, dvn_next, H, G, w.vb1, q.vbn1, w.mask_v, p, 0, y.dG2, H, y.bn_scratch));
      ESC_TRY(linear_backward(c, y.dG2, H, w.VA, H2, nullptr, nullptr, q.vlin1, G, y.dG1, H2, 0));
      ESC_TRY(bn_backward(c, w.V0, H2, nullptr, 0, y.dG1, H2, G, w.vb0, q.vbn0, y.dG1, H2, y.bn_scratch, H2));
      ESC_TRY(linear_backward(c, y.dG1, H2, w.tmp, H, nullptr, nullptr, q.vlin0, G, y.dtmp, H, 0));
      // d vn_l = d tmp (+ d vn_{l+1} through the residual); d hin = broadcast(d tmp) (+ d h_{l+1} through the residual)
      ESC_TRY(esc_dropout_bwd(y.dtmp, H, G, H, 0.f, nullptr, m->residual ? dvn_next : nullptr, H, dvn_cur, H, c.s));
      ESC_TRY(esc_segment_broadcast_add(m->residual ? dH : nullptr, H, y.dtmp, H, b->graph_ptr, G, N, H, dHin, H, c.s));
      have_dhin = true;
    } else if (m->residual) {
      float* t = dH; dH = dHin; dHin = t;          // d hin starts as d h_{l+1}: accumulate into that buffer
      have_dhin = true;
    }
    ESC_TRY(esc_gine_aggregate_bwd(w.hin, H, w.e, H, y.dagg, H, b->out_ptr, b->out_edge, b->out_dst, q.eps, N, H, w.d_e, H,
                                   dHin, H, have_dhin ? 1 : 0, y.deps_part + (int64_t)l * 2 * N, c.s));
    eps_jobs.push_back(esc_sum_job{y.deps_part + (int64_t)l * 2 * N, N * esc_gine_aggregate_bwd_deps_slots(H), q.deps});
    // edge term: bond tables and edge_encoder_pos — edge stream
    if (es.ok) ESC_TRY(chain(es.de_ready[l], (hipStream_t)c.s, es.stream));
    // bond tables: on the edge stream — except for the LAST layer processed (l == 0), whose edge-term backward opens the tail of
    // the step: there the table gradient runs on the node stream (d_e is its own product; it has the atom tables' scratch to
    // itself until the encoders below) and the edge stream goes straight to the Linear that completes d(z_emb): 4.34 -> 4.31 ms/step
    const bool bonds_on_node = l == 0 && sch.bonds_on_node;
    ESC_TRY(esc_bag_bwd_table(w.d_e, H, H, b->bonds.col_ptr, b->bonds.c_row, b->bonds.ones, b->bonds.c_col, b->bonds.n_entries,
                              m->bond_rows, y.dTcat + q.bond_row0 * H, bonds_on_node ? y.emb_scratch_n : y.emb_scratch,
                              bonds_on_node ? c.s : ce.s));
    ESC_TRY(linear_backward(ce, w.d_e, H, y.Zemb, H, nullptr, nullptr, q.pos, E, y.dZemb, H, last ? 0 : 1));
    // d hin_l is complete: d h_l = d hin_l, d vn_l += add_pool(d hin_l)
    ESC_TRY(esc_segment_pool_fwd(dHin, H, b->graph_ptr, G, H, 0, y.poolG, H, c.s));
    ESC_TRY(esc_dropout_bwd(y.poolG, H, G, H, 0.f, nullptr, last ? nullptr : dvn_cur, H, dvn_cur, H, c.s));
    dvn_next = dvn_cur;
    dvn_cur = dvn_cur == y.dvn_a ? y.dvn_b : y.dvn_a;
    { float* t = dH; dH = dHin; dHin = t; }       // dH = d h_l
  }
  // encoders
  ESC_TRY(esc_bag_bwd_table(dH, H, H, b->atoms.col_ptr, b->atoms.c_row, b->atoms.ones, b->atoms.c_col, b->atoms.n_entries,
                            m->atom_rows, y.dTcat, y.emb_scratch_n, c.s));
  ESC_TRY(esc_embed_bwd(dvn_next, H, b->zero_idx, G, 1, H, m->vn_dw, c.s));
  // z_embedding + bag: the tail of the edge pipeline (d(z_emb) is complete in edge-stream order)
  ESC_TRY(bn_backward_drop(ce, sch.drop_z1, y.Yzd, H, y.dZemb, H, E, y.zb1, m->zbn1, y.mask_z1, p, 1, y.dYz, H, ce.y.bn_scratch));
  ESC_TRY(linear_backward(ce, y.dYz, H, y.A0, H, nullptr, nullptr, m->zlin, E, y.dA0, H, 0));
  ESC_TRY(bn_backward_drop(ce, sch.drop_z0, y.Zd, H, y.dA0, H, E, y.zb0, m->zbn0, y.mask_z0, p, 1, y.dA0, H, ce.y.bn_scratch));
  ESC_TRY(esc_bag_bwd_table_rows(y.dA0, H, H, b->col_ptr, b->col_row, b->col_val, b->col_col, y.Z, m->z_rows, E, 1,
                                 m->dz_table, y.bag_scratch, ce.s));
  if (es.ok && !edge_jobs.empty()) ESC_TRY(esc_slab_reduce_jobs(edge_jobs.data(), (int)edge_jobs.size(), es.stream));
  // node-side reductions overlap the edge tail; then join and hand the packed table gradients back to the tables
  if (!eps_jobs.empty()) ESC_TRY(esc_reduce_sum_jobs(eps_jobs.data(), (int)eps_jobs.size(), c.s));
  if (c.jobs && !c.jobs->empty()) ESC_TRY(esc_slab_reduce_jobs(c.jobs->data(), (int)c.jobs->size(), c.s));
  if (es.ok) ESC_TRY(chain(es.joined, es.stream, (hipStream_t)c.s));
  return esc_table_unpack_grad(&m->tables, H, y.dTcat, c.s);
}

static int check_ogb(const esc_ogb_gnn_t* m, const esc_ogb_batch_t* b, const float* ws, bool train, bool need_y) {
  ESC_REQUIRE(m && b && ws, "esc_ogb: null pointer");
  ESC_REQUIRE(m->num_layers >= 1 && m->num_layers <= ESC_MAX_LAYERS, "esc_ogb: %ld layers unsupported", (long)m->num_layers);
  ESC_REQUIRE(m->hidden > 0 && m->hidden % 4 == 0 && m->num_tasks >= 1, "esc_ogb: hidden must be a multiple of 4");
  ESC_REQUIRE(m->drop_ratio >= 0.f && m->drop_ratio < 1.f, "esc_ogb: drop_ratio %g outside [0,1)", (double)m->drop_ratio);
  ESC_REQUIRE(m->tables.count > 0 && m->tables.count <= ESC_MAX_TABLES && m->atom_rows > 0 && m->bond_rows > 0 && m->vn_w,
              "esc_ogb: encoder tables missing");
  ESC_REQUIRE(b->N >= 2 && b->E >= 2 && b->Z >= 0 && b->G >= 2, "esc_ogb: batch needs >= 2 nodes, edges and graphs (BatchNorm statistics)");
  ESC_REQUIRE(b->graph_ptr && b->zero_idx && b->in_ptr && b->row_ptr && b->atoms.row_ptr && b->atoms.idx && b->atoms.ones &&
              b->bonds.row_ptr && b->bonds.idx && b->bonds.ones, "esc_ogb: null batch arrays");
  ESC_REQUIRE(!train || ((b->y || !need_y) && b->out_ptr && b->col_ptr && b->atoms.col_ptr && b->atoms.c_row && b->atoms.c_col &&
                         b->bonds.col_ptr && b->bonds.c_row && b->bonds.c_col && m->vn_dw), "esc_ogb: null training arrays");
  ESC_REQUIRE(aligned16(ws), "esc_ogb: workspace must be 16-byte aligned");
  return ESC_OK;
}

static OgbCtx make_ogb(const esc_ogb_gnn_t* m, const esc_ogb_batch_t* b, float* ws, void* stream, bool train) {
  OgbCtx z{m, b, plan_layout_ogb(m, b->N, b->E, b->Z, b->G, b->atoms.n_entries, b->bonds.n_entries, ws, train),
           Ctx{nullptr, nullptr, Layout{}, stream, train}, train ? m->drop_ratio : 0.f};
  z.c.y.H = m->hidden; z.c.y.N = b->N; z.c.y.E = b->E;
  z.c.y.col_stats = z.o.col_stats; z.c.y.bn_scratch = z.o.bn_scratch;
  z.c.y.col_stats_e = z.o.col_stats_e; z.c.y.bn_scratch_e = z.o.bn_scratch_e;
  z.c.act = 1;
  return z;
}

static int check(const esc_nested_gin_t* m, const esc_batch_t* b, const float* ws, bool train, bool need_y = true) {
  ESC_REQUIRE(m && b && ws, "esc_engine: null pointer");
  ESC_REQUIRE(m->num_layers >= 1 && m->num_layers <= ESC_MAX_LAYERS, "esc_engine: %ld layers unsupported", (long)m->num_layers);
  ESC_REQUIRE(m->hidden > 0 && m->hidden % 4 == 0 && m->in_dim > 0, "esc_engine: hidden must be a multiple of 4");
  ESC_REQUIRE(b->N >= 2 && b->E >= 2 && b->Z >= 0, "esc_engine: batch needs >= 2 nodes and edges (BatchNorm statistics)");
  ESC_REQUIRE(b->x && b->in_ptr && b->row_ptr && (!train || ((b->y || !need_y) && b->out_ptr && b->col_ptr)), "esc_engine: null batch arrays");
  ESC_REQUIRE(aligned16(ws), "esc_engine: workspace must be 16-byte aligned");
  ESC_REQUIRE(m->n_counters >= 0 && m->n_counters <= ESC_MAX_BN_COUNTERS, "esc_engine: bad BatchNorm counter list");
  for (int64_t i = 0; i < m->n_counters; ++i) ESC_REQUIRE(m->counters[i] != nullptr, "esc_engine: null BatchNorm counter");
  return ESC_OK;
}

static int copy_floats(float* dst, const float* src, int64_t n, void* stream, const char* what) {
  if (hipMemcpyAsync(dst, src, sizeof(float) * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess) {
    set_error("%s: copy failed", what);
    return ESC_ELAUNCH;
  }
  return ESC_OK;
}

}  // namespace esc

using namespace esc;

extern "C" {

int esc_engine_set_two_stream_min_edges(int64_t edges) {
  g_two_stream_min_edges = edges < 0 ? 0 : edges;
  return ESC_OK;
}

/* bit 1: the edge pipeline on a second stream; bit 6: every cross-stream dependency an event record (see ArmedEvent) and the readout
 * block one launch; bit 7: the readout Linear's edge-stream block one launch (see kReadoutDxLds); bit 8: the former boundary between
 * two steps, through the caller's stream (see Seam).  The other bits selected schedules
 * that have been retired (DESIGN.md *Retired step-engine switches*) and are ignored. */
int esc_engine_set_side_stream(int on) {
  g_use_edge_stream = (on & 2) != 0;
  g_plain_events = (on & 64) != 0;
  g_readout_one_launch = (on & 128) != 0;
  g_legacy_seam = (on & 256) != 0;
  seam_reset();
  return ESC_OK;
}

/* ---- the step boundary (escgnn_step.h; see Seam) -------------------------------------------------------------------------- */
int esc_engine_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int64_t n_early,
                         double lr, double beta1, double beta2, double eps, int64_t step, void* stream) {
  ESC_REQUIRE(param && grad && exp_avg && exp_avg_sq, "esc_engine_adam_step: null pointer");
  ESC_REQUIRE(n >= 0 && n_early >= 0 && n_early <= n && step >= 1, "esc_engine_adam_step: bad n/n_early/step");
  Seam& sm = seam();
  // the buffers are the ones the step that has just ended trained: its edge parameters and their gradients lie in the late part
  const bool split = sm.stage == 1 && !g_legacy_seam && sm.stream == (hipStream_t)stream && n_early < n &&
                     sm.z_table >= param + n_early && sm.z_table < param + n && sm.dz_table >= grad + n_early && sm.dz_table < grad + n;
  seam_reset();
  if (!split) return adam_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, nullptr, stream);
  EdgeStream& es = edge_stream();          // (stage 1: the step ran on it)
  if (!es.ok) return adam_launch(param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step, nullptr, stream);
  // the late part on the edge stream, behind its last reduce and behind caller_done (the gradients of that part which the node
  // stream finishes: conv[0].lin's, reduced with the node-side jobs); late_done is the stop event of the launch
  ESC_TRY(wait(es.stream, es.caller_done));
  {
    const ArmedEvent arm(es.late_done, true);
    ESC_TRY(adam_launch(param + n_early, grad + n_early, exp_avg + n_early, exp_avg_sq + n_early, n - n_early, lr, beta1, beta2, eps, step,
                        nullptr, es.stream));
    ESC_TRY(chain_armed(es.late_done, arm, es.stream, nullptr));
  }
  // ... the rest beside it; the caller's stream then holds every parameter in its order, as after one launch over all of them
  ESC_TRY(adam_launch(param, grad, exp_avg, exp_avg_sq, n_early, lr, beta1, beta2, eps, step, nullptr, stream));
  ESC_TRY(wait((hipStream_t)stream, es.late_done));
  sm.stage = 2;
  sm.late_lo = param + n_early; sm.late_hi = param + n;
  ++sm.split_steps;
  return ESC_OK;
}

int esc_engine_claim_fast_seam(void) {
  Seam& sm = seam();
  sm.claimed = sm.stage == 2;
  return ESC_OK;
}

int esc_engine_drop_fast_seam(void) {
  seam_reset();
  return ESC_OK;
}

int64_t esc_engine_seam_count(int which) { return which == 0 ? seam().taken : which == 1 ? seam().split_steps : -1; }

/* diagnostics: mean milliseconds between the phase marks of the last recorded steps (ESC_PHASE_TIMING=1); call after a
 * device synchronise.  out[0..5]: start->edge-forward done, start->node-forward done, node-forward done->node-backward done,
 * node-backward done->edge-backward done (negative: the edge pipeline finished first), start->end of step, end->next start */
int esc_engine_phase_times(double* out, int skip) {
  PhaseRing& p = phases();
  for (int i = 0; i < 6; ++i) out[i] = 0.0;
  if (!p.on || p.steps < 2) return 0;
  const int first = p.steps > PhaseRing::RING ? p.steps - PhaseRing::RING + 1 : 0;
  int n = 0;
  for (int sidx = first + skip; sidx < p.steps; ++sidx) {
    hipEvent_t* e = p.ev[sidx % PhaseRing::RING];
    bool ok = true;
    for (int k = 0; k < PH_COUNT; ++k) ok = ok && e[k] != nullptr;
    if (!ok) continue;
    float t[6] = {};
    if (hipEventElapsedTime(&t[0], e[PH_START], e[PH_EDGE_FWD_DONE]) != hipSuccess) continue;
    (void)hipEventElapsedTime(&t[1], e[PH_START], e[PH_NODE_FWD_DONE]);
    (void)hipEventElapsedTime(&t[2], e[PH_NODE_FWD_DONE], e[PH_NODE_BWD_DONE]);
    if (hipEventElapsedTime(&t[3], e[PH_NODE_BWD_DONE], e[PH_EDGE_BWD_DONE]) != hipSuccess) {
      (void)hipEventElapsedTime(&t[3], e[PH_EDGE_BWD_DONE], e[PH_NODE_BWD_DONE]); t[3] = -t[3];
    }
    (void)hipEventElapsedTime(&t[4], e[PH_START], e[PH_END]);
    if (sidx + 1 < p.steps) (void)hipEventElapsedTime(&t[5], e[PH_END], p.ev[(sidx + 1) % PhaseRing::RING][PH_START]);
    for (int i = 0; i < 6; ++i) out[i] += t[i];
    ++n;
  }
  for (int i = 0; i < 6; ++i) out[i] /= n > 0 ? n : 1;
  return n;
}

int esc_engine_set_collective(esc_allreduce_fn fn, void* user, int rank, int world, float* buf_node, float* buf_edge,
                              int64_t cap) {
  ESC_REQUIRE(fn == nullptr || (world >= 1 && rank >= 0 && rank < world && buf_node && buf_edge && cap > 0),
              "esc_engine_set_collective: bad argument");
  g_coll = Collective{fn, user, rank, world < 1 ? 1 : world, buf_node, buf_edge, cap};
  return ESC_OK;
}

int64_t esc_engine_workspace_floats(const esc_nested_gin_t* m, int64_t N, int64_t E, int64_t Z) {
  if (!m || N < 0 || E < 0 || Z < 0) return -1;
  return plan_layout(m, N, E, Z, nullptr, true).total;
}

static int train_step_impl(const esc_nested_gin_t* m, const esc_batch_t* b, float* workspace,
                           int64_t loss_denom, float* loss, float* pred, void* stream, Pending* defer);

int esc_engine_train_step(const esc_nested_gin_t* m, const esc_batch_t* b, float* workspace,
                          int64_t loss_denom, float* loss, float* pred, void* stream) {
  ESC_TRY(enter_engine());
  return train_step_impl(m, b, workspace, loss_denom, loss, pred, stream, nullptr);
}

int esc_engine_train_step_begin(const esc_nested_gin_t* m, const esc_batch_t* b, float* workspace,
                                int64_t loss_denom, float* loss, float* pred, void* stream) {
  ESC_TRY(finish_pending(pending()));      // (not enter_engine: a split optimiser step in front of this call keeps its seam)
  return train_step_impl(m, b, workspace, loss_denom, loss, pred, stream, &pending());
}


int esc_engine_train_step_end(void) { return finish_pending(pending()); }

static int train_step_impl(const esc_nested_gin_t* m, const esc_batch_t* b, float* workspace,
                           int64_t loss_denom, float* loss, float* pred, void* stream, Pending* defer) {
  // (a claim is for this call only, whatever becomes of it: taken off before the first return)
  Seam& sm = seam();
  const bool seam_offered = defer != nullptr && sm.stage == 2 && sm.claimed && !g_legacy_seam;
  seam_reset();
  int rc = check(m, b, workspace, true);
  if (rc) return rc;
  ESC_REQUIRE(loss, "esc_engine_train_step: null loss pointer");
  Ctx c{m, b, plan_layout(m, b->N, b->E, b->Z, workspace, true), stream, true};
  StepSlabs slabs(c, c.y.slabs, c.y.slab_limit, c.y.n_wgrads);
  c.sch = plan_schedule(m, c.y, run_mode(c, b->E, b->x, true));
  const int64_t denom = loss_denom > 0 ? loss_denom : b->N;
  EdgeStream& es = edge_stream_for(b->E);
  const bool head_l1 = c.sch.l1_head;
  if (head_l1) { c.l1_target = b->y; c.l1_denom = denom; }
  // the fast seam (see Seam): this call follows a split optimiser step at once, on the same stream and workspace, the caller has
  // claimed the batch, and the one parameter the ESC bag reads was updated on the edge stream
  c.fast_seam = seam_offered && es.ok && !sync_on(c) && sm.stream == (hipStream_t)stream && sm.workspace == workspace &&
                m->z_table >= sm.late_lo && m->z_table < sm.late_hi;
  if (c.fast_seam) ++sm.taken;
  ESC_TRY(forward(c));
  if (head_l1) {              // the loss VALUE: on the edge stream (idle here), ordered behind the head by forward(); the step's join covers it
    ESC_TRY(esc_l1_loss(c.y.pred, b->y, b->N, denom, 1.0f, loss, nullptr, es.stream));
  } else {
    ESC_TRY(esc_l1_loss(c.y.pred, b->y, b->N, denom, 1.0f, loss, c.y.dpred, stream));
  }
  mark(PH_NODE_FWD_DONE, stream);
  if (pred) ESC_TRY(copy_floats(pred, c.y.pred, b->N, stream, "esc_engine_train_step"));
  rc = backward(c, defer);
  if (defer != nullptr) defer->workspace = workspace;      // (what the next call's argument is compared with)
  return rc;
}

// The step as an autograd node: forward in training mode (batch statistics, activations kept in `workspace`), then —
// with the gradient of ANY loss w.r.t. the predictions — the backward.  The workspace must be left untouched in
// between.  This is what lets `NestedGIN_eff.forward` itself run on the engine inside a user's own training loop.
int esc_engine_forward_train(const esc_nested_gin_t* m, const esc_batch_t* b, float* workspace, float* pred,
                             void* stream) {
  ESC_TRY(enter_engine());
  int rc = check(m, b, workspace, true, false);
  if (rc) return rc;
  ESC_REQUIRE(pred, "esc_engine_forward_train: null output");
  Ctx c{m, b, plan_layout(m, b->N, b->E, b->Z, workspace, true), stream, true};
  StepSlabs slabs(c, c.y.slabs, c.y.slab_limit, 0);
  c.sch = plan_schedule(m, c.y, run_mode(c, b->E, b->x));
  ESC_TRY(forward(c));
  return copy_floats(pred, c.y.pred, b->N, stream, "esc_engine_forward_train");
}

int esc_engine_backward(const esc_nested_gin_t* m, const esc_batch_t* b, float* workspace, const float* dpred,
                        void* stream) {
  ESC_TRY(enter_engine());
  int rc = check(m, b, workspace, true, false);
  if (rc) return rc;
  ESC_REQUIRE(dpred, "esc_engine_backward: null gradient");
  Ctx c{m, b, plan_layout(m, b->N, b->E, b->Z, workspace, true), stream, true};
  StepSlabs slabs(c, c.y.slabs, c.y.slab_limit, c.y.n_wgrads);
  c.sch = plan_schedule(m, c.y, run_mode(c, b->E, b->x));
  ESC_TRY(copy_floats(c.y.dpred, dpred, b->N, stream, "esc_engine_backward"));
  return backward(c, nullptr);
}

int esc_engine_predict(const esc_nested_gin_t* m, const esc_batch_t* b, float* workspace, float* pred,
                       void* stream) {
  ESC_TRY(enter_engine());
  int rc = check(m, b, workspace, false);
  if (rc) return rc;
  ESC_REQUIRE(pred, "esc_engine_predict: null output");
  Ctx c{m, b, plan_layout(m, b->N, b->E, b->Z, workspace, false), stream, false};
  c.sch = plan_schedule(m, c.y, run_mode(c, b->E, b->x));
  ESC_TRY(forward(c));
  return copy_floats(pred, c.y.pred, b->N, stream, "esc_engine_predict");
}

// ---- ZINC variant ------------------------------------------------------------------------------------------------------
int64_t esc_zinc_workspace_floats(const esc_zinc_gin_t* m, int64_t N, int64_t E, int64_t Z, int64_t G) {
  if (!m || N < 0 || E < 0 || Z < 0 || G < 0) return -1;
  return plan_layout_zinc(m, N, E, Z, G, nullptr, true).total + 64;
}

// rows of pred / dpred / y: one per graph, or one per node (node_readout)
static int64_t zinc_rows(const esc_zinc_gin_t* m, const esc_mol_batch_t* b) { return m->node_readout ? b->N : b->G; }

int esc_zinc_train_step(const esc_zinc_gin_t* m, const esc_mol_batch_t* b, float* workspace, int64_t loss_denom,
                        float* loss, float* pred, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_zinc(m, b, workspace, true, true);
  if (rc) return rc;
  ESC_REQUIRE(loss, "esc_zinc_train_step: null loss pointer");
  ZincCtx z = make_zinc(m, b, workspace, stream, true);
  StepSlabs slabs(z.c, z.c.y.slabs, z.c.y.slab_limit, z.c.y.n_wgrads);
  z.c.sch = plan_schedule_zinc(m, z.c.y, run_mode(z.c, b->E));
  const int64_t R = zinc_rows(m, b);
  ESC_TRY(forward_zinc(z));
  ESC_TRY(esc_l1_loss(z.c.y.pred, b->y, R, loss_denom > 0 ? loss_denom : R, 1.0f, loss, z.c.y.dpred, stream));
  if (pred) ESC_TRY(copy_floats(pred, z.c.y.pred, R, stream, "esc_zinc_train_step"));
  return backward_zinc(z);
}

int esc_zinc_forward_train(const esc_zinc_gin_t* m, const esc_mol_batch_t* b, float* workspace, float* pred, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_zinc(m, b, workspace, true, false);
  if (rc) return rc;
  ESC_REQUIRE(pred, "esc_zinc_forward_train: null output");
  ZincCtx z = make_zinc(m, b, workspace, stream, true);
  StepSlabs slabs(z.c, z.c.y.slabs, z.c.y.slab_limit, 0);
  z.c.sch = plan_schedule_zinc(m, z.c.y, run_mode(z.c, b->E));
  ESC_TRY(forward_zinc(z));
  return copy_floats(pred, z.c.y.pred, zinc_rows(m, b), stream, "esc_zinc_forward_train");
}

int esc_zinc_backward(const esc_zinc_gin_t* m, const esc_mol_batch_t* b, float* workspace, const float* dpred, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_zinc(m, b, workspace, true, false);
  if (rc) return rc;
  ESC_REQUIRE(dpred, "esc_zinc_backward: null gradient");
  ZincCtx z = make_zinc(m, b, workspace, stream, true);
  StepSlabs slabs(z.c, z.c.y.slabs, z.c.y.slab_limit, z.c.y.n_wgrads);
  z.c.sch = plan_schedule_zinc(m, z.c.y, run_mode(z.c, b->E));
  ESC_TRY(copy_floats(z.c.y.dpred, dpred, zinc_rows(m, b), stream, "esc_zinc_backward"));
  return backward_zinc(z);
}

int esc_zinc_predict(const esc_zinc_gin_t* m, const esc_mol_batch_t* b, float* workspace, float* pred, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_zinc(m, b, workspace, false, false);
  if (rc) return rc;
  ESC_REQUIRE(pred, "esc_zinc_predict: null output");
  ZincCtx z = make_zinc(m, b, workspace, stream, false);
  z.c.sch = plan_schedule_zinc(m, z.c.y, run_mode(z.c, b->E));
  ESC_TRY(forward_zinc(z));
  return copy_floats(pred, z.c.y.pred, zinc_rows(m, b), stream, "esc_zinc_predict");
}

// ---- OGB molecule variant ------------------------------------------------------------------------------------------------
int64_t esc_ogb_workspace_floats(const esc_ogb_gnn_t* m, int64_t N, int64_t E, int64_t Z, int64_t G, int64_t atom_entries,
                                 int64_t bond_entries) {
  if (!m || N < 0 || E < 0 || Z < 0 || G < 0 || atom_entries < 0 || bond_entries < 0) return -1;
  return plan_layout_ogb(m, N, E, Z, G, atom_entries, bond_entries, nullptr, true).total + 64;
}

int esc_ogb_train_step(const esc_ogb_gnn_t* m, const esc_ogb_batch_t* b, float* workspace, int64_t loss_denom, float* loss,
                       float* logits, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_ogb(m, b, workspace, true, true);
  if (rc) return rc;
  ESC_REQUIRE(loss, "esc_ogb_train_step: null loss pointer");
  OgbCtx z = make_ogb(m, b, workspace, stream, true);
  StepSlabs slabs(z.c, z.o.slabs, z.o.slab_limit, z.o.n_wgrads);
  z.sch = plan_schedule_ogb(m, z.o, run_mode(z.c, b->E));
  ESC_TRY(forward_ogb(z));
  ESC_TRY(esc_bce_logits_loss(z.o.logits, b->y, b->G * m->num_tasks, loss_denom, loss, z.o.dlogits, stream));
  if (logits) ESC_TRY(copy_floats(logits, z.o.logits, b->G * m->num_tasks, stream, "esc_ogb_train_step"));
  return backward_ogb(z);
}

int esc_ogb_forward_train(const esc_ogb_gnn_t* m, const esc_ogb_batch_t* b, float* workspace, float* logits, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_ogb(m, b, workspace, true, false);
  if (rc) return rc;
  ESC_REQUIRE(logits, "esc_ogb_forward_train: null output");
  OgbCtx z = make_ogb(m, b, workspace, stream, true);
  StepSlabs slabs(z.c, z.o.slabs, z.o.slab_limit, 0);
  z.sch = plan_schedule_ogb(m, z.o, run_mode(z.c, b->E));
  ESC_TRY(forward_ogb(z));
  return copy_floats(logits, z.o.logits, b->G * m->num_tasks, stream, "esc_ogb_forward_train");
}

int esc_ogb_backward(const esc_ogb_gnn_t* m, const esc_ogb_batch_t* b, float* workspace, const float* dlogits, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_ogb(m, b, workspace, true, false);
  if (rc) return rc;
  ESC_REQUIRE(dlogits, "esc_ogb_backward: null gradient");
  OgbCtx z = make_ogb(m, b, workspace, stream, true);
  StepSlabs slabs(z.c, z.o.slabs, z.o.slab_limit, z.o.n_wgrads);
  z.sch = plan_schedule_ogb(m, z.o, run_mode(z.c, b->E));
  ESC_TRY(copy_floats(z.o.dlogits, dlogits, b->G * m->num_tasks, stream, "esc_ogb_backward"));
  return backward_ogb(z);
}

int esc_ogb_predict(const esc_ogb_gnn_t* m, const esc_ogb_batch_t* b, float* workspace, float* logits, void* stream) {
  ESC_TRY(enter_engine());
  int rc = check_ogb(m, b, workspace, false, false);
  if (rc) return rc;
  ESC_REQUIRE(logits, "esc_ogb_predict: null output");
  OgbCtx z = make_ogb(m, b, workspace, stream, false);
  z.sch = plan_schedule_ogb(m, z.o, run_mode(z.c, b->E));
  ESC_TRY(forward_ogb(z));
  return copy_floats(logits, z.o.logits, b->G * m->num_tasks, stream, "esc_ogb_predict");
}

}  // extern "C"
