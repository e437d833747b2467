// engine_plan.h — what the three step engines (engine.hip: counting, ZINC, OGB-mol) decide on the host before anything is launched:
// the workspace layout of a call, the weight gradients a training step produces, and how much split-M slab scratch and how many
// deferred reduce jobs they take, and the SCHEDULE of the call (second half of this file: every decision the bodies used to take
// between their launches).  Host-only, no HIP header: tests/engine_plan_host.cpp and tests/engine_schedule_host.cpp compile it with a
// plain host compiler under sanitizers.  The weight_grads* functions are the ONLY place that enumerates a family's weight gradients: the slab region
// of the layout (slab_floats), the job budget of the entries (reduce_jobs) and the bound of the cursor that the backward* bodies
// take their regions from (SlabCursor) all derive from that list.
#pragma once
#include <cstdint>
#include <vector>

#include "linear_plan.h"
#include "norm_plan.h"
#include "sparse_plan.h"
#include "../../include/escgnn_step.h"

namespace esc {

inline int64_t round64(int64_t n) { return (n + 63) & ~63LL; }          // 256-byte granules keep every buffer float4-aligned

struct Arena {
  float* base;
  int64_t off;
  float* take(int64_t n) {
    float* p = base ? base + off : nullptr;
    off += round64(n);
    return p;
  }
};

// ---- the weight gradients of one training step --------------------------------------------------------------------------
struct WGrad { int64_t M, N, K; };          // rows, out_dim, in_dim: dW [N, K] (+ db [N]) summed over M rows
struct WGradList {
  std::vector<WGrad> g;                     // in the order the family's backward issues them
  int split = -1;                           // >= 0: g[split], g[split + 1] are column blocks of ONE Linear (same M, N), which a
};                                          // backward that does not split it reduces whole, as (M, N, K0 + K1)

// counting model: lin2; lin1 as its column blocks [0, L*H) (edge stream) and [L*H, W) (node chain); per GINE layer nn.lin1, nn.lin0,
// conv.lin; x_embedding's two; z_embedding's Linear
inline WGradList weight_grads(const esc_nested_gin_t* m, int64_t N, int64_t E) {
  const int64_t H = m->hidden, L = m->num_layers, C0 = m->in_dim;
  WGradList w;
  w.g.push_back({N, 1, H});
  w.split = (int)w.g.size();
  w.g.push_back({N, H, L * H});
  w.g.push_back({N, H, H});
  for (int64_t l = L - 1; l >= 0; --l) {
    const int64_t C = l == 0 ? C0 : H;
    w.g.push_back({N, H, H});
    w.g.push_back({N, H, C});
    w.g.push_back({E, C, H});
  }
  w.g.push_back({N, H, H});
  w.g.push_back({N, H, C0});
  w.g.push_back({E, H, H});
  return w;
}

// ZINC: lin2, lin1 over the R readout rows (graphs, or nodes with node_readout); per layer nn.lin1, nn.lin0, conv.lin over
// [z_emb | edge type]; z_embedding's Linear
inline WGradList weight_grads_zinc(const esc_zinc_gin_t* m, int64_t N, int64_t E, int64_t G) {
  const int64_t H = m->hidden, L = m->num_layers, C0 = m->node_emb.dim, Wz = H + m->edge_emb.dim, R = m->node_readout ? N : G;
  WGradList w;
  w.g.push_back({R, 1, H});
  w.g.push_back({R, H, L * H});
  for (int64_t l = L - 1; l >= 0; --l) {
    const int64_t C = l == 0 ? C0 : H;
    w.g.push_back({N, H, H});
    w.g.push_back({N, H, C});
    w.g.push_back({E, C, Wz});
  }
  w.g.push_back({E, H, H});
  return w;
}

// OGB-mol: the head; per layer mlp's lin1, lin0, the virtual-node MLP's vlin1, vlin0 (not in the last layer), edge_encoder_pos;
// z_embedding's Linear
inline WGradList weight_grads_ogb(const esc_ogb_gnn_t* m, int64_t N, int64_t E, int64_t G) {
  const int64_t H = m->hidden, L = m->num_layers, T = m->num_tasks, H2 = 2 * H;
  WGradList w;
  w.g.push_back({G, T, H});
  for (int64_t l = L - 1; l >= 0; --l) {
    w.g.push_back({N, H, H2});
    w.g.push_back({N, H2, H});
    if (l < L - 1) {
      w.g.push_back({G, H, H2});
      w.g.push_back({G, H2, H});
    }
    w.g.push_back({E, H, H});
  }
  w.g.push_back({E, H, H});
  return w;
}

inline int64_t slab_floats(const WGrad& g) { return round64(plan::bwd_weight_scratch(g.M, g.N, g.K)); }
// one private region per weight gradient; a split Linear gets the larger of its two forms (the `fine` granularity of
// bwd_weight_scratch can differ between the whole and its blocks)
inline int64_t slab_floats(const WGradList& w) {
  int64_t total = 0;
  for (const WGrad& g : w.g) total += slab_floats(g);
  if (w.split >= 0) {
    const WGrad &a = w.g[w.split], &b = w.g[w.split + 1];
    const int64_t blocks = slab_floats(a) + slab_floats(b), whole = slab_floats(WGrad{a.M, a.N, a.K + b.K});
    if (whole > blocks) total += whole - blocks;
  }
  return total;
}
inline int reduce_jobs(const WGradList& w) { return (int)w.g.size(); }          // one deferred reduce per weight gradient

// The slab region as the backward walks it: every weight gradient takes its own part, nothing past `limit`.
struct SlabCursor {
  float* base;
  int64_t off, limit;
  float* peek() const { return base + off; }                 // where the next region starts (the `_ok` probes look at its alignment)
  float* take(int64_t M, int64_t N, int64_t K) {             // null: the region is exhausted
    const int64_t n = round64(plan::bwd_weight_scratch(M, N, K));
    if (off + n > limit) return nullptr;
    float* p = base + off;
    off += n;
    return p;
  }
};

// ---- workspace layouts ------------------------------------------------------------------------------------------------------
struct BnWs { float *mean, *invstd, *scale, *shift, *nglob, *coef; };     // nglob: rows over all ranks (SyncBN); coef: float2[C] of the backward
struct MlpWs { float *Y0, *Y1; BnWs b0, b1; float* A1 = nullptr; };   // A1: materialised hidden activation (ELU models)

struct Layout {
  int64_t N, E, Z, H, L, C0, W;   // W = (L+1)*H
  // forward state
  float *Zb, *Yz; BnWs zb0, zb1;
  float *A0, *Zemb;               // relu(BN(Zb)) and z_emb = relu(BN(Yz)), materialised (see forward())
  float* e[ESC_MAX_LAYERS]; float* agg[ESC_MAX_LAYERS]; MlpWs conv[ESC_MAX_LAYERS];
  int64_t ld_e[ESC_MAX_LAYERS];   // leading dimension of e[l]: C, or (L-1)*H when the H-wide edge terms are column blocks of ONE matrix
  float *e_cat, *w_cat;           // batched edge terms: [E, (L-1)*H] and the packed [(L-1)*H + (L-1), H] weights ++ biases
  MlpWs xemb; float *cat, *Yl; BnWs bl; float *pred, *dpred;
  // backward scratch
  float *dcat, *dAl, *dT1, *dT2, *dagg, *dZemb, *dAz, *deps_part;
  float* d_e[ESC_MAX_LAYERS];      // one per GINE layer: the edge stream consumes d_e[l] while the node chain moves on
  float *bn_scratch, *bag_scratch, *slabs;
  int64_t slab_limit; int n_wgrads;   // floats of the slab region (slab_floats) and the weight gradients that share it (reduce_jobs)
  float *col_stats;               // GEMM-epilogue BatchNorm partials: float2[ceil(rows/32)][H]
  float *bst_part;                // BatchNorm-backward column sums left by a dX epilogue / an aggregate backward: float2[slots][H]
  float *bn_scratch_e, *col_stats_e;   // the edge stream's own BatchNorm scratch / GEMM-epilogue partials
  // ZINC variant: node features from a table, [z_emb | edge type] edge-term input, pooled readout
  float *cat_scale, *cat_shift;     // (scale, shift) of the BatchNorm that produced each H-wide slice of cat: [(L+1)*H]
  float *X0, *dX0, *Zcat, *dZcat, *pooled, *dpool, *Al;
  int64_t G, D, Wz;                 // graphs, type-embedding width, Wz = H + D
  int64_t total;
};

// slots of bst_part a layout reserves (counting: float2[slots][H]; OGB: float2[slots][2H]) — what the slot counts of the schedules
// below are held against (tests/test_engine_schedule_cpu.py)
inline int64_t bst_slots(int64_t N) { return N / 4 + 2; }
inline int64_t bst_slots_ogb(int64_t N) { return N / 64 + 2; }
inline BnWs take_bn(Arena& a, int64_t C) { BnWs w; w.mean = a.take(C); w.invstd = a.take(C); w.scale = a.take(C); w.shift = a.take(C); w.nglob = a.take(16); w.coef = a.take(2 * C); return w; }

inline Layout plan_layout(const esc_nested_gin_t* m, int64_t N, int64_t E, int64_t Z, float* base, bool train) {
  Layout y{};
  Arena a{base, 0};
  const int64_t H = m->hidden, L = m->num_layers, C0 = m->in_dim;
  y.N = N; y.E = E; y.Z = Z; y.H = H; y.L = L; y.C0 = C0; y.W = (L + 1) * H;
  y.Zb = a.take(E * H); y.Yz = a.take(E * H); y.zb0 = take_bn(a, H); y.zb1 = take_bn(a, H);
  y.A0 = a.take(E * H); y.Zemb = a.take(E * H);
  // the H-wide edge terms e_1 .. e_{L-1} = lin_l(z_emb) of ALL layers as ONE GEMM [E, H] x [H, (L-1)*H]
  // over packed weights (one launch of 119 x 6 tiles instead of three of 119 x 2), their outputs column blocks of one matrix; see
  // DESIGN.md for what it measured.
  const bool batched = L >= 3;                              // (two or more H-wide edge terms)
  if (batched) { y.e_cat = a.take(E * (L - 1) * H); y.w_cat = a.take(((L - 1) * H + (L - 1)) * H); }
  for (int l = 0; l < L; ++l) {
    const int64_t C = l == 0 ? C0 : H;
    if (batched && l >= 1) { y.e[l] = base ? y.e_cat + (int64_t)(l - 1) * H : nullptr; y.ld_e[l] = (L - 1) * H; }
    else { y.e[l] = a.take(E * C); y.ld_e[l] = C; }
    y.agg[l] = a.take(N * C);
    y.conv[l].Y0 = a.take(N * H); y.conv[l].Y1 = a.take(N * H);
    y.conv[l].b0 = take_bn(a, H); y.conv[l].b1 = take_bn(a, H);
  }
  y.xemb.Y0 = a.take(N * H); y.xemb.Y1 = a.take(N * H); y.xemb.b0 = take_bn(a, H); y.xemb.b1 = take_bn(a, H);
  y.cat = a.take(N * y.W); y.Yl = a.take(N * H); y.bl = take_bn(a, H);
  y.cat_scale = a.take(y.W); y.cat_shift = a.take(y.W);       // the slices' BatchNorm coefficients side by side (readout prologue)
  if (base) {
    y.xemb.b1.scale = y.cat_scale; y.xemb.b1.shift = y.cat_shift;
    for (int l = 0; l < L; ++l) { y.conv[l].b1.scale = y.cat_scale + (int64_t)(l + 1) * H; y.conv[l].b1.shift = y.cat_shift + (int64_t)(l + 1) * H; }
  }
  y.pred = a.take(N); y.dpred = a.take(N);
  y.bn_scratch = a.take(norm::scratch_floats(H));
  y.col_stats = a.take(2 * ((E > N ? E : N) / 32 + 1) * H);
  y.bn_scratch_e = a.take(norm::scratch_floats(H));
  y.col_stats_e = a.take(2 * (E / 32 + 1) * H);
  if (train) {
    y.bst_part = a.take(2 * bst_slots(N) * H);
    y.dcat = a.take(N * y.W); y.dAl = a.take(N * H); y.dT1 = a.take(N * H); y.dT2 = a.take(N * H);
    y.dagg = a.take(N * H); y.dZemb = a.take(E * H); y.dAz = a.take(E * H);
    for (int l = 0; l < L; ++l) y.d_e[l] = a.take(E * (l == 0 ? C0 : H));
    y.deps_part = a.take(2 * N * (L > 0 ? L : 1));        // one vector per GINE layer, summed together at the end
    y.bag_scratch = a.take(sparse::scratch_floats(Z, H));
    // one private slab region per weight gradient, whether its ordered reduce is deferred to ONE launch at the end or runs at once
    const WGradList wg = weight_grads(m, N, E);
    y.slab_limit = slab_floats(wg); y.n_wgrads = reduce_jobs(wg);
    y.slabs = a.take(y.slab_limit);                        // (the last buffer: its size moves no other offset)
  }
  y.total = a.off;
  return y;
}

inline Layout plan_layout_zinc(const esc_zinc_gin_t* m, int64_t N, int64_t E, int64_t Z, int64_t G, float* base, bool train) {
  Layout y{};
  Arena a{base, 0};
  const int64_t H = m->hidden, L = m->num_layers, D = m->edge_emb.dim, C0 = m->node_emb.dim;
  y.N = N; y.E = E; y.Z = Z; y.H = H; y.L = L; y.C0 = C0; y.W = L * H; y.G = G; y.D = D; y.Wz = H + D;
  y.X0 = a.take(N * C0);
  y.Zb = a.take(E * H); y.Yz = a.take(E * H); y.zb0 = take_bn(a, H); y.zb1 = take_bn(a, H);
  y.A0 = a.take(E * H); y.Zcat = a.take(E * y.Wz);
  const int64_t lb = C0 == H ? 0 : 1, nb = L - lb;            // the H-wide edge terms: layers lb .. L-1, batched into one GEMM (see plan_layout())
  const bool batched = nb >= 2;
  if (batched) { y.e_cat = a.take(E * nb * H); y.w_cat = a.take(nb * H * y.Wz + nb * H); }
  for (int l = 0; l < L; ++l) {
    const int64_t C = l == 0 ? C0 : H;
    if (batched && l >= lb) { y.e[l] = base ? y.e_cat + (int64_t)(l - lb) * H : nullptr; y.ld_e[l] = nb * H; }
    else { y.e[l] = a.take(E * C); y.ld_e[l] = C; }
    y.agg[l] = a.take(N * C);
    y.conv[l].Y0 = a.take(N * H); y.conv[l].Y1 = a.take(N * H); y.conv[l].A1 = a.take(N * H);
    y.conv[l].b0 = take_bn(a, H); y.conv[l].b1 = take_bn(a, H);
  }
  // readout rows: the G pooled rows, or (node_readout) the N node rows of cat itself — no pooled / dpool then
  const bool nodes = m->node_readout != 0;
  const int64_t R = nodes ? N : G;
  y.cat = a.take(N * y.W); y.pooled = nodes ? nullptr : a.take(G * y.W); y.Yl = a.take(R * H); y.Al = a.take(R * H);
  y.bl = take_bn(a, H);
  y.pred = a.take(R); y.dpred = a.take(R);
  y.bn_scratch = a.take(norm::scratch_floats(H));
  y.col_stats = a.take(2 * ((E > N ? E : N) / 32 + 1) * H);
  y.bn_scratch_e = a.take(norm::scratch_floats(H));
  y.col_stats_e = a.take(2 * (E / 32 + 1) * H);
  if (train) {
    y.dcat = a.take(N * y.W); y.dpool = nodes ? nullptr : a.take(G * y.W); y.dAl = a.take(R * H);
    y.bst_part = a.take(2 * (N / 4 + E / 64 + 4) * H);
    y.dT1 = a.take(N * H); y.dT2 = a.take(N * H); y.dagg = a.take(N * H); y.dX0 = a.take(N * C0);
    y.dZcat = a.take(E * y.Wz); y.dZemb = a.take(E * H); y.dAz = a.take(E * H);
    for (int l = 0; l < L; ++l) y.d_e[l] = a.take(E * (l == 0 ? C0 : H));
    y.deps_part = a.take(2 * N * (L > 0 ? L : 1));
    y.bag_scratch = a.take(sparse::scratch_floats(Z, H));
    const WGradList wg = weight_grads_zinc(m, N, E, G);
    y.slab_limit = slab_floats(wg); y.n_wgrads = reduce_jobs(wg);
    y.slabs = a.take(y.slab_limit);
  }
  y.total = a.off;
  return y;
}

struct OgbLayer {
  float *hin, *e, *agg, *Y0, *hc, *hb;            // hin = h + vn[batch]; Y0 [N,2H]; hc pre-BN; hb after BN(+ReLU)
  BnWs b0, bn;
  unsigned char* mask_h;
  float *tmp, *V0, *VA, *V1, *VB, *vn;             // virtual-node update (rows G); vn = the embedding ENTERING layer l
  BnWs vb0, vb1;
  unsigned char* mask_v;
  float* d_e;
};
struct OgbLayout {
  int64_t N, E, Z, G, H, L, T;
  float *Tcat, *dTcat, *h0, *hL;
  float *Zb, *Zd, *A0, *Yz, *Yzd, *Zemb; BnWs zb0, zb1;
  unsigned char *mask_z0, *mask_z1;
  OgbLayer l[ESC_MAX_LAYERS];
  float *h[ESC_MAX_LAYERS + 1];
  float *pooled, *logits, *dlogits;
  // backward
  float *dpooled, *dHa, *dHb, *dT, *dA1, *dagg, *dZemb, *dYz, *dA0, *dvn_a, *dvn_b, *dG1, *dG2, *dtmp, *poolG;
  float *deps_part, *bag_scratch, *emb_scratch, *emb_scratch_n, *slabs, *bn_scratch, *col_stats, *bn_scratch_e, *col_stats_e;
  int64_t slab_limit; int n_wgrads;   // as in Layout
  float *bst_part;                 // column sums of a node MLP's first BatchNorm backward, left by its second Linear's dX epilogue
  int64_t total;
};

inline unsigned char* take_bytes(Arena& a, int64_t n) { return reinterpret_cast<unsigned char*>(a.take((n + 3) / 4)); }

inline OgbLayout plan_layout_ogb(const esc_ogb_gnn_t* m, int64_t N, int64_t E, int64_t Z, int64_t G, int64_t atom_entries,
                                 int64_t bond_entries, float* base, bool train) {
  OgbLayout y{};
  Arena a{base, 0};
  const int64_t H = m->hidden, L = m->num_layers, T = m->num_tasks, H2 = 2 * H;
  const bool drop = train && m->drop_ratio > 0.f;
  y.N = N; y.E = E; y.Z = Z; y.G = G; y.H = H; y.L = L; y.T = T;
  const int64_t rows_total = m->atom_rows + L * m->bond_rows;
  y.Tcat = a.take(rows_total * H);
  y.h0 = a.take(N * H); y.h[0] = y.h0;
  y.Zb = a.take(E * H); y.Zd = drop ? a.take(E * H) : y.Zb; y.A0 = a.take(E * H);
  y.Yz = a.take(E * H); y.Yzd = drop ? a.take(E * H) : y.Yz; y.Zemb = a.take(E * H);
  y.zb0 = take_bn(a, H); y.zb1 = take_bn(a, H);
  if (drop) { y.mask_z0 = take_bytes(a, E * H); y.mask_z1 = take_bytes(a, E * H); }
  for (int l = 0; l < L; ++l) {
    OgbLayer& q = y.l[l];
    q.vn = a.take(G * H);
    q.hin = a.take(N * H);
    q.e = a.take(E * H);
    q.agg = a.take(N * H);
    q.Y0 = a.take(N * H2); q.hc = a.take(N * H); q.hb = nullptr;         // (hb is never materialised: BN -> ReLU -> dropout in one pass)
    q.b0 = take_bn(a, H2); q.bn = take_bn(a, H);
    y.h[l + 1] = a.take(N * H);
    if (drop) q.mask_h = take_bytes(a, N * H);
    if (l < L - 1) {
      q.tmp = a.take(G * H); q.V0 = a.take(G * H2); q.VA = a.take(G * H2); q.V1 = a.take(G * H); q.VB = nullptr;
      q.vb0 = take_bn(a, H2); q.vb1 = take_bn(a, H);
      if (drop) q.mask_v = take_bytes(a, G * H);
    }
  }
  y.hL = y.h[L];
  y.pooled = a.take(G * H); y.logits = a.take(G * T); y.dlogits = a.take(G * T);
  y.bn_scratch = a.take(norm::scratch_floats(H2));
  y.col_stats = a.take(2 * ((E > N ? E : N) / 32 + 1) * H2);
  y.bn_scratch_e = a.take(norm::scratch_floats(H2));         // the edge pipeline's own BatchNorm scratch / GEMM-epilogue partials
  y.col_stats_e = a.take(2 * (E / 32 + 1) * H2);
  if (train) {
    y.dTcat = a.take(rows_total * H);
    y.bst_part = a.take(2 * bst_slots_ogb(N) * H2);
    y.dpooled = a.take(G * H); y.dHa = a.take(N * H); y.dHb = a.take(N * H); y.dT = a.take(N * H);
    y.dA1 = a.take(N * H2); y.dagg = a.take(N * H);
    y.dZemb = a.take(E * H); y.dYz = a.take(E * H); y.dA0 = a.take(E * H);
    y.dvn_a = a.take(G * H); y.dvn_b = a.take(G * H); y.dG1 = a.take(G * H2); y.dG2 = a.take(G * H); y.dtmp = a.take(G * H);
    y.poolG = a.take(G * H);
    for (int l = 0; l < L; ++l) y.l[l].d_e = a.take(E * H);
    y.deps_part = a.take(2 * N * (L > 0 ? L : 1));
    y.bag_scratch = a.take(sparse::scratch_floats(Z, H));
    const int64_t ent = atom_entries > bond_entries ? atom_entries : bond_entries;
    y.emb_scratch = a.take(sparse::scratch_floats(ent, H));
    y.emb_scratch_n = a.take(sparse::scratch_floats(ent, H));
    const WGradList wg = weight_grads_ogb(m, N, E, G);
    y.slab_limit = slab_floats(wg); y.n_wgrads = reduce_jobs(wg);
    y.slabs = a.take(y.slab_limit);
  }
  y.total = a.off;
  return y;
}

// ---- the schedule of one call ------------------------------------------------------------------------------------------------
// How a step is run — which Linear+BatchNorm pairs take their statistics from a GEMM epilogue, which edge terms are issued where,
// which backward GEMMs carry a BatchNorm backward, who leaves whose column sums in bst_part — decided ONCE per entry, before
// anything is launched, as a pure function of the model descriptor (sizes; addresses for their alignment), the layout and a
// RunMode.  The bodies of engine.hip switch on the result and decide nothing themselves; the fused entries still refuse a call
// whose plan is not ok, so a schedule that promised too much is an error, never a silent other path.  Every slab probe is the
// START of the slab region: the cursor only ever moves by round64 floats, so the alignment the plans look at is the same at every
// later position (tests/test_engine_schedule_cpu.py holds that, with the `slab_off` argument).
struct RunMode {
  bool train = false;
  bool two_stream = false;               // the batch has enough edges for the second stream, and the stream exists
  bool deferred = false;                 // the weight gradients' reduces wait for one launch (Ctx::jobs): the main chain of a training entry
  bool sync = false;                     // SyncBN: a training call with a collective over more than one rank
  bool l1_head = false;                  // the entry wants d L1 / d pred out of the prediction head's launch (train_step)
  bool plain_events = false;             // esc_engine_set_side_stream bit 6
  bool readout_one_launch = false;       // ... bit 7
  const void* x = nullptr;               // counting model: the batch's node features (x_embedding's operand; the address only)
  plan::PlanKnobs linear;                // the knob values the kernels' own plans see (linear_mfma.hip, aggregate.hip, bag.hip)
  sparse::SparseKnobs aggregate, bag;
};

// a Linear followed by a BatchNorm (linear_bn() in engine.hip)
enum BnMode {
  BN_EVAL_COEF = 0,          // eval: coefficients from the running statistics
  BN_STATS_PASS,             // training: a statistics pass over the Linear's output
  BN_EPILOGUE_PARTIALS,      // ... partials from the GEMM's epilogue, then a finalize launch
  BN_EPILOGUE_MERGED         // ... and merged by the GEMM's last workgroup: no finalize launch
};
// (statistics from the epilogue: main chain only — col_stats is shared scratch — and outputs wider than 32)
inline BnMode bn_pair_mode(const RunMode& r, int64_t M, int64_t width) {
  if (!r.train) return BN_EVAL_COEF;
  if (!(width > 32 && r.deferred)) return BN_STATS_PASS;
  return (M > 1 && !r.sync) ? BN_EPILOGUE_MERGED : BN_EPILOGUE_PARTIALS;
}

// Where the edge terms e_l are issued.  Batched (the layout's e_cat): the H-wide ones come out of ONE launch, only a narrow first
// term keeps its own.  Else per-layer launches: with two streams one layer ahead of the node chain — e_{l+1} is queued behind the
// aggregate of layer l and overlaps that layer's MLP, so that a bandwidth-bound aggregate never shares the HBM with an edge-sized
// GEMM (r01: 1.255 -> 1.225 ms against two layers ahead); on one stream all of them up front, in layer order.
struct EdgeTerms {
  bool batched = false;
  bool up_front[ESC_MAX_LAYERS] = {};    // term l: its own launch before the node pipeline starts (in layer order, ahead of the batched launch)
  int behind_agg[ESC_MAX_LAYERS];        // the term launched behind layer l's aggregate, or -1
};
// own0: batched, and term 0 is not part of the batch; skip0: term 0 has gone out already (the counting model's e0_early)
inline EdgeTerms plan_edge_terms(int64_t L, bool batched, bool own0, bool skip0, bool two_stream) {
  EdgeTerms t;
  t.batched = batched;
  for (int l = 0; l < ESC_MAX_LAYERS; ++l) t.behind_agg[l] = -1;
  if (batched) { t.up_front[0] = own0; return t; }
  const int64_t ahead = two_stream ? 1 : L;
  for (int64_t l = skip0 ? 1 : 0; l < L && l < ahead; ++l) t.up_front[l] = true;
  for (int64_t l = 0; two_stream && l + ahead < L; ++l) t.behind_agg[l] = (int)(l + ahead);
  return t;
}

// The readout Linear's edge-stream block (backward(), lin1's columns [0, L*H)) goes out as two launches, the dX tiles first, and
// the node chain waits for those only.  The dX launch asks for kReadoutDxLds: one workgroup per CU, and beside it the
// kNodeLdsFloorBwd of a node tile (engine.hip) still fits — two of its 54-KB workgroups on a CU shut the node chain's launches out
// of that CU and the chain waited for slots (DESIGN.md *Step engine, readout backward*).
constexpr int kReadoutDxLds = 84 * 1024;         // bytes: 2 x 84 > 160

// ---- BatchNorm(+ReLU) backward folded into the Linear backward behind it (r03; esc_linear_bwd_both_bn) ------------------
// The node chain's backward was, per Linear -> BatchNorm -> ReLU pair, partial -> finalize -> apply -> dX+dW: four dependent
// launches.  The apply now happens while the GEMM stages its dY operand and the column sums of an MLP's FIRST BatchNorm come
// out of the dX epilogue of its second Linear: partial/finalize -> dX+dW -> finalize -> dX+dW.  The three fusions in force
// (the former ESC_BN_FUSE_BWD = 11, bits 0, 1, 3; the forms they replace stay for the shapes and modes they do not serve):
constexpr bool kBnBwdApplyInGemm = true;    // a BatchNorm backward's apply rides on the dY staging of the Linear backward behind it
constexpr bool kBnBwdSumsFromDx = true;     // its column sums come out of the dX epilogue of the Linear backward in front of it
constexpr bool kBnBwdSumsFromAgg = true;    // ... or out of the aggregate backward that completes its output gradient
inline esc_bn_bwd_fused bn_fused(const float* x, int64_t ld_x, const BnWs& w, int relu, const float* beta) {
  return esc_bn_bwd_fused{x, ld_x, w.mean, w.invstd, w.scale, w.shift, w.coef, relu, beta};
}

// One MLP's backward: its operands (stated once: the schedule plans with them, mlp_backward() launches with them) and its form.
// pre_out: `out` holds the PRE-BatchNorm rows of lin1 (the node-activation fusion), else the materialised output.
struct MlpOps {
  const esc_mlp_t* p; const MlpWs* w;
  const float* A; int64_t ld_a, M;
  const float* out; int64_t ld_out;
  const float* dOut; int64_t ld_dout;
  float* dA; int64_t ld_da;
  bool pre_out;
};
// Which of the two Linear backwards take the fused form (kBnBwdApplyInGemm): lin0 only together with lin1
struct MlpFuse { bool lin1 = false, lin0 = false; };
// ... and where the column sums of BatchNorm 1's backward come from: a pass of its own, or `slots` slots of bst_part left by the
// producer of dOut — the readout's dX epilogue (kBnBwdSumsFromDx) or the next layer's aggregate backward (kBnBwdSumsFromAgg)
enum SumsFrom { SUMS_OWN_PASS = 0, SUMS_READOUT, SUMS_AGGREGATE };
struct MlpBwd { MlpFuse fuse; SumsFrom sums = SUMS_OWN_PASS; int64_t slots = 0; };
enum AggBwd { AGG_PLAIN = 0, AGG_AFFINE, AGG_AFFINE_STATS };
// the widths esc_gine_aggregate_bwd_affine_stats serves: one wave per row (no split), its [4 waves][C] float2 of LDS
inline bool agg_stats_served(const sparse::SparseKnobs& k, int64_t C) { return sparse::deps_slots(k, C) == 1 && C <= 2048; }

inline esc_bn_bwd_next mlp_next(const Layout& y, const MlpOps& o, int act) {
  const MlpWs& w = *o.w;
  return esc_bn_bwd_next{y.bst_part, w.Y0, y.H, w.b0.mean, w.b0.invstd, w.b0.scale, w.b0.shift, act, o.p->bn0.beta};
}
inline esc_bn_bwd_fused mlp_fused1(const Layout& y, const MlpOps& o, int act) {      // what BatchNorm 1 normalised
  return bn_fused(o.pre_out ? o.out : o.w->Y1, o.pre_out ? o.ld_out : y.H, o.w->b1, act, o.p->bn1.beta);
}
inline esc_bn_bwd_fused mlp_fused0(const Layout& y, const MlpOps& o, int act) { return bn_fused(o.w->Y0, y.H, o.w->b0, act, o.p->bn0.beta); }
// ReLU MLPs whose hidden activation was never materialised (counting model; ELU models keep the elementwise launches: DESIGN.md
// *Retired step-engine switches*), statistics of this rank only, shapes the fused kernels serve
inline MlpFuse plan_mlp_fuse(const RunMode& r, const Layout& y, int act, const MlpOps& o, const float* slabs) {
  const int64_t H = y.H;
  const esc_mlp_t& p = *o.p;
  MlpFuse f;
  if (!(kBnBwdApplyInGemm && r.train && !r.sync && y.bst_part != nullptr && p.lin1.in_dim == H && p.lin1.out_dim == H)) return f;
  if (!(act == 1 && o.w->A1 == nullptr)) return f;
  const esc_bn_bwd_fused f1 = mlp_fused1(y, o, act), f0 = mlp_fused0(y, o, act);
  const esc_bn_bwd_next n0 = mlp_next(y, o, act);
  using plan::Op;
  f.lin1 = plan::plan_both_bn(r.linear, Op{o.dOut, o.ld_dout}, &f1, Op{o.w->Y0, H}, Op{p.lin1.w, H}, Op{y.dT2, H}, slabs, &n0, o.M, H, H).ok;
  f.lin0 = f.lin1 && plan::plan_both_bn(r.linear, Op{y.dT2, H}, &f0, Op{o.A, o.ld_a}, Op{p.lin0.w, p.lin0.in_dim}, Op{o.dA, o.ld_da}, slabs,
                                        static_cast<const esc_bn_bwd_next*>(nullptr), o.M, H, p.lin0.in_dim).ok;
  return f;
}

// counting model: the MLP of GINE layer l / of x_embedding
inline MlpOps conv_mlp_ops(const esc_nested_gin_t* m, const Layout& y, int l, bool pre_out) {
  const int64_t C = l == 0 ? y.C0 : y.H;
  return MlpOps{&m->conv[l].nn, &y.conv[l], y.agg[l], C, y.N, y.cat + (int64_t)(l + 1) * y.H, y.W, y.dcat + (int64_t)(l + 1) * y.H, y.W, y.dagg, C, pre_out};
}
inline MlpOps xemb_mlp_ops(const esc_nested_gin_t* m, const Layout& y, const float* x, bool pre_out) {      // (input x needs no gradient)
  return MlpOps{&m->xemb, &y.xemb, x, y.C0, y.N, y.cat, y.W, y.dcat, y.W, nullptr, 0, pre_out};
}
// ... and the readout Linear's backward over columns [col0, col0 + ncols) of cat, bn_lin1's backward folded in
inline esc_bn_bwd_fused readout_fused(const esc_nested_gin_t* m, const Layout& y) { return bn_fused(y.Yl, y.H, y.bl, 1, m->bn_lin1.beta); }
// the last layer's output gradient d(cat)[:, L*H:] is final once lin1's node-side block has written it: its dX tiles can leave the
// column sums of that layer's last BatchNorm backward
inline esc_bn_bwd_next readout_next(const Layout& y) {
  const MlpWs& wl = y.conv[y.L > 0 ? y.L - 1 : 0];
  return esc_bn_bwd_next{y.bst_part, y.cat + y.L * y.H, y.W, wl.b1.mean, wl.b1.invstd, wl.b1.scale, wl.b1.shift, 1, nullptr};     // (ReLU: beta is not read)
}
inline plan::Plan plan_readout_block(const plan::PlanKnobs& k, const esc_nested_gin_t* m, const Layout& y, int64_t col0, int64_t ncols,
                                     const esc_bn_bwd_next* next, const float* slabs) {
  const esc_bn_bwd_fused fl = readout_fused(m, y);
  using plan::Op;
  return plan::plan_both_bn(k, Op{y.dAl, y.H}, &fl, Op{y.cat + col0, y.W}, Op{m->lin1.w + col0, y.W}, Op{y.dcat + col0, y.W}, slabs, next, y.N,
                            y.H, ncols);
}

// counting model and ZINC (which takes none of the backward fusions: ELU, materialised activations)
struct Schedule {
  // forward
  BnMode zlin = BN_EVAL_COEF, xemb[2] = {}, conv[ESC_MAX_LAYERS][2] = {}, readout = BN_EVAL_COEF;
  int64_t bag_block = 0;            // > 0: the ESC bag's epilogue leaves the partials of z_embedding's first BatchNorm, this many rows each
  bool e0_early = false;            // the narrow first edge term runs BEFORE z_emb is materialised (its own prologue)
  EdgeTerms terms;
  bool node_act = false;            // the last BatchNorm+ReLU of every node MLP is applied by its consumers (see forward())
  bool l1_head = false;             // the prediction head's launch leaves the L1 gradient too
  // backward (training calls)
  bool split_lin1 = false;          // the readout Linear as two column blocks: [0, L*H) on the edge stream, [L*H, W) on the node chain
  bool fuse_lin1 = false;           // ... with bn_lin1's backward folded in (every block)
  bool ask_dx_split = false;        // the edge-stream block is asked to go out as two launches (dX tiles first) ...
  bool dx_split = false;            // ... and its plan grants it
  MlpBwd xemb_bwd, mlp[ESC_MAX_LAYERS];
  AggBwd agg[ESC_MAX_LAYERS] = {};
  bool last_dw_on_node = false;     // layer 0's conv.lin: only its input gradient stays on the edge stream
};

inline Schedule plan_schedule(const esc_nested_gin_t* m, const Layout& y, const RunMode& r, int64_t slab_off = 0) {
  Schedule s;
  const int64_t N = y.N, E = y.E, H = y.H, L = y.L, W = y.W;
  s.zlin = bn_pair_mode(r, E, m->zlin.out_dim);
  s.xemb[0] = bn_pair_mode(r, N, m->xemb.lin0.out_dim);
  s.xemb[1] = bn_pair_mode(r, N, m->xemb.lin1.out_dim);
  for (int l = 0; l < L; ++l) {
    s.conv[l][0] = bn_pair_mode(r, N, m->conv[l].nn.lin0.out_dim);
    s.conv[l][1] = bn_pair_mode(r, N, m->conv[l].nn.lin1.out_dim);
  }
  s.readout = bn_pair_mode(r, N, m->lin1.out_dim);
  s.bag_block = (r.train && !r.sync) ? sparse::bag_stats_block_rows(r.bag, m->z_table, m->z_rows, H, plan::Op{y.Zb, H}, E) : 0;
  s.e0_early = y.C0 <= 32 && L >= 1;
  s.terms = plan_edge_terms(L, y.e_cat != nullptr, !s.e0_early, s.e0_early, r.two_stream);
  s.node_act = H >= 64 && H % 4 == 0 && y.cat_scale != nullptr;
  plan::Flags head;                // the head reads pre-BatchNorm rows: (scale, shift) of bn_lin1 in its prologue
  head.pro = true;
  head.pro_aligned = plan::aligned16(y.bl.scale) && plan::aligned16(y.bl.shift);
  s.l1_head = r.l1_head && r.two_stream && H <= 1024 && y.bl.scale != nullptr && y.bl.shift != nullptr &&
              plan::plan_fwd(r.linear, plan::Op{y.Yl, H}, plan::Op{m->lin2.w, H}, 1, 1, H, head).family == plan::F_NARROW;
  if (!r.train) return s;
  const float* slabs = y.slabs ? y.slabs + slab_off : nullptr;
  const esc_bn_bwd_next* none = nullptr;
  s.split_lin1 = r.two_stream && r.deferred && L >= 1;
  const int64_t K0 = L * H;                                   // columns [0, K0) go to the edge stream
  auto lin1_ok = [&](int64_t col0, int64_t ncols, const esc_bn_bwd_next* nx) { return plan_readout_block(r.linear, m, y, col0, ncols, nx, slabs).ok; };
  s.fuse_lin1 = kBnBwdApplyInGemm && !r.sync && y.bst_part != nullptr &&
                (s.split_lin1 ? (lin1_ok(0, K0, none) && lin1_ok(K0, H, none)) : lin1_ok(0, W, none));
  for (int l = 0; l < L; ++l) s.mlp[l].fuse = plan_mlp_fuse(r, y, 1, conv_mlp_ops(m, y, l, s.node_act), slabs);
  s.xemb_bwd.fuse = plan_mlp_fuse(r, y, 1, xemb_mlp_ops(m, y, static_cast<const float*>(r.x), s.node_act), slabs);
  if (s.split_lin1) {
    s.ask_dx_split = s.fuse_lin1 && !r.readout_one_launch && !r.plain_events;
    plan::PlanKnobs k2 = r.linear;
    k2.dual_split = kReadoutDxLds;
    s.dx_split = s.ask_dx_split && plan_readout_block(k2, m, y, 0, K0, none, slabs).launches == 2;
    // (the last layer's MLP backward follows at once: it must take the fused form, or nobody reads the sums)
    const esc_bn_bwd_next nl = readout_next(y);
    if (s.fuse_lin1 && s.node_act && kBnBwdSumsFromDx && lin1_ok(K0, H, &nl) && s.mlp[L - 1].fuse.lin1) {
      s.mlp[L - 1].sums = SUMS_READOUT;
      s.mlp[L - 1].slots = plan::cdiv(N, plan::bwd_bn_block_rows(N, H, H));
    }
  }
  // d(cat)[:, l*H:(l+1)*H] is final once layer l's aggregate backward has added its share: it can leave the column sums of the
  // PREVIOUS layer's last BatchNorm backward, and that layer's MLP backward starts with the finalize
  for (int l = 0; l < L; ++l) {
    const int64_t C = l == 0 ? y.C0 : H;
    if (!(s.node_act && l > 0)) { s.agg[l] = AGG_PLAIN; continue; }
    s.agg[l] = AGG_AFFINE;
    if (kBnBwdSumsFromAgg && agg_stats_served(r.aggregate, C) && s.mlp[l - 1].fuse.lin1) {
      s.agg[l] = AGG_AFFINE_STATS;
      s.mlp[l - 1].sums = SUMS_AGGREGATE;
      s.mlp[l - 1].slots = sparse::stats_slots(N);
    }
  }
  s.last_dw_on_node = r.two_stream && r.deferred;
  return s;
}

// ZINC: the H-wide edge terms are layers lb .. L-1 (see plan_layout_zinc()); R readout rows
inline Schedule plan_schedule_zinc(const esc_zinc_gin_t* m, const Layout& y, const RunMode& r) {
  Schedule s;
  const int64_t R = m->node_readout ? y.N : y.G;
  s.zlin = bn_pair_mode(r, y.E, m->zlin.out_dim);
  for (int l = 0; l < y.L; ++l) {
    s.conv[l][0] = bn_pair_mode(r, y.N, m->conv[l].nn.lin0.out_dim);
    s.conv[l][1] = bn_pair_mode(r, y.N, m->conv[l].nn.lin1.out_dim);
  }
  s.readout = bn_pair_mode(r, R, m->lin1.out_dim);
  s.terms = plan_edge_terms(y.L, y.e_cat != nullptr, y.C0 != y.H, false, r.two_stream);
  return s;
}

// OGB-mol
struct OgbSchedule {
  BnMode zlin = BN_EVAL_COEF;                           // (without dropout: with it z_embedding's Linear is followed by the dropout, then a statistics pass)
  BnMode lin0[ESC_MAX_LAYERS] = {}, lin1[ESC_MAX_LAYERS] = {}, vlin0[ESC_MAX_LAYERS] = {}, vlin1[ESC_MAX_LAYERS] = {};
  EdgeTerms terms;
  // backward.  The hidden BatchNorm's backward loses its partial-sum pass (2H-wide rows: the most expensive of its three launches):
  // the column sums come out of lin1's dX epilogue (esc_linear_bwd_both_bn with bn == NULL), then finalize + apply
  bool hidden_from_dx[ESC_MAX_LAYERS] = {};
  int64_t hidden_slots = 0;                             // slots of bst_part that epilogue writes
  // the bond tables' gradient of the LAST layer processed (l == 0), whose edge-term backward opens the tail of the step, runs on the
  // node stream and the edge stream goes straight to the Linear that completes d(z_emb): 4.34 -> 4.31 ms/step
  bool bonds_on_node = false;
  // BatchNorm backward next to a dropout as ONE fused sequence (esc_bn_bwd_dropout): batch_norms[l], the virtual node's last
  // BatchNorm (l < L-1), z_embedding's two
  bool drop_h[ESC_MAX_LAYERS] = {}, drop_v[ESC_MAX_LAYERS] = {}, drop_z1 = false, drop_z0 = false;
};
inline esc_bn_bwd_next ogb_hidden_next(const OgbLayout& y, int l) {
  const OgbLayer& w = y.l[l];
  return esc_bn_bwd_next{y.bst_part, w.Y0, 2 * y.H, w.b0.mean, w.b0.invstd, w.b0.scale, w.b0.shift, 1, nullptr};
}
// one site: every operand float4-accessible (ReLU / no activation only, statistics of this rank only)
inline bool plan_bn_drop_fused(const RunMode& r, float p, int act, int64_t C, const void* X, const void* dY, const void* dX, const BnWs& w,
                               const esc_bn_t& bn, const void* mask, const void* scratch) {
  using plan::Op;
  return p > 0.f && !r.sync && act <= 1 && norm::mats_vec(C, {Op{X, C}, Op{dY, C}, Op{dX, C}}) &&
         norm::vecs_aligned({w.mean, w.invstd, bn.gamma, bn.beta, scratch}) && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
}
inline OgbSchedule plan_schedule_ogb(const esc_ogb_gnn_t* m, const OgbLayout& y, const RunMode& r, int64_t slab_off = 0) {
  OgbSchedule s;
  const int64_t N = y.N, E = y.E, G = y.G, H = y.H, L = y.L, H2 = 2 * H;
  const float p = r.train ? m->drop_ratio : 0.f;
  s.zlin = p > 0.f ? bn_pair_mode(r, E, 0) : bn_pair_mode(r, E, m->zlin.out_dim);
  for (int l = 0; l < L; ++l) {
    const esc_ogb_layer_t& q = m->layer[l];
    s.lin0[l] = bn_pair_mode(r, N, q.lin0.out_dim);
    s.lin1[l] = bn_pair_mode(r, N, q.lin1.out_dim);
    if (l < L - 1) { s.vlin0[l] = bn_pair_mode(r, G, q.vlin0.out_dim); s.vlin1[l] = bn_pair_mode(r, G, q.vlin1.out_dim); }
  }
  s.terms = plan_edge_terms(L, false, false, false, r.two_stream);
  if (!r.train) return s;
  const float* slabs = y.slabs ? y.slabs + slab_off : nullptr;
  s.hidden_slots = plan::cdiv(N, plan::bwd_bn_block_rows(N, H, H2));
  s.bonds_on_node = r.two_stream;
  const float* scratch_e = r.two_stream ? y.bn_scratch_e : y.bn_scratch;      // (the edge pipeline's own, when it has a stream)
  bool dH_is_a = true;                       // d h_{l+1} lives in dHa or dHb, d vn_{l+1} in dvn_a or dvn_b: as backward_ogb() swaps them
  for (int l = (int)L - 1; l >= 0; --l) {
    const esc_ogb_layer_t& q = m->layer[l];
    const OgbLayer& w = y.l[l];
    const bool last = l == (int)L - 1;
    s.drop_h[l] = plan_bn_drop_fused(r, p, last ? 0 : 1, H, w.hc, dH_is_a ? y.dHa : y.dHb, y.dT, w.bn, q.bn, w.mask_h, y.bn_scratch);
    if (kBnBwdSumsFromDx && !r.sync && y.bst_part != nullptr) {
      const esc_bn_bwd_next n0 = ogb_hidden_next(y, l);
      using plan::Op;
      s.hidden_from_dx[l] = plan::plan_both_bn(r.linear, Op{y.dT, H}, static_cast<const esc_bn_bwd_fused*>(nullptr), Op{w.Y0, H2}, Op{q.lin1.w, H2},
                                               Op{y.dA1, H2}, slabs, &n0, N, H, H2).ok;
    }
    if (!last) s.drop_v[l] = plan_bn_drop_fused(r, p, 1, H, w.V1, ((int)L - 2 - l) % 2 == 0 ? y.dvn_a : y.dvn_b, y.dG2, w.vb1, q.vbn1, w.mask_v, y.bn_scratch);
    if (last && m->residual) dH_is_a = !dH_is_a;
    dH_is_a = !dH_is_a;
  }
  s.drop_z1 = plan_bn_drop_fused(r, p, 1, H, y.Yzd, y.dZemb, y.dYz, y.zb1, m->zbn1, y.mask_z1, scratch_e);
  s.drop_z0 = plan_bn_drop_fused(r, p, 1, H, y.Zd, y.dA0, y.dA0, y.zb0, m->zbn0, y.mask_z0, scratch_e);
  return s;
}

}  // namespace esc
