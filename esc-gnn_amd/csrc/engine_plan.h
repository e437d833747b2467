// engine_plan.h — what the three step engines (engine.hip: counting, ZINC, OGB-mol) decide on the host before anything is launched:
// the workspace layout of a call, the weight gradients a training step produces, and how much split-M slab scratch and how many
// deferred reduce jobs they take.  Host-only, no HIP header: tests/engine_plan_host.cpp compiles it with a plain host compiler
// under sanitizers.  The weight_grads* functions are the ONLY place that enumerates a family's weight gradients: the slab region
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
    y.bst_part = a.take(2 * (N / 4 + 2) * H);
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
    y.bst_part = a.take(2 * (N / 64 + 2) * H2);
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

}  // namespace esc
