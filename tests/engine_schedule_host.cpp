// The step engines' schedule (esc-gnn_amd/csrc/engine_plan.h: plan_schedule, plan_schedule_zinc, plan_schedule_ogb) as a stand-alone
// host program: tests/test_engine_schedule_cpu.py feeds it model sizes, batch sizes and run modes and holds what it prints to the
// transcription in tests/engine_schedule_cases.py.  No HIP, no library: the descriptors carry sizes and ADDRESSES that are never
// read (the plans look at their alignment only) — the workspace at 1 << 32, the parameters from 1 << 36 in 256-byte steps.
//
// stdin, one request per line:
//   family L H a b c drop  N E Z G atom_entries bond_entries  train two_stream deferred sync l1_head plain_events readout_one_launch
//          slab_off misalign agg_split_bwd
//     family L H a b c drop, N .. bond_entries      as tests/engine_plan_host.cpp
//     slab_off     floats (a multiple of 64) the slab probe lies behind the start of the slab region
//     misalign     parameters moved off their 16-byte alignment by 4 bytes: bit 0 the readout's weights (lin1, lin2; OGB: none),
//                  bit 1 the node MLPs' weights (OGB: every mlp.lin1), bit 2 the BatchNorms' gamma / beta; and bit 3: the ESC bag's
//                  SparseKnobs::bag_tiled on (the table has 100 rows)
//     agg_split_bwd  the aggregate's SparseKnobs::agg_split_bwd (1: default)
//   aggstats C agg_split_bwd                        -> agg_stats_served, one number
// stdout, one line per request: key=value tokens, lists comma-separated (see emit()); the last three are checked HERE:
//     cap      slots the layout reserves in bst_part
//     agree    1: every Linear the schedule marks fused has plan_both_bn(...).ok with the operands the body passes, taken again with
//              the slab probe at the END of the region's first granule
//     entry    1: wherever the aggregate's stats form is chosen, esc_gine_aggregate_bwd_affine_stats's own requirements hold
#include <cstdio>
#include <cstring>
#include <string>

#include "engine_plan.h"

using namespace esc;

struct Params {                                     // fake parameter addresses
  uintptr_t next = static_cast<uintptr_t>(1) << 36;
  long misalign = 0;
  const float* take(int group) {
    const uintptr_t p = next + ((misalign >> group) & 1 ? 4 : 0);
    next += 256;
    return reinterpret_cast<const float*>(p);
  }
};
enum { READOUT = 0, MLP = 1, BN = 2, OTHER = 30 };

static esc_linear_t linear(Params& P, int group, int64_t in, int64_t out) {
  esc_linear_t l{};
  l.w = P.take(group); l.b = P.take(OTHER); l.in_dim = in; l.out_dim = out;
  return l;
}
static esc_bn_t bn(Params& P) {
  esc_bn_t b{};
  b.gamma = P.take(BN); b.beta = P.take(BN);
  return b;
}
static esc_mlp_t mlp(Params& P, int64_t in, int64_t H) {
  esc_mlp_t m{};
  m.lin0 = linear(P, MLP, in, H); m.bn0 = bn(P); m.lin1 = linear(P, MLP, H, H); m.bn1 = bn(P);
  return m;
}

template <class T>
static std::string join(const T* v, int n) {
  std::string s;
  for (int i = 0; i < n; ++i) s += (i ? "," : "") + std::to_string((long long)v[i]);
  return n ? s : "-";
}
static void emit_terms(const EdgeTerms& t, int L) {
  int up[ESC_MAX_LAYERS];
  for (int l = 0; l < L; ++l) up[l] = t.up_front[l];
  printf(" batched=%d up=%s behind=%s", (int)t.batched, join(up, L).c_str(), join(t.behind_agg, L).c_str());
}
static std::string mlp_str(const MlpBwd& b) {
  return std::to_string((int)b.fuse.lin1) + "," + std::to_string((int)b.fuse.lin0) + "," + std::to_string((int)b.sums) + "," + std::to_string((long long)b.slots);
}

int main() {
  char family[16];
  float* const base = reinterpret_cast<float*>(static_cast<uintptr_t>(1) << 32);
  for (;;) {
    if (scanf("%15s", family) != 1) break;
    if (!strcmp(family, "aggstats")) {
      long C, k;
      if (scanf("%ld %ld", &C, &k) != 2) return 2;
      sparse::SparseKnobs sk;
      sk.agg_split_bwd = (int)k;
      printf("%d\n", (int)agg_stats_served(sk, C));
      continue;
    }
    long L, H, a, b, c, drop, N, E, Z, G, ae, be, train, two, deferred, sync, l1, plain, one, slab_off, misalign, asb;
    if (scanf("%ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", &L, &H, &a, &b, &c, &drop, &N, &E, &Z, &G,
              &ae, &be, &train, &two, &deferred, &sync, &l1, &plain, &one, &slab_off, &misalign, &asb) != 22 ||
        L < 1 || L > ESC_MAX_LAYERS || slab_off % 64 != 0) {
      fprintf(stderr, "malformed request\n");
      return 2;
    }
    Params P;
    P.misalign = misalign;
    RunMode r;
    r.train = train; r.two_stream = two; r.deferred = deferred; r.sync = sync; r.l1_head = l1; r.plain_events = plain; r.readout_one_launch = one;
    r.x = P.take(OTHER);
    r.aggregate.agg_split_bwd = (int)asb;
    r.bag.bag_tiled = (int)(misalign >> 3 & 1);
    int agree = 1, entry = 1;
    if (!strcmp(family, "count") || !strcmp(family, "zinc")) {
      const bool count = family[0] == 'c';
      Layout y;
      Schedule s;
      esc_nested_gin_t m{};
      esc_zinc_gin_t mz{};
      if (count) {
        m.num_layers = L; m.hidden = H; m.in_dim = a; m.z_rows = 100; m.z_table = P.take(OTHER);
        m.zbn0 = bn(P); m.zlin = linear(P, OTHER, H, H); m.zbn1 = bn(P);
        m.xemb = mlp(P, a, H);
        for (int l = 0; l < L; ++l) { m.conv[l].nn = mlp(P, l == 0 ? a : H, H); m.conv[l].lin = linear(P, OTHER, H, l == 0 ? a : H); }
        m.lin1 = linear(P, READOUT, (L + 1) * H, H); m.bn_lin1 = bn(P); m.lin2 = linear(P, READOUT, H, 1);
        y = plan_layout(&m, N, E, Z, base, train != 0);
        s = plan_schedule(&m, y, r, slab_off);
      } else {
        mz.num_layers = L; mz.hidden = H; mz.z_rows = 100; mz.z_table = P.take(OTHER); mz.node_emb.dim = a; mz.edge_emb.dim = b; mz.node_readout = (int32_t)c;
        mz.zbn0 = bn(P); mz.zlin = linear(P, OTHER, H, H); mz.zbn1 = bn(P);
        for (int l = 0; l < L; ++l) { mz.conv[l].nn = mlp(P, l == 0 ? a : H, H); mz.conv[l].lin = linear(P, OTHER, H + b, l == 0 ? a : H); }
        mz.lin1 = linear(P, READOUT, L * H, H); mz.bn_lin1 = bn(P); mz.lin2 = linear(P, READOUT, H, 1);
        y = plan_layout_zinc(&mz, N, E, Z, G, base, train != 0);
        s = plan_schedule_zinc(&mz, y, r);
      }
      int c0[ESC_MAX_LAYERS], c1[ESC_MAX_LAYERS], agg[ESC_MAX_LAYERS];
      for (int l = 0; l < L; ++l) { c0[l] = s.conv[l][0]; c1[l] = s.conv[l][1]; agg[l] = s.agg[l]; }
      printf("zlin=%d xemb=%d,%d conv0=%s conv1=%s readout=%d bag=%lld e0=%d", (int)s.zlin, (int)s.xemb[0], (int)s.xemb[1], join(c0, (int)L).c_str(),
             join(c1, (int)L).c_str(), (int)s.readout, (long long)s.bag_block, (int)s.e0_early);
      emit_terms(s.terms, (int)L);
      printf(" node_act=%d l1=%d split=%d fuse_lin1=%d ask=%d dx_split=%d last_dw=%d agg=%s xemb_bwd=%s", (int)s.node_act, (int)s.l1_head, (int)s.split_lin1,
             (int)s.fuse_lin1, (int)s.ask_dx_split, (int)s.dx_split, (int)s.last_dw_on_node, join(agg, (int)L).c_str(), mlp_str(s.xemb_bwd).c_str());
      for (int l = 0; l < L; ++l) printf(" mlp%d=%s", l, mlp_str(s.mlp[l]).c_str());
      if (count && train) {               // the plans again, as the bodies' calls would take them, with the probe elsewhere in the region
        const float* slabs = y.slabs + 64 * 7;
        const esc_bn_bwd_next* none = nullptr;
        using plan::Op;
        auto mlp_agrees = [&](const MlpOps& o, const MlpBwd& how) {
          if (!how.fuse.lin1) return !how.fuse.lin0 && how.sums == SUMS_OWN_PASS;
          const esc_bn_bwd_fused f1 = mlp_fused1(y, o, 1), f0 = mlp_fused0(y, o, 1);
          const esc_bn_bwd_next n0 = mlp_next(y, o, 1);
          bool ok = plan::plan_both_bn(r.linear, Op{o.dOut, o.ld_dout}, &f1, Op{o.w->Y0, y.H}, Op{o.p->lin1.w, y.H}, Op{y.dT2, y.H}, slabs, &n0, o.M, y.H, y.H).ok;
          if (how.fuse.lin0)
            ok = ok && plan::plan_both_bn(r.linear, Op{y.dT2, y.H}, &f0, Op{o.A, o.ld_a}, Op{o.p->lin0.w, o.p->lin0.in_dim}, Op{o.dA, o.ld_da}, slabs, none, o.M,
                                          y.H, o.p->lin0.in_dim).ok;
          return ok;
        };
        for (int l = 0; l < L; ++l) agree = agree && mlp_agrees(conv_mlp_ops(&m, y, l, s.node_act), s.mlp[l]);
        agree = agree && mlp_agrees(xemb_mlp_ops(&m, y, static_cast<const float*>(r.x), s.node_act), s.xemb_bwd);
        if (s.fuse_lin1) {
          const esc_bn_bwd_next nl = readout_next(y);
          if (s.split_lin1)
            agree = agree && plan_readout_block(r.linear, &m, y, 0, L * H, none, slabs).ok &&
                    plan_readout_block(r.linear, &m, y, L * H, H, s.mlp[L - 1].sums == SUMS_READOUT ? &nl : none, slabs).ok;
          else
            agree = agree && plan_readout_block(r.linear, &m, y, 0, y.W, none, slabs).ok;
        }
        for (int l = 1; l < L; ++l)
          if (s.agg[l] == AGG_AFFINE_STATS) {
            const uintptr_t bits = reinterpret_cast<uintptr_t>(y.cat + (int64_t)l * H) | reinterpret_cast<uintptr_t>(y.e[l]) | reinterpret_cast<uintptr_t>(y.dagg) |
                                   reinterpret_cast<uintptr_t>(y.d_e[l]) | reinterpret_cast<uintptr_t>(y.dcat + (int64_t)l * H) | reinterpret_cast<uintptr_t>(y.bst_part);
            entry = entry && H >= 64 && H % 4 == 0 && H <= 2048 && y.W % 4 == 0 && y.ld_e[l] >= H && y.ld_e[l] % 4 == 0 && (bits & 15) == 0 &&
                    sparse::deps_slots(r.aggregate, H) == 1;
          }
      }
      printf(" cap=%lld agree=%d entry=%d\n", (long long)bst_slots(N), agree, entry);
    } else if (!strcmp(family, "ogb")) {
      esc_ogb_gnn_t m{};
      m.num_layers = L; m.hidden = H; m.num_tasks = a; m.atom_rows = b; m.bond_rows = c; m.drop_ratio = (float)drop / 1000.f; m.residual = 1;
      m.z_rows = 100; m.z_table = P.take(OTHER);
      m.zbn0 = bn(P); m.zlin = linear(P, OTHER, H, H); m.zbn1 = bn(P);
      for (int l = 0; l < L; ++l) {
        esc_ogb_layer_t& q = m.layer[l];
        q.pos = linear(P, OTHER, H, H); q.lin0 = linear(P, OTHER, H, 2 * H); q.bn0 = bn(P); q.lin1 = linear(P, MLP, 2 * H, H); q.bn = bn(P);
        q.vlin0 = linear(P, OTHER, H, 2 * H); q.vbn0 = bn(P); q.vlin1 = linear(P, OTHER, 2 * H, H); q.vbn1 = bn(P);
      }
      const OgbLayout y = plan_layout_ogb(&m, N, E, Z, G, ae, be, base, train != 0);
      const OgbSchedule s = plan_schedule_ogb(&m, y, r, slab_off);
      int l0[ESC_MAX_LAYERS], l1m[ESC_MAX_LAYERS], v0[ESC_MAX_LAYERS], v1[ESC_MAX_LAYERS], hid[ESC_MAX_LAYERS], dh[ESC_MAX_LAYERS], dv[ESC_MAX_LAYERS];
      for (int l = 0; l < L; ++l) {
        l0[l] = s.lin0[l]; l1m[l] = s.lin1[l]; v0[l] = s.vlin0[l]; v1[l] = s.vlin1[l]; hid[l] = s.hidden_from_dx[l]; dh[l] = s.drop_h[l]; dv[l] = s.drop_v[l];
      }
      printf("zlin=%d lin0=%s lin1=%s vlin0=%s vlin1=%s", (int)s.zlin, join(l0, (int)L).c_str(), join(l1m, (int)L).c_str(), join(v0, (int)L).c_str(),
             join(v1, (int)L).c_str());
      emit_terms(s.terms, (int)L);
      printf(" hidden=%s hidden_slots=%lld bonds_on_node=%d drop_h=%s drop_v=%s drop_z1=%d drop_z0=%d", join(hid, (int)L).c_str(), (long long)s.hidden_slots,
             (int)s.bonds_on_node, join(dh, (int)L).c_str(), join(dv, (int)L).c_str(), (int)s.drop_z1, (int)s.drop_z0);
      if (train) {
        const float* slabs = y.slabs + 64 * 7;
        for (int l = 0; l < L; ++l)
          if (s.hidden_from_dx[l]) {
            const esc_bn_bwd_next n0 = ogb_hidden_next(y, l);
            using plan::Op;
            agree = agree && plan::plan_both_bn(r.linear, Op{y.dT, H}, static_cast<const esc_bn_bwd_fused*>(nullptr), Op{y.l[l].Y0, 2 * H},
                                                Op{m.layer[l].lin1.w, 2 * H}, Op{y.dA1, 2 * H}, slabs, &n0, N, H, 2 * H).ok;
          }
      }
      printf(" cap=%lld agree=%d entry=%d\n", (long long)bst_slots_ogb(N), agree, entry);
    } else {
      fprintf(stderr, "unknown family %s\n", family);
      return 2;
    }
  }
  return 0;
}
