// The step engines' host plan (esc-gnn_amd/csrc/engine_plan.h) as a stand-alone host program: tests/test_engine_plan_cpu.py feeds
// it model and batch sizes and checks what it prints.  No HIP, no library; the descriptors carry sizes only.
//
// stdin, one request per line:
//   family L H a b c drop  N E Z G atom_entries bond_entries
//     family     count | zinc | ogb
//     a b c      count: in_dim 0 0;  zinc: node width, edge-type width, node_readout;  ogb: num_tasks, atom_rows, bond_rows
//     drop       ogb: drop_ratio in thousandths
// stdout, one line per request:
//   train_floats predict_floats slab_floats reduce_jobs walked over  n  M N K ... (n triples)
//     walked     1: a SlabCursor over slab_floats handed out a region for every listed gradient, inside the limit, in the split
//                form of the list and (a list with a split Linear) with that Linear taken whole
//     over       1: the budget is tight: the walk (a split Linear: the larger of its two forms) ended exactly at the limit, and one
//                further take of EVERY listed shape was refused and moved nothing; after the smaller form of a split Linear, which
//                leaves the difference of the two forms unused, every listed shape that does not fit that remainder was refused
#include <cstdio>
#include <cstring>

#include "engine_plan.h"

using namespace esc;

static bool walk(const WGradList& w, bool whole, bool* over, int64_t* left) {
  float* const base = reinterpret_cast<float*>(static_cast<uintptr_t>(1) << 32);
  SlabCursor cur{base, 0, slab_floats(w)};
  bool ok = true;
  for (int i = 0; i < (int)w.g.size(); ++i) {
    WGrad g = w.g[i];
    if (whole && i == w.split) { g.K += w.g[i + 1].K; ++i; }
    const float* before = cur.peek();
    const float* p = cur.take(g.M, g.N, g.K);
    ok = ok && p != nullptr && p == before && cur.off <= cur.limit && (reinterpret_cast<uintptr_t>(p) & 255) == 0;
  }
  *left = cur.limit - cur.off;
  for (const WGrad& g : w.g) {           // one further take: refused, nothing moved, unless the shape fits what this form left over
    const int64_t off = cur.off;
    const bool refused = cur.take(g.M, g.N, g.K) == nullptr;
    *over = *over && refused == (slab_floats(g) > *left) && (!refused || cur.off == off);
    cur.off = off;
  }
  return ok;
}

int main() {
  char family[16];
  long L, H, a, b, c, drop, N, E, Z, G, ae, be;
  for (;;) {
    const int got = scanf("%15s %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld %ld", family, &L, &H, &a, &b, &c, &drop, &N, &E, &Z, &G, &ae, &be);
    if (got == EOF) break;
    if (got != 13 || L < 1 || L > ESC_MAX_LAYERS) { fprintf(stderr, "malformed request\n"); return 2; }
    WGradList w;
    long long train = 0, predict = 0, slabs = 0;
    int jobs = 0;
    if (!strcmp(family, "count")) {
      esc_nested_gin_t m{};
      m.num_layers = L; m.hidden = H; m.in_dim = a;
      w = weight_grads(&m, N, E);
      const Layout t = plan_layout(&m, N, E, Z, nullptr, true);
      train = t.total; predict = plan_layout(&m, N, E, Z, nullptr, false).total; slabs = t.slab_limit; jobs = t.n_wgrads;
    } else if (!strcmp(family, "zinc")) {
      esc_zinc_gin_t m{};
      m.num_layers = L; m.hidden = H; m.node_emb.dim = a; m.edge_emb.dim = b; m.node_readout = (int32_t)c;
      w = weight_grads_zinc(&m, N, E, G);
      const Layout t = plan_layout_zinc(&m, N, E, Z, G, nullptr, true);
      train = t.total; predict = plan_layout_zinc(&m, N, E, Z, G, nullptr, false).total; slabs = t.slab_limit; jobs = t.n_wgrads;
    } else if (!strcmp(family, "ogb")) {
      esc_ogb_gnn_t m{};
      m.num_layers = L; m.hidden = H; m.num_tasks = a; m.atom_rows = b; m.bond_rows = c; m.drop_ratio = (float)drop / 1000.f;
      w = weight_grads_ogb(&m, N, E, G);
      const OgbLayout t = plan_layout_ogb(&m, N, E, Z, G, ae, be, nullptr, true);
      train = t.total; predict = plan_layout_ogb(&m, N, E, Z, G, ae, be, nullptr, false).total; slabs = t.slab_limit; jobs = t.n_wgrads;
    } else {
      fprintf(stderr, "unknown family %s\n", family);
      return 2;
    }
    if (slabs != slab_floats(w) || jobs != reduce_jobs(w)) { fprintf(stderr, "the layout does not carry the list's figures\n"); return 3; }
    bool over = true;
    int64_t left = 0, left_whole = 0;
    bool walked = walk(w, false, &over, &left);
    if (w.split >= 0) walked = walk(w, true, &over, &left_whole) && walked;
    else left_whole = left;
    over = over && (left == 0 || left_whole == 0) && left >= 0 && left_whole >= 0;
    printf("%lld %lld %lld %d %d %d  %d", train, predict, slabs, jobs, walked ? 1 : 0, over ? 1 : 0, (int)w.g.size());
    for (const WGrad& g : w.g) printf("  %lld %lld %lld", (long long)g.M, (long long)g.N, (long long)g.K);
    printf("\n");
  }
  return 0;
}
