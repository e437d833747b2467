// The sparse dispatch plan (esc-gnn_amd/csrc/sparse_plan.h) as a stand-alone host program: tests/test_sparse_plan_cpu.py feeds it
// call descriptions and compares what it prints with the transcription in tests/sparse_cases.py.  No HIP, no library.
//
// stdin, one call per line:
//   entry N C Z rows k n_cols  span acc classified counters deps  9 x (given ld off)  agg_split agg_split_bwd bag_tiled
//     entry        the `entry` of a sparse_cases.Case; N, C, Z, rows, k as there; n_cols: columns of the bag's table gradient
//     span ..      0 / 1 (counters: how many): an armed span, accumulate, classified, BatchNorm counters, d_eps wanted
//     given ld off the operands of sparse_cases.OPERANDS[entry] in order (unused slots: 0 0 0): given or NULL, leading dimension (as the
//                  entries, this program hands the plan mat(pointer, ld): the ld that comes with a NULL operand must not count),
//                  offset of the base in floats past a 16-byte boundary
// stdout, one line per call:
//   family launches  gx0 gy0 gx1 gy1 gx2 gy2  lds slots split cw refused  chunks order_offset bucket_offset
//   scratch_floats(Z, C) deps_slots(C) stats_slots(N) bag_stats_block_rows gp_bwd_blocks(N)
#include <cstdio>
#include <cstring>

#include "sparse_plan.h"

using namespace esc::sparse;

int main() {
  char entry[32];
  long N, C, Z, rows, n_cols, ld[9], off[9];
  int k, span, acc, classified, counters, deps, given[9], ks, kb, kt;
  for (;;) {
    int got = scanf("%31s %ld %ld %ld %ld %d %ld %d %d %d %d %d", entry, &N, &C, &Z, &rows, &k, &n_cols, &span, &acc, &classified, &counters, &deps);
    if (got == EOF) break;
    for (int i = 0; i < 9; ++i) got += scanf("%d %ld %ld", &given[i], &ld[i], &off[i]);
    got += scanf("%d %d %d", &ks, &kb, &kt);
    if (got != 12 + 27 + 3) { fprintf(stderr, "malformed call description\n"); return 2; }
    const SparseKnobs knobs{ks, kb, kt};
    Op o[9];
    for (int i = 0; i < 9; ++i)
      o[i] = mat(given[i] ? reinterpret_cast<const void*>(static_cast<uintptr_t>((i + 1) * (1L << 32) + 4 * off[i])) : nullptr, ld[i]);
    auto is = [&](const char* e) { return !strcmp(entry, e); };
    Plan p;
    long block_rows = 0;
    if (is("agg_fwd") || is("agg_fwd_affine")) p = plan_agg_fwd(knobs, o[0], o[1], o[2], N, C, is("agg_fwd_affine"), span != 0);
    else if (is("agg_bwd") || is("agg_bwd_affine") || is("agg_bwd_stats")) p = plan_agg_bwd(knobs, o[0], o[1], o[2], o[3], o[4], N, C, !is("agg_bwd"), is("agg_bwd_stats"));
    else if (is("pool")) p = plan_segment_pool(o[0], o[1], N, C);
    else if (is("bag_fwd") || is("bag_fwd_acc")) p = plan_bag_fwd(SparseKnobs{}, o[0].p, 0, C, o[1], N, is("bag_fwd_acc"), nullptr, false);
    else if (is("bag_fwd_rows")) {
      p = plan_bag_fwd(knobs, o[0].p, rows, C, o[1], N, acc != 0, o[2].p, given[2] != 0);
      block_rows = bag_stats_block_rows(knobs, o[0].p, rows, C, o[1], N);
    }
    else if (is("bag_bwd")) p = plan_bag_bwd(o[0], o[1].p, o[2].p, Z, C, n_cols, 0, false);
    else if (is("bag_bwd_rows")) p = plan_bag_bwd(o[0], o[1].p, o[2].p, Z, C, n_cols, rows, classified != 0);
    else if (is("classify")) p = plan_bag_classify(Z, C, rows, counters);
    else if (is("embed_bwd")) p = plan_embed_bwd(o[0], o[1].p, rows, C);
    else if (is("gp_fwd")) p = plan_gineplus_fwd(GpOps{o[0], o[1], o[2], o[3], o[4], o[6].p}, o[5], N, C);
    else if (is("gp_bwd")) p = plan_gineplus_bwd(GpOps{o[0], o[1], o[2], o[3], o[4], o[8].p}, o[5], o[6], o[7], N, C, k, deps != 0);
    else if (is("gated_fwd") || is("gated_bwd")) p = plan_gated(N, C, is("gated_bwd"));
    else { fprintf(stderr, "unknown entry %s\n", entry); return 2; }
    printf("%s %d", family_name(p).c_str(), p.launches);
    for (const Grid& g : p.grid) printf(" %u %u", g.x, g.y);
    printf(" %zu %lld %d %d %d %lld %lld %lld", p.lds, (long long)p.slots, p.split, p.cw, p.refused ? 1 : 0, (long long)p.chunks, (long long)p.order_offset,
           (long long)p.bucket_offset);
    printf(" %lld %d %lld %ld %lld\n", (long long)scratch_floats(Z, C), deps_slots(knobs, C), (long long)stats_slots(N), block_rows, (long long)gp_bwd_blocks(N));
  }
  return 0;
}
