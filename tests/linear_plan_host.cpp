// The Linear dispatch plan (esc-gnn_amd/csrc/linear_plan.h) as a stand-alone host program: tests/test_linear_plan_cpu.py feeds it
// call descriptions and compares what it prints with the transcription in tests/linear_cases.py.  No HIP, no library.
//
// stdin, one call per line:
//   entry M N K  ldX offX  ldW offW  ldY offY  lddX offdX  lddW offdW  offP  pro col_stats dx  k0 k1 k2 k3 k4 k5 k6 k7  use_dma
//     entry      fwd | bwd_input | bwd_weight | bwd_both
//     ld / off   leading dimension and offset (floats past a 16-byte boundary) of X [M,K], W [N,K], Y [M,N] (dY of the
//                gradients), dX [M,K], dW [N,K]; offP: offset of in_scale / in_shift
//     pro, col_stats, dx   0 / 1: prologue given, forward writes col_stats, bwd_both is given a dX
// stdout, one line per call:
//   family  block_rows  promised_block_rows  splits  slab_floats_written  slab_floats_promised
#include <cstdio>
#include <cstring>

#include "linear_plan.h"

using namespace esc::plan;

static Op operand(int which, long ld, long off) {
  return Op{reinterpret_cast<const void*>(static_cast<uintptr_t>((which + 1) * (1L << 32) + 4 * off)), ld};
}

int main() {
  char entry[32];
  long M, N, K, ld[5], off[5], offP;
  int pro, col_stats, dx;
  PlanKnobs k;
  for (;;) {
    int got = scanf("%31s %ld %ld %ld", entry, &M, &N, &K);
    if (got == EOF) break;
    for (int i = 0; i < 5; ++i) got += scanf("%ld %ld", &ld[i], &off[i]);
    got += scanf("%ld %d %d %d", &offP, &pro, &col_stats, &dx);
    for (int i = 0; i < KNOB_COUNT; ++i) got += scanf("%d", &k.knob[i]);
    got += scanf("%d", &k.use_dma);
    if (got != 4 + 10 + 4 + KNOB_COUNT + 1) { fprintf(stderr, "malformed call description\n"); return 2; }
    const Op X = operand(0, ld[0], off[0]), W = operand(1, ld[1], off[1]), Y = operand(2, ld[2], off[2]);
    const Op dX = dx ? operand(3, ld[3], off[3]) : Op{nullptr, ld[3]}, dW = operand(4, ld[4], off[4]);
    const void* slabs = operand(5, 0, 0).p;
    Flags f;
    f.pro = pro != 0;
    f.pro_aligned = !pro || offP % 4 == 0;
    f.col_stats = col_stats != 0;
    Plan p;
    long promised_rows = 0;
    if (!strcmp(entry, "fwd")) {
      p = plan_fwd(k, X, W, M, N, K, f);
      promised_rows = (long)stats_block_rows(k, X, W, M, N, K);
    } else if (!strcmp(entry, "bwd_input")) {
      p = plan_dx(k, Y, W, dX, M, N, K);
    } else if (!strcmp(entry, "bwd_weight")) {
      p = plan_dw(k, Y, X, slabs, M, N, K);
    } else if (!strcmp(entry, "bwd_both")) {
      p = plan_both(k, Y, X, W, dX, dW, slabs, M, N, K, f);
    } else {
      fprintf(stderr, "unknown entry %s\n", entry);
      return 2;
    }
    printf("%s %d %ld %d %lld %lld\n", family_name(p.family), p.block_rows, promised_rows, p.splits, (long long)p.slab_floats,
           (long long)bwd_weight_scratch(M, N, K));
  }
  return 0;
}
