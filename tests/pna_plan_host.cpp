// The dispatch rule of the PNA aggregate (esc-gnn_amd/csrc/pna_plan.h) as a stand-alone host program: tests/test_pna_plan_cpu.py
// feeds it sizes and compares what it prints with its transcription.  No HIP, no library.
//
// stdin, one call per line:    N C backward(0 / 1)
// stdout, one line per call:   lanes nodes_per_wave launches grid0 grid1 block max_c
#include <cstdio>

#include "pna_plan.h"

int main() {
  long N, C;
  int backward;
  for (;;) {
    const int got = scanf("%ld %ld %d", &N, &C, &backward);
    if (got == EOF) break;
    if (got != 3) { fprintf(stderr, "malformed call description\n"); return 2; }
    const esc::pna::Plan p = esc::pna::plan_aggregate(N, C, backward != 0);
    printf("%d %d %d %u %u %d %ld\n", p.lanes, p.nodes_per_wave, p.launches, p.grid[0], p.grid[1], esc::pna::BLOCK, (long)esc::pna::MAX_C);
  }
  return 0;
}
