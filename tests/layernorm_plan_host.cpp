// The work-split rule of the per-graph LayerNorm (esc-gnn_amd/csrc/layernorm_plan.h) as a stand-alone host program:
// tests/test_layernorm_plan_cpu.py feeds it sizes and compares what it prints with its transcription.  No HIP, no library.
//
// stdin, one call per line:    G C backward(0 / 1) affine(0 / 1)
// stdout, one line per call:   block lanes rows launches grid0 grid1 chains max_c
#include <cstdio>

#include "layernorm_plan.h"

int main() {
  long G, C;
  int backward, affine;
  for (;;) {
    const int got = scanf("%ld %ld %d %d", &G, &C, &backward, &affine);
    if (got == EOF) break;
    if (got != 4) { fprintf(stderr, "malformed call description\n"); return 2; }
    const esc::layernorm::Plan p = esc::layernorm::plan_layer_norm(G, C, backward != 0, affine != 0);
    printf("%d %d %d %d %u %u %d %ld\n", p.block, p.lanes, p.rows, p.launches, p.grid[0], p.grid[1], esc::layernorm::CHAINS,
           (long)esc::layernorm::MAX_C);
  }
  return 0;
}
