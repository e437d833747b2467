// plan_both_bn of the Linear dispatch plan (esc-gnn_amd/csrc/linear_plan.h) as a stand-alone host program:
// tests/test_readout_plan_cpu.py asks it for the plan of esc_linear_bwd_both_bn calls with PlanKnobs::dual_split off and on.
// No HIP, no library.
//
// stdin, one call per line:   M N K  ldX offX  next  request
//     ldX / offX   leading dimension and offset (floats past a 16-byte boundary) of X [M,K]
//     next         0 / 1: the call also leaves the sums of the next BatchNorm backward
//     request      PlanKnobs::dual_split
// stdout, one line per call:  family  bm  splits  per_split  slab_floats_written  slab_floats_promised  launches  dx_lds
#include <cstdio>

#include "linear_plan.h"

using namespace esc::plan;

static const void* at(int which, long off) { return reinterpret_cast<const void*>(static_cast<uintptr_t>((which + 1) * (1L << 32) + 4 * off)); }

int main() {
  long M, N, K, ldx, offx;
  int next, request;
  for (;;) {
    const int got = scanf("%ld %ld %ld %ld %ld %d %d", &M, &N, &K, &ldx, &offx, &next, &request);
    if (got == EOF) break;
    if (got != 7) { fprintf(stderr, "malformed call description\n"); return 2; }
    PlanKnobs k;
    k.dual_split = request;
    const BnOps bn{at(0, 0), N, at(1, 0), at(2, 0), at(3, 0), at(4, 0), at(5, 0), 1};
    const NextOps nx{at(6, 0), at(7, 0), K, at(8, 0), at(9, 0), at(10, 0), at(11, 0), 1};
    const Plan p = plan_both_bn(k, Op{at(12, 0), N}, &bn, Op{at(13, offx), ldx}, Op{at(14, 0), K}, Op{at(15, 0), K}, at(16, 0), next ? &nx : nullptr,
                                M, N, K);
    printf("%s %d %d %d %lld %lld %d %d\n", family_name(p.family), p.bm, p.splits, p.per_split, (long long)p.slab_floats,
           (long long)bwd_weight_scratch(M, N, K), p.launches, p.dx_lds);
  }
  return 0;
}
