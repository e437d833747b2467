// plan_both_bn of the Linear dispatch plan (esc-gnn_amd/csrc/linear_plan.h) as a stand-alone host program, for every operand of an
// esc_linear_bwd_both_bn call: tests/test_bnb_cases_cpu.py asks it for the plan of each record of tests/bnb_cases.py and holds
// bnb_cases.family_of against the answer.  No HIP, no library.  (tests/readout_plan_host.cpp asks about PlanKnobs::dual_split on
// one operand; this one describes the whole call.)
//
// stdin, one call per line, integers:
//     M N K  bn next  bn_act next_act  dx_null  bn_beta next_beta  request
//     ld off            x 6   dOut [M,N], bn.x [M,N], X [M,K], W [N,K], dX [M,K], next.x [M,K]   (off: floats past a 16-byte boundary)
//     off               x 13  bn: mean invstd scale shift coef beta; next: partial mean invstd scale shift beta; slabs
//   bn / next      0 / 1: the structure is given          bn_beta / next_beta   0: its beta is NULL
//   request        PlanKnobs::dual_split
// stdout, one line per call:  family  bm  block_rows  splits  per_split  slab_floats_written  slab_floats_promised  launches
#include <cstdio>

#include "linear_plan.h"

using namespace esc::plan;

static const void* at(int which, long off) { return reinterpret_cast<const void*>(static_cast<uintptr_t>((which + 1) * (1L << 36) + 4 * off)); }

int main() {
  for (;;) {
    long M, N, K, ld[6], off[6], voff[13];
    int bn, next, bn_act, next_act, dx_null, bn_beta, next_beta, request;
    int got = scanf("%ld %ld %ld %d %d %d %d %d %d %d %d", &M, &N, &K, &bn, &next, &bn_act, &next_act, &dx_null, &bn_beta, &next_beta, &request);
    if (got == EOF) break;
    if (got != 11) { fprintf(stderr, "malformed call description\n"); return 2; }
    for (int i = 0; i < 6; ++i)
      if (scanf("%ld %ld", &ld[i], &off[i]) != 2) { fprintf(stderr, "malformed matrix description\n"); return 2; }
    for (int i = 0; i < 13; ++i)
      if (scanf("%ld", &voff[i]) != 1) { fprintf(stderr, "malformed vector description\n"); return 2; }
    PlanKnobs k;
    k.dual_split = request;
    const BnOps b{at(1, off[1]), ld[1], at(6, voff[0]), at(7, voff[1]), at(8, voff[2]), at(9, voff[3]), at(10, voff[4]), bn_act,
                  bn_beta ? at(11, voff[5]) : nullptr};
    const NextOps n{at(12, voff[6]), at(5, off[5]), ld[5], at(13, voff[7]), at(14, voff[8]), at(15, voff[9]), at(16, voff[10]), next_act,
                    next_beta ? at(17, voff[11]) : nullptr};
    const Op dX{dx_null ? nullptr : at(4, off[4]), ld[4]};
    const Plan p = plan_both_bn(k, Op{at(0, off[0]), ld[0]}, bn ? &b : nullptr, Op{at(2, off[2]), ld[2]}, Op{at(3, off[3]), ld[3]}, dX,
                                at(18, voff[12]), next ? &n : nullptr, M, N, K);
    printf("%s %d %d %d %d %lld %lld %d\n", family_name(p.family), p.bm, p.block_rows, p.splits, p.per_split, (long long)p.slab_floats,
           (long long)bwd_weight_scratch(M, N, K), p.launches);
  }
  return 0;
}
