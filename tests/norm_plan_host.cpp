// The BatchNorm dispatch plan (esc-gnn_amd/csrc/norm_plan.h) as a stand-alone host program: tests/test_norm_plan_cpu.py feeds it
// call descriptions and compares what it prints with the transcription in tests/norm_cases.py.  No HIP, no library.
//
// stdin, one call per line:
//   entry M C  ldX offX  ldY offY  lddY offdY  lddX offdX  offMean offGamma offP offS  has_Y affine nograd extra  k8 k9 k12 k13
//     entry      the `entry` of a norm_cases.Case (stats, apply, bwd, bwd_dropout, ...)
//     ld / off   leading dimension and offset (floats past a 16-byte boundary) of the matrices X, Y, dY, dX; offsets of mean /
//                invstd, gamma / beta, scale / shift, and of the scratch (bwd_apply: of its coef operand)
//     has_Y, affine, nograd   0 / 1: Y given, gamma / beta given, dgamma / dbeta NOT given
//     extra      bwd_dropout: mask_on_output; else unused
// stdout, one line per call:
//   family  launches  slots  gx0 gy0 gx1 gy1 gx2 gy2  scratch_floats
#include <cstdio>
#include <cstring>

#include "norm_plan.h"

using namespace esc::norm;

static const void* at(int which, long off) { return reinterpret_cast<const void*>(static_cast<uintptr_t>((which + 1) * (1L << 32) + 4 * off)); }

int main() {
  char entry[32];
  long M, C, ld[4], off[4], off_mean, off_gamma, off_p, off_s, extra;
  int has_y, affine, nograd, k8, k9, k12, k13;
  for (;;) {
    int got = scanf("%31s %ld %ld", entry, &M, &C);
    if (got == EOF) break;
    for (int i = 0; i < 4; ++i) got += scanf("%ld %ld", &ld[i], &off[i]);
    got += scanf("%ld %ld %ld %ld %d %d %d %ld %d %d %d %d", &off_mean, &off_gamma, &off_p, &off_s, &has_y, &affine, &nograd, &extra, &k8, &k9, &k12, &k13);
    if (got != 3 + 8 + 12) { fprintf(stderr, "malformed call description\n"); return 2; }
    const NormKnobs k{k8 != 0, k9, k12 != 0, k13 != 0};
    const Op X{at(0, off[0]), ld[0]}, Y{at(1, off[1]), ld[1]}, dY{at(2, off[2]), ld[2]}, dX{at(3, off[3]), ld[3]};
    const void *gamma = affine ? at(5, off_gamma) : nullptr, *beta = affine ? at(6, off_gamma) : nullptr, *S = at(9, off_s);
    const void *dgamma = nograd ? nullptr : at(10, 0), *dbeta = nograd ? nullptr : at(11, 0);
    // (as norm.hip's ops_of: an operand the call does not have is NULL; the scratch is `partial` except for bwd_apply, whose coef it is)
    BwdOps o{X, has_y ? Y : Op{nullptr, 0}, dY, Op{nullptr, 0}, at(4, off_mean), at(4, off_mean + C), gamma, beta, S, nullptr, nullptr, nullptr};
    Plan p;
    if (!strcmp(entry, "stats")) p = plan_stats(X, S, M, C);
    else if (!strcmp(entry, "stats_partials")) p = plan_columns(F_PARTIALS_32, C);
    else if (!strcmp(entry, "stats_partials_rows")) p = plan_columns(F_PARTIALS_ROWS, C);
    else if (!strcmp(entry, "affine_fold")) p = plan_affine_fold(M, C);
    else if (!strcmp(entry, "apply")) p = plan_apply(X, Y, M, C);
    else if (!strcmp(entry, "affine")) p = plan_affine(X, Y, at(7, off_p), at(8, off_p), M, C);
    else if (!strcmp(entry, "eval_coef")) p = plan_columns(F_EVAL_COEF, C);
    else if (!strcmp(entry, "coef_partials")) p = plan_columns(F_COEF_PARTIALS, C);
    else if (!strcmp(entry, "bwd_sums")) p = plan_bwd_reduce(k, o, M, C, false, false);
    else if (!strcmp(entry, "bwd_coef")) p = plan_bwd_reduce(k, o, M, C, true, true);
    else {
      o.dX = dX;
      if (!strcmp(entry, "bwd")) { o.dgamma = dgamma; o.dbeta = dbeta; p = plan_bwd(k, o, M, C); }
      else if (!strcmp(entry, "bwd_apply")) { o.partial = nullptr; o.coef = S; p = plan_bwd_apply(o, M, C); }
      else if (!strcmp(entry, "bwd_dropout")) p = plan_bwd_dropout(k, o, M, C, extra != 0);
      else { fprintf(stderr, "unknown entry %s\n", entry); return 2; }
    }
    printf("%s %d %d", family_name(p).c_str(), p.launches, p.slots);
    for (const Grid& g : p.grid) printf(" %u %u", g.x, g.y);
    printf(" %lld\n", (long long)scratch_floats(C));
  }
  return 0;
}
