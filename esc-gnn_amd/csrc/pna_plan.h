// pna_plan.h — how many lanes own a node and on which grids the PNA aggregate (pna.hip) runs: decided ONCE, on the host.
//
// Host-only C++ like sparse_plan.h (g++ compiles it alone, tests/pna_plan_host.cpp does); a pure function of N and C.  The
// lanes-per-node thresholds are GatedGCN's (sparse_plan.h: GG_GROUP16_MAX_C, GG_GROUP32_MAX_C), for GatedGCN's reasons (DESIGN
// 6q): a row of C floats is covered by float4 lanes, so 16 lanes cover C <= 64, 32 lanes C <= 128, and a whole wave loops over
// anything wider.  Not a family of sparse_plan.h's tables: the three kernels have one form each.
#pragma once
#include "sparse_plan.h"

namespace esc {
namespace pna {

constexpr int64_t MAX_C = 1024;               // esc_pna_max_channels
constexpr int BLOCK = 256;                    // threads of every workgroup: four waves

struct Plan {
  int lanes = 0;                              // float4 lanes that own one node: 16 | 32 | 64
  int nodes_per_wave = 0;                     // 64 / lanes
  int launches = 0;
  unsigned grid[2] = {0, 0};                  // workgroups of each launch, in launch order
};

inline int lanes_per_node(int64_t C) { return C <= sparse::GG_GROUP16_MAX_C ? 16 : C <= sparse::GG_GROUP32_MAX_C ? 32 : 64; }

// forward: one launch over the destination view; backward: the destination view, then the source view - a group per node each
inline Plan plan_aggregate(int64_t N, int64_t C, bool backward) {
  Plan p;
  p.lanes = lanes_per_node(C);
  p.nodes_per_wave = 64 / p.lanes;
  p.launches = backward ? 2 : 1;
  for (int i = 0; i < p.launches; ++i) p.grid[i] = (unsigned)sparse::cdiv(N * p.lanes, BLOCK);
  return p;
}

}  // namespace pna
}  // namespace esc
