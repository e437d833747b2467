// layernorm_plan.h — how a workgroup of the per-graph LayerNorm (layernorm.hip) is cut and on which grids it runs: decided ONCE,
// on the host.
//
// Host-only C++ like pna_plan.h (g++ compiles it alone, tests/layernorm_plan_host.cpp does); a pure function of G and C.  One
// workgroup owns a graph.  A row of C floats is Q = C / 4 float4 lanes; a workgroup of `block` threads is R = block / Q row lanes
// of Q column lanes each (the block % Q threads left over idle), thread t = rl * Q + cl owns column lane cl of the rows rl, rl + R,
// rl + 2R, ... of its graph.  A thread therefore never changes its columns - weight and bias are read once - and every sum of
// the kernels runs in an order fixed by (n, C): the thread's rows in ascending order, the wave, the waves in ascending order.
// Nothing here sees the batch: a graph is cut the same way alone and beside any other graphs.
// The block grows with the width so that a wide row still leaves several row lanes: 256 threads up to C = 64 (R >= 16),
// 512 up to C = 128 (R >= 16), 1024 beyond (R = 13 at C = 300, 4 at C = 1024).
#pragma once
#include <cstdint>

namespace esc {
namespace layernorm {

constexpr int64_t MAX_C = 1024;               // esc_graph_layer_norm_max_channels: Q <= 256, so R >= 1 at every block
constexpr int BLOCK256_MAX_C = 64;            // widest row of a 256-thread workgroup
constexpr int BLOCK512_MAX_C = 128;           // ... of a 512-thread one
constexpr int CHAINS = 64;                    // the second backward launch: interleaved chains over the graphs, one wave

struct Plan {
  int block = 0;                              // threads of the per-graph workgroup: 256 | 512 | 1024
  int lanes = 0;                              // Q: float4 lanes that cover a row
  int rows = 0;                               // R: rows a workgroup covers in one pass
  int launches = 0;
  unsigned grid[2] = {0, 0};                  // workgroups of each launch, in launch order
};

inline int block_threads(int64_t C) { return C <= BLOCK256_MAX_C ? 256 : C <= BLOCK512_MAX_C ? 512 : 1024; }

// forward: one workgroup per graph.  backward: the same, then - with an affine - one wave per float4 of d_weight | d_bias that
// sums the per-graph partials (2 Q workgroups of CHAINS threads)
inline Plan plan_layer_norm(int64_t G, int64_t C, bool backward, bool affine) {
  Plan p;
  p.block = block_threads(C);
  p.lanes = (int)(C / 4);
  p.rows = p.block / p.lanes;
  p.launches = backward && affine ? 2 : 1;
  p.grid[0] = (unsigned)G;
  if (p.launches == 2) p.grid[1] = (unsigned)(2 * p.lanes);
  return p;
}

}  // namespace layernorm
}  // namespace esc
