// row_walk.h — the frame of the row kernels of the message-passing layers (aggregate.hip, gineplus.hip, gatedgcn.hip; DESIGN.md
// 6s), once: the row accessors, the batched walk over a node's range of a sorted
// edge view, the group of float4 lanes that owns a node with its column loop, and the host side of a lane-group file (the limits
// check, the choice of an instantiation by the plan's lanes per node).
//
// The walk.  A wave, or a group of lanes, owns a node and walks its range [beg, end) of the view in batches of BATCH slots:
// every read of a batch is issued before the first use, so a batch costs one round of memory latency and the typical in-degree
// (6-7 for the counting graphs, 2-4 for the molecules) costs ONE round instead of one per edge.  A short tail is padded, not
// peeled: a slot past the end reads the node's LAST edge again (position clamped to end - 1: a valid address, a row that is in
// the cache already) and its contribution is masked, so the loop keeps one shape and its reads stay unconditional.  Slots are
// used in ascending position, so every column sums its edges in edge order and the result is bit-stable, whatever else shares
// the wave, the workgroup or the launch.  beg == end runs no batch: end - 1 is never formed for an empty range.
#pragma once
#include "common.h"

namespace esc {

// ---- VEC consecutive floats of a row <-> registers (16-, 8- or 4-byte accesses) -------------------------------------------------
template <int VEC> __device__ __forceinline__ void row_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) { const float4 a = *reinterpret_cast<const float4*>(p); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
  else if constexpr (VEC == 2) { const float2 a = *reinterpret_cast<const float2*>(p); v[0] = a.x; v[1] = a.y; }
  else v[0] = *p;
}
template <int VEC> __device__ __forceinline__ void row_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else if constexpr (VEC == 2) *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
  else *p = v[0];
}

// ---- the walk -----------------------------------------------------------------------------------------------------------------
// fetch(u, jj, live) for every slot u of a batch, jj the clamped position and live whether the slot is inside the range; then
// use(u) in ascending u - for the live slots alone (MASK), or for every slot where fetch has recorded what a dead slot must not
// do (GINE+'s distance 0).  The batch's registers are the caller's locals, indexed by u.
template <int BATCH, bool MASK = true, class Fetch, class Use>
__device__ __forceinline__ void segment_batches(int beg, int end, Fetch fetch, Use use) {
  for (int j = beg; j < end; j += BATCH) {
#pragma unroll
    for (int u = 0; u < BATCH; ++u) fetch(u, min(j + u, end - 1), j + u < end);
#pragma unroll
    for (int u = 0; u < BATCH; ++u) {
      if (!MASK || j + u < end) use(u);                   // uniform over the owner of the node
    }
  }
}

// ---- a group of LG float4 lanes per node ---------------------------------------------------------------------------------------
// the node of this lane's group and the first column of the lane; false: nothing to do.  A wave holds 64 / LG groups.
template <int LG>
__device__ __forceinline__ bool group_locate(int N, int& node, int& c0) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t g = t / LG;
  node = (int)g;
  c0 = (int)(t - g * LG) * 4;
  return g < N;
}

// body(node, c, beg, end) for the lane's four columns c .. c + 3 of its node, pass by pass (one pass up to C = LG * 4), with
// the node's range of the view whose segment pointers are ptr.  The groups of a wave walk their own ranges: the walk inside
// body diverges between groups, never inside one.
template <int LG, class Body>
__device__ __forceinline__ void group_columns(const int* __restrict__ ptr, int N, int C, Body body) {
  int node, c0;
  if (!group_locate<LG>(N, node, c0)) return;
  const int beg = ptr[node], end = ptr[node + 1];
  for (int c = c0; c < C; c += LG * 4) body(node, c, beg, end);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the instantiation of a kernel template over LG for the plan's lanes per node (sparse::plan_gated's cw)
#define ESC_GROUP_KERNEL(kernel, lanes) ((lanes) == 16 ? kernel<16> : (lanes) == 32 ? kernel<32> : kernel<64>)

struct RowLd {
  const char* name;
  int64_t ld;
};

// what the entries of a lane-group file check before anything is launched; 0 or an error code with the message set.
// max_query: the entry that answers max_c
template <int NL, int NP>
inline int group_limits(const char* fn, const char* max_query, int64_t max_c, int64_t N, int64_t E, int64_t C, const RowLd (&ld)[NL],
                        const void* const (&p)[NP]) {
  ESC_REQUIRE(C >= 4 && C <= max_c && C % 4 == 0, "%s: C=%ld: the width must be a multiple of 4 with 4 <= C <= %ld (%s)", fn, (long)C, (long)max_c,
              max_query);
  for (const RowLd& l : ld)
    ESC_REQUIRE(l.ld >= C && l.ld % 4 == 0, "%s: leading dimension %s=%ld: every leading dimension must be >= C=%ld and a multiple of 4", fn, l.name,
                (long)l.ld, (long)C);
  for (const void* q : p) ESC_REQUIRE(aligned16(q), "%s: every pointer must be 16-byte aligned", fn);
  ESC_REQUIRE(N >= 0 && E >= 0 && N < (1LL << 31) / 64 && E < (1LL << 31), "%s: bad sizes N=%ld E=%ld", fn, (long)N, (long)E);
  return ESC_OK;
}

}  // namespace esc
