// attention.hip — multi-head self-attention over the nodes of every graph of a ragged batch (include/escgnn_gps.h): what the
// reference's GPSLayer runs as to_dense_batch + torch.nn.MultiheadAttention(key_padding_mask) + gather
// (GraphGPS/graphgps/layer/gps_layer.py:234-236,269-286), here straight off graph_ptr: no pad, no mask tensor, no gather and no
// [B, heads, n_max, n_max] score tensor.
//
// Work split: one workgroup per (graph, head), one thread per row.  The K and V slices of the pair (n x head_dim
// each, a few KB at ZINC's 23 nodes x 16) sit in LDS; every thread walks all n keys with ITS query in registers, so all lanes of
// a wave read the same LDS row at the same time — a broadcast, no bank conflict whatever the row stride.  Scores are never
// stored: the softmax takes two passes over the keys (maximum, then exp / sum / PV) and recomputes the dot products: the same
// FMAs per key as the rescaling of an online softmax, and every weight is rounded once.  Plain fp32 FMAs: the workload (128 pairs of 23 x 23
// x 16) is launch- and latency-bound, there is no tile for the f32 MFMA to fill.
// The backward is ONE launch in two phases over the same LDS: phase A (thread = query i, K and V resident) forms
// delta_i = sum_j P_ij dPd_ij and dQ_i; phase B (thread = key j, the scaled Q and dO resident, delta and lse beside them) forms
// dK_j and dV_j.  Both phases recompute S from the same products in the same order (dot<>), so P agrees bit for bit between them.
// Every output row has exactly one writer: no atomics, no cross-workgroup sum, bit-identical run to run.
// head_dim is padded with zero columns to DP = 4, 8, 16, 32 or 64 in LDS and registers (0 * 0 adds exactly nothing), which keeps
// the register arrays compile-time sized with five instantiations.
//
// The biased entry points (include/escgnn_spd.h) are the same kernels with BIAS = true: S_ij gains
// table[min(spd_ij, 100)], the head's 101 entries of the bias table staged in LDS and one byte of the graph's shortest-path matrix
// read per pair - the same single addition in the forward and in both phases of the backward, so P still agrees bit for bit.
// The table's gradient is a histogram of dS by distance: in phase A thread i adds dS_ij to ITS column of the LDS bins
// (bins[b * blockDim + tid]: lanes on consecutive banks, nobody else's words), thread b then sums row b over the threads in a
// fixed rotated order (start at thread b: again consecutive banks) into one partial per (graph, head, b), and a second launch
// sums the partials over the graphs.  No float atomics, one writer per value.  With BIAS = false every `if constexpr` below
// vanishes and the instantiation is the code this file had before the bias existed.
#include "common.h"
#include "../../include/escgnn_gps.h"
#include "../../include/escgnn_spd.h"

namespace esc {

constexpr int ATTN_LDS_FLOATS = 32768;       // K and V (or Q and dO) of one (graph, head): 128 KiB of the CU's 160 KiB
constexpr int ATTN_MAX_NODES = 1024;

constexpr int ATTN_BINS = 101;               // rows of the bias table: the distances 0..99 and row 100 (no path, the padding row)
constexpr int ATTN_TABLE_FLOATS = 104;       // ... as they sit in LDS (a multiple of 4: what follows stays 16-byte aligned)
constexpr int ATTN_LDS_BYTES = 160 * 1024;   // the CU's LDS: the budget of the biased backward

inline int attn_pad(int d) { return d <= 4 ? 4 : d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }
inline int64_t attn_limit(int d) {
  const int64_t fit = ATTN_LDS_FLOATS / 2 / attn_pad(d);
  return fit < ATTN_MAX_NODES ? fit : ATTN_MAX_NODES;
}
// the biased kernels: K and V (then Q and dO), lse and delta resident - (2 DP + 2) floats per node - beside the table and the
// 101 x 256 bins of the backward, inside ATTN_LDS_BYTES; a multiple of 4, and never above the unbiased limit
inline int64_t attn_bias_limit(int d) {
  const int64_t fit = ((ATTN_LDS_BYTES - 4 * (ATTN_TABLE_FLOATS + ATTN_BINS * 256)) / (4 * (2 * attn_pad(d) + 2))) & ~3LL;
  return fit < attn_limit(d) ? fit : attn_limit(d);
}

// keys per trip of the loops over the LDS rows: at one wave per SIMD nothing else hides the LDS latency of a row's reads
template <int DP> constexpr int attn_unroll = DP <= 16 ? 4 : 1;      // (wider rows already fill the registers)

// sum_c reg[c] * row[c] as one FMA chain in ascending c; `row` is a 16-byte aligned LDS row read as float4 (all lanes the same
// address: broadcast).  Phase A and phase B of the backward call it with the operands swapped: same products, same order.
template <int DP>
__device__ __forceinline__ float dot(const float (&reg)[DP], const float* row) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < DP; c += 4) {
    const float4 r = *reinterpret_cast<const float4*>(row + c);
    s = fmaf(reg[c], r.x, s);
    s = fmaf(reg[c + 1], r.y, s);
    s = fmaf(reg[c + 2], r.z, s);
    s = fmaf(reg[c + 3], r.w, s);
  }
  return s;
}
// acc[c] += w * row[c]
template <int DP>
__device__ __forceinline__ void axpy(float (&acc)[DP], float w, const float* row) {
#pragma unroll
  for (int c = 0; c < DP; c += 4) {
    const float4 r = *reinterpret_cast<const float4*>(row + c);
    acc[c] = fmaf(w, r.x, acc[c]);
    acc[c + 1] = fmaf(w, r.y, acc[c + 1]);
    acc[c + 2] = fmaf(w, r.z, acc[c + 2]);
    acc[c + 3] = fmaf(w, r.w, acc[c + 3]);
  }
}
// acc[c] += w * (row[c] - row0[c])
template <int DP>
__device__ __forceinline__ void axpy_diff(float (&acc)[DP], float w, const float* row, const float* row0) {
#pragma unroll
  for (int c = 0; c < DP; c += 4) {
    const float4 r = *reinterpret_cast<const float4*>(row + c);
    const float4 z = *reinterpret_cast<const float4*>(row0 + c);
    acc[c] = fmaf(w, r.x - z.x, acc[c]);
    acc[c + 1] = fmaf(w, r.y - z.y, acc[c + 1]);
    acc[c + 2] = fmaf(w, r.z - z.z, acc[c + 2]);
    acc[c + 3] = fmaf(w, r.w - z.w, acc[c + 3]);
  }
}
// d columns (a multiple of 4) of a global row into DP registers (zero beyond d), times `mul`
template <int DP>
__device__ __forceinline__ void load_row(float (&reg)[DP], const float* src, int d, float mul) {
#pragma unroll
  for (int c = 0; c < DP; c += 4) {
    const bool in = c < d;
#pragma unroll
    for (int u = 0; u < 4; ++u) reg[c + u] = in ? src[c + u] * mul : 0.f;
  }
}
// ... and d columns of DP registers, times `mul`, into a global row
template <int DP>
__device__ __forceinline__ void store_row(float* dst, const float (&reg)[DP], int d, float mul) {
#pragma unroll
  for (int c = 0; c < DP; c += 4) {
    if (c < d) {
#pragma unroll
      for (int u = 0; u < 4; ++u) dst[c + u] = reg[c + u] * mul;
    }
  }
}
// rows [n0, n0+n) x d columns of two global matrices into two LDS tiles of row stride DP (zero beyond d), the first times `mul`
template <int DP>
__device__ __forceinline__ void stage_pair(float* A, float* B, const float* a_src, int64_t lda, const float* b_src, int64_t ldb, int n,
                                           int d, float mul) {
  for (int t = threadIdx.x; t < n * DP; t += blockDim.x) {
    const int r = t / DP, c = t % DP;
    A[t] = c < d ? a_src[(int64_t)r * lda + c] * mul : 0.f;
    B[t] = c < d ? b_src[(int64_t)r * ldb + c] : 0.f;
  }
}

// the operands of the biased instantiations (BIAS = false never reads them)
struct AttnBias {
  const unsigned char* spd; const float* table;      // spd [spd_pairs] bytes in pair_ptr's layout; table [101, heads]
  float* partial;                                     // backward: [heads, 101, G] sums of dS of one (graph, head) by distance
  int64_t spd_pairs;
};
// S_ij of a biased instantiation: the scaled product plus the head's table entry of the pair's distance byte (above 100: row 100)
template <bool BIAS>
__device__ __forceinline__ float biased(float s, const float* Bs, const unsigned char* sp, int at) {
  if constexpr (BIAS) {
    const int b = sp[at];
    return s + Bs[b < ATTN_BINS - 1 ? b : ATTN_BINS - 1];
  } else {
    return s;
  }
}
// the head's column of the table into LDS (the caller's barrier follows)
__device__ __forceinline__ void stage_table(float* Bs, const float* table, int heads, int a) {
  for (int t = threadIdx.x; t < ATTN_BINS; t += blockDim.x) Bs[t] = table[t * heads + a];
}

struct AttnShape {
  const int32_t* graph_ptr; const int64_t* pair_ptr;
  int N, cap, heads, d;                      // cap: rows the LDS tiles hold (>= the largest graph the caller announced)
  int64_t mask_pairs;                        // pairs per head the mask buffer has room for (>= pair_ptr[G])
  float scale, p, inv_keep;
};
// node range of this workgroup's graph and the offset of its mask bytes in the head's block; false (for the whole workgroup)
// when there is nothing to do or the graph does not fit
__device__ __forceinline__ bool attn_graph(const AttnShape& z, int head, int& n0, int& n, unsigned long long& mbase) {
  n0 = z.graph_ptr[blockIdx.x];
  n = z.graph_ptr[blockIdx.x + 1] - n0;
  if (!(n > 0 && n <= z.cap && n0 >= 0 && n0 <= z.N - n)) return false;
  const int64_t m0 = z.pair_ptr[blockIdx.x], total = z.pair_ptr[gridDim.x];     // ... and its n*n mask bytes inside the buffer
  mbase = (unsigned long long)head * total + m0;
  return m0 >= 0 && z.pair_ptr[blockIdx.x + 1] - m0 == (int64_t)n * n && m0 <= total - (int64_t)n * n && (z.p <= 0.f || total <= z.mask_pairs);
}

template <int DP, bool BIAS>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ qkv, int64_t ld, AttnShape z, unsigned long long seed,
                                                       float* __restrict__ out, int64_t ldo, float* __restrict__ lse,
                                                       unsigned char* __restrict__ mask, AttnBias bz) {
  constexpr int UJ = attn_unroll<DP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ks = reinterpret_cast<float*>(smem);
  float* Vs = Ks + (size_t)z.cap * DP;
  [[maybe_unused]] float* Bs = Vs + (size_t)z.cap * DP;               // BIAS: the head's table
  [[maybe_unused]] const unsigned char* sp = nullptr;                 // BIAS: the graph's distance bytes
  int n0, n;
  unsigned long long mbase;
  const int a = blockIdx.y, d = z.d, H = z.heads * z.d;
  if (!attn_graph(z, a, n0, n, mbase)) return;
  if constexpr (BIAS) {
    if (z.pair_ptr[gridDim.x] > bz.spd_pairs) return;                 // the bytes would leave the buffer: skipped, like the mask's rule
    sp = bz.spd + z.pair_ptr[blockIdx.x];
    stage_table(Bs, bz.table, z.heads, a);
  }
  const float* rows = qkv + (int64_t)n0 * ld + a * d;
  stage_pair<DP>(Ks, Vs, rows + H, ld, rows + 2 * H, ld, n, d, 1.f);
  __syncthreads();
  const bool drop = z.p > 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float q[DP];
    load_row<DP>(q, rows + (int64_t)i * ld, d, z.scale);
    float m = -INFINITY;
#pragma unroll UJ
    for (int j = 0; j < n; ++j) m = fmaxf(m, biased<BIAS>(dot<DP>(q, Ks + j * DP), Bs, sp, i * n + j));
    float acc[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) acc[c] = 0.f;
    float l = 0.f;
    const unsigned long long mrow = mbase + (unsigned long long)i * n;
#pragma unroll UJ
    for (int j = 0; j < n; ++j) {
      const float e = expf(biased<BIAS>(dot<DP>(q, Ks + j * DP), Bs, sp, i * n + j) - m);
      l += e;
      float w = e;
      if (drop) {
        const bool keep = uniform01(seed, mrow + j) >= z.p;
        mask[mrow + j] = keep ? 1 : 0;
        w = keep ? e * z.inv_keep : 0.f;
      }
      axpy<DP>(acc, w, Vs + j * DP);
    }
    store_row<DP>(out + (int64_t)(n0 + i) * ldo + a * d, acc, d, 1.f / l);
    lse[(int64_t)a * z.N + n0 + i] = m + logf(l);
  }
}

template <int DP, bool BIAS>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ qkv, int64_t ld, const float* __restrict__ d_out,
                                                       int64_t ldg, const float* __restrict__ lse, const unsigned char* __restrict__ mask,
                                                       AttnShape z, float* __restrict__ d_qkv, AttnBias bz) {
  constexpr int UJ = attn_unroll<DP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* T0 = reinterpret_cast<float*>(smem);          // phase A: K, phase B: Q * scale
  float* T1 = T0 + (size_t)z.cap * DP;                 // phase A: V, phase B: dO
  float* Ls = T1 + (size_t)z.cap * DP;                 // lse of the rows
  float* Ds = Ls + z.cap;                              // delta of the rows
  [[maybe_unused]] float* Bs = Ds + z.cap;             // BIAS: the head's table ...
  [[maybe_unused]] float* bins = Bs + ATTN_TABLE_FLOATS;               // ... and [101][blockDim] sums of dS: one column per thread
  [[maybe_unused]] const unsigned char* sp = nullptr;  // BIAS: the graph's distance bytes
  int n0, n;
  unsigned long long mbase;
  const int a = blockIdx.y, d = z.d, H = z.heads * z.d;
  if constexpr (BIAS) {
    float* part = bz.partial + (int64_t)a * ATTN_BINS * gridDim.x + blockIdx.x;      // [a][b][g]
    if (!attn_graph(z, a, n0, n, mbase) || z.pair_ptr[gridDim.x] > bz.spd_pairs) {   // skipped: the second launch still adds its slots
      for (int b = threadIdx.x; b < ATTN_BINS; b += blockDim.x) part[(int64_t)b * gridDim.x] = 0.f;
      return;
    }
    sp = bz.spd + z.pair_ptr[blockIdx.x];
    stage_table(Bs, bz.table, z.heads, a);
    for (int t = threadIdx.x; t < ATTN_BINS * (int)blockDim.x; t += blockDim.x) bins[t] = 0.f;
  } else {
    if (!attn_graph(z, a, n0, n, mbase)) return;
  }
  const float* rows = qkv + (int64_t)n0 * ld + a * d;
  const float* grows = d_out + (int64_t)n0 * ldg + a * d;
  float* drows = d_qkv + (int64_t)n0 * 3 * H + a * d;
  const bool drop = z.p > 0.f;

  // ---- phase A: thread = query i; delta_i = sum_j P_ij dPd_ij, then dQ_i = scale * sum_j P_ij (dPd_ij - delta_i) (K_j - K_0)
  stage_pair<DP>(T0, T1, rows + H, ld, rows + 2 * H, ld, n, d, 1.f);
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    float q[DP], g[DP];
    load_row<DP>(q, rows + (int64_t)i * ld, d, z.scale);
    load_row<DP>(g, grows + (int64_t)i * ldg, d, 1.f);
    const float L = lse[(int64_t)a * z.N + n0 + i];
    const unsigned char* mrow = mask + mbase + (unsigned long long)i * n;
    float delta = 0.f;
#pragma unroll UJ
    for (int j = 0; j < n; ++j) {
      const float P = expf(biased<BIAS>(dot<DP>(q, T0 + j * DP), Bs, sp, i * n + j) - L);
      float dp = dot<DP>(g, T1 + j * DP);
      if (drop) dp = mrow[j] ? dp * z.inv_keep : 0.f;
      delta = fmaf(P, dp, delta);
    }
    float dq[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) dq[c] = 0.f;
#pragma unroll UJ
    for (int j = 0; j < n; ++j) {
      const float P = expf(biased<BIAS>(dot<DP>(q, T0 + j * DP), Bs, sp, i * n + j) - L);
      float dp = dot<DP>(g, T1 + j * DP);
      if (drop) dp = mrow[j] ? dp * z.inv_keep : 0.f;
      // sum_j P_ij (dPd_ij - delta_i) is 0 by the definition of delta, so any one row may be taken off every K_j: with K_0, a
      // graph whose keys are all equal (one node included) gets d_q = 0 exactly instead of a rounding residue times K
      axpy_diff<DP>(dq, P * (dp - delta), T0 + j * DP, T0);
      if constexpr (BIAS) {                              // dS_ij into this thread's column of its distance's row
        const int b = sp[i * n + j];
        bins[(b < ATTN_BINS - 1 ? b : ATTN_BINS - 1) * blockDim.x + threadIdx.x] += P * (dp - delta);
      }
    }
    store_row<DP>(drows + (int64_t)i * 3 * H, dq, d, z.scale);
    Ls[i] = L;
    Ds[i] = delta;
  }
  __syncthreads();
  if constexpr (BIAS) {                                  // row b over the threads, from thread b on (blockDim is 64 or 256: a power of two)
    for (int b = threadIdx.x; b < ATTN_BINS; b += blockDim.x) {
      float s = 0.f;
      for (int k = 0; k < (int)blockDim.x; ++k) s += bins[b * blockDim.x + ((k + b) & (blockDim.x - 1))];
      bz.partial[((int64_t)a * ATTN_BINS + b) * gridDim.x + blockIdx.x] = s;
    }
  }

  // ---- phase B: thread = key j; dV_j = sum_i Pd_ij dO_i, dK_j = sum_i P_ij (dPd_ij - delta_i) (scale * Q_i)
  stage_pair<DP>(T0, T1, rows, ld, grows, ldg, n, d, z.scale);
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    float k[DP], v[DP], dk[DP], dv[DP];
    load_row<DP>(k, rows + (int64_t)j * ld + H, d, 1.f);
    load_row<DP>(v, rows + (int64_t)j * ld + 2 * H, d, 1.f);
#pragma unroll
    for (int c = 0; c < DP; ++c) dk[c] = dv[c] = 0.f;
#pragma unroll UJ
    for (int i = 0; i < n; ++i) {
      const float P = expf(biased<BIAS>(dot<DP>(k, T0 + i * DP), Bs, sp, i * n + j) - Ls[i]);
      float dp = dot<DP>(v, T1 + i * DP);
      float pd = P;
      if (drop) {
        const bool keep = mask[mbase + (unsigned long long)i * n + j] != 0;
        dp = keep ? dp * z.inv_keep : 0.f;
        pd = keep ? P * z.inv_keep : 0.f;
      }
      axpy<DP>(dv, pd, T1 + i * DP);
      axpy<DP>(dk, P * (dp - Ds[i]), T0 + i * DP);
    }
    store_row<DP>(drows + (int64_t)j * 3 * H + H, dk, d, 1.f);
    store_row<DP>(drows + (int64_t)j * 3 * H + 2 * H, dv, d, 1.f);
  }
}

// d_table[b, a] = the sum over the graphs of partial[a][b][g]: one wave per value, lane l adds the graphs l, l + 64, ... in
// ascending order, thread 0 the 64 lanes' sums in ascending lane - a fixed order for a given G
__global__ __launch_bounds__(64) void attn_bias_reduce_kernel(const float* __restrict__ partial, int64_t G, int heads, float* __restrict__ d_table) {
  __shared__ float lanes[WAVE];
  const int a = blockIdx.x / ATTN_BINS, b = blockIdx.x % ATTN_BINS;
  const float* row = partial + ((int64_t)a * ATTN_BINS + b) * G;
  float s = 0.f;
  for (int64_t g = threadIdx.x; g < G; g += WAVE) s += row[g];
  lanes[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int l = 0; l < WAVE; ++l) t += lanes[l];
    d_table[b * heads + a] = t;
  }
}

// what the entry points check before anything is launched; cap = the LDS tiles' row count; limit: the entry point's own
static int attn_check(const char* who, int64_t ld_qkv, const void* graph_ptr, const void* pair_ptr, int64_t G, int64_t N,
                      int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p, int64_t limit, const char* limit_name,
                      int& cap) {
  ESC_REQUIRE(head_dim > 0 && head_dim <= 64 && head_dim % 4 == 0, "%s: head_dim %d must be a multiple of 4 and at most 64", who, head_dim);
  ESC_REQUIRE(heads > 0 && heads <= 65535, "%s: %d heads outside 1..65535", who, heads);
  ESC_REQUIRE(G >= 0 && N >= 0 && N < (1LL << 31) && G < (1LL << 31) && mask_pairs >= 0 && max_nodes >= 0,
              "%s: bad sizes G=%ld N=%ld mask_pairs=%ld max_nodes=%ld", who, (long)G, (long)N, (long)mask_pairs, (long)max_nodes);
  ESC_REQUIRE(max_nodes <= limit, "%s: a graph of %ld nodes exceeds the limit of %ld nodes per graph at head_dim %d (%s)", who,
              (long)max_nodes, (long)limit, head_dim, limit_name);
  ESC_REQUIRE(ld_qkv >= 3LL * heads * head_dim, "%s: leading dimension %ld below 3 * heads * head_dim = %ld", who, (long)ld_qkv,
              3L * heads * head_dim);
  ESC_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout rate %g outside [0, 1)", who, (double)p);
  ESC_REQUIRE(G == 0 || N == 0 || (graph_ptr && pair_ptr), "%s: null pointer", who);
  cap = (int)((max_nodes + 3) & ~3LL);
  return ESC_OK;
}

#define ESC_ATTN_DISPATCH(LAUNCH)                    \
  switch (attn_pad(head_dim)) {                      \
    case 4: LAUNCH(4); break;                        \
    case 8: LAUNCH(8); break;                        \
    case 16: LAUNCH(16); break;                      \
    case 32: LAUNCH(32); break;                      \
    default: LAUNCH(64); break;                      \
  }

// the two forward entry points: `bias` picks the instantiation, bz is read by the biased one alone
static int attn_fwd(const char* who, bool bias, int64_t limit, const char* limit_name, const float* qkv, int64_t ld_qkv,
                    const int32_t* graph_ptr, const int64_t* pair_ptr, const AttnBias& bz, int64_t G, int64_t N, int64_t mask_pairs,
                    int64_t max_nodes, int heads, int head_dim, float p, uint64_t seed, float* out, int64_t ld_out, float* lse,
                    uint8_t* mask, void* stream) {
  int cap = 0;
  const int rc = attn_check(who, ld_qkv, graph_ptr, pair_ptr, G, N, mask_pairs, max_nodes, heads, head_dim, p, limit, limit_name, cap);
  if (rc != ESC_OK) return rc;
  ESC_REQUIRE(ld_out >= (int64_t)heads * head_dim, "%s: leading dimension of out %ld below H = %d", who, (long)ld_out, heads * head_dim);
  ESC_REQUIRE(!bias || bz.spd_pairs >= 0, "%s: bad size spd_pairs=%ld", who, (long)bz.spd_pairs);
  if (G == 0 || N == 0 || max_nodes == 0) return ESC_OK;
  ESC_REQUIRE(qkv && out && lse && (p <= 0.f || mask) && (!bias || (bz.spd && bz.table)), "%s: null pointer", who);
  const AttnShape z{graph_ptr, pair_ptr, (int)N, cap, heads, head_dim, mask_pairs, (float)(1.0 / sqrt((double)head_dim)), p,
                    (float)(1.0 / (1.0 - (double)p))};
  const dim3 grid((unsigned)G, (unsigned)heads), block(max_nodes <= 64 ? 64 : 256);
#define ESC_ATTN_FWD_AS(DP, BIAS, LDS)                                                                                            \
  do {                                                                                                                            \
    const size_t lds = (LDS);                                                                                                     \
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)attn_fwd_kernel<DP, BIAS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    esc::launch(-1, attn_fwd_kernel<DP, BIAS>, grid, block, lds, (hipStream_t)stream, qkv, ld_qkv, z, (unsigned long long)seed, out, ld_out, lse, \
                (unsigned char*)mask, bz);                                                                                        \
  } while (0)
#define ESC_ATTN_FWD(DP)                                                                                                          \
  do {                                                                                                                            \
    if (bias) ESC_ATTN_FWD_AS(DP, true, ((size_t)2 * cap * DP + ATTN_TABLE_FLOATS) * sizeof(float));                              \
    else ESC_ATTN_FWD_AS(DP, false, (size_t)2 * cap * DP * sizeof(float));                                                        \
  } while (0)
  ESC_ATTN_DISPATCH(ESC_ATTN_FWD)
#undef ESC_ATTN_FWD
#undef ESC_ATTN_FWD_AS
  return ESC_OK;
}

// ... and the two backward entry points; the biased one's second launch (the sum of the partials) is its caller's
static int attn_bwd(const char* who, bool bias, int64_t limit, const char* limit_name, const float* qkv, int64_t ld_qkv, const float* d_out,
                    int64_t ld_dout, const float* lse, const uint8_t* mask, const int32_t* graph_ptr, const int64_t* pair_ptr,
                    const AttnBias& bz, int64_t G, int64_t N, int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p,
                    float* d_qkv, void* stream, bool& launched) {
  int cap = 0;
  launched = false;
  const int rc = attn_check(who, ld_qkv, graph_ptr, pair_ptr, G, N, mask_pairs, max_nodes, heads, head_dim, p, limit, limit_name, cap);
  if (rc != ESC_OK) return rc;
  ESC_REQUIRE(ld_dout >= (int64_t)heads * head_dim, "%s: leading dimension of d_out %ld below H = %d", who, (long)ld_dout, heads * head_dim);
  ESC_REQUIRE(!bias || bz.spd_pairs >= 0, "%s: bad size spd_pairs=%ld", who, (long)bz.spd_pairs);
  if (G == 0 || N == 0 || max_nodes == 0) return ESC_OK;
  ESC_REQUIRE(qkv && d_out && lse && d_qkv && (p <= 0.f || mask) && (!bias || (bz.spd && bz.table && bz.partial)), "%s: null pointer", who);
  const AttnShape z{graph_ptr, pair_ptr, (int)N, cap, heads, head_dim, mask_pairs, (float)(1.0 / sqrt((double)head_dim)), p,
                    (float)(1.0 / (1.0 - (double)p))};
  const dim3 grid((unsigned)G, (unsigned)heads), block(max_nodes <= 64 ? 64 : 256);
#define ESC_ATTN_BWD_AS(DP, BIAS, LDS)                                                                                            \
  do {                                                                                                                            \
    const size_t lds = (LDS);                                                                                                     \
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)attn_bwd_kernel<DP, BIAS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    esc::launch(-1, attn_bwd_kernel<DP, BIAS>, grid, block, lds, (hipStream_t)stream, qkv, ld_qkv, d_out, ld_dout, lse, (const unsigned char*)mask, z, \
                d_qkv, bz);                                                                                                       \
  } while (0)
#define ESC_ATTN_BWD(DP)                                                                                                          \
  do {                                                                                                                            \
    if (bias) ESC_ATTN_BWD_AS(DP, true, ((size_t)2 * cap * DP + 2 * cap + ATTN_TABLE_FLOATS + (size_t)ATTN_BINS * block.x) * sizeof(float)); \
    else ESC_ATTN_BWD_AS(DP, false, ((size_t)2 * cap * DP + 2 * cap) * sizeof(float));                                            \
  } while (0)
  ESC_ATTN_DISPATCH(ESC_ATTN_BWD)
#undef ESC_ATTN_BWD
#undef ESC_ATTN_BWD_AS
  launched = true;
  return ESC_OK;
}

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_graph_attention_max_nodes(int head_dim) {
  return head_dim > 0 && head_dim <= 64 && head_dim % 4 == 0 ? attn_limit(head_dim) : 0;
}

int esc_graph_attention_fwd(const float* qkv, int64_t ld_qkv, const int32_t* graph_ptr, const int64_t* pair_ptr, int64_t G,
                            int64_t N, int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p, uint64_t seed,
                            float* out, int64_t ld_out, float* lse, uint8_t* mask, void* stream) {
  const int rc = attn_fwd("esc_graph_attention_fwd", false, attn_limit(head_dim), "esc_graph_attention_max_nodes", qkv, ld_qkv, graph_ptr,
                          pair_ptr, AttnBias{nullptr, nullptr, nullptr, 0}, G, N, mask_pairs, max_nodes, heads, head_dim, p, seed, out, ld_out,
                          lse, mask, stream);
  if (rc != ESC_OK) return rc;
  ESC_CHECK_LAUNCH("esc_graph_attention_fwd");
  return ESC_OK;
}

int esc_graph_attention_bwd(const float* qkv, int64_t ld_qkv, const float* d_out, int64_t ld_dout, const float* lse,
                            const uint8_t* mask, const int32_t* graph_ptr, const int64_t* pair_ptr, int64_t G, int64_t N,
                            int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p, float* d_qkv, void* stream) {
  bool launched = false;
  const int rc = attn_bwd("esc_graph_attention_bwd", false, attn_limit(head_dim), "esc_graph_attention_max_nodes", qkv, ld_qkv, d_out, ld_dout,
                          lse, mask, graph_ptr, pair_ptr, AttnBias{nullptr, nullptr, nullptr, 0}, G, N, mask_pairs, max_nodes, heads, head_dim,
                          p, d_qkv, stream, launched);
  if (rc != ESC_OK) return rc;
  ESC_CHECK_LAUNCH("esc_graph_attention_bwd");
  return ESC_OK;
}

int64_t esc_graph_attention_bias_max_nodes(int head_dim) {
  return head_dim > 0 && head_dim <= 64 && head_dim % 4 == 0 ? attn_bias_limit(head_dim) : 0;
}

int64_t esc_graph_attention_bias_scratch_floats(int64_t G, int heads) {
  return G > 0 && heads > 0 ? (int64_t)ATTN_BINS * heads * G : 0;
}

int esc_graph_attention_bias_fwd(const float* qkv, int64_t ld_qkv, const int32_t* graph_ptr, const int64_t* pair_ptr,
                                 const uint8_t* spd, int64_t spd_pairs, const float* bias_table, int64_t G, int64_t N,
                                 int64_t mask_pairs, int64_t max_nodes, int heads, int head_dim, float p, uint64_t seed, float* out,
                                 int64_t ld_out, float* lse, uint8_t* mask, void* stream) {
  const int rc = attn_fwd("esc_graph_attention_bias_fwd", true, attn_bias_limit(head_dim), "esc_graph_attention_bias_max_nodes", qkv, ld_qkv,
                          graph_ptr, pair_ptr, AttnBias{(const unsigned char*)spd, bias_table, nullptr, spd_pairs}, G, N, mask_pairs,
                          max_nodes, heads, head_dim, p, seed, out, ld_out, lse, mask, stream);
  if (rc != ESC_OK) return rc;
  ESC_CHECK_LAUNCH("esc_graph_attention_bias_fwd");
  return ESC_OK;
}

int esc_graph_attention_bias_bwd(const float* qkv, int64_t ld_qkv, const float* d_out, int64_t ld_dout, const float* lse,
                                 const uint8_t* mask, const int32_t* graph_ptr, const int64_t* pair_ptr, const uint8_t* spd,
                                 int64_t spd_pairs, const float* bias_table, int64_t G, int64_t N, int64_t mask_pairs,
                                 int64_t max_nodes, int heads, int head_dim, float p, float* d_qkv, float* partial,
                                 int64_t partial_floats, float* d_table, void* stream) {
  const char* who = "esc_graph_attention_bias_bwd";
  bool launched = false;
  ESC_REQUIRE(d_table, "%s: null pointer", who);
  ESC_REQUIRE(G <= 0 || N <= 0 || max_nodes <= 0 || partial_floats >= esc_graph_attention_bias_scratch_floats(G, heads),
              "%s: scratch of %ld floats below the %ld of esc_graph_attention_bias_scratch_floats", who, (long)partial_floats,
              (long)esc_graph_attention_bias_scratch_floats(G, heads));
  const int rc = attn_bwd(who, true, attn_bias_limit(head_dim), "esc_graph_attention_bias_max_nodes", qkv, ld_qkv, d_out, ld_dout, lse, mask,
                          graph_ptr, pair_ptr, AttnBias{(const unsigned char*)spd, bias_table, partial, spd_pairs}, G, N, mask_pairs,
                          max_nodes, heads, head_dim, p, d_qkv, stream, launched);
  if (rc != ESC_OK) return rc;
  ESC_CHECK_LAUNCH(who);
  // nothing was launched (no graph, no node): the sum over no graphs, zeros
  esc::launch(-1, attn_bias_reduce_kernel, dim3((unsigned)(heads * ATTN_BINS)), dim3(WAVE), 0, (hipStream_t)stream, (const float*)partial,
              launched ? G : (int64_t)0, heads, d_table);
  ESC_CHECK_LAUNCH(who);
  return ESC_OK;
}

}  // extern "C"
