// layernorm.hip — the per-graph LayerNorm of the GPS layer (include/escgnn_layernorm.h): what PyG's
// norm.LayerNorm(dim_h) in graph mode does as a degree count, two scatter-adds, two gathers and the elementwise ops between
// them - one mean and one variance over ALL nodes and ALL channels of each graph - as ONE launch off graph_ptr, with the residual
// add in front of the norm folded in; its backward as one launch per graph plus the ordered sum of the affine's partials.
//
//   forward   h = x (+ r);  mean = sum h / M;  c = h - mean;  var = sum c*c / M;  rstd = 1 / sqrt(var + eps);  y = c rstd w + b
//   backward  gh = g w;  xhat = c rstd;  s1 = sum gh;  s2 = sum gh xhat;  d_x = rstd (gh - s1 / M - xhat s2 / M)
//             partial[graph] = (sum_i g xhat | sum_i g) per column;  d_weight | d_bias = the partials summed over the graphs
//
// Work split (layernorm_plan.h): one workgroup per graph, thread t = rl * Q + cl owns the float4 column lane cl of the rows rl,
// rl + R, ... of its graph.  Its first LN_CACHE rows stay in registers between the passes - every graph of the ZINC batch is
// read once - and the rest is read again from the L2 in batches of LN_BATCH rows with every read of a batch issued before its
// first use (a short tail reads the graph's last row again, masked).  There is no node limit and no staging in LDS.
// The variance is the centred second pass.  Every sum runs in an order fixed by (n, C): the thread's rows in ascending order,
// the xor butterfly of its wave, the waves in ascending order; the column partials: the row lanes in ascending order.  So y,
// stats and d_x of a graph have the same bits alone and inside any batch.  No atomics; every output element is written once.
// Built with -ffp-contract=off (Makefile).
#include "common.h"
#include "graph_wave.h"
#include "layernorm_plan.h"
#include "../../include/escgnn_layernorm.h"

namespace esc {

constexpr int LN_CACHE = 4;               // rows a thread keeps in registers: n <= 4 R covers 64 nodes at C = 64
constexpr int LN_BATCH = 4;               // rows of one round of reads beyond them

// what both directions read and write per row
struct LnArgs {
  const float* x; int64_t ld_x;
  const float* r; int64_t ld_r;           // the residual, or NULL
  const int* graph_ptr;
  int N, C;
  const float* weight;                    // the affine's scale, or NULL
  float* out; int64_t ld_out;             // forward: y;  backward: d_x
};

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float sum4(float4 a) { return (a.x + a.y) + (a.z + a.w); }

// the sum of v over the workgroup, in every thread: the wave's butterfly, then the T / 64 waves in ascending order
template <int T>
__device__ __forceinline__ float ln_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                                            // the previous sum has been read
  if (lane_id() == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < T / 64; ++w) s += red[w];
  return s;
}

// what a thread knows of its graph; ok: the range is ordered and inside [0, N]
struct LnCut {
  int b, n, Q, R, cl, first;              // first: the thread's first row, n for a thread that owns none
  bool ok;
};

template <int T>
__device__ __forceinline__ LnCut ln_cut(const int* __restrict__ graph_ptr, int N, int C) {
  LnCut k;
  const int b = graph_ptr[blockIdx.x], e = graph_ptr[blockIdx.x + 1];
  k.ok = b >= 0 && e >= b && e <= N;
  k.b = b;
  k.n = e - b;
  k.Q = C >> 2;
  k.R = T / k.Q;
  const int rl = threadIdx.x / k.Q;
  k.cl = threadIdx.x - rl * k.Q;
  k.first = rl < k.R ? rl : k.n;
  return k;
}

// body(row, value) for the thread's rows in ascending order: the cached ones, then the rest in batches.  load(row) reads row
// `row` < n of the graph at the thread's columns.
template <class V, class Load, class Body>
__device__ __forceinline__ void ln_rows(const LnCut& k, const V (&cache)[LN_CACHE], Load load, Body body) {
#pragma unroll
  for (int u = 0; u < LN_CACHE; ++u) {
    if (k.first + u * k.R < k.n) body(k.first + u * k.R, cache[u]);
  }
  for (int row = k.first + LN_CACHE * k.R; row < k.n; row += LN_BATCH * k.R) {
    V v[LN_BATCH];
#pragma unroll
    for (int u = 0; u < LN_BATCH; ++u) v[u] = load(min(row + u * k.R, k.n - 1));
#pragma unroll
    for (int u = 0; u < LN_BATCH; ++u) {
      if (row + u * k.R < k.n) body(row + u * k.R, v[u]);
    }
  }
}

// h = x (+ r) at the thread's columns of row `row` of the batch: ONE addition per element
__device__ __forceinline__ float4 ln_h(const LnArgs& a, size_t row, int c) {
  float4 h = ld4(a.x + row * a.ld_x + c);
  if (a.r) h = add4(h, ld4(a.r + row * a.ld_r + c));
  return h;
}

template <int T>
__global__ __launch_bounds__(T) void graph_ln_fwd_kernel(LnArgs a, const float* __restrict__ bias, float eps, float* __restrict__ all_stats) {
  __shared__ float red[T / 64];
  ESC_PRIO();
  const LnCut k = ln_cut<T>(a.graph_ptr, a.N, a.C);
  if (!k.ok) return;                                          // (uniform over the workgroup: it leaves together)
  float* stats = all_stats + 2 * (size_t)blockIdx.x;          // (mean, rstd) of this graph
  if (k.n == 0) {
    if (threadIdx.x == 0) { stats[0] = 0.f; stats[1] = 0.f; }
    return;
  }
  const int c = k.cl * 4;
  const float M = (float)((int64_t)k.n * a.C);
  auto load = [&](int row) { return ln_h(a, (size_t)(k.b + row), c); };
  float4 cache[LN_CACHE];
#pragma unroll
  for (int u = 0; u < LN_CACHE; ++u) cache[u] = load(min(k.first + u * k.R, k.n - 1));
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  ln_rows(k, cache, load, [&](int, float4 h) { acc = add4(acc, h); });
  const float mean = ln_block_sum<T>(sum4(acc), red) / M;
  acc = make_float4(0.f, 0.f, 0.f, 0.f);
  ln_rows(k, cache, load, [&](int, float4 h) {
    const float4 d = make_float4(h.x - mean, h.y - mean, h.z - mean, h.w - mean);
    acc = add4(acc, make_float4(d.x * d.x, d.y * d.y, d.z * d.z, d.w * d.w));
  });
  const float var = ln_block_sum<T>(sum4(acc), red) / M;
  const float rstd = 1.f / sqrtf(var + eps);
  if (threadIdx.x == 0) { stats[0] = mean; stats[1] = rstd; }
  const bool affine = a.weight != nullptr;
  const float4 w = affine ? ld4(a.weight + c) : make_float4(1.f, 1.f, 1.f, 1.f);
  const float4 b = affine ? ld4(bias + c) : make_float4(0.f, 0.f, 0.f, 0.f);
  ln_rows(k, cache, load, [&](int row, float4 h) {
    float4 y = make_float4((h.x - mean) * rstd, (h.y - mean) * rstd, (h.z - mean) * rstd, (h.w - mean) * rstd);
    if (affine) y = make_float4(y.x * w.x + b.x, y.y * w.y + b.y, y.z * w.z + b.z, y.w * w.w + b.w);
    st4(a.out + (size_t)(k.b + row) * a.ld_out + c, y);
  });
}

struct LnPair {
  float4 h, g;
};

template <int T>
__global__ __launch_bounds__(T) void graph_ln_bwd_kernel(LnArgs a, const float* __restrict__ stats, const float* __restrict__ g, int64_t ld_g,
                                                         float* __restrict__ partial) {
  __shared__ float red[T / 64];
  __shared__ float4 col_w[T], col_b[T];
  ESC_PRIO();
  const LnCut k = ln_cut<T>(a.graph_ptr, a.N, a.C);
  const int c = k.cl * 4;
  float* part = partial ? partial + (size_t)blockIdx.x * 2 * a.C + c : nullptr;      // [G, 2, C], or none without an affine
  if (!k.ok || k.n == 0) {                                    // skipped or empty: a zero partial, nothing else
    if (part && threadIdx.x < k.Q) {
      st4(part, make_float4(0.f, 0.f, 0.f, 0.f));
      st4(part + a.C, make_float4(0.f, 0.f, 0.f, 0.f));
    }
    return;
  }
  const float M = (float)((int64_t)k.n * a.C);
  const float mean = stats[2 * (size_t)blockIdx.x], rstd = stats[2 * (size_t)blockIdx.x + 1];
  const float4 w = a.weight ? ld4(a.weight + c) : make_float4(1.f, 1.f, 1.f, 1.f);
  auto load = [&](int row) {
    LnPair v;
    v.h = ln_h(a, (size_t)(k.b + row), c);
    v.g = ld4(g + (size_t)(k.b + row) * ld_g + c);
    return v;
  };
  auto xhat = [&](float4 h) { return make_float4((h.x - mean) * rstd, (h.y - mean) * rstd, (h.z - mean) * rstd, (h.w - mean) * rstd); };
  LnPair cache[LN_CACHE];
#pragma unroll
  for (int u = 0; u < LN_CACHE; ++u) cache[u] = load(min(k.first + u * k.R, k.n - 1));
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1, pw = s1, pb = s1;
  ln_rows(k, cache, load, [&](int, LnPair v) {
    const float4 xh = xhat(v.h);
    const float4 gh = make_float4(v.g.x * w.x, v.g.y * w.y, v.g.z * w.z, v.g.w * w.w);
    s1 = add4(s1, gh);
    s2 = add4(s2, make_float4(gh.x * xh.x, gh.y * xh.y, gh.z * xh.z, gh.w * xh.w));
    pw = add4(pw, make_float4(v.g.x * xh.x, v.g.y * xh.y, v.g.z * xh.z, v.g.w * xh.w));
    pb = add4(pb, v.g);
  });
  const float k1 = ln_block_sum<T>(sum4(s1), red) / M;
  const float k2 = ln_block_sum<T>(sum4(s2), red) / M;
  if (part) {                                                 // the column sums: the row lanes in ascending order
    col_w[threadIdx.x] = pw;
    col_b[threadIdx.x] = pb;
    __syncthreads();
    if (threadIdx.x < k.Q) {
      const int lanes = min(k.R, k.n);                        // a row lane beyond the graph's rows holds zeros
      float4 tw = col_w[k.cl], tb = col_b[k.cl];
      for (int rl = 1; rl < lanes; ++rl) {
        tw = add4(tw, col_w[rl * k.Q + k.cl]);
        tb = add4(tb, col_b[rl * k.Q + k.cl]);
      }
      st4(part, tw);
      st4(part + a.C, tb);
    }
  }
  ln_rows(k, cache, load, [&](int row, LnPair v) {
    const float4 xh = xhat(v.h);
    float4 d;
    d.x = rstd * ((v.g.x * w.x - k1) - xh.x * k2); d.y = rstd * ((v.g.y * w.y - k1) - xh.y * k2);
    d.z = rstd * ((v.g.z * w.z - k1) - xh.z * k2); d.w = rstd * ((v.g.w * w.w - k1) - xh.w * k2);
    st4(a.out + (size_t)(k.b + row) * a.ld_out + c, d);
  });
}

// d_weight | d_bias [c .. c + 3] = the sum over the graphs of partial[g][0 | 1][c .. c + 3]: one wave per float4, lane l adds the
// graphs l, l + CHAINS, ... in ascending order, thread 0 the lanes' sums in ascending lane - a fixed order for a given G
__global__ __launch_bounds__(layernorm::CHAINS) void graph_ln_reduce_kernel(const float* __restrict__ partial, int G, int C,
                                                                           float* __restrict__ d_weight, float* __restrict__ d_bias) {
  __shared__ float4 lanes[layernorm::CHAINS];
  const int Q = C >> 2, which = blockIdx.x / Q, c = (blockIdx.x - which * Q) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int g = threadIdx.x; g < G; g += layernorm::CHAINS) s = add4(s, ld4(partial + ((size_t)g * 2 + which) * C + c));
  lanes[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < min(layernorm::CHAINS, G); ++l) t = add4(t, lanes[l]);
    st4((which ? d_bias : d_weight) + c, t);
  }
}

// what both entries check before anything is launched; 0 or an error code with the message set
template <int NL, int NP>
static int ln_limits(const char* fn, int64_t G, int64_t N, int64_t C, const RowLd (&ld)[NL], const void* const (&p)[NP]) {
  if (const int rc = group_limits(fn, "esc_graph_layer_norm_max_channels", layernorm::MAX_C, N, 0, C, ld, p)) return rc;
  ESC_REQUIRE(G >= 0 && G < (1LL << 31) - 1, "%s: bad sizes G=%ld N=%ld", fn, (long)G, (long)N);
  return ESC_OK;
}

#define ESC_LN_KERNEL(kernel, block) ((block) == 256 ? kernel<256> : (block) == 512 ? kernel<512> : kernel<1024>)

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_graph_layer_norm_max_channels(void) { return layernorm::MAX_C; }

int esc_graph_layer_norm_fwd(const float* x, int64_t ld_x, const float* r, int64_t ld_r, const int32_t* graph_ptr, int64_t G, int64_t N,
                             int64_t C, const float* weight, const float* bias, float eps, float* y, int64_t ld_y, float* stats,
                             void* stream) {
  const char* fn = "esc_graph_layer_norm_fwd";
  const RowLd ld[] = {{"ld_x", ld_x}, {"ld_r", r ? ld_r : C}, {"ld_y", ld_y}};
  const void* const ptrs[] = {x, r, weight, bias, y};
  if (const int rc = ln_limits(fn, G, N, C, ld, ptrs)) return rc;
  ESC_REQUIRE((weight == nullptr) == (bias == nullptr), "%s: weight and bias come together (both or neither)", fn);
  if (G == 0 || N == 0) return ESC_OK;
  ESC_REQUIRE(x && graph_ptr && y && stats, "%s: null pointer", fn);
  const layernorm::Plan p = layernorm::plan_layer_norm(G, C, false, weight != nullptr);
  const LnArgs a{x, ld_x, r, ld_r, graph_ptr, (int)N, (int)C, weight, y, ld_y};
  esc::launch(-1, ESC_LN_KERNEL(graph_ln_fwd_kernel, p.block), dim3(p.grid[0]), dim3(p.block), 0, (hipStream_t)stream, a, bias, eps, stats);
  ESC_CHECK_LAUNCH(fn);
  return ESC_OK;
}

int esc_graph_layer_norm_bwd(const float* x, int64_t ld_x, const float* r, int64_t ld_r, const float* stats, const float* g, int64_t ld_g,
                             const int32_t* graph_ptr, int64_t G, int64_t N, int64_t C, const float* weight, float* d_x, int64_t ld_dx,
                             float* d_weight, float* d_bias, float* partial, void* stream) {
  const char* fn = "esc_graph_layer_norm_bwd";
  const RowLd ld[] = {{"ld_x", ld_x}, {"ld_r", r ? ld_r : C}, {"ld_g", ld_g}, {"ld_dx", ld_dx}};
  const void* const ptrs[] = {x, r, g, weight, d_x, d_weight, d_bias, partial};
  if (const int rc = ln_limits(fn, G, N, C, ld, ptrs)) return rc;
  const bool affine = weight != nullptr;
  ESC_REQUIRE(affine == (d_weight != nullptr) && affine == (d_bias != nullptr) && (affine == (partial != nullptr) || G == 0 || N == 0),
              "%s: weight, d_weight, d_bias and partial come together (all or none)", fn);
  const bool rows = G > 0 && N > 0;
  ESC_REQUIRE(!rows || (x && stats && g && graph_ptr && d_x), "%s: null pointer", fn);
  const layernorm::Plan p = layernorm::plan_layer_norm(G, C, true, affine);
  hipStream_t s = (hipStream_t)stream;
  if (rows) {
    const LnArgs a{x, ld_x, r, ld_r, graph_ptr, (int)N, (int)C, weight, d_x, ld_dx};
    esc::launch(-1, ESC_LN_KERNEL(graph_ln_bwd_kernel, p.block), dim3(p.grid[0]), dim3(p.block), 0, s, a, stats, g, ld_g, partial);
  }
  if (affine)                                                 // without rows no partial was written: the sum over zero graphs
    esc::launch(-1, graph_ln_reduce_kernel, dim3(p.grid[1]), dim3(layernorm::CHAINS), 0, s, (const float*)partial, rows ? (int)G : 0, (int)C,
                d_weight, d_bias);
  ESC_CHECK_LAUNCH(fn);
  return ESC_OK;
}

}  // extern "C"
