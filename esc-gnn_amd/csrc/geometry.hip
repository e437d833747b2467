// geometry.hip — the geometric pieces of the QM9 run: the `Distance` transform over many graphs, the dense node input
// cat([x, pos], 1) + node_type_embedding(node_type), and the MSE training loss.
//
// Restates the reference's distance.py:25-47 (edge length from `pos`, divided by the graph's own maximum, appended to the
// bond one-hot; run_qm9.py:226-231 applies it to every graph on every access, on the CPU), qm9_models.py:106-107 and
// run_qm9.py:348 (F.mse_loss).  Built with -ffp-contract=off: every product and sum below rounds on its own.
#include "common.h"

namespace esc {

// max that lets a NaN through (torch.max does): distances are >= 0 otherwise
__device__ __forceinline__ float nan_max(float m, float d) { return (d > m || d != d) ? d : m; }

__device__ __forceinline__ float edge_length(const float* __restrict__ pos, int64_t ld, int64_t a, int64_t b, int squared,
                                             float& rx, float& ry, float& rz) {
  rx = pos[b * ld] - pos[a * ld];
  ry = pos[b * ld + 1] - pos[a * ld + 1];
  rz = pos[b * ld + 2] - pos[a * ld + 2];
  const float s = (rx * rx + ry * ry) + rz * rz;
  return squared ? s : sqrtf(s);
}

// One workgroup per graph.  Pass 1 checks every node id and reduces the graph's maximum (wave shuffles, then LDS): nothing
// is written before the whole graph is known to be valid.  Pass 2 recomputes each length (same expression, same bits) and
// writes it divided by the maximum.  No atomics: a result depends on its own graph only, never on the grid.
__global__ __launch_bounds__(256) void edge_distance_kernel(const float* __restrict__ pos, int64_t ld_pos,
                                                            const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                            const int64_t* __restrict__ node_ptr,
                                                            const int64_t* __restrict__ edge_ptr, int64_t total_nodes,
                                                            int64_t total_edges, int norm, int squared, int relative_pos,
                                                            int use_max_value, float max_value, float* __restrict__ out,
                                                            int64_t ld_out, int64_t col, int32_t* __restrict__ status) {
  __shared__ float wmax[4];
  __shared__ int bad;
  const int g = blockIdx.x, tid = threadIdx.x;
  const int64_t n0 = node_ptr[g], n1 = node_ptr[g + 1];
  const int64_t e0 = edge_ptr[g], e1 = edge_ptr[g + 1];
  const int64_t n = n1 - n0;
  if (n0 < 0 || n < 0 || n1 > total_nodes || e0 < 0 || e1 < e0 || e1 > total_edges) {   // uniform
    if (tid == 0) status[g] = ESC_EINVAL;
    return;
  }
  if (tid == 0) { status[g] = ESC_OK; bad = 0; }
  if (e1 == e0) return;                                  // a graph without edges: nothing to write (distance.py:36)
  __syncthreads();
  const float* gpos = pos + n0 * ld_pos;
  float m = -INFINITY;
  for (int64_t e = e0 + tid; e < e1; e += 256) {
    const int64_t a = src[e], b = dst[e];
    if (a < 0 || b < 0 || a >= n || b >= n) { bad = 1; continue; }
    float rx, ry, rz;
    m = nan_max(m, edge_length(gpos, ld_pos, a, b, squared, rx, ry, rz));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_xor(m, o, 64));
  if ((tid & 63) == 0) wmax[tid >> 6] = m;
  __syncthreads();
  if (bad) {                                             // uniform: the whole workgroup leaves, nothing is written
    if (tid == 0) status[g] = ESC_EINVAL;
    return;
  }
  m = nan_max(nan_max(wmax[0], wmax[1]), nan_max(wmax[2], wmax[3]));
  const float div = use_max_value ? max_value : m;
  for (int64_t e = e0 + tid; e < e1; e += 256) {
    float rx, ry, rz;
    float d = edge_length(gpos, ld_pos, src[e], dst[e], squared, rx, ry, rz);
    if (norm) d = d / div;                               // 0 / 0 = NaN for a graph of self loops, as the reference gives
    float* o = out + e * ld_out + col;
    o[0] = d;
    if (relative_pos) { o[1] = rx; o[2] = ry; o[3] = rz; }
  }
}

// out[i, :F] = x[i, :] + table[t_i, :F];  out[i, F:F+3] = pos[i, :] + table[t_i, F:F+3]   (one add per element; a type
// outside the table contributes a zero row and raises *bad)
__global__ __launch_bounds__(256) void node_input_fwd_kernel(const float* __restrict__ x, int64_t ld_x, const float* __restrict__ pos,
                                                             int64_t ld_pos, const int64_t* __restrict__ node_type,
                                                             const float* __restrict__ table, int64_t rows, int F, int64_t N,
                                                             float* __restrict__ out, int64_t ld_out, int* __restrict__ bad) {
  const int W = F + 3;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * W) return;
  const int64_t i = t / W;
  const int c = (int)(t % W);
  const int64_t r = node_type[i];
  const float v = c < F ? x[i * ld_x + c] : pos[i * ld_pos + (c - F)];
  float w = 0.f;
  if (r >= 0 && r < rows) w = table[r * W + c];
  else if (bad) *bad = 1;
  out[i * ld_out + c] = v + w;
}

// single workgroup (M is the graph count of a batch); differences, squares and the sum in fp64, fixed order, one rounding
__global__ __launch_bounds__(1024) void mse_loss_kernel(const float* __restrict__ pred, const float* __restrict__ y, int64_t M,
                                                        double denom, float grad_scale, float* __restrict__ loss,
                                                        float* __restrict__ dpred) {
  ESC_PRIO();
  __shared__ double sh[16];
  double acc = 0.0;
  const double gs = 2.0 * (double)grad_scale / denom;
  for (int64_t i = threadIdx.x; i < M; i += blockDim.x) {
    const double d = (double)pred[i] - (double)y[i];
    acc += d * d;
    if (dpred) dpred[i] = (float)(d * gs);
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += sh[w];
    loss[0] = (float)(t / denom);
  }
}

}  // namespace esc

using namespace esc;

extern "C" {

int esc_edge_distance(const float* pos, int64_t ld_pos, const int64_t* src, const int64_t* dst, const int64_t* node_ptr,
                      const int64_t* edge_ptr, int64_t G, int64_t total_nodes, int64_t total_edges, int norm, int squared,
                      int relative_pos, int use_max_value, float max_value, float* out, int64_t ld_out, int64_t col,
                      int32_t* status, void* stream) {
  ESC_REQUIRE(G >= 0 && total_nodes >= 0 && total_edges >= 0, "esc_edge_distance: negative size");
  if (G == 0) return ESC_OK;
  ESC_REQUIRE(node_ptr && edge_ptr && status, "esc_edge_distance: null graph arrays");
  ESC_REQUIRE((src && dst && out) || total_edges == 0, "esc_edge_distance: null edge arrays");
  ESC_REQUIRE(pos || total_nodes == 0, "esc_edge_distance: null pos");
  ESC_REQUIRE(ld_pos >= 3, "esc_edge_distance: pos rows hold 3 coordinates (ld_pos=%ld)", (long)ld_pos);
  ESC_REQUIRE(col >= 0 && ld_out >= col + (relative_pos ? 4 : 1), "esc_edge_distance: columns %ld.. do not fit rows of %ld",
              (long)col, (long)ld_out);
  ESC_REQUIRE(G < (1LL << 31), "esc_edge_distance: too many graphs in one call");
  esc::launch(ESC_K_FEATURES, edge_distance_kernel, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, pos, ld_pos, src, dst,
              node_ptr, edge_ptr, total_nodes, total_edges, norm, squared, relative_pos, use_max_value, max_value, out, ld_out,
              col, status);
  ESC_CHECK_LAUNCH("esc_edge_distance");
  return ESC_OK;
}

int esc_node_input_fwd(const float* x, int64_t ld_x, const float* pos, int64_t ld_pos, const int64_t* node_type,
                       const float* table, int64_t rows, int64_t F, int64_t N, float* out, int64_t ld_out, int32_t* bad_flag,
                       void* stream) {
  ESC_REQUIRE(N >= 0 && rows > 0 && F >= 1 && F < (1 << 20), "esc_node_input_fwd: bad shape rows=%ld F=%ld N=%ld", (long)rows,
              (long)F, (long)N);
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(x && pos && node_type && table && out, "esc_node_input_fwd: null pointer");
  ESC_REQUIRE(ld_x >= F && ld_pos >= 3 && ld_out >= F + 3, "esc_node_input_fwd: leading dimensions %ld / %ld / %ld too small",
              (long)ld_x, (long)ld_pos, (long)ld_out);
  ESC_REQUIRE(cdiv(N * (F + 3), 256) < (1LL << 31), "esc_node_input_fwd: too many rows in one call");
  esc::launch(ESC_K_BAG_FWD, node_input_fwd_kernel, dim3((unsigned)cdiv(N * (F + 3), 256)), dim3(256), 0, (hipStream_t)stream, x,
              ld_x, pos, ld_pos, node_type, table, rows, (int)F, N, out, ld_out, (int*)bad_flag);
  ESC_CHECK_LAUNCH("esc_node_input_fwd");
  return ESC_OK;
}

// x and pos are data: the only gradient is the table's, the small-table segmented sum of embed.hip (one workgroup per row)
int esc_node_input_bwd(const float* g, int64_t ld_g, const int64_t* node_type, int64_t N, int64_t rows, int64_t F,
                       float* dtable, void* stream) {
  ESC_REQUIRE(F >= 1, "esc_node_input_bwd: F=%ld", (long)F);
  return esc_embed_bwd(g, ld_g, node_type, N, rows, F + 3, dtable, stream);
}

int esc_mse_loss(const float* pred, const float* y, int64_t M, int64_t denom, float grad_scale, float* loss, float* dpred,
                 void* stream) {
  ESC_REQUIRE(pred && y && loss, "esc_mse_loss: null pointer");
  ESC_REQUIRE(M > 0 && denom > 0, "esc_mse_loss: empty batch");
  esc::launch(-1, mse_loss_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, pred, y, M, (double)denom, grad_scale, loss, dpred);
  ESC_CHECK_LAUNCH("esc_mse_loss");
  return ESC_OK;
}

}  // extern "C"
