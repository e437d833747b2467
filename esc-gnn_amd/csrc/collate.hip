// collate.hip — device-side Batch.from_data_list: gather B graphs out of the HBM-resident dataset store and emit
// (i) the reference's batch tensors, bit-identical to the reference's batch.py:25-149 (edge_index += running node count,
// pos_batch += running edge count :70-71, pos_enc/pos_index unshifted :72-73, batch = graph id :120-123), and (ii) the
// compact int32 execution plan (CSR by destination / source, bag rows, bag columns) by offsetting per-graph views that
// were sorted once when the store was built.  Two launches per batch: the per-column counts, then ONE fill.
//
// What the fill is built around (DESIGN.md §4 *Collate*): the pass moves ~45 MB, so its byte floor is ~10 us, and what it
// cost before was latency — pointer-to-pointer prologues and a three-deep dependent chain per bag entry.  Here
//   * a workgroup's first loads are DATA: the graph's ranges and running offsets come from the staged block the host built,
//   * every store view is int32, graph-local and already in the order it is written in (one load + one add per output),
//   * the (graph, column)-sorted bag view resolves its destination from LDS: each bag workgroup scans the column totals
//     itself (no scan launch) and adds its graph's prefix row, so an entry is load -> LDS -> store,
//   * the node, edge and bag sections of a graph are different workgroups (grid.y), all resident at once.
#include "common.h"

namespace esc {

// per-column running counts over the batch's graphs: prefix[b][c] = #entries of column c in graphs
// 0..b-1 of the batch, total[c] = over all graphs.  One wave per column: lanes take 64 graphs at a
// time and a wave prefix scan replaces the serial dependent-load chain.
__global__ __launch_bounds__(256) void collate_col_count_kernel(const int* __restrict__ col_cnt_all, int n_cols,
                                                                const int64_t* __restrict__ graph_ids, int B,
                                                                int* __restrict__ prefix, int* __restrict__ total) {
  const int c = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (c >= n_cols) return;
  const int lane = lane_id();
  int run = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + lane;
    const int v = (b < B) ? col_cnt_all[(size_t)graph_ids[b] * n_cols + c] : 0;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (b < B) prefix[(size_t)b * n_cols + c] = run + incl - v;
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) total[c] = run;
}

// two consecutive entries of a row-order store array: the int32 copy (one 8-byte load when `wide8`), or the int64 source
// where a value of the array does not fit int32
__device__ __forceinline__ void load2(const int32_t* __restrict__ p32, const int64_t* __restrict__ p64, int64_t s, bool wide8,
                                      int64_t& v0, int64_t& v1) {
  if (p32) {
    if (wide8) {
      const int2 t = *reinterpret_cast<const int2*>(p32 + s);
      v0 = t.x; v1 = t.y;
    } else {
      v0 = p32[s]; v1 = p32[s + 1];
    }
  } else {
    v0 = p64[s]; v1 = p64[s + 1];
  }
}
__device__ __forceinline__ int64_t load1(const int32_t* __restrict__ p32, const int64_t* __restrict__ p64, int64_t s) {
  return p32 ? (int64_t)p32[s] : p64[s];
}
// int32 plan value = low 32 bits of (graph-local value + running offset), as the (int) conversion of the int64 sum gives
__device__ __forceinline__ int add32(int v, int64_t off) { return (int)((unsigned)v + (unsigned)off); }
__device__ __forceinline__ bool al(const void* p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

constexpr int FILL_T = 256;

// grid (B, bag_parts + 2): blockIdx.y < bag_parts: a slice of the graph's bag entries (row view and column view);
// == bag_parts: its edges (+ attribute rows); == bag_parts + 1: its nodes, features, targets and the closing pointers
__global__ __launch_bounds__(FILL_T) void collate_fill_kernel(esc_collate_args a, int bag_parts) {
  extern __shared__ int s_col[];                         // [n_cols] column base of this graph (bag workgroups)
  __shared__ int s_wsum[FILL_T / WAVE];
  const int b = blockIdx.x, role = blockIdx.y, tid = threadIdx.x;
  const int64_t B = a.B;
  const int64_t* __restrict__ start = a.stage + B;
  const int64_t* __restrict__ count = a.stage + 5 * B;
  const int64_t* __restrict__ offs = a.stage + 9 * B;
  // the graph's header: twelve independent (scalar) loads
  const int64_t n0 = start[b], e0 = start[B + b], z0 = start[2 * B + b], y0 = start[3 * B + b];
  const int64_t n_g = count[b], e_g = count[B + b], z_g = count[2 * B + b], y_g = count[3 * B + b];
  const int64_t no = offs[b], eo = offs[(B + 1) + b], zo = offs[2 * (B + 1) + b], yo = offs[3 * (B + 1) + b];

  if (role == bag_parts + 1) {                           // ---- nodes ----
    for (int64_t i = tid; i < n_g; i += FILL_T) {
      a.batch[no + i] = b;
      a.in_ptr[no + i] = add32(a.in_ptr32[n0 + i], eo);
      a.out_ptr[no + i] = add32(a.out_ptr32[n0 + i], eo);
    }
    if (a.x_long) {                                      // categorical features: exact in fp32, handed out as int64
      for (int64_t i = tid; i < n_g * a.x_dim; i += FILL_T) a.x_long[no * a.x_dim + i] = (int64_t)a.x_all[n0 * a.x_dim + i];
    } else {
      for (int64_t i = tid; i < n_g * a.x_dim; i += FILL_T) a.x[no * a.x_dim + i] = a.x_all[n0 * a.x_dim + i];
    }
    for (int64_t i = tid; i < y_g * a.y_dim; i += FILL_T) a.y[yo * a.y_dim + i] = a.y_all[y0 * a.y_dim + i];
    if (tid == 0) {
      if (a.graph_ptr) {
        a.graph_ptr[b] = (int)no;
        if (b == B - 1) a.graph_ptr[B] = (int)a.N;
      }
      if (b == B - 1) { a.in_ptr[a.N] = (int)a.E; a.out_ptr[a.N] = (int)a.E; a.row_ptr[a.E] = (int)a.Z; }
    }
    return;
  }
  if (role == bag_parts) {                               // ---- edges ----
    for (int64_t k = tid; k < e_g; k += FILL_T) {
      const int64_t s = e0 + k, d = eo + k;
      const int64_t src = load1(a.esrc32, a.esrc_all, s), dst = load1(a.edst32, a.edst_all, s);
      const int ie = a.in_edge32[s], is = a.in_src32[s], oe = a.out_edge32[s], od = a.out_dst32[s], rp = a.row_ptr32[s];
      a.edge_index[d] = src + no;
      a.edge_index[a.E + d] = dst + no;
      a.in_edge[d] = add32(ie, eo);
      a.in_src[d] = add32(is, no);
      a.out_edge[d] = add32(oe, eo);
      a.out_dst[d] = add32(od, no);
      a.row_ptr[d] = add32(rp, zo);
    }
    if (a.edge_attr) {                                   // attribute rows travel with their edges
      const int64_t words = e_g * a.ea_words;
      const uint32_t* __restrict__ src = static_cast<const uint32_t*>(a.edge_attr_all) + e0 * a.ea_words;
      uint32_t* __restrict__ dst = static_cast<uint32_t*>(a.edge_attr) + eo * a.ea_words;
      if (((words & 3) == 0) && al(src, 15) && al(dst, 15)) {
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);
        uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
        for (int64_t i = tid; i < (words >> 2); i += FILL_T) d4[i] = s4[i];
      } else {
        for (int64_t i = tid; i < words; i += FILL_T) dst[i] = src[i];
      }
    }
    return;
  }

  // ---- bag entries ----
  // column base of this graph, in LDS: exclusive scan of the batch's column totals (= col_ptr) + the graph's prefix row
  const int n = (int)a.n_cols;
  for (int i = tid; i < n; i += FILL_T) s_col[i] = a.col_total[i];
  __syncthreads();
  {
    const int per = (n + FILL_T - 1) / FILL_T;
    const int beg = min(tid * per, n), end = min(beg + per, n);
    int sum = 0;
    for (int i = beg; i < end; ++i) sum += s_col[i];
    const int lane = lane_id(), w = tid >> 6;
    int incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) s_wsum[w] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int k = 0; k < w; ++k) run += s_wsum[k];
    for (int i = beg; i < end; ++i) {
      const int v = s_col[i];
      s_col[i] = run;
      run += v;
    }
    if (b == 0 && role == 0 && tid == FILL_T - 1) a.col_ptr[n] = run;      // the last thread's running sum is the total
  }
  __syncthreads();
  if (b == 0 && role == 0) {                             // one workgroup leaves col_ptr for the plan
    for (int i = tid; i < n; i += FILL_T) a.col_ptr[i] = s_col[i];
  }
  {
    const int* __restrict__ prow = a.col_prefix + (size_t)b * n;
    for (int i = tid; i < n; i += FILL_T) s_col[i] += prow[i];
  }
  __syncthreads();
  if (z_g <= 0) return;

  const int64_t gt = (int64_t)role * FILL_T + tid, nth = (int64_t)bag_parts * FILL_T;

  // column (CSC) view: entry j of the graph in (column, edge) order -> its slot of the batch's column
  {
    const int32_t* __restrict__ ccol = a.c_col32 + z0;
    const int32_t* __restrict__ crow = a.c_row32 + z0;
    const int32_t* __restrict__ cval = a.c_val32 + z0;
    const int32_t* __restrict__ crank = a.c_rank_all + z0;
    for (int64_t j0 = gt; j0 < z_g; j0 += 4 * nth) {
      int cc[4], r[4], v[4], rk[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {                      // all loads of the four entries first (clamped: stores are guarded)
        const int64_t j = min(j0 + u * nth, z_g - 1);
        cc[u] = ccol[j]; r[u] = crow[j]; v[u] = cval[j]; rk[u] = crank[j];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (j0 + u * nth < z_g) {
          const int dest = s_col[cc[u]] + rk[u];
          a.col_row[dest] = add32(r[u], eo);
          a.col_val[dest] = v[u];
          a.col_col[dest] = cc[u];
        }
      }
    }
  }

  // row view: the reference's three int64 tensors and the int32 (index, value) pairs, two entries per thread so that the
  // int64 outputs leave as 16-byte stores.  Pairs are aligned on the DESTINATION (zo + j even); an odd first / last entry
  // is written on its own.
  auto one = [&](int64_t j) {
    const int64_t s = z0 + j, d = zo + j;
    const int64_t v = load1(a.pos_enc32, a.pos_enc_all, s), c = load1(a.pos_index32, a.pos_index_all, s);
    const int64_t r = load1(a.pos_batch32, a.pos_batch_all, s);
    a.pos_enc[d] = v; a.pos_index[d] = c; a.pos_batch[d] = r + eo;
    a.bag_idx[d] = (int)c; a.bag_val[d] = (int)v;
  };
  const int64_t head = (zo & 1) ? 1 : 0;
  const int64_t pairs = (z_g - head) >> 1;
  if (gt == 0 && head) one(0);
  if (gt == nth - 1 && ((z_g - head) & 1)) one(z_g - 1);
  const bool src8 = (((z0 + head) & 1) == 0) && al(a.pos_enc32, 7) && al(a.pos_index32, 7) && al(a.pos_batch32, 7);
  const bool out16 = al(a.pos_enc, 15) && al(a.pos_index, 15) && al(a.pos_batch, 15);
  const bool out8 = al(a.bag_idx, 7) && al(a.bag_val, 7);
  for (int64_t p0 = gt; p0 < pairs; p0 += 2 * nth) {
    int64_t v[4], c[4], r[4];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t s = z0 + head + 2 * min(p0 + u * nth, pairs - 1);
      load2(a.pos_enc32, a.pos_enc_all, s, src8, v[2 * u], v[2 * u + 1]);
      load2(a.pos_index32, a.pos_index_all, s, src8, c[2 * u], c[2 * u + 1]);
      load2(a.pos_batch32, a.pos_batch_all, s, src8, r[2 * u], r[2 * u + 1]);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (p0 + u * nth >= pairs) continue;
      const int64_t d = zo + head + 2 * (p0 + u * nth);
      const int64_t v0 = v[2 * u], v1 = v[2 * u + 1], c0 = c[2 * u], c1 = c[2 * u + 1];
      const int64_t r0 = r[2 * u] + eo, r1 = r[2 * u + 1] + eo;
      if (out16) {
        *reinterpret_cast<longlong2*>(a.pos_enc + d) = make_longlong2(v0, v1);
        *reinterpret_cast<longlong2*>(a.pos_index + d) = make_longlong2(c0, c1);
        *reinterpret_cast<longlong2*>(a.pos_batch + d) = make_longlong2(r0, r1);
      } else {
        a.pos_enc[d] = v0; a.pos_enc[d + 1] = v1;
        a.pos_index[d] = c0; a.pos_index[d + 1] = c1;
        a.pos_batch[d] = r0; a.pos_batch[d + 1] = r1;
      }
      if (out8) {
        *reinterpret_cast<int2*>(a.bag_idx + d) = make_int2((int)c0, (int)c1);
        *reinterpret_cast<int2*>(a.bag_val + d) = make_int2((int)v0, (int)v1);
      } else {
        a.bag_idx[d] = (int)c0; a.bag_idx[d + 1] = (int)c1;
        a.bag_val[d] = (int)v0; a.bag_val[d + 1] = (int)v1;
      }
    }
  }
}

}  // namespace esc

using namespace esc;

extern "C" {

int esc_collate_cols(const int32_t* col_cnt_all, int64_t n_cols, const int64_t* graph_ids, int64_t B,
                     int32_t* col_prefix, int32_t* col_total, void* stream) {
  ESC_REQUIRE(col_cnt_all && graph_ids && col_prefix && col_total, "esc_collate_cols: null pointer");
  ESC_REQUIRE(n_cols > 0 && B > 0 && B < (1 << 24), "esc_collate_cols: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  esc::launch(ESC_K_COLLATE, collate_col_count_kernel, dim3((unsigned)cdiv(n_cols, 4)), dim3(256), 0, s, col_cnt_all, (int)n_cols, graph_ids, (int)B, col_prefix, col_total);
  ESC_CHECK_LAUNCH("esc_collate_cols");
  return ESC_OK;
}

int esc_collate_fill(const esc_collate_args* args, void* stream) {
  ESC_REQUIRE(args, "esc_collate_fill: null args");
  const esc_collate_args& a = *args;
  ESC_REQUIRE(a.B > 0 && a.B < (1LL << 31) && a.x_dim >= 0 && a.y_dim >= 0, "esc_collate_fill: bad sizes");
  ESC_REQUIRE(a.n_cols > 0 && a.n_cols <= 12288, "esc_collate_fill: n_cols must be in 1..12288 (the column bases live in LDS)");
  ESC_REQUIRE(a.N >= 0 && a.E >= 0 && a.Z >= 0 && a.Z < (1LL << 31), "esc_collate_fill: bad totals");
  ESC_REQUIRE(a.stage && a.esrc_all && a.edst_all && a.pos_enc_all && a.pos_index_all && a.pos_batch_all, "esc_collate_fill: null index arrays");
  ESC_REQUIRE(a.in_ptr32 && a.out_ptr32 && a.in_edge32 && a.in_src32 && a.out_edge32 && a.out_dst32 && a.row_ptr32, "esc_collate_fill: null edge views");
  ESC_REQUIRE(a.c_col32 && a.c_row32 && a.c_val32 && a.c_rank_all && a.col_total && a.col_prefix, "esc_collate_fill: null column views");
  ESC_REQUIRE(a.batch && a.edge_index && a.pos_enc && a.pos_index && a.pos_batch, "esc_collate_fill: null outputs");
  ESC_REQUIRE(a.in_ptr && a.in_edge && a.in_src && a.out_ptr && a.out_edge && a.out_dst && a.row_ptr && a.bag_idx && a.bag_val &&
              a.col_ptr && a.col_row && a.col_val && a.col_col, "esc_collate_fill: null plan outputs");
  ESC_REQUIRE((a.x || a.x_long || a.x_dim == 0) && (a.y || a.y_dim == 0) && (!a.edge_attr || (a.edge_attr_all && a.ea_words > 0)),
              "esc_collate_fill: bad optional outputs");
  // about four bag entries per thread; every workgroup pays one LDS scan of the column totals, so no more slices than that
  int64_t parts = cdiv(a.Z, a.B * 4 * FILL_T);
  parts = parts < 1 ? 1 : (parts > 64 ? 64 : parts);
  hipStream_t s = (hipStream_t)stream;
  esc::launch(ESC_K_COLLATE, collate_fill_kernel, dim3((unsigned)a.B, (unsigned)(parts + 2)), dim3(FILL_T), (size_t)a.n_cols * sizeof(int), s,
              a, (int)parts);
  ESC_CHECK_LAUNCH("esc_collate_fill");
  return ESC_OK;
}

}  // extern "C"
