// lappe.hip — the Laplacian positional encoding of the graph transformer (include/escgnn_lappe.h): what the
// reference computes on the host with numpy.linalg.eigh per graph at dataset load (GraphGPS/graphgps/transform/posenc_stats.py),
// collates as the EigVecs / EigVals keys, and encodes with LapPENodeEncoder (graphgps/encoder/laplace_pos_encoder.py).
//
// esc_laplacian_eig: one workgroup of 256 threads per graph.  L = D - A is built in fp64, column-major, and handed to the
// one-sided Jacobi of jacobi_pinv.h as it stands: for a positive semi-definite matrix the right singular vectors V are
// eigenvectors and the column norms of G = L V the eigenvalues (null columns: norm ~ 1e-15, and V's columns there span the
// kernel because V stays orthogonal).  The two n x n matrices live in LDS up to EIG_LDS_NODES nodes and on a slab of the
// caller's scratch above.  The column stride is n | 1 doubles: the sub-lanes of one Jacobi pair read consecutive doubles of
// a column (ds_read_b64, conflict-free), different pairs read different columns, and an odd stride in 8-byte units spreads
// the column heads over all 32 double-wide bank pairs.  The workgroup size and every loop bound depend on the graph alone
// (never on max_nodes or the launch), and the file is built without FMA contraction, so a graph's bits are the same alone
// and in any batch.
// esc_lappe_gather: one workgroup per graph of the batch copies its n x K rows of the two resident tables (ragged_graphs.h).
// esc_lappe_encode_fwd: one thread per node, the (zero-padded) weights in LDS, read as broadcasts.
// esc_lappe_encode_bwd: launch 1 — a workgroup per block of ENC_ROWS rows; its row x frequency terms go through LDS in chunks:
// phase 1, a thread per term, recomputes the hidden activations and leaves [a | dh | da | v | l | 1] of the term as one LDS row;
// phase 2, a thread per parameter, adds the products of two columns of those rows over the chunk in term order (in fp64: one chain
// runs over a thousand terms of either sign).  Launch 2 adds the workgroups' partials in workgroup order.  No atomics anywhere.
#include "ragged_graphs.h"
#include "jacobi_pinv.h"
#include "../../include/escgnn_lappe.h"

namespace esc {

constexpr int EIG_NT = 256;
constexpr int EIG_MAX_NODES = 256;
constexpr int LAPPE_MAX_FREQS = 32;
constexpr int EIG_LDS_MATRIX_BYTES = 128 * 1024;     // the two matrices of one graph: 128 KiB of the CU's 160 KiB at most

constexpr int eig_ld(int n) { return n | 1; }
constexpr int64_t eig_matrix_bytes(int n) { return (int64_t)2 * n * eig_ld(n) * (int64_t)sizeof(double); }
constexpr int eig_lds_nodes_of(int64_t bytes) {
  int n = 0;
  while (eig_matrix_bytes(n + 1) <= bytes) ++n;
  return n;
}
constexpr int EIG_LDS_NODES = eig_lds_nodes_of(EIG_LDS_MATRIX_BYTES);      // 90: 2 * 90 * 91 * 8 = 131 040 bytes
static_assert(EIG_LDS_NODES == 90, "the header states 90");
// LDS beside the matrices: lam[cap] red[8] nrm[LAPPE_MAX_FREQS] (doubles), order[LAPPE_MAX_FREQS] (ints)
inline size_t eig_lds_bytes(int cap) {
  const int in_lds = cap < EIG_LDS_NODES ? cap : EIG_LDS_NODES;
  return (size_t)eig_matrix_bytes(in_lds) + (size_t)(cap + 8 + LAPPE_MAX_FREQS) * sizeof(double) + LAPPE_MAX_FREQS * sizeof(int);
}

struct EigArgs {
  const int64_t* src; const int64_t* dst; const int64_t* node_ptr; const int64_t* edge_ptr;
  int64_t N, E, scratch_doubles;
  int local, K, cap, lds_cap;                // cap: max_nodes as told; lds_cap: the graph size the LDS matrices hold
  double* scratch;
  float* vecs; float* vals;
};

// the decomposition of one graph on matrices in LDS or global memory (one call site each: the address space is known there)
__device__ __forceinline__ void eig_graph(const EigArgs& a, double* __restrict__ Gm, double* __restrict__ Vm, int n, int ld, int64_t n0,
                                          int64_t base, int64_t e0, int64_t e1, double* lam, double* red, double* nrm, int* order) {
  const int tid = threadIdx.x;
  for (int idx = tid; idx < n * n; idx += EIG_NT) {
    const int c = idx / n, r = idx % n;
    Gm[(size_t)c * ld + r] = 0.0;
    Vm[(size_t)c * ld + r] = (c == r) ? 1.0 : 0.0;
  }
  __syncthreads();
  for (int64_t e = e0 + tid; e < e1; e += EIG_NT) {          // A symmetrised: plain stores of one value, order free
    int64_t s, t;
    (void)edge_ends(a.src, a.dst, e, base, n, s, t);          // (checked by the caller's pass over the same edges)
    if (s != t) {
      Gm[(size_t)t * ld + s] = -1.0;
      Gm[(size_t)s * ld + t] = -1.0;
    }
  }
  __syncthreads();
  for (int j = tid; j < n; j += EIG_NT) {                    // the degree: the diagonal is still 0
    double deg = 0.0;
    for (int i = 0; i < n; ++i) deg -= Gm[(size_t)j * ld + i];
    Gm[(size_t)j * ld + j] = deg;
  }
  __syncthreads();
  (void)jacobi_orthogonalise<EIG_NT>(Gm, Vm, n, ld, red);
  __syncthreads();
  for (int j = tid; j < n; j += EIG_NT) {                    // eigenvalue = column norm of G = L V
    double s2 = 0.0;
    for (int i = 0; i < n; ++i) { const double t = Gm[(size_t)j * ld + i]; s2 += t * t; }
    lam[j] = sqrt(s2);
  }
  __syncthreads();
  for (int j = tid; j < n; j += EIG_NT) {                    // ascending, equal values in column order
    const double lj = lam[j];
    int rank = 0;
    for (int i = 0; i < n; ++i) rank += (lam[i] < lj || (lam[i] == lj && i < j)) ? 1 : 0;
    if (rank < a.K) order[rank] = j;
  }
  __syncthreads();
  const int kept = n < a.K ? n : a.K;
  for (int r = tid; r < kept; r += EIG_NT) {
    const double* v = Vm + (size_t)order[r] * ld;
    double s2 = 0.0;
    for (int i = 0; i < n; ++i) s2 += v[i] * v[i];
    const double nr = sqrt(s2);
    nrm[r] = nr > 1e-12 ? nr : 1e-12;
  }
  __syncthreads();
  const float nan = __int_as_float(0x7fc00000);
  for (int t = tid; t < n * a.K; t += EIG_NT) {
    const int i = t / a.K, r = t % a.K;
    float vec = nan, val = nan;
    if (r < kept) {
      const int j = order[r];
      vec = (float)(Vm[(size_t)j * ld + i] / nrm[r]);
      val = (float)(lam[j] > 0.0 ? lam[j] : 0.0);
    }
    a.vecs[(n0 + i) * a.K + r] = vec;
    a.vals[(n0 + i) * a.K + r] = val;
  }
}

__global__ __launch_bounds__(EIG_NT) void lap_eig_kernel(EigArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const GraphRange r = graph_range(a.node_ptr, a.edge_ptr, blockIdx.x, a.N, a.E);
  const int64_t n0 = r.n0, e0 = r.e0, e1 = r.e1;
  // (all of this is uniform over the workgroup: it leaves together)
  if (!(r.ok && r.n1 > n0 && r.n1 - n0 <= a.cap)) return;     // an empty graph and one over max_nodes are skipped
  const int n = (int)(r.n1 - n0);
  const int64_t base = a.local ? 0 : n0;
  int bad = 0;
  for (int64_t e = e0 + tid; e < e1; e += EIG_NT) {
    int64_t s, t;
    if (!edge_ends(a.src, a.dst, e, base, n, s, t)) bad = 1;
  }
  if (__syncthreads_or(bad)) return;
  double* lam = reinterpret_cast<double*>(smem);
  double* red = lam + a.cap;
  double* nrm = red + 8;
  int* order = reinterpret_cast<int*>(nrm + LAPPE_MAX_FREQS);
  const int ld = eig_ld(n);
  if (n <= a.lds_cap) {
    double* Gm = reinterpret_cast<double*>(order + LAPPE_MAX_FREQS);
    eig_graph(a, Gm, Gm + (size_t)ld * n, n, ld, n0, base, e0, e1, lam, red, nrm, order);
  } else {
    const int64_t off = 2 * n0 * eig_ld(a.cap);             // this graph's slab: 2 * n * (cap | 1) doubles
    if (off + 2 * (int64_t)ld * n > a.scratch_doubles) return;
    double* Gm = a.scratch + off;
    eig_graph(a, Gm, Gm + (size_t)ld * n, n, ld, n0, base, e0, e1, lam, red, nrm, order);
  }
}

// ---- the DeepSet encoder ---------------------------------------------------------------------------------------------------------
// P is padded with zero weights to PP = 4, 8, 16 or 32 in LDS and registers (a padded hidden unit is ReLU(0) = 0 and a padded
// output 0: they add exactly nothing), which keeps the register arrays compile-time sized with four instantiations.
constexpr int ENC_ROWS = 32;                 // rows per workgroup of the backward: the fixed row partition
constexpr int ENC_NT = 256;
inline int enc_pad(int P) { return P <= 4 ? 4 : P <= 8 ? 8 : P <= 16 ? 16 : 32; }
inline int64_t enc_params(int P) { return 2LL * P * P + 7LL * P; }
template <int PP> constexpr int enc_weight_floats = 2 * PP * PP + 7 * PP;     // wa0[2PP] wa1[2PP] ba[2PP] w1t[2PP][PP] b1[PP]
template <int PP> constexpr int enc_chunk = 2048 / PP < 256 ? 2048 / PP : 256;  // terms per chunk of the backward
template <int PP> constexpr int enc_row_floats = 5 * PP + 3;                     // [a 2PP | dh PP | da 2PP | v | l | 1]: odd, no bank conflict between terms

template <int PP>
__device__ __forceinline__ void enc_stage(float* W, const float* __restrict__ wA, const float* __restrict__ bA,
                                          const float* __restrict__ w1, const float* __restrict__ b1, int P) {
  float* wa0 = W; float* wa1 = wa0 + 2 * PP; float* ba = wa1 + 2 * PP; float* w1t = ba + 2 * PP; float* bb = w1t + 2 * PP * PP;
  for (int q = threadIdx.x; q < 2 * PP; q += blockDim.x) {
    const bool in = q < 2 * P;
    wa0[q] = in ? wA[2 * q] : 0.f; wa1[q] = in ? wA[2 * q + 1] : 0.f; ba[q] = in ? bA[q] : 0.f;
  }
  for (int t = threadIdx.x; t < 2 * PP * PP; t += blockDim.x) {
    const int q = t / PP, p = t % PP;
    w1t[t] = (q < 2 * P && p < P) ? w1[p * 2 * P + q] : 0.f;
  }
  for (int p = threadIdx.x; p < PP; p += blockDim.x) bb[p] = p < P ? b1[p] : 0.f;
}

// h = W1 ReLU(WA [v, l] + bA) + b1 (before its ReLU); the hidden activations go to a_out when it is not null
template <int PP>
__device__ __forceinline__ void enc_hidden(const float* W, float v, float l, float (&h)[PP], float* a_out) {
  const float* wa0 = W; const float* wa1 = wa0 + 2 * PP; const float* ba = wa1 + 2 * PP; const float* w1t = ba + 2 * PP;
  const float* bb = w1t + 2 * PP * PP;
#pragma unroll
  for (int p = 0; p < PP; ++p) h[p] = bb[p];
#pragma unroll 1
  for (int q = 0; q < 2 * PP; ++q) {                      // (not unrolled: the weights stay in LDS, read as broadcasts)
    const float act = fmaxf(fmaf(wa0[q], v, fmaf(wa1[q], l, ba[q])), 0.f);
    if (a_out) a_out[q] = act;
#pragma unroll
    for (int p = 0; p < PP; p += 4) {
      const float4 w = *reinterpret_cast<const float4*>(w1t + q * PP + p);
      h[p] = fmaf(w.x, act, h[p]); h[p + 1] = fmaf(w.y, act, h[p + 1]);
      h[p + 2] = fmaf(w.z, act, h[p + 2]); h[p + 3] = fmaf(w.w, act, h[p + 3]);
    }
  }
}

template <int PP>
__global__ __launch_bounds__(64) void lappe_fwd_kernel(const float* __restrict__ vecs, const float* __restrict__ vals,
                                                       const float* __restrict__ signs, const float* __restrict__ wA,
                                                       const float* __restrict__ bA, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, int64_t N, int K, int P, float* __restrict__ out,
                                                       int64_t ldo) {
  __shared__ __attribute__((aligned(16))) float W[enc_weight_floats<PP>];
  enc_stage<PP>(W, wA, bA, w1, b1, P);
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= N) return;
  float acc[PP];
#pragma unroll
  for (int p = 0; p < PP; ++p) acc[p] = 0.f;
  for (int j = 0; j < K; ++j) {
    float v = vecs[i * K + j], l = vals[i * K + j];
    if (v != v) continue;                                  // the term is dropped
    if (signs) v *= signs[j];
    if (l != l) l = 0.f;
    float h[PP];
    enc_hidden<PP>(W, v, l, h, nullptr);
#pragma unroll
    for (int p = 0; p < PP; ++p) acc[p] += fmaxf(h[p], 0.f);
  }
#pragma unroll
  for (int p = 0; p < PP; ++p)
    if (p < P) out[i * ldo + p] = acc[p];
}

template <int PP>
__global__ __launch_bounds__(ENC_NT) void lappe_bwd_kernel(const float* __restrict__ vecs, const float* __restrict__ vals,
                                                           const float* __restrict__ signs, const float* __restrict__ wA,
                                                           const float* __restrict__ bA, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ d_out, int64_t ldg,
                                                           int64_t N, int K, int P, float* __restrict__ partial) {
  constexpr int T = enc_chunk<PP>, RS = enc_row_floats<PP>;
  constexpr int NPT = (enc_weight_floats<PP> + ENC_NT - 1) / ENC_NT;          // parameters per thread
  __shared__ __attribute__((aligned(16))) float W[enc_weight_floats<PP>];
  __shared__ float rows[T * RS];
  const int tid = threadIdx.x;
  enc_stage<PP>(W, wA, bA, w1, b1, P);
  const float* w1t = W + 6 * PP;
  // this thread's parameters: flat index over (d_wA [2P, 2], d_bA [2P], d_w1 [P, 2P], d_b1 [P]) -> the two row columns whose
  // product, summed over the terms, is that gradient
  const int nparams = 2 * P * P + 7 * P;
  int ox[NPT], oy[NPT];
  double acc[NPT];                                         // fp64: a block sums up to ENC_ROWS * 32 terms of either sign in one chain
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = tid + u * ENC_NT;
    acc[u] = 0.0;
    ox[u] = oy[u] = 0;
    if (idx < 4 * P) { ox[u] = 3 * PP + idx / 2; oy[u] = 5 * PP + idx % 2; }
    else if (idx < 6 * P) { ox[u] = 3 * PP + idx - 4 * P; oy[u] = 5 * PP + 2; }
    else if (idx < 6 * P + 2 * P * P) { const int k = idx - 6 * P; ox[u] = 2 * PP + k / (2 * P); oy[u] = k % (2 * P); }
    else if (idx < nparams) { ox[u] = 2 * PP + idx - 6 * P - 2 * P * P; oy[u] = 5 * PP + 2; }
  }
  const int64_t r0 = (int64_t)blockIdx.x * ENC_ROWS;
  const int terms = ENC_ROWS * K;
  for (int c0 = 0; c0 < terms; c0 += T) {
    __syncthreads();                                       // the weights are staged / the previous chunk's rows are consumed
    if (tid < T) {                                         // ---- phase 1: thread = term
      const int tt = c0 + tid;
      const int64_t i = r0 + tt / K;
      const int j = tt % K;
      float* R = rows + tid * RS;
      float v = (tt < terms && i < N) ? vecs[i * K + j] : __int_as_float(0x7fc00000);
      if (v == v) {
        float l = vals[i * K + j];
        if (signs) v *= signs[j];
        if (l != l) l = 0.f;
        float h[PP];
        enc_hidden<PP>(W, v, l, h, R);
#pragma unroll
        for (int p = 0; p < PP; ++p) {
          h[p] = (p < P && h[p] > 0.f) ? d_out[i * ldg + p] : 0.f;       // dh
          R[2 * PP + p] = h[p];
        }
#pragma unroll 1
        for (int q = 0; q < 2 * PP; ++q) {
          float s = 0.f;
#pragma unroll
          for (int p = 0; p < PP; p += 4) {
            const float4 w = *reinterpret_cast<const float4*>(w1t + q * PP + p);
            s = fmaf(w.x, h[p], s); s = fmaf(w.y, h[p + 1], s); s = fmaf(w.z, h[p + 2], s); s = fmaf(w.w, h[p + 3], s);
          }
          R[3 * PP + q] = R[q] > 0.f ? s : 0.f;                           // da
        }
        R[5 * PP] = v; R[5 * PP + 1] = l; R[5 * PP + 2] = 1.f;
      } else {
        for (int c = 0; c < RS; ++c) R[c] = 0.f;                          // a dropped term: exact zeros everywhere
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NPT; ++u) {                        // ---- phase 2: thread = parameter, terms in order
      double s = acc[u];
      for (int t = 0; t < T; ++t) s += (double)rows[t * RS + ox[u]] * (double)rows[t * RS + oy[u]];     // (the product is exact)
      acc[u] = s;
    }
  }
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int idx = tid + u * ENC_NT;
    if (idx < nparams) partial[(int64_t)blockIdx.x * nparams + idx] = (float)acc[u];
  }
}

__global__ __launch_bounds__(256) void lappe_bwd_sum_kernel(const float* __restrict__ partial, int64_t blocks, int P, float* __restrict__ d_wA,
                                                            float* __restrict__ d_bA, float* __restrict__ d_w1, float* __restrict__ d_b1) {
  const int nparams = 2 * P * P + 7 * P;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= nparams) return;
  double sum = 0.0;
  for (int64_t w = 0; w < blocks; ++w) sum += (double)partial[w * nparams + idx];
  const float s = (float)sum;
  if (idx < 4 * P) d_wA[idx] = s;
  else if (idx < 6 * P) d_bA[idx - 4 * P] = s;
  else if (idx < 6 * P + 2 * P * P) d_w1[idx - 6 * P] = s;
  else d_b1[idx - 6 * P - 2 * P * P] = s;
}

static int enc_check(const char* who, int64_t N, int K, int P) {
  ESC_REQUIRE(P > 0 && P <= 32 && P % 4 == 0, "%s: dim_pe %d must be a multiple of 4 and at most 32", who, P);
  ESC_REQUIRE(K >= 1 && K <= LAPPE_MAX_FREQS, "%s: max_freqs %d outside 1..%d", who, K, LAPPE_MAX_FREQS);
  ESC_REQUIRE(N >= 0 && N < (1LL << 31) / LAPPE_MAX_FREQS, "%s: bad size N=%ld", who, (long)N);
  return ESC_OK;
}

#define ESC_LAPPE_DISPATCH(LAUNCH)               \
  switch (enc_pad(P)) {                          \
    case 4: LAUNCH(4); break;                    \
    case 8: LAUNCH(8); break;                    \
    case 16: LAUNCH(16); break;                  \
    default: LAUNCH(32); break;                  \
  }

}  // namespace esc

using namespace esc;

extern "C" {

int64_t esc_laplacian_eig_max_nodes(void) { return EIG_MAX_NODES; }
int64_t esc_laplacian_eig_lds_nodes(void) { return EIG_LDS_NODES; }

int64_t esc_laplacian_eig_scratch_bytes(int64_t N, int64_t max_nodes) {
  if (N <= 0 || max_nodes <= EIG_LDS_NODES || max_nodes > EIG_MAX_NODES) return 0;
  return 2 * N * eig_ld((int)max_nodes) * (int64_t)sizeof(double);
}

int esc_laplacian_eig(const int64_t* src, const int64_t* dst, int64_t E, const int64_t* node_ptr, const int64_t* edge_ptr,
                      int64_t G, int64_t N, int edges_local, int max_freqs, int64_t max_nodes, void* scratch,
                      int64_t scratch_bytes, float* eigvecs, float* eigvals, void* stream) {
  ESC_REQUIRE(max_freqs >= 1 && max_freqs <= LAPPE_MAX_FREQS, "esc_laplacian_eig: max_freqs %d outside 1..%d", max_freqs, LAPPE_MAX_FREQS);
  ESC_REQUIRE(G >= 0 && N >= 0 && E >= 0 && G < (1LL << 31) && N < (1LL << 31) / LAPPE_MAX_FREQS && E < (1LL << 31) && max_nodes >= 0 &&
              scratch_bytes >= 0, "esc_laplacian_eig: bad sizes G=%ld N=%ld E=%ld max_nodes=%ld scratch_bytes=%ld", (long)G, (long)N,
              (long)E, (long)max_nodes, (long)scratch_bytes);
  ESC_REQUIRE(max_nodes <= EIG_MAX_NODES, "esc_laplacian_eig: a graph of %ld nodes exceeds the limit of %d nodes per graph "
              "(esc_laplacian_eig_max_nodes)", (long)max_nodes, EIG_MAX_NODES);
  if (G == 0 || N == 0 || max_nodes == 0) return ESC_OK;
  const int64_t need = esc_laplacian_eig_scratch_bytes(N, max_nodes);
  ESC_REQUIRE(scratch_bytes >= need && (need == 0 || scratch), "esc_laplacian_eig: %ld bytes of scratch, %ld needed at max_nodes %ld "
              "(esc_laplacian_eig_scratch_bytes)", (long)scratch_bytes, (long)need, (long)max_nodes);
  ESC_REQUIRE(node_ptr && edge_ptr && eigvecs && eigvals && (E == 0 || (src && dst)), "esc_laplacian_eig: null pointer");
  const int cap = (int)max_nodes;
  const EigArgs a{src, dst, node_ptr, edge_ptr, N, E, need ? scratch_bytes / (int64_t)sizeof(double) : 0, edges_local ? 1 : 0, max_freqs,
                  cap, cap < EIG_LDS_NODES ? cap : EIG_LDS_NODES, (double*)scratch, eigvecs, eigvals};
  const size_t lds = eig_lds_bytes(cap);
  if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)lap_eig_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  esc::launch(-1, lap_eig_kernel, dim3((unsigned)G), dim3(EIG_NT), lds, (hipStream_t)stream, a);
  ESC_CHECK_LAUNCH("esc_laplacian_eig");
  return ESC_OK;
}

int esc_lappe_gather(const float* vecs_all, const float* vals_all, const int64_t* node_ptr_all, int64_t G_all, int64_t N_all,
                     const int64_t* graph_ids, const int32_t* graph_ptr, int64_t B, int64_t N, int K, float* vecs,
                     float* vals, void* stream) {
  ESC_REQUIRE(K >= 1 && K <= LAPPE_MAX_FREQS, "esc_lappe_gather: max_freqs %d outside 1..%d", K, LAPPE_MAX_FREQS);
  ESC_REQUIRE(G_all >= 0 && N_all >= 0 && B >= 0 && N >= 0 && B < (1LL << 31) && N < (1LL << 31) / LAPPE_MAX_FREQS,
              "esc_lappe_gather: bad sizes G_all=%ld N_all=%ld B=%ld N=%ld", (long)G_all, (long)N_all, (long)B, (long)N);
  if (B == 0 || N == 0 || G_all == 0) return ESC_OK;
  ESC_REQUIRE(vecs_all && vals_all && node_ptr_all && graph_ids && graph_ptr && vecs && vals, "esc_lappe_gather: null pointer");
  esc::launch(-1, table_gather_kernel<2>, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, GatherTables<2>{{vecs_all, vals_all}, {vecs, vals}},
              node_ptr_all, G_all, N_all, graph_ids, graph_ptr, N, K, (int64_t)K);
  ESC_CHECK_LAUNCH("esc_lappe_gather");
  return ESC_OK;
}

int esc_lappe_encode_fwd(const float* eigvecs, const float* eigvals, const float* signs, const float* wA, const float* bA,
                         const float* w1, const float* b1, int64_t N, int K, int P, float* out, int64_t ld_out, void* stream) {
  const int rc = enc_check("esc_lappe_encode_fwd", N, K, P);
  if (rc != ESC_OK) return rc;
  ESC_REQUIRE(ld_out >= P, "esc_lappe_encode_fwd: leading dimension of out %ld below dim_pe = %d", (long)ld_out, P);
  if (N == 0) return ESC_OK;
  ESC_REQUIRE(eigvecs && eigvals && wA && bA && w1 && b1 && out, "esc_lappe_encode_fwd: null pointer");
  const dim3 grid((unsigned)cdiv(N, 64)), block(64);
#define ESC_LAPPE_FWD(PP) \
  esc::launch(-1, lappe_fwd_kernel<PP>, grid, block, 0, (hipStream_t)stream, eigvecs, eigvals, signs, wA, bA, w1, b1, N, K, P, out, ld_out)
  ESC_LAPPE_DISPATCH(ESC_LAPPE_FWD)
#undef ESC_LAPPE_FWD
  ESC_CHECK_LAUNCH("esc_lappe_encode_fwd");
  return ESC_OK;
}

int64_t esc_lappe_encode_block_rows(void) { return ENC_ROWS; }

int64_t esc_lappe_encode_scratch_floats(int64_t N, int P) {
  return (N > 0 && P > 0 && P <= 32) ? cdiv(N, ENC_ROWS) * enc_params(P) : 0;
}

int esc_lappe_encode_bwd(const float* eigvecs, const float* eigvals, const float* signs, const float* wA, const float* bA,
                         const float* w1, const float* b1, const float* d_out, int64_t ld_dout, int64_t N, int K, int P,
                         float* scratch, int64_t scratch_floats, float* d_wA, float* d_bA, float* d_w1, float* d_b1,
                         void* stream) {
  const int rc = enc_check("esc_lappe_encode_bwd", N, K, P);
  if (rc != ESC_OK) return rc;
  ESC_REQUIRE(ld_dout >= P, "esc_lappe_encode_bwd: leading dimension of d_out %ld below dim_pe = %d", (long)ld_dout, P);
  const int64_t need = esc_lappe_encode_scratch_floats(N, P);
  ESC_REQUIRE(scratch_floats >= need, "esc_lappe_encode_bwd: %ld floats of scratch, %ld needed (esc_lappe_encode_scratch_floats)",
              (long)scratch_floats, (long)need);
  ESC_REQUIRE(d_wA && d_bA && d_w1 && d_b1 && (N == 0 || (eigvecs && eigvals && wA && bA && w1 && b1 && d_out && scratch)),
              "esc_lappe_encode_bwd: null pointer");
  const int64_t blocks = cdiv(N, ENC_ROWS);
  if (blocks > 0) {
    const dim3 grid((unsigned)blocks), block(ENC_NT);
#define ESC_LAPPE_BWD(PP) \
  esc::launch(-1, lappe_bwd_kernel<PP>, grid, block, 0, (hipStream_t)stream, eigvecs, eigvals, signs, wA, bA, w1, b1, d_out, ld_dout, N, K, P, scratch)
    ESC_LAPPE_DISPATCH(ESC_LAPPE_BWD)
#undef ESC_LAPPE_BWD
    ESC_CHECK_LAUNCH("esc_lappe_encode_bwd");
  }
  esc::launch(-1, lappe_bwd_sum_kernel, dim3((unsigned)cdiv(enc_params(P), 256)), dim3(256), 0, (hipStream_t)stream, (const float*)scratch, blocks,
              P, d_wA, d_bA, d_w1, d_b1);
  ESC_CHECK_LAUNCH("esc_lappe_encode_bwd");
  return ESC_OK;
}

}  // extern "C"
