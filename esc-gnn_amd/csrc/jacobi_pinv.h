// jacobi_pinv.h — the one-sided Jacobi SVD behind every pseudo-inverse of a graph Laplacian in this library
// (features.hip: one per rd class of an edge-rooted ego-net; subgraphs.hip: one per node-rooted subgraph).
#pragma once
#include "common.h"

namespace esc {

// ---- the Laplacian L = D_in - A of a node set, column-major with leading dimension ld (scipy csgraph.laplacian) ------------
// Gm = 0, Vm = I over the leading m x m; a barrier follows before the first laplacian_add_edge
template <int NT>
__device__ __forceinline__ void laplacian_clear(double* Gm, double* Vm, int m, int ld) {
  for (int idx = threadIdx.x; idx < m * m; idx += NT) {
    const int cc = idx / m, rr = idx % m;
    Gm[(size_t)cc * ld + rr] = 0.0;
    Vm[(size_t)cc * ld + rr] = (cc == rr) ? 1.0 : 0.0;
  }
}

// the non-loop sub-edge ls -> lt (local indices; which edges enter L is the caller's membership test).  Integer values: the
// order of the atomics is free.
__device__ __forceinline__ void laplacian_add_edge(double* Gm, int ld, int ls, int lt) {
  atomicAdd(&Gm[(size_t)lt * ld + ls], -1.0);               // L[s][t] -= 1   (column-major: [col t][row s])
  atomicAdd(&Gm[(size_t)lt * ld + lt], 1.0);                // L[t][t] += 1   (in-degree, loops excluded)
}

// resistance distance of local nodes a and b from the pseudo-inverse P (P[i][j] at P[j*ld + i]): l_aa + l_bb - l_ab - l_ba, in
// exactly this association (the reference's fp64 expression; the result is rounded to fp32 and, in features.hip, truncated)
__device__ __forceinline__ double resistance(const double* __restrict__ P, int ld, int a, int b) {
  return ((P[(size_t)a * ld + a] + P[(size_t)b * ld + b]) - P[(size_t)b * ld + a]) - P[(size_t)a * ld + b];
}

// ---- one-sided Jacobi SVD based pseudo-inverse probe, NT threads, column-major matrices (LDS or global) -----
// On entry Gm = L (m x m), Vm = I.  On exit Gm = L*V with mutually orthogonal columns.
// Returns the squared-norm threshold below which a column counts as numerically null:
// 4 (m eps)^2 ||L||_F^2, i.e. scipy.linalg.pinv's default cutoff max(M,N)*eps*sigma_max with a
// small margin (||L||_F >= sigma_max).  Null columns are neither rotated nor inverted.
template <int NT>
__device__ double jacobi_orthogonalise(double* __restrict__ Gm, double* __restrict__ Vm, int m, int ld, double* red) {
  const int tid = threadIdx.x;
  double fro2 = 0.0;
  for (int idx = tid; idx < m * m; idx += NT) {
    const double v = Gm[(size_t)(idx / m) * ld + (idx % m)];
    fro2 += v * v;
  }
  fro2 = wave_sum(fro2);
  if (NT > 64) {                                  // fixed order over the waves: the threshold is the same in every thread
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = fro2;
    __syncthreads();
    fro2 = 0.0;
    for (int w = 0; w < NT / 64; ++w) fro2 += red[w];
    __syncthreads();
  }
  const double meps = (double)m * 2.220446049250313e-16;
  const double null2 = 4.0 * meps * meps * fro2;
  if (m < 2 || fro2 == 0.0) return null2;
  const int M = (m + 1) & ~1;                  // round-robin needs an even player count (last = dummy)
  const int npairs = M / 2;
  int S = 1;                                   // sub-lanes per pair (power of two, inside one wave)
  while (S < 64 && npairs * S * 2 <= NT) S *= 2;
  if (NT > 64 && S < 8) S = 8;                 // global-memory matrices: 8 consecutive rows per pair = one 64-B segment
  const int pairs_per_pass = NT / S;
  for (int sweep = 0; sweep < 40; ++sweep) {
    int rotated = 0;
    for (int r = 0; r < M - 1; ++r) {
      for (int p0 = 0; p0 < npairs; p0 += pairs_per_pass) {
        const int pi = p0 + tid / S, sub = tid % S;
        int p = -1, q = -1;
        if (pi < npairs) {
          const int a = pi, b = M - 1 - pi;
          p = (a == 0) ? 0 : 1 + ((a - 1 + r) % (M - 1));
          q = 1 + ((b - 1 + r) % (M - 1));
          if (p > q) { const int t = p; p = q; q = t; }
          if (q >= m) p = -1;                  // paired with the dummy player
        }
        double al = 0.0, be = 0.0, ga = 0.0;
        if (p >= 0) {
          const double* gp = Gm + (size_t)p * ld;
          const double* gq = Gm + (size_t)q * ld;
          for (int i = sub; i < m; i += S) {
            const double x = gp[i], y = gq[i];
            al += x * x; be += y * y; ga += x * y;
          }
        }
        for (int o = 1; o < S; o <<= 1) {
          al += __shfl_xor(al, o, 64); be += __shfl_xor(be, o, 64); ga += __shfl_xor(ga, o, 64);
        }
        bool rot = false;
        double c = 1.0, s = 0.0;
        if (p >= 0 && al > null2 && be > null2 && fabs(ga) > 1e-15 * sqrt(al * be)) {
          const double zeta = (be - al) / (2.0 * ga);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          c = 1.0 / sqrt(1.0 + t * t);
          s = c * t;
          rot = true;
        }
        if (rot) {
          double* gp = Gm + (size_t)p * ld; double* gq = Gm + (size_t)q * ld;
          double* vp = Vm + (size_t)p * ld; double* vq = Vm + (size_t)q * ld;
          for (int i = sub; i < m; i += S) {
            const double x = gp[i], y = gq[i];
            gp[i] = c * x - s * y; gq[i] = s * x + c * y;
            const double u = vp[i], w = vq[i];
            vp[i] = c * u - s * w; vq[i] = s * u + c * w;
          }
        }
        rotated |= __syncthreads_or(rot ? 1 : 0);
      }
    }
    if (!rotated) break;
  }
  return null2;
}

// squared singular values = squared column norms of the orthogonalised Gm; numerically-null ones are dropped (pinv cutoff).
// Then P = V diag(1/s^2) G^T, written over V row by row: P[i][j'] = sum_j V[i][j] G[j'][j] / s_j^2, so that on exit
// P[i][j] sits at Vm[j*ld + i].  inv_s2 and vrow hold m doubles each.  Every thread of the workgroup calls it.
template <int NT>
__device__ void pinv_from_jacobi(const double* __restrict__ Gm, double* __restrict__ Vm, int m, int ld, double null2,
                                 double* __restrict__ inv_s2, double* __restrict__ vrow) {
  const int tid = threadIdx.x;
  for (int j = tid; j < m; j += NT) {
    double s2 = 0.0;
    for (int i = 0; i < m; ++i) { const double t = Gm[(size_t)j * ld + i]; s2 += t * t; }
    inv_s2[j] = (s2 > null2) ? 1.0 / s2 : 0.0;
  }
  __syncthreads();
  for (int i = 0; i < m; ++i) {
    for (int j = tid; j < m; j += NT) vrow[j] = Vm[(size_t)j * ld + i] * inv_s2[j];
    __syncthreads();
    for (int jp = tid; jp < m; jp += NT) {
      double acc = 0.0;
      for (int j = 0; j < m; ++j) acc += vrow[j] * Gm[(size_t)j * ld + jp];
      Vm[(size_t)jp * ld + i] = acc;
    }
    __syncthreads();
  }
}

}  // namespace esc
