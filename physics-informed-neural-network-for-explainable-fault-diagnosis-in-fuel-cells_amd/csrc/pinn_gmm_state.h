// The mixture's device state block as the kernels that read it see it (pinn_gmm.hip fits and evaluates it, pinn_shap.hip
// explains its posterior, pinn_faultsets.hip ranks its rows): the word offsets of include/pinn_hip.h's layout, the parameters
// staged in LDS, and the per-row E-step that pinn_gmm.hip and pinn_faultsets.hip share to the byte.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kHdr = 8;                     // 8-byte words of the state header

// state block: header words, then weights[K], means[K][D], covariances[K][D][D], precisions_cholesky[K][D][D], logdet[K]
__host__ __device__ inline size_t st_weights() { return kHdr; }
__host__ __device__ inline size_t st_means(int K) { return kHdr + (size_t)K; }
__host__ __device__ inline size_t st_cov(int K, int D) { return st_means(K) + (size_t)K * D; }
__host__ __device__ inline size_t st_chol(int K, int D) { return st_cov(K, D) + (size_t)K * D * D; }
__host__ __device__ inline size_t st_logdet(int K, int D) { return st_chol(K, D) + (size_t)K * D * D; }
__host__ __device__ inline size_t st_words(int K, int D) { return st_logdet(K, D) + (size_t)K; }

// parameters of the state in LDS: means, upper-triangular precisions_cholesky (packed by columns), logdet, log weights
struct Staged {
  double* mu;      // [K][D]
  double* U;       // [K][D (D + 1) / 2]
  double* ld;      // [K]
  double* lw;      // [K]
};

__device__ __forceinline__ void stage_params(const double* __restrict__ st, int K, int D, const Staged& s, bool density) {
  const int T = D * (D + 1) / 2;
  for (int e = threadIdx.x; e < K * D; e += blockDim.x) s.mu[e] = st[st_means(K) + e];
  if (density) {
    for (int e = threadIdx.x; e < K * T; e += blockDim.x) {
      const int k = e / T, t = e - k * T;
      int i, j;
      untri(t, &i, &j);
      s.U[e] = st[st_chol(K, D) + ((size_t)k * D + i) * D + j];
    }
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
      s.ld[k] = st[st_logdet(K, D) + k];
      s.lw[k] = log(st[st_weights() + k]);
    }
  }
  __syncthreads();
}

// log(w_k N(x | mu_k, Sigma_k)) for every k into lp[k * stride]; returns log_prob_norm (scipy's logsumexp: max, sum, log)
__device__ __forceinline__ double estep_row(const double x[kRowsMaxD], int K, int D, const Staged& s, double* lp, int stride) {
#pragma clang fp contract(fast)                             // as pinn_gmm.hip is built, also where the including file is not
  const double c = (double)D * 1.8378770664093453;          // D log(2 pi)
  double m = -INFINITY;
  for (int k = 0; k < K; ++k) {
    double d[kRowsMaxD];
#pragma unroll
    for (int i = 0; i < kRowsMaxD; ++i) d[i] = i < D ? x[i] - s.mu[k * D + i] : 0.0;
    const double* U = s.U + k * (D * (D + 1) / 2);
    double q = 0.0;
#pragma unroll
    for (int j = 0; j < kRowsMaxD; ++j) {
      if (j < D) {
        double y = 0.0;
#pragma unroll
        for (int i = 0; i <= j; ++i) y += d[i] * U[tri(i, j)];
        q += y * y;
      }
    }
    const double v = (-0.5 * (c + q) + s.ld[k]) + s.lw[k];
    lp[k * stride] = v;
    m = v > m ? v : m;
  }
  if (m == -INFINITY) return m;                             // every density underflowed: nothing to normalise
  double sum = 0.0;
  for (int k = 0; k < K; ++k) sum += exp(lp[k * stride] - m);
  return log(sum) + m;
}

}  // namespace
}  // namespace pinn
