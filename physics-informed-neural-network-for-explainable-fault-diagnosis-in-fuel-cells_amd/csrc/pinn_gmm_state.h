// The mixture's device state block as the kernels that read it see it (pinn_gmm.hip fits and evaluates it, pinn_shap.hip
// explains its posterior): the word offsets of include/pinn_hip.h's layout and the parameters staged in LDS.
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

}  // namespace
}  // namespace pinn
