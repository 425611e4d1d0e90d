// pinn_loss.h -- the aleatoric loss (01:916-927), its gradient, the layout of the loss partials and the MC-dropout finish:
// the arithmetic every training family (fused fp32 / bf16 / split-operand, wide, any layers list) has to agree on, stated once.
// Device code only, no state; every function takes the flags of the translation unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace pinn {

// One loss partial = kLossTerms doubles per workgroup (per 16 rows in the general path).  Producers fill the first kLossSums
// slots and zero the spare ones; the reductions (grad_finalize_kernel, gen::finalize_kernel) report the first kLossOut to the
// host and turn kLossDu, kLossDz into the gradients of the two scalar head biases b_p and bv_2.
constexpr int kLossNll = 0;     // sum of 0.5 prec e^2 + 0.5 logvar
constexpr int kLossAbs = 1;     // sum of |logvar|
constexpr int kLossMse = 2;     // sum of (y - u)^2
constexpr int kLossDu = 3;      // sum of d loss / d u
constexpr int kLossDz = 4;      // sum of d loss / d z
constexpr int kLossSums = 5;
constexpr int kLossOut = 4;
constexpr int kLossTerms = 8;

// logvar = log(softplus(z) + 1e-6), softplus with torch's threshold 20 (01:432-434)
__device__ __forceinline__ float softplus_f32(float z) { return z > 20.0f ? z : log1pf(expf(z)); }
__device__ __forceinline__ float var_of(float z) { return softplus_f32(z) + 1e-6f; }
__device__ __forceinline__ float logvar_of(float z) { return logf(var_of(z)); }
// softplus'(z); torch: 1 above the threshold
__device__ __forceinline__ float softplus_slope(float z) { return z > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-z)); }
// g * d logvar / dz = g * softplus'(z) / (softplus(z) + 1e-6) from slope = softplus_slope(z), var = var_of(z): the product with
// the upstream gradient first, then the division -- the rounding every family's dz has
__device__ __forceinline__ float through_logvar(float g, float slope, float var) { return g * slope / var; }

// A lane's running sums over its rows.
struct LossSums {
  float nll = 0.f, abs = 0.f, mse = 0.f, du = 0.f, dz = 0.f;
};

// One row of the loss: its gradient du, dz (already / N, inv_n = 1 / N; zero on a row that is not valid) and, on the lanes with
// `take` set, its three terms and its gradient added to `sums`.
__device__ __forceinline__ void loss_row(float u, float z, float y, float inv_n, bool valid, bool take, float& du, float& dz, LossSums& sums) {
  du = 0.f; dz = 0.f;
  const float var = var_of(z);
  const float s = logf(var);                 // logvar
  const float prec = expf(-s);               // precision = exp(-logvar), 01:919
  const float e = y - u;
  if (valid) {
    du = -(prec * e) * inv_n;
    const float sgn = (s > 0.f) ? 1.f : ((s < 0.f) ? -1.f : 0.f);
    const float ds = (-0.5f * prec * e * e + 0.5f + 0.01f * sgn) * inv_n;
    dz = through_logvar(ds, softplus_slope(z), var);
    if (take) {
      sums.nll += 0.5f * prec * e * e + 0.5f * s;
      sums.abs += fabsf(s);
      sums.mse += e * e;
      sums.du += du;
      sums.dz += dz;
    }
  }
}

// The workgroup's loss partial from its lanes' sums: a double shuffle tree per wave, then the WAVES wave sums in order.
// Every thread of the workgroup calls it (one barrier); red is LDS of at least WAVES rows.
template <int WAVES>
__device__ __forceinline__ void store_loss_partials(const LossSums& s, double (*red)[kLossTerms], double* loss_part, int lane, int wave) {
  float terms[kLossSums];
  terms[kLossNll] = s.nll; terms[kLossAbs] = s.abs; terms[kLossMse] = s.mse; terms[kLossDu] = s.du; terms[kLossDz] = s.dz;
#pragma unroll
  for (int k = 0; k < kLossSums; ++k) {
    double v = (double)terms[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < kLossTerms) {
    double t = 0.0;
    if (threadIdx.x < kLossSums)
      for (int w = 0; w < WAVES; ++w) t += red[w][threadIdx.x];
    loss_part[(long long)blockIdx.x * kLossTerms + threadIdx.x] = t;
  }
}

// MC-dropout finish (01:1483, 1486): a_u = sqrt(exp(mean_t logvar_t)), e_u = population std of the passes from Welford's m2
__device__ __forceinline__ void mc_finish(float m2, float sum_logvar, int n_passes, float& a_u, float& e_u) {
  const float inv_t = 1.0f / (float)n_passes;
  const float var = m2 * inv_t;
  a_u = expf(0.5f * (sum_logvar * inv_t));
  e_u = sqrtf(var);
}

// Wave maximum of a non-negative float, then one atomicMax on its bits by the lanes with `writer` set.  Non-negative floats order
// like unsigned integers, so the word does not depend on the order of the waves (bitwise reproducible); fmaxf drops a NaN.
__device__ __forceinline__ void wave_max_to(unsigned* word, float v, bool writer) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  if (writer) atomicMax(word, __float_as_uint(v));
}

}  // namespace pinn
