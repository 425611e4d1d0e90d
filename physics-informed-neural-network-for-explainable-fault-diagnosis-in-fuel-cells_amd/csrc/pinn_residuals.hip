// pinn_residuals.hip -- fused physics-residual pass for gfx950 (HBM-bound, K1 of DESIGN.md).
//
// One pass over the normalised rows evaluates the four residual models of the reference
//   net_f_V 01:724-765, net_f_T_simple 01:869-914, net_f_H 01:621-722, net_f_O 01:535-619
// (01 = 01_train_pinn_multiphysics_model.py), optionally stores their per-row tuples, and
// reduces every sum the five physics-parameter trainers need (stage loss + analytic
// d loss / d lambda) with wave64 shuffles -> LDS -> one partial per workgroup,
// finished by a fixed-order second kernel (bitwise reproducible, no float atomics).
//
// This file holds the kernels and the entry points.  The models themselves (the de-normalised row, each model's
// parameter-independent and parameter-dependent part, its accumulation, the Euler step of net_f_T) and the two reductions
// (block_sums, sums_finalize) are stated once in pinn_physics.h; the one-pass kernel, the cached stage passes, the persistent
// stage kernel and both backwards are assembled from those pieces, so they cannot disagree on a formula.
//
// Compiled with -ffp-contract=off: every float op here and in pinn_physics.h is rounded exactly like the
// reference's separate torch ops, so only the transcendental calls can differ (<= 2 ulp).
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>
#include "../../include/pinn_hip.h"
#include "pinn_physics.h"
#include "pinn_rows.h"

namespace {

using pinn::clear_error;
using pinn::launch_status;

constexpr int kThreads = 256;

// every term one row contributes: load -> parameter-independent part -> parameter-dependent part with its sums -> optional columns
template <bool kCols>
__device__ __forceinline__ void row_terms(long long row, const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ y,
                                          const AffineDev& aff, const LamDev& L, unsigned flags, float* __restrict__ cols, long long ld,
                                          float (&acc)[PINN_NSUMS]) {
  const RowPhys r = load_row(x, row, aff, flags);
  const float yv = (y != nullptr) ? y[row] : 0.0f;
  const Current cur = current_of(r.r0);

  if (flags & PINN_RES_V) {
    const float un = u[row];
    const VoltPre p = volt_pre(r, cur.i5, un, aff, L.P_H2O);
    const VoltTerms t = volt_terms(p, L, y != nullptr, yv, un, aff, acc);
    if (kCols) {
      cols[PINN_C_FV * ld + row] = t.f;
      cols[PINN_C_VACT * ld + row] = t.V_act;
      cols[PINN_C_VOHM * ld + row] = t.V_ohm;
      cols[PINN_C_VCONC * ld + row] = t.V_conc;
      cols[PINN_C_ENERNST * ld + row] = p.E;
      cols[PINN_C_VEST5 * ld + row] = t.V_est5;
      cols[PINN_C_I * ld + row] = p.i5;
      cols[PINN_C_VOUT5 * ld + row] = p.V_out * 5.0f;
    }
  }

  if (flags & PINN_RES_T) {
    const ThermPre p = therm_pre(r);
    const ThermTerms t = therm_terms(p, L, acc);
    if (kCols) {
      cols[PINN_C_FT * ld + row] = t.f;
      cols[PINN_C_TPRED * ld + row] = t.T_pred;
      cols[PINN_C_TOUT * ld + row] = p.T_out;
    }
  }

  if (flags & PINN_RES_H) {
    const FlowPre p = hydrogen_pre(cur.It, r.r6);
    const FlowTerms t = hydrogen_terms(p, L, acc);
    if (kCols) {
      cols[PINN_C_FH * ld + row] = t.f;
      cols[PINN_C_ACTH * ld + row] = p.act;
      cols[PINN_C_TGTH * ld + row] = t.tgt;
      cols[PINN_C_ITOT * ld + row] = p.It;
    }
  }

  if (flags & PINN_RES_O) {
    const FlowPre p = oxygen_pre(cur.It, r.r7);
    const FlowTerms t = oxygen_terms(p, L, acc);
    if (kCols) {
      cols[PINN_C_FO * ld + row] = t.f;
      cols[PINN_C_ACTO * ld + row] = p.act;
      cols[PINN_C_TGTO * ld + row] = t.tgt;
      cols[PINN_C_QO2 * ld + row] = p.Q;
      cols[PINN_C_O2FLOW * ld + row] = p.o2;
    }
  }
}

// kFlags: the one stage model of the call as a constant (its terms and sums alone exist), or 0: `flags` at run time, any combination
template <bool kCols, unsigned kFlags>
__global__ __launch_bounds__(kThreads) void residuals_kernel(
    const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ y, AffineDev aff,
    const float* __restrict__ lambdas, unsigned flags_rt, long long n_rows, float* __restrict__ cols, long long ld,
    double* __restrict__ partials) {
  const unsigned flags = kFlags ? kFlags : flags_rt;
  const LamDev L = load_lambdas(lambdas);
  float acc[PINN_NSUMS];
#pragma unroll
  for (int s = 0; s < PINN_NSUMS; ++s) acc[s] = 0.0f;

  const long long stride = (long long)gridDim.x * kThreads;
  for (long long row = (long long)blockIdx.x * kThreads + threadIdx.x; row < n_rows; row += stride)
    row_terms<kCols>(row, x, u, y, aff, L, flags, cols, ld, acc);

  if (partials == nullptr) return;
  block_sums<live_sums(kFlags).lo, live_sums(kFlags).hi, kThreads>(acc, partials + (long long)blockIdx.x * PINN_NSUMS);
}

// Adam (torch defaults) + clamp for the <= 5 scalars of a physics stage, one thread.
struct StageDef {
  int n;
  int idx[5];
  float lo[5], hi[5];
};

// bc1 = 1 - 0.9^step, bc2 = 1 - 0.999^step (torch computes them in double)
// (forceinline: in the persistent kernel `stage` is a compile-time constant per instantiation, so the parameter table, the
//  loops over it and the gradient arrays dissolve into registers; as a called function they lived in scratch)
__device__ __forceinline__ void lambda_step_body(int stage, const double* sums, double inv_n, float vn_scale, float lr, double bc1, double bc2, float* lambdas,
                                 float* adam, float* loss_out) {
  StageDef d;
  float g[5];
  bool has_grad[5];
  float total = 0.f, physics = 0.f;
  if (stage == PINN_STAGE_LAMBDA_PM || stage == PINN_STAGE_LAMBDA_F) {
    // 01:992-997 bounds; lambda_4 is in the optimizer but never receives a gradient
    d.n = 4;
    d.idx[0] = PINN_L1; d.idx[1] = PINN_L2; d.idx[2] = PINN_L3; d.idx[3] = PINN_L4;
    d.lo[0] = (float)(0.167 * 0.5); d.hi[0] = (float)(0.167 * 5);
    d.lo[1] = (float)(2.36e-6 * 0.1); d.hi[1] = (float)(2.36e-6 * 2.1);
    d.lo[2] = 2.0f; d.hi[2] = (float)(2.0 * 5.2);
    d.lo[3] = 0.1f; d.hi[3] = 10.0f;
    has_grad[3] = false; g[3] = 0.f;
    if (stage == PINN_STAGE_LAMBDA_F) {
      physics = (float)(sums[PINN_S_FV2] * inv_n);
      for (int k = 0; k < 3; ++k) { g[k] = (float)(2.0 * sums[PINN_S_FV_D1 + k] * inv_n); has_grad[k] = true; }
    } else {
      physics = (float)(sums[PINN_S_YV2] * inv_n);
      // d/dlambda mean((y - (5 V_est s + m))^2) = -(2/N) * 5 s * sum (y - Vn) df/dlambda
      for (int k = 0; k < 3; ++k) {
        g[k] = (float)(-2.0 * 5.0 * (double)vn_scale * sums[PINN_S_YV_D1 + k] * inv_n);
        has_grad[k] = true;
      }
    }
    total = physics + (float)(sums[PINN_S_YU2] * inv_n);
  } else if (stage == PINN_STAGE_THERMAL) {
    d.n = 5;
    for (int k = 0; k < 5; ++k) { d.idx[k] = PINN_LT1 + k; d.lo[k] = -10000.f; d.hi[k] = 10000.f; has_grad[k] = false; g[k] = 0.f; }
    g[0] = (float)(2.0 * sums[PINN_S_FT_D1] * inv_n); has_grad[0] = true;
    g[2] = (float)(2.0 * sums[PINN_S_FT_D3] * inv_n); has_grad[2] = true;
    g[4] = (float)(2.0 * sums[PINN_S_FT_D5] * inv_n); has_grad[4] = true;
    total = physics = (float)(sums[PINN_S_FT2] * inv_n);
  } else if (stage == PINN_STAGE_HYDROGEN) {
    d.n = 4;
    for (int k = 0; k < 4; ++k) d.idx[k] = PINN_LH1 + k;
    d.lo[0] = 0.5f; d.hi[0] = 50.f; d.lo[1] = -20.f; d.hi[1] = 20.f; d.lo[2] = 50.f; d.hi[2] = 1000.f; d.lo[3] = 0.f; d.hi[3] = 20.f;
    for (int k = 0; k < 3; ++k) { g[k] = (float)(2.0 * sums[PINN_S_FH_D1 + k] * inv_n); has_grad[k] = true; }
    has_grad[3] = false; g[3] = 0.f;
    total = physics = (float)(sums[PINN_S_FH2] * inv_n);
  } else {
    d.n = 4;
    for (int k = 0; k < 4; ++k) d.idx[k] = PINN_LO1 + k;
    d.lo[0] = 1.5f; d.hi[0] = 8.f; d.lo[1] = -20.f; d.hi[1] = 20.f; d.lo[2] = 50.f; d.hi[2] = 1000.f; d.lo[3] = 0.f; d.hi[3] = 20.f;
    for (int k = 0; k < 3; ++k) { g[k] = (float)(2.0 * sums[PINN_S_FO_D1 + k] * inv_n); has_grad[k] = true; }
    has_grad[3] = false; g[3] = 0.f;
    total = physics = (float)(sums[PINN_S_FO2] * inv_n);
  }
  // torch.optim.Adam (single tensor path): bias corrections in double, tensor math in float32
  const float step_size = (float)((double)lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if (k >= d.n) break;
    const int id = d.idx[k];
    float p = lambdas[id];
    if (has_grad[k]) {          // a parameter whose .grad is None is skipped entirely
      float m = adam[id], v = adam[PINN_NLAMBDA + id];
      m = m * 0.9f + g[k] * 0.1f;                          // lerp(m, g, 1-b1)
      v = v * 0.999f + (g[k] * g[k]) * 0.001f;
      const float denom = sqrtf(v) / bc2_sqrt + 1e-8f;
      p = p - step_size * (m / denom);
      adam[id] = m; adam[PINN_NLAMBDA + id] = v;
    }
    lambdas[id] = clamp_t(p, d.lo[k], d.hi[k]);       // .data = clamp(.data, lo, hi) AFTER step
  }
  if (loss_out) { loss_out[0] = total; loss_out[1] = physics; }
}

__global__ void lambda_step_kernel(int stage, const double* __restrict__ sums, double inv_n, float vn_scale, float lr,
                                   int step, float* __restrict__ lambdas, float* __restrict__ adam,
                                   float* __restrict__ loss_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  lambda_step_body(stage, sums, inv_n, vn_scale, lr, 1.0 - pow(0.9, (double)step), 1.0 - pow(0.999, (double)step), lambdas, adam, loss_out);
}

// ---------------------------------------------------------------------------------------
// Persistent stage driver: a physics-parameter stage is thousands of strictly sequential
// iterations of "residual pass over all rows -> <= 5 scalar gradients -> Adam -> clamp" (01:1008-1055, 1107-1151,
// 1204-1274, 1354-1391; 46 007 iterations in the reference schedule).  At the reference's data sizes (1e3 - 1e4
// rows) three launches per iteration are pure launch latency (~21 us / iteration); here ONE workgroup of 1024
// threads runs all iterations of a stage: rows from L2, sums in LDS (double, fixed order), StepLR / Adam / clamp by
// thread 0 on the LDS copy of the parameters, a log row every `log_every` epochs.
// ---------------------------------------------------------------------------------------
constexpr int kStageThreads = 1024;
constexpr int kLogFloats = PINN_STAGE_LOG_FLOATS;   // [0..1] total / physics loss, [2] lr of the next epoch, [3..19] lambdas, [20..51] sums
constexpr int kCacheFloats = 6;
// how many of them a stage model fills (stage_prepare): the rest of a row's slots is never read
constexpr int cached_floats(unsigned flags) { return (flags & PINN_RES_V) ? 6 : ((flags & PINN_RES_T) ? 4 : 2); }

// Everything of a row that does not depend on the stage's parameters is computed ONCE (the de-normalisation with its
// float64 divides, powf / expf of the Nernst terms, the flow ratios): 6 floats per row, struct-of-arrays in d_work.
// stage_prepare packs the *_pre part of the one stage model, stage_terms unpacks it and runs the *_terms part: the functions
// row_terms runs back to back, so the two paths differ only in the order of the row sums.
//   V: i5, b, E, V_out, y, u    T: It6, mc, T_in, T_out    H, O: It, act
__device__ __forceinline__ void stage_prepare(long long row, const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ y,
                                              const AffineDev& aff, float P_H2O, unsigned flags, float (&c)[kCacheFloats]) {
  const RowPhys r = load_row(x, row, aff, flags);
  const Current cur = current_of(r.r0);
#pragma unroll
  for (int k = 0; k < kCacheFloats; ++k) c[k] = 0.0f;
  if (flags & PINN_RES_V) {
    const float un = u[row];
    const VoltPre p = volt_pre(r, cur.i5, un, aff, P_H2O);
    c[0] = p.i5; c[1] = p.b; c[2] = p.E; c[3] = p.V_out;
    c[4] = y[row];
    c[5] = un;
  } else if (flags & PINN_RES_T) {
    const ThermPre p = therm_pre(r);
    c[0] = p.It6; c[1] = p.mc; c[2] = p.T_in; c[3] = p.T_out;
  } else if (flags & PINN_RES_H) {
    const FlowPre p = hydrogen_pre(cur.It, r.r6);
    c[0] = p.It; c[1] = p.act;
  } else {
    const FlowPre p = oxygen_pre(cur.It, r.r7);
    c[0] = p.It; c[1] = p.act;
  }
}
// the parameter-dependent rest with its sums (the cached passes require y)
__device__ __forceinline__ void stage_terms(const float (&c)[kCacheFloats], const AffineDev& aff, const LamDev& L, unsigned flags,
                                            float (&acc)[PINN_NSUMS]) {
  if (flags & PINN_RES_V) {
    VoltPre p;
    p.i5 = c[0]; p.b = c[1]; p.E = c[2]; p.V_out = c[3];
    volt_terms(p, L, true, c[4], c[5], aff, acc);
  } else if (flags & PINN_RES_T) {
    ThermPre p;
    p.It6 = c[0]; p.mc = c[1]; p.T_in = c[2]; p.T_out = c[3];
    therm_terms(p, L, acc);
  } else {
    FlowPre p;
    p.It = c[0]; p.act = c[1]; p.Qp = p.Q = p.o2 = 0.0f;   // (not part of the cache: only columns and the backward read them)
    if (flags & PINN_RES_H) hydrogen_terms(p, L, acc);
    else oxygen_terms(p, L, acc);
  }
}

// One instantiation per stage kind: with the flags a constant only that stage's sums, cache columns and parameters exist (as
// one kernel with run-time flags it held all 32 accumulators per thread: 128 registers, 28 of them spilled, 144 B of scratch
// per lane touched in every iteration).
template <unsigned kFlags>
__global__ __launch_bounds__(kStageThreads) void stage_run_kernel(
    int stage_rt, const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ y, AffineDev aff,
    long long n_rows, double lr0, double gamma, int lr_step, int first_epoch, int n_iters, float* __restrict__ lambdas,
    float* __restrict__ adam, float* __restrict__ loss_out, float* __restrict__ log, int log_every, double* __restrict__ sums_out,
    float* __restrict__ work) {
  __shared__ double sums[PINN_NSUMS];
  __shared__ float lam_s[PINN_NLAMBDA], adam_s[2 * PINN_NLAMBDA], loss_s[2];
  constexpr unsigned flags = kFlags;
  // (the voltage stage has two variants, chosen at run time; the others are fixed by the flags)
  const int stage = kFlags == PINN_RES_T ? PINN_STAGE_THERMAL : (kFlags == PINN_RES_H ? PINN_STAGE_HYDROGEN : (kFlags == PINN_RES_O ? PINN_STAGE_OXYGEN
                    : (stage_rt == PINN_STAGE_LAMBDA_F ? PINN_STAGE_LAMBDA_F : PINN_STAGE_LAMBDA_PM)));
  const int tid = threadIdx.x;
  if (tid < PINN_NLAMBDA) lam_s[tid] = lambdas[tid];
  if (tid < 2 * PINN_NLAMBDA) adam_s[tid] = adam[tid];
  if (tid < PINN_NSUMS) sums[tid] = 0.0;
  {   // parameter-independent part of every row, once
    const LamDev L0 = load_lambdas(lambdas);
    for (long long row = tid; row < n_rows; row += kStageThreads) {
      float c[kCacheFloats];
      stage_prepare(row, x, u, y, aff, L0.P_H2O, flags, c);
#pragma unroll
      for (int k = 0; k < kCacheFloats; ++k) work[k * n_rows + row] = c[k];
    }
  }
  __syncthreads();
  constexpr int n_cached = cached_floats(kFlags);
  const double inv_n = 1.0 / (double)n_rows;
  // thread 0's optimizer state: beta^step as running products (pow() once), the StepLR rate recomputed at its edges
  double b1p = pow(0.9, (double)first_epoch), b2p = pow(0.999, (double)first_epoch);
  float lr = (float)(lr0 * pow(gamma, (double)(first_epoch / lr_step)));
  for (int it = 0; it < n_iters; ++it) {
    const int epoch = first_epoch + it;
    const LamDev L = load_lambdas(lam_s);
    float acc[PINN_NSUMS];
#pragma unroll
    for (int s = 0; s < PINN_NSUMS; ++s) acc[s] = 0.0f;
    // several rows per trip: their (L2) loads are all in flight before the first is used (the voltage stage, six cached floats
    // and nine sums per row, has registers for two; the others for four)
    constexpr int kTrip = (kFlags & PINN_RES_V) ? 2 : 4;
    for (long long row0 = tid; row0 < n_rows; row0 += kTrip * kStageThreads) {
      float c[kTrip][kCacheFloats];
#pragma unroll
      for (int q = 0; q < kTrip; ++q) {
        const long long row = row0 + q * kStageThreads;
        const long long rr = row < n_rows ? row : row0;
#pragma unroll
        for (int k = 0; k < kCacheFloats; ++k) c[q][k] = k < n_cached ? work[k * n_rows + rr] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < kTrip; ++q)
        if (row0 + q * kStageThreads < n_rows) stage_terms(c[q], aff, L, flags, acc);
    }
    block_sums<live_sums(kFlags).lo, live_sums(kFlags).hi, kStageThreads>(acc, sums);   // the sums this stage reads; the rest stay 0
    __syncthreads();
    if (tid == 0) {
      if (it > 0 && epoch % lr_step == 0) lr = (float)(lr0 * pow(gamma, (double)(epoch / lr_step)));
      b1p *= 0.9; b2p *= 0.999;
      lambda_step_body(stage, sums, inv_n, aff.vn_scale, lr, 1.0 - b1p, 1.0 - b2p, lam_s, adam_s, loss_s);
      if (log && log_every > 0 && epoch % log_every == 0) {
        float* row = log + (long long)(epoch / log_every - first_epoch / log_every) * kLogFloats;
        row[0] = loss_s[0]; row[1] = loss_s[1];
        row[2] = (float)(lr0 * pow(gamma, (double)((epoch + 1) / lr_step)));
        for (int k = 0; k < PINN_NLAMBDA; ++k) row[3 + k] = lam_s[k];
        for (int k = 0; k < PINN_NSUMS; ++k) row[20 + k] = (float)sums[k];
      }
    }
    __syncthreads();
  }
  if (tid < PINN_NLAMBDA) lambdas[tid] = lam_s[tid];
  if (tid < 2 * PINN_NLAMBDA) adam[tid] = adam_s[tid];
  if (tid < 2 && loss_out) loss_out[tid] = loss_s[tid];
  if (tid < PINN_NSUMS && sums_out) sums_out[tid] = sums[tid];
}

// ---------------------------------------------------------------------------------------
// The same split for any row count / several processes: the parameter-independent row cache once per trainer call
// (pinn_residuals_prepare), then per iteration one pass over the 8 - 24 B/row cache instead of the 40 B/row inputs and
// their float64 de-normalisation, powf / expf (pinn_residuals_cached).  Sums come out in pinn_residuals' layout.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void stage_prepare_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                                 const float* __restrict__ y, AffineDev aff,
                                                                 const float* __restrict__ lambdas, unsigned flags, long long n_rows,
                                                                 float* __restrict__ cache) {
  const LamDev L0 = load_lambdas(lambdas);
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long row = (long long)blockIdx.x * kThreads + threadIdx.x; row < n_rows; row += stride) {
    float c[kCacheFloats];
    stage_prepare(row, x, u, y, aff, L0.P_H2O, flags, c);
#pragma unroll
    for (int k = 0; k < kCacheFloats; ++k) cache[k * n_rows + row] = c[k];
  }
}

// One instantiation per stage kind, as the persistent kernel: only that stage's cache columns, terms and sums exist, and only its
// range of sums is reduced and stored.  (With run-time flags every workgroup shuffled, staged and stored all 32 sums, at most
// nine of them other than zero: the epilogue, not the 8 - 24 B/row of loads, set the time at 1e6 rows.)  Grid, rows per thread
// and every order of summation are those of the run-time form, so each sum keeps its bits.
template <unsigned kFlags>
__global__ __launch_bounds__(kThreads) void residuals_cached_kernel(const float* __restrict__ cache, AffineDev aff,
                                                                    const float* __restrict__ lambdas, long long n_rows,
                                                                    double* __restrict__ partials) {
  const LamDev L = load_lambdas(lambdas);
  constexpr int n_cached = cached_floats(kFlags);
  float acc[PINN_NSUMS];
#pragma unroll
  for (int s = 0; s < PINN_NSUMS; ++s) acc[s] = 0.0f;
  const long long stride = (long long)gridDim.x * kThreads;
  // two rows per trip: both rows' loads in flight before the first is used
  for (long long row0 = (long long)blockIdx.x * kThreads + threadIdx.x; row0 < n_rows; row0 += 2 * stride) {
    float c[2][kCacheFloats];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const long long row = row0 + q * stride;
      const long long rr = row < n_rows ? row : row0;
#pragma unroll
      for (int k = 0; k < kCacheFloats; ++k) c[q][k] = k < n_cached ? cache[k * n_rows + rr] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (row0 + q * stride < n_rows) stage_terms(c[q], aff, L, kFlags, acc);
  }
  block_sums<live_sums(kFlags).lo, live_sums(kFlags).hi, kThreads>(acc, partials + (long long)blockIdx.x * PINN_NSUMS);
}

static AffineDev affine_dev(const pinn_affine_t* aff) {
  AffineDev a;
  for (int c = 0; c < 8; ++c) { a.x_min[c] = aff->x_min[c]; a.x_scale[c] = aff->x_scale[c]; }
  a.y_min = aff->y_min; a.y_scale = aff->y_scale; a.vn_scale = aff->vn_scale; a.vn_min = aff->vn_min;
  return a;
}
static int row_blocks(long long n_rows) { return pinn::row_blocks(n_rows, kThreads, kMaxBlocks); }
static bool one_stage_flag(unsigned flags) { return flags == PINN_RES_V || flags == PINN_RES_T || flags == PINN_RES_H || flags == PINN_RES_O; }

// The run-time stage flag as a template argument, written once for every kernel that is instantiated per stage model: calls
// fn(std::integral_constant<unsigned, F>) for the one-stage flag F and returns true; any other value calls nothing and returns false.
template <typename Fn>
static bool with_stage_flag(unsigned flags, Fn&& fn) {
  switch (flags) {
    case PINN_RES_V: fn(std::integral_constant<unsigned, PINN_RES_V>{}); return true;
    case PINN_RES_T: fn(std::integral_constant<unsigned, PINN_RES_T>{}); return true;
    case PINN_RES_H: fn(std::integral_constant<unsigned, PINN_RES_H>{}); return true;
    case PINN_RES_O: fn(std::integral_constant<unsigned, PINN_RES_O>{}); return true;
    default: return false;
  }
}

// ---------------------------------------------------------------------------------------
// net_f_T (01:767-867): the Euler energy balance row t-1 -> t.  Row t reads the de-normalised current, coolant flow,
// inlet and outlet temperature and the DNN's eval-mode voltage of row t - 1 (a halo of ONE row: under row sharding the
// caller passes the last row of the previous shard as x_halo / u_halo) and its own outlet temperature; the step itself is
// euler_step of pinn_physics.h, which the backward shares:
//   T_pred[t] = T_out[t-1] + ((Q_el - Q_cool - Q_rad) / lT2) 0.1;   T_pred[0] = T_out[0] (01:857);   f = T_out - T_pred
// every float op rounded separately, in the reference's order (this file is built with -ffp-contract=off).
// 32 B/row + 4 B/row (u) read -- the previous row's line is an L1/L2 hit --, 12 B/row written: HBM-bound.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void net_f_T_kernel(const float* __restrict__ x, const float* __restrict__ u,
                                                           const float* __restrict__ x_halo, const float* __restrict__ u_halo, AffineDev aff,
                                                           const float* __restrict__ lambdas, long long n_rows, float* __restrict__ f_out,
                                                           float* __restrict__ t_pred, float* __restrict__ t_real) {
  const float lT1 = lambdas[PINN_LT1], lT2 = lambdas[PINN_LT2], lT3 = lambdas[PINN_LT3], lT4 = lambdas[PINN_LT4];
  for (long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x; row < n_rows; row += (long long)gridDim.x * blockDim.x) {
    const float T_out = denorm(x[row * 8 + 5], aff.x_min[5], aff.x_scale[5]);
    float pred = T_out;                                      // first row of the series (01:857)
    const float* xp = row > 0 ? x + (row - 1) * 8 : x_halo;
    if (xp != nullptr) {
      const float4 pa = reinterpret_cast<const float4*>(xp)[0];
      const float4 pb = reinterpret_cast<const float4*>(xp)[1];
      const float un = row > 0 ? u[row - 1] : u_halo[0];
      const EulerFwd e = euler_step(pa, pb, un, aff, lT1, lT2, lT3, lT4);
      pred = e.T_prev + e.dT * 0.1f;
    }
    f_out[row] = T_out - pred;
    t_pred[row] = pred;
    t_real[row] = T_out;
  }
}

// ---------------------------------------------------------------------------------------
// Vector-Jacobian products of the two passes above (torch autograd's backward of the oracle's restatement of 01:535-914).
// Nothing is saved between the calls: every row's terms are recomputed from x, u and the parameters by the forward's own
// functions (pinn_physics.h, each called inside the guard of the node that needs it), then back-propagated op by op in the order torch's
// derivative formulas use: a / b -> (g / b, -g * ((a / b) / b)), log -> g / x, exp -> g * exp(x), pow -> g * p x^(p-1),
// clamp -> inclusive mask, where -> nothing through the condition, abs -> sign.  A node is visited only when an upstream
// column that reaches it is present (gmask), so NaN rows (I >= lambda_3: log of a negative number) give NaN exactly where
// torch's autograd does.  Gradients with respect to the de-normalised inputs become gradients of the normalised ones by
// the chain rule of x_phys = (x_n - x_min) / x_scale.  Parameter gradients: float64 per thread, wave64 shuffle -> LDS ->
// one partial per workgroup -> a fixed-order final reduction (no float atomics: bitwise repeatable).
// ---------------------------------------------------------------------------------------
#define PINN_BIT(c) (1u << (c))
constexpr unsigned kGradColsV = PINN_BIT(PINN_C_FV) | PINN_BIT(PINN_C_VACT) | PINN_BIT(PINN_C_VOHM) | PINN_BIT(PINN_C_VCONC) |
                                PINN_BIT(PINN_C_ENERNST) | PINN_BIT(PINN_C_VEST5) | PINN_BIT(PINN_C_I) | PINN_BIT(PINN_C_VOUT5);
constexpr unsigned kGradColsT = PINN_BIT(PINN_C_FT) | PINN_BIT(PINN_C_TPRED) | PINN_BIT(PINN_C_TOUT);
constexpr unsigned kGradColsH = PINN_BIT(PINN_C_FH) | PINN_BIT(PINN_C_ACTH) | PINN_BIT(PINN_C_TGTH) | PINN_BIT(PINN_C_ITOT);
constexpr unsigned kGradColsO = PINN_BIT(PINN_C_FO) | PINN_BIT(PINN_C_ACTO) | PINN_BIT(PINN_C_TGTO) | PINN_BIT(PINN_C_QO2) |
                                PINN_BIT(PINN_C_O2FLOW);

__host__ __device__ inline unsigned grad_cols_of(unsigned flags) {
  return ((flags & PINN_RES_V) ? kGradColsV : 0u) | ((flags & PINN_RES_T) ? kGradColsT : 0u) | ((flags & PINN_RES_H) ? kGradColsH : 0u) |
         ((flags & PINN_RES_O) ? kGradColsO : 0u);
}

// one row: accumulates the parameter gradients into acc, returns d/d x_phys in gr[8] and d/d u in gu
__device__ __forceinline__ void row_backward(long long row, const float* __restrict__ x, const float* __restrict__ u, const AffineDev& aff,
                                             const LamDev& L, unsigned flags, const float* __restrict__ g, long long ld, unsigned gmask,
                                             double (&acc)[PINN_NLAMBDA], float (&gr)[8], float& gu) {
  const bool fV = flags & PINN_RES_V, fT = flags & PINN_RES_T, fH = flags & PINN_RES_H, fO = flags & PINN_RES_O;
  const RowPhys r = load_row(x, row, aff, flags);
#pragma unroll
  for (int c = 0; c < 8; ++c) gr[c] = 0.0f;
  gu = 0.0f;
  // upstream gradient of column c (absent columns are not read; gmask is wave-uniform)
  auto G = [&](int c) -> float { return (gmask & PINN_BIT(c)) ? g[(long long)c * ld + row] : 0.0f; };
  auto has = [&](unsigned bits) -> bool { return (gmask & bits) != 0u; };

  const Current cur = current_of(r.r0);
  const float i5 = cur.i5, It = cur.It;
  float gi5 = 0.0f;  // d / d i5 of the V, H and O models (T_simple has its own i = I/270 + 1e-6)

  if (fV) {
    const float gFV = G(PINN_C_FV), gVest = gFV + G(PINN_C_VEST5) * 5.0f;
    const float l1 = L.l1, l2 = L.l2, l3 = L.l3;
    float gi = G(PINN_C_I), gb = 0.0f, gTk = 0.0f;
    const float Tk = kelvin(r.r5);
    const ThermalVoltage tv = thermal_voltage(Tk);
    const float RT = tv.RT, b = tv.b;
    if (has(PINN_BIT(PINN_C_FV) | PINN_BIT(PINN_C_VEST5) | PINN_BIT(PINN_C_VACT))) {      // V_act = (-b) log(i / l2)
      const float gA = gVest + G(PINN_C_VACT);
      const float q = i5 / l2, La = logf(q);
      gb -= gA * La;
      const float gq = (gA * (-b)) / q;
      gi += gq / l2;
      acc[PINN_L2] += (double)(-gq * (q / l2));
    }
    if (has(PINN_BIT(PINN_C_FV) | PINN_BIT(PINN_C_VEST5) | PINN_BIT(PINN_C_VOHM))) {      // V_ohm = -(i l1)
      const float gp = -(gVest + G(PINN_C_VOHM));
      gi += gp * l1;
      acc[PINN_L1] += (double)(gp * i5);
    }
    if (has(PINN_BIT(PINN_C_FV) | PINN_BIT(PINN_C_VEST5) | PINN_BIT(PINN_C_VCONC))) {     // V_conc = (0.5 b) log(1 - i / l3)
      const float gC = gVest + G(PINN_C_VCONC);
      const float t = i5 / l3, w = 1.0f - t, Lc = logf(w);
      gb += (gC * Lc) * 0.5f;
      const float gt = -((gC * (0.5f * b)) / w);
      gi += gt / l3;
      acc[PINN_L3] += (double)(-gt * (t / l3));
    }
    if (has(PINN_BIT(PINN_C_FV) | PINN_BIT(PINN_C_VEST5) | PINN_BIT(PINN_C_ENERNST))) {   // E = c - (RT log(P_H2O / (pp_H2 sqrt(pp_O2)))) / 192970
      const float gE = gVest + G(PINN_C_ENERNST);
      const Nernst n = nernst_pressures(i5, Tk, r.r3, r.r4, L.P_H2O);
      const float Tk_p = n.Tk_p, a1 = n.a1, e1 = n.e1, q1 = n.q1, pp_H2 = n.pp_H2, a2 = n.a2, e2 = n.e2, q2 = n.q2, pp_O2 = n.pp_O2;
      const float s = sqrtf(pp_O2), D = pp_H2 * s, z = L.P_H2O / D, LE = logf(z);
      const float gnum = (-gE) / 192970.0f;
      gTk += (gnum * LE) * 8.314f;
      const float gz = (gnum * RT) / z;
      const float gD = -gz * (z / D);
      const float gpp1 = gD * s, gs = gD * pp_H2;
      const float gpp2 = gs * (0.5f / s);                   // pow(x, 0.5) -> g 0.5 x^-0.5
      const float ge2 = -gpp2 * (q2 / e2), ga2 = ge2 * e2;
      const float gin = gpp1 * 0.5f;
      const float ge1 = -gin * (q1 / e1), ga1 = ge1 * e1;
      gi += (ga2 / Tk_p) * 4.192f + (ga1 / Tk_p) * 1.653f;
      const float gTkp = -ga2 * (a2 / Tk_p) - ga1 * (a1 / Tk_p);
      gTk += gTkp * (1.334f * powf(Tk, 0.334f));
      gr[3] += (gin / e1) / 101.0f;
      gr[4] += (gpp2 / e2) / 101.0f;
    }
    gTk += (gb / 96485.0f) * 8.314f;
    gr[5] += gTk;
    gi5 += gi;
    // V_out = denorm(u) / 5 (the caller's DNN output; VOUT5 = 5 V_out)
    const float gVout = G(PINN_C_VOUT5) * 5.0f - gFV;
    gu = (float)((double)(gVout / 5.0f) / aff.y_scale);
  }

  if (fT) {
    const float gF = G(PINN_C_FT);
    gr[5] += gF + G(PINN_C_TOUT);
    if (has(PINN_BIT(PINN_C_FT) | PINN_BIT(PINN_C_TPRED))) {    // T_pred = lT1 I + lT3 (m + 1e-6) + 0.5 T_in + lT5
      const float gP = G(PINN_C_TPRED) - gF;
      const ThermPre p = therm_pre(r);
      acc[PINN_LT1] += (double)(gP * p.It6);
      acc[PINN_LT3] += (double)(gP * p.mc);
      acc[PINN_LT5] += (double)gP;
      gr[0] += ((gP * L.lT1) * 270.0f) / 270.0f;
      gr[1] += gP * L.lT3;
      gr[2] += gP * 0.5f;
    }
  }

  if (fH) {
    const float gF = G(PINN_C_FH);
    float gIt = G(PINN_C_ITOT);
    if (has(PINN_BIT(PINN_C_FH) | PINN_BIT(PINN_C_ACTH))) {     // act = (h2 + 1e-6) / clamp_min(Q, 1e-8)
      const float ga = gF + G(PINN_C_ACTH);
      const FlowPre p = hydrogen_pre(It, r.r6);
      const float Qp = p.Qp, Q = p.Q, act = p.act;
      gr[6] += ga / Q;
      const float gQ = -ga * (act / Q);
      const float gQp = (Qp >= 1e-8f) ? gQ : 0.0f;
      gIt += (((gQp * 60.0f) * 22.4f) * 5.0f) / 192970.0f;
    }
    if (has(PINN_BIT(PINN_C_FH) | PINN_BIT(PINN_C_TGTH))) {     // target = where(It <= lH3, lH1 + lH2 It / 100, lH1 + lH2 lH3 / 100)
      const float gt = G(PINN_C_TGTH) - gF;
      acc[PINN_LH1] += (double)gt;
      if (hydrogen_target(It, L).lin) {
        acc[PINN_LH2] += (double)(gt * (It / 100.0f));
        gIt += (gt * L.lH2) / 100.0f;
      } else {
        acc[PINN_LH2] += (double)(gt * (L.lH3 / 100.0f));
        acc[PINN_LH3] += (double)((gt * L.lH2) / 100.0f);
      }
    }
    gi5 += gIt * 270.0f;
  }

  if (fO) {
    const float gF = G(PINN_C_FO);
    float gIt = 0.0f;
    const bool pAct = has(PINN_BIT(PINN_C_FO) | PINN_BIT(PINN_C_ACTO));
    if (pAct || has(PINN_BIT(PINN_C_QO2) | PINN_BIT(PINN_C_O2FLOW))) {
      const FlowPre p = oxygen_pre(It, r.r7);
      const float Qp = p.Qp, Q = p.Q;
      float gQ = G(PINN_C_QO2), go2 = G(PINN_C_O2FLOW);
      if (pAct) {                                               // f = (act - tgt) + clamp_min(1 - act, 0) 10,  act = o2 / Q
        const float act = p.act;
        float ga = gF + G(PINN_C_ACTO);
        if (gmask & PINN_BIT(PINN_C_FO)) ga -= ((1.0f - act) >= 0.0f) ? gF * 10.0f : 0.0f;
        go2 += ga / Q;
        gQ += -ga * (act / Q);
      }
      if (pAct || has(PINN_BIT(PINN_C_QO2))) {
        const float gQp = (Qp >= 1e-8f) ? gQ : 0.0f;
        gIt += (((gQp * 60.0f) * 22.4f) / 385940.0f) * 5.0f;
      }
      gr[7] += go2 * 0.21f;
    }
    if (has(PINN_BIT(PINN_C_FO) | PINN_BIT(PINN_C_TGTO))) {     // target = clamp(where(It <= |lO3|, ...), 1.05, 15)
      const float gt = G(PINN_C_TGTO) - gF;
      const Target tg = oxygen_target(It, L);
      const float thr = tg.thr, raw = tg.raw;
      const bool lin = tg.lin;
      const float gw = (raw >= 1.05f && raw <= 15.0f) ? gt : 0.0f;
      acc[PINN_LO1] += (double)gw;
      if (lin) {
        acc[PINN_LO2] += (double)(gw * (It / 100.0f));
        gIt += (gw * L.lO2) / 100.0f;
      } else {
        acc[PINN_LO2] += (double)(gw * (thr / 100.0f));
        const float sgn = (L.lO3 > 0.0f) ? 1.0f : ((L.lO3 < 0.0f) ? -1.0f : 0.0f);
        acc[PINN_LO3] += (double)(((gw * L.lO2) / 100.0f) * sgn);
      }
    }
    gi5 += gIt * 270.0f;
  }
  gr[0] += gi5 / 270.0f;
}

// d / d x_phys -> d / d x_n (x_phys = (x_n - x_min) / x_scale), one row of 8
__device__ __forceinline__ void store_gx_row(float* __restrict__ gx, long long row, const float (&gr)[8], const AffineDev& aff) {
  float o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = (float)((double)gr[c] / aff.x_scale[c]);
  reinterpret_cast<float4*>(gx)[row * 2] = make_float4(o[0], o[1], o[2], o[3]);
  reinterpret_cast<float4*>(gx)[row * 2 + 1] = make_float4(o[4], o[5], o[6], o[7]);
}

// (parameter gradients: float64 per thread -> partials[blockIdx.x * PINN_NSUMS + k], k < PINN_NLAMBDA, by block_sums)
__global__ __launch_bounds__(kThreads) void residuals_backward_kernel(
    const float* __restrict__ x, const float* __restrict__ u, AffineDev aff, const float* __restrict__ lambdas, unsigned flags,
    long long n_rows, const float* __restrict__ g, long long ld, unsigned gmask, float* __restrict__ gu_out, float* __restrict__ gx_out,
    double* __restrict__ partials) {
  const LamDev L = load_lambdas(lambdas);
  double acc[PINN_NLAMBDA];
#pragma unroll
  for (int k = 0; k < PINN_NLAMBDA; ++k) acc[k] = 0.0;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long row = (long long)blockIdx.x * kThreads + threadIdx.x; row < n_rows; row += stride) {
    float gr[8], gu;
    row_backward(row, x, u, aff, L, flags, g, ld, gmask, acc, gr, gu);
    if (gx_out != nullptr) store_gx_row(gx_out, row, gr, aff);
    if (gu_out != nullptr) gu_out[row] = gu;
  }
  block_sums<0, PINN_NLAMBDA, kThreads>(acc, partials + (long long)blockIdx.x * PINN_NSUMS);
}

// Backward of one Euler step t (net_f_T_kernel's arithmetic) with respect to its predecessor row p = t - 1 (or the halo):
// g = dL/dT_pred[t].  Returns d/d x_phys of p's columns 0, 1, 2, 5 and d/d u[p]; accumulates lambda_T1..T4.
struct EulerGrad { float g0, g1, g2, g5, gu; };
__device__ __forceinline__ EulerGrad euler_step_backward(float4 pa, float4 pb, float un, float g, const AffineDev& aff, float lT1, float lT2,
                                                         float lT3, float lT4, double (&acc)[PINN_NLAMBDA]) {
  const EulerFwd s = euler_step(pa, pb, un, aff, lT1, lT2, lT3, lT4);
  const float I_tot = s.I_tot, V_rev = s.V_rev, V_cell = s.V_cell, A = s.A, B = s.B, C = s.C, dTc = s.dTc, m_cool = s.m_cool, dT = s.dT;
  // T_pred = T_prev + dT 0.1
  float gTp = g;
  const float gdT = g * 0.1f;
  const float gnum = gdT / lT2;
  acc[PINN_LT2] += (double)(-gdT * (dT / lT2));
  const float gA = gnum * lT4;                     // Q_el = A lT4
  acc[PINN_LT4] += (double)(gnum * A);
  const float gI = gA * V_rev - gA * V_cell;
  gTp += (gA * I_tot) * -0.0009f;                  // V_rev = 1.229 - 0.0009 (Tk - 298.15)
  const float gVcell = -(gA * I_tot);
  const float gB = -gnum * lT1;                    // Q_cool = B lT1
  acc[PINN_LT1] += (double)(-gnum * B);
  const float gdTc = gB * (m_cool * 4180.0f);
  gTp += gdTc;
  const float gC = -gnum * lT3;                    // Q_rad = C lT3
  acc[PINN_LT3] += (double)(-gnum * C);
  gTp += gC * (20.0f * 0.2f);
  EulerGrad e;
  e.g0 = (gI * 270.0f) / 270.0f;
  e.g1 = (gB * dTc) * 4180.0f;
  e.g2 = -gdTc;
  e.g5 = gTp;
  e.gu = (float)((double)(gVcell / 5.0f) / aff.y_scale);
  return e;
}

// Thread r owns row r: its own T_out terms (f = T_out - T_pred, the T_out output, T_pred[0] = T_out[0] without a halo) and the
// step r + 1, whose gradient lands on row r (x[r], u[r]).  Global thread 0 also runs the halo step (row 0's predecessor).
__global__ __launch_bounds__(kThreads) void net_f_T_backward_kernel(
    const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ x_halo, const float* __restrict__ u_halo, AffineDev aff,
    const float* __restrict__ lambdas, long long n_rows, const float* __restrict__ gf, const float* __restrict__ gpred,
    const float* __restrict__ greal, float* __restrict__ gu_out, float* __restrict__ gx_out, float* __restrict__ gx_halo,
    float* __restrict__ gu_halo, double* __restrict__ partials) {
  const float lT1 = lambdas[PINN_LT1], lT2 = lambdas[PINN_LT2], lT3 = lambdas[PINN_LT3], lT4 = lambdas[PINN_LT4];
  double acc[PINN_NLAMBDA];
#pragma unroll
  for (int k = 0; k < PINN_NLAMBDA; ++k) acc[k] = 0.0;
  const bool step_path = gf != nullptr || gpred != nullptr;       // T_pred reached by an upstream gradient
  auto gp_at = [&](long long t) -> float { return (gpred ? gpred[t] : 0.0f) - (gf ? gf[t] : 0.0f); };
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long row = (long long)blockIdx.x * kThreads + threadIdx.x; row < n_rows; row += stride) {
    float gr[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) gr[c] = 0.0f;
    float gu = 0.0f;
    gr[5] = (gf ? gf[row] : 0.0f) + (greal ? greal[row] : 0.0f);
    if (row == 0 && x_halo == nullptr && step_path) gr[5] += gp_at(0);
    const float4 pa = reinterpret_cast<const float4*>(x)[row * 2];
    const float4 pb = reinterpret_cast<const float4*>(x)[row * 2 + 1];
    if (row + 1 < n_rows && step_path) {
      const EulerGrad e = euler_step_backward(pa, pb, u[row], gp_at(row + 1), aff, lT1, lT2, lT3, lT4, acc);
      gr[0] += e.g0; gr[1] += e.g1; gr[2] += e.g2; gr[5] += e.g5;
      gu = e.gu;
    }
    if (gx_out != nullptr) store_gx_row(gx_out, row, gr, aff);
    if (gu_out != nullptr) gu_out[row] = gu;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (gx_halo != nullptr || gu_halo != nullptr || x_halo != nullptr)) {
    float hr[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) hr[c] = 0.0f;
    float hu = 0.0f;
    if (x_halo != nullptr && n_rows > 0 && step_path) {
      const float4 pa = reinterpret_cast<const float4*>(x_halo)[0];
      const float4 pb = reinterpret_cast<const float4*>(x_halo)[1];
      const EulerGrad e = euler_step_backward(pa, pb, u_halo[0], gp_at(0), aff, lT1, lT2, lT3, lT4, acc);
      hr[0] = e.g0; hr[1] = e.g1; hr[2] = e.g2; hr[5] = e.g5;
      hu = e.gu;
    }
    if (gx_halo != nullptr) store_gx_row(gx_halo, 0, hr, aff);
    if (gu_halo != nullptr) gu_halo[0] = hu;
  }
  block_sums<0, PINN_NLAMBDA, kThreads>(acc, partials + (long long)blockIdx.x * PINN_NSUMS);
}

// the PINN_NLAMBDA parameter gradients of a backward from its workgroups' partials
static void launch_lambda_grad_finalize(const void* d_work, int blocks, float* d_glambda, hipStream_t st) {
  hipLaunchKernelGGL(sums_finalize<float>, dim3(1), dim3(1024), 0, st, (const double*)d_work, blocks, 0, PINN_NLAMBDA, d_glambda);
}

}  // namespace

extern "C" size_t pinn_residuals_workspace_bytes(void) { return (size_t)kMaxBlocks * PINN_NSUMS * sizeof(double); }

extern "C" int pinn_residuals(const float* d_x, const float* d_u, const float* d_y, const pinn_affine_t* aff,
                              const float* d_lambda, unsigned flags, long long n_rows, float* d_cols, long long ld,
                              double* d_sums, void* d_work, size_t work_bytes, void* stream) {
  if ((!d_x && n_rows > 0) || !aff || !d_lambda || n_rows < 0 || (flags & ~PINN_RES_ALL)) return PINN_E_ARG;
  if ((flags & PINN_RES_V) && !d_u && n_rows > 0) return PINN_E_ARG;
  if (d_cols && ld < n_rows) return PINN_E_ARG;
  if (d_sums && !d_work) return PINN_E_ARG;
  if (d_sums && work_bytes < pinn_residuals_workspace_bytes()) return PINN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  clear_error();   // drop a stale error left by another HIP user of this thread
  const AffineDev a = affine_dev(aff);
  const int blocks = row_blocks(n_rows);
  double* partials = d_sums ? (double*)d_work : nullptr;
  // the kernel's compile-time flags: the one stage model of a sums-only call, else 0 (run-time flags, all sums).  The instantiation
  // launched and the range the finalize reads both follow from this one value.
  const unsigned kf = (!d_cols && one_stage_flag(flags)) ? flags : 0u;
  if (n_rows > 0 || d_sums) {
    auto launch = [&](auto cols, auto f) {
      hipLaunchKernelGGL((residuals_kernel<decltype(cols)::value, decltype(f)::value>), dim3(blocks), dim3(kThreads), 0, st, d_x, d_u, d_y, a,
                         d_lambda, flags, n_rows, d_cols, ld, partials);
    };
    const std::integral_constant<unsigned, 0u> run_time_flags;
    if (d_cols) launch(std::true_type{}, run_time_flags);
    else if (!with_stage_flag(kf, [&](auto f) { launch(std::false_type{}, f); })) launch(std::false_type{}, run_time_flags);
  }
  if (d_sums) {
    const SumRange live = live_sums(kf);
    hipLaunchKernelGGL(sums_finalize<double>, dim3(1), dim3(1024), 0, st, (const double*)partials, blocks, live.lo, live.hi, d_sums);
  }
  return launch_status();
}

extern "C" int pinn_lambda_step(int stage, const double* d_sums, long long n_global, float vn_scale, float lr, int step,
                                float* d_lambda, float* d_adam, float* d_loss, void* stream) {
  if (stage < 0 || stage > PINN_STAGE_OXYGEN || !d_sums || n_global <= 0 || step < 1 || !d_lambda || !d_adam)
    return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(lambda_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stage, d_sums, 1.0 / (double)n_global,
                     vn_scale, lr, step, d_lambda, d_adam, d_loss);
  return launch_status();
}

extern "C" size_t pinn_lambda_stage_workspace_bytes(long long n_rows) { return n_rows > 0 ? (size_t)n_rows * 6 * sizeof(float) : 0; }

extern "C" int pinn_lambda_stage_run(int stage, unsigned flags, const float* d_x, const float* d_u, const float* d_y, const pinn_affine_t* aff,
                                     long long n_rows, double lr0, double gamma, int lr_step, int first_epoch, int n_iters, float* d_lambda,
                                     float* d_adam, float* d_loss, float* d_log, int log_every, double* d_sums, void* d_work, size_t work_bytes,
                                     void* stream) {
  if (stage < 0 || stage > PINN_STAGE_OXYGEN || !d_x || !aff || !d_lambda || !d_adam || n_rows <= 0 || n_rows > PINN_STAGE_RUN_MAX_ROWS ||
      n_iters < 0 || first_epoch < 0 || lr_step < 1)
    return PINN_E_ARG;
  if (!one_stage_flag(flags)) return PINN_E_ARG;
  // the stage names the parameters and the loss, the flag the row model: a pair that contradicts itself is refused, not reinterpreted
  const unsigned stage_flag = stage == PINN_STAGE_THERMAL ? PINN_RES_T : (stage == PINN_STAGE_HYDROGEN ? PINN_RES_H
                              : (stage == PINN_STAGE_OXYGEN ? PINN_RES_O : PINN_RES_V));
  if (flags != stage_flag) return PINN_E_ARG;
  if ((flags & PINN_RES_V) && (!d_u || !d_y)) return PINN_E_ARG;
  if (d_log && log_every > 0 && first_epoch % log_every) return PINN_E_ARG;
  if (!d_work) return PINN_E_ARG;
  if (work_bytes < pinn_lambda_stage_workspace_bytes(n_rows)) return PINN_E_WORKSPACE;
  if (n_iters == 0) return PINN_OK;
  clear_error();
  const AffineDev a = affine_dev(aff);
  with_stage_flag(flags, [&](auto f) {
    hipLaunchKernelGGL((stage_run_kernel<decltype(f)::value>), dim3(1), dim3(kStageThreads), 0, (hipStream_t)stream, stage, d_x, d_u, d_y, a,
                       n_rows, lr0, gamma, lr_step, first_epoch, n_iters, d_lambda, d_adam, d_loss, d_log, log_every, d_sums, (float*)d_work);
  });
  return launch_status();
}

extern "C" int pinn_residuals_prepare(const float* d_x, const float* d_u, const float* d_y, const pinn_affine_t* aff,
                                      const float* d_lambda, unsigned flags, long long n_rows, float* d_cache, void* stream) {
  if (!d_x || !aff || !d_lambda || !d_cache || n_rows <= 0 || !one_stage_flag(flags)) return PINN_E_ARG;
  if ((flags & PINN_RES_V) && (!d_u || !d_y)) return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(stage_prepare_kernel, dim3(row_blocks(n_rows)), dim3(kThreads), 0, (hipStream_t)stream, d_x, d_u, d_y, affine_dev(aff),
                     d_lambda, flags, n_rows, d_cache);
  return launch_status();
}

extern "C" int pinn_residuals_cached(const float* d_cache, const pinn_affine_t* aff, const float* d_lambda, unsigned flags,
                                     long long n_rows, double* d_sums, void* d_work, size_t work_bytes, void* stream) {
  if (!d_cache || !aff || !d_lambda || !d_sums || n_rows <= 0 || !one_stage_flag(flags)) return PINN_E_ARG;
  if (!d_work) return PINN_E_ARG;
  if (work_bytes < pinn_residuals_workspace_bytes()) return PINN_E_WORKSPACE;
  clear_error();
  hipStream_t st = (hipStream_t)stream;
  const int blocks = row_blocks((n_rows + 1) / 2);
  const AffineDev a = affine_dev(aff);
  with_stage_flag(flags, [&](auto f) {
    hipLaunchKernelGGL((residuals_cached_kernel<decltype(f)::value>), dim3(blocks), dim3(kThreads), 0, st, d_cache, a, d_lambda, n_rows,
                       (double*)d_work);
  });
  const SumRange live = live_sums(flags);
  hipLaunchKernelGGL(sums_finalize<double>, dim3(1), dim3(1024), 0, st, (const double*)d_work, blocks, live.lo, live.hi, d_sums);
  return launch_status();
}

extern "C" int pinn_net_f_t(const float* d_x, const float* d_u, const float* d_x_halo, const float* d_u_halo, const pinn_affine_t* aff,
                            const float* d_lambda, long long n_rows, float* d_f, float* d_t_pred, float* d_t_real, void* stream) {
  if (n_rows < 0 || !aff || !d_lambda || (n_rows > 0 && (!d_x || !d_f || !d_t_pred || !d_t_real))) return PINN_E_ARG;
  if (n_rows > 1 && !d_u) return PINN_E_ARG;
  if ((d_x_halo == nullptr) != (d_u_halo == nullptr)) return PINN_E_ARG;
  if (n_rows == 0) return PINN_OK;
  clear_error();
  hipLaunchKernelGGL(net_f_T_kernel, dim3(row_blocks(n_rows)), dim3(kThreads), 0, (hipStream_t)stream, d_x, d_u, d_x_halo, d_u_halo,
                     affine_dev(aff), d_lambda, n_rows, d_f, d_t_pred, d_t_real);
  return launch_status();
}

static bool misaligned16(const void* p) { return ((unsigned long long)(size_t)p & 15ull) != 0ull; }

extern "C" int pinn_residuals_backward(const float* d_x, const float* d_u, const pinn_affine_t* aff, const float* d_lambda, unsigned flags,
                                       long long n_rows, const float* d_g, long long ld, unsigned gmask, float* d_glambda, float* d_gu,
                                       float* d_gx, void* d_work, size_t work_bytes, void* stream) {
  if (n_rows < 0 || !aff || !d_lambda || !d_glambda || (flags & ~PINN_RES_ALL)) return PINN_E_ARG;
  if (gmask & ~grad_cols_of(flags)) return PINN_E_ARG;             // a column the requested residuals do not produce
  if (n_rows > 0 && (!d_x || misaligned16(d_x) || misaligned16(d_gx))) return PINN_E_ARG;
  if ((flags & PINN_RES_V) && n_rows > 0 && !d_u) return PINN_E_ARG;
  if (gmask && n_rows > 0 && (!d_g || ld < n_rows)) return PINN_E_ARG;
  if (!d_work) return PINN_E_ARG;
  if (work_bytes < pinn_residuals_workspace_bytes()) return PINN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const int blocks = row_blocks(n_rows);
  hipLaunchKernelGGL(residuals_backward_kernel, dim3(blocks), dim3(kThreads), 0, st, d_x, d_u, affine_dev(aff), d_lambda, flags, n_rows,
                     d_g, ld, gmask, d_gu, d_gx, (double*)d_work);
  launch_lambda_grad_finalize(d_work, blocks, d_glambda, st);
  return launch_status();
}

extern "C" int pinn_net_f_t_backward(const float* d_x, const float* d_u, const float* d_x_halo, const float* d_u_halo,
                                     const pinn_affine_t* aff, const float* d_lambda, long long n_rows, const float* d_gf,
                                     const float* d_gt_pred, const float* d_gt_real, float* d_glambda, float* d_gu, float* d_gx,
                                     float* d_gx_halo, float* d_gu_halo, void* d_work, size_t work_bytes, void* stream) {
  if (n_rows < 0 || !aff || !d_lambda || !d_glambda) return PINN_E_ARG;
  if (n_rows > 0 && (!d_x || misaligned16(d_x) || misaligned16(d_gx))) return PINN_E_ARG;
  if (n_rows > 1 && !d_u) return PINN_E_ARG;
  if ((d_x_halo == nullptr) != (d_u_halo == nullptr) || misaligned16(d_x_halo) || misaligned16(d_gx_halo)) return PINN_E_ARG;
  if (!d_x_halo && (d_gx_halo || d_gu_halo)) return PINN_E_ARG;
  if (!d_work) return PINN_E_ARG;
  if (work_bytes < pinn_residuals_workspace_bytes()) return PINN_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const int blocks = row_blocks(n_rows);
  hipLaunchKernelGGL(net_f_T_backward_kernel, dim3(blocks), dim3(kThreads), 0, st, d_x, d_u, d_x_halo, d_u_halo, affine_dev(aff), d_lambda,
                     n_rows, d_gf, d_gt_pred, d_gt_real, d_gu, d_gx, d_gx_halo, d_gu_halo, (double*)d_work);
  launch_lambda_grad_finalize(d_work, blocks, d_glambda, st);
  return launch_status();
}

