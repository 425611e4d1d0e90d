// pinn_identify.hip -- which physics parameter moved: per-window identification of the polarisation and thermal parameters
//   pinn_id_fit    Levenberg-Marquardt over windows of a four-column table, theta [3] with its covariance per window
//
// The statement of the problem, the solver and the status codes are in include/pinn_hip.h; identify.py's host backend states
// the same solver in numpy.  One workgroup owns a window from its first row pass to its covariance: the loop has no host
// synchronisation, reads nothing another workgroup writes and uses no float atomics.  The window's rows live in registers
// (kPerThread positions of four doubles per thread = 128 VGPRs) when it has at most PINN_ID_ONCHIP_ROWS
// positions; a longer window reads them again every pass.  Both forms visit positions t, t + 256, ... per thread in order
// and reduce alike, so they give the same sums.  Built with -ffp-contract=off: every operation is rounded on its own.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kPerThread = PINN_ID_ONCHIP_ROWS / kThreads;      // 16 positions per thread on chip
constexpr int kIdMaxBlocks = 256;                               // one workgroup per CU (the rows and what the compiler hoists out
                                                                // of the passes fill the register file); grid-stride beyond
constexpr int kSums = PINN_ID_NORMAL_WORDS;                     // A [6], g [3], sse, n_used, max i: the d_normal row
constexpr int kG = 6, kSse = 9, kN = 10, kImax = 11;
constexpr double kPivotMin = 1.0 / 1099511627776.0;             // 2^-40: smallest pivot of the scaled normal matrix
constexpr double kMuMin = 1e-15, kMuMax = 1e15;

static_assert(kPerThread * kThreads == PINN_ID_ONCHIP_ROWS && kPerThread <= 32, "on-chip rows are a mask bit per position");

struct IdOpts { double tol, xtol, mu0; int max_passes; };

template <int kModel>
__device__ __forceinline__ bool row_valid(bool ok, const double x[kRowsMaxD]) {
  const bool fin = isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(x[3]);
  return ok && fin && (kModel != PINN_ID_VOLTAGE || (x[0] > 0.0 && x[1] > 0.0));
}

// one used row: residual, Jacobian row, and their products into the twelve sums
template <int kModel>
__device__ __forceinline__ void row_terms(double x0, double x1, double x2, double x3, const double th[3], double acc[kSums]) {
  double r, j0, j1, j2;
  if (kModel == PINN_ID_VOLTAGE) {
    const double ic = x0 * th[2];
    r = (((x2 - x1 * (log(x0) - th[1])) - x0 * th[0]) + (0.5 * x1) * log1p(-ic)) - x3;
    j0 = -x0; j1 = x1; j2 = -((0.5 * x1) * x0) / (1.0 - ic);
  } else {
    r = x3 - (((th[0] * x0 + th[1] * x1) + 0.5 * x2) + th[2]);
    j0 = -x0; j1 = -x1; j2 = -1.0;
  }
  acc[0] += j0 * j0; acc[1] += j0 * j1; acc[2] += j1 * j1; acc[3] += j0 * j2; acc[4] += j1 * j2; acc[5] += j2 * j2;
  acc[kG] += j0 * r; acc[kG + 1] += j1 * r; acc[kG + 2] += j2 * r;
  acc[kSse] += r * r;
  acc[kN] += 1.0;
  acc[kImax] = fmax(acc[kImax], x0);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the window's rows as the pass reads them: registers (mask bit k: position t + 256 k is used) or the table itself
struct OnChip {
  double x0[kPerThread], x1[kPerThread], x2[kPerThread], x3[kPerThread];
  unsigned mask;
};

template <int kModel>
__device__ __forceinline__ void row_pass(bool onchip, const OnChip& c, const Rows& a, long long start, long long len, const double th[3],
                                         double (*red)[kSums], double* tot, double out[kSums]) {
  double acc[kSums];
#pragma unroll
  for (int s = 0; s < kSums; ++s) acc[s] = 0.0;
  acc[kImax] = -INFINITY;
  if (onchip) {
#pragma unroll
    for (int k = 0; k < kPerThread; ++k)
      if ((c.mask >> k) & 1u) row_terms<kModel>(c.x0[k], c.x1[k], c.x2[k], c.x3[k], th, acc);
  } else {
    for (long long j = threadIdx.x; j < len; j += kThreads) {
      double x[kRowsMaxD];
      const bool ok = load_row(a, start + j, x);
      if (row_valid<kModel>(ok, x)) row_terms<kModel>(x[0], x[1], x[2], x[3], th, acc);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = 0; s < kSums; ++s) {
    const double v = s == kImax ? wave_max(acc[s]) : wave_sum(acc[s]);
    if (lane == 0) red[wave][s] = v;
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double v = red[0][threadIdx.x];
    for (int w = 1; w < kWaves; ++w) v = threadIdx.x == kImax ? fmax(v, red[w][threadIdx.x]) : v + red[w][threadIdx.x];
    tot[threadIdx.x] = v;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kSums; ++s) out[s] = tot[s];
}

// Cholesky factor of the packed symmetric M + shift I; false when a pivot is not above pmin
__device__ __forceinline__ bool chol3(const double M[6], double shift, double pmin, double L[6]) {
  double p = M[0] + shift;
  if (!(p > pmin)) return false;
  L[0] = sqrt(p);
  L[1] = M[1] / L[0];
  L[3] = M[3] / L[0];
  p = (M[2] + shift) - L[1] * L[1];
  if (!(p > pmin)) return false;
  L[2] = sqrt(p);
  L[4] = (M[4] - L[3] * L[1]) / L[2];
  p = ((M[5] + shift) - L[3] * L[3]) - L[4] * L[4];
  if (!(p > pmin)) return false;
  L[5] = sqrt(p);
  return true;
}
__device__ __forceinline__ void chol3_forward(const double L[6], const double b[3], double y[3]) {
  y[0] = b[0] / L[0];
  y[1] = (b[1] - L[1] * y[0]) / L[2];
  y[2] = ((b[2] - L[3] * y[0]) - L[4] * y[1]) / L[5];
}
__device__ __forceinline__ void chol3_backward(const double L[6], const double y[3], double x[3]) {
  x[2] = y[2] / L[5];
  x[1] = (y[1] - L[4] * x[2]) / L[2];
  x[0] = ((y[0] - L[1] * x[1]) - L[3] * x[2]) / L[0];
}

__device__ __forceinline__ bool finite3(const double v[3]) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }
__device__ __forceinline__ bool finite_sums(const double s[kSums]) {
  bool f = true;
#pragma unroll
  for (int k = 0; k <= kSse; ++k) f = f && isfinite(s[k]);
  return f;
}
template <int kModel>
__device__ __forceinline__ bool in_domain(const double th[3], double imax) {
  return kModel != PINN_ID_VOLTAGE || th[2] * imax < 1.0;
}

template <int kModel>
__global__ __launch_bounds__(kThreads) void id_fit_kernel(Rows a, const long long* __restrict__ win_start, const long long* __restrict__ win_len,
                                                          long long n_windows, const double* __restrict__ theta0, long long theta0_stride,
                                                          IdOpts o, double* __restrict__ fit, double* __restrict__ normal) {
  __shared__ double red[kWaves][kSums];
  __shared__ double tot[kSums];
  const double nan = quiet_nan();
  for (long long w = blockIdx.x; w < n_windows; w += gridDim.x) {
    const long long start = win_start[w], len = win_len[w];
    double* fr = fit + w * PINN_ID_FIT_WORDS;
    double* nr = normal ? normal + w * PINN_ID_NORMAL_WORDS : nullptr;
    if (start < 0 || len < 0 || len > PINN_ID_MAX_WINDOW || start > a.n - len) {     // uniform: every thread reads the same two words
      if (threadIdx.x < PINN_ID_FIT_WORDS) fr[threadIdx.x] = threadIdx.x < 12 ? nan : (threadIdx.x == 14 ? 6.0 : 0.0);
      if (nr && threadIdx.x < kSums) nr[threadIdx.x] = nan;
      continue;
    }
    const bool onchip = len <= PINN_ID_ONCHIP_ROWS;
    OnChip c;
    c.mask = 0u;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      double x[kRowsMaxD];
#pragma unroll
      for (int i = 0; i < kRowsMaxD; ++i) x[i] = 0.0;
      const long long j = threadIdx.x + (long long)k * kThreads;
      if (onchip && j < len) {
        const bool ok = load_row(a, start + j, x);
        if (row_valid<kModel>(ok, x)) c.mask |= 1u << k;
      }
      c.x0[k] = x[0]; c.x1[k] = x[1]; c.x2[k] = x[2]; c.x3[k] = x[3];
    }

    // one call site of the row pass: every trip evaluates one point, the start point first
    double th[3], cur[kSums], tr[kSums], tht[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) tht[k] = th[k] = theta0[w * theta0_stride + k];
#pragma unroll
    for (int s = 0; s < kSums; ++s) cur[s] = 0.0;
    int passes = 0, status = -1;
    double mu = o.mu0, m = nan;
    double sc[3], C[6], gs[3], L[6], y[3], z[3];
    while (status < 0) {
      row_pass<kModel>(onchip, c, a, start, len, tht, red, tot, tr);
      const bool first = passes == 0;
      ++passes;
      const bool fine = finite3(tht) && in_domain<kModel>(tht, tr[kImax]) && finite_sums(tr);
      if (first || (fine && tr[kSse] < cur[kSse])) {
#pragma unroll
        for (int k = 0; k < 3; ++k) th[k] = tht[k];
#pragma unroll
        for (int s = 0; s < kSums; ++s) cur[s] = tr[s];
        if (first) {
          if (cur[kN] < 4.0) status = 3;
          else if (!fine) status = 4;
        } else {
          mu = fmax(mu / 10.0, kMuMin);
        }
      } else {
        mu *= 10.0;
        if (mu > kMuMax) status = 2;
      }
      if (status >= 0) break;
      // Marquardt scaling and the certificate m at the current point
      if (!(cur[0] > 0.0 && cur[2] > 0.0 && cur[5] > 0.0)) { status = 5; break; }
      sc[0] = 1.0 / sqrt(cur[0]); sc[1] = 1.0 / sqrt(cur[2]); sc[2] = 1.0 / sqrt(cur[5]);
      C[0] = 1.0; C[1] = (cur[1] * sc[0]) * sc[1]; C[2] = 1.0; C[3] = (cur[3] * sc[0]) * sc[2]; C[4] = (cur[4] * sc[1]) * sc[2]; C[5] = 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) gs[k] = cur[kG + k] * sc[k];
      if (!chol3(C, 0.0, kPivotMin, L)) { status = 5; break; }
      if (cur[kSse] == 0.0) { m = 0.0; status = 0; break; }
      chol3_forward(L, gs, y);
      m = sqrt(((y[0] * y[0] + y[1] * y[1]) + y[2] * y[2]) / (cur[kSse] / (cur[kN] - 3.0)));
      if (m <= o.tol) { status = 0; break; }
      if (passes >= o.max_passes) { status = 1; break; }
      // trial step (A + mu D) d = -g
      chol3(C, mu, 0.0, L);
      chol3_forward(L, gs, y);
      chol3_backward(L, y, z);
      bool small = true;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double d = -(z[k] * sc[k]);
        small = small && fabs(d) <= o.xtol * (fabs(th[k]) + o.xtol);
        tht[k] = th[k] + d;
      }
      if (small) status = 0;
    }

    if (threadIdx.x == 0) {
      double out[PINN_ID_FIT_WORDS];
#pragma unroll
      for (int k = 0; k < 12; ++k) out[k] = nan;
      out[12] = cur[kN]; out[13] = (double)passes; out[14] = (double)status; out[15] = 0.0;
      if (status != 3 && status != 4) {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = th[k];
        out[9] = cur[kSse]; out[11] = mu;
      }
      if (status <= 2) {
        out[10] = m;
        chol3(C, 0.0, kPivotMin, L);            // the undamped factor again: a trial step may have replaced it
        const double s2 = cur[kSse] / (cur[kN] - 3.0);
#pragma unroll
        for (int q = 0; q < 3; ++q) {           // column q of C^-1, scaled back: s2 A^-1 = s2 S C^-1 S
          double e[3] = {q == 0 ? 1.0 : 0.0, q == 1 ? 1.0 : 0.0, q == 2 ? 1.0 : 0.0};
          chol3_forward(L, e, y);
          chol3_backward(L, y, z);
#pragma unroll
          for (int p = 0; p <= q; ++p) out[3 + tri(p, q)] = s2 * ((z[p] * sc[p]) * sc[q]);
        }
      }
#pragma unroll
      for (int k = 0; k < PINN_ID_FIT_WORDS; ++k) fr[k] = out[k];
      if (nr) {
#pragma unroll
        for (int s = 0; s < kSums; ++s) nr[s] = cur[s];
      }
    }
    __syncthreads();
  }
}

inline bool positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

}  // namespace
}  // namespace pinn

using namespace pinn;

extern "C" int pinn_id_fit(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int model,
                           const long long* d_row_index, long long n, const long long* d_win_start, const long long* d_win_len,
                           long long n_windows, const double* d_theta0, long long theta0_stride, const pinn_id_opts_t* opts,
                           double* d_fit, double* d_normal, void* stream) {
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, 4, 1, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (model != PINN_ID_VOLTAGE && model != PINN_ID_THERMAL) return PINN_E_ARG;
  if (n_windows < 0 || (theta0_stride != 0 && theta0_stride != 3)) return PINN_E_ARG;
  IdOpts o = {1e-8, 1e-14, 1e-3, 100};
  if (opts) {
    if (!positive_finite(opts->tol) || !positive_finite(opts->xtol) || !positive_finite(opts->mu0) || opts->max_passes < 0 || opts->reserved != 0)
      return PINN_E_ARG;
    o.tol = opts->tol; o.xtol = opts->xtol; o.mu0 = opts->mu0; o.max_passes = opts->max_passes;
  }
  if (misaligned8(d_win_start) || misaligned8(d_win_len) || misaligned8(d_theta0) || misaligned8(d_fit) || misaligned8(d_normal)) return PINN_E_ARG;
  if (n_windows == 0) return PINN_OK;
  if (!d_win_start || !d_win_len || !d_theta0 || !d_fit) return PINN_E_ARG;
  clear_error();
  const int blocks = (int)(n_windows < kIdMaxBlocks ? n_windows : kIdMaxBlocks);
  if (model == PINN_ID_VOLTAGE)
    hipLaunchKernelGGL(id_fit_kernel<PINN_ID_VOLTAGE>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a, d_win_start, d_win_len, n_windows,
                       d_theta0, theta0_stride, o, d_fit, d_normal);
  else
    hipLaunchKernelGGL(id_fit_kernel<PINN_ID_THERMAL>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, a, d_win_start, d_win_len, n_windows,
                       d_theta0, theta0_stride, o, d_fit, d_normal);
  return launch_status();
}
