// Fault detection on the device (reference script 02, cited as 02:<line>): StandardScaler + multinomial logistic
// regression (02:195-207) and the ROC curve / AUC of 1 - P(normal) (02:552-557).  All arithmetic is float64.
//   pinn_lr_scaler     mean_, var_, scale_, class counts and class weights of the training rows (two passes)
//   pinn_lr_pass       loss, gradient and Hessian sums of one row pass at the state's point (for tests and tools)
//   pinn_lr_newton     damped Newton iterations, two launches each, no host synchronisation between them
//   pinn_lr_posterior  decision_function, predict_proba, predict and p_fault per row, one launch
//   pinn_lr_roc        boundaries of the sorted scores, fps / tps, drop_intermediate, fpr / tpr and the integer area
//   pinn_lr_batch_*    scaler, Newton iterations, validation scores and the integer area for a batch of models over column
//                      subsets of one array: grids of (row blocks, candidates) and one workgroup per candidate around the
//                      single model's bodies (lr_stats_body, lr_rows_body, lr_final_body, post_scores), so that a
//                      candidate's bytes are the single model's
//
// The row pass follows pinn_gmm.hip: a workgroup takes tiles of 128 rows, one thread per row standardises its row and
// writes (z, 1), the class probabilities, the sample weight and the loss term into LDS; then every thread owns up to 12 of
// the 1 + P + H output sums (loss; gradient, P = C (D + 1); Hessian blocks c <= d, upper triangles, H = C (C + 1) / 2 x
// (D + 1) (D + 2) / 2) and adds the tile's 128 terms to them in row order, in registers.  Workgroup sums go to the
// workspace; a one-workgroup launch adds them in index order, adds the penalty and decides the step.  No float atomics, no
// workgroup waits on another: stream order is the only dependency and the same call gives the same bytes every time.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pinn_rows.h"

static_assert(PINN_LR_MAX_FEAT == PINN_GMM_MAX_FEAT && PINN_LR_MAX_CLASSES <= PINN_GMM_MAX_COMP,
              "pinn_rows.h sizes Rows and bounds make_rows by the mixture's limits");

namespace pinn {
namespace {

constexpr int kRows = 128;                  // rows per tile = threads per workgroup of the row pass
constexpr int kMaxC = PINN_LR_MAX_CLASSES, kMaxD = PINN_LR_MAX_FEAT, kMaxH = PINN_LR_MAX_HESS;
constexpr int kMaxP = 65;                   // largest C (D + 1) under the three limits (C = 13, D = 4)
constexpr int kMaxSums = 1 + kMaxP + kMaxH;
constexpr int kMaxOut = (kMaxSums + kRows - 1) / kRows;                        // output sums per thread: 12
constexpr int kMaxBlocks = 1024;            // workgroups of a row pass = partial sums per output
constexpr int kFinThreads = 256;
constexpr int kHdr = PINN_LR_ST_HEADER;
constexpr double kEps = 2.220446049250313e-16;

enum { FIN_SUMS = 0, FIN_NEWTON = 1 };

// state block: header, then theta [P] (the point the next pass evaluates), accepted [P], direction [P], gradient [P] of the
// accepted point, mean [D], scale [D], var [D], class_weight [C], class_count [C] (64-bit integers).
// theta is laid out [C][D + 1]: the D coefficients of a class, then its intercept.
__host__ __device__ inline int n_par(int C, int D) { return C * (D + 1); }
__host__ __device__ inline int n_hess(int C, int D) { return (C * (C + 1) / 2) * ((D + 1) * (D + 2) / 2); }
__host__ __device__ inline size_t st_theta() { return kHdr; }
__host__ __device__ inline size_t st_prev(int C, int D) { return kHdr + (size_t)n_par(C, D); }
__host__ __device__ inline size_t st_dir(int C, int D) { return kHdr + 2 * (size_t)n_par(C, D); }
__host__ __device__ inline size_t st_grad(int C, int D) { return kHdr + 3 * (size_t)n_par(C, D); }
__host__ __device__ inline size_t st_mean(int C, int D) { return kHdr + 4 * (size_t)n_par(C, D); }
__host__ __device__ inline size_t st_scale(int C, int D) { return st_mean(C, D) + D; }
__host__ __device__ inline size_t st_var(int C, int D) { return st_mean(C, D) + 2 * D; }
__host__ __device__ inline size_t st_cw(int C, int D) { return st_mean(C, D) + 3 * D; }
__host__ __device__ inline size_t st_count(int C, int D) { return st_cw(C, D) + C; }
__host__ __device__ inline size_t st_words(int C, int D) { return st_count(C, D) + C; }

inline bool in_limits(int C, int D) {
  return C >= 2 && C <= kMaxC && D >= 1 && D <= kMaxD && n_hess(C, D) <= kMaxH && n_par(C, D) <= kMaxP;
}

__device__ __forceinline__ bool stopped(const double* st) {
  const long long* h = reinterpret_cast<const long long*>(st);
  return h[PINN_LR_ST_CONVERGED] != 0 || h[PINN_LR_ST_STATUS] != 0 || h[PINN_LR_ST_ITER] >= h[PINN_LR_ST_MAXITER];
}

// The model of a row, shared by the fit and the posterior: z = (x - mean) / scale into u[0..D), the scores of the R
// parameter rows W [R][ldw] (+ intercept at W[r][D] when with_b) into s[r * stride]: products added in feature order.
__device__ __forceinline__ void row_scores(const double x[kMaxD], int D, int R, const double* mean, const double* scale,
                                           const double* W, int ldw, bool with_b, double* u, double* s, int stride) {
#pragma unroll
  for (int i = 0; i < kMaxD; ++i)
    if (i < D) u[i] = (x[i] - mean[i]) / scale[i];
  for (int r = 0; r < R; ++r) {
    double v = 0.0;
    for (int i = 0; i < D; ++i) v += W[r * ldw + i] * u[i];
    if (with_b) v += W[r * ldw + D];
    s[r * stride] = v;
  }
}

// softmax in place over s[0..C): returns logsumexp (scipy's order: max, sum, log); s becomes exp(s - max) / sum
__device__ __forceinline__ double softmax_inplace(double* s, int C) {
  double m = s[0];
  for (int c = 1; c < C; ++c) m = s[c] > m ? s[c] : m;
  double sum = 0.0;
  for (int c = 0; c < C; ++c) { s[c] = exp(s[c] - m); sum += s[c]; }
  for (int c = 0; c < C; ++c) s[c] /= sum;
  return log(sum) + m;
}

// ---- the row pass.  part: [gridDim.x][n_sums]
// (bx of gx: the workgroup's place among those of its model, which is blockIdx.x of gridDim.x in both launch forms)
__device__ __forceinline__ void lr_rows_body(const Rows& a, const double* __restrict__ st, const long long* __restrict__ y_in, int force,
                                             double* __restrict__ part, unsigned bx, unsigned gx) {
  __shared__ double s_p[kRows * kMaxC];          // probabilities, row stride C | 1
  __shared__ double s_u[kRows * (kMaxD + 1)];    // (z, 1), row stride (D + 1) | 1
  __shared__ double s_w[kRows], s_l[kRows];
  __shared__ int s_y[kRows];
  __shared__ double s_th[kMaxP], s_mean[kMaxD], s_scale[kMaxD], s_cw[kMaxC];
  if (!force && stopped(st)) return;
  const int C = a.K, D = a.D, Cp = C | 1, Up = (D + 1) | 1, t = threadIdx.x, P = n_par(C, D);
  for (int e = t; e < P; e += kRows) s_th[e] = st[st_theta() + e];
  if (t < D) { s_mean[t] = st[st_mean(C, D) + t]; s_scale[t] = st[st_scale(C, D) + t]; }
  if (t < C) s_cw[t] = st[st_cw(C, D) + t];
  __syncthreads();

  // the outputs of this thread: o = t + q kRows -> loss | gradient (c, i) | Hessian (c <= d, i <= j)
  const int nT = (D + 1) * (D + 2) / 2, n_sums = 1 + P + n_hess(C, D);
  int oc[kMaxOut], od[kMaxOut], oi[kMaxOut], oj[kMaxOut];
  double acc[kMaxOut];
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q) {
    const int o = t + q * kRows;
    acc[q] = 0.0;
    oc[q] = -2; od[q] = -1; oi[q] = 0; oj[q] = 0;
    if (o == 0) {
      oc[q] = -1;
    } else if (o <= P) {
      oc[q] = (o - 1) / (D + 1);
      oi[q] = (o - 1) - oc[q] * (D + 1);
    } else if (o < n_sums) {
      const int h = o - 1 - P, pc = h / nT;
      untri(pc, &oc[q], &od[q]);
      untri(h - pc * nT, &oi[q], &oj[q]);
    }
  }

  const long long tiles = (a.n + kRows - 1) / kRows;
  for (long long tile = bx; tile < tiles; tile += gx) {
    const long long j = tile * kRows + t;
    double x[kMaxD];
    bool ok = false;
    long long cls = -1;
    if (j < a.n) {
      ok = load_row(a, j, x);
      cls = y_in[j];
    }
    ok = ok && cls >= 0 && cls < C;                           // a class outside [0, C) adds nothing
    double* p = s_p + t * Cp;
    double* u = s_u + t * Up;
    if (ok) {
      row_scores(x, D, C, s_mean, s_scale, s_th, D + 1, true, u, p, 1);
      u[D] = 1.0;
      const double sy = p[cls];
      const double lse = softmax_inplace(p, C);
      s_w[t] = s_cw[cls];
      s_l[t] = s_cw[cls] * (lse - sy);
      s_y[t] = (int)cls;
    } else {
      for (int c = 0; c < C; ++c) p[c] = 0.0;
      for (int i = 0; i <= D; ++i) u[i] = 0.0;
      s_w[t] = 0.0; s_l[t] = 0.0; s_y[t] = -1;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxOut; ++q) {
      const int c = oc[q];
      if (c == -2) continue;
      double s = acc[q];
      if (c == -1) {
#pragma unroll 4
        for (int rr = 0; rr < kRows; ++rr) s += s_l[rr];
      } else if (od[q] < 0) {
        const int i = oi[q];
#pragma unroll 4
        for (int rr = 0; rr < kRows; ++rr) s += s_w[rr] * (s_p[rr * Cp + c] - (s_y[rr] == c ? 1.0 : 0.0)) * s_u[rr * Up + i];
      } else {
        const int d = od[q], i = oi[q], jj = oj[q];
        const double delta = c == d ? 1.0 : 0.0;
#pragma unroll 4
        for (int rr = 0; rr < kRows; ++rr)
          s += s_w[rr] * s_p[rr * Cp + c] * (delta - s_p[rr * Cp + d]) * (s_u[rr * Up + i] * s_u[rr * Up + jj]);
      }
      acc[q] = s;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q)
    if (oc[q] != -2) part[(size_t)bx * n_sums + t + q * kRows] = acc[q];
}

__global__ __launch_bounds__(kRows) void lr_rows_kernel(Rows a, const double* __restrict__ st, const long long* __restrict__ y_in,
                                                        int force, double* __restrict__ part) {
  lr_rows_body(a, st, y_in, force, part, blockIdx.x, gridDim.x);
}

// ---- sums of the partials in index order, then the step.  One workgroup.  tot: [n_sums] (kept in the workspace).
__device__ __forceinline__ void lr_final_body(double* __restrict__ st, int C, int D, int mode, int n_part, long long n, double tol, double l2,
                                              int fit_intercept, const double* __restrict__ part, double* __restrict__ tot) {
  __shared__ double A[kMaxP * kMaxP];
  __shared__ double g[kMaxP], dirv[kMaxP];
  __shared__ int s_flag;
  long long* hdr = reinterpret_cast<long long*>(st);
  if (mode == FIN_NEWTON && stopped(st)) return;
  const int P = n_par(C, D), nT = (D + 1) * (D + 2) / 2, n_sums = 1 + P + n_hess(C, D), t = threadIdx.x, D1 = D + 1;
  for (int o = t; o < n_sums; o += kFinThreads) {
    double s = 0.0;
    for (int b = 0; b < n_part; ++b) s += part[(size_t)b * n_sums + o];
    tot[o] = s;
  }
  __syncthreads();
  if (mode == FIN_SUMS) return;

  double* theta = st + st_theta();
  double* prev = st + st_prev(C, D);
  double* dir = st + st_dir(C, D);
  const double sw_sum = st[PINN_LR_ST_SWSUM];
  // F = loss + l2 / 2 |W|^2; gradient + l2 W; a parameter that is not fitted has gradient 0
  if (t == 0) {
    double pen = 0.0;
    for (int c = 0; c < C; ++c)
      for (int i = 0; i < D; ++i) pen += theta[c * D1 + i] * theta[c * D1 + i];
    const double F = tot[0] + 0.5 * l2 * pen;
    int bad = !(F == F) || !(fabs(F) < INFINITY);
    for (int p = 0; p < P; ++p) {
      const int i = p % D1;
      double v = tot[1 + p] + (i < D ? l2 * theta[p] : 0.0);
      if (i == D && !fit_intercept) v = 0.0;
      if (!(v == v)) bad = 1;
      g[p] = v;
    }
    int flag = 0;                                             // 0 accept, 1 reject, 2 fail
    const long long phase = hdr[PINN_LR_ST_PHASE];
    if (phase == 0) {
      if (bad) flag = 2;
    } else {
      // Armijo on the stored directional derivative, with a floor at the rounding of the loss sum itself
      const double Fp = st[PINN_LR_ST_F], step = st[PINN_LR_ST_STEP], dd = st[PINN_LR_ST_DD];
      const double floor_ = 4.0 * (double)n * kEps * fabs(tot[0]);
      if (bad || !(F <= Fp + 1e-4 * step * dd + floor_)) flag = 1;
    }
    if (flag == 1) {
      const double step = 0.5 * st[PINN_LR_ST_STEP];
      hdr[PINN_LR_ST_PASSES] += 1;
      if (step < 9.094947017729282e-13) {                     // 2^-40: the direction gives no decrease
        for (int p = 0; p < P; ++p) theta[p] = prev[p];
        hdr[PINN_LR_ST_STATUS] = PINN_LR_STALLED;
      } else {
        st[PINN_LR_ST_STEP] = step;
        for (int p = 0; p < P; ++p) theta[p] = prev[p] + step * dir[p];
      }
    } else if (flag == 2) {
      hdr[PINN_LR_ST_STATUS] = PINN_LR_NAN;
    } else {
      double gmax = 0.0;
      for (int p = 0; p < P; ++p) {
        prev[p] = theta[p];
        st[st_grad(C, D) + p] = g[p];
        gmax = fabs(g[p]) > gmax ? fabs(g[p]) : gmax;
      }
      st[PINN_LR_ST_F] = F;
      st[PINN_LR_ST_GMAX] = gmax / sw_sum;
      hdr[PINN_LR_ST_PASSES] += 1;
      if (phase != 0) hdr[PINN_LR_ST_ITER] += 1;
      hdr[PINN_LR_ST_PHASE] = 1;
      if (gmax / sw_sum <= tol) { hdr[PINN_LR_ST_CONVERGED] = 1; flag = 3; }
    }
    s_flag = flag;
  }
  __syncthreads();
  if (s_flag != 0) return;

  // Hessian, full P x P from the upper triangles: H[(c,i),(d,j)] = T[pair(c,d)][tri(min(i,j), max(i,j))], + l2 on the
  // coefficients' diagonal, + kappa on every pair of intercepts: the rank-one term that pins the sum of the intercepts.
  const double kappa = sw_sum / (double)C;
  // Far from the minimum the probabilities saturate and the factorisation can fail in rounding: it is then repeated with a
  // ridge of 1e-6, 1e-4, 1e-2 sum sw on the diagonal, which changes the direction (still one of descent), not the minimiser.
  for (int attempt = 0; attempt < 4; ++attempt) {
    const double ridge = attempt == 0 ? 0.0 : sw_sum * (attempt == 1 ? 1e-6 : (attempt == 2 ? 1e-4 : 1e-2));
    for (int e = t; e < P * P; e += kFinThreads) {
      const int r = e / P, q = e - r * P;
      int c = r / D1, i = r - c * D1, d = q / D1, j = q - d * D1;
      if (c > d) { const int tc = c; c = d; d = tc; }
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      double v = tot[1 + P + tri(c, d) * nT + tri(lo, hi)];
      if (r == q && i < D) v += l2;
      if (i == D && j == D) v += kappa;
      if (r == q) v += ridge;
      if (!fit_intercept && (i == D || j == D)) v = r == q ? 1.0 : 0.0;
      A[e] = v;
    }
    __syncthreads();
    if (t == 0) s_flag = 0;
    __syncthreads();
    // Cholesky A = L L^T, right-looking, L in the lower triangle
    for (int k = 0; k < P; ++k) {
      if (t == 0) {
        const double piv = A[k * P + k];
        if (!(piv > 0.0) || !(piv < INFINITY)) s_flag = 2; else A[k * P + k] = sqrt(piv);
      }
      __syncthreads();
      if (s_flag == 2) break;
      const double lkk = A[k * P + k];
      for (int r = k + 1 + t; r < P; r += kFinThreads) A[r * P + k] /= lkk;
      __syncthreads();
      const int m = P - k - 1;
      for (int e = t; e < m * m; e += kFinThreads) {
        const int r = k + 1 + e / m, q = k + 1 + e % m;
        if (q <= r) A[r * P + q] -= A[r * P + k] * A[q * P + k];
      }
      __syncthreads();
    }
    if (s_flag != 2) break;
  }
  if (t == 0) {
    if (s_flag == 2) {
      for (int p = 0; p < P; ++p) theta[p] = prev[p];
      hdr[PINN_LR_ST_STATUS] = PINN_LR_SINGULAR;
    } else {
      for (int r = 0; r < P; ++r) {                           // L w = -g
        double v = -g[r];
        for (int q = 0; q < r; ++q) v -= A[r * P + q] * dirv[q];
        dirv[r] = v / A[r * P + r];
      }
      for (int r = P - 1; r >= 0; --r) {                      // L^T dir = w
        double v = dirv[r];
        for (int q = r + 1; q < P; ++q) v -= A[q * P + r] * dirv[q];
        dirv[r] = v / A[r * P + r];
      }
      double dd = 0.0;
      int bad = 0;
      for (int p = 0; p < P; ++p) { dd += g[p] * dirv[p]; bad |= !(dirv[p] == dirv[p]); }
      if (bad || !(dd < 0.0)) {
        // dd == 0 only with a zero gradient, which the tolerance test has already taken unless tol is 0
        if (!bad && dd == 0.0) hdr[PINN_LR_ST_CONVERGED] = 1; else hdr[PINN_LR_ST_STATUS] = bad ? PINN_LR_NAN : PINN_LR_SINGULAR;
      } else {
        st[PINN_LR_ST_DD] = dd;
        st[PINN_LR_ST_STEP] = 1.0;
        for (int p = 0; p < P; ++p) { dir[p] = dirv[p]; theta[p] = prev[p] + dirv[p]; }
      }
    }
  }
}

__global__ __launch_bounds__(kFinThreads) void lr_final_kernel(double* __restrict__ st, int C, int D, int mode, int n_part, long long n,
                                                               double tol, double l2, int fit_intercept,
                                                               const double* __restrict__ part, double* __restrict__ tot) {
  lr_final_body(st, C, D, mode, n_part, n, tol, l2, fit_intercept, part, tot);
}

// ---- scaler: sums of x (pass 0) or of (x - mean)^2 (pass 1) per feature, class counts.  part: [grid][D], cnt: [grid][C]
__device__ __forceinline__ void lr_stats_body(const Rows& a, const double* __restrict__ st, const long long* __restrict__ y_in, int pass,
                                              double* __restrict__ part, long long* __restrict__ cnt, unsigned bx, unsigned gx) {
  __shared__ double s_x[kRows * (kMaxD + 1)];
  __shared__ int s_y[kRows];
  const int C = a.K, D = a.D, Dp = D | 1, t = threadIdx.x;
  const double mean = (pass == 1 && t < D) ? st[st_mean(C, D) + t] : 0.0;
  double acc = 0.0;
  long long count = 0;
  const long long tiles = (a.n + kRows - 1) / kRows;
  for (long long tile = bx; tile < tiles; tile += gx) {
    const long long j = tile * kRows + t;
    double x[kMaxD];
    bool ok = false;
    long long cls = -1;
    if (j < a.n) {
      ok = load_row(a, j, x);
      cls = y_in ? y_in[j] : 0;
    }
    ok = ok && cls >= 0 && cls < C;
    s_y[t] = ok ? (int)cls : -1;
#pragma unroll
    for (int i = 0; i < kMaxD; ++i)
      if (i < D) s_x[t * Dp + i] = ok ? x[i] : (pass == 1 ? quiet_nan() : 0.0);
    __syncthreads();
    if (t < D) {
      for (int rr = 0; rr < kRows; ++rr) {
        if (pass == 0) acc += s_x[rr * Dp + t];
        else if (s_y[rr] >= 0) { const double d = s_x[rr * Dp + t] - mean; acc += d * d; }
      }
    } else if (t - kMaxD >= 0 && t - kMaxD < C) {
      for (int rr = 0; rr < kRows; ++rr) count += s_y[rr] == t - kMaxD ? 1 : 0;
    }
    __syncthreads();
  }
  if (t < D) part[(size_t)bx * D + t] = acc;
  else if (t - kMaxD >= 0 && t - kMaxD < C) cnt[(size_t)bx * C + (t - kMaxD)] = count;
}

__global__ __launch_bounds__(kRows) void lr_stats_kernel(Rows a, const double* __restrict__ st, const long long* __restrict__ y_in, int pass,
                                                         double* __restrict__ part, long long* __restrict__ cnt) {
  lr_stats_body(a, st, y_in, pass, part, cnt, blockIdx.x, gridDim.x);
}

__device__ __forceinline__ void lr_stats_final_body(double* __restrict__ st, int C, int D, int pass, int balanced, int n_part,
                                                    const double* __restrict__ part, const long long* __restrict__ cnt) {
  __shared__ long long s_cnt[kMaxC];
  long long* hdr = reinterpret_cast<long long*>(st);
  const int t = threadIdx.x;
  if (t < C) {
    long long s = 0;
    for (int b = 0; b < n_part; ++b) s += cnt[(size_t)b * C + t];
    s_cnt[t] = s;
  }
  __syncthreads();
  long long n = 0;
  for (int c = 0; c < C; ++c) n += s_cnt[c];
  if (t < D) {
    double s = 0.0;
    for (int b = 0; b < n_part; ++b) s += part[(size_t)b * D + t];
    if (pass == 0) {
      st[st_mean(C, D) + t] = n > 0 ? s / (double)n : 0.0;
    } else {
      const double var = n > 0 ? s / (double)n : 0.0, mean = st[st_mean(C, D) + t];
      double scale = sqrt(var);
      // scikit-learn's _is_constant_feature and _handle_zeros_in_scale
      const double nm = (double)n * mean * kEps, bound = (double)n * kEps * var + nm * nm;
      if (var <= bound || scale < 10.0 * kEps) scale = 1.0;
      st[st_var(C, D) + t] = var;
      st[st_scale(C, D) + t] = scale;
    }
  }
  if (pass == 1 && t == 0) {
    double sw = 0.0;
    for (int c = 0; c < C; ++c) {
      const double w = !balanced ? 1.0 : (s_cnt[c] > 0 ? (double)n / ((double)C * (double)s_cnt[c]) : 0.0);
      st[st_cw(C, D) + c] = w;
      reinterpret_cast<long long*>(st)[st_count(C, D) + c] = s_cnt[c];
      sw += w * (double)s_cnt[c];
    }
    st[PINN_LR_ST_SWSUM] = sw;
    hdr[PINN_LR_ST_NSEEN] = n;
    hdr[PINN_LR_ST_C] = C;
    hdr[PINN_LR_ST_D] = D;
  }
}

__global__ __launch_bounds__(64) void lr_stats_final_kernel(double* __restrict__ st, int C, int D, int pass, int balanced, int n_part,
                                                            const double* __restrict__ part, const long long* __restrict__ cnt) {
  lr_stats_final_body(st, C, D, pass, balanced, n_part, part, cnt);
}

// The posterior's scores of a row into p[0..C): R parameter rows W [R][D + 1] (coefficients, then the intercept), R = 1 for
// two classes (scores (-d, d)); NaN for a row that read nothing.  Shared with the batched score.
__device__ __forceinline__ void post_scores(const double x[kMaxD], bool ok, int C, int D, int R, const double* mean, const double* scale,
                                            const double* W, double* p) {
  double u[kMaxD];
  if (ok) {
    row_scores(x, D, R, mean, scale, W, D + 1, true, u, p, 1);
    if (R == 1) { p[1] = p[0]; p[0] = -p[1]; }
  } else {
    for (int c = 0; c < C; ++c) p[c] = quiet_nan();
  }
}

__device__ __forceinline__ int first_max(const double* p, int C) {
  int best = 0;
  for (int c = 1; c < C; ++c) best = p[c] > p[best] ? c : best;
  return best;
}

// ---- posterior of given rows: one thread per row, every output optional.
// model: mean [D], scale [D], W [R][D], b [R]; R = 1 for two classes (scikit-learn's coef_ [1, D]: scores (-d, d)), else C.
__global__ __launch_bounds__(kRows) void lr_posterior_kernel(Rows a, const double* __restrict__ model, int normal, double* __restrict__ dec_out,
                                                             double* __restrict__ proba_out, long long* __restrict__ pred_out,
                                                             double* __restrict__ pf_out) {
  __shared__ double s_p[kRows * kMaxC];
  __shared__ double s_mean[kMaxD], s_scale[kMaxD], s_W[kMaxC * (kMaxD + 1)];
  const int C = a.K, D = a.D, Cp = C | 1, R = C == 2 ? 1 : C, t = threadIdx.x;
  if (t < D) { s_mean[t] = model[t]; s_scale[t] = model[D + t]; }
  for (int e = t; e < R * (D + 1); e += kRows) {
    const int r = e / (D + 1), i = e - r * (D + 1);
    s_W[e] = i < D ? model[2 * D + r * D + i] : model[2 * D + R * D + r];
  }
  __syncthreads();
  const long long j = (long long)blockIdx.x * kRows + t;
  if (j >= a.n) return;
  double x[kMaxD];
  const bool ok = load_row(a, j, x);
  double* p = s_p + t * Cp;
  post_scores(x, ok, C, D, R, s_mean, s_scale, s_W, p);
  if (dec_out) {
    if (R == 1) dec_out[j] = p[1];
    else for (int c = 0; c < C; ++c) dec_out[j * C + c] = p[c];
  }
  const int best = first_max(p, C);
  if (pred_out) pred_out[j] = ok ? best : -1;
  if (proba_out || pf_out) {
    if (ok) softmax_inplace(p, C);
    if (proba_out)
      for (int c = 0; c < C; ++c) proba_out[j * C + c] = p[c];
    if (pf_out) pf_out[j] = 1.0 - p[normal];
  }
}

// ---- ROC.  Scores come sorted descending; element i closes a group of equal scores when score[i] != score[i + 1].
// Integer scans with tile sums: a launch sums tiles, a one-workgroup launch scans the tile sums, a launch rescans its tile
// with the offset.  Stage 1 compacts (fps, tps, threshold) at the boundaries; stage 2 keeps the corners
// (drop_intermediate) and divides.
constexpr int kTile = 256;

__device__ __forceinline__ void block_scan2(long long* sa, long long* sb, int t) {      // inclusive, in place, kTile entries
  for (int off = 1; off < kTile; off <<= 1) {
    const long long va = t >= off ? sa[t - off] : 0, vb = t >= off ? sb[t - off] : 0;
    __syncthreads();
    sa[t] += va; sb[t] += vb;
    __syncthreads();
  }
}

__device__ __forceinline__ bool roc_boundary(const double* score, long long i, long long n) {
  return i == n - 1 || score[i] != score[i + 1];
}

__global__ __launch_bounds__(kTile) void roc_tiles1_kernel(const double* __restrict__ score, const long long* __restrict__ pos, long long n,
                                                           long long* __restrict__ tile_pos, long long* __restrict__ tile_flag) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x;
  const long long i = (long long)blockIdx.x * kTile + t;
  sa[t] = i < n ? (pos[i] != 0) : 0;
  sb[t] = i < n ? roc_boundary(score, i, n) : 0;
  __syncthreads();
  block_scan2(sa, sb, t);
  if (t == kTile - 1) { tile_pos[blockIdx.x] = sa[t]; tile_flag[blockIdx.x] = sb[t]; }
}

// exclusive scan of nt tile sums in place (both arrays; b may be NULL); totals to tot_a / tot_b.  One workgroup.
__global__ __launch_bounds__(kTile) void roc_scan_tiles_kernel(long long* __restrict__ a, long long* __restrict__ b, long long nt,
                                                               long long* __restrict__ tot_a, long long* __restrict__ tot_b) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x;
  const long long per = (nt + kTile - 1) / kTile, lo = t * per, hi = lo + per < nt ? lo + per : nt;
  long long xa = 0, xb = 0;
  for (long long k = lo; k < hi; ++k) { xa += a[k]; if (b) xb += b[k]; }
  sa[t] = xa; sb[t] = xb;
  __syncthreads();
  block_scan2(sa, sb, t);
  long long ra = sa[t] - xa, rb = sb[t] - xb;
  for (long long k = lo; k < hi; ++k) {
    const long long va = a[k];
    a[k] = ra; ra += va;
    if (b) { const long long vb = b[k]; b[k] = rb; rb += vb; }
  }
  if (t == kTile - 1) { *tot_a = sa[t]; if (tot_b) *tot_b = sb[t]; }
}

__global__ __launch_bounds__(kTile) void roc_emit1_kernel(const double* __restrict__ score, const long long* __restrict__ pos, long long n,
                                                          const long long* __restrict__ tile_pos, const long long* __restrict__ tile_flag,
                                                          long long* __restrict__ fps, long long* __restrict__ tps, double* __restrict__ thr) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x;
  const long long i = (long long)blockIdx.x * kTile + t;
  const bool bd = i < n && roc_boundary(score, i, n);
  sa[t] = i < n ? (pos[i] != 0) : 0;
  sb[t] = bd;
  __syncthreads();
  block_scan2(sa, sb, t);
  if (bd) {
    const long long k = tile_flag[blockIdx.x] + sb[t] - 1, tp = tile_pos[blockIdx.x] + sa[t];
    tps[k] = tp;
    fps[k] = 1 + i - tp;
    thr[k] = score[i];
  }
}

// per boundary k < m: the area term dfps (tps[k - 1] + tps[k]) and the corner flag; tile sums of both
__global__ __launch_bounds__(kTile) void roc_tiles2_kernel(const long long* __restrict__ fps, const long long* __restrict__ tps,
                                                           const long long* __restrict__ d_m, int drop, long long* __restrict__ keep,
                                                           long long* __restrict__ tile_keep, long long* __restrict__ tile_area) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x;
  const long long m = *d_m, k = (long long)blockIdx.x * kTile + t;
  long long kp = 0, area = 0;
  if (k < m) {
    const long long f0 = k > 0 ? fps[k - 1] : 0, t0 = k > 0 ? tps[k - 1] : 0;
    area = (fps[k] - f0) * (t0 + tps[k]);
    kp = 1;
    if (drop && m > 2 && k > 0 && k < m - 1)
      kp = (fps[k + 1] - 2 * fps[k] + fps[k - 1]) != 0 || (tps[k + 1] - 2 * tps[k] + tps[k - 1]) != 0;
    keep[k] = kp;
  }
  sa[t] = kp; sb[t] = area;
  __syncthreads();
  block_scan2(sa, sb, t);
  if (t == kTile - 1) { tile_keep[blockIdx.x] = sa[t]; tile_area[blockIdx.x] = sb[t]; }
}

__global__ __launch_bounds__(kTile) void roc_emit2_kernel(const long long* __restrict__ fps, const long long* __restrict__ tps,
                                                          const double* __restrict__ thr, const long long* __restrict__ keep,
                                                          const long long* __restrict__ tile_keep, long long n, long long* __restrict__ cnt,
                                                          long long* __restrict__ o_fps, long long* __restrict__ o_tps, double* __restrict__ o_thr,
                                                          double* __restrict__ o_fpr, double* __restrict__ o_tpr) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x;
  const long long m = cnt[PINN_LR_ROC_M], k = (long long)blockIdx.x * kTile + t;
  const long long kp = k < m ? keep[k] : 0;
  sa[t] = kp; sb[t] = 0;
  __syncthreads();
  block_scan2(sa, sb, t);
  if (kp) {
    // output point 0 is scikit-learn's (0, 0, inf)
    const long long q = 1 + tile_keep[blockIdx.x] + sa[t] - 1;
    const long long P = cnt[PINN_LR_ROC_POS], N = n - P;
    if (o_fps) o_fps[q] = fps[k];
    if (o_tps) o_tps[q] = tps[k];
    if (o_thr) o_thr[q] = thr[k];
    if (o_fpr) o_fpr[q] = N > 0 ? (double)fps[k] / (double)N : quiet_nan();
    if (o_tpr) o_tpr[q] = P > 0 ? (double)tps[k] / (double)P : quiet_nan();
  }
  if (k == 0) {
    cnt[PINN_LR_ROC_N] = n - cnt[PINN_LR_ROC_POS];
    if (o_fps) o_fps[0] = 0;
    if (o_tps) o_tps[0] = 0;
    if (o_thr) o_thr[0] = INFINITY;
    if (o_fpr) o_fpr[0] = 0.0;
    if (o_tpr) o_tpr[0] = 0.0;
  }
}

// ---- batches of models over column subsets (feature selection).  Candidate c: n_feat[c] columns cols[c][0..n_feat[c]) of
// the shared array, state block c * stride words into the states, its own totals, partials and class-count partials in
// the workspace.  Every kernel below places a candidate's workgroups as the single launch places them (blockIdx.x of
// gridDim.x) and calls the single model's body: the bytes of a candidate are those of the single-model calls.
struct Batch {
  const int* n_feat;          // device, [n_batch]
  const int* cols;            // device, [n_batch][max_feat]
  int max_feat;
  size_t stride;              // words of a state block
  size_t tot_w, part_w, cnt_w;   // words of a candidate's totals, partials and count partials
};

__device__ __forceinline__ int batch_feat(const Batch& b, int c) {
  const int D = b.n_feat[c];
  return D >= 1 && D <= b.max_feat ? D : 1;
}

// The rows of candidate c.  A column outside [0, ld) reads nothing for any row, as a gather index outside the array does.
__device__ __forceinline__ Rows batch_rows(const Rows& base, const Batch& b, int c) {
  Rows a = base;
  const int D = batch_feat(b, c);
  bool ok = D == b.n_feat[c];
  a.D = D;
#pragma unroll
  for (int i = 0; i < kMaxD; ++i) {
    int col = i < D ? b.cols[(size_t)c * b.max_feat + i] : 0;
    if (col < 0 || col >= base.ld) { ok = false; col = 0; }
    a.col[i] = col;
  }
  if (!ok) a.n_arr = 0;
  return a;
}

__global__ __launch_bounds__(kRows) void lr_batch_stats_kernel(Rows base, Batch b, const double* __restrict__ st_all,
                                                               const long long* __restrict__ y_in, int pass, double* __restrict__ part_all,
                                                               long long* __restrict__ cnt_all) {
  const int c = blockIdx.y;
  const Rows a = batch_rows(base, b, c);
  lr_stats_body(a, st_all + c * b.stride, y_in, pass, part_all + c * b.part_w, cnt_all + c * b.cnt_w, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64) void lr_batch_stats_final_kernel(Batch b, double* __restrict__ st_all, int C, int pass, int balanced, int n_part,
                                                                  const double* __restrict__ part_all, const long long* __restrict__ cnt_all) {
  const int c = blockIdx.x;
  lr_stats_final_body(st_all + c * b.stride, C, batch_feat(b, c), pass, balanced, n_part, part_all + c * b.part_w, cnt_all + c * b.cnt_w);
}

__global__ __launch_bounds__(kRows) void lr_batch_rows_kernel(Rows base, Batch b, const double* __restrict__ st_all,
                                                              const long long* __restrict__ y_in, double* __restrict__ part_all) {
  const int c = blockIdx.y;
  const double* st = st_all + c * b.stride;
  if (stopped(st)) return;                                    // before the candidate's columns are even read
  const Rows a = batch_rows(base, b, c);
  lr_rows_body(a, st, y_in, 0, part_all + c * b.part_w, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(kFinThreads) void lr_batch_final_kernel(Batch b, double* __restrict__ st_all, int C, int n_part, long long n,
                                                                     double tol, double l2, int fit_intercept,
                                                                     const double* __restrict__ part_all, double* __restrict__ tot_all) {
  const int c = blockIdx.x;
  lr_final_body(st_all + c * b.stride, C, batch_feat(b, c), FIN_NEWTON, n_part, n, tol, l2, fit_intercept, part_all + c * b.part_w,
                tot_all + c * b.tot_w);
}

// Score of a second row set under every candidate's accepted point: the posterior's arithmetic per row (its model block is
// the state's mean, scale and accepted point; for two classes the row of class 1), then -log p[y], the hit and p_fault.
// A workgroup adds the terms of a tile in row order and its tiles in order; loss partials [gridDim.x], then hit partials.
__global__ __launch_bounds__(kRows) void lr_batch_score_kernel(Rows base, Batch b, const double* __restrict__ st_all,
                                                               const long long* __restrict__ y_in, int normal, double* __restrict__ pf_out,
                                                               double* __restrict__ part_all) {
  __shared__ double s_p[kRows * kMaxC];
  __shared__ double s_mean[kMaxD], s_scale[kMaxD], s_W[kMaxC * (kMaxD + 1)];
  __shared__ double s_l[kRows];
  __shared__ int s_h[kRows];
  const int c = blockIdx.y, t = threadIdx.x;
  const double* st = st_all + c * b.stride;
  const Rows a = batch_rows(base, b, c);
  const int C = a.K, D = a.D, Cp = C | 1, R = C == 2 ? 1 : C;
  if (t < D) { s_mean[t] = st[st_mean(C, D) + t]; s_scale[t] = st[st_scale(C, D) + t]; }
  for (int e = t; e < R * (D + 1); e += kRows) s_W[e] = st[st_prev(C, D) + (R == 1 ? D + 1 : 0) + e];
  __syncthreads();
  double loss = 0.0;
  long long hits = 0;
  const long long tiles = (a.n + kRows - 1) / kRows;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long j = tile * kRows + t;
    double term = 0.0;
    int hit = 0;
    if (j < a.n) {
      double x[kMaxD];
      const bool ok = load_row(a, j, x);
      const long long cls = y_in[j];
      double* p = s_p + t * Cp;
      post_scores(x, ok, C, D, R, s_mean, s_scale, s_W, p);
      const int best = first_max(p, C);
      if (ok) softmax_inplace(p, C);
      if (pf_out) pf_out[(size_t)c * a.n + j] = 1.0 - p[normal];
      if (ok && cls >= 0 && cls < C) {                        // a class outside [0, C) adds nothing
        term = -log(p[cls]);
        hit = best == cls;
      }
    }
    s_l[t] = term;
    s_h[t] = hit;
    __syncthreads();
    if (t == 0) {
      for (int rr = 0; rr < kRows; ++rr) loss += s_l[rr];
    } else if (t == 64) {
      for (int rr = 0; rr < kRows; ++rr) hits += s_h[rr];
    }
    __syncthreads();
  }
  double* part = part_all + c * b.part_w;
  if (t == 0) part[blockIdx.x] = loss;
  else if (t == 64) reinterpret_cast<long long*>(part)[gridDim.x + blockIdx.x] = hits;
}

__global__ __launch_bounds__(64) void lr_batch_score_final_kernel(Batch b, int n_part, const double* __restrict__ part_all,
                                                                  double* __restrict__ loss_out, long long* __restrict__ hits_out) {
  const int c = blockIdx.x, t = threadIdx.x;
  const double* part = part_all + c * b.part_w;
  if (t == 0) {
    double s = 0.0;
    for (int k = 0; k < n_part; ++k) s += part[k];
    loss_out[c] = s;
  } else if (t == 1) {
    long long s = 0;
    for (int k = 0; k < n_part; ++k) s += reinterpret_cast<const long long*>(part)[n_part + k];
    hits_out[c] = s;
  }
}

// The integers of pinn_lr_roc for n_batch rows of sorted scores, one workgroup per row walking its tiles in order.  Carried
// from tile to tile: the positives so far and the last boundary (index and positives through it).  A boundary adds
// dfps (tps_prev + tps), which needs the boundary before it: the one compacted just before it in this tile, or the carried one.
__global__ __launch_bounds__(kTile) void roc_batch_kernel(const double* __restrict__ score_all, const long long* __restrict__ pos_all, long long n,
                                                          long long* __restrict__ counts_all) {
  __shared__ long long sa[kTile], sb[kTile];
  __shared__ int s_bidx[kTile];
  const int t = threadIdx.x;
  const double* score = score_all + (size_t)blockIdx.x * n;
  const long long* pos = pos_all + (size_t)blockIdx.x * n;
  long long carry_tp = 0, last_idx = -1, last_tp = 0, area = 0, m = 0;
  for (long long base = 0; base < n; base += kTile) {
    const long long i = base + t;
    const bool bd = i < n && roc_boundary(score, i, n);
    sa[t] = i < n ? (pos[i] != 0) : 0;
    sb[t] = bd;
    __syncthreads();
    block_scan2(sa, sb, t);
    if (bd) s_bidx[sb[t] - 1] = t;
    __syncthreads();
    if (bd) {
      const long long k = sb[t] - 1, tp = carry_tp + sa[t], fp = 1 + i - tp;
      long long tp0 = last_tp, fp0 = last_idx + 1 - last_tp;
      if (k > 0) {
        const int q = s_bidx[k - 1];
        tp0 = carry_tp + sa[q];
        fp0 = 1 + base + q - tp0;
      }
      area += (fp - fp0) * (tp0 + tp);
      m += 1;
    }
    const long long nb = sb[kTile - 1];
    if (nb > 0) {
      const int q = s_bidx[nb - 1];
      last_idx = base + q;
      last_tp = carry_tp + sa[q];
    }
    carry_tp += sa[kTile - 1];
    __syncthreads();
  }
  sa[t] = area; sb[t] = m;
  __syncthreads();
  block_scan2(sa, sb, t);
  if (t == kTile - 1) {
    long long* cnt = counts_all + (size_t)blockIdx.x * PINN_LR_ROC_COUNTS;
    cnt[PINN_LR_ROC_POS] = carry_tp;
    cnt[PINN_LR_ROC_N] = n - carry_tp;
    cnt[PINN_LR_ROC_M] = sb[t];
    cnt[PINN_LR_ROC_KEPT] = 0;
    cnt[PINN_LR_ROC_U2] = sa[t];
    for (int k = PINN_LR_ROC_U2 + 1; k < PINN_LR_ROC_COUNTS; ++k) cnt[k] = 0;
  }
}

struct Ws {
  double *tot, *part;
  long long* cnt;
};

// workspace: totals [n_sums] (first, so that the caller can read the summed pass), partials, class-count partials
inline Ws carve(void* d_ws, int C, int D) {
  char* w = static_cast<char*>(d_ws);
  Ws s;
  const size_t n_sums = 1 + (size_t)n_par(C, D) + n_hess(C, D);
  s.tot = reinterpret_cast<double*>(w); w += align256(n_sums * sizeof(double));
  s.part = reinterpret_cast<double*>(w); w += align256((size_t)kMaxBlocks * n_sums * sizeof(double));
  s.cnt = reinterpret_cast<long long*>(w);
  return s;
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_lr_state_bytes(int n_classes, int n_feat) {
  if (!pinn::in_limits(n_classes, n_feat)) return 0;
  return pinn::st_words(n_classes, n_feat) * sizeof(double);
}

extern "C" size_t pinn_lr_workspace_bytes(long long n_rows, int n_classes, int n_feat) {
  using namespace pinn;
  if (n_rows < 0 || !in_limits(n_classes, n_feat)) return 0;
  const size_t n_sums = 1 + (size_t)n_par(n_classes, n_feat) + n_hess(n_classes, n_feat);
  return align256(n_sums * sizeof(double)) + align256((size_t)kMaxBlocks * n_sums * sizeof(double)) +
         align256((size_t)kMaxBlocks * kMaxC * sizeof(long long));
}

#define LR_COMMON_CHECKS()                                                                          \
  if (!in_limits(n_classes, n_feat)) return PINN_E_ARG;                                             \
  Rows a;                                                                                           \
  {                                                                                                 \
    const int rc_ = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_classes, d_row_index, n, &a);  \
    if (rc_ != PINN_OK) return rc_;                                                                 \
  }                                                                                                 \
  if (!d_state || !d_ws || !d_y || misaligned8(d_state) || misaligned8(d_ws) || misaligned8(d_y)) return PINN_E_ARG; \
  if (n < 1) return PINN_E_ARG;                                                                     \
  if (ws_bytes < pinn_lr_workspace_bytes(n, n_classes, n_feat)) return PINN_E_WORKSPACE;            \
  const Ws w = carve(d_ws, n_classes, n_feat);                                                      \
  hipStream_t st = (hipStream_t)stream;                                                             \
  clear_error()

extern "C" int pinn_lr_scaler(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                              const long long* d_row_index, long long n, const long long* d_y, int n_classes, int balanced,
                              double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  LR_COMMON_CHECKS();
  const int nb = row_blocks(n, kRows, kMaxBlocks);
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(lr_stats_kernel, dim3((unsigned)nb), dim3(kRows), 0, st, a, d_state, d_y, pass, w.part, w.cnt);
    hipLaunchKernelGGL(lr_stats_final_kernel, dim3(1), dim3(64), 0, st, d_state, n_classes, n_feat, pass, balanced, nb, w.part, w.cnt);
  }
  return launch_status();
}

extern "C" int pinn_lr_pass(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                            const long long* d_row_index, long long n, const long long* d_y, int n_classes,
                            const double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  LR_COMMON_CHECKS();
  const int nb = row_blocks(n, kRows, kMaxBlocks);
  hipLaunchKernelGGL(lr_rows_kernel, dim3((unsigned)nb), dim3(kRows), 0, st, a, d_state, d_y, 1, w.part);
  hipLaunchKernelGGL(lr_final_kernel, dim3(1), dim3(kFinThreads), 0, st, const_cast<double*>(d_state), n_classes, n_feat, FIN_SUMS, nb, n,
                     0.0, 0.0, 1, w.part, w.tot);
  return launch_status();
}

extern "C" int pinn_lr_newton(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                              const long long* d_row_index, long long n, const long long* d_y, int n_classes, int n_passes,
                              double tol, double l2, int fit_intercept, double* d_state, void* d_ws, size_t ws_bytes,
                              void* stream) {
  using namespace pinn;
  LR_COMMON_CHECKS();
  if (n_passes < 0 || n_passes > 100000 || !(tol >= 0.0) || !(l2 > 0.0) || !(l2 < INFINITY)) return PINN_E_ARG;
  const int nb = row_blocks(n, kRows, kMaxBlocks);
  for (int it = 0; it < n_passes; ++it) {
    hipLaunchKernelGGL(lr_rows_kernel, dim3((unsigned)nb), dim3(kRows), 0, st, a, d_state, d_y, 0, w.part);
    hipLaunchKernelGGL(lr_final_kernel, dim3(1), dim3(kFinThreads), 0, st, d_state, n_classes, n_feat, FIN_NEWTON, nb, n, tol, l2,
                       fit_intercept, w.part, w.tot);
  }
  return launch_status();
}

extern "C" int pinn_lr_posterior(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                 const long long* d_row_index, long long n, int n_classes, const double* d_model,
                                 int normal_class, double* d_decision, double* d_proba, long long* d_pred, double* d_p_fault,
                                 void* stream) {
  using namespace pinn;
  if (!in_limits(n_classes, n_feat)) return PINN_E_ARG;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_classes, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_model || misaligned8(d_model) || misaligned8(d_decision) || misaligned8(d_proba) || misaligned8(d_pred) || misaligned8(d_p_fault))
    return PINN_E_ARG;
  if (normal_class < 0 || normal_class >= n_classes) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  const long long tiles = (n + kRows - 1) / kRows;
  if (tiles > 0x7fffffffLL) return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(lr_posterior_kernel, dim3((unsigned)tiles), dim3(kRows), 0, (hipStream_t)stream, a, d_model, normal_class,
                     d_decision, d_proba, d_pred, d_p_fault);
  return launch_status();
}

// ROC workspace: tile sums (4 arrays), then fps, tps, thresholds and keep flags at the boundaries, [n] each
extern "C" size_t pinn_lr_roc_workspace_bytes(long long n) {
  using namespace pinn;
  if (n < 0) return 0;
  const size_t nt = (size_t)((n + kTile - 1) / kTile) + 1;
  return 4 * align256(nt * 8) + 4 * align256((size_t)(n + 1) * 8);
}

extern "C" int pinn_lr_roc(const double* d_score_sorted, const long long* d_pos_sorted, long long n, int drop_intermediate,
                           long long* d_counts, long long* d_fps, long long* d_tps, double* d_thresholds, double* d_fpr,
                           double* d_tpr, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (n < 1 || !d_score_sorted || !d_pos_sorted || !d_counts || !d_ws) return PINN_E_ARG;
  if (misaligned8(d_score_sorted) || misaligned8(d_pos_sorted) || misaligned8(d_counts) || misaligned8(d_fps) || misaligned8(d_tps) ||
      misaligned8(d_thresholds) || misaligned8(d_fpr) || misaligned8(d_tpr) || misaligned8(d_ws))
    return PINN_E_ARG;
  if (ws_bytes < pinn_lr_roc_workspace_bytes(n)) return PINN_E_WORKSPACE;
  const long long nt = (n + kTile - 1) / kTile;
  if (nt > 0x7fffffffLL) return PINN_E_ARG;
  char* w = static_cast<char*>(d_ws);
  const size_t tb = align256((size_t)(nt + 1) * 8), nb = align256((size_t)(n + 1) * 8);
  long long* tile_a = reinterpret_cast<long long*>(w); w += tb;
  long long* tile_b = reinterpret_cast<long long*>(w); w += tb;
  long long* tile_c = reinterpret_cast<long long*>(w); w += tb;
  long long* tile_d = reinterpret_cast<long long*>(w); w += tb;
  long long* fps = reinterpret_cast<long long*>(w); w += nb;
  long long* tps = reinterpret_cast<long long*>(w); w += nb;
  double* thr = reinterpret_cast<double*>(w); w += nb;
  long long* keep = reinterpret_cast<long long*>(w);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  hipError_t e = hipMemsetAsync(d_counts, 0, PINN_LR_ROC_COUNTS * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)nt), block(kTile);
  hipLaunchKernelGGL(roc_tiles1_kernel, grid, block, 0, st, d_score_sorted, d_pos_sorted, n, tile_a, tile_b);
  hipLaunchKernelGGL(roc_scan_tiles_kernel, dim3(1), block, 0, st, tile_a, tile_b, nt, d_counts + PINN_LR_ROC_POS, d_counts + PINN_LR_ROC_M);
  hipLaunchKernelGGL(roc_emit1_kernel, grid, block, 0, st, d_score_sorted, d_pos_sorted, n, tile_a, tile_b, fps, tps, thr);
  // the number of boundaries stays on the device: the second stage is launched for n and every workgroup beyond it idles
  hipLaunchKernelGGL(roc_tiles2_kernel, grid, block, 0, st, fps, tps, d_counts + PINN_LR_ROC_M, drop_intermediate, keep, tile_c, tile_d);
  hipLaunchKernelGGL(roc_scan_tiles_kernel, dim3(1), block, 0, st, tile_c, tile_d, nt, d_counts + PINN_LR_ROC_KEPT, d_counts + PINN_LR_ROC_U2);
  hipLaunchKernelGGL(roc_emit2_kernel, grid, block, 0, st, fps, tps, thr, keep, tile_c, n, d_counts, d_fps, d_tps, d_thresholds, d_fpr, d_tpr);
  return launch_status();
}

// ---- batches of models over column subsets
namespace pinn {
namespace {

inline size_t batch_sums(int C, int max_feat) { return 1 + (size_t)n_par(C, max_feat) + n_hess(C, max_feat); }
inline size_t words256(size_t words) { return align256(words * 8) / 8; }

struct BatchWs {
  double *tot, *part;
  long long* cnt;
};

// Everything the batch entry points check before a launch; fills the rows head (without columns), the batch and the workspace.
inline int make_batch(const double* d_arr, long long ld, long long n_arr_rows, const long long* d_row_index, long long n, int n_classes,
                      int n_batch, const int* n_feat, const int* cols, int max_feat, const int* d_n_feat, const int* d_cols,
                      const void* d_state, void* d_ws, size_t ws_bytes, Rows* a, Batch* b, BatchWs* w, int* nb_out) {
  if (n_batch < 1 || n_batch > PINN_LR_MAX_BATCH || !in_limits(n_classes, max_feat)) return PINN_E_ARG;
  if (!n_feat || !cols || !d_n_feat || !d_cols || !d_state || !d_ws || misaligned8(d_state) || misaligned8(d_ws)) return PINN_E_ARG;
  if (((unsigned long long)d_n_feat & 3) || ((unsigned long long)d_cols & 3)) return PINN_E_ARG;
  const int col0 = 0;
  const int rc = make_rows(d_arr, ld, n_arr_rows, &col0, 1, n_classes, d_row_index, n, a);
  if (rc != PINN_OK) return rc;
  if (n < 1) return PINN_E_ARG;
  for (int c = 0; c < n_batch; ++c) {
    if (n_feat[c] < 1 || n_feat[c] > max_feat) return PINN_E_ARG;
    for (int i = 0; i < n_feat[c]; ++i) {
      const int col = cols[(size_t)c * max_feat + i];
      if (col < 0 || col >= ld) return PINN_E_ARG;
    }
  }
  if (ws_bytes < pinn_lr_batch_workspace_bytes(n, n_batch, n_classes, max_feat)) return PINN_E_WORKSPACE;
  const int nb = row_blocks(n, kRows, kMaxBlocks);
  const size_t ns = batch_sums(n_classes, max_feat);
  b->n_feat = d_n_feat; b->cols = d_cols; b->max_feat = max_feat;
  b->stride = pinn_lr_batch_state_stride(n_classes, max_feat) / 8;
  b->tot_w = words256(ns); b->part_w = words256((size_t)nb * ns); b->cnt_w = words256((size_t)nb * kMaxC);
  w->tot = static_cast<double*>(d_ws);
  w->part = w->tot + (size_t)n_batch * b->tot_w;
  w->cnt = reinterpret_cast<long long*>(w->part + (size_t)n_batch * b->part_w);
  *nb_out = nb;
  return PINN_OK;
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_lr_batch_state_stride(int n_classes, int max_feat) {
  if (!pinn::in_limits(n_classes, max_feat)) return 0;
  return pinn::align256(pinn::st_words(n_classes, max_feat) * sizeof(double));
}

extern "C" size_t pinn_lr_batch_workspace_bytes(long long n_rows, int n_batch, int n_classes, int max_feat) {
  using namespace pinn;
  if (n_rows < 0 || n_batch < 1 || n_batch > PINN_LR_MAX_BATCH || !in_limits(n_classes, max_feat)) return 0;
  const size_t nb = (size_t)row_blocks(n_rows, kRows, kMaxBlocks), ns = batch_sums(n_classes, max_feat);
  return (size_t)n_batch * 8 * (words256(ns) + words256(nb * ns) + words256(nb * kMaxC));
}

#define LR_BATCH_CHECKS(state_ptr)                                                                                        \
  Rows a;                                                                                                                 \
  Batch b;                                                                                                                \
  BatchWs w;                                                                                                              \
  int nb = 0;                                                                                                             \
  {                                                                                                                       \
    const int rc_ = make_batch(d_arr, ld, n_arr_rows, d_row_index, n, n_classes, n_batch, n_feat, cols, max_feat, d_n_feat, d_cols, \
                               state_ptr, d_ws, ws_bytes, &a, &b, &w, &nb);                                               \
    if (rc_ != PINN_OK) return rc_;                                                                                       \
  }                                                                                                                       \
  if (!d_y || misaligned8(d_y)) return PINN_E_ARG;                                                                        \
  hipStream_t st = (hipStream_t)stream;                                                                                   \
  clear_error()

extern "C" int pinn_lr_batch_scaler(const double* d_arr, long long ld, long long n_arr_rows, const long long* d_row_index, long long n,
                                    const long long* d_y, int n_classes, int n_batch, const int* n_feat, const int* cols, int max_feat,
                                    const int* d_n_feat, const int* d_cols, int balanced, double* d_state, void* d_ws, size_t ws_bytes,
                                    void* stream) {
  using namespace pinn;
  LR_BATCH_CHECKS(d_state);
  const dim3 grid((unsigned)nb, (unsigned)n_batch);
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(lr_batch_stats_kernel, grid, dim3(kRows), 0, st, a, b, d_state, d_y, pass, w.part, w.cnt);
    hipLaunchKernelGGL(lr_batch_stats_final_kernel, dim3((unsigned)n_batch), dim3(64), 0, st, b, d_state, n_classes, pass, balanced, nb, w.part,
                       w.cnt);
  }
  return launch_status();
}

extern "C" int pinn_lr_batch_newton(const double* d_arr, long long ld, long long n_arr_rows, const long long* d_row_index, long long n,
                                    const long long* d_y, int n_classes, int n_batch, const int* n_feat, const int* cols, int max_feat,
                                    const int* d_n_feat, const int* d_cols, int n_passes, double tol, double l2, int fit_intercept,
                                    double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  LR_BATCH_CHECKS(d_state);
  if (n_passes < 0 || n_passes > 100000 || !(tol >= 0.0) || !(l2 > 0.0) || !(l2 < INFINITY)) return PINN_E_ARG;
  const dim3 grid((unsigned)nb, (unsigned)n_batch);
  for (int it = 0; it < n_passes; ++it) {
    hipLaunchKernelGGL(lr_batch_rows_kernel, grid, dim3(kRows), 0, st, a, b, d_state, d_y, w.part);
    hipLaunchKernelGGL(lr_batch_final_kernel, dim3((unsigned)n_batch), dim3(kFinThreads), 0, st, b, d_state, n_classes, nb, n, tol, l2,
                       fit_intercept, w.part, w.tot);
  }
  return launch_status();
}

extern "C" int pinn_lr_batch_score(const double* d_arr, long long ld, long long n_arr_rows, const long long* d_row_index, long long n,
                                   const long long* d_y, int n_classes, int n_batch, const int* n_feat, const int* cols, int max_feat,
                                   const int* d_n_feat, const int* d_cols, const double* d_state, int normal_class, double* d_loss_sum,
                                   long long* d_hits, double* d_p_fault, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  LR_BATCH_CHECKS(d_state);
  if (!d_loss_sum || !d_hits || misaligned8(d_loss_sum) || misaligned8(d_hits) || misaligned8(d_p_fault)) return PINN_E_ARG;
  if (normal_class < 0 || normal_class >= n_classes) return PINN_E_ARG;
  hipLaunchKernelGGL(lr_batch_score_kernel, dim3((unsigned)nb, (unsigned)n_batch), dim3(kRows), 0, st, a, b, d_state, d_y, normal_class,
                     d_p_fault, w.part);
  hipLaunchKernelGGL(lr_batch_score_final_kernel, dim3((unsigned)n_batch), dim3(64), 0, st, b, nb, w.part, d_loss_sum, d_hits);
  return launch_status();
}

extern "C" int pinn_lr_batch_auc(const double* d_score_sorted, const long long* d_pos_sorted, long long n, int n_batch, long long* d_counts,
                                 void* stream) {
  using namespace pinn;
  if (n < 1 || n_batch < 1 || n_batch > PINN_LR_MAX_BATCH || !d_score_sorted || !d_pos_sorted || !d_counts) return PINN_E_ARG;
  if (misaligned8(d_score_sorted) || misaligned8(d_pos_sorted) || misaligned8(d_counts)) return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(roc_batch_kernel, dim3((unsigned)n_batch), dim3(kTile), 0, (hipStream_t)stream, d_score_sorted, d_pos_sorted, n, d_counts);
  return launch_status();
}
