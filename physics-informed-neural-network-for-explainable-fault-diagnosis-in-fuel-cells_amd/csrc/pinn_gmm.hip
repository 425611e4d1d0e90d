// Full-covariance Gaussian mixture for fault diagnosis on the device (reference script 03, cited as 03:<line>):
//   pinn_gmm_mstep_init  parameters from initial responsibilities or labels (scikit-learn's _initialize)
//   pinn_gmm_em          EM iterations without a host synchronisation between them, with scikit-learn's stopping rule
//   pinn_gmm_posterior   log_prob_norm, responsibilities, fault probabilities and argmax per row        (03:416-424)
//   pinn_gmm_label_map   P(fault | component) from training rows                                        (03:394-414)
//   pinn_gmm_kmeans      Lloyd iterations for the package's own initialisation
//   pinn_gmm_batch_*     the same for up to 1024 candidates (component count x seed) at once, with the k-means++ seeding and
//                        a log-likelihood sum per candidate: model selection (pinn_amd.selection)
// All arithmetic is float64.
//
// One row pass serves all of them: a workgroup takes tiles of 128 rows, one thread per row writes the row's weights over
// the K components (responsibilities of the E-step, given responsibilities, a one-hot label, or the nearest centre) into
// LDS; then every thread owns up to 12 of the K x F output sums and adds the tile's 128 terms to them in row order.  The
// F columns are (1, d, d d^T upper triangle) with d = x - mean_k of the state the pass started from: second moments are
// accumulated about the previous mean and corrected by the mean's move, never as raw moments.  Workgroup sums go to the
// workspace; a one-workgroup launch adds them in index order, does the M-step and the K Cholesky factorisations, the lower
// bound and the convergence test.  No float atomics, no workgroup waits on another: stream order is the only dependency,
// and the same call gives the same bytes every time.  Once the state's converged flag or status word is set every later
// launch returns at once and the parameters stay as they are.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_rows.h"
#include "pinn_gmm_state.h"

namespace pinn {
namespace {

constexpr int kRows = 128;                  // rows per tile = threads per workgroup of the row pass
constexpr int kMaxK = PINN_GMM_MAX_COMP, kMaxD = PINN_GMM_MAX_FEAT, kMaxC = PINN_GMM_MAX_CLASSES;
constexpr int kTri = kMaxD * (kMaxD + 1) / 2;
constexpr int kMaxOut = (kMaxK * (1 + kMaxD + kTri) + kRows - 1) / kRows;      // output sums per thread: 12
constexpr int kMaxBlocks = 1024;            // workgroups of a row pass = partial sums per output
constexpr int kFinThreads = 256;

enum { SRC_ESTEP = 0, SRC_RESP = 1, SRC_LABELS = 2, SRC_NEAREST = 3 };
enum { OUT_MOMENTS = 0, OUT_CLASS = 1 };
enum { FIN_MEANS = 0, FIN_INIT = 1, FIN_EM = 2, FIN_KMEANS = 3, FIN_MAP = 4 };

__device__ __forceinline__ bool stopped(const double* st) {
  const long long* h = reinterpret_cast<const long long*>(st);
  return h[PINN_GMM_ST_CONVERGED] != 0 || h[PINN_GMM_ST_STATUS] != 0;
}

// ---- the row pass: K x F sums per workgroup.  F = n_f columns; OUT_MOMENTS: (1, d_i, d_i d_j i <= j) cut to n_f, OUT_CLASS:
// one column per class.  part: [gridDim.x][K * n_f]; part_l: [gridDim.x] sums of log_prob_norm (SRC_ESTEP) or of the
// squared distance to the nearest centre (SRC_NEAREST).
__device__ __forceinline__ void rows_pass(const Rows& a, const double* __restrict__ st, int src, int out, int n_f,
                                          const double* __restrict__ resp_in, const long long* __restrict__ lab_in,
                                          const long long* __restrict__ cls_in, long long* __restrict__ lab_out, int force,
                                          double* __restrict__ part, double* __restrict__ part_l) {
  __shared__ double s_r[kRows * (kMaxK + 1)];
  __shared__ double s_x[kRows * (kMaxD + 1)];
  __shared__ double s_mu[kMaxK * kMaxD], s_U[kMaxK * kTri], s_ld[kMaxK], s_lw[kMaxK];
  __shared__ double s_l[kRows];
  __shared__ int s_cls[kRows];
  if (!force && stopped(st)) return;
  const int K = a.K, D = a.D, Kp = K | 1, Dp = D | 1, t = threadIdx.x;
  const Staged sp{s_mu, s_U, s_ld, s_lw};
  stage_params(st, K, D, sp, src == SRC_ESTEP);

  // the outputs of this thread: o = t + q kRows -> (component, column)
  const int KF = K * n_f;
  int ok_[kMaxOut], oi[kMaxOut], oj[kMaxOut];
  double acc[kMaxOut];
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q) {
    const int o = t + q * kRows;
    acc[q] = 0.0;
    ok_[q] = -1; oi[q] = -1; oj[q] = -1;
    if (o < KF) {
      const int k = o / n_f, f = o - k * n_f;
      ok_[q] = k;
      if (out == OUT_CLASS) {
        oi[q] = f;
      } else if (f >= 1 && f <= D) {
        oi[q] = f - 1;
      } else if (f > D) {
        untri(f - 1 - D, &oi[q], &oj[q]);
      }
    }
  }

  double lsum = 0.0;
  const long long tiles = (a.n + kRows - 1) / kRows;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long j = tile * kRows + t;
    double x[kMaxD];
    bool ok = false;
    if (j < a.n) ok = load_row(a, j, x);
    else {
#pragma unroll
      for (int i = 0; i < kMaxD; ++i) x[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < kMaxD; ++i)
      if (i < D) s_x[t * Dp + i] = x[i];
    double* r = s_r + t * Kp;
    if (!ok) {
      for (int k = 0; k < K; ++k) r[k] = 0.0;
    } else if (src == SRC_ESTEP) {
      const double lpn = estep_row(x, K, D, sp, r, 1);
      for (int k = 0; k < K; ++k) r[k] = exp(r[k] - lpn);
      lsum += lpn;
    } else if (src == SRC_RESP) {
      for (int k = 0; k < K; ++k) r[k] = resp_in[j * K + k];
    } else if (src == SRC_LABELS) {
      const long long l = lab_in[j];
      for (int k = 0; k < K; ++k) r[k] = (l == k) ? 1.0 : 0.0;
    } else {                                                  // nearest centre, the first of equals
      int best = 0;
      double bd = INFINITY;
      for (int k = 0; k < K; ++k) {
        double d2 = 0.0;
#pragma unroll
        for (int i = 0; i < kMaxD; ++i)
          if (i < D) { const double d = x[i] - s_mu[k * D + i]; d2 += d * d; }
        if (d2 < bd) { bd = d2; best = k; }
      }
      for (int k = 0; k < K; ++k) r[k] = (k == best) ? 1.0 : 0.0;
      if (lab_out) lab_out[j] = best;
      lsum += bd;
    }
    if (out == OUT_CLASS) s_cls[t] = (ok && cls_in) ? (int)cls_in[j] : -1;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxOut; ++q) {
      const int k = ok_[q];
      if (k >= 0) {
        const int i = oi[q], jj = oj[q];
        double s = acc[q];
        if (out == OUT_CLASS) {
          for (int rr = 0; rr < kRows; ++rr) s += s_cls[rr] == i ? s_r[rr * Kp + k] : 0.0;
        } else if (i < 0) {
          for (int rr = 0; rr < kRows; ++rr) s += s_r[rr * Kp + k];
        } else if (jj < 0) {
          const double m = s_mu[k * D + i];
          for (int rr = 0; rr < kRows; ++rr) s += s_r[rr * Kp + k] * (s_x[rr * Dp + i] - m);
        } else {
          const double mi = s_mu[k * D + i], mj = s_mu[k * D + jj];
          for (int rr = 0; rr < kRows; ++rr) s += s_r[rr * Kp + k] * ((s_x[rr * Dp + i] - mi) * (s_x[rr * Dp + jj] - mj));
        }
        acc[q] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q)
    if (ok_[q] >= 0) part[(size_t)blockIdx.x * KF + t + q * kRows] = acc[q];
  s_l[t] = lsum;
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int rr = 0; rr < kRows; ++rr) s += s_l[rr];
    part_l[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(kRows) void gmm_rows_kernel(Rows a, const double* __restrict__ st, int src, int out, int n_f,
                                                         const double* __restrict__ resp_in, const long long* __restrict__ lab_in,
                                                         const long long* __restrict__ cls_in, long long* __restrict__ lab_out,
                                                         int force, double* __restrict__ part, double* __restrict__ part_l) {
  rows_pass(a, st, src, out, n_f, resp_in, lab_in, cls_in, lab_out, force, part, part_l);
}

// ---- the M-step of component k from its summed moments m[n_f] about the shift `sh` (the mean the pass started from):
// n_k, the new mean and, unless mode is FIN_MEANS, the covariance about it (+ reg on the diagonal), its Cholesky factor,
// precisions_cholesky and the log-determinant.  Returns 1 when the covariance is not positive definite.
__device__ __forceinline__ int mstep_component(const double* __restrict__ m, const double* __restrict__ sh, int D, int mode, double reg,
                                               double* __restrict__ nk_out, double* __restrict__ mu_out, double* __restrict__ cv,
                                               double* __restrict__ U, double* __restrict__ ld_out) {
  const double eps10 = 10.0 * 2.220446049250313e-16;
  const double s0 = m[0], nk = s0 + eps10, frac = s0 / nk;
  *nk_out = nk;
  double dm[kMaxD], e[kMaxD];
  for (int i = 0; i < D; ++i) {
    dm[i] = m[1 + i] / nk;                                    // sum r (x - shift) / n_k
    const double mu = dm[i] + sh[i] * frac;                   // = sum r x / n_k
    mu_out[i] = mu;
    e[i] = mu - sh[i];
  }
  if (mode == FIN_MEANS) return 0;
  // covariance about the new mean from the moments about the shift: S2 / n_k - e dm^T - dm e^T + (S0 / n_k) e e^T
  for (int j = 0; j < D; ++j)
    for (int i = 0; i <= j; ++i) {
      double v = m[1 + D + tri(i, j)] / nk - e[i] * dm[j] - dm[i] * e[j] + frac * e[i] * e[j];
      if (i == j) v += reg;
      cv[i * D + j] = v;
      cv[j * D + i] = v;
    }
  // Cholesky cov = L L^T, then U = L^-T
  double L[kMaxD][kMaxD];
  for (int j = 0; j < D; ++j) {
    double s = cv[j * D + j];
    for (int p = 0; p < j; ++p) s -= L[j][p] * L[j][p];
    if (!(s > 0.0) || !(s < INFINITY)) return 1;
    const double piv = sqrt(s);
    L[j][j] = piv;
    for (int i = j + 1; i < D; ++i) {
      double v = cv[i * D + j];
      for (int p = 0; p < j; ++p) v -= L[i][p] * L[j][p];
      L[i][j] = v / piv;
    }
  }
  double ld = 0.0;
  for (int c = 0; c < D; ++c) {                               // column c of L^-1 by forward substitution; U[c][r] = Linv[r][c]
    double z[kMaxD];
    for (int r = 0; r < D; ++r) {
      double v = r == c ? 1.0 : 0.0;
      for (int p = c; p < r; ++p) v -= L[r][p] * z[p];
      z[r] = r < c ? 0.0 : v / L[r][r];
      U[c * D + r] = z[r];
    }
  }
  for (int i = 0; i < D; ++i) ld += log(U[i * D + i]);
  *ld_out = ld;
  return ld == ld ? 0 : 1;
}

// ---- sums of the partials in index order, then what the mode asks for.  One workgroup per state.
// tot: [K * n_f] totals (kept in the workspace for the caller), then [1] the total of part_l.
__device__ __forceinline__ void final_pass(double* __restrict__ st, int K, int D, int C, int mode, int n_f, int n_part, long long n,
                                           double reg, double tol, const double* __restrict__ part, const double* __restrict__ part_l,
                                           double* __restrict__ tot, double* __restrict__ map_out) {
  __shared__ double n_mu[kMaxK * kMaxD], n_cov[kMaxK * kMaxD * kMaxD], n_U[kMaxK * kMaxD * kMaxD], n_ld[kMaxK], n_nk[kMaxK];
  __shared__ int s_fail[kMaxK];
  __shared__ double s_sum;
  long long* hdr = reinterpret_cast<long long*>(st);
  if (mode != FIN_MAP && mode != FIN_MEANS && mode != FIN_INIT && stopped(st)) return;
  const int KF = K * n_f, t = threadIdx.x;
  for (int o = t; o < KF; o += kFinThreads) {
    double s = 0.0;
    for (int g = 0; g < n_part; ++g) s += part[(size_t)g * KF + o];
    tot[o] = s;
  }
  if (t == 0) {
    double s = 0.0;
    for (int g = 0; g < n_part; ++g) s += part_l[g];
    tot[KF] = s;
  }
  __syncthreads();

  if (mode == FIN_MAP) {                                      // 03:397-414
    if (t < K) {
      double s = 0.0;
      for (int c = 0; c < C; ++c) s += tot[t * C + c];
      for (int c = 0; c < C; ++c) map_out[t * C + c] = s > 0.0 ? tot[t * C + c] / s : 1.0 / (double)C;
    }
    return;
  }
  const double* mean = st + st_means(K);
  if (mode == FIN_KMEANS) {
    if (t < K) {
      const double s0 = tot[t * n_f];
      int moved = 0;
      for (int i = 0; i < D; ++i) {
        const double old = mean[t * D + i];
        const double nw = s0 > 0.0 ? old + tot[t * n_f + 1 + i] / s0 : old;     // an empty cluster keeps its centre
        n_mu[t * D + i] = nw;
        moved |= nw != old;
      }
      s_fail[t] = moved;
    }
    __syncthreads();
    if (t < K)
      for (int i = 0; i < D; ++i) st[st_means(K) + t * D + i] = n_mu[t * D + i];
    if (t == 0) {
      int moved = 0;
      for (int k = 0; k < K; ++k) moved |= s_fail[k];
      hdr[PINN_GMM_ST_ITER] += 1;
      st[PINN_GMM_ST_LOWER] = tot[KF];                        // inertia of the assignment to the previous centres
      if (!moved) hdr[PINN_GMM_ST_CONVERGED] = 1;
    }
    return;
  }

  if (t < K)
    s_fail[t] = mstep_component(tot + t * n_f, mean + t * D, D, mode, reg, n_nk + t, n_mu + t * D, n_cov + t * D * D, n_U + t * D * D, n_ld + t);
  __syncthreads();
  if (t == 0) {
    int fail = 0;
    double s = 0.0;
    for (int k = 0; k < K; ++k) { fail |= s_fail[k]; s += n_nk[k]; }
    s_sum = s;
    if (fail) hdr[PINN_GMM_ST_STATUS] = PINN_GMM_SINGULAR;
    s_fail[0] = fail;
  }
  __syncthreads();
  if (s_fail[0]) return;                                      // the state keeps the last good parameters
  if (t < K) {
    for (int i = 0; i < D; ++i) st[st_means(K) + t * D + i] = n_mu[t * D + i];
    if (mode != FIN_MEANS) {
      st[st_weights() + t] = n_nk[t] / (mode == FIN_INIT ? (double)n : s_sum);
      for (int i = 0; i < D * D; ++i) {
        st[st_cov(K, D) + (size_t)t * D * D + i] = n_cov[t * D * D + i];
        st[st_chol(K, D) + (size_t)t * D * D + i] = n_U[t * D * D + i];
      }
      st[st_logdet(K, D) + t] = n_ld[t];
    }
  }
  if (t == 0 && mode == FIN_INIT) {
    hdr[PINN_GMM_ST_ITER] = 0;
    hdr[PINN_GMM_ST_K] = K;
    hdr[PINN_GMM_ST_D] = D;
    st[PINN_GMM_ST_LOWER] = -INFINITY;
    st[PINN_GMM_ST_PREV] = -INFINITY;
    st[PINN_GMM_ST_CHANGE] = INFINITY;
  }
  if (t == 0 && mode == FIN_EM) {                             // scikit-learn's loop: mean log_prob_norm of the E-step just done
    const double lb = tot[KF] / (double)n, prev = st[PINN_GMM_ST_LOWER], change = lb - prev;
    st[PINN_GMM_ST_PREV] = prev;
    st[PINN_GMM_ST_LOWER] = lb;
    st[PINN_GMM_ST_CHANGE] = change;
    hdr[PINN_GMM_ST_ITER] += 1;
    if (fabs(change) < tol) hdr[PINN_GMM_ST_CONVERGED] = 1;
  }
}

__global__ __launch_bounds__(kFinThreads) void gmm_final_kernel(double* __restrict__ st, int K, int D, int C, int mode, int n_f, int n_part,
                                                                 long long n, double reg, double tol, const double* __restrict__ part,
                                                                 const double* __restrict__ part_l, double* __restrict__ tot,
                                                                 double* __restrict__ map_out) {
  final_pass(st, K, D, C, mode, n_f, n_part, n, reg, tol, part, part_l, tot, map_out);
}

// ---- a batch of candidates: the same two passes, one more grid dimension.  Candidate c has k[c] components, its state
// block (the single-model layout for its own K) at st + c * st_words and its own block of the workspace: totals, partials
// of n_part workgroups, log-likelihood partials, and the running minimum of squared distances of the seeding.
constexpr int kMaxB = PINN_GMM_MAX_BATCH;
constexpr int kSeedThreads = 256;

struct Batch {
  double* st;
  char* ws;
  size_t st_words, ws_block, off_part, off_l, off_d2;
  int n_batch, n_part;
  unsigned char k[kMaxB];
};

struct BatchWs {
  double *tot, *part, *part_l, *d2;
};

__device__ __forceinline__ BatchWs cand_ws(const Batch& b, int c) {
  char* w = b.ws + (size_t)c * b.ws_block;
  return BatchWs{reinterpret_cast<double*>(w), reinterpret_cast<double*>(w + b.off_part), reinterpret_cast<double*>(w + b.off_l),
                 reinterpret_cast<double*>(w + b.off_d2)};
}

// grid (row blocks, candidates).  lab_in / lab_out: [n_batch][n]
__global__ __launch_bounds__(kRows) void gmm_batch_rows_kernel(Rows a, Batch b, int src, int n_f, const long long* __restrict__ lab_in,
                                                               long long* __restrict__ lab_out, int force) {
  const int c = blockIdx.y;
  a.K = b.k[c];
  const BatchWs w = cand_ws(b, c);
  rows_pass(a, b.st + (size_t)c * b.st_words, src, OUT_MOMENTS, n_f, nullptr, lab_in ? lab_in + (size_t)c * a.n : nullptr, nullptr,
            lab_out ? lab_out + (size_t)c * a.n : nullptr, force, w.part, w.part_l);
}

// one workgroup per candidate
__global__ __launch_bounds__(kFinThreads) void gmm_batch_final_kernel(Batch b, int D, int mode, int n_f, long long n, double reg, double tol) {
  const int c = blockIdx.x;
  const BatchWs w = cand_ws(b, c);
  final_pass(b.st + (size_t)c * b.st_words, b.k[c], D, 0, mode, n_f, b.n_part, n, reg, tol, w.part, w.part_l, w.tot, nullptr);
}

// the log-likelihood partials of a row pass in index order: out[c]
__global__ __launch_bounds__(kFinThreads) void gmm_batch_sum_kernel(Batch b, double* __restrict__ out) {
  const int c = blockIdx.x * kFinThreads + threadIdx.x;
  if (c >= b.n_batch) return;
  const double* pl = cand_ws(b, c).part_l;
  double s = 0.0;
  for (int g = 0; g < b.n_part; ++g) s += pl[g];
  out[c] = s;
}

// ---- k-means++ seeds, one workgroup per candidate: centre 0 is row first[c]; centre k is the first position whose
// inclusive cumulative sum of d2 (the squared distance to the nearest centre so far) exceeds u[c][k - 1] x total, or n - 1
// when none does.  The sum has a fixed order: thread t sums positions [t chunk, (t + 1) chunk) in order, thread 0 adds the
// chunk sums in order, and the cumulative sum at a position is its chunk's offset plus the chunk's running sum.
__global__ __launch_bounds__(kSeedThreads) void gmm_batch_seed_kernel(Rows a, Batch b, int max_comp, const long long* __restrict__ first,
                                                                      const double* __restrict__ u, long long* __restrict__ picks) {
  __shared__ double s_c[kSeedThreads];
  __shared__ long long s_pick;
  const int c = blockIdx.x, K = b.k[c], D = a.D, t = threadIdx.x;
  double* st = b.st + (size_t)c * b.st_words;
  double* d2 = cand_ws(b, c).d2;
  const long long n = a.n, chunk = (n + kSeedThreads - 1) / kSeedThreads;
  const long long lo = (long long)t * chunk < n ? (long long)t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  if (t == 0) {
    long long* hdr = reinterpret_cast<long long*>(st);
    hdr[PINN_GMM_ST_K] = K;
    hdr[PINN_GMM_ST_D] = D;
    st[PINN_GMM_ST_LOWER] = -INFINITY;
    st[PINN_GMM_ST_PREV] = -INFINITY;
    st[PINN_GMM_ST_CHANGE] = INFINITY;
  }
  long long pick = first[c];
  pick = pick < 0 ? 0 : (pick > n - 1 ? n - 1 : pick);
  for (int k = 0; k < K; ++k) {
    double cx[kMaxD];
    load_row(a, pick, cx);
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < kMaxD; ++i)
        if (i < D) st[st_means(K) + k * D + i] = cx[i];
      if (picks) picks[(size_t)c * max_comp + k] = pick;
    }
    if (k == K - 1) break;
    for (long long j = t; j < n; j += kSeedThreads) {
      double x[kMaxD];
      load_row(a, j, x);
      double dd = 0.0;
#pragma unroll
      for (int i = 0; i < kMaxD; ++i)
        if (i < D) { const double d = x[i] - cx[i]; dd += d * d; }
      d2[j] = (k == 0 || dd < d2[j]) ? dd : d2[j];
    }
    __syncthreads();
    double s = 0.0;
    for (long long j = lo; j < hi; ++j) s += d2[j];
    s_c[t] = s;
    __syncthreads();
    if (t == 0) {
      double run = 0.0;
      for (int q = 0; q < kSeedThreads; ++q) { run += s_c[q]; s_c[q] = run; }
      s_pick = n - 1;
    }
    __syncthreads();
    const double target = u[(size_t)c * (max_comp - 1) + k] * s_c[kSeedThreads - 1];
    const double before = t > 0 ? s_c[t - 1] : 0.0;
    if (s_c[t] > target && !(t > 0 && before > target)) {     // the first chunk that passes the target holds the pick
      double run = 0.0;
      for (long long j = lo; j < hi; ++j) {
        run += d2[j];
        if (before + run > target) { s_pick = j; break; }
      }
    }
    __syncthreads();
    pick = s_pick;
  }
}

// ---- posterior of given rows: one thread per row, every output optional
__global__ __launch_bounds__(kRows) void gmm_posterior_kernel(Rows a, const double* __restrict__ st, const double* __restrict__ map, int C,
                                                              double* __restrict__ lpn_out, double* __restrict__ resp_out,
                                                              double* __restrict__ prob_out, long long* __restrict__ pred_out) {
  __shared__ double s_r[kRows * (kMaxK + 1)];
  __shared__ double s_mu[kMaxK * kMaxD], s_U[kMaxK * kTri], s_ld[kMaxK], s_lw[kMaxK];
  __shared__ double s_map[kMaxK * kMaxC];
  const int K = a.K, D = a.D, Kp = K | 1, t = threadIdx.x;
  const Staged sp{s_mu, s_U, s_ld, s_lw};
  if (map)
    for (int e = t; e < K * C; e += kRows) s_map[e] = map[e];
  stage_params(st, K, D, sp, true);
  const long long j = (long long)blockIdx.x * kRows + t;
  if (j >= a.n) return;
  double x[kMaxD];
  const bool ok = load_row(a, j, x);
  double* r = s_r + t * Kp;
  double lpn = quiet_nan();
  if (ok) {
    lpn = estep_row(x, K, D, sp, r, 1);
    for (int k = 0; k < K; ++k) r[k] = exp(r[k] - lpn);
  } else {
    for (int k = 0; k < K; ++k) r[k] = quiet_nan();
  }
  if (lpn_out) lpn_out[j] = lpn;
  if (resp_out)
    for (int k = 0; k < K; ++k) resp_out[j * K + k] = r[k];
  if (map && (prob_out || pred_out)) {                        // 03:418-424
    double y[kMaxC];
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      y[c] = 0.0;
      if (c < C) {
        double v = 0.0;
        for (int k = 0; k < K; ++k) v += r[k] * s_map[k * C + c];
        if (v == v) v = v < 1e-12 ? 1e-12 : (v > 1.0 ? 1.0 : v);
        y[c] = v;
        sum += v;
      }
    }
    int best = 0;
    double bv = -INFINITY;
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) {
      if (c < C) {
        const double v = y[c] / sum;
        if (prob_out) prob_out[j * C + c] = v;
        if (v > bv) { bv = v; best = c; }
      }
    }
    if (pred_out) pred_out[j] = best;
  }
}

inline int n_moments(int D) { return 1 + D + D * (D + 1) / 2; }

struct Ws {
  double *tot, *part, *part_l;
};

// workspace: totals [K F + 1] (first, so that the caller can read the summed moments), partials, log-likelihood partials
inline Ws carve(void* d_ws, int K, int D) {
  char* w = static_cast<char*>(d_ws);
  Ws s;
  const size_t KF = (size_t)K * n_moments(D) > (size_t)K * kMaxC ? (size_t)K * n_moments(D) : (size_t)K * kMaxC;
  s.tot = reinterpret_cast<double*>(w); w += align256((KF + 1) * sizeof(double));
  s.part = reinterpret_cast<double*>(w); w += align256((size_t)kMaxBlocks * KF * sizeof(double));
  s.part_l = reinterpret_cast<double*>(w);
  return s;
}

inline void launch_rows(const Rows& a, const double* st, int src, int out, int n_f, const double* resp, const long long* lab,
                        const long long* cls, long long* lab_out, int force, const Ws& w, hipStream_t s) {
  hipLaunchKernelGGL(gmm_rows_kernel, dim3((unsigned)row_blocks(a.n, kRows, kMaxBlocks)), dim3(kRows), 0, s, a, st, src, out, n_f, resp, lab, cls, lab_out,
                     force, w.part, w.part_l);
}

inline void launch_final(double* st, const Rows& a, int C, int mode, int n_f, double reg, double tol, const Ws& w, double* map_out,
                         hipStream_t s) {
  hipLaunchKernelGGL(gmm_final_kernel, dim3(1), dim3(kFinThreads), 0, s, st, a.K, a.D, C, mode, n_f, row_blocks(a.n, kRows, kMaxBlocks), a.n, reg, tol,
                     w.part, w.part_l, w.tot, map_out);
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_gmm_state_bytes(int n_comp, int n_feat) {
  if (n_comp < 1 || n_comp > pinn::kMaxK || n_feat < 1 || n_feat > pinn::kMaxD) return 0;
  return pinn::st_words(n_comp, n_feat) * sizeof(double);
}

extern "C" size_t pinn_gmm_workspace_bytes(long long n_rows, int n_comp, int n_feat) {
  using namespace pinn;
  if (n_rows < 0 || n_comp < 1 || n_comp > kMaxK || n_feat < 1 || n_feat > kMaxD) return 0;
  const size_t KF = (size_t)n_comp * n_moments(n_feat) > (size_t)n_comp * kMaxC ? (size_t)n_comp * n_moments(n_feat) : (size_t)n_comp * kMaxC;
  return align256((KF + 1) * sizeof(double)) + align256((size_t)kMaxBlocks * KF * sizeof(double)) + align256(kMaxBlocks * sizeof(double));
}

#define GMM_COMMON_CHECKS()                                                                      \
  Rows a;                                                                                        \
  {                                                                                              \
    const int rc_ = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_comp, d_row_index, n, &a);  \
    if (rc_ != PINN_OK) return rc_;                                                              \
  }                                                                                              \
  if (!d_state || !d_ws || misaligned8(d_state) || misaligned8(d_ws)) return PINN_E_ARG;         \
  if (ws_bytes < pinn_gmm_workspace_bytes(n, n_comp, n_feat)) return PINN_E_WORKSPACE;           \
  const Ws w = carve(d_ws, n_comp, n_feat);                                                      \
  hipStream_t st = (hipStream_t)stream;                                                          \
  clear_error()

extern "C" int pinn_gmm_mstep_init(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                   const long long* d_row_index, long long n, int n_comp, const double* d_resp,
                                   const long long* d_labels, double reg_covar, double* d_state, void* d_ws, size_t ws_bytes,
                                   void* stream) {
  using namespace pinn;
  GMM_COMMON_CHECKS();
  if ((d_resp == nullptr) == (d_labels == nullptr) || n < 1 || !(reg_covar >= 0.0) || misaligned8(d_resp) || misaligned8(d_labels))
    return PINN_E_ARG;
  const int src = d_resp ? SRC_RESP : SRC_LABELS, F = n_moments(n_feat);
  hipError_t e = hipMemsetAsync(d_state, 0, pinn_gmm_state_bytes(n_comp, n_feat), st);      // shift 0 for the first pass
  if (e != hipSuccess) return (int)e;
  launch_rows(a, d_state, src, OUT_MOMENTS, 1 + n_feat, d_resp, d_labels, nullptr, nullptr, 1, w, st);
  launch_final(d_state, a, 0, FIN_MEANS, 1 + n_feat, reg_covar, 0.0, w, nullptr, st);
  launch_rows(a, d_state, src, OUT_MOMENTS, F, d_resp, d_labels, nullptr, nullptr, 1, w, st);    // second pass: about the means
  launch_final(d_state, a, 0, FIN_INIT, F, reg_covar, 0.0, w, nullptr, st);
  return launch_status();
}

extern "C" int pinn_gmm_em(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                           const long long* d_row_index, long long n, int n_comp, int n_iters, double tol, double reg_covar,
                           double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  GMM_COMMON_CHECKS();
  if (n < 1 || n_iters < 0 || n_iters > 100000 || !(tol >= 0.0) || !(reg_covar >= 0.0)) return PINN_E_ARG;
  const int F = n_moments(n_feat);
  for (int it = 0; it < n_iters; ++it) {
    launch_rows(a, d_state, SRC_ESTEP, OUT_MOMENTS, F, nullptr, nullptr, nullptr, nullptr, 0, w, st);
    launch_final(d_state, a, 0, FIN_EM, F, reg_covar, tol, w, nullptr, st);
  }
  return launch_status();
}

extern "C" int pinn_gmm_kmeans(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                               const long long* d_row_index, long long n, int n_comp, int n_iters, double* d_state,
                               long long* d_labels, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  GMM_COMMON_CHECKS();
  if (n < 1 || n_iters < 0 || n_iters > 100000 || misaligned8(d_labels)) return PINN_E_ARG;
  const int F = 1 + n_feat;
  for (int it = 0; it < n_iters; ++it) {
    launch_rows(a, d_state, SRC_NEAREST, OUT_MOMENTS, F, nullptr, nullptr, nullptr, nullptr, 0, w, st);
    launch_final(d_state, a, 0, FIN_KMEANS, F, 0.0, 0.0, w, nullptr, st);
  }
  if (d_labels)                                             // the assignment to the final centres
    launch_rows(a, d_state, SRC_NEAREST, OUT_MOMENTS, F, nullptr, nullptr, nullptr, d_labels, 1, w, st);
  return launch_status();
}

extern "C" int pinn_gmm_label_map(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                  const long long* d_row_index, long long n, int n_comp, const double* d_state,
                                  const long long* d_class, int n_classes, double* d_map, void* d_ws, size_t ws_bytes,
                                  void* stream) {
  using namespace pinn;
  GMM_COMMON_CHECKS();
  if (n_classes < 1 || n_classes > kMaxC || !d_map || (n > 0 && !d_class) || misaligned8(d_class) || misaligned8(d_map)) return PINN_E_ARG;
  launch_rows(a, d_state, SRC_ESTEP, OUT_CLASS, n_classes, nullptr, nullptr, d_class, nullptr, 1, w, st);
  launch_final(const_cast<double*>(d_state), a, n_classes, FIN_MAP, n_classes, 0.0, 0.0, w, d_map, st);
  return launch_status();
}

extern "C" int pinn_gmm_posterior(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                  const long long* d_row_index, long long n, int n_comp, const double* d_state,
                                  const double* d_map, int n_classes, double* d_log_prob_norm, double* d_resp, double* d_y_prob,
                                  long long* d_y_pred, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_comp, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_state || misaligned8(d_state) || misaligned8(d_map) || misaligned8(d_log_prob_norm) || misaligned8(d_resp) ||
      misaligned8(d_y_prob) || misaligned8(d_y_pred))
    return PINN_E_ARG;
  if (d_map ? (n_classes < 1 || n_classes > kMaxC) : (d_y_prob || d_y_pred)) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  const long long tiles = (n + kRows - 1) / kRows;
  if (tiles > 0x7fffffffLL) return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(gmm_posterior_kernel, dim3((unsigned)tiles), dim3(kRows), 0, (hipStream_t)stream, a, d_state, d_map, n_classes,
                     d_log_prob_norm, d_resp, d_y_prob, d_y_pred);
  return launch_status();
}

// ---- batches of candidates
extern "C" size_t pinn_gmm_batch_state_stride(int max_comp, int n_feat) { return pinn_gmm_state_bytes(max_comp, n_feat); }

extern "C" size_t pinn_gmm_batch_workspace_bytes(long long n_rows, int n_batch, int max_comp, int n_feat) {
  using namespace pinn;
  if (n_rows < 0 || n_batch < 1 || n_batch > kMaxB || max_comp < 1 || max_comp > kMaxK || n_feat < 1 || n_feat > kMaxD) return 0;
  const size_t KF = (size_t)max_comp * n_moments(n_feat), nb = (size_t)row_blocks(n_rows, kRows, kMaxBlocks);
  return (size_t)n_batch * (align256((KF + 1) * sizeof(double)) + align256(nb * KF * sizeof(double)) + align256(nb * sizeof(double)) +
                            align256((size_t)n_rows * sizeof(double)));
}

namespace pinn {
namespace {

// checks shared by the batch entry points; fills `a` and `b`
inline int make_batch(const double* d_arr, long long ld, long long n_arr, const int* cols, int n_feat, const long long* d_row_index,
                      long long n, int n_batch, const int* n_comp, int max_comp, const double* d_state, void* d_ws, size_t ws_bytes,
                      Rows* a, Batch* b) {
  const int rc = make_rows(d_arr, ld, n_arr, cols, n_feat, max_comp, d_row_index, n, a);
  if (rc != PINN_OK) return rc;
  if (n < 1 || n_batch < 1 || n_batch > kMaxB || !n_comp || !d_state || !d_ws || misaligned8(d_state) || misaligned8(d_ws)) return PINN_E_ARG;
  for (int c = 0; c < n_batch; ++c)
    if (n_comp[c] < 1 || n_comp[c] > max_comp) return PINN_E_ARG;
  if (ws_bytes < pinn_gmm_batch_workspace_bytes(n, n_batch, max_comp, n_feat)) return PINN_E_WORKSPACE;
  const size_t KF = (size_t)max_comp * n_moments(n_feat), nb = (size_t)row_blocks(n, kRows, kMaxBlocks);
  b->st = const_cast<double*>(d_state);
  b->ws = static_cast<char*>(d_ws);
  b->st_words = st_words(max_comp, n_feat);
  b->off_part = align256((KF + 1) * sizeof(double));
  b->off_l = b->off_part + align256(nb * KF * sizeof(double));
  b->off_d2 = b->off_l + align256(nb * sizeof(double));
  b->ws_block = b->off_d2 + align256((size_t)n * sizeof(double));
  b->n_batch = n_batch;
  b->n_part = (int)nb;
  for (int c = 0; c < kMaxB; ++c) b->k[c] = (unsigned char)(c < n_batch ? n_comp[c] : 0);
  return PINN_OK;
}

inline void launch_batch_rows(const Rows& a, const Batch& b, int src, int n_f, const long long* lab_in, long long* lab_out, int force,
                              hipStream_t s) {
  hipLaunchKernelGGL(gmm_batch_rows_kernel, dim3((unsigned)b.n_part, (unsigned)b.n_batch), dim3(kRows), 0, s, a, b, src, n_f, lab_in, lab_out, force);
}

inline void launch_batch_final(const Rows& a, const Batch& b, int mode, int n_f, double reg, double tol, hipStream_t s) {
  hipLaunchKernelGGL(gmm_batch_final_kernel, dim3((unsigned)b.n_batch), dim3(kFinThreads), 0, s, b, a.D, mode, n_f, a.n, reg, tol);
}

}  // namespace
}  // namespace pinn

#define GMM_BATCH_CHECKS()                                                                                                  \
  Rows a;                                                                                                                   \
  Batch b;                                                                                                                  \
  {                                                                                                                         \
    const int rc_ = make_batch(d_arr, ld, n_arr_rows, cols, n_feat, d_row_index, n, n_batch, n_comp, max_comp, d_state, d_ws, \
                               ws_bytes, &a, &b);                                                                           \
    if (rc_ != PINN_OK) return rc_;                                                                                         \
  }                                                                                                                         \
  hipStream_t st = (hipStream_t)stream

extern "C" int pinn_gmm_batch_seed(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                   const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp,
                                   const long long* d_first, const double* d_u, double* d_state, long long* d_picks, void* d_ws,
                                   size_t ws_bytes, void* stream) {
  using namespace pinn;
  GMM_BATCH_CHECKS();
  if (!d_first || (max_comp > 1 && !d_u) || misaligned8(d_first) || misaligned8(d_u) || misaligned8(d_picks)) return PINN_E_ARG;
  clear_error();
  hipError_t e = hipMemsetAsync(d_state, 0, (size_t)n_batch * pinn_gmm_batch_state_stride(max_comp, n_feat), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(gmm_batch_seed_kernel, dim3((unsigned)n_batch), dim3(kSeedThreads), 0, st, a, b, max_comp, d_first, d_u, d_picks);
  return launch_status();
}

extern "C" int pinn_gmm_batch_kmeans(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                     const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp,
                                     int n_iters, double* d_state, long long* d_labels, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  GMM_BATCH_CHECKS();
  if (n_iters < 0 || n_iters > 100000 || !d_labels || misaligned8(d_labels)) return PINN_E_ARG;
  clear_error();
  const int F = 1 + n_feat;
  for (int it = 0; it < n_iters; ++it) {
    launch_batch_rows(a, b, SRC_NEAREST, F, nullptr, nullptr, 0, st);
    launch_batch_final(a, b, FIN_KMEANS, F, 0.0, 0.0, st);
  }
  launch_batch_rows(a, b, SRC_NEAREST, F, nullptr, d_labels, 1, st);     // the assignment to the final centres
  return launch_status();
}

extern "C" int pinn_gmm_batch_mstep_init(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                         const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp,
                                         const long long* d_labels, double reg_covar, double* d_state, void* d_ws, size_t ws_bytes,
                                         void* stream) {
  using namespace pinn;
  GMM_BATCH_CHECKS();
  if (!d_labels || misaligned8(d_labels) || !(reg_covar >= 0.0)) return PINN_E_ARG;
  clear_error();
  const int F = n_moments(n_feat);
  hipError_t e = hipMemsetAsync(d_state, 0, (size_t)n_batch * pinn_gmm_batch_state_stride(max_comp, n_feat), st);   // shift 0 for the first pass
  if (e != hipSuccess) return (int)e;
  launch_batch_rows(a, b, SRC_LABELS, 1 + n_feat, d_labels, nullptr, 1, st);
  launch_batch_final(a, b, FIN_MEANS, 1 + n_feat, reg_covar, 0.0, st);
  launch_batch_rows(a, b, SRC_LABELS, F, d_labels, nullptr, 1, st);      // second pass: about the means
  launch_batch_final(a, b, FIN_INIT, F, reg_covar, 0.0, st);
  return launch_status();
}

extern "C" int pinn_gmm_batch_em(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                 const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp, int n_iters,
                                 double tol, double reg_covar, double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  GMM_BATCH_CHECKS();
  if (n_iters < 0 || n_iters > 100000 || !(tol >= 0.0) || !(reg_covar >= 0.0)) return PINN_E_ARG;
  clear_error();
  const int F = n_moments(n_feat);
  for (int it = 0; it < n_iters; ++it) {
    launch_batch_rows(a, b, SRC_ESTEP, F, nullptr, nullptr, 0, st);
    launch_batch_final(a, b, FIN_EM, F, reg_covar, tol, st);
  }
  return launch_status();
}

extern "C" int pinn_gmm_batch_score(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                    const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp,
                                    const double* d_state, double* d_sum, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  GMM_BATCH_CHECKS();
  if (!d_sum || misaligned8(d_sum)) return PINN_E_ARG;
  clear_error();
  launch_batch_rows(a, b, SRC_ESTEP, 1, nullptr, nullptr, 1, st);         // the sums of log_prob_norm ride with the weight sums
  hipLaunchKernelGGL(gmm_batch_sum_kernel, dim3((unsigned)((n_batch + kFinThreads - 1) / kFinThreads)), dim3(kFinThreads), 0, st, b, d_sum);
  return launch_status();
}
