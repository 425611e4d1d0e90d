// Exact t-SNE on the device: the two-dimensional embeddings of reference scripts 02 and 03.
//   pinn_tsne_affinities  joint probabilities P [n][n] of the rows (perplexity root per row, then symmetrised in place)
//   pinn_tsne_kl_grad     one pair pass and reduction at a given embedding: raw sums, KL and gradient (tests and timing)
//   pinn_tsne_descend     queued gradient-descent iterations with scikit-learn 1.7's update rule and schedule
// All arithmetic is float64, every operation rounded on its own (built with -ffp-contract=off): embedding.py's host
// backend states the same operations in the same order, so an iteration gives the same embedding bit for bit.  exp and log
// are the libraries' own: they enter P and the KL, and the KL enters the checks at every 50th iteration (best error, no
// progress), so the two backends stop at the same iteration unless two errors lie within rounding of each other.
//
// Affinities: one workgroup per row i.  The squared distances to all rows go into row i of the n x n workspace, the
// minimum is subtracted, and beta_i is the root of H_i(beta) = log(perplexity): Newton steps kept inside a bracket
// (bisection when a step leaves it), until |H - log perp| <= 1e-12 or 200 steps.  The row then holds p_{j|i}.  A row whose m
// nearest rows lie at exactly the same distance with log m >= log perp (duplicated rows) has no root: H falls to log m only;
// it gets the limit beta -> infinity, 1 / m on those rows, and the status PINN_TSNE_DUPLICATES.  A tiled
// launch symmetrises in place: the block of tile pair (a, b), a <= b, reads both tiles through LDS and writes both.
//
// Iteration: a pair pass and one one-workgroup launch.  Pair pass: a workgroup of 4 waves takes 16 rows, a wave 4 of them;
// tiles of 256 y_j are staged in LDS, lanes run along j (a wave reads 512 contiguous bytes of every P row per step), every
// lane keeps its sums over j = lane, lane + 64, ... in registers and a butterfly of wave shuffles adds the 64 lanes.  The
// one-workgroup launch adds the per-row sums (thread t takes rows t, t + 1024, ..., then a halving tree), forms KL and the
// gradient, applies the update and takes the stopping decision in the state's header.  The terms with log are summed
// only in the iterations whose error scikit-learn computes (every 50th and the last).
//
// No float atomics, no workgroup waits on another: stream order is the only dependency and every sum has a fixed order,
// so the same call gives the same bytes every time.  Once the header's done word is set every later launch returns at once.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kMaxD = PINN_TSNE_MAX_FEAT;
constexpr long long kMaxN = PINN_TSNE_MAX_ROWS;
constexpr int kHdr = PINN_TSNE_ST_HEADER;
constexpr int kAffThreads = 256;
constexpr int kSymTile = 32, kSymThreads = 256;
constexpr int kPairThreads = 256, kPairWaves = kPairThreads / 64, kRowsPerWave = 4, kPairRows = kPairWaves * kRowsPerWave, kPairTile = 256;
constexpr int kFinThreads = 1024;
constexpr int kSums = PINN_TSNE_ROW_SUMS;      // Z, Ax, Ay, Rx, Ry, sum P log P, sum P log(1 + d^2), sum P
constexpr int kExplore = 250, kCheck = 50;     // scikit-learn's _EXPLORATION_MAX_ITER and _N_ITER_CHECK
constexpr double kEps = 2.220446049250313e-16;
constexpr int kBetaSteps = 200;
constexpr double kBetaTol = 1e-12;

static_assert(kMaxD <= kRowsMaxD, "pinn_rows.h carries the feature limit");
static_assert(kPairTile % 64 == 0, "a lane keeps the same residue of j in every tile");

enum { FIN_EVAL = 0, FIN_STEP = 1 };

// workspace: P [n][n], per-row sums [n][kSums], gradient [n][2], scalars [PINN_TSNE_SCALARS]
__host__ __device__ inline size_t ws_rows_off(long long n) { return ((size_t)n * n * 8 + 255) & ~(size_t)255; }
__host__ __device__ inline size_t ws_grad_off(long long n) { return ws_rows_off(n) + (((size_t)n * kSums * 8 + 255) & ~(size_t)255); }
__host__ __device__ inline size_t ws_scal_off(long long n) { return ws_grad_off(n) + (((size_t)n * 2 * 8 + 255) & ~(size_t)255); }
__host__ __device__ inline size_t ws_total(long long n) { return ws_scal_off(n) + 256; }

// sum of v over the workgroup, the same value in every thread: thread t's value enters at leaf t of a halving tree
template <int T>
__device__ __forceinline__ double block_sum(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int w = T / 2; w > 0; w >>= 1) {
    if (t < w) s[t] += s[t + w];
    __syncthreads();
  }
  return s[0];
}

template <int T>
__device__ __forceinline__ double block_min(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int w = T / 2; w > 0; w >>= 1) {
    if (t < w) s[t] = fmin(s[t], s[t + w]);
    __syncthreads();
  }
  return s[0];
}

// ---- conditional probabilities of row i.  P: the n x n workspace; psum[i * kSums] gets sum_j p_{j|i}.
__global__ __launch_bounds__(kAffThreads) void tsne_cond_kernel(Rows a, double log_perp, double* __restrict__ P, double* __restrict__ rows_out,
                                                                double* __restrict__ beta_out, double* __restrict__ h_out,
                                                                long long* __restrict__ status) {
  __shared__ double s_red[kAffThreads];
  const long long n = a.n, i = blockIdx.x;
  const int t = threadIdx.x;
  double* row = P + (size_t)i * n;
  double xi[kRowsMaxD], xj[kRowsMaxD];
  const bool ok_i = load_row(a, i, xi);
  double dmin = INFINITY, bad = ok_i ? 0.0 : 1.0;
  for (long long j = t; j < n; j += kAffThreads) {
    const bool ok = load_row(a, j, xj);
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < kRowsMaxD; ++k)
      if (k < a.D) { const double e = xi[k] - xj[k]; d += e * e; }
    if (!ok || !(d - d == 0.0)) bad = 1.0;
    row[j] = d;
    if (j != i) dmin = fmin(dmin, d);
  }
  bad = block_sum<kAffThreads>(bad, s_red);
  if (bad != 0.0) {                                              // a row that is not finite: its distances spoil every row
    for (long long j = t; j < n; j += kAffThreads) row[j] = 0.0;
    if (t == 0) { status[i] = PINN_TSNE_NAN; beta_out[i] = quiet_nan(); h_out[i] = quiet_nan(); rows_out[i * kSums] = 0.0; }
    return;
  }
  dmin = block_min<kAffThreads>(dmin, s_red);
  double cnt = 0.0;
  for (long long j = t; j < n; j += kAffThreads) cnt += (j != i && row[j] == dmin) ? 1.0 : 0.0;
  const double m = block_sum<kAffThreads>(cnt, s_red);          // an integer below 2^53: exact in any order
  if (log(m) >= log_perp) {                                      // H(beta) > log m >= log perp for every beta: the limit
    double ps = 0.0;
    for (long long j = t; j < n; j += kAffThreads) {
      const double p = (j != i && row[j] == dmin) ? 1.0 / m : 0.0;
      row[j] = p;
      ps += p;
    }
    ps = block_sum<kAffThreads>(ps, s_red);
    if (t == 0) { status[i] = PINN_TSNE_DUPLICATES; beta_out[i] = INFINITY; h_out[i] = log(m); rows_out[i * kSums] = ps; }
    return;
  }

  double beta = 1.0, lo = 0.0, hi = INFINITY, H = 0.0, S = 1.0;
  bool conv = false;
  for (int step = 0; step < kBetaSteps; ++step) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long j = t; j < n; j += kAffThreads) {
      if (j == i) continue;
      const double d = row[j] - dmin, e = exp(-beta * d);
      s0 += e; s1 += d * e; s2 += d * d * e;
    }
    S = block_sum<kAffThreads>(s0, s_red);
    const double E = block_sum<kAffThreads>(s1, s_red) / S, V = block_sum<kAffThreads>(s2, s_red) / S - E * E;
    H = log(S) + beta * E;                                       // entropy in nats; dH/dbeta = -beta V
    const double diff = H - log_perp;
    if (fabs(diff) <= kBetaTol) { conv = true; break; }
    if (diff > 0.0) lo = beta; else hi = beta;                   // H falls with beta
    double nb = beta + diff / (beta * V);
    if (!(nb > lo && nb < hi)) nb = hi == INFINITY ? 2.0 * beta : 0.5 * (lo + hi);
    if (nb == beta) break;                                       // the bracket has closed
    beta = nb;
  }
  double ps = 0.0;
  for (long long j = t; j < n; j += kAffThreads) {
    const double p = j == i ? 0.0 : exp(-beta * (row[j] - dmin)) / S;
    row[j] = p;
    ps += p;
  }
  ps = block_sum<kAffThreads>(ps, s_red);
  if (t == 0) {
    status[i] = conv ? 0 : PINN_TSNE_NOT_CONVERGED;
    beta_out[i] = beta; h_out[i] = H; rows_out[i * kSums] = ps;
  }
}

// S = max(sum of all entries of p + p^T, eps) = twice the sum of the row sums.  One workgroup.
__global__ __launch_bounds__(kFinThreads) void tsne_psum_kernel(const double* __restrict__ rows_in, long long n, double* __restrict__ scal) {
  __shared__ double s_red[kFinThreads];
  double s = 0.0;
  for (long long i = threadIdx.x; i < n; i += kFinThreads) s += rows_in[i * kSums];
  s = block_sum<kFinThreads>(s, s_red);
  if (threadIdx.x == 0) scal[PINN_TSNE_SC_PSUM] = fmax(2.0 * s, kEps);
}

// P_ij = max((p_{j|i} + p_{i|j}) / S, eps) in place, diagonal 0.  Block (a, b) with a <= b owns tiles (a, b) and (b, a).
__global__ __launch_bounds__(kSymThreads) void tsne_sym_kernel(double* __restrict__ P, long long n, const double* __restrict__ scal) {
  __shared__ double s_a[kSymTile][kSymTile + 1], s_b[kSymTile][kSymTile + 1];
  const int ta = blockIdx.y, tb = blockIdx.x;
  if (ta > tb) return;
  const double S = scal[PINN_TSNE_SC_PSUM];
  const long long r0 = (long long)ta * kSymTile, c0 = (long long)tb * kSymTile;
  const int tx = threadIdx.x % kSymTile, ty = threadIdx.x / kSymTile;
  for (int r = ty; r < kSymTile; r += kSymThreads / kSymTile) {
    const bool in_a = r0 + r < n && c0 + tx < n, in_b = c0 + r < n && r0 + tx < n;
    s_a[r][tx] = in_a ? P[(size_t)(r0 + r) * n + c0 + tx] : 0.0;   // tile (a, b): rows r0.., columns c0..
    s_b[r][tx] = in_b ? P[(size_t)(c0 + r) * n + r0 + tx] : 0.0;   // tile (b, a): rows c0.., columns r0..
  }
  __syncthreads();
  for (int r = ty; r < kSymTile; r += kSymThreads / kSymTile) {
    if (r0 + r < n && c0 + tx < n) {
      const double v = fmax((s_a[r][tx] + s_b[tx][r]) / S, kEps);
      P[(size_t)(r0 + r) * n + c0 + tx] = (r0 + r == c0 + tx) ? 0.0 : v;
    }
    if (ta != tb && c0 + r < n && r0 + tx < n) P[(size_t)(c0 + r) * n + r0 + tx] = fmax((s_a[tx][r] + s_b[r][tx]) / S, kEps);
  }
}

// ---- the pair pass
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

template <bool kErr>
__device__ __forceinline__ void pair_body(const double* __restrict__ P, const double* __restrict__ Y, long long n, double* __restrict__ rows_out,
                                          double2* s_y) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long base = (long long)blockIdx.x * kPairRows + wave * kRowsPerWave;
  long long ri[kRowsPerWave];
  double yx[kRowsPerWave], yy[kRowsPerWave], acc[kRowsPerWave][kSums];
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
    ri[r] = base + r < n ? base + r : n - 1;                    // a row past the end reads the last row and is not written
    yx[r] = Y[2 * ri[r]]; yy[r] = Y[2 * ri[r] + 1];
#pragma unroll
    for (int f = 0; f < kSums; ++f) acc[r][f] = 0.0;
  }
  for (long long j0 = 0; j0 < n; j0 += kPairTile) {
    __syncthreads();
    if (j0 + t < n) s_y[t] = make_double2(Y[2 * (j0 + t)], Y[2 * (j0 + t) + 1]);
    __syncthreads();
    const int len = n - j0 < kPairTile ? (int)(n - j0) : kPairTile;
    for (int jj = lane; jj < len; jj += 64) {
      const double2 yj = s_y[jj];
      const long long j = j0 + jj;
#pragma unroll
      for (int r = 0; r < kRowsPerWave; ++r) {
        const double p = P[(size_t)ri[r] * n + j];
        const double dx = yx[r] - yj.x, dy = yy[r] - yj.y, q = 1.0 + (dx * dx + dy * dy);
        const double w = j == ri[r] ? 0.0 : 1.0 / q, pw = p * w, w2 = w * w;
        acc[r][0] += w;
        acc[r][1] += pw * dx; acc[r][2] += pw * dy;
        acc[r][3] += w2 * dx; acc[r][4] += w2 * dy;
        if (kErr && p > 0.0) {
          acc[r][5] += p * log(p); acc[r][6] += p * log(q); acc[r][7] += p;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kRowsPerWave; ++r) {
#pragma unroll
    for (int f = 0; f < kSums; ++f) {
      const double s = wave_sum(acc[r][f]);
      if (lane == 0 && base + r < n) rows_out[(base + r) * kSums + f] = s;
    }
  }
}

// does iteration `it` of a phase that ends before `max_it` compute the error?  (scikit-learn's compute_error)
__device__ __forceinline__ bool wants_error(long long it, long long max_it) { return (it + 1) % kCheck == 0 || it == max_it - 1; }

__global__ __launch_bounds__(kPairThreads) void tsne_pair_kernel(const double* __restrict__ P, const double* __restrict__ Y, long long n,
                                                                  const double* __restrict__ st, int max_iter, double* __restrict__ rows_out) {
  __shared__ double2 s_y[kPairTile];
  bool err = true;
  if (st) {                                                      // a descent iteration: the header says whether and what
    const long long* h = reinterpret_cast<const long long*>(st);
    if (h[PINN_TSNE_ST_DONE] != 0 || h[PINN_TSNE_ST_STATUS] != 0) return;
    err = wants_error(h[PINN_TSNE_ST_ITER], h[PINN_TSNE_ST_PHASE] == 0 ? kExplore : max_iter);
  }
  if (err) pair_body<true>(P, Y, n, rows_out, s_y);
  else pair_body<false>(P, Y, n, rows_out, s_y);
}

// ---- sums over rows, KL, gradient; FIN_STEP: the update of scikit-learn's _gradient_descent and the schedule of _tsne
__global__ __launch_bounds__(kFinThreads) void tsne_finish_kernel(int mode, long long n, double* __restrict__ st, double* __restrict__ Y, const double* __restrict__ rows_in,
                                                                   double* __restrict__ grad, double* __restrict__ scal, double alpha_eval,
                                                                   int max_iter, double exaggeration, double lr, int no_progress, double min_grad) {
  __shared__ double s_red[kFinThreads];
  __shared__ int s_reset;
  long long* h = reinterpret_cast<long long*>(st);
  const int t = threadIdx.x;
  bool err = true;
  double alpha = alpha_eval, mom = 0.0;
  long long it = 0, max_it = 0;
  int phase = 0;
  if (mode == FIN_STEP) {
    if (h[PINN_TSNE_ST_DONE] != 0 || h[PINN_TSNE_ST_STATUS] != 0) return;
    it = h[PINN_TSNE_ST_ITER];
    phase = (int)h[PINN_TSNE_ST_PHASE];
    max_it = phase == 0 ? kExplore : max_iter;
    err = wants_error(it, max_it);
    alpha = phase == 0 ? exaggeration : 1.0;
    mom = phase == 0 ? 0.5 : 0.8;
  }
  double z = 0.0, a5 = 0.0, a6 = 0.0, a7 = 0.0;
  for (long long i = t; i < n; i += kFinThreads) {
    z += rows_in[i * kSums];
    if (err) { a5 += rows_in[i * kSums + 5]; a6 += rows_in[i * kSums + 6]; a7 += rows_in[i * kSums + 7]; }
  }
  const double Z = block_sum<kFinThreads>(z, s_red);
  double kl = quiet_nan(), plogp = 0.0, plogq = 0.0, sp = 0.0;
  if (err) {
    plogp = block_sum<kFinThreads>(a5, s_red);
    plogq = block_sum<kFinThreads>(a6, s_red);
    sp = block_sum<kFinThreads>(a7, s_red);
    kl = alpha * (((plogp + log(alpha) * sp) + plogq) + sp * log(Z));      // sum (alpha P) log(alpha P / (w / Z))
  }
  double* upd = nullptr;
  double* gain = nullptr;
  if (mode == FIN_STEP) { upd = st + kHdr + 2 * n; gain = upd + 2 * n; }
  double g2 = 0.0;
  for (long long e = t; e < 2 * n; e += kFinThreads) {
    const long long i = e >> 1;
    const int c = (int)(e & 1);
    double g = 4.0 * (alpha * rows_in[i * kSums + 1 + c] - rows_in[i * kSums + 3 + c] / Z);
    grad[e] = g;
    if (mode == FIN_STEP) {
      const double u = upd[e];
      double gn = gain[e];
      gn = u * g < 0.0 ? gn + 0.2 : gn * 0.8;
      gn = gn < 0.01 ? 0.01 : gn;
      g *= gn;
      const double un = mom * u - lr * g;
      gain[e] = gn; upd[e] = un; Y[e] += un;
    }
    g2 += g * g;
  }
  const double gnorm = sqrt(block_sum<kFinThreads>(g2, s_red));
  if (t == 0) {
    scal[PINN_TSNE_SC_Z] = Z; scal[PINN_TSNE_SC_KL] = kl; scal[PINN_TSNE_SC_SUMP] = sp; scal[PINN_TSNE_SC_PLOGP] = plogp;
    scal[PINN_TSNE_SC_PLOGQ] = plogq; scal[PINN_TSNE_SC_GNORM] = gnorm;
    s_reset = 0;
  }
  if (mode != FIN_STEP) return;
  if (t == 0) {
    h[PINN_TSNE_ST_LAST] = it;
    st[PINN_TSNE_ST_GNORM] = gnorm;
    st[PINN_TSNE_ST_Z] = Z;
    if (err) st[PINN_TSNE_ST_ERROR] = kl;
    int stop = 0;
    if (!(gnorm - gnorm == 0.0) || (err && !(kl - kl == 0.0))) {
      h[PINN_TSNE_ST_STATUS] = PINN_TSNE_NAN;
      stop = -1;
    } else {
      if ((it + 1) % kCheck == 0) {
        const long long np = phase == 0 ? kExplore : no_progress;
        if (kl < st[PINN_TSNE_ST_BEST_ERROR]) { st[PINN_TSNE_ST_BEST_ERROR] = kl; h[PINN_TSNE_ST_BEST_ITER] = it; }
        else if (it - h[PINN_TSNE_ST_BEST_ITER] > np) stop = PINN_TSNE_STOP_NO_PROGRESS;
        if (!stop && gnorm <= min_grad) stop = PINN_TSNE_STOP_GRAD_NORM;
      }
      if (!stop && it + 1 >= max_it) stop = PINN_TSNE_STOP_MAX_ITER;
    }
    if (stop > 0 && phase == 0 && !(stop == PINN_TSNE_STOP_MAX_ITER && max_iter <= kExplore)) {
      h[PINN_TSNE_ST_PHASE] = 1;                                 // the second phase starts from update 0, gains 1, no best error
      h[PINN_TSNE_ST_ITER] = it + 1;
      h[PINN_TSNE_ST_BEST_ITER] = it + 1;
      st[PINN_TSNE_ST_BEST_ERROR] = DBL_MAX;
      h[PINN_TSNE_ST_STOP1] = stop;
      s_reset = 1;
    } else if (stop != 0) {
      h[PINN_TSNE_ST_DONE] = 1;
      h[PINN_TSNE_ST_STOP] = stop > 0 ? stop : 0;
    } else {
      h[PINN_TSNE_ST_ITER] = it + 1;
    }
  }
  __syncthreads();
  if (s_reset)
    for (long long e = t; e < 2 * n; e += kFinThreads) { upd[e] = 0.0; gain[e] = 1.0; }
}

// header of a fresh run; update 0, gains 1.  The embedding is the caller's.
__global__ __launch_bounds__(kFinThreads) void tsne_init_kernel(double* __restrict__ st, long long n) {
  long long* h = reinterpret_cast<long long*>(st);
  const int t = threadIdx.x;
  if (t < kHdr) h[t] = 0;
  __syncthreads();
  if (t == 0) {
    h[PINN_TSNE_ST_N] = n;
    st[PINN_TSNE_ST_BEST_ERROR] = DBL_MAX;
    st[PINN_TSNE_ST_ERROR] = DBL_MAX;
  }
  double* upd = st + kHdr + 2 * n;
  for (long long e = t; e < 2 * n; e += kFinThreads) { upd[e] = 0.0; upd[2 * n + e] = 1.0; }
}

inline bool rows_ok(long long n) { return n >= 2 && n <= kMaxN; }

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_tsne_state_bytes(long long n_rows) {
  if (!pinn::rows_ok(n_rows)) return 0;
  return ((size_t)pinn::kHdr + 6 * (size_t)n_rows) * sizeof(double);
}

extern "C" size_t pinn_tsne_workspace_bytes(long long n_rows) {
  if (!pinn::rows_ok(n_rows)) return 0;
  return pinn::ws_total(n_rows);
}

extern "C" int pinn_tsne_affinities(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                    const long long* d_row_index, long long n, double perplexity, double* d_beta, double* d_entropy,
                                    long long* d_status, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, 1, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (n_feat > kMaxD || !rows_ok(n) || !(perplexity > 0.0) || !(perplexity < (double)n)) return PINN_E_ARG;
  if (!d_beta || !d_entropy || !d_status || !d_ws || misaligned8(d_beta) || misaligned8(d_entropy) || misaligned8(d_status) || misaligned8(d_ws))
    return PINN_E_ARG;
  if (ws_bytes < ws_total(n)) return PINN_E_WORKSPACE;
  char* w = static_cast<char*>(d_ws);
  double* P = reinterpret_cast<double*>(w);
  double* rows_out = reinterpret_cast<double*>(w + ws_rows_off(n));
  double* scal = reinterpret_cast<double*>(w + ws_scal_off(n));
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const unsigned tiles = (unsigned)((n + kSymTile - 1) / kSymTile);
  hipLaunchKernelGGL(tsne_cond_kernel, dim3((unsigned)n), dim3(kAffThreads), 0, st, a, log(perplexity), P, rows_out, d_beta, d_entropy, d_status);
  hipLaunchKernelGGL(tsne_psum_kernel, dim3(1), dim3(kFinThreads), 0, st, rows_out, n, scal);
  hipLaunchKernelGGL(tsne_sym_kernel, dim3(tiles, tiles), dim3(kSymThreads), 0, st, P, n, scal);
  return launch_status();
}

extern "C" int pinn_tsne_kl_grad(long long n, const double* d_Y, double exaggeration, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (!rows_ok(n) || !d_Y || !d_ws || misaligned8(d_Y) || misaligned8(d_ws) || !(exaggeration > 0.0)) return PINN_E_ARG;
  if (ws_bytes < ws_total(n)) return PINN_E_WORKSPACE;
  char* w = static_cast<char*>(d_ws);
  const double* P = reinterpret_cast<const double*>(w);
  double* rows_out = reinterpret_cast<double*>(w + ws_rows_off(n));
  double* grad = reinterpret_cast<double*>(w + ws_grad_off(n));
  double* scal = reinterpret_cast<double*>(w + ws_scal_off(n));
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const unsigned G = (unsigned)((n + kPairRows - 1) / kPairRows);
  hipLaunchKernelGGL(tsne_pair_kernel, dim3(G), dim3(kPairThreads), 0, st, P, d_Y, n, (const double*)nullptr, 0, rows_out);
  hipLaunchKernelGGL(tsne_finish_kernel, dim3(1), dim3(kFinThreads), 0, st, (int)FIN_EVAL, n, (double*)nullptr, const_cast<double*>(d_Y), rows_out, grad, scal,
                     exaggeration, 0, 1.0, 0.0, 0, 0.0);
  return launch_status();
}

extern "C" int pinn_tsne_descend(long long n, int init, int n_iter, int max_iter, double early_exaggeration, double learning_rate,
                                 int n_iter_without_progress, double min_grad_norm, double* d_state, void* d_ws, size_t ws_bytes,
                                 void* stream) {
  using namespace pinn;
  if (!rows_ok(n) || !d_state || !d_ws || misaligned8(d_state) || misaligned8(d_ws)) return PINN_E_ARG;
  if (n_iter < 0 || n_iter > 100000 || max_iter < kExplore || n_iter_without_progress < 0 || !(early_exaggeration > 0.0) ||
      !(learning_rate > 0.0) || !(min_grad_norm >= 0.0))
    return PINN_E_ARG;
  if (ws_bytes < ws_total(n)) return PINN_E_WORKSPACE;
  char* w = static_cast<char*>(d_ws);
  const double* P = reinterpret_cast<const double*>(w);
  double* rows_out = reinterpret_cast<double*>(w + ws_rows_off(n));
  double* grad = reinterpret_cast<double*>(w + ws_grad_off(n));
  double* scal = reinterpret_cast<double*>(w + ws_scal_off(n));
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const unsigned G = (unsigned)((n + kPairRows - 1) / kPairRows);
  if (init) hipLaunchKernelGGL(tsne_init_kernel, dim3(1), dim3(kFinThreads), 0, st, d_state, n);
  for (int it = 0; it < n_iter; ++it) {
    hipLaunchKernelGGL(tsne_pair_kernel, dim3(G), dim3(kPairThreads), 0, st, P, d_state + kHdr, n, (const double*)d_state, max_iter, rows_out);
    hipLaunchKernelGGL(tsne_finish_kernel, dim3(1), dim3(kFinThreads), 0, st, (int)FIN_STEP, n, d_state, d_state + kHdr, rows_out, grad, scal, 1.0, max_iter,
                       early_exaggeration, learning_rate, n_iter_without_progress, min_grad_norm);
  }
  return launch_status();
}
