// Script 05's Sup_SVM on the device (reference script 05, cited as 05:<line>): StandardScaler, then a one-vs-one linear SVC
// (05:323-341), every pair solved to the optimum by a primal-dual interior-point method on the dual.  All arithmetic is
// float64, every operation rounded on its own (-ffp-contract=off): the host backend states the same arithmetic.
//   pinn_svm_pass      the sums of one row pass at the state's point (for tests and tools)
//   pinn_svm_ipm       interior-point iterations, six launches each, no host synchronisation between them
//   pinn_svm_decision  pairwise decision values, votes and the prediction per row, one launch
//
// A pair (a, b), a < b, solves min 1/2 al'Q al - e'al, t'al = 0, 0 <= al <= c over the rows of its two classes, Q = V V',
// V = diag(t) Z.  With multipliers s (al >= 0), z (al <= c) and beta (the equality; it is the intercept), w = V'al,
// d = s / al + z / (c - al) and u = (z-scores, 1), eliminating the row unknowns leaves per pair
//     (diag(I, 0) + sum u u' / d) (dw, dbeta) = sum g t u / d - (w - V'al, 0) + (0, t'al),   dal = (g - t u.(dw, dbeta)) / d.
// Mehrotra's predictor has g = 1 - t f (f = w.z + beta); the corrector adds sigma mu (1 / al - 1 / (c - al)) and the
// second-order terms, which reach the right-hand side through two vector sums of the predictor's pass.  An iteration:
//   pass B  predictor directions per row; step to the boundary (min), mu_aff's coefficients and the two vectors (sums)
//   pass C  final directions per row, written to the workspace; step to the boundary (min); V'dal and t'dal (sums), from
//           which the one-workgroup launch takes one step of refinement of (dw, dbeta)
//   pass A  applies the step and the refinement to (al, s, z) and sums the matrix, the right-hand side, V'al, the complementarity and the gap
// each followed by a one-workgroup launch that adds the workgroups' partials in index order and does the pair's small
// solve.  A thread owns a row; a row of class k has C - 1 slots, slot j its j-th other class in increasing order, and
// contributes to those C - 1 pairs.  Tiles of 128 rows put their terms into LDS, then every thread owns output sums and adds
// the tile's terms to them in row order, in registers.  No float atomics, no workgroup waits on another: stream order is
// the only dependency and the same call gives the same bytes every time.  A pair that has converged or failed is skipped by
// every later launch.  A row that cannot be placed (a gather index outside the array, a class outside [0, C)) adds to no sum,
// but its workgroup flags it and the one-workgroup launch fails every pair of that launch with PINN_SVM_RANGE.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_ovo.h"

namespace pinn {
namespace {

constexpr int kRows = 128;                  // rows per tile = threads per workgroup of a row pass
constexpr int kMaxC = kOvoMaxC, kMaxD = kOvoMaxD, kMaxP = kOvoMaxP, kMaxSlots = kMaxC - 1;
constexpr int kD1 = kMaxD + 1;              // (z, 1)
constexpr int kTerms = 6;                   // per row and slot in LDS
constexpr int kMaxSums = kD1 * (kD1 + 1) / 2 + 2 * kD1 + 3;
constexpr int kMaxOut = (kMaxP * kMaxSums + kRows - 1) / kRows;
constexpr int kMaxBlocks = 1024;            // workgroups of a row pass = partial sums per output
constexpr int kFinThreads = 256;
constexpr int kHdr = PINN_SVM_ST_HEADER, kPW = PINN_SVM_PAIR_WORDS, kScratch = 128;
constexpr double kStartSlack = 1.0, kStepToBoundary = 0.995, kMuFloor = 0.1;

enum { PASS_A = 0, PASS_B = 1, PASS_C = 2 };
enum { MODE_RUN = 0, MODE_SUMS = 1 };

__host__ __device__ inline int n_tri(int D) { return (D + 1) * (D + 2) / 2; }
__host__ __device__ inline int n_sums_a(int D) { return n_tri(D) + 2 * (D + 1) + 3; }
__host__ __device__ inline int n_sums_b(int D) { return 2 + 2 * (D + 1); }
// state block: the prefix of pinn_ovo.h, then alpha, s, z [n][C - 1]
__host__ __device__ inline size_t st_words(long long n, int C, int D) { return st_alpha(C, D, kHdr, kPW) + 3 * (size_t)n * (C - 1); }

__device__ __forceinline__ bool pair_stopped(const double* pb) {
  const long long* h = reinterpret_cast<const long long*>(pb);
  return h[PINN_SVM_P_CONVERGED] != 0 || h[PINN_SVM_P_STATUS] != 0;
}

// the largest step that keeps v + step dv >= 0
__device__ __forceinline__ double boundary(double v, double dv) { return dv < 0.0 ? -v / dv : INFINITY; }

struct Pass {
  double* st;               // state block
  const long long* y;       // class index per row position
  double *dal, *ds, *dz;    // final directions [n][C - 1] (workspace)
  double* part;             // [grid][P n_sums]
  double* pmin;             // [grid][P]
  double* pbad;             // [grid]: 1 where the workgroup met a row that cannot be placed
  int mode;
};

// ---- a row pass.  PASS_A: part = the sums of n_sums_a per pair; PASS_B: n_sums_b and pmin; PASS_C: D + 1 sums and pmin.
template <int PASS>
__global__ __launch_bounds__(kRows) void svm_rows_kernel(Rows a, Pass k) {
  __shared__ double s_term[kRows * kMaxSlots * kTerms];
  __shared__ double s_u[kRows * kD1];
  __shared__ int s_cls[kRows];
  __shared__ double s_w[kMaxP * kD1], s_daff[kMaxP * kD1], s_dir[kMaxP * kD1];
  __shared__ double s_theta[kMaxP], s_sigmu[kMaxP], s_ka[kMaxP], s_kb[kMaxP];
  __shared__ int s_phase[kMaxP];            // -1: the pair takes no part in this launch
  __shared__ double s_mean[kMaxD], s_scale[kMaxD], s_bound[kMaxC];
  __shared__ int s_any, s_bad;
  const int C = a.K, D = a.D, D1 = D + 1, P = n_pairs(C), S1 = C - 1, t = threadIdx.x;
  const int nS = PASS == PASS_A ? n_sums_a(D) : (PASS == PASS_B ? n_sums_b(D) : D1), nT = n_tri(D);
  if (t == 0) { s_any = 0; s_bad = 0; }
  __syncthreads();
  if (t < P) {
    const double* pb = k.st + kHdr + (size_t)t * kPW;
    const long long* pi = reinterpret_cast<const long long*>(pb);
    int phase = (int)pi[PINN_SVM_P_PHASE];
    if (k.mode == MODE_SUMS) phase = 2;
    else if (pair_stopped(pb) || (PASS != PASS_A && phase != 2)) phase = -1;
    s_phase[t] = phase;
    if (phase >= 0) s_any = 1;
    for (int i = 0; i < D1; ++i) {
      s_w[t * kD1 + i] = i < D ? pb[PINN_SVM_P_W + i] : pb[PINN_SVM_P_BETA];
      s_daff[t * kD1 + i] = pb[PINN_SVM_P_DAFF + i];
      s_dir[t * kD1 + i] = pb[(PASS == PASS_A ? PINN_SVM_P_FIX : PINN_SVM_P_DIR) + i];      // pass A applies the refinement
    }
    s_theta[t] = pb[PINN_SVM_P_THETA];
    s_sigmu[t] = pb[PINN_SVM_P_SIGMU];
    s_ka[t] = pb[PINN_SVM_P_KA];
    s_kb[t] = pb[PINN_SVM_P_KB];
  }
  if (t < D) { s_mean[t] = k.st[st_mean(C, kHdr, kPW) + t]; s_scale[t] = k.st[st_mean(C, kHdr, kPW) + D + t]; }
  if (t < C) s_bound[t] = k.st[st_bound(C, D, kHdr, kPW) + t];
  __syncthreads();
  if (!s_any) {                              // every pair has stopped
    if (t == 0) k.pbad[blockIdx.x] = 0.0;
    return;
  }

  double* g_al = k.st + st_alpha(C, D, kHdr, kPW);
  double* g_s = g_al + (size_t)a.n * S1;
  double* g_z = g_s + (size_t)a.n * S1;
  double acc[kMaxOut];
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q) acc[q] = 0.0;
  double tmin = INFINITY;

  const long long tiles = (a.n + kRows - 1) / kRows;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long j = tile * kRows + t;
    double x[kRowsMaxD];
    bool ok = false;
    long long cls = -1;
    if (j < a.n) {
      ok = load_row(a, j, x);
      cls = k.y[j];
    }
    ok = ok && cls >= 0 && cls < C;                           // a class outside [0, C) adds nothing
    if (j < a.n && !ok) s_bad = 1;                            // every writer stores the same value
    s_cls[t] = ok ? (int)cls : -1;
    double* u = s_u + t * kD1;
    bool fin = true;
    for (int i = 0; i < D; ++i) {
      u[i] = ok ? (x[i] - s_mean[i]) / s_scale[i] : 0.0;
      fin = fin && finite(u[i]);
    }
    u[D] = 1.0;
    if (ok) {
      const int kc = (int)cls;
      const double c = s_bound[kc];
      for (int slot = 0; slot < S1; ++slot) {
        const int other = slot < kc ? slot : slot + 1;
        const bool first = kc < other;
        const int p = first ? pair_index(kc, other, C) : pair_index(other, kc, C);
        const double tt = first ? 1.0 : -1.0;
        double* T = s_term + (t * kMaxSlots + slot) * kTerms;
        const int phase = s_phase[p];
        T[5] = INFINITY;
        if (phase < 0) {
          for (int e = 0; e < 5; ++e) T[e] = 0.0;
          continue;
        }
        if (!fin) {                                           // a row that is not finite spoils every sum of its pairs
          for (int e = 0; e < kTerms; ++e) T[e] = quiet_nan();
          continue;
        }
        const size_t idx = (size_t)j * S1 + slot;
        const double* w = s_w + p * kD1;
        double f = 0.0;
        for (int i = 0; i < D; ++i) f += w[i] * u[i];
        f += w[D];
        const double tf = tt * f;
        double al, s, z;
        if (PASS == PASS_A && phase == 0) {                   // the starting alpha: a fixed fraction of the bound per side
          al = c * (first ? s_ka[p] : s_kb[p]);
          g_al[idx] = al;
          T[0] = 0.0; T[1] = 0.0; T[2] = al * tt; T[3] = 0.0; T[4] = 0.0; T[5] = 0.0;
          continue;
        }
        al = g_al[idx];
        if (PASS == PASS_A && phase == 1) {                   // the starting multipliers: no dual residual
          const double rho = tf - 1.0;
          s = (rho > 0.0 ? rho : 0.0) + kStartSlack;
          z = (rho < 0.0 ? -rho : 0.0) + kStartSlack;
          g_s[idx] = s; g_z[idx] = z;
        } else {
          s = g_s[idx]; z = g_z[idx];
          if (PASS == PASS_A && phase == 3) {                 // the step the last iteration decided, with its refinement
            const double th = s_theta[p];
            const double* fx = s_dir + p * kD1;
            double ux = 0.0;
            for (int i = 0; i < D1; ++i) ux += u[i] * fx[i];
            const double dfix = -(1.0 / (s / al + z / (c - al))) * tt * ux;
            const double al_n = al + th * (k.dal[idx] + dfix);
            const double s_n = s + th * (k.ds[idx] - s / al * dfix);
            const double z_n = z + th * (k.dz[idx] + z / (c - al) * dfix);
            al = al_n; s = s_n; z = z_n;
            g_al[idx] = al; g_s[idx] = s; g_z[idx] = z;
          }
        }
        const double ca = c - al;
        const double dinv = 1.0 / (s / al + z / ca);
        const double g_aff = 1.0 - tf;
        if (PASS == PASS_A) {
          const double h = 1.0 - tf;
          T[0] = dinv;
          T[1] = dinv * g_aff * tt;
          T[2] = al * tt;
          T[3] = s * al + z * ca;
          T[4] = al;
          T[5] = c * (h > 0.0 ? h : 0.0);
          continue;
        }
        // predictor
        const double* da_ = s_daff + p * kD1;
        double ud = 0.0;
        for (int i = 0; i < D1; ++i) ud += u[i] * da_[i];
        const double da = dinv * (g_aff - tt * ud);
        const double dsa = -s - s * da / al, dza = -z + z * da / ca;
        if (PASS == PASS_B) {
          double th = boundary(al, da);
          double v = boundary(ca, -da); th = v < th ? v : th;
          v = boundary(s, dsa); th = v < th ? v : th;
          v = boundary(z, dza); th = v < th ? v : th;
          T[0] = s * da + al * dsa + dza * ca - z * da;
          T[1] = dsa * da - dza * da;
          T[2] = dinv * (1.0 / al - 1.0 / ca) * tt;
          T[3] = dinv * (-dsa * da / al - dza * da / ca) * tt;
          T[4] = 0.0;
          T[5] = th;
          continue;
        }
        // corrector
        const double sigmu = s_sigmu[p];
        const double* dd_ = s_dir + p * kD1;
        double uf = 0.0;
        for (int i = 0; i < D1; ++i) uf += u[i] * dd_[i];
        const double g = g_aff + sigmu * (1.0 / al - 1.0 / ca) - dsa * da / al - dza * da / ca;
        const double dal = dinv * (g - tt * uf);
        const double ds = (sigmu - s * al - dsa * da - s * dal) / al;
        const double dz = (sigmu - z * ca + dza * da + z * dal) / ca;
        k.dal[idx] = dal; k.ds[idx] = ds; k.dz[idx] = dz;
        double th = boundary(al, dal);
        double v = boundary(ca, -dal); th = v < th ? v : th;
        v = boundary(s, ds); th = v < th ? v : th;
        v = boundary(z, dz); th = v < th ? v : th;
        if (!(th == th)) th = -1.0;                           // a direction that is not a number: the final launch fails the pair
        T[0] = 0.0; T[1] = 0.0; T[2] = dal * tt; T[3] = 0.0; T[4] = 0.0;
        T[5] = th;
      }
    }
    __syncthreads();
    {
#pragma unroll
      for (int q = 0; q < kMaxOut; ++q) {
        const int o = t + q * kRows;
        if (o >= P * nS) continue;
        const int p = o / nS, e = o - p * nS;
        if (s_phase[p] < 0) continue;
        int pa = 0, rem = p;
        while (rem >= C - 1 - pa) { rem -= C - 1 - pa; ++pa; }
        const int pb_ = pa + 1 + rem;
        int ti, bi = D, bj = D;                               // the term, and the two factors of u (u[D] = 1)
        if (PASS == PASS_A) {
          if (e < nT) { ti = 0; untri(e, &bi, &bj); }
          else if (e < nT + D1) { ti = 1; bi = e - nT; }
          else if (e < nT + 2 * D1) { ti = 2; bi = e - nT - D1; }
          else ti = 3 + (e - nT - 2 * D1);
        } else if (PASS == PASS_B) {
          if (e < 2) ti = e;
          else if (e < 2 + D1) { ti = 2; bi = e - 2; }
          else { ti = 3; bi = e - 2 - D1; }
        } else {
          ti = 2; bi = e;
        }
        double s = acc[q];
#pragma unroll 4
        for (int rr = 0; rr < kRows; ++rr) {
          const int c = s_cls[rr];
          const int slot = c == pa ? pb_ - 1 : (c == pb_ ? pa : -1);
          if (slot >= 0) s += s_term[(rr * kMaxSlots + slot) * kTerms + ti] * (s_u[rr * kD1 + bi] * s_u[rr * kD1 + bj]);
        }
        acc[q] = s;
      }
    }
    if (PASS != PASS_A && t < P && s_phase[t] >= 0) {
      int pa = 0, rem = t;
      while (rem >= C - 1 - pa) { rem -= C - 1 - pa; ++pa; }
      const int pb_ = pa + 1 + rem;
      for (int rr = 0; rr < kRows; ++rr) {
        const int c = s_cls[rr];
        const int slot = c == pa ? pb_ - 1 : (c == pb_ ? pa : -1);
        if (slot >= 0) {
          const double v = s_term[(rr * kMaxSlots + slot) * kTerms + 5];
          tmin = v < tmin ? v : tmin;
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q) {
    const int o = t + q * kRows;
    if (o < P * nS) k.part[(size_t)blockIdx.x * P * nS + o] = acc[q];
  }
  if (PASS != PASS_A && t < P) k.pmin[(size_t)blockIdx.x * P + t] = tmin;
  if (t == 0) k.pbad[blockIdx.x] = s_bad ? 1.0 : 0.0;        // the loop's last barrier is behind every store to s_bad
}

// L L' = M in place (lower triangle), false when a pivot is not positive
__device__ inline bool cholesky(double* M, int n) {
  for (int c = 0; c < n; ++c) {
    double piv = M[c * n + c];
    for (int q = 0; q < c; ++q) piv -= M[c * n + q] * M[c * n + q];
    if (!(piv > 0.0) || !(piv < INFINITY)) return false;
    piv = sqrt(piv);
    M[c * n + c] = piv;
    for (int r = c + 1; r < n; ++r) {
      double v = M[r * n + c];
      for (int q = 0; q < c; ++q) v -= M[r * n + q] * M[c * n + q];
      M[r * n + c] = v / piv;
    }
  }
  return true;
}

__device__ inline void chol_solve(const double* L, int n, const double* rhs, double* out) {
  for (int r = 0; r < n; ++r) {
    double v = rhs[r];
    for (int q = 0; q < r; ++q) v -= L[r * n + q] * out[q];
    out[r] = v / L[r * n + r];
  }
  for (int r = n - 1; r >= 0; --r) {
    double v = out[r];
    for (int q = r + 1; q < n; ++q) v -= L[q * n + r] * out[q];
    out[r] = v / L[r * n + r];
  }
}

// ---- sums of the partials in index order, then the pair's decision.  One workgroup; thread p decides pair p.
// tot: [P n_sums] (kept in the workspace), scratch: [P][kScratch] (the factor and the predictor's right-hand side)
__global__ __launch_bounds__(kFinThreads) void svm_final_kernel(double* __restrict__ st, int C, int D, int pass, int mode, int n_part,
                                                                double gap_tol, const double* __restrict__ part,
                                                                const double* __restrict__ pmin, const double* __restrict__ pbad,
                                                                double* __restrict__ tot, double* __restrict__ scratch) {
  __shared__ int s_active[kMaxP];
  const int P = n_pairs(C), D1 = D + 1, nT = n_tri(D), t = threadIdx.x;
  const int nS = pass == PASS_A ? n_sums_a(D) : (pass == PASS_B ? n_sums_b(D) : D1);
  long long* hdr = reinterpret_cast<long long*>(st);
  if (t < P) {
    const double* pb = st + kHdr + (size_t)t * kPW;
    const long long phase = reinterpret_cast<const long long*>(pb)[PINN_SVM_P_PHASE];
    s_active[t] = mode == MODE_SUMS || (!pair_stopped(pb) && (pass == PASS_A || phase == 2));
  }
  __syncthreads();
  for (int o = t; o < P * nS; o += kFinThreads) {
    if (!s_active[o / nS]) continue;
    double s = 0.0;
    for (int b = 0; b < n_part; ++b) s += part[(size_t)b * P * nS + o];
    tot[o] = s;
  }
  __syncthreads();
  if (mode == MODE_SUMS) return;

  if (t < P && s_active[t]) {
    double* pb = st + kHdr + (size_t)t * kPW;
    long long* pi = reinterpret_cast<long long*>(pb);
    double* L = scratch + (size_t)t * kScratch;
    double* rhs_aff = L + kD1 * kD1;
    const double* S = tot + (size_t)t * nS;
    double theta = INFINITY;
    if (pass != PASS_A)
      for (int b = 0; b < n_part; ++b) { const double v = pmin[(size_t)b * P + t]; theta = v < theta ? v : theta; }
    bool bad = false;
    for (int b = 0; b < n_part; ++b) bad = bad || pbad[b] != 0.0;
    if (bad) {
      pi[PINN_SVM_P_STATUS] = PINN_SVM_RANGE;
    } else if (pass == PASS_A) {
      const double* Wsum = S + nT + D1;
      if (pi[PINN_SVM_P_PHASE] == 0) {
        bool okw = true;
        for (int i = 0; i < D; ++i) { pb[PINN_SVM_P_W + i] = Wsum[i]; okw = okw && finite(Wsum[i]); }
        pb[PINN_SVM_P_BETA] = 0.0;
        pi[PINN_SVM_P_PHASE] = 1;
        if (!okw) pi[PINN_SVM_P_STATUS] = PINN_SVM_NAN;
      } else {
        bool fin = true;
        for (int e = 0; e < nS; ++e) fin = fin && finite(S[e]);
        const double m = pb[PINN_SVM_P_M], compl_ = S[nT + 2 * D1], sum_al = S[nT + 2 * D1 + 1], hinge = S[nT + 2 * D1 + 2];
        double ww = 0.0, vv = 0.0;
        double rw = 0.0;                                      // max |w - V'alpha|
        for (int i = 0; i < D; ++i) {
          ww += pb[PINN_SVM_P_W + i] * pb[PINN_SVM_P_W + i]; vv += Wsum[i] * Wsum[i];
          pb[PINN_SVM_P_RW + i] = pb[PINN_SVM_P_W + i] - Wsum[i];
          const double r = fabs(pb[PINN_SVM_P_RW + i]);
          rw = r > rw ? r : rw;
        }
        const double primal = 0.5 * ww + hinge, dual = sum_al - 0.5 * vv, gap = primal - dual;
        pb[PINN_SVM_P_MU] = compl_ / (2.0 * m);
        pb[PINN_SVM_P_GAP] = gap; pb[PINN_SVM_P_PRIMAL] = primal; pb[PINN_SVM_P_DUAL] = dual;
        pb[PINN_SVM_P_COMPL] = compl_; pb[PINN_SVM_P_TALPHA] = Wsum[D]; pb[PINN_SVM_P_SUMALPHA] = sum_al;
        pi[PINN_SVM_P_PHASE] = 2;
        if (!fin) {
          pi[PINN_SVM_P_STATUS] = PINN_SVM_NAN;
        } else if (gap <= gap_tol * (primal > 1.0 ? primal : 1.0) && fabs(Wsum[D]) <= 1e-12 * sum_al && rw <= 1e-13 * sum_al) {
          pi[PINN_SVM_P_CONVERGED] = 1;
        } else {
          for (int r = 0; r < D1; ++r)
            for (int q = 0; q < D1; ++q) {
              const int lo = r < q ? r : q, hi = r < q ? q : r;
              L[r * D1 + q] = S[hi * (hi + 1) / 2 + lo] + ((r == q && r < D) ? 1.0 : 0.0);
            }
          for (int i = 0; i < D1; ++i) {
            double v = S[nT + i];
            if (i < D) v -= pb[PINN_SVM_P_W + i] - Wsum[i];
            else v += Wsum[D];
            rhs_aff[i] = v;
          }
          if (!cholesky(L, D1)) pi[PINN_SVM_P_STATUS] = PINN_SVM_SINGULAR;
          else chol_solve(L, D1, rhs_aff, pb + PINN_SVM_P_DAFF);
        }
      }
    } else if (pass == PASS_B) {
      const double th = theta < 1.0 ? theta : 1.0, m = pb[PINN_SVM_P_M], mu = pb[PINN_SVM_P_MU];
      const double mu_aff = (pb[PINN_SVM_P_COMPL] + th * S[0] + th * th * S[1]) / (2.0 * m);
      double ratio = mu_aff / mu;
      ratio = ratio > 0.0 ? (ratio < 1.0 ? ratio : 1.0) : 0.0;          // NaN -> 0
      // no complementarity below a tenth of what gap_tol asks for: the matrix entries grow like 1 / mu, and so does the rounding
      const double primal = pb[PINN_SVM_P_PRIMAL], floor_ = kMuFloor * gap_tol * (primal > 1.0 ? primal : 1.0) / (2.0 * m);
      double sigmu = ratio * ratio * ratio * mu;
      sigmu = sigmu > floor_ ? sigmu : floor_;
      double rhs[kD1];
      for (int i = 0; i < D1; ++i) rhs[i] = rhs_aff[i] + sigmu * S[2 + i] + S[2 + D1 + i];
      chol_solve(L, D1, rhs, pb + PINN_SVM_P_DIR);
      pb[PINN_SVM_P_SIGMU] = sigmu;
      pb[PINN_SVM_P_THETA_AFF] = th;
      bool fin = finite(sigmu);
      for (int i = 0; i < D1; ++i) fin = fin && finite(pb[PINN_SVM_P_DIR + i]);
      if (!fin) pi[PINN_SVM_P_STATUS] = PINN_SVM_NAN;
    } else {
      double th = kStepToBoundary * theta;
      th = th < 1.0 ? th : 1.0;
      if (!(th > 0.0)) {
        pi[PINN_SVM_P_STATUS] = PINN_SVM_NAN;
      } else {
        // The entries of the normal equations grow like 1 / mu, so the row directions satisfy V'dal = dw and t'dal = -t'al
        // only to about eps |M| |d|: near the end that is 1e-12, which the hinge sum does not forgive.  One step of refinement
        // with the sums of the row directions themselves: M fix = (V'dal - (w - V'al) - dw, t'dal + t'al); pass A subtracts t u.fix / d.
        double e[kD1];
        for (int i = 0; i < D; ++i) e[i] = S[i] - pb[PINN_SVM_P_DIR + i] - pb[PINN_SVM_P_RW + i];
        e[D] = S[D] + pb[PINN_SVM_P_TALPHA];
        chol_solve(L, D1, e, pb + PINN_SVM_P_FIX);
        pb[PINN_SVM_P_THETA] = th;
        for (int i = 0; i < D; ++i) pb[PINN_SVM_P_W + i] = pb[PINN_SVM_P_W + i] + th * (pb[PINN_SVM_P_DIR + i] + pb[PINN_SVM_P_FIX + i]);
        pb[PINN_SVM_P_BETA] = pb[PINN_SVM_P_BETA] + th * (pb[PINN_SVM_P_DIR + D] + pb[PINN_SVM_P_FIX + D]);
        pi[PINN_SVM_P_ITER] += 1;
        pi[PINN_SVM_P_PHASE] = 3;
      }
    }
  }
  __syncthreads();
  if (t == 0) {
    long long conv = 1, status = 0, iter = 0;
    for (int p = 0; p < P; ++p) {
      const long long* pi = reinterpret_cast<const long long*>(st + kHdr + (size_t)p * kPW);
      conv = conv && pi[PINN_SVM_P_CONVERGED] != 0;
      status |= pi[PINN_SVM_P_STATUS];
      iter = pi[PINN_SVM_P_ITER] > iter ? pi[PINN_SVM_P_ITER] : iter;
    }
    hdr[PINN_SVM_ST_ITER] = iter; hdr[PINN_SVM_ST_CONVERGED] = conv; hdr[PINN_SVM_ST_STATUS] = status;
  }
}

// ---- decision of given rows: one thread per row, every output optional.
// model: mean [D], scale [D], W [P][D], b [P]; a value is positive for the pair's first class
__global__ __launch_bounds__(kRows) void svm_decision_kernel(Rows a, const double* __restrict__ model, double* __restrict__ dec_out,
                                                             long long* __restrict__ votes_out, long long* __restrict__ pred_out) {
  __shared__ double s_mean[kMaxD], s_scale[kMaxD], s_W[kMaxP * kMaxD], s_b[kMaxP];
  const int C = a.K, D = a.D, P = n_pairs(C), t = threadIdx.x;
  if (t < D) { s_mean[t] = model[t]; s_scale[t] = model[D + t]; }
  for (int e = t; e < P * D; e += kRows) s_W[e] = model[2 * D + e];
  if (t < P) s_b[t] = model[2 * D + P * D + t];
  __syncthreads();
  const long long j = (long long)blockIdx.x * kRows + t;
  if (j >= a.n) return;
  double x[kRowsMaxD], u[kMaxD];
  const bool ok = load_row(a, j, x);
  for (int i = 0; i < D; ++i) u[i] = (x[i] - s_mean[i]) / s_scale[i];
  const auto value = [&](int, int, int p) {
    double v = 0.0;
    for (int i = 0; i < D; ++i) v += s_W[p * D + i] * u[i];
    return v + s_b[p];
  };
  ovo_decide(value, ok, C, j, dec_out, votes_out, pred_out);
}

struct Ws {
  double *tot, *scratch, *part, *pmin, *pbad, *dal, *ds, *dz;
};

// workspace: totals [P n_sums_a] (first, so that the caller can read the summed pass), the pairs' scratch, partials,
// partial minima and flags, the three direction arrays
inline size_t carve(void* d_ws, long long n, int C, int D, Ws* s) {
  char* w = static_cast<char*>(d_ws);
  const size_t P = n_pairs(C), nS = n_sums_a(D), rows = align256((size_t)n * (C - 1) * sizeof(double));
  size_t o = 0;
  if (s) s->tot = reinterpret_cast<double*>(w + o);
  o += align256(P * nS * sizeof(double));
  if (s) s->scratch = reinterpret_cast<double*>(w + o);
  o += align256(P * kScratch * sizeof(double));
  if (s) s->part = reinterpret_cast<double*>(w + o);
  o += align256((size_t)kMaxBlocks * P * nS * sizeof(double));
  if (s) s->pmin = reinterpret_cast<double*>(w + o);
  o += align256((size_t)kMaxBlocks * P * sizeof(double));
  if (s) s->pbad = reinterpret_cast<double*>(w + o);
  o += align256((size_t)kMaxBlocks * sizeof(double));
  if (s) { s->dal = reinterpret_cast<double*>(w + o); s->ds = reinterpret_cast<double*>(w + o + rows); s->dz = reinterpret_cast<double*>(w + o + 2 * rows); }
  return o + 3 * rows;
}

template <int PASS>
inline void launch_pass(const Rows& a, const Pass& k, int nb, int C, int D, int mode, double gap_tol, const Ws& w, hipStream_t st) {
  hipLaunchKernelGGL(svm_rows_kernel<PASS>, dim3((unsigned)nb), dim3(kRows), 0, st, a, k);
  hipLaunchKernelGGL(svm_final_kernel, dim3(1), dim3(kFinThreads), 0, st, k.st, C, D, PASS, mode, nb, gap_tol, w.part, w.pmin, w.pbad, w.tot, w.scratch);
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_svm_state_bytes(long long n_rows, int n_classes, int n_feat) {
  if (n_rows < 0 || !pinn::in_limits(n_classes, n_feat)) return 0;
  return pinn::st_words(n_rows, n_classes, n_feat) * sizeof(double);
}

extern "C" size_t pinn_svm_workspace_bytes(long long n_rows, int n_classes, int n_feat) {
  if (n_rows < 0 || !pinn::in_limits(n_classes, n_feat)) return 0;
  return pinn::carve(nullptr, n_rows, n_classes, n_feat, nullptr);
}

#define SVM_COMMON_CHECKS()                                                                         \
  if (!pinn::in_limits(n_classes, n_feat)) return PINN_E_ARG;                                       \
  Rows a;                                                                                           \
  {                                                                                                 \
    const int rc_ = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_classes, d_row_index, n, &a);  \
    if (rc_ != PINN_OK) return rc_;                                                                 \
  }                                                                                                 \
  if (!d_state || !d_ws || !d_y || misaligned8(d_state) || misaligned8(d_ws) || misaligned8(d_y)) return PINN_E_ARG; \
  if (n < 1) return PINN_E_ARG;                                                                     \
  if (ws_bytes < pinn_svm_workspace_bytes(n, n_classes, n_feat)) return PINN_E_WORKSPACE;           \
  Ws w;                                                                                             \
  carve(d_ws, n, n_classes, n_feat, &w);                                                            \
  hipStream_t st = (hipStream_t)stream;                                                             \
  const int nb = row_blocks(n, kRows, kMaxBlocks);                                                  \
  clear_error()

extern "C" int pinn_svm_pass(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                             const long long* d_row_index, long long n, const long long* d_y, int n_classes,
                             const double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  SVM_COMMON_CHECKS();
  const Pass k = {const_cast<double*>(d_state), d_y, w.dal, w.ds, w.dz, w.part, w.pmin, w.pbad, MODE_SUMS};
  launch_pass<PASS_A>(a, k, nb, n_classes, n_feat, MODE_SUMS, 0.0, w, st);
  return launch_status();
}

extern "C" int pinn_svm_ipm(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                            const long long* d_row_index, long long n, const long long* d_y, int n_classes, int init,
                            int n_iter, double gap_tol, double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  SVM_COMMON_CHECKS();
  if (n_iter < 0 || n_iter > 100000 || !(gap_tol > 0.0)) return PINN_E_ARG;
  const Pass k = {d_state, d_y, w.dal, w.ds, w.dz, w.part, w.pmin, w.pbad, MODE_RUN};
  if (init) {                                   // alpha and w = V'alpha, then s and z and the sums at the starting point
    launch_pass<PASS_A>(a, k, nb, n_classes, n_feat, MODE_RUN, gap_tol, w, st);
    launch_pass<PASS_A>(a, k, nb, n_classes, n_feat, MODE_RUN, gap_tol, w, st);
  }
  for (int it = 0; it < n_iter; ++it) {
    launch_pass<PASS_B>(a, k, nb, n_classes, n_feat, MODE_RUN, gap_tol, w, st);
    launch_pass<PASS_C>(a, k, nb, n_classes, n_feat, MODE_RUN, gap_tol, w, st);
    launch_pass<PASS_A>(a, k, nb, n_classes, n_feat, MODE_RUN, gap_tol, w, st);
  }
  return launch_status();
}

extern "C" int pinn_svm_decision(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                 const long long* d_row_index, long long n, int n_classes, const double* d_model,
                                 double* d_decision, long long* d_votes, long long* d_pred, void* stream) {
  using namespace pinn;
  if (!in_limits(n_classes, n_feat)) return PINN_E_ARG;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_classes, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_model || misaligned8(d_model) || misaligned8(d_decision) || misaligned8(d_votes) || misaligned8(d_pred)) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  const long long tiles = (n + kRows - 1) / kRows;
  if (tiles > 0x7fffffffLL) return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(svm_decision_kernel, dim3((unsigned)tiles), dim3(kRows), 0, (hipStream_t)stream, a, d_model, d_decision, d_votes, d_pred);
  return launch_status();
}
