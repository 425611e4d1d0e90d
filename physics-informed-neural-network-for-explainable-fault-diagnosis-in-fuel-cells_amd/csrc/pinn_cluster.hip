// Clustering baselines of the method comparison on the device (reference script 05, cited as 05:<line>):
//   pinn_km_lloyd        Lloyd iterations with scikit-learn's stopping rule, labels / inertia / n_iter left in the state
//   pinn_ward_tree       Ward dendrogram by the nearest-neighbour chain on cluster means and sizes, O(n) memory
//   pinn_cluster_means   mean of the rows of every label
//   pinn_cluster_assign  nearest centre, and the class distribution of that cluster                    (05:384-392)
// All arithmetic is float64, every operation rounded on its own (built with -ffp-contract=off).
//
// k-means: a workgroup takes tiles of 128 rows, one thread per row finds the nearest centre and writes the label into
// LDS; then every thread owns up to 5 of the K x (1 + 2 D) sums (count, sum of d, sum of d^2 with d = x - the centre the
// pass started from) and adds the tile's terms in row order.  Workgroup sums go to the workspace; a one-workgroup launch
// adds them in index order, moves the centres and tests scikit-learn's two stopping rules.  "The labels did not change"
// is a count every workgroup keeps while it overwrites the labels, so the test needs no host read.
//
// Ward: one chain step is two launches: a scan of all slots for the nearest neighbour of the chain's tip (argmin by
// (distance, index): the result does not depend on the order of the reduction), then a one-workgroup decision that merges
// tip and predecessor or pushes the neighbour.  This is the general form; a single-workgroup form with the slots in LDS
// for small n is not in the tree (it was not measured).
//
// No float atomics, no workgroup waits on another: stream order is the only dependency, and the same call gives the same
// bytes every time.  Once a state's converged flag or status word is set every later launch returns at once.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kT = 128;                     // rows per tile = threads per workgroup of a row pass
constexpr int kMaxK = PINN_CL_MAX_CLUSTERS, kMaxD = PINN_CL_MAX_FEAT, kMaxC = PINN_CL_MAX_CLASSES;
constexpr int kMaxOut = (kMaxK * (1 + 2 * kMaxD) + kT - 1) / kT;      // output sums per thread: 5
constexpr int kMaxBlocks = 1024;            // workgroups of a row pass = partial sums per output
constexpr int kFinThreads = 256;
constexpr int kHdr = PINN_CL_ST_HEADER;     // 8-byte words of a state header
constexpr int kScanThreads = 256, kScanBlocks = 256;

static_assert(kMaxD == kRowsMaxD && kMaxK == kRowsMaxK, "pinn_rows.h carries the same limits");

enum { LAB_ASSIGN = 0, LAB_WRITE = 1, LAB_GIVEN = 2, LAB_FINISH = 3 };
enum { FIN_MEAN = 0, FIN_VAR = 1, FIN_LLOYD = 2, FIN_FINISH = 3, FIN_LABEL_MEANS = 4 };

// k-means state: header, centres [K][D], counts [K] (doubles), mean [D], labels [n] (64-bit integers)
__host__ __device__ inline size_t km_centres() { return kHdr; }
__host__ __device__ inline size_t km_counts(int K, int D) { return kHdr + (size_t)K * D; }
__host__ __device__ inline size_t km_mean(int K, int D) { return km_counts(K, D) + (size_t)K; }
__host__ __device__ inline size_t km_labels(int K, int D) { return km_mean(K, D) + (size_t)D; }
__host__ __device__ inline size_t km_words(long long n, int K, int D) { return km_labels(K, D) + (size_t)n; }

// Ward state: header, mean [n][D], size [n], chain [n], lo [n], hi [n] (64-bit integers), height [n]
__host__ __device__ inline size_t wd_mean() { return kHdr; }
__host__ __device__ inline size_t wd_size(long long n, int D) { return kHdr + (size_t)n * D; }
__host__ __device__ inline size_t wd_chain(long long n, int D) { return wd_size(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_lo(long long n, int D) { return wd_chain(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_hi(long long n, int D) { return wd_lo(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_height(long long n, int D) { return wd_hi(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_words(long long n, int D) { return wd_height(n, D) + (size_t)n; }

__device__ __forceinline__ bool stopped(const double* st) {
  const long long* h = reinterpret_cast<const long long*>(st);
  return h[PINN_CL_ST_CONVERGED] != 0 || h[PINN_CL_ST_STATUS] != 0;
}

// nearest of K centres [K][D] by sum (x - c)^2, the first of equals
__device__ __forceinline__ int nearest(const double x[kMaxD], const double* __restrict__ mu, int K, int D, double* d2_out) {
  int best = 0;
  double bd = INFINITY;
  for (int k = 0; k < K; ++k) {
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < kMaxD; ++i)
      if (i < D) { const double d = x[i] - mu[k * D + i]; d2 += d * d; }
    if (d2 < bd) { bd = d2; best = k; }
  }
  *d2_out = bd;
  return best;
}

// ---- the row pass: K x F sums per workgroup, F = 1 + 2 D columns (1, d_i, d_i^2) with d = x - centre of the row's label.
// part: [gridDim.x][K * F]; part_chg: [gridDim.x] labels that differ from the stored ones (LAB_WRITE).
__global__ __launch_bounds__(kT) void km_rows_kernel(Rows a, const double* __restrict__ st, const double* __restrict__ centres, int mode,
                                                     long long* __restrict__ labels, int force, double* __restrict__ part,
                                                     long long* __restrict__ part_chg) {
  __shared__ double s_x[kT * (kMaxD + 1)];
  __shared__ double s_mu[kMaxK * kMaxD];
  __shared__ int s_lab[kT];
  __shared__ long long s_chg[kT];
  if (!force && stopped(st)) return;
  const int K = a.K, D = a.D, Dp = D | 1, F = 1 + 2 * D, KF = K * F, t = threadIdx.x;
  if (mode == LAB_FINISH) mode = reinterpret_cast<const long long*>(st)[PINN_KM_ST_STRICT] != 0 ? LAB_GIVEN : LAB_WRITE;
  for (int e = t; e < K * D; e += kT) s_mu[e] = centres[e];
  __syncthreads();

  int ok_[kMaxOut], of[kMaxOut];
  double acc[kMaxOut];
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q) {
    const int o = t + q * kT;
    acc[q] = 0.0;
    ok_[q] = -1; of[q] = 0;
    if (o < KF) { ok_[q] = o / F; of[q] = o - ok_[q] * F; }
  }

  long long chg = 0;
  const long long tiles = (a.n + kT - 1) / kT;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long j = tile * kT + t;
    double x[kMaxD];
    int lab = -1;
    if (j < a.n) {
      const bool ok = load_row(a, j, x);
      if (mode == LAB_GIVEN) {
        const long long l = labels[j];
        lab = (ok && l >= 0 && l < K) ? (int)l : -1;
      } else {
        double d2;
        if (ok) lab = nearest(x, s_mu, K, D, &d2);
        if (mode == LAB_WRITE) {
          chg += labels[j] != (long long)lab;
          labels[j] = lab;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < kMaxD; ++i) x[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < kMaxD; ++i)
      if (i < D) s_x[t * Dp + i] = x[i];
    s_lab[t] = lab;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kMaxOut; ++q) {
      const int k = ok_[q];
      if (k >= 0) {
        const int f = of[q];
        double s = acc[q];
        if (f == 0) {
          for (int rr = 0; rr < kT; ++rr) s += s_lab[rr] == k ? 1.0 : 0.0;
        } else if (f <= D) {
          const double m = s_mu[k * D + f - 1];
          for (int rr = 0; rr < kT; ++rr) s += s_lab[rr] == k ? s_x[rr * Dp + f - 1] - m : 0.0;
        } else {
          const double m = s_mu[k * D + f - 1 - D];
          for (int rr = 0; rr < kT; ++rr) {
            const double d = s_x[rr * Dp + f - 1 - D] - m;
            s += s_lab[rr] == k ? d * d : 0.0;
          }
        }
        acc[q] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kMaxOut; ++q)
    if (ok_[q] >= 0) part[(size_t)blockIdx.x * KF + t + q * kT] = acc[q];
  s_chg[t] = chg;
  __syncthreads();
  if (t == 0) {
    long long s = 0;
    for (int rr = 0; rr < kT; ++rr) s += s_chg[rr];
    part_chg[blockIdx.x] = s;
  }
}

// ---- sums of the partials in index order, then what the mode asks for.  One workgroup.  K: clusters of the pass;
// tot: [K * F] totals (kept at the start of the workspace for the caller).
__global__ __launch_bounds__(kFinThreads) void km_final_kernel(double* __restrict__ st, double* __restrict__ centres, double* __restrict__ counts,
                                                                int K, int D, int mode, int n_part, long long n, int K_state, double tol,
                                                                const double* __restrict__ part, const long long* __restrict__ part_chg,
                                                                double* __restrict__ tot) {
  __shared__ double n_mu[kMaxK * kMaxD], s_shift[kMaxK], s_in[kMaxK];
  long long* hdr = reinterpret_cast<long long*>(st);
  if (mode == FIN_LLOYD && stopped(st)) return;
  const int F = 1 + 2 * D, KF = K * F, t = threadIdx.x;
  for (int o = t; o < KF; o += kFinThreads) {
    double s = 0.0;
    for (int g = 0; g < n_part; ++g) s += part[(size_t)g * KF + o];
    tot[o] = s;
  }
  __syncthreads();

  if (mode == FIN_MEAN) {                                      // K = 1, centre 0: the column means
    if (t < D) st[km_mean(K_state, D) + t] = tot[0] > 0.0 ? tot[1 + t] / tot[0] : 0.0;
    return;
  }
  if (mode == FIN_VAR) {                                       // K = 1, centre = the means: tol_abs = tol mean_j var_j (KMeans._tolerance)
    if (t == 0) {
      double s = 0.0;
      for (int i = 0; i < D; ++i) s += tot[0] > 0.0 ? tot[1 + D + i] / tot[0] : 0.0;
      hdr[PINN_CL_ST_ITER] = 0; hdr[PINN_CL_ST_CONVERGED] = 0; hdr[PINN_CL_ST_STATUS] = 0;
      hdr[PINN_KM_ST_K] = K_state; hdr[PINN_KM_ST_D] = D; hdr[PINN_KM_ST_N] = n;
      hdr[PINN_KM_ST_STRICT] = 0; hdr[PINN_KM_ST_CHANGED] = 0; hdr[PINN_KM_ST_DONE] = 0;
      st[PINN_KM_ST_INERTIA] = INFINITY; st[PINN_KM_ST_SHIFT] = INFINITY;
      st[PINN_KM_ST_TOL_ABS] = tol * (s / (double)D);
    }
    return;
  }
  if (t < K) {
    const double cnt = tot[t * F];
    double sh = 0.0, in = 0.0;
    for (int i = 0; i < D; ++i) {
      const double old = centres[t * D + i];
      const double nw = (mode != FIN_FINISH && cnt > 0.0) ? old + tot[t * F + 1 + i] / cnt : old;   // an empty cluster keeps its centre
      n_mu[t * D + i] = nw;
      sh += (nw - old) * (nw - old);
      in += tot[t * F + 1 + D + i];
    }
    s_shift[t] = sh;
    s_in[t] = in;
  }
  __syncthreads();
  double shift = 0.0, inertia = 0.0;
  for (int k = 0; k < K; ++k) { shift += s_shift[k]; inertia += s_in[k]; }
  const bool bad = !(shift == shift) || !(inertia == inertia);
  if (bad && mode != FIN_LABEL_MEANS) {
    if (t == 0) hdr[PINN_CL_ST_STATUS] = PINN_CL_NAN;            // the state keeps the last good centres
    return;
  }
  if (t < K) {
    for (int i = 0; i < D; ++i) centres[t * D + i] = n_mu[t * D + i];
    if (counts) counts[t] = tot[t * F];
  }
  if (t != 0 || mode == FIN_LABEL_MEANS) return;
  if (mode == FIN_FINISH) {
    st[PINN_KM_ST_INERTIA] = inertia;
    hdr[PINN_KM_ST_DONE] = 1;
    return;
  }
  long long chg = 0;
  for (int g = 0; g < n_part; ++g) chg += part_chg[g];
  hdr[PINN_CL_ST_ITER] += 1;
  hdr[PINN_KM_ST_CHANGED] = chg;
  st[PINN_KM_ST_INERTIA] = inertia;                             // of the assignment to the centres the pass started from
  st[PINN_KM_ST_SHIFT] = shift;
  if (chg == 0) {                                               // scikit-learn's strict convergence
    hdr[PINN_KM_ST_STRICT] = 1;
    hdr[PINN_CL_ST_CONVERGED] = 1;
  } else if (shift <= st[PINN_KM_ST_TOL_ABS]) {
    hdr[PINN_CL_ST_CONVERGED] = 1;
  }
}

// ---- Ward
// d^2 between clusters (mean a, size sa) and (mean b, size sb); the same bytes with the arguments exchanged
__device__ __forceinline__ double ward_d2(const double* a, double sa, const double* __restrict__ b, double sb, int D) {
  double ss = 0.0;
#pragma unroll
  for (int i = 0; i < kMaxD; ++i)
    if (i < D) { const double d = a[i] - b[i]; ss += d * d; }
  return 2.0 * (sa * sb) / (sa + sb) * ss;
}

__global__ __launch_bounds__(kScanThreads) void ward_init_kernel(Rows a, double* __restrict__ st) {
  const long long j = (long long)blockIdx.x * kScanThreads + threadIdx.x;
  if (j >= a.n) return;
  double x[kMaxD];
  const bool ok = load_row(a, j, x);
  for (int i = 0; i < a.D; ++i) st[wd_mean() + (size_t)j * a.D + i] = x[i];
  reinterpret_cast<long long*>(st)[wd_size(a.n, a.D) + j] = ok ? 1 : 0;
}

// header, and the first active slot as the chain's start.  One thread.
__global__ void ward_start_kernel(double* __restrict__ st, long long n, int D) {
  long long* hdr = reinterpret_cast<long long*>(st);
  const long long* size = hdr + wd_size(n, D);
  for (int w = 0; w < kHdr; ++w) hdr[w] = 0;
  hdr[PINN_WARD_ST_N] = n; hdr[PINN_WARD_ST_D] = D;
  long long f = 0;
  while (f < n && size[f] == 0) ++f;
  hdr[PINN_WARD_ST_FIRST] = f;
  if (f >= n) { hdr[PINN_CL_ST_CONVERGED] = 1; return; }
  hdr[wd_chain(n, D)] = f;
  hdr[PINN_WARD_ST_CHAIN] = 1;
}

__device__ __forceinline__ bool closer(double d, long long j, double d2, long long j2) { return d < d2 || (d == d2 && j < j2); }

// nearest active slot of the chain's tip: per workgroup the minimum by (d^2, index)
__global__ __launch_bounds__(kScanThreads) void ward_scan_kernel(const double* __restrict__ st, long long n, int D, double* __restrict__ part_d,
                                                                  long long* __restrict__ part_j) {
  __shared__ double s_d[kScanThreads];
  __shared__ long long s_j[kScanThreads];
  if (stopped(st)) return;
  const long long* hdr = reinterpret_cast<const long long*>(st);
  const long long* size = hdr + wd_size(n, D);
  const long long tip = hdr[wd_chain(n, D) + hdr[PINN_WARD_ST_CHAIN] - 1];
  double tm[kMaxD];
#pragma unroll
  for (int i = 0; i < kMaxD; ++i) tm[i] = i < D ? st[wd_mean() + (size_t)tip * D + i] : 0.0;
  const double ts = (double)size[tip];
  double best = INFINITY;
  long long bj = n;
  const int t = threadIdx.x;
  for (long long j = (long long)blockIdx.x * kScanThreads + t; j < n; j += (long long)gridDim.x * kScanThreads) {
    const long long s = size[j];
    if (s > 0 && j != tip) {
      const double d = ward_d2(tm, ts, st + wd_mean() + (size_t)j * D, (double)s, D);
      if (d < best) { best = d; bj = j; }                     // j ascends: the first of equals stays
    }
  }
  s_d[t] = best; s_j[t] = bj;
  __syncthreads();
  for (int w = kScanThreads / 2; w > 0; w >>= 1) {
    if (t < w && closer(s_d[t + w], s_j[t + w], s_d[t], s_j[t])) { s_d[t] = s_d[t + w]; s_j[t] = s_j[t + w]; }
    __syncthreads();
  }
  if (t == 0) { part_d[blockIdx.x] = s_d[0]; part_j[blockIdx.x] = s_j[0]; }
}

// scipy's rule: the chain's predecessor is the candidate to begin with and another slot replaces it only when strictly
// closer; then either the merge of tip and predecessor or a push.  One workgroup.
__global__ __launch_bounds__(kScanThreads) void ward_decide_kernel(double* __restrict__ st, long long n, int D, int n_part,
                                                                    const double* __restrict__ part_d, const long long* __restrict__ part_j) {
  __shared__ double s_d[kScanThreads];
  __shared__ long long s_j[kScanThreads];
  if (stopped(st)) return;
  const int t = threadIdx.x;
  s_d[t] = t < n_part ? part_d[t] : INFINITY;
  s_j[t] = t < n_part ? part_j[t] : n;
  __syncthreads();
  for (int w = kScanThreads / 2; w > 0; w >>= 1) {
    if (t < w && closer(s_d[t + w], s_j[t + w], s_d[t], s_j[t])) { s_d[t] = s_d[t + w]; s_j[t] = s_j[t + w]; }
    __syncthreads();
  }
  if (t != 0) return;
  long long* hdr = reinterpret_cast<long long*>(st);
  long long* size = hdr + wd_size(n, D);
  long long* chain = hdr + wd_chain(n, D);
  double* mean = st + wd_mean();
  const double dmin = s_d[0];
  const long long jmin = s_j[0];
  long long L = hdr[PINN_WARD_ST_CHAIN];
  const long long tip = chain[L - 1];
  hdr[PINN_CL_ST_ITER] += 1;
  double d0 = INFINITY;
  long long pred = -1;
  if (L > 1) {
    pred = chain[L - 2];
    d0 = ward_d2(mean + (size_t)tip * D, (double)size[tip], mean + (size_t)pred * D, (double)size[pred], D);
  }
  if (dmin < d0) {                                              // push (jmin < n: a finite distance was found)
    if (L >= n) { hdr[PINN_CL_ST_STATUS] = PINN_CL_NAN; return; }   // cannot happen with ordered distances: the chain holds distinct slots
    chain[L] = jmin;
    hdr[PINN_WARD_ST_CHAIN] = L + 1;
    return;
  }
  if (L < 2) {                                                  // no other active slot: nothing is left to merge
    hdr[PINN_CL_ST_CONVERGED] = 1;
    return;
  }
  const long long lo = tip < pred ? tip : pred, hi = tip < pred ? pred : tip, m = hdr[PINN_WARD_ST_MERGES];
  const double sl = (double)size[lo], sh = (double)size[hi], w = sl / (sl + sh);
  hdr[wd_lo(n, D) + m] = lo;
  hdr[wd_hi(n, D) + m] = hi;
  st[wd_height(n, D) + m] = sqrt(d0);
  for (int i = 0; i < D; ++i) {                                 // the size-weighted mean, as a step from the higher slot's mean
    const double mh = mean[(size_t)hi * D + i];
    mean[(size_t)hi * D + i] = mh + w * (mean[(size_t)lo * D + i] - mh);
  }
  size[hi] = size[hi] + size[lo];
  size[lo] = 0;
  L -= 2;
  hdr[PINN_WARD_ST_MERGES] = m + 1;
  if (m + 1 >= n - 1) hdr[PINN_CL_ST_CONVERGED] = 1;
  if (L == 0) {
    long long f = hdr[PINN_WARD_ST_FIRST];
    while (f < n && size[f] == 0) ++f;                          // slots never come back: the cursor only moves up
    hdr[PINN_WARD_ST_FIRST] = f;
    chain[0] = f;
    L = 1;
  }
  hdr[PINN_WARD_ST_CHAIN] = L;
}

// ---- nearest centre and the class distribution of that cluster: one thread per row, every output optional
__global__ __launch_bounds__(kT) void cluster_assign_kernel(Rows a, const double* __restrict__ centres, const double* __restrict__ map, int C,
                                                            long long* __restrict__ idx_out, double* __restrict__ d2_out,
                                                            double* __restrict__ prob_out, long long* __restrict__ pred_out) {
  __shared__ double s_mu[kMaxK * kMaxD];
  __shared__ double s_map[kMaxK * kMaxC];
  const int K = a.K, D = a.D, t = threadIdx.x;
  for (int e = t; e < K * D; e += kT) s_mu[e] = centres[e];
  if (map)
    for (int e = t; e < K * C; e += kT) s_map[e] = map[e];
  __syncthreads();
  const long long j = (long long)blockIdx.x * kT + t;
  if (j >= a.n) return;
  double x[kMaxD];
  const bool ok = load_row(a, j, x);
  double d2 = quiet_nan();
  int k = -1;
  if (ok) k = nearest(x, s_mu, K, D, &d2);
  if (idx_out) idx_out[j] = k;
  if (d2_out) d2_out[j] = d2;
  if (map && (prob_out || pred_out)) {
    int best = -1;
    double bv = -INFINITY;
    for (int c = 0; c < C; ++c) {
      const double v = ok ? s_map[k * C + c] : quiet_nan();
      if (prob_out) prob_out[j * C + c] = v;
      if (v > bv) { bv = v; best = c; }
    }
    if (pred_out) pred_out[j] = best;
  }
}

struct Ws {
  double *tot, *part;
  long long* part_chg;
};

inline size_t km_tot_bytes(int K, int D) { return align256((size_t)K * (1 + 2 * D) * sizeof(double)); }
inline size_t km_part_bytes(int K, int D) { return align256((size_t)kMaxBlocks * K * (1 + 2 * D) * sizeof(double)); }

// workspace: totals [K F] (first, so that the caller can read the summed terms), partials, changed-label counts
inline Ws carve(void* d_ws, int K, int D) {
  char* w = static_cast<char*>(d_ws);
  Ws s;
  s.tot = reinterpret_cast<double*>(w); w += km_tot_bytes(K, D);
  s.part = reinterpret_cast<double*>(w); w += km_part_bytes(K, D);
  s.part_chg = reinterpret_cast<long long*>(w);
  return s;
}

inline bool limits_ok(int K, int D) { return K >= 1 && K <= kMaxK && D >= 1 && D <= kMaxD; }

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_km_state_bytes(long long n_rows, int n_clusters, int n_feat) {
  if (n_rows < 0 || !pinn::limits_ok(n_clusters, n_feat)) return 0;
  return pinn::km_words(n_rows, n_clusters, n_feat) * sizeof(double);
}

extern "C" size_t pinn_km_workspace_bytes(long long n_rows, int n_clusters, int n_feat) {
  using namespace pinn;
  if (n_rows < 0 || !limits_ok(n_clusters, n_feat)) return 0;
  return km_tot_bytes(n_clusters, n_feat) + km_part_bytes(n_clusters, n_feat) + align256(kMaxBlocks * sizeof(long long));
}

extern "C" int pinn_km_lloyd(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                             const long long* d_row_index, long long n, int n_clusters, int init, int n_iters, double tol, int finish,
                             double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_clusters, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_state || !d_ws || misaligned8(d_state) || misaligned8(d_ws)) return PINN_E_ARG;
  if (n < 1 || n_iters < 0 || n_iters > 100000 || !(tol >= 0.0)) return PINN_E_ARG;
  if (ws_bytes < pinn_km_workspace_bytes(n, n_clusters, n_feat)) return PINN_E_WORKSPACE;
  const Ws w = carve(d_ws, n_clusters, n_feat);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const int K = n_clusters, D = n_feat, G = row_blocks(n, kT, kMaxBlocks);
  double* centres = d_state + km_centres();
  double* counts = d_state + km_counts(K, D);
  double* mean = d_state + km_mean(K, D);
  long long* labels = reinterpret_cast<long long*>(d_state + km_labels(K, D));
  if (init) {
    hipError_t e = hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(long long), st);        // label -1: the first pass changes every row
    if (e == hipSuccess) e = hipMemsetAsync(mean, 0, (size_t)D * sizeof(double), st);
    if (e != hipSuccess) return (int)e;
    Rows one = a;
    one.K = 1;
    hipLaunchKernelGGL(km_rows_kernel, dim3(G), dim3(kT), 0, st, one, d_state, mean, (int)LAB_ASSIGN, nullptr, 1, w.part, w.part_chg);
    hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(kFinThreads), 0, st, d_state, nullptr, nullptr, 1, D, (int)FIN_MEAN, G, n, K, tol, w.part,
                       w.part_chg, w.tot);
    hipLaunchKernelGGL(km_rows_kernel, dim3(G), dim3(kT), 0, st, one, d_state, mean, (int)LAB_ASSIGN, nullptr, 1, w.part, w.part_chg);
    hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(kFinThreads), 0, st, d_state, nullptr, nullptr, 1, D, (int)FIN_VAR, G, n, K, tol, w.part,
                       w.part_chg, w.tot);
  }
  for (int it = 0; it < n_iters; ++it) {
    hipLaunchKernelGGL(km_rows_kernel, dim3(G), dim3(kT), 0, st, a, d_state, centres, (int)LAB_WRITE, labels, 0, w.part, w.part_chg);
    hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(kFinThreads), 0, st, d_state, centres, counts, K, D, (int)FIN_LLOYD, G, n, K, tol, w.part,
                       w.part_chg, w.tot);
  }
  if (finish) {        // not strict: the assignment to the final centres; strict: the labels stay.  Inertia to the final centres.
    hipLaunchKernelGGL(km_rows_kernel, dim3(G), dim3(kT), 0, st, a, d_state, centres, (int)LAB_FINISH, labels, 1, w.part, w.part_chg);
    hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(kFinThreads), 0, st, d_state, centres, counts, K, D, (int)FIN_FINISH, G, n, K, tol, w.part,
                       w.part_chg, w.tot);
  }
  return launch_status();
}

extern "C" int pinn_cluster_means(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                  const long long* d_row_index, long long n, int n_clusters, const long long* d_labels,
                                  double* d_centres, double* d_counts, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_clusters, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_labels || !d_centres || !d_ws || misaligned8(d_labels) || misaligned8(d_centres) || misaligned8(d_counts) || misaligned8(d_ws) || n < 1)
    return PINN_E_ARG;
  if (ws_bytes < pinn_km_workspace_bytes(n, n_clusters, n_feat)) return PINN_E_WORKSPACE;
  const Ws w = carve(d_ws, n_clusters, n_feat);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const int G = row_blocks(n, kT, kMaxBlocks);
  hipLaunchKernelGGL(km_rows_kernel, dim3(G), dim3(kT), 0, st, a, nullptr, d_centres, (int)LAB_GIVEN, const_cast<long long*>(d_labels), 1, w.part,
                     w.part_chg);
  hipLaunchKernelGGL(km_final_kernel, dim3(1), dim3(kFinThreads), 0, st, nullptr, d_centres, d_counts, n_clusters, n_feat, (int)FIN_LABEL_MEANS, G, n,
                     n_clusters, 0.0, w.part, w.part_chg, w.tot);
  return launch_status();
}

extern "C" size_t pinn_ward_state_bytes(long long n_rows, int n_feat) {
  if (n_rows < 1 || n_rows > 0x7fffffffLL || n_feat < 1 || n_feat > pinn::kMaxD) return 0;
  return pinn::wd_words(n_rows, n_feat) * sizeof(double);
}

extern "C" size_t pinn_ward_workspace_bytes(long long n_rows, int n_feat) {
  if (n_rows < 1 || n_rows > 0x7fffffffLL || n_feat < 1 || n_feat > pinn::kMaxD) return 0;
  return 2 * pinn::align256(pinn::kScanBlocks * sizeof(double));
}

extern "C" int pinn_ward_tree(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                              const long long* d_row_index, long long n, int init, int n_steps, double* d_state, void* d_ws,
                              size_t ws_bytes, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, 1, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_state || !d_ws || misaligned8(d_state) || misaligned8(d_ws)) return PINN_E_ARG;
  if (n < 1 || n > 0x7fffffffLL || n_steps < 0 || n_steps > 1000000) return PINN_E_ARG;
  if (ws_bytes < pinn_ward_workspace_bytes(n, n_feat)) return PINN_E_WORKSPACE;
  double* part_d = static_cast<double*>(d_ws);
  long long* part_j = reinterpret_cast<long long*>(static_cast<char*>(d_ws) + align256(kScanBlocks * sizeof(double)));
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const int G = row_blocks(n, kScanThreads, kScanBlocks), D = n_feat;
  if (init) {
    hipLaunchKernelGGL(ward_init_kernel, dim3((unsigned)((n + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0, st, a, d_state);
    hipLaunchKernelGGL(ward_start_kernel, dim3(1), dim3(1), 0, st, d_state, n, D);
  }
  for (int s = 0; s < n_steps; ++s) {
    hipLaunchKernelGGL(ward_scan_kernel, dim3(G), dim3(kScanThreads), 0, st, d_state, n, D, part_d, part_j);
    hipLaunchKernelGGL(ward_decide_kernel, dim3(1), dim3(kScanThreads), 0, st, d_state, n, D, G, part_d, part_j);
  }
  return launch_status();
}

extern "C" int pinn_cluster_assign(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                   const long long* d_row_index, long long n, int n_clusters, const double* d_centres,
                                   const double* d_map, int n_classes, long long* d_cluster, double* d_dist2, double* d_y_prob,
                                   long long* d_y_pred, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_clusters, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_centres || misaligned8(d_centres) || misaligned8(d_map) || misaligned8(d_cluster) || misaligned8(d_dist2) || misaligned8(d_y_prob) ||
      misaligned8(d_y_pred))
    return PINN_E_ARG;
  if (d_map ? (n_classes < 1 || n_classes > kMaxC) : (d_y_prob || d_y_pred)) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  const long long tiles = (n + kT - 1) / kT;
  if (tiles > 0x7fffffffLL) return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(cluster_assign_kernel, dim3((unsigned)tiles), dim3(kT), 0, (hipStream_t)stream, a, d_centres, d_map, n_classes, d_cluster,
                     d_dist2, d_y_prob, d_y_pred);
  return launch_status();
}
