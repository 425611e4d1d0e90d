// Clustering baselines of the method comparison on the device (reference script 05, cited as 05:<line>):
//   pinn_km_lloyd        Lloyd iterations with scikit-learn's stopping rule, labels / inertia / n_iter left in the state
//   pinn_ward_tree       Ward dendrogram by the nearest-neighbour chain on cluster means and sizes, O(n) memory
//   pinn_cluster_means   mean of the rows of every label
//   pinn_cluster_assign  nearest centre, and the class distribution of that cluster                    (05:384-392)
// All arithmetic is float64, every operation rounded on its own (built with -ffp-contract=off).
//
// k-means: the Lloyd state machine of pinn_lloyd.h, instantiated for rows read in place (a thread per row), 32 clusters,
// 8 features, 128 threads and at most 1024 workgroups; pinn_cluster_means is one pass of its kernels over given labels.
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
#include "pinn_lloyd.h"
#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kT = kLloydTile;              // threads per workgroup of a row pass, one per row of a tile
constexpr int kMaxK = PINN_CL_MAX_CLUSTERS, kMaxD = PINN_CL_MAX_FEAT, kMaxC = PINN_CL_MAX_CLASSES;
constexpr int kMaxBlocks = 1024;            // workgroups of a row pass = partial sums per output
constexpr int kHdr = PINN_CL_ST_HEADER;     // 8-byte words of a state header
constexpr int kScanThreads = 256, kScanBlocks = 256;

static_assert(kMaxD == kRowsMaxD && kMaxK == kRowsMaxK, "pinn_rows.h carries the same limits");

// Ward state: header, mean [n][D], size [n], chain [n], lo [n], hi [n] (64-bit integers), height [n]
__host__ __device__ inline size_t wd_mean() { return kHdr; }
__host__ __device__ inline size_t wd_size(long long n, int D) { return kHdr + (size_t)n * D; }
__host__ __device__ inline size_t wd_chain(long long n, int D) { return wd_size(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_lo(long long n, int D) { return wd_chain(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_hi(long long n, int D) { return wd_lo(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_height(long long n, int D) { return wd_hi(n, D) + (size_t)n; }
__host__ __device__ inline size_t wd_words(long long n, int D) { return wd_height(n, D) + (size_t)n; }

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
  if (ok) k = nearest<kMaxD>(x, s_mu, K, D, &d2);
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
  return lloyd_workspace_bytes(kMaxBlocks, n_clusters, n_feat);
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
  return lloyd_queue<RowsSrc, kMaxK, kMaxD, kT>(RowsSrc{a}, n, n_feat, n_clusters, kMaxBlocks, init, n_iters, tol, finish, d_state, d_ws,
                                                (hipStream_t)stream);
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
  const LloydWs w = lloyd_carve(d_ws, kMaxBlocks, n_clusters, n_feat);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const int G = row_blocks(n, kT, kMaxBlocks);
  hipLaunchKernelGGL((lloyd_rows_kernel<RowsSrc, kMaxK, kMaxD, kT>), dim3(G), dim3(kT), 0, st, RowsSrc{a}, n, n_feat, n_clusters, nullptr, d_centres,
                     (int)LAB_GIVEN, const_cast<long long*>(d_labels), 1, w.part, w.part_chg);
  hipLaunchKernelGGL((lloyd_final_kernel<kMaxK, kMaxD, kLloydFinThreads>), dim3(1), dim3(kLloydFinThreads), 0, st, nullptr, d_centres, d_counts,
                     n_clusters, n_feat, (int)FIN_LABEL_MEANS, G, n, n_clusters, 0.0, w.part, w.part_chg, w.tot);
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
