// Lloyd's k-means as one state machine, for pinn_km_lloyd / pinn_cluster_means (pinn_cluster.hip: rows read in place, up to
// 8 features) and pinn_sp_lloyd (pinn_spectral.hip: packed rows of up to 32 columns).  All arithmetic is float64; both
// files are built with -ffp-contract=off.
//
// One pass is two launches.  The row pass: a workgroup takes tiles of 128 rows, a source brings a tile into LDS, one thread
// per row finds the nearest centre and writes the label into LDS; then every thread owns some of the K x (1 + 2 D) sums
// (count, sum of d, sum of d^2 with d = x - the centre the pass started from), kept in registers, and adds the tile's terms
// in row order.  Workgroup sums go to the workspace; a one-workgroup launch adds them in index order, moves the centres and
// tests scikit-learn's two stopping rules.  "The labels did not change" is a count every workgroup keeps while it
// overwrites the labels, so the test needs no host read.
//
// What fixes the bytes of a result: the tile height (rows of a tile in row order), the cap on workgroups (a workgroup's
// tiles in grid-stride order) and the index order of the workgroup partials.  Threads per workgroup and the limits do not:
// two instantiations that launch the same number of workgroups give the same bytes.  No float atomics, no workgroup waits
// on another: stream order is the only dependency.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "../../include/pinn_hip.h"
#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kLloydTile = 128;             // rows per tile of a row pass
constexpr int kLloydFinThreads = 256;

enum { LAB_ASSIGN = 0, LAB_WRITE = 1, LAB_GIVEN = 2, LAB_FINISH = 3 };
enum { FIN_MEAN = 0, FIN_VAR = 1, FIN_LLOYD = 2, FIN_FINISH = 3, FIN_LABEL_MEANS = 4 };

// k-means state: header, centres [K][D], counts [K] (doubles), mean [D], labels [n] (64-bit integers)
__host__ __device__ inline size_t km_centres() { return PINN_CL_ST_HEADER; }
__host__ __device__ inline size_t km_counts(int K, int D) { return km_centres() + (size_t)K * D; }
__host__ __device__ inline size_t km_mean(int K, int D) { return km_counts(K, D) + (size_t)K; }
__host__ __device__ inline size_t km_labels(int K, int D) { return km_mean(K, D) + (size_t)D; }
__host__ __device__ inline size_t km_words(long long n, int K, int D) { return km_labels(K, D) + (size_t)n; }

__device__ __forceinline__ bool stopped(const double* st) {
  const long long* h = reinterpret_cast<const long long*>(st);
  return h[PINN_CL_ST_CONVERGED] != 0 || h[PINN_CL_ST_STATUS] != 0;
}

// nearest of K centres [K][D] by sum (x - c)^2 added in column order, the first of equals.  A row of up to kRowsMaxD columns
// may live in registers, which want constant indices: its column loop is unrolled in full; a wider row is read where it lies.
template <int MaxD>
__device__ __forceinline__ int nearest(const double* x, const double* __restrict__ mu, int K, int D, double* d2_out) {
  int best = 0;
  double bd = INFINITY;
  for (int k = 0; k < K; ++k) {
    double d2 = 0.0;
    if constexpr (MaxD <= kRowsMaxD) {
#pragma unroll
      for (int i = 0; i < MaxD; ++i)
        if (i < D) { const double d = x[i] - mu[k * D + i]; d2 += d * d; }
    } else {
      for (int i = 0; i < D; ++i) { const double d = x[i] - mu[k * D + i]; d2 += d * d; }
    }
    if (d2 < bd) { bd = d2; best = k; }
  }
  *d2_out = bd;
  return best;
}

// ---- sources of a row pass.  stage() brings the tile that starts at row r0 (`rows` of its 128 exist) into s_x [128][D | 1],
// zeros for the rows that do not exist, and tells thread t < 128 whether row t read something.
struct RowsSrc {                            // rows read in place, a thread per row; an index outside the array reads nothing
  Rows a;
  __device__ __forceinline__ bool stage(long long r0, int rows, int D, int t, int, double* __restrict__ s_x) const {
    if (t >= kLloydTile) return false;
    double x[kRowsMaxD];
    bool ok = false;
    if (t < rows) {
      ok = load_row(a, r0 + t, x);
    } else {
#pragma unroll
      for (int i = 0; i < kRowsMaxD; ++i) x[i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < kRowsMaxD; ++i)
      if (i < D) s_x[t * (D | 1) + i] = x[i];
    return ok;
  }
};

struct PackedSrc {                          // a packed [n][D] block, copied by the whole workgroup
  const double* X;
  __device__ __forceinline__ bool stage(long long r0, int rows, int D, int t, int threads, double* __restrict__ s_x) const {
    for (int e = t; e < kLloydTile * D; e += threads) {
      const int r = e / D, c = e - r * D;
      s_x[r * (D | 1) + c] = r < rows ? X[r0 * D + e] : 0.0;
    }
    return t < rows;
  }
};

// ---- the row pass: K x F sums per workgroup, F = 1 + 2 D columns (1, d_i, d_i^2) with d = x - centre of the row's label.
// part: [gridDim.x][K * F]; part_chg: [gridDim.x] labels that differ from the stored ones (LAB_WRITE).
template <class Src, int MaxK, int MaxD, int Threads>
__global__ __launch_bounds__(Threads) void lloyd_rows_kernel(Src src, long long n, int D, int K, const double* __restrict__ st,
                                                             const double* __restrict__ centres, int mode, long long* __restrict__ labels,
                                                             int force, double* __restrict__ part, long long* __restrict__ part_chg) {
  constexpr int kR = kLloydTile, kOut = (MaxK * (1 + 2 * MaxD) + Threads - 1) / Threads;      // output sums per thread
  static_assert(Threads >= kR, "one thread per row of a tile");
  static_assert(!std::is_same<Src, RowsSrc>::value || MaxD == kRowsMaxD, "RowsSrc stages rows of up to kRowsMaxD columns");
  __shared__ double s_x[kR * (MaxD + 1)];
  __shared__ double s_mu[MaxK * MaxD];
  __shared__ int s_lab[kR];
  __shared__ long long s_chg[kR];
  if (!force && stopped(st)) return;
  const int Dp = D | 1, F = 1 + 2 * D, KF = K * F, t = threadIdx.x;
  if (mode == LAB_FINISH) mode = reinterpret_cast<const long long*>(st)[PINN_KM_ST_STRICT] != 0 ? LAB_GIVEN : LAB_WRITE;
  for (int e = t; e < K * D; e += Threads) s_mu[e] = centres[e];

  int ok_[kOut], of[kOut];
  double acc[kOut];
#pragma unroll
  for (int q = 0; q < kOut; ++q) {
    const int o = t + q * Threads;
    acc[q] = 0.0;
    ok_[q] = -1; of[q] = 0;
    if (o < KF) { ok_[q] = o / F; of[q] = o - ok_[q] * F; }
  }

  long long chg = 0;
  const long long tiles = (n + kR - 1) / kR;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long r0 = tile * kR;
    const int rows = (int)(n - r0 < (long long)kR ? n - r0 : (long long)kR);
    __syncthreads();
    const bool ok = src.stage(r0, rows, D, t, Threads, s_x);
    __syncthreads();
    if (t < kR) {
      int lab = -1;
      if (t < rows) {
        const long long j = r0 + t;
        if (mode == LAB_GIVEN) {
          const long long l = labels[j];
          lab = (ok && l >= 0 && l < K) ? (int)l : -1;
        } else {
          double d2;
          if (ok) lab = nearest<MaxD>(s_x + t * Dp, s_mu, K, D, &d2);
          if (mode == LAB_WRITE) {
            chg += labels[j] != (long long)lab;
            labels[j] = lab;
          }
        }
      }
      s_lab[t] = lab;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kOut; ++q) {
      const int k = ok_[q];
      if (k >= 0) {
        const int f = of[q];
        double s = acc[q];
        if (f == 0) {
          for (int rr = 0; rr < kR; ++rr) s += s_lab[rr] == k ? 1.0 : 0.0;
        } else if (f <= D) {
          const double m = s_mu[k * D + f - 1];
          for (int rr = 0; rr < kR; ++rr) s += s_lab[rr] == k ? s_x[rr * Dp + f - 1] - m : 0.0;
        } else {
          const double m = s_mu[k * D + f - 1 - D];
          for (int rr = 0; rr < kR; ++rr) {
            const double d = s_x[rr * Dp + f - 1 - D] - m;
            s += s_lab[rr] == k ? d * d : 0.0;
          }
        }
        acc[q] = s;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < kOut; ++q)
    if (ok_[q] >= 0) part[(size_t)blockIdx.x * KF + t + q * Threads] = acc[q];
  if (t < kR) s_chg[t] = chg;
  __syncthreads();
  if (t == 0) {
    long long s = 0;
    for (int rr = 0; rr < kR; ++rr) s += s_chg[rr];
    part_chg[blockIdx.x] = s;
  }
}

// ---- sums of the partials in index order, then what the mode asks for.  One workgroup.  K: clusters of the pass;
// tot: [K * F] totals (kept at the start of the workspace for the caller).  FIN_LABEL_MEANS takes no state; counts may be null.
template <int MaxK, int MaxD, int Threads>
__global__ __launch_bounds__(Threads) void lloyd_final_kernel(double* __restrict__ st, double* __restrict__ centres, double* __restrict__ counts,
                                                              int K, int D, int mode, int n_part, long long n, int K_state, double tol,
                                                              const double* __restrict__ part, const long long* __restrict__ part_chg,
                                                              double* __restrict__ tot) {
  __shared__ double n_mu[MaxK * MaxD], s_shift[MaxK], s_in[MaxK];
  long long* hdr = reinterpret_cast<long long*>(st);
  if (mode == FIN_LLOYD && stopped(st)) return;
  const int F = 1 + 2 * D, KF = K * F, t = threadIdx.x;
  for (int o = t; o < KF; o += Threads) {
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

// ---- workspace: totals [K F] (first, so that the caller can read the summed terms), partials of at most max_blocks
// workgroups, changed-label counts
struct LloydWs {
  double *tot, *part;
  long long* part_chg;
};

inline size_t lloyd_tot_bytes(int K, int D) { return align256((size_t)K * (1 + 2 * D) * sizeof(double)); }
inline size_t lloyd_part_bytes(int max_blocks, int K, int D) { return align256((size_t)max_blocks * K * (1 + 2 * D) * sizeof(double)); }
inline size_t lloyd_workspace_bytes(int max_blocks, int K, int D) {
  return lloyd_tot_bytes(K, D) + lloyd_part_bytes(max_blocks, K, D) + align256(max_blocks * sizeof(long long));
}

inline LloydWs lloyd_carve(void* d_ws, int max_blocks, int K, int D) {
  char* w = static_cast<char*>(d_ws);
  LloydWs s;
  s.tot = reinterpret_cast<double*>(w); w += lloyd_tot_bytes(K, D);
  s.part = reinterpret_cast<double*>(w); w += lloyd_part_bytes(max_blocks, K, D);
  s.part_chg = reinterpret_cast<long long*>(w);
  return s;
}

// ---- the queue of launches of an entry point whose arguments are checked: with init the column means and tol_abs (two
// passes over one cluster), n_iters iterations (they return at once after the state has stopped), with finish the last
// assignment (not strict: to the final centres; strict: the labels stay) and the inertia to the final centres.
template <class Src, int MaxK, int MaxD, int Threads>
int lloyd_queue(const Src& src, long long n, int D, int K, int max_blocks, int init, int n_iters, double tol, int finish, double* d_state,
                void* d_ws, hipStream_t st) {
  const LloydWs w = lloyd_carve(d_ws, max_blocks, K, D);
  clear_error();
  const int G = row_blocks(n, kLloydTile, max_blocks);
  double* centres = d_state + km_centres();
  double* counts = d_state + km_counts(K, D);
  double* mean = d_state + km_mean(K, D);
  long long* labels = reinterpret_cast<long long*>(d_state + km_labels(K, D));
  auto pass = [&](int K_pass, double* from, int lab_mode, long long* lab, int force, double* to, double* cnt, int fin_mode) {
    hipLaunchKernelGGL((lloyd_rows_kernel<Src, MaxK, MaxD, Threads>), dim3(G), dim3(Threads), 0, st, src, n, D, K_pass, d_state, from, lab_mode, lab,
                       force, w.part, w.part_chg);
    hipLaunchKernelGGL((lloyd_final_kernel<MaxK, MaxD, kLloydFinThreads>), dim3(1), dim3(kLloydFinThreads), 0, st, d_state, to, cnt, K_pass, D,
                       fin_mode, G, n, K, tol, w.part, w.part_chg, w.tot);
  };
  if (init) {
    hipError_t e = hipMemsetAsync(labels, 0xff, (size_t)n * sizeof(long long), st);        // label -1: the first pass changes every row
    if (e == hipSuccess) e = hipMemsetAsync(mean, 0, (size_t)D * sizeof(double), st);
    if (e != hipSuccess) return (int)e;
    pass(1, mean, LAB_ASSIGN, nullptr, 1, nullptr, nullptr, FIN_MEAN);
    pass(1, mean, LAB_ASSIGN, nullptr, 1, nullptr, nullptr, FIN_VAR);
  }
  for (int it = 0; it < n_iters; ++it) pass(K, centres, LAB_WRITE, labels, 0, centres, counts, FIN_LLOYD);
  if (finish) pass(K, centres, LAB_FINISH, labels, 1, centres, counts, FIN_FINISH);
  return launch_status();
}

}  // namespace
}  // namespace pinn
