// What the analysis kernels (risk, gmm, lr, cluster, iforest, svm, tsne) share: rows of a float64 array read in place, the
// packed upper triangle, the workgroup count of a row pass and the status of a launch.  Position j reads row ridx[j]
// (NULL: row j) of a row-major array with leading dimension ld, columns col[D]; an index outside the array reads nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pinn_hip.h"

namespace pinn {
namespace {

constexpr int kRowsMaxD = PINN_GMM_MAX_FEAT, kRowsMaxK = PINN_GMM_MAX_COMP;

struct Rows {
  const double* arr;
  long long ld, n_arr, n;
  const long long* ridx;
  int D, K;
  int col[kRowsMaxD];
};

__device__ __forceinline__ bool load_row(const Rows& a, long long j, double x[kRowsMaxD]) {
  const long long row = a.ridx ? a.ridx[j] : j;
  const bool ok = row >= 0 && row < a.n_arr;               // a gather index outside the array reads nothing
  const double* r = a.arr + (ok ? row : 0) * a.ld;
#pragma unroll
  for (int i = 0; i < kRowsMaxD; ++i) x[i] = (ok && i < a.D) ? r[a.col[i]] : 0.0;
  return ok;
}

// Segments of a series (risk, hmm): ss[ns] ascending start positions, NULL or ns <= 1 for one segment.
// segment of position j: the last s with seg_start[s] <= j; segment 0 always starts at 0
__device__ __forceinline__ long long seg_of(const long long* __restrict__ ss, long long ns, long long j) {
  if (!ss || ns <= 1) return 0;
  long long lo = 0, hi = ns;
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (ss[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ long long seg_begin(const long long* __restrict__ ss, long long s) { return (ss && s > 0) ? ss[s] : 0; }

__device__ __forceinline__ long long seg_next(const long long* __restrict__ ss, long long ns, long long s, long long n) {
  return (ss && s + 1 < ns) ? ss[s + 1] : n;
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// packed upper triangle, column by column: (i, j), i <= j, sits at j (j + 1) / 2 + i
__device__ __forceinline__ int tri(int i, int j) { return j * (j + 1) / 2 + i; }

__device__ __forceinline__ void untri(int p, int* i, int* j) {
  int jj = 0;
  while ((jj + 1) * (jj + 2) / 2 <= p) ++jj;
  *j = jj;
  *i = p - jj * (jj + 1) / 2;
}

inline bool misaligned8(const void* p) { return ((unsigned long long)p & 7) != 0; }

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// workgroups of a row pass over n rows: one per tile, at least 1, at most max_blocks.  It is also the number of partial
// sums per output, so it fixes the order of every sum.
inline int row_blocks(long long n, int tile, int max_blocks) {
  const long long tiles = (n + tile - 1) / tile;
  return (int)(tiles < 1 ? 1 : (tiles > max_blocks ? max_blocks : tiles));
}

// status of an entry point's launches: clear the sticky error before the first, read it after the last
inline void clear_error() { (void)hipGetLastError(); }

inline int launch_status() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? PINN_OK : (int)e;
}

// checks shared by every entry point that reads rows; fills `a`
inline int make_rows(const double* d_arr, long long ld, long long n_arr, const int* cols, int n_feat, int n_comp,
                     const long long* d_row_index, long long n, Rows* a) {
  if (n < 0 || n_arr < 0 || ld < 1 || !cols || n_feat < 1 || n_feat > kRowsMaxD || n_comp < 1 || n_comp > kRowsMaxK) return PINN_E_ARG;
  for (int i = 0; i < n_feat; ++i)
    if (cols[i] < 0 || cols[i] >= ld) return PINN_E_ARG;
  if (!d_row_index && n > n_arr) return PINN_E_ARG;
  if (n > 0 && !d_arr) return PINN_E_ARG;
  if (misaligned8(d_arr) || misaligned8(d_row_index)) return PINN_E_ARG;
  a->arr = d_arr; a->ld = ld; a->n_arr = n_arr; a->n = n; a->ridx = d_row_index; a->D = n_feat; a->K = n_comp;
  for (int i = 0; i < kRowsMaxD; ++i) a->col[i] = i < n_feat ? cols[i] : 0;
  return PINN_OK;
}

}  // namespace
}  // namespace pinn
