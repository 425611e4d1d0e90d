// What the two one-vs-one SVC files (pinn_svm.hip, pinn_ksvm.hip) share: pairs and their order, the limits, the prefix of the
// state block and the end of a decision: votes and the prediction from a row's pairwise values.  Integers, indices and
// comparisons only; every sum stays in its file.  The host twin is _classify.py.
#pragma once
#include <math.h>
#include "pinn_rows.h"

namespace pinn {
namespace {

static_assert(PINN_SVM_MAX_CLASSES == PINN_KSVM_MAX_CLASSES && PINN_SVM_MAX_FEAT == PINN_KSVM_MAX_FEAT, "the two SVCs share their limits");
constexpr int kOvoMaxC = PINN_SVM_MAX_CLASSES, kOvoMaxD = PINN_SVM_MAX_FEAT, kOvoMaxP = kOvoMaxC * (kOvoMaxC - 1) / 2;
__host__ __device__ inline int n_pairs(int C) { return C * (C - 1) / 2; }
__host__ __device__ constexpr int pair_index(int a, int b, int C) { return a * (2 * C - a - 1) / 2 + (b - a - 1); }      // a < b
constexpr int q8(int a, int b) { return pair_index(a, b, kOvoMaxC); }      // among the pairs of kOvoMaxC classes: a compile-time index
inline bool in_limits(int C, int D) { return C >= 2 && C <= kOvoMaxC && D >= 1 && D <= kOvoMaxD; }
__device__ __forceinline__ bool finite(double v) { return fabs(v) < INFINITY; }      // false for NaN
// both state blocks begin: header [hdr], pair blocks [P][pw], mean [D], scale [D], bound [C] (C x class weight), alpha [n][C - 1]
__host__ __device__ inline size_t st_mean(int C, int hdr, int pw) { return hdr + (size_t)n_pairs(C) * pw; }
__host__ __device__ inline size_t st_bound(int C, int D, int hdr, int pw) { return st_mean(C, hdr, pw) + 2 * D; }
__host__ __device__ inline size_t st_alpha(int C, int D, int hdr, int pw) { return st_bound(C, D, hdr, pw) + C; }

// The end of a decision of row j.  value(a, b, p) gives the value of pair p = (a, b), positive for a, from what the kernel
// holds in registers (a and b are compile-time indices there: q8).  A vote for a where the value is > 0, else for b; the
// first maximum wins; a row that reads nothing (!ok) gives NaN, no votes and -1.  Every output is optional.  The loops run to
// kOvoMaxC, so the votes stay in registers.
template <class Value>
__device__ __forceinline__ void ovo_decide(Value value, bool ok, int C, long long j, double* __restrict__ dec_out,
                                           long long* __restrict__ votes_out, long long* __restrict__ pred_out) {
  int votes[kOvoMaxC] = {};
#pragma unroll
  for (int ca = 0; ca < kOvoMaxC; ++ca)
#pragma unroll
    for (int cb = ca + 1; cb < kOvoMaxC; ++cb) {
      if (cb >= C) continue;
      const int p = pair_index(ca, cb, C);
      double x = value(ca, cb, p);
      if (!ok) x = quiet_nan();
      if (dec_out) dec_out[j * n_pairs(C) + p] = x;
      if (x > 0.0) votes[ca] += 1; else votes[cb] += 1;
    }
  int best = 0, bv = votes[0];
#pragma unroll
  for (int c = 1; c < kOvoMaxC; ++c)
    if (c < C && votes[c] > bv) { bv = votes[c]; best = c; }          // the first maximum
#pragma unroll
  for (int c = 0; c < kOvoMaxC; ++c)
    if (votes_out && c < C) votes_out[j * C + c] = ok ? votes[c] : 0;
  if (pred_out) pred_out[j] = ok ? best : -1;
}

}  // namespace
}  // namespace pinn
