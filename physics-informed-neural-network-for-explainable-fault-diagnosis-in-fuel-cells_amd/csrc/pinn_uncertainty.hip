// Calibration of the voltage network's uncertainty columns and conformal bands on the device (no reference script: the
// definitions are the header's, include/pinn_hip.h):
//   pinn_unc_score      one row pass: per-group sums of 1, r, r^2, s, s^2, z, z^2, nll, crps, coverage hits and the PIT histogram
//   pinn_unc_quantiles  exact order statistics of a score per group: a radix select over keys computed on the fly
//   pinn_unc_update     the online band: one launch of one workgroup per chunk, the state header and score ring on the device
// Predictive law: y ~ N(y_pred, v), v = a ale^2 + b epi^2 + c, s = sqrt(v), r = y_true - y_pred, z = r / s.  All arithmetic is
// float64 and separately rounded (built with -ffp-contract=off); z, |z| and every comparison use +, *, sqrt, / and <= only, so
// everything counted from z is the host backend's to the bit.  log, erfc and exp enter the nll / crps terms alone.
//
// No workgroup waits on another: partial sums and histograms meet in one-workgroup launches that follow in stream order.
// Integer counts use integer atomics (LDS, and global for the select's histograms): their result does not depend on the
// order.  Float sums have a fixed order: lanes by a shuffle tree, steps of a wave in row order, waves and workgroups in
// index order.  The same call gives the same bytes.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kThreads = 256;
constexpr int kTile = PINN_UNC_TILE;            // rows of a workgroup's step through the array
constexpr int kItems = kTile / kThreads;
constexpr int kMaxBlocks = PINN_UNC_MAX_BLOCKS;
constexpr int kSums = PINN_UNC_SUMS;
constexpr int kCnt = 1 + PINN_UNC_MAX_LEVELS + PINN_UNC_MAX_BINS;      // per group: n, hits[16], pit[64]
constexpr int kCntAll = PINN_UNC_MAX_GROUPS * kCnt + 1;                // and the skipped rows of the call
constexpr int kMaxTargets = PINN_UNC_MAX_TARGETS;
constexpr int kDigits = 256, kPasses = 8;       // the select reads the 64-bit key a byte at a time, the top byte first
constexpr int kCollect = PINN_UNC_COLLECT;      // a target whose prefix at most this many keys carry stops counting and gathers them

// words of the select's device header; the histograms [targets][256] and the gathered keys [targets][kCollect] follow it
constexpr int kHdrPrefix = 0, kHdrRank = 64, kHdrState = 128, kHdrSlot = 192, kHdrN = 256, kHdrCount = 320, kHdrWords = 384;
// a target counts bytes (live), is finished (done), or gathers the keys that carry its prefix in the next pass (gather)
constexpr unsigned long long kLive = 0ull, kDone = 1ull, kGather = 2ull;

constexpr double kLog2Pi = 1.8378770664093453, kInvSqrt2 = 0.7071067811865476, kInvSqrt2Pi = 0.3989422804014327,
                 kInvSqrtPi = 0.5641895835477563;

struct UncDev {
  const double* arr;
  long long ld, n_arr, n;
  const long long* ridx;
  int c_true, c_pred, c_ale, c_epi, c_label, n_labels, kind, c_score;       // c_label < 0: one group, no label read
  double a, b, c;
  signed char table[PINN_UNC_MAX_LABELS];
};

struct ScoreArgs {
  int L, B;
  double z_level[PINN_UNC_MAX_LEVELS];
  double z_edge[PINN_UNC_MAX_BINS];
};

struct Levels {
  double level[PINN_UNC_MAX_QUANTILES];
};

struct RowVal {
  bool valid;
  int g;
  double yp, r, s, v, z;
};

__device__ __forceinline__ bool finite_word(double x) { return fabs(x) <= 1.7976931348623157e308; }     // false for NaN and +-inf

// the row behind position j, or nullptr when the gather index lies outside the array
__device__ __forceinline__ const double* row_of(const UncDev& a, long long j) {
  const long long row = a.ridx ? a.ridx[j] : j;
  return (row >= 0 && row < a.n_arr) ? a.arr + row * a.ld : nullptr;
}

// group of a row: the label is used when 0 <= label < n_labels (a NaN fails both), truncated, and looked up
__device__ __forceinline__ int group_of(const UncDev& a, const signed char* table, const double* r) {
  if (a.c_label < 0) return 0;
  const double lab = r[a.c_label];
  if (!(lab >= 0.0 && lab < (double)a.n_labels)) return -1;
  return table[(int)lab];
}

__device__ __forceinline__ RowVal read_row(const UncDev& a, const signed char* table, long long j) {
  RowVal o;
  o.valid = false; o.g = -1;
  o.yp = o.r = o.s = o.v = o.z = quiet_nan();
  const double* r = row_of(a, j);
  if (!r) return o;
  const int g = group_of(a, table, r);
  if (g < 0) return o;
  const double yt = r[a.c_true], yp = r[a.c_pred], ale = r[a.c_ale], epi = r[a.c_epi];
  const double v = (a.a * ale) * ale + (a.b * epi) * epi + a.c;
  if (!finite_word(yt) || !finite_word(yp) || !finite_word(v) || !(v > 0.0)) return o;
  o.valid = true; o.g = g; o.yp = yp; o.v = v;
  o.s = sqrt(v);
  o.r = yt - yp;
  o.z = o.r / o.s;
  return o;
}

// the usual monotone map from a double to 64 bits that order as unsigned integers; -0 is +0
__device__ __forceinline__ unsigned long long key_of(double x) {
  unsigned long long b = (unsigned long long)__double_as_longlong(x);
  if (x == 0.0) b = 0ull;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// the score of position j and its group; false when the row is not valid for this kind
__device__ __forceinline__ bool score_of(const UncDev& a, const signed char* table, long long j, int* g, double* score) {
  if (a.kind == PINN_UNC_COLUMN) {
    const double* r = row_of(a, j);
    if (!r) return false;
    const int gg = group_of(a, table, r);
    const double x = r[a.c_score];
    if (gg < 0 || !finite_word(x)) return false;
    *g = gg; *score = x;
    return true;
  }
  const RowVal o = read_row(a, table, j);
  if (!o.valid) return false;
  *g = o.g;
  *score = a.kind == PINN_UNC_ABS_Z ? fabs(o.z) : o.z;
  return true;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

__device__ __forceinline__ void load_table(const UncDev& a, signed char* s_table) {
  for (int i = threadIdx.x; i < PINN_UNC_MAX_LABELS; i += kThreads) s_table[i] = a.table[i];
}

// ---- scoring: workgroup b takes the tiles b, b + blocks, ...; a wave adds its 64 rows of a step group by group
__global__ __launch_bounds__(kThreads) void unc_score_kernel(UncDev a, ScoreArgs p, int G, double* __restrict__ part_sum,
                                                              unsigned long long* __restrict__ part_cnt, double* __restrict__ z_out,
                                                              double* __restrict__ phi_out, double* __restrict__ crps_out,
                                                              double* __restrict__ nll_out) {
  __shared__ unsigned long long s_cnt[kCntAll];
  __shared__ double s_sum[kThreads / 64][PINN_UNC_MAX_GROUPS][kSums];
  __shared__ double s_level[PINN_UNC_MAX_LEVELS], s_edge[PINN_UNC_MAX_BINS];
  __shared__ signed char s_table[PINN_UNC_MAX_LABELS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < kCntAll; i += kThreads) s_cnt[i] = 0ull;
  for (int i = threadIdx.x; i < (kThreads / 64) * PINN_UNC_MAX_GROUPS * kSums; i += kThreads) (&s_sum[0][0][0])[i] = 0.0;
  if (threadIdx.x < PINN_UNC_MAX_LEVELS) s_level[threadIdx.x] = p.z_level[threadIdx.x];
  if (threadIdx.x < PINN_UNC_MAX_BINS) s_edge[threadIdx.x] = p.z_edge[threadIdx.x];
  load_table(a, s_table);
  __syncthreads();

  const long long tiles = (a.n + kTile - 1) / kTile;
  unsigned long long skipped = 0;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    for (int k = 0; k < kItems; ++k) {
      const long long j = tile * kTile + (long long)k * kThreads + threadIdx.x;
      const bool in = j < a.n;
      RowVal o;
      o.valid = false; o.g = -1;
      o.yp = o.r = o.s = o.v = o.z = 0.0;
      double t[kSums];
      double phi = quiet_nan(), crps = quiet_nan(), nll = quiet_nan(), z = quiet_nan();
      if (in) {
        o = read_row(a, s_table, j);
        if (o.valid) {
          z = o.z;
          const double zz = z * z;
          phi = 0.5 * erfc(-z * kInvSqrt2);
          const double pdf = exp(-0.5 * zz) * kInvSqrt2Pi;
          nll = 0.5 * (kLog2Pi + log(o.v) + zz);
          crps = o.s * (z * (2.0 * phi - 1.0) + 2.0 * pdf - kInvSqrtPi);
          int bin = 0;
          for (int e = 0; e + 1 < p.B; ++e) bin += s_edge[e] <= z ? 1 : 0;
          atomicAdd(&s_cnt[o.g * kCnt + 1 + PINN_UNC_MAX_LEVELS + bin], 1ull);
        } else {
          ++skipped;
        }
        if (z_out) z_out[j] = z;
        if (phi_out) phi_out[j] = phi;
        if (crps_out) crps_out[j] = crps;
        if (nll_out) nll_out[j] = nll;
      }
      t[0] = 1.0; t[1] = o.r; t[2] = o.r * o.r; t[3] = o.s; t[4] = o.v; t[5] = z; t[6] = z * z; t[7] = nll; t[8] = crps;
      const double az = fabs(z);
      for (int g = 0; g < G; ++g) {
        const bool mine = o.valid && o.g == g;
        const unsigned long long m = __ballot(mine);
        if (!m) continue;                                     // the same for every lane of the wave
#pragma unroll
        for (int i = 0; i < kSums; ++i) {
          const double v = wave_sum(mine ? t[i] : 0.0);
          if (lane == 0) s_sum[wave][g][i] += v;
        }
        if (lane == 0) atomicAdd(&s_cnt[g * kCnt], (unsigned long long)__popcll(m));
        for (int l = 0; l < p.L; ++l) {
          const unsigned long long h = __ballot(mine && az <= s_level[l]);
          if (lane == 0 && h) atomicAdd(&s_cnt[g * kCnt + 1 + l], (unsigned long long)__popcll(h));
        }
      }
    }
  }
  if (skipped) atomicAdd(&s_cnt[kCntAll - 1], skipped);
  __syncthreads();
  if (threadIdx.x < G * kSums) {
    const int g = threadIdx.x / kSums, i = threadIdx.x - g * kSums;
    double v = s_sum[0][g][i];
    for (int w = 1; w < kThreads / 64; ++w) v += s_sum[w][g][i];
    part_sum[(long long)blockIdx.x * (PINN_UNC_MAX_GROUPS * kSums) + threadIdx.x] = v;
  }
  for (int i = threadIdx.x; i < kCntAll; i += kThreads) part_cnt[(long long)blockIdx.x * kCntAll + i] = s_cnt[i];
}

// the partials of every workgroup in index order
__global__ __launch_bounds__(kThreads) void unc_score_final_kernel(int G, int L, int B, int n_part, const double* __restrict__ part_sum,
                                                                    const unsigned long long* __restrict__ part_cnt,
                                                                    double* __restrict__ sums, long long* __restrict__ n_out,
                                                                    long long* __restrict__ hits, long long* __restrict__ pit,
                                                                    long long* __restrict__ skipped) {
  if (threadIdx.x < G * kSums) {
    double v = part_sum[threadIdx.x];
    for (int b = 1; b < n_part; ++b) v += part_sum[(long long)b * (PINN_UNC_MAX_GROUPS * kSums) + threadIdx.x];
    sums[threadIdx.x] = v;
  }
  for (int i = threadIdx.x; i < kCntAll; i += kThreads) {
    const int g = i / kCnt, w = i - g * kCnt;
    const bool last = i == kCntAll - 1;
    if (!last && (g >= G || (w >= 1 && w < 1 + PINN_UNC_MAX_LEVELS && w - 1 >= L) || (w >= 1 + PINN_UNC_MAX_LEVELS && w - 1 - PINN_UNC_MAX_LEVELS >= B)))
      continue;
    unsigned long long c = 0;
    for (int b = 0; b < n_part; ++b) c += part_cnt[(long long)b * kCntAll + i];
    if (last) skipped[0] = (long long)c;
    else if (w == 0) n_out[g] = (long long)c;
    else if (w < 1 + PINN_UNC_MAX_LEVELS) hits[g * L + (w - 1)] = (long long)c;
    else pit[g * B + (w - 1 - PINN_UNC_MAX_LEVELS)] = (long long)c;
  }
}

// ---- select: header and histograms start at zero, every target's histogram slot is its group's first target
__global__ __launch_bounds__(kThreads) void unc_select_init_kernel(int Q, int T, unsigned long long* __restrict__ hdr) {
  const int total = kHdrWords + T * kDigits;                  // the key lists need no start value: a count says how much of one is written
  for (int i = threadIdx.x; i < total; i += kThreads) {
    unsigned long long v = 0ull;
    if (i >= kHdrSlot && i < kHdrSlot + T) v = (unsigned long long)(((i - kHdrSlot) / Q) * Q);
    hdr[i] = v;
  }
}

// one digit pass: a valid row whose key carries a live target's prefix counts its next byte in that target's histogram; one
// that carries a gathering target's prefix appends its key to the target's list (at most kCollect keys carry it, counted in
// the pass before; their order in the list is arbitrary and the finish does not depend on it).  Targets that still share
// group and prefix share one histogram or list (the lowest of them leads), so a row adds once for them.
__global__ __launch_bounds__(kThreads) void unc_select_kernel(UncDev a, int Q, int T, int pass, unsigned long long* __restrict__ hdr,
                                                               unsigned long long* __restrict__ ghist) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned int* s_hist = reinterpret_cast<unsigned int*>(smem);
  __shared__ unsigned long long s_prefix[kMaxTargets];
  __shared__ int s_live[kMaxTargets];
  __shared__ int s_any;
  __shared__ signed char s_table[PINN_UNC_MAX_LABELS];
  if (threadIdx.x == 0) s_any = 0;
  __syncthreads();
  if (threadIdx.x < kMaxTargets) {
    const int t = threadIdx.x;
    const unsigned long long state = t < T ? hdr[kHdrState + t] : kDone;
    const bool leads = t < T && state != kDone && hdr[kHdrSlot + t] == (unsigned long long)t;
    s_prefix[t] = t < T ? hdr[kHdrPrefix + t] : 0ull;
    s_live[t] = !leads ? 0 : (state == kLive ? 1 : 2);
    if (leads) s_any = 1;
  }
  load_table(a, s_table);
  for (int i = threadIdx.x; i < T * kDigits; i += kThreads) s_hist[i] = 0u;
  __syncthreads();
  if (!s_any) return;                                         // the same for every thread of every workgroup

  const int shift = 56 - 8 * pass;
  const long long tiles = (a.n + kTile - 1) / kTile;
  unsigned long long* keys = ghist + (long long)T * kDigits;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll 2
    for (int k = 0; k < kItems; ++k) {
      const long long j = tile * kTile + (long long)k * kThreads + threadIdx.x;
      if (j >= a.n) break;
      int g;
      double score;
      if (!score_of(a, s_table, j, &g, &score)) continue;
      const unsigned long long key = key_of(score);
      const unsigned long long head = pass == 0 ? 0ull : key >> (shift + 8);
      const unsigned int digit = (unsigned int)(key >> shift) & 255u;
      for (int q = 0; q < Q; ++q) {
        const int t = g * Q + q;
        if (!s_live[t] || head != s_prefix[t]) continue;
        if (s_live[t] == 1) {
          atomicAdd(&s_hist[t * kDigits + digit], 1u);
        } else {
          const unsigned long long at = atomicAdd(&hdr[kHdrCount + t], 1ull);
          if (at < (unsigned long long)kCollect) keys[(long long)t * kCollect + at] = key;
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < T * kDigits; i += kThreads) {
    const unsigned int c = s_hist[i];
    if (c) atomicAdd(&ghist[i], (unsigned long long)c);
  }
}

// after a pass, before the narrowing: workgroup t finishes target t when its keys were gathered in this pass.  The k-th smallest
// of c keys is the one with fewer than k keys below it and at least k keys at or below it: counted, not sorted, so ties and
// the arbitrary order of the list do not matter.
__global__ __launch_bounds__(kThreads) void unc_gather_finish_kernel(int T, const unsigned long long* __restrict__ hdr,
                                                                      const unsigned long long* __restrict__ ghist, double* __restrict__ q_out) {
  __shared__ unsigned long long s_keys[kCollect];
  const int t = blockIdx.x;
  if (hdr[kHdrState + t] != kGather) return;                  // the same for every thread of the workgroup
  const unsigned long long slot = hdr[kHdrSlot + t], rem = hdr[kHdrRank + t];
  unsigned long long c = hdr[kHdrCount + slot];
  c = c > (unsigned long long)kCollect ? (unsigned long long)kCollect : c;
  const unsigned long long* keys = ghist + (long long)T * kDigits + (long long)slot * kCollect;
  for (int i = threadIdx.x; i < (int)c; i += kThreads) s_keys[i] = keys[i];
  __syncthreads();
  for (int i = threadIdx.x; i < (int)c; i += kThreads) {
    const unsigned long long mine = s_keys[i];
    unsigned long long below = 0, upto = 0;
    for (int j = 0; j < (int)c; ++j) {
      const unsigned long long other = s_keys[j];
      below += other < mine ? 1ull : 0ull;
      upto += other <= mine ? 1ull : 0ull;
    }
    if (below < rem && rem <= upto) q_out[t] = unkey(mine);   // every thread that gets here writes the same value
  }
}

// after a pass: every live target takes the byte that holds its remaining rank, and the histograms return to zero.  After the
// first pass the group sizes are known (the histogram of a group's first target holds every valid row of the group), and with
// them the ranks.
__global__ __launch_bounds__(kThreads) void unc_narrow_kernel(int G, int Q, int pass, int conformal, Levels lv, long long n,
                                                               unsigned long long* __restrict__ hdr, unsigned long long* __restrict__ ghist,
                                                               double* __restrict__ q_out, long long* __restrict__ rank_out,
                                                               long long* __restrict__ n_out, long long* __restrict__ skipped_out) {
  __shared__ unsigned long long s_prefix[kMaxTargets];
  __shared__ int s_state[kMaxTargets];
  __shared__ long long s_n[PINN_UNC_MAX_GROUPS];
  const int T = G * Q, t = threadIdx.x;
  if (pass == 0) {
    if (t < G) {
      const unsigned long long* h = ghist + (long long)(t * Q) * kDigits;
      unsigned long long c = 0;
      for (int b = 0; b < kDigits; ++b) c += h[b];
      s_n[t] = (long long)c;
      hdr[kHdrN + t] = c;
      n_out[t] = (long long)c;
    }
    __syncthreads();
    if (t == 0) {
      long long used = 0;
      for (int g = 0; g < G; ++g) used += s_n[g];
      skipped_out[0] = n - used;
    }
    if (t < T) {
      const long long ng = s_n[t / Q];
      const double level = lv.level[t % Q];
      long long k = 0;
      unsigned long long state = 0ull;
      if (ng == 0) {
        q_out[t] = quiet_nan();
        state = 1ull;
      } else {
        if (conformal) {
          k = (long long)ceil((double)(ng + 1) * level);
        } else {
          k = (long long)ceil((double)ng * level);
          k = k < 1 ? 1 : (k > ng ? ng : k);
        }
        if (k > ng) {
          q_out[t] = __longlong_as_double(0x7ff0000000000000LL);
          state = 1ull;
        }
      }
      rank_out[t] = k;
      hdr[kHdrRank + t] = (unsigned long long)k;
      hdr[kHdrState + t] = state;
    }
    __syncthreads();
  }
  if (t < T) {
    unsigned long long prefix = hdr[kHdrPrefix + t];
    int state = (int)hdr[kHdrState + t];
    if (state == (int)kGather) {                              // gathered in this pass and finished by the launch before this one
      state = (int)kDone;
      hdr[kHdrState + t] = kDone;
    } else if (state == (int)kLive) {
      const unsigned long long* h = ghist + (long long)hdr[kHdrSlot + t] * kDigits;
      const unsigned long long rem = hdr[kHdrRank + t];
      unsigned long long before = 0;
      int b = 0;
      for (; b < kDigits - 1; ++b) {
        const unsigned long long c = h[b];
        if (before + c >= rem) break;
        before += c;
      }
      prefix = (prefix << 8) | (unsigned long long)b;
      hdr[kHdrPrefix + t] = prefix;
      hdr[kHdrRank + t] = rem - before;
      if (pass == kPasses - 1) {
        q_out[t] = unkey(prefix);
      } else if (h[b] <= (unsigned long long)kCollect) {      // few keys carry the new prefix: the next pass gathers them
        state = (int)kGather;
        hdr[kHdrState + t] = kGather;
      }
    }
    s_prefix[t] = prefix;
    s_state[t] = state;
  }
  __syncthreads();                                            // every read of the histograms is done
  for (int i = threadIdx.x; i < T * kDigits; i += kThreads) ghist[i] = 0ull;
  if (t < T) {
    hdr[kHdrCount + t] = 0ull;
    int slot = t;                                             // equal prefixes had equal bin counts, so they are in the same state
    for (int u = (t / Q) * Q; u < t; ++u)
      if (s_state[u] != (int)kDone && s_state[u] == s_state[t] && s_prefix[u] == s_prefix[t]) { slot = u; break; }
    hdr[kHdrSlot + t] = (unsigned long long)slot;
  }
}

// ---- the online band: one workgroup, thread t owns the rows t * 8 .. t * 8 + 7 of the chunk
struct UpdateArgs {
  double level, gamma, alpha_min, alpha_max;
  int window, learn;
};

constexpr int kStFill = 0, kStPos = 1, kStAlpha = 2, kStQ = 3, kStValid = 4, kStMiss = 5;

__global__ __launch_bounds__(kThreads) void unc_update_kernel(UncDev a, UpdateArgs u, unsigned long long* __restrict__ state,
                                                               double* __restrict__ lo_out, double* __restrict__ hi_out,
                                                               double* __restrict__ z_out, int* __restrict__ flag_out) {
  __shared__ unsigned long long s_ring[PINN_UNC_MAX_WINDOW];
  __shared__ int s_scan[kThreads], s_miss[kThreads];
  const int W = u.window, n = (int)a.n;
  const long long fill = (long long)state[kStFill], pos = (long long)state[kStPos];
  const double alpha = __longlong_as_double((long long)state[kStAlpha]), q = __longlong_as_double((long long)state[kStQ]);
  const long long n_valid = (long long)state[kStValid], n_miss = (long long)state[kStMiss];
  unsigned long long* ring = state + PINN_UNC_STATE_HEADER;
  if (u.learn)
    for (int i = threadIdx.x; i < W; i += kThreads) s_ring[i] = ring[i];

  double score[kItems];
  bool ok[kItems];
  int cnt = 0, miss = 0;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int j = (int)threadIdx.x * kItems + k;
    ok[k] = false;
    score[k] = 0.0;
    if (j < n) {
      const RowVal o = read_row(a, a.table, j);
      double lo = quiet_nan(), hi = quiet_nan();
      int flag = -1;
      if (o.valid) {
        const double az = fabs(o.z), half = q * o.s;
        lo = o.yp - half;
        hi = o.yp + half;
        flag = az <= q ? 0 : 1;
        ok[k] = true;
        score[k] = az;
        ++cnt;
        miss += flag;
      }
      if (lo_out) lo_out[j] = lo;
      if (hi_out) hi_out[j] = hi;
      if (z_out) z_out[j] = o.z;
      if (flag_out) flag_out[j] = flag;
    }
  }
  if (!u.learn) return;                                       // the state bytes stay as they are

  // inclusive scans of the valid and miss counts in thread order
  s_scan[threadIdx.x] = cnt;
  s_miss[threadIdx.x] = miss;
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    const int c = threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0, m = threadIdx.x >= d ? s_miss[threadIdx.x - d] : 0;
    __syncthreads();
    s_scan[threadIdx.x] += c;
    s_miss[threadIdx.x] += m;
    __syncthreads();
  }
  const int nv = s_scan[kThreads - 1], nm = s_miss[kThreads - 1];
  int e = s_scan[threadIdx.x] - cnt;                           // valid rows before this thread's
  // the valid scores enter the ring in row order; of more than W only the last W arrive, each at a place of its own
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    if (ok[k]) {
      if (e >= nv - W) s_ring[(pos + e) % W] = (unsigned long long)__double_as_longlong(score[k]);
      ++e;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < W; i += kThreads) ring[i] = s_ring[i];
  const long long m = fill + nv < W ? fill + nv : W;
  double alpha1 = alpha;
  if (nv > 0) {
    alpha1 = alpha + u.gamma * ((1.0 - u.level) - (double)nm / (double)nv);
    alpha1 = alpha1 < u.alpha_min ? u.alpha_min : alpha1;
    alpha1 = alpha1 > u.alpha_max ? u.alpha_max : alpha1;
  }
  long long kth = (long long)ceil((double)(m + 1) * (1.0 - alpha1));
  kth = kth < 1 ? 1 : kth;

  // sort the m scores: non-negative doubles order as their bits; the padding is above every score
  int npad = 2;
  while (npad < m) npad <<= 1;
  __syncthreads();                                            // the ring image is written out
  for (int i = (int)m + threadIdx.x; i < npad; i += kThreads) s_ring[i] = ~0ull;
  __syncthreads();
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (npad >> 1); t += kThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long xa = s_ring[i], xb = s_ring[l];
        if ((xa > xb) == ((i & k) == 0)) { s_ring[i] = xb; s_ring[l] = xa; }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const double q1 = kth > m ? __longlong_as_double(0x7ff0000000000000LL) : __longlong_as_double((long long)s_ring[kth - 1]);
    state[kStFill] = (unsigned long long)m;
    state[kStPos] = (unsigned long long)((pos + nv) % W);
    state[kStAlpha] = (unsigned long long)__double_as_longlong(alpha1);
    state[kStQ] = (unsigned long long)__double_as_longlong(q1);
    state[kStValid] = (unsigned long long)(n_valid + nv);
    state[kStMiss] = (unsigned long long)(n_miss + nm);
  }
}

inline bool finite_host(double x) { return x - x == 0.0; }

// checks shared by the three entry points; fills `a`.  cols = (y_true, y_pred, ale, epi).
inline int make_unc(const double* d_arr, long long ld, long long n_arr, const int* cols, int n_cols, const long long* d_row_index,
                    long long n, int label_col, const int* label_table, int n_labels, int n_groups, const double* var_model,
                    UncDev* a) {
  Rows r;
  if (n_cols != 4) return PINN_E_ARG;
  const int rc = make_rows(d_arr, ld, n_arr, cols, 4, 1, d_row_index, n, &r);
  if (rc != PINN_OK) return rc;
  if (!var_model || n_groups < 1 || n_groups > PINN_UNC_MAX_GROUPS) return PINN_E_ARG;
  for (int i = 0; i < 3; ++i)
    if (!finite_host(var_model[i]) || var_model[i] < 0.0) return PINN_E_ARG;
  a->arr = r.arr; a->ld = r.ld; a->n_arr = r.n_arr; a->n = r.n; a->ridx = r.ridx;
  a->c_true = cols[0]; a->c_pred = cols[1]; a->c_ale = cols[2]; a->c_epi = cols[3];
  a->a = var_model[0]; a->b = var_model[1]; a->c = var_model[2];
  a->kind = PINN_UNC_ABS_Z; a->c_score = 0;
  for (int i = 0; i < PINN_UNC_MAX_LABELS; ++i) a->table[i] = -1;
  if (label_col < 0) {                                        // one group: no label is read
    if (label_col != -1 || n_groups != 1) return PINN_E_ARG;
    a->c_label = -1; a->n_labels = 0;
    return PINN_OK;
  }
  if (label_col >= ld || !label_table || n_labels < 1 || n_labels > PINN_UNC_MAX_LABELS) return PINN_E_ARG;
  for (int i = 0; i < n_labels; ++i) {
    if (label_table[i] < -1 || label_table[i] >= n_groups) return PINN_E_ARG;
    a->table[i] = (signed char)label_table[i];
  }
  a->c_label = label_col; a->n_labels = n_labels;
  return PINN_OK;
}

inline size_t score_ws_bytes(long long n) {
  const size_t blocks = (size_t)row_blocks(n, kTile, kMaxBlocks);
  return align256(blocks * PINN_UNC_MAX_GROUPS * kSums * sizeof(double)) + align256(blocks * kCntAll * sizeof(unsigned long long));
}

inline size_t select_ws_bytes(int targets) {
  return align256(((size_t)kHdrWords + (size_t)targets * (kDigits + kCollect)) * sizeof(unsigned long long));
}

}  // namespace
}  // namespace pinn

using namespace pinn;

extern "C" size_t pinn_unc_workspace_bytes(long long n, int n_groups, int n_quantiles) {
  if (n < 0 || n_groups < 1 || n_groups > PINN_UNC_MAX_GROUPS || n_quantiles < 1 || n_quantiles > PINN_UNC_MAX_QUANTILES ||
      n_groups * n_quantiles > PINN_UNC_MAX_TARGETS)
    return 0;
  const size_t s = score_ws_bytes(n), q = select_ws_bytes(n_groups * n_quantiles);
  return s > q ? s : q;
}

extern "C" int pinn_unc_score(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_cols,
                              const long long* d_row_index, long long n, int label_col, const int* label_table, int n_labels,
                              int n_groups, const double* var_model, const double* z_level, int n_levels, const double* z_edge,
                              int n_bins, double* d_sums, long long* d_n, long long* d_hits, long long* d_pit, long long* d_n_skipped,
                              double* d_z, double* d_phi, double* d_crps, double* d_nll, void* d_ws, size_t ws_bytes, void* stream) {
  UncDev a;
  const int rc = make_unc(d_arr, ld, n_arr_rows, cols, n_cols, d_row_index, n, label_col, label_table, n_labels, n_groups, var_model, &a);
  if (rc != PINN_OK) return rc;
  if (n_levels < 1 || n_levels > PINN_UNC_MAX_LEVELS || n_bins < 1 || n_bins > PINN_UNC_MAX_BINS || !z_level || (n_bins > 1 && !z_edge))
    return PINN_E_ARG;
  ScoreArgs p;
  p.L = n_levels; p.B = n_bins;
  for (int i = 0; i < PINN_UNC_MAX_LEVELS; ++i) {
    p.z_level[i] = i < n_levels ? z_level[i] : 0.0;
    if (i < n_levels && !(z_level[i] >= 0.0)) return PINN_E_ARG;
  }
  for (int i = 0; i < PINN_UNC_MAX_BINS; ++i) {
    p.z_edge[i] = i < n_bins - 1 ? z_edge[i] : 0.0;
    if (i < n_bins - 1 && (z_edge[i] != z_edge[i] || (i > 0 && !(z_edge[i] > z_edge[i - 1])))) return PINN_E_ARG;
  }
  if (!d_sums || !d_n || !d_hits || !d_pit || !d_n_skipped) return PINN_E_ARG;
  if (misaligned8(d_sums) || misaligned8(d_n) || misaligned8(d_hits) || misaligned8(d_pit) || misaligned8(d_n_skipped) || misaligned8(d_z) ||
      misaligned8(d_phi) || misaligned8(d_crps) || misaligned8(d_nll) || misaligned8(d_ws))
    return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  if (!d_ws) return PINN_E_ARG;
  if (ws_bytes < pinn_unc_workspace_bytes(n, n_groups, 1)) return PINN_E_WORKSPACE;
  const int blocks = row_blocks(n, kTile, kMaxBlocks);
  double* part_sum = static_cast<double*>(d_ws);
  unsigned long long* part_cnt = reinterpret_cast<unsigned long long*>(
      static_cast<char*>(d_ws) + align256((size_t)blocks * PINN_UNC_MAX_GROUPS * kSums * sizeof(double)));
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  hipLaunchKernelGGL(unc_score_kernel, dim3(blocks), dim3(kThreads), 0, st, a, p, n_groups, part_sum, part_cnt, d_z, d_phi, d_crps, d_nll);
  hipLaunchKernelGGL(unc_score_final_kernel, dim3(1), dim3(kThreads), 0, st, n_groups, n_levels, n_bins, blocks, part_sum, part_cnt, d_sums,
                     d_n, d_hits, d_pit, d_n_skipped);
  return launch_status();
}

extern "C" int pinn_unc_quantiles(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_cols,
                                  const long long* d_row_index, long long n, int label_col, const int* label_table, int n_labels,
                                  int n_groups, const double* var_model, int kind, int score_col, const double* levels, int n_quantiles,
                                  int conformal, double* d_q, long long* d_rank, long long* d_n, long long* d_n_skipped, void* d_ws,
                                  size_t ws_bytes, void* stream) {
  UncDev a;
  const int rc = make_unc(d_arr, ld, n_arr_rows, cols, n_cols, d_row_index, n, label_col, label_table, n_labels, n_groups, var_model, &a);
  if (rc != PINN_OK) return rc;
  if (kind != PINN_UNC_ABS_Z && kind != PINN_UNC_Z && kind != PINN_UNC_COLUMN) return PINN_E_ARG;
  if (kind == PINN_UNC_COLUMN && (score_col < 0 || score_col >= ld)) return PINN_E_ARG;
  if (!levels || n_quantiles < 1 || n_quantiles > PINN_UNC_MAX_QUANTILES || n_groups * n_quantiles > PINN_UNC_MAX_TARGETS) return PINN_E_ARG;
  Levels lv;
  for (int i = 0; i < PINN_UNC_MAX_QUANTILES; ++i) {
    lv.level[i] = i < n_quantiles ? levels[i] : 0.5;
    if (i < n_quantiles && !(levels[i] > 0.0 && levels[i] <= 1.0)) return PINN_E_ARG;
  }
  if (n > (1LL << 40)) return PINN_E_ARG;                     // a workgroup's 32-bit histogram words hold its share of the rows
  if (!d_q || !d_rank || !d_n || !d_n_skipped) return PINN_E_ARG;
  if (misaligned8(d_q) || misaligned8(d_rank) || misaligned8(d_n) || misaligned8(d_n_skipped) || misaligned8(d_ws)) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  if (!d_ws) return PINN_E_ARG;
  if (ws_bytes < pinn_unc_workspace_bytes(n, n_groups, n_quantiles)) return PINN_E_WORKSPACE;
  a.kind = kind;
  a.c_score = kind == PINN_UNC_COLUMN ? score_col : 0;
  const int T = n_groups * n_quantiles;
  const int blocks = row_blocks(n, kTile, kMaxBlocks);
  const size_t lds = (size_t)T * kDigits * sizeof(unsigned int);
  unsigned long long* hdr = static_cast<unsigned long long*>(d_ws);
  unsigned long long* ghist = hdr + kHdrWords;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  if (lds + 2048 > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)unc_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(unc_select_init_kernel, dim3(1), dim3(kThreads), 0, st, n_quantiles, T, hdr);
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(unc_select_kernel, dim3(blocks), dim3(kThreads), lds, st, a, n_quantiles, T, pass, hdr, ghist);
    if (pass > 0) hipLaunchKernelGGL(unc_gather_finish_kernel, dim3(T), dim3(kThreads), 0, st, T, hdr, ghist, d_q);
    hipLaunchKernelGGL(unc_narrow_kernel, dim3(1), dim3(kThreads), 0, st, n_groups, n_quantiles, pass, conformal ? 1 : 0, lv, n, hdr, ghist,
                       d_q, d_rank, d_n, d_n_skipped);
  }
  return launch_status();
}

extern "C" size_t pinn_unc_state_bytes(int window) {
  if (window < 1 || window > PINN_UNC_MAX_WINDOW) return 0;
  return ((size_t)PINN_UNC_STATE_HEADER + (size_t)window) * sizeof(double);
}

extern "C" int pinn_unc_update(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_cols,
                               const long long* d_row_index, long long n, const double* var_model, double level, double gamma,
                               double alpha_min, double alpha_max, int window, int learn, void* d_state, double* d_lo, double* d_hi,
                               double* d_z, int* d_flag, void* stream) {
  UncDev a;
  const int rc = make_unc(d_arr, ld, n_arr_rows, cols, n_cols, d_row_index, n, -1, nullptr, 0, 1, var_model, &a);
  if (rc != PINN_OK) return rc;
  if (n > PINN_UNC_MAX_CHUNK || window < 1 || window > PINN_UNC_MAX_WINDOW) return PINN_E_ARG;
  if (!(level > 0.0 && level < 1.0) || !(gamma >= 0.0) || !finite_host(gamma) || !(alpha_min >= 0.0) || !(alpha_max <= 1.0) ||
      !(alpha_min <= alpha_max))
    return PINN_E_ARG;
  if (!d_state || misaligned8(d_state) || misaligned8(d_lo) || misaligned8(d_hi) || misaligned8(d_z) || ((unsigned long long)d_flag & 3) != 0)
    return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  UpdateArgs u;
  u.level = level; u.gamma = gamma; u.alpha_min = alpha_min; u.alpha_max = alpha_max; u.window = window; u.learn = learn ? 1 : 0;
  clear_error();
  hipLaunchKernelGGL(unc_update_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, a, u, static_cast<unsigned long long*>(d_state), d_lo,
                     d_hi, d_z, d_flag);
  return launch_status();
}
