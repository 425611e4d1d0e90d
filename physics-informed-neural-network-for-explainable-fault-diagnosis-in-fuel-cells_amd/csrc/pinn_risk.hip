// Risk function RF(t) and first-alarm search on the device (reference script 04, cited as 04:<line>):
//   pinn_rf_stats       mu / sigma of the residual columns over the normal rows      (04:181-197)
//   pinn_rf_series      S_tot -> decaying integral C -> logistic RF_inst -> smoothed  (04:201-285)
//   pinn_rf_first_alarm first sample at or past a threshold, per segment              (04:289-300)
//   pinn_rf_sweep       many parameter sets over the same segments: first alarms, alarm rows and peak per (set, segment)
// All arithmetic is float64 and separately rounded (built with -ffp-contract=off).
//
// The two recurrences  C(t) = lambda C(t-1) + S(t)  and  RF_s(t) = alpha RF(t) + (1-alpha) RF_s(t-1)  are scans over
// (flag, multiplier, offset) triples; a flag marks a segment start and discards everything to its left.  They run as
// reduce-then-scan: one launch reduces every 2048-row tile to one triple, a one-workgroup launch turns the triples
// into the value entering each tile (tile order, fixed), a third launch finishes each tile.  Stream order between
// launches is the only dependency between workgroups: no workgroup ever waits on another inside a launch.  A call of
// at most one tile is a single launch.  Reductions are fixed-order (shuffle tree, then partials in index order): the
// same call gives the same bytes every time.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kThreads = 256;
constexpr int kItems = 8;                       // consecutive rows per thread in the scans
constexpr int kTile = kThreads * kItems;        // rows per workgroup
constexpr int kPad = kTile + kTile / kItems;    // LDS image: one pad word per 8 values (conflict-free blocked reads)
constexpr int kStatBlocks = 1024;               // upper limit of partial sums in pinn_rf_stats

struct RiskDev {
  int n_cols, n_layers, p_is_two, pad_;
  int col[PINN_RF_MAX_COLS], layer_of[PINN_RF_MAX_COLS];
  double w[PINN_RF_MAX_COLS], beta[PINN_RF_MAX_LAYERS];
  double p, inv_p, z_safe, lambda, k, c0, c_max, alpha, one_minus_alpha, l0, denom;
};

struct StatsDev {
  int n_cols, n_normal, label_col, pass;
  int col[PINN_RF_MAX_COLS];
  long long normal[PINN_RF_MAX_COLS];
};

// x -> f ? b : m x + b.  f is kept as a 64-bit word so that the struct has no padding in the workspace.
struct Op {
  double m, b;
  long long f;
};

__device__ __forceinline__ Op op_identity() { Op o; o.m = 1.0; o.b = 0.0; o.f = 0; return o; }

// "l, then r".  m is always finite (a product of multipliers), so an identity on either side changes no bit.
__device__ __forceinline__ Op combine(const Op& l, const Op& r) {
  Op o;
  o.m = r.f ? r.m : r.m * l.m;
  o.b = r.f ? r.b : r.m * l.b + r.b;
  o.f = r.f | l.f;
  return o;
}

__device__ __forceinline__ double apply(const Op& o, double x) { return o.f ? o.b : o.m * x + o.b; }

__device__ __forceinline__ int pidx(int i) { return i + (i >> 3); }

// np.clip: NaN stays NaN (fmin / fmax would return the bound)
__device__ __forceinline__ double clip_nan(double x, double lo, double hi) {
  if (x != x) return x;
  x = x < lo ? lo : x;
  return x > hi ? hi : x;
}

// Exclusive prefix of the threads' aggregates in thread order (identity for thread 0); *total = the workgroup's aggregate.
__device__ __forceinline__ Op block_exclusive(const Op& mine, Op* s_wave, Op* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Op inc = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    Op o;
    o.m = __shfl_up(inc.m, d, 64);
    o.b = __shfl_up(inc.b, d, 64);
    o.f = __shfl_up(inc.f, d, 64);
    if (lane >= d) inc = combine(o, inc);
  }
  Op prev;
  prev.m = __shfl_up(inc.m, 1, 64);
  prev.b = __shfl_up(inc.b, 1, 64);
  prev.f = __shfl_up(inc.f, 1, 64);
  if (lane == 0) prev = op_identity();
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  Op pre = op_identity(), tot = op_identity();
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    const Op a = s_wave[w];
    if (w < wave) pre = combine(pre, a);
    tot = combine(tot, a);
  }
  __syncthreads();                        // s_wave may be reused by the next scan
  *total = tot;
  return combine(pre, prev);
}

// S_tot of one row from its z-scores (04:240-259); the layer sums go to S_layers[L * n + j] when it is given
__device__ __forceinline__ double s_of_z(const RiskDev& a, const double z[PINN_RF_MAX_COLS], double* __restrict__ S_layers,
                                         long long n, long long j) {
  double term[PINN_RF_MAX_COLS];
#pragma unroll
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    term[d] = 0.0;
    if (d < a.n_cols) {
      const double t = fabs(z[d]) - a.z_safe;
      const double at = (t > 0.0 || t != t) ? t : 0.0;        // np.maximum(0, .): NaN propagates
      term[d] = a.w[d] * (a.p_is_two ? at * at : pow(at, a.p));
    }
  }
  double S = 0.0;
#pragma unroll
  for (int L = 0; L < PINN_RF_MAX_LAYERS; ++L) {
    if (L < a.n_layers) {
      double acc = 0.0;
      bool used = false;
#pragma unroll
      for (int d = 0; d < PINN_RF_MAX_COLS; ++d)
        if (d < a.n_cols && a.layer_of[d] == L) { acc = used ? acc + term[d] : term[d]; used = true; }
      const double Sl = used ? (a.p_is_two ? sqrt(acc) : pow(acc, a.inv_p)) : 0.0;
      if (S_layers) S_layers[(long long)L * n + j] = Sl;
      S += a.beta[L] * Sl;
    }
  }
  return S;
}

// ---- per-row instantaneous intensity S_tot (04:233-259), rows taken striped so that neighbouring lanes read neighbouring rows
__device__ __forceinline__ void stage_s(const RiskDev& a, const double* __restrict__ arr, long long ld, long long n_arr,
                                        const double* __restrict__ mu, const double* __restrict__ sigma,
                                        const long long* __restrict__ ridx, long long tile0, long long n, double* __restrict__ S_out,
                                        double* __restrict__ S_layers, double* s_val) {
  double m[PINN_RF_MAX_COLS], sg[PINN_RF_MAX_COLS];
#pragma unroll
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    m[d] = d < a.n_cols ? mu[d] : 0.0;
    sg[d] = d < a.n_cols ? sigma[d] : 1.0;
  }
#pragma unroll 2
  for (int k = 0; k < kItems; ++k) {
    const int i = k * kThreads + threadIdx.x;
    const long long j = tile0 + i;
    if (j >= n) break;
    const long long row = ridx ? ridx[j] : j;
    const bool ok = row >= 0 && row < n_arr;                  // a gather index outside the array reads nothing: the row is NaN
    const double* r = arr + (ok ? row : 0) * ld;
    double z[PINN_RF_MAX_COLS];
#pragma unroll
    for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
      z[d] = 0.0;
      if (d < a.n_cols) {
        const double R = ok ? r[a.col[d]] : quiet_nan();
        z[d] = (R - m[d]) / sg[d];
      }
    }
    const double S = s_of_z(a, z, S_layers, n, j);
    if (S_out) S_out[j] = S;
    s_val[pidx(i)] = S;
  }
}

// striped global <-> LDS image <-> blocked registers
__device__ __forceinline__ void load_tile(const double* __restrict__ src, long long tile0, long long n, double* s_val) {
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int i = k * kThreads + threadIdx.x;
    if (tile0 + i < n) s_val[pidx(i)] = src[tile0 + i];
  }
}

__device__ __forceinline__ void store_tile(const double v[kItems], double* __restrict__ dst, long long tile0, long long n, double* s_val) {
  __syncthreads();                        // every blocked read of the previous image is done
#pragma unroll
  for (int k = 0; k < kItems; ++k) s_val[pidx(threadIdx.x * kItems + k)] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const int i = k * kThreads + threadIdx.x;
    if (tile0 + i < n) dst[tile0 + i] = s_val[pidx(i)];
  }
}

__device__ __forceinline__ void blocked_from_lds(const double* s_val, double v[kItems]) {
#pragma unroll
  for (int k = 0; k < kItems; ++k) v[k] = s_val[pidx(threadIdx.x * kItems + k)];
}

// One tile of one recurrence.  WHICH 0: C from S (04:262-264), WHICH 1: RF_smooth from RF_inst (04:276-279).
// `entering` is the value of the recurrence just before the tile (ignored where a segment starts).  With agg_only the
// tile's aggregate is all that is produced.  The 8 values of a thread are then advanced with the reference's own
// expression, so inside a thread's run the operation sequence is the sequential loop's.
template <int WHICH>
__device__ __forceinline__ Op tile_recurrence(const RiskDev& a, const double v[kItems], long long tile0, long long n,
                                              const long long* __restrict__ ss, long long ns, const double* __restrict__ cin,
                                              double* __restrict__ cout, double entering, bool agg_only, Op* s_wave,
                                              double out[kItems]) {
  const long long j0 = tile0 + (long long)threadIdx.x * kItems;
  Op ops[kItems];
  long long seg[kItems];
  bool last[kItems];
  long long s = 0, begin = 0, next = n;
  if (j0 < n) {
    s = seg_of(ss, ns, j0);
    begin = seg_begin(ss, s);
    next = seg_next(ss, ns, s, n);
  }
  Op agg = op_identity();
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const long long j = j0 + k;
    ops[k] = op_identity();
    seg[k] = 0;
    last[k] = false;
    if (j < n) {
      while (j >= next && s + 1 < ns) {
        ++s;
        begin = seg_begin(ss, s);
        next = seg_next(ss, ns, s, n);
      }
      Op o;
      if (j == begin) {
        o.f = 1;
        o.m = 0.0;
        if (WHICH == 0) o.b = cin ? a.lambda * cin[2 * s] + v[k] : 0.0;               // 04:262-263: C[0] = 0, S_tot[0] unused
        else o.b = cin ? a.alpha * v[k] + a.one_minus_alpha * cin[2 * s + 1] : v[k];    // 04:277
      } else {
        o.f = 0;
        o.m = WHICH == 0 ? a.lambda : a.one_minus_alpha;
        o.b = WHICH == 0 ? v[k] : a.alpha * v[k];
      }
      ops[k] = o;
      seg[k] = s;
      last[k] = j + 1 == next || j + 1 == n;
      agg = combine(agg, o);
    }
  }
  Op total;
  const Op excl = block_exclusive(agg, s_wave, &total);
  if (agg_only) return total;
  double x = apply(excl, entering);
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    x = apply(ops[k], x);
    out[k] = x;
    if (last[k] && cout) cout[2 * seg[k] + WHICH] = x;
  }
  return total;
}

__device__ __forceinline__ double rf_inst(const RiskDev& a, double C) {
  const double cc = clip_nan(C, 0.0, a.c_max);
  const double L = 1.0 / (1.0 + exp(-a.k * (cc - a.c0)));
  return clip_nan((L - a.l0) / a.denom, 0.0, 1.0);
}

#define RF_ROWS_ARGS                                                                                                         \
  const double *__restrict__ arr, long long ld, long long n_arr, const double *__restrict__ mu, const double *__restrict__ sigma, \
      const long long *__restrict__ ridx, long long n, const long long *__restrict__ ss, long long ns, const double *__restrict__ cin

// n <= kTile: everything in one workgroup and one launch (the monitor's chunk)
__global__ __launch_bounds__(kThreads) void rf_single_kernel(RiskDev a, RF_ROWS_ARGS, double* __restrict__ S_layers,
                                                              double* __restrict__ S_out, double* __restrict__ C_out,
                                                              double* __restrict__ RF_out, double* __restrict__ RFs_out,
                                                              double* __restrict__ cout) {
  __shared__ double s_val[kPad];
  __shared__ Op s_wave[kThreads / 64];
  stage_s(a, arr, ld, n_arr, mu, sigma, ridx, 0, n, S_out, S_layers, s_val);
  __syncthreads();
  double v[kItems], c[kItems], rf[kItems], rs[kItems];
  blocked_from_lds(s_val, v);
  tile_recurrence<0>(a, v, 0, n, ss, ns, cin, cout, 0.0, false, s_wave, c);
  if (C_out) store_tile(c, C_out, 0, n, s_val);
#pragma unroll
  for (int k = 0; k < kItems; ++k) rf[k] = rf_inst(a, c[k]);
  if (RF_out) store_tile(rf, RF_out, 0, n, s_val);
  tile_recurrence<1>(a, rf, 0, n, ss, ns, cin, cout, 0.0, false, s_wave, rs);
  if (RFs_out) store_tile(rs, RFs_out, 0, n, s_val);
}

// pass 1: S_tot of every row (stored) and the tile aggregates of the C recurrence
__global__ __launch_bounds__(kThreads) void rf_pass1_kernel(RiskDev a, RF_ROWS_ARGS, double* __restrict__ S_layers,
                                                             double* __restrict__ S_out, Op* __restrict__ agg) {
  __shared__ double s_val[kPad];
  __shared__ Op s_wave[kThreads / 64];
  const long long tile0 = (long long)blockIdx.x * kTile;
  stage_s(a, arr, ld, n_arr, mu, sigma, ridx, tile0, n, S_out, S_layers, s_val);
  __syncthreads();
  double v[kItems], unused[kItems];
  blocked_from_lds(s_val, v);
  const Op total = tile_recurrence<0>(a, v, tile0, n, ss, ns, cin, nullptr, 0.0, true, s_wave, unused);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// the value entering every tile, from the tile aggregates in tile order: one workgroup, each thread a run of consecutive tiles
__global__ __launch_bounds__(kThreads) void rf_carry_kernel(const Op* __restrict__ agg, long long n_tiles, double* __restrict__ entering) {
  __shared__ Op s_wave[kThreads / 64];
  const long long chunk = (n_tiles + kThreads - 1) / kThreads;
  const long long t0 = (long long)threadIdx.x * chunk;
  const long long t1 = t0 + chunk < n_tiles ? t0 + chunk : n_tiles;
  Op mine = op_identity();
  for (long long t = t0; t < t1; ++t) mine = combine(mine, agg[t]);
  Op total;
  const Op excl = block_exclusive(mine, s_wave, &total);
  double x = apply(excl, 0.0);          // tile 0 begins with a segment start, so this 0 never reaches a result
  for (long long t = t0; t < t1; ++t) {
    entering[t] = x;
    x = apply(agg[t], x);
  }
}

// pass 2: finish C, the pointwise logistic, and the tile aggregates of the smoothing recurrence
__global__ __launch_bounds__(kThreads) void rf_pass2_kernel(RiskDev a, const double* __restrict__ S_in, long long n,
                                                             const long long* __restrict__ ss, long long ns,
                                                             const double* __restrict__ cin, const double* __restrict__ entering,
                                                             double* __restrict__ C_out, double* __restrict__ RF_out,
                                                             double* __restrict__ cout, Op* __restrict__ agg) {
  __shared__ double s_val[kPad];
  __shared__ Op s_wave[kThreads / 64];
  const long long tile0 = (long long)blockIdx.x * kTile;
  load_tile(S_in, tile0, n, s_val);
  __syncthreads();
  double v[kItems], c[kItems], rf[kItems], unused[kItems];
  blocked_from_lds(s_val, v);
  tile_recurrence<0>(a, v, tile0, n, ss, ns, cin, cout, entering[blockIdx.x], false, s_wave, c);
  if (C_out) store_tile(c, C_out, tile0, n, s_val);
#pragma unroll
  for (int k = 0; k < kItems; ++k) rf[k] = rf_inst(a, c[k]);
  store_tile(rf, RF_out, tile0, n, s_val);
  const Op total = tile_recurrence<1>(a, rf, tile0, n, ss, ns, cin, nullptr, 0.0, true, s_wave, unused);
  if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// pass 3: finish RF_smooth
__global__ __launch_bounds__(kThreads) void rf_pass3_kernel(RiskDev a, const double* __restrict__ RF_in, long long n,
                                                             const long long* __restrict__ ss, long long ns,
                                                             const double* __restrict__ cin, const double* __restrict__ entering,
                                                             double* __restrict__ RFs_out, double* __restrict__ cout) {
  __shared__ double s_val[kPad];
  __shared__ Op s_wave[kThreads / 64];
  const long long tile0 = (long long)blockIdx.x * kTile;
  load_tile(RF_in, tile0, n, s_val);
  __syncthreads();
  double v[kItems], rs[kItems];
  blocked_from_lds(s_val, v);
  tile_recurrence<1>(a, v, tile0, n, ss, ns, cin, cout, entering[blockIdx.x], false, s_wave, rs);
  if (RFs_out) store_tile(rs, RFs_out, tile0, n, s_val);
}

// ---- first alarm: only the first position of a run of matches (or a matching segment start) reaches the atomic
__global__ void alarm_init_kernel(unsigned long long* out, long long ns) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < ns) out[i] = ~0ull;           // reads as -1 (no alarm) when nothing lowers it
}

__device__ __forceinline__ double alarm_value(const double* __restrict__ series, long long stride, long long n_src,
                                              const long long* __restrict__ ridx, long long j) {
  const long long row = ridx ? ridx[j] : j;
  return (row >= 0 && row < n_src) ? series[row * stride] : quiet_nan();
}

__global__ __launch_bounds__(kThreads) void alarm_kernel(const double* __restrict__ series, long long stride, long long n_src,
                                                          const long long* __restrict__ ridx, long long n,
                                                          const long long* __restrict__ ss, long long ns, int below, int relative,
                                                          double thr, unsigned long long* __restrict__ out) {
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const long long s = seg_of(ss, ns, j);
  long long begin = seg_begin(ss, s);
  if (begin > j) begin = j;
  const double t = relative ? alarm_value(series, stride, n_src, ridx, begin) + thr : thr;
  const double v = alarm_value(series, stride, n_src, ridx, j);
  const bool hit = below ? v <= t : v >= t;          // NaN never matches
  if (!hit) return;
  if (j > begin) {
    const double pv = alarm_value(series, stride, n_src, ridx, j - 1);
    if (below ? pv <= t : pv >= t) return;           // an earlier position of this segment matches as well
  }
  atomicMin(out + s, (unsigned long long)(j - begin));
}

// ---- mu / sigma over the normal rows: per-workgroup partials, then one workgroup sums them in index order
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

// sums s[8] and counts c[9] of the workgroup, valid in thread 0
__device__ __forceinline__ void block_sums(double s[PINN_RF_MAX_COLS], long long c[PINN_RF_MAX_COLS + 1], double* s_d, long long* s_c) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    const double v = wave_sum(s[d]);
    if (lane == 0) s_d[wave * PINN_RF_MAX_COLS + d] = v;
  }
#pragma unroll
  for (int d = 0; d <= PINN_RF_MAX_COLS; ++d) {
    const long long v = wave_sum(c[d]);
    if (lane == 0) s_c[wave * (PINN_RF_MAX_COLS + 1) + d] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
      double v = s_d[d];
      for (int w = 1; w < kThreads / 64; ++w) v += s_d[w * PINN_RF_MAX_COLS + d];
      s[d] = v;
    }
    for (int d = 0; d <= PINN_RF_MAX_COLS; ++d) {
      long long v = s_c[d];
      for (int w = 1; w < kThreads / 64; ++w) v += s_c[w * (PINN_RF_MAX_COLS + 1) + d];
      c[d] = v;
    }
  }
}

// pass 0: sums of the values; pass 1: sums of the squares centred on mu (numpy's two-pass nanstd)
__global__ __launch_bounds__(kThreads) void stats_partial_kernel(StatsDev a, const double* __restrict__ arr, long long ld, long long n,
                                                                  const double* __restrict__ mu, double* __restrict__ part,
                                                                  long long* __restrict__ cpart) {
  __shared__ double s_d[(kThreads / 64) * PINN_RF_MAX_COLS];
  __shared__ long long s_c[(kThreads / 64) * (PINN_RF_MAX_COLS + 1)];
  double s[PINN_RF_MAX_COLS], m[PINN_RF_MAX_COLS];
  long long c[PINN_RF_MAX_COLS + 1];
#pragma unroll
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    s[d] = 0.0;
    c[d] = 0;
    m[d] = (a.pass == 1 && d < a.n_cols) ? mu[d] : 0.0;
  }
  c[PINN_RF_MAX_COLS] = 0;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const double* r = arr + i * ld;
    const double lab = r[a.label_col];
    if (lab != lab) continue;
    const long long li = (long long)lab;               // astype(int): truncation
    bool normal = false;
    for (int q = 0; q < a.n_normal; ++q) normal = normal || li == a.normal[q];
    if (!normal) continue;
    ++c[PINN_RF_MAX_COLS];
#pragma unroll
    for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
      if (d < a.n_cols) {
        const double v = r[a.col[d]];
        if (v == v) {                                   // a NaN leaves this column only
          const double dv = v - m[d];
          s[d] += a.pass == 1 ? dv * dv : v;
          ++c[d];
        }
      }
    }
  }
  block_sums(s, c, s_d, s_c);
  if (threadIdx.x == 0) {
    for (int d = 0; d < PINN_RF_MAX_COLS; ++d) part[(long long)blockIdx.x * PINN_RF_MAX_COLS + d] = s[d];
    for (int d = 0; d <= PINN_RF_MAX_COLS; ++d) cpart[(long long)blockIdx.x * (PINN_RF_MAX_COLS + 1) + d] = c[d];
  }
}

__global__ __launch_bounds__(kThreads) void stats_final_kernel(StatsDev a, const double* __restrict__ part, const long long* __restrict__ cpart,
                                                                int n_part, double* __restrict__ mu, double* __restrict__ sigma,
                                                                long long* __restrict__ count) {
  __shared__ double s_d[(kThreads / 64) * PINN_RF_MAX_COLS];
  __shared__ long long s_c[(kThreads / 64) * (PINN_RF_MAX_COLS + 1)];
  double s[PINN_RF_MAX_COLS];
  long long c[PINN_RF_MAX_COLS + 1];
#pragma unroll
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) { s[d] = 0.0; c[d] = 0; }
  c[PINN_RF_MAX_COLS] = 0;
  for (int g = threadIdx.x; g < n_part; g += kThreads) {
#pragma unroll
    for (int d = 0; d < PINN_RF_MAX_COLS; ++d) s[d] += part[(long long)g * PINN_RF_MAX_COLS + d];
#pragma unroll
    for (int d = 0; d <= PINN_RF_MAX_COLS; ++d) c[d] += cpart[(long long)g * (PINN_RF_MAX_COLS + 1) + d];
  }
  block_sums(s, c, s_d, s_c);
  if (threadIdx.x == 0) {
    for (int d = 0; d < a.n_cols; ++d) {
      if (a.pass == 0) {
        mu[d] = s[d] / (double)c[d];                    // 0 / 0 = NaN for a column without values, as nanmean
      } else {
        double sg = c[d] > 1 ? sqrt(s[d] / (double)(c[d] - 1)) : quiet_nan();      // ddof = 1
        if (sg == 0.0) sg = 1e-6;                       // 04:196
        sigma[d] = sg;
      }
    }
    if (a.pass == 0 && count)
      for (int d = 0; d <= PINN_RF_MAX_COLS; ++d) count[d] = c[d];
  }
}

// ---- sweep of parameter sets: z-scores staged once as [D][n] columns, then one workgroup per (candidate, segment)
struct SweepShape {
  int n_cols, n_layers;
  int col[PINN_RF_MAX_COLS], layer_of[PINN_RF_MAX_COLS];
};

// words of a candidate (include/pinn_hip.h)
constexpr int kCandP = 12, kCandZSafe = 13, kCandLambda = 14, kCandK = 15, kCandC0 = 16, kCandCMax = 17, kCandAlpha = 18,
              kCandWarn = 19, kCandDanger = 20;
constexpr long long kNoPosition = 0x7fffffffffffffffLL;

__device__ __forceinline__ bool finite_word(double x) { return fabs(x) <= 1.7976931348623157e308; }     // false for NaN and +-inf

// z = (R - mu) / sigma of every position and column, the division as in stage_s; column d begins at z + d * zs
__global__ __launch_bounds__(kThreads) void sweep_stage_kernel(SweepShape sh, const double* __restrict__ arr, long long ld, long long n_arr,
                                                                const double* __restrict__ mu, const double* __restrict__ sigma,
                                                                const long long* __restrict__ ridx, long long n,
                                                                double* __restrict__ z, long long zs) {
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const long long row = ridx ? ridx[j] : j;
  const bool ok = row >= 0 && row < n_arr;                    // a gather index outside the array reads nothing: the row is NaN
  const double* r = arr + (ok ? row : 0) * ld;
#pragma unroll
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    if (d < sh.n_cols) {
      const double R = ok ? r[sh.col[d]] : quiet_nan();
      z[(long long)d * zs + j] = (R - mu[d]) / sigma[d];
    }
  }
}

// Workgroup b evaluates candidate b / ns on segment b % ns: it walks the segment tile by tile in order, the values of both
// recurrences entering a tile held in registers (the workgroup's aggregate applied to the value that entered the tile
// before, as rf_carry_kernel does between tiles), and writes four words and the carry: nothing per row.  A thread keeps its
// own first positions, count and maximum over all tiles; they meet once, after the last tile, in lane and wave order.
__global__ __launch_bounds__(kThreads) void rf_sweep_kernel(SweepShape sh, const double* __restrict__ z, long long zs, long long n,
                                                             const long long* __restrict__ ss, long long ns,
                                                             const double* __restrict__ cand, long long* __restrict__ first_warn,
                                                             long long* __restrict__ first_danger, long long* __restrict__ n_warn,
                                                             double* __restrict__ peak, double* __restrict__ carry, int* __restrict__ bad) {
  __shared__ double s_val[kPad];
  __shared__ Op s_wave[kThreads / 64];
  __shared__ long long s_int[kThreads / 64][3];
  __shared__ double s_peak[kThreads / 64];
  __shared__ RiskDev s_a;
  __shared__ double s_thr[2];
  __shared__ int s_bad;
  const long long b = blockIdx.x;
  const long long p = b / ns, s = b - p * ns;
  // the candidate's 24 words are read once, by thread 0, and its RiskDev lives in LDS: every thread reads the same words
  // from there when it needs them, so none of them has to stay in a vector register across the tile loop
  if (threadIdx.x == 0) {
    const double* __restrict__ c = cand + p * PINN_RF_SWEEP_WORDS;
    bool is_bad = false;
    for (int q = 0; q < PINN_RF_SWEEP_WORDS; ++q) is_bad = is_bad || !finite_word(c[q]);
    is_bad = is_bad || c[kCandP] == 0.0;
    s_bad = is_bad ? 1 : 0;
    if (s == 0) bad[p] = s_bad;
    if (is_bad) {
      first_warn[b] = -1; first_danger[b] = -1; n_warn[b] = 0; peak[b] = quiet_nan();
      if (carry) { carry[2 * b] = quiet_nan(); carry[2 * b + 1] = quiet_nan(); }
    } else {
      RiskDev a;
      a.n_cols = sh.n_cols; a.n_layers = sh.n_layers; a.p_is_two = c[kCandP] == 2.0; a.pad_ = 0;
      for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
        const bool in = d < sh.n_cols;
        a.col[d] = 0;
        a.layer_of[d] = in ? sh.layer_of[d] : -1;
        a.w[d] = in ? c[d] : 0.0;
      }
      for (int l = 0; l < PINN_RF_MAX_LAYERS; ++l) a.beta[l] = l < sh.n_layers ? c[PINN_RF_MAX_COLS + l] : 0.0;
      a.p = c[kCandP]; a.inv_p = 1.0 / a.p; a.z_safe = c[kCandZSafe]; a.lambda = c[kCandLambda];
      a.k = c[kCandK]; a.c0 = c[kCandC0]; a.c_max = c[kCandCMax];
      a.alpha = c[kCandAlpha]; a.one_minus_alpha = 1.0 - a.alpha;
      a.l0 = 1.0 / (1.0 + exp(-a.k * (0.0 - a.c0)));                                 // 04:268-270
      const double l_max = 1.0 / (1.0 + exp(-a.k * (a.c_max - a.c0)));
      a.denom = (l_max - a.l0) != 0.0 ? (l_max - a.l0) : 1e-6;
      s_a = a;
      s_thr[0] = c[kCandWarn];
      s_thr[1] = c[kCandDanger];
    }
  }
  __syncthreads();
  if (s_bad) return;                                          // the same for every thread of the workgroup
  const RiskDev& a = s_a;
  const double warn = s_thr[0], danger = s_thr[1];

  long long begin = seg_begin(ss, s), next = seg_next(ss, ns, s, n);
  begin = begin < 0 ? 0 : (begin > n ? n : begin);            // starts are device data: a wrong one must not read past z
  next = next < begin ? begin : (next > n ? n : next);
  const long long len = next - begin;
  const double* __restrict__ zseg = z + begin;
  double* cout = carry ? carry + 2 * b : nullptr;
  if (len == 0 && cout && threadIdx.x == 0) { cout[0] = quiet_nan(); cout[1] = quiet_nan(); }

  double enter_c = 0.0, enter_r = 0.0;      // tile 0 begins with the segment start, so these zeros never reach a result
  long long fw = kNoPosition, fd = kNoPosition, cnt = 0;
  double pk = quiet_nan();
  for (long long tile0 = 0; tile0 < len; tile0 += kTile) {
#pragma unroll 2
    for (int k = 0; k < kItems; ++k) {
      const int i = k * kThreads + threadIdx.x;
      const long long j = tile0 + i;
      if (j >= len) break;
      double zr[PINN_RF_MAX_COLS];
#pragma unroll
      for (int d = 0; d < PINN_RF_MAX_COLS; ++d) zr[d] = d < sh.n_cols ? zseg[(long long)d * zs + j] : 0.0;
      s_val[pidx(i)] = s_of_z(a, zr, nullptr, 0, 0);
    }
    __syncthreads();
    double v[kItems], cv[kItems], rf[kItems], rs[kItems];
    blocked_from_lds(s_val, v);
    const Op tc = tile_recurrence<0>(a, v, tile0, len, nullptr, 1, nullptr, cout, enter_c, false, s_wave, cv);
#pragma unroll
    for (int k = 0; k < kItems; ++k) rf[k] = rf_inst(a, cv[k]);
    const Op tr = tile_recurrence<1>(a, rf, tile0, len, nullptr, 1, nullptr, cout, enter_r, false, s_wave, rs);
    enter_c = apply(tc, enter_c);
    enter_r = apply(tr, enter_r);
    const long long j0 = tile0 + (long long)threadIdx.x * kItems;
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
      const long long j = j0 + k;
      if (j < len) {
        const double x = rs[k];
        if (x >= warn) { ++cnt; fw = fw < j ? fw : j; }        // NaN never matches
        if (x >= danger) fd = fd < j ? fd : j;
        if (x == x && !(pk >= x)) pk = x;                       // and never enters the peak
      }
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const long long ofw = __shfl_down(fw, d, 64), ofd = __shfl_down(fd, d, 64);
    const double opk = __shfl_down(pk, d, 64);
    cnt += __shfl_down(cnt, d, 64);
    fw = fw < ofw ? fw : ofw;
    fd = fd < ofd ? fd : ofd;
    if (opk == opk && !(pk >= opk)) pk = opk;
  }
  if (lane == 0) { s_int[wave][0] = fw; s_int[wave][1] = fd; s_int[wave][2] = cnt; s_peak[wave] = pk; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) {
      fw = fw < s_int[w][0] ? fw : s_int[w][0];
      fd = fd < s_int[w][1] ? fd : s_int[w][1];
      cnt += s_int[w][2];
      const double opk = s_peak[w];
      if (opk == opk && !(pk >= opk)) pk = opk;
    }
    first_warn[b] = fw == kNoPosition ? -1 : fw;
    first_danger[b] = fd == kNoPosition ? -1 : fd;
    n_warn[b] = cnt;
    peak[b] = pk;
  }
}

inline long long n_tiles_of(long long n) { return (n + kTile - 1) / kTile; }

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_rf_stats_workspace_bytes(void) {
  return (size_t)pinn::kStatBlocks * (PINN_RF_MAX_COLS * sizeof(double) + (PINN_RF_MAX_COLS + 1) * sizeof(long long));
}

extern "C" int pinn_rf_stats(const double* d_arr, long long ld, long long n_rows, const int* cols, int n_cols, int label_col,
                             const long long* normal_labels, int n_normal, double* d_mu, double* d_sigma, long long* d_count,
                             void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (n_rows < 0 || ld < 1 || !cols || n_cols < 1 || n_cols > PINN_RF_MAX_COLS || !normal_labels || n_normal < 1 ||
      n_normal > PINN_RF_MAX_COLS || label_col < 0 || label_col >= ld)
    return PINN_E_ARG;
  for (int d = 0; d < n_cols; ++d)
    if (cols[d] < 0 || cols[d] >= ld) return PINN_E_ARG;
  if (!d_mu || !d_sigma || !d_ws || (n_rows > 0 && !d_arr)) return PINN_E_ARG;
  if (misaligned8(d_arr) || misaligned8(d_mu) || misaligned8(d_sigma) || misaligned8(d_count) || misaligned8(d_ws)) return PINN_E_ARG;
  if (ws_bytes < pinn_rf_stats_workspace_bytes()) return PINN_E_WORKSPACE;
  StatsDev a;
  a.n_cols = n_cols; a.n_normal = n_normal; a.label_col = label_col;
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    a.col[d] = d < n_cols ? cols[d] : 0;
    a.normal[d] = d < n_normal ? normal_labels[d] : 0;
  }
  long long blocks = (n_rows + kThreads - 1) / kThreads;
  blocks = blocks < 1 ? 1 : (blocks > kStatBlocks ? kStatBlocks : blocks);
  double* part = static_cast<double*>(d_ws);
  long long* cpart = reinterpret_cast<long long*>(part + (size_t)kStatBlocks * PINN_RF_MAX_COLS);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  for (int pass = 0; pass < 2; ++pass) {
    a.pass = pass;
    hipLaunchKernelGGL(stats_partial_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, a, d_arr, ld, n_rows, d_mu, part, cpart);
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(kThreads), 0, st, a, part, cpart, (int)blocks, d_mu, d_sigma, d_count);
  }
  return launch_status();
}

extern "C" size_t pinn_rf_workspace_bytes(long long n_rows, long long n_segments) {
  using namespace pinn;
  (void)n_segments;                       // segments cost no workspace: starts are looked up, not expanded into flags
  if (n_rows <= kTile) return 0;          // a single launch needs none
  const size_t t = (size_t)n_tiles_of(n_rows);
  return 2 * align256((size_t)n_rows * sizeof(double)) + 2 * align256(t * sizeof(Op)) + 2 * align256(t * sizeof(double));
}

extern "C" int pinn_rf_series(const double* d_arr, long long ld, long long n_arr_rows, const pinn_rf_params_t* prm,
                              const double* d_mu, const double* d_sigma, const long long* d_row_index, long long n,
                              const long long* d_seg_start, long long n_segments, const double* d_carry_in, double* d_S_layers,
                              double* d_S_tot, double* d_C, double* d_RF_inst, double* d_RF_smooth, double* d_carry_out,
                              void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (!prm || n < 0 || n_arr_rows < 0 || ld < 1 || n_segments < 0 || (n_segments > 0 && !d_seg_start)) return PINN_E_ARG;
  if (prm->n_cols < 1 || prm->n_cols > PINN_RF_MAX_COLS || prm->n_layers < 0 || prm->n_layers > PINN_RF_MAX_LAYERS) return PINN_E_ARG;
  for (int d = 0; d < prm->n_cols; ++d)
    if (prm->col[d] < 0 || prm->col[d] >= ld || prm->layer_of[d] >= prm->n_layers || !isfinite(prm->w[d])) return PINN_E_ARG;
  const double scal[7] = {prm->p_layer, prm->z_safe, prm->lambda_decay, prm->k_logistic, prm->c0_logistic, prm->c_max, prm->alpha_smooth};
  for (double v : scal)
    if (!isfinite(v)) return PINN_E_ARG;
  if (prm->p_layer == 0.0) return PINN_E_ARG;
  if (d_row_index == nullptr && n > n_arr_rows) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  if (!d_arr || !d_mu || !d_sigma) return PINN_E_ARG;
  if (misaligned8(d_arr) || misaligned8(d_mu) || misaligned8(d_sigma) || misaligned8(d_row_index) || misaligned8(d_seg_start) ||
      misaligned8(d_carry_in) || misaligned8(d_S_layers) || misaligned8(d_S_tot) || misaligned8(d_C) || misaligned8(d_RF_inst) ||
      misaligned8(d_RF_smooth) || misaligned8(d_carry_out) || misaligned8(d_ws))
    return PINN_E_ARG;
  const long long ns = n_segments > 0 ? n_segments : 1;
  RiskDev a;
  a.n_cols = prm->n_cols; a.n_layers = prm->n_layers; a.p_is_two = prm->p_layer == 2.0; a.pad_ = 0;
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    const bool in = d < prm->n_cols;
    a.col[d] = in ? prm->col[d] : 0;
    a.layer_of[d] = in ? prm->layer_of[d] : -1;
    a.w[d] = in ? prm->w[d] : 0.0;
  }
  for (int l = 0; l < PINN_RF_MAX_LAYERS; ++l) a.beta[l] = l < prm->n_layers ? prm->beta[l] : 0.0;
  a.p = prm->p_layer; a.inv_p = 1.0 / prm->p_layer; a.z_safe = prm->z_safe; a.lambda = prm->lambda_decay;
  a.k = prm->k_logistic; a.c0 = prm->c0_logistic; a.c_max = prm->c_max;
  a.alpha = prm->alpha_smooth; a.one_minus_alpha = 1.0 - prm->alpha_smooth;
  a.l0 = 1.0 / (1.0 + exp(-a.k * (0.0 - a.c0)));                                   // 04:268-270
  const double l_max = 1.0 / (1.0 + exp(-a.k * (a.c_max - a.c0)));
  a.denom = (l_max - a.l0) != 0.0 ? (l_max - a.l0) : 1e-6;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  if (n <= kTile) {
    hipLaunchKernelGGL(rf_single_kernel, dim3(1), dim3(kThreads), 0, st, a, d_arr, ld, n_arr_rows, d_mu, d_sigma, d_row_index, n,
                       d_seg_start, ns, d_carry_in, d_S_layers, d_S_tot, d_C, d_RF_inst, d_RF_smooth, d_carry_out);
  } else {
    if (!d_ws) return PINN_E_ARG;
    if (ws_bytes < pinn_rf_workspace_bytes(n, ns)) return PINN_E_WORKSPACE;
    const long long tiles = n_tiles_of(n);
    if (tiles > 0x7fffffffLL) return PINN_E_ARG;
    char* w = static_cast<char*>(d_ws);
    double* s_buf = reinterpret_cast<double*>(w); w += align256((size_t)n * sizeof(double));
    double* rf_buf = reinterpret_cast<double*>(w); w += align256((size_t)n * sizeof(double));
    Op* agg_c = reinterpret_cast<Op*>(w); w += align256((size_t)tiles * sizeof(Op));
    Op* agg_r = reinterpret_cast<Op*>(w); w += align256((size_t)tiles * sizeof(Op));
    double* ent_c = reinterpret_cast<double*>(w); w += align256((size_t)tiles * sizeof(double));
    double* ent_r = reinterpret_cast<double*>(w);
    double* S = d_S_tot ? d_S_tot : s_buf;
    double* RF = d_RF_inst ? d_RF_inst : rf_buf;
    const dim3 grid((unsigned)tiles), block(kThreads);
    hipLaunchKernelGGL(rf_pass1_kernel, grid, block, 0, st, a, d_arr, ld, n_arr_rows, d_mu, d_sigma, d_row_index, n, d_seg_start, ns,
                       d_carry_in, d_S_layers, S, agg_c);
    hipLaunchKernelGGL(rf_carry_kernel, dim3(1), block, 0, st, agg_c, tiles, ent_c);
    hipLaunchKernelGGL(rf_pass2_kernel, grid, block, 0, st, a, S, n, d_seg_start, ns, d_carry_in, ent_c, d_C, RF, d_carry_out, agg_r);
    hipLaunchKernelGGL(rf_carry_kernel, dim3(1), block, 0, st, agg_r, tiles, ent_r);
    hipLaunchKernelGGL(rf_pass3_kernel, grid, block, 0, st, a, RF, n, d_seg_start, ns, d_carry_in, ent_r, d_RF_smooth, d_carry_out);
  }
  return launch_status();
}

extern "C" size_t pinn_rf_sweep_workspace_bytes(long long n, int n_cols) {
  using namespace pinn;
  if (n <= 0 || n_cols < 1) return 0;
  return (size_t)n_cols * align256((size_t)n * sizeof(double));
}

extern "C" int pinn_rf_sweep(const double* d_arr, long long ld, long long n_arr_rows, const pinn_rf_params_t* shape,
                             const double* d_mu, const double* d_sigma, const long long* d_row_index, long long n,
                             const long long* d_seg_start, long long n_segments, const double* d_cand, long long n_cand,
                             long long* d_first_warn, long long* d_first_danger, long long* d_n_warn, double* d_peak,
                             double* d_carry_out, int* d_bad, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (!shape || n < 0 || n_arr_rows < 0 || ld < 1 || n_segments < 0 || (n_segments > 0 && !d_seg_start) || n_cand < 1) return PINN_E_ARG;
  if (shape->n_cols < 1 || shape->n_cols > PINN_RF_MAX_COLS || shape->n_layers < 0 || shape->n_layers > PINN_RF_MAX_LAYERS) return PINN_E_ARG;
  for (int d = 0; d < shape->n_cols; ++d)
    if (shape->col[d] < 0 || shape->col[d] >= ld || shape->layer_of[d] >= shape->n_layers) return PINN_E_ARG;
  if (d_row_index == nullptr && n > n_arr_rows) return PINN_E_ARG;
  const long long ns = n_segments > 0 ? n_segments : 1;
  if (n_cand > 0x7fffffffLL / ns) return PINN_E_ARG;            // one workgroup per (candidate, segment)
  if (!d_cand || !d_first_warn || !d_first_danger || !d_n_warn || !d_peak || !d_bad) return PINN_E_ARG;
  if (n > 0 && (!d_arr || !d_mu || !d_sigma || !d_ws)) return PINN_E_ARG;
  if (misaligned8(d_arr) || misaligned8(d_mu) || misaligned8(d_sigma) || misaligned8(d_row_index) || misaligned8(d_seg_start) ||
      misaligned8(d_cand) || misaligned8(d_first_warn) || misaligned8(d_first_danger) || misaligned8(d_n_warn) || misaligned8(d_peak) ||
      misaligned8(d_carry_out) || ((unsigned long long)d_bad & 3) != 0 || misaligned8(d_ws))
    return PINN_E_ARG;
  if (ws_bytes < pinn_rf_sweep_workspace_bytes(n, shape->n_cols)) return PINN_E_WORKSPACE;
  const long long stage_blocks = (n + kThreads - 1) / kThreads;
  if (stage_blocks > 0x7fffffffLL) return PINN_E_ARG;
  SweepShape sh;
  sh.n_cols = shape->n_cols; sh.n_layers = shape->n_layers;
  for (int d = 0; d < PINN_RF_MAX_COLS; ++d) {
    const bool in = d < shape->n_cols;
    sh.col[d] = in ? shape->col[d] : 0;
    sh.layer_of[d] = in ? shape->layer_of[d] : -1;
  }
  double* z = static_cast<double*>(d_ws);
  const long long zs = (long long)(align256((size_t)n * sizeof(double)) / sizeof(double));
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  if (n > 0)
    hipLaunchKernelGGL(sweep_stage_kernel, dim3((unsigned)stage_blocks), dim3(kThreads), 0, st, sh, d_arr, ld, n_arr_rows, d_mu, d_sigma,
                       d_row_index, n, z, zs);
  hipLaunchKernelGGL(rf_sweep_kernel, dim3((unsigned)(n_cand * ns)), dim3(kThreads), 0, st, sh, z, zs, n, d_seg_start, ns, d_cand,
                     d_first_warn, d_first_danger, d_n_warn, d_peak, d_carry_out, d_bad);
  return launch_status();
}

extern "C" int pinn_rf_first_alarm(const double* d_series, long long stride, long long n_src_rows, const long long* d_row_index,
                                   long long n, const long long* d_seg_start, long long n_segments, int mode, int relative,
                                   double threshold, long long* d_first, void* stream) {
  using namespace pinn;
  if (n < 0 || n_src_rows < 0 || stride < 1 || n_segments < 0 || (n_segments > 0 && !d_seg_start) || !d_first) return PINN_E_ARG;
  if (mode != PINN_RF_ABOVE && mode != PINN_RF_BELOW) return PINN_E_ARG;
  if (threshold != threshold) return PINN_E_ARG;
  if (d_row_index == nullptr && n > n_src_rows) return PINN_E_ARG;
  if (n > 0 && !d_series) return PINN_E_ARG;
  if (misaligned8(d_series) || misaligned8(d_row_index) || misaligned8(d_seg_start) || misaligned8(d_first)) return PINN_E_ARG;
  const long long ns = n_segments > 0 ? n_segments : 1;
  const long long blocks = (n + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffffLL || (ns + kThreads - 1) / kThreads > 0x7fffffffLL) return PINN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(d_first);
  hipLaunchKernelGGL(alarm_init_kernel, dim3((unsigned)((ns + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, out, ns);
  if (n > 0)
    hipLaunchKernelGGL(alarm_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, st, d_series, stride, n_src_rows, d_row_index, n,
                       d_seg_start, ns, mode == PINN_RF_BELOW ? 1 : 0, relative ? 1 : 0, threshold, out);
  return launch_status();
}
