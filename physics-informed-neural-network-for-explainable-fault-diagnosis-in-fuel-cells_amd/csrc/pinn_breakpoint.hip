// pinn_breakpoint.hip -- the hydrogen and oxygen excess-ratio laws per window: y = a + b min(x, c) / 100, breakpoint included
//   pinn_bp_fit    exact enumeration of the at most 2 m candidate breakpoints of a window from running sums, theta [3] with
//                  its covariance, the profile interval of c and the evidence for a plateau, per window
//
// The statement of the problem, the solver, the sum orders and the status codes are in include/pinn_hip.h; supply.py's host
// backend states the same solver in numpy.  One workgroup owns a window from its gather to its covariance: it reads nothing
// another workgroup writes and uses no float atomics.
//
// LDS: the compacted rows as three separate arrays, x [cap] and y [cap] float64 and the rank in position order [cap] 16 bit
// (18 bytes a row: 4096 rows are 76.5 KB, two workgroups per CU), not as (x, y) pairs: the network's compare-exchange reads
// only x and the rank on most steps, and consecutive lanes then read consecutive 8-byte words (ds_read_b64, conflict-free),
// where pairs would spend half of every bank row on y.  The walks read row t R + r in lane t: at R = 16 that is a stride of
// 128 bytes, 16 lanes on a bank, so row i sits at i + (i >> 4): the stride becomes 136 bytes, conflict-free for the two
// 32-lane groups of a ds_read_b64 (R = 8: 2-way, R <= 4: the 32 lanes share at most 4 bank rows).
// Built with -ffp-contract=off: every operation is rounded on its own.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kBpMaxBlocks = 512;                               // two workgroups per CU fit beside each other at the longest window; grid-stride beyond
constexpr int kMom = 6;                                         // running sums: 1, z, y, zz, zy, yy
constexpr int kFree = 1 << 16;                                  // candidate key: k for a knot, kFree + k for a free candidate
constexpr double kPivotMin = 1.0 / 1099511627776.0;             // 2^-40: smallest pivot of the scaled normal matrix
constexpr double kQDefault = 3.841458820694124;

static_assert(PINN_BP_MAX_WINDOW == 4096 && PINN_BP_MAX_WINDOW < kFree, "ranks are 16 bit, keys hold k below kFree");

__host__ __device__ __forceinline__ int padded(int i) { return i + (i >> 4); }
inline size_t bp_lds_bytes(int npad) { return ((size_t)(npad + (npad >> 4)) * 18 + 15) & ~(size_t)15; }

// exclusive prefix and total of the 256 threads' values, per sum: Hillis-Steele over the wave's lanes, then the waves in order
__device__ __forceinline__ void block_scan(const double v[kMom], double excl[kMom], double tot[kMom], double (*ws)[kMom]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double e[kMom];
#pragma unroll
  for (int s = 0; s < kMom; ++s) {
    double inc = v[s];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    const double ex = __shfl_up(inc, 1, 64);
    e[s] = lane == 0 ? 0.0 : ex;
    if (lane == 63) ws[wave][s] = inc;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < kMom; ++s) {
    double t = 0.0, off = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave) off = t;
      t += ws[w][s];
    }
    excl[s] = off + e[s];
    tot[s] = t;
  }
  __syncthreads();                                              // ws is free for the next scan
}

// SSE of the knot candidate at k = p[0] rows (prefix sums p, totals T, centred z_k) with its centred regression
__device__ __forceinline__ double knot_sse(const double p[kMom], const double T[kMom], double m, double zk, bool two, double* alpha,
                                           double* beta, bool* constant) {
  const double rem = m - p[0];
  const double Su = p[1] + rem * zk, Suu = p[3] + rem * (zk * zk), Suy = p[4] + zk * (T[2] - p[2]);
  const double Duu = Suu - Su * Su / m, Duy = Suy - Su * T[2] / m, Dyy = T[5] - T[2] * T[2] / m;
  if (two && Duu > 0.0) {
    *beta = Duy / Duu;
    *alpha = (T[2] - *beta * Su) / m;
    *constant = false;
    return Dyy - Duy * Duy / Duu;
  }
  *beta = 0.0;
  *alpha = T[2] / m;
  *constant = true;
  return Dyy;
}

__device__ __forceinline__ bool better(double s, int key, double bs, int bkey) { return s < bs || (s == bs && key < bkey); }

// Cholesky factor of the packed symmetric M; false when a pivot is not above pmin (as pinn_identify.hip)
__device__ __forceinline__ bool chol3(const double M[6], double pmin, double L[6]) {
  double p = M[0];
  if (!(p > pmin)) return false;
  L[0] = sqrt(p);
  L[1] = M[1] / L[0];
  L[3] = M[3] / L[0];
  p = M[2] - L[1] * L[1];
  if (!(p > pmin)) return false;
  L[2] = sqrt(p);
  L[4] = (M[4] - L[3] * L[1]) / L[2];
  p = (M[5] - L[3] * L[3]) - L[4] * L[4];
  if (!(p > pmin)) return false;
  L[5] = sqrt(p);
  return true;
}
__device__ __forceinline__ void chol3_solve(const double L[6], const double b[3], double x[3]) {
  double y[3];
  y[0] = b[0] / L[0];
  y[1] = (b[1] - L[1] * y[0]) / L[2];
  y[2] = ((b[2] - L[3] * y[0]) - L[4] * y[1]) / L[5];
  x[2] = y[2] / L[5];
  x[1] = (y[1] - L[4] * x[2]) / L[2];
  x[0] = ((y[0] - L[1] * x[1]) - L[3] * x[2]) / L[0];
}

__device__ __forceinline__ void write_empty(double* fr, double n_used, double status) {
  const double nan = quiet_nan();
  const int t = threadIdx.x;
  if (t < PINN_BP_FIT_WORDS) fr[t] = (t < 10 || (t >= 15 && t <= 20)) ? nan : (t == 12 ? n_used : (t == 14 ? status : 0.0));
}

__global__ __launch_bounds__(kThreads) void bp_fit_kernel(Rows a, const long long* __restrict__ win_start, const long long* __restrict__ win_len,
                                                          long long n_windows, int npad_max, double q, double* __restrict__ fit) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double ws[kWaves][kMom];
  __shared__ double wbest[kWaves], wlo[kWaves], whi[kWaves], win_theta[4];
  __shared__ int wkey[kWaves], wcnt[kWaves], win_kind[2];
  const int cap = npad_max + (npad_max >> 4);
  double* xs = reinterpret_cast<double*>(smem);
  double* ys = xs + cap;
  unsigned short* ids = reinterpret_cast<unsigned short*>(ys + cap);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double nan = quiet_nan();

  for (long long w = blockIdx.x; w < n_windows; w += gridDim.x) {
    const long long start = win_start[w], len = win_len[w];     // uniform: every thread reads the same two words
    double* fr = fit + w * PINN_BP_FIT_WORDS;
    if (start < 0 || len < 0 || len > npad_max || start > a.n - len) {
      write_empty(fr, 0.0, 6.0);
      continue;
    }
    // gather and compact in position order: rank r < len <= npad_max, so padded(r) < cap
    int m = 0;
    for (long long j0 = 0; j0 < len; j0 += kThreads) {
      const long long j = j0 + threadIdx.x;
      double x[kRowsMaxD];
      bool used = false;
      if (j < len) {
        const bool ok = load_row(a, start + j, x);
        used = ok && isfinite(x[0]) && isfinite(x[1]);
      }
      const unsigned long long bal = __ballot(used);
      if (lane == 0) wcnt[wave] = __popcll(bal);
      __syncthreads();
      int off = m, total = 0;
#pragma unroll
      for (int v = 0; v < kWaves; ++v) {
        if (v < wave) off += wcnt[v];
        total += wcnt[v];
      }
      if (used) {
        const int r = off + __popcll(bal & ((1ull << lane) - 1ull));
        const int p = padded(r);
        xs[p] = x[0]; ys[p] = x[1]; ids[p] = (unsigned short)r;
      }
      m += total;
      __syncthreads();
    }
    if (m < 4) {
      write_empty(fr, (double)m, 3.0);
      continue;
    }
    int npad = 4;
    while (npad < m) npad <<= 1;                                // m <= len <= npad_max, a power of two: npad <= npad_max
    for (int i = m + threadIdx.x; i < npad; i += kThreads) {
      const int p = padded(i);
      xs[p] = INFINITY; ys[p] = 0.0; ids[p] = (unsigned short)i;
    }
    __syncthreads();

    // bitonic network on the keys (x, rank): the keys are distinct, so the sorted order is unique
    for (int k = 2; k <= npad; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = threadIdx.x; t < (npad >> 1); t += kThreads) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const int pi = padded(i), pl = padded(l);
          const double xa = xs[pi], xb = xs[pl];
          const unsigned short ia = ids[pi], ib = ids[pl];
          const bool gt = xa > xb || (xa == xb && ia > ib);
          if (gt == ((i & k) == 0)) {
            const double ya = ys[pi], yb = ys[pl];
            xs[pi] = xb; xs[pl] = xa; ys[pi] = yb; ys[pl] = ya; ids[pi] = ib; ids[pl] = ia;
          }
        }
        __syncthreads();
      }
    }

    const int R = npad >= kThreads ? npad / kThreads : 1;
    const int i0 = min((int)threadIdx.x * R, m), i1 = min(i0 + R, m);
    const double dm = (double)m;
    const double x_first = xs[0], x_last = xs[padded(m - 1)];
    double v[kMom], ex[kMom], T[kMom];

    // the window means
#pragma unroll
    for (int s = 0; s < kMom; ++s) v[s] = 0.0;
    for (int i = i0; i < i1; ++i) {
      v[0] += xs[padded(i)] / 100.0;
      v[1] += ys[padded(i)];
    }
    block_scan(v, ex, T, ws);
    const double zbar = T[0] / dm, ybar = T[1] / dm;

    // the six centred sums: thread totals, then every thread's exclusive prefix
#pragma unroll
    for (int s = 0; s < kMom; ++s) v[s] = 0.0;
    for (int i = i0; i < i1; ++i) {
      const double z = xs[padded(i)] / 100.0 - zbar, y = ys[padded(i)] - ybar;
      v[0] += 1.0; v[1] += z; v[2] += y; v[3] += z * z; v[4] += z * y; v[5] += y * y;
    }
    block_scan(v, ex, T, ws);

    // first walk: the candidates of the thread's rows
    double bs = INFINITY, ba = nan, bb = nan, bc = nan;
    int bkey = INT_MAX, bkind = 3;
    double p[kMom];
#pragma unroll
    for (int s = 0; s < kMom; ++s) p[s] = ex[s];
    for (int i = i0; i < i1; ++i) {
      const double xi = xs[padded(i)];
      const double z = xi / 100.0 - zbar, y = ys[padded(i)] - ybar;
      p[0] += 1.0; p[1] += z; p[2] += y; p[3] += z * z; p[4] += z * y; p[5] += y * y;
      const int k = i + 1;
      const double xn = k < m ? xs[padded(k)] : INFINITY;
      if (!(xi < xn)) continue;
      const bool two = xi > x_first;
      double alpha, beta;
      bool constant;
      const double s = knot_sse(p, T, dm, z, two, &alpha, &beta, &constant);
      if (better(s, k, bs, bkey)) {
        bs = s; bkey = k; bkind = constant ? 3 : (k == m ? 2 : 1);
        ba = (ybar + alpha) - beta * zbar; bb = beta; bc = xi;
      }
      if (k >= 2 && k <= m - 1 && two) {
        const double dk = (double)k, nr = dm - dk;
        const double Lzz = p[3] - p[1] * p[1] / dk, Lzy = p[4] - p[1] * p[2] / dk, Lyy = p[5] - p[2] * p[2] / dk;
        const double bl = Lzy / Lzz, al = (p[2] - bl * p[1]) / dk;
        const double ry = T[2] - p[2], d = ry / nr;
        const double sf = (Lyy - Lzy * Lzy / Lzz) + ((T[5] - p[5]) - ry * ry / nr);
        const double c = ((d - al) / bl + zbar) * 100.0;
        if (Lzz > 0.0 && bl != 0.0 && c >= xi && c <= xn && better(sf, kFree + k, bs, bkey)) {
          bs = sf; bkey = kFree + k; bkind = 0;
          ba = (ybar + al) - bl * zbar; bb = bl; bc = c;
        }
      }
    }
    // the block's winner: the order (sse, key) is total on comparable SSEs, so the butterfly's order does not matter
    double gs = bs;
    int gkey = bkey;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(gs, o, 64);
      const int ok = __shfl_xor(gkey, o, 64);
      if (better(os, ok, gs, gkey)) { gs = os; gkey = ok; }
    }
    if (lane == 0) { wbest[wave] = gs; wkey[wave] = gkey; }
    __syncthreads();
    gs = wbest[0]; gkey = wkey[0];
#pragma unroll
    for (int v2 = 1; v2 < kWaves; ++v2)
      if (better(wbest[v2], wkey[v2], gs, gkey)) { gs = wbest[v2]; gkey = wkey[v2]; }
    if (gkey != INT_MAX && gkey == bkey) {                       // the one thread that owns row k
      win_theta[0] = ba; win_theta[1] = bb; win_theta[2] = bkind == 2 ? INFINITY : bc; win_theta[3] = bc;
      win_kind[0] = bkind;
    }
    __syncthreads();
    if (gkey == INT_MAX) {                                       // no candidate has a comparable SSE (sums not finite)
      if (threadIdx.x < PINN_BP_FIT_WORDS) {
        const int t = threadIdx.x;
        fr[t] = t == 12 ? dm : (t == 14 ? 5.0 : (t == 19 ? x_first : (t == 20 ? x_last : ((t == 10 || t == 11 || t == 13 || t > 20) ? 0.0 : nan))));
      }
      __syncthreads();
      continue;
    }
    const double th_a = win_theta[0], th_b = win_theta[1], th_c = win_theta[2], c_own = win_theta[3];
    const int kind = win_kind[0], kwin = gkey >= kFree ? gkey - kFree : gkey;
    const double thr = gs * (1.0 + q / (dm - 3.0));

    // second walk: the direct sums at the winner and the profile interval
    double clo = c_own, chi = c_own;
#pragma unroll
    for (int s = 0; s < kMom; ++s) { v[s] = 0.0; p[s] = ex[s]; }
    for (int i = i0; i < i1; ++i) {
      const double xi = xs[padded(i)], yi = ys[padded(i)];
      const double u = fmin(xi, th_c) / 100.0, r = (yi - th_a) - th_b * u;
      v[0] += u; v[1] += u * u; v[2] += xi > th_c ? 1.0 : 0.0; v[3] += r * r;
      const double z = xi / 100.0 - zbar, y = yi - ybar;
      p[0] += 1.0; p[1] += z; p[2] += y; p[3] += z * z; p[4] += z * y; p[5] += y * y;
      const int k = i + 1;
      const double xn = k < m ? xs[padded(k)] : INFINITY;
      if (!(xi < xn)) continue;
      v[4] += 1.0;
      double alpha, beta;
      bool constant;
      if (knot_sse(p, T, dm, z, xi > x_first, &alpha, &beta, &constant) <= thr) { clo = fmin(clo, xi); chi = fmax(chi, xi); }
    }
    double S[kMom], unused[kMom];
    block_scan(v, unused, S, ws);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      clo = fmin(clo, __shfl_xor(clo, o, 64));
      chi = fmax(chi, __shfl_xor(chi, o, 64));
    }
    if (lane == 0) { wlo[wave] = clo; whi[wave] = chi; }
    __syncthreads();

    if (threadIdx.x == 0) {
      for (int v2 = 0; v2 < kWaves; ++v2) { clo = fmin(clo, wlo[v2]); chi = fmax(chi, whi[v2]); }
      // outwards to the next current on either side: the profile crosses the threshold inside that gap
      int lo = 0, hi = m;
      while (lo < hi) {                                          // first row with x >= clo
        const int mid = (lo + hi) >> 1;
        if (xs[padded(mid)] < clo) lo = mid + 1; else hi = mid;
      }
      if (lo > 0) clo = xs[padded(lo - 1)];
      lo = 0; hi = m;
      while (lo < hi) {                                          // first row with x > chi
        const int mid = (lo + hi) >> 1;
        if (xs[padded(mid)] <= chi) lo = mid + 1; else hi = mid;
      }
      if (lo < m) chi = xs[padded(lo)];
      double out[PINN_BP_FIT_WORDS];
#pragma unroll
      for (int k = 0; k < PINN_BP_FIT_WORDS; ++k) out[k] = k < 9 ? nan : 0.0;
      out[0] = th_a; out[1] = th_b; out[2] = th_c;
      out[9] = S[3]; out[10] = (double)kind; out[11] = (double)kwin; out[12] = dm; out[13] = S[4];
      double alpha, beta;
      bool constant;
      double pm[kMom];
#pragma unroll
      for (int s = 0; s < kMom; ++s) pm[s] = T[s];
      out[15] = knot_sse(pm, T, dm, x_last / 100.0 - zbar, x_last > x_first, &alpha, &beta, &constant);
      out[16] = T[5] - T[2] * T[2] / dm;
      out[17] = clo; out[18] = chi; out[19] = x_first; out[20] = x_last;
      int status = 0;
      if (!(x_first < x_last)) {
        status = 7;
        out[2] = nan; out[17] = nan; out[18] = nan;
      } else {
        // the normal matrix; kind 2 takes the 2 x 2 block, the third row and column of the scaled matrix the identity's
        const double g = th_b / 100.0;
        const bool line = kind == 2;
        const double A22 = line ? 1.0 : (g * g) * S[2];
        if (!(S[1] > 0.0 && A22 > 0.0)) {
          status = 5;
        } else {
          const double sc[3] = {1.0 / sqrt(dm), 1.0 / sqrt(S[1]), 1.0 / sqrt(A22)};
          double C[6], L[6], zc[3];
          C[0] = 1.0; C[1] = (S[0] * sc[0]) * sc[1]; C[2] = 1.0;
          C[3] = line ? 0.0 : ((g * S[2]) * sc[0]) * sc[2];
          C[4] = line ? 0.0 : (((g * (th_c / 100.0)) * S[2]) * sc[1]) * sc[2];
          C[5] = 1.0;
          if (!chol3(C, kPivotMin, L)) {
            status = 5;
          } else {
            const double s2 = S[3] / (dm - (line ? 2.0 : 3.0));
#pragma unroll
            for (int qq = 0; qq < 3; ++qq) {       // column qq of C^-1, scaled back: s2 A^-1 = s2 S C^-1 S
              const double e[3] = {qq == 0 ? 1.0 : 0.0, qq == 1 ? 1.0 : 0.0, qq == 2 ? 1.0 : 0.0};
              chol3_solve(L, e, zc);
#pragma unroll
              for (int pp = 0; pp <= qq; ++pp) out[3 + tri(pp, qq)] = (line && qq == 2) ? nan : s2 * ((zc[pp] * sc[pp]) * sc[qq]);
            }
          }
        }
      }
      out[14] = (double)status;
#pragma unroll
      for (int k = 0; k < PINN_BP_FIT_WORDS; ++k) fr[k] = out[k];
    }
    __syncthreads();
  }
}

}  // namespace
}  // namespace pinn

using namespace pinn;

extern "C" int pinn_bp_fit(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, const long long* d_row_index,
                           long long n, const long long* d_win_start, const long long* d_win_len, long long n_windows,
                           long long max_window, const pinn_bp_opts_t* opts, double* d_fit, void* stream) {
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, 2, 1, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (n_windows < 0 || max_window < 0) return PINN_E_ARG;
  double q = kQDefault;
  if (opts) {
    if (!(opts->q > 0.0 && opts->q <= 1.7976931348623157e308) || opts->reserved != 0 || opts->reserved2 != 0) return PINN_E_ARG;
    q = opts->q;
  }
  if (misaligned8(d_win_start) || misaligned8(d_win_len) || misaligned8(d_fit)) return PINN_E_ARG;
  if (n_windows == 0) return PINN_OK;
  if (!d_win_start || !d_win_len || !d_fit) return PINN_E_ARG;
  int npad = 4;
  while (npad < max_window && npad < PINN_BP_MAX_WINDOW) npad <<= 1;
  const size_t lds = bp_lds_bytes(npad);
  clear_error();
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)bp_fit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  const int blocks = (int)(n_windows < kBpMaxBlocks ? n_windows : kBpMaxBlocks);
  hipLaunchKernelGGL(bp_fit_kernel, dim3(blocks), dim3(kThreads), lds, (hipStream_t)stream, a, d_win_start, d_win_len, n_windows, npad, q,
                     d_fit);
  return launch_status();
}
