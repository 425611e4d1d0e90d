// Temporal diagnosis on the device: a hidden Markov chain over the fault classes (include/pinn_hip.h)
//   pinn_hmm_forward_backward  filtered and smoothed posteriors, log-likelihood, expected transition counts
//   pinn_hmm_viterbi           the most probable state path
//   pinn_hmm_mstep             expected counts -> next transition matrix, convergence flag in the device model
// All arithmetic is float64.
//
// The forward pass is a prefix product of M_t = A diag(b_t), the backward pass a suffix product of the same matrices, the
// Viterbi scores a max-plus prefix product of log A + log b_t: three scans over (flag, S x S matrix, exponent) elements.
// A flag marks a segment start and discards everything on its far side.  After every product of the sum-product scans
// the matrix is scaled by an exact power of two (frexp / ldexp of its largest entry) and the exponent accumulated as a
// 64-bit integer, so the scaling rounds nothing.  Structure as pinn_risk.hip, reduce-then-scan: one launch reduces every
// 1024-row tile to one element, a one-workgroup launch turns them into the vector entering each tile (tile order, fixed),
// a third launch finishes each tile.  Stream order is the only dependency between workgroups.  A call of at most one tile
// is a single launch.
//
// Inside a tile: a workgroup is one wave, a thread takes 16 consecutive rows.  Only a *vector* has to enter a thread's run
// (S values), not a matrix, so no matrix scan is needed inside a tile: every thread multiplies its rows into one matrix
// (S^3 per row, in registers: 64 doubles = 128 VGPRs at S = 8, one wave per SIMD has 512), the 64 matrices meet in LDS
// (64 x 67 doubles = 34 KB, the odd stride keeps the b64 accesses of neighbouring lanes on different banks; four
// workgroups per CU, one per SIMD), and thread k carries the entering vector through matrices 0 .. k-1 (S^2 each, broadcast
// reads) before it walks its own rows with vector steps.  The reduce launch folds the 64 matrices by a fixed tree instead.
// S is padded to 2, 4 or 8 with zero rows and columns: a padded product adds exact zeros, so the bytes do not depend on it.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kThreads = 64;
constexpr int kRun = PINN_HMM_ROWS_PER_THREAD;
constexpr int kTile = PINN_HMM_TILE;
constexpr int kPart = 72;                       // words of a tile's partial counts: xi [8][8], then the gamma sums [8]
constexpr int kMIter = 0, kMConv = 1, kMPrev = 3, kMGain = 4;
constexpr int kMA = PINN_HMM_MODEL_A, kMP0 = PINN_HMM_MODEL_P0, kMIP = PINN_HMM_MODEL_INV_PRIOR, kMHist = PINN_HMM_HEADER;
constexpr unsigned kIdentityMap = 0x76543210u;
static_assert(kTile == kThreads * kRun, "a tile is one wave of runs");

struct Hmm {
  Rows rows;
  const double* model;
  const long long* ss;
  long long ns;
  const double* cin;
  int check, want_xi;
  double *alpha, *gamma, *loglik, *xi, *gsum, *cout;       // forward-backward outputs (alpha is never NULL in a kernel)
  long long* path;                                          // Viterbi outputs (loglik and cout as above)
  unsigned* words;                                          // backpointer maps [n]
  double *agg, *ent, *part;                                 // tile elements, entering vectors, partial counts
  unsigned *magg, *ment;                                    // tile maps and the state entering each tile from the right
  long long tiles;
};

__device__ __forceinline__ double ninf() { return __longlong_as_double(0xfff0000000000000LL); }

// the two semirings: (+, *) and (max, +); -inf + x = -inf and max(-inf, x) = x are IEEE's own rules (no +inf ever occurs)
template <bool MP> __device__ __forceinline__ double mul(double a, double b) { return MP ? a + b : a * b; }
template <bool MP> __device__ __forceinline__ double add(double a, double b) { return MP ? (b > a ? b : a) : a + b; }
template <bool MP> __device__ __forceinline__ double zero() { return MP ? ninf() : 0.0; }
template <bool MP> __device__ __forceinline__ double one() { return MP ? 0.0 : 1.0; }
__device__ __forceinline__ double log0(double x) { return x > 0.0 ? log(x) : ninf(); }

template <int SP> struct Dim {
  static constexpr int kMat = SP * SP, kElem = 2 + SP * SP, kStride = (2 + SP * SP) | 1;      // words; [0] flag, [1] exponent
};

// scale by the power of two that brings the largest entry into [0.5, 1); returns the exponent taken out
template <int N> __device__ __forceinline__ int renorm(double* v) {
  double mx = 0.0;
#pragma unroll
  for (int x = 0; x < N; ++x) mx = v[x] > mx ? v[x] : mx;
  if (!(mx > 0.0)) return 0;
  int ex;
  (void)frexp(mx, &ex);
#pragma unroll
  for (int x = 0; x < N; ++x) v[x] = ldexp(v[x], -ex);
  return ex;
}

// q <- q R, R [SP][SP] anywhere
template <int SP, bool MP> __device__ __forceinline__ void mul_right(double* q, const double* R) {
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    double row[SP];
#pragma unroll
    for (int k = 0; k < SP; ++k) row[k] = q[i * SP + k];
#pragma unroll
    for (int c = 0; c < SP; ++c) {
      double acc = zero<MP>();
#pragma unroll
      for (int k = 0; k < SP; ++k) acc = add<MP>(acc, mul<MP>(row[k], R[k * SP + c]));
      q[i * SP + c] = acc;
    }
  }
}

// u <- u R (a row vector)
template <int SP, bool MP> __device__ __forceinline__ void vec_right(double* u, const double* R) {
  double row[SP];
#pragma unroll
  for (int k = 0; k < SP; ++k) row[k] = u[k];
#pragma unroll
  for (int c = 0; c < SP; ++c) {
    double acc = zero<MP>();
#pragma unroll
    for (int k = 0; k < SP; ++k) acc = add<MP>(acc, mul<MP>(row[k], R[k * SP + c]));
    u[c] = acc;
  }
}

// u <- R u (a column vector), sum-product only
template <int SP> __device__ __forceinline__ void vec_left(double* u, const double* R) {
  double col[SP];
#pragma unroll
  for (int k = 0; k < SP; ++k) col[k] = u[k];
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < SP; ++k) acc += R[i * SP + k] * col[k];
    u[i] = acc;
  }
}

// A (or log A), p0 (or log p0) and 1 / prior into LDS, padded with the semiring's zero
template <int SP, bool MP> __device__ __forceinline__ void load_model(const double* __restrict__ model, int S, double* sA, double* sp0, double* sip) {
  for (int q = threadIdx.x; q < SP * SP; q += kThreads) {
    const int i = q / SP, c = q % SP;
    const double a = (i < S && c < S) ? model[kMA + i * PINN_HMM_MAX_STATES + c] : 0.0;
    sA[q] = MP ? log0(a) : a;
  }
  if (threadIdx.x < SP) {
    const int i = threadIdx.x;
    const double p = i < S ? model[kMP0 + i] : 0.0;
    sp0[i] = MP ? log0(p) : p;
    sip[i] = i < S ? model[kMIP + i] : 0.0;
  }
  __syncthreads();
}

// emissions of position j (their logarithms under max-plus); a missing row is all ones
template <int SP, bool MP> __device__ __forceinline__ void load_b(const Rows& a, long long j, const double* sip, double* b) {
  double x[kRowsMaxD];
  const bool ok = load_row(a, j, x);
  bool bad = !ok, any = false;
#pragma unroll
  for (int i = 0; i < SP; ++i) {
    const double v = i < a.D ? x[i] * sip[i] : 0.0;
    b[i] = v;
    if (i < a.D) {
      bad = bad || !(v >= 0.0) || v > 1.7976931348623157e308;
      any = any || v > 0.0;
    }
  }
  if (bad || !any) {
#pragma unroll
    for (int i = 0; i < SP; ++i) b[i] = i < a.D ? 1.0 : 0.0;
  }
  if (MP) {
#pragma unroll
    for (int i = 0; i < SP; ++i) b[i] = log0(b[i]);
  }
}

// The segment starts among a thread's rows.  Bit k: position j0 + k begins a segment (k = kRun: the first position after
// the run); seg0: the segment of position j0.
struct Run {
  unsigned starts;
  long long seg0;
};

__device__ __forceinline__ Run make_run(const long long* __restrict__ ss, long long ns, long long j0, long long n) {
  Run r;
  r.starts = 0;
  r.seg0 = 0;
  if (j0 >= n) return r;
  long long s = seg_of(ss, ns, j0);
  r.seg0 = s;
  if (seg_begin(ss, s) == j0) r.starts |= 1u;
  long long next = seg_next(ss, ns, s, n);
  for (int k = 1; k <= kRun; ++k) {
    const long long j = j0 + k;
    if (j < n && j == next) {
      r.starts |= 1u << k;
      ++s;
      next = seg_next(ss, ns, s, n);
    }
  }
  return r;
}

__device__ __forceinline__ bool run_start(const Run& r, int k) { return (r.starts >> k) & 1u; }
__device__ __forceinline__ long long run_seg(const Run& r, int k) { return r.seg0 + __popc(r.starts & ((2u << k) - 1u) & ~1u); }

// the state after the first position of segment s, before scaling: p0 o b, or (carry A) o b
template <int SP, bool MP> __device__ __forceinline__ void start_vec(const Hmm& h, const double* sA, const double* sp0, long long s,
                                                                      const double* b, double* v) {
  const int S = h.rows.D;
  if (!h.cin) {
#pragma unroll
    for (int c = 0; c < SP; ++c) v[c] = mul<MP>(sp0[c], b[c]);
    return;
  }
  const double* cr = h.cin + s * (2 * S + 1) + (MP ? S + 1 : 0);
  double u[SP];
#pragma unroll
  for (int i = 0; i < SP; ++i) u[i] = i < S ? cr[i] : zero<MP>();
  vec_right<SP, MP>(u, sA);
#pragma unroll
  for (int c = 0; c < SP; ++c) v[c] = mul<MP>(u[c], b[c]);
}

// The product of a thread's rows as one element.  Forward (BWD = false): "rows in time order", a segment start replaces
// everything before it by the constant map to its start vector (all rows of q equal).  Backward: the same product read as
// beta_{j0 - 1} = q beta_{j0 + kRun - 1}; a segment start at t makes beta_{t-1} = 1 whatever lies to its right, so q becomes
// its row sums in every column and stays as it is.
template <int SP, bool MP, bool BWD>
__device__ __forceinline__ void thread_element(const Hmm& h, const double* sA, const double* sp0, const double* sip, long long j0,
                                               const Run& run, double* q, long long* f_out, long long* e_out) {
  long long f = 0, e = 0;
#pragma unroll
  for (int x = 0; x < SP * SP; ++x) q[x] = (x / SP == x % SP) ? one<MP>() : zero<MP>();
#pragma unroll 1
  for (int k = 0; k < kRun; ++k) {
    const long long j = j0 + k;
    if (j >= h.rows.n || (BWD && f)) break;
    const bool st = run_start(run, k);
    if (BWD && st) {
#pragma unroll
      for (int i = 0; i < SP; ++i) {
        double r = 0.0;
#pragma unroll
        for (int c = 0; c < SP; ++c) r += q[i * SP + c];
#pragma unroll
        for (int c = 0; c < SP; ++c) q[i * SP + c] = r;
      }
      f = 1;
    } else {
      double b[SP];
      load_b<SP, MP>(h.rows, j, sip, b);
      if (st) {
        double v[SP];
        start_vec<SP, MP>(h, sA, sp0, run_seg(run, k), b, v);
#pragma unroll
        for (int x = 0; x < SP * SP; ++x) q[x] = v[x % SP];
        f = 1;
        e = 0;
      } else {
        mul_right<SP, MP>(q, sA);
#pragma unroll
        for (int x = 0; x < SP * SP; ++x) q[x] = mul<MP>(q[x], b[x % SP]);
      }
    }
    if (!MP) e += renorm<SP * SP>(q);
  }
  *f_out = f;
  *e_out = e;
}

template <int SP> __device__ __forceinline__ void put_element(double* dst, const double* q, long long f, long long e) {
  dst[0] = __longlong_as_double(f);
  dst[1] = __longlong_as_double(e);
#pragma unroll
  for (int x = 0; x < SP * SP; ++x) dst[2 + x] = q[x];
}

// L <- "L, then R" (L in LDS, R in LDS or in the workspace), the flag rule of its direction
template <int SP, bool MP, bool BWD> __device__ __forceinline__ void lds_combine(double* L, const double* R) {
  const long long lf = __double_as_longlong(L[0]), rf = __double_as_longlong(R[0]);
  if (!BWD && rf) {
    for (int x = 0; x < Dim<SP>::kElem; ++x) L[x] = R[x];
    return;
  }
  if (BWD && lf) return;
  double q[SP * SP];
#pragma unroll
  for (int x = 0; x < SP * SP; ++x) q[x] = L[2 + x];
  mul_right<SP, MP>(q, R + 2);
  long long e = __double_as_longlong(L[1]) + __double_as_longlong(R[1]);
  if (!MP) e += renorm<SP * SP>(q);
  put_element<SP>(L, q, BWD ? rf : lf, e);
}

// the workgroup's element from its threads' elements in LDS, by a fixed tree; left in slot 0
template <int SP, bool MP, bool BWD> __device__ __forceinline__ void tile_fold(double* s_el) {
  __syncthreads();
  for (int d = 1; d < kThreads; d <<= 1) {
    if ((threadIdx.x & (2 * d - 1)) == 0) lds_combine<SP, MP, BWD>(s_el + threadIdx.x * Dim<SP>::kStride, s_el + (threadIdx.x + d) * Dim<SP>::kStride);
    __syncthreads();
  }
}

// one element applied to the vector entering it: forward u <- u M, backward u <- M u
template <int SP, bool MP, bool BWD> __device__ __forceinline__ void apply(const double* el, double* u, long long* e) {
  const long long f = __double_as_longlong(el[0]);
  if (f) {
#pragma unroll
    for (int c = 0; c < SP; ++c) u[c] = BWD ? el[2 + c * SP] : el[2 + c];       // any column / any row of a constant map
    *e = __double_as_longlong(el[1]);
    return;
  }
  if (BWD) vec_left<SP>(u, el + 2); else vec_right<SP, MP>(u, el + 2);
  *e += __double_as_longlong(el[1]);
  if (!MP) *e += renorm<SP>(u);
}

// the vector entering thread k's run from the one entering the workgroup's: through the elements before (after) it in LDS
template <int SP, bool MP, bool BWD> __device__ __forceinline__ void thread_entering(const double* s_el, double* u, long long* e) {
  __syncthreads();
#pragma unroll 1
  for (int q = 0; q < kThreads - 1; ++q) {
    const int k = BWD ? kThreads - 1 - q : q;
    if (BWD ? k > (int)threadIdx.x : k < (int)threadIdx.x) apply<SP, MP, BWD>(s_el + k * Dim<SP>::kStride, u, e);
  }
}

__device__ __forceinline__ int lowest_argmax(const double* u, int S) {
  int arg = 0;
  double best = ninf();
  for (int i = 0; i < S; ++i)
    if (u[i] > best) { best = u[i]; arg = i; }
  return arg;
}

// ---- forward: filtered distributions, log-likelihood and carry, from the vector entering the thread's run
template <int SP> __device__ __forceinline__ void forward_walk(const Hmm& h, const double* sA, const double* sp0, const double* sip,
                                                                long long j0, const Run& run, double* u, long long e) {
  const int S = h.rows.D;
  const long long n = h.rows.n;
#pragma unroll 1
  for (int k = 0; k < kRun; ++k) {
    const long long j = j0 + k;
    if (j >= n) break;
    double b[SP];
    load_b<SP, false>(h.rows, j, sip, b);
    if (run_start(run, k)) {
      start_vec<SP, false>(h, sA, sp0, run_seg(run, k), b, u);
      e = 0;
    } else {
      vec_right<SP, false>(u, sA);
#pragma unroll
      for (int c = 0; c < SP; ++c) u[c] *= b[c];
    }
    e += renorm<SP>(u);
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < SP; ++c) sum += u[c];
    double* out = h.alpha + j * S;
#pragma unroll
    for (int c = 0; c < SP; ++c)
      if (c < S) out[c] = u[c] / sum;
    if (run_start(run, k + 1) || j + 1 == n) {                 // the last position of its segment
      const long long s = run_seg(run, k);
      const int cs = 2 * S + 1;
      const double L = (double)e * 0.6931471805599453 + log(sum) + (h.cin ? h.cin[s * cs + S] : 0.0);
      if (h.loglik) h.loglik[s] = L;
      if (h.cout) {
#pragma unroll
        for (int c = 0; c < SP; ++c)
          if (c < S) h.cout[s * cs + c] = u[c] / sum;
        h.cout[s * cs + S] = L;
      }
    }
  }
}

// ---- backward: smoothed distributions and the thread's share of the expected counts, from beta of its last row
template <int SP> __device__ __forceinline__ void backward_walk(const Hmm& h, const double* sA, const double* sip, long long j0,
                                                                 const Run& run, double* u, double* acc, double* gs) {
  const int S = h.rows.D;
  const long long n = h.rows.n;
#pragma unroll 1
  for (int k = kRun - 1; k >= 0; --k) {
    const long long j = j0 + k;
    if (j >= n) continue;
    const bool st = run_start(run, k), last = run_start(run, k + 1) || j + 1 == n;
    double g[SP], sum = 0.0;
#pragma unroll
    for (int c = 0; c < SP; ++c) {
      g[c] = c < S ? h.alpha[j * S + c] * u[c] : 0.0;
      sum += g[c];
    }
#pragma unroll
    for (int c = 0; c < SP; ++c) {
      g[c] = g[c] / sum;
      if (h.gamma && c < S) h.gamma[j * S + c] = g[c];
      if (!last) gs[c] += g[c];
    }
    if (st) {
#pragma unroll
      for (int c = 0; c < SP; ++c) u[c] = c < S ? 1.0 : 0.0;
      continue;
    }
    double b[SP], w[SP], ap[SP];
    load_b<SP, false>(h.rows, j, sip, b);
#pragma unroll
    for (int c = 0; c < SP; ++c) {
      w[c] = b[c] * u[c];
      u[c] = w[c];
      ap[c] = c < S ? h.alpha[(j - 1) * S + c] : 0.0;         // j > 0: position 0 begins a segment
    }
    vec_left<SP>(u, sA);                                        // beta of j - 1, before scaling
    if (h.want_xi) {
      double tot = 0.0;
#pragma unroll
      for (int i = 0; i < SP; ++i) tot += ap[i] * u[i];
      const double inv = 1.0 / tot;
#pragma unroll
      for (int i = 0; i < SP; ++i) {
        const double ai = ap[i] * inv;
#pragma unroll
        for (int c = 0; c < SP; ++c) acc[i * SP + c] += ai * (sA[i * SP + c] * w[c]);
      }
    }
    (void)renorm<SP>(u);
  }
}

// the workgroup's counts from its threads', in thread order: to `part` ([8][8] then [8] words, a tile's partial) when it is
// given, else to the call's own outputs
template <int SP> __device__ __forceinline__ void tile_counts(const Hmm& h, const double* acc, const double* gs, double* s_el, double* s_gs,
                                                               double* part) {
  const int S = h.rows.D;
  __syncthreads();                                 // the elements in s_el are done with
#pragma unroll
  for (int x = 0; x < SP * SP; ++x) s_el[threadIdx.x * Dim<SP>::kStride + x] = acc[x];
#pragma unroll
  for (int c = 0; c < SP; ++c) s_gs[threadIdx.x * (SP + 1) + c] = gs[c];
  __syncthreads();
  const int x = threadIdx.x;
  if (x < SP * SP) {
    double v = 0.0;
    for (int t = 0; t < kThreads; ++t) v += s_el[t * Dim<SP>::kStride + x];
    const int i = x / SP, c = x % SP;
    if (part) part[i * PINN_HMM_MAX_STATES + c] = v;
    else if (h.xi && i < S && c < S) h.xi[i * S + c] = v;
  }
  if (x < SP) {
    double v = 0.0;
    for (int t = 0; t < kThreads; ++t) v += s_gs[t * (SP + 1) + x];
    if (part) part[64 + x] = v;
    else if (h.gsum && x < S) h.gsum[x] = v;
  }
}

#define HMM_SHARED(SP)                                                  \
  __shared__ double s_el[kThreads * Dim<SP>::kStride];                 \
  __shared__ double sA[SP * SP], sp0[SP], sip[SP]

__device__ __forceinline__ bool skip(const Hmm& h) { return h.check && h.model[kMConv] != 0.0; }

// n <= kTile: one workgroup, one launch
template <int SP> __global__ __launch_bounds__(kThreads) void fb_single_kernel(Hmm h, int backward) {
  HMM_SHARED(SP);
  __shared__ double s_gs[kThreads * (SP + 1)];
  if (skip(h)) return;
  load_model<SP, false>(h.model, h.rows.D, sA, sp0, sip);
  const long long j0 = (long long)threadIdx.x * kRun;
  const Run run = make_run(h.ss, h.ns, j0, h.rows.n);
  double q[SP * SP], u[SP];
  long long f, e;
  thread_element<SP, false, false>(h, sA, sp0, sip, j0, run, q, &f, &e);
  put_element<SP>(s_el + threadIdx.x * Dim<SP>::kStride, q, f, e);
#pragma unroll
  for (int c = 0; c < SP; ++c) u[c] = 1.0;         // position 0 begins a segment: never reaches a result
  e = 0;
  thread_entering<SP, false, false>(s_el, u, &e);
  forward_walk<SP>(h, sA, sp0, sip, j0, run, u, e);
  if (!backward) return;
  __syncthreads();                                 // alpha of every row is written, the forward elements are done with
  thread_element<SP, false, true>(h, sA, sp0, sip, j0, run, q, &f, &e);
  put_element<SP>(s_el + threadIdx.x * Dim<SP>::kStride, q, f, e);
#pragma unroll
  for (int c = 0; c < SP; ++c) u[c] = c < h.rows.D ? 1.0 : 0.0;
  thread_entering<SP, false, true>(s_el, u, &e);
  double gs[SP];
#pragma unroll
  for (int x = 0; x < SP * SP; ++x) q[x] = 0.0;
#pragma unroll
  for (int c = 0; c < SP; ++c) gs[c] = 0.0;
  backward_walk<SP>(h, sA, sip, j0, run, u, q, gs);
  if (h.want_xi) tile_counts<SP>(h, q, gs, s_el, s_gs, nullptr);
}

// launch 1 of a scan: every tile's element
template <int SP, bool MP, bool BWD> __global__ __launch_bounds__(kThreads) void reduce_kernel(Hmm h) {
  HMM_SHARED(SP);
  if (skip(h)) return;
  load_model<SP, MP>(h.model, h.rows.D, sA, sp0, sip);
  const long long j0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kRun;
  const Run run = make_run(h.ss, h.ns, j0, h.rows.n);
  double q[SP * SP];
  long long f, e;
  thread_element<SP, MP, BWD>(h, sA, sp0, sip, j0, run, q, &f, &e);
  put_element<SP>(s_el + threadIdx.x * Dim<SP>::kStride, q, f, e);
  tile_fold<SP, MP, BWD>(s_el);
  for (int x = threadIdx.x; x < Dim<SP>::kElem; x += kThreads) h.agg[(long long)blockIdx.x * Dim<SP>::kElem + x] = s_el[x];
}

// launch 2: the vector entering every tile (from the left, or from the right), tile order; each thread a run of tiles
template <int SP, bool MP, bool BWD> __global__ __launch_bounds__(kThreads) void carry_kernel(Hmm h) {
  __shared__ double s_el[kThreads * Dim<SP>::kStride];
  if (skip(h)) return;
  const long long chunk = (h.tiles + kThreads - 1) / kThreads;
  const long long t0 = (long long)threadIdx.x * chunk;
  const long long t1 = t0 + chunk < h.tiles ? t0 + chunk : h.tiles;
  double* mine = s_el + threadIdx.x * Dim<SP>::kStride;
  mine[0] = __longlong_as_double(0);
  mine[1] = __longlong_as_double(0);
  for (int x = 0; x < SP * SP; ++x) mine[2 + x] = (x / SP == x % SP) ? one<MP>() : zero<MP>();
  for (long long t = t0; t < t1; ++t) lds_combine<SP, MP, BWD>(mine, h.agg + t * Dim<SP>::kElem);
  double u[SP];
  long long e = 0;
#pragma unroll
  for (int c = 0; c < SP; ++c) u[c] = (!MP && c >= h.rows.D) ? 0.0 : one<MP>();
  thread_entering<SP, MP, BWD>(s_el, u, &e);
  for (long long q = 0; q < t1 - t0; ++q) {
    const long long t = BWD ? t1 - 1 - q : t0 + q;
    double* o = h.ent + t * (SP + 1);
    o[0] = __longlong_as_double(e);
#pragma unroll
    for (int c = 0; c < SP; ++c) o[1 + c] = u[c];
    apply<SP, MP, BWD>(h.agg + t * Dim<SP>::kElem, u, &e);
  }
}

// launch 3, forward
template <int SP> __global__ __launch_bounds__(kThreads) void fwd_finish_kernel(Hmm h) {
  HMM_SHARED(SP);
  if (skip(h)) return;
  load_model<SP, false>(h.model, h.rows.D, sA, sp0, sip);
  const long long j0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kRun;
  const Run run = make_run(h.ss, h.ns, j0, h.rows.n);
  double q[SP * SP], u[SP];
  long long f, e;
  thread_element<SP, false, false>(h, sA, sp0, sip, j0, run, q, &f, &e);
  put_element<SP>(s_el + threadIdx.x * Dim<SP>::kStride, q, f, e);
  const double* in = h.ent + (long long)blockIdx.x * (SP + 1);
  e = __double_as_longlong(in[0]);
#pragma unroll
  for (int c = 0; c < SP; ++c) u[c] = in[1 + c];
  thread_entering<SP, false, false>(s_el, u, &e);
  forward_walk<SP>(h, sA, sp0, sip, j0, run, u, e);
}

// launch 3, backward
template <int SP> __global__ __launch_bounds__(kThreads) void bwd_finish_kernel(Hmm h) {
  HMM_SHARED(SP);
  __shared__ double s_gs[kThreads * (SP + 1)];
  if (skip(h)) return;
  load_model<SP, false>(h.model, h.rows.D, sA, sp0, sip);
  const long long j0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kRun;
  const Run run = make_run(h.ss, h.ns, j0, h.rows.n);
  double q[SP * SP], u[SP], gs[SP];
  long long f, e;
  thread_element<SP, false, true>(h, sA, sp0, sip, j0, run, q, &f, &e);
  put_element<SP>(s_el + threadIdx.x * Dim<SP>::kStride, q, f, e);
  const double* in = h.ent + (long long)blockIdx.x * (SP + 1);
#pragma unroll
  for (int c = 0; c < SP; ++c) u[c] = in[1 + c];
  thread_entering<SP, false, true>(s_el, u, &e);
#pragma unroll
  for (int x = 0; x < SP * SP; ++x) q[x] = 0.0;
#pragma unroll
  for (int c = 0; c < SP; ++c) gs[c] = 0.0;
  backward_walk<SP>(h, sA, sip, j0, run, u, q, gs);
  if (h.want_xi) tile_counts<SP>(h, q, gs, s_el, s_gs, h.part + (long long)blockIdx.x * kPart);
}

// the tiles' partial counts summed in tile order
__global__ __launch_bounds__(kThreads) void counts_kernel(Hmm h) {
  if (skip(h)) return;
  const int S = h.rows.D;
  for (int x = threadIdx.x; x < kPart; x += kThreads) {
    double v = 0.0;
    for (long long t = 0; t < h.tiles; ++t) v += h.part[t * kPart + x];
    if (x < 64) {
      const int i = x / PINN_HMM_MAX_STATES, c = x % PINN_HMM_MAX_STATES;
      if (h.xi && i < S && c < S) h.xi[i * S + c] = v;
    } else if (h.gsum && x - 64 < S) {
      h.gsum[x - 64] = v;
    }
  }
}

// ---- Viterbi: scores, backpointer maps, then the path as a suffix composition of the maps
__device__ __forceinline__ unsigned map_const(int s) { return 0x11111111u * (unsigned)s; }
__device__ __forceinline__ int map_at(unsigned m, int s) { return (m >> (4 * s)) & 15u; }
__device__ __forceinline__ unsigned map_compose(unsigned f, unsigned g) {       // s -> f(g(s))
  unsigned o = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) o |= (unsigned)map_at(f, map_at(g, s)) << (4 * s);
  return o;
}

// words[j] maps the state at j + 1 to the state at j (a constant at the last position of a segment)
template <int SP> __device__ __forceinline__ void viterbi_walk(const Hmm& h, const double* sA, const double* sp0, const double* sip,
                                                                long long j0, const Run& run, double* u) {
  const int S = h.rows.D;
  const long long n = h.rows.n;
#pragma unroll 1
  for (int k = 0; k < kRun; ++k) {
    const long long j = j0 + k;
    if (j >= n) break;
    double b[SP];
    load_b<SP, true>(h.rows, j, sip, b);
    if (run_start(run, k)) {
      if (j > 0) h.words[j - 1] = map_const(lowest_argmax(u, S));
      start_vec<SP, true>(h, sA, sp0, run_seg(run, k), b, u);
    } else {
      double nu[SP];
      unsigned word = 0;
#pragma unroll
      for (int c = 0; c < SP; ++c) {
        double best = ninf();
        int arg = 0;
#pragma unroll
        for (int i = 0; i < SP; ++i) {
          const double v = u[i] + sA[i * SP + c];
          if (v > best) { best = v; arg = i; }
        }
        nu[c] = best + b[c];
        word |= (unsigned)arg << (4 * c);
      }
#pragma unroll
      for (int c = 0; c < SP; ++c) u[c] = nu[c];
      h.words[j - 1] = word;                                    // j > 0: position 0 begins a segment
    }
    if (j + 1 == n) h.words[j] = map_const(lowest_argmax(u, S));
    if (run_start(run, k + 1) || j + 1 == n) {
      const long long s = run_seg(run, k);
      const int cs = 2 * S + 1;
      if (h.loglik) h.loglik[s] = u[lowest_argmax(u, S)];
      if (h.cout)
        for (int c = 0; c < S; ++c) h.cout[s * cs + S + 1 + c] = u[c];
    }
  }
}

// the path of a tile from the state entering it from the right; words and path in global memory, the threads' maps in LDS
__device__ __forceinline__ unsigned thread_map(const Hmm& h, long long j0) {
  unsigned m = kIdentityMap;
  for (int k = 0; k < kRun; ++k)
    if (j0 + k < h.rows.n) m = map_compose(m, h.words[j0 + k]);
  return m;
}

__device__ __forceinline__ void path_walk(const Hmm& h, long long j0, const unsigned* s_map, int state) {
  __syncthreads();
  for (int k = kThreads - 1; k > (int)threadIdx.x; --k) state = map_at(s_map[k], state);
  for (int k = kRun - 1; k >= 0; --k) {
    const long long j = j0 + k;
    if (j >= h.rows.n) continue;
    state = map_at(h.words[j], state);
    h.path[j] = state;
  }
}

template <int SP> __global__ __launch_bounds__(kThreads) void viterbi_single_kernel(Hmm h) {
  HMM_SHARED(SP);
  __shared__ unsigned s_map[kThreads];
  load_model<SP, true>(h.model, h.rows.D, sA, sp0, sip);
  const long long j0 = (long long)threadIdx.x * kRun;
  const Run run = make_run(h.ss, h.ns, j0, h.rows.n);
  double q[SP * SP], u[SP];
  long long f, e = 0;
  thread_element<SP, true, false>(h, sA, sp0, sip, j0, run, q, &f, &e);
  put_element<SP>(s_el + threadIdx.x * Dim<SP>::kStride, q, f, e);
#pragma unroll
  for (int c = 0; c < SP; ++c) u[c] = 0.0;
  thread_entering<SP, true, false>(s_el, u, &e);
  viterbi_walk<SP>(h, sA, sp0, sip, j0, run, u);
  __syncthreads();                                 // every word is written
  s_map[threadIdx.x] = thread_map(h, j0);
  path_walk(h, j0, s_map, 0);
}

template <int SP> __global__ __launch_bounds__(kThreads) void viterbi_finish_kernel(Hmm h) {
  HMM_SHARED(SP);
  load_model<SP, true>(h.model, h.rows.D, sA, sp0, sip);
  const long long j0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kRun;
  const Run run = make_run(h.ss, h.ns, j0, h.rows.n);
  double q[SP * SP], u[SP];
  long long f, e = 0;
  thread_element<SP, true, false>(h, sA, sp0, sip, j0, run, q, &f, &e);
  put_element<SP>(s_el + threadIdx.x * Dim<SP>::kStride, q, f, e);
  const double* in = h.ent + (long long)blockIdx.x * (SP + 1);
#pragma unroll
  for (int c = 0; c < SP; ++c) u[c] = in[1 + c];
  thread_entering<SP, true, false>(s_el, u, &e);
  viterbi_walk<SP>(h, sA, sp0, sip, j0, run, u);
}

__global__ __launch_bounds__(kThreads) void map_reduce_kernel(Hmm h) {
  __shared__ unsigned s_map[kThreads];
  const long long j0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kRun;
  s_map[threadIdx.x] = thread_map(h, j0);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned m = kIdentityMap;
    for (int k = 0; k < kThreads; ++k) m = map_compose(m, s_map[k]);
    h.magg[blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(kThreads) void map_carry_kernel(Hmm h) {
  __shared__ unsigned s_map[kThreads];
  const long long chunk = (h.tiles + kThreads - 1) / kThreads;
  const long long t0 = (long long)threadIdx.x * chunk;
  const long long t1 = t0 + chunk < h.tiles ? t0 + chunk : h.tiles;
  unsigned m = kIdentityMap;
  for (long long t = t0; t < t1; ++t) m = map_compose(m, h.magg[t]);
  s_map[threadIdx.x] = m;
  __syncthreads();
  int state = 0;                                   // the last word of the series is a constant: this 0 never reaches a result
  for (int k = kThreads - 1; k > (int)threadIdx.x; --k) state = map_at(s_map[k], state);
  for (long long t = t1 - 1; t >= t0; --t) {
    h.ment[t] = (unsigned)state;
    state = map_at(h.magg[t], state);
  }
}

__global__ __launch_bounds__(kThreads) void map_finish_kernel(Hmm h) {
  __shared__ unsigned s_map[kThreads];
  const long long j0 = (long long)blockIdx.x * kTile + (long long)threadIdx.x * kRun;
  s_map[threadIdx.x] = thread_map(h, j0);
  path_walk(h, j0, s_map, (int)h.ment[blockIdx.x]);
}

// ---- M-step: one workgroup
__global__ __launch_bounds__(kThreads) void mstep_kernel(double* __restrict__ model, int S, const double* __restrict__ xi,
                                                          const double* __restrict__ loglik, long long ns,
                                                          const double* __restrict__ pseudo, double tol, int max_hist) {
  const bool done = model[kMConv] != 0.0;
  __syncthreads();                                 // every thread has read the flag before thread 0 may set it
  if (done) return;
  const int i = threadIdx.x;
  if (i < S) {
    double* row = model + kMA + i * PINN_HMM_MAX_STATES;
    double cnt[PINN_HMM_MAX_STATES], tot = 0.0;
    for (int j = 0; j < S; ++j) {
      cnt[j] = row[j] > 0.0 ? xi[i * S + j] + (pseudo ? pseudo[i * S + j] : 0.0) : 0.0;
      tot += cnt[j];
    }
    if (tot > 0.0)
      for (int j = 0; j < S; ++j) row[j] = cnt[j] / tot;
  }
  if (i == 0) {
    double L = 0.0;
    for (long long s = 0; s < ns; ++s) L += loglik[s];
    const long long it = (long long)model[kMIter];
    const double gain = L - model[kMPrev];
    if (it < max_hist) model[kMHist + it] = L;
    if (it > 0 && fabs(gain) < tol) model[kMConv] = 1.0;
    model[kMGain] = it > 0 ? gain : 0.0;
    model[kMPrev] = L;
    model[kMIter] = (double)(it + 1);
  }
}

inline int padded(int S) { return S <= 2 ? 2 : (S <= 4 ? 4 : 8); }

struct Layout {
  size_t alpha, agg, ent, part, words, magg, ment, total;
};

inline Layout layout_of(long long n, int S) {
  const size_t SP = (size_t)padded(S), tiles = (size_t)((n + kTile - 1) / kTile);
  Layout L;
  size_t o = 0;
  L.alpha = o; o += align256((size_t)n * S * sizeof(double));
  L.agg = o; o += align256(tiles * (2 + SP * SP) * sizeof(double));
  L.ent = o; o += align256(tiles * (SP + 1) * sizeof(double));
  L.part = o; o += align256(tiles * kPart * sizeof(double));
  L.words = o; o += align256((size_t)n * sizeof(unsigned));
  L.magg = o; o += align256(tiles * sizeof(unsigned));
  L.ment = o; o += align256(tiles * sizeof(unsigned));
  L.total = o;
  return L;
}

// the checks every scan entry point shares; fills h except its outputs
inline int make_hmm(const double* d_arr, long long ld, long long n_arr, const int* cols, int S, const long long* ridx, long long n,
                    const double* d_model, const long long* d_seg, long long n_seg, const double* d_cin, void* d_ws, size_t ws_bytes,
                    Hmm* h) {
  const int rc = make_rows(d_arr, ld, n_arr, cols, S, 1, ridx, n, &h->rows);
  if (rc != PINN_OK) return rc;
  if (!d_model || n_seg < 0 || (n_seg > 0 && !d_seg)) return PINN_E_ARG;
  if (misaligned8(d_model) || misaligned8(d_seg) || misaligned8(d_cin) || misaligned8(d_ws)) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  if (!d_ws) return PINN_E_ARG;
  const Layout L = layout_of(n, S);
  if (ws_bytes < L.total) return PINN_E_WORKSPACE;
  if ((n + kTile - 1) / kTile > 0x7fffffffLL) return PINN_E_ARG;
  char* w = static_cast<char*>(d_ws);
  h->model = d_model; h->ss = n_seg > 0 ? d_seg : nullptr; h->ns = n_seg > 0 ? n_seg : 1; h->cin = d_cin;
  h->check = 0; h->want_xi = 0;
  h->alpha = reinterpret_cast<double*>(w + L.alpha); h->gamma = nullptr; h->loglik = nullptr; h->xi = nullptr; h->gsum = nullptr;
  h->cout = nullptr; h->path = nullptr;
  h->words = reinterpret_cast<unsigned*>(w + L.words);
  h->agg = reinterpret_cast<double*>(w + L.agg); h->ent = reinterpret_cast<double*>(w + L.ent);
  h->part = reinterpret_cast<double*>(w + L.part);
  h->magg = reinterpret_cast<unsigned*>(w + L.magg); h->ment = reinterpret_cast<unsigned*>(w + L.ment);
  h->tiles = (n + kTile - 1) / kTile;
  return PINN_OK;
}

template <int SP> void launch_forward_backward(const Hmm& h, bool backward, hipStream_t st) {
  const dim3 block(kThreads), single(1), grid((unsigned)h.tiles);
  if (h.tiles == 1) {
    hipLaunchKernelGGL(fb_single_kernel<SP>, single, block, 0, st, h, backward ? 1 : 0);
    return;
  }
  hipLaunchKernelGGL((reduce_kernel<SP, false, false>), grid, block, 0, st, h);
  hipLaunchKernelGGL((carry_kernel<SP, false, false>), single, block, 0, st, h);
  hipLaunchKernelGGL(fwd_finish_kernel<SP>, grid, block, 0, st, h);
  if (!backward) return;
  hipLaunchKernelGGL((reduce_kernel<SP, false, true>), grid, block, 0, st, h);
  hipLaunchKernelGGL((carry_kernel<SP, false, true>), single, block, 0, st, h);
  hipLaunchKernelGGL(bwd_finish_kernel<SP>, grid, block, 0, st, h);
  if (h.want_xi) hipLaunchKernelGGL(counts_kernel, single, block, 0, st, h);
}

template <int SP> void launch_viterbi(const Hmm& h, hipStream_t st) {
  const dim3 block(kThreads), single(1), grid((unsigned)h.tiles);
  if (h.tiles == 1) {
    hipLaunchKernelGGL(viterbi_single_kernel<SP>, single, block, 0, st, h);
    return;
  }
  hipLaunchKernelGGL((reduce_kernel<SP, true, false>), grid, block, 0, st, h);
  hipLaunchKernelGGL((carry_kernel<SP, true, false>), single, block, 0, st, h);
  hipLaunchKernelGGL(viterbi_finish_kernel<SP>, grid, block, 0, st, h);
  hipLaunchKernelGGL(map_reduce_kernel, grid, block, 0, st, h);
  hipLaunchKernelGGL(map_carry_kernel, single, block, 0, st, h);
  hipLaunchKernelGGL(map_finish_kernel, grid, block, 0, st, h);
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_hmm_workspace_bytes(long long n, int n_states) {
  if (n <= 0 || n_states < 1 || n_states > PINN_HMM_MAX_STATES) return 0;
  return pinn::layout_of(n, n_states).total;
}

extern "C" int pinn_hmm_forward_backward(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_states,
                                         const long long* d_row_index, long long n, const double* d_model,
                                         const long long* d_seg_start, long long n_segments, const double* d_carry_in,
                                         int respect_converged, double* d_alpha, double* d_gamma, double* d_loglik, double* d_xi,
                                         double* d_gamma_sum, double* d_carry_out, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  Hmm h;
  if (misaligned8(d_alpha) || misaligned8(d_gamma) || misaligned8(d_loglik) || misaligned8(d_xi) || misaligned8(d_gamma_sum) ||
      misaligned8(d_carry_out))
    return PINN_E_ARG;
  const int rc = make_hmm(d_arr, ld, n_arr_rows, cols, n_states, d_row_index, n, d_model, d_seg_start, n_segments, d_carry_in, d_ws,
                          ws_bytes, &h);
  if (rc != PINN_OK || n == 0) return rc;
  h.check = respect_converged ? 1 : 0;
  h.want_xi = (d_xi || d_gamma_sum) ? 1 : 0;
  if (d_alpha) h.alpha = d_alpha;
  h.gamma = d_gamma; h.loglik = d_loglik; h.xi = d_xi; h.gsum = d_gamma_sum; h.cout = d_carry_out;
  const bool backward = d_gamma || h.want_xi;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  switch (padded(n_states)) {
    case 2: launch_forward_backward<2>(h, backward, st); break;
    case 4: launch_forward_backward<4>(h, backward, st); break;
    default: launch_forward_backward<8>(h, backward, st); break;
  }
  return launch_status();
}

extern "C" int pinn_hmm_viterbi(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_states,
                                const long long* d_row_index, long long n, const double* d_model, const long long* d_seg_start,
                                long long n_segments, const double* d_carry_in, long long* d_path, double* d_logprob,
                                double* d_carry_out, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  Hmm h;
  if (!d_path || misaligned8(d_path) || misaligned8(d_logprob) || misaligned8(d_carry_out)) return PINN_E_ARG;
  const int rc = make_hmm(d_arr, ld, n_arr_rows, cols, n_states, d_row_index, n, d_model, d_seg_start, n_segments, d_carry_in, d_ws,
                          ws_bytes, &h);
  if (rc != PINN_OK || n == 0) return rc;
  h.path = d_path; h.loglik = d_logprob; h.cout = d_carry_out;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  switch (padded(n_states)) {
    case 2: launch_viterbi<2>(h, st); break;
    case 4: launch_viterbi<4>(h, st); break;
    default: launch_viterbi<8>(h, st); break;
  }
  return launch_status();
}

extern "C" int pinn_hmm_mstep(double* d_model, int n_states, const double* d_xi, const double* d_loglik, long long n_segments,
                              const double* d_pseudo, double tol, int max_hist, void* stream) {
  using namespace pinn;
  if (!d_model || !d_xi || !d_loglik || n_states < 1 || n_states > PINN_HMM_MAX_STATES || n_segments < 0 || max_hist < 0 || tol != tol)
    return PINN_E_ARG;
  if (misaligned8(d_model) || misaligned8(d_xi) || misaligned8(d_loglik) || misaligned8(d_pseudo)) return PINN_E_ARG;
  if (n_segments == 0) return PINN_OK;
  clear_error();
  hipLaunchKernelGGL(mstep_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, d_model, n_states, d_xi, d_loglik, n_segments, d_pseudo,
                     tol, max_hist);
  return launch_status();
}
