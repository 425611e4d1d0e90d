// The RBF-kernel SVC that script 05 names (05:323-341 calls it "RBF" and runs kernel="linear"; pinn_svm.hip is what it runs):
// StandardScaler, then a one-vs-one SVC with K(x, y) = exp(-gamma |x - y|^2), every pair solved by libsvm's SMO with
// second-order working-set selection in float64, without shrinking and without a kernel cache.  All arithmetic is float64,
// every operation rounded on its own (-ffp-contract=off): the host backend (ksvm.py) states the same arithmetic.
//   pinn_ksvm_smo       SMO iterations of every pair, two row passes each, no host synchronisation between them
//   pinn_ksvm_finish    rho, the objectives, the gap and the violation per pair at the state's point, one launch
//   pinn_ksvm_decision  pairwise decision values, votes and the prediction per row, one launch
//
// A pair (a, b), a < b, solves min 1/2 al'Q al - e'al, t'al = 0, 0 <= al <= c over the rows of its two classes,
// Q_ij = t_i t_j K_ij, with the gradient G = Q al - e kept per row.  A grid dimension is the pair, the other the row tiles:
// workgroup (x, p) owns the rows of tiles x, x + gridDim.x, ... that belong to pair p, and it alone writes their alpha and G.
//   select (pass A)  every workgroup of a pair reduces the i-candidates that the update pass left (one record per workgroup,
//                    at most kMaxBlocks), checks gmax - gmin <= tol on them, evaluates K(z_i, .) on its rows (kept in the
//                    workspace) and leaves its best j-candidate, with a copy of the winning i-record, as a record
//   update (pass B)  every workgroup reduces the j-candidates, computes libsvm's clipped two-variable update from the two
//                    records (the same arithmetic on the same inputs everywhere), adds the two kernel columns to G of its
//                    rows, writes alpha of i and j where it owns them and leaves its i-candidate and its share of gmin
// A pass reads only records that the pass before it wrote, and the pair block is written by workgroup 0 of the update pass
// alone, so no workgroup waits on another: stream order is the only dependency.  The first of equal candidates wins (the
// lowest row position), whatever the order of the reduction.  No float atomics; the same call gives the same bytes.  Once
// a pair's CONVERGED or STATUS word is set every later launch returns at once for it.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_ovo.h"

namespace pinn {
namespace {

constexpr int kT = 256;                      // threads of a workgroup = rows of a tile
constexpr int kMaxC = kOvoMaxC, kMaxD = kOvoMaxD, kMaxP = kOvoMaxP;
constexpr int kMaxBlocks = 1024;             // workgroups per pair = candidate records per pair
constexpr int kHdr = PINN_KSVM_ST_HEADER, kPW = PINN_KSVM_PAIR_WORDS;
constexpr int kRecI = 8, kRecJ = 16;         // words of a record
constexpr int kSvTile = PINN_KSVM_SV_TILE;   // support rows per LDS tile of the decision kernel
constexpr long long kNone = 0x7fffffffffffffffLL;
constexpr double kTau = 1e-12;
// record words: [0] row position (-1: none), [1] key, [2] alpha, [3] G, [4] c, [5] t, [6] aux (i: the workgroup's min of -tG
// over I_low; j: K_ij), [7] flags (i: status bits of the rows; j: 1 = stop | status bits << 8)

// state block: the prefix of pinn_ovo.h, then alpha and G [n][C - 1]
__host__ __device__ inline size_t st_words(long long n, int C, int D) { return st_alpha(C, D, kHdr, kPW) + 2 * (size_t)n * (C - 1); }

struct KArgs {
  double* st;               // state block
  const long long* y;       // class index per row position
  double* candI;            // [P][kMaxBlocks][kRecI]
  double* candJ;            // [P][kMaxBlocks][kRecJ]
  double* kcol;             // [n][C - 1]: K(z_i, row) of the running iteration
  long long* log;           // NULL or [P][n_log][2]
  double gamma, tol;
  int n_log, it;
};

struct Cand {
  double key;
  long long idx;
  double al, G, c, t, aux;
};

__device__ __forceinline__ Cand no_cand() { return {-INFINITY, kNone, 0.0, 0.0, 0.0, 0.0, 0.0}; }

__device__ __forceinline__ bool better(double k2, long long i2, double k1, long long i1) { return k2 > k1 || (k2 == k1 && i2 < i1); }

struct Shared {
  double key[kT];
  long long idx[kT];
  double mn[kT];
  long long fl[kT];
  double rec[8];
};

// the best candidate of the workgroup (largest key, the lowest position of equals), the smallest `mn` and the ORed flags,
// the same in every thread afterwards
__device__ inline void block_best(Shared& s, Cand& m, double& mn, long long& fl) {
  const int t = threadIdx.x;
  s.key[t] = m.key; s.idx[t] = m.idx; s.mn[t] = mn; s.fl[t] = fl;
  __syncthreads();
  for (int h = kT / 2; h > 0; h >>= 1) {
    if (t < h) {
      if (better(s.key[t + h], s.idx[t + h], s.key[t], s.idx[t])) { s.key[t] = s.key[t + h]; s.idx[t] = s.idx[t + h]; }
      if (s.mn[t + h] < s.mn[t]) s.mn[t] = s.mn[t + h];
      s.fl[t] |= s.fl[t + h];
    }
    __syncthreads();
  }
  const long long win = s.idx[0];
  if (win != kNone && m.idx == win) { s.rec[0] = m.key; s.rec[1] = m.al; s.rec[2] = m.G; s.rec[3] = m.c; s.rec[4] = m.t; s.rec[5] = m.aux; }
  mn = s.mn[0]; fl = s.fl[0];
  __syncthreads();
  if (win == kNone) m = no_cand();
  else m = {s.rec[0], win, s.rec[1], s.rec[2], s.rec[3], s.rec[4], s.rec[5]};
  __syncthreads();
}

__device__ __forceinline__ void store_rec(double* r, const Cand& m, long long flags) {
  long long* ri = reinterpret_cast<long long*>(r);
  ri[0] = m.idx == kNone ? -1 : m.idx;
  r[1] = m.key; r[2] = m.al; r[3] = m.G; r[4] = m.c; r[5] = m.t; r[6] = m.aux;
  ri[7] = flags;
}

__device__ __forceinline__ Cand load_rec(const double* r) {
  const long long idx = reinterpret_cast<const long long*>(r)[0];
  if (idx < 0) return no_cand();
  return {r[1], idx, r[2], r[3], r[4], r[5], r[6]};
}

// z-scores of position j; false when the position reads nothing
__device__ __forceinline__ bool load_z(const Rows& a, long long j, const double* mean, const double* scale, double z[kMaxD]) {
  double x[kRowsMaxD];
  const bool ok = load_row(a, j, x);
#pragma unroll
  for (int i = 0; i < kMaxD; ++i) z[i] = (ok && i < a.D) ? (x[i] - mean[i]) / scale[i] : 0.0;
  return ok;
}

// exp(-gamma |u - v|^2), the squared differences added in feature order
__device__ __forceinline__ double rbf(const double u[kMaxD], const double v[kMaxD], int D, double gamma) {
  double d2 = 0.0;
#pragma unroll
  for (int i = 0; i < kMaxD; ++i)
    if (i < D) { const double d = u[i] - v[i]; d2 += d * d; }
  return exp(-(gamma * d2));
}

struct PairView {
  int a, b;                 // class indices
  bool stopped;
};

__device__ __forceinline__ PairView pair_view(const double* st, int p, int C) {
  const long long* pi = reinterpret_cast<const long long*>(st + kHdr + (size_t)p * kPW);
  PairView v;
  v.a = (int)pi[PINN_KSVM_P_A]; v.b = (int)pi[PINN_KSVM_P_B];
  v.stopped = pi[PINN_KSVM_P_CONVERGED] != 0 || pi[PINN_KSVM_P_STATUS] != 0 || v.a < 0 || v.a >= v.b || v.b >= C;
  return v;
}

// ---- pass A: the i-candidate of the pair, the stopping rule, K(z_i, .) and this workgroup's j-candidate
__global__ __launch_bounds__(kT) void ksvm_select_kernel(Rows a, KArgs k) {
  __shared__ Shared s;
  __shared__ double s_mean[kMaxD], s_scale[kMaxD], s_bound[kMaxC];
  const int C = a.K, D = a.D, S1 = C - 1, t = threadIdx.x, p = blockIdx.y, nb = gridDim.x;
  const PairView pv = pair_view(k.st, p, C);
  if (pv.stopped) return;
  if (t < D) { s_mean[t] = k.st[st_mean(C, kHdr, kPW) + t]; s_scale[t] = k.st[st_mean(C, kHdr, kPW) + D + t]; }
  if (t < C) s_bound[t] = k.st[st_bound(C, D, kHdr, kPW) + t];
  Cand I = no_cand();
  double gmin = INFINITY;
  long long flags = 0;
  for (int r = t; r < nb; r += kT) {
    const double* rec = k.candI + ((size_t)p * kMaxBlocks + r) * kRecI;
    const Cand c = load_rec(rec);
    if (better(c.key, c.idx, I.key, I.idx)) I = c;
    gmin = rec[6] < gmin ? rec[6] : gmin;
    flags |= reinterpret_cast<const long long*>(rec)[7];
  }
  block_best(s, I, gmin, flags);                       // its first barrier is behind the loads of s_mean, s_scale and s_bound
  const double gmax = I.key;
  if (!flags && I.idx != kNone && I.idx >= a.n) flags = PINN_KSVM_RANGE;      // a record that no pass of this fit wrote
  const bool stop = flags != 0 || !(gmax - gmin > k.tol);
  double* out = k.candJ + ((size_t)p * kMaxBlocks + blockIdx.x) * kRecJ;
  I.aux = gmin;
  if (stop) {
    if (t == 0) { store_rec(out, no_cand(), 1 | (flags << 8)); store_rec(out + kRecI, I, 0); }
    return;
  }
  double zi[kMaxD], z[kMaxD];
  load_z(a, I.idx, s_mean, s_scale, zi);
  double* g_al = k.st + st_alpha(C, D, kHdr, kPW);
  double* g_G = g_al + (size_t)a.n * S1;
  Cand J = no_cand();
  const long long tiles = (a.n + kT - 1) / kT;
  for (long long tile = blockIdx.x; tile < tiles; tile += nb) {
    const long long j = tile * kT + t;
    if (j >= a.n) continue;
    const long long cls = k.y[j];
    if (cls != pv.a && cls != pv.b) continue;
    if (!load_z(a, j, s_mean, s_scale, z)) continue;
    const bool first = cls == pv.a;
    const size_t e = (size_t)j * S1 + (first ? pv.b - 1 : pv.a);
    const double tt = first ? 1.0 : -1.0, c = s_bound[cls];
    const double K = rbf(z, zi, D, k.gamma);
    k.kcol[e] = K;
    const double al = g_al[e], G = g_G[e];
    const bool low = first ? al > 0.0 : al < c;
    const double b = gmax + tt * G;
    if (low && b > 0.0) {
      double q = 2.0 - 2.0 * K;
      if (!(q > 0.0)) q = kTau;
      const double key = (b * b) / q;                   // libsvm minimises -b^2 / a
      if (better(key, j, J.key, J.idx)) J = {key, j, al, G, c, tt, K};
    }
  }
  double unused = INFINITY;
  long long none = 0;
  block_best(s, J, unused, none);
  if (t == 0) { store_rec(out, J, 0); store_rec(out + kRecI, I, 0); }
}

// ---- pass B (INIT: alpha = 0, G = -e and the row checks instead of an update): the update and the next i-candidates
template <bool INIT>
__global__ __launch_bounds__(kT) void ksvm_update_kernel(Rows a, KArgs k) {
  __shared__ Shared s;
  __shared__ double s_mean[kMaxD], s_scale[kMaxD], s_bound[kMaxC];
  const int C = a.K, D = a.D, S1 = C - 1, t = threadIdx.x, p = blockIdx.y, nb = gridDim.x;
  double* pb = k.st + kHdr + (size_t)p * kPW;
  long long* pi = reinterpret_cast<long long*>(pb);
  PairView pv = pair_view(k.st, p, C);
  if (INIT) {
    pv.stopped = pv.a < 0 || pv.a >= pv.b || pv.b >= C;
    if (blockIdx.x == 0 && t == 0) {
      pi[PINN_KSVM_P_ITER] = 0; pi[PINN_KSVM_P_CONVERGED] = 0; pi[PINN_KSVM_P_STATUS] = pv.stopped ? PINN_KSVM_RANGE : 0;
      pi[PINN_KSVM_P_I] = -1; pi[PINN_KSVM_P_J] = -1;
      for (int w = PINN_KSVM_P_NFREE; w < kPW; ++w) pb[w] = 0.0;
    }
  }
  if (pv.stopped) return;
  if (t < D) { s_mean[t] = k.st[st_mean(C, kHdr, kPW) + t]; s_scale[t] = k.st[st_mean(C, kHdr, kPW) + D + t]; }
  if (t < C) s_bound[t] = k.st[st_bound(C, D, kHdr, kPW) + t];
  __syncthreads();
  Cand I = no_cand(), J = no_cand();
  double ai = 0.0, aj = 0.0, di = 0.0, dj = 0.0;
  double zj[kMaxD], z[kMaxD];
  if (!INIT) {
    const double* rec0 = k.candJ + (size_t)p * kMaxBlocks * kRecJ;
    const long long stopw = reinterpret_cast<const long long*>(rec0)[7];
    I = load_rec(rec0 + kRecI);
    if (stopw) {                                        // every workgroup of the pair reads the same word
      if (blockIdx.x == 0 && t == 0) {
        pb[PINN_KSVM_P_GMAX] = I.key; pb[PINN_KSVM_P_GMIN] = rec0[kRecI + 6];
        if (stopw >> 8) pi[PINN_KSVM_P_STATUS] = stopw >> 8;
        else pi[PINN_KSVM_P_CONVERGED] = 1;
      }
      return;
    }
    for (int r = t; r < nb; r += kT) {
      const Cand c = load_rec(k.candJ + ((size_t)p * kMaxBlocks + r) * kRecJ);
      if (better(c.key, c.idx, J.key, J.idx)) J = c;
    }
    double unused = INFINITY;
    long long none = 0;
    block_best(s, J, unused, none);
    if (J.idx == kNone || J.idx >= a.n || I.idx == kNone || I.idx >= a.n) {      // cannot be while gmax - gmin > tol holds finite numbers
      if (blockIdx.x == 0 && t == 0) pi[PINN_KSVM_P_STATUS] = PINN_KSVM_NAN;
      return;
    }
    // libsvm's update of (alpha_i, alpha_j): Q_ii = Q_jj = 1, Q_ij = t_i t_j K_ij, so both cases divide by 2 - 2 K_ij
    const double Kij = J.aux;
    double q = 2.0 - 2.0 * Kij;
    if (!(q > 0.0)) q = kTau;
    ai = I.al; aj = J.al;
    if (I.t != J.t) {
      const double delta = (-I.G - J.G) / q, diff = ai - aj;
      ai += delta; aj += delta;
      if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
      else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
      if (diff > I.c - J.c) { if (ai > I.c) { ai = I.c; aj = I.c - diff; } }
      else { if (aj > J.c) { aj = J.c; ai = J.c + diff; } }
    } else {
      const double delta = (I.G - J.G) / q, sum = ai + aj;
      ai -= delta; aj += delta;
      if (sum > I.c) { if (ai > I.c) { ai = I.c; aj = sum - I.c; } }
      else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
      if (sum > J.c) { if (aj > J.c) { aj = J.c; ai = sum - J.c; } }
      else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
    }
    di = ai - I.al; dj = aj - J.al;
    load_z(a, J.idx, s_mean, s_scale, zj);
  }
  double* g_al = k.st + st_alpha(C, D, kHdr, kPW);
  double* g_G = g_al + (size_t)a.n * S1;
  Cand N = no_cand();
  double gmin = INFINITY;
  long long flags = 0;
  const long long tiles = (a.n + kT - 1) / kT;
  for (long long tile = blockIdx.x; tile < tiles; tile += nb) {
    const long long j = tile * kT + t;
    if (j >= a.n) continue;
    const long long cls = k.y[j];
    if (INIT && (cls < 0 || cls >= C)) flags |= PINN_KSVM_RANGE;
    if (cls != pv.a && cls != pv.b) continue;
    const bool ok = load_z(a, j, s_mean, s_scale, z);
    const bool first = cls == pv.a;
    const size_t e = (size_t)j * S1 + (first ? pv.b - 1 : pv.a);
    const double tt = first ? 1.0 : -1.0, c = s_bound[cls];
    double al, G;
    if (INIT) {
      al = 0.0; G = -1.0;
      g_al[e] = al; g_G[e] = G;
      if (!ok) { flags |= PINN_KSVM_RANGE; continue; }
      bool fin = true;
      for (int i = 0; i < D; ++i) fin = fin && finite(z[i]);
      if (!fin) { flags |= PINN_KSVM_NAN; continue; }
    } else {
      if (!ok) continue;
      const double Ki = k.kcol[e], Kj = rbf(z, zj, D, k.gamma);
      G = g_G[e] + tt * ((I.t * Ki) * di + (J.t * Kj) * dj);
      g_G[e] = G;
      al = g_al[e];
      if (j == I.idx) { al = ai; g_al[e] = al; }
      if (j == J.idx) { al = aj; g_al[e] = al; }
    }
    const double v = -(tt * G);
    const bool up = first ? al < c : al > 0.0, low = first ? al > 0.0 : al < c;
    if (up && better(v, j, N.key, N.idx)) N = {v, j, al, G, c, tt, 0.0};
    if (low && v < gmin) gmin = v;
  }
  block_best(s, N, gmin, flags);
  if (t == 0) {
    N.aux = gmin;
    store_rec(k.candI + ((size_t)p * kMaxBlocks + blockIdx.x) * kRecI, N, flags);
    if (!INIT && blockIdx.x == 0) {
      pi[PINN_KSVM_P_ITER] += 1; pi[PINN_KSVM_P_I] = I.idx; pi[PINN_KSVM_P_J] = J.idx;
      pb[PINN_KSVM_P_GMAX] = I.key; pb[PINN_KSVM_P_GMIN] = I.aux;
      if (k.log && k.it < k.n_log) {
        long long* lg = k.log + ((size_t)p * k.n_log + k.it) * 2;
        lg[0] = I.idx; lg[1] = J.idx;
      }
    }
  }
}

__device__ inline double block_sum(double* buf, double v) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int h = kT / 2; h > 0; h >>= 1) {
    if (t < h) buf[t] = buf[t] + buf[t + h];
    __syncthreads();
  }
  const double r = buf[0];
  __syncthreads();
  return r;
}

__device__ inline double block_min(double* buf, double v) {
  const int t = threadIdx.x;
  buf[t] = v;
  __syncthreads();
  for (int h = kT / 2; h > 0; h >>= 1) {
    if (t < h) buf[t] = buf[t + h] < buf[t] ? buf[t + h] : buf[t];
    __syncthreads();
  }
  const double r = buf[0];
  __syncthreads();
  return r;
}

// ---- the certificate of every pair at the state's point: one workgroup per pair walks the rows twice (rho first, then the
// hinge sum that needs it).  Thread t adds rows t, t + kT, ... in that order, then the threads' sums are added as a tree.
__global__ __launch_bounds__(kT) void ksvm_finish_kernel(Rows a, KArgs k) {
  __shared__ double buf[kT];
  __shared__ double s_bound[kMaxC];
  const int C = a.K, D = a.D, S1 = C - 1, t = threadIdx.x, p = blockIdx.x;
  double* pb = k.st + kHdr + (size_t)p * kPW;
  long long* pi = reinterpret_cast<long long*>(pb);
  const int ca = (int)pi[PINN_KSVM_P_A], cb = (int)pi[PINN_KSVM_P_B];
  if (ca < 0 || ca >= cb || cb >= C) return;
  if (t < C) s_bound[t] = k.st[st_bound(C, D, kHdr, kPW) + t];
  __syncthreads();
  const double* g_al = k.st + st_alpha(C, D, kHdr, kPW);
  const double* g_G = g_al + (size_t)a.n * S1;
  double n_free = 0.0, s_free = 0.0, ub = INFINITY, nlb = INFINITY, s_al = 0.0, s_aq = 0.0, s_ta = 0.0, ngmax = INFINITY, gmin = INFINITY;
  for (long long j = t; j < a.n; j += kT) {
    const long long cls = k.y[j];
    if (cls != ca && cls != cb) continue;
    const bool first = cls == ca;
    const size_t e = (size_t)j * S1 + (first ? cb - 1 : ca);
    const double tt = first ? 1.0 : -1.0, c = s_bound[cls], al = g_al[e], G = g_G[e], tG = tt * G;
    const bool at_c = al >= c, at_0 = al <= 0.0;
    if (at_c) { if (first) nlb = -tG < nlb ? -tG : nlb; else ub = tG < ub ? tG : ub; }
    else if (at_0) { if (first) ub = tG < ub ? tG : ub; else nlb = -tG < nlb ? -tG : nlb; }
    else { n_free += 1.0; s_free += tG; }
    s_al += al; s_aq += al * (G + 1.0); s_ta += tt * al;
    const double v = -tG;
    const bool up = first ? al < c : al > 0.0, low = first ? al > 0.0 : al < c;
    if (up && -v < ngmax) ngmax = -v;
    if (low && v < gmin) gmin = v;
  }
  n_free = block_sum(buf, n_free); s_free = block_sum(buf, s_free);
  s_al = block_sum(buf, s_al); s_aq = block_sum(buf, s_aq); s_ta = block_sum(buf, s_ta);
  ub = block_min(buf, ub); nlb = block_min(buf, nlb); ngmax = block_min(buf, ngmax); gmin = block_min(buf, gmin);
  const double rho = n_free > 0.0 ? s_free / n_free : (ub + -nlb) / 2.0;
  const double b = -rho;
  double hinge = 0.0;
  for (long long j = t; j < a.n; j += kT) {
    const long long cls = k.y[j];
    if (cls != ca && cls != cb) continue;
    const bool first = cls == ca;
    const size_t e = (size_t)j * S1 + (first ? cb - 1 : ca);
    const double tt = first ? 1.0 : -1.0, h = -g_G[e] - tt * b;
    hinge += s_bound[cls] * (h > 0.0 ? h : 0.0);
  }
  hinge = block_sum(buf, hinge);
  if (t == 0) {
    const double primal = 0.5 * s_aq + hinge, dual = s_al - 0.5 * s_aq;
    pb[PINN_KSVM_P_RHO] = rho; pb[PINN_KSVM_P_PRIMAL] = primal; pb[PINN_KSVM_P_DUAL] = dual; pb[PINN_KSVM_P_GAP] = primal - dual;
    pb[PINN_KSVM_P_SUMALPHA] = s_al; pb[PINN_KSVM_P_TALPHA] = s_ta; pb[PINN_KSVM_P_VIOLATION] = -ngmax - gmin;
    pi[PINN_KSVM_P_NFREE] = (long long)n_free;
  }
}

// ---- decision of given rows: one thread per row; the support rows pass through LDS in tiles of kSvTile
template <int KC>
__device__ __forceinline__ void add_support(double acc[kMaxP], const double* cf, double K, int C) {
#pragma unroll
  for (int o = 0; o < kMaxC; ++o) {
    if (o == KC) continue;
    if (o < C) acc[o < KC ? q8(o, KC) : q8(KC, o)] += cf[o < KC ? o : o - 1] * K;
  }
}

__global__ __launch_bounds__(kSvTile) void ksvm_decision_kernel(Rows a, const double* __restrict__ scaler, const double* __restrict__ sv,
                                                                const double* __restrict__ coef, const long long* __restrict__ sv_cls,
                                                                long long n_sv, const double* __restrict__ rho, double gamma,
                                                                double* __restrict__ dec_out, long long* __restrict__ votes_out,
                                                                long long* __restrict__ pred_out) {
  __shared__ double s_sv[kSvTile * kMaxD], s_cf[kSvTile * (kMaxC - 1)];
  __shared__ int s_cls[kSvTile];
  __shared__ double s_mean[kMaxD], s_scale[kMaxD];
  const int C = a.K, D = a.D, S1 = C - 1, t = threadIdx.x;
  if (t < kMaxD) { s_mean[t] = (scaler && t < D) ? scaler[t] : 0.0; s_scale[t] = (scaler && t < D) ? scaler[D + t] : 1.0; }
  __syncthreads();
  const long long j = (long long)blockIdx.x * kSvTile + t;
  double z[kMaxD];
  bool ok = false;
  if (j < a.n) ok = load_z(a, j, s_mean, s_scale, z);
  else
    for (int i = 0; i < kMaxD; ++i) z[i] = 0.0;
  double acc[kMaxP];
#pragma unroll
  for (int q = 0; q < kMaxP; ++q) acc[q] = 0.0;
  for (long long s0 = 0; s0 < n_sv; s0 += kSvTile) {
    const long long m = n_sv - s0 < kSvTile ? n_sv - s0 : kSvTile;
    __syncthreads();
    if (t < m) {
      for (int i = 0; i < kMaxD; ++i) s_sv[t * kMaxD + i] = i < D ? sv[(s0 + t) * D + i] : 0.0;
      for (int i = 0; i < kMaxC - 1; ++i) s_cf[t * (kMaxC - 1) + i] = i < S1 ? coef[(s0 + t) * S1 + i] : 0.0;
      const long long c = sv_cls[s0 + t];
      s_cls[t] = (c >= 0 && c < C) ? (int)c : -1;       // a class outside [0, C) adds nothing
    }
    __syncthreads();
    for (int r = 0; r < (int)m; ++r) {
      const double K = rbf(z, s_sv + r * kMaxD, D, gamma);
      const double* cf = s_cf + r * (kMaxC - 1);
      switch (s_cls[r]) {
        case 0: add_support<0>(acc, cf, K, C); break;
        case 1: add_support<1>(acc, cf, K, C); break;
        case 2: add_support<2>(acc, cf, K, C); break;
        case 3: add_support<3>(acc, cf, K, C); break;
        case 4: add_support<4>(acc, cf, K, C); break;
        case 5: add_support<5>(acc, cf, K, C); break;
        case 6: add_support<6>(acc, cf, K, C); break;
        case 7: add_support<7>(acc, cf, K, C); break;
        default: break;
      }
    }
  }
  if (j >= a.n) return;
  ovo_decide([&](int ca, int cb, int p) { return acc[q8(ca, cb)] - rho[p]; }, ok, C, j, dec_out, votes_out, pred_out);
}

struct Ws {
  double *candI, *candJ, *kcol;
};

inline size_t carve(void* d_ws, long long n, int C, Ws* s) {
  char* w = static_cast<char*>(d_ws);
  const size_t P = n_pairs(C);
  size_t o = 0;
  if (s) s->candI = reinterpret_cast<double*>(w + o);
  o += align256(P * kMaxBlocks * kRecI * sizeof(double));
  if (s) s->candJ = reinterpret_cast<double*>(w + o);
  o += align256(P * kMaxBlocks * kRecJ * sizeof(double));
  if (s) s->kcol = reinterpret_cast<double*>(w + o);
  return o + align256((size_t)n * (C - 1) * sizeof(double));
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_ksvm_state_bytes(long long n_rows, int n_classes, int n_feat) {
  if (n_rows < 0 || !pinn::in_limits(n_classes, n_feat)) return 0;
  return pinn::st_words(n_rows, n_classes, n_feat) * sizeof(double);
}

extern "C" size_t pinn_ksvm_workspace_bytes(long long n_rows, int n_classes, int n_feat) {
  if (n_rows < 0 || !pinn::in_limits(n_classes, n_feat)) return 0;
  return pinn::carve(nullptr, n_rows, n_classes, nullptr);
}

extern "C" int pinn_ksvm_smo(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                             const long long* d_row_index, long long n, const long long* d_y, int n_classes, double gamma,
                             int init, int n_iters, double tol, double* d_state, long long* d_log, void* d_ws, size_t ws_bytes,
                             void* stream) {
  using namespace pinn;
  if (!in_limits(n_classes, n_feat)) return PINN_E_ARG;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_classes, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_state || !d_ws || !d_y || misaligned8(d_state) || misaligned8(d_ws) || misaligned8(d_y) || n < 1) return PINN_E_ARG;
  if (n_iters < 0 || n_iters > 1000000 || !(tol > 0.0) || !(gamma > 0.0) || !(gamma < INFINITY) || misaligned8(d_log)) return PINN_E_ARG;
  if (ws_bytes < pinn_ksvm_workspace_bytes(n, n_classes, n_feat)) return PINN_E_WORKSPACE;
  Ws w;
  carve(d_ws, n, n_classes, &w);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)row_blocks(n, kT, kMaxBlocks), (unsigned)n_pairs(n_classes));
  clear_error();
  KArgs k = {d_state, d_y, w.candI, w.candJ, w.kcol, d_log, gamma, tol, n_iters, 0};
  if (init) hipLaunchKernelGGL(ksvm_update_kernel<true>, grid, dim3(kT), 0, st, a, k);
  for (int it = 0; it < n_iters; ++it) {
    k.it = it;
    hipLaunchKernelGGL(ksvm_select_kernel, grid, dim3(kT), 0, st, a, k);
    hipLaunchKernelGGL(ksvm_update_kernel<false>, grid, dim3(kT), 0, st, a, k);
  }
  return launch_status();
}

extern "C" int pinn_ksvm_finish(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                const long long* d_row_index, long long n, const long long* d_y, int n_classes, double* d_state,
                                void* stream) {
  using namespace pinn;
  if (!in_limits(n_classes, n_feat)) return PINN_E_ARG;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_classes, d_row_index, n, &a);      // the rows give n and the limits; they are not read
  if (rc != PINN_OK) return rc;
  if (!d_state || !d_y || misaligned8(d_state) || misaligned8(d_y) || n < 1) return PINN_E_ARG;
  clear_error();
  const KArgs k = {d_state, d_y, nullptr, nullptr, nullptr, nullptr, 0.0, 0.0, 0, 0};
  hipLaunchKernelGGL(ksvm_finish_kernel, dim3((unsigned)n_pairs(n_classes)), dim3(kT), 0, (hipStream_t)stream, a, k);
  return launch_status();
}

extern "C" int pinn_ksvm_decision(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                  const long long* d_row_index, long long n, int n_classes, const double* d_scaler,
                                  const double* d_sv, const double* d_coef, const long long* d_sv_class, long long n_sv,
                                  const double* d_rho, double gamma, double* d_decision, long long* d_votes, long long* d_pred,
                                  void* stream) {
  using namespace pinn;
  if (!in_limits(n_classes, n_feat)) return PINN_E_ARG;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_classes, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (n_sv < 0 || !d_rho || (n_sv > 0 && (!d_sv || !d_coef || !d_sv_class)) || !(gamma > 0.0) || !(gamma < INFINITY)) return PINN_E_ARG;
  if (misaligned8(d_scaler) || misaligned8(d_sv) || misaligned8(d_coef) || misaligned8(d_sv_class) || misaligned8(d_rho) ||
      misaligned8(d_decision) || misaligned8(d_votes) || misaligned8(d_pred))
    return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  const long long tiles = (n + kSvTile - 1) / kSvTile;
  if (tiles > 0x7fffffffLL) return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(ksvm_decision_kernel, dim3((unsigned)tiles), dim3(kSvTile), 0, (hipStream_t)stream, a, d_scaler, d_sv, d_coef,
                     d_sv_class, n_sv, d_rho, gamma, d_decision, d_votes, d_pred);
  return launch_status();
}
