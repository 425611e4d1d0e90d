// Conformal fault sets and unknown-fault rejection (include/pinn_hip.h and faultsets.py state the statistics).
//   pinn_fs_build   calibration scores and classes -> the state block: counts, places, a merge sort by ranks per table
//   pinn_fs_rank    y_prob rows -> scores, counts against the sorted tables, set masks per level, tallies
//   pinn_fs_gmm     the same from rows read in place under a mixture: posterior, label map, scores, ranks, masks in one launch
//
// The ranking is one thread per row.  A thread forms its C scores in registers and finds, per class, the number of table
// entries below its score (a lower bound), so count = n_c - that number is an integer both backends agree on to the bit; the
// level test is count >= kmin[c][l] with kmin computed by the caller in exact rationals.  Where the tables are searched is the
// regime: all of them staged in LDS; every 16th entry (the first of each 128-byte line) staged in LDS, searched there, then one
// line of 15 further entries read from global memory and counted; or a binary search in global memory.  The three give the
// same integers by construction.  Tallies are integer atomics in LDS, flushed by integer atomics to global memory at the end
// of a workgroup: no float atomics, and no workgroup waits on another.  float64, every operation rounded on its own; the
// mixture's own arithmetic (estep_row, fault_prob_row) is contracted as pinn_gmm.hip is built, so that y_prob, y_pred and
// log_prob_norm have pinn_gmm_posterior's bytes.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_mlp_core.h"
#include "pinn_rows.h"
#include "pinn_gmm_state.h"

namespace pinn {
namespace {

constexpr int kC = PINN_FS_MAX_CLASSES, kL = PINN_FS_MAX_LEVELS, kT = kC + 1, kLine = PINN_FS_LINE;
constexpr int kTile = PINN_FS_TILE, kGmmTile = PINN_FS_GMM_TILE, kBlocks = PINN_FS_MAX_BLOCKS, kWords = PINN_FS_TALLY_WORDS;
constexpr int kMaxK = PINN_GMM_MAX_COMP, kMaxD = PINN_GMM_MAX_FEAT, kTri = kMaxD * (kMaxD + 1) / 2;
constexpr int kBuildThreads = 256;
constexpr long long kMaxRows = 1LL << 40;     // a workgroup's int32 tallies cannot overflow below this

// what a ranking launch knows about the calibration, by value in the kernel arguments
struct Cal {
  const double* tab;                          // the first table entry (behind the header); NULL: scores only
  int C, L, kind, randomized, draw, regime;
  unsigned seed_lo, seed_hi;
  long long first;
  int n[kT], off[kT], soff[kT];               // table sizes, first entries, first sampled entries (regime SAMPLED)
  int kmin[kC * kL];                          // [c][l] with the stride kL
  int staged;                                 // entries staged in LDS
};

struct Out {
  const long long* y;
  int* count;
  unsigned short* mask;
  unsigned char *size, *novel, *missing;
  double* scores;
  unsigned long long* tally;
  int* any_count;
};

inline int pad_line(long long n) { return (int)((n + kLine - 1) / kLine * kLine); }

// ---- scores of a posterior row
__device__ __forceinline__ bool row_missing(const double p[kC], int C) {
  bool bad = false, any = false;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    if (c < C) {
      const double v = p[c];
      if (!(v >= 0.0) || v == INFINITY) bad = true;
      if (v > 0.0) any = true;
    }
  }
  return bad || !any;
}

__device__ __forceinline__ double uniform_of(const Cal& P, long long pos) {
  if (!P.randomized) return 1.0;
  const unsigned long long row = (unsigned long long)(P.first + pos);
  unsigned w[4];
  philox4x32_10((unsigned)row, (unsigned)(row >> 32), (unsigned)P.draw, 0u, P.seed_lo, P.seed_hi, w);
  return (double)(((unsigned long long)w[0] << 21) | (unsigned long long)(w[1] >> 11)) * 0x1p-53;
}

__device__ __forceinline__ void posterior_scores(const double p[kC], int C, int kind, double u, double s[kC]) {
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    s[c] = 0.0;
    if (c >= C) continue;
    if (kind == PINN_FS_LAC) {
      s[c] = 1.0 - p[c];
    } else if (kind == PINN_FS_MARGIN) {
      double m = -INFINITY;
#pragma unroll
      for (int k = 0; k < kC; ++k)
        if (k < C && k != c) m = p[k] > m ? p[k] : m;
      s[c] = C == 1 ? -p[c] : m - p[c];
    } else {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < kC; ++k)
        if (k < C && (p[k] > p[c] || (p[k] == p[c] && k < c))) acc += p[k];
      s[c] = acc + u * p[c];
    }
  }
}

// ---- the tables
__device__ __forceinline__ void stage_tables(const Cal& P, double* __restrict__ lds) {
  if (P.tab && P.regime == PINN_FS_REGIME_LDS) {
    for (int e = threadIdx.x; e < P.staged; e += blockDim.x) lds[e] = P.tab[e];
  } else if (P.tab && P.regime == PINN_FS_REGIME_SAMPLED) {
    for (int c = 0; c <= P.C; ++c) {
      const int ns = (P.n[c] + kLine - 1) / kLine;
      for (int i = threadIdx.x; i < ns; i += blockDim.x) lds[P.soff[c] + i] = P.tab[P.off[c] + i * kLine];
    }
  }
  __syncthreads();
}

// entries of T[0 .. n) below s (T ascending, no NaN; s is no NaN)
__device__ __forceinline__ int lower_bound(const double* __restrict__ T, int n, double s) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// #{t in T_c : t >= s}
__device__ __forceinline__ int count_ge(const Cal& P, const double* __restrict__ lds, int c, double s) {
  const int n = P.n[c];
  const double* __restrict__ T = P.tab + P.off[c];
  int lt;
  if (P.regime == PINN_FS_REGIME_LDS) {
    lt = lower_bound(lds + P.off[c], n, s);
  } else if (P.regime == PINN_FS_REGIME_SAMPLED) {
    const int j = lower_bound(lds + P.soff[c], (n + kLine - 1) / kLine, s);      // sampled entries below s
    lt = 0;
    if (j > 0) {                              // T[16 (j - 1)] < s <= T[16 j]: the answer lies in that line
      const int base = kLine * (j - 1) + 1, end = kLine * j < n ? kLine * j : n;
      int below = 0;
      for (int i = base; i < end; ++i) below += T[i] < s ? 1 : 0;
      lt = base + below;
    }
  } else {
    lt = lower_bound(T, n, s);
  }
  return n - lt;
}

// counts, masks and tallies of one row from its scores
__device__ __forceinline__ void rank_row(const Cal& P, const double* __restrict__ lds, int* s_tally, long long j, bool miss,
                                         const double s[kC], double s_any, const Out& o) {
  const int C = P.C, L = P.L;
  if (o.scores) {
#pragma unroll
    for (int c = 0; c < kC; ++c)
      if (c < C) o.scores[j * C + c] = miss ? quiet_nan() : s[c];
  }
  if (o.missing) o.missing[j] = miss ? 1 : 0;
  if (!P.tab) return;
  int cnt[kC];
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    cnt[c] = -1;
    if (c < C) {
      if (!miss) cnt[c] = count_ge(P, lds, c, s[c]);
      if (o.count) o.count[j * C + c] = cnt[c];
    }
  }
  if (o.any_count) o.any_count[j] = miss ? -1 : count_ge(P, lds, C, s_any);
  long long y = -1;
  const bool tally = o.y != nullptr && !miss;
  if (tally) {
    y = o.y[j];
    if (y >= 0 && y < C) atomicAdd(&s_tally[PINN_FS_T_N + (int)y], 1); else atomicAdd(&s_tally[PINN_FS_T_OUT_N], 1);
  }
#pragma unroll
  for (int l = 0; l < kL; ++l) {
    if (l >= L) continue;
    unsigned m = 0;
    int sz = 0;
#pragma unroll
    for (int c = 0; c < kC; ++c) {
      if (c < C && !miss && cnt[c] >= P.kmin[c * kL + l]) { m |= 1u << c; ++sz; }
    }
    if (o.mask) o.mask[j * L + l] = (unsigned short)m;
    if (o.size) o.size[j * L + l] = (unsigned char)sz;
    if (o.novel) o.novel[j * L + l] = (!miss && sz == 0) ? 1 : 0;
    if (tally) {
      if (y >= 0 && y < C) {
        const bool in = (m >> (int)y) & 1u;
        if (in) atomicAdd(&s_tally[PINN_FS_T_COVERED + (int)y * kL + l], 1);
        atomicAdd(&s_tally[PINN_FS_T_HIST + l * kT + sz], 1);
        if (in && sz == 1) atomicAdd(&s_tally[PINN_FS_T_SINGLE + l], 1);
      } else if (sz == 0) {
        atomicAdd(&s_tally[PINN_FS_T_OUT_NOVEL + l], 1);
      }
    }
  }
}

__device__ __forceinline__ void flush_tally(const int* s_tally, unsigned long long* __restrict__ tally) {
  __syncthreads();
  if (!tally) return;
  for (int e = threadIdx.x; e < kWords; e += blockDim.x)
    if (s_tally[e] != 0) atomicAdd(&tally[e], (unsigned long long)s_tally[e]);
}

__global__ __launch_bounds__(kTile) void fs_rank_kernel(const double* __restrict__ yp, long long n, Cal P, Out o) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ int s_tally[kWords];
  for (int e = threadIdx.x; e < kWords; e += kTile) s_tally[e] = 0;
  stage_tables(P, lds);
  const int C = P.C;
  for (long long tile = blockIdx.x; tile * kTile < n; tile += gridDim.x) {
    const long long j = tile * kTile + threadIdx.x;
    if (j >= n) continue;
    double p[kC], s[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) p[c] = c < C ? yp[j * C + c] : 0.0;
    bool miss = row_missing(p, C);
    posterior_scores(p, C, P.kind, uniform_of(P, j), s);
#pragma unroll
    for (int c = 0; c < kC; ++c)
      if (c < C && s[c] != s[c]) miss = true;
    rank_row(P, lds, s_tally, j, miss, s, 0.0, o);
  }
  flush_tally(s_tally, o.tally);
}

// ---- the fused form: rows in place under a mixture
// fault probabilities of a row from its responsibilities, the arithmetic of pinn_gmm_posterior (03:418-424); returns the argmax
__device__ __forceinline__ int fault_prob_row(const double* __restrict__ r, int K, int C, const double* __restrict__ s_map, double y[kC]) {
#pragma clang fp contract(fast)                             // as pinn_gmm.hip is built
  double sum = 0.0;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    y[c] = 0.0;
    if (c < C) {
      double v = 0.0;
      for (int k = 0; k < K; ++k) v += r[k] * s_map[k * C + c];
      if (v == v) v = v < 1e-12 ? 1e-12 : (v > 1.0 ? 1.0 : v);
      y[c] = v;
      sum += v;
    }
  }
  int best = 0;
  double bv = -INFINITY;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    if (c < C) {
      const double v = y[c] / sum;
      y[c] = v;
      if (v > bv) { bv = v; best = c; }
    }
  }
  return best;
}

// density scores from lp[k] = log(w_k N(x | mu_k, Sigma_k)); lm: log m [K][C] then log pi [C]
__device__ __forceinline__ void density_scores(const double* __restrict__ lp, int K, int C, const double* __restrict__ lm, double s[kC]) {
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    s[c] = 0.0;
    if (c >= C) continue;
    const double lpi = lm[K * C + c];
    double m = -INFINITY;
    bool any = false;
    for (int k = 0; k < K; ++k) {
      const double l = lm[k * C + c];
      if (l > -INFINITY) {
        const double t = lp[k] + l;
        m = t > m ? t : m;
        any = true;
      }
    }
    if (!any || lpi == -INFINITY) { s[c] = INFINITY; continue; }
    double lse = m;
    if (m != -INFINITY) {
      double sum = 0.0;
      for (int k = 0; k < K; ++k) {
        const double l = lm[k * C + c];
        if (l > -INFINITY) sum += exp((lp[k] + l) - m);
      }
      lse = log(sum) + m;
    }
    s[c] = -(lse - lpi);
  }
}

__global__ __launch_bounds__(kGmmTile) void fs_gmm_kernel(Rows a, const double* __restrict__ st, const double* __restrict__ map,
                                                          const double* __restrict__ logmap, Cal P, Out o, double* __restrict__ prob_out,
                                                          long long* __restrict__ pred_out, double* __restrict__ lpn_out,
                                                          double* __restrict__ any_score) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  __shared__ double s_r[kGmmTile * (kMaxK + 1)];
  __shared__ double s_mu[kMaxK * kMaxD], s_U[kMaxK * kTri], s_ld[kMaxK], s_lw[kMaxK];
  __shared__ double s_map[kMaxK * kC], s_lm[kMaxK * kC + kC];
  __shared__ int s_tally[kWords];
  const int K = a.K, D = a.D, C = P.C, Kp = K | 1, t = threadIdx.x;
  const Staged sp{s_mu, s_U, s_ld, s_lw};
  for (int e = t; e < kWords; e += kGmmTile) s_tally[e] = 0;
  for (int e = t; e < K * C; e += kGmmTile) s_map[e] = map[e];
  if (logmap)
    for (int e = t; e < K * C + C; e += kGmmTile) s_lm[e] = logmap[e];
  stage_params(st, K, D, sp, true);
  stage_tables(P, lds);
  double* r = s_r + t * Kp;
  for (long long tile = blockIdx.x; tile * kGmmTile < a.n; tile += gridDim.x) {
    const long long j = tile * kGmmTile + t;
    if (j >= a.n) continue;
    double x[kMaxD];
    const bool ok = load_row(a, j, x);
    bool finite = ok;
#pragma unroll
    for (int i = 0; i < kMaxD; ++i)
      if (i < D && !(x[i] - x[i] == 0.0)) finite = false;
    double lpn = quiet_nan(), s[kC], s_any = 0.0;
#pragma unroll
    for (int c = 0; c < kC; ++c) s[c] = 0.0;                 // a row that cannot be read forms no score
    bool miss = false;
    if (ok) {
      lpn = estep_row(x, K, D, sp, r, 1);
      if (P.kind == PINN_FS_DENSITY) {
        density_scores(r, K, C, s_lm, s);
        s_any = -lpn;
        miss = !finite || s_any != s_any;
      }
      for (int k = 0; k < K; ++k) r[k] = exp(r[k] - lpn);
    } else {
      for (int k = 0; k < K; ++k) r[k] = quiet_nan();
      miss = true;
    }
    if (lpn_out) lpn_out[j] = lpn;
    double y[kC];
    const int best = fault_prob_row(r, K, C, s_map, y);
    if (prob_out) {
#pragma unroll
      for (int c = 0; c < kC; ++c)
        if (c < C) prob_out[j * C + c] = y[c];
    }
    if (pred_out) pred_out[j] = best;
    if (P.kind != PINN_FS_DENSITY) {
      miss = row_missing(y, C);
      posterior_scores(y, C, P.kind, uniform_of(P, j), s);
    }
#pragma unroll
    for (int c = 0; c < kC; ++c)
      if (c < C && s[c] != s[c]) miss = true;
    if (any_score) any_score[j] = miss ? quiet_nan() : s_any;
    rank_row(P, lds, s_tally, j, miss, s, s_any, o);
  }
  flush_tally(s_tally, o.tally);
}

// ---- building the state
// header counts: n_c of every table and the skipped rows
__global__ __launch_bounds__(kBuildThreads) void fs_count_kernel(const double* __restrict__ sc, const double* __restrict__ any,
                                                                 const long long* __restrict__ cls, long long n, int C,
                                                                 unsigned long long* __restrict__ h) {
  __shared__ int s_n[kT + 1];
  if (threadIdx.x <= kT) s_n[threadIdx.x] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * kBuildThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kBuildThreads) {
    const long long c = cls[i];
    bool ok = c >= 0 && c < C;
    if (ok) { const double v = sc[i * C + c]; ok = v == v; }
    if (ok && any) { const double v = any[i]; ok = v == v; }
    if (ok) {
      atomicAdd(&s_n[(int)c], 1);
      if (any) atomicAdd(&s_n[C], 1);
    } else {
      atomicAdd(&s_n[kT], 1);
    }
  }
  __syncthreads();
  if (threadIdx.x < kT && s_n[threadIdx.x]) atomicAdd(&h[PINN_FS_H_NCAL + threadIdx.x], (unsigned long long)s_n[threadIdx.x]);
  if (threadIdx.x == kT && s_n[kT]) atomicAdd(&h[5], (unsigned long long)s_n[kT]);
}

__global__ void fs_offsets_kernel(long long* __restrict__ h, int C, int kind, unsigned long long seed, int randomized,
                                  unsigned long long* __restrict__ cursor) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  h[0] = PINN_FS_MAGIC; h[1] = C; h[2] = kind; h[3] = (long long)seed; h[4] = randomized;
  long long o = 0, status = 0;
  for (int c = 0; c <= C; ++c) {
    const long long nc = h[PINN_FS_H_NCAL + c];
    if (c < C && nc > PINN_FS_MAX_CAL) status = 1;
    h[PINN_FS_H_OFFSET + c] = o;
    o += (nc + kLine - 1) / kLine * kLine;
    cursor[c] = 0;
  }
  h[6] = status;
}

__global__ __launch_bounds__(kBuildThreads) void fs_place_kernel(const double* __restrict__ sc, const double* __restrict__ any,
                                                                 const long long* __restrict__ cls, long long n, int C,
                                                                 const long long* __restrict__ h, double* __restrict__ tab,
                                                                 unsigned long long* __restrict__ cursor) {
  if (h[6] != 0) return;
  for (long long i = (long long)blockIdx.x * kBuildThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kBuildThreads) {
    const long long c = cls[i];
    if (c < 0 || c >= C) continue;
    const double v = sc[i * C + c];
    if (v != v) continue;
    if (any) {
      const double w = any[i];
      if (w != w) continue;
      tab[h[PINN_FS_H_OFFSET + C] + (long long)atomicAdd(&cursor[C], 1ULL)] = w + 0.0;
    }
    tab[h[PINN_FS_H_OFFSET + c] + (long long)atomicAdd(&cursor[c], 1ULL)] = v + 0.0;
  }
}

// one pass of the merge sort: runs of `width` entries of every table (grid y) merge in pairs from src into dst; an entry's
// place is its rank in its own run plus the entries of the sibling run below it (left run) or not above it (right run)
__global__ __launch_bounds__(kBuildThreads) void fs_merge_kernel(const long long* __restrict__ h, const double* __restrict__ src,
                                                                 double* __restrict__ dst, long long width) {
  if (h[6] != 0) return;
  const int c = blockIdx.y;
  const long long n = h[PINN_FS_H_NCAL + c], off = h[PINN_FS_H_OFFSET + c];
  const double* __restrict__ S = src + off;
  double* __restrict__ Dd = dst + off;
  for (long long i = (long long)blockIdx.x * kBuildThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kBuildThreads) {
    const double key = S[i];
    const long long base = i / (2 * width) * (2 * width), mid = base + width < n ? base + width : n;
    const long long end = base + 2 * width < n ? base + 2 * width : n;
    long long lo, hi;
    if (i < mid) {                            // left run: entries of the right run below the key
      lo = mid; hi = end;
      while (lo < hi) { const long long m = (lo + hi) >> 1; if (S[m] < key) lo = m + 1; else hi = m; }
      Dd[i + (lo - mid)] = key;
    } else {                                  // right run: entries of the left run not above the key
      lo = base; hi = mid;
      while (lo < hi) { const long long m = (lo + hi) >> 1; if (S[m] <= key) lo = m + 1; else hi = m; }
      Dd[(i - mid) + lo] = key;
    }
  }
}

// ---- host side
inline long long table_words(long long n, int C) { return 2 * n + (long long)kLine * (C + 1); }

// fills P from the host arguments and picks the regime; returns the LDS bytes in *lds
inline int make_cal(const void* d_state, const long long* n_cal, const long long* kmin, int C, int L, int kind, int randomized,
                    unsigned long long seed, int draw, long long first, int regime, long long n, int lds_cap, bool density, Cal* P,
                    size_t* lds) {
  if (C < 1 || C > kC || kind < PINN_FS_LAC || kind > PINN_FS_DENSITY || (kind == PINN_FS_DENSITY) != density) return PINN_E_ARG;
  if (regime < PINN_FS_REGIME_AUTO || regime > PINN_FS_REGIME_GLOBAL || misaligned8(d_state)) return PINN_E_ARG;
  if (draw != PINN_FS_DRAW_CAL && draw != PINN_FS_DRAW_TEST) return PINN_E_ARG;
  *P = Cal{};
  P->C = C; P->L = L; P->kind = kind; P->randomized = randomized != 0 && kind == PINN_FS_APS; P->draw = draw;
  P->seed_lo = (unsigned)seed; P->seed_hi = (unsigned)(seed >> 32); P->first = first;
  *lds = 0;
  if (!d_state) {
    P->regime = PINN_FS_REGIME_GLOBAL;
    return L == 0 ? PINN_OK : PINN_E_ARG;
  }
  if (L < 1 || L > kL || !n_cal || !kmin) return PINN_E_ARG;
  long long o = 0, so = 0;
  for (int c = 0; c <= C; ++c) {
    const long long nc = n_cal[c];
    if (nc < 0 || nc > (c < C ? (long long)PINN_FS_MAX_CAL : (long long)C * PINN_FS_MAX_CAL)) return PINN_E_ARG;
    P->n[c] = (int)nc; P->off[c] = (int)o; P->soff[c] = (int)so;
    o += pad_line(nc);
    so += (nc + kLine - 1) / kLine;
  }
  for (int c = 0; c < C; ++c)
    for (int l = 0; l < L; ++l) {
      const long long k = kmin[c * L + l];
      if (k < 0 || k > n_cal[c] + 1) return PINN_E_ARG;
      P->kmin[c * kL + l] = (int)k;
    }
  P->tab = reinterpret_cast<const double*>(d_state) + PINN_FS_HEADER;
  const bool fits_all = o <= lds_cap, fits_sampled = so <= lds_cap;
  if (regime == PINN_FS_REGIME_AUTO)          // as measured: small tables under many rows are staged, nothing else
    regime = (n >= PINN_FS_STAGE_MIN_ROWS && fits_all && o <= PINN_FS_AUTO_LDS_ENTRIES) ? PINN_FS_REGIME_LDS : PINN_FS_REGIME_GLOBAL;
  if ((regime == PINN_FS_REGIME_LDS && !fits_all) || (regime == PINN_FS_REGIME_SAMPLED && !fits_sampled)) return PINN_E_ARG;
  P->regime = regime;
  P->staged = regime == PINN_FS_REGIME_LDS ? (int)o : (regime == PINN_FS_REGIME_SAMPLED ? (int)so : 0);
  *lds = (size_t)P->staged * sizeof(double);
  return PINN_OK;
}

inline int make_out(const long long* d_y, int* d_count, unsigned short* d_mask, unsigned char* d_size, unsigned char* d_novel,
                    unsigned char* d_missing, double* d_scores, long long* d_tally, int* d_any_count, bool ranks, Out* o) {
  if (misaligned8(d_y) || misaligned8(d_scores) || misaligned8(d_tally) || ((unsigned long long)d_count & 3) || ((unsigned long long)d_mask & 1) ||
      ((unsigned long long)d_any_count & 3))
    return PINN_E_ARG;
  if (d_y && !d_tally) return PINN_E_ARG;
  if (!ranks && (d_y || d_count || d_mask || d_size || d_novel || d_tally || d_any_count)) return PINN_E_ARG;
  *o = Out{d_y, d_count, d_mask, d_size, d_novel, d_missing, d_scores, reinterpret_cast<unsigned long long*>(d_tally), d_any_count};
  return PINN_OK;
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_fs_state_bytes(long long n_cal, int n_classes) {
  using namespace pinn;
  if (n_classes < 1 || n_classes > kC || n_cal < 0 || n_cal > (long long)n_classes * PINN_FS_MAX_CAL) return 0;
  return align256((size_t)(PINN_FS_HEADER + table_words(n_cal, n_classes)) * sizeof(double));
}

extern "C" size_t pinn_fs_workspace_bytes(long long n, int n_classes) {
  using namespace pinn;
  if (n_classes < 1 || n_classes > kC || n < 0 || n > (long long)n_classes * PINN_FS_MAX_CAL) return 0;
  return 256 + align256((size_t)table_words(n, n_classes) * sizeof(double));
}

extern "C" int pinn_fs_build(const double* d_scores, const double* d_any, const long long* d_class, long long n, int n_classes, int kind,
                             unsigned long long seed, int randomized, void* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  const int C = n_classes;
  if (C < 1 || C > kC || n < 0 || n > (long long)C * PINN_FS_MAX_CAL || kind < PINN_FS_LAC || kind > PINN_FS_DENSITY) return PINN_E_ARG;
  if (!d_state || !d_ws || misaligned8(d_state) || misaligned8(d_ws) || misaligned8(d_scores) || misaligned8(d_any) || misaligned8(d_class))
    return PINN_E_ARG;
  if (n > 0 && (!d_scores || !d_class)) return PINN_E_ARG;
  if (ws_bytes < pinn_fs_workspace_bytes(n, C)) return PINN_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  long long* h = reinterpret_cast<long long*>(d_state);
  double* tab = reinterpret_cast<double*>(d_state) + PINN_FS_HEADER;
  unsigned long long* cursor = reinterpret_cast<unsigned long long*>(d_ws);
  double* buf = reinterpret_cast<double*>(reinterpret_cast<char*>(d_ws) + 256);
  clear_error();
  if (hipMemsetAsync(d_state, 0, PINN_FS_HEADER * sizeof(double), s) != hipSuccess) return launch_status();
  const int blocks = row_blocks(n, kBuildThreads, kBlocks);
  if (n > 0)
    hipLaunchKernelGGL(fs_count_kernel, dim3(blocks), dim3(kBuildThreads), 0, s, d_scores, d_any, d_class, n, C, reinterpret_cast<unsigned long long*>(h));
  hipLaunchKernelGGL(fs_offsets_kernel, dim3(1), dim3(1), 0, s, h, C, kind, seed, randomized != 0 ? 1 : 0, cursor);
  if (n > 0) {
    hipLaunchKernelGGL(fs_place_kernel, dim3(blocks), dim3(kBuildThreads), 0, s, d_scores, d_any, d_class, n, C, h, tab, cursor);
    // runs double until they hold the longest table a call of n rows can make; an even number of passes ends in the state
    const long long longest = d_any ? n : (n < PINN_FS_MAX_CAL ? n : (long long)PINN_FS_MAX_CAL);
    int passes = 0;
    for (long long w = 1; w < longest; w *= 2) ++passes;
    passes += passes & 1;
    double *src = tab, *dst = buf;
    long long w = 1;
    for (int p = 0; p < passes; ++p, w *= 2) {
      hipLaunchKernelGGL(fs_merge_kernel, dim3(blocks, C + 1), dim3(kBuildThreads), 0, s, h, src, dst, w);
      double* tmp = src; src = dst; dst = tmp;
    }
  }
  return launch_status();
}

extern "C" int pinn_fs_rank(const double* d_y_prob, long long n, int n_classes, const void* d_state, const long long* n_cal,
                            const long long* kmin, int n_levels, int kind, int randomized, unsigned long long seed, int draw_kind,
                            long long first, int regime, const long long* d_y, int* d_count, unsigned short* d_mask, unsigned char* d_size,
                            unsigned char* d_novel, unsigned char* d_missing, double* d_scores, long long* d_tally, void* stream) {
  using namespace pinn;
  Cal P;
  Out o;
  size_t lds;
  if (n < 0 || n > kMaxRows || first < 0 || misaligned8(d_y_prob) || (n > 0 && !d_y_prob)) return PINN_E_ARG;
  int rc = make_cal(d_state, n_cal, kmin, n_classes, n_levels, kind, randomized, seed, draw_kind, first, regime, n, PINN_FS_LDS_ENTRIES, false, &P,
                    &lds);
  if (rc != PINN_OK) return rc;
  rc = make_out(d_y, d_count, d_mask, d_size, d_novel, d_missing, d_scores, d_tally, nullptr, d_state != nullptr, &o);
  if (rc != PINN_OK) return rc;
  if (n == 0) return PINN_OK;
  clear_error();
  hipLaunchKernelGGL(fs_rank_kernel, dim3((unsigned)row_blocks(n, kTile, kBlocks)), dim3(kTile), lds, (hipStream_t)stream, d_y_prob, n, P, o);
  return launch_status();
}

extern "C" int pinn_fs_gmm(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                           const long long* d_row_index, long long n, int n_comp, const double* d_gmm_state, const double* d_map,
                           int n_classes, const double* d_logmap, const void* d_state, const long long* n_cal, const long long* kmin,
                           int n_levels, int kind, int randomized, unsigned long long seed, int draw_kind, long long first, int regime,
                           const long long* d_y, int* d_count, unsigned short* d_mask, unsigned char* d_size, unsigned char* d_novel,
                           unsigned char* d_missing, double* d_scores, long long* d_tally, double* d_y_prob, long long* d_y_pred,
                           double* d_log_prob_norm, double* d_any_score, int* d_any_count, void* stream) {
  using namespace pinn;
  Rows a;
  Cal P;
  Out o;
  size_t lds;
  int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, n_comp, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (n > kMaxRows || first < 0 || !d_gmm_state || !d_map || misaligned8(d_gmm_state) || misaligned8(d_map) || misaligned8(d_logmap) ||
      misaligned8(d_y_prob) || misaligned8(d_y_pred) || misaligned8(d_log_prob_norm) || misaligned8(d_any_score))
    return PINN_E_ARG;
  if ((kind == PINN_FS_DENSITY) != (d_logmap != nullptr)) return PINN_E_ARG;
  rc = make_cal(d_state, n_cal, kmin, n_classes, n_levels, kind, randomized, seed, draw_kind, first, regime, n, PINN_FS_GMM_LDS_ENTRIES,
                kind == PINN_FS_DENSITY, &P, &lds);
  if (rc != PINN_OK) return rc;
  if (kind != PINN_FS_DENSITY && (d_any_score || d_any_count)) return PINN_E_ARG;
  rc = make_out(d_y, d_count, d_mask, d_size, d_novel, d_missing, d_scores, d_tally, d_any_count, d_state != nullptr, &o);
  if (rc != PINN_OK) return rc;
  if (n == 0) return PINN_OK;
  clear_error();
  hipLaunchKernelGGL(fs_gmm_kernel, dim3((unsigned)row_blocks(n, kGmmTile, kBlocks)), dim3(kGmmTile), lds, (hipStream_t)stream, a, d_gmm_state, d_map,
                     d_logmap, P, o, d_y_prob, d_y_pred, d_log_prob_norm, d_any_score);
  return launch_status();
}
