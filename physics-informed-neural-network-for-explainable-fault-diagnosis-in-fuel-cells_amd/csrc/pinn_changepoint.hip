// pinn_changepoint.hip -- penalised change-point segmentation of the rows by exact optimal partitioning (with PELT's pruning)
//   pinn_cp_segment   prefix sums of the centred, standardised rows per segment (three launches), then the solver: one
//                     workgroup per (segment, penalty), continued by further queued launches from its workspace
//   pinn_cp_window    one segment of at most PINN_CP_MAX_WINDOW rows, prefix sums included, in one launch of one workgroup
//
// The statement of the problem, the sum orders, the pruning rule and the status bits are in include/pinn_hip.h;
// changepoint.py's host backend states the same solver in numpy.  A workgroup reads nothing another workgroup of the same
// launch writes and uses no float atomics.
//
// The solver's block: the 64 lanes of a wave are the block's steps, each with S(t), Q(t) of its step in registers.  The
// candidates known before the block are staged 256 at a time in LDS, column by column (S_q of candidate j at buf[q * 256 + j]:
// the staging stores are conflict-free and every read in the evaluation loop is one address for the whole wave, a broadcast);
// each wave takes 64 of them in ascending order, so a strict < keeps the smallest s on a tie inside a wave and the four
// waves merge on (value, s).  Wave 0 then finishes the triangular part: at iteration i lane i's F is final, it is broadcast
// with S, Q of its step and the later lanes take it as a candidate.  Three barriers per block and two per 256 candidates in
// each of the two passes over the list (evaluation, compaction), where the step-by-step loop has two per step.
// Built with -ffp-contract=off: every operation is rounded on its own.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = PINN_CP_TILE, kBlock = PINN_CP_BLOCK, kMaxD = PINN_CP_MAX_FEAT, kCols = 2 * kMaxD;
constexpr int kHdr = 8;                                         // 8-byte words of a pair's header: next step, list length, evaluations, done
constexpr long long kMaxLaunches = 1 << 16;

static_assert(kTile == kThreads && kBlock == 64 && kMaxD == kRowsMaxD, "one thread per tile row, one lane per step");

struct CpArgs {
  Rows a;
  const long long* ss;                                          // device segment starts (NULL: one segment)
  long long ns;
  long long ring_start, ring_size;                              // ring_size > 0: position j reads row (ring_start + j) mod ring_size
  double mu[kMaxD], sigma[kMaxD];
  int scale, kind, min_len, prune, block_steps, n_pen, first;
  long long max_len, cap, cp_cap, stride;                       // stride = n + segments: rows of the prefix table, words of a penalty's F, last, list
  double var_floor;
  double pen[PINN_CP_MAX_PEN];
  double *pre, *ttot, *F;
  int *tflag, *sflag, *last, *cand;
  long long* hdr;
  double* outF;
  long long *ncp, *cp, *evals, *status;
};

struct Shared {
  double buf[kCols * kThreads];                                 // a tile's rows [256][2 D], or 256 staged candidates [2 D][256]
  double cF[kThreads];
  int cs[kThreads];
  double wbv[kWaves][kBlock];
  int wbs[kWaves][kBlock];
  long long wev[kWaves];
  int wcnt[kWaves];
  int L;
};

__device__ __forceinline__ long long tile_slot(long long lo, long long seg, long long tile) { return lo / kTile + seg + tile; }

// z of position j: the standardised columns; false when the row reads nothing or a z is not finite
__device__ __forceinline__ bool read_z(const CpArgs& g, long long j, double z[kMaxD]) {
  const long long p = g.ring_size > 0 ? (g.ring_start + j) % g.ring_size : j;
  bool ok = load_row(g.a, p, z);
#pragma unroll
  for (int d = 0; d < kMaxD; ++d) {
    if (d < g.a.D) {
      if (g.scale) z[d] = (z[d] - g.mu[d]) / g.sigma[d];
      ok = ok && isfinite(z[d]);
    }
  }
  return ok;
}

// one tile of a segment [lo, lo + m): the running sums inside the tile to rows base + 1 + j of the prefix table, the tile's totals and flag
__device__ void tile_scan(const CpArgs& g, long long lo, long long m, long long base, long long tile, long long slot, Shared& sh) {
  const int D = g.a.D, C = 2 * D, tid = threadIdx.x;
  double z0[kMaxD], z[kMaxD];
  read_z(g, lo, z0);
  const long long j = tile * kTile + tid;
  bool bad = false;
  if (j < m) bad = !read_z(g, lo + j, z);
#pragma unroll
  for (int d = 0; d < kMaxD; ++d) {
    if (d < D) {
      const double c = j < m ? z[d] - z0[d] : 0.0;
      sh.buf[tid * kCols + d] = c;
      sh.buf[tid * kCols + D + d] = c * c;
    }
  }
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  if (tid < C) {
    double acc = 0.0;
    for (int i = 0; i < kTile; ++i) {
      acc += sh.buf[i * kCols + tid];
      sh.buf[i * kCols + tid] = acc;
    }
    g.ttot[slot * C + tid] = acc;
  }
  __syncthreads();
  if (j < m)
    for (int q = 0; q < C; ++q) g.pre[(base + 1 + j) * C + q] = sh.buf[tid * kCols + q];
  if (tile == 0 && tid < C) g.pre[base * C + tid] = 0.0;
  if (tid == 0) g.tflag[slot] = any_bad;
  __syncthreads();                                              // buf is free for the next tile
}

// the tile totals of a segment to exclusive offsets, tile by tile; the segment's flag.  Threads 0 .. 2 D - 1 and thread 0.
__device__ void tile_offsets(const CpArgs& g, long long lo, long long m, long long seg) {
  const int C = 2 * g.a.D, tid = threadIdx.x;
  const long long tiles = (m + kTile - 1) / kTile, s0 = tile_slot(lo, seg, 0);
  if (tid < C) {
    double acc = 0.0;
    for (long long k = 0; k < tiles; ++k) {
      const double t = g.ttot[(s0 + k) * C + tid];
      g.ttot[(s0 + k) * C + tid] = acc;
      acc += t;
    }
  }
  if (tid == 0) {
    int bad = 0;
    for (long long k = 0; k < tiles; ++k) bad |= g.tflag[s0 + k];
    g.sflag[seg] = bad;
  }
}

__device__ void tile_finish(const CpArgs& g, long long lo, long long m, long long base, long long tile, long long slot) {
  const int C = 2 * g.a.D;
  const long long j = tile * kTile + threadIdx.x;
  if (j < m)
    for (int q = 0; q < C; ++q) g.pre[(base + 1 + j) * C + q] = g.ttot[slot * C + q] + g.pre[(base + 1 + j) * C + q];
}

__global__ __launch_bounds__(kThreads) void cp_tile_kernel(CpArgs g) {
  __shared__ Shared sh;
  const long long seg = blockIdx.y, lo = seg_begin(g.ss, seg), m = seg_next(g.ss, g.ns, seg, g.a.n) - lo;
  const long long tile = blockIdx.x;
  if (tile * kTile >= m) return;
  tile_scan(g, lo, m, lo + seg, tile, tile_slot(lo, seg, tile), sh);
}

__global__ __launch_bounds__(64) void cp_offsets_kernel(CpArgs g) {
  const long long seg = blockIdx.x, lo = seg_begin(g.ss, seg), m = seg_next(g.ss, g.ns, seg, g.a.n) - lo;
  tile_offsets(g, lo, m, seg);
}

__global__ __launch_bounds__(kThreads) void cp_finish_kernel(CpArgs g) {
  const long long seg = blockIdx.y, lo = seg_begin(g.ss, seg), m = seg_next(g.ss, g.ns, seg, g.a.n) - lo;
  const long long tile = blockIdx.x;
  if (tile * kTile >= m) return;
  tile_finish(g, lo, m, lo + seg, tile, tile_slot(lo, seg, tile));
}

// C(s, t) from the prefix rows at s (ps) and t (pt): [S_0 .. S_{D-1}, Q_0 .. Q_{D-1}] each, len = t - s
__device__ __forceinline__ double seg_cost(int kind, int D, const double ps[kCols], const double pt[kCols], double len, double var_floor) {
  const double inv = 1.0 / len;
  double c = 0.0;
#pragma unroll
  for (int d = 0; d < kMaxD; ++d) {
    if (d < D) {
      const double dS = pt[d] - ps[d], dQ = pt[kMaxD + d] - ps[kMaxD + d];
      const double x = dQ - (dS * dS) * inv;
      const double ssq = x > 0.0 ? x : 0.0;
      if (kind == PINN_CP_MEAN) {
        c += ssq;
      } else {
        const double vv = ssq * inv;
        const double v = vv > var_floor ? vv : var_floor;
        c += len * log(v) + ssq / v;
      }
    }
  }
  return c;
}

// a prefix row into registers: S at [0, D), Q at [kMaxD, kMaxD + D)
__device__ __forceinline__ void load_pre(const double* __restrict__ row, int D, double p[kCols]) {
#pragma unroll
  for (int d = 0; d < kMaxD; ++d) {
    p[d] = d < D ? row[d] : 0.0;
    p[kMaxD + d] = d < D ? row[D + d] : 0.0;
  }
}

__device__ __forceinline__ bool better(double v, int s, double bv, int bs) { return v < bv || (v == bv && s < bs); }

// the (segment, penalty) pair of this workgroup, from its state in the workspace until it is finished or `cap` is reached
__device__ void solve_pair(const CpArgs& g, long long seg, int pen, long long lo, long long m, Shared& sh) {
  const int D = g.a.D, C = 2 * D, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long base = lo + seg, pair = seg * g.n_pen + pen;
  const double* pre = g.pre + base * C;                         // row t of the segment's prefix table: pre + t C, t = 0 .. m
  double* F = g.F + (long long)pen * g.stride + base;           // m + 1 words each
  int* last = g.last + (long long)pen * g.stride + base;
  int* cand = g.cand + (long long)pen * g.stride + base;
  long long* hdr = g.hdr + pair * kHdr;
  const double beta = g.pen[pen], inf = INFINITY;
  const int B = g.block_steps, min_len = g.min_len;
  const long long max_len = g.max_len > 0 ? g.max_len : m;

  long long t0 = 0, evals = 0;
  int L = 0;
  if (g.first) {
    if (g.sflag[seg]) {
      if (tid == 0) {
        g.outF[pair] = quiet_nan(); g.ncp[pair] = 0; g.evals[pair] = 0; g.status[pair] = PINN_CP_BAD_ROW;
        hdr[0] = m; hdr[1] = 0; hdr[2] = 0; hdr[3] = 1;
      }
      return;
    }
    if (tid == 0) F[0] = -beta;
    __syncthreads();
  } else {
    if (hdr[3] != 0) return;                                    // uniform: finished in an earlier launch
    t0 = hdr[0]; L = (int)hdr[1]; evals = hdr[2];
  }

  long long ev = 0, work = 0;
  while (t0 < m) {
    const long long t1 = t0 + B < m ? t0 + B : m;
    const int nb = (int)(t1 - t0);
    // the candidates that become admissible in this block and are known before it: s = t0 + 1 - min_len + lane <= t0
    if (wave == 0) {
      const long long s = t0 + 1 - min_len + lane;
      const bool ok = lane < nb && s >= 0 && s <= t0 && F[s] < inf;
      const unsigned long long bal = __ballot(ok);
      if (ok) cand[L + __popcll(bal & ((1ull << lane) - 1ull))] = (int)s;     // at most one entry per s <= t0: inside the m + 1 words
      if (lane == 0) sh.L = L + __popcll(bal);
    }
    __syncthreads();
    L = sh.L;
    const int L_block = L;

    const long long t = t0 + 1 + lane;                          // this lane's step
    const bool valid = lane < nb;
    double pt[kCols];
    load_pre(pre + (valid ? t : t0) * C, D, pt);
    double bv = inf;
    int bs = INT_MAX;
    for (int i0 = 0; i0 < L; i0 += kThreads) {
      const int i = i0 + tid;
      if (i < L) {
        const int s = cand[i];
        sh.cs[tid] = s;
        sh.cF[tid] = F[s];
        for (int q = 0; q < D; ++q) {
          sh.buf[q * kThreads + tid] = pre[(long long)s * C + q];
          sh.buf[(kMaxD + q) * kThreads + tid] = pre[(long long)s * C + D + q];
        }
      }
      __syncthreads();
      const int cnt = L - i0 < kThreads ? L - i0 : kThreads;
      const int j1 = cnt < wave * 64 + 64 ? cnt : wave * 64 + 64;
      for (int j = wave * 64; j < j1; ++j) {
        const int s = sh.cs[j];
        const long long len = t - s;
        if (valid && len >= min_len && len <= max_len) {
          double ps[kCols];
#pragma unroll
          for (int d = 0; d < kMaxD; ++d) {
            ps[d] = d < D ? sh.buf[d * kThreads + j] : 0.0;
            ps[kMaxD + d] = d < D ? sh.buf[(kMaxD + d) * kThreads + j] : 0.0;
          }
          const double v = (sh.cF[j] + seg_cost(g.kind, D, ps, pt, (double)len, g.var_floor)) + beta;
          ++ev;
          if (v < bv) { bv = v; bs = s; }                       // ascending s inside a wave: a tie keeps the smaller
        }
      }
      __syncthreads();
    }
    sh.wbv[wave][lane] = bv;
    sh.wbs[wave][lane] = bs;
    __syncthreads();

    if (wave == 0) {
#pragma unroll
      for (int w = 1; w < kWaves; ++w)
        if (better(sh.wbv[w][lane], sh.wbs[w][lane], bv, bs)) { bv = sh.wbv[w][lane]; bs = sh.wbs[w][lane]; }
      // the triangular part: candidate s = t0 + 1 + i is lane i's step; its F is final once the candidates before it are in
      for (int i = 0; (long long)i + min_len < nb; ++i) {
        const double Fs = __shfl(bv, i, 64);
        double ps[kCols];
#pragma unroll
        for (int d = 0; d < kMaxD; ++d) {
          ps[d] = d < D ? __shfl(pt[d], i, 64) : 0.0;
          ps[kMaxD + d] = d < D ? __shfl(pt[kMaxD + d], i, 64) : 0.0;
        }
        const long long len = lane - i;
        if (Fs < inf && valid && len >= min_len && len <= max_len) {
          const double v = (Fs + seg_cost(g.kind, D, ps, pt, (double)len, g.var_floor)) + beta;
          ++ev;
          if (v < bv) { bv = v; bs = (int)(t0 + 1 + i); }
        }
      }
      if (valid) {
        F[t] = bv;
        last[t] = bv < inf ? bs : -1;
      }
      // the candidates of this block that became admissible inside it: s in (t0, t1 - min_len]
      const bool ok = valid && t + min_len <= t1 && bv < inf;
      const unsigned long long bal = __ballot(ok);
      if (ok) cand[L + __popcll(bal & ((1ull << lane) - 1ull))] = (int)t;
      if (lane == 0) sh.L = L + __popcll(bal);
    }
    __syncthreads();
    L = sh.L;

    // compaction: the max_len rule and, with prune, the test at t* = t1 + 1 - min_len
    const long long tstar = t1 + 1 - min_len, lowest = t1 + 1 - max_len;
    const bool test = g.prune != 0 && tstar >= 1;
    double pstar[kCols];
    load_pre(pre + (test ? tstar : 0) * C, D, pstar);
    const double Fstar = test ? F[tstar] : inf;
    int newL = 0;
    for (int i0 = 0; i0 < L; i0 += kThreads) {
      const int i = i0 + tid;
      int s = 0;
      bool keep = false;
      if (i < L) {
        s = cand[i];
        keep = s >= lowest;
        if (keep && test && tstar - s >= min_len) {
          double ps[kCols];
          load_pre(pre + (long long)s * C, D, ps);
          const double v = F[s] + seg_cost(g.kind, D, ps, pstar, (double)(tstar - s), g.var_floor);
          if (v > Fstar) keep = false;
        }
      }
      const unsigned long long bal = __ballot(keep);
      if (lane == 0) sh.wcnt[wave] = __popcll(bal);
      __syncthreads();                                          // every read of this chunk is done
      int off = newL, total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        if (w < wave) off += sh.wcnt[w];
        total += sh.wcnt[w];
      }
      if (keep) cand[off + __popcll(bal & ((1ull << lane) - 1ull))] = s;      // at or before its old place
      newL += total;
      __syncthreads();
    }
    L = newL;
    work += (long long)L_block * nb;
    t0 = t1;
    if (work >= g.cap) break;
  }

  // the evaluations of this launch
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ev += __shfl_xor(ev, o, 64);
  if (lane == 0) sh.wev[wave] = ev;
  __syncthreads();
  if (tid == 0) {
    for (int w = 0; w < kWaves; ++w) evals += sh.wev[w];
    hdr[0] = t0; hdr[1] = L; hdr[2] = evals;
    if (t0 >= m) {
      const double Fm = F[m];
      long long status = 0, k = 0;
      if (Fm < inf) {
        for (long long u = m; last[u] > 0; u = last[u]) ++k;
        long long idx = k;
        for (long long u = m; last[u] > 0; u = last[u]) {
          --idx;
          if (idx < g.cp_cap) g.cp[pair * g.cp_cap + idx] = lo + last[u];
        }
        if (k > g.cp_cap) status |= PINN_CP_OVERFLOW;
      } else {
        status |= PINN_CP_INFEASIBLE;
      }
      g.outF[pair] = Fm; g.ncp[pair] = k; g.evals[pair] = evals; g.status[pair] = status;
      hdr[3] = 1;
    } else {
      hdr[3] = 0;
    }
  }
}

__global__ __launch_bounds__(kThreads) void cp_solve_kernel(CpArgs g) {
  __shared__ Shared sh;
  const long long seg = blockIdx.y, lo = seg_begin(g.ss, seg), m = seg_next(g.ss, g.ns, seg, g.a.n) - lo;
  solve_pair(g, seg, (int)blockIdx.x, lo, m, sh);
}

__global__ __launch_bounds__(kThreads) void cp_window_kernel(CpArgs g) {
  __shared__ Shared sh;
  const long long m = g.a.n, tiles = (m + kTile - 1) / kTile;
  for (long long k = 0; k < tiles; ++k) tile_scan(g, 0, m, 0, k, k, sh);
  tile_offsets(g, 0, m, 0);
  __syncthreads();
  for (long long k = 0; k < tiles; ++k) tile_finish(g, 0, m, 0, k, k);
  __syncthreads();
  for (int pen = 0; pen < g.n_pen; ++pen) {
    solve_pair(g, 0, pen, 0, m, sh);
    __syncthreads();
  }
}

struct Layout {
  size_t pre, ttot, tflag, sflag, hdr, F, last, cand, total;
};

inline bool cp_sizes_ok(long long n, int D, long long ns, int n_pen) {
  return n >= 0 && D >= 1 && D <= kMaxD && ns >= 1 && ns <= PINN_CP_MAX_SEGMENTS && n_pen >= 1 && n_pen <= PINN_CP_MAX_PEN &&
         n + ns < (1LL << 31);
}

inline Layout cp_layout(long long n, int D, long long ns, int n_pen) {
  const size_t stride = (size_t)(n + ns), slots = (size_t)(n / kTile + ns + 1), C = 2 * (size_t)D;
  Layout l;
  size_t o = 0;
  l.pre = o;   o += align256(stride * C * sizeof(double));
  l.ttot = o;  o += align256(slots * C * sizeof(double));
  l.tflag = o; o += align256(slots * sizeof(int));
  l.sflag = o; o += align256((size_t)ns * sizeof(int));
  l.hdr = o;   o += align256((size_t)ns * n_pen * kHdr * sizeof(long long));
  l.F = o;     o += align256(stride * n_pen * sizeof(double));
  l.last = o;  o += align256(stride * n_pen * sizeof(int));
  l.cand = o;  o += align256(stride * n_pen * sizeof(int));
  l.total = o;
  return l;
}

inline bool finite_nonneg(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }

// the checks both entry points share after make_rows; fills everything of `g` but the segments, the ring and the workspace
inline int cp_common(const double* mu, const double* sigma, const pinn_cp_opts_t* opts, const double* penalties, int n_pen, double* d_F,
                     long long* d_n_cp, long long* d_cp, long long cp_cap, long long* d_evals, long long* d_status, CpArgs* g) {
  if (!opts || !penalties || n_pen < 1 || n_pen > PINN_CP_MAX_PEN || cp_cap < 0) return PINN_E_ARG;
  if (opts->kind != PINN_CP_MEAN && opts->kind != PINN_CP_MEANVAR) return PINN_E_ARG;
  if (opts->min_len < (opts->kind == PINN_CP_MEAN ? 1 : 2)) return PINN_E_ARG;
  if (opts->max_len < 0 || (opts->max_len != 0 && opts->max_len < opts->min_len)) return PINN_E_ARG;
  if (opts->block_steps < 0 || opts->block_steps > kBlock || opts->launch_evals < 0) return PINN_E_ARG;
  if (!finite_nonneg(opts->var_floor)) return PINN_E_ARG;
  for (int p = 0; p < n_pen; ++p)
    if (!finite_nonneg(penalties[p])) return PINN_E_ARG;
  if ((mu == nullptr) != (sigma == nullptr)) return PINN_E_ARG;
  g->scale = mu != nullptr;
  for (int d = 0; d < kMaxD; ++d) {
    g->mu[d] = 0.0;
    g->sigma[d] = 1.0;
    if (mu && d < g->a.D) {
      if (!(mu[d] >= -1.7976931348623157e308 && mu[d] <= 1.7976931348623157e308) || !(sigma[d] > 0.0 && sigma[d] <= 1.7976931348623157e308))
        return PINN_E_ARG;
      g->mu[d] = mu[d];
      g->sigma[d] = sigma[d];
    }
  }
  if (!d_F || !d_n_cp || !d_evals || !d_status || (cp_cap > 0 && !d_cp)) return PINN_E_ARG;
  if (misaligned8(d_F) || misaligned8(d_n_cp) || misaligned8(d_cp) || misaligned8(d_evals) || misaligned8(d_status)) return PINN_E_ARG;
  g->kind = opts->kind; g->min_len = opts->min_len; g->max_len = opts->max_len; g->prune = opts->prune;
  g->block_steps = opts->block_steps > 0 ? opts->block_steps : kBlock;
  g->cap = opts->launch_evals > 0 ? opts->launch_evals : PINN_CP_LAUNCH_EVALS;
  g->var_floor = opts->var_floor;
  g->n_pen = n_pen;
  for (int p = 0; p < PINN_CP_MAX_PEN; ++p) g->pen[p] = p < n_pen ? penalties[p] : 0.0;
  g->cp_cap = cp_cap;
  g->outF = d_F; g->ncp = d_n_cp; g->cp = d_cp; g->evals = d_evals; g->status = d_status;
  g->first = 1;
  return PINN_OK;
}

inline void cp_workspace(CpArgs* g, void* d_ws, long long n, long long ns) {
  const Layout l = cp_layout(n, g->a.D, ns, g->n_pen);
  char* w = static_cast<char*>(d_ws);
  g->stride = n + ns;
  g->pre = reinterpret_cast<double*>(w + l.pre);
  g->ttot = reinterpret_cast<double*>(w + l.ttot);
  g->tflag = reinterpret_cast<int*>(w + l.tflag);
  g->sflag = reinterpret_cast<int*>(w + l.sflag);
  g->hdr = reinterpret_cast<long long*>(w + l.hdr);
  g->F = reinterpret_cast<double*>(w + l.F);
  g->last = reinterpret_cast<int*>(w + l.last);
  g->cand = reinterpret_cast<int*>(w + l.cand);
}

}  // namespace
}  // namespace pinn

using namespace pinn;

extern "C" size_t pinn_cp_workspace_bytes(long long n, int n_feat, long long n_segments, int n_pen) {
  const long long ns = n_segments > 0 ? n_segments : (n_segments == 0 ? 1 : -1);
  if (n <= 0 || !cp_sizes_ok(n, n_feat, ns, n_pen)) return 0;
  return cp_layout(n, n_feat, ns, n_pen).total;
}

extern "C" int pinn_cp_segment(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                               const long long* d_row_index, long long n, const double* mu, const double* sigma,
                               const long long* seg_starts, const long long* d_seg_starts, long long n_segments,
                               const pinn_cp_opts_t* opts, const double* penalties, int n_pen, double* d_F, long long* d_n_cp,
                               long long* d_cp, long long cp_cap, long long* d_evals, long long* d_status, void* d_ws, size_t ws_bytes,
                               void* stream) {
  CpArgs g = {};
  int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, 1, d_row_index, n, &g.a);
  if (rc != PINN_OK) return rc;
  rc = cp_common(mu, sigma, opts, penalties, n_pen, d_F, d_n_cp, d_cp, cp_cap, d_evals, d_status, &g);
  if (rc != PINN_OK) return rc;
  if (n_segments < 0 || n_segments > PINN_CP_MAX_SEGMENTS || misaligned8(d_seg_starts) || misaligned8(d_ws)) return PINN_E_ARG;
  if (n_segments > 0 && (!seg_starts || !d_seg_starts)) return PINN_E_ARG;
  const long long ns = n_segments > 0 ? n_segments : 1;
  if (n == 0) return n_segments > 1 ? PINN_E_ARG : PINN_OK;
  long long longest = n;
  if (n_segments > 0) {
    if (seg_starts[0] != 0) return PINN_E_ARG;
    longest = 0;
    for (long long s = 0; s < n_segments; ++s) {
      const long long hi = s + 1 < n_segments ? seg_starts[s + 1] : n;
      if (hi <= seg_starts[s]) return PINN_E_ARG;               // descending, repeated or beyond the rows
      if (hi - seg_starts[s] > longest) longest = hi - seg_starts[s];
    }
  }
  if (!cp_sizes_ok(n, n_feat, ns, n_pen)) return PINN_E_ARG;
  if (!d_ws) return PINN_E_ARG;
  if (ws_bytes < cp_layout(n, n_feat, ns, n_pen).total) return PINN_E_WORKSPACE;
  g.ss = n_segments > 0 ? d_seg_starts : nullptr;
  g.ns = n_segments;
  cp_workspace(&g, d_ws, n, ns);

  // launches of the solver: the worst case of the longest segment over the cap, the cap raised until they are few enough
  const long long span = g.max_len > 0 && g.max_len + kBlock < longest + 1 ? g.max_len + kBlock : longest + 1;
  const double worst = (double)longest * (double)span;
  if (worst / (double)g.cap > (double)kMaxLaunches) g.cap = (long long)(worst / (double)kMaxLaunches) + 1;
  long long launches = (long long)(worst / (double)g.cap) + 1;

  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((longest + kTile - 1) / kTile);
  clear_error();
  hipLaunchKernelGGL(cp_tile_kernel, dim3(tiles, (unsigned)ns), dim3(kThreads), 0, st, g);
  hipLaunchKernelGGL(cp_offsets_kernel, dim3((unsigned)ns), dim3(64), 0, st, g);
  hipLaunchKernelGGL(cp_finish_kernel, dim3(tiles, (unsigned)ns), dim3(kThreads), 0, st, g);
  for (long long k = 0; k < launches; ++k) {
    g.first = k == 0;
    hipLaunchKernelGGL(cp_solve_kernel, dim3((unsigned)n_pen, (unsigned)ns), dim3(kThreads), 0, st, g);
  }
  return launch_status();
}

extern "C" int pinn_cp_window(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat, long long ring_start,
                              long long n, const double* mu, const double* sigma, const pinn_cp_opts_t* opts, const double* penalties,
                              int n_pen, double* d_F, long long* d_n_cp, long long* d_cp, long long cp_cap, long long* d_evals,
                              long long* d_status, void* d_ws, size_t ws_bytes, void* stream) {
  CpArgs g = {};
  int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, 1, nullptr, n, &g.a);
  if (rc != PINN_OK) return rc;
  rc = cp_common(mu, sigma, opts, penalties, n_pen, d_F, d_n_cp, d_cp, cp_cap, d_evals, d_status, &g);
  if (rc != PINN_OK) return rc;
  if (n > PINN_CP_MAX_WINDOW || ring_start < 0 || (ring_start > 0 && ring_start >= n_arr_rows) || misaligned8(d_ws)) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  if (!d_ws) return PINN_E_ARG;
  if (ws_bytes < cp_layout(n, n_feat, 1, n_pen).total) return PINN_E_WORKSPACE;
  g.ss = nullptr;
  g.ns = 0;
  g.ring_start = ring_start;
  g.ring_size = n_arr_rows;
  g.cap = LLONG_MAX;
  cp_workspace(&g, d_ws, n, 1);
  clear_error();
  hipLaunchKernelGGL(cp_window_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, g);
  return launch_status();
}
