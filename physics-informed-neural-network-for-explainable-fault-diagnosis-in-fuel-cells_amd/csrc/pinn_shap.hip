// Exact Shapley attributions on the device: which input made the model say so.  All 2^D coalitions of D <= 8 inputs are
// enumerated against a background set of B rows (the interventional value v(S; x) = mean over b of f(x on S, b elsewhere));
// nothing is sampled.  phi_j = sum over S of c_j(S) v(S) with c_j(S) = (|S| - 1)! (D - |S|)! / D! for j in S and
// -|S|! (D - |S| - 1)! / D! otherwise.  float64 throughout, every sum in a fixed order, no float atomics.
//   pinn_shap_gmm      f = the fault probabilities of pinn_gmm_posterior, fused: no hybrid row and no coalition value
//                      reaches HBM
//   pinn_shap_hybrid   any model, step 1: the hybrid rows of a chunk of rows, dense, float32 or float64
//   pinn_shap_reduce   any model, step 2: the model's outputs on those rows -> phi, base, fx
//
// The fused kernel.  A workgroup owns a tile of 128 rows (one thread per row) and one split of the background, whose rows
// it stages through LDS in blocks of 32.  The mixture's parameters and the label map are staged once per call as one
// padded record per component (shap_stage_kernel) and read with indices that are the same in every lane, i.e. through the
// scalar cache into SGPRs: held in LDS instead, their broadcast reads kept the LDS pipe of a CU busy for twice the time
// its four SIMDs need for the float64 arithmetic (DESIGN 3p has the two timings).  LDS holds what differs per lane, the K
// log densities of the hybrid row.  For every (row, background row) the thread walks the 2^D - 2 proper coalitions,
// evaluates the posterior of the hybrid row in the direct form (z - mu_k) U_k, the arithmetic of pinn_gmm_posterior with one
// exponential per component (responsibility = exp(lp_k - max) / sum instead of exp(lp_k - log_prob_norm)), and adds
// c_j(S) f(z) to its D x 4 accumulators: classes are taken four at a time (grid z), so that the accumulators stay in
// registers.  The direct form is chosen over the Gray-code update of (z - mu_k) U_k: every f(z) then carries the rounding
// of one posterior evaluation and nothing of the walk before it, so the 2 delta bound on phi holds with delta the
// posterior's own error; an updated residual would add up to 2^D roundings of cancelling terms.  The two end coalitions do
// not depend on the other operand: f(x) and f(b) are one pinn_gmm_posterior call each, and enter as (fx - base) / D.  The
// splits' sums go to the workspace and are added in split order, so the order of every sum depends on B alone: a row's
// bytes do not depend on which other rows are in the call.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_rows.h"
#include "pinn_gmm_state.h"

namespace pinn {
namespace {

constexpr int kTile = PINN_SHAP_TILE;         // rows per workgroup of the fused kernel = its threads
constexpr int kBg = PINN_SHAP_BG_BLOCK;       // background rows per LDS block
constexpr int kMaxSplit = PINN_SHAP_MAX_SPLIT;   // workgroups along the background = partial sums per output
constexpr int kCls = 4;                       // classes per pass of the fused kernel
constexpr int kMaxK = PINN_GMM_MAX_COMP, kMaxD = PINN_GMM_MAX_FEAT, kMaxC = PINN_GMM_MAX_CLASSES;
constexpr int kTri = kMaxD * (kMaxD + 1) / 2;
constexpr int kRedThreads = 256;

// timing ablation only (tools/build_variant.py with -DPINN_SHAP_NO_EXP, read by tools/time_shap.py --fused-only): the exponential
// of the fused kernel replaced by one multiply-add on the same operand, to read the share of exp in the kernel's time.
#ifdef PINN_SHAP_NO_EXP
#define PINN_SHAP_EXP(v) (1.0 + 1e-3 * (v))
#else
#define PINN_SHAP_EXP(v) exp(v)
#endif

// c_j(S) by |S|: in[s] for j in S (s >= 1), out[s] for j not in S (s <= D - 1, negative)
struct Weights {
  double in[kMaxD + 1], out[kMaxD + 1];
};

inline Weights make_weights(int D) {
  double f[kMaxD + 1];
  f[0] = 1.0;
  for (int i = 1; i <= kMaxD; ++i) f[i] = f[i - 1] * i;       // exact
  Weights w;
  for (int s = 0; s <= kMaxD; ++s) {
    w.in[s] = (s >= 1 && s <= D) ? f[s - 1] * f[D - s] / f[D] : 0.0;
    w.out[s] = (s <= D - 1) ? -(f[s] * f[D - s - 1] / f[D]) : 0.0;
  }
  return w;
}

// how the background is cut: blocks of kBg rows, `per` blocks to a split, `n` splits.  A function of B alone.
struct Split {
  long long blocks;
  int per, n;
};

inline Split make_split(long long B) {
  Split s;
  s.blocks = (B + kBg - 1) / kBg;
  s.per = (int)((s.blocks + kMaxSplit - 1) / kMaxSplit);
  s.n = (int)((s.blocks + s.per - 1) / s.per);
  return s;
}

// ---- the mixture as the fused kernel reads it: one record of doubles per component, padded to the kernel's DMAX and CMAX
// with zeros so that its loops need no bounds (a padded column adds 0 to the quadratic form, a padded class is never
// written): mu [DMAX], U [DMAX (DMAX + 1) / 2] (upper triangle by columns), logdet, log weight, map [CMAX].  Every index
// into it is the same in all lanes: the compiler reads a record through the scalar cache in a few wide loads, and the LDS
// is left to the per-lane log densities.
constexpr int kParWords = kMaxK * (kMaxD + kTri + 2 + kMaxC);

__host__ __device__ inline int rec_words(int DMAX, int CMAX) { return DMAX + DMAX * (DMAX + 1) / 2 + 2 + CMAX; }

__global__ __launch_bounds__(kRedThreads) void shap_stage_kernel(const double* __restrict__ st, const double* __restrict__ map, int K, int D,
                                                                 int C, int DMAX, int CMAX, double* __restrict__ par) {
  const int TM = DMAX * (DMAX + 1) / 2, R = rec_words(DMAX, CMAX);
  for (int e = threadIdx.x; e < K * R; e += kRedThreads) {
    const int k = e / R, o = e - k * R;
    double v = 0.0;
    if (o < DMAX) {
      if (o < D) v = st[st_means(K) + k * D + o];
    } else if (o < DMAX + TM) {
      int i, j;
      untri(o - DMAX, &i, &j);
      if (j < D) v = st[st_chol(K, D) + ((size_t)k * D + i) * D + j];
    } else if (o == DMAX + TM) {
      v = st[st_logdet(K, D) + k];
    } else if (o == DMAX + TM + 1) {
      v = log(st[st_weights() + k]);
    } else if (o - (DMAX + TM + 2) < C) {
      v = map[k * C + o - (DMAX + TM + 2)];
    }
    par[e] = v;
  }
}

// ---- the fused kernel: part [splits][n][D][C] = sum over the split's background rows and the proper coalitions of c_j(S) f(z)
template <int DMAX, int CMAX>
__global__ __launch_bounds__(kTile) void shap_gmm_kernel(Rows a, Rows bg, const double* __restrict__ par, int C, Weights w, int per,
                                                         double* __restrict__ part) {
  __shared__ double s_lp[kMaxK * kTile];
  __shared__ double s_b[kBg * DMAX];
  constexpr int TM = DMAX * (DMAX + 1) / 2, R = DMAX + TM + 2 + CMAX;
  const int K = a.K, D = a.D, t = threadIdx.x, c0 = blockIdx.z * kCls;

  const long long j = (long long)blockIdx.x * kTile + t;
  const bool live = j < a.n;
  double x[kMaxD];
  if (live) load_row(a, j, x);                                // a row that reads nothing: zeros here, NaN from its fx
  double acc[DMAX][kCls];
#pragma unroll
  for (int f = 0; f < DMAX; ++f)
#pragma unroll
    for (int cc = 0; cc < kCls; ++cc) acc[f][cc] = 0.0;

  const double cst = (double)D * 1.8378770664093453;          // D log(2 pi)
  const int nS = 1 << D;
  double* lp = s_lp + t;
  const long long blk0 = (long long)blockIdx.y * per, nblk = (bg.n + kBg - 1) / kBg;
  for (long long blk = blk0; blk < blk0 + per && blk < nblk; ++blk) {
    __syncthreads();
    if (t < kBg) {
      double xb[kMaxD];
      const long long p = blk * kBg + t;
      if (p < bg.n) {
        load_row(bg, p, xb);                                  // a position that reads nothing: NaN from the base
#pragma unroll
        for (int i = 0; i < DMAX; ++i) s_b[t * DMAX + i] = xb[i];
      }
    }
    __syncthreads();
    if (!live) continue;
    const long long left = bg.n - blk * kBg;
    const int nb = left < kBg ? (int)left : kBg;
    for (int bb = 0; bb < nb; ++bb) {
      double b[DMAX];
#pragma unroll
      for (int i = 0; i < DMAX; ++i) b[i] = s_b[bb * DMAX + i];
      for (int S = 1; S < nS - 1; ++S) {
        double z[DMAX];
#pragma unroll
        for (int i = 0; i < DMAX; ++i) z[i] = ((S >> i) & 1) ? x[i] : b[i];
        // log(w_k N(z | mu_k, Sigma_k)) as pinn_gmm_posterior has it
        double m = -INFINITY;
        for (int k = 0; k < K; ++k) {
          const double* __restrict__ mu = par + k * R;
          const double* __restrict__ U = mu + DMAX;
          double d[DMAX];
#pragma unroll
          for (int i = 0; i < DMAX; ++i) d[i] = z[i] - mu[i];
          double q = 0.0;
#pragma unroll
          for (int jj = 0; jj < DMAX; ++jj) {
            double y = 0.0;
#pragma unroll
            for (int i = 0; i <= jj; ++i) y += d[i] * U[tri(i, jj)];
            q += y * y;
          }
          const double v = (-0.5 * (cst + q) + mu[DMAX + TM]) + mu[DMAX + TM + 1];
          lp[k * kTile] = v;
          m = v > m ? v : m;
        }
        // responsibilities x map, not yet normalised: one exponential per component
        double sum = 0.0, v[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) v[c] = 0.0;
        for (int k = 0; k < K; ++k) {
          const double e = PINN_SHAP_EXP(lp[k * kTile] - m);            // NaN when every density underflowed, as the posterior
          const double* __restrict__ mp = par + k * R + (DMAX + TM + 2);
          sum += e;
#pragma unroll
          for (int c = 0; c < CMAX; ++c) v[c] += e * mp[c];
        }
        // clip(resp @ map, 1e-12, 1) renormalised (03:418-421); the classes of this pass are kept
        double y[kCls], tot = 0.0;
#pragma unroll
        for (int cc = 0; cc < kCls; ++cc) y[cc] = 0.0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
          double u = v[c] / sum;
          if (u == u) u = u < 1e-12 ? 1e-12 : (u > 1.0 ? 1.0 : u);
          tot += c < C ? u : 0.0;
#pragma unroll
          for (int cc = 0; cc < kCls; ++cc) y[cc] = (c == c0 + cc) ? u : y[cc];
        }
        const int s = __popc(S);
        const double w_in = w.in[s], w_out = w.out[s];
#pragma unroll
        for (int cc = 0; cc < kCls; ++cc) {
          const double u = y[cc] / tot;
#pragma unroll
          for (int f = 0; f < DMAX; ++f) acc[f][cc] += (((S >> f) & 1) ? w_in : w_out) * u;
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int f = 0; f < DMAX; ++f)
#pragma unroll
    for (int cc = 0; cc < kCls; ++cc)
      if (f < D && c0 + cc < C) part[(((size_t)blockIdx.y * a.n + j) * D + f) * C + c0 + cc] = acc[f][cc];
}

// base [C] = the mean of fb [B][C]: 256 contiguous chunks, then the chunk sums in order
__global__ __launch_bounds__(kRedThreads) void shap_base_kernel(const double* __restrict__ fb, long long B, int C, double* __restrict__ base) {
  __shared__ double s_s[kRedThreads];
  const int t = threadIdx.x;
  const long long len = (B + kRedThreads - 1) / kRedThreads;
  for (int c = 0; c < C; ++c) {
    double s = 0.0;
    for (long long p = t * len; p < (t + 1) * len && p < B; ++p) s += fb[p * C + c];
    s_s[t] = s;
    __syncthreads();
    if (t == 0) {
      double tot = 0.0;
      for (int q = 0; q < kRedThreads; ++q) tot += s_s[q];
      base[c] = tot / (double)B;
    }
    __syncthreads();
  }
}

// phi = (the splits' sums in split order) / B + (fx - base) / D; a NaN base (a background position that reads nothing)
// makes every output NaN
__global__ __launch_bounds__(kRedThreads) void shap_final_kernel(const double* __restrict__ part, int splits, long long n, int D, int C,
                                                                 long long B, double w_full, const double* __restrict__ base,
                                                                 double* __restrict__ fx, double* __restrict__ phi) {
  const long long DC = (long long)D * C, total = n * DC;
  for (long long e = (long long)blockIdx.x * kRedThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kRedThreads) {
    const long long j = e / DC;
    const int r = (int)(e - j * DC), f = r / C, c = r - f * C;
    double s = 0.0;
    for (int g = 0; g < splits; ++g) s += part[(size_t)g * total + e];
    const double bs = base[c];
    double fv = fx[j * C + c];
    if (bs != bs) fv = bs;
    phi[e] = s / (double)B + (fv - bs) * w_full;
    if (f == 0 && bs != bs) fx[j * C + c] = bs;
  }
}

// ---- the generic path
// out [(r 2^D + S) B + b][D]: row r of the chunk where bit i of S is set, background row b elsewhere
template <typename T>
__global__ __launch_bounds__(kRedThreads) void shap_hybrid_kernel(Rows a, Rows bg, long long row0, long long n_chunk, T* __restrict__ out) {
  const int D = a.D;
  const long long B = bg.n, total = (n_chunk << D) * B * D;
  for (long long e = (long long)blockIdx.x * kRedThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kRedThreads) {
    const long long h = e / D, q = h / B;
    const int i = (int)(e - h * D), S = (int)(q & ((1 << D) - 1));
    const long long b = h - q * B, r = q >> D;
    const bool own = (S >> i) & 1;
    const Rows& src = own ? a : bg;
    const long long p = own ? row0 + r : b;
    const long long row = src.ridx ? src.ridx[p] : p;
    const bool ok = row >= 0 && row < src.n_arr;
    out[e] = ok ? (T)src.arr[row * src.ld + src.col[i]] : (T)quiet_nan();
  }
}

// f [(r 2^D + S) B + b][C] -> v(S) = the mean over b in b order (the full coalition: its first value, which is f(x)), then
// phi_j = sum over S in S order of c_j(S) v(S).  One workgroup per row.
template <typename T>
__global__ __launch_bounds__(kRedThreads) void shap_reduce_kernel(const T* __restrict__ fv, int D, long long B, int C, Weights w,
                                                                  double* __restrict__ phi, double* __restrict__ base, double* __restrict__ fx) {
  __shared__ double s_v[(1 << kMaxD) * kMaxC];
  const int nS = 1 << D, t = threadIdx.x;
  const long long r = blockIdx.x;
  for (int idx = t; idx < nS * C; idx += kRedThreads) {
    const int S = idx / C, c = idx - S * C;
    const T* p = fv + ((size_t)(r * nS + S) * B) * C + c;
    double s;
    if (S == nS - 1) {
      s = (double)p[0];
    } else {
      s = 0.0;
      for (long long b = 0; b < B; ++b) s += (double)p[b * C];
      s = s / (double)B;
    }
    s_v[idx] = s;
  }
  __syncthreads();
  for (int idx = t; idx < D * C; idx += kRedThreads) {
    const int f = idx / C, c = idx - f * C;
    double s = 0.0;
    for (int S = 0; S < nS; ++S) {
      const int sz = __popc(S);
      s += (((S >> f) & 1) ? w.in[sz] : w.out[sz]) * s_v[S * C + c];
    }
    phi[r * D * C + idx] = s;
  }
  for (int c = t; c < C; c += kRedThreads) {
    fx[r * C + c] = s_v[(nS - 1) * C + c];
    if (base && r == 0) base[c] = s_v[c];
  }
}

inline int grid_for(long long total) {
  const long long g = (total + kRedThreads - 1) / kRedThreads;
  return (int)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

// the two row heads of an entry point: the same number of features in both
inline int make_pair(const double* d_arr, long long ld, long long n_arr, const int* cols, int n_feat, const long long* d_row_index, long long n,
                     const double* d_bg, long long ld_bg, long long n_bg_arr, const int* cols_bg, int n_feat_bg, const long long* d_bg_index,
                     long long n_bg, int n_comp, Rows* a, Rows* b) {
  int rc = make_rows(d_arr, ld, n_arr, cols, n_feat, n_comp, d_row_index, n, a);
  if (rc != PINN_OK) return rc;
  rc = make_rows(d_bg, ld_bg, n_bg_arr, cols_bg, n_feat_bg, n_comp, d_bg_index, n_bg, b);
  if (rc != PINN_OK) return rc;
  return (n_feat_bg != n_feat || n_bg < 1) ? PINN_E_ARG : PINN_OK;
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_shap_gmm_workspace_bytes(long long n_rows, long long n_background, int n_feat, int n_classes) {
  using namespace pinn;
  if (n_rows < 0 || n_background < 1 || n_feat < 1 || n_feat > kMaxD || n_classes < 1 || n_classes > kMaxC) return 0;
  const Split s = make_split(n_background);
  return align256(kParWords * sizeof(double)) + align256((size_t)n_background * n_classes * sizeof(double)) +
         align256((size_t)s.n * (size_t)n_rows * n_feat * n_classes * sizeof(double));
}

extern "C" int pinn_shap_gmm(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                             const long long* d_row_index, long long n, const double* d_bg, long long ld_bg, long long n_bg_rows,
                             const int* cols_bg, int n_feat_bg, const long long* d_bg_index, long long n_bg, int n_comp,
                             const double* d_state, const double* d_map, int n_classes, double* d_phi, double* d_base, double* d_fx,
                             void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  Rows a, b;
  const int rc = make_pair(d_arr, ld, n_arr_rows, cols, n_feat, d_row_index, n, d_bg, ld_bg, n_bg_rows, cols_bg, n_feat_bg, d_bg_index, n_bg,
                           n_comp, &a, &b);
  if (rc != PINN_OK) return rc;
  if (!d_state || !d_map || !d_phi || !d_base || !d_fx || !d_ws || n_classes < 1 || n_classes > kMaxC) return PINN_E_ARG;
  if (misaligned8(d_state) || misaligned8(d_map) || misaligned8(d_phi) || misaligned8(d_base) || misaligned8(d_fx) ||
      ((unsigned long long)d_ws & 255) != 0)
    return PINN_E_ARG;
  if (ws_bytes < pinn_shap_gmm_workspace_bytes(n, n_bg, n_feat, n_classes)) return PINN_E_WORKSPACE;
  if (n == 0) return PINN_OK;
  const long long tiles = (n + kTile - 1) / kTile;
  if (tiles > 0x7fffffffLL) return PINN_E_ARG;
  const int D = n_feat, C = n_classes;
  const Split s = make_split(n_bg);
  double* par = static_cast<double*>(d_ws);
  double* fb = reinterpret_cast<double*>(static_cast<char*>(d_ws) + align256(kParWords * sizeof(double)));
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(fb) + align256((size_t)n_bg * C * sizeof(double)));
  hipStream_t sm = (hipStream_t)stream;
  // the end coalitions: f(x) and f(b), the posterior itself
  int e = pinn_gmm_posterior(d_arr, ld, n_arr_rows, cols, n_feat, d_row_index, n, n_comp, d_state, d_map, C, nullptr, nullptr, d_fx, nullptr, stream);
  if (e != PINN_OK) return e;
  e = pinn_gmm_posterior(d_bg, ld_bg, n_bg_rows, cols_bg, n_feat, d_bg_index, n_bg, n_comp, d_state, d_map, C, nullptr, nullptr, fb, nullptr, stream);
  if (e != PINN_OK) return e;
  clear_error();
  const Weights w = make_weights(D);
  const dim3 grid((unsigned)tiles, (unsigned)s.n, (unsigned)((C + kCls - 1) / kCls));
  if (D > 1) {
    const int DMAX = D <= 4 ? 4 : 8, CMAX = C <= kCls ? kCls : kMaxC;
    hipLaunchKernelGGL(shap_stage_kernel, dim3(1), dim3(kRedThreads), 0, sm, d_state, d_map, n_comp, D, C, DMAX, CMAX, par);
    if (DMAX == 4 && CMAX == kCls)
      hipLaunchKernelGGL((shap_gmm_kernel<4, kCls>), grid, dim3(kTile), 0, sm, a, b, par, C, w, s.per, part);
    else if (DMAX == 4)
      hipLaunchKernelGGL((shap_gmm_kernel<4, kMaxC>), grid, dim3(kTile), 0, sm, a, b, par, C, w, s.per, part);
    else if (CMAX == kCls)
      hipLaunchKernelGGL((shap_gmm_kernel<8, kCls>), grid, dim3(kTile), 0, sm, a, b, par, C, w, s.per, part);
    else
      hipLaunchKernelGGL((shap_gmm_kernel<8, kMaxC>), grid, dim3(kTile), 0, sm, a, b, par, C, w, s.per, part);
  }
  hipLaunchKernelGGL(shap_base_kernel, dim3(1), dim3(kRedThreads), 0, sm, fb, n_bg, C, d_base);
  hipLaunchKernelGGL(shap_final_kernel, dim3(grid_for(n * D * C)), dim3(kRedThreads), 0, sm, part, D > 1 ? s.n : 0, n, D, C, n_bg, w.in[D],
                     d_base, d_fx, d_phi);
  return launch_status();
}

extern "C" int pinn_shap_hybrid(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                                const long long* d_row_index, long long n, const double* d_bg, long long ld_bg, long long n_bg_rows,
                                const int* cols_bg, int n_feat_bg, const long long* d_bg_index, long long n_bg, long long row0,
                                long long n_chunk, int f64, void* d_out, void* stream) {
  using namespace pinn;
  Rows a, b;
  const int rc = make_pair(d_arr, ld, n_arr_rows, cols, n_feat, d_row_index, n, d_bg, ld_bg, n_bg_rows, cols_bg, n_feat_bg, d_bg_index, n_bg,
                           1, &a, &b);
  if (rc != PINN_OK) return rc;
  if (row0 < 0 || n_chunk < 0 || row0 + n_chunk > n || !d_out || ((unsigned long long)d_out & (f64 ? 7 : 3)) != 0) return PINN_E_ARG;
  if (n_chunk > (0x7fffffffffffffffLL >> (n_feat + 4)) / n_bg) return PINN_E_ARG;     // the element count stays in 64 bits
  if (n_chunk == 0) return PINN_OK;
  clear_error();
  const long long total = (n_chunk << n_feat) * n_bg * n_feat;
  if (f64)
    hipLaunchKernelGGL(shap_hybrid_kernel<double>, dim3(grid_for(total)), dim3(kRedThreads), 0, (hipStream_t)stream, a, b, row0, n_chunk,
                       static_cast<double*>(d_out));
  else
    hipLaunchKernelGGL(shap_hybrid_kernel<float>, dim3(grid_for(total)), dim3(kRedThreads), 0, (hipStream_t)stream, a, b, row0, n_chunk,
                       static_cast<float*>(d_out));
  return launch_status();
}

extern "C" int pinn_shap_reduce(const void* d_f, int f64, long long n_chunk, int n_feat, long long n_bg, int n_classes, double* d_phi,
                                double* d_base, double* d_fx, void* stream) {
  using namespace pinn;
  if (n_chunk < 0 || n_chunk > 0x7fffffffLL || n_feat < 1 || n_feat > kMaxD || n_bg < 1 || n_classes < 1 || n_classes > kMaxC) return PINN_E_ARG;
  if (!d_f || !d_phi || !d_fx || ((unsigned long long)d_f & (f64 ? 7 : 3)) != 0 || misaligned8(d_phi) || misaligned8(d_base) || misaligned8(d_fx))
    return PINN_E_ARG;
  if (n_chunk == 0) return PINN_OK;
  clear_error();
  const Weights w = make_weights(n_feat);
  if (f64)
    hipLaunchKernelGGL(shap_reduce_kernel<double>, dim3((unsigned)n_chunk), dim3(kRedThreads), 0, (hipStream_t)stream,
                       static_cast<const double*>(d_f), n_feat, n_bg, n_classes, w, d_phi, d_base, d_fx);
  else
    hipLaunchKernelGGL(shap_reduce_kernel<float>, dim3((unsigned)n_chunk), dim3(kRedThreads), 0, (hipStream_t)stream,
                       static_cast<const float*>(d_f), n_feat, n_bg, n_classes, w, d_phi, d_base, d_fx);
  return launch_status();
}
