// ROC inference on the device: the integers behind DeLong's covariance of K AUCs and the stratified paired bootstrap.
//   pinn_auc_components   per classifier: tied groups of the ascending scores, a[i] / b[j] per row, group numbers, U2
//   pinn_auc_cross_sums   exact 128-bit sums of products of two component vectors, every pair k <= l
//   pinn_auc_bootstrap    a workgroup per resample: Philox draws, a histogram of the negatives by group, its scan, and
//                         the sum over the positive draws
//
// Everything is an integer: there is no float arithmetic in this file, the only atomics are integer adds (their sum does
// not depend on the order of arrival), and no workgroup waits on another.  The scans follow pinn_lr_roc (pinn_lr.hip): a
// launch sums tiles, a one-workgroup launch scans the tile sums, a launch rescans its tile with the offset.
#include <hip/hip_runtime.h>

#include "../../include/pinn_hip.h"
#include "pinn_mlp_core.h"
#include "pinn_rows.h"

namespace pinn {
namespace {

typedef unsigned long long u64;

constexpr int kTile = PINN_AUC_TILE, kMaxK = PINN_AUC_MAX_SCORES, kCnt = PINN_AUC_COUNTS;
constexpr int kCrossBlocks = 256;           // workgroups of the cross sums per pair = partial sums per output
constexpr int kBootThreads = 256, kBootLds = PINN_AUC_BOOT_LDS_GROUPS;

// 48 KiB of histogram + 2 KiB of reduction scratch: three resamples share the 160 KiB of a CU, and the static 64 KiB limit holds
static_assert(kBootLds * 4 + kBootThreads * 8 <= 64 * 1024, "the bootstrap's LDS image must fit a static allocation");

// inclusive scan of kTile entries of two arrays, in place (as pinn_lr.hip's block_scan2)
__device__ __forceinline__ void scan2(long long* sa, long long* sb, int t) {
  for (int off = 1; off < kTile; off <<= 1) {
    const long long va = t >= off ? sa[t - off] : 0, vb = t >= off ? sb[t - off] : 0;
    __syncthreads();
    sa[t] += va; sb[t] += vb;
    __syncthreads();
  }
}

__device__ __forceinline__ bool group_start(const double* s, long long i) { return i == 0 || s[i - 1] != s[i]; }
__device__ __forceinline__ bool group_end(const double* s, long long i, long long n) { return i == n - 1 || s[i] != s[i + 1]; }

// tile sums of the positive flags and of the group starts; blockIdx.y is the classifier
__global__ __launch_bounds__(kTile) void auc_tiles_kernel(const double* __restrict__ score, const long long* __restrict__ pos, long long n,
                                                          long long nt1, long long* __restrict__ tile_pos, long long* __restrict__ tile_start) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x, k = blockIdx.y;
  const long long i = (long long)blockIdx.x * kTile + t;
  const double* s = score + (size_t)k * n;
  sa[t] = i < n ? (pos[(size_t)k * n + i] != 0) : 0;
  sb[t] = i < n ? group_start(s, i) : 0;
  __syncthreads();
  scan2(sa, sb, t);
  if (t == kTile - 1) { tile_pos[k * nt1 + blockIdx.x] = sa[t]; tile_start[k * nt1 + blockIdx.x] = sb[t]; }
}

// exclusive scan of nt tile sums in place (both arrays), totals to two words of the classifier's counts.  One workgroup per
// classifier, none reads what another writes.
__global__ __launch_bounds__(kTile) void auc_scan_tiles_kernel(long long* __restrict__ a_all, long long* __restrict__ b_all, long long nt,
                                                               long long nt1, long long* __restrict__ counts, int word_a, int word_b) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x, k = blockIdx.x;
  long long* a = a_all + k * nt1;
  long long* b = b_all + k * nt1;
  const long long per = (nt + kTile - 1) / kTile, lo = t * per, hi = lo + per < nt ? lo + per : nt;
  long long xa = 0, xb = 0;
  for (long long j = lo; j < hi; ++j) { xa += a[j]; xb += b[j]; }
  sa[t] = xa; sb[t] = xb;
  __syncthreads();
  scan2(sa, sb, t);
  long long ra = sa[t] - xa, rb = sb[t] - xb;
  for (long long j = lo; j < hi; ++j) {
    const long long va = a[j], vb = b[j];
    a[j] = ra; ra += va;
    b[j] = rb; rb += vb;
  }
  if (t == kTile - 1) { counts[k * kCnt + word_a] = sa[t]; counts[k * kCnt + word_b] = sb[t]; }
}

// rescan with the tile offsets: every element's group number, and at the end of group g the positives and the elements up
// to and including it
__global__ __launch_bounds__(kTile) void auc_ends_kernel(const double* __restrict__ score, const long long* __restrict__ pos, long long n,
                                                         long long nt1, const long long* __restrict__ tile_pos,
                                                         const long long* __restrict__ tile_start, int* __restrict__ gid,
                                                         long long* __restrict__ end_pos, long long* __restrict__ end_all) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x, k = blockIdx.y;
  const long long i = (long long)blockIdx.x * kTile + t;
  const double* s = score + (size_t)k * n;
  sa[t] = i < n ? (pos[(size_t)k * n + i] != 0) : 0;
  sb[t] = i < n ? group_start(s, i) : 0;
  __syncthreads();
  scan2(sa, sb, t);
  if (i < n) {
    const long long g = tile_start[k * nt1 + blockIdx.x] + sb[t] - 1;            // 0 <= g <= i: element 0 starts a group
    gid[(size_t)k * n + i] = (int)g;
    if (group_end(s, i, n)) {
      end_pos[(size_t)k * n + g] = tile_pos[k * nt1 + blockIdx.x] + sa[t];
      end_all[(size_t)k * n + g] = i + 1;
    }
  }
}

// a or b of every element from its group's counts, scattered to row order with the group number; tile sums of a and of b
__global__ __launch_bounds__(kTile) void auc_finish_kernel(const long long* __restrict__ pos, const long long* __restrict__ rows, long long n,
                                                           long long nt1, const int* __restrict__ gid, const long long* __restrict__ end_pos,
                                                           const long long* __restrict__ end_all, long long* __restrict__ counts,
                                                           long long* __restrict__ comp, int* __restrict__ group,
                                                           long long* __restrict__ tile_a, long long* __restrict__ tile_b) {
  __shared__ long long sa[kTile], sb[kTile];
  const int t = threadIdx.x, k = blockIdx.y;
  const long long i = (long long)blockIdx.x * kTile + t;
  const size_t base = (size_t)k * n;
  long long va = 0, vb = 0;
  if (i < n) {
    const long long m = counts[k * kCnt + PINN_AUC_POS];
    const int g = gid[base + i];
    const long long p1 = end_pos[base + g], a1 = end_all[base + g];
    const long long p0 = g > 0 ? end_pos[base + g - 1] : 0, a0 = g > 0 ? end_all[base + g - 1] : 0;
    const long long n1 = a1 - p1, n0 = a0 - p0;                  // negatives up to the end of the group, and below it
    const bool is_pos = pos[base + i] != 0;
    if (is_pos) va = 2 * n0 + (n1 - n0);
    else vb = 2 * (m - p1) + (p1 - p0);
    const long long row = rows[base + i];
    if (row >= 0 && row < n) {
      comp[base + row] = is_pos ? va : vb;
      group[base + row] = g;
    }
    if (i == 0) counts[k * kCnt + PINN_AUC_NEG] = n - m;
  }
  sa[t] = va; sb[t] = vb;
  __syncthreads();
  scan2(sa, sb, t);
  if (t == kTile - 1) { tile_a[k * nt1 + blockIdx.x] = sa[t]; tile_b[k * nt1 + blockIdx.x] = sb[t]; }
}

// ---- cross sums.  A 128-bit accumulator is two 64-bit words; an add carries when the low word wraps.
__device__ __forceinline__ void add128(u64& lo, u64& hi, u64 plo, u64 phi) {
  lo += plo;
  hi += phi + (lo < plo ? 1ull : 0ull);
}

__global__ __launch_bounds__(kTile) void cross_partial_kernel(const u64* __restrict__ comp, long long ld, long long rows,
                                                              u64* __restrict__ partial) {
  __shared__ u64 slo[kTile], shi[kTile];
  const int t = threadIdx.x, p = blockIdx.y;
  int k, l;
  untri(p, &k, &l);
  const u64* x = comp + (size_t)k * ld;
  const u64* y = comp + (size_t)l * ld;
  u64 lo = 0, hi = 0;
  for (long long i = (long long)blockIdx.x * kTile + t; i < rows; i += (long long)gridDim.x * kTile)
    add128(lo, hi, x[i] * y[i], __umul64hi(x[i], y[i]));
  slo[t] = lo; shi[t] = hi;
  __syncthreads();
  for (int off = kTile / 2; off > 0; off >>= 1) {
    if (t < off) {
      u64 a = slo[t], b = shi[t];
      add128(a, b, slo[t + off], shi[t + off]);
      slo[t] = a; shi[t] = b;
    }
    __syncthreads();
  }
  if (t == 0) {
    partial[((size_t)p * gridDim.x + blockIdx.x) * 2] = slo[0];
    partial[((size_t)p * gridDim.x + blockIdx.x) * 2 + 1] = shi[0];
  }
}

// one workgroup: thread p adds the partials of pair p in index order
__global__ __launch_bounds__(64) void cross_final_kernel(const u64* __restrict__ partial, int pairs, int nb, u64* __restrict__ out) {
  const int p = threadIdx.x;
  if (p >= pairs) return;
  u64 lo = 0, hi = 0;
  for (int b = 0; b < nb; ++b) add128(lo, hi, partial[((size_t)p * nb + b) * 2], partial[((size_t)p * nb + b) * 2 + 1]);
  out[2 * p] = lo;
  out[2 * p + 1] = hi;
}

// ---- bootstrap.  Draws 2 q and 2 q + 1 of a stratum come from one Philox call at the counter (q, resample, kind, stratum).
__device__ __forceinline__ void boot_draws(unsigned q, unsigned r, unsigned stratum, unsigned seed_lo, unsigned seed_hi, u64 size,
                                           long long* i0, long long* i1) {
  unsigned o[4];
  philox4x32_10(q, r, (unsigned)PINN_AUC_DRAW_BOOT, stratum, seed_lo, seed_hi, o);
  *i0 = (long long)__umul64hi((u64)o[0] | ((u64)o[1] << 32), size);
  *i1 = (long long)__umul64hi((u64)o[2] | ((u64)o[3] << 32), size);
}

struct BootArgs {
  const int* gpos;
  const int* gneg;
  long long m, n, first;
  int K;
  int G[kMaxK];
  unsigned seed_lo, seed_hi;
  long long* u2;
  unsigned* slices;
  long long slice_words;
};

// One classifier of one resample.  c [G] first counts the negative draws per group, then holds the inclusive scan of the
// counts: for a positive draw in group g, 2 below[g] + count[g] = c[g - 1] + c[g].  kGlobal: c is in global memory, where
// the atomics act at the L2 and the plain loads and stores around them go through this CU's L1; a device-scope fence on
// either side of the atomics keeps the three in order.
template <bool kGlobal>
__device__ __forceinline__ u64 boot_one(unsigned* c, int G, const int* __restrict__ gp, const int* __restrict__ gn, long long m,
                                        long long n, unsigned r, unsigned seed_lo, unsigned seed_hi, u64* red) {
  const int t = threadIdx.x;
  for (int g = t; g < G; g += kBootThreads) c[g] = 0;
  if (kGlobal) __threadfence();
  __syncthreads();
  for (long long q = t; 2 * q < n; q += kBootThreads) {
    long long i0, i1;
    boot_draws((unsigned)q, r, 0u, seed_lo, seed_hi, (u64)n, &i0, &i1);
    const int g0 = gn[i0];
    if ((unsigned)g0 < (unsigned)G) atomicAdd(&c[g0], 1u);
    if (2 * q + 1 < n) {
      const int g1 = gn[i1];
      if ((unsigned)g1 < (unsigned)G) atomicAdd(&c[g1], 1u);
    }
  }
  if (kGlobal) __threadfence();
  __syncthreads();
  // inclusive scan in place: every thread owns a run of `per` entries
  const long long per = ((long long)G + kBootThreads - 1) / kBootThreads, lo = t * per, hi = lo + per < G ? lo + per : G;
  u64 x = 0;
  for (long long j = lo; j < hi; ++j) x += c[j];
  red[t] = x;
  __syncthreads();
  for (int off = 1; off < kBootThreads; off <<= 1) {
    const u64 v = t >= off ? red[t - off] : 0;
    __syncthreads();
    red[t] += v;
    __syncthreads();
  }
  u64 run = red[t] - x;
  for (long long j = lo; j < hi; ++j) { run += c[j]; c[j] = (unsigned)run; }
  __syncthreads();
  u64 acc = 0;
  for (long long q = t; 2 * q < m; q += kBootThreads) {
    long long i0, i1;
    boot_draws((unsigned)q, r, 1u, seed_lo, seed_hi, (u64)m, &i0, &i1);
    const int g0 = gp[i0];
    if ((unsigned)g0 < (unsigned)G) acc += (u64)c[g0] + (g0 > 0 ? (u64)c[g0 - 1] : 0ull);
    if (2 * q + 1 < m) {
      const int g1 = gp[i1];
      if ((unsigned)g1 < (unsigned)G) acc += (u64)c[g1] + (g1 > 0 ? (u64)c[g1 - 1] : 0ull);
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int off = kBootThreads / 2; off > 0; off >>= 1) {
    if (t < off) red[t] += red[t + off];
    __syncthreads();
  }
  const u64 total = red[0];
  __syncthreads();                       // red and c are free for the next classifier
  return total;
}

__global__ __launch_bounds__(kBootThreads) void boot_kernel(BootArgs a) {
  __shared__ unsigned hist[kBootLds];
  __shared__ u64 red[kBootThreads];
  const long long b = blockIdx.x;
  const unsigned r = (unsigned)(a.first + b);
  unsigned* slice = a.slices ? a.slices + (size_t)b * a.slice_words : nullptr;
  for (int k = 0; k < a.K; ++k) {
    const int G = a.G[k];
    const int* gp = a.gpos + (size_t)k * a.m;
    const int* gn = a.gneg + (size_t)k * a.n;
    u64 total;
    if (G <= kBootLds) total = boot_one<false>(hist, G, gp, gn, a.m, a.n, r, a.seed_lo, a.seed_hi, red);
    else total = boot_one<true>(slice, G, gp, gn, a.m, a.n, r, a.seed_lo, a.seed_hi, red);
    if (threadIdx.x == 0) a.u2[b * a.K + k] = (long long)total;
  }
}

inline bool auc_shape_ok(long long n, int K) { return n >= 1 && n <= 0x7fffffffLL && K >= 1 && K <= kMaxK; }

inline long long boot_slice_words(int K, const long long* groups) {
  long long g = 0;
  for (int k = 0; k < K; ++k)
    if (groups[k] > kBootLds && groups[k] > g) g = groups[k];
  return (long long)(align256((size_t)g * 4) / 4);
}

}  // namespace
}  // namespace pinn

// workspace: four tile arrays [K][nt + 1], then the group numbers in sorted order [K][n] (32-bit) and the positives and
// elements at every group's end, [K][n] each
extern "C" size_t pinn_auc_components_workspace_bytes(long long n, int n_scores) {
  using namespace pinn;
  if (!auc_shape_ok(n, n_scores)) return 0;
  const size_t nt1 = (size_t)((n + kTile - 1) / kTile) + 1, K = (size_t)n_scores;
  return 4 * align256(K * nt1 * 8) + align256(K * (size_t)n * 4) + 2 * align256(K * (size_t)n * 8);
}

extern "C" int pinn_auc_components(const double* d_score_sorted, const long long* d_pos_sorted, const long long* d_row_sorted,
                                   long long n, int n_scores, long long* d_counts, long long* d_comp, int* d_group, void* d_ws,
                                   size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (!auc_shape_ok(n, n_scores) || !d_score_sorted || !d_pos_sorted || !d_row_sorted || !d_counts || !d_comp || !d_group || !d_ws)
    return PINN_E_ARG;
  if (misaligned8(d_score_sorted) || misaligned8(d_pos_sorted) || misaligned8(d_row_sorted) || misaligned8(d_counts) || misaligned8(d_comp) ||
      ((unsigned long long)d_group & 3) != 0 || misaligned8(d_ws))
    return PINN_E_ARG;
  if (ws_bytes < pinn_auc_components_workspace_bytes(n, n_scores)) return PINN_E_WORKSPACE;
  const long long nt = (n + kTile - 1) / kTile, nt1 = nt + 1;
  const size_t K = (size_t)n_scores, tb = align256(K * (size_t)nt1 * 8);
  char* w = static_cast<char*>(d_ws);
  long long* tile_a = reinterpret_cast<long long*>(w); w += tb;
  long long* tile_b = reinterpret_cast<long long*>(w); w += tb;
  long long* tile_c = reinterpret_cast<long long*>(w); w += tb;
  long long* tile_d = reinterpret_cast<long long*>(w); w += tb;
  int* gid = reinterpret_cast<int*>(w); w += align256(K * (size_t)n * 4);
  long long* end_pos = reinterpret_cast<long long*>(w); w += align256(K * (size_t)n * 8);
  long long* end_all = reinterpret_cast<long long*>(w);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  hipError_t e = hipMemsetAsync(d_counts, 0, K * kCnt * sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)nt, (unsigned)n_scores), block(kTile);
  hipLaunchKernelGGL(auc_tiles_kernel, grid, block, 0, st, d_score_sorted, d_pos_sorted, n, nt1, tile_a, tile_b);
  hipLaunchKernelGGL(auc_scan_tiles_kernel, dim3((unsigned)n_scores), block, 0, st, tile_a, tile_b, nt, nt1, d_counts, PINN_AUC_POS, PINN_AUC_GROUPS);
  hipLaunchKernelGGL(auc_ends_kernel, grid, block, 0, st, d_score_sorted, d_pos_sorted, n, nt1, tile_a, tile_b, gid, end_pos, end_all);
  hipLaunchKernelGGL(auc_finish_kernel, grid, block, 0, st, d_pos_sorted, d_row_sorted, n, nt1, gid, end_pos, end_all, d_counts, d_comp,
                     d_group, tile_c, tile_d);
  hipLaunchKernelGGL(auc_scan_tiles_kernel, dim3((unsigned)n_scores), block, 0, st, tile_c, tile_d, nt, nt1, d_counts, PINN_AUC_U2, PINN_AUC_U2B);
  return launch_status();
}

extern "C" size_t pinn_auc_cross_sums_workspace_bytes(long long rows, int n_scores) {
  using namespace pinn;
  if (rows < 1 || n_scores < 1 || n_scores > kMaxK) return 0;
  const size_t pairs = (size_t)n_scores * (n_scores + 1) / 2;
  return align256(pairs * (size_t)row_blocks(rows, kTile, kCrossBlocks) * 16);
}

extern "C" int pinn_auc_cross_sums(const long long* d_comp, long long ld, long long rows, int n_scores, unsigned long long* d_sums,
                                   void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (rows < 1 || ld < rows || n_scores < 1 || n_scores > kMaxK || !d_comp || !d_sums || !d_ws) return PINN_E_ARG;
  if (misaligned8(d_comp) || misaligned8(d_sums) || misaligned8(d_ws)) return PINN_E_ARG;
  if (ws_bytes < pinn_auc_cross_sums_workspace_bytes(rows, n_scores)) return PINN_E_WORKSPACE;
  const int pairs = n_scores * (n_scores + 1) / 2, nb = row_blocks(rows, kTile, kCrossBlocks);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  hipLaunchKernelGGL(cross_partial_kernel, dim3((unsigned)nb, (unsigned)pairs), dim3(kTile), 0, st, reinterpret_cast<const u64*>(d_comp), ld,
                     rows, static_cast<u64*>(d_ws));
  hipLaunchKernelGGL(cross_final_kernel, dim3(1), dim3(64), 0, st, static_cast<const u64*>(d_ws), pairs, nb, d_sums);
  return launch_status();
}

// a slice of the largest group count beyond the LDS limit per resample; nothing when every histogram fits in LDS
extern "C" size_t pinn_auc_bootstrap_workspace_bytes(long long n_boot, int n_scores, const long long* groups) {
  using namespace pinn;
  if (n_boot < 1 || n_scores < 1 || n_scores > kMaxK || !groups) return 0;
  for (int k = 0; k < n_scores; ++k)
    if (groups[k] < 1 || groups[k] > 0x7fffffffLL) return 0;
  return (size_t)n_boot * (size_t)boot_slice_words(n_scores, groups) * 4;
}

extern "C" int pinn_auc_bootstrap(const int* d_group_pos, const int* d_group_neg, long long m, long long n, int n_scores,
                                  const long long* groups, unsigned long long seed, long long first, long long n_boot,
                                  long long* d_u2, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (m < 1 || n < 1 || m > 0x7fffffffLL || n > 0x7fffffffLL || n_scores < 1 || n_scores > kMaxK || !groups || !d_group_pos ||
      !d_group_neg || !d_u2)
    return PINN_E_ARG;
  if (first < 0 || n_boot < 1 || n_boot > 0x7fffffffLL || first + n_boot > 0x100000000LL) return PINN_E_ARG;
  for (int k = 0; k < n_scores; ++k)
    if (groups[k] < 1 || groups[k] > m + n) return PINN_E_ARG;
  if (((unsigned long long)d_group_pos & 3) != 0 || ((unsigned long long)d_group_neg & 3) != 0 || misaligned8(d_u2) || misaligned8(d_ws))
    return PINN_E_ARG;
  const size_t need = pinn_auc_bootstrap_workspace_bytes(n_boot, n_scores, groups);
  if (need > 0 && !d_ws) return PINN_E_ARG;
  if (ws_bytes < need) return PINN_E_WORKSPACE;
  BootArgs a;
  a.gpos = d_group_pos; a.gneg = d_group_neg; a.m = m; a.n = n; a.first = first; a.K = n_scores;
  for (int k = 0; k < kMaxK; ++k) a.G[k] = k < n_scores ? (int)groups[k] : 0;
  a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
  a.u2 = d_u2;
  a.slice_words = boot_slice_words(n_scores, groups);
  a.slices = need > 0 ? static_cast<unsigned*>(d_ws) : nullptr;
  clear_error();
  hipLaunchKernelGGL(boot_kernel, dim3((unsigned)n_boot), dim3(kBootThreads), 0, (hipStream_t)stream, a);
  return launch_status();
}
