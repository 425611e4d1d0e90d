// Isolation forest on the device: the unsupervised anomaly score of reference script 02 (02:571-596).
//   pinn_if_score   every row descends every tree; depth sum, score and prediction in one launch
//   pinn_if_fit     all trees in one launch, one workgroup (one wave) per tree
// Sums are float64 and every operation is rounded on its own (built with -ffp-contract=off), so that the host backend
// states the same arithmetic.  The leaf values come from the host; nothing here calls log.
//
// Scoring.  A descent is a chain of dependent 8-byte lookups (about 8 per tree, 200 trees), so the time goes to latency,
// not to bytes.  The forest (0.2-1.6 MB) does not fit LDS whole: a workgroup stages consecutive trees, at most
// PINN_IF_LDS_NODES nodes (32 KB) at a time, while every thread keeps the float32 features of its rows in registers and
// adds the leaf values tree by tree: the order of the sum is the tree order whatever the grouping.  512 threads and 36 KB
// leave room for four workgroups on a CU.  Variant 1 reads the nodes from global memory instead (the forest stays in L2).
//
// Fitting.  One wave builds one tree in LDS (the subsample as float32, an index list that is partitioned in place) with an
// explicit stack, so nodes are numbered in pre-order as scikit-learn numbers them, and every draw is keyed by
// (seed, tree, node): nothing depends on the launch geometry.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_mlp_core.h"
#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kIfD = PINN_IF_MAX_FEAT, kIfHdr = PINN_IF_HEADER, kIfCap = PINN_IF_LDS_NODES;
constexpr int kScoreThreads = 512;
constexpr int kFitThreads = 64, kMaxSamples = PINN_IF_MAX_SAMPLES, kStack = 16;
constexpr unsigned kLeafBit = 0x80000000u;
enum { IF_DRAW_SPLIT = 0, IF_DRAW_PERM = 1 };

static_assert(kIfD == kRowsMaxD, "pinn_rows.h carries the same feature limit");
static_assert(kIfCap >= PINN_IF_MAX_NODES + 1, "one tree must fit the staged group");

// 8-byte words from the start of the block
__host__ __device__ inline size_t if_leaf_table() { return kIfHdr; }
__host__ __device__ inline size_t if_tree_off() { return kIfHdr + PINN_IF_MAX_LEAF_VALUES; }
__host__ __device__ inline size_t if_groups() { return if_tree_off() + (PINN_IF_MAX_TREES + 2) / 2; }
__host__ __device__ inline size_t if_nodes() { return if_groups() + (PINN_IF_MAX_TREES + 2) / 2; }

// A row's features as one vector value: elements of an array would be selected by address, which takes the array out of
// the registers; elements of a vector are selected by value.
template <int DP>
struct FeatVec {
  typedef float type __attribute__((ext_vector_type(DP)));
};

// feature f of a row: a tree of selects on the bits of f
template <int DP>
__device__ __forceinline__ float pick_feature(const typename FeatVec<DP>::type x, unsigned f) {
  const bool b0 = f & 1u, b1 = f & 2u, b2 = f & 4u;
  if constexpr (DP == 2) {
    return b0 ? x[1] : x[0];
  } else if constexpr (DP == 4) {
    const float lo = b0 ? x[1] : x[0], hi = b0 ? x[3] : x[2];
    return b1 ? hi : lo;
  } else {
    const float v0 = b0 ? x[1] : x[0], v1 = b0 ? x[3] : x[2], v2 = b0 ? x[5] : x[4], v3 = b0 ? x[7] : x[6];
    const float lo = b1 ? v1 : v0, hi = b1 ? v3 : v2;
    return b2 ? hi : lo;
  }
}

// trees [t0, t1) in tree order: every row's chain walks to its leaf, then the leaf value is added to the row's sum
template <int R, int DP>
__device__ __forceinline__ void descend(const typename FeatVec<DP>::type (&x)[R], double (&sum)[R], const uint2* __restrict__ nd, int t0, int t1,
                                        const int* __restrict__ toff, int shift, const double* __restrict__ leaf, unsigned n_leaf) {
  for (int t = t0; t < t1; ++t) {
    const int o = toff[t - shift], last = toff[t - shift + 1] - o - 1;
    const uint2* tree = nd + o;
    uint2 cur[R];
#pragma unroll
    for (int r = 0; r < R; ++r) cur[r] = tree[0];
    bool any = true;
    for (int step = 0; step <= PINN_IF_MAX_NODES && any; ++step) {     // a well-formed tree ends long before the bound
      any = false;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (!(cur[r].y & kLeafBit)) {
          const float thr = __uint_as_float(cur[r].x);
          const float xv = pick_feature<DP>(x[r], (cur[r].y >> 16) & 7u);
          int child = (int)(cur[r].y & 0xffffu) + (xv <= thr ? 0 : 1);
          child = child < last ? child : last;
          cur[r] = tree[child];
          any = true;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned li = cur[r].x < n_leaf ? cur[r].x : n_leaf - 1u;
      sum[r] = sum[r] + leaf[li];
    }
  }
}

// R rows per thread (independent chains in flight), DP features kept (the forest's, padded), kLds: nodes staged through LDS
template <int R, int DP, bool kLds>
__global__ __launch_bounds__(kScoreThreads) void if_score_kernel(Rows a, const unsigned long long* __restrict__ forest, double offset,
                                                                double* __restrict__ sum_out, double* __restrict__ score_out,
                                                                long long* __restrict__ pred_out) {
  __shared__ uint2 s_nodes[kLds ? kIfCap : 1];
  __shared__ int s_off[kLds ? PINN_IF_MAX_TREES + 1 : 1];
  const long long* hdr = reinterpret_cast<const long long*>(forest);
  const int tid = threadIdx.x;
  const bool good = hdr[PINN_IF_H_MAGIC] == PINN_IF_MAGIC && hdr[PINN_IF_H_FEAT] == a.D && hdr[PINN_IF_H_TREES] >= 1 &&
                    hdr[PINN_IF_H_TREES] <= PINN_IF_MAX_TREES && hdr[PINN_IF_H_LEAF_VALUES] >= 1 &&
                    hdr[PINN_IF_H_LEAF_VALUES] <= PINN_IF_MAX_LEAF_VALUES;
  const int T = good ? (int)hdr[PINN_IF_H_TREES] : 0;
  const int G = good && hdr[PINN_IF_H_GROUPS] >= 1 && hdr[PINN_IF_H_GROUPS] <= T ? (int)hdr[PINN_IF_H_GROUPS] : 0;
  const unsigned n_leaf = good ? (unsigned)hdr[PINN_IF_H_LEAF_VALUES] : 1u;
  const double den = reinterpret_cast<const double*>(forest)[PINN_IF_H_DEN];
  const double* leaf = reinterpret_cast<const double*>(forest) + if_leaf_table();
  const int* off = reinterpret_cast<const int*>(forest + if_tree_off());
  const int* grp = reinterpret_cast<const int*>(forest + if_groups());
  const uint2* nodes = reinterpret_cast<const uint2*>(forest + if_nodes());

  typename FeatVec<DP>::type x[R];
  bool ok[R];
  double sum[R];
  const long long base = (long long)blockIdx.x * (kScoreThreads * R);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long j = base + (long long)r * kScoreThreads + tid;
    double xd[kIfD] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    ok[r] = j < a.n && load_row(a, j, xd);
    sum[r] = 0.0;
#pragma unroll
    for (int i = 0; i < DP; ++i) {
      const float v = (float)xd[i];                              // scikit-learn scores a float32 copy of X
      if (!isfinite(v)) ok[r] = false;
      x[r][i] = ok[r] ? v : 0.0f;
    }
  }

  if constexpr (kLds) {
    for (int g = 0; g < G; ++g) {
      const int t0 = min(max(grp[g], 0), T), t1 = min(max(grp[g + 1], t0), T);
      const int n0 = off[t0], cnt = off[t1] - n0;
      __syncthreads();                                           // the previous group has been read by every thread
      for (int i = tid; i < cnt && i < kIfCap; i += kScoreThreads) s_nodes[i] = nodes[n0 + i];
      for (int i = tid; i <= t1 - t0; i += kScoreThreads) s_off[i] = off[t0 + i] - n0;
      __syncthreads();
      descend<R, DP>(x, sum, s_nodes, t0, t1, s_off, t0, leaf, n_leaf);
    }
  } else {
    descend<R, DP>(x, sum, nodes, 0, T, off, 0, leaf, n_leaf);
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long j = base + (long long)r * kScoreThreads + tid;
    if (j >= a.n) continue;
    const bool valid = ok[r] && good;
    const double s = valid ? sum[r] : quiet_nan();
    const double ratio = den != 0.0 ? s / den : (valid ? 1.0 : quiet_nan());
    const double sc = -exp2(-ratio);
    if (sum_out) sum_out[j] = s;
    if (score_out) score_out[j] = sc;
    if (pred_out) pred_out[j] = (sc - offset >= 0.0) ? 1 : -1;
  }
}

// ---- fitting
__device__ __forceinline__ unsigned mix32(unsigned h) {
  h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
  return h;
}

// position i of a tree's subsample: a Feistel permutation of [0, 4^k) walked until it falls into [0, n)
__device__ __forceinline__ unsigned feistel_walk(unsigned i, unsigned n, int k, const unsigned (&key)[4]) {
  const unsigned mask = (1u << k) - 1u;
  unsigned v = i;
  do {
    unsigned L = v >> k, Rr = v & mask;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned nx = L ^ (mix32(Rr ^ key[r]) & mask);
      L = Rr; Rr = nx;
    }
    v = (L << k) | Rr;
  } while (v >= n);
  return v;
}

__device__ __forceinline__ float wave_min(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kFitThreads) void if_fit_kernel(Rows a, int m, int max_depth, unsigned seed_lo, unsigned seed_hi,
                                                            int* __restrict__ feature, double* __restrict__ threshold,
                                                            int* __restrict__ left, int* __restrict__ right, int* __restrict__ n_node,
                                                            int* __restrict__ node_count, long long* __restrict__ samples,
                                                            int* __restrict__ status) {
  __shared__ float s_x[kMaxSamples * kIfD];
  __shared__ int s_idx[kMaxSamples], s_tmp[kMaxSamples];
  __shared__ int s_stack[kStack][5];                             // start, end, depth, parent, is the right child
  const int tree = blockIdx.x, lane = threadIdx.x, D = a.D, M = 2 * m - 1;
  feature += (size_t)tree * M; threshold += (size_t)tree * M; left += (size_t)tree * M; right += (size_t)tree * M;
  n_node += (size_t)tree * M; samples += (size_t)tree * m;

  unsigned key[4];
  philox4x32_10((unsigned)tree, 0u, (unsigned)IF_DRAW_PERM, 0u, seed_lo, seed_hi, key);
  const unsigned n = (unsigned)a.n;
  int bits = 1;
  while (bits < 32 && ((n - 1u) >> bits) != 0u) ++bits;
  const int k = (bits + 1) / 2;
  int bad = 0;
  for (int i = lane; i < m; i += kFitThreads) {
    const unsigned p = feistel_walk((unsigned)i, n, k, key);
    samples[i] = (long long)p;
    double xd[kIfD];
    const bool ok = load_row(a, (long long)p, xd);
    for (int f = 0; f < D; ++f) {
      float v = (float)xd[f];
      if (!ok || !isfinite(v)) { bad = 1; v = 0.0f; }
      s_x[i * D + f] = v;
    }
    s_idx[i] = i;
  }
  bad = wave_sum(bad);
  if (lane == 0) {
    status[tree] = bad ? 1 : 0;
    s_stack[0][0] = 0; s_stack[0][1] = m; s_stack[0][2] = 0; s_stack[0][3] = -1; s_stack[0][4] = 0;
  }
  __syncthreads();

  int sp = 1, count = 0;
  while (sp > 0 && count < M) {
    --sp;
    const int start = s_stack[sp][0], end = s_stack[sp][1], depth = s_stack[sp][2], parent = s_stack[sp][3], is_right = s_stack[sp][4];
    __syncthreads();                                             // the entry is read before lane 0 overwrites it
    const int id = count++, nn = end - start;
    if (lane == 0) {
      n_node[id] = nn;
      if (parent >= 0) (is_right ? right : left)[parent] = id;
    }
    float lo[kIfD], hi[kIfD];
    int nc = 0;
    if (nn > 1 && depth < max_depth) {
#pragma unroll
      for (int f = 0; f < kIfD; ++f) { lo[f] = INFINITY; hi[f] = -INFINITY; }
      for (int i = start + lane; i < end; i += kFitThreads) {
        const float* row = s_x + s_idx[i] * D;
#pragma unroll
        for (int f = 0; f < kIfD; ++f)
          if (f < D) { lo[f] = fminf(lo[f], row[f]); hi[f] = fmaxf(hi[f], row[f]); }
      }
#pragma unroll
      for (int f = 0; f < kIfD; ++f)
        if (f < D) { lo[f] = wave_min(lo[f]); hi[f] = wave_max(hi[f]); nc += lo[f] < hi[f] ? 1 : 0; }
    }
    if (nc == 0) {                                               // one row, the depth limit, or rows equal in every feature
      if (lane == 0) { feature[id] = -2; threshold[id] = -2.0; left[id] = -1; right[id] = -1; }
      continue;
    }
    unsigned draw[4];
    philox4x32_10((unsigned)tree, (unsigned)id, (unsigned)IF_DRAW_SPLIT, 0u, seed_lo, seed_hi, draw);
    const int want = (int)(((unsigned long long)draw[0] * (unsigned)nc) >> 32);
    int fsel = 0, seen = 0;
    float flo = 0.0f, fhi = 0.0f;
#pragma unroll
    for (int f = 0; f < kIfD; ++f)
      if (f < D && lo[f] < hi[f]) {
        if (seen == want) { fsel = f; flo = lo[f]; fhi = hi[f]; }
        ++seen;
      }
    const double dlo = (double)flo, dhi = (double)fhi;
    const double u = (double)draw[1] * 0x1p-32;
    double t = dlo + u * (dhi - dlo);
    if (t >= dhi) t = dlo;                                       // scikit-learn's random splitter
    int mine = 0;
    for (int i = start + lane; i < end; i += kFitThreads) mine += (double)s_x[s_idx[i] * D + fsel] <= t ? 1 : 0;
    const int NL = wave_sum(mine);
    int cl = 0, cr = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int b = start; b < end; b += kFitThreads) {
      const int i = b + lane;
      const bool valid = i < end;
      const int r = valid ? s_idx[i] : 0;
      const bool goes_left = valid && (double)s_x[r * D + fsel] <= t;
      const unsigned long long mL = __ballot(goes_left), mR = __ballot(valid && !goes_left);
      if (valid) s_tmp[goes_left ? start + cl + __popcll(mL & below) : start + NL + cr + __popcll(mR & below)] = r;
      cl += __popcll(mL); cr += __popcll(mR);
    }
    __syncthreads();
    for (int i = start + lane; i < end; i += kFitThreads) s_idx[i] = s_tmp[i];
    if (lane == 0) {
      feature[id] = fsel; threshold[id] = t;
      if (sp + 2 <= kStack) {
        s_stack[sp][0] = start + NL; s_stack[sp][1] = end; s_stack[sp][2] = depth + 1; s_stack[sp][3] = id; s_stack[sp][4] = 1;
        s_stack[sp + 1][0] = start; s_stack[sp + 1][1] = start + NL; s_stack[sp + 1][2] = depth + 1; s_stack[sp + 1][3] = id; s_stack[sp + 1][4] = 0;
      }
    }
    if (sp + 2 <= kStack) sp += 2;
    __syncthreads();
  }
  if (lane == 0) node_count[tree] = count;
}

template <int R, int DP>
void launch_score(int variant, unsigned blocks, hipStream_t st, const Rows& a, const unsigned long long* forest, double offset, double* sum,
                  double* score, long long* pred) {
  if (variant == 0)
    hipLaunchKernelGGL((if_score_kernel<R, DP, true>), dim3(blocks), dim3(kScoreThreads), 0, st, a, forest, offset, sum, score, pred);
  else
    hipLaunchKernelGGL((if_score_kernel<R, DP, false>), dim3(blocks), dim3(kScoreThreads), 0, st, a, forest, offset, sum, score, pred);
}

template <int R>
void launch_score_d(int variant, unsigned blocks, hipStream_t st, const Rows& a, const unsigned long long* forest, double offset, double* sum,
                    double* score, long long* pred) {
  if (a.D <= 2) launch_score<R, 2>(variant, blocks, st, a, forest, offset, sum, score, pred);
  else if (a.D <= 4) launch_score<R, 4>(variant, blocks, st, a, forest, offset, sum, score, pred);
  else launch_score<R, 8>(variant, blocks, st, a, forest, offset, sum, score, pred);
}

}  // namespace
}  // namespace pinn

extern "C" size_t pinn_if_forest_bytes(int n_trees, int max_nodes_per_tree) {
  if (n_trees < 1 || n_trees > PINN_IF_MAX_TREES || max_nodes_per_tree < 1 || max_nodes_per_tree > PINN_IF_MAX_NODES) return 0;
  return 8 * (pinn::if_nodes() + (size_t)n_trees * (size_t)max_nodes_per_tree);
}

extern "C" int pinn_if_score(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                             const long long* d_row_index, long long n, const void* d_forest, double offset, double* d_depth_sum,
                             double* d_score, long long* d_pred, int variant, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, 1, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!d_forest || misaligned8(d_forest) || misaligned8(d_depth_sum) || misaligned8(d_score) || misaligned8(d_pred)) return PINN_E_ARG;
  if (variant != 0 && variant != 1) return PINN_E_ARG;
  if (n == 0) return PINN_OK;
  // four rows per thread once that still fills the device; one row per thread below (the same sums either way)
  const bool many = n >= 4LL * kScoreThreads * 1024;
  const long long per = (long long)kScoreThreads * (many ? 4 : 1);
  const long long blocks = (n + per - 1) / per;
  if (blocks > 0x7fffffffLL) return PINN_E_ARG;
  clear_error();
  const unsigned long long* f = static_cast<const unsigned long long*>(d_forest);
  if (many) launch_score_d<4>(variant, (unsigned)blocks, (hipStream_t)stream, a, f, offset, d_depth_sum, d_score, d_pred);
  else launch_score_d<1>(variant, (unsigned)blocks, (hipStream_t)stream, a, f, offset, d_depth_sum, d_score, d_pred);
  return launch_status();
}

extern "C" int pinn_if_fit(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                           const long long* d_row_index, long long n, int n_trees, int max_samples, int max_depth,
                           unsigned long long seed, int* d_feature, double* d_threshold, int* d_left, int* d_right, int* d_n_node,
                           int* d_node_count, long long* d_samples, int* d_status, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, 1, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (n_trees < 1 || n_trees > PINN_IF_MAX_TREES || max_samples < 1 || max_samples > PINN_IF_MAX_SAMPLES || max_samples > n ||
      n > 0x7fffffffLL || max_depth < 0 || max_depth > kStack - 2)
    return PINN_E_ARG;
  if (!d_feature || !d_threshold || !d_left || !d_right || !d_n_node || !d_node_count || !d_samples || !d_status) return PINN_E_ARG;
  if (misaligned8(d_threshold) || misaligned8(d_samples) || ((unsigned long long)d_feature & 3) || ((unsigned long long)d_left & 3) ||
      ((unsigned long long)d_right & 3) || ((unsigned long long)d_n_node & 3) || ((unsigned long long)d_node_count & 3) ||
      ((unsigned long long)d_status & 3))
    return PINN_E_ARG;
  clear_error();
  hipLaunchKernelGGL(if_fit_kernel, dim3((unsigned)n_trees), dim3(kFitThreads), 0, (hipStream_t)stream, a, max_samples, max_depth,
                     (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), d_feature, d_threshold, d_left, d_right, d_n_node, d_node_count,
                     d_samples, d_status);
  return launch_status();
}
