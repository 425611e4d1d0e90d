// Spectral clustering on the device, the `Spectral` baseline of the method comparison (reference script 05:455-512):
//   pinn_sp_knn        the k nearest positions of every position by (squared distance, position)
//   pinn_sp_affinity   CSR of A = 0.5 (C + C^T) without its diagonal, degrees and their roots
//   pinn_sp_eigs       the K largest eigenpairs of S = D^{-1/2} A D^{-1/2} by Chebyshev-filtered subspace iteration
//   pinn_sp_embed      scikit-learn's embedding q_j / dd with its sign rule
//   pinn_sp_lloyd      the Lloyd state machine of pinn_lloyd.h on packed rows of up to 32 columns
// All arithmetic is float64, every operation rounded on its own (built with -ffp-contract=off).
//
// The eigen stage works on a block of m = min(n, K + 16) columns.  One outer iteration is a queue of launches: S Q (a
// thread per element, the row's entries in CSR order), H = Q^T S Q (tiles of 32 rows through LDS, per-workgroup partial
// sums, added in index order by the next launch), a one-workgroup Jacobi diagonalisation of H in LDS (round-robin pairs:
// m / 2 rotations at a time), a row pass that rotates Q and S Q and sums the squared residuals, a one-workgroup decision
// (converged, or the filter's interval and degree), the Chebyshev steps (one launch each; those beyond the degree return
// at once) and two orthonormalisations by the Gram matrix, which reuse the Gram, Jacobi and row-pass kernels.
//
// No float atomics, no workgroup waits on another: stream order is the only dependency, and the same call gives the same
// bytes every time.  Integer atomics count the transposed neighbour lists and hand out their slots; every row is then
// placed by rank.  Once a state's converged flag or status word is set every later launch returns at once.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/pinn_hip.h"
#include "pinn_lloyd.h"
#include "pinn_rows.h"

namespace pinn {
namespace {

constexpr int kT = 128;                      // positions per workgroup of the neighbour search = candidates per LDS tile
constexpr int kMaxD = PINN_SP_MAX_FEAT, kMaxNb = PINN_SP_MAX_NEIGHBORS, kMaxK = PINN_SP_MAX_COMPONENTS;
constexpr int kMaxM = kMaxK + PINN_SP_GUARD; // columns of the block: 48
constexpr int kHdr = PINN_CL_ST_HEADER;
constexpr int kRowT = 64;                    // threads of a workgroup that owns one row of the affinity
constexpr int kBT = 256;                     // threads of the block kernels
constexpr int kGR = 32;                      // rows per tile of the Gram and rotation passes
constexpr int kGBlocks = 128;                // workgroups of those passes = partial sums per output
constexpr int kGOut = (kMaxM * kMaxM + kBT - 1) / kBT;       // outputs per thread of the Gram pass: 9
constexpr int kROut = (kGR * kMaxM + kBT - 1) / kBT;         // elements per thread of a rotation tile: 6
constexpr int kSweeps = 30;
constexpr int kLMaxD = PINN_SP_MAX_DIM, kLMaxK = PINN_SP_MAX_CLUSTERS;
constexpr int kLBlocks = 256;                // workgroups of a Lloyd row pass = partial sums per output

static_assert(kMaxD == kRowsMaxD, "pinn_rows.h carries the same limit");

enum { GRAM_H = 0, GRAM_SRC = 1, GRAM_A = 2 };
enum { JAC_RITZ = 0, JAC_ORTHO = 1 };
enum { ROT_RITZ = 0, ROT_SRC = 1, ROT_A = 2 };

__host__ __device__ inline int block_cols(long long n, int K) { return (int)(n < (long long)(K + PINN_SP_GUARD) ? n : (long long)(K + PINN_SP_GUARD)); }

// eigen state: header, theta [m], residuals [m], vectors [n][m]
__host__ __device__ inline size_t eg_theta() { return kHdr; }
__host__ __device__ inline size_t eg_res(int m) { return kHdr + (size_t)m; }
__host__ __device__ inline size_t eg_q(int m) { return kHdr + 2 * (size_t)m; }
__host__ __device__ inline size_t eg_words(long long n, int m) { return eg_q(m) + (size_t)n * m; }

// ---------------------------------------------------------------------------------------------- neighbour search
// One thread per position keeps its k best candidates, sorted, in LDS (slot-major: no bank conflicts).  Candidates come in
// ascending position, so "strictly smaller distance moves ahead" orders equal distances by position.
__global__ __launch_bounds__(kT) void sp_knn_kernel(Rows a, int k, int include_self, long long* __restrict__ idx_out,
                                                    double* __restrict__ d2_out, long long* __restrict__ status) {
  __shared__ double s_y[kT * (kMaxD + 1)];
  __shared__ int s_ok[kT];
  __shared__ double s_d[kMaxNb * kT];
  __shared__ int s_j[kMaxNb * kT];
  const int t = threadIdx.x, D = a.D, Dp = D | 1;
  const long long i = (long long)blockIdx.x * kT + t;
  double x[kMaxD];
  bool ok = false;
  if (i < a.n) ok = load_row(a, i, x);
  int cnt = 0;
  for (long long base = 0; base < a.n; base += kT) {
    const long long j = base + t;
    double y[kMaxD];
    bool yok = false;
    if (j < a.n) yok = load_row(a, j, y);
#pragma unroll
    for (int c = 0; c < kMaxD; ++c)
      if (c < D) s_y[t * Dp + c] = yok ? y[c] : 0.0;
    s_ok[t] = yok ? 1 : 0;
    __syncthreads();
    if (ok) {
      const int lim = (int)(a.n - base < (long long)kT ? a.n - base : (long long)kT);
      for (int r = 0; r < lim; ++r) {
        if (!s_ok[r]) continue;
        const long long jj = base + r;
        if (!include_self && jj == i) continue;
        double d2 = 0.0;
#pragma unroll
        for (int c = 0; c < kMaxD; ++c)
          if (c < D) { const double d = x[c] - s_y[r * Dp + c]; d2 += d * d; }
        int pos;
        if (cnt < k) pos = cnt++;
        else if (d2 < s_d[(k - 1) * kT + t]) pos = k - 1;
        else continue;
        while (pos > 0 && s_d[(pos - 1) * kT + t] > d2) {
          s_d[pos * kT + t] = s_d[(pos - 1) * kT + t];
          s_j[pos * kT + t] = s_j[(pos - 1) * kT + t];
          --pos;
        }
        s_d[pos * kT + t] = d2;
        s_j[pos * kT + t] = (int)jj;
      }
    }
    __syncthreads();
  }
  if (i >= a.n) return;
  for (int q = 0; q < k; ++q) {
    idx_out[i * k + q] = q < cnt ? (long long)s_j[q * kT + t] : -1LL;
    d2_out[i * k + q] = q < cnt ? s_d[q * kT + t] : quiet_nan();
  }
  if (!ok) status[0] = PINN_SP_BAD_ROW;                    // every writer stores the same word
}

// ---------------------------------------------------------------------------------------------- affinity
__device__ __forceinline__ bool edge_ok(long long j, long long i, long long n) { return j >= 0 && j < n && j != i; }

// in-degree of every position (integer atomics: the result does not depend on the order)
__global__ __launch_bounds__(kBT) void aff_count_kernel(long long n, int k, const long long* __restrict__ knn, unsigned long long* __restrict__ incnt) {
  const long long e = (long long)blockIdx.x * kBT + threadIdx.x;
  if (e >= n * k) return;
  const long long i = e / k, j = knn[e];
  if (edge_ok(j, i, n)) atomicAdd(&incnt[j], 1ULL);
}

// out[0] = 0, out[i + 1] = in[0] + .. + in[i].  One workgroup.
__global__ __launch_bounds__(kBT) void aff_scan_kernel(long long n, const unsigned long long* __restrict__ in, long long* __restrict__ out) {
  __shared__ long long s_sum[kBT];
  const int t = threadIdx.x;
  const long long chunk = (n + kBT - 1) / kBT, lo = chunk * t, hi = lo + chunk < n ? lo + chunk : n;
  long long s = 0;
  for (long long i = lo; i < hi; ++i) s += (long long)in[i];
  s_sum[t] = s;
  __syncthreads();
  long long off = 0;
  for (int u = 0; u < t; ++u) off += s_sum[u];
  if (t == 0) out[0] = 0;
  for (long long i = lo; i < hi; ++i) { off += (long long)in[i]; out[i + 1] = off; }
}

// the transposed lists: position i goes into a slot of every j it names.  The slot order depends on the schedule; the
// write kernel places by rank, so nothing that leaves the workspace does.
__global__ __launch_bounds__(kBT) void aff_fill_kernel(long long n, int k, const long long* __restrict__ knn, const long long* __restrict__ toff,
                                                       unsigned long long* __restrict__ cursor, long long* __restrict__ tin) {
  const long long e = (long long)blockIdx.x * kBT + threadIdx.x;
  if (e >= n * k) return;
  const long long i = e / k, j = knn[e];
  if (!edge_ok(j, i, n)) return;
  const unsigned long long slot = atomicAdd(&cursor[j], 1ULL);
  tin[toff[j] + (long long)slot] = i;
}

// One workgroup per row i.  Entries of the transposed list that the row's own list holds too are marked (-1): the own
// entry then carries 1.0.  len[i] = own entries + unmarked transposed entries.
__global__ __launch_bounds__(kRowT) void aff_len_kernel(long long n, int k, const long long* __restrict__ knn, const long long* __restrict__ toff,
                                                        long long* __restrict__ tin, unsigned long long* __restrict__ len) {
  __shared__ long long s_own[kMaxNb];
  __shared__ int s_cnt;
  const long long i = blockIdx.x;
  const int t = threadIdx.x;
  if (t == 0) s_cnt = 0;
  if (t < k) { const long long j = knn[i * k + t]; s_own[t] = edge_ok(j, i, n) ? j : -1; }
  __syncthreads();
  int mine = 0;
  if (t < k && s_own[t] >= 0) {                            // a list names a position once; a repeated name counts once
    mine = 1;
    for (int u = 0; u < t; ++u) if (s_own[u] == s_own[t]) mine = 0;
  }
  const long long lo = toff[i], hi = toff[i + 1];
  for (long long p = lo + t; p < hi; p += kRowT) {
    const long long v = tin[p];
    bool dup = false;
    for (int u = 0; u < k; ++u) dup = dup || s_own[u] == v;
    if (dup) tin[p] = -1; else ++mine;
  }
  if (mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (t == 0) len[i] = (unsigned long long)s_cnt;
}

// One workgroup per row: every kept entry goes to indptr[i] + (the number of kept entries with a smaller column).
__global__ __launch_bounds__(kRowT) void aff_write_kernel(long long n, int k, const long long* __restrict__ knn, const long long* __restrict__ toff,
                                                          const long long* __restrict__ tin, const long long* __restrict__ indptr,
                                                          long long* __restrict__ indices, double* __restrict__ data, double* __restrict__ degree,
                                                          double* __restrict__ dd) {
  __shared__ long long s_own[kMaxNb];
  __shared__ int s_mutual;
  const long long i = blockIdx.x;
  const int t = threadIdx.x;
  if (t == 0) s_mutual = 0;
  if (t < k) {
    long long j = knn[i * k + t];
    if (!edge_ok(j, i, n)) j = -1;
    s_own[t] = j;
  }
  __syncthreads();
  bool again = false;                                       // a repeated name counts once, as in aff_len_kernel
  if (t < k && s_own[t] >= 0)
    for (int u = 0; u < t; ++u) again = again || s_own[u] == s_own[t];
  __syncthreads();
  if (again) s_own[t] = -1;
  __syncthreads();
  const long long lo = toff[i], hi = toff[i + 1], base = indptr[i];
  const long long total = (long long)k + (hi - lo);
  for (long long e = t; e < total; e += kRowT) {
    const bool own = e < k;
    const long long v = own ? s_own[e] : tin[lo + (e - k)];
    if (v < 0) continue;
    long long rank = 0;
    for (int u = 0; u < k; ++u) rank += (s_own[u] >= 0 && s_own[u] < v) ? 1 : 0;
    for (long long p = lo; p < hi; ++p) { const long long w = tin[p]; rank += (w >= 0 && w < v) ? 1 : 0; }
    double wgt = 0.5;
    if (own) {                                              // mutual when v names i as well
      for (int u = 0; u < k; ++u) if (knn[v * k + u] == i) { wgt = 1.0; break; }
      if (wgt == 1.0) atomicAdd(&s_mutual, 1);
    }
    indices[base + rank] = v;
    data[base + rank] = wgt;
  }
  __syncthreads();
  if (t == 0) {                                             // multiples of 0.5: exact in any order
    const long long cnt = indptr[i + 1] - base;
    const double d = 0.5 * (double)(cnt - s_mutual) + 1.0 * (double)s_mutual;
    degree[i] = d;
    dd[i] = sqrt(d);
  }
}

// ---------------------------------------------------------------------------------------------- eigen stage
struct Csr {
  const long long *indptr, *indices;
  const double* data;
  long long n, nnz;
};

// rdd[i] = 1 / dd[i]; 0 marks a row without an edge (S_ii = 1 there)
__global__ __launch_bounds__(kBT) void eg_rdd_kernel(long long n, const double* __restrict__ dd, double* __restrict__ rdd) {
  const long long i = (long long)blockIdx.x * kBT + threadIdx.x;
  if (i < n) rdd[i] = dd[i] > 0.0 ? 1.0 / dd[i] : 0.0;
}

__global__ void eg_header_kernel(double* __restrict__ st, long long n, int m, int K, double tol) {
  long long* hdr = reinterpret_cast<long long*>(st);
  for (int w = 0; w < kHdr; ++w) hdr[w] = 0;
  hdr[PINN_SP_ST_N] = n; hdr[PINN_SP_ST_M] = m; hdr[PINN_SP_ST_K] = K;
  st[PINN_SP_ST_MAXRES] = INFINITY; st[PINN_SP_ST_TOL] = tol;
}

__device__ __forceinline__ double s_row_dot(const Csr& g, const double* __restrict__ rdd, const double* __restrict__ src, long long row, int m, int col) {
  const double ri = rdd[row];
  if (!(ri > 0.0)) return src[row * m + col];
  long long p = g.indptr[row], pe = g.indptr[row + 1];
  if (p < 0) p = 0;
  if (pe > g.nnz) pe = g.nnz;
  double s = 0.0;
  for (; p < pe; ++p) {
    const long long j = g.indices[p];
    if (j < 0 || j >= g.n) continue;
    s += g.data[p] * (src[j * m + col] * rdd[j]);
  }
  return s * ri;
}

// step < 0: dst = S src.  step >= 0: Chebyshev step `step` between the buffers A (even steps read it) and B; the new block
// overwrites the one before last, of which every thread needs its own element only.
__global__ __launch_bounds__(kBT) void eg_spmm_kernel(const double* __restrict__ st, int step, Csr g, int m, const double* __restrict__ rdd,
                                                      double* __restrict__ A, double* __restrict__ B) {
  if (stopped(st)) return;
  const long long e = (long long)blockIdx.x * kBT + threadIdx.x;
  if (step < 0) {
    if (e >= g.n * m) return;
    B[e] = s_row_dot(g, rdd, A, e / m, m, (int)(e % m));
    return;
  }
  if (step >= reinterpret_cast<const long long*>(st)[PINN_SP_ST_DEGREE]) return;
  if (e >= g.n * m) return;
  const double* src = (step & 1) ? B : A;
  double* dst = (step & 1) ? A : B;
  const double c = st[PINN_SP_ST_FILT_C], w = st[PINN_SP_ST_FILT_E];
  const double s = s_row_dot(g, rdd, src, e / m, m, (int)(e % m));
  const double y = (s - c * src[e]) / w;
  dst[e] = step == 0 ? y : 2.0 * y - dst[e];
}

// where the filter left its result: A after an even number of steps (0 at the start), else B
__device__ __forceinline__ const double* filtered(const double* st, const double* A, const double* B) {
  return (reinterpret_cast<const long long*>(st)[PINN_SP_ST_DEGREE] & 1) ? B : A;
}

// part[block][m * m]: X^T Y over the block's tiles, rows in order.  GRAM_H: X = A (the vectors), Y = B (S times them);
// GRAM_SRC: X = Y = the filter's result; GRAM_A: X = Y = A.
__global__ __launch_bounds__(kBT) void eg_gram_kernel(const double* __restrict__ st, int mode, long long n, int m, const double* __restrict__ A,
                                                      const double* __restrict__ B, double* __restrict__ part) {
  __shared__ double s_x[kGR * kMaxM], s_y[kGR * kMaxM];
  if (stopped(st)) return;
  const int t = threadIdx.x, mm = m * m;
  const double* X = mode == GRAM_SRC ? filtered(st, A, B) : A;
  const double* Y = mode == GRAM_H ? B : X;
  double acc[kGOut];
  int oa[kGOut], ob[kGOut];
#pragma unroll
  for (int q = 0; q < kGOut; ++q) {
    const int o = t + q * kBT;
    acc[q] = 0.0;
    oa[q] = o < mm ? o / m : -1;
    ob[q] = o < mm ? o % m : 0;
  }
  const long long tiles = (n + kGR - 1) / kGR;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long r0 = tile * kGR;
    const int rows = (int)(n - r0 < (long long)kGR ? n - r0 : (long long)kGR);
    for (int e = t; e < rows * m; e += kBT) {
      s_x[e] = X[r0 * m + e];
      s_y[e] = Y[r0 * m + e];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kGOut; ++q) {
      if (oa[q] < 0) continue;
      double s = acc[q];
      for (int r = 0; r < rows; ++r) s += s_x[r * m + oa[q]] * s_y[r * m + ob[q]];
      acc[q] = s;
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < kGOut; ++q)
    if (oa[q] >= 0) part[(size_t)blockIdx.x * mm + t + q * kBT] = acc[q];
}

// One workgroup: the partial sums in index order, the matrix made symmetric, cyclic Jacobi with round-robin pairs
// (M / 2 disjoint rotations at a time, M - 1 rounds a sweep), eigenvalues descending (equal ones by index).
// JAC_RITZ: T = the eigenvectors, theta into the state.  JAC_ORTHO: the matrix is first scaled to unit diagonal and
// T = diag^{-1/2} U Lambda^{-1/2} with Lambda floored at 1e-15 of its largest.
__global__ __launch_bounds__(kBT) void eg_jacobi_kernel(double* __restrict__ st, int mode, int m, int n_part, const double* __restrict__ part,
                                                        double* __restrict__ T) {
  __shared__ double s_a[kMaxM * kMaxM], s_v[kMaxM * kMaxM];
  __shared__ double s_c[kMaxM / 2], s_s[kMaxM / 2], s_scale[kMaxM], s_off[kMaxM], s_dia[kMaxM];
  __shared__ int s_p[kMaxM / 2], s_q[kMaxM / 2], s_perm[kMaxM];
  if (stopped(st)) return;
  const int t = threadIdx.x, mm = m * m;
  for (int o = t; o < mm; o += kBT) {
    double s = 0.0;
    for (int g = 0; g < n_part; ++g) s += part[(size_t)g * mm + o];
    s_v[o] = s;
  }
  __syncthreads();
  if (t < m) s_scale[t] = mode == JAC_ORTHO ? (s_v[t * m + t] > 0.0 ? 1.0 / sqrt(s_v[t * m + t]) : 0.0) : 1.0;
  __syncthreads();
  for (int o = t; o < mm; o += kBT) {
    const int a = o / m, b = o % m;
    s_a[o] = 0.5 * (s_v[a * m + b] + s_v[b * m + a]) * (s_scale[a] * s_scale[b]);
  }
  __syncthreads();
  for (int o = t; o < mm; o += kBT) s_v[o] = (o / m == o % m) ? 1.0 : 0.0;
  __syncthreads();

  const int M = m + (m & 1), half = M / 2;
  for (int sweep = 0; sweep < kSweeps && m > 1; ++sweep) {
    for (int s = 0; s < M - 1; ++s) {
      if (t < half) {
        int p = t == 0 ? M - 1 : (s + t) % (M - 1);
        int q = t == 0 ? s : (s - t + M - 1) % (M - 1);
        if (p > q) { const int u = p; p = q; q = u; }
        double c = 1.0, sn = 0.0;
        bool on = q < m;
        if (on) {
          const double apq = s_a[p * m + q];
          if (apq != 0.0 && apq == apq) {
            const double tau = (s_a[q * m + q] - s_a[p * m + p]) / (2.0 * apq);
            const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tt * tt);
            sn = tt * c;
          } else {
            on = false;
          }
        }
        s_p[t] = on ? p : -1; s_q[t] = q; s_c[t] = c; s_s[t] = sn;
      }
      __syncthreads();
      for (int e = t; e < half * m; e += kBT) {              // columns p and q of the matrix and of the vectors
        const int kp = e / m, r = e % m, p = s_p[kp], q = s_q[kp];
        if (p < 0) continue;
        const double c = s_c[kp], sn = s_s[kp];
        const double ap = s_a[r * m + p], aq = s_a[r * m + q];
        s_a[r * m + p] = c * ap - sn * aq;
        s_a[r * m + q] = sn * ap + c * aq;
        const double vp = s_v[r * m + p], vq = s_v[r * m + q];
        s_v[r * m + p] = c * vp - sn * vq;
        s_v[r * m + q] = sn * vp + c * vq;
      }
      __syncthreads();
      for (int e = t; e < half * m; e += kBT) {              // rows p and q of the matrix
        const int kp = e / m, r = e % m, p = s_p[kp], q = s_q[kp];
        if (p < 0) continue;
        const double c = s_c[kp], sn = s_s[kp];
        const double ap = s_a[p * m + r], aq = s_a[q * m + r];
        s_a[p * m + r] = c * ap - sn * aq;
        s_a[q * m + r] = sn * ap + c * aq;
      }
      __syncthreads();
      if (t < half && s_p[t] >= 0) { s_a[s_p[t] * m + s_q[t]] = 0.0; s_a[s_q[t] * m + s_p[t]] = 0.0; }
      __syncthreads();
    }
    if (t < m) {
      double off = 0.0;
      for (int r = 0; r < m; ++r) if (r != t) off += s_a[r * m + t] * s_a[r * m + t];
      s_off[t] = off;
      s_dia[t] = s_a[t * m + t] * s_a[t * m + t];
    }
    __syncthreads();
    double off = 0.0, dia = 0.0;
    for (int r = 0; r < m; ++r) { off += s_off[r]; dia += s_dia[r]; }
    __syncthreads();
    if (!(off > 1e-30 * dia)) break;                       // the same sums in every thread: the branch is uniform
  }
  if (t == 0) {                                             // descending, equal values by index
    for (int r = 0; r < m; ++r) s_perm[r] = r;
    for (int r = 1; r < m; ++r) {
      const int id = s_perm[r];
      const double v = s_a[id * m + id];
      int u = r;
      while (u > 0 && s_a[s_perm[u - 1] * m + s_perm[u - 1]] < v) { s_perm[u] = s_perm[u - 1]; --u; }
      s_perm[u] = id;
    }
  }
  __syncthreads();
  const int top = s_perm[0];
  const double floor_ = 1e-15 * s_a[top * m + top];
  for (int o = t; o < mm; o += kBT) {
    const int a = o / m, c = o % m, id = s_perm[c];
    double v = s_v[a * m + id];
    if (mode == JAC_ORTHO) {
      const double lam = s_a[id * m + id];
      v = s_scale[a] * v / sqrt(lam > floor_ ? lam : floor_);
    }
    T[o] = v;
  }
  if (mode == JAC_RITZ && t < m) st[eg_theta() + t] = s_a[s_perm[t] * m + s_perm[t]];
}

// dst rows = src rows times T [m][m], tile by tile through LDS (in place: a tile is read whole before it is written).
// ROT_RITZ: A and B (= S A) are both rotated and part_res[block][m] gets the column sums of (B - theta A)^2;
// ROT_SRC: A = (the filter's result) T; ROT_A: A = A T.
__global__ __launch_bounds__(kBT) void eg_rotate_kernel(const double* __restrict__ st, int mode, long long n, int m, const double* __restrict__ T,
                                                        double* __restrict__ A, double* __restrict__ B, double* __restrict__ part_res) {
  __shared__ double s_t[kMaxM * kMaxM], s_x[kGR * kMaxM], s_y[kGR * kMaxM];
  if (stopped(st)) return;
  const int t = threadIdx.x, mm = m * m;
  for (int o = t; o < mm; o += kBT) s_t[o] = T[o];
  const double* src = mode == ROT_SRC ? filtered(st, A, B) : A;
  const double theta = (mode == ROT_RITZ && t < m) ? st[eg_theta() + t] : 0.0;
  double res = 0.0;
  const long long tiles = (n + kGR - 1) / kGR;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long r0 = tile * kGR;
    const int rows = (int)(n - r0 < (long long)kGR ? n - r0 : (long long)kGR);
    __syncthreads();
    for (int e = t; e < rows * m; e += kBT) {
      s_x[e] = src[r0 * m + e];
      if (mode == ROT_RITZ) s_y[e] = B[r0 * m + e];
    }
    __syncthreads();
    double nx[kROut], ny[kROut];
#pragma unroll
    for (int q = 0; q < kROut; ++q) {
      const int e = t + q * kBT;
      nx[q] = 0.0; ny[q] = 0.0;
      if (e < rows * m) {
        const int r = e / m, c = e % m;
        double sx = 0.0, sy = 0.0;
        for (int u = 0; u < m; ++u) sx += s_x[r * m + u] * s_t[u * m + c];
        if (mode == ROT_RITZ)
          for (int u = 0; u < m; ++u) sy += s_y[r * m + u] * s_t[u * m + c];
        nx[q] = sx; ny[q] = sy;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kROut; ++q) {
      const int e = t + q * kBT;
      if (e < rows * m) {
        A[r0 * m + e] = nx[q];
        if (mode == ROT_RITZ) { B[r0 * m + e] = ny[q]; s_x[e] = nx[q]; s_y[e] = ny[q]; }
      }
    }
    if (mode == ROT_RITZ) {
      __syncthreads();
      if (t < m)
        for (int r = 0; r < rows; ++r) { const double d = s_y[r * m + t] - theta * s_x[r * m + t]; res += d * d; }
    }
  }
  if (mode == ROT_RITZ && t < m) part_res[(size_t)blockIdx.x * m + t] = res;
}

// One workgroup: residual norms into the state, then converged, or the filter of the next launches.
__global__ __launch_bounds__(64) void eg_decide_kernel(double* __restrict__ st, int m, int K, int n_part, const double* __restrict__ part_res) {
  __shared__ double s_r[kMaxM];
  if (stopped(st)) return;
  const int t = threadIdx.x;
  if (t < m) {
    double s = 0.0;
    for (int g = 0; g < n_part; ++g) s += part_res[(size_t)g * m + t];
    s_r[t] = sqrt(s);
    st[eg_res(m) + t] = s_r[t];
  }
  __syncthreads();
  if (t != 0) return;
  long long* hdr = reinterpret_cast<long long*>(st);
  double worst = 0.0;
  bool bad = false;
  for (int c = 0; c < m; ++c) {
    const double th = st[eg_theta() + c];
    bad = bad || !(s_r[c] - s_r[c] == 0.0) || !(th - th == 0.0);
    if (c < K && s_r[c] > worst) worst = s_r[c];
  }
  hdr[PINN_CL_ST_ITER] += 1;
  hdr[PINN_SP_ST_MATVEC] += 1;
  st[PINN_SP_ST_MAXRES] = worst;
  if (bad) { hdr[PINN_CL_ST_STATUS] = PINN_SP_NAN; return; }
  if (worst <= st[PINN_SP_ST_TOL]) { hdr[PINN_CL_ST_CONVERGED] = 1; return; }
  double a = st[eg_theta() + m - 1];
  if (a < -0.99) a = -0.99;
  const double c = (a - 1.0) / 2.0, e = (a + 1.0) / 2.0, r = (1.0 - c) / e;
  int deg = PINN_SP_MAX_DEGREE;
  while (deg > 1 && !(cosh((double)deg * acosh(r)) <= 1e8)) --deg;
  st[PINN_SP_ST_FILT_C] = c;
  st[PINN_SP_ST_FILT_E] = e;
  hdr[PINN_SP_ST_DEGREE] = deg;
  hdr[PINN_SP_ST_MATVEC] += deg;
}

// ---------------------------------------------------------------------------------------------- embedding
__device__ __forceinline__ double embed_value(const double* __restrict__ q, const double* __restrict__ dd, long long i, int m, int j) {
  const double d = dd[i];
  return d > 0.0 ? q[i * m + j] / d : q[i * m + j];
}

// one workgroup per column: the sign of the entry of largest magnitude, the first of equals
__global__ __launch_bounds__(kBT) void embed_sign_kernel(long long n, int m, const double* __restrict__ q, const double* __restrict__ dd,
                                                         double* __restrict__ sign) {
  __shared__ double s_m[kBT], s_v[kBT];
  __shared__ long long s_i[kBT];
  const int t = threadIdx.x, j = blockIdx.x;
  double bm = -1.0, bv = 0.0;
  long long bi = n;
  for (long long i = t; i < n; i += kBT) {
    const double v = embed_value(q, dd, i, m, j), mag = fabs(v);
    if (mag > bm) { bm = mag; bv = v; bi = i; }             // i ascends: the first of equals stays
  }
  s_m[t] = bm; s_v[t] = bv; s_i[t] = bi;
  __syncthreads();
  for (int w = kBT / 2; w > 0; w >>= 1) {
    if (t < w && (s_m[t + w] > s_m[t] || (s_m[t + w] == s_m[t] && s_i[t + w] < s_i[t]))) {
      s_m[t] = s_m[t + w]; s_v[t] = s_v[t + w]; s_i[t] = s_i[t + w];
    }
    __syncthreads();
  }
  if (t == 0) sign[j] = s_v[0] < 0.0 ? -1.0 : 1.0;
}

__global__ __launch_bounds__(kBT) void embed_write_kernel(long long n, int m, int K, const double* __restrict__ q, const double* __restrict__ dd,
                                                          const double* __restrict__ sign, double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * kBT + threadIdx.x;
  if (e >= n * K) return;
  const long long i = e / K;
  const int j = (int)(e % K);
  out[e] = sign[j] * embed_value(q, dd, i, m, j);
}

// ---------------------------------------------------------------------------------------------- host side
inline bool rows_ok(long long n) { return n >= 1 && n <= (long long)PINN_SP_MAX_ROWS; }
inline bool eig_ok(long long n, int K) { return rows_ok(n) && K >= 1 && K <= kMaxK && (long long)K <= n; }
inline bool lloyd_ok(long long n, int K, int D) { return rows_ok(n) && K >= 1 && K <= kLMaxK && D >= 1 && D <= kLMaxD; }
inline unsigned blocks_of(long long items, int per) { return (unsigned)((items + per - 1) / per); }

struct AffWs {
  unsigned long long *incnt, *cursor, *len;
  long long *toff, *tin;
};

inline size_t aff_n_bytes(long long n) { return align256((size_t)(n + 1) * 8); }

inline AffWs aff_carve(void* d_ws, long long n) {
  char* w = static_cast<char*>(d_ws);
  AffWs s;
  s.incnt = reinterpret_cast<unsigned long long*>(w); w += aff_n_bytes(n);
  s.cursor = reinterpret_cast<unsigned long long*>(w); w += aff_n_bytes(n);
  s.len = reinterpret_cast<unsigned long long*>(w); w += aff_n_bytes(n);
  s.toff = reinterpret_cast<long long*>(w); w += aff_n_bytes(n);
  s.tin = reinterpret_cast<long long*>(w);
  return s;
}

struct EigWs {
  double *rdd, *B, *W, *T, *part, *part_res, *sign;
};

inline EigWs eig_carve(void* d_ws, long long n, int m) {
  char* w = static_cast<char*>(d_ws);
  EigWs s;
  s.rdd = reinterpret_cast<double*>(w); w += align256((size_t)n * 8);
  s.B = reinterpret_cast<double*>(w); w += align256((size_t)n * m * 8);
  s.W = reinterpret_cast<double*>(w); w += align256((size_t)n * m * 8);
  s.T = reinterpret_cast<double*>(w); w += align256((size_t)m * m * 8);
  s.part = reinterpret_cast<double*>(w); w += align256((size_t)kGBlocks * m * m * 8);
  s.part_res = reinterpret_cast<double*>(w); w += align256((size_t)kGBlocks * m * 8);
  s.sign = reinterpret_cast<double*>(w);
  return s;
}

}  // namespace
}  // namespace pinn

extern "C" int pinn_sp_knn(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                           const long long* d_row_index, long long n, int n_neighbors, int include_self, long long* d_indices,
                           double* d_dist2, long long* d_status, void* stream) {
  using namespace pinn;
  Rows a;
  const int rc = make_rows(d_arr, ld, n_arr_rows, cols, n_feat, 1, d_row_index, n, &a);
  if (rc != PINN_OK) return rc;
  if (!rows_ok(n) || n_neighbors < 1 || n_neighbors > kMaxNb) return PINN_E_ARG;
  if (!d_indices || !d_dist2 || !d_status || misaligned8(d_indices) || misaligned8(d_dist2) || misaligned8(d_status)) return PINN_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const hipError_t e = hipMemsetAsync(d_status, 0, sizeof(long long), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sp_knn_kernel, dim3(blocks_of(n, kT)), dim3(kT), 0, st, a, n_neighbors, include_self, d_indices, d_dist2, d_status);
  return launch_status();
}

extern "C" size_t pinn_sp_affinity_workspace_bytes(long long n, int n_neighbors) {
  using namespace pinn;
  if (!rows_ok(n) || n_neighbors < 1 || n_neighbors > kMaxNb) return 0;
  return 4 * aff_n_bytes(n) + align256((size_t)n * n_neighbors * 8);
}

extern "C" int pinn_sp_affinity(long long n, int n_neighbors, const long long* d_knn, long long* d_indptr, long long* d_indices,
                                double* d_data, double* d_degree, double* d_dd, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  const int k = n_neighbors;
  if (!rows_ok(n) || k < 1 || k > kMaxNb) return PINN_E_ARG;
  if (!d_knn || !d_indptr || !d_indices || !d_data || !d_degree || !d_dd || !d_ws) return PINN_E_ARG;
  if (misaligned8(d_knn) || misaligned8(d_indptr) || misaligned8(d_indices) || misaligned8(d_data) || misaligned8(d_degree) || misaligned8(d_dd) ||
      misaligned8(d_ws))
    return PINN_E_ARG;
  if (ws_bytes < pinn_sp_affinity_workspace_bytes(n, k)) return PINN_E_WORKSPACE;
  const AffWs w = aff_carve(d_ws, n);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const hipError_t e = hipMemsetAsync(d_ws, 0, 2 * aff_n_bytes(n), st);            // the counts and the slot cursors
  if (e != hipSuccess) return (int)e;
  const unsigned ge = blocks_of(n * k, kBT);
  hipLaunchKernelGGL(aff_count_kernel, dim3(ge), dim3(kBT), 0, st, n, k, d_knn, w.incnt);
  hipLaunchKernelGGL(aff_scan_kernel, dim3(1), dim3(kBT), 0, st, n, w.incnt, w.toff);
  hipLaunchKernelGGL(aff_fill_kernel, dim3(ge), dim3(kBT), 0, st, n, k, d_knn, w.toff, w.cursor, w.tin);
  hipLaunchKernelGGL(aff_len_kernel, dim3((unsigned)n), dim3(kRowT), 0, st, n, k, d_knn, w.toff, w.tin, w.len);
  hipLaunchKernelGGL(aff_scan_kernel, dim3(1), dim3(kBT), 0, st, n, w.len, d_indptr);
  hipLaunchKernelGGL(aff_write_kernel, dim3((unsigned)n), dim3(kRowT), 0, st, n, k, d_knn, w.toff, w.tin, d_indptr, d_indices, d_data, d_degree, d_dd);
  return launch_status();
}

extern "C" size_t pinn_sp_eigs_state_bytes(long long n, int n_components) {
  using namespace pinn;
  if (!eig_ok(n, n_components)) return 0;
  return eg_words(n, block_cols(n, n_components)) * sizeof(double);
}

extern "C" size_t pinn_sp_eigs_workspace_bytes(long long n, int n_components) {
  using namespace pinn;
  if (!eig_ok(n, n_components)) return 0;
  const int m = block_cols(n, n_components);
  return align256((size_t)n * 8) + 2 * align256((size_t)n * m * 8) + align256((size_t)m * m * 8) + align256((size_t)kGBlocks * m * m * 8) +
         align256((size_t)kGBlocks * m * 8) + align256((size_t)kMaxK * 8);
}

extern "C" int pinn_sp_eigs(long long n, const long long* d_indptr, const long long* d_indices, const double* d_data, long long nnz,
                            const double* d_dd, int n_components, int init, int n_outer, double tol, double* d_state, void* d_ws,
                            size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (!eig_ok(n, n_components) || nnz < 0 || n_outer < 0 || n_outer > 10000 || !(tol >= 0.0)) return PINN_E_ARG;
  if (!d_indptr || !d_dd || !d_state || !d_ws || (nnz > 0 && (!d_indices || !d_data))) return PINN_E_ARG;
  if (misaligned8(d_indptr) || misaligned8(d_indices) || misaligned8(d_data) || misaligned8(d_dd) || misaligned8(d_state) || misaligned8(d_ws))
    return PINN_E_ARG;
  if (ws_bytes < pinn_sp_eigs_workspace_bytes(n, n_components)) return PINN_E_WORKSPACE;
  const int K = n_components, m = block_cols(n, K);
  const EigWs w = eig_carve(d_ws, n, m);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  Csr g;
  g.indptr = d_indptr; g.indices = d_indices; g.data = d_data; g.n = n; g.nnz = nnz;
  double* Q = d_state + eg_q(m);
  const unsigned ge = blocks_of(n * m, kBT);
  const int G = row_blocks(n, kGR, kGBlocks);
  auto ortho = [&](int gram_mode, int rot_mode) {
    hipLaunchKernelGGL(eg_gram_kernel, dim3(G), dim3(kBT), 0, st, d_state, gram_mode, n, m, Q, w.W, w.part);
    hipLaunchKernelGGL(eg_jacobi_kernel, dim3(1), dim3(kBT), 0, st, d_state, (int)JAC_ORTHO, m, G, w.part, w.T);
    hipLaunchKernelGGL(eg_rotate_kernel, dim3(G), dim3(kBT), 0, st, d_state, rot_mode, n, m, w.T, Q, w.W, w.part_res);
  };
  if (init) {
    hipLaunchKernelGGL(eg_rdd_kernel, dim3(blocks_of(n, kBT)), dim3(kBT), 0, st, n, d_dd, w.rdd);
    hipLaunchKernelGGL(eg_header_kernel, dim3(1), dim3(1), 0, st, d_state, n, m, K, tol);
    ortho(GRAM_A, ROT_A);
    ortho(GRAM_A, ROT_A);
  }
  for (int it = 0; it < n_outer; ++it) {
    hipLaunchKernelGGL(eg_spmm_kernel, dim3(ge), dim3(kBT), 0, st, d_state, -1, g, m, w.rdd, Q, w.B);
    hipLaunchKernelGGL(eg_gram_kernel, dim3(G), dim3(kBT), 0, st, d_state, (int)GRAM_H, n, m, Q, w.B, w.part);
    hipLaunchKernelGGL(eg_jacobi_kernel, dim3(1), dim3(kBT), 0, st, d_state, (int)JAC_RITZ, m, G, w.part, w.T);
    hipLaunchKernelGGL(eg_rotate_kernel, dim3(G), dim3(kBT), 0, st, d_state, (int)ROT_RITZ, n, m, w.T, Q, w.B, w.part_res);
    hipLaunchKernelGGL(eg_decide_kernel, dim3(1), dim3(64), 0, st, d_state, m, K, G, w.part_res);
    for (int s = 0; s < PINN_SP_MAX_DEGREE; ++s)
      hipLaunchKernelGGL(eg_spmm_kernel, dim3(ge), dim3(kBT), 0, st, d_state, s, g, m, w.rdd, Q, w.W);
    ortho(GRAM_SRC, ROT_SRC);
    ortho(GRAM_A, ROT_A);
  }
  return launch_status();
}

extern "C" int pinn_sp_embed(long long n, int n_components, const double* d_dd, const double* d_state, double* d_embedding,
                             void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (!eig_ok(n, n_components)) return PINN_E_ARG;
  if (!d_dd || !d_state || !d_embedding || !d_ws || misaligned8(d_dd) || misaligned8(d_state) || misaligned8(d_embedding) || misaligned8(d_ws))
    return PINN_E_ARG;
  if (ws_bytes < pinn_sp_eigs_workspace_bytes(n, n_components)) return PINN_E_WORKSPACE;
  const int K = n_components, m = block_cols(n, K);
  const EigWs w = eig_carve(d_ws, n, m);
  hipStream_t st = (hipStream_t)stream;
  clear_error();
  const double* Q = d_state + eg_q(m);
  hipLaunchKernelGGL(embed_sign_kernel, dim3(K), dim3(kBT), 0, st, n, m, Q, d_dd, w.sign);
  hipLaunchKernelGGL(embed_write_kernel, dim3(blocks_of(n * K, kBT)), dim3(kBT), 0, st, n, m, K, Q, d_dd, w.sign, d_embedding);
  return launch_status();
}

extern "C" size_t pinn_sp_lloyd_state_bytes(long long n, int n_clusters, int n_dim) {
  if (!pinn::lloyd_ok(n, n_clusters, n_dim)) return 0;
  return pinn::km_words(n, n_clusters, n_dim) * sizeof(double);
}

extern "C" size_t pinn_sp_lloyd_workspace_bytes(long long n, int n_clusters, int n_dim) {
  using namespace pinn;
  if (!lloyd_ok(n, n_clusters, n_dim)) return 0;
  return lloyd_workspace_bytes(kLBlocks, n_clusters, n_dim);
}

extern "C" int pinn_sp_lloyd(const double* d_x, long long n, int n_dim, int n_clusters, int init, int n_iters, double tol, int finish,
                             double* d_state, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace pinn;
  if (!lloyd_ok(n, n_clusters, n_dim) || n_iters < 0 || n_iters > 100000 || !(tol >= 0.0)) return PINN_E_ARG;
  if (!d_x || !d_state || !d_ws || misaligned8(d_x) || misaligned8(d_state) || misaligned8(d_ws)) return PINN_E_ARG;
  if (ws_bytes < pinn_sp_lloyd_workspace_bytes(n, n_clusters, n_dim)) return PINN_E_WORKSPACE;
  return lloyd_queue<PackedSrc, kLMaxK, kLMaxD, kBT>(PackedSrc{d_x}, n, n_dim, n_clusters, kLBlocks, init, n_iters, tol, finish, d_state, d_ws,
                                                     (hipStream_t)stream);
}
