// pinn_general.hip -- any layers list [8, h_1, ..., h_k, 1] (01:389-438) on exact-fp32 layer-by-layer kernels for gfx950.
//
// The fused chain (pinn_mlp.hip / pinn_train.hip, H in {128, 256}) and the wide kernels (pinn_wide.hip, H in {512, 1024, 2048})
// need one width for every hidden layer.  This family takes unequal widths 1 <= h_i <= 2048: every layer is one launch of a
// tiled GEMM on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain: exact fp32) with the layer's elementwise work fused into its
// epilogue, and activations go through HBM in caller-provided workspace, one bounded row chunk at a time.
//
//   gemm_kernel<kFwd, 1>   act_out^T[f][r] = tanh(b[f] + sum_k W[f][k] act_in[r][k]), then dropout (Philox or injected bits)
//   gemm_kernel<kBwd, 1>   dpre_in[r][i] = (sum_o W[o][i] dpre_out[r][o] (+ w_p[i] du[r])) * scale * keep * (1 - a^2)
//   gemm_kernel<kWgrad, 1> slab[s][o][i] = sum_{r in slice s} dpre_out[r][o] act_in[r][i]; column i = n_in is the bias (a ones column)
//   heads_kernel           predict dot, variance-head dot, softplus / log, per-row dL/du, dL/dz, loss partials, d pre_v2
//                          (kHeadGrad: dL/du, dL/dlogvar given by the caller -- the backward of torch autograd)
//   dx_kernel              dL/dx = W_0^T dpre_0 per row (the backward's input gradient)
//   vec_grad_kernel        the two 1-row tensors (predict, last variance layer) of the gradient, per slice
//   reduce / finalize      fixed-order slab sums -> the flat gradient (state_dict layout); loss sums in fp64
//   gemm_kernel<., 2>, head2_kernel, vec_grad2_kernel   the double backward (pinn_gnet_backward2): see the section below
//   mc_moments_kernel      MC-dropout: (pass, row) pairs are virtual rows; per row, in pass order, the Welford moments of pinn_mc_dropout
//   pack, gemm<., 1>, heads, vec_grad, reduce, finalize take a member index from the launch grid (struct Members): E equal networks in
//   the launches of one, member m bit for bit the single call (pinn_gens_*); combine_kernel reads the members as a mixture
//
// Widths are padded to 32 inside the workspace only (zero weights, zero activations); the flat parameter buffer holds exactly the
// reference's tensors.  Determinism: no floating-point atomics; every output element's K order is fixed by the layer alone (the
// same 32-wide K slabs in the same order for every tile), so a row's forward / MC result does not depend on its tile or chunk.
#include "pinn_mlp_core.h"

namespace pinn {
namespace gen {

constexpr int kMaxHidden = 8;
constexpr int kMaxMat = kMaxHidden + 4;      // hidden layers, predict, variance head 0, 1, 2
constexpr int kMaxWidth = 2048;
constexpr int kLd = 36;                      // LDS row stride (floats) of a 64 x 32 operand tile
constexpr int kBK = 32;
constexpr size_t kTrainBudget = 512ull << 20;   // activation bytes per training chunk
constexpr size_t kInferBudget = 256ull << 20;   // activation bytes per inference chunk
constexpr long long kMaxChunkRows = 131072;
constexpr long long kMaxVirtualRows = 1ll << 20;
constexpr size_t kSlabBudget = 256ull << 20;

enum { kFwd = 0, kBwd = 1, kWgrad = 2 };

__host__ __device__ inline long long rup(long long v, long long m) { return (v + m - 1) / m * m; }

// ---------------------------------------------------------------------------------------
// shape, flat layout and workspace layout (host)
// ---------------------------------------------------------------------------------------
struct Shape {
  int k;                       // hidden layers
  int w[kMaxHidden];           // hidden widths
  int hk, hv1, hv2;            // last hidden width, h_k // 2, h_k // 4
  int n_mat;                   // k + 4
  int out[kMaxMat], in[kMaxMat];
  long long woff[kMaxMat], boff[kMaxMat], total;     // flat buffer (floats)
  long long reg[kMaxMat], gtotal;                    // gradient regions [out][in + 1] (bias = column in), 16-B aligned
  long long pf[kMaxMat], pt[kMaxMat], pack_total;    // packed copies: forward [mp][kp], transposed [kp][mp]; -1 = none
  int mp[kMaxMat], kp[kMaxMat];
  int word_off[kMaxHidden + 1], words;               // keep-word offset of dropout module l, words per row
  int max_wp;
  int mat_pred() const { return k; }
  int mat_v0() const { return k + 1; }
  int mat_v1() const { return k + 2; }
  int mat_v2() const { return k + 3; }
  bool is_gemm(int t) const { return t < k || t == k + 1 || t == k + 2; }
};

static int make_shape(const pinn_gnet_t* net, Shape* s) {
  if (!net) return PINN_E_ARG;
  if (net->n_in != 8 || net->n_out != 1) return PINN_E_ARCH;
  if (net->n_hidden < 1 || net->n_hidden > kMaxHidden) return PINN_E_ARCH;
  for (int l = 0; l < net->n_hidden; ++l)
    if (net->width[l] < 1 || net->width[l] > kMaxWidth) return PINN_E_ARCH;
  if (net->width[net->n_hidden - 1] < 4) return PINN_E_ARCH;
  s->k = net->n_hidden;
  for (int l = 0; l < kMaxHidden; ++l) s->w[l] = l < s->k ? net->width[l] : 0;
  s->hk = s->w[s->k - 1]; s->hv1 = s->hk / 2; s->hv2 = s->hk / 4;
  s->n_mat = s->k + 4;
  for (int t = 0; t < s->k; ++t) { s->out[t] = s->w[t]; s->in[t] = t == 0 ? 8 : s->w[t - 1]; }
  s->out[s->k] = 1;          s->in[s->k] = s->hk;
  s->out[s->k + 1] = s->hv1; s->in[s->k + 1] = s->hk;
  s->out[s->k + 2] = s->hv2; s->in[s->k + 2] = s->hv1;
  s->out[s->k + 3] = 1;      s->in[s->k + 3] = s->hv2;
  long long off = 0, g = 0, p = 0;
  s->max_wp = 0;
  for (int t = 0; t < s->n_mat; ++t) {
    s->woff[t] = off; off += rup((long long)s->out[t] * s->in[t], 4);
    s->boff[t] = off; off += rup(s->out[t], 4);
    s->reg[t] = g; g += rup((long long)s->out[t] * (s->in[t] + 1), 4);
    s->mp[t] = (int)rup(s->out[t], 32); s->kp[t] = (int)rup(s->in[t], 32);
    s->pf[t] = s->pt[t] = -1;
    if (s->is_gemm(t)) {
      s->pf[t] = p; p += (long long)s->mp[t] * s->kp[t];
      if (t != 0) { s->pt[t] = p; p += (long long)s->mp[t] * s->kp[t]; }
      if (s->mp[t] > s->max_wp) s->max_wp = s->mp[t];
    }
  }
  s->total = off; s->gtotal = g; s->pack_total = p;
  int wo = 0;
  for (int l = 0; l <= s->k; ++l) { s->word_off[l] = wo; wo += ((l < s->k ? s->w[l] : s->hv1) + 31) / 32; }
  s->words = wo;
  return PINN_OK;
}

// output activation buffer of GEMM matrix t (width mp[t]); index into Layout::act
static int act_index(const Shape& s, int t) { return t < s.k ? t : (t == s.mat_v0() ? s.k : s.k + 1); }

struct Layout {
  long long rows;              // rows (virtual rows) per chunk
  int slices; long long slice_rows;
  // [stream]: 0 = the primal activations / p, 1 = the double backward's tangent activations / q.  Inference: act[0][0..2] ping-pong
  size_t pack, act[2][kMaxHidden + 2], keep, dpre[2][2], du, dz, pz, slabs, acc, loss, ubuf, lvbuf, state, end;
};

static size_t take(size_t& at, size_t bytes) { const size_t o = at; at = (at + bytes + 255) / 256 * 256; return o; }

static long long n_chunks(long long n, long long r) { return (n + r - 1) / r; }

// weight-gradient slices of a chunk of `rows` rows: enough tiles to fill the chip, at most kSlabBudget of partial slabs, >= 128 rows each
static void slice_plan(const Shape& s, long long rows, long long* slice_rows, int* slices) {
  long long tiles = 1;
  for (int t = 0; t < s.n_mat; ++t)
    if (s.is_gemm(t)) {
      const long long tt = rup(s.out[t], 64) / 64 * (rup(s.in[t] + 1, 64) / 64);
      if (tt > tiles) tiles = tt;
    }
  long long sl = (2048 + tiles - 1) / tiles;
  const long long by_rows = rows / 128 > 1 ? rows / 128 : 1;
  const long long by_mem = (long long)(kSlabBudget / (4 * (size_t)s.gtotal)) > 1 ? (long long)(kSlabBudget / (4 * (size_t)s.gtotal)) : 1;
  if (sl > by_rows) sl = by_rows;
  if (sl > by_mem) sl = by_mem;
  if (sl < 1) sl = 1;
  *slice_rows = rup((rows + sl - 1) / sl, kBK);
  *slices = (int)((rows + *slice_rows - 1) / *slice_rows);
}

// training: every activation of a chunk is kept for the backward pass.  ns = 1: pinn_gnet_train_grads / pinn_gnet_backward (with the
// loss partials).  ns = 2: the double backward keeps a primal and a tangent activation per layer, two (p, q) ping-pong pairs and a third
// per-row scalar (du = g_u, dz = q_v2, pz = p_v2): about twice the bytes per row, so about half the chunk
static Layout train_layout(const Shape& s, long long n_rows, int ns) {
  Layout L{};
  long long per_row = s.words + 2LL * ns * s.max_wp + ns + 1;
  for (int t = 0; t < s.n_mat; ++t) if (s.is_gemm(t)) per_row += (long long)ns * s.mp[t];
  long long cap = (long long)(kTrainBudget / (4 * (size_t)per_row)) / 64 * 64;
  cap = cap < 64 ? 64 : (cap > kMaxChunkRows ? kMaxChunkRows : cap);
  L.rows = rup(n_rows < 1 ? 1 : n_rows, 64);
  if (L.rows > cap) L.rows = cap;
  slice_plan(s, L.rows, &L.slice_rows, &L.slices);
  size_t at = 0;
  L.pack = take(at, 4 * (size_t)s.pack_total);
  for (int t = 0; t < s.n_mat; ++t)
    if (s.is_gemm(t))
      for (int q = 0; q < ns; ++q) L.act[q][act_index(s, t)] = take(at, 4 * (size_t)L.rows * s.mp[t]);
  L.keep = take(at, 4 * (size_t)L.rows * s.words);
  for (int b = 0; b < 2; ++b)
    for (int q = 0; q < ns; ++q) L.dpre[q][b] = take(at, 4 * (size_t)L.rows * s.max_wp);
  L.du = take(at, 4 * (size_t)L.rows);
  L.dz = take(at, 4 * (size_t)L.rows);
  if (ns == 2) L.pz = take(at, 4 * (size_t)L.rows);
  L.slabs = take(at, 4 * (size_t)L.slices * s.gtotal);
  L.acc = take(at, 4 * (size_t)s.gtotal);
  if (ns == 1) L.loss = take(at, 8 * 8 * (size_t)(n_chunks(n_rows, L.rows) * (L.rows / 16)));
  L.end = at;
  return L;
}

// forward / MC-dropout: two ping-pong activation buffers (+ one for the variance head's second layer) per chunk of virtual rows (pass, row)
static Layout infer_layout(const Shape& s, long long n_rows, int n_passes) {
  Layout L{};
  const long long per_row = 3LL * s.max_wp + 2;
  long long cap = (long long)(kInferBudget / (4 * (size_t)per_row)) / 64 * 64;
  cap = cap < 64 ? 64 : (cap > kMaxVirtualRows ? kMaxVirtualRows : cap);
  const long long v = (n_rows < 1 ? 1 : n_rows) * (n_passes > 0 ? (long long)n_passes + 1 : 1);
  L.rows = rup(v, 64);
  if (L.rows > cap) L.rows = cap;
  size_t at = 0;
  L.pack = take(at, 4 * (size_t)s.pack_total);
  L.act[0][0] = take(at, 4 * (size_t)L.rows * s.max_wp);
  L.act[0][1] = take(at, 4 * (size_t)L.rows * s.max_wp);
  L.act[0][2] = take(at, 4 * (size_t)L.rows * s.max_wp);
  L.ubuf = take(at, 4 * (size_t)L.rows);
  L.lvbuf = take(at, 4 * (size_t)L.rows);
  L.state = take(at, 4 * 4 * (size_t)(n_passes > 0 ? n_rows : 0));
  L.end = at;
  return L;
}

// ---------------------------------------------------------------------------------------
// dropout (device copy; same Philox stream and 16-bit threshold as every other kernel)
// ---------------------------------------------------------------------------------------
struct Drop {
  int mode;
  unsigned thr[kMaxDrop];
  float scale[kMaxDrop];
  unsigned seed_lo, seed_hi, stream;
  long long row_offset;
  const unsigned* bits;
  int words;
};

static int convert(const Shape& s, const pinn_dropout_t* in, Drop* d) {
  d->mode = PINN_DROP_NONE; d->seed_lo = d->seed_hi = d->stream = 0; d->row_offset = 0; d->bits = nullptr; d->words = s.words;
  for (int l = 0; l < kMaxDrop; ++l) { d->thr[l] = 0; d->scale[l] = 1.0f; }
  if (!in) return PINN_OK;
  if (in->mode < PINN_DROP_NONE || in->mode > PINN_DROP_BITS) return PINN_E_ARG;
  if (in->d_step_counter) return PINN_E_ARG;        // general nets run launch by launch (no captured replay)
  d->mode = in->mode;
  d->row_offset = in->row_offset;
  if (in->mode == PINN_DROP_NONE) return PINN_OK;
  for (int l = 0; l <= s.k; ++l)
    if (!drop_rate(in->p[l], &d->thr[l], &d->scale[l])) return PINN_E_ARG;
  d->seed_lo = (unsigned)(in->seed & 0xFFFFFFFFull);
  d->seed_hi = (unsigned)(in->seed >> 32);
  d->stream = in->stream;
  if (in->mode == PINN_DROP_BITS) {
    if (!in->d_bits) return PINN_E_ARG;
    d->bits = in->d_bits;
  }
  return PINN_OK;
}

// ---------------------------------------------------------------------------------------
// weight packing: zero-padded forward [mp][kp] and transposed [kp][mp] copies of the GEMM matrices
// ---------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------
// the member dimension (pinn_gens_*): one launch of pack, gemm<., 1>, heads, vec_grad, reduce and finalize serves every member of an
// ensemble of n equal networks.  The member index comes from the launch grid, and member m's buffers lie m strides behind member 0's:
//   work  the workspace (4-byte words): n copies of the regions of one network's Layout -- packed weights, activations, keep words,
//         d pre-activations, du / dz, slabs, acc, loss partials.  A member's Layout is the single network's, so its chunks, slices and
//         fixed-order sums are too
//   par   the flat parameters and the flat gradient [n][pinn_gnet_param_count]
//   out   the per-row outputs u, logvar [n][n_rows]
// The input rows and the targets are shared.  Member m draws the Philox stream of seed + m.  One member (every pinn_gnet_* call):
// index 0, strides unused.  The double backward (NS = 2), dx_kernel and the MC-dropout kernels have no member dimension.
// ---------------------------------------------------------------------------------------
struct Members { int n; long long work, par, out; };

struct PackJob { long long src, dst; int out, in, mp, kp, transposed; };
struct PackArgs { const float* params; float* pack; PackJob job[2 * kMaxMat]; int n_jobs; Members mem; };

__global__ __launch_bounds__(256) void pack_kernel(PackArgs a) {
  const PackJob j = a.job[blockIdx.y];
  const float* __restrict__ params = a.params + (long long)blockIdx.z * a.mem.par;
  float* __restrict__ pack = a.pack + (long long)blockIdx.z * a.mem.work;
  const long long n = (long long)j.mp * j.kp;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    int o, i;
    if (j.transposed) { i = (int)(e / j.mp); o = (int)(e - (long long)i * j.mp); }
    else { o = (int)(e / j.kp); i = (int)(e - (long long)o * j.kp); }
    pack[j.dst + e] = (o < j.out && i < j.in) ? params[j.src + (long long)o * j.in + i] : 0.0f;
  }
}

// ---------------------------------------------------------------------------------------
// the layer GEMM: 64 x 64 output tile per 256-thread workgroup, 32 x 32 per wave (2 x 2 MFMA blocks), K slabs of 32.
// FWD / BWD: M = features (A: packed weights, K-contiguous), N = rows (B: activations [row][k], K-contiguous).
// WGRAD:     M = output features (A: d pre-activations [row][o]), N = input features (B: activations [row][i]), K = rows.
// One kernel for one activation stream (NS = 1: forward, MC-dropout, the first-order backward) and for two that share the weight
// operand (NS = 2, the double backward: primal / tangent activations in FWD, the (p, q) pair in BWD and WGRAD; expressions in the
// double-backward section below).  FWD / BWD with NS = 2 hold one weight tile and two activation tiles in LDS and two accumulator
// sets; WGRAD is one reduction over the rows of stream 0 and then of stream 1 into one accumulator set.
// ---------------------------------------------------------------------------------------
struct GemmArgs {
  const float* A; long long lda; long long a_mv, a_kv;
  const float* B; long long ldb; long long b_mv, b_kv;
  long long M, K;                // output feature extent (stores: m < M), contraction length (FWD / BWD)
  float* out; long long ldo;
  long long n_valid;             // valid rows of the chunk
  // FWD
  const float* bias; int bias_n; int module;   // dropout module of the output (-1: tanh only)
  int map_rows;                  // B rows are input rows: chunk row n -> row0 + n (MC: virtual row -> row % n_rows)
  int mc;                        // virtual rows (pass, row) of MC-dropout; NS = 1 only
  long long row0, n_rows;
  Drop drop;
  unsigned* keep; int keep_off;  // keep words [row][drop.words] (training), module word offset
  // BWD
  const float* stash; long long ld_stash; int stash_module;
  const float* wp; const float* du; int wp_n;
  const unsigned* keep_in;
  // WGRAD
  long long slice_rows; float* slab; long long slab_stride; long long reg; int out_real, in_real;
  // the second stream (NS = 2; same strides and extents as the first): WGRAD q; the tangent input / BWD q; their outputs; the kept tangent
  const float* A2; const float* B2; float* out2; const float* stash2;
  // members (NS = 1): FWD / BWD take the member from the grid's z; WGRAD, whose z counts slices, from its x = member * tiles_x + tile.
  // A, out, keep, stash, du, keep_in and slab are workspace, bias and wp parameters, B workspace unless it is the shared input rows
  Members mem; int b_shared; unsigned tiles_x;
};

// one 64 x 32 operand tile: K-contiguous source (row m, 4 consecutive k per float4)
__device__ __forceinline__ void load_kc(f32x4 (&r)[2], const float* __restrict__ p, long long ld, long long m0, long long k0,
                                        long long mv, long long kv, int tid) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long long m = m0 + (tid >> 3) + 32 * q, k = k0 + (tid & 7) * 4;
    r[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (m < mv && k < kv) r[q] = *reinterpret_cast<const f32x4*>(p + m * ld + k);
  }
}
__device__ __forceinline__ void store_kc(float* s, const f32x4 (&r)[2], int tid) {
#pragma unroll
  for (int q = 0; q < 2; ++q) *reinterpret_cast<f32x4*>(s + ((tid >> 3) + 32 * q) * kLd + (tid & 7) * 4) = r[q];
}
// MN-contiguous source: element (m, k) at p[k * ld + m], 4 consecutive m per float4
__device__ __forceinline__ void load_mc(f32x4 (&r)[2], const float* __restrict__ p, long long ld, long long m0, long long k0,
                                        long long mv, long long kv, int tid, int ones_col, float one = 1.0f) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const long long k = k0 + (tid >> 4) + 16 * q, m = m0 + (tid & 15) * 4;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (k < kv && m < mv) v = *reinterpret_cast<const f32x4*>(p + k * ld + m);
    if (ones_col >= 0) {          // columns >= the layer's real input width: the bias column (1 on valid rows), then zeros
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (m + e >= ones_col) v[e] = (m + e == ones_col && k < kv) ? one : 0.0f;
    }
    r[q] = v;
  }
}
__device__ __forceinline__ void store_mc(float* s, const f32x4 (&r)[2], int tid) {
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int k = (tid >> 4) + 16 * q, m = (tid & 15) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) s[(m + e) * kLd + k] = r[q][e];
  }
}

// row context of chunk row n in FWD: input row (for x and the Philox / bit-mask keys) and pass (-1: MC eval pass, dropout off).
// MC virtual rows come with one stream only
template <int NS>
__device__ __forceinline__ void row_ctx(const GemmArgs& a, long long n, long long& lrow, int& pass) {
  if (NS == 1 && a.mc) {
    const long long v = a.row0 + n;
    const long long q = v / a.n_rows;
    lrow = v - q * a.n_rows;
    pass = (int)q - 1;
  } else {
    lrow = a.row0 + n;
    pass = 0;
  }
}

// The keep word of the FWD output module for input row lrow (valid: the chunk row exists) in pass `pass`, feature group P (32
// features): bit 16 i + 4 kq + r keeps feature 32 P + 16 i + 4 kq + r.  Every pass over a row -- forward, MC-dropout, the first- and
// the second-order backward's recomputing forwards -- takes its masks from here, so they cannot disagree about them.
// on = the module drops in this pass.  Philox: lane quarter kq draws its own 8 bits (counter = global row, key word = module, P, kq;
// stream + pass) and the four quarters of a row are OR-ed by two shuffles, so all 64 lanes of the wave must call.  Member mem of an
// ensemble draws with seed + mem (64-bit wrap): the stream of the single call with that seed.
__device__ __forceinline__ unsigned keep_word(const GemmArgs& a, int mem, bool on, long long lrow, int pass, bool valid, int P, int kq) {
  const unsigned thr = a.module >= 0 ? a.drop.thr[a.module] : 0u;
  unsigned mine = 0;
  if (on && a.drop.mode == PINN_DROP_PHILOX) {
    const unsigned long long g = (unsigned long long)(a.drop.row_offset + lrow);
    const unsigned long long seed = (((unsigned long long)a.drop.seed_hi << 32) | a.drop.seed_lo) + (unsigned long long)mem;
    unsigned o[4];
    philox4x32_10((unsigned)g, (unsigned)(g >> 32), ((unsigned)a.module << 16) | ((unsigned)P << 2) | (unsigned)kq,
                  a.drop.stream + (unsigned)pass, (unsigned)seed, (unsigned)(seed >> 32), o);
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int idx = 4 * b + r;
        const unsigned draw = (o[idx >> 1] >> (16 * (idx & 1))) & 0xFFFFu;
        mine |= (draw >= thr ? 1u : 0u) << (16 * b + 4 * kq + r);
      }
  }
  mine |= __shfl_xor(mine, 16, 64);
  mine |= __shfl_xor(mine, 32, 64);
  unsigned word = 0xFFFFFFFFu;
  if (on && a.drop.mode == PINN_DROP_PHILOX) word = mine;
  // (a wave whose 32 features lie past the layer's padded width stores nothing; its word would be the next module's or, for the last
  // module of the last row, the word past the end of the masks)
  if (on && a.drop.mode == PINN_DROP_BITS && valid && 32LL * P < a.M)
    word = a.drop.bits[((long long)pass * a.n_rows + lrow) * a.drop.words + a.keep_off + P];
  return word;
}

// tanh of the layer epilogue.  tanh_f32 (pinn_mlp_core.h) is 1 - 2 / (e^{2x} + 1): its error is absolute, about 1.5e-7, so a
// pre-activation of 0.01 gets an activation with a relative error of 1e-5, and a head's dot product over small activations (narrow or
// deep lists) leaves the band of a float32 tanh, and so does the double backward, whose (1 - h^2) and -2 h terms read the kept h
// (tests/test_gpu_general_referee.py).  Below |x| = 1 an odd polynomial, x (1 + x^2 P(x^2)) with P the degree-9 Chebyshev interpolant
// of (tanh(s) / s - 1) / s^2 in s^2 on [0, 1], is within 1.6 ulp in float32; from 1 on tanh_f32 is within 2 ulp of its own arithmetic.
__device__ __forceinline__ float tanh_rel(float x) {
  const float x2 = x * x;
  float p = 1.3777387721347623e-05f;
  p = fmaf(p, x2, -0.00010976991325151175f);
  p = fmaf(p, x2, 0.0004508132115006447f);
  p = fmaf(p, x2, -0.0013538711937144399f);
  p = fmaf(p, x2, 0.003541822312399745f);
  p = fmaf(p, x2, -0.008846853859722614f);
  p = fmaf(p, x2, 0.021866105496883392f);
  p = fmaf(p, x2, -0.05396784096956253f);
  p = fmaf(p, x2, 0.13333331048488617f);
  p = fmaf(p, x2, -0.3333333432674408f);
  return fabsf(x) < 1.0f ? fmaf(x, x2 * p, x) : tanh_f32(x);
}

template <int MODE, int NS>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs a) {
  constexpr int NB = MODE == kWgrad ? 1 : NS;      // activation tiles in LDS and accumulator sets
  __shared__ __attribute__((aligned(16))) float As[64 * kLd];
  __shared__ __attribute__((aligned(16))) float Bs[NB][64 * kLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4, li = lane & 15;
  const int wm = wave & 1, wn = wave >> 1;
  unsigned bx = blockIdx.x;
  int mem = 0;
  if (NS == 1) {
    if (MODE == kWgrad) { mem = (int)(bx / a.tiles_x); bx -= (unsigned)mem * a.tiles_x; }
    else mem = (int)blockIdx.z;
  }
  const long long wo = mem * a.mem.work, po = mem * a.mem.par;
  const float* __restrict__ A = a.A + wo;
  const float* __restrict__ B = a.B + (a.b_shared ? 0 : wo);
  const long long m0 = (long long)blockIdx.y * 64, n0 = (long long)bx * 64;
  long long kbeg = 0, kend = a.K, span = 0;
  if (MODE == kWgrad) {
    kbeg = (long long)blockIdx.z * a.slice_rows;
    kend = kbeg + a.slice_rows;
    if (kend > a.K) kend = a.K;
    if (NS == 2) {               // the slice's rows of (p, a) at k in [kbeg, kbeg + span), then the same rows of (q, ad);
                                 // slice_rows and K are multiples of kBK, so span is whole K slabs
      span = kend - kbeg;
      kend += span;
    }
  }

  // NS = 2: acc[0] is the primal pre-activation (FWD) / abar, which becomes p (BWD); acc[1] the tangent / adbar, which becomes q
  f32x4 acc[NB][2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int s = 0; s < NB; ++s) acc[s][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (MODE == kFwd) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long m = m0 + 32 * wm + 16 * i + 4 * kq + r;
          acc[0][i][j][r] = m < a.bias_n ? a.bias[po + m] : 0.0f;
        }
      }
      if (MODE == kBwd && a.wp) {       // the predict head joins the stream of the first-order chain
        const long long n = n0 + 32 * wn + 16 * j + li;
        const float du = a.du[wo + n];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long m = m0 + 32 * wm + 16 * i + 4 * kq + r;
          acc[NB - 1][i][j][r] = (m < a.wp_n ? a.wp[po + m] : 0.0f) * du;
        }
      }
    }

  // WGRAD with NS = 2: the K slabs from kbeg + span on belong to the second stream (its bias column is 0), rows k0 - span
  auto second = [&](long long k0) { return MODE == kWgrad && NS == 2 && k0 >= kbeg + span; };
  // B rows of the FWD input layer are input rows (x, and v for the tangent), possibly virtual (MC)
  auto load_b = [&](f32x4 (&r)[2], const float* __restrict__ p, long long k0) {
    if (MODE == kWgrad) {
      const bool s2 = second(k0);
      load_mc(r, s2 ? a.B2 : B, a.ldb, n0, s2 ? k0 - span : k0, a.b_mv, a.b_kv, tid, a.in_real, s2 ? 0.0f : 1.0f);
    } else if (MODE == kFwd && a.map_rows) {
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const long long n = n0 + (tid >> 3) + 32 * q, k = k0 + (tid & 7) * 4;
        long long lrow; int pass;
        row_ctx<NS>(a, n, lrow, pass);
        r[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (n < a.n_valid && k < a.b_kv) r[q] = *reinterpret_cast<const f32x4*>(p + lrow * a.ldb + k);
      }
    } else {
      load_kc(r, p, a.ldb, n0, k0, a.b_mv, a.b_kv, tid);
    }
  };
  auto load_a = [&](f32x4 (&r)[2], long long k0) {
    const bool s2 = second(k0);
    if (MODE == kWgrad) load_mc(r, s2 ? a.A2 : A, a.lda, m0, s2 ? k0 - span : k0, a.a_mv, a.a_kv, tid, -1);
    else load_kc(r, A, a.lda, m0, k0, a.a_mv, a.a_kv, tid);
  };
  f32x4 ra[2], rb[NB][2];
  if (kbeg < kend) {
    load_a(ra, kbeg);
#pragma unroll
    for (int s = 0; s < NB; ++s) load_b(rb[s], s ? a.B2 : B, kbeg);
  }
  for (long long k = kbeg; k < kend; k += kBK) {
    __syncthreads();
    if (MODE == kWgrad) store_mc(As, ra, tid); else store_kc(As, ra, tid);
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      if (MODE == kWgrad) store_mc(Bs[s], rb[s], tid); else store_kc(Bs[s], rb[s], tid);
    }
    __syncthreads();
    if (k + kBK < kend) {      // spelled out twice: one lambda around the pair costs the single-stream forward 8 VGPRs and 2 % at thin layers
      load_a(ra, k + kBK);
#pragma unroll
      for (int s = 0; s < NB; ++s) load_b(rb[s], s ? a.B2 : B, k + kBK);
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 fa[2], fb[NB][2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const f32x4*>(As + (32 * wm + 16 * i + li) * kLd + 16 * h + 4 * kq);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int s = 0; s < NB; ++s) fb[s][j] = *reinterpret_cast<const f32x4*>(Bs[s] + (32 * wn + 16 * j + li) * kLd + 16 * h + 4 * kq);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int s = 0; s < NB; ++s)
              acc[s][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][r], fb[s][j][r], acc[s][i][j], 0, 0, 0);
    }
  }

  // acc[s][i][j][r] = C_s[m = m0 + 32 wm + 16 i + 4 kq + r][n = n0 + 32 wn + 16 j + li]
  const long long mw = m0 + 32 * wm;          // first feature of this wave's 32-feature group
  if (MODE == kWgrad) {
    float* dst = a.slab + wo + (long long)blockIdx.z * a.slab_stride + a.reg;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long o = mw + 16 * i + 4 * kq + r, c = n0 + 32 * wn + 16 * j + li;
          if (o < a.out_real && c <= a.in_real) dst[o * (a.in_real + 1) + c] = acc[0][i][j][r];
        }
    return;
  }
  const int P = (int)(mw >> 5);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long n = n0 + 32 * wn + 16 * j + li;
    const bool valid = n < a.n_valid;
    if (MODE == kFwd) {      // NS = 2: a = c h (bitwise the single stream's), ad = c (1 - h^2) zd
      long long lrow; int pass;
      row_ctx<NS>(a, n, lrow, pass);
      const bool on = a.module >= 0 && a.drop.mode != PINN_DROP_NONE && pass >= 0;
      const float scale = on ? a.drop.scale[a.module] : 1.0f;
      const unsigned word = keep_word(a, mem, on, lrow, pass, valid, P, kq);
      if (mw < a.M) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          f32x4 v, vd;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = tanh_rel(acc[0][i][j][r]);
            const bool kept = (word >> (16 * i + 4 * kq + r)) & 1u;
            v[r] = kept ? t * scale : 0.0f;
            if (NS == 2) vd[r] = (kept && valid) ? acc[NB - 1][i][j][r] * (scale * (1.0f - t * t)) : 0.0f;
          }
          *reinterpret_cast<f32x4*>(a.out + wo + n * a.ldo + mw + 16 * i + 4 * kq) = v;
          if (NS == 2) *reinterpret_cast<f32x4*>(a.out2 + n * a.ldo + mw + 16 * i + 4 * kq) = vd;
        }
        if (a.keep && a.module >= 0 && kq == 0) a.keep[wo + n * a.drop.words + a.keep_off + P] = word;
      }
    } else {      // kBwd
      if (mw < a.M) {
        const bool on = a.drop.mode != PINN_DROP_NONE && a.stash_module >= 0;
        const float scale = on ? a.drop.scale[a.stash_module] : 1.0f, inv_scale = 1.0f / scale;
        const unsigned word = a.stash_module >= 0 ? a.keep_in[wo + n * a.drop.words + a.keep_off + P] : 0xFFFFFFFFu;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const f32x4 h = *reinterpret_cast<const f32x4*>(a.stash + wo + n * a.ld_stash + mw + 16 * i + 4 * kq);
          f32x4 hd, vp, vq;
          if (NS == 2) hd = *reinterpret_cast<const f32x4*>(a.stash2 + n * a.ld_stash + mw + 16 * i + 4 * kq);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float t = h[r] * inv_scale;
            const float d = scale * (1.0f - t * t);
            const float gq = acc[NB - 1][i][j][r] * d;                          // NS = 2: the first backward's dpre, bit for bit
            const float gp = NS == 2 ? acc[0][i][j][r] * d - 2.0f * t * acc[NB - 1][i][j][r] * hd[r] : 0.0f;
            const bool kept = valid && ((word >> (16 * i + 4 * kq + r)) & 1u);
            vq[r] = kept ? gq : 0.0f;
            if (NS == 2) vp[r] = kept ? gp : 0.0f;
          }
          if (NS == 2) *reinterpret_cast<f32x4*>(a.out + n * a.ldo + mw + 16 * i + 4 * kq) = vp;
          *reinterpret_cast<f32x4*>((NS == 2 ? a.out2 : a.out + wo) + n * a.ldo + mw + 16 * i + 4 * kq) = vq;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// heads: 16 lanes per row.  u = w_p . h_k + b_p;  z = w_v2 . v2 + b_v2;  logvar = log(softplus(z) + 1e-6)
// ---------------------------------------------------------------------------------------
enum { kHeadFwd = 0, kHeadMC = 1, kHeadTrain = 2, kHeadGrad = 3 };
struct HeadArgs {
  const float* h; long long ldh; int hk;          // last hidden activation [row][ldh]
  const float* v2; long long ldv; int hv2;        // variance head's second activation [row][ldv]
  const float* wp; const float* bp; const float* wv2; const float* bv2;
  long long n_valid, row0;
  float* u; float* lv;                            // FWD: outputs at row0 + r; MC: chunk buffers at r
  const float* y; long long n_global;             // TRAIN
  const float* gu; const float* glv;              // GRAD: dL/du, dL/dlogvar at row0 + r (glv NULL: zero)
  float* du; float* dz; float* dpre_v2; long long ld_dpre; int wd; double* loss_part;
  Members mem;                                    // member = the grid's y: h, v2, du, dz, dpre_v2, loss_part are workspace, the four
                                                  // head tensors parameters, u and lv outputs; y is shared (kHeadGrad: one member)
};

__device__ __forceinline__ float sum16(float s) {
  s += __shfl_xor(s, 8, 64);
  s += __shfl_xor(s, 4, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 1, 64);
  return s;
}

template <int HM>
__global__ __launch_bounds__(256) void heads_kernel(HeadArgs a) {
  __shared__ double red[16][kLossSums];
  const int tid = threadIdx.x, g = tid & 15, rr = tid >> 4;
  const long long r = (long long)blockIdx.x * 16 + rr;      // chunk row (every one is allocated)
  const long long wo = (long long)blockIdx.y * a.mem.work, po = (long long)blockIdx.y * a.mem.par;
  const float* hrow = a.h + wo + r * a.ldh;
  const float* vrow = a.v2 + wo + r * a.ldv;
  const float* wp = a.wp + po;
  const float* wv2 = a.wv2 + po;
  float su = 0.f, sz = 0.f;
  for (int f = g; f < a.hk; f += 16) su = fmaf(wp[f], hrow[f], su);
  for (int f = g; f < a.hv2; f += 16) sz = fmaf(wv2[f], vrow[f], sz);
  const float u = sum16(su) + a.bp[po];
  const float z = sum16(sz) + a.bv2[po];
  const bool valid = r < a.n_valid;
  if (HM == kHeadFwd || HM == kHeadMC) {
    if (valid && g == 0) {
      const long long o = (HM == kHeadFwd ? a.row0 + r : r) + (long long)blockIdx.y * a.mem.out;
      a.u[o] = u;
      a.lv[o] = logvar_of(z);
    }
    return;
  }
  if (HM == kHeadGrad) {     // given upstream gradients: du = g_u, dz = g_lv * dlogvar/dz (the training head's expressions)
    float du = 0.f, dz = 0.f;
    if (valid) {
      du = a.gu[a.row0 + r];
      if (a.glv) dz = through_logvar(a.glv[a.row0 + r], softplus_slope(z), var_of(z));
    }
    if (g == 0) {
      a.du[r] = du;
      a.dz[r] = dz;
    }
    float* drow = a.dpre_v2 + r * a.ld_dpre;
    for (int f = g; f < a.wd; f += 16) {
      const float v = vrow[f];
      drow[f] = f < a.hv2 ? wv2[f] * dz * (1.0f - v * v) : 0.0f;
    }
    return;
  }
  // aleatoric_loss (01:916-927) and its gradient (pinn_loss.h): one row's terms, as doubles, per 16 lanes
  const float inv_n = (float)(1.0 / (double)a.n_global);
  float du, dz;
  LossSums row;          // this row's terms alone
  loss_row(u, z, a.y[valid ? a.row0 + r : a.row0], inv_n, valid, true, du, dz, row);
  if (g == 0) {
    a.du[wo + r] = du;
    a.dz[wo + r] = dz;
    red[rr][kLossNll] = (double)row.nll;
    red[rr][kLossAbs] = (double)row.abs;
    red[rr][kLossMse] = (double)row.mse;
    red[rr][kLossDu] = (double)du;
    red[rr][kLossDz] = (double)dz;
  }
  // d pre_v2 = w_v2[f] * dz * (1 - v2^2) (zero in the padding and on invalid rows)
  float* drow = a.dpre_v2 + wo + r * a.ld_dpre;
  for (int f = g; f < a.wd; f += 16) {
    const float v = vrow[f];
    drow[f] = f < a.hv2 ? wv2[f] * dz * (1.0f - v * v) : 0.0f;
  }
  __syncthreads();
  if (tid < kLossSums) {
    double s = 0.0;
    for (int q = 0; q < 16; ++q) s += red[q][tid];
    (a.loss_part + wo / 2)[((a.row0 / 16) + blockIdx.x) * kLossTerms + tid] = s;      // the stride is whole 256-byte blocks
  }
}

// ---------------------------------------------------------------------------------------
// the two one-row tensors of the gradient, per slice: predict (du x h_k, bias = sum du), last variance layer (dz x v2, sum dz)
// ---------------------------------------------------------------------------------------
struct VecArgs {
  const float* h; long long ldh; int hk;
  const float* v2; long long ldv; int hv2;
  const float* du; const float* dz;
  long long K, slice_rows;
  float* slab; long long slab_stride, reg_p, reg_v2;
  Members mem;          // member = the grid's z; every pointer is workspace
};
__global__ __launch_bounds__(256) void vec_grad_kernel(VecArgs a) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  const long long r0 = (long long)blockIdx.x * a.slice_rows;
  long long r1 = r0 + a.slice_rows;
  if (r1 > a.K) r1 = a.K;
  const long long wo = (long long)blockIdx.z * a.mem.work;
  const float* __restrict__ h = a.h + wo;
  const float* __restrict__ v2 = a.v2 + wo;
  const float* __restrict__ du = a.du + wo;
  const float* __restrict__ dz = a.dz + wo;
  float* dst = a.slab + wo + (long long)blockIdx.x * a.slab_stride;
  if (c <= a.hk) {
    float s = 0.f;
    for (long long r = r0; r < r1; ++r) s = fmaf(du[r], c < a.hk ? h[r * a.ldh + c] : 1.0f, s);
    dst[a.reg_p + c] = s;
  } else if (c - (a.hk + 1) <= a.hv2) {
    const int j = c - (a.hk + 1);
    float s = 0.f;
    for (long long r = r0; r < r1; ++r) s = fmaf(dz[r], j < a.hv2 ? v2[r * a.ldv + j] : 1.0f, s);
    dst[a.reg_v2 + j] = s;
  }
}

// dL/dx of the valid rows: gx[row0 + r][i] = sum_o W_0[o][i] dpre_0[r][o].  16 lanes per row; lane g takes o = g, g + 16, ... in order,
// then a fixed butterfly over the 16 lanes: a row's result depends on that row alone, not on its block or chunk.
__global__ __launch_bounds__(256) void dx_kernel(const float* __restrict__ w0, int w, const float* __restrict__ dpre, long long ld,
                                                 long long n_valid, long long row0, float* __restrict__ gx) {
  const int g = threadIdx.x & 15;
  const long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);      // chunk row (every one is allocated)
  const float* drow = dpre + r * ld;
  f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int o = g; o < w; o += 16) {
    const float d = drow[o];
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(w0 + (long long)o * 8);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(w0 + (long long)o * 8 + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { s0[i] = fmaf(a0[i], d, s0[i]); s1[i] = fmaf(a1[i], d, s1[i]); }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) { s0[i] = sum16(s0[i]); s1[i] = sum16(s1[i]); }
  if (g == 0 && r < n_valid) {
    *reinterpret_cast<f32x4*>(gx + (row0 + r) * 8) = s0;
    *reinterpret_cast<f32x4*>(gx + (row0 + r) * 8 + 4) = s1;
  }
}

// acc (+)= sum_s slab[s], slices in order, fp64 within the chunk.  Member = the grid's y (slabs and acc are workspace)
__global__ __launch_bounds__(256) void reduce_kernel(const float* __restrict__ slabs, int slices, long long total, float* __restrict__ acc,
                                                     int first, long long mem_work) {
  slabs += (long long)blockIdx.y * mem_work;
  acc += (long long)blockIdx.y * mem_work;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    double s = 0.0;
    for (int q = 0; q < slices; ++q) s += (double)slabs[(long long)q * total + e];
    acc[e] = first ? (float)s : acc[e] + (float)s;
  }
}

// padded gradient regions -> flat gradient (state_dict layout, zero padding); block 0 also sums the loss partials in order (if any)
struct FinArgs {
  const float* acc; float* grads; long long total;
  int n_mat; long long woff[kMaxMat], boff[kMaxMat], reg[kMaxMat]; int out[kMaxMat], in[kMaxMat];
  const double* loss_part; long long n_parts; double* loss;
  Members mem;          // member = the grid's y: acc and loss_part are workspace, grads a parameter-shaped buffer, loss [n][kLossOut]
};
__global__ __launch_bounds__(256) void finalize_kernel(FinArgs a) {
  const long long wo = (long long)blockIdx.y * a.mem.work;
  const float* __restrict__ acc = a.acc + wo;
  float* __restrict__ grads = a.grads + (long long)blockIdx.y * a.mem.par;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < a.total; e += (long long)gridDim.x * 256) {
    float v = 0.0f;
    for (int t = 0; t < a.n_mat; ++t) {
      const long long nw = (long long)a.out[t] * a.in[t];
      if (e >= a.woff[t] && e < a.woff[t] + nw) {
        const long long q = e - a.woff[t], o = q / a.in[t], i = q - o * a.in[t];
        v = acc[a.reg[t] + o * (a.in[t] + 1) + i];
      } else if (e >= a.boff[t] && e < a.boff[t] + a.out[t]) {
        const long long o = e - a.boff[t];
        v = acc[a.reg[t] + o * (a.in[t] + 1) + a.in[t]];
      }
    }
    grads[e] = v;
  }
  if (blockIdx.x == 0 && a.loss_part) {
    __shared__ double red[256];
    for (int q = 0; q < kLossOut; ++q) {
      double s = 0.0;
      for (long long b = threadIdx.x; b < a.n_parts; b += 256) s += (a.loss_part + wo / 2)[b * kLossTerms + q];
      red[threadIdx.x] = s;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
      }
      if (threadIdx.x == 0) a.loss[(long long)blockIdx.y * kLossOut + q] = red[0];
      __syncthreads();
    }
  }
}

// MC-dropout moments: virtual row v = (pass + 1) * n_rows + row, pass -1 = eval.  Per row, passes in order (pinn_mc_dropout's
// arithmetic): state [4][n_rows] = u_eval, Welford mean and m2 of u - u_eval, sum of logvar
__global__ __launch_bounds__(256) void mc_moments_kernel(const float* __restrict__ ub, const float* __restrict__ lvb, long long v0,
                                                         long long nv, long long n_rows, float* __restrict__ st) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  long long q = v0 > r ? (v0 - r + n_rows - 1) / n_rows : 0;
  if (q * n_rows + r >= v0 + nv) return;
  float ue = st[r], mean = st[n_rows + r], m2 = st[2 * n_rows + r], sl = st[3 * n_rows + r];
  for (; q * n_rows + r < v0 + nv; ++q) {
    const long long c = q * n_rows + r - v0;
    if (q == 0) { ue = ub[c]; mean = 0.f; m2 = 0.f; sl = 0.f; continue; }
    welford_update(mean, m2, ub[c] - ue, 1.0f / (float)q);
    sl += lvb[c];
  }
  st[r] = ue; st[n_rows + r] = mean; st[2 * n_rows + r] = m2; st[3 * n_rows + r] = sl;
}
__global__ __launch_bounds__(256) void mc_final_kernel(const float* __restrict__ st, long long n_rows, int n_passes, float* o0, float* o1,
                                                       float* o2) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  o0[r] = st[r];
  mc_finish(st[2 * n_rows + r], st[3 * n_rows + r], n_passes, o1[r], o2[r]);
}

// deep-ensemble combine (pinn_gens_combine): one thread per row, members in index order, sums in double, each result rounded once.
// Every double operation is rounded on its own: with a fused multiply-add the variance of one member, or of equal members, would be
// the rounding error of u^2 instead of exactly 0
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ u, const float* __restrict__ lv, int n_members,
                                                      long long n_rows, int rule, float* __restrict__ pred_mean, float* __restrict__ a_u,
                                                      float* __restrict__ e_u) {
#pragma clang fp contract(off)
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  double su = 0.0, suu = 0.0, sl = 0.0;
  for (int m = 0; m < n_members; ++m) {
    const double um = (double)u[(long long)m * n_rows + r], lm = (double)lv[(long long)m * n_rows + r];
    su += um;
    suu += um * um;
    sl += rule ? exp(lm) : lm;
  }
  const double mean = su / n_members;
  double var = suu / n_members - mean * mean;
  if (!(var > 0.0)) var = 0.0;
  pred_mean[r] = (float)mean;
  e_u[r] = (float)sqrt(var);
  a_u[r] = (float)sqrt(rule ? sl / n_members : exp(sl / n_members));
}

// ---------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------
static inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static int last_error() { const hipError_t e = hipGetLastError(); return e == hipSuccess ? PINN_OK : (int)e; }

static int launch_pack(const Shape& s, const Members& mb, const float* params, float* pack, hipStream_t st) {
  PackArgs pa{};
  pa.params = params; pa.pack = pack; pa.mem = mb;
  int nj = 0;
  long long mx = 0;
  for (int t = 0; t < s.n_mat; ++t) {
    if (!s.is_gemm(t)) continue;
    pa.job[nj++] = PackJob{s.woff[t], s.pf[t], s.out[t], s.in[t], s.mp[t], s.kp[t], 0};
    if (s.pt[t] >= 0) pa.job[nj++] = PackJob{s.woff[t], s.pt[t], s.out[t], s.in[t], s.mp[t], s.kp[t], 1};
    const long long n = (long long)s.mp[t] * s.kp[t];
    if (n > mx) mx = n;
  }
  pa.n_jobs = nj;
  long long gx = (mx + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)gx, nj, mb.n), dim3(256), 0, st, pa);
  return last_error();
}


template <int MODE>
static void launch_gemm(const GemmArgs& g, bool paired, dim3 grid, hipStream_t st) {
  if (paired) hipLaunchKernelGGL((gemm_kernel<MODE, 2>), grid, dim3(256), 0, st, g);
  else hipLaunchKernelGGL((gemm_kernel<MODE, 1>), grid, dim3(256), 0, st, g);
}

// every GEMM layer of the forward pass for one chunk of (virtual) rows
struct ChunkIO {
  const float* in[kMaxMat]; long long ld_in[kMaxMat];
  float* out[kMaxMat]; long long ld_out[kMaxMat];
  const float* in2[kMaxMat]; float* out2[kMaxMat];      // the tangent stream of the double backward (same strides); NULL: none
  unsigned* keep;          // training: keep words written here
};

// training: matrix t reads the kept activation of the layer below it (matrix 0: the input rows, set per call) and keeps its own
static ChunkIO train_io(const Shape& s, float* const* act, float* const* tan, unsigned* keep) {
  ChunkIO io{};
  for (int t = 0; t < s.n_mat; ++t) {
    if (!s.is_gemm(t)) continue;
    const int src = t == 0 ? -1 : (t < s.k ? t - 1 : (t == s.mat_v0() ? s.k - 1 : s.mat_v0()));
    io.out[t] = act[t]; io.ld_out[t] = s.mp[t];
    io.in[t] = src < 0 ? nullptr : act[src]; io.ld_in[t] = src < 0 ? 8 : s.mp[src];
    if (tan) { io.out2[t] = tan[t]; io.in2[t] = src < 0 ? nullptr : tan[src]; }
  }
  io.keep = keep;
  return io;
}

static void forward_layers(const Shape& s, const Members& mb, const float* params, const float* pack, const Drop& d, const ChunkIO& io,
                           long long row0, long long nv, long long rows, long long n_rows, bool mc, hipStream_t st) {
  for (int step = 0; step < s.k + 2; ++step) {
    const int t = step < s.k ? step : (step == s.k ? s.mat_v0() : s.mat_v1());
    GemmArgs g{};
    g.A = pack + s.pf[t]; g.lda = s.kp[t]; g.a_mv = s.mp[t]; g.a_kv = s.kp[t];
    g.B = io.in[t]; g.B2 = io.in2[t]; g.ldb = io.ld_in[t]; g.b_mv = rows; g.b_kv = t == 0 ? 8 : s.kp[t];
    g.M = s.mp[t]; g.K = s.kp[t];
    g.out = io.out[t]; g.out2 = io.out2[t]; g.ldo = io.ld_out[t];
    g.n_valid = nv;
    g.bias = params + s.boff[t]; g.bias_n = s.out[t];
    g.module = t < s.k ? t : (t == s.mat_v0() ? s.k : -1);
    g.map_rows = t == 0;
    g.mc = mc ? 1 : 0;
    g.row0 = row0; g.n_rows = n_rows;
    g.drop = d;
    g.keep = io.keep;
    g.keep_off = g.module >= 0 ? s.word_off[g.module] : 0;
    g.stash_module = -1;
    g.mem = mb; g.b_shared = t == 0;        // matrix 0 reads the input rows
    launch_gemm<kFwd>(g, io.out2[t] != nullptr, dim3((unsigned)(rows / 64), (unsigned)((s.mp[t] + 63) / 64), mb.n), st);
  }
}

static HeadArgs head_args(const Shape& s, const Members& mb, const float* params, const float* h, long long ldh, const float* v2,
                          long long ldv, long long nv, long long row0) {
  HeadArgs h2{};
  h2.mem = mb;
  h2.h = h; h2.ldh = ldh; h2.hk = s.hk;
  h2.v2 = v2; h2.ldv = ldv; h2.hv2 = s.hv2;
  h2.wp = params + s.woff[s.mat_pred()]; h2.bp = params + s.boff[s.mat_pred()];
  h2.wv2 = params + s.woff[s.mat_v2()]; h2.bv2 = params + s.boff[s.mat_v2()];
  h2.n_valid = nv; h2.row0 = row0;
  return h2;
}

// forward (n_passes == 0) or MC-dropout (1 eval pass + n_passes stochastic passes as virtual rows)
// n_members > 1 (forward only): o0, o1 [n_members][n_rows] from parameters [n_members][total], the workspace n_members Layouts
static int run_infer(const Shape& s, int n_members, const float* d_params, const float* d_x, long long n_rows, const Drop& d, int n_passes,
                     float* o0, float* o1, float* o2, void* d_work, size_t work_bytes, hipStream_t st) {
  const bool mc = n_passes > 0;
  const Layout L = infer_layout(s, n_rows, n_passes);
  if (!d_work || !al16(d_work)) return PINN_E_ARG;
  if (work_bytes < L.end * (size_t)n_members) return PINN_E_WORKSPACE;
  const Members mb = {n_members, (long long)(L.end / 4), s.total, n_rows};
  char* base = (char*)d_work;
  const float* pack = (const float*)(base + L.pack);
  int rc = launch_pack(s, mb, d_params, (float*)(base + L.pack), st);
  if (rc) return rc;
  float* buf[3] = {(float*)(base + L.act[0][0]), (float*)(base + L.act[0][1]), (float*)(base + L.act[0][2])};
  ChunkIO io{};
  for (int t = 0; t < s.k; ++t) {       // hidden layer t writes buf[t & 1]; v0 the other one; v1 buf[2]
    io.in[t] = t == 0 ? d_x : buf[(t - 1) & 1];
    io.ld_in[t] = t == 0 ? 8 : s.max_wp;
    io.out[t] = buf[t & 1]; io.ld_out[t] = s.max_wp;
  }
  const int c = (s.k - 1) & 1;
  io.in[s.mat_v0()] = buf[c]; io.ld_in[s.mat_v0()] = s.max_wp; io.out[s.mat_v0()] = buf[c ^ 1]; io.ld_out[s.mat_v0()] = s.max_wp;
  io.in[s.mat_v1()] = buf[c ^ 1]; io.ld_in[s.mat_v1()] = s.max_wp; io.out[s.mat_v1()] = buf[2]; io.ld_out[s.mat_v1()] = s.max_wp;
  io.keep = nullptr;
  float* ub = (float*)(base + L.ubuf);
  float* lvb = (float*)(base + L.lvbuf);
  float* state = (float*)(base + L.state);
  const long long total = mc ? n_rows * ((long long)n_passes + 1) : n_rows;
  for (long long v0 = 0; v0 < total; v0 += L.rows) {
    const long long nv = total - v0 < L.rows ? total - v0 : L.rows;
    forward_layers(s, mb, d_params, pack, d, io, v0, nv, L.rows, n_rows, mc, st);
    HeadArgs h = head_args(s, mb, d_params, buf[c], s.max_wp, buf[2], s.max_wp, nv, v0);
    if (mc) {
      h.u = ub; h.lv = lvb;
      hipLaunchKernelGGL(heads_kernel<kHeadMC>, dim3((unsigned)(L.rows / 16)), dim3(256), 0, st, h);
      hipLaunchKernelGGL(mc_moments_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, ub, lvb, v0, nv, n_rows, state);
    } else {
      h.u = o0; h.lv = o1;
      hipLaunchKernelGGL(heads_kernel<kHeadFwd>, dim3((unsigned)(L.rows / 16), mb.n), dim3(256), 0, st, h);
    }
    rc = last_error();
    if (rc) return rc;
  }
  if (mc) hipLaunchKernelGGL(mc_final_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, state, n_rows, n_passes, o0, o1, o2);
  return last_error();
}

// weight gradient of matrix t, per slice.  Double backward: dpre = p with x_in = a, dpre2 = q with x_in2 = ad (same strides)
static void wgrad(const Shape& s, const Members& mb, int t, const Layout& L, const float* dpre, long long ld_dpre, const float* x_in, long long ld_in,
                  long long nv, float* slabs, hipStream_t st, const float* dpre2 = nullptr, const float* x_in2 = nullptr) {
  GemmArgs g{};
  g.A = dpre; g.A2 = dpre2; g.lda = ld_dpre; g.a_mv = s.mp[t]; g.a_kv = nv;
  g.B = x_in; g.B2 = x_in2; g.ldb = ld_in; g.b_mv = ld_in; g.b_kv = nv;
  g.K = L.rows;
  g.n_valid = nv;
  g.slice_rows = L.slice_rows; g.slab = slabs; g.slab_stride = s.gtotal; g.reg = s.reg[t];
  g.out_real = s.out[t]; g.in_real = s.in[t];
  g.module = -1; g.stash_module = -1;
  g.mem = mb; g.b_shared = t == 0;          // matrix 0's input is the input rows
  g.tiles_x = (unsigned)((s.in[t] + 1 + 63) / 64);
  const dim3 grid(g.tiles_x * (unsigned)mb.n, (unsigned)((s.out[t] + 63) / 64), (unsigned)L.slices);
  launch_gemm<kWgrad>(g, dpre2 != nullptr, grid, st);
}

// d pre-activation of the layer feeding matrix t: (W_t^T dpre_t (+ w_p du)) * tanh' * mask.  Double backward: (dpre, dpre2) = (p, q) of
// matrix t, (dpre_in, dpre_in2) = (p, q) of that layer, from its kept activation and tangent (stash, stash2); w_p du joins the q stream
static void bwd(const Shape& s, const Members& mb, int t, const Layout& L, const float* pack, const Drop& d, const float* dpre, float* dpre_in,
                const float* stash, long long ld_stash, int module, const unsigned* keep, const float* wp, const float* du, long long nv,
                hipStream_t st, const float* dpre2 = nullptr, float* dpre_in2 = nullptr, const float* stash2 = nullptr) {
  GemmArgs g{};
  g.A = pack + s.pt[t]; g.lda = s.mp[t]; g.a_mv = s.kp[t]; g.a_kv = s.mp[t];
  g.B = dpre; g.B2 = dpre2; g.ldb = s.max_wp; g.b_mv = L.rows; g.b_kv = s.mp[t];
  g.M = s.kp[t]; g.K = s.mp[t];
  g.out = dpre_in; g.out2 = dpre_in2; g.ldo = s.max_wp;
  g.n_valid = nv;
  g.drop = d;
  g.module = -1;
  g.stash = stash; g.stash2 = stash2; g.ld_stash = ld_stash; g.stash_module = module;
  g.keep_in = keep; g.keep_off = s.word_off[module];
  g.wp = wp; g.du = du; g.wp_n = wp ? s.hk : 0;
  g.mem = mb;
  launch_gemm<kBwd>(g, dpre2 != nullptr, dim3((unsigned)(L.rows / 64), (unsigned)((s.kp[t] + 63) / 64), mb.n), st);
}

// acc (+)= the chunk's slab sums
static void launch_reduce(const Shape& s, const Members& mb, const Layout& L, const float* slabs, float* acc, bool first, hipStream_t st) {
  long long gx = (s.gtotal + 255) / 256;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)gx, mb.n), dim3(256), 0, st, slabs, L.slices, s.gtotal, acc, first ? 1 : 0, mb.work);
}

// acc -> the flat gradient; loss_part != NULL: also the loss sums of its n_parts partials
static void launch_finalize(const Shape& s, const Members& mb, const float* acc, float* grads, const double* loss_part, long long n_parts, double* loss,
                            hipStream_t st) {
  FinArgs f{};
  f.acc = acc; f.grads = grads; f.total = s.total; f.n_mat = s.n_mat;
  for (int t = 0; t < s.n_mat; ++t) { f.woff[t] = s.woff[t]; f.boff[t] = s.boff[t]; f.reg[t] = s.reg[t]; f.out[t] = s.out[t]; f.in[t] = s.in[t]; }
  f.loss_part = loss_part; f.n_parts = n_parts; f.loss = loss; f.mem = mb;
  long long gx = (s.total + 255) / 256;
  if (gx > 4096) gx = 4096;
  hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)gx, mb.n), dim3(256), 0, st, f);
}

// ---------------------------------------------------------------------------------------
// double backward (pinn_gnet_backward2): the gradient of S = <v, dL/dx> with respect to g_u, g_lv, x and the parameters.
//
// Every matrix product has one weight operand for two activation streams, so each layer is one launch of gemm_kernel<., 2>:
//   gemm_kernel<kFwd, 2>   [z ; zd] = W [a_in ; ad_in];  h = tanh z, a = c h, ad = c (1 - h^2) zd   (primal a bitwise gemm_kernel<kFwd, 1>'s)
//   gemm_kernel<kBwd, 2>   [abar ; adbar] = W^T [p ; q] (+ w_p g_u on adbar);  q_in = c (1 - h^2) adbar (bitwise the first backward's
//                          dpre), p_in = c (1 - h^2) abar - 2 h adbar ad
//   gemm_kernel<kWgrad, 2> slab[s][o][i] = sum_{r in slice s} p[r][o] a[r][i] + q[r][o] ad[r][i]; the bias column sums p alone
//   head2_kernel           z, zd, f', f'', ud, lvd; q_v2, p_v2; the (p, q) pair below the variance head's second tanh
//   vec_grad2_kernel       the two one-row tensors per slice: w_p (g_u^T ad_k, bias 0), w_v2 (q_v2^T ad_v1 + p_v2^T a_v1, bias sum p_v2)
// dS/dx = W_0^T p_0 is dx_kernel on p_0; slab sums and the flat gradient are reduce_kernel / finalize_kernel.
// ---------------------------------------------------------------------------------------
// per row (16 lanes): z, zd, f'(z), f''(z); ud = w_p . ad_k, lvd = f' zd (the gradients of S with respect to g_u, g_lv);
// q_v2 = g_lv f', p_v2 = g_lv f'' zd, and the (p, q) pair below the variance head's second tanh (no dropout there: c = 1)
struct Head2Args {
  const float* hd; long long ldh; int hk;                   // tangent of the last hidden activation
  const float* v2; const float* v2d; long long ldv; int hv2;
  const float* wp; const float* wv2; const float* bv2;
  long long n_valid, row0;
  const float* gu; const float* glv;
  float* ggu; float* gglv;                                  // outputs at row0 + r (NULL: not written)
  float* du; float* qz; float* pz;                          // chunk buffers: g_u, q_v2, p_v2
  float* dp; float* dq; long long ld_dpre; int wd;
};
__global__ __launch_bounds__(256) void head2_kernel(Head2Args a) {
  const int g = threadIdx.x & 15;
  const long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
  const float* hrow = a.hd + r * a.ldh;
  const float* vrow = a.v2 + r * a.ldv;
  const float* vdrow = a.v2d + r * a.ldv;
  float su = 0.f, sz = 0.f, sd = 0.f;
  for (int f = g; f < a.hk; f += 16) su = fmaf(a.wp[f], hrow[f], su);
  for (int f = g; f < a.hv2; f += 16) { sz = fmaf(a.wv2[f], vrow[f], sz); sd = fmaf(a.wv2[f], vdrow[f], sd); }
  const float ud = sum16(su);
  const float z = sum16(sz) + a.bv2[0];
  const float zd = sum16(sd);
  const bool valid = r < a.n_valid;
  float du = 0.f, qz = 0.f, pz = 0.f;
  if (valid) {
    const float var = var_of(z);
    const float sig = softplus_slope(z);
    const float f1 = sig / var;
    const float f2 = sig * (1.0f - sig) / var - f1 * f1;
    du = a.gu[a.row0 + r];
    if (a.glv) {
      const float glv = a.glv[a.row0 + r];
      qz = through_logvar(glv, sig, var);   // pinn_gnet_backward's dz
      pz = glv * f2 * zd;
    }
    if (g == 0) {
      if (a.ggu) a.ggu[a.row0 + r] = ud;
      if (a.gglv) a.gglv[a.row0 + r] = f1 * zd;
    }
  }
  if (g == 0) { a.du[r] = du; a.qz[r] = qz; a.pz[r] = pz; }
  float* prow = a.dp + r * a.ld_dpre;
  float* qrow = a.dq + r * a.ld_dpre;
  for (int f = g; f < a.wd; f += 16) {
    float vp = 0.f, vq = 0.f;
    if (f < a.hv2 && valid) {
      const float v = vrow[f], w = a.wv2[f];
      vq = w * qz * (1.0f - v * v);
      vp = (w * pz) * (1.0f - v * v) - 2.0f * v * (w * qz) * vdrow[f];
    }
    prow[f] = vp;
    qrow[f] = vq;
  }
}

struct Vec2Args {
  const float* hd; long long ldh; int hk;
  const float* v2; const float* v2d; long long ldv; int hv2;
  const float* du; const float* qz; const float* pz;
  long long K, slice_rows;
  float* slab; long long slab_stride, reg_p, reg_v2;
};
__global__ __launch_bounds__(256) void vec_grad2_kernel(Vec2Args a) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  const long long r0 = (long long)blockIdx.x * a.slice_rows;
  long long r1 = r0 + a.slice_rows;
  if (r1 > a.K) r1 = a.K;
  float* dst = a.slab + (long long)blockIdx.x * a.slab_stride;
  if (c <= a.hk) {
    float s = 0.f;
    if (c < a.hk)
      for (long long r = r0; r < r1; ++r) s = fmaf(a.du[r], a.hd[r * a.ldh + c], s);
    dst[a.reg_p + c] = s;                  // c == hk: dS/db_p = 0 exactly
  } else if (c - (a.hk + 1) <= a.hv2) {
    const int j = c - (a.hk + 1);
    float s = 0.f;
    for (long long r = r0; r < r1; ++r) {
      if (j < a.hv2) s = fmaf(a.pz[r], a.v2[r * a.ldv + j], fmaf(a.qz[r], a.v2d[r * a.ldv + j], s));
      else s += a.pz[r];
    }
    dst[a.reg_v2 + j] = s;
  }
}

// One call of pinn_gnet_train_grads / _train_step, pinn_gnet_backward or pinn_gnet_backward2.  Upstream: gu == NULL: aleatoric_loss on
// (x, y), gradients divided by n_global, loss sums -> loss; otherwise the given dL/du and dL/dlogvar per row (glv NULL: zero), raw sums,
// no loss.  vx != NULL: the second stream of the double backward (the section above), with ggu / gglv (each NULL: not written).
// grads NULL: no weight gradient; gx NULL: no dL/dx (dS/dx)
struct GradCall {
  const float* y; long long n_global;
  const float* gu; const float* glv;
  const float* vx; float* ggu; float* gglv;
  float* grads; float* gx; double* loss;
};

// the workspace of a chunk.  tan, dq, pz: the second stream's (NULL with one stream); loss_part: one stream only
struct ChunkBufs {
  float* act[kMaxMat]; float* tan[kMaxMat]; unsigned* keep;
  float* dp[2]; float* dq[2]; float* du; float* dz; float* pz; float* slabs; float* acc; double* loss_part;
};

// heads of a chunk: du, dz (, pz) per row and the d pre-activation(s) below the variance head's second tanh, in dp[0] (, dq[0])
static void launch_heads(const Shape& s, const Members& mb, const Layout& L, const float* params, const GradCall& c, const ChunkBufs& w, long long nv,
                         long long row0, hipStream_t st) {
  const int v1m = s.mat_v1();
  const dim3 grid((unsigned)(L.rows / 16)), blk(256);
  if (c.vx) {
    Head2Args h{};
    h.hd = w.tan[s.k - 1]; h.ldh = s.mp[s.k - 1]; h.hk = s.hk;
    h.v2 = w.act[v1m]; h.v2d = w.tan[v1m]; h.ldv = s.mp[v1m]; h.hv2 = s.hv2;
    h.wp = params + s.woff[s.mat_pred()]; h.wv2 = params + s.woff[s.mat_v2()]; h.bv2 = params + s.boff[s.mat_v2()];
    h.n_valid = nv; h.row0 = row0;
    h.gu = c.gu; h.glv = c.glv; h.ggu = c.ggu; h.gglv = c.gglv;
    h.du = w.du; h.qz = w.dz; h.pz = w.pz; h.dp = w.dp[0]; h.dq = w.dq[0]; h.ld_dpre = s.max_wp; h.wd = s.mp[v1m];
    hipLaunchKernelGGL(head2_kernel, grid, blk, 0, st, h);
    return;
  }
  HeadArgs h = head_args(s, mb, params, w.act[s.k - 1], s.mp[s.k - 1], w.act[v1m], s.mp[v1m], nv, row0);
  h.y = c.y; h.n_global = c.n_global; h.gu = c.gu; h.glv = c.glv;
  h.du = w.du; h.dz = w.dz; h.dpre_v2 = w.dp[0]; h.ld_dpre = s.max_wp; h.wd = s.mp[v1m];
  h.loss_part = w.loss_part;
  if (c.gu) hipLaunchKernelGGL(heads_kernel<kHeadGrad>, grid, blk, 0, st, h);
  else hipLaunchKernelGGL(heads_kernel<kHeadTrain>, dim3(grid.x, mb.n), blk, 0, st, h);
}

// the two one-row tensors (predict, last variance layer) of a chunk, per slice
static void launch_vec_grad(const Shape& s, const Members& mb, const Layout& L, const ChunkBufs& w, bool paired, hipStream_t st) {
  const int v1m = s.mat_v1(), cols = s.hk + 1 + s.hv2 + 1;
  const dim3 grid((unsigned)L.slices, (unsigned)((cols + 255) / 256)), blk(256);
  if (paired) {
    Vec2Args va{};
    va.hd = w.tan[s.k - 1]; va.ldh = s.mp[s.k - 1]; va.hk = s.hk;
    va.v2 = w.act[v1m]; va.v2d = w.tan[v1m]; va.ldv = s.mp[v1m]; va.hv2 = s.hv2;
    va.du = w.du; va.qz = w.dz; va.pz = w.pz; va.K = L.rows; va.slice_rows = L.slice_rows;
    va.slab = w.slabs; va.slab_stride = s.gtotal; va.reg_p = s.reg[s.mat_pred()]; va.reg_v2 = s.reg[s.mat_v2()];
    hipLaunchKernelGGL(vec_grad2_kernel, grid, blk, 0, st, va);
  } else {
    VecArgs va{};
    va.h = w.act[s.k - 1]; va.ldh = s.mp[s.k - 1]; va.hk = s.hk;
    va.v2 = w.act[v1m]; va.ldv = s.mp[v1m]; va.hv2 = s.hv2;
    va.du = w.du; va.dz = w.dz; va.K = L.rows; va.slice_rows = L.slice_rows;
    va.slab = w.slabs; va.slab_stride = s.gtotal; va.reg_p = s.reg[s.mat_pred()]; va.reg_v2 = s.reg[s.mat_v2()];
    va.mem = mb;
    hipLaunchKernelGGL(vec_grad_kernel, dim3(grid.x, grid.y, mb.n), blk, 0, st, va);
  }
}

// recomputing forward + backward of every chunk, fixed-order slab sums -> c.grads.  With one stream tan[..], dq[..] and vx are NULL, and
// the optional arguments of train_io / wgrad / bwd select the single-stream kernels
// n_members > 1 (one stream, the loss upstream): parameters, c.grads [n_members][total], c.loss [n_members][4], the workspace n_members Layouts
static int run_grads(const Shape& s, int n_members, const float* d_params, const float* d_x, long long n_rows, const pinn_dropout_t* drop,
                     const GradCall& c, void* d_work, size_t work_bytes, hipStream_t st) {
  Drop d;
  int rc = convert(s, drop, &d);
  if (rc) return rc;
  (void)hipGetLastError();
  const bool two = c.vx != nullptr;
  const Layout L = train_layout(s, n_rows, two ? 2 : 1);
  if (!d_work || !al16(d_work)) return PINN_E_ARG;
  if (work_bytes < L.end * (size_t)n_members) return PINN_E_WORKSPACE;
  const Members mb = {n_members, (long long)(L.end / 4), s.total, n_rows};
  char* base = (char*)d_work;
  const float* pack = (const float*)(base + L.pack);
  rc = launch_pack(s, mb, d_params, (float*)(base + L.pack), st);
  if (rc) return rc;
  auto f32 = [&](size_t off, bool have = true) { return have ? (float*)(base + off) : nullptr; };
  ChunkBufs w{};
  for (int t = 0; t < s.n_mat; ++t)
    if (s.is_gemm(t)) { w.act[t] = f32(L.act[0][act_index(s, t)]); w.tan[t] = f32(L.act[1][act_index(s, t)], two); }
  w.keep = (unsigned*)(base + L.keep);
  for (int b = 0; b < 2; ++b) { w.dp[b] = f32(L.dpre[0][b]); w.dq[b] = f32(L.dpre[1][b], two); }
  w.du = f32(L.du); w.dz = f32(L.dz); w.pz = f32(L.pz, two);
  w.slabs = f32(L.slabs); w.acc = f32(L.acc);
  w.loss_part = two ? nullptr : (double*)(base + L.loss);
  float* const* act = w.act; float* const* tan = w.tan; float* const* dp = w.dp; float* const* dq = w.dq;
  ChunkIO io = train_io(s, act, tan, w.keep);
  io.in[0] = d_x; io.in2[0] = c.vx;
  const int v0m = s.mat_v0(), v1m = s.mat_v1();
  const bool want_w = c.grads != nullptr, want_back = want_w || c.gx;
  const long long nch = n_chunks(n_rows, L.rows);
  for (long long ch = 0; ch < nch; ++ch) {
    const long long row0 = ch * L.rows;
    const long long nv = n_rows - row0 < L.rows ? n_rows - row0 : L.rows;
    const float* x = d_x + row0 * 8;
    const float* vx = c.vx ? c.vx + row0 * 8 : nullptr;
    forward_layers(s, mb, d_params, pack, d, io, row0, nv, L.rows, n_rows, false, st);      // primal (and tangent)
    launch_heads(s, mb, L, d_params, c, w, nv, row0, st);
    if (want_back) {
      // variance head layer 1, then layer 0 (+ the predict head; on the q stream of two), then the hidden layers top-down
      if (want_w) wgrad(s, mb, v1m, L, dp[0], s.max_wp, act[v0m], s.mp[v0m], nv, w.slabs, st, dq[0], tan[v0m]);
      bwd(s, mb, v1m, L, pack, d, dp[0], dp[1], act[v0m], s.mp[v0m], s.k, w.keep, nullptr, nullptr, nv, st, dq[0], dq[1], tan[v0m]);
      if (want_w) {
        wgrad(s, mb, v0m, L, dp[1], s.max_wp, act[s.k - 1], s.mp[s.k - 1], nv, w.slabs, st, dq[1], tan[s.k - 1]);
        launch_vec_grad(s, mb, L, w, two, st);
      }
      bwd(s, mb, v0m, L, pack, d, dp[1], dp[0], act[s.k - 1], s.mp[s.k - 1], s.k - 1, w.keep, d_params + s.woff[s.mat_pred()], w.du, nv, st,
          dq[1], dq[0], tan[s.k - 1]);
      int cur = 0;
      for (int l = s.k - 1; l >= 0; --l) {
        if (want_w) {
          if (l == 0) wgrad(s, mb, 0, L, dp[cur], s.max_wp, x, 8, nv, w.slabs, st, dq[cur], vx);
          else wgrad(s, mb, l, L, dp[cur], s.max_wp, act[l - 1], s.mp[l - 1], nv, w.slabs, st, dq[cur], tan[l - 1]);
        }
        if (l > 0) {
          bwd(s, mb, l, L, pack, d, dp[cur], dp[cur ^ 1], act[l - 1], s.mp[l - 1], l - 1, w.keep, nullptr, nullptr, nv, st, dq[cur], dq[cur ^ 1],
              tan[l - 1]);
          cur ^= 1;
        }
      }
      if (c.gx)        // dp[cur] is now d pre-activation of hidden layer 0 (two streams: p_0, dS/dx = W_0^T p_0)
        hipLaunchKernelGGL(dx_kernel, dim3((unsigned)(L.rows / 16)), dim3(256), 0, st, d_params + s.woff[0], s.w[0], (const float*)dp[cur],
                           (long long)s.max_wp, nv, row0, c.gx);
      if (want_w) launch_reduce(s, mb, L, w.slabs, w.acc, ch == 0, st);
    }
    rc = last_error();
    if (rc) return rc;
  }
  if (want_w) launch_finalize(s, mb, w.acc, c.grads, c.gu ? nullptr : w.loss_part, w.loss_part ? nch * (L.rows / 16) : 0, c.loss, st);
  return last_error();
}

}  // namespace gen
}  // namespace pinn

using namespace pinn::gen;

extern "C" long long pinn_gnet_param_count(const pinn_gnet_t* net) {
  Shape s;
  const int rc = make_shape(net, &s);
  return rc ? rc : s.total;
}

extern "C" size_t pinn_gnet_workspace_bytes(const pinn_gnet_t* net, long long n_rows, int n_passes) {
  Shape s;
  if (make_shape(net, &s) || n_rows < 0 || n_passes < 0) return 0;
  const size_t a = train_layout(s, n_rows, 1).end, b = infer_layout(s, n_rows, n_passes).end;
  return a > b ? a : b;
}

extern "C" int pinn_gnet_forward(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows, const pinn_dropout_t* drop,
                                 float* d_u, float* d_logvar, void* d_work, size_t work_bytes, void* stream) {
  Shape s;
  int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_rows < 0 || !d_params || !al16(d_params)) return PINN_E_ARG;
  if (n_rows == 0) return PINN_OK;
  if (!d_x || !al16(d_x) || !d_u || !d_logvar) return PINN_E_ARG;
  Drop d;
  rc = convert(s, drop, &d);
  if (rc) return rc;
  (void)hipGetLastError();
  return run_infer(s, 1, d_params, d_x, n_rows, d, 0, d_u, d_logvar, nullptr, d_work, work_bytes, (hipStream_t)stream);
}

extern "C" int pinn_gnet_mc_dropout(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows, const pinn_dropout_t* drop,
                                    int n_passes, float* d_pred_mean, float* d_a_u, float* d_e_u, void* d_work, size_t work_bytes,
                                    void* stream) {
  Shape s;
  int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_rows < 0 || !d_params || !al16(d_params) || n_passes < 1 || !drop) return PINN_E_ARG;
  if (n_rows == 0) return PINN_OK;
  if (!d_x || !al16(d_x) || !d_pred_mean || !d_a_u || !d_e_u) return PINN_E_ARG;
  if (drop->mode == PINN_DROP_NONE) return PINN_E_ARG;
  Drop d;
  rc = convert(s, drop, &d);
  if (rc) return rc;
  (void)hipGetLastError();
  return run_infer(s, 1, d_params, d_x, n_rows, d, n_passes, d_pred_mean, d_a_u, d_e_u, d_work, work_bytes, (hipStream_t)stream);
}

extern "C" int pinn_gnet_train_grads(const pinn_gnet_t* net, const float* d_params, const float* d_x, const float* d_y, long long n_rows,
                                     long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss, void* d_work,
                                     size_t work_bytes, void* stream) {
  Shape s;
  int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_rows < 0 || n_global < 1 || n_global < n_rows || !d_params || !al16(d_params) || !d_grads || !al16(d_grads) || !d_loss)
    return PINN_E_ARG;
  if (n_rows == 0) return PINN_OK;
  if (!d_x || !al16(d_x) || !d_y) return PINN_E_ARG;
  GradCall c{};
  c.y = d_y; c.n_global = n_global; c.grads = d_grads; c.loss = d_loss;
  return run_grads(s, 1, d_params, d_x, n_rows, drop, c, d_work, work_bytes, (hipStream_t)stream);
}

extern "C" int pinn_gnet_train_step(const pinn_gnet_t* net, float* d_params, const float* d_x, const float* d_y, long long n_rows,
                                    long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss, void* d_work,
                                    size_t work_bytes, float* d_m, float* d_v, float lr, int step, void* stream) {
  if (!d_m || !d_v || step < 1) return PINN_E_ARG;
  int rc = pinn_gnet_train_grads(net, d_params, d_x, d_y, n_rows, n_global, drop, d_grads, d_loss, d_work, work_bytes, stream);
  if (rc) return rc;
  const long long n = pinn_gnet_param_count(net);
  return pinn_adam_step(d_params, d_grads, d_m, d_v, n, lr, step, stream);
}

extern "C" int pinn_gnet_backward(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows,
                                  const pinn_dropout_t* drop, const float* d_gu, const float* d_glv, float* d_grads, float* d_gx,
                                  void* d_work, size_t work_bytes, void* stream) {
  Shape s;
  int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_rows < 0 || !d_params || !al16(d_params) || !d_grads || !al16(d_grads)) return PINN_E_ARG;
  if (n_rows == 0) return PINN_OK;
  if (!d_x || !al16(d_x) || !d_gu || (d_gx && !al16(d_gx))) return PINN_E_ARG;
  GradCall c{};
  c.n_global = n_rows; c.gu = d_gu; c.glv = d_glv; c.grads = d_grads; c.gx = d_gx;
  return run_grads(s, 1, d_params, d_x, n_rows, drop, c, d_work, work_bytes, (hipStream_t)stream);
}

extern "C" size_t pinn_gnet_backward2_workspace_bytes(const pinn_gnet_t* net, long long n_rows) {
  Shape s;
  if (make_shape(net, &s) || n_rows < 0) return 0;
  return train_layout(s, n_rows, 2).end;
}

extern "C" int pinn_gnet_backward2(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows,
                                   const pinn_dropout_t* drop, const float* d_gu, const float* d_glv, const float* d_vx, float* d_grads,
                                   float* d_gx, float* d_ggu, float* d_gglv, void* d_work, size_t work_bytes, void* stream) {
  Shape s;
  int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_rows < 0 || !d_params || !al16(d_params) || (d_grads && !al16(d_grads))) return PINN_E_ARG;
  if (n_rows == 0) {
    if (!d_grads) return PINN_OK;
    (void)hipGetLastError();
    const hipError_t e = hipMemsetAsync(d_grads, 0, sizeof(float) * (size_t)s.total, (hipStream_t)stream);
    return e == hipSuccess ? PINN_OK : (int)e;
  }
  if (!d_x || !al16(d_x) || !d_gu || !d_vx || !al16(d_vx) || (d_gx && !al16(d_gx))) return PINN_E_ARG;
  GradCall c{};
  c.gu = d_gu; c.glv = d_glv; c.vx = d_vx; c.ggu = d_ggu; c.gglv = d_gglv; c.grads = d_grads; c.gx = d_gx;
  return run_grads(s, 1, d_params, d_x, n_rows, drop, c, d_work, work_bytes, (hipStream_t)stream);
}

// ---- deep ensembles: n_members equal networks in the launches of one (the member dimension above) ------------------------------
constexpr int kMaxMembers = 32;

// the dropout modes a batched call takes: eval (NULL or PINN_DROP_NONE) and Philox; convert() rejects the rest of a bad struct
static bool gens_drop_ok(const pinn_dropout_t* drop) { return !drop || drop->mode != PINN_DROP_BITS; }

extern "C" size_t pinn_gens_workspace_bytes(const pinn_gnet_t* net, int n_members, long long n_rows) {
  Shape s;
  if (make_shape(net, &s) || n_members < 1 || n_members > kMaxMembers || n_rows < 0) return 0;
  const size_t a = train_layout(s, n_rows, 1).end, b = infer_layout(s, n_rows, 0).end;
  return (a > b ? a : b) * (size_t)n_members;
}

extern "C" int pinn_gens_train_plan(const pinn_gnet_t* net, long long n_rows, long long* chunk_rows, int* slices) {
  Shape s;
  const int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_rows < 0 || !chunk_rows || !slices) return PINN_E_ARG;
  const Layout L = train_layout(s, n_rows, 1);
  *chunk_rows = L.rows;
  *slices = L.slices;
  return PINN_OK;
}

extern "C" int pinn_gens_forward(const pinn_gnet_t* net, int n_members, const float* d_params, const float* d_x, long long n_rows,
                                 const pinn_dropout_t* drop, float* d_u, float* d_logvar, void* d_work, size_t work_bytes, void* stream) {
  Shape s;
  int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_members < 1 || n_members > kMaxMembers || n_rows < 0 || !d_params || !al16(d_params) || !gens_drop_ok(drop)) return PINN_E_ARG;
  Drop d;
  rc = convert(s, drop, &d);
  if (rc) return rc;
  if (n_rows == 0) return PINN_OK;
  if (!d_x || !al16(d_x) || !d_u || !d_logvar) return PINN_E_ARG;
  (void)hipGetLastError();
  return run_infer(s, n_members, d_params, d_x, n_rows, d, 0, d_u, d_logvar, nullptr, d_work, work_bytes, (hipStream_t)stream);
}

extern "C" int pinn_gens_train_grads(const pinn_gnet_t* net, int n_members, const float* d_params, const float* d_x, const float* d_y,
                                     long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss,
                                     void* d_work, size_t work_bytes, void* stream) {
  Shape s;
  int rc = make_shape(net, &s);
  if (rc) return rc;
  if (n_members < 1 || n_members > kMaxMembers || n_rows < 0 || n_global < 1 || n_global < n_rows || !d_params || !al16(d_params) ||
      !d_grads || !al16(d_grads) || !d_loss || !gens_drop_ok(drop))
    return PINN_E_ARG;
  Drop d;
  rc = convert(s, drop, &d);          // (run_grads converts again: a bad struct is refused before the n_rows == 0 return as well)
  if (rc) return rc;
  if (n_rows == 0) return PINN_OK;
  if (!d_x || !al16(d_x) || !d_y) return PINN_E_ARG;
  GradCall c{};
  c.y = d_y; c.n_global = n_global; c.grads = d_grads; c.loss = d_loss;
  return run_grads(s, n_members, d_params, d_x, n_rows, drop, c, d_work, work_bytes, (hipStream_t)stream);
}

extern "C" int pinn_gens_train_step(const pinn_gnet_t* net, int n_members, float* d_params, const float* d_x, const float* d_y,
                                    long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss,
                                    void* d_work, size_t work_bytes, float* d_m, float* d_v, float lr, int step, void* stream) {
  if (!d_m || !d_v || step < 1) return PINN_E_ARG;
  int rc = pinn_gens_train_grads(net, n_members, d_params, d_x, d_y, n_rows, n_global, drop, d_grads, d_loss, d_work, work_bytes, stream);
  if (rc || n_rows == 0) return rc;          // no rows: no gradient was written, so there is no step to take
  return pinn_adam_step(d_params, d_grads, d_m, d_v, (long long)n_members * pinn_gnet_param_count(net), lr, step, stream);
}

extern "C" int pinn_gens_combine(const float* d_u, const float* d_logvar, int n_members, long long n_rows, int rule, float* d_pred_mean,
                                 float* d_a_u, float* d_e_u, void* stream) {
  if (n_members < 1 || n_members > kMaxMembers || n_rows < 0 || rule < 0 || rule > 1) return PINN_E_ARG;
  if (n_rows == 0) return PINN_OK;
  if (!d_u || !d_logvar || !d_pred_mean || !d_a_u || !d_e_u) return PINN_E_ARG;
  (void)hipGetLastError();
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_u, d_logvar, n_members,
                     n_rows, rule, d_pred_mean, d_a_u, d_e_u);
  return last_error();
}
