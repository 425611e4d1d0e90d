// pinn_train.hip -- train_dnn's forward + aleatoric_loss + backward (01:949-953) for gfx950.
//
// Three kinds of kernel per step, all exact fp32 on the matrix cores:
//   K4/K5 train_chain_kernel : per 16-row wave tile, forward chain (activations in registers,
//        post-dropout activations + keep bits stashed to HBM as [tile16][feature][16]), NLL loss
//        and its gradient, backward (dgrad) chain; writes every layer's d(pre-activation) in the
//        same tiled layout.  v_mfma_f32_16x16x4_f32, two workgroups per CU.
//   K6 wgrad_kernel : dW = dpre^T . h_prev as a split-K GEMM over row tiles (K = rows), operands
//        read straight from the tiled stash as v_mfma_f32_32x32x2_f32 fragments (8 contiguous
//        floats per lane and tile), fp32 partial slabs per K-slice; bias / vector-head gradients
//        ride along as per-lane sums.  What the kernels of this family share is in pinn_wgrad_core.h
//        (device) and pinn_wgrad_args.h (arguments, tiling table, the step's problem list).
//   grad_finalize_kernel : fixed-order sum of the slabs -> flat gradient (bitwise reproducible,
//        no float atomics), already divided by the GLOBAL row count (data-parallel shards
//        all-reduce it with SUM).
#include <cstdlib>
#include "pinn_mlp_core.h"
#include "pinn_wgrad_core.h"
#include "pinn_adam_update.h"

namespace pinn {

constexpr int kMaxSlices = 256;

struct TrainArgs {
  const float* params;
  const float* x;
  const float* y;
  long long n_rows, n_global;
  int H, nh;
  DropDev drop;
  float* stash_h;    // [nh][T16][H][16]    post-dropout activations of hidden layers
  float* stash_v1;   // [T16][H/2][16]
  float* stash_v2;   // [T16][H/4][16]
  float* dpre_h;     // [nh][T16][H][16]    d loss / d pre-activation
  float* dpre_v1;
  float* dpre_v2;
  unsigned char* keep;   // [T16][nh*H/32 + H/64][64]  keep bits of every dropout module
  float* du;         // [T16*16]  d loss / d u      (already / n_global)
  float* dz;         // [T16*16]  d loss / d z
  double* loss_part; // [grid][kLossTerms]
  long long t16;     // 16-row tiles (padded to whole 64-row workgroup tiles)
};

// dpre = dh * scale * keep * (1 - a^2),  a = h / scale  (h = post-dropout activation), for blocks 2fp, 2fp+1
__device__ __forceinline__ void tanh_drop_backward_pair(f32x4& d0, f32x4& d1, const f32x4& h0, const f32x4& h1, unsigned keep,
                                                        float scale, float inv_scale) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float a0 = h0[r] * inv_scale, a1 = h1[r] * inv_scale;
    const float g0 = d0[r] * (scale * (1.0f - a0 * a0));
    const float g1 = d1[r] * (scale * (1.0f - a1 * a1));
    d0[r] = ((keep >> r) & 1u) ? g0 : 0.0f;
    d1[r] = ((keep >> (4 + r)) & 1u) ? g1 : 0.0f;
  }
}

template <int H, bool kBits>
__global__ __launch_bounds__(kThreads, 2) void train_chain_kernel(TrainArgs a) {
  constexpr int NT = H / 16, NT2 = H / 32, NT4 = H / 64, NP = H / 32;
  __shared__ __attribute__((aligned(16))) char lds_w[2 * kChunkBytes];
  __shared__ ChunkDesc tab[kMaxChunks];
  __shared__ double red[4][kLossTerms];
  __shared__ __attribute__((aligned(16))) float small[kMaxSmall];
  ParamLayout L{a.H, a.nh};
  const SmallLayout S{a.H, a.nh};
  const int n_fwd = (a.nh - 1) * NP + NP + NP / 2;
  const int n_bwd = H / 128 + H / 64 + (a.nh - 1) * NP;
  if (threadIdx.x == 0) {
    int k = build_forward_chunks(tab, L, 0);
    build_backward_chunks(tab, L, k);
  }
  load_small_params(small, a.params, L);
  Pipe pipe;
  pipe.params = a.params; pipe.tab = tab; pipe.lds = lds_w; pipe.n = n_fwd + n_bwd;
  pipe.prime();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kq = lane >> 4;
  const float* __restrict__ P = a.params;
  const bool drop = a.drop.mode != PINN_DROP_NONE;
  const float inv_n = (float)(1.0 / (double)a.n_global);
  const int n_groups = L.nh * NP + NP / 2;
  LossSums sums;

  const long long n_tiles = (a.n_rows + kTileRows - 1) / kTileRows;
  const unsigned pass0 = train_pass(a.drop);      // 0, or the device's step counter (replayed graphs)
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long long t16 = tile * 4 + wave;
    const long long lrow = t16 * 16 + (lane & 15);
    const bool valid = lrow < a.n_rows;
    const long long srow = valid ? lrow : a.n_rows - 1;
    const f32x4 xa = reinterpret_cast<const f32x4*>(a.x)[srow * 2];
    const f32x4 xb = reinterpret_cast<const f32x4*>(a.x)[srow * 2 + 1];
    const float yv = a.y[srow];
    const RowCtx c{lane, kq, a.drop.row_offset + lrow, srow, a.n_rows, pass0, a.drop.mode};
    const StashPtrs st{a.stash_h, a.stash_v1, a.stash_v2, a.keep, a.t16, t16};
    const unsigned char* keep = a.keep + (t16 * n_groups) * 64 + lane;

    // ------------------------------------------------------------------ forward (stash + keep bits written)
    float u, z;
    f32x4 v2[NT4];
    forward_pass<H, true, kBits>(P, small, L, pipe, a.drop, c, xa, xb, st, u, z, v2);

    // ------------------------------------------------------------------ aleatoric_loss (01:916-927) and its gradient
    float du, dz;
    loss_row(u, z, yv, inv_n, valid, kq == 0, du, dz, sums);
    if (lane < 16) { a.du[t16 * 16 + lane] = du; a.dz[t16 * 16 + lane] = dz; }

    // ------------------------------------------------------------------ backward: variance head
    f32x4 dh[NT];
    {
      f32x4 dpv1[NT2];
      {
        // d pre_v2 = wv2[f] * dz * (1 - v2^2)
        float* sp = tiled_ptr(a.dpre_v2, t16, H / 4, lane);
#pragma unroll
        for (int t = 0; t < NT4; ++t) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(small + S.wv2() + t * 16 + 4 * kq);
#pragma unroll
          for (int r = 0; r < 4; ++r) v2[t][r] = w[r] * dz * (1.0f - v2[t][r] * v2[t][r]);
          store_block(sp, t, v2[t]);
        }
        zero_blocks<NT2>(dpv1);
        layer_backward<NT4, NT2>(dpv1, v2, pipe, lane, H / 2);
      }
      {
        const float scale = drop ? a.drop.scale[L.nh] : 1.0f, inv_scale = 1.0f / scale;
        const float* hp = tiled_ptr(a.stash_v1, t16, H / 2, lane);
        float* sp = tiled_ptr(a.dpre_v1, t16, H / 2, lane);
        // all stash loads first (independent addresses, one exposed latency), then the arithmetic
        f32x4 hl[NT2];
        unsigned kb[NP / 2];
#pragma unroll
        for (int t = 0; t < NT2; ++t) load_block(hp, t, hl[t]);
#pragma unroll
        for (int fp = 0; fp < NP / 2; ++fp) kb[fp] = keep[(L.nh * NP + fp) * 64];
#pragma unroll
        for (int fp = 0; fp < NP / 2; ++fp) {
          tanh_drop_backward_pair(dpv1[2 * fp], dpv1[2 * fp + 1], hl[2 * fp], hl[2 * fp + 1], kb[fp], scale, inv_scale);
          store_block(sp, 2 * fp, dpv1[2 * fp]);
          store_block(sp, 2 * fp + 1, dpv1[2 * fp + 1]);
        }
      }
      // d h_last = w_p * du + Wv0^T d pre_v1
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(small + S.wp() + t * 16 + 4 * kq);
        dh[t] = w * du;
      }
      layer_backward<NT2, NT>(dh, dpv1, pipe, lane, H);
    }

    // ------------------------------------------------------------------ backward: hidden layers nh-1 .. 0
#pragma unroll 1
    for (int l = L.nh - 1; l >= 0; --l) {
      {
        const float scale = drop ? a.drop.scale[l] : 1.0f, inv_scale = 1.0f / scale;
        const float* hp = tiled_ptr(a.stash_h + (long long)l * a.t16 * H * 16, t16, H, lane);
        float* sp = tiled_ptr(a.dpre_h + (long long)l * a.t16 * H * 16, t16, H, lane);
        f32x4 hl[NT];
        unsigned kb[NP];
#pragma unroll
        for (int t = 0; t < NT; ++t) load_block(hp, t, hl[t]);
#pragma unroll
        for (int fp = 0; fp < NP; ++fp) kb[fp] = keep[(l * NP + fp) * 64];
#pragma unroll
        for (int fp = 0; fp < NP; ++fp) {
          tanh_drop_backward_pair(dh[2 * fp], dh[2 * fp + 1], hl[2 * fp], hl[2 * fp + 1], kb[fp], scale, inv_scale);
          store_block(sp, 2 * fp, dh[2 * fp]);
          store_block(sp, 2 * fp + 1, dh[2 * fp + 1]);
        }
      }
      if (l > 0) {
        f32x4 acc[NT];
        zero_blocks<NT>(acc);
        layer_backward<NT, NT>(acc, dh, pipe, lane, H);
#pragma unroll
        for (int t = 0; t < NT; ++t) dh[t] = acc[t];
      }
    }
  }

  // ---------------------------------------------------------------------- loss partial sums of this workgroup
  store_loss_partials<4>(sums, red, a.loss_part, lane, wave);
}

// ---------------------------------------------------------------------------------------
// K6: weight gradients.  dW[i][j] = sum_rows P[i][row] Q[j][row]  (+ bias / vector sums)
// MFMA 32x32x2: k-step s of a 16-row tile pairs rows (s, s + 8): lane half hh supplies row 8*hh + s,
// so a lane's operand for the 8 k-steps of a tile is 8 contiguous floats of one feature row.
// ---------------------------------------------------------------------------------------
#define PINN_MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

template <int TI, int TJ, bool QX>
__device__ __forceinline__ void wgrad_load(WFrag<TI, TJ>& f, const WgradArgs& a, long long t, int i0, int j0, int hh, int i) {
  const float* pP = a.P + ((t * a.OUT + i0 + i) * 16 + 8 * hh);
#pragma unroll
  for (int ti = 0; ti < TI; ++ti) {
    f.a[ti][0] = *reinterpret_cast<const f32x4*>(pP + ti * 512);
    f.a[ti][1] = *reinterpret_cast<const f32x4*>(pP + ti * 512 + 4);
  }
  if (!QX) {
    const float* pQ = a.Q + ((t * a.IN + j0 + i) * 16 + 8 * hh);
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      f.b[tj][0] = *reinterpret_cast<const f32x4*>(pQ + tj * 512);
      f.b[tj][1] = *reinterpret_cast<const f32x4*>(pQ + tj * 512 + 4);
    }
  } else {
    // Q = x^T: feature j = lane & 31 (< 8 valid), rows t*16 + 8*hh + s read from row-major x
#pragma unroll
    for (int sg = 0; sg < 2; ++sg)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        long long row = t * 16 + 8 * hh + 4 * sg + j;
        if (row >= a.n_rows) row = a.n_rows - 1;     // dpre of such rows is exactly 0
        f.b[0][sg][j] = (i < 8) ? a.x[row * 8 + i] : 0.0f;
      }
  }
}

template <int TI, int TJ, int WI, int WJ, bool QX>
__global__ __launch_bounds__(kThreads, 1) void wgrad_kernel(WgradArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave >= WI * WJ) return;
  const int wi = wave / WJ, wj = wave % WJ;
  const int hh = lane >> 5, i = lane & 31;
  const int i0 = blockIdx.y * (TI * 32 * WI) + wi * TI * 32, j0 = wj * TJ * 32;     // blockIdx.y: output block (wide nets' layer 0)

  f32x16 acc[TI][TJ];
  zero_acc(acc);
  // (bias sums: a slice adds up to a few thousand rows per lane one after the other, where torch sums pairwise -- fp32 over
  //  eight tiles, those partial sums in float64; float64 adds in every tile cost the layer-0 kernel a quarter of its time)
  double bsum[TI];
  float bpart[TI], vq[TJ], vr[TI];
  int n_part = 0;
#pragma unroll
  for (int ti = 0; ti < TI; ++ti) { bsum[ti] = 0.0; bpart[ti] = 0.f; vr[ti] = 0.f; }
#pragma unroll
  for (int tj = 0; tj < TJ; ++tj) vq[tj] = 0.f;

  const int slice = blockIdx.x;
  const SliceRange sr = slice_range(a, slice);
  const long long t_begin = sr.t_begin, t_end = sr.t_end;

  // software pipeline, two tiles deep where the registers allow (< 256 accumulator registers): the fragments and the
  // vector-head operands of tiles t+1 and t+2 are in flight while tile t multiplies (one tile ahead is about one HBM
  // latency of work; the layer-0 kernel streamed at 2.9 TB/s with it)
  constexpr bool kDeep = TI * TJ < 16;
  struct Side { f32x4 r[kDeep ? TI : 1][2], s2[2], s1[2]; };      // operands of the vector-head sums (prefetched iff kDeep)
  const bool want_r = wj == 0 && a.dvr, want_q = wi == 0 && a.dvq;
  auto load_r = [&](long long t, int ti, int sg) { return *reinterpret_cast<const f32x4*>(a.R + ((t * a.OUT + i0 + i) * 16 + 8 * hh) + ti * 512 + sg * 4); };
  auto load_s = [&](const float* sv, long long t, int sg) { return *reinterpret_cast<const f32x4*>(sv + t * 16 + 8 * hh + sg * 4); };
  auto fetch = [&](WFrag<TI, TJ>& f, Side& sd, long long t) {
    if (t >= t_end) t = t_end - 1;
    wgrad_load<TI, TJ, QX>(f, a, t, i0, j0, hh, i);
    if constexpr (kDeep) {
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        if (want_r) {
          sd.s2[sg] = load_s(a.s2, t, sg);
#pragma unroll
          for (int ti = 0; ti < TI; ++ti) sd.r[ti][sg] = load_r(t, ti, sg);
        }
        if (want_q) sd.s1[sg] = load_s(a.s1, t, sg);
      }
    }
  };
  auto tile = [&](const WFrag<TI, TJ>& cur, const Side& sd, long long t) {
#pragma unroll
    for (int sg = 0; sg < 2; ++sg)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int ti = 0; ti < TI; ++ti)
#pragma unroll
          for (int tj = 0; tj < TJ; ++tj) acc[ti][tj] = PINN_MFMA32(cur.a[ti][sg][j], cur.b[tj][sg][j], acc[ti][tj]);
    if (wj == 0) {
#pragma unroll
      for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) bpart[ti] += (cur.a[ti][sg][0] + cur.a[ti][sg][1]) + (cur.a[ti][sg][2] + cur.a[ti][sg][3]);
      if ((++n_part & 7) == 0) {
#pragma unroll
        for (int ti = 0; ti < TI; ++ti) { bsum[ti] += (double)bpart[ti]; bpart[ti] = 0.f; }
      }
      if (a.dvr) {
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
          f32x4 sv;
          if constexpr (kDeep) sv = sd.s2[sg]; else sv = load_s(a.s2, t, sg);
#pragma unroll
          for (int ti = 0; ti < TI; ++ti) {
            f32x4 rv;
            if constexpr (kDeep) rv = sd.r[ti][sg]; else rv = load_r(t, ti, sg);
            vr[ti] += (sv[0] * rv[0] + sv[1] * rv[1]) + (sv[2] * rv[2] + sv[3] * rv[3]);
          }
        }
      }
    }
    if (wi == 0 && a.dvq) {
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        f32x4 sv;
        if constexpr (kDeep) sv = sd.s1[sg]; else sv = load_s(a.s1, t, sg);
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
          vq[tj] += (sv[0] * cur.b[tj][sg][0] + sv[1] * cur.b[tj][sg][1]) + (sv[2] * cur.b[tj][sg][2] + sv[3] * cur.b[tj][sg][3]);
      }
    }
  };
  if constexpr (kDeep) {
    WFrag<TI, TJ> f0, f1, f2;
    Side d0, d1, d2;
    if (t_begin < t_end) { fetch(f0, d0, t_begin); fetch(f1, d1, t_begin + 1); }
    for (long long t = t_begin; t < t_end; t += 3) {
      fetch(f2, d2, t + 2);
      tile(f0, d0, t);
      if (t + 1 < t_end) { fetch(f0, d0, t + 3); tile(f1, d1, t + 1); }
      if (t + 2 < t_end) { fetch(f1, d1, t + 4); tile(f2, d2, t + 2); }
    }
  } else {
    WFrag<TI, TJ> cur, nxt;
    Side none;
    if (t_begin < t_end) fetch(cur, none, t_begin);
    for (long long t = t_begin; t < t_end; ++t) {
      fetch(nxt, none, t + 1);
      tile(cur, none, t);
      cur = nxt;
    }
  }

  // ---- write this slice's slab
  const long long so = (long long)slice * a.slab_stride;
#pragma unroll
  for (int ti = 0; ti < TI; ++ti)
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      const int col = j0 + tj * 32 + i;          // input feature (C/D layout: column on the lane)
      if (col < a.IN) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = cd_row(r, hh, i0 + ti * 32);
          a.dW[so + (long long)row * a.IN + col] = acc[ti][tj][r];
        }
      }
    }
  if (wj == 0) {
#pragma unroll
    for (int ti = 0; ti < TI; ++ti) {
      const double bl = bsum[ti] + (double)bpart[ti];
      const float b = (float)(bl + __shfl_xor(bl, 32, 64));
      if (hh == 0) a.db[so + i0 + ti * 32 + i] = b;
      if (a.dvr) {
        const float v = vr[ti] + __shfl_xor(vr[ti], 32, 64);
        if (hh == 0) a.dvr[so + i0 + ti * 32 + i] = v;
      }
    }
  }
  if (wi == 0 && a.dvq) {
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      const float v = vq[tj] + __shfl_xor(vq[tj], 32, 64);
      if (hh == 0) a.dvq[so + j0 + tj * 32 + i] = v;
    }
  }
}

// grads[e] = sum_s slab[s][e] in a fixed order; scalar head biases and the loss sums from the chain partials.
// A workgroup owns 32 groups of four consecutive parameters; its 256 threads are 8 slice lanes x 32 groups: lane q adds
// the slices q, q + 8, ... of its group (8 independent 16-B loads in flight), the eight partial sums meet in LDS and are
// added in lane order -- the same tree on every run (bitwise reproducible; no float atomics).  (One thread per group
// walking all 256 slices was 32 dependent rounds of loads: 64 us whatever the row count, a fifth of a 65 536-row step.)
// The slabs are added in float64 (the launch is bound by its 180 MB of slab reads, not by the adds) and rounded to fp32 once:
// the reduction over slices adds no rounding of its own to what the slice kernels accumulated.
constexpr int kFinLanes = 8, kFinGroups = 32;
// pinn_mlp_train_step_dev: the optimizer step in the reduction's launch (p == nullptr: gradients only).  `snap` = the step
// counter as the forward kernel of this call read it (TrainBuffers::amax + 2): the counter itself moves during this launch.
struct FinAdam {
  float* p; float* m; float* v;
  const float* coeffs; const unsigned* snap;      // device table + step snapshot (pinn_mlp_train_step_dev), or nullptr:
  float step_size, bc2_sqrt;                      // the step's two scalars by value (pinn_mlp_train_step)
};
typedef double f64x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f64x4 widen4(const f32x4& v) { return f64x4{(double)v[0], (double)v[1], (double)v[2], (double)v[3]}; }
__global__ __launch_bounds__(256) void grad_finalize_kernel(const float* __restrict__ slabs, int n_slices, long long total,
                                                            const double* __restrict__ loss_part, int n_parts,
                                                            long long off_bp, long long off_bv2, float* __restrict__ grads,
                                                            double* __restrict__ loss_out, const unsigned* __restrict__ amax,
                                                            unsigned* __restrict__ range_word, unsigned* __restrict__ step_counter,
                                                            long long e_lo, long long e_hi, int with_loss, FinAdam ad) {
  // [e_lo, e_hi): the part of the flat gradient this launch reduces (multiples of 4; the whole vector, or the head / the tail
  // of pinn_grad_split); with_loss: the launch that also owns the loss sums, the range record and the step counter (the tail)
  __shared__ f64x4 part[kFinLanes][kFinGroups];
  // pinn_net_range_status: the X3 backward chain's largest |d pre-activation| of this call is inf once a row-normalised
  // gradient has left fp16's range (a NaN alone does not move the maximum, but then the gradients are NaN: visible)
  if (with_loss && range_word && blockIdx.x == 0 && threadIdx.x == 0 && (*amax & 0x7FFFFFFFu) >= 0x7F800000u) *range_word = 1u;
  // pinn_dropout_t.d_step_counter: the gradients of this step are final with this launch; every kernel that read the counter
  // (the chain's dropout pass) ran before it, the optimizer step that reads it next runs behind it
  if (with_loss && step_counter && blockIdx.x == 0 && threadIdx.x == 0) *step_counter += 1u;
  float step_size = 0.0f, bc2_sqrt = 1.0f;
  if (ad.p) {
    if (ad.coeffs) {
      const unsigned k = __builtin_amdgcn_readfirstlane(*ad.snap);
      step_size = ad.coeffs[2 * k]; bc2_sqrt = ad.coeffs[2 * k + 1];
    } else {
      step_size = ad.step_size; bc2_sqrt = ad.bc2_sqrt;
    }
  }
  const int g = threadIdx.x & (kFinGroups - 1), q = threadIdx.x / kFinGroups;
  // every tensor starts on a multiple of 4 floats, so the two scalar head biases sit at the start of a group whose other
  // three floats are padding
  const long long e = e_lo + 4 * ((long long)blockIdx.x * kFinGroups + g);
  f64x4 s = {0.0, 0.0, 0.0, 0.0};
  if (e < e_hi) {
    int k = q;
    for (; k + 7 * kFinLanes < n_slices; k += 8 * kFinLanes) {
      f32x4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const f32x4*>(slabs + (long long)(k + j * kFinLanes) * total + e);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += widen4(v[j]);
    }
    for (; k < n_slices; k += kFinLanes) s += widen4(*reinterpret_cast<const f32x4*>(slabs + (long long)k * total + e));
  }
  part[q][g] = s;
  __syncthreads();
  if (q == 0 && e < e_hi) {
    if (e == off_bp || e == off_bv2) {
      grads[e + 1] = 0.0f; grads[e + 2] = 0.0f; grads[e + 3] = 0.0f;       // [e] itself: the loss-sum block below
    } else {
#pragma unroll
      for (int j = 1; j < kFinLanes; ++j) s += part[j][g];
      const f32x4 gv = f32x4{(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
      *reinterpret_cast<f32x4*>(grads + e) = gv;
      if (ad.p) {
        f32x4 pv = *reinterpret_cast<const f32x4*>(ad.p + e), mv = *reinterpret_cast<const f32x4*>(ad.m + e), vv = *reinterpret_cast<const f32x4*>(ad.v + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) { float pj = pv[j], mj = mv[j], vj = vv[j]; adam_update(pj, gv[j], mj, vj, step_size, bc2_sqrt); pv[j] = pj; mv[j] = mj; vv[j] = vj; }
        *reinterpret_cast<f32x4*>(ad.p + e) = pv; *reinterpret_cast<f32x4*>(ad.m + e) = mv; *reinterpret_cast<f32x4*>(ad.v + e) = vv;
      }
    }
  }
  if (blockIdx.x == 0 && with_loss) {
    // the chain's per-workgroup loss partials (<= 1024 x kLossTerms doubles): strided over the 256 threads, then a fixed
    // shuffle / LDS tree (one thread walking them serially cost ~50 us of dependent L2 latency)
    __shared__ double lred[4][kLossTerms];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kLossTerms; ++k) {
      double v = 0.0;
      for (int b = threadIdx.x; b < n_parts; b += 256) v += loss_part[(long long)b * kLossTerms + k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) lred[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kLossTerms) {
      const double t = ((lred[0][threadIdx.x] + lred[1][threadIdx.x]) + lred[2][threadIdx.x]) + lred[3][threadIdx.x];
      if (threadIdx.x < kLossOut) loss_out[threadIdx.x] = t;   // nll sum, |logvar| sum, (y-u)^2 sum, (sum du)
      if (threadIdx.x == kLossDu) grads[off_bp] = (float)t;    // d loss / d b_p  = sum du
      if (threadIdx.x == kLossDz) grads[off_bv2] = (float)t;   // d loss / d bv_2 = sum dz
      if (ad.p && (threadIdx.x == kLossDu || threadIdx.x == kLossDz)) {      // (their groups' padding floats have zero gradient: no update)
        const long long o = threadIdx.x == kLossDu ? off_bp : off_bv2;
        float pj = ad.p[o], mj = ad.m[o], vj = ad.v[o];
        adam_update(pj, (float)t, mj, vj, step_size, bc2_sqrt);
        ad.p[o] = pj; ad.m[o] = mj; ad.v[o] = vj;
      }
    }
  }
}

constexpr long long kFanOutT16 = 2048;       // row tiles below which the weight-gradient launches fan out over side streams
// Row tiles below which PINN_PREC_F32X6 at H = 256 runs every layer's weight gradient as ONE launch of 128 x 128 tiles over 32
// slices (wgrad_p_multi_kernel).  Built for the reference's 1e3 .. 1e4 rows, it wins far beyond: five launches of 256 slices
// write and read back 180 MB of slabs whatever the row count -- at BASELINE config 4's 65 536-row minibatch that was as much
// traffic as the operands themselves (weight gradients 164 -> 123 us, reduction 31 -> 6 us, step 441 -> 372 us; 131 072 rows:
// 770 -> 740; 262 144: 1356 vs 1420, the per-layer kernels' 256 x 256 tiles win from there).
#ifdef PINN_ABL_MULTI_T16
constexpr long long kMultiT16 = PINN_ABL_MULTI_T16;
#else
constexpr long long kMultiT16 = 10240;
#endif

// Side streams for the independent weight-gradient launches of one step at small row counts.  Fork / join with events on the
// caller's stream, so the pattern is legal inside a stream capture (model.train_dnn replays the step as a hipGraph, where the
// branches cost nothing on the host); created at the first small call.  One process drives one GPU (pinn_hip.h).
struct FanOut {
  hipStream_t side[3];
  hipEvent_t fork, join[3];
  bool ok = false;
  bool init() {
    if (ok) return true;
    for (int i = 0; i < 3; ++i) {
      if (hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking) != hipSuccess) return false;
      if (hipEventCreateWithFlags(&join[i], hipEventDisableTiming) != hipSuccess) return false;
    }
    if (hipEventCreateWithFlags(&fork, hipEventDisableTiming) != hipSuccess) return false;
    return ok = true;
  }
};
static FanOut g_fan;

// How the weight-gradient launches of one call are issued.  plan_workspace decides it, once, from the net and the row count; the
// route fixes the slice count, and the launch site (launch_wgrads) reads both from the Workspace.
enum WgradRoute {
  kRouteSerial,     // one launch per layer on the caller's stream
  kRouteFanOut,     // small row counts: the layers' launches are independent and short -- side by side on up to four streams
  kRouteMulti       // PINN_PREC_F32X6 at H = 256: every layer in ONE launch of 128 x 128 tiles (wgrad_p_multi_kernel)
};

struct Workspace {
  long long t16;
  size_t off_stash_h, off_stash_v1, off_stash_v2, off_dpre_h, off_dpre_v1, off_dpre_v2, off_keep, off_du, off_dz, off_loss,
      off_amax, off_rowmeta, off_stash_x, off_slabs;
  WgradRoute route;      // (the fused bf16 family issues its launches one after the other whatever the route: pinn_bf16.hip)
  int n_slices;
  size_t total;
};

static Workspace plan_workspace(const pinn_net_t* net, long long n_rows) {
  Workspace w;
  const long long H = net->hidden, nh = net->n_hidden;
  // whole workgroup tiles: 64 rows (4 wave tiles), 128 (8) for the x6 chain
  w.t16 = (net->precision >= PINN_PREC_F32X6 || net->hidden > 256) ? (n_rows + 127) / 128 * 8 : (n_rows + kTileRows - 1) / kTileRows * 4;
  size_t o = 0;
  auto take = [&](size_t bytes) { size_t at = o; o += (bytes + 255) / 256 * 256; return at; };
  w.off_stash_h = take((size_t)nh * w.t16 * H * 16 * 4);
  w.off_stash_v1 = take((size_t)w.t16 * (H / 2) * 16 * 4);
  w.off_stash_v2 = take((size_t)w.t16 * (H / 4) * 16 * 4);
  w.off_dpre_h = take((size_t)nh * w.t16 * H * 16 * 4);
  w.off_dpre_v1 = take((size_t)w.t16 * (H / 2) * 16 * 4);
  w.off_dpre_v2 = take((size_t)w.t16 * (H / 4) * 16 * 4);
  w.off_keep = take((size_t)w.t16 * (nh * (H / 32) + H / 64) * 64);
  w.off_du = take((size_t)w.t16 * 16 * 4);
  w.off_dz = take((size_t)w.t16 * 16 * 4);
  w.off_loss = take((size_t)1024 * kLossTerms * 8);
  w.off_amax = take(256);                                   // [0] TrainBuffers::amax, [1] ::emax, [2] the step counter as the forward kernel read it
  w.off_rowmeta = take((size_t)w.t16 * 256);                // struct RowMeta records
  w.off_stash_x = take((size_t)w.t16 * 2048);               // packed input rows (PINN_PREC_F32X6, fused nets)
  const long long t32 = (w.t16 + 1) / 2;
  const bool one_launch = net->precision == PINN_PREC_F32X6 && H == 256 && nh - 1 + 3 <= kMaxWgradProblems;
  w.route = (one_launch && w.t16 < kMultiT16) ? kRouteMulti : (w.t16 < kFanOutT16 ? kRouteFanOut : kRouteSerial);
  // slices = workgroups per weight-gradient launch = slabs the reduction adds.  Large row counts: one per CU.  The reference's
  // own sizes (< 32 768 rows) are bound by the slabs instead -- at 1e4 rows 256 slices wrote 67 MB per 256 x 256 layer and the
  // reduction read 180 MB, 100 of the step's 200 us --: 64 slices there, and the five layers' launches run side by side
  // (kRouteFanOut), 320 workgroups in all; kRouteMulti: 32 slices, ~450 workgroups
#ifdef PINN_ABL_MULTI_NS
  constexpr long long kMultiSlices = PINN_ABL_MULTI_NS;
#else
  constexpr long long kMultiSlices = 32;
#endif
  // wide nets: a gradient is (H / 256)^2 blocks of 256 x 256, each with its own slices -- two rounds of workgroups fill the chip, and
  // every further slice is a slab of the whole gradient written and read back (H = 1024 at 262 144 rows: 256 slices wrote 1.07 GB per
  // layer, profiles/r03/pmc_summary_wide.json; 32 slices: training step 21.05 -> 19.6 ms; 16: 20.4; 8: 25.6)
#ifdef PINN_ABL_WIDE_NS
  const long long wide_slices = PINN_ABL_WIDE_NS;
#else
  const long long hb = H / 256, wide_slices = hb > 0 && 512 / (hb * hb) > 8 ? 512 / (hb * hb) : 8;
#endif
  const long long cap = w.route == kRouteMulti ? kMultiSlices : (w.route == kRouteFanOut ? 64 : (H > 256 ? wide_slices : (long long)kMaxSlices));
  w.n_slices = (int)(t32 < cap ? (t32 < 1 ? 1 : t32) : cap);
  ParamLayout L{(int)H, (int)nh};
  w.off_slabs = take((size_t)w.n_slices * L.total() * 4);
  w.total = o;
  return w;
}

// c of the packed weight gradients' row scale t_r = 2^(e_r - E + c) (pinn_x6_core.h): 8 |h| t_r must stay a finite fp16 with
// |h| <= the largest dropout scale of the call
static int row_scale_boost(const DropDev& d, int nh) {
  float smax = 1.0f;
  if (d.mode != PINN_DROP_NONE)
    for (int l = 0; l <= nh; ++l) smax = d.scale[l] > smax ? d.scale[l] : smax;
  int c = (int)floor(log2(65504.0 / (8.0 * (double)smax)));
  return c < 0 ? 0 : (c > 12 ? 12 : c);
}

// pick the wave tiling for an [OUT x IN] gradient (visit_wgrad_tiling, pinn_wgrad_args.h) and launch it
static int dispatch_wgrad(const WgradArgs& a, hipStream_t st) {
  const int to = a.OUT / 32;
  if (a.Q == nullptr) {      // layer 0: blocks of 256 outputs
    const int out_blocks = to % 8 == 0 ? to / 8 : 1;
    return visit_wgrad_tiling_x(to % 8 == 0 ? 8 : to, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((wgrad_kernel<T::TI, T::TJ, T::WI, T::WJ, true>), dim3(a.n_slices, out_blocks), dim3(kThreads), 0, st, a);
    }) ? PINN_OK : PINN_E_ARCH;
  }
  return visit_wgrad_tiling(to, (a.IN + 31) / 32, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((wgrad_kernel<T::TI, T::TJ, T::WI, T::WJ, false>), dim3(a.n_slices), dim3(kThreads), 0, st, a);
  }) ? PINN_OK : PINN_E_ARCH;
}

// the other families' launchers, and the loss partials their chains write for n_rows rows (one per workgroup of the kernel that
// computes the loss: each family answers where it picks that kernel; fp32 / bf16: train_chain_partials, pinn_mlp_core.h)
int launch_train_chain_x6(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y, long long n_rows,
                          long long n_global, const DropDev& drop, const TrainBuffers& b, unsigned which,
                          void* stream);   // pinn_x6_train.hip; which: 1 = forward kernel, 2 = backward kernel, 3 = both
int train_chain_x6_partials(const pinn_net_t* net, long long n_rows);     // pinn_x6_train.hip
int launch_train_chain_wide(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y, long long n_rows,
                            long long n_global, const DropDev& drop, const TrainBuffers& b, void* stream);  // pinn_wide.hip
int train_chain_wide_partials(const pinn_net_t* net, long long n_rows);   // pinn_wide.hip
int launch_train_bf16(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y, long long n_rows,
                      long long n_global, const DropDev& drop, const TrainBuffers& b, unsigned phases, void* stream);
int dispatch_wgrad_x6(const WgradArgs& a, int ns, void* stream);   // pinn_x6_wgrad.hip
int dispatch_wgrad_p(const WgradPArgs& a, void* stream);            // pinn_x6_wgrad.hip: packed operands (PINN_PREC_F32X6)
int dispatch_wgrad_p_multi(const WgradPMulti& m, void* stream);     //   several of them in one launch (kRouteMulti)

// the two fused families (hidden <= 256) with kernels of their own for the whole step
static bool fused_x6(const pinn_net_t* net) { return net->precision >= PINN_PREC_F32X6 && net->hidden <= 256; }
static bool fused_bf16(const pinn_net_t* net) { return net->precision == PINN_PREC_BF16 && net->hidden <= 256; }

static int loss_partials(const pinn_net_t* net, long long n_rows) {
  if (net->hidden > 256) return train_chain_wide_partials(net, n_rows);
  if (net->precision >= PINN_PREC_F32X6) return train_chain_x6_partials(net, n_rows);
  return train_chain_partials(n_rows);
}

}  // namespace pinn

using namespace pinn;

extern "C" long long pinn_grad_split(const pinn_net_t* net) {
  if (check_net(net) != PINN_OK) return -1;
  if (fused_bf16(net)) return 0;      // the fused bf16 family launches its weight gradients as one block
  ParamLayout L{net->hidden, net->n_hidden};
  return net->n_hidden >= 2 ? L.w(net->n_hidden - 1) : L.wp();
}

extern "C" size_t pinn_train_workspace_bytes(const pinn_net_t* net, long long n_rows) {
  if (check_net(net) != PINN_OK || n_rows < 0) return 0;
  return plan_workspace(net, n_rows).total;
}

// The phase mask as the launch steps read it.  The forward / backward halves are separate kernels only in the fused x6 path;
// elsewhere either bit means the chain.  Two-part weight gradients / reduction (pinn_grad_split): the single-part bits mean both
// parts; a precision whose kernels do not split keeps everything in the "tail".
static unsigned normalize_phases(const pinn_net_t* net, unsigned phases) {
  if (!fused_x6(net) && (phases & (PINN_PHASE_CHAIN_FWD | PINN_PHASE_CHAIN_BWD))) phases |= PINN_PHASE_CHAIN;
  if (phases & PINN_PHASE_WGRAD) phases |= PINN_PHASE_WGRAD_TAIL | PINN_PHASE_WGRAD_HEAD;
  if (phases & PINN_PHASE_REDUCE) phases |= PINN_PHASE_REDUCE_TAIL | PINN_PHASE_REDUCE_HEAD;
  if (pinn_grad_split(net) == 0) {
    phases = (phases & ~(PINN_PHASE_WGRAD | PINN_PHASE_REDUCE)) | ((phases & PINN_PHASE_WGRAD_TAIL) ? PINN_PHASE_WGRAD : 0u) |
             ((phases & PINN_PHASE_REDUCE_TAIL) ? PINN_PHASE_REDUCE : 0u);
  }
  return phases;
}

// the launchers' view of the workspace
static TrainBuffers workspace_buffers(const pinn_net_t* net, const Workspace& w, char* base, const DropDev& drop) {
  TrainBuffers b{};
  b.stash_h = base + w.off_stash_h; b.stash_v1 = base + w.off_stash_v1; b.stash_v2 = base + w.off_stash_v2;
  b.dpre_h = base + w.off_dpre_h; b.dpre_v1 = base + w.off_dpre_v1; b.dpre_v2 = base + w.off_dpre_v2;
  b.keep = (unsigned char*)(base + w.off_keep);
  b.du = (float*)(base + w.off_du); b.dz = (float*)(base + w.off_dz);
  b.loss_part = (double*)(base + w.off_loss);
  b.slabs = (float*)(base + w.off_slabs); b.t16 = w.t16; b.n_slices = w.n_slices;
  if (net->precision >= PINN_PREC_F32X6 || net->hidden > 256) {      // the split-operand chains (wide nets: also bf16-mixed)
    b.amax = (unsigned*)(base + w.off_amax); b.emax = b.amax + 1;
    b.rowmeta = base + w.off_rowmeta; b.qboost = row_scale_boost(drop, net->n_hidden); b.stash_x = base + w.off_stash_x;
  }
  return b;
}

// one training call as its three launch steps see it
struct TrainCall {
  const pinn_net_t* net;
  const float* params; const float* x; const float* y;
  long long n_rows, n_global;
  unsigned phases;       // normalize_phases
  DropDev drop;
  Workspace w;
  TrainBuffers b;
  const unsigned* words; // the workspace's status words (Workspace::off_amax)
  int n_partials;        // loss_partials: what the chain writes and the reduction sums, in this call or in another
  hipStream_t st;
};

// forward + loss + backward chain
static int launch_chain(const TrainCall& c) {
  const pinn_net_t* net = c.net;
  if (fused_bf16(net)) return launch_train_bf16(net, c.params, c.x, c.y, c.n_rows, c.n_global, c.drop, c.b, c.phases & PINN_PHASE_CHAIN, c.st);
  // split-operand chain on the 16-bit matrix cores (wide nets: also bf16-mixed)
  if (net->hidden > 256) return launch_train_chain_wide(net, c.params, c.x, c.y, c.n_rows, c.n_global, c.drop, c.b, c.st);
  if (net->precision >= PINN_PREC_F32X6) {
    const unsigned which = (c.phases & PINN_PHASE_CHAIN) ? 3u : (((c.phases & PINN_PHASE_CHAIN_FWD) ? 1u : 0u) | ((c.phases & PINN_PHASE_CHAIN_BWD) ? 2u : 0u));
    return launch_train_chain_x6(net, c.params, c.x, c.y, c.n_rows, c.n_global, c.drop, c.b, which, c.st);
  }
  TrainArgs a{};
  a.params = c.params; a.x = c.x; a.y = c.y; a.n_rows = c.n_rows; a.n_global = c.n_global; a.H = net->hidden; a.nh = net->n_hidden;
  a.drop = c.drop;
  a.stash_h = (float*)c.b.stash_h; a.stash_v1 = (float*)c.b.stash_v1; a.stash_v2 = (float*)c.b.stash_v2;
  a.dpre_h = (float*)c.b.dpre_h; a.dpre_v1 = (float*)c.b.dpre_v1; a.dpre_v2 = (float*)c.b.dpre_v2;
  a.keep = c.b.keep; a.du = c.b.du; a.dz = c.b.dz; a.loss_part = c.b.loss_part; a.t16 = c.b.t16;
  const bool bits = a.drop.mode == PINN_DROP_BITS;
  if (a.H == 256) {
    if (bits) hipLaunchKernelGGL((train_chain_kernel<256, true>), dim3(c.n_partials), dim3(kThreads), 0, c.st, a);
    else hipLaunchKernelGGL((train_chain_kernel<256, false>), dim3(c.n_partials), dim3(kThreads), 0, c.st, a);
  } else {
    if (bits) hipLaunchKernelGGL((train_chain_kernel<128, true>), dim3(c.n_partials), dim3(kThreads), 0, c.st, a);
    else hipLaunchKernelGGL((train_chain_kernel<128, false>), dim3(c.n_partials), dim3(kThreads), 0, c.st, a);
  }
  return PINN_OK;
}

// The streams of one call's weight-gradient launches: the caller's, and under kRouteFanOut g_fan's three side streams in turn.
// Once the fork event is recorded, join() runs on every way out: a side stream left unjoined would invalidate a stream capture.
struct WgradStreams {
  hipStream_t st;
  bool fan;
  int n_launch = 0;
  bool used[3] = {false, false, false};
  hipStream_t pick() {
    if (!fan) return st;
    const int k = n_launch++ % 4;
    if (k == 0) return st;
    if (!used[k - 1]) { (void)hipStreamWaitEvent(g_fan.side[k - 1], g_fan.fork, 0); used[k - 1] = true; }
    return g_fan.side[k - 1];
  }
  void join() {
    for (int k = 0; k < 3; ++k)
      if (used[k]) { (void)hipEventRecord(g_fan.join[k], g_fan.side[k]); (void)hipStreamWaitEvent(st, g_fan.join[k], 0); }
  }
};

// PINN_PREC_F32X6: the chain kernels (fused nets) / layer kernels (wide nets) left every operand as fp16 fragments
// (pinn_x6_core.h), the row scales in the meta records
static int launch_wgrads_packed(const TrainCall& c, WgradStreams& s) {
  const TrainBuffers& b = c.b;
  const bool multi = c.w.route == kRouteMulti;
  WgradPMulti mp{};
  const int rc = for_each_wgrad_problem(b, c.net->hidden, c.net->n_hidden, 4, c.phases, [&](const WgradProblem& w) -> int {
    WgradPArgs p{};
    p.meta = b.rowmeta; p.emax = b.emax; p.qboost = b.qboost;
    p.t16 = b.t16; p.n_slices = b.n_slices; p.slab_stride = ParamLayout{c.net->hidden, c.net->n_hidden}.total(); p.q_log2 = 3;
    p.P = w.P; p.Q = w.Q; p.OUT = w.OUT; p.IN = w.IN; p.dW = b.slabs + w.w; p.db = b.slabs + w.b;
    if (w.kind == 0) {
      // layer 0: dW0 = d pre_0^T x with the rows as a packed group of their own (8 features of 32, stored as x / 16: any
      // |x| < 256 survives the row scale in fp16); [H][8] of the [H][32] product is written
      p.Q = (const char*)b.stash_x; p.IN = 32; p.ldW = 8; p.n_cols = 8; p.q_log2 = -4;
    }
    if (w.kind == 2) p.dvq = b.slabs + w.v;
    if (w.kind == 3) { p.s2 = b.dz; p.R = (const float*)w.R; p.dvr = b.slabs + w.v; }      // (fp32 operands)
    if (!multi) return dispatch_wgrad_p(p, (void*)s.pick());
    mp.p[mp.n] = p; mp.kind[mp.n] = w.kind; ++mp.n;
    return PINN_OK;
  });
  if (rc) return rc;
  return multi && mp.n > 0 ? dispatch_wgrad_p_multi(mp, (void*)c.st) : PINN_OK;
}

// every other precision: fp32 operands in the tiled stash.  Operand split of the kernels: 0 = exact fp32 (wgrad_kernel); 3 = three
// bf16 parts, six products (PINN_PREC_F32X6_G6); 1 = bf16-mixed (wide nets under PINN_PREC_BF16)
static int launch_wgrads_fp32_stash(const TrainCall& c, WgradStreams& s) {
  const int ns = c.net->precision == PINN_PREC_F32X6_G6 ? 3 : (c.net->precision == PINN_PREC_BF16 ? 1 : 0);
  const long long tot = ParamLayout{c.net->hidden, c.net->n_hidden}.total();
  return for_each_wgrad_problem(c.b, c.net->hidden, c.net->n_hidden, 4, c.phases, [&](const WgradProblem& w) -> int {
    const WgradArgs g = wgrad_args<WgradArgs>(w, c.b, c.x, c.n_rows, tot);
    hipStream_t st = s.pick();
    // layer 0: dW0 = dpre_0 x^T (exact fp32 at every precision)
    return ns && w.kind != 0 ? dispatch_wgrad_x6(g, ns, (void*)st) : dispatch_wgrad(g, st);
  });
}

// the per-layer weight gradients into the slices' slabs
static int launch_wgrads(const TrainCall& c) {
  if (fused_bf16(c.net)) return launch_train_bf16(c.net, c.params, c.x, c.y, c.n_rows, c.n_global, c.drop, c.b, c.phases & PINN_PHASE_WGRAD, c.st);
  WgradStreams s{c.st, c.w.route == kRouteFanOut && g_fan.init()};
  if (s.fan && hipEventRecord(g_fan.fork, c.st) != hipSuccess) return (int)hipGetLastError();
  const int rc = c.net->precision == PINN_PREC_F32X6 ? launch_wgrads_packed(c, s) : launch_wgrads_fp32_stash(c, s);
  s.join();
  return rc;
}

// fixed-order sum of the slabs -> d_grads, of the loss partials -> d_loss; fin: the optimizer step in the same launch
static void launch_reduce(const TrainCall& c, float* d_grads, double* d_loss, const FinAdam& fin) {
  const pinn_net_t* net = c.net;
  const ParamLayout L{net->hidden, net->n_hidden};
  const long long tot = L.total(), split = pinn_grad_split(net);
  // (the gradient word of the range record sits behind the pack kernel's words: pack_x6_kernel cleared it for this call)
  unsigned* rw = net->precision == PINN_PREC_F32X6 ? range_status_words(net) : nullptr;
  if (rw) rw += kRangePackBlocks * (2 * (net->n_hidden - 1) + 4);
  const unsigned* amax = fused_bf16(net) ? nullptr : c.words;      // (read next to rw only)
  auto reduce = [&](long long lo, long long hi, int with_loss) {
    hipLaunchKernelGGL(grad_finalize_kernel, dim3((unsigned)(((hi - lo) / 4 + kFinGroups - 1) / kFinGroups)), dim3(256), 0, c.st, c.b.slabs, c.b.n_slices, tot,
                       c.b.loss_part, c.n_partials, L.bp(), L.bv2(), d_grads, d_loss, amax, rw, c.drop.step_counter, lo, hi, with_loss, fin);
  };
  const bool both = (c.phases & PINN_PHASE_REDUCE_TAIL) && (c.phases & PINN_PHASE_REDUCE_HEAD);
  if (both) reduce(0, tot, 1);                               // one launch over the whole vector
  else if (c.phases & PINN_PHASE_REDUCE_TAIL) reduce(split, tot, 1);
  else if (split > 0) reduce(0, split, 0);
}

// fa: the optimizer step in the reduction's launch (pinn_mlp_train_step_dev), or nullptr
static int train_grads_impl(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y,
                            long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads,
                            double* d_loss, void* d_work, size_t work_bytes, void* stream, unsigned phases, const FinAdam* fa) {
  int rc = check_net(net);
  if (rc) return rc;
  if (!d_params || !d_x || !d_y || !d_grads || !d_loss || !d_work || n_rows <= 0 || n_global < n_rows) return PINN_E_ARG;
  if (((unsigned long long)d_grads | (unsigned long long)d_work) & 15) return PINN_E_ARG;      // 16-B vector accesses
  TrainCall c{};
  c.net = net; c.params = d_params; c.x = d_x; c.y = d_y; c.n_rows = n_rows; c.n_global = n_global; c.st = (hipStream_t)stream;
  c.phases = normalize_phases(net, phases);
  c.w = plan_workspace(net, n_rows);
  if (work_bytes < c.w.total) return PINN_E_WORKSPACE;
  (void)hipGetLastError();   // drop a stale error left by another HIP user of this thread
  if ((rc = convert_drop(net, drop, true, &c.drop))) return rc;
  c.b = workspace_buffers(net, c.w, (char*)d_work, c.drop);
  c.words = (const unsigned*)((char*)d_work + c.w.off_amax);
  c.n_partials = loss_partials(net, n_rows);
  FinAdam fin_adam{};
  if (fa) { fin_adam = *fa; fin_adam.snap = fa->coeffs ? c.words + 2 : nullptr; }

  if ((c.phases & (PINN_PHASE_CHAIN | PINN_PHASE_CHAIN_FWD | PINN_PHASE_CHAIN_BWD)) && (rc = launch_chain(c))) return rc;
  if ((c.phases & (PINN_PHASE_WGRAD_TAIL | PINN_PHASE_WGRAD_HEAD)) && (rc = launch_wgrads(c))) return rc;
  if (c.phases & (PINN_PHASE_REDUCE_TAIL | PINN_PHASE_REDUCE_HEAD)) launch_reduce(c, d_grads, d_loss, fin_adam);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? PINN_OK : (int)e;
}

extern "C" int pinn_mlp_train_grads_phases(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y,
                                           long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads,
                                           double* d_loss, void* d_work, size_t work_bytes, void* stream, unsigned phases) {
  return train_grads_impl(net, d_params, d_x, d_y, n_rows, n_global, drop, d_grads, d_loss, d_work, work_bytes, stream, phases, nullptr);
}

// One optimizer step of train_dnn (01:949-954) as ONE launch sequence that can be captured and replayed: pinn_mlp_train_grads
// with the Adam step applied by the slab reduction's own launch (at the reference's row counts a step is a chain of short
// dependent launches, and the separate optimizer launch was 5 of its ~130 us).  d_params is updated in place.
extern "C" int pinn_mlp_train_step_dev(const pinn_net_t* net, float* d_params, const float* d_x, const float* d_y,
                                       long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads,
                                       double* d_loss, void* d_work, size_t work_bytes, float* d_m, float* d_v,
                                       const float* d_coeffs, void* stream) {
  if (!net || !drop || !drop->d_step_counter || !d_m || !d_v || !d_coeffs) return PINN_E_ARG;
  if (!fused_x6(net)) return PINN_E_ARCH;      // (the kernels that leave the counter's snapshot)
  if (((unsigned long long)d_params | (unsigned long long)d_m | (unsigned long long)d_v) & 15) return PINN_E_ARG;
  const FinAdam fa{d_params, d_m, d_v, d_coeffs, nullptr, 0.0f, 1.0f};
  return train_grads_impl(net, d_params, d_x, d_y, n_rows, n_global, drop, d_grads, d_loss, d_work, work_bytes, stream, PINN_PHASE_ALL, &fa);
}

// The same with the step's scalars by value (lr from StepLR, step 1-based: pinn_adam_step's arguments): pinn_mlp_train_grads +
// pinn_adam_step in one launch sequence, for callers that launch step by step.  Every precision and width.
extern "C" void pinn_adam_coeffs(float lr, int step, float* step_size, float* bc2_sqrt);
extern "C" int pinn_mlp_train_step(const pinn_net_t* net, float* d_params, const float* d_x, const float* d_y,
                                   long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads,
                                   double* d_loss, void* d_work, size_t work_bytes, float* d_m, float* d_v, float lr, int step,
                                   void* stream) {
  if (!net || !d_m || !d_v || step < 1) return PINN_E_ARG;
  if (((unsigned long long)d_params | (unsigned long long)d_m | (unsigned long long)d_v) & 15) return PINN_E_ARG;
  FinAdam fa{d_params, d_m, d_v, nullptr, nullptr, 0.0f, 1.0f};
  pinn_adam_coeffs(lr, step, &fa.step_size, &fa.bc2_sqrt);
  return train_grads_impl(net, d_params, d_x, d_y, n_rows, n_global, drop, d_grads, d_loss, d_work, work_bytes, stream, PINN_PHASE_ALL, &fa);
}

extern "C" int pinn_mlp_train_grads(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y,
                                    long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads,
                                    double* d_loss, void* d_work, size_t work_bytes, void* stream) {
  return pinn_mlp_train_grads_phases(net, d_params, d_x, d_y, n_rows, n_global, drop, d_grads, d_loss, d_work, work_bytes,
                                     stream, PINN_PHASE_ALL);
}
