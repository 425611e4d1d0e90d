// pinn_wgrad_args.h -- host side of the weight-gradient kernels, stated once for every family (exact fp32: pinn_train.hip;
// split-bf16 and packed: pinn_x6_wgrad.hip; bf16: pinn_bf16.hip): the kernels' arguments, the wave tiling of a gradient and
// the list of a training step's weight-gradient problems.  The device pieces the kernels share are in pinn_wgrad_core.h.
#pragma once
#include "pinn_mlp_core.h"

namespace pinn {

// dW[i][j] = sum_rows P[i][row] Q[j][row]  (+ bias / vector sums), operands in the tiled stash layout; T = the stash's element
// (float, or __bf16 in the fused bf16 family)
template <class T>
struct WgradArgsT {
  const T* P;        // [T16][OUT][16]   d pre-activation of this layer
  const T* Q;        // [T16][IN][16]    its input activation (or nullptr: read x rows, IN = 8)
  const float* x;    // [n_rows][8] when Q == nullptr
  long long n_rows;
  int OUT, IN;
  long long t16;
  int n_slices;
  long long slab_stride;    // floats between consecutive slices' slabs (= padded param count)
  float* dW;                // slab of slice 0: [OUT][IN] row-major at the parameter's offset
  float* db;                // slab of slice 0: [OUT]
  const float* s1; float* dvq;                // optional: dvq[j] = sum_rows s1[row] Q[j][row]
  const float* s2; const T* R; float* dvr;    // optional: dvr[i] = sum_rows s2[row] R[i][row]
};
struct WgradArgs : WgradArgsT<float> {};

// the packed form (PINN_PREC_F32X6 on the fused nets): operands are the chain kernels' fp16 fragments, pinn_x6_core.h packed_ptr
struct WgradPArgs {
  const char* P;     // [T16][OUT / 32][2 KB]  d pre-activation in the rows' normalised units: parts hi, lo
  const char* Q;     // [T16][IN / 32][2 KB]   8 x the input activation: parts hi, lo
  const void* meta;  // [T16][256 B]: struct RowMeta records (row scales t_r, du_r norm_r as two fp16 parts, dz_r)
  const unsigned* emax;   // bits of the call's largest max(|du|, |dz|) -> E
  int qboost;             // c
  int q_log2;             // log2 of the scale the Q stash carries: 3 (8 x the activation) or -4 (the input rows, x / 16)
  int ldW, n_cols;        // 0, or (layer 0: IN = 32 of which 8 are real) the leading dimension of dW and the columns to write
  int OUT, IN;
  long long t16;
  int n_slices;
  long long slab_stride;
  float* dW; float* db;
  float* dvq;                                     // optional: dvq[j] = sum_rows du[row] Q[j][row]   (du from the meta records)
  const float* s2; const float* R; float* dvr;    // optional: dvr[i] = sum_rows dz[row] R[i][row]   (R fp32 [T16][OUT][16]; dz from the meta records, s2 only says so)
};

// several packed weight-gradient problems in one launch (small row counts, H = 256: pinn_x6_wgrad.hip wgrad_p_multi_kernel)
constexpr int kMaxWgradProblems = 12;
struct WgradPMulti {
  WgradPArgs p[kMaxWgradProblems];
  int kind[kMaxWgradProblems];        // WgradProblem::kind
  int first[kMaxWgradProblems + 1];   // (filled by the launcher) first workgroup of problem k
  int n;
};

// ---------------------------------------------------------------------------------------
// The wave tiling of an [OUT x IN] gradient on the fused nets: TI x TJ tiles of 32 x 32 per wave, WI x WJ waves.  to = OUT / 32,
// ti = IN / 32; f(WgradTiling<..>{}) is called with the table's answer, false = no kernel for this shape.
// ---------------------------------------------------------------------------------------
template <int TI_, int TJ_, int WI_, int WJ_>
struct WgradTiling { static constexpr int TI = TI_, TJ = TJ_, WI = WI_, WJ = WJ_; };

template <class F>
static bool visit_wgrad_tiling(int to, int ti, F&& f) {
  if (to == 8 && ti == 8) f(WgradTiling<4, 4, 2, 2>{});            // H = 256: hidden
  else if (to == 4 && ti == 8) f(WgradTiling<2, 4, 2, 2>{});       //          variance head 0
  else if (to == 2 && ti == 4) f(WgradTiling<1, 2, 2, 2>{});       //          variance head 1; H = 128: variance head 0
  else if (to == 4 && ti == 4) f(WgradTiling<2, 2, 2, 2>{});       // H = 128: hidden
  else if (to == 1 && ti == 2) f(WgradTiling<1, 1, 1, 2>{});       //          variance head 1
  else return false;
  return true;
}
// layer 0 from the x rows (IN = 8, padded to one tile): four waves side by side; to8 = OUT / 32 with every multiple of 8 as 8
// (the wide nets run blocks of 256 outputs)
template <class F>
static bool visit_wgrad_tiling_x(int to8, F&& f) {
  if (to8 == 8) f(WgradTiling<2, 1, 4, 1>{});
  else if (to8 == 4) f(WgradTiling<1, 1, 4, 1>{});
  else return false;
  return true;
}

// ---------------------------------------------------------------------------------------
// The weight-gradient problems of one training step, in launch order: layer 0 (with the head part), the hidden layers
// nh - 1 .. 1 (the last one belongs to the tail part: its d pre-activations are the first the backward chain finishes), the two
// variance-head layers with the vector heads riding along (tail).  A launcher turns a problem into its kernels' argument struct.
// ---------------------------------------------------------------------------------------
struct WgradProblem {
  int kind;                 // 0 layer 0, 1 hidden, 2 variance head 0 (+ predict weight: dvq), 3 variance head 1 (+ last weight: dvr)
  int OUT, IN;
  const char* P;            // d pre-activation
  const char* Q;            // input activation; nullptr: the x rows (layer 0, IN = 8)
  const char* R;            // kind 3: the operand of dvr (stash_v2)
  long long w, b, v;        // ParamLayout offsets of dW, db and (kinds 2, 3) dvq / dvr
};
// esz: bytes per stash element (4: fp32 and packed fp16 hi + lo; 2: bf16); phases: PINN_PHASE_WGRAD_HEAD / _TAIL
template <class F>
static int for_each_wgrad_problem(const TrainBuffers& b, int H, int nh, int esz, unsigned phases, F&& f) {
  const ParamLayout L{H, nh};
  const long long hb = b.t16 * H * 16 * esz;      // bytes per hidden-layer stash
  const char* sh = (const char*)b.stash_h;
  const char* dh = (const char*)b.dpre_h;
  int rc;
  if (phases & PINN_PHASE_WGRAD_HEAD) {
    if ((rc = f(WgradProblem{0, H, 8, dh, nullptr, nullptr, L.w0(), L.b0(), -1}))) return rc;
  }
  for (int l = nh - 1; l >= 1; --l) {
    if (!(phases & (l == nh - 1 ? PINN_PHASE_WGRAD_TAIL : PINN_PHASE_WGRAD_HEAD))) continue;
    if ((rc = f(WgradProblem{1, H, H, dh + l * hb, sh + (l - 1) * hb, nullptr, L.w(l), L.b(l), -1}))) return rc;
  }
  if (phases & PINN_PHASE_WGRAD_TAIL) {
    // dw_p[j] = sum du * h_last[j] rides with variance head 0, dwv2[i] = sum dz * v2[i] with variance head 1
    if ((rc = f(WgradProblem{2, H / 2, H, (const char*)b.dpre_v1, sh + (nh - 1) * hb, nullptr, L.wv0(), L.bv0(), L.wp()}))) return rc;
    if ((rc = f(WgradProblem{3, H / 4, H / 2, (const char*)b.dpre_v2, (const char*)b.stash_v1, (const char*)b.stash_v2, L.wv1(), L.bv1(), L.wv2()}))) return rc;
  }
  return PINN_OK;
}

// a problem as the arguments of the kernels that read the tiled stash (fp32 or bf16 elements)
template <class Args>
static Args wgrad_args(const WgradProblem& p, const TrainBuffers& b, const float* x, long long n_rows, long long slab_stride) {
  using T = decltype(Args::P);
  Args g{};
  g.x = x; g.n_rows = n_rows; g.t16 = b.t16; g.n_slices = b.n_slices; g.slab_stride = slab_stride;
  g.P = (T)p.P; g.Q = (T)p.Q; g.OUT = p.OUT; g.IN = p.IN; g.dW = b.slabs + p.w; g.db = b.slabs + p.b;
  if (p.kind == 2) { g.s1 = b.du; g.dvq = b.slabs + p.v; }
  if (p.kind == 3) { g.s2 = b.dz; g.R = (T)p.R; g.dvr = b.slabs + p.v; }
  return g;
}

}  // namespace pinn
