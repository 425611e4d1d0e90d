// pinn_wgrad_core.h -- what the weight-gradient kernels share on the device, stated once.
//
// Every kernel of the family computes dW = dpre^T . h over a slice of 16-row tiles on 32 x 32 MFMA tiles, plus the bias and the
// two vector-head sums, and writes them to its slice's slab: wgrad_kernel (pinn_train.hip, exact fp32), wgrad_x_kernel,
// wgrad_d_kernel, wgrad_p_body (pinn_x6_wgrad.hip, 16-bit matrix cores) and wgrad_bf16_kernel (pinn_bf16.hip).  Here: the
// contiguous slice range, the accumulators' start, the C/D row map and the slab store, the split-bf16 product order and the
// fp32 fragment type.  Every piece is forced inline.
//
// The bar for a piece to live here: every kernel that takes it compiles to the instructions it had with its own text (same opcode
// multiset, registers, spills and scratch).  hipcc's output for these kernels moves with the smallest change of form, so what missed
// the bar stays in the kernels' own text on purpose (profiles/r11/README.md has the figures): a wave's coordinates, the half-wave
// add with the db / dvr / dvq stores, the guarded and the permuted slab stores (own loops over cd_row), and Side, the vector-head
// sums and the kDeep pipeline of wgrad_kernel and wgrad_x_kernel (as one body over a policy, wgrad_x_kernel<4,4,2,2,3> spilled more).
#pragma once
#include "pinn_wgrad_args.h"

namespace pinn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- slice s of n_slices takes the row tiles [t_begin, t_end): contiguous ranges of ceil(t16 / n_slices), the last one short,
// those past the end empty (wgrad_p_body interleaves its slices instead: its own walk)
struct SliceRange {
  long long t_begin, t_end;
};
template <class Args>
__device__ __forceinline__ SliceRange slice_range(const Args& a, int slice) {
  const long long per = (a.t16 + a.n_slices - 1) / a.n_slices;
  SliceRange s;
  s.t_begin = slice * per;
  s.t_end = s.t_begin + per;
  if (s.t_end > a.t16) s.t_end = a.t16;
  return s;
}

template <int TI, int TJ>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[TI][TJ]) {
#pragma unroll
  for (int ti = 0; ti < TI; ++ti)
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[ti][tj][r] = 0.0f;
}

// ---- C/D layout of a 32 x 32 MFMA tile: the column on the lane (i), accumulator register r of lane half hh holds row cd_row.
// The terms are added onto `base` one by one, as the kernels' address arithmetic always did: cd_row(r, hh, i0 + ti * 32) and
// i0 + ti * 32 + cd_row(r, hh) are different instructions.
__device__ __forceinline__ constexpr int cd_row(int r, int hh, int base = 0) { return base + (r & 3) + 8 * (r >> 2) + 4 * hh; }
// the slab store where IN is a multiple of 32 (so: the slice's slab)
template <class Args, int TI, int TJ>
__device__ __forceinline__ void store_slab(const Args& a, long long so, const f32x16 (&acc)[TI][TJ], int i0, int j0, int hh, int i) {
#pragma unroll
  for (int ti = 0; ti < TI; ++ti)
#pragma unroll
    for (int tj = 0; tj < TJ; ++tj) {
      const int col = j0 + tj * 32 + i;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = cd_row(r, hh, i0 + ti * 32);
        a.dW[so + (long long)row * a.IN + col] = acc[ti][tj][r];
      }
    }
}

// ---- products (sa, sb) of NS bf16 parts per operand with sa + sb < NS, smallest first (wgrad_x_kernel, wgrad_d_kernel)
template <int NS, int TI, int TJ, class Parts>
__device__ __forceinline__ void split_products(f32x16 (&acc)[TI][TJ], const Parts (&pa)[TI], const Parts (&pb)[TJ]) {
#pragma unroll
  for (int tot = NS - 1; tot >= 0; --tot)
#pragma unroll
    for (int sa = 0; sa <= tot; ++sa)
#pragma unroll
      for (int ti = 0; ti < TI; ++ti)
#pragma unroll
        for (int tj = 0; tj < TJ; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pa[ti].p[sa]), __builtin_bit_cast(bf16x8, pb[tj].p[tot - sa]),
                                                                acc[ti][tj], 0, 0, 0);
}

// ---- fp32 fragments of a tile: 8 contiguous rows of one feature per lane, as two 16-B loads
template <int TI, int TJ>
struct WFrag {
  f32x4 a[TI][2], b[TJ][2];
};

}  // namespace pinn
