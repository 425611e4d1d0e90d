// pinn_physics.h -- the fuel-cell row models and the sum reductions of pinn_residuals.hip, each stated once.
//
// The four residual models of the reference
//   net_f_V 01:724-765, net_f_T_simple 01:869-914, net_f_H 01:621-722, net_f_O 01:535-619
// (01 = 01_train_pinn_multiphysics_model.py) are each cut where the stage cache cuts them: *_pre is what does not depend on the
// physics parameters (what stage_prepare stores, at most 6 floats per row), *_terms the rest: the residual, its analytic
// d/dlambda factors and their sums, accumulated there and nowhere else, and the values the columns need.  The
// one-pass kernel runs load_row -> pre -> terms (-> column stores), the cached passes pre -> pack and unpack -> terms, and the
// backward takes its forward values from the same pieces (load_row, current_of, thermal_voltage, nernst_pressures, *_pre,
// hydrogen_target / oxygen_target).  euler_step is the forward of net_f_T 01:767-867 for its kernel and for its backward.
// block_sums and sums_finalize are the one workgroup reduction and the one fixed-order final reduction of every pass.
//
// Included by pinn_residuals.hip alone and compiled under its -ffp-contract=off: every float op below is rounded exactly like
// the reference's separate torch ops, so only the transcendental calls can differ (<= 2 ulp).  Operand order and parentheses are
// the reference's.  A factor is multiplied with its residual in the function that negates it (f * (-(x)) in one expression): split
// over two functions the compiler pushes the negation into x, which gives a NaN sum the other sign.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#include "../../include/pinn_hip.h"

namespace {

constexpr int kMaxBlocks = 1024;   // 256 CUs x 4 workgroups; grid-stride beyond

struct AffineDev {
  double x_min[8];
  double x_scale[8];
  double y_min, y_scale;
  float vn_scale, vn_min;
};

__device__ __forceinline__ float denorm(float v, double mn, double sc) {
  // numpy in-place `X -= min_; X /= scale_` on a float32 array with float64 operands
  float t = (float)((double)v - mn);
  return (float)((double)t / sc);
}

// torch.clamp propagates NaN (a NaN parameter or row stays visible, 01:586-610 / 01:1040-1047); fminf / fmaxf return the
// operand that is not a NaN and would swallow it ("surface NaN")
__device__ __forceinline__ float clamp_min_t(float x, float lo) { return x != x ? x : fmaxf(x, lo); }
__device__ __forceinline__ float clamp_t(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }

// the twelve live physics parameters and the constant P_H2O of 01:745-753
struct LamDev {
  float l1, l2, l3, lT1, lT3, lT5, lH1, lH2, lH3, lO1, lO2, lO3, P_H2O;
};
__device__ __forceinline__ LamDev load_lambdas(const float* __restrict__ lambdas) {
  LamDev L;
  L.l1 = lambdas[PINN_L1]; L.l2 = lambdas[PINN_L2]; L.l3 = lambdas[PINN_L3];
  L.lT1 = lambdas[PINN_LT1]; L.lT3 = lambdas[PINN_LT3]; L.lT5 = lambdas[PINN_LT5];
  L.lH1 = lambdas[PINN_LH1]; L.lH2 = lambdas[PINN_LH2]; L.lH3 = lambdas[PINN_LH3];
  L.lO1 = lambdas[PINN_LO1]; L.lO2 = lambdas[PINN_LO2]; L.lO3 = lambdas[PINN_LO3];
  // 01:745-753  P_H2O from Tc = 55 (all float32 tensor ops in the reference)
  const float Tc = 55.0f;
  const float xw = ((-2.1794f + 0.02953f * Tc) - 9.1837e-5f * (Tc * Tc)) + 1.4454e-7f * ((Tc * Tc) * Tc);
  L.P_H2O = powf(10.0f, xw);
  return L;
}

// The de-normalised row.  The float64 divide of the sklearn-exact de-normalisation is the most expensive op of a pass: only the
// columns the requested residuals read are de-normalised (flags is wave-uniform), the others are 0.
struct RowPhys { float r0, r1, r2, r3, r4, r5, r6, r7; };
__device__ __forceinline__ RowPhys load_row(const float* __restrict__ x, long long row, const AffineDev& aff, unsigned flags) {
  const float4 xa = reinterpret_cast<const float4*>(x)[row * 2];
  const float4 xb = reinterpret_cast<const float4*>(x)[row * 2 + 1];
  const bool fV = flags & PINN_RES_V, fT = flags & PINN_RES_T, fH = flags & PINN_RES_H, fO = flags & PINN_RES_O;
  RowPhys r;
  r.r0 = denorm(xa.x, aff.x_min[0], aff.x_scale[0]);                    // I [A]
  r.r1 = fT ? denorm(xa.y, aff.x_min[1], aff.x_scale[1]) : 0.f;         // coolant flow
  r.r2 = fT ? denorm(xa.z, aff.x_min[2], aff.x_scale[2]) : 0.f;         // T_in
  r.r3 = fV ? denorm(xa.w, aff.x_min[3], aff.x_scale[3]) : 0.f;         // P_H2
  r.r4 = fV ? denorm(xb.x, aff.x_min[4], aff.x_scale[4]) : 0.f;         // P_air
  r.r5 = (fV || fT) ? denorm(xb.y, aff.x_min[5], aff.x_scale[5]) : 0.f; // T_out
  r.r6 = fH ? denorm(xb.z, aff.x_min[6], aff.x_scale[6]) : 0.f;         // H2 flow
  r.r7 = fO ? denorm(xb.w, aff.x_min[7], aff.x_scale[7]) : 0.f;         // air flow
  return r;
}

// the current density of the V, H and O models and the stack current of H and O (T_simple has its own i = I/270 + 1e-6)
struct Current { float i5, It; };
__device__ __forceinline__ Current current_of(float r0) {
  Current c;
  c.i5 = r0 / 270.0f + 1e-5f;        // 01:730, 639, 553
  c.It = c.i5 * 270.0f;              // 01:654, 557
  return c;
}

// ---- net_f_V 01:724-765 ----------------------------------------------------------------
__device__ __forceinline__ float kelvin(float celsius) { return celsius + 273.15f; }

struct ThermalVoltage { float RT, b; };
__device__ __forceinline__ ThermalVoltage thermal_voltage(float Tk) {
  ThermalVoltage t;
  t.RT = 8.314f * Tk;
  t.b = t.RT / 96485.0f;                         // R*Tk / (2*Alpha*F), 2*Alpha = 1
  return t;
}

// the partial pressures of the Nernst term, with the intermediates its backward reads
struct Nernst { float Tk_p, a1, e1, q1, pp_H2, a2, e2, q2, pp_O2; };
__device__ __forceinline__ Nernst nernst_pressures(float i5, float Tk, float r3, float r4, float P_H2O) {
  Nernst n;
  const float P_H2 = r3 / 101.0f + 1.0f;
  const float P_air = r4 / 101.0f + 1.0f;
  n.Tk_p = powf(Tk, 1.334f);
  n.a1 = 1.653f * i5 / n.Tk_p; n.e1 = expf(n.a1); n.q1 = P_H2 / n.e1;
  n.pp_H2 = 0.5f * (n.q1 - P_H2O);
  n.a2 = 4.192f * i5 / n.Tk_p; n.e2 = expf(n.a2); n.q2 = P_air / n.e2;
  n.pp_O2 = n.q2 - P_H2O;
  return n;
}

struct VoltPre { float i5, b, E, V_out; };   // cache slots 0..3 (slot 4 is y, slot 5 the DNN's u)
__device__ __forceinline__ VoltPre volt_pre(const RowPhys& r, float i5, float un, const AffineDev& aff, float P_H2O) {
  const float Tk = kelvin(r.r5);
  const Nernst n = nernst_pressures(i5, Tk, r.r3, r.r4, P_H2O);
  const ThermalVoltage t = thermal_voltage(Tk);
  VoltPre p;
  p.i5 = i5;
  p.b = t.b;
  p.E = 220170.0f / 192970.0f - (t.RT * logf(P_H2O / (n.pp_H2 * sqrtf(n.pp_O2)))) / 192970.0f;
  p.V_out = denorm(un, aff.y_min, aff.y_scale) / 5.0f;   // u detached, 01:734-737
  return p;
}

// The sums against the measured voltage yv are optional: the one-pass kernel allows y == nullptr, the cached passes require y.
struct VoltTerms { float V_act, V_ohm, V_conc, V_est5, f; };
__device__ __forceinline__ VoltTerms volt_terms(const VoltPre& p, const LamDev& L, bool has_y, float yv, float un, const AffineDev& aff,
                                                float (&acc)[PINN_NSUMS]) {
  const float i5 = p.i5, b = p.b;
  VoltTerms t;
  t.V_act = (-b) * logf(i5 / L.l2);
  t.V_ohm = -(i5 * L.l1);
  t.V_conc = (0.5f * b) * logf(1.0f - i5 / L.l3);
  const float V_est = ((p.E + t.V_act) + t.V_ohm) + t.V_conc;
  t.f = V_est - p.V_out;
  t.V_est5 = V_est * 5.0f;
  // analytic df_V/dlambda
  const float d1 = -i5;
  const float d2 = b / L.l2;
  const float d3 = 0.5f * b * i5 / (L.l3 * (L.l3 - i5));
  acc[PINN_S_FV2] += t.f * t.f;
  acc[PINN_S_FV_D1] += t.f * d1;
  acc[PINN_S_FV_D2] += t.f * d2;
  acc[PINN_S_FV_D3] += t.f * d3;
  if (has_y) {
    const float Vn = t.V_est5 * aff.vn_scale + aff.vn_min;   // 01:1025
    const float dy = yv - Vn;
    acc[PINN_S_YV2] += dy * dy;
    acc[PINN_S_YV_D1] += dy * d1;
    acc[PINN_S_YV_D2] += dy * d2;
    acc[PINN_S_YV_D3] += dy * d3;
    const float du = yv - un;
    acc[PINN_S_YU2] += du * du;
  }
  return t;
}

// ---- net_f_T_simple 01:869-914 ----------------------------------------------------------
struct ThermPre { float It6, mc, T_in, T_out; };   // cache slots 0..3
__device__ __forceinline__ ThermPre therm_pre(const RowPhys& r) {
  const float i6 = r.r0 / 270.0f + 1e-6f;     // 01:884
  ThermPre p;
  p.mc = r.r1 + 1e-6f;
  p.It6 = i6 * 270.0f;
  p.T_in = r.r2;
  p.T_out = r.r5;
  return p;
}

struct ThermTerms { float T_pred, f; };
__device__ __forceinline__ ThermTerms therm_terms(const ThermPre& p, const LamDev& L, float (&acc)[PINN_NSUMS]) {
  ThermTerms t;
  t.T_pred = ((L.lT1 * p.It6 + L.lT3 * p.mc) + 0.5f * p.T_in) + L.lT5;   // 01:905
  t.f = p.T_out - t.T_pred;
  acc[PINN_S_FT2] += t.f * t.f;
  acc[PINN_S_FT_D1] += t.f * (-p.It6);
  acc[PINN_S_FT_D3] += t.f * (-p.mc);
  acc[PINN_S_FT_D5] += -t.f;
  acc[PINN_S_FT_ABS] += fabsf(t.f);
  return t;
}

// ---- net_f_H 01:621-722 and net_f_O 01:535-619: a measured flow over the stoichiometric one, against a target ---------------
// cache slots 0..1 are It and act; the stoichiometric flow before (Qp) and after (Q) its clamp and o2 are what the columns and
// the backward read besides
struct FlowPre { float It, act, Qp, Q, o2; };
__device__ __forceinline__ FlowPre hydrogen_pre(float It, float r6) {
  FlowPre p;
  p.It = It; p.o2 = 0.0f;
  p.Qp = ((It / 192970.0f) * 5.0f) * 22.4f;   // 01:660-667
  p.Qp = p.Qp * 60.0f;
  p.Q = clamp_min_t(p.Qp, 1e-8f);
  p.act = (r6 + 1e-6f) / p.Q;
  return p;
}
__device__ __forceinline__ FlowPre oxygen_pre(float It, float r7) {
  FlowPre p;
  p.It = It;
  p.Qp = ((It * 5.0f) / 385940.0f) * 22.4f;   // 01:564-566
  p.Qp = p.Qp * 60.0f;
  p.Q = clamp_min_t(p.Qp, 1e-8f);
  p.o2 = (r7 + 1e-6f) * 0.21f;
  p.act = p.o2 / p.Q;
  return p;
}

struct Target { bool lin; float thr, raw; };   // raw: before the oxygen model's clamp
__device__ __forceinline__ Target hydrogen_target(float It, const LamDev& L) {
  Target g;
  g.thr = L.lH3;
  g.lin = It <= L.lH3;                    // 01:697-701
  g.raw = g.lin ? (L.lH1 + L.lH2 * (It / 100.0f)) : (L.lH1 + L.lH2 * (L.lH3 / 100.0f));
  return g;
}
__device__ __forceinline__ Target oxygen_target(float It, const LamDev& L) {
  Target g;
  g.thr = fabsf(L.lO3);
  g.lin = It <= g.thr;                    // 01:586-590
  g.raw = g.lin ? (L.lO1 + L.lO2 * (It / 100.0f)) : (L.lO1 + L.lO2 * (g.thr / 100.0f));
  return g;
}

struct FlowTerms { float f, tgt; };
__device__ __forceinline__ FlowTerms hydrogen_terms(const FlowPre& p, const LamDev& L, float (&acc)[PINN_NSUMS]) {
  const Target g = hydrogen_target(p.It, L);
  FlowTerms t;
  t.tgt = g.raw;
  t.f = p.act - t.tgt;
  acc[PINN_S_FH2] += t.f * t.f;
  acc[PINN_S_FH_D1] += -t.f;
  acc[PINN_S_FH_D2] += t.f * (-(g.lin ? p.It / 100.0f : L.lH3 / 100.0f));
  acc[PINN_S_FH_D3] += t.f * (-(g.lin ? 0.0f : L.lH2 / 100.0f));
  acc[PINN_S_ACTH] += p.act;
  acc[PINN_S_TGTH] += t.tgt;
  return t;
}
__device__ __forceinline__ FlowTerms oxygen_terms(const FlowPre& p, const LamDev& L, float (&acc)[PINN_NSUMS]) {
  const Target g = oxygen_target(p.It, L);
  FlowTerms t;
  t.tgt = clamp_t(g.raw, 1.05f, 15.0f);
  const float c = (g.raw >= 1.05f && g.raw <= 15.0f) ? 1.0f : 0.0f;   // torch.clamp backward is inclusive
  t.f = (p.act - t.tgt) + clamp_min_t(1.0f - p.act, 0.0f) * 10.0f;   // 01:606-610
  const float sgn = (L.lO3 > 0.0f) ? 1.0f : ((L.lO3 < 0.0f) ? -1.0f : 0.0f);
  acc[PINN_S_FO2] += t.f * t.f;
  acc[PINN_S_FO_D1] += t.f * (-c);
  acc[PINN_S_FO_D2] += t.f * (-c * (g.lin ? p.It / 100.0f : g.thr / 100.0f));
  acc[PINN_S_FO_D3] += t.f * (-c * (g.lin ? 0.0f : L.lO2 * sgn / 100.0f));
  acc[PINN_S_ACTO] += p.act;
  acc[PINN_S_TGTO] += t.tgt;
  return t;
}

// ---- net_f_T 01:767-867: the forward of one Euler step from the predecessor row (pa, pb: its two float4 halves; un: the DNN's
// voltage of that row).  T_pred = T_prev + dT 0.1.
//   I = (I/270 + 1e-5) 270;  V_rev = 1.229 - 0.0009 ((T_out + 273.15) - 298.15);  V_cell = denorm(u) / 5
//   Q_el = (I V_rev - I V_cell) lT4;  Q_cool = (m + 1e-6) 4180 (T_out - T_in) lT1;  Q_rad = 20 * 0.2 (T_out - 25) lT3
struct EulerFwd { float I_tot, V_rev, V_cell, A, B, C, dTc, m_cool, dT, T_prev; };
__device__ __forceinline__ EulerFwd euler_step(float4 pa, float4 pb, float un, const AffineDev& aff, float lT1, float lT2, float lT3, float lT4) {
  EulerFwd e;
  const float r0 = denorm(pa.x, aff.x_min[0], aff.x_scale[0]);
  e.m_cool = denorm(pa.y, aff.x_min[1], aff.x_scale[1]) + 1e-6f;
  const float T_in = denorm(pa.z, aff.x_min[2], aff.x_scale[2]);
  e.T_prev = denorm(pb.y, aff.x_min[5], aff.x_scale[5]);
  const float i5 = r0 / 270.0f + 0.00001f;
  e.I_tot = i5 * 270.0f;
  const float Tk = kelvin(e.T_prev);
  e.V_rev = 1.229f - 0.0009f * (Tk - 298.15f);
  e.V_cell = denorm(un, aff.y_min, aff.y_scale) / 5.0f;
  e.A = e.I_tot * e.V_rev - e.I_tot * e.V_cell;
  const float Q_el = e.A * lT4;
  e.dTc = e.T_prev - T_in;
  e.B = (e.m_cool * 4180.0f) * e.dTc;
  const float Q_cool = e.B * lT1;
  e.C = (20.0f * 0.2f) * (e.T_prev - 25.0f);
  const float Q_rad = e.C * lT3;
  e.dT = ((Q_el - Q_cool) - Q_rad) / lT2;
  return e;
}

// ---- reductions (bitwise reproducible, no float atomics) --------------------------------
// The sums a pass can touch: one stage model's are a contiguous range of the enum, any other flag combination gets all of them.
// Stated once for everything that reduces sums (the two row-pass kernels, the finalize, the persistent stage kernel): what lies
// outside the range is exactly 0 and costs no shuffle, no LDS round and no load.
struct SumRange { int lo, hi; };
constexpr SumRange live_sums(unsigned flags) {
  return flags == PINN_RES_V ? SumRange{PINN_S_FV2, PINN_S_YU2 + 1}
       : flags == PINN_RES_T ? SumRange{PINN_S_FT2, PINN_S_FT_ABS + 1}
       : flags == PINN_RES_H ? SumRange{PINN_S_FH2, PINN_S_TGTH + 1}
       : flags == PINN_RES_O ? SumRange{PINN_S_FO2, PINN_S_TGTO + 1}
                             : SumRange{0, PINN_NSUMS};
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// A workgroup's sums of acc[kLo..kHi-1] in double: wave64 shuffles -> LDS -> thread k adds the waves in index order and writes
// dst[kLo + k].  dst is the workgroup's row of the global partials (entries outside the range are not written: sums_finalize is
// given the same range and does not read them) or the persistent kernel's sums in LDS.  One barrier inside; the caller places
// another before dst is read by other threads and before the function is entered again.
template <int kLo, int kHi, int kBlock, typename Acc>
__device__ __forceinline__ void block_sums(const Acc& acc, double* __restrict__ dst) {
  __shared__ double red[kBlock / 64][kHi - kLo];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int s = kLo; s < kHi; ++s) {
    const double w = wave_sum((double)acc[s]);
    if (lane == 0) red[wave][s - kLo] = w;
  }
  __syncthreads();
  if (threadIdx.x < kHi - kLo) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) t += red[w][threadIdx.x];
    dst[kLo + threadIdx.x] = t;
  }
}

// Fixed-order final reduction of the sums s_lo..s_hi-1 of partials[block][PINN_NSUMS]: thread (s, j) sums partials j, j+32, ...
// then lane s adds the 32 j-sums in order.  Out = double: d_sums[PINN_NSUMS], every entry outside the range set to 0.
// Out = float: the PINN_NLAMBDA parameter gradients of the two backwards (range 0..PINN_NLAMBDA).
template <typename Out>
__global__ __launch_bounds__(1024) void sums_finalize(const double* __restrict__ partials, int n_blocks, int s_lo, int s_hi, Out* __restrict__ out) {
  constexpr int n_out = std::is_same<Out, float>::value ? PINN_NLAMBDA : PINN_NSUMS;
  __shared__ double red[32][n_out + 1];
  const int s = threadIdx.x & 31, j = threadIdx.x >> 5;
  if (s >= s_lo && s < s_hi) {
    // all loads first (independent addresses), then the adds in fixed order: not a latency-bound chain
    double v[kMaxBlocks / 32];
#pragma unroll
    for (int k = 0; k < kMaxBlocks / 32; ++k) {
      const int b = j + 32 * k;
      v[k] = b < n_blocks ? partials[(long long)b * PINN_NSUMS + s] : 0.0;
    }
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kMaxBlocks / 32; ++k) t += v[k];
    red[j][s] = t;
  }
  __syncthreads();
  if (threadIdx.x < n_out) {
    double r = 0.0;
    if (threadIdx.x >= s_lo && threadIdx.x < s_hi) {
#pragma unroll
      for (int k = 0; k < 32; ++k) r += red[k][threadIdx.x];
    }
    out[threadIdx.x] = (Out)r;
  }
}

}  // namespace
