/* pinn_hip.h -- C ABI of the MI355X (gfx950) PINN training + MC-dropout hot path.
 *
 * The reference (ZhendongS/Physics-Informed-Neural-Network-...-Fuel-Cells) has no FFI or
 * plugin interface: its hot path is the Python object surface of
 * 01_train_pinn_multiphysics_model.py (cited as 01:<line>).  Each entry point below
 * replaces the torch/sklearn/numpy work underneath one group of those methods; the
 * Python classes in the package keep the reference's names and signatures on top
 * (INTEGRATION.md shows the ctypes binding a maintainer of the reference would add).
 *
 * Conventions: every pointer named d_* is DEVICE memory owned by the caller (e.g. a torch
 * tensor's data_ptr()); every call is asynchronous on `stream` (a hipStream_t passed as
 * void*), allocates nothing, never synchronises the device and returns 0 on success or a
 * negative PINN_E_* / positive hipError_t code.  Nothing throws across the ABI.
 * One host thread per process/GPU drives the library; it is not re-entrant per workspace.
 */
#ifndef PINN_HIP_H
#define PINN_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PINN_ABI_VERSION 2   /* 2: pinn_dropout_t.d_step_counter, pinn_adam_step_dev, pinn_net_range_status; precision code 3 = F32X6_G6 */

/* error codes (negative; positive values are hipError_t) */
#define PINN_OK 0
#define PINN_E_ARG (-1)        /* null pointer / negative size / bad flag */
#define PINN_E_ARCH (-2)       /* network shape not supported by the fused kernels */
#define PINN_E_WORKSPACE (-3)  /* workspace too small */
#define PINN_E_RANGE (-4)      /* pinn_net_range_status: a weight or gradient left the domain of the split-operand kernels */

/* ---- physics parameters: float[17] on the device, order of 01:453-517 ------------------ */
enum {
  PINN_L1 = 0, PINN_L2, PINN_L3, PINN_L4,            /* voltage: r, io, il, (unused) */
  PINN_LT1, PINN_LT2, PINN_LT3, PINN_LT4, PINN_LT5,  /* thermal */
  PINN_LH1, PINN_LH2, PINN_LH3, PINN_LH4,            /* hydrogen */
  PINN_LO1, PINN_LO2, PINN_LO3, PINN_LO4,            /* oxygen */
  PINN_NLAMBDA = 17
};

/* ---- MinMaxScaler affine maps (host struct, passed by pointer, copied at call time) ----
 * x_phys = (x_n - x_min[c]) / x_scale[c]  : sklearn inverse_transform (01:542, 629, 726, 879)
 *   evaluated as two float64-operand steps each rounded to float32, like numpy does in place.
 * y likewise for the DNN output (01:735).  vn_scale / vn_min: the float32 pair train_lambda
 * builds at 01:1017-1022 to map the physics voltage back to normalised units. */
typedef struct pinn_affine {
  double x_min[8];
  double x_scale[8];
  double y_min;
  double y_scale;
  float vn_scale;
  float vn_min;
} pinn_affine_t;

/* ---- residual pass: net_f_V / net_f_T_simple / net_f_H / net_f_O  (01:724-765, 869-914,
 *      621-722, 535-619) + the stage losses mean(f^2) and their lambda gradients ---------- */
#define PINN_RES_V 1u
#define PINN_RES_T 2u
#define PINN_RES_H 4u
#define PINN_RES_O 8u
#define PINN_RES_ALL 15u

/* per-row output columns (column-major: d_cols[c * ld + row]) */
enum {
  PINN_C_FV = 0, PINN_C_VACT, PINN_C_VOHM, PINN_C_VCONC, PINN_C_ENERNST, PINN_C_VEST5, PINN_C_I, PINN_C_VOUT5,
  PINN_C_FT, PINN_C_TPRED, PINN_C_TOUT,
  PINN_C_FH, PINN_C_ACTH, PINN_C_TGTH, PINN_C_ITOT,
  PINN_C_FO, PINN_C_ACTO, PINN_C_TGTO, PINN_C_QO2, PINN_C_O2FLOW,
  PINN_NCOLS = 20
};

/* reduced sums (double[PINN_NSUMS], sums over rows -- divide by the GLOBAL row count) */
enum {
  PINN_S_FV2 = 0, PINN_S_FV_D1, PINN_S_FV_D2, PINN_S_FV_D3, /* sum f_V^2, sum f_V * df_V/dlambda_k        */
  PINN_S_YV2, PINN_S_YV_D1, PINN_S_YV_D2, PINN_S_YV_D3,     /* sum (y-Vn)^2, sum (y-Vn) * df_V/dlambda_k   */
  PINN_S_YU2,                                               /* sum (y-u)^2  (data loss, 01:1033)           */
  PINN_S_FT2, PINN_S_FT_D1, PINN_S_FT_D3, PINN_S_FT_D5, PINN_S_FT_ABS,
  PINN_S_FH2, PINN_S_FH_D1, PINN_S_FH_D2, PINN_S_FH_D3, PINN_S_ACTH, PINN_S_TGTH,
  PINN_S_FO2, PINN_S_FO_D1, PINN_S_FO_D2, PINN_S_FO_D3, PINN_S_ACTO, PINN_S_TGTO,
  PINN_NSUMS = 32
};

/* Workspace (bytes) pinn_residuals needs for its per-workgroup partial sums. */
size_t pinn_residuals_workspace_bytes(void);

/* One pass over n_rows normalised rows.
 *   d_x      [n_rows, 8] row-major float32 (normalised inputs)
 *   d_u      [n_rows] DNN mean output, normalised (needed iff flags & PINN_RES_V), else NULL
 *   d_y      [n_rows] normalised target or NULL (then the YV / YU sums are 0)
 *   d_lambda [17] float32
 *   d_cols   NULL, or PINN_NCOLS columns of leading dimension ld >= n_rows
 *   d_sums   NULL, or double[PINN_NSUMS]: overwritten with this call's sums (deterministic:
 *            per-workgroup partials in d_work, then a fixed-order final reduction)
 */
int pinn_residuals(const float* d_x, const float* d_u, const float* d_y, const pinn_affine_t* aff,
                   const float* d_lambda, unsigned flags, long long n_rows,
                   float* d_cols, long long ld, double* d_sums, void* d_work, size_t work_bytes,
                   void* stream);

/* ---- physics-parameter stage step: grads from sums -> Adam -> clamp (01:1036-1047 and the
 *      three sibling trainers).  Runs on the device so a stage needs no host round trip. ---- */
enum { PINN_STAGE_LAMBDA_PM = 0, /* train_lambda(dnn_para=False): loss mean((y-Vn)^2)+mean((y-u)^2) */
       PINN_STAGE_LAMBDA_F = 1,  /* train_lambda(dnn_para=True):  loss mean(f_V^2)+mean((y-u)^2)    */
       PINN_STAGE_THERMAL = 2, PINN_STAGE_HYDROGEN = 3, PINN_STAGE_OXYGEN = 4 };

/* d_adam: float[2*17] first/second moments (caller zeroes at stage start), d_loss: float[2]
 * (total, physics) written for logging.  `step` is the 1-based Adam step of this stage,
 * `lr` the StepLR-scheduled rate of this epoch, n_global the global row count. */
int pinn_lambda_step(int stage, const double* d_sums, long long n_global, float vn_scale,
                     float lr, int step, float* d_lambda, float* d_adam, float* d_loss, void* stream);

/* ---- a whole physics-parameter stage in ONE launch (01:999-1055, 1098-1151, 1191-1274, 1344-1391).
 * n_iters iterations, epochs first_epoch .. first_epoch + n_iters - 1, of: residual pass (exactly one of the PINN_RES_*
 * flags, and the one of `stage`: PINN_RES_V with PINN_STAGE_LAMBDA_PM / _F, PINN_RES_T / _H / _O with PINN_STAGE_THERMAL /
 * _HYDROGEN / _OXYGEN; any other pair is PINN_E_ARG) over all n_rows rows -> gradients of the stage's scalars -> Adam(lr = lr0 * gamma^(epoch / lr_step), the
 * StepLR schedule) -> clamp; the arithmetic of pinn_residuals + pinn_lambda_step, run by a single persistent
 * workgroup, so an iteration costs no launch.  For one process holding ALL rows (n_global == n_rows) and
 * n_rows <= PINN_STAGE_RUN_MAX_ROWS; larger or sharded series iterate the two calls above.
 * d_adam as in pinn_lambda_step (carried across calls); d_loss float[2] of the last iteration; d_log: NULL, or
 * float[n_logged][PINN_STAGE_LOG_FLOATS] with one row per epoch divisible by log_every (first_epoch must be):
 * [0] total loss, [1] physics loss, [2] lr of the following epoch, [3..19] the 17 parameters after the step,
 * [20..51] the PINN_NSUMS sums of that epoch (float); d_sums: NULL or double[PINN_NSUMS] of the last iteration. */
#define PINN_STAGE_RUN_MAX_ROWS 65536
#define PINN_STAGE_LOG_FLOATS 64
int pinn_lambda_stage_run(int stage, unsigned flags, const float* d_x, const float* d_u, const float* d_y, const pinn_affine_t* aff,
                          long long n_rows, double lr0, double gamma, int lr_step, int first_epoch, int n_iters, float* d_lambda,
                          float* d_adam, float* d_loss, float* d_log, int log_every, double* d_sums, void* d_work, size_t work_bytes,
                          void* stream);
size_t pinn_lambda_stage_workspace_bytes(long long n_rows);   /* d_work: the rows' parameter-independent terms, computed once per call */

/* The same split for any row count and for row shards (one process per GPU): within one trainer call x, u (the eval forward)
 * and y are fixed, so everything of a row that does not depend on the stage's parameters -- the float64 de-normalisation,
 * powf / expf of the Nernst terms, the flow ratios (A4-A7's parameter-free half) -- is computed once into d_cache
 * (float[6 * n_rows], i.e. pinn_lambda_stage_workspace_bytes(n_rows)) by pinn_residuals_prepare; every iteration then is
 * pinn_residuals_cached (8-24 B/row read) -> [all-reduce of d_sums] -> pinn_lambda_step.  flags: exactly one PINN_RES_*;
 * d_sums / d_work as for pinn_residuals (same sums, same layout; sums of other stages are 0). */
int pinn_residuals_prepare(const float* d_x, const float* d_u, const float* d_y, const pinn_affine_t* aff,
                           const float* d_lambda, unsigned flags, long long n_rows, float* d_cache, void* stream);
int pinn_residuals_cached(const float* d_cache, const pinn_affine_t* aff, const float* d_lambda, unsigned flags,
                          long long n_rows, double* d_sums, void* d_work, size_t work_bytes, void* stream);

/* net_f_T (01:767-867): the Euler energy-balance thermal model, row t-1 -> t, one fused pass (HBM-bound: 36 B/row read,
 * 12 B/row written).  d_u = the DNN's eval-mode output on the same rows (normalised units; row t uses u[t-1], as the
 * reference runs the net on X[:-1]).  Row 0 of the series has no predecessor: T_pred = T_out (01:857).  Under row
 * sharding a rank passes the LAST row of the previous shard (8 floats) and its DNN output (1 float) as d_x_halo /
 * d_u_halo (device pointers; both NULL on the shard that starts the series) -- a one-row halo, no collective.
 * Outputs: the three tuple elements (f_T = T_out - T_pred, T_pred, T_out), float[n_rows] each.  Reads lambda_T1..T4. */
int pinn_net_f_t(const float* d_x, const float* d_u, const float* d_x_halo, const float* d_u_halo, const pinn_affine_t* aff,
                 const float* d_lambda, long long n_rows, float* d_f, float* d_t_pred, float* d_t_real, void* stream);

/* ---- vector-Jacobian products of the two residual passes (torch autograd's backward) ------------------------------
 * Nothing is saved between forward and backward: each call recomputes every row's terms from d_x, d_u and d_lambda with the
 * forward's arithmetic and back-propagates them with torch's derivative rules (clamp: inclusive masks; where: nothing through
 * the condition; abs: sign; rows where the forward is NaN give NaN where torch's autograd does).  Gradients are with respect to
 * the NORMALISED inputs (chain rule through x_phys = (x_n - x_min) / x_scale and the y map of u).
 * d_glambda float[17]: the SUM over the local rows of the parameter gradients (0 for the parameters the columns do not read);
 * under row sharding the caller all-reduces it.  Deterministic: wave64 shuffles -> LDS -> one float64 partial per workgroup
 * in d_work (pinn_residuals_workspace_bytes()) -> a fixed-order final reduction; no floating-point atomics.
 * d_gu [n_rows] and d_gx [n_rows, 8] (16-byte aligned, like d_x): per row, overwritten; NULL = not computed.
 *
 * pinn_residuals_backward: pinn_residuals' per-row columns.  d_g holds upstream gradients column-major, d_g[c * ld + row],
 * for the columns c whose bit (1u << c) is set in gmask (absent columns are not read and contribute nothing); gmask may only
 * name columns of the models in `flags`.  d_u as for pinn_residuals (needed iff flags & PINN_RES_V); d_gu is d/d u. */
int pinn_residuals_backward(const float* d_x, const float* d_u, const pinn_affine_t* aff, const float* d_lambda, unsigned flags,
                            long long n_rows, const float* d_g, long long ld, unsigned gmask, float* d_glambda, float* d_gu,
                            float* d_gx, void* d_work, size_t work_bytes, void* stream);
/* pinn_net_f_t_backward: upstream gradients of its three outputs f_T, T_pred, T_out (float[n_rows] each, NULL = absent).
 * Row t's step feeds x[t-1] and u[t-1] (so d_gu[n_rows-1] = 0); d_gx also holds each row's own T_out terms.  With a halo
 * (d_x_halo, d_u_halo as for pinn_net_f_t), d_gx_halo [8] (16-byte aligned) / d_gu_halo [1] receive the gradient of the
 * previous shard's last row from this shard's first step (NULL = not computed; a row-sharded caller adds them to that row).
 * d_glambda holds lambda_T1..T4 (everything else 0). */
int pinn_net_f_t_backward(const float* d_x, const float* d_u, const float* d_x_halo, const float* d_u_halo, const pinn_affine_t* aff,
                          const float* d_lambda, long long n_rows, const float* d_gf, const float* d_gt_pred, const float* d_gt_real,
                          float* d_glambda, float* d_gu, float* d_gx, float* d_gx_halo, float* d_gu_halo, void* d_work,
                          size_t work_bytes, void* stream);

/* ---- the network ------------------------------------------------------------------------
 * Architecture [n_in=8, hidden x n_hidden, 1] + variance head hidden -> hidden/2 -> hidden/4 -> 1
 * (01:389-438).  Parameters live in ONE flat float32 device buffer in state_dict order,
 * each tensor in torch layout [out, in] row-major:
 *   W_0 b_0 ... W_{h-1} b_{h-1}  W_p b_p  Wv_0 bv_0  Wv_1 bv_1  Wv_2 bv_2
 * The fused kernels support hidden in {128, 256} (hidden % 128 == 0, <= 256), 1 <= n_hidden <= 8.
 */
#define PINN_PREC_FP32 0  /* exact fp32 matrix math (v_mfma_f32_*_f32); parity with the reference at fp32 tolerance */
#define PINN_PREC_BF16 1  /* bf16 MFMA inputs, fp32 accumulate / activations / loss / master weights (rtol ~2e-2)    */
#define PINN_PREC_F32X6 2 /* fp32-ACCURATE matrix math on the 16-bit matrix cores from split operands, fp32 accumulation; same
                             tolerances as PINN_PREC_FP32, 2-3x faster.  Every product -- forward,
                             MC-dropout, backward chain, weight gradients -- from two fp16 parts per operand, three MFMAs
                             (gradients under exact power-of-two scales: per row in the backward chain, one per call in the
                             weight gradients); gradient tensors come out as close to a float64 autograd as torch's own fp32
                             autograd does.  Wide nets (layer-by-layer kernels): the same schemes.  What the Python
                             surface uses by default.  (The name is round 1's, when every product took six MFMAs.) */
#define PINN_PREC_F32X6_G6 3 /* as F32X6 with the gradients (backward chain, weight gradients) from three bf16 parts per operand,
                                six MFMAs per product: 24-bit operands and fp32's full exponent range for every element
                                (F32X6's weight gradients keep full relative precision down to 2^-29 of the call's largest
                                d pre-activation, an absolute 2^-36 of it below).  ~20 % slower; the conservative choice. */

typedef struct pinn_net {
  int n_in;       /* 8 */
  int hidden;     /* H */
  int n_hidden;   /* number of H-wide hidden layers (3 in the reference, 01:2139) */
  int precision;  /* PINN_PREC_* */
  void* d_packed; /* every precision but PINN_PREC_FP32: device scratch of pinn_packed_bytes(net) bytes; every call re-packs the
                     bf16 weight copies from d_params into it (stateless), NULL for fp32 */
} pinn_net_t;

size_t pinn_packed_bytes(const pinn_net_t* net);             /* 0 for fp32 / unsupported shapes */

/* Domain of PINN_PREC_F32X6 / _G6 (the fp32 reference has no such limit; PINN_PREC_FP32 and _BF16 neither): the matrix
 * operands are fp16 parts under fixed power-of-two scales, so every weight of the hidden x hidden and variance-head
 * matrices must satisfy |w| < 1023.5 (fp16(64 w) finite), and the row-normalised gradients of PINN_PREC_F32X6's backward
 * chain must stay below 65504 (they do while 16 x the column abs-sums of those matrices do).  Outside it the kernels
 * produce inf / NaN -- never silently wrong finite numbers -- and record the fact in d_packed: every call that packs the
 * weights rewrites the record, pinn_mlp_train_grads adds its gradient check.  This query reads it back: it WAITS for
 * `stream` (the one entry point that synchronises) and returns PINN_OK, PINN_E_RANGE, or an argument / HIP error.
 * Call it where the host synchronises anyway (logging, fetching results); on PINN_E_RANGE switch the net to PINN_PREC_FP32. */
int pinn_net_range_status(const pinn_net_t* net, void* stream);

long long pinn_param_count(const pinn_net_t* net);          /* floats in the flat buffer, <0 on error */

/* dropout source */
enum { PINN_DROP_NONE = 0,   /* eval mode: identity                                              */
       PINN_DROP_PHILOX = 1, /* on-chip Philox4x32-10, keyed (seed, stream, global row, layer, f) */
       PINN_DROP_BITS = 2 }; /* injected bit-packed keep-masks (parity tests)         */

typedef struct pinn_dropout {
  int mode;
  float p[9];                 /* drop probability of dropout module l (hidden 0..n_hidden-1, then var head) */
  unsigned long long seed;    /* PHILOX */
  unsigned stream;            /* PHILOX: optimizer step / first pass index */
  long long row_offset;       /* global index of local row 0 (data-parallel shards) */
  const unsigned* d_bits;     /* BITS: [n_passes][n_rows][words] uint32, bit f of module l at
                                 word offset l*(H/32) (+ f/32), words = n_hidden*H/32 + H/64 */
  unsigned* d_step_counter;   /* NULL, or (pinn_mlp_train_grads on the fused nets, hidden <= 256) a device counter of completed
                                 optimizer steps: the call draws PHILOX stream `stream + *d_step_counter` (BITS: pass
                                 *d_step_counter of d_bits) and adds 1 to the counter when its gradients are final -- so ONE
                                 captured launch sequence (a hipGraph) can be replayed step after step; see pinn_adam_step_dev */
} pinn_dropout_t;

/* DNN.forward (01:421-438): d_u, d_logvar [n_rows]. */
int pinn_mlp_forward(const pinn_net_t* net, const float* d_params, const float* d_x, long long n_rows,
                     const pinn_dropout_t* drop, float* d_u, float* d_logvar, void* stream);

/* get_MC_samples (01:1413-1491) as one persistent launch: 1 eval pass + T stochastic passes
 * per row tile, reduced on chip.  d_pred_mean, d_a_u, d_e_u [n_rows] (normalised units). */
int pinn_mc_dropout(const pinn_net_t* net, const float* d_params, const float* d_x, long long n_rows,
                    const pinn_dropout_t* drop, int n_passes,
                    float* d_pred_mean, float* d_a_u, float* d_e_u, void* stream);

/* train_dnn forward + aleatoric_loss + backward (01:949-953) on a row shard.
 *   d_grads  [pinn_param_count] : SUM over local rows of d(loss_row)/dparam, already divided by
 *            n_global (so an all-reduce(SUM) over shards gives the full-batch gradient)
 *   d_loss   double[4]: sum_rows nll term, sum |logvar|, sum (y-u)^2, (spare) -- raw sums
 *   workspace from pinn_train_workspace_bytes(net, n_rows); d_grads and d_work 16-byte aligned (PINN_E_ARG otherwise)
 */
size_t pinn_train_workspace_bytes(const pinn_net_t* net, long long n_rows);
int pinn_mlp_train_grads(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y,
                         long long n_rows, long long n_global, const pinn_dropout_t* drop,
                         float* d_grads, double* d_loss, void* d_work, size_t work_bytes, void* stream);

/* The same call restricted to a subset of its kernel launches, so a benchmark can bracket one
 * kernel with events (bench.py's roofline leg).  phases = PINN_PHASE_ALL is pinn_mlp_train_grads.  Calls that together cover
 * every phase, in dependency order and on one workspace, give PINN_PHASE_ALL's result bit for bit. */
#define PINN_PHASE_CHAIN 1u   /* forward + loss + backward chain kernel (writes the activation stash) */
#define PINN_PHASE_WGRAD 2u   /* the per-layer weight-gradient kernels (read the stash)              */
#define PINN_PHASE_REDUCE 4u  /* fixed-order slab reduction -> d_grads, d_loss                       */
#define PINN_PHASE_ALL 7u
/* PINN_PREC_F32X6 / _G6 on the fused nets (hidden <= 256): the chain is two kernels, forward (+ loss) and backward; either
 * alone (the other precisions and the wide nets treat these two bits like PINN_PHASE_CHAIN) */
#define PINN_PHASE_CHAIN_FWD 8u
#define PINN_PHASE_CHAIN_BWD 16u
/* Two-part form of the weight-gradient and reduction phases, for overlapping the data-parallel all-reduce with the rest of
 * the step: the flat gradient splits at pinn_grad_split(net) floats into a HEAD [0, split) -- the input layer and every hidden
 * layer but the last -- and a TAIL [split, n) -- the last hidden layer, the predict head and the variance head, whose d
 * pre-activations the backward chain finishes first.  _TAIL / _HEAD run the weight-gradient kernels (the slab reduction) of
 * that part only; PINN_PHASE_WGRAD / _REDUCE are both parts.  pinn_grad_split is 0 (everything is "tail") where the
 * precision's kernels do not split (PINN_PREC_BF16 on the fused nets). */
#define PINN_PHASE_WGRAD_TAIL 32u
#define PINN_PHASE_WGRAD_HEAD 64u
#define PINN_PHASE_REDUCE_TAIL 128u
#define PINN_PHASE_REDUCE_HEAD 256u
long long pinn_grad_split(const pinn_net_t* net);
int pinn_mlp_train_grads_phases(const pinn_net_t* net, const float* d_params, const float* d_x, const float* d_y,
                                long long n_rows, long long n_global, const pinn_dropout_t* drop,
                                float* d_grads, double* d_loss, void* d_work, size_t work_bytes, void* stream,
                                unsigned phases);

/* torch.optim.Adam defaults (01:939): flat vectors of n floats; step is 1-based. */
int pinn_adam_step(float* d_params, const float* d_grads, float* d_m, float* d_v, long long n,
                   float lr, int step, void* stream);

/* The same step with its two scalars read on the DEVICE, for a captured (hipGraph) training step that is replayed with
 * nothing but device state changing (train_dnn at the reference's data sizes is launch-bound: 01:939-955, 12 002 steps of
 * ~1e4 rows).  d_coeffs: float[2 * n_steps], entry k = the coefficients of step k + 1 as pinn_adam_coeffs gives them (the host
 * arithmetic of pinn_adam_step, so both paths are bit-identical); d_step_counter: the counter pinn_mlp_train_grads advanced
 * (pinn_dropout_t.d_step_counter): this call applies entry *d_step_counter - 1. */
void pinn_adam_coeffs(float lr, int step, float* step_size, float* bc2_sqrt);      /* host only */
int pinn_adam_step_dev(float* d_params, const float* d_grads, float* d_m, float* d_v, long long n,
                       const float* d_coeffs, const unsigned* d_step_counter, void* stream);

/* pinn_mlp_train_grads + pinn_adam_step_dev as one launch sequence with the optimizer step applied by the gradient reduction's
 * own launch: one full train_dnn step (01:949-954) with nothing but device state changing, for capture and replay.  Arguments
 * as for the two calls (drop->d_step_counter is required; d_params is updated in place; d_grads receives the gradients the
 * step applied).  Bit-identical to the two calls.  PINN_PREC_F32X6 / _G6 on the fused nets (hidden <= 256), PINN_E_ARCH otherwise. */
int pinn_mlp_train_step_dev(const pinn_net_t* net, float* d_params, const float* d_x, const float* d_y,
                            long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads,
                            double* d_loss, void* d_work, size_t work_bytes, float* d_m, float* d_v,
                            const float* d_coeffs, void* stream);
/* The same with the step's two scalars by value (pinn_adam_step's lr and 1-based step): pinn_mlp_train_grads + pinn_adam_step
 * as one launch sequence for callers that launch step by step.  Bit-identical to the two calls.  Every precision and width. */
int pinn_mlp_train_step(const pinn_net_t* net, float* d_params, const float* d_x, const float* d_y,
                        long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads,
                        double* d_loss, void* d_work, size_t work_bytes, float* d_m, float* d_v, float lr, int step,
                        void* stream);

/* ---- any layers list: exact-fp32 layer-by-layer kernels (pinn_general.hip) -----------------------------------------
 * The entry points above run [8, H x k, 1] with one width H.  These run the reference's DNN(p, logvar, layers) (01:389-438) for
 * any layers = [8, h_1, ..., h_k, 1]: 1 <= k <= 8 hidden layers of widths 1 <= h_i <= 2048 (unequal widths allowed), the last
 * one h_k >= 4; the variance head is h_k -> h_k // 2 -> h_k // 4 -> 1 (floor division, 01:412-419).  n_in = 8 (the physics
 * residuals read 8 fixed columns) and n_out = 1; anything else is PINN_E_ARCH.
 * Flat layout: the reference's tensors in state_dict order, each torch [out, in] row-major and starting on a 16-byte boundary:
 *   W_0 [h_1, 8] b_0  W_1 [h_2, h_1] b_1 ...  W_p [1, h_k] b_p  Wv_0 [h_k/2, h_k] bv_0  Wv_1 [h_k/4, h_k/2] bv_1  Wv_2 [1, h_k/4] bv_2
 * (for equal widths this is pinn_param_count's layout).
 * Dropout modules: l = 0 .. k-1 after hidden layer l, l = k after Wv_0.  Philox: the same stream as every other kernel, keyed
 * (seed, stream + pass, global row, module, feature), 16-bit threshold round(65536 p); PINN_DROP_BITS: bit f & 31 of word
 * word_l + f / 32 of a row, word_l = sum_{j<l} ceil(w_j / 32) over w = (h_1, ..., h_k, h_k / 2), words per row = the total.
 * d_step_counter must be NULL (these nets run launch by launch).
 * Arithmetic: exact fp32 (v_mfma_f32_16x16x4_f32, a k-ordered fmaf chain); no range limit, no packed copies in the net.  Widths
 * are padded to 32 inside the workspace only.  Deterministic: no floating-point atomics; a row's forward / MC result does not
 * depend on the rows around it; two identical calls are bitwise equal.  The workspace (16-byte aligned) holds padded weight
 * copies and one bounded chunk of activations: pinn_gnet_workspace_bytes(net, n_rows, n_passes) is enough for forward and
 * train_grads on n_rows rows and, with n_passes > 0, for MC-dropout with n_passes passes. */
typedef struct pinn_gnet {
  int n_in;         /* 8 */
  int n_hidden;     /* k */
  int width[8];     /* h_1 .. h_k (entries past k ignored) */
  int n_out;        /* 1 */
  int reserved;     /* 0 */
} pinn_gnet_t;

long long pinn_gnet_param_count(const pinn_gnet_t* net);             /* floats in the flat buffer; < 0: PINN_E_ARCH / PINN_E_ARG */
size_t pinn_gnet_workspace_bytes(const pinn_gnet_t* net, long long n_rows, int n_passes);   /* 0 for an unsupported net */
/* as pinn_mlp_forward */
int pinn_gnet_forward(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows, const pinn_dropout_t* drop,
                      float* d_u, float* d_logvar, void* d_work, size_t work_bytes, void* stream);
/* as pinn_mc_dropout: 1 eval pass + n_passes stochastic passes (PHILOX stream `stream + t`, BITS pass t), processed as virtual rows
 * (pass, row); per row the moments of pinn_mc_dropout in pass order */
int pinn_gnet_mc_dropout(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows, const pinn_dropout_t* drop,
                         int n_passes, float* d_pred_mean, float* d_a_u, float* d_e_u, void* d_work, size_t work_bytes, void* stream);
/* as pinn_mlp_train_grads: d_grads [pinn_gnet_param_count] already divided by n_global, d_loss double[4] raw sums
 * (nll, |logvar|, (y-u)^2, sum dL/du) */
int pinn_gnet_train_grads(const pinn_gnet_t* net, const float* d_params, const float* d_x, const float* d_y, long long n_rows,
                          long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss, void* d_work,
                          size_t work_bytes, void* stream);
/* pinn_gnet_train_grads + pinn_adam_step (lr, 1-based step by value), like pinn_mlp_train_step */
int pinn_gnet_train_step(const pinn_gnet_t* net, float* d_params, const float* d_x, const float* d_y, long long n_rows,
                         long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss, void* d_work,
                         size_t work_bytes, float* d_m, float* d_v, float lr, int step, void* stream);
/* Vector-Jacobian product of pinn_gnet_forward (torch autograd's backward).  Recomputes the forward of rows [0, n_rows) with
 * `drop` -- the struct the forward used (PHILOX stream / row_offset, or BITS d_bits of the pass); NULL = eval -- and
 * back-propagates d_gu[r] = dL/du_r and d_glv[r] = dL/dlogvar_r (d_glv NULL: zero).
 * d_grads [pinn_gnet_param_count]: sum over the rows, NOT normalised, overwritten, padding zero (state_dict layout).
 * d_gx [n_rows, 8] = dL/dx (NULL: not computed).  Workspace: pinn_gnet_workspace_bytes(net, n_rows, 0).
 * Deterministic: no floating-point atomics; a row's d_gx does not depend on its tile, chunk or neighbours. */
int pinn_gnet_backward(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows,
                       const pinn_dropout_t* drop, const float* d_gu, const float* d_glv, float* d_grads, float* d_gx,
                       void* d_work, size_t work_bytes, void* stream);

/* Double backward of pinn_gnet_forward: the gradient of S = <v, dL/dx> = sum_r sum_i d_vx[r][i] * d_gx[r][i], where d_gx is what
 * pinn_gnet_backward returns for (d_gu, d_glv), with respect to the parameters, x, g_u and g_lv (torch autograd's backward of a
 * backward taken under create_graph=True, through dL/dx only).  Recomputes the forward and its tangent along v with `drop`, the
 * struct the forward used.  d_vx [n_rows, 8] is required; d_glv NULL: zero.  Each output may be NULL and is then not computed:
 * d_grads [pinn_gnet_param_count] = dS/dtheta, raw sums over the rows, overwritten, padding zero (state_dict layout; the
 * predict bias entry is exactly 0); d_gx [n_rows, 8] = dS/dx; d_ggu, d_gglv [n_rows] = dS/dg_u, dS/dg_lv.
 * n_rows == 0: nothing runs but d_grads (if given) is zeroed.  Workspace: pinn_gnet_backward2_workspace_bytes(net, n_rows)
 * (0 for an unsupported net).  Deterministic like pinn_gnet_backward: a row's d_gx, d_ggu, d_gglv do not depend on its tile,
 * chunk or neighbours. */
size_t pinn_gnet_backward2_workspace_bytes(const pinn_gnet_t* net, long long n_rows);
int pinn_gnet_backward2(const pinn_gnet_t* net, const float* d_params, const float* d_x, long long n_rows,
                        const pinn_dropout_t* drop, const float* d_gu, const float* d_glv, const float* d_vx,
                        float* d_grads, float* d_gx, float* d_ggu, float* d_gglv, void* d_work, size_t work_bytes, void* stream);

/* ---- deep ensembles: n_members equal networks in the launches of one (pinn_general.hip) ---------------------------
 * n_members copies of one pinn_gnet_t, 1 <= n_members <= 32 (PINN_E_ARG otherwise), on the same rows d_x (and targets d_y): every
 * kernel of the pinn_gnet_* forward and training step takes the member from its launch grid, so a call is as many launches as
 * one network's.  d_params, d_grads, d_m, d_v: [n_members, pinn_gnet_param_count(net)] contiguous (the count is a multiple of 4
 * floats, so every member starts 16-byte aligned); d_u, d_logvar: [n_members, n_rows]; d_loss: double [n_members][4].
 * Member m of a call is bit for bit the pinn_gnet_* call on member m's slices with drop->seed + m (64-bit wrap) for the seed and
 * everything else of `drop` as given: a member's chunks, weight-gradient slices and fixed-order sums are those of the single
 * network at this n_rows, whatever n_members is.  drop: NULL / PINN_DROP_NONE or PINN_DROP_PHILOX; PINN_DROP_BITS and a
 * non-NULL d_step_counter are PINN_E_ARG.  No floating-point atomics.
 * Checks as pinn_gnet_*: NULL or misaligned pointers PINN_E_ARG, a workspace (16-byte aligned) below
 * pinn_gens_workspace_bytes(net, n_members, n_rows) PINN_E_WORKSPACE, a bad net PINN_E_ARCH, all before any launch;
 * n_rows == 0 returns PINN_OK and does nothing. */
size_t pinn_gens_workspace_bytes(const pinn_gnet_t* net, int n_members, long long n_rows);   /* 0: unsupported net, bad argument */
/* what fixes the order of a member's training sums at n_rows rows: the rows of a chunk and the weight-gradient slices of a chunk */
int pinn_gens_train_plan(const pinn_gnet_t* net, long long n_rows, long long* chunk_rows, int* slices);
/* as pinn_gnet_forward, per member */
int pinn_gens_forward(const pinn_gnet_t* net, int n_members, const float* d_params, const float* d_x, long long n_rows,
                      const pinn_dropout_t* drop, float* d_u, float* d_logvar, void* d_work, size_t work_bytes, void* stream);
/* as pinn_gnet_train_grads, per member: each member's gradient divided by n_global and its four raw loss sums */
int pinn_gens_train_grads(const pinn_gnet_t* net, int n_members, const float* d_params, const float* d_x, const float* d_y,
                          long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss,
                          void* d_work, size_t work_bytes, void* stream);
/* pinn_gens_train_grads + one pinn_adam_step over all n_members * pinn_gnet_param_count elements (Adam is elementwise) */
int pinn_gens_train_step(const pinn_gnet_t* net, int n_members, float* d_params, const float* d_x, const float* d_y,
                         long long n_rows, long long n_global, const pinn_dropout_t* drop, float* d_grads, double* d_loss,
                         void* d_work, size_t work_bytes, float* d_m, float* d_v, float lr, int step, void* stream);
/* The ensemble as a mixture, per row, members in index order, sums in double, each output rounded once to float32:
 *   pred_mean = mean_m u_m;  e_u = sqrt(max(mean_m u_m^2 - pred_mean^2, 0)) (population form; exactly 0 for equal members);
 *   rule 0: a_u = sqrt(exp(mean_m logvar_m)) (get_MC_samples' form);  rule 1: a_u = sqrt(mean_m exp(logvar_m)) (mixture variance).
 * d_u, d_logvar [n_members, n_rows]; outputs [n_rows].  Any other rule: PINN_E_ARG. */
int pinn_gens_combine(const float* d_u, const float* d_logvar, int n_members, long long n_rows, int rule, float* d_pred_mean,
                      float* d_a_u, float* d_e_u, void* stream);

/* ---- results assembly: create_comprehensive_results_array_v2 (01:1877-2010) -----------------------------------
 * Fills d_out = float64 [n_rows, 22] row-major (the `comprehensive_results` layout scripts 02-05 read):
 *   0-7 inputs and 8 target, de-normalised like sklearn's inverse_transform on float32 (aff->x_*, aff->y_*; 01:1916-1917);
 *   9 = (pred_mean - mc_min) / (mc_scale + 1e-12), 10 / 11 = a_u, e_u / (mc_scale + 1e-12) (float64, 01:1925-1936),
 *   each smoothed by a centred moving average of `window` rows with pandas' even-window semantics, separately inside
 *   every segment [d_seg_end[k-1], d_seg_end[k]) (ascending exclusive ends, the last == n_rows; n_segments == 0: one
 *   segment; 01:1830-1872, 01:1971-1986); 12 = col 8 - col 9; 13-16 = f_V, f_T, f_H2, f_O2; 17 = d_labels (NULL: 0);
 *   18-21 = 5*V_est, T_pred, H2 and O2 excess ratios -- taken from d_cols as pinn_residuals(PINN_RES_ALL) wrote them.
 * d_pred_mean / d_a_u / d_e_u: pinn_mc_dropout's outputs.  1 <= window <= 1024; d_x and d_out 16-byte aligned. */
int pinn_results_assemble(const float* d_x, const float* d_y, const pinn_affine_t* aff, double mc_min, double mc_scale,
                          int window, const long long* d_seg_end, int n_segments, const float* d_pred_mean,
                          const float* d_a_u, const float* d_e_u, const float* d_cols, long long ld,
                          const float* d_labels, long long n_rows, double* d_out, void* stream);

/* ---- risk function RF(t) and first alarm: reference script 04 (cited as 04:<line>) ---------------------------
 * All arrays are float64.  d_arr is row-major with leading dimension ld (the 22-column results array, or any array that
 * holds the residual columns); a column list col[] names the D <= 8 residual columns (04: res, pV, pT, pH, pO = 12..16).
 * Positions, rows and segment starts are 64-bit.  Results do not depend on the run: every reduction has a fixed order. */
#define PINN_RF_MAX_COLS 8
#define PINN_RF_MAX_LAYERS 4
#define PINN_RF_ABOVE 0      /* first position with series >= threshold */
#define PINN_RF_BELOW 1      /* first position with series <= threshold */

/* host struct, copied at call time */
typedef struct pinn_rf_params {
  int n_cols;                          /* D */
  int n_layers;                        /* <= 4 */
  int col[PINN_RF_MAX_COLS];           /* column of d_arr per residual */
  int layer_of[PINN_RF_MAX_COLS];      /* layer of each residual, -1: in no layer */
  double w[PINN_RF_MAX_COLS];          /* feature weights */
  double beta[PINN_RF_MAX_LAYERS];     /* layer weights, summed in layer order */
  double p_layer, z_safe, lambda_decay, k_logistic, c0_logistic, c_max, alpha_smooth;
} pinn_rf_params_t;

/* estimate_mu_sigma_normal (04:181-197): nanmean and nanstd(ddof=1) of the columns over the rows whose label column,
 * truncated to an integer, is one of normal_labels[n_normal] (host array, <= 8).  A NaN removes its row from its own
 * column only; sigma == 0 becomes 1e-6.  Two passes (mean, centred squares).  d_mu, d_sigma: [n_cols].  d_count (may be
 * NULL): long long [9], the values counted per column and, at [8], the normal rows.  cols: host array. */
size_t pinn_rf_stats_workspace_bytes(void);
int pinn_rf_stats(const double* d_arr, long long ld, long long n_rows, const int* cols, int n_cols, int label_col,
                  const long long* normal_labels, int n_normal, double* d_mu, double* d_sigma, long long* d_count,
                  void* d_ws, size_t ws_bytes, void* stream);

/* compute_rf_time_series (04:201-285) over n positions.  Position j reads row d_row_index[j] of d_arr (NULL: row j; an
 * index outside [0, n_arr_rows) reads nothing and gives a NaN row).  d_seg_start[n_segments]: strictly ascending
 * positions at which both recurrences restart, d_seg_start[0] == 0 (n_segments == 0: one segment).  d_carry_in (may be
 * NULL) and d_carry_out (may be NULL): [n_segments][2] = (C, RF_smooth) before the first / at the last position of every
 * segment.  Without carry-in C[first] = 0 (S_tot[first] unused, as the reference's loop starts at t = 1) and
 * RF_smooth[first] = RF_inst[first]; with it C[first] = lambda C_prev + S_tot[first] and RF_smooth[first] =
 * alpha RF_inst[first] + (1 - alpha) RF_smooth_prev.  Outputs, each [n] and each may be NULL: d_S_tot, d_C, d_RF_inst,
 * d_RF_smooth; d_S_layers [n_layers][n].  n <= 2048 runs as one launch and needs no workspace (d_ws may be NULL,
 * pinn_rf_workspace_bytes returns 0); otherwise five launches, the workspace holding two [n] arrays and the tile sums. */
size_t pinn_rf_workspace_bytes(long long n_rows, long long n_segments);
int pinn_rf_series(const double* d_arr, long long ld, long long n_arr_rows, const pinn_rf_params_t* prm,
                   const double* d_mu, const double* d_sigma, const long long* d_row_index, long long n,
                   const long long* d_seg_start, long long n_segments, const double* d_carry_in, double* d_S_layers,
                   double* d_S_tot, double* d_C, double* d_RF_inst, double* d_RF_smooth, double* d_carry_out,
                   void* d_ws, size_t ws_bytes, void* stream);

/* Sweep of RF parameter sets (calibration): n_cand candidates over the same positions and segments in two launches.
 * The candidate table d_cand is [n_cand][PINN_RF_SWEEP_WORDS] float64 in device memory:
 *   0..7 w[d] | 8..11 beta[l] | 12 p_layer | 13 z_safe | 14 lambda_decay | 15 k_logistic | 16 c0_logistic |
 *   17 c_max | 18 alpha_smooth | 19 warn threshold | 20 danger threshold | 21..23 reserved, 0
 * Of `shape`, n_cols, n_layers, col[] and layer_of[] are read; the rest is ignored.  Per (candidate, segment) the result is
 * that of pinn_rf_series without carry-in on that segment followed by pinn_rf_first_alarm(PINN_RF_ABOVE) at the
 * candidate's two thresholds: C[first] = 0, RF_smooth[first] = RF_inst[first], NaN never matches and never enters the
 * peak, a gather index outside the array reads nothing.  Outputs, each [n_cand][n_segments] (n_segments == 0: one segment):
 * d_first_warn, d_first_danger (position from the segment's start, -1: none), d_n_warn (rows with RF_smooth >= warn),
 * d_peak (maximum of the non-NaN RF_smooth, NaN if there is none), d_carry_out (may be NULL) [..][2] = (C, RF_smooth) at
 * the segment's last row.  d_bad [n_cand]: 1 where any of a candidate's 24 words is not finite or its p_layer is 0; such a
 * candidate gets -1 / 0 / NaN and the call still returns PINN_OK.  n_cand >= 1 and n_cand * n_segments <= 2^31 - 1.  The
 * workspace holds z = (R - mu) / sigma as [n_cols][n] columns.  Nothing per row is written, no workgroup waits on
 * another, and two calls give the same bytes. */
#define PINN_RF_SWEEP_WORDS 24
size_t pinn_rf_sweep_workspace_bytes(long long n, int n_cols);
int pinn_rf_sweep(const double* d_arr, long long ld, long long n_arr_rows, const pinn_rf_params_t* shape,
                  const double* d_mu, const double* d_sigma, const long long* d_row_index, long long n,
                  const long long* d_seg_start, long long n_segments, const double* d_cand, long long n_cand,
                  long long* d_first_warn, long long* d_first_danger, long long* d_n_warn, double* d_peak,
                  double* d_carry_out, int* d_bad, void* d_ws, size_t ws_bytes, void* stream);

/* find_first_alarm_index (04:289-300) per segment: d_first[s] = the first position, counted from the segment's start, whose
 * value is >= (PINN_RF_ABOVE) or <= (PINN_RF_BELOW) the threshold, or -1.  NaN never matches.  Position j reads
 * d_series[row * stride] with row = d_row_index[j] (NULL: j).  relative != 0: the threshold of a segment is the value at
 * its first position plus `threshold` (04:389: V[0] - 0.1), read on the device. */
int pinn_rf_first_alarm(const double* d_series, long long stride, long long n_src_rows, const long long* d_row_index,
                        long long n, const long long* d_seg_start, long long n_segments, int mode, int relative,
                        double threshold, long long* d_first, void* stream);

/* ---- Gaussian-mixture fault diagnosis: reference script 03 (cited as 03:<line>) ---------------------------------
 * A full-covariance mixture of n_comp <= 32 components over n_feat <= 8 columns, float64 throughout.  Rows are read in
 * place: position j reads row d_row_index[j] of d_arr (NULL: row j; an index outside [0, n_arr_rows) reads nothing,
 * adds nothing to a sum and gives NaN outputs), columns cols[n_feat] (host array) of a row-major array with leading
 * dimension ld.  Every reduction has a fixed order: the same call gives the same bytes.
 *
 * The model lives in a device-resident state block of pinn_gmm_state_bytes() bytes, 8-byte words:
 *   [PINN_GMM_ST_ITER] iterations done, [.._CONVERGED] 1 once |change| < tol, [.._STATUS] 0 or PINN_GMM_SINGULAR,
 *   [.._K], [.._D] (64-bit integers); [.._LOWER] lower bound, [.._PREV] the one before, [.._CHANGE] their difference
 *   (doubles); then weights[K], means[K][D], covariances[K][D][D], precisions_cholesky[K][D][D] (upper triangular, as
 *   scikit-learn's attribute of that name), log-determinants of precisions_cholesky [K].
 * A caller may also fill the block itself (means_init / precisions_init, k-means centres).  Once CONVERGED or STATUS is
 * set, every later launch of pinn_gmm_em / pinn_gmm_kmeans returns at once and leaves the parameters untouched.  A
 * covariance that is not positive definite sets STATUS and is not stored: the block keeps the last good parameters.
 * After pinn_gmm_mstep_init and pinn_gmm_em the workspace begins with the summed moments of the last pass,
 * [K][1 + D + D (D + 1) / 2] = (sum r, sum r d_i, sum r d_i d_j for i <= j, by columns j) with d = x - the mean the pass
 * started from. */
#define PINN_GMM_MAX_COMP 32
#define PINN_GMM_MAX_FEAT 8
#define PINN_GMM_MAX_CLASSES 16
#define PINN_GMM_SINGULAR 1
#define PINN_GMM_ST_ITER 0
#define PINN_GMM_ST_CONVERGED 1
#define PINN_GMM_ST_STATUS 2
#define PINN_GMM_ST_K 3
#define PINN_GMM_ST_D 4
#define PINN_GMM_ST_LOWER 5
#define PINN_GMM_ST_PREV 6
#define PINN_GMM_ST_CHANGE 7

size_t pinn_gmm_state_bytes(int n_comp, int n_feat);                       /* 0 for sizes outside the limits */
size_t pinn_gmm_workspace_bytes(long long n_rows, int n_comp, int n_feat);

/* scikit-learn's _initialize: parameters from responsibilities d_resp [n][n_comp] or from one label per position d_labels
 * (one-hot; exactly one of the two is non-NULL): n_k = sum r + 10 eps, means, covariances about them (two passes)
 * + reg_covar on the diagonal, weights n_k / n.  Resets the header (iterations 0, lower bound -inf). */
int pinn_gmm_mstep_init(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                        const long long* d_row_index, long long n, int n_comp, const double* d_resp,
                        const long long* d_labels, double reg_covar, double* d_state, void* d_ws, size_t ws_bytes,
                        void* stream);

/* n_iters EM iterations, two launches each and no host synchronisation: E-step with the state's parameters fused with
 * the moment sums, then the M-step (weights n_k / sum n_k), Cholesky, lower bound = mean log_prob_norm of that E-step,
 * and scikit-learn's test |lower bound - previous| < tol, which sets CONVERGED after the M-step of that iteration. */
int pinn_gmm_em(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                const long long* d_row_index, long long n, int n_comp, int n_iters, double tol, double reg_covar,
                double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* n_iters Lloyd iterations on the state's means as centres (nearest centre, the first of equals; an empty cluster keeps
 * its centre; CONVERGED once no centre moves; LOWER = inertia).  d_labels (may be NULL): the assignment to the final centres. */
int pinn_gmm_kmeans(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                    const long long* d_row_index, long long n, int n_comp, int n_iters, double* d_state, long long* d_labels,
                    void* d_ws, size_t ws_bytes, void* stream);

/* Label-posterior mapping (03:394-414): d_map [n_comp][n_classes] = sum over positions of responsibility x
 * one-hot(d_class[j]) (a class outside [0, n_classes) adds nothing), normalised per component; 1 / n_classes where a
 * component's sum is not positive.  n_classes <= 16. */
int pinn_gmm_label_map(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                       const long long* d_row_index, long long n, int n_comp, const double* d_state, const long long* d_class,
                       int n_classes, double* d_map, void* d_ws, size_t ws_bytes, void* stream);

/* One launch.  Outputs, each may be NULL: d_log_prob_norm [n] (score_samples), d_resp [n][n_comp] (predict_proba) and,
 * with d_map [n_comp][n_classes]: d_y_prob [n][n_classes] = clip(resp @ map, 1e-12, 1) renormalised (03:418-421) and
 * d_y_pred [n] its first maximum. */
int pinn_gmm_posterior(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                       const long long* d_row_index, long long n, int n_comp, const double* d_state, const double* d_map,
                       int n_classes, double* d_log_prob_norm, double* d_resp, double* d_y_prob, long long* d_y_pred,
                       void* stream);

/* ---- batches of mixtures: model selection over component counts and seeds --------------------------------------
 * n_batch <= PINN_GMM_MAX_BATCH candidates are seeded, initialised, iterated and scored together over one row set (the row
 * head above), one tol and one reg_covar.  Candidate c has n_comp[c] components (host array, 1..max_comp, max_comp <= 32).
 * Its state block starts c * pinn_gmm_batch_state_stride(max_comp, n_feat) bytes into d_state and has exactly the
 * single-model layout for its own n_comp[c]: the block is a valid d_state of pinn_gmm_posterior / _label_map / _em.  Every
 * entry point is a fixed number of launches for the whole batch without a host synchronisation; the row passes run on a
 * grid of (row blocks, candidates), the M-steps with one workgroup per candidate, and both are the single model's code: a
 * candidate's bytes are those of the single-model calls and do not depend on what else is in the batch.  A candidate
 * whose CONVERGED or STATUS word is set is skipped by every later launch and keeps its parameters; a covariance that is
 * not positive definite sets that candidate's STATUS only.  n >= 1.  NULL or misaligned pointers, n_batch outside
 * 1..PINN_GMM_MAX_BATCH and an n_comp[c] outside 1..max_comp: PINN_E_ARG; a workspace below
 * pinn_gmm_batch_workspace_bytes(n, n_batch, max_comp, n_feat): PINN_E_WORKSPACE; both before any launch. */
#define PINN_GMM_MAX_BATCH 1024

size_t pinn_gmm_batch_state_stride(int max_comp, int n_feat);               /* bytes; 0 for sizes outside the limits */
size_t pinn_gmm_batch_workspace_bytes(long long n_rows, int n_batch, int max_comp, int n_feat);   /* likewise */

/* k-means++ seeds, one workgroup per candidate.  Zeroes the state blocks, writes their headers and the n_comp[c] centres
 * into the means.  Centre 0 is position d_first[c] (clamped to [0, n)); centre k is the first position whose inclusive
 * cumulative sum of the squared distance to the nearest centre so far exceeds d_u[c][k - 1] x total, n - 1 when none does
 * (numpy's searchsorted(side="right") clamped; a zero total picks n - 1).  d_u: [n_batch][max_comp - 1] uniforms in [0, 1)
 * (may be NULL when max_comp is 1).  The sum has a fixed order (256 contiguous chunks, then the chunk sums).  d_picks (may
 * be NULL): [n_batch][max_comp] the positions picked. */
int pinn_gmm_batch_seed(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                        const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp,
                        const long long* d_first, const double* d_u, double* d_state, long long* d_picks, void* d_ws,
                        size_t ws_bytes, void* stream);

/* pinn_gmm_kmeans per candidate: n_iters Lloyd iterations, then the assignment to the final centres, d_labels [n_batch][n]. */
int pinn_gmm_batch_kmeans(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                          const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp, int n_iters,
                          double* d_state, long long* d_labels, void* d_ws, size_t ws_bytes, void* stream);

/* pinn_gmm_mstep_init per candidate from its labels d_labels [n_batch][n]. */
int pinn_gmm_batch_mstep_init(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                              const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp,
                              const long long* d_labels, double reg_covar, double* d_state, void* d_ws, size_t ws_bytes,
                              void* stream);

/* pinn_gmm_em per candidate: n_iters iterations, two launches each for the whole batch. */
int pinn_gmm_batch_em(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                      const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp, int n_iters,
                      double tol, double reg_covar, double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* d_sum[c] = the sum of log_prob_norm over the row set under candidate c's parameters, in a fixed order (rows of a tile,
 * tiles of a workgroup, workgroups).  The row set need not be the one the candidates were fitted on. */
int pinn_gmm_batch_score(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                         const long long* d_row_index, long long n, int n_batch, const int* n_comp, int max_comp,
                         const double* d_state, double* d_sum, void* d_ws, size_t ws_bytes, void* stream);

/* ---- fault detection: reference script 02 (cited as 02:<line>) ---------------------------------------------------
 * StandardScaler + multinomial logistic regression with an L2 penalty (02:195-207) and the ROC curve / AUC of
 * 1 - P(normal) (02:552-557), float64 throughout.  Rows are read in place as for the mixture above (column list, optional
 * gather list, leading dimension; an index outside [0, n_arr_rows) reads nothing and adds nothing).  d_y holds one class
 * index per position; a class outside [0, n_classes) adds nothing.  Every reduction has a fixed order.
 *
 * Limits: 2 <= n_classes <= PINN_LR_MAX_CLASSES, 1 <= n_feat <= PINN_LR_MAX_FEAT and
 * n_classes (n_classes + 1) / 2 x (n_feat + 1) (n_feat + 2) / 2 <= PINN_LR_MAX_HESS (the Hessian sums of a row pass):
 * every (C, D) with C <= 5, D <= 8 and with C <= 13, D <= 4 is inside.  Outside: PINN_E_ARG, sizes 0.
 *
 * With z = (x - mean) / scale, s_c = W_c . z + b_c, sample weights sw = class_weight[y], the fit minimises
 *   F(W, b) = sum_i sw_i (logsumexp_c s_ic - s_i,y_i) + l2 / 2 sum_c |W_c|^2        (l2 = 1 / C of scikit-learn)
 * by damped Newton iterations.  The state block (pinn_lr_state_bytes() bytes, 8-byte words) holds the header
 *   [.._ITER] accepted iterations, [.._CONVERGED] 1 once max |grad F| / sum sw <= tol, [.._STATUS] 0 or PINN_LR_SINGULAR /
 *   _NAN / _STALLED, [.._C], [.._D], [.._PASSES] row passes judged, [.._PHASE] 0 until the first point is accepted,
 *   [.._NSEEN] rows counted by the scaler, [.._MAXITER] iterations after which every launch returns at once (64-bit
 *   integers); [.._F] F at the accepted point, [.._STEP] the step length of the proposed point, [.._DD] grad . direction at
 *   the accepted point, [.._GMAX] max |grad F| / sum sw there, [.._SWSUM] sum sw (doubles);
 * then theta [C][D + 1] (coefficients of a class, then its intercept: the point the next pass evaluates), the accepted
 * point, the Newton direction and the gradient at the accepted point (each [C][D + 1]), mean [D], scale [D], var [D],
 * class_weight [C], class_count [C] (64-bit integers).  The caller zeroes the block, writes the starting point into theta
 * and MAXITER, and calls pinn_lr_scaler (or fills mean / scale / class_weight / SWSUM itself).  Once CONVERGED or STATUS
 * is set or MAXITER is reached every later launch returns at once; a failed factorisation or a NaN stores nothing: theta
 * is the last accepted point. */
#define PINN_LR_MAX_CLASSES 13
#define PINN_LR_MAX_FEAT 8
#define PINN_LR_MAX_HESS 1365
#define PINN_LR_SINGULAR 1
#define PINN_LR_NAN 2
#define PINN_LR_STALLED 3
#define PINN_LR_ST_ITER 0
#define PINN_LR_ST_CONVERGED 1
#define PINN_LR_ST_STATUS 2
#define PINN_LR_ST_C 3
#define PINN_LR_ST_D 4
#define PINN_LR_ST_F 5
#define PINN_LR_ST_STEP 6
#define PINN_LR_ST_DD 7
#define PINN_LR_ST_PASSES 8
#define PINN_LR_ST_GMAX 9
#define PINN_LR_ST_SWSUM 10
#define PINN_LR_ST_PHASE 11
#define PINN_LR_ST_NSEEN 12
#define PINN_LR_ST_MAXITER 13
#define PINN_LR_ST_HEADER 16

size_t pinn_lr_state_bytes(int n_classes, int n_feat);                      /* 0 for sizes outside the limits */
size_t pinn_lr_workspace_bytes(long long n_rows, int n_classes, int n_feat);

/* StandardScaler.fit and the class weights, four launches: mean (pass 1), var = mean of (x - mean)^2 (pass 2), scale =
 * sqrt(var), 1 where scikit-learn takes the feature for constant; class counts; class_weight = n / (C count) with
 * balanced != 0, else 1; SWSUM, NSEEN, C, D. */
int pinn_lr_scaler(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                   const long long* d_row_index, long long n, const long long* d_y, int n_classes, int balanced,
                   double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* One row pass at the state's theta, whatever the header says; the state is not changed.  Afterwards the workspace begins
 * with the sums [1 + P + H]: the loss sum; the gradient sums [C][D + 1] of sw (p_c - y_c) (z, 1); the Hessian sums of
 * sw p_c (delta_cd - p_d) (z, 1)_i (z, 1)_j for c <= d (pairs by columns d) and i <= j (by columns j).  No penalty. */
int pinn_lr_pass(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                 const long long* d_row_index, long long n, const long long* d_y, int n_classes, const double* d_state,
                 void* d_ws, size_t ws_bytes, void* stream);

/* n_passes times (row pass at theta, one-workgroup judgement), no host synchronisation.  The judgement accepts the point
 * (the first one always; later ones by Armijo's rule F <= F_acc + 1e-4 step DD, with a floor of 4 n eps loss for the
 * rounding of the sum), or restores the accepted point with half the step.  After accepting it tests the tolerance,
 * factorises the Hessian (Cholesky; + sum sw / C on every pair of intercepts, which pins their sum) and proposes the
 * Newton step.  fit_intercept == 0 leaves the intercepts where they start. */
int pinn_lr_newton(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                   const long long* d_row_index, long long n, const long long* d_y, int n_classes, int n_passes, double tol,
                   double l2, int fit_intercept, double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* One launch.  d_model: mean [D], scale [D], W [R][D], b [R] with R = 1 for two classes (scikit-learn's coef_ [1, D]:
 * the scores are (-d, d)) and R = n_classes otherwise.  Outputs, each may be NULL: d_decision [n] (two classes) or
 * [n][n_classes], d_proba [n][n_classes] = softmax of the scores, d_pred [n] the first maximum, d_p_fault [n] =
 * 1 - proba[normal_class].  A row that reads nothing gives NaN and -1. */
int pinn_lr_posterior(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                      const long long* d_row_index, long long n, int n_classes, const double* d_model, int normal_class,
                      double* d_decision, double* d_proba, long long* d_pred, double* d_p_fault, void* stream);

/* ROC curve of scores sorted descending (d_pos_sorted: non-zero = positive, in the same order), six launches.  d_counts
 * [PINN_LR_ROC_COUNTS]: positives, negatives, distinct scores, points kept (without the origin), and the area as the
 * integer U2 = sum dfps (tps_prev + tps): AUC = U2 / (2 positives negatives).  Curve outputs, each may be NULL and each
 * with room for n + 1 entries: point 0 is (0, 0, inf), then the kept points; drop_intermediate != 0 keeps the first, the
 * last and every point where the second difference of fps or tps is not zero, as scikit-learn does. */
#define PINN_LR_ROC_POS 0
#define PINN_LR_ROC_N 1
#define PINN_LR_ROC_M 2
#define PINN_LR_ROC_KEPT 3
#define PINN_LR_ROC_U2 4
#define PINN_LR_ROC_COUNTS 8
size_t pinn_lr_roc_workspace_bytes(long long n);
int pinn_lr_roc(const double* d_score_sorted, const long long* d_pos_sorted, long long n, int drop_intermediate,
                long long* d_counts, long long* d_fps, long long* d_tps, double* d_thresholds, double* d_fpr, double* d_tpr,
                void* d_ws, size_t ws_bytes, void* stream);

/* ---- batches of logistic regressions: feature selection over column subsets ------------------------------------
 * n_batch <= PINN_LR_MAX_BATCH candidates are standardised, fitted and scored together.  They share the array and the
 * row set (d_arr, ld, n_arr_rows, d_row_index, n: the row head above without its column list), d_y, n_classes, tol, l2,
 * fit_intercept and balanced.  Candidate c reads n_feat[c] columns (1..max_feat), cols[c * max_feat + i], i < n_feat[c].
 * Both lists are given twice: as host arrays, which are checked before any launch, and as device copies d_n_feat, d_cols of
 * the same layout, which the kernels read.  A kernel that meets a column outside [0, ld) in the device copy reads nothing
 * for that candidate's rows, as a gather index outside the array reads nothing.
 *
 * The state block of candidate c starts c * pinn_lr_batch_state_stride(n_classes, max_feat) bytes into d_state and has
 * exactly the single-model layout for (n_classes, n_feat[c]): it is a valid d_state of pinn_lr_newton and, from its mean,
 * scale and accepted point, of pinn_lr_posterior's model block.  The caller zeroes the blocks and writes the starting point
 * and MAXITER into each, as for the single model.
 *
 * The row passes run on a grid of (row blocks, candidates), the judgements with one workgroup per candidate, and both are
 * the single model's device code with the same tile-to-workgroup map, the same row_blocks(n, 128, 1024) partials per sum and
 * the same order of every sum: a candidate's bytes are those of the single-model calls and do not depend on what else is in
 * the batch.  A candidate whose header says stopped (CONVERGED, STATUS, or ITER >= MAXITER) returns at once in both kernels
 * while the others go on.  No entry point synchronises with the host.
 *
 * The workspace holds, per candidate, the totals, row_blocks(n, 128, 1024) partials per sum and as many class-count partials:
 * it grows with the rows, so that 4096 candidates over 1.3e3 rows stay within a few MiB.
 *
 * n_batch outside 1..PINN_LR_MAX_BATCH, an n_feat[c] outside 1..max_feat, a column outside [0, ld), (n_classes, max_feat)
 * outside the limits of the single model, NULL or misaligned pointers: PINN_E_ARG; a workspace below
 * pinn_lr_batch_workspace_bytes(n, n_batch, n_classes, max_feat): PINN_E_WORKSPACE; both before any launch. */
#define PINN_LR_MAX_BATCH 4096

size_t pinn_lr_batch_state_stride(int n_classes, int max_feat);             /* bytes; 0 for sizes outside the limits */
size_t pinn_lr_batch_workspace_bytes(long long n_rows, int n_batch, int n_classes, int max_feat);   /* likewise */

/* pinn_lr_scaler per candidate, four launches for the whole batch: mean, var, scale, class counts, class weights, SWSUM,
 * NSEEN, C, D of every state block. */
int pinn_lr_batch_scaler(const double* d_arr, long long ld, long long n_arr_rows, const long long* d_row_index, long long n,
                         const long long* d_y, int n_classes, int n_batch, const int* n_feat, const int* cols, int max_feat,
                         const int* d_n_feat, const int* d_cols, int balanced, double* d_state, void* d_ws, size_t ws_bytes,
                         void* stream);

/* pinn_lr_newton per candidate: n_passes times (row pass, judgement), two launches each for the whole batch. */
int pinn_lr_batch_newton(const double* d_arr, long long ld, long long n_arr_rows, const long long* d_row_index, long long n,
                         const long long* d_y, int n_classes, int n_batch, const int* n_feat, const int* cols, int max_feat,
                         const int* d_n_feat, const int* d_cols, int n_passes, double tol, double l2, int fit_intercept,
                         double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* Scores of a row set (which need not be the one fitted on, with its own d_y) under every candidate's accepted point, two
 * launches: d_loss_sum [n_batch] the sum of -log p[y] (unweighted; rows of a tile, tiles of a workgroup, workgroups, each in
 * index order), d_hits [n_batch] the rows whose first-maximum class equals y, and d_p_fault (may be NULL) [n_batch][n] =
 * 1 - p[normal_class], the bytes that pinn_lr_posterior writes for the same model.  A row that reads nothing or whose class is
 * outside [0, n_classes) adds nothing to either sum; the former gets a NaN p_fault. */
int pinn_lr_batch_score(const double* d_arr, long long ld, long long n_arr_rows, const long long* d_row_index, long long n,
                        const long long* d_y, int n_classes, int n_batch, const int* n_feat, const int* cols, int max_feat,
                        const int* d_n_feat, const int* d_cols, const double* d_state, int normal_class, double* d_loss_sum,
                        long long* d_hits, double* d_p_fault, void* d_ws, size_t ws_bytes, void* stream);

/* The integers of pinn_lr_roc for n_batch rows of scores, one launch: d_score_sorted [n_batch][n], each row sorted
 * descending, d_pos_sorted [n_batch][n] the flags gathered with them, d_counts [n_batch][PINN_LR_ROC_COUNTS] with positives,
 * negatives, distinct scores and U2 at PINN_LR_ROC_POS, _N, _M and _U2 (the other words are 0).  Equal scores form one
 * group, as in pinn_lr_roc, so U2 is its U2 exactly. */
int pinn_lr_batch_auc(const double* d_score_sorted, const long long* d_pos_sorted, long long n, int n_batch, long long* d_counts,
                      void* stream);

/* ---- clustering baselines of the method comparison: reference script 05 (cited as 05:<line>) -------------------------
 * k-means and Ward agglomerative clustering with nearest-centre assignment, float64 throughout, every operation rounded on
 * its own.  Rows are read in place as for the mixture above (column list, optional gather list, leading dimension; an index
 * outside [0, n_arr_rows) reads nothing and adds nothing).  Every reduction has a fixed order, there are no float atomics
 * and no workgroup waits on another: the same call gives the same bytes.
 *
 * Limits: n_feat <= PINN_CL_MAX_FEAT; n_clusters <= PINN_CL_MAX_CLUSTERS for k-means, the label means and the assignment;
 * n_classes <= PINN_CL_MAX_CLASSES.  Outside: PINN_E_ARG, sizes 0.  Ward takes any number of rows below 2^31.
 *
 * Both state blocks begin with PINN_CL_ST_HEADER 8-byte words, of which [PINN_CL_ST_ITER] (Lloyd iterations / chain steps
 * done), [.._CONVERGED] and [.._STATUS] (0 or PINN_CL_NAN) are common.  Once CONVERGED or STATUS is set, every later
 * queued Lloyd or Ward launch returns at its first instruction. */
#define PINN_CL_MAX_CLUSTERS 32
#define PINN_CL_MAX_FEAT 8
#define PINN_CL_MAX_CLASSES 16
#define PINN_CL_NAN 1
#define PINN_CL_ST_ITER 0
#define PINN_CL_ST_CONVERGED 1
#define PINN_CL_ST_STATUS 2
#define PINN_CL_ST_HEADER 16

/* k-means state: header; centres [K][D]; counts [K] (doubles: rows of every cluster in the last pass); column means [D];
 * labels [n] (64-bit integers).  Header: [.._K], [.._D], [.._N]; [.._INERTIA] (after an iteration: of the assignment to the
 * centres it started from; after the finishing pass: to the final centres), [.._SHIFT] = sum |new - old|^2 of the last
 * iteration, [.._TOL_ABS] = tol x the mean over columns of the variance (doubles); [.._STRICT] 1 when the stop was "the labels
 * equal the previous ones", [.._CHANGED] labels changed by the last iteration, [.._DONE] 1 after the finishing pass. */
#define PINN_KM_ST_K 3
#define PINN_KM_ST_D 4
#define PINN_KM_ST_INERTIA 5
#define PINN_KM_ST_SHIFT 6
#define PINN_KM_ST_TOL_ABS 7
#define PINN_KM_ST_STRICT 8
#define PINN_KM_ST_CHANGED 9
#define PINN_KM_ST_DONE 10
#define PINN_KM_ST_N 11

size_t pinn_km_state_bytes(long long n_rows, int n_clusters, int n_feat);    /* 0 for sizes outside the limits */
size_t pinn_km_workspace_bytes(long long n_rows, int n_clusters, int n_feat);

/* Lloyd iterations with scikit-learn 1.7's stopping rule on the centres the caller wrote into the state.
 * init != 0: labels = -1, then two row passes for the column means and variances, which set TOL_ABS from `tol` and reset the
 * header.  n_iters times two launches, no host synchronisation: every row goes to the nearest centre (sum (x - c)^2, the
 * first of equals) and overwrites its label, counting the changed ones; per-tile sums in a fixed order give the new centres
 * (old + sum (x - old) / count; an empty cluster keeps its centre, where scikit-learn relocates it); CONVERGED is set when no
 * label changed (STRICT) or else when SHIFT <= TOL_ABS.  finish != 0: the finishing pass, whatever the header says: unless
 * STRICT one more assignment against the final centres; inertia to the final centres; DONE.
 * After every pass the workspace begins with the summed terms [K][1 + 2 D] = (count, sum d_i, sum d_i^2), d = x - the
 * centre the pass started from. */
int pinn_km_lloyd(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                  const long long* d_row_index, long long n, int n_clusters, int init, int n_iters, double tol, int finish,
                  double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* d_centres [n_clusters][n_feat] += mean of (x - d_centres) over the positions whose d_labels entry names the cluster (a
 * label outside [0, n_clusters) adds nothing; a cluster without rows keeps what it holds); d_counts [n_clusters] (may be
 * NULL).  Workspace as for pinn_km_lloyd. */
int pinn_cluster_means(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                       const long long* d_row_index, long long n, int n_clusters, const long long* d_labels,
                       double* d_centres, double* d_counts, void* d_ws, size_t ws_bytes, void* stream);

/* Ward state: header; slot arrays mean [n][D] and size [n] (0: inactive); the chain stack [n]; the merge records lo [n],
 * hi [n] (slot numbers, lo < hi) and height [n] (n - 1 used), in the order the merges were made; sizes, chain and slots are
 * 64-bit integers.  Header: [.._N], [.._D], [.._MERGES], [.._CHAIN] the chain's length, [.._FIRST] a lower bound of the
 * first active slot. */
#define PINN_WARD_ST_N 3
#define PINN_WARD_ST_D 4
#define PINN_WARD_ST_MERGES 5
#define PINN_WARD_ST_CHAIN 6
#define PINN_WARD_ST_FIRST 7

size_t pinn_ward_state_bytes(long long n_rows, int n_feat);                 /* 0 for sizes outside the limits */
size_t pinn_ward_workspace_bytes(long long n_rows, int n_feat);

/* The Ward dendrogram of n positions by the nearest-neighbour chain on cluster means and sizes,
 * d^2(A, B) = 2 |A| |B| / (|A| + |B|) |mean_A - mean_B|^2, on O(n) memory.  init != 0: every position becomes a slot of
 * size 1 (0 when it reads nothing) and the chain starts at the first active slot.  n_steps chain steps of two launches, no
 * host synchronisation: a scan of all slots for the minimum of d^2(tip, j) by (d^2, j); then scipy's rule: the chain's
 * predecessor is the candidate to begin with and the scan's minimum replaces it only when strictly smaller.  If the
 * predecessor stays, the step merges: record (lo, hi, sqrt(d^2)), slot hi takes the size-weighted mean and the summed size,
 * slot lo becomes inactive, two slots leave the chain, and an empty chain restarts at the first active slot.  Otherwise the
 * minimum is pushed.  CONVERGED after n - 1 merges (or when no second active slot is left); 3 (n - 1) steps always suffice. */
int pinn_ward_tree(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                   const long long* d_row_index, long long n, int init, int n_steps, double* d_state, void* d_ws,
                   size_t ws_bytes, void* stream);

/* One launch, one thread per position.  d_centres [n_clusters][n_feat], d_map [n_clusters][n_classes] (may be NULL).
 * Outputs, each may be NULL: d_cluster [n] the nearest centre by sum (x - c)^2 (the first of equals), d_dist2 [n] that sum,
 * d_y_prob [n][n_classes] the map's row of that cluster (05:388-390), d_y_pred [n] its first maximum.  A position that
 * reads nothing gives -1 and NaN. */
int pinn_cluster_assign(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                        const long long* d_row_index, long long n, int n_clusters, const double* d_centres,
                        const double* d_map, int n_classes, long long* d_cluster, double* d_dist2, double* d_y_prob,
                        long long* d_y_pred, void* stream);

/* ---- isolation forest: the unsupervised anomaly score of reference script 02 (cited as 02:<line>) ---------------------
 * Scoring a given forest restates scikit-learn's IsolationForest.score_samples: the row is cast to float32, descends every
 * tree by x32 <= threshold, the leaf values (depth + 1) + c(n_node_samples) - 1 are added in tree order in float64, and the
 * score is -2^(-sum / den), den = n_trees c(max_samples).  Fitting is the package's own counter-based construction with
 * scikit-learn's rules (not its draws).  Rows are read in place as above; a position that reads nothing gives NaN.
 *
 * Limits: n_trees <= PINN_IF_MAX_TREES, max_samples <= PINN_IF_MAX_SAMPLES, n_feat <= PINN_IF_MAX_FEAT, a tree of at most
 * PINN_IF_MAX_NODES nodes, at most PINN_IF_MAX_LEAF_VALUES distinct leaf values in a forest.  Outside: PINN_E_ARG, size 0.
 *
 * The forest block (8-byte aligned), written by the host:
 *   header          PINN_IF_HEADER 8-byte words: [PINN_IF_H_MAGIC] = PINN_IF_MAGIC, [.._TREES], [.._NODES] (the largest node
 *                   count of a tree), [.._FEAT], [.._LEAF_VALUES], [.._TOTAL_NODES], [.._GROUPS] (64-bit integers) and
 *                   [.._DEN] (double; 0 gives the exponent -1, as scikit-learn does for one training row)
 *   leaf table      PINN_IF_MAX_LEAF_VALUES doubles: the distinct leaf values, computed on the host with numpy
 *   tree offsets    PINN_IF_MAX_TREES + 2 32-bit integers: tree t owns nodes [off[t], off[t + 1]) of the node array
 *   group starts    PINN_IF_MAX_TREES + 2 32-bit integers: group g is trees [grp[g], grp[g + 1]), consecutive trees whose
 *                   nodes together are at most PINN_IF_LDS_NODES: what a workgroup holds in LDS at a time
 *   nodes           8 bytes each, the root of a tree first, the two children of a node adjacent (left, then right):
 *                   word 0: inner node: the float32 threshold, the largest float32 <= the float64 threshold (for a float32
 *                           x, x <= t64 exactly when x <= that float32); leaf: index into the leaf table
 *                   word 1: bits 0-15 the left child (node number inside the tree), bits 16-18 the feature, bit 31 leaf */
#define PINN_IF_MAX_TREES 1024
#define PINN_IF_MAX_SAMPLES 1024
#define PINN_IF_MAX_FEAT 8
#define PINN_IF_MAX_NODES 2047
#define PINN_IF_MAX_LEAF_VALUES 16384
#define PINN_IF_LDS_NODES 4096
#define PINN_IF_MAGIC 0x49464f52
#define PINN_IF_HEADER 16
#define PINN_IF_H_MAGIC 0
#define PINN_IF_H_TREES 1
#define PINN_IF_H_NODES 2
#define PINN_IF_H_FEAT 3
#define PINN_IF_H_LEAF_VALUES 4
#define PINN_IF_H_TOTAL_NODES 5
#define PINN_IF_H_GROUPS 6
#define PINN_IF_H_DEN 7

size_t pinn_if_forest_bytes(int n_trees, int max_nodes_per_tree);            /* 0 for sizes outside the limits */

/* One launch, no workgroup waits on another, every position on its own: the result does not depend on the grid or on how the
 * caller cuts the rows into calls.  Outputs, each may be NULL: d_depth_sum [n] the float64 sum of the leaf values in tree
 * order, d_score [n] = -2^(-sum / den), d_pred [n] = +1 when score - offset >= 0, else -1.  A position that reads nothing
 * or whose float32 features are not all finite gives NaN, NaN and -1.  n_feat must be the forest's.
 * variant 0: the trees pass through LDS group by group while a thread keeps its rows' features in registers;
 * variant 1: every node is read from global memory (the L2 cache); kept for measurements, the same results. */
int pinn_if_score(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                  const long long* d_row_index, long long n, const void* d_forest, double offset, double* d_depth_sum,
                  double* d_score, long long* d_pred, int variant, void* stream);

/* Fits n_trees trees in one launch, one workgroup per tree, no host synchronisation.  Tree t draws max_samples distinct
 * positions of the n: position i of the subsample is i sent through a four-round Feistel permutation of [0, 4^k) keyed by
 * Philox4x32-10 at counter (t, 0, 1, 0) under the key `seed`, walked until it falls below n.  The rows are gathered as
 * float32.  A node splits while depth < max_depth and it holds more than one row and some feature is not constant on it:
 * Philox at counter (t, node, 0, 0) gives r0, r1; the feature is number floor(r0 c / 2^32) of the c non-constant ones, the
 * threshold t = lo + r1 2^-32 (hi - lo) in float64, t = lo when t >= hi; rows with x <= t go left.  Outputs in
 * scikit-learn's shape, nodes in pre-order, stride 2 max_samples - 1 per tree: d_feature, d_left, d_right, d_n_node (32-bit
 * integers), d_threshold (doubles); leaves carry -2, -2.0, -1, -1.  d_node_count [n_trees], d_samples [n_trees][max_samples]
 * (64-bit positions), d_status [n_trees]: 1 when a drawn row lies outside the array or is not finite (it then counts as 0). */
int pinn_if_fit(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                const long long* d_row_index, long long n, int n_trees, int max_samples, int max_depth,
                unsigned long long seed, int* d_feature, double* d_threshold, int* d_left, int* d_right, int* d_n_node,
                int* d_node_count, long long* d_samples, int* d_status, void* stream);

int pinn_abi_version(void);

/* ---- Script 05's Sup_SVM: one-vs-one linear SVC, interior point on the dual (pinn_svm.hip) --------------------------------
 * Rows are read in place as in the modules above (array, leading dimension, column list, optional gather list); d_y holds
 * the class index 0..n_classes-1 of every row position.  Limits: n_feat <= PINN_SVM_MAX_FEAT, 2 <= n_classes <=
 * PINN_SVM_MAX_CLASSES (28 pairs).  Outside: PINN_E_ARG, sizes 0.
 *
 * Pairs (a, b), a < b, in the order (0,1), (0,2), ..., (C-2,C-1).  The state block, in 8-byte words:
 *   header       PINN_SVM_ST_HEADER words: [.._ITER] (the largest iteration count of a pair), [.._CONVERGED] (every pair has),
 *                [.._STATUS] (the pairs' status words ORed: 0, PINN_SVM_NAN, PINN_SVM_SINGULAR, PINN_SVM_RANGE: a gather index
 *                outside the array or a class index outside [0, n_classes)), [.._C], [.._D], [.._P], [.._N]
 *   pair blocks  [P][PINN_SVM_PAIR_WORDS]: integers [PINN_SVM_P_ITER], [.._CONVERGED], [.._STATUS], [.._PHASE] (0: fresh,
 *                1: alpha and w set, 2: iterating, 3: a step waits to be applied), [.._A], [.._B]; doubles [.._M] (rows of the
 *                pair), [.._KA], [.._KB] (the starting alpha as a fraction of the bound, per side), [.._MU], [.._THETA],
 *                [.._SIGMU], [.._GAP] (primal - dual at the point), [.._PRIMAL], [.._DUAL], [.._THETA_AFF], [.._COMPL],
 *                [.._TALPHA], [.._SUMALPHA], [.._W .. + n_feat) (positive for class a), [.._BETA] (the intercept),
 *                [.._DAFF .. + n_feat + 1), [.._DIR .. + n_feat + 1) and [.._FIX .. + n_feat + 1) (predictor and final
 *                direction of (w, beta), and the refinement of the latter), [.._RW .. + n_feat) (w - V'alpha at the point)
 *   mean [D], scale [D], bound [C] (C x class weight: the upper bound of alpha of a row of that class)
 *   alpha, s, z  [n][C - 1] each: slot j of a row of class k belongs to its j-th other class in increasing order
 * The caller zeroes the block and fills [.._A], [.._B], [.._M], [.._KA], [.._KB], mean, scale and bound.  Once a pair's
 * CONVERGED or STATUS is set every later launch skips it.
 *
 * A row pass sums per pair, in this order: the upper triangle of sum u u' / d (u = (z-scores, 1), entry (i <= j) at
 * j (j + 1) / 2 + i), sum g t u / d [D + 1], sum alpha t u [D + 1] (the last is t'alpha), sum s alpha + z (c - alpha),
 * sum alpha, sum c max(0, 1 - t f).  pinn_svm_pass leaves them at the start of the workspace, [P][that many]. */
#define PINN_SVM_MAX_FEAT 8
#define PINN_SVM_MAX_CLASSES 8
#define PINN_SVM_NAN 1
#define PINN_SVM_SINGULAR 2
#define PINN_SVM_RANGE 4
#define PINN_SVM_ST_HEADER 16
#define PINN_SVM_ST_ITER 0
#define PINN_SVM_ST_CONVERGED 1
#define PINN_SVM_ST_STATUS 2
#define PINN_SVM_ST_C 3
#define PINN_SVM_ST_D 4
#define PINN_SVM_ST_P 5
#define PINN_SVM_ST_N 6
#define PINN_SVM_PAIR_WORDS 80
#define PINN_SVM_P_ITER 0
#define PINN_SVM_P_CONVERGED 1
#define PINN_SVM_P_STATUS 2
#define PINN_SVM_P_PHASE 3
#define PINN_SVM_P_A 4
#define PINN_SVM_P_B 5
#define PINN_SVM_P_M 6
#define PINN_SVM_P_KA 7
#define PINN_SVM_P_KB 8
#define PINN_SVM_P_MU 9
#define PINN_SVM_P_THETA 10
#define PINN_SVM_P_SIGMU 11
#define PINN_SVM_P_GAP 12
#define PINN_SVM_P_PRIMAL 13
#define PINN_SVM_P_DUAL 14
#define PINN_SVM_P_THETA_AFF 15
#define PINN_SVM_P_COMPL 16
#define PINN_SVM_P_TALPHA 17
#define PINN_SVM_P_SUMALPHA 18
#define PINN_SVM_P_W 20
#define PINN_SVM_P_BETA 28
#define PINN_SVM_P_DAFF 30
#define PINN_SVM_P_DIR 40
#define PINN_SVM_P_FIX 50
#define PINN_SVM_P_RW 60

size_t pinn_svm_state_bytes(long long n_rows, int n_classes, int n_feat);        /* 0 for sizes outside the limits */
size_t pinn_svm_workspace_bytes(long long n_rows, int n_classes, int n_feat);

/* One row pass at the state's point (alpha, s, z, w, beta as they stand; nothing is written to the state): the sums
 * above, at the start of the workspace.  For tests and tools. */
int pinn_svm_pass(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                  const long long* d_row_index, long long n, const long long* d_y, int n_classes, const double* d_state,
                  void* d_ws, size_t ws_bytes, void* stream);

/* Queues n_iter interior-point iterations of every pair (init != 0: the starting point first), six launches each, without
 * a host synchronisation.  A pair converges when primal - dual <= gap_tol max(1, primal), |t'alpha| <= 1e-12 sum alpha
 * and max |w - V'alpha| <= 1e-13 sum alpha.
 * After the call the state is consistent: alpha, w, beta and the gap belong to the same point.
 * An iteration starts from what the last one left in the workspace (the pairs' Cholesky factors and the predictor's
 * right-hand sides, behind the sums): a call with init == 0 must be given the workspace of the call before it, unchanged,
 * and the same rows, d_y and gap_tol.  The workspace of a call with init != 0 may hold anything. */
int pinn_svm_ipm(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                 const long long* d_row_index, long long n, const long long* d_y, int n_classes, int init, int n_iter,
                 double gap_tol, double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* One launch: z-scores, the P pairwise values w.z + b [n][P], the votes [n][C] (a where the value is > 0, else b) and the
 * prediction [n] (the first maximum of the votes; -1 for a gather index outside the array).  Every output may be NULL.
 * d_model: mean [D], scale [D], W [P][D], b [P]. */
int pinn_svm_decision(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                      const long long* d_row_index, long long n, int n_classes, const double* d_model, double* d_decision,
                      long long* d_votes, long long* d_pred, void* stream);

/* ---- Exact t-SNE: the two-dimensional embeddings of scripts 02 and 03 (pinn_tsne.hip) ------------------------------------
 * Rows are read in place as in the modules above (array, leading dimension, column list, optional gather list).  Limits:
 * n_feat <= PINN_TSNE_MAX_FEAT, 2 <= n <= PINN_TSNE_MAX_ROWS (the workspace holds P as n x n float64: 8 n^2 bytes, 8 GiB at
 * the limit, 968 MB at the reference's 1.1e4 rows).  Outside: PINN_E_ARG, sizes 0.
 *
 * Workspace, every part at a multiple of 256 bytes: P [n][n]; the per-row sums of the last pair pass [n][PINN_TSNE_ROW_SUMS]
 * = (Z_i, A_ix, A_iy, R_ix, R_iy, sum_j P log P, sum_j P log(1 + d^2), sum_j P) with w = 1 / (1 + d^2), d = |y_i - y_j|,
 * Z_i = sum_j w, A_i = sum_j P w (y_i - y_j), R_i = sum_j w^2 (y_i - y_j), j != i; the gradient [n][2] =
 * 4 (alpha A_i - R_i / Z); PINN_TSNE_SCALARS doubles: [.._SC_PSUM] (the sum of p + p^T that the affinities were divided by),
 * [.._SC_Z], [.._SC_KL] = alpha (sum P log P + log(alpha) sum P + sum P log(1 + d^2) + sum P log Z), [.._SC_SUMP],
 * [.._SC_PLOGP], [.._SC_PLOGQ], [.._SC_GNORM] (of the gradient; in a descent iteration of gains x gradient).  The three sums
 * with log are formed only where the error is wanted: always in pinn_tsne_kl_grad, in a descent iteration every 50th
 * and the last of a phase (scikit-learn's compute_error); elsewhere they keep what the last such pass left.
 *
 * State block, in 8-byte words: PINN_TSNE_ST_HEADER header words, Y [n][2], update [n][2], gains [n][2].  Header: integers
 * [.._ITER] (the iteration that runs next), [.._DONE], [.._STATUS] (0 or PINN_TSNE_NAN), [.._N], [.._PHASE] (0: early
 * exaggeration, momentum 0.5, iterations 0..249; 1: momentum 0.8, up to max_iter), [.._BEST_ITER], [.._LAST] (the last
 * iteration that ran: n_iter_), [.._STOP] and [.._STOP1] (why the run / the first phase ended: PINN_TSNE_STOP_*); doubles
 * [.._BEST_ERROR], [.._ERROR] (the last KL computed), [.._GNORM], [.._Z]. */
#define PINN_TSNE_MAX_FEAT 8
#define PINN_TSNE_MAX_ROWS 32768
#define PINN_TSNE_NAN 1
#define PINN_TSNE_NOT_CONVERGED 2
#define PINN_TSNE_DUPLICATES 4
#define PINN_TSNE_ROW_SUMS 8
#define PINN_TSNE_SCALARS 32
#define PINN_TSNE_SC_PSUM 0
#define PINN_TSNE_SC_Z 1
#define PINN_TSNE_SC_KL 2
#define PINN_TSNE_SC_SUMP 3
#define PINN_TSNE_SC_PLOGP 4
#define PINN_TSNE_SC_PLOGQ 5
#define PINN_TSNE_SC_GNORM 6
#define PINN_TSNE_ST_HEADER 16
#define PINN_TSNE_ST_ITER 0
#define PINN_TSNE_ST_DONE 1
#define PINN_TSNE_ST_STATUS 2
#define PINN_TSNE_ST_N 3
#define PINN_TSNE_ST_PHASE 4
#define PINN_TSNE_ST_BEST_ERROR 5
#define PINN_TSNE_ST_BEST_ITER 6
#define PINN_TSNE_ST_ERROR 7
#define PINN_TSNE_ST_GNORM 8
#define PINN_TSNE_ST_LAST 9
#define PINN_TSNE_ST_STOP 10
#define PINN_TSNE_ST_STOP1 11
#define PINN_TSNE_ST_Z 12
#define PINN_TSNE_STOP_MAX_ITER 1
#define PINN_TSNE_STOP_NO_PROGRESS 2
#define PINN_TSNE_STOP_GRAD_NORM 3

size_t pinn_tsne_state_bytes(long long n_rows);          /* 0 for sizes outside the limits */
size_t pinn_tsne_workspace_bytes(long long n_rows);

/* Joint probabilities of the rows into the workspace's P.  Per row i the root beta_i of H_i(beta) = log(perplexity), H_i
 * the entropy in nats of p_{j|i} ~ exp(-beta |x_i - x_j|^2): Newton steps inside a bracket until |H - log perplexity| <=
 * 1e-12 or 200 steps; then P_ij = max((p_{j|i} + p_{i|j}) / S, 2.220446049250313e-16), diagonal 0, symmetric bit for bit.
 * d_beta [n], d_entropy [n] (H_i at beta_i), d_status [n]: 0, PINN_TSNE_NAN (this row or any other is not finite, or a
 * gather index lies outside the array; the row of P is 0), PINN_TSNE_NOT_CONVERGED, or PINN_TSNE_DUPLICATES (no error: the
 * m nearest rows lie at exactly the same distance and log m >= log perplexity, so H > log perplexity for every beta; the row
 * gets the limit beta -> infinity, p = 1 / m on those rows, d_beta = infinity, d_entropy = log m).  0 < perplexity < n. */
int pinn_tsne_affinities(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                         const long long* d_row_index, long long n, double perplexity, double* d_beta, double* d_entropy,
                         long long* d_status, void* d_ws, size_t ws_bytes, void* stream);

/* One pair pass and reduction at the embedding d_Y [n][2] with the workspace's P and exaggeration alpha: per-row sums,
 * gradient and scalars are left in the workspace.  Nothing else is written.  For tests and timing. */
int pinn_tsne_kl_grad(long long n, const double* d_Y, double exaggeration, void* d_ws, size_t ws_bytes, void* stream);

/* Queues n_iter iterations (two launches each) without a host synchronisation: scikit-learn 1.7's _gradient_descent
 * (gains += 0.2 where update x gradient < 0, else x 0.8, floor 0.01; update = momentum update - learning_rate gains gradient;
 * Y += update) under the schedule of its _tsne: the checks every 50th iteration (best error, n_iter_without_progress - 250
 * in the first phase -, min_grad_norm), the change of phase after iteration 249 or an earlier stop with update and gains
 * reset; with max_iter == 250 the run ends with the first phase when that ran to its end.  Once DONE or STATUS is set the
 * remaining iterations do nothing.  init != 0: the header, update and gains are set first and Y is the caller's; init == 0
 * continues from the block as it stands (the caller may have written any consistent state).  max_iter >= 250. */
int pinn_tsne_descend(long long n, int init, int n_iter, int max_iter, double early_exaggeration, double learning_rate,
                      int n_iter_without_progress, double min_grad_norm, double* d_state, void* d_ws, size_t ws_bytes,
                      void* stream);

/* ---- Spectral clustering: the `Spectral` baseline of script 05 (05:455-512; pinn_spectral.hip) ---------------------------
 * The k-nearest-neighbour graph of the rows, its symmetric affinity A = 0.5 (C + C^T) as CSR, the K largest eigenpairs of
 * S = D^{-1/2} A D^{-1/2} (D = diag(A 1); a row without an edge has S_ii = 1, as scikit-learn's Laplacian gives it the
 * eigenvalue 0), scikit-learn's embedding D^{-1/2} q_j with its sign rule, and Lloyd's k-means on rows of up to 32 columns.
 * float64 throughout, every operation rounded on its own; every sum has a fixed order, there are no float atomics and no
 * workgroup waits on another: the same call gives the same bytes.  Integer atomics only count and hand out slots whose
 * order is sorted away afterwards.
 *
 * Limits: n_feat <= PINN_SP_MAX_FEAT, n_neighbors <= PINN_SP_MAX_NEIGHBORS, n_components <= PINN_SP_MAX_COMPONENTS,
 * n_clusters <= PINN_SP_MAX_CLUSTERS, n_dim <= PINN_SP_MAX_DIM, 1 <= n <= PINN_SP_MAX_ROWS (the graph search compares all
 * pairs of rows and keeps 32-bit positions).  Outside: PINN_E_ARG, sizes 0.
 *
 * The eigen state and the Lloyd state begin with PINN_CL_ST_HEADER 8-byte words with [PINN_CL_ST_ITER], [.._CONVERGED] and
 * [.._STATUS] (0 or PINN_SP_NAN) as in the clustering block above: once CONVERGED or STATUS is set, every later queued
 * launch returns at its first instruction. */
#define PINN_SP_MAX_FEAT 8
#define PINN_SP_MAX_NEIGHBORS 32
#define PINN_SP_MAX_COMPONENTS 32
#define PINN_SP_MAX_CLUSTERS 32
#define PINN_SP_MAX_DIM 32
#define PINN_SP_MAX_ROWS 16777216
#define PINN_SP_GUARD 16            /* columns of the block beyond n_components */
#define PINN_SP_MAX_DEGREE 40       /* Chebyshev steps of one filter */
#define PINN_SP_NAN 1
#define PINN_SP_BAD_ROW 2           /* pinn_sp_knn: a position read nothing */

/* d_indices [n][n_neighbors] (64-bit) and d_dist2 [n][n_neighbors]: per position the n_neighbors nearest positions by
 * (sum_i (x_i - y_i)^2 added in column order, position), itself among them when include_self != 0.  Candidates are staged
 * through LDS in tiles of 128 positions.  A position that reads nothing (gather index outside the array) has no neighbours
 * (-1, NaN), is nobody's neighbour and sets d_status[0] (one 64-bit word, else 0) to PINN_SP_BAD_ROW; lists that cannot be
 * filled end in (-1, NaN). */
int pinn_sp_knn(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                const long long* d_row_index, long long n, int n_neighbors, int include_self, long long* d_indices,
                double* d_dist2, long long* d_status, void* stream);

/* CSR of A = 0.5 (C + C^T) without its diagonal from the neighbour lists d_knn [n][n_neighbors] (entries outside [0, n) are
 * skipped): d_indptr [n + 1], d_indices and d_data (0.5 or 1.0) with room for 2 n n_neighbors entries, columns ascending in
 * every row; d_degree [n] = A 1 and d_dd [n] = sqrt(degree).  Six launches: counts of the transposed lists, a scan, the
 * fill (slots by integer atomics), the length of every row, a scan, and one workgroup per row that places every entry at
 * its rank, so the bytes do not depend on the schedule.  A row may be of any length. */
size_t pinn_sp_affinity_workspace_bytes(long long n, int n_neighbors);
int pinn_sp_affinity(long long n, int n_neighbors, const long long* d_knn, long long* d_indptr, long long* d_indices,
                     double* d_data, double* d_degree, double* d_dd, void* d_ws, size_t ws_bytes, void* stream);

/* Eigen state: header; Ritz values [m] descending; column residuals |S q_i - theta_i q_i| [m]; Ritz vectors [n][m];
 * m = min(n, n_components + PINN_SP_GUARD).  Header: integers [.._N], [.._M], [.._K], [.._MATVEC] (products of S with the
 * block), [.._DEGREE] (of the last filter); doubles [.._MAXRES] (largest residual of the first K columns), [.._FILT_C],
 * [.._FILT_E] (centre and half width of the damped interval), [.._TOL]. */
#define PINN_SP_ST_N 3
#define PINN_SP_ST_M 4
#define PINN_SP_ST_K 5
#define PINN_SP_ST_MATVEC 6
#define PINN_SP_ST_DEGREE 7
#define PINN_SP_ST_MAXRES 8
#define PINN_SP_ST_FILT_C 9
#define PINN_SP_ST_FILT_E 10
#define PINN_SP_ST_TOL 11

size_t pinn_sp_eigs_state_bytes(long long n, int n_components);
size_t pinn_sp_eigs_workspace_bytes(long long n, int n_components);

/* Chebyshev-filtered subspace iteration for the n_components largest eigenpairs of S on the block the caller wrote into
 * the state's vectors.  init != 0: the header is reset and the block orthonormalised (twice).  n_outer outer iterations are
 * queued without a host synchronisation, each: S Q (row pass in CSR order); H = Q^T S Q by per-tile partial sums added in
 * index order; one workgroup diagonalises H (cyclic Jacobi in LDS, round-robin pairs, eigenvalues descending); a row pass
 * rotates Q and S Q and sums the squared residuals; one workgroup takes the roots and sets CONVERGED when the largest of
 * the first K is <= tol, else decides the filter: a = max(theta_m, -0.99), c = (a - 1) / 2, e = (a + 1) / 2, degree = the
 * largest deg <= PINN_SP_MAX_DEGREE with cosh(deg acosh((1 - c) / e)) <= 1e8; PINN_SP_MAX_DEGREE launches of
 * Y_{j+1} = 2 (S Y_j - c Y_j) / e - Y_{j-1} (Y_1 = (S Y_0 - c Y_0) / e), those beyond the degree returning at once; then
 * twice: G = Y^T Y, one workgroup scales G to unit diagonal, diagonalises it, floors the eigenvalues at 1e-15 of the largest
 * and Y <- Y diag(G)^{-1/2} U Lambda^{-1/2}.  The bound 1e8 on the filter's growth makes a rescaling of the block needless.
 * nnz: entries d_indices and d_data hold (entries of d_indptr beyond it are cut, columns outside [0, n) skipped). */
int pinn_sp_eigs(long long n, const long long* d_indptr, const long long* d_indices, const double* d_data, long long nnz,
                 const double* d_dd, int n_components, int init, int n_outer, double tol, double* d_state, void* d_ws,
                 size_t ws_bytes, void* stream);

/* d_embedding [n][n_components] = q_j[i] / dd[i] (dd = 1 for a row without an edge), columns in descending eigenvalue, every
 * column with the sign that makes its entry of largest magnitude (the first of equals) positive.  Two launches; workspace
 * as for pinn_sp_eigs. */
int pinn_sp_embed(long long n, int n_components, const double* d_dd, const double* d_state, double* d_embedding,
                  void* d_ws, size_t ws_bytes, void* stream);

/* pinn_km_lloyd on a packed block d_x [n][n_dim]: the same state layout (header words PINN_KM_ST_*, centres [K][n_dim],
 * counts [K], column means [n_dim], labels [n]), stopping rule, rule for an empty cluster, finishing pass and workspace
 * head ([K][1 + 2 n_dim] summed terms). */
size_t pinn_sp_lloyd_state_bytes(long long n, int n_clusters, int n_dim);
size_t pinn_sp_lloyd_workspace_bytes(long long n, int n_clusters, int n_dim);
int pinn_sp_lloyd(const double* d_x, long long n, int n_dim, int n_clusters, int init, int n_iters, double tol, int finish,
                  double* d_state, void* d_ws, size_t ws_bytes, void* stream);

/* ---- The RBF-kernel SVC that script 05 names: one-vs-one, libsvm's SMO in float64 (pinn_ksvm.hip) -------------------------
 * Rows are read in place as in the modules above; d_y holds the class index 0..n_classes-1 of every row position.  Limits:
 * n_feat <= PINN_KSVM_MAX_FEAT, 2 <= n_classes <= PINN_KSVM_MAX_CLASSES (28 pairs).  Outside: PINN_E_ARG, sizes 0.
 *
 * A pair (a, b), a < b, in the order (0,1), (0,2), ..., (C-2,C-1), solves min 1/2 al'Q al - e'al, t'al = 0, 0 <= al <= c
 * over the rows of its two classes in position order, Q_ij = t_i t_j exp(-gamma |z_i - z_j|^2), t = +1 for class a, z the
 * z-scores (x - mean) / scale, the squared differences added in feature order.  The state block, in 8-byte words:
 *   header       PINN_KSVM_ST_HEADER words, for the caller's use (the kernels read none of them)
 *   pair blocks  [P][PINN_KSVM_PAIR_WORDS]: integers [PINN_KSVM_P_ITER], [.._CONVERGED], [.._STATUS] (0, PINN_KSVM_NAN: a row
 *                of the pair is not finite, PINN_KSVM_RANGE: a gather index outside the array or a class index outside
 *                [0, n_classes)), [.._A], [.._B], [.._I], [.._J] (the last working set, row positions), [.._NFREE]; doubles
 *                [.._GMAX], [.._GMIN] (of the last selection), and from pinn_ksvm_finish [.._RHO], [.._PRIMAL], [.._DUAL],
 *                [.._GAP], [.._SUMALPHA], [.._TALPHA], [.._VIOLATION] (gmax - gmin at the point)
 *   mean [D], scale [D], bound [C] (C x class weight: the upper bound of alpha of a row of that class)
 *   alpha, G     [n][C - 1] each: slot j of a row of class k belongs to its j-th other class in increasing order
 * The caller fills [.._A], [.._B], mean, scale and bound.  Once a pair's CONVERGED or STATUS is set every later launch of
 * pinn_ksvm_smo leaves the pair alone. */
#define PINN_KSVM_MAX_FEAT 8
#define PINN_KSVM_MAX_CLASSES 8
#define PINN_KSVM_NAN 1
#define PINN_KSVM_RANGE 4
#define PINN_KSVM_SV_TILE 128       /* support rows per LDS tile of pinn_ksvm_decision */
#define PINN_KSVM_ST_HEADER 16
#define PINN_KSVM_PAIR_WORDS 24
#define PINN_KSVM_P_ITER 0
#define PINN_KSVM_P_CONVERGED 1
#define PINN_KSVM_P_STATUS 2
#define PINN_KSVM_P_A 3
#define PINN_KSVM_P_B 4
#define PINN_KSVM_P_I 5
#define PINN_KSVM_P_J 6
#define PINN_KSVM_P_NFREE 7
#define PINN_KSVM_P_GMAX 8
#define PINN_KSVM_P_GMIN 9
#define PINN_KSVM_P_RHO 10
#define PINN_KSVM_P_PRIMAL 11
#define PINN_KSVM_P_DUAL 12
#define PINN_KSVM_P_GAP 13
#define PINN_KSVM_P_SUMALPHA 14
#define PINN_KSVM_P_TALPHA 15
#define PINN_KSVM_P_VIOLATION 16

size_t pinn_ksvm_state_bytes(long long n_rows, int n_classes, int n_feat);       /* 0 for sizes outside the limits */
size_t pinn_ksvm_workspace_bytes(long long n_rows, int n_classes, int n_feat);

/* Queues n_iters SMO iterations of every pair, two launches each, without a host synchronisation (init != 0: first one
 * launch that sets alpha = 0, G = -e, the pair blocks' running words and checks the rows).  An iteration: i = the first
 * maximum of -t G over I_up; it stops the pair (CONVERGED) when gmax - gmin <= tol; j = the first minimum of -b^2 / a over
 * the rows of I_low with b = gmax + t_j G_j > 0, a = 2 - 2 K_ij (1e-12 where that is not positive); libsvm's clipped update
 * of (alpha_i, alpha_j); G += t (t_i K_i dalpha_i + t_j K_j dalpha_j).  A status is recorded by the first iteration after
 * the launch that found it.  d_log: NULL, or [P][n_iters][2] 64-bit words that receive (i, j) of every iteration a pair
 * did in this call (the others keep what the caller wrote).  A call with init == 0 must be given the workspace of the call
 * before it, unchanged, and the same rows, d_y, gamma and tol; the workspace of a call with init != 0 may hold anything. */
int pinn_ksvm_smo(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                  const long long* d_row_index, long long n, const long long* d_y, int n_classes, double gamma, int init,
                  int n_iters, double tol, double* d_state, long long* d_log, void* d_ws, size_t ws_bytes, void* stream);

/* One launch, a workgroup per pair: libsvm's rho (the mean of t G over the rows with 0 < alpha < c, else the midpoint of the
 * two bounds), al'Q al = sum alpha (G + 1), primal = 1/2 al'Q al + sum c max(0, -G - t b) with b = -rho, dual = sum alpha -
 * 1/2 al'Q al, their difference, sum alpha, t'alpha, the number of free rows and gmax - gmin, into the pair blocks.  It reads
 * the state and d_y alone: no workspace, and of the rows only their number. */
int pinn_ksvm_finish(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                     const long long* d_row_index, long long n, const long long* d_y, int n_classes, double* d_state,
                     void* stream);

/* One launch, a thread per row: the P pairwise values sum_s coef[s][slot] K(z, sv_s) - rho[p] [n][P], the terms added in the
 * order of the support rows, the votes [n][C] (a where the value is > 0, else b) and the prediction [n] (the first maximum
 * of the votes; -1 for a gather index outside the array).  Every output may be NULL.  d_scaler: NULL or mean [D], scale [D]
 * of the rows; d_sv [n_sv][D] packed z-scores; d_coef [n_sv][C - 1]: t alpha in the slot layout; d_sv_class [n_sv]. */
int pinn_ksvm_decision(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                       const long long* d_row_index, long long n, int n_classes, const double* d_scaler, const double* d_sv,
                       const double* d_coef, const long long* d_sv_class, long long n_sv, const double* d_rho, double gamma,
                       double* d_decision, long long* d_votes, long long* d_pred, void* stream);

/* ---- ROC inference: DeLong's covariance of K AUCs and the stratified paired bootstrap ----------------------------------
 * Everything is an integer.  With m positives, n negatives and psi = 1, 1/2, 0 for a positive score above, equal to, below
 * a negative one, a positive row i carries a[i] = 2 #{neg < s_i} + #{neg == s_i} (= 2 n V10) and a negative row j carries
 * b[j] = 2 #{pos > s_j} + #{pos == s_j} (= 2 m V01); sum a = sum b = U2, the integer of the ROC entry point above.  No
 * float arithmetic, integer atomics only, no workgroup waits on another: the same call gives the same bytes.
 * Limits: 1 <= n_scores <= PINN_AUC_MAX_SCORES, 1 <= n < 2^31.  Outside: PINN_E_ARG, sizes 0. */
#define PINN_AUC_MAX_SCORES 8
#define PINN_AUC_TILE 256              /* elements of one scan tile */
#define PINN_AUC_BOOT_LDS_GROUPS 12288 /* a histogram of up to this many groups is held in LDS (48 KiB of a CU's 160 KiB) */
#define PINN_AUC_DRAW_BOOT 2           /* Philox draw kind of the bootstrap (0 and 1 are the isolation forest's) */
#define PINN_AUC_POS 0
#define PINN_AUC_NEG 1
#define PINN_AUC_GROUPS 2
#define PINN_AUC_U2 3
#define PINN_AUC_U2B 4
#define PINN_AUC_COUNTS 8

/* Five launches for all n_scores classifiers.  Per classifier k: d_score_sorted [k][n] ascending, d_pos_sorted [k][n]
 * (non-zero = positive) and d_row_sorted [k][n] (the row number of every element) in that order.  Equal scores form a group
 * (+0.0 == -0.0); groups are numbered from 0 in ascending order.  Out: d_comp [k][n] in row order, a[row] for a positive
 * row and b[row] for a negative one; d_group [k][n] the row's group number; d_counts [k][PINN_AUC_COUNTS]: positives,
 * negatives, groups, U2 = sum a, and sum b.  A row number outside [0, n) writes nothing. */
size_t pinn_auc_components_workspace_bytes(long long n, int n_scores);
int pinn_auc_components(const double* d_score_sorted, const long long* d_pos_sorted, const long long* d_row_sorted,
                        long long n, int n_scores, long long* d_counts, long long* d_comp, int* d_group, void* d_ws,
                        size_t ws_bytes, void* stream);

/* Two launches.  d_comp [n_scores][ld], rows <= ld entries of each read as unsigned 64-bit integers.  Out: d_sums
 * [n_scores (n_scores + 1) / 2][2], the pair (k, l), k <= l, at l (l + 1) / 2 + k: the low and the high 64-bit word of
 * sum_i comp[k][i] comp[l][i], exact below 2^128.  Workgroup partials are added in index order by one workgroup. */
size_t pinn_auc_cross_sums_workspace_bytes(long long rows, int n_scores);
int pinn_auc_cross_sums(const long long* d_comp, long long ld, long long rows, int n_scores, unsigned long long* d_sums,
                        void* d_ws, size_t ws_bytes, void* stream);

/* One launch, a workgroup per resample first .. first + n_boot - 1 (below 2^32).  d_group_pos [n_scores][m] and d_group_neg
 * [n_scores][n]: group numbers of the positive and of the negative rows; groups [n_scores] (a HOST array): the group counts.
 * Resample r draws n negatives, then m positives, with replacement: draw t of stratum s (0 negatives, 1 positives) takes
 * the 64 bits (word 2 (t & 1), word 2 (t & 1) + 1 as low, high) of Philox4x32-10 at the counter (t >> 1, r,
 * PINN_AUC_DRAW_BOOT, s) under the key seed, and its index is the high 64 bits of bits x stratum size.  Per classifier the
 * negatives are counted by group (integer atomics, in LDS up to PINN_AUC_BOOT_LDS_GROUPS groups, else in the workgroup's
 * slice of the workspace), the counts are scanned, and d_u2 [n_boot][n_scores] = sum over the positive draws of
 * 2 below[g] + count[g].  A group number outside [0, groups[k]) adds nothing. */
size_t pinn_auc_bootstrap_workspace_bytes(long long n_boot, int n_scores, const long long* groups);
int pinn_auc_bootstrap(const int* d_group_pos, const int* d_group_neg, long long m, long long n, int n_scores,
                       const long long* groups, unsigned long long seed, long long first, long long n_boot,
                       long long* d_u2, void* d_ws, size_t ws_bytes, void* stream);

/* ---- exact Shapley attributions: which input made the model say so -------------------------------------------------
 * f is a model with D <= PINN_GMM_MAX_FEAT inputs and C <= PINN_GMM_MAX_CLASSES outputs, the background a set of B rows.
 * The value of a coalition S of inputs at a row x is the interventional one, v(S; x) = (1 / B) sum over b of f(z) with
 * z_i = x_i for i in S and b_i otherwise, and the attribution of input j is
 *   phi_j(x) = sum over S without j of |S|! (D - |S| - 1)! / D! (v(S + j) - v(S)),
 * over all 2^D coalitions: nothing is sampled.  base = v(none), the mean prediction over the background; fx = v(all) = f(x);
 * sum over j of phi_j = fx - base.  Outputs: d_phi [n][D][C], d_base [C], d_fx [n][C], float64.  Every sum has a fixed order
 * that depends on B alone: the same call gives the same bytes, and a row's bytes do not depend on the other rows of the call.
 *
 * Rows and background are two row heads as above (array, leading dimension, rows of the array, column list, gather list or
 * NULL, positions), with the same number of columns; they may be the same array.  A row position that reads nothing gets
 * NaN outputs; a background position that reads nothing makes every output NaN.  Checks as make_rows': PINN_E_ARG for
 * NULL or misaligned pointers and sizes outside the limits (n_bg >= 1), PINN_E_WORKSPACE for a workspace below
 * pinn_shap_gmm_workspace_bytes (256-byte aligned), both before any launch.
 *
 * pinn_shap_gmm: f = d_y_prob of pinn_gmm_posterior under d_state and d_map [n_comp][n_classes], fused: a workgroup takes
 * PINN_SHAP_TILE rows and one split of the background, staged through LDS in blocks of PINN_SHAP_BG_BLOCK rows (at most
 * PINN_SHAP_MAX_SPLIT splits of whole blocks), and walks the coalitions on-chip; neither a hybrid row nor a coalition value is
 * written.  d_fx is what pinn_gmm_posterior writes for the rows.  n = 0 writes nothing. */
#define PINN_SHAP_TILE 128
#define PINN_SHAP_BG_BLOCK 32
#define PINN_SHAP_MAX_SPLIT 32

size_t pinn_shap_gmm_workspace_bytes(long long n_rows, long long n_background, int n_feat, int n_classes);   /* 0 outside the limits */
int pinn_shap_gmm(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                  const long long* d_row_index, long long n, const double* d_bg, long long ld_bg, long long n_bg_rows,
                  const int* cols_bg, int n_feat_bg, const long long* d_bg_index, long long n_bg, int n_comp,
                  const double* d_state, const double* d_map, int n_classes, double* d_phi, double* d_base, double* d_fx,
                  void* d_ws, size_t ws_bytes, void* stream);

/* Any model, in two calls with the caller's model between them.  pinn_shap_hybrid writes the hybrid rows of the row
 * positions row0 .. row0 + n_chunk - 1 as a dense array d_out [n_chunk * 2^D * B][D], float64 (f64 != 0) or float32: row-major
 * over (row, coalition, background), i.e. hybrid row (r * 2^D + S) * B + b takes column i from row r where bit i of S is
 * set and from background row b otherwise (NaN where that position reads nothing).  pinn_shap_reduce takes the model's
 * outputs on those rows, d_f [n_chunk * 2^D * B][C] float64 or float32, and returns d_phi [n_chunk][D][C], d_fx [n_chunk][C]
 * and, when d_base is not NULL, d_base [C] from the chunk's first row; it sums in float64, background rows in order, then
 * coalitions in order.  fx is the model's output on the first hybrid row of the full coalition, which is the row itself. */
int pinn_shap_hybrid(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                     const long long* d_row_index, long long n, const double* d_bg, long long ld_bg, long long n_bg_rows,
                     const int* cols_bg, int n_feat_bg, const long long* d_bg_index, long long n_bg, long long row0,
                     long long n_chunk, int f64, void* d_out, void* stream);
int pinn_shap_reduce(const void* d_f, int f64, long long n_chunk, int n_feat, long long n_bg, int n_classes, double* d_phi,
                     double* d_base, double* d_fx, void* stream);

/* ---- temporal diagnosis: a hidden Markov chain over the fault classes, the per-row posteriors as emissions ----------
 * S <= PINN_HMM_MAX_STATES states.  The rows are a row head as above with S columns (array, leading dimension, rows of the
 * array, column list, gather list or NULL, positions).  The emission of position t is b_t(s) = column s * inv_prior[s];
 * a position whose b_t is all zero, or holds a negative or non-finite value, or reads nothing, is missing: b_t = 1.
 * Emissions are scale-free: a row may be multiplied by any positive constant (the log-likelihood moves by its logarithm).
 *
 * d_model, float64 words: [0] iterations done, [1] converged, [3] last log-likelihood, [4] last gain (written by
 * pinn_hmm_mstep); A(i, j) at PINN_HMM_MODEL_A + 8 i + j (row-stochastic, zeros allowed), p0 at PINN_HMM_MODEL_P0,
 * inv_prior at PINN_HMM_MODEL_INV_PRIOR (ones for none), the log-likelihood history from PINN_HMM_HEADER on.
 *
 * d_seg_start [n_segments] (ascending, the first 0; n_segments = 0: one segment) restarts the chain from p0.  A carry holds
 * 2 S + 1 words per segment: the filtered distribution [S], the log-likelihood so far, the Viterbi scores [S].  With
 * d_carry_in the first position of segment s continues from it instead of p0; pinn_hmm_forward_backward reads and writes
 * the first S + 1 words, pinn_hmm_viterbi the last S.
 *
 * The recurrences are scans: an element is a flag, an S x S matrix and a 64-bit exponent; after every product the matrix
 * is scaled by the exact power of two that brings its largest entry into [0.5, 1).  Reduce-then-scan over tiles of
 * PINN_HMM_TILE positions (64 threads, PINN_HMM_ROWS_PER_THREAD consecutive positions each): one launch reduces every
 * tile, a one-workgroup launch scans the tile elements in tile order, a third finishes each tile; n <= PINN_HMM_TILE is one
 * launch.  No float atomics and a fixed order everywhere: the same call gives the same bytes.
 *
 * pinn_hmm_forward_backward: outputs, each skipped when NULL: d_alpha [n][S] filtered, d_gamma [n][S] smoothed, d_loglik
 * [segments], d_xi [S][S] expected transition counts, d_gamma_sum [S] (sum of gamma over positions with a successor in
 * their segment), d_carry_out.  Without d_gamma, d_xi and d_gamma_sum no backward launch runs.  With respect_converged != 0
 * every launch returns at once when word [1] of the model is set.
 * pinn_hmm_viterbi: max-plus scan of log A(i, j) + log b_t(j) (log 0 = -inf), backpointers = the lowest maximising i, the
 * path as a suffix composition of the backpointer maps (one 32-bit word per position) from the lowest arg-max of each
 * segment's last scores.  d_path [n] int64, d_logprob [segments], d_carry_out.
 * pinn_hmm_mstep: one launch.  A(i, j) <- (xi(i, j) + pseudo(i, j)) / their row total over the j with A(i, j) > 0; a zero
 * of A stays zero and a row whose total is zero keeps its values.  Appends the sum of d_loglik to the history (while it
 * has room: max_hist entries), counts the iteration and sets word [1] when |gain| < tol from the second iteration on.
 * Returns at once when word [1] is already set.  d_xi [S][S], d_pseudo [S][S] or NULL.
 *
 * Checks, on the host before any launch: PINN_E_ARG for NULL or misaligned pointers, S outside 1 .. PINN_HMM_MAX_STATES
 * and negative sizes; PINN_E_WORKSPACE for a workspace below pinn_hmm_workspace_bytes(n, S) (256-byte aligned; 0 outside
 * the limits); n = 0 (pinn_hmm_mstep: n_segments = 0) returns PINN_OK without a launch. */
#define PINN_HMM_MAX_STATES 8
#define PINN_HMM_TILE 1024
#define PINN_HMM_ROWS_PER_THREAD 16
#define PINN_HMM_HEADER 96
#define PINN_HMM_MODEL_A 16
#define PINN_HMM_MODEL_P0 80
#define PINN_HMM_MODEL_INV_PRIOR 88

size_t pinn_hmm_workspace_bytes(long long n, int n_states);
int pinn_hmm_forward_backward(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_states,
                              const long long* d_row_index, long long n, const double* d_model, const long long* d_seg_start,
                              long long n_segments, const double* d_carry_in, int respect_converged, double* d_alpha,
                              double* d_gamma, double* d_loglik, double* d_xi, double* d_gamma_sum, double* d_carry_out,
                              void* d_ws, size_t ws_bytes, void* stream);
int pinn_hmm_viterbi(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_states,
                     const long long* d_row_index, long long n, const double* d_model, const long long* d_seg_start,
                     long long n_segments, const double* d_carry_in, long long* d_path, double* d_logprob,
                     double* d_carry_out, void* d_ws, size_t ws_bytes, void* stream);
int pinn_hmm_mstep(double* d_model, int n_states, const double* d_xi, const double* d_loglik, long long n_segments,
                   const double* d_pseudo, double tol, int max_hist, void* stream);

/* ---- parameter identification: which physics parameter moved, per window, with a covariance -------------------------
 * A table is a row head as above with four columns (array, leading dimension, rows of the array, cols[4], gather list or
 * NULL, positions); p = 3 parameters per model.
 *   PINN_ID_VOLTAGE  columns (i, b, E, v), theta = (r, q, c) = (lambda_1, ln lambda_2, 1 / lambda_3):
 *                    residual E - b (ln i - q) - i r + 0.5 b log1p(-i c) - v, Jacobian row (-i, b, -0.5 b i / (1 - i c));
 *                    domain 1 - i c > 0 on every used row, tested as c max_i < 1.
 *   PINN_ID_THERMAL  columns (It, mc, T_in, T_out), theta = (lambda_T1, lambda_T3, lambda_T5):
 *                    residual T_out - (theta0 It + theta1 mc + 0.5 T_in + theta2), Jacobian row (-It, -mc, -1).
 * A position is missing (skipped, not counted) when it reads nothing or one of its four entries is not finite; for the
 * voltage model also when i <= 0 or b <= 0.
 *
 * Window w is the positions [d_win_start[w], d_win_start[w] + d_win_len[w]) of the gathered sequence; windows may overlap.
 * One workgroup of 256 threads runs the whole Levenberg-Marquardt loop of a window (grid-stride over windows, no other
 * workgroup involved, no float atomics).  Windows of at most PINN_ID_ONCHIP_ROWS positions keep their rows in registers
 * over all passes, longer ones (up to PINN_ID_MAX_WINDOW) read them again every pass; either way thread t adds positions
 * t, t + 256, ... in order, then a wave butterfly, then the four waves in index order: the same call gives the same
 * bytes and a window's bytes do not depend on the other windows of the call.
 *
 * The solver, per window: one row pass per trial point returns sse = r'r, A = J'J, g = J'r, n_used and max i.  With
 * D = diag(A) and C = D^-1/2 A D^-1/2 the trial step solves (A + mu D) d = -g by a Cholesky factorisation of C + mu I
 * (mu starts at opts->mu0); the trial theta + d is accepted when it is finite, inside the domain and sse_t < sse, then
 * mu = max(mu / 10, 1e-15), else mu *= 10.  Before every trial: s2 = sse / (n_used - 3), m = sqrt(g' A^-1 g / s2), which
 * bounds every component's first-order distance to the stationary point in its standard errors.  Status, in this order:
 *   6 bad window (negative start or length, length > PINN_ID_MAX_WINDOW, end beyond n)   3 n_used < 4
 *   4 theta0 not finite or outside the domain, or sums not finite   5 a diagonal entry of A not positive or a pivot of
 *   C's factorisation <= 2^-40   0 sse == 0, m <= tol, or every |d_k| <= xtol (|theta_k| + xtol)
 *   1 passes >= max_passes (the first pass counts; max_passes = 0 evaluates at theta0)   2 mu > 1e15.
 *
 * d_fit [n_windows][16]: theta [3], the covariance s2 A^-1 packed column by column [6], sse, m, mu, n_used, passes, status,
 * 0.  Status 3, 4 and 6: NaN but for n_used, passes and status; status 5: theta, sse and mu, the rest NaN.
 * d_normal (NULL: skipped) [n_windows][12], at the returned theta: A packed [6], g [3], sse, n_used, max i; NaN for status 6.
 * d_theta0 [3] with theta0_stride 0, [n_windows][3] with 3.  opts NULL: tol 1e-8, xtol 1e-14, mu0 1e-3, max_passes 100.
 *
 * Checks, on the host before any launch: PINN_E_ARG for NULL or misaligned pointers, a model or stride outside the above,
 * negative counts, options that are not finite and positive (max_passes < 0, reserved != 0); n_windows = 0 returns PINN_OK. */
#define PINN_ID_VOLTAGE 0
#define PINN_ID_THERMAL 1
#define PINN_ID_MAX_WINDOW 65536
#define PINN_ID_ONCHIP_ROWS 4096
#define PINN_ID_FIT_WORDS 16
#define PINN_ID_NORMAL_WORDS 12

typedef struct pinn_id_opts { double tol, xtol, mu0; int max_passes; int reserved; } pinn_id_opts_t;

int pinn_id_fit(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int model,
                const long long* d_row_index, long long n, const long long* d_win_start, const long long* d_win_len,
                long long n_windows, const double* d_theta0, long long theta0_stride, const pinn_id_opts_t* opts,
                double* d_fit, double* d_normal, void* stream);

/* ---- supply laws: the hydrogen and oxygen excess-ratio models per window, breakpoint included ------------------------
 * A table is a row head as for pinn_id_fit with two columns (x, y) = (It [A], act): array, leading dimension, rows of the
 * array, cols[2], gather list or NULL, positions.  The model is y = a + b min(x, c) / 100, theta = (a, b, c) = (l1, l2, l3)
 * of hydrogen_target / oxygen_target (the oxygen model's clamp and its penalty on act < 1 do not depend on theta and are
 * not part of the fit; its |l3| means c is reported non-negative whenever the currents are).  A position is missing
 * (skipped, not counted) when it reads nothing or one of its two entries is not finite.
 *
 * Window w is the positions [d_win_start[w], d_win_start[w] + d_win_len[w]) of the gathered sequence; windows may overlap.
 * max_window bounds the lengths of the call (at most PINN_BP_MAX_WINDOW is used): it sizes the dynamic LDS, rounded up to
 * a power of two, and a longer window is answered by status 6 from a bounds test, not by a read.
 *
 * The objective is only piecewise smooth in c, so the solver enumerates instead of iterating.  Per window, the used rows
 * sorted by (x, position), m = n_used:
 *   1 centring and sums: z = x / 100 and y are centred on the window means; running sums of (1, z, y, zz, zy, yy) in
 *     sorted order.
 *   2 candidates, only at k with x_(k) < x_(k+1) or k = m:
 *       knot k: c = x_(k), the two-parameter regression of y on u = min(z, z_k) over all rows; when x_(k) = x_(1) (u has
 *               one value) or the centred sum of uu is not positive, the constant model.
 *       free k (2 <= k <= m - 1, x_(k) > x_(1)): a line on the first k rows, the mean d of the rest, c = (d - a) / b;
 *               admissible only if the left sum of zz is positive, b != 0 and x_(k) <= c <= x_(k+1).
 *     Each candidate's SSE comes from the sums.  The smallest wins; on equal SSE a knot beats a free candidate, then the
 *     smaller k.  (For a fixed gap the model is linear in (a, b, d); where the unconstrained optimum of a gap is not
 *     admissible the constrained one lies on the gap's boundary, which is a knot, or at b = 0, which every knot contains.)
 *   3 one more pass over the rows at the winning theta: the direct sse, the normal matrix A = J'J of the Jacobian row
 *     (1, u, (b / 100) [x > c]) with u = min(x, c) / 100; sse_line (the knot at k = m) and sse_const come from the sums.
 *   4 cov = s2 A^-1, s2 = sse / (m - 3), by the scaled Cholesky factorisation and the 2^-40 pivot rule of pinn_id_fit.
 *     kind 2: the 2 x 2 block with s2 = sse / (m - 2), the c entries of cov NaN and c = +inf.
 *   5 c_lo / c_hi: the smallest and largest of the winner's own c (kind 2 and 3: its knot) and of the knot values whose
 *     SSE from the sums is <= sse_min (1 + q / (m - 3)), each moved outwards to the next current of the window where there
 *     is one (the profile crosses the threshold somewhere inside that gap; without this step the interval held the true
 *     c in 76 % of windows at a nominal 95 %, with it in 98 %): an interval to the resolution of the window's own
 *     currents.  At a knot the covariance is a one-sided linearisation, and `kind` says so.
 *
 * One workgroup of 256 threads owns a window (grid-stride over windows, no other workgroup involved, no float atomics):
 * it compacts the used rows into LDS in position order, sorts them by (x, position) with a bitonic network padded with
 * +inf keys to the next power of two m_pad, and thread t owns the sorted rows [t R, (t + 1) R), R = max(1, m_pad / 256).
 * Every sum adds a thread's rows in sorted order, then scans the 256 thread totals: Hillis-Steele over the 64 lanes of a
 * wave in steps 1, 2, ... 32, then the four waves in index order; a thread's running sums start at its exclusive prefix.
 * The same call gives the same bytes; a window's bytes depend neither on the other windows of the call nor on whether its
 * rows are read packed or through a gather list.
 *
 * d_fit [n_windows][24]: theta [3], cov packed column by column [6], sse, kind (0 free, 1 knot, 2 line: no row beyond c,
 * 3 constant), k, n_used, distinct currents, status, sse_line, sse_const, c_lo, c_hi, x_min, x_max, 0, 0, 0.
 * Status, in this order: 6 bad window (negative start or length, length > max_window or PINN_BP_MAX_WINDOW, end beyond n):
 * words 0..9 and 15..20 NaN, 10..13 zero; 3 n_used < 4: the same with n_used; 7 fewer than two distinct currents:
 * a = mean y, b = 0, c, cov, c_lo and c_hi NaN; 5 no candidate with a comparable SSE, a diagonal entry of A not positive
 * or a pivot <= 2^-40 (the constant model always ends here): theta and sse reported, cov NaN; 0 otherwise.
 * opts NULL: q = 3.841458820694124, the 95 % point of chi-square with one degree of freedom.
 *
 * Checks, on the host before any launch: PINN_E_ARG for NULL or misaligned pointers, ld < 1, a column outside the array,
 * negative counts, n beyond the rows without a gather list, q not finite and positive, reserved words not 0; n_windows = 0
 * returns PINN_OK after the options check. */
#define PINN_BP_MAX_WINDOW 4096
#define PINN_BP_FIT_WORDS 24

typedef struct pinn_bp_opts { double q; int reserved; int reserved2; } pinn_bp_opts_t;

int pinn_bp_fit(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, const long long* d_row_index,
                long long n, const long long* d_win_start, const long long* d_win_len, long long n_windows,
                long long max_window, const pinn_bp_opts_t* opts, double* d_fit, void* stream);

/* ---- uncertainty calibration and conformal bands: are the voltage network's standard deviations honest? -------------
 * Predictive law, per row: y ~ N(y_pred, v), v = a ale^2 + b epi^2 + c computed as ((a ale) ale + (b epi) epi) + c, with the
 * variance model var_model = (a, b, c), finite and non-negative; s = sqrt(v), r = y_true - y_pred, z = r / s.
 * The rows are a row head as above with the four columns cols = (y_true, y_pred, ale, epi): array, leading dimension, rows
 * of the array, cols[4], n_cols = 4, gather list or NULL, positions.
 *
 * Valid rows.  A position is valid when its gather index lies inside the array, its label maps to a group, y_true and
 * y_pred are finite, and v is finite and > 0.  Every other position is skipped and counted (n_skipped).
 * Groups.  label_col >= 0: the row's label x is used when 0 <= x < n_labels (n_labels <= PINN_UNC_MAX_LABELS; a NaN fails),
 * truncated to an integer, and label_table[label] (host array) is the group 0 .. n_groups - 1 or -1 for "skip";
 * n_groups <= PINN_UNC_MAX_GROUPS.  label_col = -1: every row is in group 0, no label is read, n_groups must be 1.
 * Arithmetic.  float64, every operation rounded on its own.  z, |z| and every comparison use +, *, sqrt, / and <= only: z
 * and everything counted from it are the bits a float64 numpy restatement gives.  log, erfc and exp enter the nll and crps
 * terms and the per-row Phi only.
 *
 * pinn_unc_score: one row pass and a one-workgroup launch that adds the workgroups' partials in index order.
 *   z_level [n_levels] (n_levels <= PINN_UNC_MAX_LEVELS, each >= 0) and z_edge [n_bins - 1] (strictly ascending, n_bins <=
 *   PINN_UNC_MAX_BINS) are host arrays of z-values, not probabilities.
 *   d_sums [n_groups][PINN_UNC_SUMS]: sums over the group's valid rows of 1, r, r^2, s, v (= s^2), z, z^2, nll, crps with
 *     nll = 0.5 (log 2 pi + log v + z^2),  Phi = 0.5 erfc(-z / sqrt 2),  phi = exp(-0.5 z^2) / sqrt(2 pi),
 *     crps = s (z (2 Phi - 1) + 2 phi - 1 / sqrt pi), the closed form for a Gaussian.
 *   d_n [n_groups], d_hits [n_groups][n_levels] = #{|z| <= z_level[l]}, d_pit [n_groups][n_bins] (a row's bin is the number
 *   of edges <= z), d_n_skipped [1]: int64.  Per-row outputs [n], each skipped when NULL: d_z, d_phi, d_crps, d_nll (NaN on
 *   a row that is not valid).
 *   Order of a float sum: workgroup b of row_blocks(n, PINN_UNC_TILE, PINN_UNC_MAX_BLOCKS) takes the tiles b, b + blocks,
 *   ...; a wave adds the 64 rows of a step by a shuffle tree and the steps in row order, then the four waves and the
 *   workgroups in index order.  Counts use integer atomics in LDS.  No float atomics.
 *
 * pinn_unc_quantiles: exact order statistics of a score per group, n_quantiles <= PINN_UNC_MAX_QUANTILES levels in (0, 1],
 *   n_groups * n_quantiles <= PINN_UNC_MAX_TARGETS.  kind: PINN_UNC_ABS_Z (|z|), PINN_UNC_Z (z), PINN_UNC_COLUMN (the value
 *   of column score_col; valid = inside the array, label mapped, value finite; the four columns are not read).
 *   Keys: the bits of the double (-0 taken as +0), all flipped for a negative value, the sign bit set otherwise: unsigned
 *   order = numeric order.  The result is the k-th smallest score (1-based) of the group's n_g valid rows, with k computed on
 *   the device in float64:  conformal != 0: k = ceil((n_g + 1) level), k > n_g gives +inf;  conformal = 0: k = ceil(n_g level)
 *   clipped to [1, n_g].  An empty group gives NaN and rank 0.
 *   d_q [n_groups][n_quantiles], d_rank [n_groups][n_quantiles] (k), d_n [n_groups], d_n_skipped [1].
 *   Method: eight passes over the rows read in place, the key's bytes from the top; scores are computed on the fly and
 *   never stored.  A pass counts, per target, the next byte of the rows that carry the target's prefix: 32-bit integer atomics
 *   on a [targets][256] histogram in LDS, merged by 64-bit integer atomics into the workspace.  Targets that still share
 *   group and prefix share one histogram.  After each pass a one-workgroup launch moves every target's prefix and remaining
 *   rank on in a device header and clears the histograms; the first also counts n_g.  A target whose new prefix at most
 *   PINN_UNC_COLLECT keys carry stops counting: the next pass appends those keys to a list in the workspace (an integer
 *   atomic hands out the places; their order is arbitrary), and a launch of one workgroup per target picks the key with
 *   fewer than k keys below it and at least k at or below it, by counting, so neither ties nor the order matter.  Passes
 *   in which no target is left return at once.  No host synchronisation between passes and no workgroup waits on
 *   another.  n <= 2^40.
 *
 * pinn_unc_update: the online band, one launch of one workgroup per chunk of n <= PINN_UNC_MAX_CHUNK positions (one group).
 *   d_state: 8-byte words; [0] fill and [1] next position of the ring (int64), [2] alpha_t, [3] q_t (float64), [4] valid and
 *   [5] missed rows so far (int64), [6..7] zero, then the ring of the last `window` scores |z| from word
 *   PINN_UNC_STATE_HEADER on; pinn_unc_state_bytes(window) bytes, window <= PINN_UNC_MAX_WINDOW (0 outside).
 *   1 every position gets lo / hi = y_pred -+ q_t s, z and a flag (1: |z| <= q_t is false, 0: inside, -1 and NaNs: not valid),
 *     with q_t as at the start of the chunk; each output is skipped when NULL (d_flag is int32).
 *   2 learn != 0: the valid rows' scores enter the ring in row order (of more than `window` the last `window` remain).
 *   3 alpha <- clip(alpha + gamma ((1 - level) - misses / valid), alpha_min, alpha_max); skipped when valid = 0.
 *   4 q <- the k-th smallest of the m ring entries, k = max(1, ceil((m + 1) (1 - alpha))) in float64, +inf when k > m.
 *   The ring image is sorted by a bitonic network in LDS (non-negative doubles order as their bits).  learn = 0 leaves
 *   every byte of the state as it is.  0 < level < 1, gamma >= 0 and finite, 0 <= alpha_min <= alpha_max <= 1.
 *
 * Checks, on the host before any launch: PINN_E_ARG for NULL or misaligned pointers and sizes outside the limits (edges
 * that do not ascend, a label table entry outside -1 .. n_groups - 1, n_cols != 4); PINN_E_WORKSPACE for a workspace below
 * pinn_unc_workspace_bytes(n, n_groups, n_quantiles) (256-byte aligned, enough for either entry point; pinn_unc_score asks
 * for n_quantiles = 1; 0 outside the limits); n = 0 returns PINN_OK without a launch. */
#define PINN_UNC_TILE 2048
#define PINN_UNC_MAX_BLOCKS 1024
#define PINN_UNC_SUMS 9
#define PINN_UNC_MAX_GROUPS 16
#define PINN_UNC_MAX_LABELS 64
#define PINN_UNC_MAX_LEVELS 16
#define PINN_UNC_MAX_BINS 64
#define PINN_UNC_MAX_QUANTILES 8
#define PINN_UNC_MAX_TARGETS 64
#define PINN_UNC_COLLECT 256
#define PINN_UNC_MAX_WINDOW 4096
#define PINN_UNC_MAX_CHUNK 2048
#define PINN_UNC_STATE_HEADER 8
#define PINN_UNC_ABS_Z 0
#define PINN_UNC_Z 1
#define PINN_UNC_COLUMN 2

size_t pinn_unc_workspace_bytes(long long n, int n_groups, int n_quantiles);
size_t pinn_unc_state_bytes(int window);
int pinn_unc_score(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_cols,
                   const long long* d_row_index, long long n, int label_col, const int* label_table, int n_labels,
                   int n_groups, const double* var_model, const double* z_level, int n_levels, const double* z_edge,
                   int n_bins, double* d_sums, long long* d_n, long long* d_hits, long long* d_pit, long long* d_n_skipped,
                   double* d_z, double* d_phi, double* d_crps, double* d_nll, void* d_ws, size_t ws_bytes, void* stream);
int pinn_unc_quantiles(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_cols,
                       const long long* d_row_index, long long n, int label_col, const int* label_table, int n_labels,
                       int n_groups, const double* var_model, int kind, int score_col, const double* levels, int n_quantiles,
                       int conformal, double* d_q, long long* d_rank, long long* d_n, long long* d_n_skipped, void* d_ws,
                       size_t ws_bytes, void* stream);
int pinn_unc_update(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_cols,
                    const long long* d_row_index, long long n, const double* var_model, double level, double gamma,
                    double alpha_min, double alpha_max, int window, int learn, void* d_state, double* d_lo, double* d_hi,
                    double* d_z, int* d_flag, void* stream);

/* ---- conformal fault sets and unknown-fault rejection (csrc/pinn_faultsets.hip; faultsets.py states the statistics) ----
 * Scores.  float64, every operation rounded on its own, sums in ascending class or component order, p = a row of y_prob:
 *   PINN_FS_LAC     s_c = 1 - p_c
 *   PINN_FS_MARGIN  s_c = max_{k != c} p_k - p_c (n_classes = 1: -p_c)
 *   PINN_FS_APS     s_c = sum_{k : p_k > p_c or (p_k == p_c and k < c)} p_k + u p_c, u = 1 unless randomized; then u =
 *                   ((w0 << 21) | (w1 >> 11)) 2^-53 from the Philox4x32-10 block of the counter (row_lo, row_hi, draw_kind, 0)
 *                   under the key seed, row = first + position (draw_kind: PINN_FS_DRAW_CAL or PINN_FS_DRAW_TEST)
 *   PINN_FS_DENSITY (pinn_fs_gmm only) s_c = -(logsumexp_{k : logm_kc > -inf}(lp_k + logm_kc) - logpi_c), lp_k as the mixture's
 *                   E-step forms it, the logsumexp as max, sum in ascending k, log; +inf when logpi_c = -inf.  d_logmap holds
 *                   log m [n_comp][n_classes] then log pi [n_classes], computed by the caller.  s_any = -log_prob_norm.
 * A row is missing when an entry of p is non-finite or negative, when all are zero, or when a score is NaN (density kind: when
 * a feature is non-finite or the gather index lies outside the array): count -1, mask 0, size 0, novel 0, missing 1, no tally.
 *
 * Calibration state (d_state), 8-byte words: a header of PINN_FS_HEADER words, then the ascending tables as float64, class
 * after class and the pooled table (class index n_classes) last, each starting on a multiple of PINN_FS_LINE entries.
 * Header (int64): [0] magic, [1] n_classes, [2] kind, [3] seed, [4] randomized, [5] rows skipped, [6] status (1: a class holds
 * more than PINN_FS_MAX_CAL rows; the tables are then not written), [16 + c] n_c, [40 + c] first entry of table c.
 * pinn_fs_state_bytes(n_cal, n_classes): bytes for n_cal calibration rows in all (0 outside the limits: n_cal < 0 or
 * > n_classes PINN_FS_MAX_CAL, n_classes outside 1 .. PINN_FS_MAX_CLASSES).
 *
 * pinn_fs_build: d_scores [n][n_classes] and d_class [n] in, the state out.  Row i contributes d_scores[i][d_class[i]] + 0 to
 *   table d_class[i] (and d_any[i] + 0 to the pooled table when d_any is given); a row whose class lies outside the range or
 *   whose score (or d_any[i]) is NaN is skipped and counted.  Counting, placing (an integer atomic hands out the places)
 *   and a merge sort of every table by ranks (ceil(log2 n) passes between the state and the workspace, each element's place
 *   is its own rank plus a binary search in the sibling run) all run inside the library; a sorted multiset of non-NaN doubles
 *   with one zero has one byte image, so the order of placing does not matter.
 *
 * pinn_fs_rank: one thread per row of d_y_prob [n][n_classes], tiles of PINN_FS_TILE rows, at most PINN_FS_MAX_BLOCKS
 *   workgroups striding over the tiles.  n_cal [n_classes + 1] (host) are the table sizes as the header has them, kmin
 *   [n_classes][n_levels] (host) the integer thresholds: class c is in the set at level l iff count_c >= kmin[c][l], count_c =
 *   n_c - #{t in T_c : t < s_c}.  Outputs, each skipped when NULL: d_count int32 [n][n_classes], d_mask uint16 [n][n_levels]
 *   (bit c), d_size uint8 [n][n_levels], d_novel uint8 [n][n_levels] (size 0 and not missing), d_missing uint8 [n], d_scores
 *   [n][n_classes] (NaN on a missing row).  With d_y [n] the tallies are added to d_tally (PINN_FS_TALLY_WORDS int64 words,
 *   zeroed by the caller; integer atomics in LDS, then to global memory): n [16], covered [16][8], size_hist [8][17] and
 *   singleton_correct [8] over rows with 0 <= y < n_classes, outside_n and outside_novel [8] over the others.  d_state = NULL
 *   (with n_levels = 0 and no output but d_scores and d_missing) computes scores only.
 *   Where the tables are searched (the integers do not depend on it): PINN_FS_REGIME_LDS all tables staged in LDS (their
 *   padded entries <= PINN_FS_LDS_ENTRIES); PINN_FS_REGIME_SAMPLED every PINN_FS_LINE-th entry in LDS (<= PINN_FS_LDS_ENTRIES
 *   of them), searched on-chip, then one 128-byte line read and counted; PINN_FS_REGIME_GLOBAL binary search in global
 *   memory.  PINN_FS_REGIME_AUTO takes LDS from PINN_FS_STAGE_MIN_ROWS rows on when the padded entries are at most
 *   PINN_FS_AUTO_LDS_ENTRIES, and GLOBAL otherwise: as measured on an MI355X, where SAMPLED lost at every shape
 *   and stays a forced regime.  A forced regime that does not fit is PINN_E_ARG.
 *
 * pinn_fs_gmm: the same from rows read in place under a mixture (d_gmm_state, d_map [n_comp][n_classes] as
 *   pinn_gmm_posterior takes them), tiles of PINN_FS_GMM_TILE rows; also d_y_prob, d_y_pred, d_log_prob_norm with
 *   pinn_gmm_posterior's bytes, d_any_score [n] (s_any) and d_any_count int32 [n] (density kind), each skipped when NULL.
 *
 * Checks, on the host before any launch: PINN_E_ARG for NULL or misaligned pointers, n_classes, n_levels, kind, regime, a
 * negative kmin or n_cal, n_cal beyond the cap; PINN_E_WORKSPACE for a workspace below pinn_fs_workspace_bytes(n, n_classes)
 * (256-byte aligned; 0 outside the limits).  n = 0 returns PINN_OK without a launch. */
#define PINN_FS_MAX_CLASSES 16
#define PINN_FS_MAX_LEVELS 8
#define PINN_FS_MAX_CAL (1 << 20)
#define PINN_FS_TILE 256
#define PINN_FS_GMM_TILE 64
#define PINN_FS_MAX_BLOCKS 1024
#define PINN_FS_LINE 16
#define PINN_FS_HEADER 64
#define PINN_FS_LDS_ENTRIES 7680       /* what a forced regime may stage (60 KiB); pinn_fs_gmm: PINN_FS_GMM_LDS_ENTRIES */
#define PINN_FS_GMM_LDS_ENTRIES 3072
#define PINN_FS_AUTO_LDS_ENTRIES 1536  /* what PINN_FS_REGIME_AUTO stages: measured faster at 1360 entries, slower at 7648 */
#define PINN_FS_STAGE_MIN_ROWS (1 << 20) /* and from this many rows on: below it the regimes measure alike */
#define PINN_FS_LAC 0
#define PINN_FS_MARGIN 1
#define PINN_FS_APS 2
#define PINN_FS_DENSITY 3
#define PINN_FS_DRAW_CAL 3             /* Philox draw kinds (0 and 1 are the isolation forest's, 2 the ROC bootstrap's) */
#define PINN_FS_DRAW_TEST 4
#define PINN_FS_REGIME_AUTO 0
#define PINN_FS_REGIME_LDS 1
#define PINN_FS_REGIME_SAMPLED 2
#define PINN_FS_REGIME_GLOBAL 3
#define PINN_FS_MAGIC 0x46534554
#define PINN_FS_H_NCAL 16
#define PINN_FS_H_OFFSET 40
#define PINN_FS_T_N 0
#define PINN_FS_T_COVERED 16
#define PINN_FS_T_HIST 144
#define PINN_FS_T_SINGLE 280
#define PINN_FS_T_OUT_N 288
#define PINN_FS_T_OUT_NOVEL 289
#define PINN_FS_TALLY_WORDS 304

size_t pinn_fs_state_bytes(long long n_cal, int n_classes);
size_t pinn_fs_workspace_bytes(long long n, int n_classes);
int pinn_fs_build(const double* d_scores, const double* d_any, const long long* d_class, long long n, int n_classes, int kind,
                  unsigned long long seed, int randomized, void* d_state, void* d_ws, size_t ws_bytes, void* stream);
int pinn_fs_rank(const double* d_y_prob, long long n, int n_classes, const void* d_state, const long long* n_cal,
                 const long long* kmin, int n_levels, int kind, int randomized, unsigned long long seed, int draw_kind,
                 long long first, int regime, const long long* d_y, int* d_count, unsigned short* d_mask, unsigned char* d_size,
                 unsigned char* d_novel, unsigned char* d_missing, double* d_scores, long long* d_tally, void* stream);
int pinn_fs_gmm(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                const long long* d_row_index, long long n, int n_comp, const double* d_gmm_state, const double* d_map,
                int n_classes, const double* d_logmap, const void* d_state, const long long* n_cal, const long long* kmin,
                int n_levels, int kind, int randomized, unsigned long long seed, int draw_kind, long long first, int regime,
                const long long* d_y, int* d_count, unsigned short* d_mask, unsigned char* d_size, unsigned char* d_novel,
                unsigned char* d_missing, double* d_scores, long long* d_tally, double* d_y_prob, long long* d_y_pred,
                double* d_log_prob_norm, double* d_any_score, int* d_any_count, void* stream);

/* ---- pinn_cp_*: penalised change-point segmentation of the rows (csrc/pinn_changepoint.hip; changepoint.py) ---------------
 * Where the statistics of up to PINN_CP_MAX_FEAT columns change, by exact optimal partitioning.  The rows are a row head as
 * above; `seg_starts` (host) and `d_seg_starts` (its device copy) hold n_segments strictly ascending start positions, the
 * first 0, the last below n (n_segments = 0, both NULL: one segment); n_segments <= PINN_CP_MAX_SEGMENTS and
 * n + n_segments < 2^31.  Segments are independent problems.  `mu`, `sigma` (host, [n_feat], both or neither): z = (x - mu) / sigma.
 *
 * The problem.  For a segment of m rows a partition 0 = tau_0 < ... < tau_k < tau_{k+1} = m with every piece at least
 * min_len and at most max_len long (max_len = 0: no upper limit) minimises sum_i C(tau_i, tau_{i+1}) + beta k.  With S, Q
 * the prefix sums of c and c^2 per column, c = z - z(first row of the segment), len = t - s, inv = 1 / len:
 *   SS_d(s, t) = max(Q_d(t) - Q_d(s) - (S_d(t) - S_d(s))^2 * inv, 0)
 *   PINN_CP_MEAN     C = sum_d SS_d                                                 min_len >= 1
 *   PINN_CP_MEANVAR  C = sum_d [len log v_d + SS_d / v_d], v_d = max(SS_d * inv, var_floor)       min_len >= 2
 * summed over d ascending from 0.  F(0) = -beta, F(t) = min over admissible s of (F(s) + C(s, t)) + beta, +inf without an
 * admissible s; ties go to the smallest s; last[t] is the arg-min and the change points are the walk of `last` from m.
 *
 * Prefix sums: tiles of PINN_CP_TILE positions counted from the segment's first row; inside a tile the sum runs row by row
 * from 0.0; the tile totals are summed tile by tile from 0.0 into exclusive offsets; S = offset + sum inside the tile.  A
 * row that reads nothing or holds a non-finite z flags its segment: status PINN_CP_BAD_ROW, F = NaN, no change point.
 *
 * The solver: one workgroup per (segment, penalty), steps in blocks of block_steps (0: PINN_CP_BLOCK, at most that).  A
 * candidate s joins the list in the block that holds step s + min_len.  Candidates known before a block are evaluated for
 * all its steps in parallel, the triangular part inside the block is finished by one wave.  After a block that ends at
 * t1 a candidate leaves the list when s < t1 + 1 - max_len, or, with prune != 0, when F(s) + C(s, t*) > F(t*) at
 * t* = t1 + 1 - min_len >= s + min_len (PELT's test at the last step that already permits leaving: s is not needed from
 * step t* + min_len = t1 + 1 on).  Pruning never changes F or the change points.  `evals` counts the (s, t) pairs that
 * entered a minimum (the one test per candidate and block is not counted).  A launch stops after the block at which the
 * sum of list length x steps reaches launch_evals (0: PINN_CP_LAUNCH_EVALS) and the next queued launch continues from
 * the workspace; a finished pair returns at once.  No workgroup waits on another, no float atomics; a pair's bytes do not
 * depend on what else is in the call.
 *
 * Outputs per (segment, penalty), at [segment * n_pen + penalty]: d_F = F(m), d_n_cp, d_evals, d_status (bits below),
 * d_cp [.. * cp_cap] ascending change points as positions of the call (segment start + tau); more than cp_cap sets
 * PINN_CP_OVERFLOW and keeps the first cp_cap.  PINN_CP_INFEASIBLE: no admissible partition (F = +inf).
 * pinn_cp_window: the same for one segment of n <= PINN_CP_MAX_WINDOW rows in a single launch of one workgroup, prefix sums
 * included; position j reads row (ring_start + j) mod n_arr_rows of the array (a ring of rows; ring_start = 0: the rows as they stand).
 *
 * Checks, on the host before any launch: PINN_E_ARG for NULL or misaligned pointers, n_feat outside 1 .. PINN_CP_MAX_FEAT,
 * n_pen outside 1 .. PINN_CP_MAX_PEN, a kind other than the two, min_len below the kind's minimum, max_len != 0 below
 * min_len, block_steps outside 0 .. PINN_CP_BLOCK, a non-finite or negative penalty, var_floor, launch_evals or cp_cap,
 * sigma not finite and positive, seg_starts that do not ascend strictly from 0 inside n; PINN_E_WORKSPACE for a workspace
 * below pinn_cp_workspace_bytes (256-byte aligned; 0 outside the limits); n = 0 returns PINN_OK without a launch. */
#define PINN_CP_MAX_FEAT 8
#define PINN_CP_MAX_PEN 16
#define PINN_CP_MAX_SEGMENTS 65535
#define PINN_CP_MAX_WINDOW 4096
#define PINN_CP_TILE 256
#define PINN_CP_BLOCK 64
#define PINN_CP_LAUNCH_EVALS (1LL << 24)
#define PINN_CP_MEAN 0
#define PINN_CP_MEANVAR 1
#define PINN_CP_BAD_ROW 1
#define PINN_CP_OVERFLOW 2
#define PINN_CP_INFEASIBLE 4

typedef struct {
  int kind, min_len;
  long long max_len;
  int prune, block_steps;
  double var_floor;
  long long launch_evals;
} pinn_cp_opts_t;

size_t pinn_cp_workspace_bytes(long long n, int n_feat, long long n_segments, int n_pen);
int pinn_cp_segment(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat,
                    const long long* d_row_index, long long n, const double* mu, const double* sigma,
                    const long long* seg_starts, const long long* d_seg_starts, long long n_segments,
                    const pinn_cp_opts_t* opts, const double* penalties, int n_pen, double* d_F, long long* d_n_cp,
                    long long* d_cp, long long cp_cap, long long* d_evals, long long* d_status, void* d_ws, size_t ws_bytes,
                    void* stream);
int pinn_cp_window(const double* d_arr, long long ld, long long n_arr_rows, const int* cols, int n_feat, long long ring_start,
                   long long n, const double* mu, const double* sigma, const pinn_cp_opts_t* opts, const double* penalties,
                   int n_pen, double* d_F, long long* d_n_cp, long long* d_cp, long long cp_cap, long long* d_evals,
                   long long* d_status, void* d_ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PINN_HIP_H */
