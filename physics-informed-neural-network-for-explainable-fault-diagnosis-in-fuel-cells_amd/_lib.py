"""ctypes binding of libpinn_hip.so -- the only route from Python to the HIP kernels.

There is NO CPU fallback: if the library is missing or a call fails, an exception is raised.
All pointers handed over are raw device pointers (torch tensors' data_ptr()); torch only
provides device memory and the current stream.
"""
import ctypes
import os

from . import _build

c_void_p, c_int, c_uint, c_ll, c_float, c_size_t = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_longlong,
                                                    ctypes.c_float, ctypes.c_size_t)

NLAMBDA, NCOLS, NSUMS = 17, 20, 32
RES_V, RES_T, RES_H, RES_O, RES_ALL = 1, 2, 4, 8, 15
DROP_NONE, DROP_PHILOX, DROP_BITS = 0, 1, 2
STAGE_LAMBDA_PM, STAGE_LAMBDA_F, STAGE_THERMAL, STAGE_HYDROGEN, STAGE_OXYGEN = 0, 1, 2, 3, 4

# column / sum indices (include/pinn_hip.h)
C = {n: i for i, n in enumerate(
    ["FV", "VACT", "VOHM", "VCONC", "ENERNST", "VEST5", "I", "VOUT5", "FT", "TPRED", "TOUT",
     "FH", "ACTH", "TGTH", "ITOT", "FO", "ACTO", "TGTO", "QO2", "O2FLOW"])}
S = {n: i for i, n in enumerate(
    ["FV2", "FV_D1", "FV_D2", "FV_D3", "YV2", "YV_D1", "YV_D2", "YV_D3", "YU2",
     "FT2", "FT_D1", "FT_D3", "FT_D5", "FT_ABS", "FH2", "FH_D1", "FH_D2", "FH_D3", "ACTH", "TGTH",
     "FO2", "FO_D1", "FO_D2", "FO_D3", "ACTO", "TGTO"])}


class Affine(ctypes.Structure):
    _fields_ = [("x_min", ctypes.c_double * 8), ("x_scale", ctypes.c_double * 8), ("y_min", ctypes.c_double),
                ("y_scale", ctypes.c_double), ("vn_scale", c_float), ("vn_min", c_float)]


PREC_FP32, PREC_BF16, PREC_F32X6, PREC_F32X6_G6 = 0, 1, 2, 3
PHASE_CHAIN, PHASE_WGRAD, PHASE_REDUCE, PHASE_ALL = 1, 2, 4, 7
PHASE_WGRAD_TAIL, PHASE_WGRAD_HEAD, PHASE_REDUCE_TAIL, PHASE_REDUCE_HEAD = 32, 64, 128, 256
STAGE_RUN_MAX_ROWS, STAGE_LOG_FLOATS = 65536, 64


class Net(ctypes.Structure):
    _fields_ = [("n_in", c_int), ("hidden", c_int), ("n_hidden", c_int), ("precision", c_int), ("d_packed", c_void_p)]

    def __init__(self, n_in=8, hidden=256, n_hidden=3, precision=0, d_packed=None):
        super().__init__(n_in, hidden, n_hidden, precision, d_packed)


class GNet(ctypes.Structure):
    """pinn_gnet_t: any layers list [8, h_1, ..., h_k, 1] (pinn_general.hip)."""
    _fields_ = [("n_in", c_int), ("n_hidden", c_int), ("width", c_int * 8), ("n_out", c_int), ("reserved", c_int)]

    def __init__(self, layers):
        layers = [int(v) for v in layers]
        hid = layers[1:-1]
        w = (c_int * 8)(*(hid[:8] + [0] * (8 - min(len(hid), 8))))
        super().__init__(layers[0], len(hid), w, layers[-1], 0)


class Dropout(ctypes.Structure):
    _fields_ = [("mode", c_int), ("p", c_float * 9), ("seed", ctypes.c_ulonglong), ("stream", c_uint),
                ("row_offset", c_ll), ("d_bits", c_void_p), ("d_step_counter", c_void_p)]


class RFParams(ctypes.Structure):
    """pinn_rf_params_t (pinn_risk.hip)."""
    _fields_ = [("n_cols", c_int), ("n_layers", c_int), ("col", c_int * 8), ("layer_of", c_int * 8), ("w", ctypes.c_double * 8),
                ("beta", ctypes.c_double * 4), ("p_layer", ctypes.c_double), ("z_safe", ctypes.c_double),
                ("lambda_decay", ctypes.c_double), ("k_logistic", ctypes.c_double), ("c0_logistic", ctypes.c_double),
                ("c_max", ctypes.c_double), ("alpha_smooth", ctypes.c_double)]


RF_ABOVE, RF_BELOW, RF_TILE = 0, 1, 2048
RF_SWEEP_WORDS = 24                     # float64 words of one candidate of pinn_rf_sweep (include/pinn_hip.h)

# pinn_gmm.hip: limits, status and the 8-byte words of the state header
GMM_MAX_COMP, GMM_MAX_FEAT, GMM_MAX_CLASSES, GMM_SINGULAR, GMM_TILE, GMM_MAX_BATCH = 32, 8, 16, 1, 128, 1024
GMM_ST_ITER, GMM_ST_CONVERGED, GMM_ST_STATUS, GMM_ST_K, GMM_ST_D, GMM_ST_LOWER, GMM_ST_PREV, GMM_ST_CHANGE, GMM_ST_HEADER = range(9)

# pinn_cluster.hip: limits, status and the 8-byte words of the state headers
CL_MAX_CLUSTERS, CL_MAX_FEAT, CL_MAX_CLASSES, CL_NAN, CL_TILE, CL_ST_HEADER = 32, 8, 16, 1, 128, 16
CL_ST_ITER, CL_ST_CONVERGED, CL_ST_STATUS = 0, 1, 2
KM_ST_K, KM_ST_D, KM_ST_INERTIA, KM_ST_SHIFT, KM_ST_TOL_ABS, KM_ST_STRICT, KM_ST_CHANGED, KM_ST_DONE, KM_ST_N = range(3, 12)
WARD_ST_N, WARD_ST_D, WARD_ST_MERGES, WARD_ST_CHAIN, WARD_ST_FIRST = range(3, 8)

# pinn_lr.hip: limits, status and the 8-byte words of the state header and of the ROC counts
LR_MAX_CLASSES, LR_MAX_FEAT, LR_MAX_HESS, LR_SINGULAR, LR_NAN, LR_STALLED, LR_TILE = 13, 8, 1365, 1, 2, 3, 128
LR_MAX_BATCH = 4096
(LR_ST_ITER, LR_ST_CONVERGED, LR_ST_STATUS, LR_ST_C, LR_ST_D, LR_ST_F, LR_ST_STEP, LR_ST_DD, LR_ST_PASSES, LR_ST_GMAX, LR_ST_SWSUM,
 LR_ST_PHASE, LR_ST_NSEEN, LR_ST_MAXITER) = range(14)
LR_ST_HEADER = 16
LR_ROC_POS, LR_ROC_N, LR_ROC_M, LR_ROC_KEPT, LR_ROC_U2, LR_ROC_COUNTS = 0, 1, 2, 3, 4, 8

# pinn_iforest.hip: limits and the 8-byte words of the forest block's header
IF_MAX_TREES, IF_MAX_SAMPLES, IF_MAX_FEAT, IF_MAX_NODES, IF_MAX_LEAF_VALUES, IF_LDS_NODES = 1024, 1024, 8, 2047, 16384, 4096
IF_MAGIC, IF_HEADER = 0x49464f52, 16
IF_H_MAGIC, IF_H_TREES, IF_H_NODES, IF_H_FEAT, IF_H_LEAF_VALUES, IF_H_TOTAL_NODES, IF_H_GROUPS, IF_H_DEN = range(8)

# pinn_svm.hip: limits, status and the 8-byte words of the state header and of a pair's block
SVM_MAX_FEAT, SVM_MAX_CLASSES, SVM_NAN, SVM_SINGULAR, SVM_RANGE, SVM_ST_HEADER, SVM_PAIR_WORDS = 8, 8, 1, 2, 4, 16, 80
SVM_ST_ITER, SVM_ST_CONVERGED, SVM_ST_STATUS, SVM_ST_C, SVM_ST_D, SVM_ST_P, SVM_ST_N = range(7)
(SVM_P_ITER, SVM_P_CONVERGED, SVM_P_STATUS, SVM_P_PHASE, SVM_P_A, SVM_P_B, SVM_P_M, SVM_P_KA, SVM_P_KB, SVM_P_MU, SVM_P_THETA, SVM_P_SIGMU,
 SVM_P_GAP, SVM_P_PRIMAL, SVM_P_DUAL, SVM_P_THETA_AFF, SVM_P_COMPL, SVM_P_TALPHA, SVM_P_SUMALPHA) = range(19)
SVM_P_W, SVM_P_BETA, SVM_P_DAFF, SVM_P_DIR, SVM_P_FIX, SVM_P_RW = 20, 28, 30, 40, 50, 60

# pinn_ksvm.hip: limits, status and the 8-byte words of the state header and of a pair's block
KSVM_MAX_FEAT, KSVM_MAX_CLASSES, KSVM_NAN, KSVM_RANGE, KSVM_SV_TILE, KSVM_ST_HEADER, KSVM_PAIR_WORDS = 8, 8, 1, 4, 128, 16, 24
(KSVM_P_ITER, KSVM_P_CONVERGED, KSVM_P_STATUS, KSVM_P_A, KSVM_P_B, KSVM_P_I, KSVM_P_J, KSVM_P_NFREE, KSVM_P_GMAX, KSVM_P_GMIN, KSVM_P_RHO,
 KSVM_P_PRIMAL, KSVM_P_DUAL, KSVM_P_GAP, KSVM_P_SUMALPHA, KSVM_P_TALPHA, KSVM_P_VIOLATION) = range(17)

# pinn_tsne.hip: limits, status, per-row sums, workspace scalars and the 8-byte words of the state header
TSNE_MAX_FEAT, TSNE_MAX_ROWS, TSNE_NAN, TSNE_NOT_CONVERGED, TSNE_ROW_SUMS, TSNE_SCALARS, TSNE_ST_HEADER = 8, 32768, 1, 2, 8, 32, 16
TSNE_SC_PSUM, TSNE_SC_Z, TSNE_SC_KL, TSNE_SC_SUMP, TSNE_SC_PLOGP, TSNE_SC_PLOGQ, TSNE_SC_GNORM = range(7)
(TSNE_ST_ITER, TSNE_ST_DONE, TSNE_ST_STATUS, TSNE_ST_N, TSNE_ST_PHASE, TSNE_ST_BEST_ERROR, TSNE_ST_BEST_ITER, TSNE_ST_ERROR, TSNE_ST_GNORM,
 TSNE_ST_LAST, TSNE_ST_STOP, TSNE_ST_STOP1, TSNE_ST_Z) = range(13)
TSNE_STOP_MAX_ITER, TSNE_STOP_NO_PROGRESS, TSNE_STOP_GRAD_NORM, TSNE_DUPLICATES = 1, 2, 3, 4

# pinn_spectral.hip: limits, status and the 8-byte words of the eigen state's header (the Lloyd state has k-means' words)
SP_MAX_FEAT, SP_MAX_NEIGHBORS, SP_MAX_COMPONENTS, SP_MAX_CLUSTERS, SP_MAX_DIM, SP_MAX_ROWS, SP_GUARD = 8, 32, 32, 32, 32, 1 << 24, 16
SP_NAN, SP_BAD_ROW = 1, 2
SP_ST_N, SP_ST_M, SP_ST_K, SP_ST_MATVEC, SP_ST_DEGREE, SP_ST_MAXRES, SP_ST_FILT_C, SP_ST_FILT_E, SP_ST_TOL = range(3, 12)

# pinn_rocstat.hip: limits, the scan tile, the LDS / workspace switch of the bootstrap histogram and the 8-byte words of the counts
AUC_MAX_SCORES, AUC_TILE, AUC_BOOT_LDS_GROUPS, AUC_DRAW_BOOT, AUC_COUNTS = 8, 256, 12288, 2, 8
AUC_POS, AUC_NEG, AUC_GROUPS, AUC_U2, AUC_U2B = range(5)

# pinn_hmm.hip: limits, the scan tile and the 8-byte words of the device model
HMM_MAX_STATES, HMM_TILE, HMM_ROWS_PER_THREAD, HMM_HEADER, HMM_MODEL_A, HMM_MODEL_P0, HMM_MODEL_INV_PRIOR = 8, 1024, 16, 96, 16, 80, 88
HMM_ITER, HMM_CONVERGED, HMM_PREV, HMM_GAIN = 0, 1, 3, 4

# pinn_identify.hip: models, limits and the 8-byte words of a fit row and of a normal-equations row
ID_VOLTAGE, ID_THERMAL, ID_MAX_WINDOW, ID_ONCHIP_ROWS, ID_FIT_WORDS, ID_NORMAL_WORDS = 0, 1, 65536, 4096, 16, 12


class IdOpts(ctypes.Structure):
    """pinn_id_opts_t (pinn_identify.hip)."""
    _fields_ = [("tol", ctypes.c_double), ("xtol", ctypes.c_double), ("mu0", ctypes.c_double), ("max_passes", c_int), ("reserved", c_int)]


# pinn_breakpoint.hip: the longest window and the 8-byte words of a fit row
BP_MAX_WINDOW, BP_FIT_WORDS = 4096, 24


class BpOpts(ctypes.Structure):
    """pinn_bp_opts_t (pinn_breakpoint.hip)."""
    _fields_ = [("q", ctypes.c_double), ("reserved", c_int), ("reserved2", c_int)]


# pinn_uncertainty.hip: the row tile and the limit of partial sums (they fix the order of every float sum), the limits,
# the 8-byte words of the monitor's state header and the score kinds
UNC_TILE, UNC_MAX_BLOCKS, UNC_SUMS, UNC_MAX_GROUPS, UNC_MAX_LABELS, UNC_MAX_LEVELS, UNC_MAX_BINS = 2048, 1024, 9, 16, 64, 16, 64
UNC_MAX_QUANTILES, UNC_MAX_TARGETS, UNC_MAX_WINDOW, UNC_MAX_CHUNK, UNC_STATE_HEADER = 8, 64, 4096, 2048, 8
UNC_ABS_Z, UNC_Z, UNC_COLUMN = 0, 1, 2
UNC_COLLECT = 256                       # the select gathers a target's keys once at most this many carry its prefix

# pinn_faultsets.hip: limits, row tiles, the on-chip table budgets and the row count below which nothing is staged, score kinds,
# Philox draw kinds, table regimes, and the 8-byte words of the state header and of the tallies
FS_MAX_CLASSES, FS_MAX_LEVELS, FS_MAX_CAL, FS_TILE, FS_GMM_TILE, FS_MAX_BLOCKS, FS_LINE, FS_HEADER = 16, 8, 1 << 20, 256, 64, 1024, 16, 64
FS_LDS_ENTRIES, FS_GMM_LDS_ENTRIES, FS_AUTO_LDS_ENTRIES, FS_STAGE_MIN_ROWS = 7680, 3072, 1536, 1 << 20
FS_LAC, FS_MARGIN, FS_APS, FS_DENSITY, FS_DRAW_CAL, FS_DRAW_TEST = 0, 1, 2, 3, 3, 4
FS_REGIME_AUTO, FS_REGIME_LDS, FS_REGIME_SAMPLED, FS_REGIME_GLOBAL = range(4)
FS_MAGIC, FS_H_NCAL, FS_H_OFFSET = 0x46534554, 16, 40
FS_T_N, FS_T_COVERED, FS_T_HIST, FS_T_SINGLE, FS_T_OUT_N, FS_T_OUT_NOVEL, FS_TALLY_WORDS = 0, 16, 144, 280, 288, 289, 304

# pinn_changepoint.hip: limits, the prefix tile, the solver's step block, the default cap of a launch, cost kinds and status bits
CP_MAX_FEAT, CP_MAX_PEN, CP_MAX_SEGMENTS, CP_MAX_WINDOW, CP_TILE, CP_BLOCK, CP_LAUNCH_EVALS = 8, 16, 65535, 4096, 256, 64, 1 << 24
CP_MEAN, CP_MEANVAR, CP_BAD_ROW, CP_OVERFLOW, CP_INFEASIBLE = 0, 1, 1, 2, 4


class CpOpts(ctypes.Structure):
    """pinn_cp_opts_t (pinn_changepoint.hip)."""
    _fields_ = [("kind", c_int), ("min_len", c_int), ("max_len", c_ll), ("prune", c_int), ("block_steps", c_int),
                ("var_floor", ctypes.c_double), ("launch_evals", c_ll)]


class PinnError(RuntimeError):
    pass


class PinnRangeError(PinnError):
    """A weight or gradient left the domain of the split-operand precisions (include/pinn_hip.h: PINN_E_RANGE)."""


E_RANGE = -4


# the head of every entry point that reads rows of the results array in place (_device._DevRows.head()):
# array, leading dimension, rows of the array, columns, their number, gather index or NULL, rows to read
_ROWS = [c_void_p, c_ll, c_ll, ctypes.POINTER(c_int), c_int, c_void_p, c_ll]
# what follows it in the pinn_gmm_batch_* entry points: candidates, their component counts (host array), the largest count
_BATCH = [c_int, ctypes.POINTER(c_int), c_int]
# the head of the pinn_lr_batch_* entry points: array, leading dimension, rows of the array, gather index or NULL, rows to
# read, class indices, classes; candidates, their feature counts and column lists (host arrays), the largest count, and the
# device copies of both lists
_LR_BATCH = [c_void_p, c_ll, c_ll, c_void_p, c_ll, c_void_p, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_int,
             c_void_p, c_void_p]
# what follows it in pinn_unc_score / pinn_unc_quantiles: label column, label table (host array), labels, groups
_UNC_GROUPS = [c_int, ctypes.POINTER(c_int), c_int, c_int]
_c_dp = ctypes.POINTER(ctypes.c_double)    # a host array of float64
_c_llp = ctypes.POINTER(c_ll)              # a host array of int64
# what pinn_fs_rank and pinn_fs_gmm share from the calibration state on: state, table sizes and thresholds (host arrays), levels,
# kind, randomized, seed, draw kind, first row, regime; classes or NULL; count, mask, size, novel, missing, scores, tallies
_FS_RANK = [c_void_p, _c_llp, _c_llp, c_int, c_int, c_int, ctypes.c_ulonglong, c_int, c_ll, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
            c_void_p, c_void_p, c_void_p, c_void_p]

# what pinn_cp_segment and pinn_cp_window share from the options on: options, penalties (host array), their number; F, change
# point counts, change points, their capacity, evaluations, status; workspace and its size
_CP_TAIL = [ctypes.POINTER(CpOpts), _c_dp, c_int, c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_size_t]

_SIGS = {
    "pinn_abi_version": (c_int, []),
    "pinn_residuals_workspace_bytes": (c_size_t, []),
    "pinn_residuals": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(Affine), c_void_p, c_uint, c_ll, c_void_p, c_ll,
                               c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lambda_step": (c_int, [c_int, c_void_p, c_ll, c_float, c_float, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_lambda_stage_run": (c_int, [c_int, ctypes.c_uint, c_void_p, c_void_p, c_void_p, ctypes.POINTER(Affine), c_ll, ctypes.c_double,
                                      ctypes.c_double, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lambda_stage_workspace_bytes": (c_size_t, [c_ll]),
    "pinn_param_count": (c_ll, [ctypes.POINTER(Net)]),
    "pinn_packed_bytes": (c_size_t, [ctypes.POINTER(Net)]),
    "pinn_net_range_status": (c_int, [ctypes.POINTER(Net), c_void_p]),
    "pinn_mlp_forward": (c_int, [ctypes.POINTER(Net), c_void_p, c_void_p, c_ll, ctypes.POINTER(Dropout), c_void_p, c_void_p,
                                 c_void_p]),
    "pinn_mc_dropout": (c_int, [ctypes.POINTER(Net), c_void_p, c_void_p, c_ll, ctypes.POINTER(Dropout), c_int, c_void_p,
                                c_void_p, c_void_p, c_void_p]),
    "pinn_train_workspace_bytes": (c_size_t, [ctypes.POINTER(Net), c_ll]),
    "pinn_grad_split": (c_ll, [ctypes.POINTER(Net)]),
    "pinn_mlp_train_grads": (c_int, [ctypes.POINTER(Net), c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_mlp_train_grads_phases": (c_int, [ctypes.POINTER(Net), c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                            c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_uint]),
    "pinn_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_float, c_int, c_void_p]),
    "pinn_adam_coeffs": (None, [c_float, c_int, ctypes.POINTER(c_float), ctypes.POINTER(c_float)]),
    "pinn_adam_step_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_void_p]),
    "pinn_mlp_train_step_dev": (c_int, [ctypes.POINTER(Net), c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_mlp_train_step": (c_int, [ctypes.POINTER(Net), c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                    c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "pinn_residuals_prepare": (c_int, [c_void_p, c_void_p, c_void_p, ctypes.POINTER(Affine), c_void_p, c_uint, c_ll, c_void_p, c_void_p]),
    "pinn_residuals_cached": (c_int, [c_void_p, ctypes.POINTER(Affine), c_void_p, c_uint, c_ll, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_net_f_t": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(Affine), c_void_p, c_ll, c_void_p, c_void_p, c_void_p,
                             c_void_p]),
    "pinn_residuals_backward": (c_int, [c_void_p, c_void_p, ctypes.POINTER(Affine), c_void_p, c_uint, c_ll, c_void_p, c_ll, c_uint, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_net_f_t_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.POINTER(Affine), c_void_p, c_ll, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gnet_param_count": (c_ll, [ctypes.POINTER(GNet)]),
    "pinn_gnet_workspace_bytes": (c_size_t, [ctypes.POINTER(GNet), c_ll, c_int]),
    "pinn_gnet_forward": (c_int, [ctypes.POINTER(GNet), c_void_p, c_void_p, c_ll, ctypes.POINTER(Dropout), c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    "pinn_gnet_mc_dropout": (c_int, [ctypes.POINTER(GNet), c_void_p, c_void_p, c_ll, ctypes.POINTER(Dropout), c_int, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gnet_train_grads": (c_int, [ctypes.POINTER(GNet), c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gnet_train_step": (c_int, [ctypes.POINTER(GNet), c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "pinn_gnet_backward": (c_int, [ctypes.POINTER(GNet), c_void_p, c_void_p, c_ll, ctypes.POINTER(Dropout), c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gnet_backward2_workspace_bytes": (c_size_t, [ctypes.POINTER(GNet), c_ll]),
    "pinn_gnet_backward2": (c_int, [ctypes.POINTER(GNet), c_void_p, c_void_p, c_ll, ctypes.POINTER(Dropout), c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gens_workspace_bytes": (c_size_t, [ctypes.POINTER(GNet), c_int, c_ll]),
    "pinn_gens_train_plan": (c_int, [ctypes.POINTER(GNet), c_ll, ctypes.POINTER(c_ll), ctypes.POINTER(c_int)]),
    "pinn_gens_forward": (c_int, [ctypes.POINTER(GNet), c_int, c_void_p, c_void_p, c_ll, ctypes.POINTER(Dropout), c_void_p, c_void_p,
                                  c_void_p, c_size_t, c_void_p]),
    "pinn_gens_train_grads": (c_int, [ctypes.POINTER(GNet), c_int, c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                      c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gens_train_step": (c_int, [ctypes.POINTER(GNet), c_int, c_void_p, c_void_p, c_void_p, c_ll, c_ll, ctypes.POINTER(Dropout),
                                     c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_float, c_int, c_void_p]),
    "pinn_gens_combine": (c_int, [c_void_p, c_void_p, c_int, c_ll, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_results_assemble": (c_int, [c_void_p, c_void_p, ctypes.POINTER(Affine), ctypes.c_double, ctypes.c_double, c_int, c_void_p, c_int,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_ll, c_void_p, c_void_p]),
    "pinn_rf_stats_workspace_bytes": (c_size_t, []),
    "pinn_rf_stats": (c_int, [c_void_p, c_ll, c_ll, ctypes.POINTER(c_int), c_int, c_int, ctypes.POINTER(c_ll), c_int, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_rf_workspace_bytes": (c_size_t, [c_ll, c_ll]),
    "pinn_rf_series": (c_int, [c_void_p, c_ll, c_ll, ctypes.POINTER(RFParams), c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_rf_sweep_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_rf_sweep": (c_int, [c_void_p, c_ll, c_ll, ctypes.POINTER(RFParams), c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                              c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_rf_first_alarm": (c_int, [c_void_p, c_ll, c_ll, c_void_p, c_ll, c_void_p, c_ll, c_int, c_int, ctypes.c_double, c_void_p,
                                    c_void_p]),
    "pinn_gmm_state_bytes": (c_size_t, [c_int, c_int]),
    "pinn_gmm_workspace_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_gmm_mstep_init": (c_int, _ROWS + [c_int, c_void_p, c_void_p, ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_em": (c_int, _ROWS + [c_int, c_int, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_kmeans": (c_int, _ROWS + [c_int, c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_label_map": (c_int, _ROWS + [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_posterior": (c_int, _ROWS + [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_gmm_batch_state_stride": (c_size_t, [c_int, c_int]),
    "pinn_gmm_batch_workspace_bytes": (c_size_t, [c_ll, c_int, c_int, c_int]),
    "pinn_gmm_batch_seed": (c_int, _ROWS + _BATCH + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_batch_kmeans": (c_int, _ROWS + _BATCH + [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_batch_mstep_init": (c_int, _ROWS + _BATCH + [c_void_p, ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_batch_em": (c_int, _ROWS + _BATCH + [c_int, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_gmm_batch_score": (c_int, _ROWS + _BATCH + [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lr_state_bytes": (c_size_t, [c_int, c_int]),
    "pinn_lr_workspace_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_lr_scaler": (c_int, _ROWS + [c_void_p, c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lr_pass": (c_int, _ROWS + [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lr_newton": (c_int, _ROWS + [c_void_p, c_int, c_int, ctypes.c_double, ctypes.c_double, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lr_posterior": (c_int, _ROWS + [c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_lr_roc_workspace_bytes": (c_size_t, [c_ll]),
    "pinn_lr_roc": (c_int, [c_void_p, c_void_p, c_ll, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_size_t, c_void_p]),
    "pinn_lr_batch_state_stride": (c_size_t, [c_int, c_int]),
    "pinn_lr_batch_workspace_bytes": (c_size_t, [c_ll, c_int, c_int, c_int]),
    "pinn_lr_batch_scaler": (c_int, _LR_BATCH + [c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lr_batch_newton": (c_int, _LR_BATCH + [c_int, ctypes.c_double, ctypes.c_double, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lr_batch_score": (c_int, _LR_BATCH + [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_lr_batch_auc": (c_int, [c_void_p, c_void_p, c_ll, c_int, c_void_p, c_void_p]),
    "pinn_km_state_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_km_workspace_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_km_lloyd": (c_int, _ROWS + [c_int, c_int, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_cluster_means": (c_int, _ROWS + [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_ward_state_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_ward_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_ward_tree": (c_int, _ROWS + [c_int, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_cluster_assign": (c_int, _ROWS + [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_if_forest_bytes": (c_size_t, [c_int, c_int]),
    "pinn_if_score": (c_int, _ROWS + [c_void_p, ctypes.c_double, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "pinn_if_fit": (c_int, _ROWS + [c_int, c_int, c_int, ctypes.c_ulonglong, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p]),
    "pinn_svm_state_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_svm_workspace_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_svm_pass": (c_int, _ROWS + [c_void_p, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_svm_ipm": (c_int, _ROWS + [c_void_p, c_int, c_int, c_int, ctypes.c_double, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_svm_decision": (c_int, _ROWS + [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_ksvm_state_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_ksvm_workspace_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_ksvm_smo": (c_int, _ROWS + [c_void_p, c_int, ctypes.c_double, c_int, c_int, ctypes.c_double, c_void_p, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "pinn_ksvm_finish": (c_int, _ROWS + [c_void_p, c_int, c_void_p, c_void_p]),
    "pinn_ksvm_decision": (c_int, _ROWS + [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_ll, c_void_p, ctypes.c_double, c_void_p, c_void_p,
                                           c_void_p, c_void_p]),
    "pinn_tsne_state_bytes": (c_size_t, [c_ll]),
    "pinn_tsne_workspace_bytes": (c_size_t, [c_ll]),
    "pinn_tsne_affinities": (c_int, _ROWS + [ctypes.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_tsne_kl_grad": (c_int, [c_ll, c_void_p, ctypes.c_double, c_void_p, c_size_t, c_void_p]),
    "pinn_tsne_descend": (c_int, [c_ll, c_int, c_int, c_int, ctypes.c_double, ctypes.c_double, c_int, ctypes.c_double, c_void_p, c_void_p,
                                  c_size_t, c_void_p]),
    "pinn_sp_knn": (c_int, _ROWS + [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_sp_affinity_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_sp_affinity": (c_int, [c_ll, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_sp_eigs_state_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_sp_eigs_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_sp_eigs": (c_int, [c_ll, c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_int, c_int, c_int, ctypes.c_double, c_void_p, c_void_p,
                             c_size_t, c_void_p]),
    "pinn_sp_embed": (c_int, [c_ll, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_sp_lloyd_state_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_sp_lloyd_workspace_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_sp_lloyd": (c_int, [c_void_p, c_ll, c_int, c_int, c_int, c_int, ctypes.c_double, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_auc_components_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_auc_components": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_auc_cross_sums_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_auc_cross_sums": (c_int, [c_void_p, c_ll, c_ll, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_auc_bootstrap_workspace_bytes": (c_size_t, [c_ll, c_int, ctypes.POINTER(c_ll)]),
    "pinn_auc_bootstrap": (c_int, [c_void_p, c_void_p, c_ll, c_ll, c_int, ctypes.POINTER(c_ll), ctypes.c_ulonglong, c_ll, c_ll, c_void_p,
                                   c_void_p, c_size_t, c_void_p]),
    "pinn_shap_gmm_workspace_bytes": (c_size_t, [c_ll, c_ll, c_int, c_int]),
    "pinn_shap_gmm": (c_int, _ROWS + _ROWS + [c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_shap_hybrid": (c_int, _ROWS + _ROWS + [c_ll, c_ll, c_int, c_void_p, c_void_p]),
    "pinn_shap_reduce": (c_int, [c_void_p, c_int, c_ll, c_int, c_ll, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_hmm_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_hmm_forward_backward": (c_int, _ROWS + [c_void_p, c_void_p, c_ll, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                  c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_hmm_viterbi": (c_int, _ROWS + [c_void_p, c_void_p, c_ll, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_hmm_mstep": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_ll, c_void_p, ctypes.c_double, c_int, c_void_p]),
    "pinn_id_fit": (c_int, [c_void_p, c_ll, c_ll, ctypes.POINTER(c_int), c_int, c_void_p, c_ll, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                            ctypes.POINTER(IdOpts), c_void_p, c_void_p, c_void_p]),
    "pinn_bp_fit": (c_int, [c_void_p, c_ll, c_ll, ctypes.POINTER(c_int), c_void_p, c_ll, c_void_p, c_void_p, c_ll, c_ll,
                            ctypes.POINTER(BpOpts), c_void_p, c_void_p]),
    "pinn_unc_workspace_bytes": (c_size_t, [c_ll, c_int, c_int]),
    "pinn_unc_state_bytes": (c_size_t, [c_int]),
    "pinn_unc_score": (c_int, _ROWS + _UNC_GROUPS + [_c_dp, _c_dp, c_int, _c_dp, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_unc_quantiles": (c_int, _ROWS + _UNC_GROUPS + [_c_dp, c_int, c_int, _c_dp, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                         c_void_p, c_size_t, c_void_p]),
    "pinn_unc_update": (c_int, _ROWS + [_c_dp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_int, c_int, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_fs_state_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_fs_workspace_bytes": (c_size_t, [c_ll, c_int]),
    "pinn_fs_build": (c_int, [c_void_p, c_void_p, c_void_p, c_ll, c_int, c_int, ctypes.c_ulonglong, c_int, c_void_p, c_void_p, c_size_t, c_void_p]),
    "pinn_fs_rank": (c_int, [c_void_p, c_ll, c_int] + _FS_RANK + [c_void_p]),
    "pinn_fs_gmm": (c_int, _ROWS + [c_int, c_void_p, c_void_p, c_int, c_void_p] + _FS_RANK + [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "pinn_cp_workspace_bytes": (c_size_t, [c_ll, c_int, c_ll, c_int]),
    "pinn_cp_segment": (c_int, _ROWS + [_c_dp, _c_dp, _c_llp, c_void_p, c_ll] + _CP_TAIL + [c_void_p]),
    "pinn_cp_window": (c_int, [c_void_p, c_ll, c_ll, ctypes.POINTER(c_int), c_int, c_ll, c_ll, _c_dp, _c_dp] + _CP_TAIL + [c_void_p]),
}

_lib = None


def lib_path():
    return _build.LIB


def load(build_if_missing=True):
    """Load (building first if needed and possible) the HIP library. Raises if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    # torch must be imported BEFORE the library: torch bundles its own HIP runtime (libamdhip64.so.7);
    # loading ours first would pull /opt/rocm's copy as a second runtime, and streams / device
    # pointers from torch are meaningless to a different runtime instance (hipErrorNoDevice).
    import torch  # noqa: F401
    path = _build.LIB
    override = os.environ.get("PINN_HIP_LIB")      # experiments: load another build of the same ABI
    if override:
        path, build_if_missing = override, False
    if build_if_missing:
        try:
            path = _build.build()          # no-op when the library matches the sources (content hashes)
        except _build.NoCompiler:
            # a box without hipcc may only run a library that was built from exactly these sources;
            # a compile or link FAILURE (BuildError) always propagates: never run a stale binary
            if not _build.is_current():
                raise PinnError("libpinn_hip.so is missing or does not match the sources in %s, and hipcc is not "
                                "available to rebuild it" % _build.CSRC)
    if not os.path.exists(path):
        raise PinnError("libpinn_hip.so is missing (%s): build it with __graft_entry__.build()" % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)          # AttributeError if the library does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.pinn_abi_version() != 2:
        raise PinnError("libpinn_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise PinnError("%s failed with code %d" % (what, rc))


def declared_symbols():
    return list(_SIGS.keys())
