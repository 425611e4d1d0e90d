"""MI355X-native PINN training + MC-dropout hot path (gfx950 HIP kernels behind a C ABI).

Public surface mirrors the reference's `01_train_pinn_multiphysics_model.py`:
`PhysicsInformedNN`, `DNN`, `get_MC_samples`, `create_comprehensive_results_array_v2`,
`create_fault_labels`, `smooth_by_segments`, `_moving_average_centered`; the steps either side of the hot path:
`load_data_normal_raw`, `load_data_fault_raw`, `combine_and_normalize_datasets`, `add_noise_to_combined_data` (ingest),
`plot_model_results_detailed_split` (its statistics; no figure), and `save_checkpoint` / `load_checkpoint`; and the
stage after the results array, script 04's risk function: `estimate_mu_sigma_normal`, `compute_rf_time_series`,
`find_first_alarm_index`, `compute_rf_advance_for_condition`, with `rf_advance_for_conditions`, `RiskMonitor` and the calibration of its parameters, `rf_grid`, `rf_sweep`, `calibrate_rf` (risk); and script 03's Gaussian-mixture
fault diagnosis: `fit_gmm_and_get_probabilities`, `extract_X_y`, the spec parsers, with `DeviceGMM`, `FaultDiagnoser` and
`classification_metrics` (diagnosis); and script 02's fault detection: `build_classifier`, `explain_coefficients`, with
`DeviceStandardScaler`, `DeviceLogisticRegression`, `roc_curve`, `auc`, `auc_score`, `stratified_split`,
`evaluate_feature_groups`, `FaultDetector`, and script 05's `run_supervised_lr`, `compute_macro_metrics` (detection; its
`parse_features` and `parse_group_spec` are script 02's variants and stay in the submodule); and the rest of script 05, the method comparison:
`fit_kmeans_posterior`, `fit_agglomerative_posterior`, `fit_gmm_and_get_predictions`, `load_data_for_fault_4class`, with
`DeviceKMeans`, `DeviceWard`, `compare_methods` and `ClusterDiagnoser` (comparison); and script 02's unsupervised detector, the
isolation forest: `DeviceIsolationForest` and `AnomalyMonitor` (anomaly); and script 05's Sup_SVM, a one-vs-one linear SVC solved
by interior point: `run_supervised_svm_rbf`, with `DeviceLinearSVC`, `build_svm_classifier` and `SVMDiagnoser` (svm), reached
from `compare_methods` through `device_extras` (comparison); and the t-SNE embeddings of scripts 02 and 03, the exact method:
`DeviceTSNE`, `joint_probabilities`, `kl_and_gradient`, `trustworthiness`, `tsne_of_test_samples`, `scatter_by_features`,
`TSNE_PARAMS` (embedding); and script 05's Spectral, spectral clustering of a k-nearest-neighbour graph:
`fit_spectral_posterior`, with `DeviceSpectralClustering`, `knn_graph`, `knn_affinity` and `spectral_embedding` (spectral),
reached from `compare_methods` through `spectral_extras` (comparison); and the RBF-kernel SVC that script 05 names for Sup_SVM
(it runs the linear one), one-vs-one and solved by SMO in float64: `run_supervised_svm_kernel`, with `DeviceKernelSVC`,
`build_kernel_svm_classifier` and `KernelSVMDiagnoser` (ksvm), reached from `compare_methods` through `kernel_extras` (comparison);
and what script 02's four AUCs leave open, their intervals and paired tests: `auc_components`, `delong_covariance`, `auc_ci`,
`delong_test`, `compare_aucs`, `bootstrap_auc`, `compare_feature_groups` (rocstat); and the choice of the mixture's size and
seed, all candidates fitted and scored in one batch: `gmm_sweep`, `select_gmm`, `GMMSweep` (selection); and the choice of script 02's feature group, every column subset of
a pool fitted and scored in one batch: `feature_subsets`, `feature_sweep`, `select_features`, `forward_select`,
`FeatureSweep`, `ForwardPath` (featsel); and the question after
a diagnosis, which input made the model say so, as exact Shapley values over all coalitions: `shapley_diagnosis`,
`shapley_values`, `voltage_predictor`, `DiagnosisExplainer`, `global_importance`, `top_features` (explain); and the time
axis every per-row diagnosis ignores, a hidden Markov chain over the fault classes with the posteriors as emissions:
`DeviceHMM` (filter, smoother, Viterbi path, Baum-Welch for the transitions), `TemporalDiagnoser`, `sticky_transitions`,
`transitions_from_labels`, `scaled_likelihood` (temporal); and which physical quantity of the stack moved, the polarisation
and thermal parameters identified per window with covariances: `voltage_table`, `thermal_table`, `sliding_windows`,
`fit_windows`, `fit_baseline`, `drift`, `WindowFit`, `ParameterTracker` (identify); and the same question for the two
starvation faults, the hydrogen and oxygen excess-ratio laws fitted per window with their breakpoint by exact enumeration:
`flow_table`, `fit_breakpoints`, `fit_breakpoint_baseline`, `BreakpointFit`, `SupplyTracker`, `supply_law` (supply); and
whether the voltage network's own standard deviations are honest, reliability scores, exact conformal quantiles and an online
band: `score_uncertainty`, `conformal_quantiles`, `conformal_band`, `UncertaintyMonitor`, `UncertaintyReport`, `Quantiles`
(uncertainty); and how sure the diagnosis itself is and whether it is none of the trained faults, conformal fault sets with
class-conditional coverage and unknown-fault rejection: `calibrate`, `calibrate_gmm`, `p_values`, `prediction_sets`,
`evaluate_sets`, `GMMSetDiagnoser`, `SetCalibration`, `FaultSets`, `SetReport` (faultsets); and a second source of the
epistemic column beside MC-dropout, E networks trained and evaluated in the launches of one: `DeepEnsemble` (ensemble); and
where the regimes of a recording begin when nobody typed the boundaries, exact penalised change-point segmentation of the
residual columns: `segment`, `penalty_path`, `select_penalty`, `segment_table`, `labels_from_segments`, `diagnose_segments`,
`ChangeMonitor` (changepoint).
Submodules are imported lazily so that `pinn_amd.synth` (numpy only) works without torch/HIP.
"""
import importlib

_LAZY = {
    "DNN": "model", "PhysicsInformedNN": "model",
    "get_MC_samples": "mc",
    "create_comprehensive_results_array_v2": "results", "create_fault_labels": "results",
    "smooth_by_segments": "results", "_moving_average_centered": "results",
    "add_noise_to_combined_data": "ingest", "load_data_normal_raw": "ingest", "load_data_fault_raw": "ingest",
    "combine_and_normalize_datasets": "ingest",
    "model_statistics": "report", "plot_model_results_detailed_split": "report",
    "save_checkpoint": "report", "load_checkpoint": "report",
    "estimate_mu_sigma_normal": "risk", "compute_rf_time_series": "risk", "find_first_alarm_index": "risk",
    "compute_rf_advance_for_condition": "risk", "rf_advance_for_conditions": "risk", "rf_series": "risk", "RiskMonitor": "risk",
    "rf_grid": "risk", "rf_sweep": "risk", "calibrate_rf": "risk", "RFSweep": "risk", "RFCalibration": "risk",
    "DeviceGMM": "diagnosis", "FaultDiagnoser": "diagnosis", "fit_gmm_and_get_probabilities": "diagnosis",
    "classification_metrics": "diagnosis", "extract_X_y": "diagnosis", "parse_features": "diagnosis",
    "parse_group_spec": "diagnosis", "build_label_mapper": "diagnosis", "normalize_feature_spec": "diagnosis",
    "DeviceStandardScaler": "detection", "DeviceLogisticRegression": "detection", "build_classifier": "detection",
    "explain_coefficients": "detection", "roc_curve": "detection", "auc": "detection", "auc_score": "detection",
    "stratified_split": "detection", "evaluate_feature_groups": "detection", "FaultDetector": "detection",
    "run_supervised_lr": "detection", "compute_macro_metrics": "detection",
    "DeviceKMeans": "comparison", "DeviceWard": "comparison", "compare_methods": "comparison", "ClusterDiagnoser": "comparison",
    "fit_kmeans_posterior": "comparison", "fit_agglomerative_posterior": "comparison", "fit_gmm_and_get_predictions": "comparison",
    "load_data_for_fault_4class": "comparison", "cluster_class_map": "comparison", "assign_clusters": "comparison",
    "CLASS_NAMES_EN": "comparison", "N_CLASSES": "comparison",
    "DeviceIsolationForest": "anomaly", "AnomalyMonitor": "anomaly",
    "DeviceLinearSVC": "svm", "run_supervised_svm_rbf": "svm", "build_svm_classifier": "svm", "SVMDiagnoser": "svm",
    "device_extras": "comparison",
    "DeviceKernelSVC": "ksvm", "run_supervised_svm_kernel": "ksvm", "build_kernel_svm_classifier": "ksvm", "KernelSVMDiagnoser": "ksvm",
    "kernel_extras": "comparison",
    "DeviceTSNE": "embedding", "joint_probabilities": "embedding", "kl_and_gradient": "embedding", "trustworthiness": "embedding",
    "tsne_of_test_samples": "embedding", "scatter_by_features": "embedding", "TSNE_PARAMS": "embedding",
    "DeviceSpectralClustering": "spectral", "fit_spectral_posterior": "spectral", "knn_graph": "spectral", "knn_affinity": "spectral",
    "spectral_embedding": "spectral", "spectral_extras": "comparison",
    "auc_components": "rocstat", "delong_covariance": "rocstat", "auc_ci": "rocstat", "delong_test": "rocstat",
    "compare_aucs": "rocstat", "bootstrap_auc": "rocstat", "compare_feature_groups": "rocstat",
    "gmm_sweep": "selection", "select_gmm": "selection", "GMMSweep": "selection",
    "feature_subsets": "featsel", "feature_sweep": "featsel", "select_features": "featsel", "forward_select": "featsel",
    "FeatureSweep": "featsel", "ForwardPath": "featsel",
    "shapley_values": "explain", "shapley_diagnosis": "explain", "voltage_predictor": "explain", "DiagnosisExplainer": "explain",
    "global_importance": "explain", "top_features": "explain", "Shapley": "explain",
    "DeviceHMM": "temporal", "TemporalDiagnoser": "temporal", "sticky_transitions": "temporal",
    "transitions_from_labels": "temporal", "scaled_likelihood": "temporal",
    "voltage_table": "identify", "thermal_table": "identify", "sliding_windows": "identify", "fit_windows": "identify",
    "fit_baseline": "identify", "drift": "identify", "WindowFit": "identify", "ParameterTracker": "identify",
    "flow_table": "supply", "fit_breakpoints": "supply", "fit_breakpoint_baseline": "supply", "BreakpointFit": "supply",
    "SupplyTracker": "supply", "supply_law": "supply",
    "score_uncertainty": "uncertainty", "conformal_quantiles": "uncertainty", "conformal_band": "uncertainty",
    "UncertaintyMonitor": "uncertainty", "UncertaintyReport": "uncertainty", "Quantiles": "uncertainty",
    "calibrate": "faultsets", "calibrate_gmm": "faultsets", "p_values": "faultsets", "prediction_sets": "faultsets",
    "evaluate_sets": "faultsets", "GMMSetDiagnoser": "faultsets", "SetCalibration": "faultsets", "FaultSets": "faultsets",
    "SetReport": "faultsets", "PValues": "faultsets",
    "DeepEnsemble": "ensemble",
    "segment": "changepoint", "default_penalty": "changepoint", "penalty_path": "changepoint", "select_penalty": "changepoint",
    "segment_table": "changepoint", "labels_from_segments": "changepoint", "diagnose_segments": "changepoint",
    "ChangeMonitor": "changepoint", "Segmentation": "changepoint", "PenaltyPath": "changepoint",
}


def __getattr__(name):
    if name in _LAZY:
        return getattr(importlib.import_module("." + _LAZY[name], __name__), name)
    try:
        return importlib.import_module("." + name, __name__)
    except ModuleNotFoundError as e:
        raise AttributeError(name) from e
