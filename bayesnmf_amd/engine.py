"""ctypes binding of the C ABI in include/bnmf.h (libbnmf.so, HIP/gfx950 only).

This is the Python equivalent of the R `.Call` shim in r/bnmf_shim.c: logic-free marshalling.
There is no CPU fallback: if the library is missing or no GPU is visible the calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbnmf.so")
_LIB = None

NMETRIC = 11
NKERNEL = 8
METRIC_NAMES = ["iter", "RMSE", "KL", "loglikelihood", "logposterior", "n_params", "BIC",
                "rank", "temp", "P_mean_acceptance_rate", "E_mean_acceptance_rate"]
IDS = dict(P=0, E=1, A=2, R=3, Z=4, ZsumK=5, ZsumG=6, sigmasq=7,
           Alpha_p=10, Beta_p=11, Alpha_e=12, Beta_e=13, Mu_p=14, Sigmasq_p=15, Mu_e=16,
           Sigmasq_e=17, Lambda_p=18, Lambda_e=19, Alpha=20, Beta=21,
           A_p=30, B_p=31, C_p=32, D_p=33, M_p=34, S_p=35,
           A_e=40, B_e=41, C_e=42, D_e=43, M_e=44, S_e=45,
           P_acceptance_rate=50, E_acceptance_rate=51, Mhat=60)
LIKELIHOOD = dict(poisson=0, normal=1)
PRIOR = dict(truncnormal=0, exponential=1, gamma=2)
RANK_METHOD = dict(SBFI=0, BFI=1)
MATH_FN = dict(log=0, exp=1, lgamma=2, digamma=3, qnorm=4, log_pnorm=5, sqrt=6, recip=7)
SAMPLER = dict(rgamma=0, rtnorm0=1, rnorm=2, ralpha=3, runif=4, rexp=5, ralpha_fast=6, ralpha_fast_wave=7, rpois=8)


class BnmfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libbnmf error {code}: {msg}")
        self.code = code


class BnmfConfig(C.Structure):
    _fields_ = [("K", C.c_int32), ("G", C.c_int32), ("N", C.c_int32),
                ("likelihood", C.c_int32), ("prior", C.c_int32), ("MH", C.c_int32),
                ("learning_rank", C.c_int32), ("rank_method", C.c_int32),
                ("save_Z", C.c_int32), ("window", C.c_int32),
                ("seed", C.c_uint64), ("chain_id", C.c_uint32), ("device", C.c_int32),
                ("temperature", C.POINTER(C.c_double)), ("n_temperature", C.c_int64)]


# every symbol include/bnmf.h declares (checked by tests/test_abi.py)
class BnmfMapInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_patterns", C.c_int32), ("top_counts", C.c_int32 * 5), ("_pad", C.c_int32),
                ("rmse", C.c_double), ("kl", C.c_double)]


class BnmfConvergenceControl(C.Structure):
    _fields_ = [("MAP_over", C.c_int32), ("MAP_every", C.c_int32), ("Ninarow_nochange", C.c_int32), ("Ninarow_nobest", C.c_int32),
                ("miniters", C.c_int32), ("maxiters", C.c_int32), ("metric", C.c_int32), ("_pad", C.c_int32), ("tol", C.c_double)]


class BnmfConvergenceState(C.Structure):
    _fields_ = [("converged", C.c_int32), ("why", C.c_int32), ("best_iter", C.c_int32), ("inarow_na", C.c_int32),
                ("inarow_no_change", C.c_int32), ("inarow_no_best", C.c_int32), ("have_prev", C.c_int32), ("n_checks", C.c_int32),
                ("prev_MAP_metric", C.c_double), ("best_MAP_metric", C.c_double), ("prev_percent_change", C.c_double)]


class BnmfStateDesc(C.Structure):
    _fields_ = [("K", C.c_int32), ("G", C.c_int32), ("N", C.c_int32), ("likelihood", C.c_int32), ("prior", C.c_int32), ("MH", C.c_int32),
                ("learning_rank", C.c_int32), ("rank_method", C.c_int32), ("save_Z", C.c_int32), ("window", C.c_int32),
                ("seed", C.c_uint64), ("chain_id", C.c_uint32), ("format_version", C.c_int32), ("n_temperature", C.c_int64),
                ("data_hash", C.c_uint64), ("temperature_hash", C.c_uint64), ("first_iter", C.c_int32), ("last_iter", C.c_int32),
                ("n_records", C.c_int32), ("_pad", C.c_int32), ("bytes", C.c_int64)]


class BnmfWaicInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_high_var", C.c_int32), ("lppd", C.c_double), ("p_waic", C.c_double),
                ("elpd_waic", C.c_double), ("waic", C.c_double), ("se_elpd", C.c_double), ("mean_loglik", C.c_double)]


class BnmfMixingInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_half", C.c_int32), ("n_const", C.c_int64), ("n_ran_out", C.c_int64), ("n_low_ess", C.c_int64),
                ("n_high_rhat", C.c_int64), ("min_ess_P_at", C.c_int64), ("min_ess_E_at", C.c_int64), ("max_rhat_P_at", C.c_int64),
                ("max_rhat_E_at", C.c_int64), ("min_ess_P", C.c_double), ("min_ess_E", C.c_double), ("max_rhat_P", C.c_double),
                ("max_rhat_E", C.c_double)]


class BnmfPpcInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_tail_cells", C.c_int64), ("p_T1", C.c_double), ("p_T2", C.c_double),
                ("mean_T1_obs", C.c_double), ("mean_T1_rep", C.c_double), ("mean_T2_obs", C.c_double), ("mean_T2_rep", C.c_double)]


class BnmfAttrInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("_pad", C.c_int32), ("n_present", C.c_int64), ("min_load", C.c_double), ("total", C.c_double)]


class BnmfProjectInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_steps", C.c_int32), ("n_present", C.c_int64), ("min_load", C.c_double), ("total", C.c_double),
                ("max_rel_change", C.c_double), ("min_cosine", C.c_double), ("min_cosine_at", C.c_int64)]


class BnmfDecomposeInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_steps", C.c_int32), ("R", C.c_int32), ("_pad", C.c_int32), ("n_present", C.c_int64),
                ("min_share", C.c_double), ("max_rel_change", C.c_double), ("min_cosine", C.c_double), ("min_cosine_at", C.c_int64)]


class BnmfContrastInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_groups", C.c_int32), ("n_pairs", C.c_int32), ("n_left_out", C.c_int32), ("n_credible", C.c_int64 * 3),
                ("min_load", C.c_double), ("credible_interval", C.c_double)]


class BnmfRegressInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("Q", C.c_int32), ("n_included", C.c_int32), ("n_left_out", C.c_int32), ("n_blocks", C.c_int32),
                ("min_pivot_at", C.c_int32), ("n_credible", (C.c_int64 * 16) * 3), ("credible_interval", C.c_double), ("min_pivot_ratio", C.c_double)]


class BnmfCoactivityInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_included", C.c_int32), ("n_left_out", C.c_int32), ("n_pairs", C.c_int32), ("n_blocks", C.c_int32),
                ("_pad", C.c_int32), ("n_credible", C.c_int64 * 3), ("max_cosine_at", C.c_int64), ("max_cosine", C.c_double),
                ("min_load", C.c_double), ("credible_interval", C.c_double)]


class BnmfStabilityInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_points", C.c_int32), ("n_extra", C.c_int32), ("n_left_out", C.c_int32), ("n_clusters", C.c_int32),
                ("min_stability_at", C.c_int32), ("n_negative", C.c_int64), ("mean_silhouette", C.c_double), ("min_stability", C.c_double)]


class BnmfReconstructionInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_undefined", C.c_int32), ("n_poor", C.c_int64), ("n_needed", C.c_int64), ("worst_at", C.c_int64),
                ("min_cosine", C.c_double), ("min_drop", C.c_double), ("worst_cosine", C.c_double)]


class BnmfSimilarityInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_included", C.c_int32), ("n_left_out", C.c_int32), ("top_k", C.c_int32), ("n_query", C.c_int32),
                ("_pad", C.c_int32), ("n_pairs", C.c_int64), ("n_similar_pairs", C.c_int64), ("n_isolated", C.c_int64),
                ("least_typical_at", C.c_int64), ("mean_similarity", C.c_double), ("least_typical", C.c_double), ("min_cosine", C.c_double)]


class BnmfSubtypesInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_matched", C.c_int32), ("n_unmatched", C.c_int32), ("n_included", C.c_int32), ("n_left_out", C.c_int32),
                ("C", C.c_int32), ("n_steps", C.c_int32), ("n_query", C.c_int32), ("n_not_converged", C.c_int32), ("n_certain", C.c_int32),
                ("n_never_assigned", C.c_int32), ("smallest_subtype_at", C.c_int32), ("least_certain_at", C.c_int64), ("mean_certainty", C.c_double),
                ("least_certain", C.c_double), ("smallest_subtype", C.c_double), ("min_certainty", C.c_double)]


class BnmfResidualsInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_flat", C.c_int32), ("n_included", C.c_int32), ("n_left_out", C.c_int32), ("n_steps", C.c_int32),
                ("n_biased", C.c_int32), ("n_overdispersed", C.c_int32), ("worst_type_at", C.c_int32), ("min_agreement_at", C.c_int32), ("_pad", C.c_int32),
                ("lambda", C.c_double), ("share", C.c_double), ("move", C.c_double), ("mean_share", C.c_double), ("min_agreement", C.c_double),
                ("worst_type", C.c_double), ("max_dispersion", C.c_double)]


class BnmfTradeoffInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_matched", C.c_int32), ("n_unmatched", C.c_int32), ("n_included", C.c_int32), ("n_left_out", C.c_int32),
                ("n_sets", C.c_int32), ("n_query", C.c_int32), ("n_traded", C.c_int32), ("strongest_pair_at", C.c_int32), ("_pad", C.c_int32),
                ("strongest_pair", C.c_double), ("mean_ratio", C.c_double), ("min_corr", C.c_double)]


class BnmfPruneInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_included", C.c_int32), ("n_undefined", C.c_int32), ("n_single", C.c_int32), ("n_steps", C.c_int32),
                ("_pad", C.c_int32), ("trials", C.c_int64), ("max_change", C.c_double), ("max_loss", C.c_double)]


class BnmfSummaryInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_aligned", C.c_int32), ("n_included", C.c_int32), ("n_left_out", C.c_int32), ("n_levels", C.c_int32),
                ("n_blocks", C.c_int32), ("n_nonfinite", C.c_int64), ("min_load", C.c_double), ("credible_interval", C.c_double)]


class BnmfRelabelInfo(C.Structure):
    _fields_ = [("n_used", C.c_int32), ("n_aligned", C.c_int32), ("n_unmatched", C.c_int32), ("rounds", C.c_int32), ("converged", C.c_int32),
                ("n_switched", C.c_int32), ("n_changed_last", C.c_int32), ("_pad", C.c_int32), ("mean_cosine", C.c_double),
                ("min_cosine", C.c_double), ("min_cosine_at", C.c_int64)]


ATTR_LOAD_ROWS = ["load_mean", "load_var", "share", "p_present"]
PROJ_FIT_ROWS = ["cosine", "rel_l1", "rel_change"]
DEC_WEIGHT_ROWS = ["weight_mean", "weight_var", "share", "p_present"]
CON_STATS = ["load", "share", "prevalence"]
CON_GROUP_ROWS = ["mean", "var", "lower", "upper"]
CON_PAIR_ROWS = ["mean", "var", "lower", "upper", "p_greater", "p_less"]
CON_MAX_GROUPS = 64
REG_STATS = ["load", "share", "sqrt_load"]
REG_COEF_ROWS = ["mean", "var", "lower", "upper", "p_greater", "p_less"]
REG_FIT_ROWS = ["r2_mean", "r2_lower", "r2_upper", "r2_samples", "sigma2_mean"]
REG_MAX_Q = 16
COA_STATS = ["pearson", "spearman", "copresence", "cosine"]
COA_PAIR_ROWS = ["mean", "var", "lower", "upper", "p_greater", "p_less", "n_valid"]
STAB_POINT_ROWS = ["silhouette", "a", "b", "nearest"]
STAB_FACTOR_ROWS = ["members", "stability", "min_silhouette", "mean_a", "mean_b", "share_negative"]
REC_TUMOUR_ROWS = ["cosine", "cosine_var", "min_cosine_sample", "rel_l1", "rmse", "p_good"]
REC_DROP_ROWS = ["drop_mean", "drop_var", "loo_cosine", "p_needed"]
REC_SIGNATURE_ROWS = ["n_tumours", "mean_drop", "max_drop"]
SIM_ROWS = ["mean", "var", "p_similar"]
SIM_TUMOUR_ROWS = ["typicality", "nearest_mean", "degree"]
SIM_MAX_K = 32
SUB_TUMOUR_ROWS = ("certainty", "assigned", "runner_up")
SUB_ROWS = ("mean", "var", "lower", "upper")
SUB_SERIES_ROWS = ("inertia", "steps", "n_assigned")
RES_TYPE_ROWS = ("bias", "bias_var", "p_positive", "dispersion", "dispersion_var")
RES_COMPONENT_ROWS = ("vbar", "mean", "var", "p_positive")
RES_TUMOUR_ROWS = ("score", "score_var", "chi")
RES_SERIES_ROWS = ("trace", "lambda", "share", "move", "agreement")
TRD_TUMOUR_ROWS = ("min_corr", "n_defined", "total_ratio")
TRD_PAIR_ROWS = ("mean_corr", "n_defined", "p_negative", "p_positive", "mean_cov")
TRD_SET_ROWS = ("mean", "var_sum", "sum_var", "ratio")
TRD_MAX_C = 32
PRN_LOAD_ROWS = ("load_mean", "load_var", "share", "p_kept")
PRN_TUMOUR_ROWS = ("cos_0", "cos_f", "n_kept", "n_kept_min", "n_kept_max", "rel_change", "mean_trials")
PRN_SERIES_ROWS = ("n_kept", "cos_f")
PRN_SIGNATURE_ROWS = ("n_tumours", "mean_p_kept", "total_load")
SUM_SCALARS = ("prevalence", "total", "fraction", "mean_present")
SUM_FAMILIES = ("load_all", "load_present", "share_all")
SUM_ROWS = ("mean", "var", "lower", "upper", "n_valid")
SUM_MAX_Q = 8
PPC_COL_ROWS = ["T1_obs_col", "T1_rep_col", "p_T1_col", "T2_obs_col", "T2_rep_col", "p_T2_col"]
PPC_SERIES_ROWS = ["T1_obs", "T1_rep", "T2_obs", "T2_rep"]
PPC_CELL_ROWS = ["mean_cell", "var_cell", "p_less_cell", "p_equal_cell"]
NMIX = 11
MIX_ROWS = ["mean", "var", "ess", "mcse", "rhat", "pairs", "exit", "mean_a", "var_a", "mean_b", "var_b"]
NMAPROW = 17
CC_METRICS = ["loglikelihood", "logposterior", "RMSE", "KL", "BIC"]
WHY = {0: None, 1: "no change", 2: "no best", 3: "max iters"}

ABI_SYMBOLS = ["bnmf_create", "bnmf_create_f64", "bnmf_destroy", "bnmf_set_array", "bnmf_get_array", "bnmf_get_array_i32",
               "bnmf_init", "bnmf_run", "bnmf_window", "bnmf_map", "bnmf_run_until", "bnmf_run_post_warmup", "bnmf_assign", "bnmf_map_at",
               "bnmf_assign_at", "bnmf_label_switching", "bnmf_get_iter", "bnmf_profile",
               "bnmf_kernel_name", "bnmf_ubench", "bnmf_test_math", "bnmf_test_sampler", "bnmf_test_philox", "bnmf_test_philox7",
               "bnmf_device_info", "bnmf_device_count", "bnmf_last_error", "bnmf_version", "bnmf_probe_overlap", "bnmf_trim", "bnmf_get_stat",
               "bnmf_save_state", "bnmf_load_state", "bnmf_state_info", "bnmf_set_fixed", "bnmf_get_fixed",
               "bnmf_waic", "bnmf_waic_at", "bnmf_mixing", "bnmf_mixing_at", "bnmf_ppc", "bnmf_ppc_at",
               "bnmf_attribution", "bnmf_attribution_at", "bnmf_relabel", "bnmf_relabel_at", "bnmf_project", "bnmf_project_at",
               "bnmf_decompose", "bnmf_decompose_at", "bnmf_contrast", "bnmf_contrast_at", "bnmf_regress", "bnmf_regress_at",
               "bnmf_coactivity", "bnmf_coactivity_at", "bnmf_stability", "bnmf_stability_at",
               "bnmf_reconstruction", "bnmf_reconstruction_at", "bnmf_similarity", "bnmf_similarity_at",
               "bnmf_subtypes", "bnmf_subtypes_at", "bnmf_residuals", "bnmf_residuals_at",
               "bnmf_tradeoff", "bnmf_tradeoff_at", "bnmf_prune", "bnmf_prune_at", "bnmf_summary", "bnmf_summary_at"]


def lib():
    """Load libbnmf.so; raises (never falls back) when it has not been built."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise BnmfError(-100, f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
        L.bnmf_create.argtypes = [C.POINTER(BnmfConfig), ip, C.POINTER(C.c_void_p)]
        L.bnmf_create_f64.argtypes = [C.POINTER(BnmfConfig), dp, C.POINTER(C.c_void_p)]
        L.bnmf_destroy.argtypes = [C.c_void_p]
        L.bnmf_set_array.argtypes = [C.c_void_p, C.c_int, dp, C.c_size_t]
        L.bnmf_get_array.argtypes = [C.c_void_p, C.c_int, dp, C.c_size_t]
        L.bnmf_get_array_i32.argtypes = [C.c_void_p, C.c_int, ip, C.c_size_t]
        L.bnmf_init.argtypes = [C.c_void_p, dp]
        L.bnmf_run.argtypes = [C.c_void_p, C.c_int, C.c_int, dp]
        L.bnmf_window.argtypes = [C.c_void_p, C.c_int, C.c_int, dp]
        L.bnmf_map.argtypes = [C.c_void_p, C.c_int, C.c_double, dp, dp, dp, dp, dp, dp, dp, dp, ip, C.POINTER(BnmfMapInfo)]
        L.bnmf_run_until.argtypes = [C.c_void_p, C.POINTER(BnmfConvergenceControl), C.POINTER(BnmfConvergenceState), dp, C.c_int,
                                     C.POINTER(C.c_int), dp, C.c_int, C.POINTER(C.c_int)]
        L.bnmf_run_post_warmup.argtypes = [C.c_void_p, C.POINTER(BnmfConvergenceControl), C.POINTER(BnmfConvergenceState), C.c_int, dp, C.c_int,
                                           C.POINTER(C.c_int), dp, C.c_int, C.POINTER(C.c_int)]
        L.bnmf_assign.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_int, ip, dp, C.c_double, dp, ip, dp, dp, dp]
        L.bnmf_map_at.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, dp, dp, dp, dp, dp, dp, dp, dp, ip, C.POINTER(BnmfMapInfo)]
        L.bnmf_assign_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp, C.c_int, ip, dp, C.c_double, dp, ip, dp, dp, dp]
        L.bnmf_label_switching.argtypes = [C.c_void_p, ip, C.c_int, dp, C.c_int, ip, dp, ip]
        L.bnmf_get_iter.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.bnmf_profile.argtypes = [C.c_void_p, C.c_int, C.c_int, dp]
        L.bnmf_kernel_name.restype = C.c_char_p
        L.bnmf_kernel_name.argtypes = [C.c_int]
        L.bnmf_ubench.argtypes = [C.c_int, dp, dp]
        L.bnmf_test_math.argtypes = [C.c_int, C.c_int, dp, dp, C.c_size_t]
        L.bnmf_test_sampler.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_uint32, dp, dp, dp, dp, C.c_size_t]
        L.bnmf_test_philox.argtypes = [C.c_int, up, up, up]
        L.bnmf_test_philox7.argtypes = [C.c_int, up, up, up]
        L.bnmf_device_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        L.bnmf_device_count.restype = C.c_int
        L.bnmf_probe_overlap.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.bnmf_trim.argtypes = [C.c_int, C.POINTER(C.c_size_t)]
        L.bnmf_get_stat.argtypes = [C.c_void_p, C.c_int, dp]
        L.bnmf_save_state.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_size_t)]
        L.bnmf_load_state.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]
        L.bnmf_state_info.argtypes = [C.c_char_p, C.POINTER(BnmfStateDesc)]
        L.bnmf_set_fixed.argtypes = [C.c_void_p, C.c_int, ip, C.c_size_t]
        L.bnmf_get_fixed.argtypes = [C.c_void_p, C.c_int, ip, C.c_size_t]
        L.bnmf_waic.argtypes = [C.c_void_p, C.c_int, ip, dp, dp, C.POINTER(BnmfWaicInfo)]
        L.bnmf_waic_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp, dp, C.POINTER(BnmfWaicInfo)]
        L.bnmf_mixing.argtypes = [C.c_void_p, C.c_int, ip, ip, dp, dp, C.POINTER(BnmfMixingInfo)]
        L.bnmf_mixing_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, dp, dp, C.POINTER(BnmfMixingInfo)]
        L.bnmf_ppc.argtypes = [C.c_void_p, C.c_int, ip, dp, dp, dp, C.POINTER(BnmfPpcInfo)]
        L.bnmf_ppc_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp, dp, dp, C.POINTER(BnmfPpcInfo)]
        L.bnmf_attribution.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, dp, dp, dp, C.POINTER(BnmfAttrInfo)]
        L.bnmf_attribution_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, C.c_double, dp, dp, dp, C.POINTER(BnmfAttrInfo)]
        L.bnmf_project.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_int, C.c_int, C.c_double, dp, dp, dp, dp, C.POINTER(BnmfProjectInfo)]
        L.bnmf_project_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp, C.c_int, C.c_int, C.c_double, dp, dp, dp, dp, C.POINTER(BnmfProjectInfo)]
        L.bnmf_decompose.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_int, ip, C.c_int, C.c_double, dp, dp, ip, ip, dp, C.POINTER(BnmfDecomposeInfo)]
        L.bnmf_decompose_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp, C.c_int, ip, C.c_int, C.c_double, dp, dp, ip, ip, dp,
                                        C.POINTER(BnmfDecomposeInfo)]
        L.bnmf_contrast.argtypes = [C.c_void_p, C.c_int, ip, ip, C.c_double, C.c_double, dp, dp, dp, ip, C.POINTER(BnmfContrastInfo)]
        L.bnmf_contrast_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, C.c_double, C.c_double, dp, dp, dp, ip, C.POINTER(BnmfContrastInfo)]
        L.bnmf_regress.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_int, ip, C.c_double, dp, dp, dp, dp, C.POINTER(BnmfRegressInfo)]
        L.bnmf_regress_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp, C.c_int, ip, C.c_double, dp, dp, dp, dp, C.POINTER(BnmfRegressInfo)]
        L.bnmf_coactivity.argtypes = [C.c_void_p, C.c_int, ip, ip, C.c_double, C.c_double, dp, dp, C.POINTER(BnmfCoactivityInfo)]
        L.bnmf_coactivity_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, C.c_double, C.c_double, dp, dp, C.POINTER(BnmfCoactivityInfo)]
        lp = C.POINTER(C.c_int64)
        L.bnmf_stability.argtypes = [C.c_void_p, C.c_int, ip, ip, dp, ip, C.c_int, dp, dp, dp, dp, lp, C.POINTER(BnmfStabilityInfo)]
        L.bnmf_stability_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, dp, ip, C.c_int, dp, dp, dp, dp, lp, C.POINTER(BnmfStabilityInfo)]
        L.bnmf_reconstruction.argtypes = [C.c_void_p, C.c_int, ip, C.c_double, C.c_double, dp, dp, dp, dp, C.POINTER(BnmfReconstructionInfo)]
        L.bnmf_reconstruction_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, C.c_double, C.c_double, dp, dp, dp, dp, C.POINTER(BnmfReconstructionInfo)]
        L.bnmf_similarity.argtypes = [C.c_void_p, C.c_int, ip, ip, ip, C.c_int, C.c_int, C.c_double, ip, dp, dp, dp, C.POINTER(BnmfSimilarityInfo)]
        L.bnmf_similarity_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, ip, C.c_int, C.c_int, C.c_double, ip, dp, dp, dp, C.POINTER(BnmfSimilarityInfo)]
        sub = [ip, ip, ip, dp, C.c_int, C.c_int, ip, C.c_int, C.c_double, dp, ip, dp, dp, dp, dp, ip, dp, C.POINTER(BnmfSubtypesInfo)]
        L.bnmf_subtypes.argtypes = [C.c_void_p, C.c_int] + sub
        L.bnmf_subtypes_at.argtypes = [C.c_void_p, C.c_int, C.c_int] + sub
        res = [ip, ip, C.c_int, C.c_double, dp, dp, dp, dp, dp, C.POINTER(BnmfResidualsInfo)]
        L.bnmf_residuals.argtypes = [C.c_void_p, C.c_int] + res
        L.bnmf_residuals_at.argtypes = [C.c_void_p, C.c_int, C.c_int] + res
        trd = [ip, ip, ip, ip, C.c_int, ip, C.c_int, C.c_double, dp, ip, dp, dp, dp, C.POINTER(BnmfTradeoffInfo)]
        L.bnmf_tradeoff.argtypes = [C.c_void_p, C.c_int] + trd
        L.bnmf_tradeoff_at.argtypes = [C.c_void_p, C.c_int, C.c_int] + trd
        prn = [ip, ip, C.c_int, C.c_double, dp, dp, dp, dp, dp, C.POINTER(BnmfPruneInfo)]
        L.bnmf_prune.argtypes = [C.c_void_p, C.c_int] + prn
        L.bnmf_prune_at.argtypes = [C.c_void_p, C.c_int, C.c_int] + prn
        smy = [ip, ip, ip, C.c_double, dp, C.c_int, C.c_double, dp, dp, C.POINTER(BnmfSummaryInfo)]
        L.bnmf_summary.argtypes = [C.c_void_p, C.c_int] + smy
        L.bnmf_summary_at.argtypes = [C.c_void_p, C.c_int, C.c_int] + smy
        L.bnmf_relabel.argtypes = [C.c_void_p, C.c_int, ip, dp, C.c_int, ip, dp, lp, dp, dp, dp, dp, C.POINTER(BnmfRelabelInfo)]
        L.bnmf_relabel_at.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, dp, C.c_int, ip, dp, lp, dp, dp, dp, dp, C.POINTER(BnmfRelabelInfo)]
        L.bnmf_last_error.restype = C.c_char_p
        L.bnmf_version.restype = C.c_int
        _LIB = L
    return _LIB


_RUN = None


def _run_fn():
    """bnmf_run with plain-integer argument types (handle and buffer as addresses): no per-call conversion objects"""
    global _RUN
    if _RUN is None:
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p)
        _RUN = proto(("bnmf_run", lib()))
    return _RUN


def _chk(rc):
    if rc != 0:
        raise BnmfError(rc, lib().bnmf_last_error().decode())


_IP = C.POINTER(C.c_int32)


def _dp(a):
    """Pointer to a float64 array's data; None stays None (an optional argument of the ABI)."""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def device_count():
    return lib().bnmf_device_count()


def ubench(device=0):
    """Measured ceilings: (Philox4x32-10 words/s with nothing else in the loop, device-to-device copy GB/s)."""
    a, b = C.c_double(), C.c_double()
    _chk(lib().bnmf_ubench(device, C.byref(a), C.byref(b)))
    return a.value, b.value


def trim(device=0):
    """Release what destroyed handles left cached on the device (rings, streams); returns the bytes of device memory given back."""
    b = C.c_size_t(0)
    _chk(lib().bnmf_trim(device, C.byref(b)))
    return b.value


def state_info(path):
    """Validate a chain state file (every checksum) and describe it, without a handle or a device (bnmf_state_info)."""
    d = BnmfStateDesc()
    _chk(lib().bnmf_state_info(os.fsencode(path), C.byref(d)))
    out = {name: getattr(d, name) for name, _ in BnmfStateDesc._fields_ if name != "_pad"}
    inv = lambda m, v: next(k for k, x in m.items() if x == v)   # noqa: E731
    out.update(likelihood=inv(LIKELIHOOD, d.likelihood), prior=inv(PRIOR, d.prior), rank_method=inv(RANK_METHOD, d.rank_method),
               MH=bool(d.MH), learning_rank=bool(d.learning_rank), save_Z=bool(d.save_Z))
    return out


def device_info(device=0):
    buf = C.create_string_buffer(512)
    _chk(lib().bnmf_device_info(device, buf, 512))
    return buf.value.decode()


def test_math(fn, x, device=0):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    _chk(lib().bnmf_test_math(device, MATH_FN[fn], _dp(x), _dp(out), x.size))
    return out


def test_sampler(which, a=None, b=None, c=None, n=None, seed=1, chain=0, var=2, elem0=0, it=1, device=0):
    arrs = []
    for v in (a, b, c):
        if v is None:
            arrs.append(None)
        else:
            arrs.append(np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64),
                                                             (n,) if n else np.shape(a)), dtype=np.float64))
    if n is None:
        n = arrs[0].size
    out = np.empty(n)
    _chk(lib().bnmf_test_sampler(device, SAMPLER[which], seed, chain, var, elem0, it,
                                 *[_dp(v) if v is not None else None for v in arrs], _dp(out), n))
    return out


def test_philox(ctr, key, device=0, rounds=10):
    c = (C.c_uint32 * 4)(*ctr)
    k = (C.c_uint32 * 2)(*key)
    o = (C.c_uint32 * 4)()
    _chk((lib().bnmf_test_philox7 if rounds == 7 else lib().bnmf_test_philox)(device, c, k, o))
    return [int(v) for v in o]


class Engine:
    """One chain on one MI355X.  Thin wrapper: every method is one C-ABI call."""

    def __init__(self, M, N, likelihood="poisson", prior="gamma", MH=False, learning_rank=False,
                 rank_method="SBFI", seed=1, chain_id=0, temperature=None, save_Z=False,
                 window=0, device=0):
        # Normal: the data as float64, any real value (bnmf_create_f64); Poisson: int32 counts (bnmf_create)
        normal = likelihood == "normal"
        M = np.asfortranarray(M, dtype=np.float64 if normal else np.int32)
        self.K, self.G = M.shape
        self.N = int(N)
        self._temp = None if temperature is None else np.ascontiguousarray(temperature, dtype=np.float64)
        cfg = BnmfConfig(self.K, self.G, self.N, LIKELIHOOD[likelihood], PRIOR[prior], int(MH),
                         int(learning_rank), RANK_METHOD[rank_method], int(save_Z), int(window),
                         int(seed), int(chain_id), int(device),
                         _dp(self._temp) if self._temp is not None else None,
                         0 if self._temp is None else self._temp.size)
        h = C.c_void_p()
        if normal:
            _chk(lib().bnmf_create_f64(C.byref(cfg), _dp(M), C.byref(h)))
        else:
            _chk(lib().bnmf_create(C.byref(cfg), M.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h)))
        self._h = h
        self._hv = h.value
        self._run = _run_fn()
        self.M = M

    def close(self):
        if getattr(self, "_h", None):
            lib().bnmf_destroy(self._h)
            self._h = None
            self._hv = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _shape(self, name):
        K, G, N = self.K, self.G, self.N
        if name == "A":
            return (1, N)
        if name == "R":
            return (1,)
        if name == "Z":
            return (K, N, G)
        if name in ("sigmasq", "Alpha", "Beta"):
            return (G,)
        if name == "Mhat":
            return (K, G)
        if name in ("P", "ZsumG", "P_acceptance_rate") or name.endswith("_p"):
            return (K, N)
        return (N, G)

    def set(self, name, value):
        v = np.asarray(value, dtype=np.float64)
        flat = np.ascontiguousarray(v.ravel(order="F"))
        _chk(lib().bnmf_set_array(self._h, IDS[name], _dp(flat), flat.size))

    def get(self, name):
        shp = self._shape(name)
        n = int(np.prod(shp))
        if name in ("Z", "ZsumK", "ZsumG"):
            out = np.empty(n, dtype=np.int32)
            _chk(lib().bnmf_get_array_i32(self._h, IDS[name], out.ctypes.data_as(C.POINTER(C.c_int32)), n))
        else:
            out = np.empty(n)
            _chk(lib().bnmf_get_array(self._h, IDS[name], _dp(out), n))
        return out.reshape(shp, order="F")

    def set_fixed(self, name, mask):
        """Hold the columns of P flagged in mask (length N, 0 / 1) at the value set("P", ...) gives them (bnmf_set_fixed); before
        init() / load_state()."""
        m = np.asarray(mask)
        if m.dtype.kind == "f" and not (m == np.floor(m)).all():
            raise BnmfError(-1, "set_fixed: the mask holds a value that is neither 0 nor 1")
        m = np.ascontiguousarray(m.ravel(), dtype=np.int32)
        _chk(lib().bnmf_set_fixed(self._h, IDS[name], m.ctypes.data_as(C.POINTER(C.c_int32)), m.size))

    def get_fixed(self, name):
        """The mask of fixed columns (bnmf_get_fixed): int32, length N; zeros if none was set."""
        out = np.empty(self.N, dtype=np.int32)
        _chk(lib().bnmf_get_fixed(self._h, IDS[name], out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
        return out

    def init(self):
        row = np.empty(NMETRIC)
        _chk(lib().bnmf_init(self._h, _dp(row)))
        return row

    def run(self, n_iter, converged=False, metrics=True):
        out = np.empty((n_iter, NMETRIC)) if metrics else None
        # (the hot call of every driver loop: the bound function and the handle's integer value are looked up once, the buffer goes in as
        # its address — the generic path cost 16 us per call, 1 % of a 20-iteration call at the metric configuration)
        rc = self._run(self._hv, n_iter, 1 if converged else 0, out.ctypes.data if metrics else None)
        if rc != 0:
            _chk(rc)
        return out

    def profile(self, n_iter, converged=False):
        out = np.zeros(NKERNEL)
        _chk(lib().bnmf_profile(self._h, n_iter, int(converged), _dp(out)))
        return {lib().bnmf_kernel_name(i).decode(): out[i] for i in range(NKERNEL)}

    def window(self, name, last_n):
        shp = self._shape(name)
        out = np.empty((last_n, int(np.prod(shp))))
        _chk(lib().bnmf_window(self._h, IDS[name], last_n, _dp(out)))
        return [out[i].reshape(shp, order="F") for i in range(last_n)]

    def run_until(self, cc, state=None):
        """Warm-up to convergence in one C-ABI call.  cc: new_convergence_control() dict; state: BnmfConvergenceState to
        continue from (None = fresh).  Returns (metrics rows, MAP rows [n_checks x NMAPROW], state)."""
        c = BnmfConvergenceControl(cc["MAP_over"], cc["MAP_every"], cc["Ninarow_nochange"], cc["Ninarow_nobest"], cc["miniters"],
                                   cc["maxiters"], CC_METRICS.index(cc["metric"]), 0, cc["tol"])
        st = state or BnmfConvergenceState()
        cap_rows = max(cc["maxiters"] - self.iter, 0) + 1
        cap_checks = cap_rows // cc["MAP_every"] + 2
        rows, maps = np.empty((cap_rows, NMETRIC)), np.empty((cap_checks, NMAPROW))
        nr, nc = C.c_int(), C.c_int()
        _chk(lib().bnmf_run_until(self._h, C.byref(c), C.byref(st), _dp(rows), cap_rows, C.byref(nr), _dp(maps), cap_checks, C.byref(nc)))
        return rows[:nr.value].copy(), maps[:nc.value].copy(), st

    def run_post_warmup(self, cc, state, post_warmup):
        """The MH models' post-warm-up tail in one C-ABI call.  Returns (metrics rows, MAP rows, state)."""
        c = BnmfConvergenceControl(cc["MAP_over"], cc["MAP_every"], cc["Ninarow_nochange"], cc["Ninarow_nobest"], cc["miniters"],
                                   cc["maxiters"], CC_METRICS.index(cc["metric"]), 0, cc["tol"])
        cap_rows = int(post_warmup) + 1
        cap_checks = cap_rows // cc["MAP_every"] + 3
        rows, maps = np.empty((cap_rows, NMETRIC)), np.empty((cap_checks, NMAPROW))
        nr, nc = C.c_int(), C.c_int()
        _chk(lib().bnmf_run_post_warmup(self._h, C.byref(c), C.byref(state), int(post_warmup), _dp(rows), cap_rows, C.byref(nr), _dp(maps),
                                        cap_checks, C.byref(nc)))
        return rows[:nr.value].copy(), maps[:nc.value].copy(), state

    # ---- the posterior calls on a recorded range: three helpers, then one method per call ----
    def _used(self, name, used, last_n):
        """The used argument of call `name`: (pointer to its int32 copy or None, S = the number of used samples)."""
        if used is None:
            return None, max(int(last_n), 0)
        u = np.ascontiguousarray(used, dtype=np.int32)
        if u.size != last_n:
            raise BnmfError(-2, f"{name}: used has {u.size} entries for {last_n} samples")
        return u.ctypes.data_as(_IP), int((u != 0).sum())       # (the pointer keeps u alive)

    def _range_call(self, name, last_n, end_iter, *args):
        """bnmf_<name> over the last `last_n` samples, or with end_iter bnmf_<name>_at over the `last_n` that end at iteration end_iter."""
        if end_iter is None:
            _chk(getattr(lib(), "bnmf_" + name)(self._h, last_n, *args))
        else:
            _chk(getattr(lib(), "bnmf_" + name + "_at")(self._h, int(end_iter), last_n, *args))

    @staticmethod
    def _info(info):
        return {name: getattr(info, name) for name, _ in info._fields_ if name != "_pad"}

    def assign(self, last_n, reference_P, used=None, keep=None, MAP_P=None, credible_interval=0.95, end_iter=None):
        """assign_signatures_ensemble_ over recorded samples: votes (N x R), assigned reference per signature (-1 = not
        kept), cosine of the MAP estimate and credible bounds of the per-sample cosines.  The samples are the last `last_n`
        recorded ones, or with end_iter the `last_n` that end at iteration end_iter (bnmf_assign_at)."""
        N = self.N
        ref = np.asfortranarray(reference_P, dtype=np.float64)
        R = ref.shape[1]
        u = None if used is None else np.ascontiguousarray(used, dtype=np.int32)
        kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.int32)
        mp = None if MAP_P is None else np.asfortranarray(MAP_P, dtype=np.float64)
        votes, asg = np.zeros(N * R), np.empty(N, dtype=np.int32)
        mc, lo, hi = np.empty(N), np.empty(N), np.empty(N)
        self._range_call("assign", last_n, end_iter, None if u is None else u.ctypes.data_as(_IP), _dp(ref.ravel(order="F")), R,
                         None if kp is None else kp.ctypes.data_as(_IP), None if mp is None else _dp(mp.ravel(order="F")),
                         float(credible_interval), _dp(votes), asg.ctypes.data_as(_IP), _dp(mc), _dp(lo), _dp(hi))
        return dict(votes=votes.reshape((N, R), order="F"), assigned=asg, MAP_cosine=mc, lower_cosine=lo, upper_cosine=hi)

    def map(self, last_n, credible_interval=0.95, end_iter=None):
        """get_MAP_ over the last `last_n` recorded samples, or with end_iter the `last_n` that end at iteration end_iter
        (bnmf_map_at), on the device (one C-ABI call)."""
        K, G, N = self.K, self.G, self.N
        Pm, Em, Am, top = np.empty(K * N), np.empty(N * G), np.empty(N), np.empty(5 * N)
        ci = credible_interval is not None and credible_interval > 0
        Pl, Pu, El, Eu = (np.empty(K * N), np.empty(K * N), np.empty(N * G), np.empty(N * G)) if ci else (None,) * 4
        used = np.empty(last_n, dtype=np.int32)
        info = BnmfMapInfo()
        self._range_call("map", last_n, end_iter, float(credible_interval) if ci else 0.0, _dp(Pm), _dp(Em), _dp(Am), _dp(top),
                         _dp(Pl), _dp(Pu), _dp(El), _dp(Eu), used.ctypes.data_as(_IP), C.byref(info))
        f = lambda a, shp: None if a is None else a.reshape(shp, order="F")   # noqa: E731
        npat = min(info.n_patterns, 5)
        return dict(P=f(Pm, (K, N)), E=f(Em, (N, G)), A=Am.reshape(1, N), used=used.astype(bool),
                    P_lower=f(Pl, (K, N)), P_upper=f(Pu, (K, N)), E_lower=f(El, (N, G)), E_upper=f(Eu, (N, G)),
                    top_A=top.reshape(5, N)[:npat], top_counts=[int(c) for c in info.top_counts][:npat],
                    n_used=info.n_used, n_patterns=info.n_patterns, rmse=info.rmse, kl=info.kl)

    def waic(self, last_n, used=None, end_iter=None, pointwise=False):
        """WAIC over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last `last_n`, or with
        end_iter of the `last_n` that end at iteration end_iter (bnmf_waic / bnmf_waic_at), on the device.  Returns the info fields;
        with pointwise also lppd_col, p_waic_col, mean_loglik_col (G) and lppd_cell, p_waic_cell (K x G)."""
        K, G = self.K, self.G
        u, _ = self._used("waic", used, last_n)
        col = np.empty(3 * G) if pointwise else None
        cell = np.empty(2 * K * G) if pointwise else None
        info = BnmfWaicInfo()
        self._range_call("waic", last_n, end_iter, u, _dp(col), _dp(cell), C.byref(info))
        out = self._info(info)
        if pointwise:
            out.update(lppd_col=col[:G], p_waic_col=col[G:2 * G], mean_loglik_col=col[2 * G:],
                       lppd_cell=cell[:K * G].reshape((K, G), order="F"), p_waic_cell=cell[K * G:].reshape((K, G), order="F"))
        return out

    def ppc(self, last_n, used=None, end_iter=None, pointwise=False):
        """Posterior predictive checks over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last
        `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_ppc / bnmf_ppc_at), on the device.  Returns the
        info fields, col (6 x G) with its rows also by name (PPC_COL_ROWS: the mean over the used samples of T on the data and on the
        replicate and p = #(T_rep >= T_obs) / S, for T1 and T2), series (4 x S) with its rows by name (PPC_SERIES_ROWS: the whole-matrix
        values per used sample); with pointwise also mean_cell, var_cell, p_less_cell, p_equal_cell and pit = p_less + 0.5 p_equal (K x G)."""
        K, G = self.K, self.G
        u, S = self._used("ppc", used, last_n)
        col = np.empty((6, G))
        series = np.empty((4, S))
        cell = np.empty((4, K * G)) if pointwise else None
        info = BnmfPpcInfo()
        self._range_call("ppc", last_n, end_iter, u, _dp(col), _dp(cell), _dp(series), C.byref(info))
        out = self._info(info)
        out.update(col=col, series=series)
        out.update({name: col[i] for i, name in enumerate(PPC_COL_ROWS)})
        out.update({name: series[i] for i, name in enumerate(PPC_SERIES_ROWS)})
        if pointwise:
            out.update({name: cell[i].reshape((K, G), order="F") for i, name in enumerate(PPC_CELL_ROWS)})
            out["pit"] = out["p_less_cell"] + 0.5 * out["p_equal_cell"]
        return out

    def attribution(self, last_n, used=None, end_iter=None, min_load=1.0, prob=False):
        """Signature attribution over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last
        `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_attribution / bnmf_attribution_at), on the
        device.  Returns the info fields, load (4 x N x G) with its rows also by name (ATTR_LOAD_ROWS: the mean and variance over the
        used samples of the mutations of tumour g attributed to factor n, the mean share of the tumour's load, and the fraction of
        samples whose load is >= min_load), series (S x N: the cohort's load per used sample and factor); with prob also prob
        (K x N x G: the probability that a mutation of type k in tumour g came from factor n)."""
        K, G, N = self.K, self.G, self.N
        u, S = self._used("attribution", used, last_n)
        load = np.empty((4, N * G))
        series = np.empty((S, N))
        pr = np.empty(K * N * G) if prob else None
        info = BnmfAttrInfo()
        self._range_call("attribution", last_n, end_iter, u, float(min_load), _dp(load), _dp(pr), _dp(series), C.byref(info))
        out = self._info(info)
        out.update(load=np.stack([row.reshape((N, G), order="F") for row in load]), series=series)
        out.update({name: out["load"][i] for i, name in enumerate(ATTR_LOAD_ROWS)})
        if prob:
            out["prob"] = pr.reshape((K, N, G), order="F")
        return out

    def project(self, last_n, X, used=None, end_iter=None, n_steps=200, min_load=1.0, exposures=False):
        """Exposures of the new tumours X (K x J, not negative) under the signatures of the recorded samples flagged in used (length
        last_n, oldest first; None = all) of the last `last_n`, or with end_iter of the `last_n` that end at iteration end_iter
        (bnmf_project / bnmf_project_at), on the device: every column is refitted to every sample's renormalised signatures by n_steps
        steps of the KL multiplicative update.  Returns the info fields, load (4 x N x J) with its rows also by name (ATTR_LOAD_ROWS:
        the mean and variance over the used samples of the exposure of tumour j to factor n, its mean share of the tumour, and the
        fraction of samples whose exposure is >= min_load), fit (3 x J) with its rows by name (PROJ_FIT_ROWS: the mean cosine and mean
        relative L1 error of the fit, the largest relative change of the last step), series (S x N: the exposures summed over the new
        tumours); with exposures also exposures (S x N x J), every used sample's own."""
        K, N = self.K, self.N
        Xf = np.asfortranarray(X, dtype=np.float64)
        if Xf.ndim != 2 or Xf.shape[0] != K:
            raise BnmfError(-2, f"project: X has shape {Xf.shape}, K = {K} rows are needed")
        J = Xf.shape[1]
        u, S = self._used("project", used, last_n)
        load, fit, series = np.empty((4, N * J)), np.empty((3, J)), np.empty((S, N))
        ex = np.empty((S, N * J)) if exposures else None
        info = BnmfProjectInfo()
        self._range_call("project", last_n, end_iter, u, _dp(Xf.ravel(order="F")), J, int(n_steps), float(min_load), _dp(load), _dp(fit), _dp(series),
                         _dp(ex), C.byref(info))
        out = self._info(info)
        out.update(load=np.stack([row.reshape((N, J), order="F") for row in load]), fit=fit, series=series)
        out.update({name: out["load"][i] for i, name in enumerate(ATTR_LOAD_ROWS)})
        out.update({name: fit[i] for i, name in enumerate(PROJ_FIT_ROWS)})
        if exposures:
            out["exposures"] = np.stack([row.reshape((N, J), order="F") for row in ex]) if S else np.empty((0, N, J))
        return out

    def decompose(self, last_n, reference_P, used=None, end_iter=None, keep=None, n_steps=200, min_share=0.05, weights=False):
        """The recorded signatures as mixtures of the references reference_P (K x R, not negative, no all-zero column), over the recorded
        samples flagged in used (length last_n, oldest first; None = all) of the last `last_n`, or with end_iter of the `last_n` that end
        at iteration end_iter (bnmf_decompose / bnmf_decompose_at), on the device: every renormalised column of every sample's P is
        refitted to the normalised catalogue by n_steps steps of the KL multiplicative update, the references below min_share of the
        column are dropped and n_steps more steps refit the rest (min_share = 0: no pruning, one stage).  keep (length N, None = all):
        the factors to decompose.  Returns the info fields, weight (4 x R x N) with its rows also by name (DEC_WEIGHT_ROWS: the mean and
        variance over the used samples of the weight of reference r in factor n, its mean share of the factor, and the fraction of
        samples whose weight is >= min_share), fit (3 x N) with its rows by name (PROJ_FIT_ROWS), nactive (S x N: the references left
        per sample and factor) and included (N: the samples in which the factor took part); with weights also weights (S x R x N),
        every used sample's own."""
        K, N = self.K, self.N
        ref = np.asfortranarray(reference_P, dtype=np.float64)
        if ref.ndim != 2 or ref.shape[0] != K:
            raise BnmfError(-2, f"decompose: reference_P has shape {ref.shape}, K = {K} rows are needed")
        R = ref.shape[1]
        u, S = self._used("decompose", used, last_n)
        kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.int32)
        if kp is not None and kp.size != N:
            raise BnmfError(-2, f"decompose: keep has {kp.size} entries for {N} factors")
        weight, fit = np.empty((4, R * N)), np.empty((3, N))
        nact, inc = np.empty((S, N), dtype=np.int32), np.empty(N, dtype=np.int32)
        ws = np.empty((S, R * N)) if weights else None
        info = BnmfDecomposeInfo()
        self._range_call("decompose", last_n, end_iter, u, _dp(ref.ravel(order="F")), R, None if kp is None else kp.ctypes.data_as(_IP), int(n_steps),
                         float(min_share), _dp(weight), _dp(fit), nact.ctypes.data_as(_IP), inc.ctypes.data_as(_IP), _dp(ws), C.byref(info))
        out = self._info(info)
        out.update(weight=np.stack([row.reshape((R, N), order="F") for row in weight]), fit=fit, nactive=nact, included=inc)
        out.update({name: out["weight"][i] for i, name in enumerate(DEC_WEIGHT_ROWS)})
        out.update({name: fit[i] for i, name in enumerate(PROJ_FIT_ROWS)})
        if weights:
            out["weights"] = np.stack([row.reshape((R, N), order="F") for row in ws]) if S else np.empty((0, R, N))
        return out

    def contrast(self, last_n, groups, used=None, end_iter=None, min_load=1.0, credible_interval=0.95, series=False):
        """Group contrasts of exposures over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last
        `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_contrast / bnmf_contrast_at), on the device.
        groups (length G): the label 0 .. C-1 of every tumour, -1 = left out.  Per used sample, group and factor the group's mean
        renormalised exposure (load), mean share of the tumour's total and prevalence (the fraction of its tumours with a load >=
        min_load) are one draw each from the posterior of that group statistic.  Returns the info fields (n_credible a list per
        statistic), sizes (C), group (3 x 4 x N x C: per statistic of CON_STATS the rows CON_GROUP_ROWS) and pair (3 x 6 x N x NP: the
        rows CON_PAIR_ROWS of the difference a - b of the pairs a < b, a ascending, then b; p_greater / p_less the fraction of samples
        with a positive / negative difference), pairs (the NP pairs (a, b)); with series also series (3 x S x N x C), every used
        sample's values.  credible_interval None or <= 0: no interval, lower / upper are NaN."""
        N, G = self.N, self.G
        gl = np.ascontiguousarray(groups, dtype=np.int32)
        if gl.ndim != 1 or gl.size != G:
            raise BnmfError(-2, f"contrast: groups has shape {gl.shape}, G = {G} labels are needed")
        u, S = self._used("contrast", used, last_n)
        Cn = min(max(int(gl.max(initial=-1)) + 1, 1), CON_MAX_GROUPS)      # (a label the library refuses sizes nothing)
        NP = Cn * (Cn - 1) // 2
        grp, pr = np.empty((3, 4, N * Cn)), np.empty((3, 6, N * NP))
        ser = np.empty((3, S, N * Cn)) if series else None
        sizes = np.empty(Cn, dtype=np.int32)
        ci = 0.0 if credible_interval is None else float(credible_interval)
        info = BnmfContrastInfo()
        self._range_call("contrast", last_n, end_iter, u, gl.ctypes.data_as(_IP), float(min_load), ci, _dp(grp), _dp(pr), _dp(ser),
                         sizes.ctypes.data_as(_IP), C.byref(info))
        out = self._info(info)
        out["n_credible"] = [int(v) for v in info.n_credible]
        out.update(sizes=sizes, group=grp.reshape((3, 4, Cn, N)).transpose(0, 1, 3, 2), pair=pr.reshape((3, 6, NP, N)).transpose(0, 1, 3, 2),
                   pairs=[(a, b) for a in range(Cn) for b in range(a + 1, Cn)])
        if series:
            out["series"] = ser.reshape((3, S, Cn, N)).transpose(0, 1, 3, 2)
        return out

    def regress(self, last_n, design, include=None, used=None, end_iter=None, credible_interval=0.95, series=False):
        """Regression of exposures on tumour covariates over the recorded samples flagged in used (length last_n, oldest first; None =
        all) of the last `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_regress / bnmf_regress_at), on
        the device.  design (G x Q, Q <= REG_MAX_Q) is taken as given: the caller supplies the column of ones.  include (length G of
        0 / 1, None = all): the tumours that enter the fit.  Per used sample, response (REG_STATS: the load, its share of the tumour's
        total, its square root) and factor the least-squares coefficients are one draw from the posterior of the cohort's own
        coefficient (the tumours' sampling error is not added).  Returns the info fields (n_credible 3 x Q: the factors whose interval
        for a column excludes 0), coef (3 x 6 x N x Q: the rows REG_COEF_ROWS) and fit (3 x 5 x N: the rows REG_FIT_ROWS); with series
        also coef_series (3 x S x N x Q) and r2_series (3 x S x N).  credible_interval None or <= 0: no interval, lower / upper are NaN."""
        N, G = self.N, self.G
        D = np.asfortranarray(design, dtype=np.float64)
        if D.ndim != 2 or D.shape[0] != G:
            raise BnmfError(-2, f"regress: design has shape {D.shape}, G = {G} rows are needed")
        Q = D.shape[1]
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"regress: include has shape {inc.shape}, G = {G} flags are needed")
        u, S = self._used("regress", used, last_n)
        coef, fit = np.empty((3, 6, N * Q)), np.empty((3, 5, N))
        cser = np.empty((3, S, N * Q)) if series else None
        rser = np.empty((3, S, N)) if series else None
        ci = 0.0 if credible_interval is None else float(credible_interval)
        info = BnmfRegressInfo()
        self._range_call("regress", last_n, end_iter, u, _dp(D.ravel(order="F")), Q, None if inc is None else inc.ctypes.data_as(_IP), ci, _dp(coef),
                         _dp(fit), _dp(cser), _dp(rser), C.byref(info))
        out = self._info(info)
        out["n_credible"] = np.array([[int(v) for v in row][:max(Q, 0)] for row in info.n_credible], dtype=np.int64)
        out.update(coef=coef.reshape((3, 6, Q, N)).transpose(0, 1, 3, 2), fit=fit)
        if series:
            out.update(coef_series=cser.reshape((3, S, Q, N)).transpose(0, 1, 3, 2), r2_series=rser)
        return out

    def coactivity(self, last_n, include=None, used=None, end_iter=None, min_load=1.0, credible_interval=0.95, series=False):
        """Co-activity of the signatures over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last
        `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_coactivity / bnmf_coactivity_at), on the device.
        include (length G of 0 / 1, None = all): the tumours that enter.  Per used sample and pair of factors a < b the Pearson and the
        Spearman (midrank) correlation of their loads across the included tumours, the phi coefficient of their presence (load >=
        min_load) and the cosine of their two columns of P are one draw each from the posterior of that statistic.  Returns the info
        fields (n_credible a list for the first three statistics), pairs (the NP pairs (a, b), a ascending, then b) and pair (4 x 7 x
        NP: per statistic of COA_STATS the rows COA_PAIR_ROWS over the samples whose value is not NaN); with series also series (4 x S
        x NP), every used sample's values.  credible_interval None or <= 0: no interval, lower / upper are NaN."""
        N, G = self.N, self.G
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"coactivity: include has shape {inc.shape}, G = {G} flags are needed")
        u, S = self._used("coactivity", used, last_n)
        NP = N * (N - 1) // 2
        pr = np.empty((4, 7, NP))
        ser = np.empty((4, S, NP)) if series else None
        ci = 0.0 if credible_interval is None else float(credible_interval)
        info = BnmfCoactivityInfo()
        self._range_call("coactivity", last_n, end_iter, u, None if inc is None else inc.ctypes.data_as(_IP), float(min_load), ci, _dp(pr), _dp(ser),
                         C.byref(info))
        out = self._info(info)
        out["n_credible"] = [int(v) for v in info.n_credible]
        out.update(pair=pr, pairs=[(a, b) for a in range(N) for b in range(a + 1, N)])
        if series:
            out["series"] = ser
        return out

    def coactivity_at(self, end_iter, n_samples, **kw):
        """coactivity over the n_samples iterations that end at end_iter (bnmf_coactivity_at)."""
        return self.coactivity(n_samples, end_iter=end_iter, **kw)

    def stability(self, last_n, labels=None, used=None, end_iter=None, extra_P=None, extra_label=None):
        """Silhouette stability of the recorded signatures over the samples flagged in used (length last_n, oldest first; None = all) of
        the last `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_stability / bnmf_stability_at), on the
        device: every recorded column of P is a point, its cluster is labels[row of the sample][n] (last_n x N over the whole range, -1
        = left out; None = the factor), the distance is the cosine distance, and extra_P (K x X) with extra_label (X values in 0 .. N-1)
        adds further columns (other chains, a catalogue).  Returns the info fields, point (4 x (S N + X): STAB_POINT_ROWS; NaN, NaN, NaN,
        -1 at a left-out position), factor (6 x N: STAB_FACTOR_ROWS), between (N x N mean distances between clusters), medoid (K x N:
        the consensus signatures, columns summing to 1) and medoid_at (N point indices, -1 = empty cluster)."""
        K, N = self.K, self.N
        u, S = self._used("stability", used, last_n)
        lb = None
        if labels is not None:
            lb = np.ascontiguousarray(labels, dtype=np.int32)
            if lb.shape != (last_n, N):
                raise BnmfError(-2, f"stability: labels is {lb.shape}, not {(last_n, N)}")
        X, ex, el = 0, None, None
        if extra_P is not None:
            ex = np.asarray(extra_P, dtype=np.float64)
            if ex.ndim != 2 or ex.shape[0] != K:
                raise BnmfError(-2, f"stability: extra_P is {ex.shape}, K = {K} rows are needed")
            X = ex.shape[1]
            el = np.ascontiguousarray(extra_label if extra_label is not None else [], dtype=np.int32)
            if el.shape != (X,):
                raise BnmfError(-2, f"stability: extra_label has shape {el.shape} for {X} extra columns")
            ex = np.ascontiguousarray(ex.ravel(order="F"))
        NPT = S * N + X
        point, factor, between, medoid = np.empty((4, NPT)), np.empty((6, N)), np.empty((N, N)), np.empty(K * N)
        mat = np.empty(N, dtype=np.int64)
        info = BnmfStabilityInfo()
        self._range_call("stability", last_n, end_iter, u, None if lb is None else lb.ctypes.data_as(_IP), _dp(ex) if X else None,
                         el.ctypes.data_as(_IP) if X else None, X, _dp(point), _dp(factor), _dp(between), _dp(medoid),
                         mat.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(info))
        out = self._info(info)
        out.update(point=point, factor=factor, between=between, medoid=medoid.reshape((K, N), order="F"), medoid_at=mat)
        return out

    def stability_at(self, end_iter, n_samples, **kw):
        """stability over the n_samples iterations that end at end_iter (bnmf_stability_at)."""
        return self.stability(n_samples, end_iter=end_iter, **kw)

    def reconstruction(self, last_n, used=None, end_iter=None, min_cosine=0.9, min_drop=0.01, drop=True):
        """Reconstruction quality per tumour over the recorded samples flagged in used (length last_n, oldest first; None = all) of the
        last `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_reconstruction / bnmf_reconstruction_at), on
        the device.  Returns the info fields, tumour (6 x G) with its rows also by name (REC_TUMOUR_ROWS: the mean, variance and smallest
        value over the used samples of the cosine between the tumour's data and its fit, the mean relative L1 error and RMSE, the
        fraction of samples whose cosine is >= min_cosine; NaN for an all-zero tumour), series (S: the cohort's mean cosine per used
        sample) and signature (3 x N, REC_SIGNATURE_ROWS: the tumours that need the signature, the mean and the largest mean drop); with
        drop also drop (4 x N x G) and its rows by name (REC_DROP_ROWS: the mean and variance of the loss of cosine when factor n is
        left out of the fit without a refit, the mean leave-one-out cosine, the fraction of samples whose drop is >= min_drop)."""
        G, N = self.G, self.N
        u, S = self._used("reconstruction", used, last_n)
        tum, series, sig = np.empty((6, G)), np.empty(S), np.empty((3, N))
        dr = np.empty((4, N * G)) if drop else None
        info = BnmfReconstructionInfo()
        self._range_call("reconstruction", last_n, end_iter, u, float(min_cosine), float(min_drop), _dp(tum), _dp(dr), _dp(series), _dp(sig), C.byref(info))
        out = self._info(info)
        out.update(tumour=tum, series=series, signature=sig)
        out.update({name: tum[i] for i, name in enumerate(REC_TUMOUR_ROWS)})
        if drop:
            out["drop"] = np.stack([row.reshape((N, G), order="F") for row in dr])
            out.update({name: out["drop"][i] for i, name in enumerate(REC_DROP_ROWS)})
        return out

    def reconstruction_at(self, end_iter, n_samples, **kw):
        """reconstruction over the n_samples iterations that end at end_iter (bnmf_reconstruction_at)."""
        return self.reconstruction(n_samples, end_iter=end_iter, **kw)

    def similarity(self, last_n, include=None, query=None, top_k=10, min_cosine=0.9, used=None, end_iter=None, tumour=True):
        """Similarity of the tumours over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last
        `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_similarity / bnmf_similarity_at), on the device.
        include (length G of 0 / 1, None = all): the tumours that enter.  Per used sample the cosine of two tumours' renormalised
        exposure vectors is one draw from its posterior; it is a sum over the factors, so label switching does not touch it.  Returns the
        info fields; with top_k > 0 neighbour_at (G x top_k: the other members with the largest mean cosine, the lower tumour first
        among equals, -1 = none) and neighbour (3 x G x top_k, the rows SIM_ROWS); with query (Q tumours) dense (3 x Q x G: the rows
        SIM_ROWS of query[q] against every tumour, NaN on itself and on the left-out tumours); with tumour the 3 x G table and its rows by
        name (SIM_TUMOUR_ROWS: the mean over the other members of the mean cosine, the mean cosine of the first neighbour, the number of
        other members whose cosine is >= min_cosine in at least half of the samples).  top_k = 0, tumour = False and a query: only the Q
        rows are computed."""
        G = self.G
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"similarity: include has shape {inc.shape}, G = {G} flags are needed")
        qv = None if query is None else np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
        Q = 0 if qv is None else int(qv.size)
        k = int(top_k)
        u, _ = self._used("similarity", used, last_n)
        kk = min(max(k, 0), SIM_MAX_K)                         # (an invalid top_k is refused by the library: the buffers only have to exist)
        nat = np.empty((G, kk), dtype=np.int32) if kk > 0 else None
        nb = np.empty((3, G, kk)) if kk > 0 else None
        dn = np.empty((3, Q, G)) if Q > 0 else None
        tum = np.empty((3, G)) if tumour else None
        info = BnmfSimilarityInfo()
        self._range_call("similarity", last_n, end_iter, u, None if inc is None else inc.ctypes.data_as(_IP), None if qv is None else qv.ctypes.data_as(_IP),
                         Q, k, float(min_cosine), None if nat is None else nat.ctypes.data_as(_IP), _dp(nb), _dp(dn), _dp(tum), C.byref(info))
        out = self._info(info)
        if nat is not None:
            out.update(neighbour_at=nat, neighbour=nb)
        if dn is not None:
            out.update(dense=dn, query=qv.copy())
        if tumour:
            out["tumour"] = tum
            out.update({name: tum[i] for i, name in enumerate(SIM_TUMOUR_ROWS)})
        return out

    def similarity_at(self, end_iter, n_samples, **kw):
        """similarity over the n_samples iterations that end at end_iter (bnmf_similarity_at)."""
        return self.similarity(n_samples, end_iter=end_iter, **kw)

    def subtypes(self, last_n, centres0, include=None, perm=None, n_steps=50, query=None, min_certainty=0.9, used=None, end_iter=None, labels=False):
        """Subtypes of the tumours over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last
        `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_subtypes / bnmf_subtypes_at), on the device: every
        used sample's share profiles are clustered by at most n_steps Lloyd steps from centres0 (N x C), the same start for every sample.
        include (length G of 0 / 1, None = all): the tumours that enter.  perm (last_n x N over the whole range, relabel's; a row of -1
        leaves the sample out; None = identity) aligns the factors first.  Returns the info fields, membership (C x G), label (G, -1 =
        none), tumour (3 x G) and its rows by name (SUB_TUMOUR_ROWS), centre (4 x N x C) and size (4 x C) (the rows SUB_ROWS over the
        matched samples, interval 0.95), series (3 x S: SUB_SERIES_ROWS, NaN for an unmatched sample); with query (Q tumours) together
        (Q x G: the share of samples in which query[q] and g carry the same label); with labels the S x G labels of every used sample
        (-1 unassigned, -2 left out or unmatched)."""
        G, N = self.G, self.N
        c0 = np.asarray(centres0, dtype=np.float64)
        if c0.ndim != 2 or c0.shape[0] != N:
            raise BnmfError(-2, f"subtypes: centres0 has shape {c0.shape}, N = {N} rows are needed")
        c0 = np.asfortranarray(c0)
        Cn = int(c0.shape[1])
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"subtypes: include has shape {inc.shape}, G = {G} flags are needed")
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        if pm is not None and pm.shape != (last_n, N):
            raise BnmfError(-2, f"subtypes: perm is {pm.shape}, not {(last_n, N)}")
        qv = None if query is None else np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
        Q = 0 if qv is None else int(qv.size)
        u, S = self._used("subtypes", used, last_n)
        Cb = min(max(Cn, 1), 32)                               # (an invalid C is refused by the library: the buffers only have to exist)
        mem, lab, tum = np.empty((Cb, G)), np.empty(G, dtype=np.int32), np.empty((3, G))
        cen, siz, ser = np.empty((4, Cb, N)), np.empty((4, Cb)), np.empty((3, S))
        tog = np.empty((Q, G)) if Q > 0 else None
        lbs = np.empty((S, G), dtype=np.int32) if labels else None
        info = BnmfSubtypesInfo()
        ipt = lambda v: None if v is None else v.ctypes.data_as(_IP)  # noqa: E731
        self._range_call("subtypes", last_n, end_iter, u, ipt(inc), ipt(pm), _dp(c0), Cn, int(n_steps), ipt(qv), Q, float(min_certainty), _dp(mem), ipt(lab),
                         _dp(tum), _dp(cen), _dp(siz), _dp(tog), ipt(lbs), _dp(ser), C.byref(info))
        out = self._info(info)
        out.update(membership=mem, label=lab, tumour=tum, centre=np.ascontiguousarray(cen.transpose(0, 2, 1)), size=siz, series=ser)
        out.update({name: tum[i] for i, name in enumerate(SUB_TUMOUR_ROWS)})
        if tog is not None:
            out.update(together=tog, query=qv.copy())
        if lbs is not None:
            out["labels"] = lbs
        return out

    def subtypes_at(self, end_iter, n_samples, centres0, **kw):
        """subtypes over the n_samples iterations that end at end_iter (bnmf_subtypes_at)."""
        return self.subtypes(n_samples, centres0, end_iter=end_iter, **kw)

    def residuals(self, last_n, include=None, n_steps=100, max_dispersion=2.0, used=None, end_iter=None):
        """Residual structure over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last `last_n`,
        or with end_iter of the `last_n` that end at iteration end_iter (bnmf_residuals / bnmf_residuals_at), on the device: per used
        sample the standardised residuals of every cell, their K x K second-moment matrix over the included tumours (include: length G
        of 0 / 1, None = all), its leading component by n_steps power steps and every tumour's score on it.  Returns the info fields,
        gram (K x K: the mean matrix), type (5 x K: RES_TYPE_ROWS), component (4 x K: RES_COMPONENT_ROWS), tumour (3 x G:
        RES_TUMOUR_ROWS, NaN for a left-out tumour) and series (5 x S: RES_SERIES_ROWS, NaN for a flat sample), and the rows of type,
        component and tumour by name.  max_dispersion only sets the count n_overdispersed: a reporting convention, not a test."""
        G, K = self.G, self.K
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"residuals: include has shape {inc.shape}, G = {G} flags are needed")
        u, S = self._used("residuals", used, last_n)
        gram, typ, comp, tum, ser = np.empty((K, K)), np.empty((5, K)), np.empty((4, K)), np.empty((3, G)), np.empty((5, S))
        info = BnmfResidualsInfo()
        self._range_call("residuals", last_n, end_iter, u, None if inc is None else inc.ctypes.data_as(_IP), int(n_steps), float(max_dispersion), _dp(gram),
                         _dp(typ), _dp(comp), _dp(tum), _dp(ser), C.byref(info))
        out = self._info(info)
        out.update(gram=gram, type=typ, component=comp, tumour=tum, series=ser)
        out.update({name: typ[i] for i, name in enumerate(RES_TYPE_ROWS)})
        out["vbar"] = comp[0]
        out.update({name: tum[i] for i, name in enumerate(RES_TUMOUR_ROWS)})
        return out

    def residuals_at(self, end_iter, n_samples, **kw):
        """residuals over the n_samples iterations that end at end_iter (bnmf_residuals_at)."""
        return self.residuals(n_samples, end_iter=end_iter, **kw)

    def tradeoff(self, last_n, include=None, perm=None, sets=None, query=None, min_corr=0.5, used=None, end_iter=None):
        """Trade-offs between signatures within a tumour over the recorded samples flagged in used (length last_n, oldest first; None =
        all) of the last `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_tradeoff / bnmf_tradeoff_at), on
        the device: per included tumour (include: length G of 0 / 1, None = all) the N x N covariance of its aligned renormalised
        exposures over the samples.  perm (last_n x N over the whole range, relabel's; a row of -1 leaves the sample out; None =
        identity) aligns the factors first.  sets (length N of 0 .. C-1, -1 = in no set; None = no sets).  Returns the info fields,
        tumour (3 x G: TRD_TUMOUR_ROWS, NaN for a left-out tumour; not spread by name, min_corr is the info field), pair_at (G), pair
        (5 x N x N: TRD_PAIR_ROWS, symmetric, the diagonal NaN), setstat (4 x C x G: TRD_SET_ROWS) and with query (Q tumours) dense
        (Q x 2 x N x N: the covariance and the correlation matrix of every query tumour).  min_corr only sets the counts: a reporting
        convention, not a test."""
        G, N = self.G, self.N
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"tradeoff: include has shape {inc.shape}, G = {G} flags are needed")
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        if pm is not None and pm.shape != (last_n, N):
            raise BnmfError(-2, f"tradeoff: perm is {pm.shape}, not {(last_n, N)}")
        st = None if sets is None else np.ascontiguousarray(sets, dtype=np.int32)
        if st is not None and (st.ndim != 1 or st.size != N):
            raise BnmfError(-2, f"tradeoff: sets has shape {st.shape}, N = {N} labels are needed")
        Cn = 0 if st is None else int(st.max()) + 1
        qv = None if query is None else np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
        Q = 0 if qv is None else int(qv.size)
        u, S = self._used("tradeoff", used, last_n)
        Cb = min(max(Cn, 0), TRD_MAX_C)                        # (an invalid C is refused by the library: the buffers only have to exist)
        tum, pat, par, sst = np.empty((3, G)), np.empty(G, dtype=np.int32), np.empty((5, N, N)), np.empty((4, Cb, G))
        den = np.empty((Q, 2, N, N)) if Q > 0 else None
        info = BnmfTradeoffInfo()
        ipt = lambda v: None if v is None else v.ctypes.data_as(_IP)  # noqa: E731
        self._range_call("tradeoff", last_n, end_iter, u, ipt(inc), ipt(pm), ipt(st), Cn, ipt(qv), Q, float(min_corr), _dp(tum), ipt(pat), _dp(par), _dp(den),
                         _dp(sst) if Cb > 0 else None, C.byref(info))
        out = self._info(info)
        out.update(tumour=tum, pair_at=pat, pair=par, setstat=sst)
        if den is not None:
            out.update(dense=den, query=qv.copy())
        return out

    def tradeoff_at(self, end_iter, n_samples, **kw):
        """tradeoff over the n_samples iterations that end at end_iter (bnmf_tradeoff_at)."""
        return self.tradeoff(n_samples, end_iter=end_iter, **kw)

    def prune(self, last_n, include=None, n_steps=20, max_loss=0.01, used=None, end_iter=None, exposures=False):
        """Sparse per-tumour assignment with refit over the recorded samples flagged in used (length last_n, oldest first; None = all) of
        the last `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_prune / bnmf_prune_at), on the device:
        per sample and included tumour (include: length G of 0 / 1, None = all) backward elimination of the sample's signatures from its
        own exposures, with n_steps KL steps of refit after every removal, while the cosine stays within max_loss of the full refit's.
        Returns the info fields, load (4 x N x G) with its rows also by name (PRN_LOAD_ROWS: mean and variance of the sparse exposure,
        mean share, the probability that the tumour keeps the signature), tumour (7 x G, PRN_TUMOUR_ROWS; not spread by name), series
        (2 x S, PRN_SERIES_ROWS), signature (3 x N, PRN_SIGNATURE_ROWS) and with exposures also exposures (S x N x G: every used
        sample's sparse exposures).  NaN for an all-zero or left-out tumour.  n_steps and max_loss are reporting conventions, not
        tests; rel_change tells whether n_steps sufficed."""
        G, N = self.G, self.N
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"prune: include has shape {inc.shape}, G = {G} flags are needed")
        u, S = self._used("prune", used, last_n)
        ld, tum, series, sig = np.empty((4, N * G)), np.empty((7, G)), np.empty((2, S)), np.empty((3, N))
        ex = np.empty((S, N * G)) if exposures else None
        info = BnmfPruneInfo()
        self._range_call("prune", last_n, end_iter, u, None if inc is None else inc.ctypes.data_as(_IP), int(n_steps), float(max_loss), _dp(ld), _dp(tum),
                         _dp(series), _dp(sig), _dp(ex), C.byref(info))
        out = self._info(info)
        out.update(load=np.stack([row.reshape((N, G), order="F") for row in ld]), tumour=tum, series=series, signature=sig)
        out.update({name: out["load"][i] for i, name in enumerate(PRN_LOAD_ROWS)})
        if exposures:
            out["exposures"] = np.stack([row.reshape((N, G), order="F") for row in ex]) if S else np.empty((0, N, G))
        return out

    def prune_at(self, end_iter, n_samples, **kw):
        """prune over the n_samples iterations that end at end_iter (bnmf_prune_at)."""
        return self.prune(n_samples, end_iter=end_iter, **kw)

    def summary(self, last_n, probs=(0.05, 0.25, 0.5, 0.75, 0.95), include=None, perm=None, min_load=1.0, credible_interval=0.95, used=None,
                end_iter=None, series=False):
        """Cohort summary of the signatures over the recorded samples flagged in used (length last_n, oldest first; None = all) of the
        last `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_summary / bnmf_summary_at), on the device:
        per used sample and factor the prevalence (the share of the included tumours with a load >= min_load), the total load, its
        fraction of the cohort's, the mean load of the carriers, and at every level of probs (1 .. SUM_MAX_Q values in [0, 1],
        ascending) the exact type-7 quantile of all loads, of the carriers' loads and of the shares.  include (length G of 0 / 1,
        None = all): the tumours that enter.  perm (last_n x N over the whole range, relabel's; a row of -1 leaves the sample out; None
        = identity): a value goes to the place of its label.  Returns the info fields, names (the 4 + 3 L statistics: SUM_SCALARS, then
        per family of SUM_FAMILIES and level "family_level"), probs and stat (NSTAT x 5 x N: the rows SUM_ROWS over the samples whose
        value is not NaN); with series also series (NSTAT x S x N).  credible_interval None or <= 0: no interval."""
        N, G = self.N, self.G
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        L = int(pr.size)
        inc = None if include is None else np.ascontiguousarray(include, dtype=np.int32)
        if inc is not None and (inc.ndim != 1 or inc.size != G):
            raise BnmfError(-2, f"summary: include has shape {inc.shape}, G = {G} flags are needed")
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.int32)
        if pm is not None and pm.shape != (last_n, N):
            raise BnmfError(-2, f"summary: perm is {pm.shape}, not {(last_n, N)}")
        u, S = self._used("summary", used, last_n)
        Lb = min(max(L, 1), SUM_MAX_Q)                         # (an invalid L is refused by the library: the buffers only have to exist)
        nstat = 4 + 3 * Lb
        st = np.empty((nstat, 5, N))
        ser = np.empty((nstat, S, N)) if series else None
        ci = 0.0 if credible_interval is None else float(credible_interval)
        info = BnmfSummaryInfo()
        ipt = lambda v: None if v is None else v.ctypes.data_as(_IP)  # noqa: E731
        self._range_call("summary", last_n, end_iter, u, ipt(inc), ipt(pm), float(min_load), _dp(pr), L, ci, _dp(st), _dp(ser), C.byref(info))
        out = self._info(info)
        out.update(stat=st, probs=pr.copy(), names=list(SUM_SCALARS) + [f"{fam}_{p:g}" for fam in SUM_FAMILIES for p in pr])
        if series:
            out["series"] = ser
        return out

    def summary_at(self, end_iter, n_samples, **kw):
        """summary over the n_samples iterations that end at end_iter (bnmf_summary_at)."""
        return self.summary(n_samples, end_iter=end_iter, **kw)

    def mixing(self, last_n, used=None, end_iter=None, keep=None, arrays=True):
        """Mixing diagnostics over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last `last_n`,
        or with end_iter of the `last_n` that end at iteration end_iter (bnmf_mixing / bnmf_mixing_at), on the device.  A lag counts used
        samples: a used with gaps is treated as one contiguous series.  keep (length N, None = all): the factors that enter the summary.
        Returns the info fields; with arrays also, for every name in MIX_ROWS, name_P (K x N) and name_E (N x G)."""
        K, G, N = self.K, self.G, self.N
        u, _ = self._used("mixing", used, last_n)
        kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.int32)
        if kp is not None and kp.size != N:
            raise BnmfError(-2, f"mixing: keep has {kp.size} entries for {N} factors")
        oP = np.empty((NMIX, K * N)) if arrays else None
        oE = np.empty((NMIX, N * G)) if arrays else None
        info = BnmfMixingInfo()
        self._range_call("mixing", last_n, end_iter, u, None if kp is None else kp.ctypes.data_as(_IP), _dp(oP), _dp(oE), C.byref(info))
        out = self._info(info)
        if arrays:
            for i, name in enumerate(MIX_ROWS):
                out[name + "_P"] = oP[i].reshape((K, N), order="F")
                out[name + "_E"] = oE[i].reshape((N, G), order="F")
        return out

    def relabel(self, last_n, used=None, end_iter=None, pivot_P=None, max_rounds=10, aligned=False):
        """Label-switching correction over the recorded samples flagged in used (length last_n, oldest first; None = all) of the last
        `last_n`, or with end_iter of the `last_n` that end at iteration end_iter (bnmf_relabel / bnmf_relabel_at), on the device: every
        sample's factors are permuted to the labels of a pivot (pivot_P, K x N; None = the newest used sample's P) so that the total
        cosine is largest, and the pivot is iterated to the aligned mean for at most max_rounds rounds.  Returns the info fields, perm
        (S x N int32: the label factor n of sample s receives; -1 = the sample is unmatched), cosine (S x N), confusion (N x N int64),
        P_mean, P_var (K x N) and E_mean, E_var (N x G) of the aligned, renormalised samples; with aligned also aligned_P (S x K x N)
        and aligned_E (S x N x G), the aligned samples themselves (NaN for an unmatched one)."""
        K, G, N = self.K, self.G, self.N
        u, S = self._used("relabel", used, last_n)
        pv = None
        if pivot_P is not None:
            pv = np.asarray(pivot_P, dtype=np.float64)
            if pv.shape != (K, N):
                raise BnmfError(-2, f"relabel: pivot_P is {pv.shape}, not {(K, N)}")
            pv = np.ascontiguousarray(pv.ravel(order="F"))
        perm, cos, conf = np.empty((S, N), dtype=np.int32), np.empty((S, N)), np.empty((N, N), dtype=np.int64)
        oP, oE = np.empty((2, K * N)), np.empty((2, N * G))
        aP = np.empty((S, K * N)) if aligned else None
        aE = np.empty((S, N * G)) if aligned else None
        info = BnmfRelabelInfo()
        self._range_call("relabel", last_n, end_iter, u, _dp(pv), int(max_rounds), perm.ctypes.data_as(_IP), _dp(cos),
                         conf.ctypes.data_as(C.POINTER(C.c_int64)), _dp(oP), _dp(oE), _dp(aP), _dp(aE), C.byref(info))
        out = self._info(info)
        out.update(perm=perm, cosine=cos, confusion=conf, P_mean=oP[0].reshape((K, N), order="F"), P_var=oP[1].reshape((K, N), order="F"),
                   E_mean=oE[0].reshape((N, G), order="F"), E_var=oE[1].reshape((N, G), order="F"))
        if aligned:
            out.update(aligned_P=aP.reshape((S, N, K)).transpose(0, 2, 1), aligned_E=aE.reshape((S, G, N)).transpose(0, 2, 1))
        return out

    def label_switching(self, iters, reference_P):
        """plot_label_switching's per-sample hungarian_assignment diagonal over the recorded iterations `iters`, on the device
        (bnmf_label_switching): assigned (0-based reference column, -1 = no partner), cosine and included (A_t != 0), each
        (len(iters), N)."""
        N = self.N
        it = np.ascontiguousarray(np.atleast_1d(iters), dtype=np.int32)
        ref = np.asfortranarray(reference_P, dtype=np.float64)
        R = ref.shape[1]
        ip = C.POINTER(C.c_int32)
        asg, cos, inc = np.empty((it.size, N), dtype=np.int32), np.empty((it.size, N)), np.empty((it.size, N), dtype=np.int32)
        _chk(lib().bnmf_label_switching(self._h, it.ctypes.data_as(ip), it.size, _dp(ref.ravel(order="F")), R, asg.ctypes.data_as(ip),
                                        _dp(cos), inc.ctypes.data_as(ip)))
        return dict(assigned=asg, cosine=cos, included=inc.astype(bool))

    def save_state(self, path, since_iter=0):
        """Write the chain's state to `path` (bnmf_save_state): since_iter = 0 a full record (file created or truncated), S > 0 a delta
        appended to a file whose last record is this chain at iteration S.  Returns the bytes written."""
        b = C.c_size_t(0)
        _chk(lib().bnmf_save_state(self._h, os.fsencode(path), int(since_iter), C.byref(b)))
        return b.value

    def load_state(self, path):
        """Replay the records of `path` into this engine, instead of init() (bnmf_load_state).  Returns the iteration it is then at."""
        it = C.c_int(0)
        _chk(lib().bnmf_load_state(self._h, os.fsencode(path), C.byref(it)))
        return it.value

    def stat(self, what):
        """Sizes of the handle's per-iteration buffers (bnmf_get_stat)."""
        v = C.c_double()
        _chk(lib().bnmf_get_stat(self._h, int(what), C.byref(v)))
        return v.value

    @property
    def iter(self):
        it = C.c_int()
        _chk(lib().bnmf_get_iter(self._h, C.byref(it)))
        return it.value
