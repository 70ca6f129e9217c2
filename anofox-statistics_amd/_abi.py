"""ctypes binding of libanofox_stats_hip.so (include/anofox_stats_hip.h).

The library is the product; this module only declares its C ABI.  There is no
fallback: if the shared object is missing or a symbol is absent, import fails.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ANOFOX_STATS_HIP_LIB selects another build of the same ABI (used for the diagnostic build with stamps)
LIB_PATH = os.environ.get("ANOFOX_STATS_HIP_LIB") or os.path.join(_HERE, "libanofox_stats_hip.so")

# --- enums (anofox_stats_hip.h) ------------------------------------------------
ERROR_SUCCESS = 0
ERROR_INVALID_INPUT = 1
ERROR_SINGULAR_MATRIX = 2
ERROR_CONVERGENCE_FAILURE = 3
ERROR_INVALID_ALPHA = 4
ERROR_INVALID_L1_RATIO = 5
ERROR_INSUFFICIENT_DATA = 6
ERROR_ALLOCATION_FAILURE = 7
ERROR_SERIALIZATION_ERROR = 8
ERROR_DIMENSION_MISMATCH = 9
ERROR_NO_VALID_DATA = 10
ERROR_INTERNAL = 99
STATUS_NULL_TOO_FEW_ROWS = 100
STATUS_UNREFINED = 101   # a streaming state could neither resolve nor refit the group: NaN record, SQL NULL

SOLVER = {"qr": 0, "svd": 1, "cholesky": 2}
LAMBDA_SCALING = {"raw": 0, "glmnet": 1}
HC_TYPE = {"none": 0, "hc0": 1, "hc1": 2, "hc2": 3, "hc3": 4}
MODEL = {"ols": 0, "ridge": 1, "wls": 2}

_DP = C.POINTER(C.c_double)


class AnofoxError(C.Structure):
    _fields_ = [("code", C.c_int), ("message", C.c_char * 256)]

    def text(self) -> str:
        return self.message.decode("utf-8", "replace")


class AnofoxDataArray(C.Structure):
    _fields_ = [("data", _DP), ("validity", C.POINTER(C.c_uint8)), ("len", C.c_size_t)]


class AnofoxFitResultCore(C.Structure):
    _fields_ = [("coefficients", _DP), ("coefficients_len", C.c_size_t), ("intercept", C.c_double),
                ("r_squared", C.c_double), ("adj_r_squared", C.c_double), ("residual_std_error", C.c_double),
                ("n_observations", C.c_size_t), ("n_features", C.c_size_t)]


class AnofoxFitResultInference(C.Structure):
    _fields_ = [("std_errors", _DP), ("t_values", _DP), ("p_values", _DP), ("ci_lower", _DP), ("ci_upper", _DP),
                ("len", C.c_size_t), ("confidence_level", C.c_double), ("f_statistic", C.c_double),
                ("f_pvalue", C.c_double)]


class AnofoxOlsOptions(C.Structure):
    _fields_ = [("fit_intercept", C.c_bool), ("compute_inference", C.c_bool), ("confidence_level", C.c_double),
                ("solver", C.c_int), ("hc_type", C.c_int)]


class AnofoxRidgeOptions(C.Structure):
    _fields_ = [("alpha", C.c_double), ("fit_intercept", C.c_bool), ("compute_inference", C.c_bool),
                ("confidence_level", C.c_double), ("solver", C.c_int), ("lambda_scaling", C.c_int)]


class AnofoxWlsOptions(C.Structure):
    _fields_ = AnofoxOlsOptions._fields_


class AnofoxHipBatchOptions(C.Structure):
    _fields_ = [("model", C.c_int), ("fit_intercept", C.c_bool), ("compute_inference", C.c_bool),
                ("confidence_level", C.c_double), ("alpha", C.c_double), ("solver", C.c_int),
                ("lambda_scaling", C.c_int), ("hc_type", C.c_int)]


class AnofoxHipKernelTimes(C.Structure):
    _fields_ = [("accumulate_ms", C.c_double), ("accumulate_count", C.c_int64), ("solve_ms", C.c_double),
                ("solve_count", C.c_int64), ("predict_ms", C.c_double), ("predict_count", C.c_int64),
                ("accumulate_ms_min", C.c_double), ("accumulate_ms_max", C.c_double)]


class AnofoxHipWindowFrame(C.Structure):
    """ROWS BETWEEN start_preceding PRECEDING AND end_preceding PRECEDING; start_preceding < 0 = UNBOUNDED."""
    _fields_ = [("start_preceding", C.c_int64), ("end_preceding", C.c_int64)]


class AnofoxPredictionResult(C.Structure):
    _fields_ = [("yhat", C.c_double), ("yhat_lower", C.c_double), ("yhat_upper", C.c_double)]


RESIDUALS_HAS_STANDARDIZED, RESIDUALS_HAS_STUDENTIZED, RESIDUALS_HAS_LEVERAGE = 1, 2, 4


class AnofoxResidualsResult(C.Structure):  # anofox_stats_ffi.h:527-536
    _fields_ = [("raw", C.POINTER(C.c_double)), ("standardized", C.POINTER(C.c_double)),
                ("studentized", C.POINTER(C.c_double)), ("leverage", C.POINTER(C.c_double)), ("len", C.c_size_t),
                ("has_standardized", C.c_bool), ("has_studentized", C.c_bool), ("has_leverage", C.c_bool)]


class AnofoxElasticNetOptions(C.Structure):  # anofox_stats_ffi.h:384-397, 40 bytes
    _fields_ = [("alpha", C.c_double), ("l1_ratio", C.c_double), ("fit_intercept", C.c_bool),
                ("max_iterations", C.c_uint32), ("tolerance", C.c_double), ("lambda_scaling", C.c_int)]


class AnofoxHipElasticNetBatchOptions(C.Structure):
    _fields_ = [("fit_intercept", C.c_bool), ("alpha", C.c_double), ("l1_ratio", C.c_double),
                ("max_iterations", C.c_uint32), ("tolerance", C.c_double), ("lambda_scaling", C.c_int)]


class AnofoxRlsOptions(C.Structure):  # anofox_stats_ffi.h:593-600, 24 bytes
    _fields_ = [("forgetting_factor", C.c_double), ("fit_intercept", C.c_bool), ("initial_p_diagonal", C.c_double)]


class AnofoxHipRlsBatchOptions(C.Structure):
    _fields_ = [("fit_intercept", C.c_bool), ("forgetting_factor", C.c_double), ("initial_p_diagonal", C.c_double)]


class AnofoxBlsOptions(C.Structure):  # anofox_stats_ffi.h:1186-1201, 56 bytes
    _fields_ = [("fit_intercept", C.c_bool), ("lower_bounds", _DP), ("lower_bounds_len", C.c_size_t),
                ("upper_bounds", _DP), ("upper_bounds_len", C.c_size_t), ("max_iterations", C.c_uint32),
                ("tolerance", C.c_double)]


class AnofoxBlsFitResultCore(C.Structure):  # anofox_stats_ffi.h:1206-1227, 80 bytes
    _fields_ = [("coefficients", _DP), ("coefficients_len", C.c_size_t), ("intercept", C.c_double), ("ssr", C.c_double),
                ("r_squared", C.c_double), ("n_observations", C.c_size_t), ("n_features", C.c_size_t),
                ("n_active_constraints", C.c_size_t), ("at_lower_bound", C.POINTER(C.c_bool)),
                ("at_upper_bound", C.POINTER(C.c_bool))]


class AnofoxHipBlsBatchOptions(C.Structure):
    _fields_ = AnofoxBlsOptions._fields_


class AnofoxQuantileOptions(C.Structure):  # anofox_stats_ffi.h:1371-1380, 24 bytes
    _fields_ = [("tau", C.c_double), ("fit_intercept", C.c_bool), ("max_iterations", C.c_uint32), ("tolerance", C.c_double)]


class AnofoxQuantileFitResultCore(C.Structure):  # anofox_stats_ffi.h:1385-1398, 48 bytes
    _fields_ = [("coefficients", _DP), ("coefficients_len", C.c_size_t), ("intercept", C.c_double), ("tau", C.c_double),
                ("n_observations", C.c_size_t), ("n_features", C.c_size_t)]


class AnofoxHipQuantileBatchOptions(C.Structure):
    _fields_ = AnofoxQuantileOptions._fields_


class AnofoxGlmFitResultCore(C.Structure):  # anofox_stats_ffi.h:715-741, 88 bytes
    _fields_ = [("coefficients", _DP), ("coefficients_len", C.c_size_t), ("intercept", C.c_double), ("deviance", C.c_double),
                ("null_deviance", C.c_double), ("pseudo_r_squared", C.c_double), ("aic", C.c_double), ("dispersion", C.c_double),
                ("n_observations", C.c_size_t), ("n_features", C.c_size_t), ("iterations", C.c_uint32), ("converged", C.c_bool)]


class AnofoxPriorSpec(C.Structure):  # anofox_stats_ffi.h:775-779, 24 bytes
    _fields_ = [("kind", C.c_int), ("loc", C.c_double), ("scale", C.c_double)]


class AnofoxPoissonOptions(C.Structure):  # anofox_stats_ffi.h:796-819, 80 bytes
    _fields_ = [("fit_intercept", C.c_bool), ("link", C.c_int), ("max_iterations", C.c_uint32), ("tolerance", C.c_double),
                ("compute_inference", C.c_bool), ("confidence_level", C.c_double), ("lambda_", C.c_double),
                ("priors", C.POINTER(AnofoxPriorSpec)), ("priors_len", C.c_size_t), ("vcov", C.c_int), ("offset_column", C.c_size_t)]


class AnofoxBinomialOptions(C.Structure):  # anofox_stats_ffi.h:824-847, 80 bytes
    _fields_ = AnofoxPoissonOptions._fields_


class AnofoxLogisticOptions(C.Structure):  # anofox_stats_ffi.h:1008-1026, 80 bytes
    _fields_ = [("fit_intercept", C.c_bool), ("compute_inference", C.c_bool), ("confidence_level", C.c_double),
                ("lambda_", C.c_double), ("threshold", C.c_double), ("max_iterations", C.c_uint32), ("tolerance", C.c_double),
                ("priors", C.POINTER(AnofoxPriorSpec)), ("priors_len", C.c_size_t), ("vcov", C.c_int), ("offset_column", C.c_size_t)]


class AnofoxLogisticFitExtras(C.Structure):  # anofox_stats_ffi.h:1032-1037
    _fields_ = [("accuracy", C.c_double), ("threshold", C.c_double)]


GLM_FAMILY = {"poisson": 0, "binomial": 1, "logistic": 1}


class AnofoxHipGlmBatchOptions(C.Structure):
    _fields_ = [("family", C.c_int32), ("fit_intercept", C.c_bool), ("max_iterations", C.c_uint32), ("tolerance", C.c_double),
                ("lambda_", C.c_double), ("compute_inference", C.c_bool), ("confidence_level", C.c_double)]


AFT_WEIBULL, AFT_LOGNORMAL, AFT_LOGLOGISTIC, AFT_EXPONENTIAL = 0, 1, 2, 3


class AnofoxAftOptions(C.Structure):  # anofox_stats_ffi.h:2304-2315, 64 bytes
    _fields_ = [("dist", C.c_int), ("fit_intercept", C.c_bool), ("max_iterations", C.c_uint32), ("tolerance", C.c_double),
                ("compute_inference", C.c_bool), ("confidence_level", C.c_double), ("priors", C.POINTER(AnofoxPriorSpec)),
                ("priors_len", C.c_size_t), ("vcov", C.c_int)]


class AnofoxAftFitResultCore(C.Structure):  # anofox_stats_ffi.h:2320-2337, 104 bytes
    _fields_ = [("coefficients", _DP), ("coefficients_len", C.c_size_t), ("intercept", C.c_double), ("scale", C.c_double),
                ("log_likelihood", C.c_double), ("null_log_likelihood", C.c_double), ("aic", C.c_double), ("bic", C.c_double),
                ("n_observations", C.c_size_t), ("n_events", C.c_size_t), ("n_censored", C.c_size_t), ("n_features", C.c_size_t),
                ("iterations", C.c_uint32), ("converged", C.c_bool)]


class AnofoxAftInference(C.Structure):  # anofox_stats_ffi.h:2342-2354, 72 bytes
    _fields_ = [("std_errors", _DP), ("z_values", _DP), ("p_values", _DP), ("ci_lower", _DP), ("ci_upper", _DP),
                ("len", C.c_size_t), ("confidence_level", C.c_double), ("intercept_std_error", C.c_double),
                ("log_scale_std_error", C.c_double)]


class AnofoxHipAftBatchOptions(C.Structure):
    _fields_ = [("dist", C.c_int), ("fit_intercept", C.c_int), ("max_iterations", C.c_uint32), ("tolerance", C.c_double),
                ("compute_inference", C.c_int), ("confidence_level", C.c_double)]


class AnofoxHipAftPredictOptions(C.Structure):  # horizon NaN: risk is not asked for
    _fields_ = [("quantile", C.c_double), ("horizon", C.c_double)]


TAU_DERSIMONIAN_LAIRD, TAU_NONE = 0, 1


class AnofoxEbShrinkOptions(C.Structure):  # anofox_stats_ffi.h:2396-2400, 16 bytes; tau_squared NaN: estimate it
    _fields_ = [("method", C.c_int), ("tau_squared", C.c_double)]


class AnofoxHipEbShrinkOptions(C.Structure):  # the batch entries' options: the same layout
    _fields_ = [("method", C.c_int), ("tau_squared", C.c_double)]


class AnofoxCorrelationOptions(C.Structure):  # anofox_stats_ffi.h:1709-1714, 16 bytes; confidence_level NaN: no interval
    _fields_ = [("alternative", C.c_int), ("confidence_level", C.c_double)]


class AnofoxKendallOptions(C.Structure):  # anofox_stats_ffi.h:1731-1738, 16 bytes
    _fields_ = [("alternative", C.c_int), ("tau_type", C.c_int), ("confidence_level", C.c_double)]


class AnofoxCorrelationResult(C.Structure):  # anofox_stats_ffi.h:1611-1628, 64 bytes
    _fields_ = [("r", C.c_double), ("statistic", C.c_double), ("p_value", C.c_double), ("ci_lower", C.c_double), ("ci_upper", C.c_double),
                ("confidence_level", C.c_double), ("n", C.c_size_t), ("method", C.c_char_p)]


class AnofoxHipCorBatchOptions(C.Structure):  # the correlation batch entries' options, 24 bytes
    _fields_ = [("method", C.c_int32), ("alternative", C.c_int32), ("tau_type", C.c_int32), ("confidence_level", C.c_double)]


class AnofoxTestResult(C.Structure):  # anofox_stats_ffi.h:1555-1583, 96 bytes
    _fields_ = [("statistic", C.c_double), ("p_value", C.c_double), ("df", C.c_double), ("effect_size", C.c_double), ("ci_lower", C.c_double),
                ("ci_upper", C.c_double), ("confidence_level", C.c_double), ("n", C.c_size_t), ("n1", C.c_size_t), ("n2", C.c_size_t),
                ("alternative", C.c_int), ("method", C.c_char_p)]


class AnofoxMannWhitneyOptions(C.Structure):  # anofox_stats_ffi.h:1696-1707, 24 bytes; exact = true is refused
    _fields_ = [("alternative", C.c_int), ("exact", C.c_bool), ("continuity_correction", C.c_bool), ("confidence_level", C.c_double),
                ("mu", C.c_double)]


class AnofoxWilcoxonOptions(C.Structure):  # anofox_stats_ffi.h:1920-1931, the same 24 bytes
    _fields_ = AnofoxMannWhitneyOptions._fields_


class AnofoxHipRankTestBatchOptions(C.Structure):  # the rank test batch entries' options, 24 bytes
    _fields_ = [("test", C.c_int32), ("alternative", C.c_int32), ("continuity_correction", C.c_int32), ("mu", C.c_double)]


class AnofoxAnovaResult(C.Structure):  # anofox_stats_ffi.h:1588-1607, 72 bytes
    _fields_ = [("f_statistic", C.c_double), ("p_value", C.c_double), ("df_between", C.c_size_t), ("df_within", C.c_size_t),
                ("ss_between", C.c_double), ("ss_within", C.c_double), ("n_groups", C.c_size_t), ("n", C.c_size_t), ("method", C.c_char_p)]


class AnofoxTTestOptions(C.Structure):  # anofox_stats_ffi.h:1682-1691, 32 bytes
    _fields_ = [("alternative", C.c_int), ("confidence_level", C.c_double), ("var_equal", C.c_bool), ("mu", C.c_double)]


class AnofoxBrunnerMunzelOptions(C.Structure):  # anofox_stats_ffi.h:1799-1804, 16 bytes
    _fields_ = [("alternative", C.c_int), ("confidence_level", C.c_double)]


class AnofoxJarqueBeraResult(C.Structure):  # anofox_stats_ffi.h:621-632, 40 bytes; nothing to free
    _fields_ = [("statistic", C.c_double), ("p_value", C.c_double), ("skewness", C.c_double), ("kurtosis", C.c_double), ("n", C.c_size_t)]


class AnofoxHipNormalityTestBatchOptions(C.Structure):  # the normality test batch entries' options, 8 bytes
    _fields_ = [("test", C.c_int32), ("reserved", C.c_int32)]


class AnofoxChiSquareResult(C.Structure):  # anofox_stats_ffi.h:1634-1643, 32 bytes; method released by anofox_free_chisq_result
    _fields_ = [("statistic", C.c_double), ("p_value", C.c_double), ("df", C.c_size_t), ("method", C.c_char_p)]


class AnofoxChiSquareOptions(C.Structure):  # anofox_stats_ffi.h:1743-1746, 1 byte
    _fields_ = [("correction", C.c_bool)]


class AnofoxFisherExactOptions(C.Structure):  # anofox_stats_ffi.h:1751-1756, 16 bytes
    _fields_ = [("alternative", C.c_int), ("confidence_level", C.c_double)]


class AnofoxHipCategoricalTestBatchOptions(C.Structure):  # the categorical test batch entries' options, 24 bytes
    _fields_ = [("test", C.c_int32), ("alternative", C.c_int32), ("correction", C.c_int32), ("exact", C.c_int32),
                ("confidence_level", C.c_double)]


class AnofoxHipSampleTestBatchOptions(C.Structure):  # the sample test batch entries' options, 40 bytes
    _fields_ = [("test", C.c_int32), ("alternative", C.c_int32), ("kind", C.c_int32), ("mu", C.c_double), ("trim", C.c_double),
                ("confidence_level", C.c_double)]


class AnofoxHipPermTestBatchOptions(C.Structure):  # the permutation test batch entries' options, 32 bytes
    _fields_ = [("test", C.c_int32), ("alternative", C.c_int32), ("n_permutations", C.c_int64), ("seed", C.c_uint64), ("sigma", C.c_double)]


class AnofoxEnergyDistanceOptions(C.Structure):  # anofox_stats_ffi.h:1761-1768, 24 bytes
    _fields_ = [("n_permutations", C.c_size_t), ("seed", C.c_uint64), ("has_seed", C.c_bool)]


class AnofoxMmdOptions(C.Structure):  # anofox_stats_ffi.h:1773-1780, the same 24 bytes
    _fields_ = AnofoxEnergyDistanceOptions._fields_


class AnofoxHipGlmmOptions(C.Structure):  # the batch entries' options (anofox_stats_hip.h), 40 bytes
    _fields_ = [("family", C.c_int), ("fit_intercept", C.c_int), ("reml", C.c_int), ("max_iterations", C.c_uint32),
                ("tolerance", C.c_double), ("compute_inference", C.c_int), ("confidence_level", C.c_double)]


class AnofoxHipGlmmPredictOptions(C.Structure):  # anofox_stats_hip.h, 16 bytes; interval 0 none, 1 confidence, 2 prediction
    _fields_ = [("interval", C.c_int), ("level", C.c_double)]


class AnofoxGlmmOptions(C.Structure):  # anofox_stats_ffi.h:2442-2460, 88 bytes
    _fields_ = [("family", C.c_int), ("fit_intercept", C.c_bool), ("max_iterations", C.c_uint32), ("tolerance", C.c_double),
                ("compute_inference", C.c_bool), ("confidence_level", C.c_double), ("reml", C.c_bool), ("theta", C.c_double),
                ("power", C.c_double), ("offset_column", C.c_size_t), ("random_slopes", C.POINTER(C.c_size_t)),
                ("random_slopes_len", C.c_size_t)]


class AnofoxGlmmResult(C.Structure):  # anofox_stats_ffi.h:2462-2504, 264 bytes
    _fields_ = [("coefficients", C.POINTER(C.c_double)), ("coefficients_len", C.c_size_t), ("intercept", C.c_double),
                ("std_errors", C.POINTER(C.c_double)), ("z_values", C.POINTER(C.c_double)), ("p_values", C.POINTER(C.c_double)),
                ("ci_lower", C.POINTER(C.c_double)), ("ci_upper", C.POINTER(C.c_double)), ("inference_len", C.c_size_t),
                ("intercept_std_error", C.c_double), ("confidence_level", C.c_double), ("var_group", C.c_double),
                ("var_residual", C.c_double), ("icc", C.c_double), ("log_likelihood", C.c_double), ("aic", C.c_double), ("bic", C.c_double),
                ("deviance", C.c_double), ("n_observations", C.c_size_t), ("n_groups", C.c_size_t), ("n_features", C.c_size_t),
                ("iterations", C.c_uint32), ("converged", C.c_bool), ("ranef_group", C.POINTER(C.c_int32)),
                ("ranef_value", C.POINTER(C.c_double)), ("ranef_se", C.POINTER(C.c_double)), ("ranef_n", C.POINTER(C.c_int64)),
                ("ranef_len", C.c_size_t), ("random_cov", C.POINTER(C.c_double)), ("random_dim", C.c_size_t),
                ("ranef_effects", C.POINTER(C.c_double)), ("factor_var", C.POINTER(C.c_double)), ("factor_n_levels", C.POINTER(C.c_int64)),
                ("factor_len", C.c_size_t)]


class AnofoxEbShrinkResult(C.Structure):  # anofox_stats_ffi.h:2405-2418, 96 bytes
    _fields_ = [("mu", C.c_double), ("mu_se", C.c_double), ("tau_squared", C.c_double), ("i_squared", C.c_double), ("q", C.c_double),
                ("n_groups", C.c_size_t), ("estimate", C.POINTER(C.c_double)), ("se", C.POINTER(C.c_double)),
                ("shrunken", C.POINTER(C.c_double)), ("shrunken_se", C.POINTER(C.c_double)), ("weight", C.POINTER(C.c_double)),
                ("len", C.c_size_t)]


# every symbol include/anofox_stats_hip.h declares: name -> (restype, argtypes)
_ERRP = C.POINTER(AnofoxError)
_CTX = C.c_void_p
SYMBOLS = {
    "anofox_ols_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxOlsOptions,
                                  C.POINTER(AnofoxFitResultCore), C.POINTER(AnofoxFitResultInference), _ERRP]),
    "anofox_ridge_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxRidgeOptions,
                                    C.POINTER(AnofoxFitResultCore), C.POINTER(AnofoxFitResultInference), _ERRP]),
    "anofox_wls_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxDataArray,
                                  AnofoxWlsOptions, C.POINTER(AnofoxFitResultCore),
                                  C.POINTER(AnofoxFitResultInference), _ERRP]),
    "anofox_free_result_core": (None, [C.POINTER(AnofoxFitResultCore)]),
    "anofox_free_result_inference": (None, [C.POINTER(AnofoxFitResultInference)]),
    "anofox_compute_aic": (C.c_bool, [C.c_double, C.c_size_t, C.c_size_t, _DP, _ERRP]),
    "anofox_compute_bic": (C.c_bool, [C.c_double, C.c_size_t, C.c_size_t, _DP, _ERRP]),
    "anofox_hip_core_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_inference_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_max_features": (C.c_size_t, []),
    "anofox_hip_context_create": (C.c_bool, [C.c_int, C.POINTER(_CTX), _ERRP]),
    "anofox_hip_context_destroy": (None, [_CTX]),
    "anofox_hip_context_set_stream": (C.c_bool, [_CTX, C.c_void_p, _ERRP]),
    "anofox_hip_context_synchronize": (C.c_bool, [_CTX, _ERRP]),
    "anofox_hip_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                               C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipBatchOptions, C.c_void_p,
                                               C.c_void_p, _ERRP]),
    "anofox_hip_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                             C.POINTER(_DP), _DP, AnofoxHipBatchOptions, _DP, _DP, _ERRP]),
    "anofox_t_critical": (C.c_double, [C.c_double, C.c_size_t]),
    "anofox_predict_with_interval": (C.c_bool, [_DP, C.c_size_t, C.c_double, _DP, C.c_size_t, C.c_double, C.c_size_t,
                                                C.c_double, C.POINTER(AnofoxPredictionResult)]),
    "anofox_predict": (C.c_bool, [C.POINTER(AnofoxDataArray), C.c_size_t, _DP, C.c_size_t, C.c_double,
                                  C.POINTER(_DP), C.POINTER(C.c_size_t), _ERRP]),
    "anofox_free_predictions": (None, [_DP]),
    "anofox_compute_vif": (C.c_bool, [C.POINTER(AnofoxDataArray), C.c_size_t, C.POINTER(_DP), C.POINTER(C.c_size_t), _ERRP]),
    "anofox_free_vif": (None, [_DP]),
    "anofox_compute_residuals": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, C.c_double,
                                            C.c_bool, C.POINTER(AnofoxResidualsResult), _ERRP]),
    "anofox_free_residuals": (None, [C.POINTER(AnofoxResidualsResult)]),
    "anofox_hip_residuals_max_features": (C.c_size_t, []),
    "anofox_hip_residuals_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(C.c_void_p), C.c_void_p, C.c_bool, C.c_bool, C.c_void_p,
                                                     C.c_void_p, _ERRP]),
    "anofox_hip_residuals_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP, _DP,
                                                   C.POINTER(_DP), _DP, C.c_bool, C.c_bool, _DP, _DP, _ERRP]),
    "anofox_hip_vif_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_vif_max_features": (C.c_size_t, []),
    "anofox_hip_vif_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p),
                                               C.c_void_p, _ERRP]),
    "anofox_hip_vif_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), C.POINTER(_DP),
                                             _DP, _ERRP]),
    "anofox_hip_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                       C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                                       AnofoxHipBatchOptions, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                     C.POINTER(_DP), _DP, C.POINTER(C.c_int64), AnofoxHipBatchOptions,
                                                     _DP, _DP, _ERRP]),
    "anofox_hip_fit_predict_expanding_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p,
                                                           C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                                           AnofoxHipBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_fit_predict_expanding_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64),
                                                         _DP, C.POINTER(_DP), _DP, AnofoxHipBatchOptions, _DP, _ERRP]),
    "anofox_hip_fit_predict_window_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p,
                                                        C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                                        AnofoxHipWindowFrame, AnofoxHipBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_fit_predict_window_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64),
                                                      _DP, C.POINTER(_DP), _DP, AnofoxHipWindowFrame,
                                                      AnofoxHipBatchOptions, _DP, _ERRP]),
    "anofox_hip_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p,
                                                   C.POINTER(C.c_void_p), C.c_void_p, C.c_double, C.c_void_p, _ERRP]),
    "anofox_hip_context_enable_timing": (C.c_bool, [_CTX, C.c_bool, _ERRP]),
    "anofox_hip_context_collect_timing": (C.c_bool, [_CTX, C.POINTER(AnofoxHipKernelTimes), _ERRP]),
    "anofox_hip_context_use_own_stream": (C.c_bool, [_CTX, _ERRP]),
    "anofox_hip_context_set_accumulate_gate": (C.c_bool, [_CTX, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_context_last_refine_count": (C.c_bool, [_CTX, C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_version": (C.c_char_p, []),
    "anofox_hip_comm_unique_id": (C.c_bool, [C.c_void_p, _ERRP]),
    "anofox_hip_comm_create": (C.c_bool, [_CTX, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p), _ERRP]),
    "anofox_hip_comm_destroy": (None, [C.c_void_p]),
    "anofox_hip_comm_world_size": (C.c_int, [C.c_void_p]),
    "anofox_hip_comm_rank": (C.c_int, [C.c_void_p]),
    "anofox_hip_comm_ranks_seen": (C.c_int, [C.c_void_p]),
    "anofox_hip_gather_records_device": (C.c_bool, [C.c_void_p, C.c_void_p, C.c_int64, C.c_size_t, C.c_void_p, _ERRP]),
    "anofox_hip_context_last_window_refit_count": (C.c_bool, [_CTX, C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_fit_predict_frames_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                                        C.c_void_p, C.c_void_p, AnofoxHipBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_fit_predict_frames_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, _DP, C.POINTER(_DP), _DP, C.POINTER(C.c_int64),
                                                      C.POINTER(C.c_int64), AnofoxHipBatchOptions, _DP, _ERRP]),
    "anofox_hip_information_criteria_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_void_p, AnofoxHipBatchOptions,
                                                                C.c_void_p, _ERRP]),
    "anofox_hip_information_criteria_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, _DP, AnofoxHipBatchOptions, _DP, _ERRP]),
    "anofox_hip_agg_state_max_features": (C.c_size_t, []),
    "anofox_hip_agg_state_create": (C.c_bool, [_CTX, C.c_size_t, AnofoxHipBatchOptions, C.c_int64, C.POINTER(C.c_void_p), _ERRP]),
    "anofox_hip_agg_state_destroy": (None, [C.c_void_p]),
    "anofox_hip_agg_state_reserve": (C.c_bool, [C.c_void_p, C.c_int64, _ERRP]),
    "anofox_hip_agg_state_retain_rows": (C.c_bool, [C.c_void_p, C.c_size_t, _ERRP]),
    "anofox_hip_agg_state_retain_rows_host": (C.c_bool, [C.c_void_p, C.c_size_t, _ERRP]),
    "anofox_hip_agg_state_retaining": (C.c_int, [C.c_void_p]),
    "anofox_hip_agg_state_retained_host_bytes": (C.c_size_t, [C.c_void_p]),
    "anofox_hip_agg_state_retained_bytes": (C.c_size_t, [C.c_void_p]),
    "anofox_hip_agg_state_slots": (C.c_int64, [C.c_void_p]),
    "anofox_hip_agg_state_rows": (C.c_int64, [C.c_void_p]),
    "anofox_hip_agg_state_update_host": (C.c_bool, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_update_device": (C.c_bool, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_combine": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_combine_ex": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_bool, _ERRP]),
    "anofox_hip_agg_state_finalize_slots_host": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, _DP, _DP, C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_agg_state_release_slots": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_reset": (C.c_bool, [C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_record_len": (C.c_size_t, [C.c_void_p]),
    "anofox_hip_agg_state_export_slots_host": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_import_slots_host": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_finalize_host": (C.c_bool, [C.c_void_p, C.c_int64, _DP, _DP, C.POINTER(C.c_int64), C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_finalize_device": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_finalize_elasticnet_host": (C.c_bool, [C.c_void_p, C.c_int64, AnofoxHipElasticNetBatchOptions, _DP,
                                                                 C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_finalize_elasticnet_device": (C.c_bool, [C.c_void_p, C.c_int64, AnofoxHipElasticNetBatchOptions, C.c_void_p,
                                                                   C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_finalize_elasticnet_slots_host": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, AnofoxHipElasticNetBatchOptions,
                                                                       _DP, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_agg_state_finalize_bls_host": (C.c_bool, [C.c_void_p, C.c_int64, AnofoxHipBlsBatchOptions, _DP, C.POINTER(C.c_int32),
                                                          C.POINTER(C.c_int64), C.c_void_p, _ERRP]),
    "anofox_hip_agg_state_finalize_bls_device": (C.c_bool, [C.c_void_p, C.c_int64, AnofoxHipBlsBatchOptions, C.c_void_p, C.c_void_p,
                                                            _ERRP]),
    "anofox_hip_agg_state_finalize_bls_slots_host": (C.c_bool, [C.c_void_p, C.c_int64, C.c_void_p, AnofoxHipBlsBatchOptions, _DP,
                                                                C.POINTER(C.c_int32), C.POINTER(C.c_int64), _ERRP]),
    "anofox_elasticnet_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxElasticNetOptions,
                                         C.POINTER(AnofoxFitResultCore), _ERRP]),
    "anofox_hip_elasticnet_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                          C.POINTER(C.c_void_p), AnofoxHipElasticNetBatchOptions, C.c_void_p,
                                                          C.c_void_p, _ERRP]),
    "anofox_hip_elasticnet_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                        C.POINTER(_DP), AnofoxHipElasticNetBatchOptions, _DP,
                                                        C.POINTER(C.c_int32), _ERRP]),
    "anofox_hip_elasticnet_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                                  C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipElasticNetBatchOptions,
                                                                  C.c_double, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_elasticnet_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                                C.POINTER(_DP), C.POINTER(C.c_int64), AnofoxHipElasticNetBatchOptions,
                                                                C.c_double, _DP, _DP, _ERRP]),
    "anofox_hip_elasticnet_fit_predict_window_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                                   C.POINTER(C.c_void_p), AnofoxHipWindowFrame,
                                                                   AnofoxHipElasticNetBatchOptions, C.c_double, C.c_void_p, _ERRP]),
    "anofox_hip_elasticnet_fit_predict_window_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                                 C.POINTER(_DP), AnofoxHipWindowFrame, AnofoxHipElasticNetBatchOptions,
                                                                 C.c_double, _DP, _ERRP]),
    "anofox_hip_elasticnet_fit_predict_frames_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                                                   C.c_void_p, C.c_void_p, AnofoxHipElasticNetBatchOptions, C.c_double,
                                                                   C.c_void_p, _ERRP]),
    "anofox_hip_elasticnet_fit_predict_frames_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, _DP, C.POINTER(_DP), C.POINTER(C.c_int64),
                                                                 C.POINTER(C.c_int64), AnofoxHipElasticNetBatchOptions, C.c_double,
                                                                 _DP, _ERRP]),
    "anofox_rls_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxRlsOptions,
                                  C.POINTER(AnofoxFitResultCore), _ERRP]),
    "anofox_hip_rls_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.POINTER(C.c_void_p), AnofoxHipRlsBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_rls_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                 C.POINTER(_DP), AnofoxHipRlsBatchOptions, _DP, _ERRP]),
    "anofox_hip_rls_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                           C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipRlsBatchOptions,
                                                           C.c_double, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_rls_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                         C.POINTER(_DP), C.POINTER(C.c_int64), AnofoxHipRlsBatchOptions,
                                                         C.c_double, _DP, _DP, _ERRP]),
    "anofox_hip_rls_fit_predict_window_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                            C.POINTER(C.c_void_p), AnofoxHipWindowFrame,
                                                            AnofoxHipRlsBatchOptions, C.c_double, C.c_void_p, _ERRP]),
    "anofox_hip_rls_fit_predict_window_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                          C.POINTER(_DP), AnofoxHipWindowFrame, AnofoxHipRlsBatchOptions,
                                                          C.c_double, _DP, _ERRP]),
    "anofox_hip_rls_fit_predict_frames_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                                            C.c_void_p, C.c_void_p, AnofoxHipRlsBatchOptions, C.c_double,
                                                            C.c_void_p, _ERRP]),
    "anofox_hip_rls_fit_predict_frames_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, _DP, C.POINTER(_DP), C.POINTER(C.c_int64),
                                                          C.POINTER(C.c_int64), AnofoxHipRlsBatchOptions, C.c_double,
                                                          _DP, _ERRP]),
    "anofox_bls_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxBlsOptions,
                                  C.POINTER(AnofoxBlsFitResultCore), _ERRP]),
    "anofox_nnls_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t,
                                   C.POINTER(AnofoxBlsFitResultCore), _ERRP]),
    "anofox_free_bls_result": (None, [C.POINTER(AnofoxBlsFitResultCore)]),
    "anofox_hip_bls_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_bls_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                   C.POINTER(C.c_void_p), AnofoxHipBlsBatchOptions, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_bls_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                 C.POINTER(_DP), AnofoxHipBlsBatchOptions, _DP, C.POINTER(C.c_int32), _ERRP]),
    "anofox_hip_bls_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                           C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipBlsBatchOptions,
                                                           C.c_double, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_bls_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                         C.POINTER(_DP), C.POINTER(C.c_int64), AnofoxHipBlsBatchOptions,
                                                         C.c_double, _DP, _DP, _ERRP]),
    "anofox_quantile_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxQuantileOptions,
                                       C.POINTER(AnofoxQuantileFitResultCore), _ERRP]),
    "anofox_free_quantile_result": (None, [C.POINTER(AnofoxQuantileFitResultCore)]),
    "anofox_hip_quantile_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_quantile_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                        C.POINTER(C.c_void_p), AnofoxHipQuantileBatchOptions, C.c_void_p, C.c_void_p,
                                                        _ERRP]),
    "anofox_hip_quantile_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                      C.POINTER(_DP), AnofoxHipQuantileBatchOptions, _DP, C.POINTER(C.c_int32), _ERRP]),
    "anofox_hip_quantile_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                                C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipQuantileBatchOptions,
                                                                C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_quantile_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                              C.POINTER(_DP), C.POINTER(C.c_int64), AnofoxHipQuantileBatchOptions,
                                                              _DP, _DP, _ERRP]),
    "anofox_quantile_fit_path": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxQuantileOptions, _DP,
                                            C.c_size_t, C.POINTER(AnofoxQuantileFitResultCore), _ERRP]),
    "anofox_hip_quantile_fit_path_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                             C.POINTER(C.c_void_p), AnofoxHipQuantileBatchOptions, _DP, C.c_size_t,
                                                             C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_quantile_fit_path_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                           C.POINTER(_DP), AnofoxHipQuantileBatchOptions, _DP, C.c_size_t, _DP,
                                                           C.POINTER(C.c_int32), _ERRP]),
    "anofox_hip_quantile_fit_predict_path_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                                     C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipQuantileBatchOptions,
                                                                     _DP, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_quantile_fit_predict_path_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                                   C.POINTER(_DP), C.POINTER(C.c_int64), AnofoxHipQuantileBatchOptions,
                                                                   _DP, C.c_size_t, _DP, C.POINTER(C.c_int32), _DP, _ERRP]),
    "anofox_hip_quantile_fit_predict_window_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                                 C.POINTER(C.c_void_p), AnofoxHipWindowFrame,
                                                                 AnofoxHipQuantileBatchOptions, C.c_void_p, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_quantile_fit_predict_window_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                               C.POINTER(_DP), AnofoxHipWindowFrame, AnofoxHipQuantileBatchOptions,
                                                               _DP, _DP, C.POINTER(C.c_int32), _ERRP]),
    "anofox_hip_quantile_fit_predict_frames_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                                                 C.c_void_p, C.c_void_p, AnofoxHipQuantileBatchOptions, C.c_void_p,
                                                                 C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_quantile_fit_predict_frames_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, _DP, C.POINTER(_DP), C.POINTER(C.c_int64),
                                                               C.POINTER(C.c_int64), AnofoxHipQuantileBatchOptions, _DP, _DP,
                                                               C.POINTER(C.c_int32), _ERRP]),
    "anofox_hip_quantile_window_plan": (C.c_bool, [C.c_int64, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64),
                                                   C.POINTER(C.c_int64), C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_int64,
                                                   C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_quantile_window_test_hooks": (None, [C.c_int64, C.c_int64]),
    "anofox_hip_quantile_window_stats": (C.c_bool, [_CTX, C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_glm_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_glm_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                                   C.c_void_p, AnofoxHipGlmBatchOptions, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_glm_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP, C.POINTER(_DP), _DP,
                                                 AnofoxHipGlmBatchOptions, _DP, _DP, _ERRP]),
    "anofox_hip_glm_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                           C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, AnofoxHipGlmBatchOptions,
                                                           C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_glm_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                         C.POINTER(_DP), _DP, C.POINTER(C.c_int64), AnofoxHipGlmBatchOptions, _DP, _DP,
                                                         _ERRP]),
    "anofox_hip_glm_fit_predict_interval_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                                    C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                                                    AnofoxHipGlmBatchOptions, C.c_double, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_glm_fit_predict_interval_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                                  C.POINTER(_DP), _DP, C.POINTER(C.c_int64), AnofoxHipGlmBatchOptions,
                                                                  C.c_double, _DP, _DP, _ERRP]),
    "anofox_hip_glm_fit_accuracy_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                            C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipGlmBatchOptions, C.c_double,
                                                            C.c_void_p, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_glm_fit_accuracy_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                          C.POINTER(_DP), _DP, AnofoxHipGlmBatchOptions, C.c_double, _DP, _DP, _DP,
                                                          _ERRP]),
    "anofox_hip_glm_fit_predict_window_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                            C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipWindowFrame,
                                                            AnofoxHipGlmBatchOptions, C.c_double, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_glm_fit_predict_window_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                          C.POINTER(_DP), _DP, AnofoxHipWindowFrame, AnofoxHipGlmBatchOptions,
                                                          C.c_double, _DP, _DP, _ERRP]),
    "anofox_hip_glm_fit_predict_frames_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p),
                                                            C.c_void_p, C.c_void_p, C.c_void_p, AnofoxHipGlmBatchOptions, C.c_double,
                                                            C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_glm_fit_predict_frames_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, _DP, C.POINTER(_DP), _DP,
                                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), AnofoxHipGlmBatchOptions,
                                                          C.c_double, _DP, _DP, _ERRP]),
    "anofox_hip_glm_window_plan": (C.c_bool, [C.c_int64, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64),
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_glm_window_test_hooks": (None, [C.c_int64, C.c_int64, C.c_int]),
    "anofox_hip_glm_window_stats": (C.c_bool, [_CTX, C.POINTER(C.c_int64), _ERRP]),
    "anofox_poisson_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxPoissonOptions,
                                      C.POINTER(AnofoxGlmFitResultCore), C.POINTER(AnofoxFitResultInference), _ERRP]),
    "anofox_binomial_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxBinomialOptions,
                                       C.POINTER(AnofoxGlmFitResultCore), C.POINTER(AnofoxFitResultInference), _ERRP]),
    "anofox_logistic_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxLogisticOptions,
                                       C.POINTER(AnofoxGlmFitResultCore), C.POINTER(AnofoxFitResultInference),
                                       C.POINTER(AnofoxLogisticFitExtras), _ERRP]),
    "anofox_free_glm_result": (None, [C.POINTER(AnofoxGlmFitResultCore)]),
    "anofox_hip_aft_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_aft_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p),
                                                   C.c_void_p, AnofoxHipAftBatchOptions, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_aft_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP, C.POINTER(_DP), _DP,
                                                 AnofoxHipAftBatchOptions, _DP, _DP, _ERRP]),
    "anofox_hip_aft_test_hooks": (None, [C.c_int64]),
    "anofox_hip_aft_pred_len": (C.c_size_t, []),
    "anofox_hip_aft_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                           C.POINTER(C.c_void_p), C.c_void_p, AnofoxHipAftBatchOptions,
                                                           AnofoxHipAftPredictOptions, C.c_void_p, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_aft_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64), _DP,
                                                         C.POINTER(_DP), _DP, AnofoxHipAftBatchOptions, AnofoxHipAftPredictOptions,
                                                         _DP, _DP, _DP, _ERRP]),
    "anofox_aft_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, AnofoxDataArray, AnofoxAftOptions,
                                  C.POINTER(AnofoxAftFitResultCore), C.POINTER(AnofoxAftInference), _ERRP]),
    "anofox_free_aft_result": (None, [C.POINTER(AnofoxAftFitResultCore)]),
    "anofox_free_aft_inference": (None, [C.POINTER(AnofoxAftInference)]),
    "anofox_hip_eb_shrink_summary_len": (C.c_size_t, []),
    "anofox_hip_eb_shrink_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_int64, AnofoxHipEbShrinkOptions, C.c_void_p, C.c_void_p, _ERRP]),
    "anofox_hip_eb_shrink_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.c_size_t, _DP, C.c_int64, _DP,
                                                   C.c_int64, AnofoxHipEbShrinkOptions, _DP, _DP, _ERRP]),
    "anofox_hip_eb_shrink_test_hooks": (None, [C.c_int, C.c_int64, C.c_int64]),
    "anofox_eb_shrink": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxEbShrinkOptions, C.POINTER(AnofoxEbShrinkResult), _ERRP]),
    "anofox_free_eb_shrink_result": (None, [C.POINTER(AnofoxEbShrinkResult)]),
    "anofox_hip_cor_record_len": (C.c_size_t, []),
    "anofox_hip_cor_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, AnofoxHipCorBatchOptions,
                                               C.c_void_p, _ERRP]),
    "anofox_hip_cor_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _DP, _DP, AnofoxHipCorBatchOptions, _DP, _ERRP]),
    "anofox_hip_cor_test_hooks": (None, [C.c_int64]),
    "anofox_pearson_cor": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxCorrelationOptions, C.POINTER(AnofoxCorrelationResult), _ERRP]),
    "anofox_spearman_cor": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxCorrelationOptions, C.POINTER(AnofoxCorrelationResult), _ERRP]),
    "anofox_kendall_cor": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxKendallOptions, C.POINTER(AnofoxCorrelationResult), _ERRP]),
    "anofox_free_correlation_result": (None, [C.POINTER(AnofoxCorrelationResult)]),
    "anofox_hip_rank_test_record_len": (C.c_size_t, []),
    "anofox_hip_rank_test_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     AnofoxHipRankTestBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_rank_test_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _DP, _DP, C.POINTER(C.c_int32),
                                                   AnofoxHipRankTestBatchOptions, _DP, _ERRP]),
    "anofox_hip_rank_test_hooks": (None, [C.c_int64]),
    "anofox_mann_whitney_u": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxMannWhitneyOptions, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_wilcoxon_signed_rank": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxWilcoxonOptions, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_kruskal_wallis": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_free_test_result": (None, [C.POINTER(AnofoxTestResult)]),
    "anofox_hip_sample_test_record_len": (C.c_size_t, []),
    "anofox_hip_sample_test_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       AnofoxHipSampleTestBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_sample_test_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _DP, _DP, C.POINTER(C.c_int32),
                                                     AnofoxHipSampleTestBatchOptions, _DP, _ERRP]),
    "anofox_hip_sample_test_hooks": (None, [C.c_int64]),
    "anofox_t_test": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxTTestOptions, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_yuen_test": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, C.c_double, C.c_int, C.c_double, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_brunner_munzel": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxBrunnerMunzelOptions, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_one_way_anova": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, C.POINTER(AnofoxAnovaResult), _ERRP]),
    "anofox_brown_forsythe": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_free_anova_result": (None, [C.POINTER(AnofoxAnovaResult)]),
    "anofox_hip_normality_test_record_len": (C.c_size_t, []),
    "anofox_hip_normality_test_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, AnofoxHipNormalityTestBatchOptions,
                                                          C.c_void_p, _ERRP]),
    "anofox_hip_normality_test_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _DP, AnofoxHipNormalityTestBatchOptions,
                                                        _DP, _ERRP]),
    "anofox_hip_normality_test_hooks": (None, [C.c_int64]),
    "anofox_shapiro_wilk": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_dagostino_k2": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_jarque_bera": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxJarqueBeraResult), _ERRP]),
    "anofox_hip_categorical_test_record_len": (C.c_size_t, []),
    "anofox_hip_categorical_test_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            AnofoxHipCategoricalTestBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_categorical_test_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                                          C.POINTER(C.c_int32), AnofoxHipCategoricalTestBatchOptions, _DP, _ERRP]),
    "anofox_hip_categorical_test_hooks": (None, [C.c_int64]),
    "anofox_chisq_test": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxChiSquareOptions, C.POINTER(AnofoxChiSquareResult), _ERRP]),
    "anofox_free_chisq_result": (None, [C.POINTER(AnofoxChiSquareResult)]),
    "anofox_g_test": (C.c_bool, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t, C.POINTER(AnofoxChiSquareResult), _ERRP]),
    "anofox_cramers_v": (C.c_bool, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t, _DP, _ERRP]),
    "anofox_contingency_coef": (C.c_bool, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_size_t, _DP, _ERRP]),
    "anofox_phi_coefficient": (C.c_bool, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, _DP, _ERRP]),
    "anofox_fisher_exact": (C.c_bool, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, AnofoxFisherExactOptions,
                                       C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_mcnemar_test": (C.c_bool, [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_bool, C.c_bool,
                                       C.POINTER(AnofoxChiSquareResult), _ERRP]),
    "anofox_hip_perm_test_record_len": (C.c_size_t, []),
    "anofox_hip_perm_test_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     AnofoxHipPermTestBatchOptions, C.c_void_p, _ERRP]),
    "anofox_hip_perm_test_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.POINTER(C.c_int64), _DP, C.POINTER(C.c_int32),
                                                   AnofoxHipPermTestBatchOptions, _DP, _ERRP]),
    "anofox_hip_perm_test_hooks": (None, [C.c_int64]),
    "anofox_energy_distance": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxEnergyDistanceOptions, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_mmd": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, AnofoxMmdOptions, C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_permutation_t_test": (C.c_bool, [AnofoxDataArray, AnofoxDataArray, C.c_int, C.c_size_t, C.c_uint64, C.c_bool,
                                             C.POINTER(AnofoxTestResult), _ERRP]),
    "anofox_hip_glmm_record_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_glmm_inference_len": (C.c_size_t, [C.c_size_t]),
    "anofox_hip_glmm_test_hooks": (None, [C.c_int, C.c_int]),
    "anofox_hip_glmm_fit_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.POINTER(C.c_void_p), AnofoxHipGlmmOptions, C.c_void_p, C.c_void_p, C.c_void_p,
                                                    C.c_void_p, _ERRP]),
    "anofox_hip_glmm_fit_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64),
                                                  C.POINTER(C.c_int64), _DP, C.POINTER(_DP), AnofoxHipGlmmOptions, _DP, _DP, _DP,
                                                  C.POINTER(C.c_int64), _ERRP]),
    "anofox_hip_glmm_pred_len": (C.c_size_t, []),
    "anofox_hip_glmm_fit_predict_batch_device": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_size_t, C.c_int64, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.POINTER(C.c_void_p), AnofoxHipGlmmOptions,
                                                            AnofoxHipGlmmPredictOptions, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, _ERRP]),
    "anofox_hip_glmm_fit_predict_batch_host": (C.c_bool, [_CTX, C.c_int64, C.c_int64, C.c_size_t, C.c_int64, C.POINTER(C.c_int64),
                                                          C.POINTER(C.c_int64), _DP, C.POINTER(_DP), AnofoxHipGlmmOptions,
                                                          AnofoxHipGlmmPredictOptions, _DP, _DP, _DP, C.POINTER(C.c_int64), _DP, _ERRP]),
    "anofox_glmm_fit": (C.c_bool, [AnofoxDataArray, C.POINTER(AnofoxDataArray), C.c_size_t, C.POINTER(C.c_int32), C.c_size_t,
                                   C.c_void_p, C.c_size_t, AnofoxGlmmOptions, C.POINTER(AnofoxGlmmResult), _ERRP]),
    "anofox_free_glmm_result": (None, [C.POINTER(AnofoxGlmmResult)]),
    "anofox_aft_cdf": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_int]),
    "anofox_aft_quantile": (C.c_double, [C.c_double, C.c_double, C.c_double, C.c_int]),
    "anofox_hip_host_alloc": (C.c_void_p, [C.c_size_t]),
    "anofox_hip_host_free": (None, [C.c_void_p]),
}

_lib = None


def load():
    """Load the shared library and bind every declared symbol.  Raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C anofox-statistics_amd/csrc` "
            "(or __graft_entry__.build()).  There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class AnofoxStatsError(RuntimeError):
    """A failed library call; carries the AnofoxErrorCode."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code
