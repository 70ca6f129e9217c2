"""anofox-statistics_amd — MI355X-native grouped least-squares (ols_fit_agg / ridge_fit_agg / wls_fit_agg).

The product is libanofox_stats_hip.so (hand-written HIP for gfx950 behind the C ABI of
include/anofox_stats_hip.h).  This package is its host-side mirror of the reference's operator
interface: the aggregates (aggregate.py), the scalar functions (scalar.py), the options parser
(options.py), plus device-resident and multi-GPU drivers (runtime.py, distributed.py).

Importing the package loads the shared library and fails if it is missing — there is no CPU fallback.
"""
from . import _abi

_abi.load()

from ._abi import AnofoxStatsError  # noqa: E402
from .aggregate import (StreamingStates, FitAggResult, FitPredictAggResult, OlsFitAgg, OlsFitPredictAgg, RidgeFitAgg,  # noqa: E402
                        RidgeFitPredictAgg, WlsFitAgg, WlsFitPredictAgg, SQL_FUNCTIONS, ols_fit_agg,
                        ols_fit_predict_agg, ridge_fit_agg, ridge_fit_predict_agg, wls_fit_agg, wls_fit_predict_agg,
                        result_from_records, ols_fit_predict, ridge_fit_predict, wls_fit_predict, vif_agg,
                        residuals_diagnostics_agg, ElasticNetFitPredictAgg, elasticnet_fit_predict_agg,
                        elasticnet_fit_predict, RlsFitAgg, rls_fit_agg, RlsFitPredictAgg, rls_fit_predict_agg,
                        rls_fit_predict, BlsFitAggResult, BlsFitAgg, NnlsFitAgg, BlsFitPredictAgg, bls_fit_agg, nnls_fit_agg,
                        bls_fit_predict_agg, bls_result_from_records, QuantileFitPredictAgg, quantile_fit_predict_agg,
                        QuantilePathFitPredictAgg, QuantilePathFitPredictAggResult, quantile_path_fit_predict_agg,
                        quantile_fit_predict)
from .options import (ElasticNetOptions, ElasticNetPredictOptions, InvalidInputException, RegressionOptions,  # noqa: E402
                      parse_elasticnet_options, parse_elasticnet_predict_options, parse_options, RlsOptions,
                      parse_rls_options, BlsOptions, parse_bls_options, parse_nnls_options, parse_bls_predict_options,
                      QuantileOptions, parse_quantile_options, QuantilePathOptions, parse_quantile_path_options)
from .runtime import (AggState, Context, quantile_fit_predict_window_host, quantile_fit_predict_frames_host,  # noqa: E402
                      quantile_window_plan, quantile_window_test_hooks, quantile_window_stats, quantile_fit_path_batch_host,
                      quantile_fit_path_batch_device, quantile_fit_predict_path_batch_host, quantile_fit_batch_host,
                      quantile_fit_predict_batch_host, bls_fit_batch_host, bls_fit_predict_batch_host, rls_fit_batch_host,
                      rls_fit_predict_batch_host, rls_fit_predict_window_host, rls_fit_predict_frames_host,
                      elasticnet_fit_batch_host, elasticnet_fit_predict_batch_host, elasticnet_fit_predict_frames_host,
                      elasticnet_fit_predict_window_host, information_criteria_host, fit_predict_frames_host, fit_batch_host,
                      fit_predict_batch_host, fit_predict_expanding_host, fit_predict_window_host, vif_batch_host,
                      residuals_batch_host)
from .glm import (GlmFitAggResult, binomial_fit_agg, glm_fit_batch_device, glm_fit_batch_host, glm_fit_predict_batch_device, glm_fit_predict_batch_host,  # noqa: E402
                  logistic_fit, logistic_fit_agg, poisson_fit, poisson_fit_agg, poisson_fit_predict_agg,
                  GlmFitPredictResult, binomial_fit_predict, logistic_fit_predict, poisson_fit_predict, glm_fit_predict_window_host,
                  glm_fit_predict_frames_host, glm_fit_predict_window_device, glm_fit_predict_frames_device, glm_window_plan,
                  glm_window_stats, glm_window_test_hooks)
from .options import GlmOptions, parse_binomial_options, parse_poisson_options  # noqa: E402
from .aft import (AftFitAggResult, AftFitPredictAggResult, AftOptions, aft_cdf, aft_fit, aft_fit_agg, aft_fit_batch_device,  # noqa: E402
                  aft_fit_batch_host, aft_fit_predict_agg, aft_fit_predict_batch_device, aft_fit_predict_batch_host, aft_quantile,
                  aft_test_hooks, parse_aft_options)
from .eb_shrink import (EbShrinkOptions, ShrunkCoefficients, eb_shrink, eb_shrink_agg, eb_shrink_batch_device, eb_shrink_batch_host,  # noqa: E402
                        eb_shrink_test_hooks, parse_eb_shrink_options, shrink_coefficients)
from .correlation import (CorrelationAggResult, CorrelationOptions, cor_batch_device, cor_batch_host, cor_test_hooks, kendall,  # noqa: E402
                          kendall_agg, parse_correlation_options, pearson, pearson_agg, spearman, spearman_agg)
from .rank_tests import (RankTestAggResult, RankTestOptions, kruskal_wallis, kruskal_wallis_agg, mann_whitney_u, mann_whitney_u_agg,  # noqa: E402
                         parse_rank_test_options, rank_test_batch_device, rank_test_batch_host, rank_test_hooks, wilcoxon_signed_rank,
                         wilcoxon_signed_rank_agg)
from .sample_tests import (SampleTestAggResult, SampleTestOptions, brown_forsythe, brown_forsythe_agg, brunner_munzel,  # noqa: E402
                           brunner_munzel_agg, one_way_anova, one_way_anova_agg, paired_t_test, paired_t_test_agg, parse_sample_test_options,
                           sample_test_batch_device, sample_test_batch_host, sample_test_hooks, t_test, t_test_agg, yuen, yuen_agg)
from .normality_tests import (NormalityTestAggResult, dagostino_k2, dagostino_k2_agg, jarque_bera, jarque_bera_agg,  # noqa: E402
                              normality_test_batch_device, normality_test_batch_host, normality_test_hooks, shapiro_wilk,
                              shapiro_wilk_agg)
from .categorical_tests import (CategoricalTestAggResult, CategoricalTestOptions, categorical_test_batch_device,  # noqa: E402
                                categorical_test_batch_host, categorical_test_hooks, chisq_test, chisq_test_agg, contingency_coef,
                                contingency_coef_agg, cramers_v, cramers_v_agg, fisher_exact, fisher_exact_agg, g_test, g_test_agg,
                                mcnemar_agg, mcnemar_test, parse_categorical_test_options, phi_coefficient, phi_coefficient_agg)
from .perm_tests import (PermTestAggResult, PermTestOptions, energy_distance, energy_distance_agg, mmd, mmd_agg,  # noqa: E402
                         parse_perm_test_options, perm_test_batch_device, perm_test_batch_host, perm_test_hooks, permutation_t_test,
                         permutation_t_test_agg)
from .glmm import (GlmmFitAggResult, GlmmFitPredictAggResult, GlmmOptions, glmm_fit, glmm_fit_agg, glmm_fit_batch_device,  # noqa: E402
                   glmm_fit_batch_host, glmm_fit_predict_agg, glmm_fit_predict_batch_device, glmm_fit_predict_batch_host, glmm_test_hooks,
                   parse_glmm_options)
from .scalar import quantile_fit, quantile_fit_path, aic, bic, elasticnet_fit, rls_fit, ols_fit, predict, predict_with_interval, ridge_fit, t_critical, vif, wls_fit, residuals_diagnostics  # noqa: E402

# the scalar functions under their SQL names (src/table_functions/{ols,ridge,wls}_fit.cpp, predict.cpp,
# src/scalar_functions/{aic_bic,vif}.cpp) and the deprecated aggregate aliases
SQL_FUNCTIONS.update({
    "anofox_stats_ols_fit": ols_fit, "ols_fit": ols_fit,
    "anofox_stats_ridge_fit": ridge_fit, "ridge_fit": ridge_fit,
    "anofox_stats_wls_fit": wls_fit, "wls_fit": wls_fit,
    "anofox_stats_elasticnet_fit": elasticnet_fit, "elasticnet_fit": elasticnet_fit,
    "anofox_stats_rls_fit": rls_fit, "rls_fit": rls_fit,
    "anofox_stats_quantile_fit": quantile_fit, "quantile_fit": quantile_fit,
    "anofox_stats_quantile_fit_path": quantile_fit_path, "quantile_fit_path": quantile_fit_path,
    "anofox_stats_poisson_fit": poisson_fit, "poisson_fit": poisson_fit,
    "anofox_stats_logistic_fit": logistic_fit, "logistic_fit": logistic_fit,
    "anofox_stats_poisson_fit_predict": poisson_fit_predict, "poisson_fit_predict": poisson_fit_predict,
    "anofox_stats_logistic_fit_predict": logistic_fit_predict, "logistic_fit_predict": logistic_fit_predict,
    "anofox_stats_binomial_fit_predict": binomial_fit_predict, "binomial_fit_predict": binomial_fit_predict,
    "anofox_stats_aft_fit": aft_fit, "aft_fit": aft_fit,
    "anofox_stats_aft_cdf": aft_cdf, "aft_cdf": aft_cdf, "anofox_stats_aft_quantile": aft_quantile, "aft_quantile": aft_quantile,
    "anofox_stats_eb_shrink": eb_shrink, "eb_shrink": eb_shrink,
    "anofox_stats_eb_shrink_agg": eb_shrink_agg, "eb_shrink_agg": eb_shrink_agg,
    "anofox_stats_pearson": pearson, "pearson": pearson, "anofox_stats_pearson_agg": pearson_agg, "pearson_agg": pearson_agg,
    "anofox_stats_spearman": spearman, "spearman": spearman, "anofox_stats_spearman_agg": spearman_agg, "spearman_agg": spearman_agg,
    "anofox_stats_kendall": kendall, "kendall": kendall, "anofox_stats_kendall_agg": kendall_agg, "kendall_agg": kendall_agg,
    "anofox_stats_energy_distance": energy_distance, "energy_distance": energy_distance,
    "anofox_stats_energy_distance_agg": energy_distance_agg, "energy_distance_agg": energy_distance_agg,
    "anofox_stats_mmd": mmd, "mmd": mmd, "anofox_stats_mmd_agg": mmd_agg, "mmd_agg": mmd_agg,
    "anofox_stats_permutation_t_test": permutation_t_test, "permutation_t_test": permutation_t_test,
    "anofox_stats_permutation_t_test_agg": permutation_t_test_agg, "permutation_t_test_agg": permutation_t_test_agg,
    "anofox_stats_mann_whitney_u": mann_whitney_u, "mann_whitney_u": mann_whitney_u,
    "anofox_stats_mann_whitney_u_agg": mann_whitney_u_agg, "mann_whitney_u_agg": mann_whitney_u_agg,
    "anofox_stats_wilcoxon_signed_rank": wilcoxon_signed_rank, "wilcoxon_signed_rank": wilcoxon_signed_rank,
    "anofox_stats_wilcoxon_signed_rank_agg": wilcoxon_signed_rank_agg, "wilcoxon_signed_rank_agg": wilcoxon_signed_rank_agg,
    "anofox_stats_kruskal_wallis": kruskal_wallis, "kruskal_wallis": kruskal_wallis,
    "anofox_stats_kruskal_wallis_agg": kruskal_wallis_agg, "kruskal_wallis_agg": kruskal_wallis_agg,
    "anofox_stats_t_test": t_test, "t_test": t_test, "anofox_stats_t_test_agg": t_test_agg, "t_test_agg": t_test_agg,
    "anofox_stats_paired_t_test": paired_t_test, "paired_t_test": paired_t_test,
    "anofox_stats_paired_t_test_agg": paired_t_test_agg, "paired_t_test_agg": paired_t_test_agg,
    "anofox_stats_yuen": yuen, "yuen": yuen, "anofox_stats_yuen_agg": yuen_agg, "yuen_agg": yuen_agg,
    "anofox_stats_one_way_anova": one_way_anova, "one_way_anova": one_way_anova,
    "anofox_stats_one_way_anova_agg": one_way_anova_agg, "one_way_anova_agg": one_way_anova_agg,
    "anofox_stats_brown_forsythe": brown_forsythe, "brown_forsythe": brown_forsythe,
    "anofox_stats_brown_forsythe_agg": brown_forsythe_agg, "brown_forsythe_agg": brown_forsythe_agg,
    "anofox_stats_brunner_munzel": brunner_munzel, "brunner_munzel": brunner_munzel,
    "anofox_stats_brunner_munzel_agg": brunner_munzel_agg, "brunner_munzel_agg": brunner_munzel_agg,
    "anofox_stats_shapiro_wilk": shapiro_wilk, "shapiro_wilk": shapiro_wilk,
    "anofox_stats_shapiro_wilk_agg": shapiro_wilk_agg, "shapiro_wilk_agg": shapiro_wilk_agg,
    "anofox_stats_dagostino_k2": dagostino_k2, "dagostino_k2": dagostino_k2,
    "anofox_stats_dagostino_k2_agg": dagostino_k2_agg, "dagostino_k2_agg": dagostino_k2_agg,
    "anofox_stats_jarque_bera": jarque_bera, "jarque_bera": jarque_bera,
    "anofox_stats_jarque_bera_agg": jarque_bera_agg, "jarque_bera_agg": jarque_bera_agg,
    "anofox_stats_chisq_test": chisq_test, "chisq_test": chisq_test,
    "anofox_stats_chisq_test_agg": chisq_test_agg, "chisq_test_agg": chisq_test_agg,
    "anofox_stats_g_test": g_test, "g_test": g_test, "anofox_stats_g_test_agg": g_test_agg, "g_test_agg": g_test_agg,
    "anofox_stats_fisher_exact": fisher_exact, "fisher_exact": fisher_exact,
    "anofox_stats_fisher_exact_agg": fisher_exact_agg, "fisher_exact_agg": fisher_exact_agg,
    "anofox_stats_mcnemar_test": mcnemar_test, "mcnemar_test": mcnemar_test,
    "anofox_stats_mcnemar_agg": mcnemar_agg, "mcnemar_agg": mcnemar_agg,
    "anofox_stats_cramers_v": cramers_v, "cramers_v": cramers_v,
    "anofox_stats_cramers_v_agg": cramers_v_agg, "cramers_v_agg": cramers_v_agg,
    "anofox_stats_phi_coefficient": phi_coefficient, "phi_coefficient": phi_coefficient,
    "anofox_stats_phi_coefficient_agg": phi_coefficient_agg, "phi_coefficient_agg": phi_coefficient_agg,
    "anofox_stats_contingency_coef": contingency_coef, "contingency_coef": contingency_coef,
    "anofox_stats_contingency_coef_agg": contingency_coef_agg, "contingency_coef_agg": contingency_coef_agg,
    "anofox_stats_glmm_fit": glmm_fit, "glmm_fit": glmm_fit, "anofox_stats_glmm_fit_agg": glmm_fit_agg, "glmm_fit_agg": glmm_fit_agg,
    "anofox_stats_glmm_fit_predict_agg": glmm_fit_predict_agg, "glmm_fit_predict_agg": glmm_fit_predict_agg,
    "anofox_stats_predict": predict,
    "anofox_stats_aic": aic, "aic": aic, "anofox_stats_bic": bic, "bic": bic,
    "anofox_stats_vif": vif, "vif": vif,
    "anofox_stats_residuals_diagnostics": residuals_diagnostics, "residuals_diagnostics": residuals_diagnostics,
    "ridge_predict_agg": ridge_fit_predict_agg, "wls_predict_agg": wls_fit_predict_agg,
})

__all__ = [
    "AggState", "StreamingStates", "information_criteria_host", "fit_predict_frames_host", "AnofoxStatsError", "Context", "FitAggResult", "InvalidInputException", "OlsFitAgg", "RegressionOptions",
    "RidgeFitAgg", "SQL_FUNCTIONS", "WlsFitAgg", "aic", "bic", "fit_batch_host", "ols_fit", "ols_fit_agg",
    "parse_options", "result_from_records", "ridge_fit", "ridge_fit_agg", "wls_fit", "wls_fit_agg",
    "FitPredictAggResult", "OlsFitPredictAgg", "RidgeFitPredictAgg", "WlsFitPredictAgg", "fit_predict_batch_host",
    "ols_fit_predict_agg", "ridge_fit_predict_agg", "wls_fit_predict_agg", "predict", "predict_with_interval",
    "t_critical", "fit_predict_expanding_host", "fit_predict_window_host", "ols_fit_predict", "ridge_fit_predict", "wls_fit_predict",
    "vif", "vif_agg", "vif_batch_host", "residuals_diagnostics", "residuals_diagnostics_agg", "residuals_batch_host",
    "ElasticNetOptions", "elasticnet_fit", "elasticnet_fit_batch_host", "parse_elasticnet_options",
    "ElasticNetPredictOptions", "parse_elasticnet_predict_options", "ElasticNetFitPredictAgg", "elasticnet_fit_predict_agg",
    "elasticnet_fit_predict", "elasticnet_fit_predict_batch_host", "elasticnet_fit_predict_window_host",
    "elasticnet_fit_predict_frames_host",
    "RlsOptions", "parse_rls_options", "rls_fit", "RlsFitAgg", "rls_fit_agg", "RlsFitPredictAgg", "rls_fit_predict_agg",
    "rls_fit_predict", "rls_fit_batch_host", "rls_fit_predict_batch_host", "rls_fit_predict_window_host",
    "rls_fit_predict_frames_host",
    "BlsOptions", "parse_bls_options", "parse_nnls_options", "parse_bls_predict_options", "BlsFitAggResult", "BlsFitAgg",
    "NnlsFitAgg", "BlsFitPredictAgg", "bls_fit_agg", "nnls_fit_agg", "bls_fit_predict_agg", "bls_result_from_records",
    "bls_fit_batch_host", "bls_fit_predict_batch_host",
    "QuantileOptions", "parse_quantile_options", "quantile_fit", "QuantileFitPredictAgg", "quantile_fit_predict_agg",
    "quantile_fit_batch_host", "quantile_fit_predict_batch_host",
    "QuantilePathOptions", "parse_quantile_path_options", "quantile_fit_path", "QuantilePathFitPredictAgg",
    "QuantilePathFitPredictAggResult", "quantile_path_fit_predict_agg", "quantile_fit_path_batch_host",
    "quantile_fit_path_batch_device", "quantile_fit_predict_path_batch_host",
    "quantile_fit_predict", "quantile_fit_predict_window_host", "quantile_fit_predict_frames_host", "quantile_window_plan",
    "quantile_window_test_hooks", "quantile_window_stats",
    "GlmOptions", "parse_poisson_options", "parse_binomial_options", "GlmFitAggResult", "poisson_fit_agg", "binomial_fit_agg",
    "logistic_fit_agg", "poisson_fit_predict_agg", "poisson_fit", "logistic_fit", "glm_fit_batch_host",
    "glm_fit_predict_batch_host", "glm_fit_batch_device", "glm_fit_predict_batch_device",
    "GlmFitPredictResult", "poisson_fit_predict", "logistic_fit_predict", "binomial_fit_predict", "glm_fit_predict_window_host",
    "glm_fit_predict_frames_host", "glm_fit_predict_window_device", "glm_fit_predict_frames_device", "glm_window_plan",
    "glm_window_stats", "glm_window_test_hooks",
    "AftOptions", "parse_aft_options", "AftFitAggResult", "aft_fit_agg", "aft_fit", "aft_cdf", "aft_quantile", "aft_fit_batch_host",
    "aft_fit_batch_device", "aft_test_hooks", "AftFitPredictAggResult", "aft_fit_predict_agg", "aft_fit_predict_batch_host",
    "aft_fit_predict_batch_device",
    "EbShrinkOptions", "parse_eb_shrink_options", "ShrunkCoefficients", "eb_shrink", "eb_shrink_agg", "eb_shrink_batch_host",
    "eb_shrink_batch_device", "eb_shrink_test_hooks", "shrink_coefficients",
    "CorrelationOptions", "CorrelationAggResult", "parse_correlation_options", "pearson", "spearman", "kendall", "pearson_agg",
    "spearman_agg", "kendall_agg", "cor_batch_host", "cor_batch_device", "cor_test_hooks",
    "RankTestOptions", "RankTestAggResult", "parse_rank_test_options", "mann_whitney_u", "wilcoxon_signed_rank", "kruskal_wallis",
    "mann_whitney_u_agg", "wilcoxon_signed_rank_agg", "kruskal_wallis_agg", "rank_test_batch_host", "rank_test_batch_device",
    "rank_test_hooks",
    "PermTestOptions", "PermTestAggResult", "parse_perm_test_options", "energy_distance", "mmd", "permutation_t_test",
    "energy_distance_agg", "mmd_agg", "permutation_t_test_agg", "perm_test_batch_host", "perm_test_batch_device", "perm_test_hooks",
    "SampleTestOptions", "SampleTestAggResult", "parse_sample_test_options", "t_test", "paired_t_test", "yuen", "one_way_anova",
    "brown_forsythe", "brunner_munzel", "t_test_agg", "paired_t_test_agg", "yuen_agg", "one_way_anova_agg", "brown_forsythe_agg",
    "brunner_munzel_agg", "sample_test_batch_host", "sample_test_batch_device", "sample_test_hooks",
    "NormalityTestAggResult", "shapiro_wilk", "dagostino_k2", "jarque_bera", "shapiro_wilk_agg", "dagostino_k2_agg", "jarque_bera_agg",
    "normality_test_batch_host", "normality_test_batch_device", "normality_test_hooks",
    "CategoricalTestOptions", "CategoricalTestAggResult", "parse_categorical_test_options", "chisq_test", "g_test", "fisher_exact",
    "mcnemar_test", "cramers_v", "phi_coefficient", "contingency_coef", "chisq_test_agg", "g_test_agg", "fisher_exact_agg", "mcnemar_agg",
    "cramers_v_agg", "phi_coefficient_agg", "contingency_coef_agg", "categorical_test_batch_host", "categorical_test_batch_device",
    "categorical_test_hooks",
    "GlmmOptions", "GlmmFitAggResult", "parse_glmm_options", "glmm_fit", "glmm_fit_agg", "glmm_fit_batch_host", "glmm_fit_batch_device", "glmm_test_hooks",
    "GlmmFitPredictAggResult", "glmm_fit_predict_agg", "glmm_fit_predict_batch_host", "glmm_fit_predict_batch_device",
]


def version() -> str:
    return _abi.load().anofox_hip_version().decode()
