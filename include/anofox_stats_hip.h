/*
 * anofox_stats_hip.h — C ABI of libanofox_stats_hip.so, the MI355X (gfx950)
 * implementation of anofox-statistics' grouped least-squares path
 * (ols_fit_agg / ridge_fit_agg / wls_fit_agg).
 *
 * Two layers:
 *
 *  (1) The reference's own FFI surface for this path, same symbols, same
 *      struct layouts, same ownership and error conventions, so that the
 *      DuckDB C++ layer (src/aggregate_functions/{ols,ridge,wls}_aggregate.cpp,
 *      src/table_functions/{ols,ridge,wls}_fit.cpp, ...) links against this
 *      library instead of the Rust staticlib without source changes.
 *      Each declaration cites the reference interface it replaces
 *      (paths under the reference repository).
 *
 *  (2) New batched entry points (no reference counterpart): one call fits
 *      every group of an aggregate Finalize vector — or a whole GROUP BY —
 *      on the GPU.  Plain pointers and sizes only; no HIP, torch or C++ types.
 *
 * All arithmetic is IEEE-754 binary64.  Every entry point runs on the GPU;
 * there is no CPU fallback: without a usable HIP device the calls fail with
 * ANOFOX_ERROR_INTERNAL and a message.
 */
#ifndef ANOFOX_STATS_HIP_H
#define ANOFOX_STATS_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* exported symbols (the library is built with -fvisibility=hidden) */
#if defined(__GNUC__)
#define ANOFOX_HIP_API __attribute__((visibility("default")))
#else
#define ANOFOX_HIP_API
#endif

/* ------------------------------------------------------------------------ */
/* (1) Reference-compatible types.  Skipped when the reference's own header */
/* (src/include/anofox_stats_ffi.h) was included first.                     */
/* ------------------------------------------------------------------------ */
#ifndef ANOFOX_STATS_FFI_H

/* replaces AnofoxErrorCode, src/include/anofox_stats_ffi.h:18-31
 * (Rust mirror: crates/anofox-stats-ffi/src/types.rs:6-21) */
typedef enum {
	ANOFOX_ERROR_SUCCESS = 0,
	ANOFOX_ERROR_INVALID_INPUT = 1,
	ANOFOX_ERROR_SINGULAR_MATRIX = 2,
	ANOFOX_ERROR_CONVERGENCE_FAILURE = 3,
	ANOFOX_ERROR_INVALID_ALPHA = 4,
	ANOFOX_ERROR_INVALID_L1_RATIO = 5,
	ANOFOX_ERROR_INSUFFICIENT_DATA = 6,
	ANOFOX_ERROR_ALLOCATION_FAILURE = 7,
	ANOFOX_ERROR_SERIALIZATION_ERROR = 8,
	ANOFOX_ERROR_DIMENSION_MISMATCH = 9,
	ANOFOX_ERROR_NO_VALID_DATA = 10,
	ANOFOX_ERROR_INTERNAL = 99
} AnofoxErrorCode;

/* replaces AnofoxError, anofox_stats_ffi.h:36-39 — 260 bytes, message NUL-terminated, <= 255 chars */
typedef struct {
	AnofoxErrorCode code;
	char message[256];
} AnofoxError;

/* replaces AnofoxDataArray, anofox_stats_ffi.h:44-51 — 24 bytes, passed by value.
 * validity: LSB-first bitmask, bit i == 0 means NULL (treated as NaN, types.rs:66-89); may be NULL. */
typedef struct {
	const double *data;
	const uint8_t *validity;
	size_t len;
} AnofoxDataArray;

/* replaces AnofoxFitResultCore, anofox_stats_ffi.h:56-73 — 64 bytes */
typedef struct {
	double *coefficients; /* malloc'ed by the callee, released by anofox_free_result_core */
	size_t coefficients_len;
	double intercept; /* NaN when fit_intercept == false */
	double r_squared;
	double adj_r_squared;
	double residual_std_error;
	size_t n_observations;
	size_t n_features;
} AnofoxFitResultCore;

/* replaces AnofoxFitResultInference, anofox_stats_ffi.h:78-97 — 72 bytes; arrays are slopes only */
typedef struct {
	double *std_errors;
	double *t_values;
	double *p_values;
	double *ci_lower;
	double *ci_upper;
	size_t len;
	double confidence_level;
	double f_statistic;
	double f_pvalue;
} AnofoxFitResultInference;

/* replaces AnofoxSolverType, anofox_stats_ffi.h:102-106.  Accepted for API
 * compatibility; the GPU path always factors the shifted normal equations by
 * Cholesky (the reference's solvers agree to 1e-10 on well-conditioned data,
 * test/sql/regression/test_map_options.test:65-79). */
typedef enum { ANOFOX_SOLVER_QR = 0, ANOFOX_SOLVER_SVD = 1, ANOFOX_SOLVER_CHOLESKY = 2 } AnofoxSolverType;

/* replaces AnofoxLambdaScaling, anofox_stats_ffi.h:111-114 */
typedef enum { ANOFOX_LAMBDA_SCALING_RAW = 0, ANOFOX_LAMBDA_SCALING_GLMNET = 1 } AnofoxLambdaScaling;

/* replaces AnofoxHcType, anofox_stats_ffi.h:119-125 */
typedef enum {
	ANOFOX_HC_NONE = 0,
	ANOFOX_HC_HC0 = 1,
	ANOFOX_HC_HC1 = 2,
	ANOFOX_HC_HC2 = 3,
	ANOFOX_HC_HC3 = 4
} AnofoxHcType;

/* replaces AnofoxOlsOptions, anofox_stats_ffi.h:130-141 — 24 bytes */
typedef struct {
	bool fit_intercept;
	bool compute_inference;
	double confidence_level;
	AnofoxSolverType solver;
	AnofoxHcType hc_type;
} AnofoxOlsOptions;

/* replaces AnofoxRidgeOptions, anofox_stats_ffi.h:352-364 — 32 bytes */
typedef struct {
	double alpha;
	bool fit_intercept;
	bool compute_inference;
	double confidence_level;
	AnofoxSolverType solver;
	AnofoxLambdaScaling lambda_scaling;
} AnofoxRidgeOptions;

/* replaces AnofoxWlsOptions, anofox_stats_ffi.h:446-457 — 24 bytes */
typedef struct {
	bool fit_intercept;
	bool compute_inference;
	double confidence_level;
	AnofoxSolverType solver;
	AnofoxHcType hc_type;
} AnofoxWlsOptions;

/* replaces anofox_ols_fit, anofox_stats_ffi.h:155-156 (Rust: crates/anofox-stats-ffi/src/lib.rs:98-265).
 * One group, column-major x (one AnofoxDataArray per feature).  Returns false and fills *out_error on
 * failure, handing out no allocation.  out_inference may be NULL; when it is not and the fit produced
 * no inference block it is reset to {NULLs, len 0, NaNs} (types.rs:151-165). */
ANOFOX_HIP_API bool anofox_ols_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxOlsOptions options,
                    AnofoxFitResultCore *out_core, AnofoxFitResultInference *out_inference, AnofoxError *out_error);

/* replaces anofox_ridge_fit, anofox_stats_ffi.h:378-379 (lib.rs:984-1155) */
ANOFOX_HIP_API bool anofox_ridge_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxRidgeOptions options,
                      AnofoxFitResultCore *out_core, AnofoxFitResultInference *out_inference, AnofoxError *out_error);

/* replaces anofox_wls_fit, anofox_stats_ffi.h:472-474 (lib.rs:1384-1555) */
ANOFOX_HIP_API bool anofox_wls_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxDataArray weights,
                    AnofoxWlsOptions options, AnofoxFitResultCore *out_core, AnofoxFitResultInference *out_inference,
                    AnofoxError *out_error);

/* replaces anofox_free_result_core, anofox_stats_ffi.h:161 (lib.rs:272-280) — NULL-safe, idempotent */
ANOFOX_HIP_API void anofox_free_result_core(AnofoxFitResultCore *result);

/* replaces anofox_free_result_inference, anofox_stats_ffi.h:166 (lib.rs:287-311) */
ANOFOX_HIP_API void anofox_free_result_inference(AnofoxFitResultInference *result);

/* replaces anofox_compute_aic / anofox_compute_bic, anofox_stats_ffi.h:570,582 (lib.rs:1932-2011):
 * n ln(rss/n) + 2k  and  n ln(rss/n) + k ln n;  rss == 0 -> -inf;  n == 0 or rss < 0 -> InvalidInput.
 * Scalar helpers, evaluated on the host (they touch no data). */
ANOFOX_HIP_API bool anofox_compute_aic(double rss, size_t n, size_t k, double *out_aic, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_compute_bic(double rss, size_t n, size_t k, double *out_bic, AnofoxError *out_error);

/* ---- prediction helpers of the fit-predict family ---- */

/* replaces anofox_t_critical, anofox_stats_ffi.h:655 (lib.rs:2217-2231): Student-t quantile at (1 + c)/2;
 * NaN when df == 0 or c is outside (0, 1).  Scalar helper, evaluated on the host. */
ANOFOX_HIP_API double anofox_t_critical(double confidence_level, size_t df);

/* replaces AnofoxPredictionResult, anofox_stats_ffi.h:660-667 */
typedef struct {
	double yhat;
	double yhat_lower;
	double yhat_upper;
} AnofoxPredictionResult;

/* replaces anofox_predict_with_interval, anofox_stats_ffi.h:686-688 (lib.rs:2264-2349): one new observation,
 * simplified interval yhat -/+ t * rse * sqrt(1 + 1/n); NaN coefficients are skipped; bounds = yhat when no
 * interval can be formed.  Scalar helper, evaluated on the host. */
ANOFOX_HIP_API bool anofox_predict_with_interval(const double *coefficients, size_t coefficients_len, double intercept,
                                  const double *x_new, size_t x_len, double residual_std_error, size_t n_observations,
                                  double confidence_level, AnofoxPredictionResult *out_result);

/* replaces anofox_predict / anofox_free_predictions, anofox_stats_ffi.h:489-495 (lib.rs:1568-1664,
 * crates/anofox-stats-core/src/models/predict.rs:17-64): y = intercept (0 when NaN) + sum_j coef_j x_j for every row
 * (NaN coefficients propagate, as upstream).  Runs on the GPU; *out_predictions is malloc'ed. */
ANOFOX_HIP_API bool anofox_predict(const AnofoxDataArray *x, size_t x_count, const double *coefficients, size_t coefficients_len,
                    double intercept, double **out_predictions, size_t *out_predictions_len, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_predictions(double *predictions);

/* replaces anofox_compute_vif / anofox_free_vif, anofox_stats_ffi.h:516-522 (lib.rs:1688-1750 over
 * crates/anofox-stats-core/src/diagnostics/vif.rs:23-98): feature j regressed on all the others by OLS with an
 * intercept, VIF_j = 1 / (1 - R^2_j); inf when that fit fails or R^2 >= 0.9999, 1 when R^2 < 0; a single feature
 * gives {1.0}.  Runs on the GPU (one Gram matrix for all p regressions); *out_vif is malloc'ed. */
ANOFOX_HIP_API bool anofox_compute_vif(const AnofoxDataArray *x, size_t x_count, double **out_vif, size_t *out_vif_len,
                        AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_vif(double *vif);

/* replaces AnofoxResidualsResult / anofox_compute_residuals / anofox_free_residuals, anofox_stats_ffi.h:527-558
 * (lib.rs:1752-1920 over crates/anofox-stats-core/src/diagnostics/residuals.rs:30-145): raw = y - y_hat;
 * standardized = raw / s when residual_std_error s is not NaN; with x and include_studentized the leverage
 * h_i = x~_i' (X~'X~)^-1 x~_i of the intercept-augmented design and studentized = raw / (s sqrt(max(1 - h, 1e-10))).
 * A rank-deficient design yields no leverage (has_leverage = false).  Runs on the GPU; x_count <= 32. */
typedef struct {
	double *raw;
	double *standardized;
	double *studentized;
	double *leverage;
	size_t len;
	bool has_standardized;
	bool has_studentized;
	bool has_leverage;
} AnofoxResidualsResult;
ANOFOX_HIP_API bool anofox_compute_residuals(AnofoxDataArray y, AnofoxDataArray y_hat, const AnofoxDataArray *x, size_t x_count,
                              double residual_std_error, bool include_studentized, AnofoxResidualsResult *out_result,
                              AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_residuals(AnofoxResidualsResult *result);

/* replaces AnofoxElasticNetOptions, anofox_stats_ffi.h:384-397 — 40 bytes: alpha @0, l1_ratio @8, fit_intercept @16,
 * max_iterations @20, tolerance @24, lambda_scaling @32 */
typedef struct {
	double alpha;        /* penalty strength, >= 0 */
	double l1_ratio;     /* share of the L1 part in [0, 1]: 0 = ridge, 1 = lasso */
	bool fit_intercept;
	uint32_t max_iterations; /* coordinate-descent sweeps at most */
	double tolerance;    /* a sweep that moves no coefficient by more than tolerance sqrt(S_yy / C_jj) ends the solve */
	AnofoxLambdaScaling lambda_scaling;
} AnofoxElasticNetOptions;

/* replaces anofox_elasticnet_fit, anofox_stats_ffi.h:410-411 (over crates/anofox-stats-core/src/models/elasticnet.rs):
 * one group through anofox_hip_elasticnet_fit_batch_host, with anofox_ols_fit's conventions.  The objective, the solve
 * and the statuses: DESIGN.md §1 "Elastic net".  No inference block (the reference has none either). */
ANOFOX_HIP_API bool anofox_elasticnet_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxElasticNetOptions options,
                           AnofoxFitResultCore *out_core, AnofoxError *out_error);

/* replaces AnofoxRlsOptions, anofox_stats_ffi.h:593-600 — 24 bytes: forgetting_factor @0, fit_intercept @8,
 * initial_p_diagonal @16 */
typedef struct {
	double forgetting_factor;  /* lambda in (0, 1]; 1 = no forgetting */
	bool fit_intercept;
	double initial_p_diagonal; /* P = initial_p_diagonal I before the first row, > 0 */
} AnofoxRlsOptions;

/* replaces anofox_rls_fit, anofox_stats_ffi.h:611-612 (over crates/anofox-stats-core/src/models/rls.rs): one group through
 * anofox_hip_rls_fit_batch_host, with anofox_elasticnet_fit's conventions.  The filter and the statuses: DESIGN.md §1
 * "Recursive least squares".  r_squared, adj_r_squared and residual_std_error are NaN, as the reference's. */
ANOFOX_HIP_API bool anofox_rls_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxRlsOptions options,
                    AnofoxFitResultCore *out_core, AnofoxError *out_error);

/* replaces AnofoxBlsOptions, anofox_stats_ffi.h:1186-1201 — 56 bytes: fit_intercept @0, lower_bounds @8, lower_bounds_len @16,
 * upper_bounds @24, upper_bounds_len @32, max_iterations @40, tolerance @48 */
typedef struct {
	bool fit_intercept;
	const double *lower_bounds; /* NULL = no lower bounds, one value = every column */
	size_t lower_bounds_len;    /* 0, 1 or the number of features */
	const double *upper_bounds;
	size_t upper_bounds_len;
	uint32_t max_iterations;    /* outer active-set iterations at most */
	double tolerance;           /* |b_j - bound_j| < tolerance sets the bound flags */
} AnofoxBlsOptions;

/* replaces AnofoxBlsFitResultCore, anofox_stats_ffi.h:1206-1227 — 80 bytes: coefficients @0, coefficients_len @8,
 * intercept @16, ssr @24, r_squared @32, n_observations @40, n_features @48, n_active_constraints @56,
 * at_lower_bound @64, at_upper_bound @72 */
typedef struct {
	double *coefficients;
	size_t coefficients_len;
	double intercept; /* NaN without an intercept */
	double ssr;
	double r_squared;
	size_t n_observations;
	size_t n_features;
	size_t n_active_constraints;
	bool *at_lower_bound;
	bool *at_upper_bound;
} AnofoxBlsFitResultCore;

/* replace anofox_bls_fit / anofox_nnls_fit / anofox_free_bls_result, anofox_stats_ffi.h:1242-1263 (over
 * crates/anofox-stats-core/src/models/bls.rs): one group through anofox_hip_bls_fit_batch_host, with anofox_elasticnet_fit's
 * conventions.  Both bound arrays absent = NNLS; anofox_nnls_fit is that without an intercept, 1000 iterations, tolerance
 * 1e-10.  The minimiser, the flags and the statuses: DESIGN.md §1 "Bounded least squares".  The three arrays are malloc'ed;
 * anofox_free_bls_result frees and nulls them (NULL-safe). */
ANOFOX_HIP_API bool anofox_bls_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxBlsOptions options,
                    AnofoxBlsFitResultCore *out_core, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_nnls_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxBlsFitResultCore *out_core,
                     AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_bls_result(AnofoxBlsFitResultCore *result);

/* replaces AnofoxQuantileOptions, anofox_stats_ffi.h:1371-1380 — 24 bytes: tau @0, fit_intercept @8, max_iterations @12,
 * tolerance @16 */
typedef struct {
	double tau;              /* the quantile, in (0, 1) */
	bool fit_intercept;
	uint32_t max_iterations; /* simplex pivots at most */
	double tolerance;        /* accepted and unused: the result is the exact vertex */
} AnofoxQuantileOptions;

/* replaces AnofoxQuantileFitResultCore, anofox_stats_ffi.h:1385-1398 — 48 bytes: coefficients @0, coefficients_len @8,
 * intercept @16, tau @24, n_observations @32, n_features @40 */
typedef struct {
	double *coefficients;
	size_t coefficients_len;
	double intercept; /* NaN without an intercept */
	double tau;
	size_t n_observations;
	size_t n_features;
} AnofoxQuantileFitResultCore;

/* replace anofox_quantile_fit / anofox_free_quantile_result, anofox_stats_ffi.h:1411-1417 (over
 * crates/anofox-stats-core/src/models/quantile.rs): one group through anofox_hip_quantile_fit_batch_host, with
 * anofox_elasticnet_fit's conventions.  tau outside (0, 1) or NaN: false with ANOFOX_ERROR_INVALID_INPUT.  The minimiser and
 * the statuses: DESIGN.md §1 "Quantile regression" (fit_intercept = false really fits without an intercept).  The
 * coefficients are malloc'ed; anofox_free_quantile_result frees and nulls them (NULL-safe). */
ANOFOX_HIP_API bool anofox_quantile_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxQuantileOptions options,
                         AnofoxQuantileFitResultCore *out_core, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_quantile_result(AnofoxQuantileFitResultCore *result);
/* anofox_quantile_fit at every tau of a grid from one fit (the tau path below): out_results[t] (n_taus of them, the caller's
 * array) is the result at taus[t], each freed by anofox_free_quantile_result.  options.tau is ignored.  1 <= n_taus <= 64; a
 * tau outside (0, 1) or NaN fails the call with ANOFOX_ERROR_INVALID_INPUT; after a failure no result holds memory. */
ANOFOX_HIP_API bool anofox_quantile_fit_path(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxQuantileOptions options,
                              const double *taus, size_t n_taus, AnofoxQuantileFitResultCore *out_results, AnofoxError *out_error);

/* replace AnofoxPoissonLink / AnofoxBinomialLink, anofox_stats_ffi.h:697-710.  Only the canonical links (0) are built. */
typedef enum { ANOFOX_POISSON_LINK_LOG = 0, ANOFOX_POISSON_LINK_IDENTITY = 1, ANOFOX_POISSON_LINK_SQRT = 2 } AnofoxPoissonLink;
typedef enum { ANOFOX_BINOMIAL_LINK_LOGIT = 0, ANOFOX_BINOMIAL_LINK_PROBIT = 1, ANOFOX_BINOMIAL_LINK_CLOGLOG = 2 } AnofoxBinomialLink;

/* replaces AnofoxGlmFitResultCore, anofox_stats_ffi.h:715-741 — 88 bytes: coefficients @0, coefficients_len @8, intercept @16,
 * deviance @24, null_deviance @32, pseudo_r_squared @40, aic @48, dispersion @56, n_observations @64, n_features @72,
 * iterations @80, converged @84 */
typedef struct {
	double *coefficients; /* malloc'ed by the callee, released by anofox_free_glm_result */
	size_t coefficients_len;
	double intercept; /* NaN without an intercept */
	double deviance;
	double null_deviance;
	double pseudo_r_squared;
	double aic;
	double dispersion;
	size_t n_observations;
	size_t n_features;
	uint32_t iterations;
	bool converged;
} AnofoxGlmFitResultCore;

/* replace AnofoxPriorKind / AnofoxPriorSpec / AnofoxVcovType, anofox_stats_ffi.h:759-791.  Priors are not built: a non-NULL
 * priors pointer fails the call; only ANOFOX_VCOV_LAPLACE is built. */
typedef enum { ANOFOX_PRIOR_FLAT = 0, ANOFOX_PRIOR_NORMAL = 1, ANOFOX_PRIOR_LAPLACE = 2 } AnofoxPriorKind;
typedef struct {
	AnofoxPriorKind kind;
	double loc;
	double scale;
} AnofoxPriorSpec;
typedef enum { ANOFOX_VCOV_LAPLACE = 0, ANOFOX_VCOV_SANDWICH = 1, ANOFOX_VCOV_NAIVE = 2 } AnofoxVcovType;

/* replaces AnofoxPoissonOptions, anofox_stats_ffi.h:796-819 — 80 bytes: fit_intercept @0, link @4, max_iterations @8,
 * tolerance @16, compute_inference @24, confidence_level @32, lambda @40, priors @48, priors_len @56, vcov @64,
 * offset_column @72 (1-based index into x of the offset column, 0 = none) */
typedef struct {
	bool fit_intercept;
	AnofoxPoissonLink link;
	uint32_t max_iterations;
	double tolerance;
	bool compute_inference;
	double confidence_level;
	double lambda;
	const AnofoxPriorSpec *priors;
	size_t priors_len;
	AnofoxVcovType vcov;
	size_t offset_column;
} AnofoxPoissonOptions;

/* replaces AnofoxBinomialOptions, anofox_stats_ffi.h:824-847 — the layout of AnofoxPoissonOptions with the binomial link */
typedef struct {
	bool fit_intercept;
	AnofoxBinomialLink link;
	uint32_t max_iterations;
	double tolerance;
	bool compute_inference;
	double confidence_level;
	double lambda;
	const AnofoxPriorSpec *priors;
	size_t priors_len;
	AnofoxVcovType vcov;
	size_t offset_column;
} AnofoxBinomialOptions;

/* replaces AnofoxLogisticOptions, anofox_stats_ffi.h:1008-1026 — 80 bytes: fit_intercept @0, compute_inference @1,
 * confidence_level @8, lambda @16, threshold @24, max_iterations @32, tolerance @40, priors @48, priors_len @56, vcov @64,
 * offset_column @72 */
typedef struct {
	bool fit_intercept;
	bool compute_inference;
	double confidence_level;
	double lambda;
	double threshold; /* the classification threshold on P(y = 1), in [0, 1] */
	uint32_t max_iterations;
	double tolerance;
	const AnofoxPriorSpec *priors;
	size_t priors_len;
	AnofoxVcovType vcov;
	size_t offset_column;
} AnofoxLogisticOptions;

/* replaces AnofoxLogisticFitExtras, anofox_stats_ffi.h:1032-1037: the share of the fitted rows with [mu >= threshold] == y,
 * and the threshold echoed */
typedef struct {
	double accuracy;
	double threshold;
} AnofoxLogisticFitExtras;

/* replace anofox_poisson_fit / anofox_binomial_fit / anofox_logistic_fit / anofox_free_glm_result, anofox_stats_ffi.h:953-1059
 * (over crates/anofox-stats-core/src/models/glm.rs and glm_engine/): one group through anofox_hip_glm_fit_batch_host below,
 * with anofox_ols_fit's conventions.  offset_column is split out of x on the host (design.rs:186-202).  A link other than
 * log / logit, non-NULL priors or a vcov other than Laplace: false with ANOFOX_ERROR_INVALID_INPUT and "glm: ... is not
 * built".  anofox_logistic_fit wants y in {0, 1} and threshold in [0, 1].  The contract: DESIGN.md §1 "Generalised linear
 * models".  out_inference (may be NULL) gets z values in t_values and NaN in f_statistic / f_pvalue.  A call that fails leaves
 * out_core zeroed (NaN in its doubles), out_inference reset to {NULLs, len 0, NaNs} and out_extras NaN: nothing to free. */
ANOFOX_HIP_API bool anofox_poisson_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxPoissonOptions options,
                        AnofoxGlmFitResultCore *out_core, AnofoxFitResultInference *out_inference, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_binomial_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxBinomialOptions options,
                         AnofoxGlmFitResultCore *out_core, AnofoxFitResultInference *out_inference, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_logistic_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxLogisticOptions options,
                         AnofoxGlmFitResultCore *out_result, AnofoxFitResultInference *out_inference,
                         AnofoxLogisticFitExtras *out_extras, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_glm_result(AnofoxGlmFitResultCore *result);

/* replaces AnofoxAftDistribution, anofox_stats_ffi.h:2293-2299: the distribution of T; exponential is Weibull with scale 1 */
typedef enum {
	ANOFOX_AFT_WEIBULL = 0,
	ANOFOX_AFT_LOGNORMAL = 1,
	ANOFOX_AFT_LOGLOGISTIC = 2,
	ANOFOX_AFT_EXPONENTIAL = 3
} AnofoxAftDistribution;

/* replaces AnofoxAftOptions, anofox_stats_ffi.h:2304-2315 — 64 bytes: dist @0, fit_intercept @4, max_iterations @8,
 * tolerance @16, compute_inference @24, confidence_level @32, priors @40, priors_len @48, vcov @56 */
typedef struct {
	AnofoxAftDistribution dist;
	bool fit_intercept;
	uint32_t max_iterations;
	double tolerance;
	bool compute_inference;
	double confidence_level;
	const AnofoxPriorSpec *priors; /* not built: has to be NULL */
	size_t priors_len;
	AnofoxVcovType vcov; /* every value gives the same covariance without priors */
} AnofoxAftOptions;

/* replaces AnofoxAftFitResultCore, anofox_stats_ffi.h:2320-2337 — 104 bytes: coefficients @0, coefficients_len @8, intercept @16,
 * scale @24, log_likelihood @32, null_log_likelihood @40, aic @48, bic @56, n_observations @64, n_events @72, n_censored @80,
 * n_features @88, iterations @96, converged @100 */
typedef struct {
	double *coefficients; /* on the log-time scale; malloc'ed by the callee, released by anofox_free_aft_result */
	size_t coefficients_len;
	double intercept; /* NaN without an intercept */
	double scale;     /* sigma; exactly 1.0 for the exponential distribution */
	double log_likelihood;
	double null_log_likelihood; /* of the intercept-only model; NaN without an intercept */
	double aic;
	double bic;
	size_t n_observations;
	size_t n_events;
	size_t n_censored;
	size_t n_features;
	uint32_t iterations;
	bool converged;
} AnofoxAftFitResultCore;

/* replaces AnofoxAftInference, anofox_stats_ffi.h:2342-2354 — 72 bytes: five arrays @0..32, len @40, confidence_level @48,
 * intercept_std_error @56, log_scale_std_error @64 */
typedef struct {
	double *std_errors; /* the five arrays: one entry per feature, released by anofox_free_aft_inference */
	double *z_values;
	double *p_values;
	double *ci_lower;
	double *ci_upper;
	size_t len;
	double confidence_level;
	double intercept_std_error; /* NaN without an intercept */
	double log_scale_std_error; /* NaN when the scale is fixed */
} AnofoxAftInference;

/* replace anofox_aft_fit / anofox_free_aft_result / anofox_free_aft_inference / anofox_aft_cdf / anofox_aft_quantile,
 * anofox_stats_ffi.h:2356-2383 (over crates/anofox-stats-core/src/models/aft.rs and aft_dist.rs): one group through
 * anofox_hip_aft_fit_batch_host below, with anofox_ols_fit's conventions.  event: 1 = observed, 0 = right-censored.  Non-NULL
 * priors: false with ANOFOX_ERROR_INVALID_INPUT and "aft: priors are not built"; more than 32 features: "aft: n_features > 32
 * is not built"; a tolerance that is not finite and positive, max_iterations = 0, an unknown dist, or a confidence_level outside
 * (0, 1) with inference: "aft: invalid options"; all three before any device is touched.  A group status other than 0 is false
 * with that status as the error code.  The contract: DESIGN.md §1 "Accelerated failure time models".  A call that fails leaves
 * out_core zeroed (NaN in its doubles) and out_inference reset to {NULLs, len 0, NaNs}: nothing to free.
 * anofox_aft_cdf: P(T <= t) at the linear predictor eta and the scale, 0 for t <= 0.  anofox_aft_quantile: the p-quantile of T,
 * p clamped to [1e-12, 1 - 1e-12].  Plain host functions. */
ANOFOX_HIP_API bool anofox_aft_fit(AnofoxDataArray time, const AnofoxDataArray *x, size_t x_count, AnofoxDataArray event,
                    AnofoxAftOptions options, AnofoxAftFitResultCore *out_core, AnofoxAftInference *out_inference,
                    AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_aft_result(AnofoxAftFitResultCore *result);
ANOFOX_HIP_API void anofox_free_aft_inference(AnofoxAftInference *inf);
ANOFOX_HIP_API double anofox_aft_cdf(double t, double eta, double scale, AnofoxAftDistribution dist);
ANOFOX_HIP_API double anofox_aft_quantile(double p, double eta, double scale, AnofoxAftDistribution dist);

/* replaces AnofoxTauMethod, anofox_stats_ffi.h:2390-2394 */
typedef enum { ANOFOX_TAU_DERSIMONIAN_LAIRD = 0, ANOFOX_TAU_NONE = 1 } AnofoxTauMethod;

/* replaces AnofoxEbShrinkOptions, anofox_stats_ffi.h:2396-2400 — 16 bytes: method @0, tau_squared @8 */
typedef struct {
	AnofoxTauMethod method;
	double tau_squared; /* NaN: estimate it */
} AnofoxEbShrinkOptions;

/* replaces AnofoxEbShrinkResult, anofox_stats_ffi.h:2405-2418 — 96 bytes: five doubles @0..32, n_groups @40, five arrays
 * @48..80 (each `len` long, in input order, malloc'ed by the callee, released by anofox_free_eb_shrink_result), len @88 */
typedef struct {
	double mu;
	double mu_se;
	double tau_squared;
	double i_squared;
	double q;
	size_t n_groups;
	double *estimate;
	double *se;
	double *shrunken;
	double *shrunken_se;
	double *weight;
	size_t len;
} AnofoxEbShrinkResult;

/* replace anofox_eb_shrink / anofox_free_eb_shrink_result, anofox_stats_ffi.h:2423-2427: one set through
 * anofox_hip_eb_shrink_batch_host (below), NULL entries of the validity bitmaps as NaN (pairs that are not usable).  False, with the
 * result zeroed and nothing to free: an empty input (ANOFOX_ERROR_INVALID_INPUT), unequal lengths
 * (ANOFOX_ERROR_DIMENSION_MISMATCH), a fixed tau_squared that is negative or infinite (ANOFOX_ERROR_INVALID_INPUT), the first
 * three before any device is touched, and fewer than 2 usable pairs (ANOFOX_ERROR_INSUFFICIENT_DATA). */
ANOFOX_HIP_API bool anofox_eb_shrink(AnofoxDataArray estimate, AnofoxDataArray se, AnofoxEbShrinkOptions options,
                      AnofoxEbShrinkResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_eb_shrink_result(AnofoxEbShrinkResult *result);

/* replace AnofoxAlternative and AnofoxKendallType, anofox_stats_ffi.h:1549-1553 and 1722-1726 */
typedef enum { ANOFOX_ALTERNATIVE_TWO_SIDED = 0, ANOFOX_ALTERNATIVE_LESS = 1, ANOFOX_ALTERNATIVE_GREATER = 2 } AnofoxAlternative;
typedef enum { ANOFOX_KENDALL_TAU_A = 0, ANOFOX_KENDALL_TAU_B = 1, ANOFOX_KENDALL_TAU_C = 2 } AnofoxKendallType;

/* replaces AnofoxCorrelationOptions, anofox_stats_ffi.h:1709-1714 — 16 bytes: alternative @0, confidence_level @8 */
typedef struct {
	AnofoxAlternative alternative;
	double confidence_level; /* in (0, 1); NaN: no interval */
} AnofoxCorrelationOptions;

/* replaces AnofoxKendallOptions, anofox_stats_ffi.h:1731-1738 — 16 bytes: alternative @0, tau_type @4, confidence_level @8 (not
 * read: Kendall's tau has no interval) */
typedef struct {
	AnofoxAlternative alternative;
	AnofoxKendallType tau_type;
	double confidence_level;
} AnofoxKendallOptions;

/* replaces AnofoxCorrelationResult, anofox_stats_ffi.h:1611-1628 — 64 bytes: six doubles @0..40, n @48, method @56 (malloc'ed by the
 * callee, released by anofox_free_correlation_result) */
typedef struct {
	double r; /* Kendall: tau */
	double statistic;
	double p_value;
	double ci_lower;
	double ci_upper;
	double confidence_level; /* Kendall: NaN */
	size_t n;
	char *method; /* "Pearson correlation", "Spearman rank correlation", "Kendall's TauA" / "TauB" / "TauC" */
} AnofoxCorrelationResult;

/* replace anofox_pearson_cor / anofox_spearman_cor / anofox_kendall_cor / anofox_free_correlation_result,
 * anofox_stats_ffi.h:1827-1840 and 2198: one group through anofox_hip_cor_batch_host (below), NULL entries of the validity
 * bitmaps as NaN (rows that are not valid).  False with ANOFOX_ERROR_INVALID_INPUT (the reference's code for every failure of
 * these three), the result zeroed and nothing to free, before any device is touched: out_result NULL, unequal lengths
 * ("<Name> correlation requires equal length vectors"), an unknown alternative or tau type or a confidence level outside (0, 1)
 * ("correlation: ..."), fewer than 3 valid pairs ("<Name> correlation requires at least 3 valid pairs"). */
ANOFOX_HIP_API bool anofox_pearson_cor(AnofoxDataArray x, AnofoxDataArray y, AnofoxCorrelationOptions options,
                        AnofoxCorrelationResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_spearman_cor(AnofoxDataArray x, AnofoxDataArray y, AnofoxCorrelationOptions options,
                         AnofoxCorrelationResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_kendall_cor(AnofoxDataArray x, AnofoxDataArray y, AnofoxKendallOptions options,
                        AnofoxCorrelationResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_correlation_result(AnofoxCorrelationResult *result);

/* replaces AnofoxTestResult, anofox_stats_ffi.h:1555-1583 — 96 bytes: seven doubles @0..48, n @56, n1 @64, n2 @72, alternative @80,
 * method @88 (malloc'ed by the callee, released by anofox_free_test_result) */
typedef struct {
	double statistic; /* W, V or H */
	double p_value;
	double df;          /* Kruskal-Wallis: k - 1; NaN otherwise */
	double effect_size; /* NaN, as in the reference */
	double ci_lower;    /* NaN: the Hodges-Lehmann interval is not built */
	double ci_upper;
	double confidence_level; /* the option, echoed (0.95 where it is not > 0); Kruskal-Wallis: NaN */
	size_t n;
	size_t n1;
	size_t n2;
	AnofoxAlternative alternative;
	char *method; /* "Mann-Whitney U test", "Wilcoxon signed-rank test", "Kruskal-Wallis H test" */
} AnofoxTestResult;

/* replaces AnofoxMannWhitneyOptions, anofox_stats_ffi.h:1696-1707 — 24 bytes: alternative @0, exact @4, continuity_correction @5,
 * confidence_level @8, mu @16 (NaN: 0) */
typedef struct {
	AnofoxAlternative alternative;
	bool exact; /* true fails: exact p-values are not built */
	bool continuity_correction;
	double confidence_level;
	double mu;
} AnofoxMannWhitneyOptions;

/* replaces AnofoxWilcoxonOptions, anofox_stats_ffi.h:1920-1931 — the same 24 bytes */
typedef struct {
	AnofoxAlternative alternative;
	bool exact;
	bool continuity_correction;
	double confidence_level;
	double mu;
} AnofoxWilcoxonOptions;

/* replace anofox_mann_whitney_u / anofox_kruskal_wallis / anofox_wilcoxon_signed_rank / anofox_free_test_result,
 * anofox_stats_ffi.h:1845, 1863, 1936 and 2188: one group through anofox_hip_rank_test_batch_host (below), NULL entries of the
 * validity bitmaps as NaN.  Kruskal-Wallis takes the group ids as doubles and, as the reference does, pairs values and ids up to
 * the shorter array, drops a pair with a NaN in either and keys the groups by the id cast to an integer (towards zero).
 * n / n1 / n2 follow the reference: Mann-Whitney n1 + n2, n1, n2; Wilcoxon the valid pairs three times; Kruskal-Wallis N, 0, 0.
 * False with ANOFOX_ERROR_INVALID_INPUT, the result zeroed and nothing to free, before any device is touched: out_result NULL,
 * exact = true ("<method>: exact p-values are not built"), an unknown alternative or a mu that is infinite ("rank test: ..."),
 * "Mann-Whitney U test requires at least 1 observation per group", "Wilcoxon signed-rank test requires equal length samples",
 * "Wilcoxon signed-rank test requires at least 2 valid pairs", "Kruskal-Wallis test requires at least 2 groups" and "... at least 3
 * observations" (the aggregate's rule). */
ANOFOX_HIP_API bool anofox_mann_whitney_u(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxMannWhitneyOptions options,
                           AnofoxTestResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_wilcoxon_signed_rank(AnofoxDataArray x, AnofoxDataArray y, AnofoxWilcoxonOptions options,
                                 AnofoxTestResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_kruskal_wallis(AnofoxDataArray values, AnofoxDataArray groups, AnofoxTestResult *out_result,
                           AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_test_result(AnofoxTestResult *result);

/* replaces AnofoxAnovaResult, anofox_stats_ffi.h:1588-1607 — 72 bytes: f_statistic @0, p_value @8, df_between @16, df_within @24,
 * ss_between @32, ss_within @40, n_groups @48, n @56, method @64 (malloc'ed by the callee, released by anofox_free_anova_result) */
typedef struct {
	double f_statistic;
	double p_value;
	size_t df_between;
	size_t df_within;
	double ss_between;
	double ss_within;
	size_t n_groups;
	size_t n;
	char *method; /* "Fisher One-way ANOVA" */
} AnofoxAnovaResult;

/* replaces AnofoxTTestOptions, anofox_stats_ffi.h:1682-1691 — 32 bytes: alternative @0, confidence_level @8, var_equal @16, mu @24
 * (NaN: 0) */
typedef struct {
	AnofoxAlternative alternative;
	double confidence_level;
	bool var_equal; /* true: Student's pooled variance; false: Welch */
	double mu;
} AnofoxTTestOptions;

/* replaces AnofoxBrunnerMunzelOptions, anofox_stats_ffi.h:1799-1804 — 16 bytes */
typedef struct {
	AnofoxAlternative alternative;
	double confidence_level;
} AnofoxBrunnerMunzelOptions;

/* replace anofox_t_test / anofox_brunner_munzel / anofox_one_way_anova / anofox_yuen_test / anofox_brown_forsythe /
 * anofox_free_anova_result, anofox_stats_ffi.h:1811, 1851, 1857, 2133, 2139 and the ANOVA result's release: one group through
 * anofox_hip_sample_test_batch_host (below), NULL entries of the validity bitmaps as NaN.  The two-sample scalars take group1 as
 * sample 1; the k-sample scalars take the group ids as doubles and pair, drop and key them as anofox_kruskal_wallis does.
 * AnofoxTestResult: statistic, p_value, df, the interval (Brown-Forsythe: NaN) and the confidence level echoed (Brown-Forsythe:
 * NaN); effect_size NaN but for Brunner-Munzel, whose it is phat; n = n1 + n2, n1, n2 (Brown-Forsythe: N, 0, 0); method
 * "Welch t-test" / "Student t-test", "Yuen test (trim=0.20)", "Brunner-Munzel test", "Brown-Forsythe test".
 * False with ANOFOX_ERROR_INVALID_INPUT, the result zeroed and nothing to free, before any device is touched: out_result NULL,
 * an option the batch entry refuses ("sample test: ..."), "t-test requires at least 2 observations in group 1" (or 2; Yuen test:
 * 4; Brunner-Munzel test: 2), "ANOVA requires at least 2 groups", "ANOVA requires at least 2 observations per group (group i has
 * m)" (i in the order of first appearance) and the same two for "Brown-Forsythe test". */
ANOFOX_HIP_API bool anofox_t_test(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxTTestOptions options, AnofoxTestResult *out_result,
                   AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_brunner_munzel(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxBrunnerMunzelOptions options,
                           AnofoxTestResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_one_way_anova(AnofoxDataArray values, AnofoxDataArray groups, AnofoxAnovaResult *out_result,
                          AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_yuen_test(AnofoxDataArray group1, AnofoxDataArray group2, double trim, AnofoxAlternative alternative,
                      double confidence_level, AnofoxTestResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_brown_forsythe(AnofoxDataArray values, AnofoxDataArray groups, AnofoxTestResult *out_result,
                           AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_anova_result(AnofoxAnovaResult *result);

/* replaces AnofoxJarqueBeraResult, anofox_stats_ffi.h:621-632 — 40 bytes: four doubles @0..24, n @32; nothing to free */
typedef struct {
	double statistic;
	double p_value;
	double skewness;
	double kurtosis; /* excess */
	size_t n;
} AnofoxJarqueBeraResult;

/* replace anofox_shapiro_wilk / anofox_dagostino_k2 / anofox_jarque_bera, anofox_stats_ffi.h:1817, 1822 and 642: one group through
 * anofox_hip_normality_test_batch_host (below), NULL entries of the validity bitmap as NaN (rows that are not valid).
 * AnofoxTestResult: statistic (W or K2), p_value, df NaN (K2: 2.0), effect_size, the interval and the confidence level NaN,
 * n the valid rows, n1 = n2 = 0, alternative two-sided, method "Shapiro-Wilk test" / "D'Agostino K-squared test" (released by
 * anofox_free_test_result).
 * False, the result zeroed and nothing to free: out_result NULL (ANOFOX_ERROR_INVALID_INPUT); before any device is touched
 * "Shapiro-Wilk test requires at least 3 observations", "D'Agostino K-squared test requires at least 8 observations",
 * "Jarque-Bera test requires at least 3 observations" (ANOFOX_ERROR_INSUFFICIENT_DATA) and "Shapiro-Wilk test is limited to
 * n <= 5000" (ANOFOX_ERROR_INVALID_INPUT); "Data has zero variance" (ANOFOX_ERROR_INVALID_INPUT) for K2 and Jarque-Bera of
 * values that are all equal.  Constant data gives Shapiro-Wilk W = 1 and p = 1. */
ANOFOX_HIP_API bool anofox_shapiro_wilk(AnofoxDataArray data, AnofoxTestResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_dagostino_k2(AnofoxDataArray data, AnofoxTestResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_jarque_bera(AnofoxDataArray data, AnofoxJarqueBeraResult *out_result, AnofoxError *out_error);

/* replaces AnofoxChiSquareResult, anofox_stats_ffi.h:1634-1643 — 32 bytes: statistic @0, p_value @8, df @16, method @24 (malloc'ed
 * by the callee, released by anofox_free_chisq_result) */
typedef struct {
	double statistic;
	double p_value;
	size_t df;
	char *method;
} AnofoxChiSquareResult;

/* replaces AnofoxChiSquareOptions, anofox_stats_ffi.h:1743-1746 — 1 byte */
typedef struct {
	bool correction; /* Yates' correction on a 2 x 2 table */
} AnofoxChiSquareOptions;

/* replaces AnofoxFisherExactOptions, anofox_stats_ffi.h:1751-1756 — 16 bytes: alternative @0, confidence_level @8 */
typedef struct {
	AnofoxAlternative alternative;
	double confidence_level; /* in (0, 1); NaN: no interval */
} AnofoxFisherExactOptions;

/* replace anofox_chisq_test, anofox_fisher_exact, anofox_cramers_v, anofox_g_test, anofox_mcnemar_test, anofox_phi_coefficient,
 * anofox_contingency_coef and anofox_free_chisq_result, anofox_stats_ffi.h:1869, 1875, 2009, 2022, 2029, 2036, 2041 and 2203.  The
 * definitions: the grouped categorical tests below, DESIGN.md §1 "Categorical tests".
 * anofox_chisq_test: rows where either entry is NaN or not valid are dropped, the labels are cast as `value as usize` casts them
 * (toward zero, negative values to 0), and the group goes through anofox_hip_categorical_test_batch_host; the table is that of the
 * labels that occur (the reference sizes its table by the largest label).  method "Pearson's Chi-squared test".
 * The table-taking entries read a table flattened row by row, row i with row_lengths[i] cells; empty rows and columns are dropped.
 * They and the cell-taking entries ([[a, b], [c, d]]) touch no device.  anofox_fisher_exact: statistic = the sample odds ratio
 * a d/(b c), effect_size = the conditional maximum-likelihood odds ratio, ci_lower / ci_upper its exact interval at
 * options.confidence_level (one-sided for a one-sided alternative), df NaN, n = a + b + c + d, n1 = n2 = 0, method "Fisher's exact
 * test" (released by anofox_free_test_result).  anofox_mcnemar_test: df 1, or 0 with exact (the statistic is then NaN).
 * False, the result zeroed and nothing to free: out_result NULL, "Invalid table data" (a NULL table or no rows), a table with
 * fewer than 2 occupied rows or columns, an unknown alternative or a confidence level outside (0, 1) that is not NaN
 * (ANOFOX_ERROR_INVALID_INPUT); "No valid data pairs" and an all-zero 2 x 2 table (ANOFOX_ERROR_INSUFFICIENT_DATA). */
ANOFOX_HIP_API bool anofox_chisq_test(AnofoxDataArray row_var, AnofoxDataArray col_var, AnofoxChiSquareOptions options,
                       AnofoxChiSquareResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_fisher_exact(size_t a, size_t b, size_t c, size_t d, AnofoxFisherExactOptions options, AnofoxTestResult *out_result,
                         AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_cramers_v(const size_t *table, const size_t *row_lengths, size_t n_rows, double *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_g_test(const size_t *table, const size_t *row_lengths, size_t n_rows, AnofoxChiSquareResult *out_result,
                   AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_mcnemar_test(size_t a, size_t b, size_t c, size_t d, bool correction, bool exact, AnofoxChiSquareResult *out_result,
                         AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_phi_coefficient(size_t a, size_t b, size_t c, size_t d, double *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_contingency_coef(const size_t *table, const size_t *row_lengths, size_t n_rows, double *out_result,
                             AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_chisq_result(AnofoxChiSquareResult *result);

/* replaces AnofoxGlmmFamily, anofox_stats_ffi.h:2433-2440 */
typedef enum {
	ANOFOX_GLMM_GAUSSIAN = 0,
	ANOFOX_GLMM_POISSON = 1,
	ANOFOX_GLMM_BINOMIAL = 2,
	ANOFOX_GLMM_NEGBINOMIAL = 3,
	ANOFOX_GLMM_GAMMA = 4,
	ANOFOX_GLMM_TWEEDIE = 5
} AnofoxGlmmFamily;

/* replaces AnofoxGlmmOptions, anofox_stats_ffi.h:2442-2460 — 88 bytes: family @0, fit_intercept @4, max_iterations @8,
 * tolerance @16, compute_inference @24, confidence_level @32, reml @40, theta @48, power @56, offset_column @64 (1-based, 0:
 * none), random_slopes @72, random_slopes_len @80.  Only the Gaussian family without an offset and without random slopes is
 * built (DESIGN.md §1 "Linear mixed models"); theta and power are not read. */
typedef struct {
	AnofoxGlmmFamily family;
	bool fit_intercept;
	uint32_t max_iterations;
	double tolerance;
	bool compute_inference;
	double confidence_level;
	bool reml;
	double theta;
	double power;
	size_t offset_column;
	const size_t *random_slopes;
	size_t random_slopes_len;
} AnofoxGlmmOptions;

/* replaces AnofoxGlmmResult, anofox_stats_ffi.h:2462-2504 — 264 bytes.  coefficients (coefficients_len = n_features); the five
 * inference arrays (inference_len = n_features with compute_inference, else NULL and 0); per level, in first-seen order of the
 * caller's ids, ranef_group / ranef_value / ranef_se (NaN: not built) / ranef_n and ranef_effects (= ranef_value, random_dim =
 * 1); random_cov = {var_group}; factor_var and factor_n_levels NULL with factor_len 0.  Every array is malloc'ed by the callee
 * and released by anofox_free_glmm_result. */
typedef struct {
	double *coefficients;
	size_t coefficients_len;
	double intercept;
	double *std_errors;
	double *z_values;
	double *p_values;
	double *ci_lower;
	double *ci_upper;
	size_t inference_len;
	double intercept_std_error;
	double confidence_level;
	double var_group;
	double var_residual;
	double icc;
	double log_likelihood;
	double aic;
	double bic;
	double deviance;
	size_t n_observations;
	size_t n_groups;
	size_t n_features;
	uint32_t iterations;
	bool converged;
	int32_t *ranef_group;
	double *ranef_value;
	double *ranef_se;
	int64_t *ranef_n;
	size_t ranef_len;
	double *random_cov;
	size_t random_dim;
	double *ranef_effects;
	double *factor_var;
	int64_t *factor_n_levels;
	size_t factor_len;
} AnofoxGlmmResult;

/* replace anofox_glmm_fit / anofox_free_glmm_result, anofox_stats_ffi.h:2511-2516: one panel through
 * anofox_hip_glmm_fit_batch_host (below).  Rows are grouped by group_ids (ids < 0 are dropped, the others compacted in
 * first-seen order); NULL entries of the validity bitmaps are NaN (rows that are not valid).  False with the result zeroed and
 * nothing to free, before any device is touched: an empty y, unequal lengths, more than 32 features, invalid options, and
 * ANOFOX_ERROR_INVALID_INPUT with "glmm: ... is not built" for a family other than Gaussian, n_extra_factors > 0, a non-empty
 * random_slopes or an offset column.  A panel status other than 0 is false with that status as the error code. */
ANOFOX_HIP_API bool anofox_glmm_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, const int32_t *group_ids, size_t n_obs,
                     const int32_t *const *extra_group_ids, size_t n_extra_factors, AnofoxGlmmOptions options,
                     AnofoxGlmmResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_free_glmm_result(AnofoxGlmmResult *result);

/* replaces AnofoxEnergyDistanceOptions, anofox_stats_ffi.h:1761-1768 — 24 bytes: n_permutations @0, seed @8, has_seed @16 */
typedef struct {
	size_t n_permutations;
	uint64_t seed;
	bool has_seed; /* false: the seed is drawn from the host's entropy */
} AnofoxEnergyDistanceOptions;

/* replaces AnofoxMmdOptions, anofox_stats_ffi.h:1773-1780 — the same 24 bytes */
typedef struct {
	size_t n_permutations;
	uint64_t seed;
	bool has_seed;
} AnofoxMmdOptions;

/* replace anofox_energy_distance / anofox_mmd / anofox_permutation_t_test, anofox_stats_ffi.h:1881, 1887 and 2179: one group
 * (group1 as sample 1, NaN entries dropped) through anofox_hip_perm_test_batch_host (below); the result is released by
 * anofox_free_test_result.  method: "Energy distance test (B permutations)", "MMD test (Gaussian kernel, B permutations)",
 * "Permutation t-test (B permutations)".  effect_size is the statistic for the first two, as the reference's wrapper sets it; df is
 * Welch's df for the t-test (the reference leaves it NaN) and NaN otherwise; the interval and its level are NaN.  The statistics and
 * the permutation stream are this library's own: a p-value is not the reference's for the same seed.
 * False with ANOFOX_ERROR_INVALID_INPUT, the result zeroed and nothing to free, before any device is touched: out_result NULL, an
 * unknown alternative or n_permutations above 1000000 ("permutation test: ..."), "<test> requires at least 2 observations in group
 * 1" / "... group 2", "<test> is not defined on infinite values", and for MMD more than 1462 observations ("mmd: group too
 * large"). */
ANOFOX_HIP_API bool anofox_energy_distance(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxEnergyDistanceOptions options,
                            AnofoxTestResult *out_result, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_mmd(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxMmdOptions options, AnofoxTestResult *out_result,
                AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_permutation_t_test(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxAlternative alternative,
                               size_t n_permutations, uint64_t seed, bool has_seed, AnofoxTestResult *out_result,
                               AnofoxError *out_error);

#endif /* ANOFOX_STATS_FFI_H */

/* ------------------------------------------------------------------------ */
/* (2) Batched GPU entry points (new surface).                               */
/*                                                                          */
/* Natural call site in the reference: the per-state loop of                 */
/* OlsAggFinalize (src/aggregate_functions/ols_aggregate.cpp:249-338, and    */
/* ridge_aggregate.cpp:255-345, wls_aggregate.cpp:268-362), which today      */
/* makes one anofox_*_fit call per group.                                    */
/*                                                                          */
/* Data layout ("grouped columns"): rows sorted by group; group g owns rows  */
/* [row_offsets[g], row_offsets[g+1]).  y is one array of n_rows doubles,    */
/* each feature j is one array x_cols[j] of n_rows doubles (the same         */
/* one-array-per-feature layout as AnofoxDataArray x[] — just concatenated   */
/* over groups), w likewise for WLS.  NULL inputs are encoded as NaN.        */
/* ------------------------------------------------------------------------ */

typedef struct AnofoxHipContext AnofoxHipContext; /* one device + one stream + reusable workspace */

typedef enum { ANOFOX_HIP_MODEL_OLS = 0, ANOFOX_HIP_MODEL_RIDGE = 1, ANOFOX_HIP_MODEL_WLS = 2 } AnofoxHipModel;

/* Union of AnofoxOlsOptions / AnofoxRidgeOptions / AnofoxWlsOptions (same field meaning). */
typedef struct {
	AnofoxHipModel model;
	bool fit_intercept;
	bool compute_inference;
	double confidence_level;
	double alpha; /* ridge only; < 0 -> every group fails with ANOFOX_ERROR_INVALID_ALPHA */
	AnofoxSolverType solver;
	AnofoxLambdaScaling lambda_scaling;
	AnofoxHcType hc_type; /* HC0..HC3 replace se/t/p/ci (OLS, WLS); ignored for ridge and without inference */
} AnofoxHipBatchOptions;

/* Per-group status word stored in the core record: an AnofoxErrorCode, or this value for groups the
 * aggregate maps to SQL NULL before calling the fit (fewer than 2 rows, ols_aggregate.cpp:263-267). */
#define ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS 100
/* A streaming aggregate state could not bring this group to the contract's accuracy: its solve asked for the
 * refinement passes (ill-conditioned, or fitting almost exactly) and the group's rows are no longer there — no row log,
 * or one that outgrew its budgets.  The record is NaN; the SQL layer returns NULL and counts it. */
#define ANOFOX_HIP_STATUS_UNREFINED 101

/* Result records, row-major f64, one per group:
 *   core[g]      = { coefficients[0..p), intercept, r_squared, adj_r_squared, residual_std_error,
 *                    n_observations, status }                                   length p + 6
 *   inference[g] = { std_errors[p], t_values[p], p_values[p], ci_lower[p], ci_upper[p],
 *                    f_statistic, f_pvalue }                                    length 5p + 2
 * Fields of the STRUCT the aggregates return (ols_aggregate.cpp:74-96); n_features is the constant p.
 * status != 0  =>  the group is SQL NULL and every other field is NaN.
 * Constant columns give NaN coefficients / inference entries (models/ols.rs:167-171,191-206). */
ANOFOX_HIP_API size_t anofox_hip_core_record_len(size_t n_features);
ANOFOX_HIP_API size_t anofox_hip_inference_record_len(size_t n_features);

/* Largest n_features the library accepts. */
ANOFOX_HIP_API size_t anofox_hip_max_features(void);

/* device_id < 0 selects the current HIP device.  The context owns a stream; calls on one context are
 * serialised, different contexts (e.g. one per DuckDB worker thread) are independent. */
ANOFOX_HIP_API bool anofox_hip_context_create(int device_id, AnofoxHipContext **out_ctx, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_context_destroy(AnofoxHipContext *ctx);

/* Launch on a caller-owned hipStream_t (passed as void*) instead of the context's own (non-blocking) stream.
 * NULL is a stream too — HIP's default stream, which is what PyTorch's default stream is — and is used as given;
 * anofox_hip_context_use_own_stream goes back to the context's stream. */
ANOFOX_HIP_API bool anofox_hip_context_set_stream(AnofoxHipContext *ctx, void *hip_stream, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_context_use_own_stream(AnofoxHipContext *ctx, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_context_synchronize(AnofoxHipContext *ctx, AnofoxError *out_error);
/* Pipelining hook for callers that alternate consecutive batches between two contexts on two streams, so that the
 * small solve / refinement kernels of batch k overlap the HBM-bound accumulate kernel of batch k + 1: the fit entry
 * points make the stream wait for `wait_event` (hipEvent_t as void*, may be NULL) before the accumulate kernel and
 * record `record_event` (may be NULL) right after it.  Chaining the events keeps the accumulate kernels of the two
 * contexts from running against each other.  The gate is ONE-SHOT: it applies to the next fit call on this context
 * only and is cleared by it (the event handles stay the caller's; the library never keeps them past that call). */
ANOFOX_HIP_API bool anofox_hip_context_set_accumulate_gate(AnofoxHipContext *ctx, void *wait_event, void *record_event,
                                            AnofoxError *out_error);

/*
 * Device-resident batch fit.  d_* are device pointers on the context's device; x_cols is a HOST array of
 * n_features device pointers.  d_w may be NULL unless model == WLS.  d_inference may be NULL unless
 * options.compute_inference.  Asynchronous on the context's stream; outputs are complete after
 * anofox_hip_context_synchronize (or a synchronisation of the caller's stream).
 * Returns false (nothing launched) on invalid arguments; per-group failures are reported in the records.
 */
ANOFOX_HIP_API bool anofox_hip_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                 const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                 const double *d_w, AnofoxHipBatchOptions options, double *d_core, double *d_inference,
                                 AnofoxError *out_error);

/* Same with host pointers: stages inputs to the GPU, runs the device path, copies the records back,
 * synchronous.  ctx may be NULL (a per-thread default context on the current device is used). */
ANOFOX_HIP_API bool anofox_hip_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                               const int64_t *row_offsets, const double *y, const double *const *x_cols,
                               const double *w, AnofoxHipBatchOptions options, double *core, double *inference,
                               AnofoxError *out_error);

/*
 * Grouped elastic net (anofox_stats_elasticnet_fit_agg): per group, over the rows with finite y and x, minimise
 *     1/2 sum_i (y_i - b0 - x_i'b)^2 + lam (l1_ratio sum |b_j| + (1 - l1_ratio)/2 sum b_j^2)
 * with lam = alpha (RAW) or n alpha / sd_y (GLMNET, as ridge), by cyclic coordinate descent from b = 0 on the moments
 * of the accumulate kernels (DESIGN.md §1 "Elastic net").  Records: core[g] as above (length p + 6); statuses 4
 * (alpha < 0), 5 (l1_ratio outside [0, 1]), 6, 10, ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS.  iterations (may be NULL):
 * iterations[g] = sweeps run, negated when max_iterations stopped the group (its last iterate is returned, status 0).
 */
typedef struct {
	bool fit_intercept;
	double alpha;
	double l1_ratio;
	uint32_t max_iterations;
	double tolerance;
	AnofoxLambdaScaling lambda_scaling;
} AnofoxHipElasticNetBatchOptions;

ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                            AnofoxHipElasticNetBatchOptions options, double *d_core, int32_t *d_iterations,
                                            AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                          const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                          AnofoxHipElasticNetBatchOptions options, double *core, int32_t *iterations,
                                          AnofoxError *out_error);

/*
 * Elastic net fit + predict (anofox_stats_elasticnet_fit_predict_agg, src/aggregate_functions/
 * elasticnet_predict_aggregate.cpp:300-395): the fit of anofox_hip_elasticnet_fit_batch_* on each group's training rows
 * (finite y and x), then every row gets {yhat, yhat_lower, yhat_upper} (pred, [n_rows x 3], NaN = SQL NULL) with the
 * simplified interval of anofox_predict_with_interval (the record's sigma and n) at confidence_level, as
 * anofox_hip_fit_predict_batch_*.  train_counts (optional) is what the "fewer than 2 training rows -> NULL" rule looks at
 * (:309); core receives the records (p + 6).  A group whose status is not 0 predicts NaN everywhere.
 */
ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                    const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                    const int64_t *d_train_counts, AnofoxHipElasticNetBatchOptions options,
                                                    double confidence_level, double *d_core, double *d_pred, AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                  const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                  const int64_t *train_counts, AnofoxHipElasticNetBatchOptions options,
                                                  double confidence_level, double *core, double *pred, AnofoxError *out_error);

/*
 * Grouped bounded least squares (anofox_stats_bls_fit_agg, anofox_stats_nnls_fit_agg): per group, over the rows with finite
 * y and x, the minimiser of 1/2 sum_i (y_i - b0 - x_i'b)^2 subject to lower_j <= b_j <= upper_j over the non-constant
 * columns, b0 free (absent without an intercept), by an active-set method with a Cholesky solve on the free set, on the
 * moments of the accumulate kernels (DESIGN.md §1 "Bounded least squares").  The bounds are HOST arrays shared by all groups
 * of the call (also in the device form; they travel in the kernel arguments): length 0 = that side unbounded, 1 = every
 * column, n_features = per column; both absent = NNLS (lower 0).  Any other length, a NaN bound or lower_j > upper_j gives
 * every group status 1.  Records (anofox_hip_bls_record_len(p) = 3p + 6 doubles):
 *   bls[g] = { coefficients[0..p), intercept, ssr, r_squared, n_observations, n_active_constraints, status,
 *              at_lower_bound[p], at_upper_bound[p] (0.0 / 1.0) }
 * status != 0 => every other field is NaN; statuses 1, 6, 10, ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS.  A coefficient the solve
 * holds on a bound is stored as exactly that bound.  iterations (may be NULL): iterations[g] = outer iterations run, negated
 * when max_iterations stopped the group (its last feasible iterate is returned, status 0).
 */
typedef struct {
	bool fit_intercept;
	const double *lower_bounds;
	size_t lower_bounds_len;
	const double *upper_bounds;
	size_t upper_bounds_len;
	uint32_t max_iterations;
	double tolerance;
} AnofoxHipBlsBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_bls_record_len(size_t n_features);
ANOFOX_HIP_API bool anofox_hip_bls_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                     const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                     AnofoxHipBlsBatchOptions options, double *d_bls, int32_t *d_iterations,
                                     AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_bls_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                   const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                   AnofoxHipBlsBatchOptions options, double *bls, int32_t *iterations, AnofoxError *out_error);

/*
 * Bounded least squares fit + predict (anofox_stats_bls_fit_predict_agg, src/aggregate_functions/
 * bls_fit_predict_aggregate.cpp:330-452): the fit above on each group's training rows, then every row gets {yhat, yhat_lower,
 * yhat_upper} as anofox_hip_elasticnet_fit_predict_batch_*.  core receives records in the REGRESSION layout (p + 6), which
 * the predict kernels read: { coefficients[p], intercept, r_squared, ssr, sigma, n_observations, status } with the
 * reference's sigma = sqrt(ssr / df), df = n_observations - n_features - [intercept] over ALL columns in unsigned 64-bit
 * arithmetic (it wraps when constant columns make it negative: sigma ~ 0), NaN when df = 0 or ssr is NaN.
 */
ANOFOX_HIP_API bool anofox_hip_bls_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                             const int64_t *d_train_counts, AnofoxHipBlsBatchOptions options,
                                             double confidence_level, double *d_core, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_bls_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                           const int64_t *train_counts, AnofoxHipBlsBatchOptions options,
                                           double confidence_level, double *core, double *pred, AnofoxError *out_error);

/*
 * Grouped quantile regression (anofox_quantile_fit, anofox_stats_quantile_fit_predict_agg): per group, over the rows with
 * finite y and x, THE minimiser of the pinball loss sum_i rho_tau(y_i - b0 - x_i'b), rho_tau(r) = r (tau - [r < 0]) — the
 * exact vertex of the linear program, by a simplex over the rows, one wavefront per group (DESIGN.md §1 "Quantile
 * regression").  1 <= n_features <= 32; more fails the call with ANOFOX_ERROR_INVALID_INPUT.  tolerance is accepted and
 * unused.  Records (anofox_hip_quantile_record_len(p) = p + 6 doubles):
 *   quantile[g] = { coefficients[0..p), intercept (NaN without one), tau, loss (the pinball sum over the valid rows),
 *                   n_basis_rows (k minus the artificials left: the rank of the design), n_observations, status }
 * status != 0 => every other field is NaN; statuses 1 (tau not in (0, 1) or NaN: every group of the call), 6 (fewer valid
 * rows than p + [intercept]; equality is allowed and interpolates), 10, ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS.  2 (the final
 * basis factorised with an exactly zero pivot: a guard, not expected).  An aliased
 * column's coefficient is exactly 0.0.  iterations (may be NULL): iterations[g] = simplex pivots, negated when
 * max_iterations (or the ceiling 1000 + 50 k) stopped the group (its last vertex is returned, status 0; with max_iterations = 0
 * that is beta = 0 with count 0 and n_basis_rows = 0).
 */
typedef struct {
	double tau;
	bool fit_intercept;
	uint32_t max_iterations;
	double tolerance;
} AnofoxHipQuantileBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_quantile_record_len(size_t n_features);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                          const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                          AnofoxHipQuantileBatchOptions options, double *d_quantile, int32_t *d_iterations,
                                          AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_quantile_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                        const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                        AnofoxHipQuantileBatchOptions options, double *quantile, int32_t *iterations,
                                        AnofoxError *out_error);

/*
 * Quantile regression fit + predict (anofox_stats_quantile_fit_predict_agg, src/aggregate_functions/
 * quantile_fit_predict_aggregate.cpp:269-345): the fit above on each group's training rows, then every row gets
 * pred = {yhat, NaN, NaN} ([n_rows x 3]; there is no interval; a non-finite yhat is NaN = SQL NULL).  core receives records in
 * the REGRESSION layout (p + 6): { coefficients[p], intercept, NaN, NaN, NaN, n_observations, status }.  Fewer than 2
 * training rows (train_counts, optional) or a failed fit: status != 0 and NaN for every row of the group.
 */
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                  const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                  const int64_t *d_train_counts, AnofoxHipQuantileBatchOptions options,
                                                  double *d_core, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                const int64_t *train_counts, AnofoxHipQuantileBatchOptions options,
                                                double *core, double *pred, AnofoxError *out_error);

/*
 * The tau path: the fit above at every tau of a grid in ONE call (DESIGN.md §1 "Quantile regression", "tau path").  A group's
 * wavefront stages its rows once and walks the valid tau in ascending order (ties in the caller's order), pivoting from each
 * tau's optimal vertex to the next, so the result does not depend on the caller's order and equal tau give identical records.
 * taus is HOST memory in every variant (the grid travels in the kernel arguments), 1 <= n_taus <= 64: NULL, 0 or more fails
 * the call.  options.tau is ignored.  quantile[(g n_taus + t)] is the record (layout above) of group g at taus[t], iterations
 * [n_groups x n_taus] (may be NULL) its pivots from the vertex the tau before left, with max_iterations and the sign
 * convention per tau.  A tau outside (0, 1) or NaN: status 1, iteration count 0 (and a NaN pred column) at that position for
 * every group; the other positions are fitted normally.  The row rules fail a group at every tau alike; status 2 at one tau
 * fails every later tau (ascending) of that group too.  Each record is an optimal vertex of its tau: when the optimum is not
 * unique it may be another vertex than the single-tau call returns, with the same loss.
 * The fit-predict variants also write pred[n_rows x n_taus]: pred[i n_taus + t] = b0 + x_i'b at taus[t] for EVERY row of the
 * groups (rows with a NaN y: prediction rows), written by the group's wavefront right after the record; NaN where an x of the
 * row is not finite or the fit at that tau failed.  train_counts as anofox_hip_quantile_fit_predict_batch_*.  The records
 * keep the quantile layout.  The device variant does not write rows outside [row_offsets[0], row_offsets[n_groups]).
 */
ANOFOX_HIP_API bool anofox_hip_quantile_fit_path_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                               const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                               AnofoxHipQuantileBatchOptions options, const double *taus, size_t n_taus,
                                               double *d_quantile, int32_t *d_iterations, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_path_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                             AnofoxHipQuantileBatchOptions options, const double *taus, size_t n_taus,
                                             double *quantile, int32_t *iterations, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_path_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features,
                                                       int64_t n_rows, const int64_t *d_row_offsets, const double *d_y,
                                                       const double *const *x_cols, const int64_t *d_train_counts,
                                                       AnofoxHipQuantileBatchOptions options, const double *taus, size_t n_taus,
                                                       double *d_quantile, int32_t *d_iterations, double *d_pred,
                                                       AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_path_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features,
                                                     int64_t n_rows, const int64_t *row_offsets, const double *y,
                                                     const double *const *x_cols, const int64_t *train_counts,
                                                     AnofoxHipQuantileBatchOptions options, const double *taus, size_t n_taus,
                                                     double *quantile, int32_t *iterations, double *pred, AnofoxError *out_error);


/*
 * Grouped generalised linear models (anofox_poisson_fit / anofox_binomial_fit / anofox_logistic_fit and the aggregates
 * poisson_fit_agg, binomial_fit_agg, logistic_fit_agg, poisson_fit_predict_agg): per group, over the rows whose y, x and offset
 * are all finite, THE minimiser of deviance(beta) + lambda sum_j beta_j^2 (the intercept not penalised) for Poisson / log or
 * binomial / logit, by the reference's IRLS loop fused into one kernel, one wavefront per group (DESIGN.md §1 "Generalised
 * linear models").  1 <= n_features <= 32; more fails the call.  offset (may be NULL): one double per row, added to eta.
 * Records (anofox_hip_glm_record_len(p) = p + 11 doubles):
 *   glm[g] = { coefficients[0..p), intercept (NaN without one), deviance, null_deviance (at mu = mean y of the valid rows),
 *              pseudo_r_squared, aic, dispersion, n_observations, n_params, iterations, converged, status }
 * status != 0 => every other field is NaN; statuses 1 (invalid options: every group of the call; or a finite y outside the
 * support: y < 0 for Poisson, y outside [0, 1] for binomial), 3 (no convergence in max_iterations), 6 (fewer valid rows than
 * max(k, 1), k = the fitted columns + [intercept]), 10 (no valid row), ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS (fit-predict only).
 * A column that is constant over the valid rows (with an intercept) or aliased has a NaN coefficient.
 * inference (may be NULL): [n_groups x 5 p] = { se[p], z[p], p[p], ci_lower[p], ci_upper[p] } per group, the intercept
 * stripped; NaN when compute_inference is false, for a failed group and for a dropped or aliased column.
 * Invalid options: tolerance not finite and positive, lambda < 0 or NaN, an unknown family, max_iterations = 0, and a
 * confidence_level outside (0, 1) while compute_inference is set.
 */
#define ANOFOX_HIP_GLM_POISSON 0  /* log link */
#define ANOFOX_HIP_GLM_BINOMIAL 1 /* logit link; logistic is the same fit */
typedef struct {
	int32_t family;
	bool fit_intercept;
	uint32_t max_iterations;
	double tolerance;
	double lambda;
	bool compute_inference;
	double confidence_level;
} AnofoxHipGlmBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_glm_record_len(size_t n_features);
ANOFOX_HIP_API bool anofox_hip_glm_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                     const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                     const double *d_offset, AnofoxHipGlmBatchOptions options, double *d_records,
                                     double *d_inference, AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_glm_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                   const int64_t *row_offsets, const double *y, const double *const *x_cols, const double *offset,
                                   AnofoxHipGlmBatchOptions options, double *records, double *inference, AnofoxError *out_error);
/*
 * Fit + predict (poisson_fit_predict_agg): the fit above on each group's rows with a finite y, then pred = {mu, NaN, NaN}
 * ([n_rows x 3], the response scale, no interval) for every row of the group, training or not; a row with a non-finite x or
 * offset gets NaN.  core: the records above.  Fewer than 2 training rows (train_counts, optional; the group's rows without
 * it) or a failed fit: status != 0 and NaN for every row of the group.  The same kernel writes records and predictions.
 */
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                             const double *d_offset, const int64_t *d_train_counts,
                                             AnofoxHipGlmBatchOptions options, double *d_core, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                           const double *offset, const int64_t *train_counts, AnofoxHipGlmBatchOptions options,
                                           double *core, double *pred, AnofoxError *out_error);
/*
 * Fit + predict with the interval of poisson_fit_predict_agg: the entry points above plus interval_z.  interval_z == 0 is exactly
 * anofox_hip_glm_fit_predict_batch_*.  interval_z > 0 (finite), Poisson: the lane that writes mu of a row also writes, for every
 * row with a finite mu,  s = sqrt(dispersion) / max(mu, 0.001),  pred[3 i + 1] = max(0, exp(eta - interval_z s)),
 * pred[3 i + 2] = exp(eta + interval_z s),  eta the full linear predictor (offset included): the reference's formula
 * (poisson_fit_predict_aggregate.cpp:471-478, 498-502), kept as it stands.  A non-finite mu leaves all three NaN.
 * interval_z negative or not finite, or > 0 with the binomial family: false, ANOFOX_ERROR_INVALID_INPUT, "glm: ...", no launch.
 */
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_interval_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features,
                                                      int64_t n_rows, const int64_t *d_row_offsets, const double *d_y,
                                                      const double *const *x_cols, const double *d_offset,
                                                      const int64_t *d_train_counts, AnofoxHipGlmBatchOptions options,
                                                      double interval_z, double *d_core, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_interval_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features,
                                                    int64_t n_rows, const int64_t *row_offsets, const double *y,
                                                    const double *const *x_cols, const double *offset, const int64_t *train_counts,
                                                    AnofoxHipGlmBatchOptions options, double interval_z, double *core, double *pred,
                                                    AnofoxError *out_error);
/*
 * The fit with the training accuracy of logistic_fit_agg: anofox_hip_glm_fit_batch_* plus accuracy[n_groups], binomial family only
 * (Poisson, or a threshold that is not finite: false with a "glm: ..." message, no launch).  accuracy[g] = the share of the group's
 * fitted rows (y, x and offset finite) with (mu >= threshold ? 1.0 : 0.0) == y, mu computed as the prediction pass of fit-predict
 * computes it, so that it equals a count over pred[:, 0] exactly; the wavefront that holds beta counts, nothing per row leaves the
 * device.  NaN for a failed group; a fitted group has at least one such row (status 6 / 10 otherwise), so never 0 / 0.
 */
ANOFOX_HIP_API bool anofox_hip_glm_fit_accuracy_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                              const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                              const double *d_offset, AnofoxHipGlmBatchOptions options, double threshold,
                                              double *d_records, double *d_inference, double *d_accuracy, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glm_fit_accuracy_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                            const double *offset, AnofoxHipGlmBatchOptions options, double threshold, double *records,
                                            double *inference, double *accuracy, AnofoxError *out_error);

/*
 * Information criteria as batched outputs of the fit records: what the SQL functions
 * aic(rss, n, k) / bic(rss, n, k) (src/scalar_functions/aic_bic.cpp:12-110 over
 * crates/anofox-stats-core/src/diagnostics/information_criteria.rs:15-33,67-85) give when they are applied to every
 * group's fit with k = estimated parameters (coefficients that are not NaN, + 1 with an intercept) and
 * rss = residual_std_error^2 (n_observations - k):  out[g] = { rss, aic, bic },  aic = n ln(rss / n) + 2 k,
 * bic = n ln(rss / n) + k ln n,  rss == 0 -> -inf (:24-26),  NaN for NULL groups and for n == k.
 * `core` = records of anofox_hip_fit_batch_* fitted with the same `options` (fit_intercept and model are used).
 */
ANOFOX_HIP_API bool anofox_hip_information_criteria_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features,
                                                  const double *d_core, AnofoxHipBatchOptions options, double *d_out,
                                                  AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_information_criteria_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features,
                                                const double *core, AnofoxHipBatchOptions options, double *out,
                                                AnofoxError *out_error);

/*
 * fit + predict in one batch: the `*_fit_predict_agg` aggregates (src/aggregate_functions/ols_predict_aggregate.cpp:
 * 322-425, ridge/wls likewise).  Every row of every group gets {yhat, yhat_lower, yhat_upper} (d_pred, [n_rows x 3],
 * NaN = SQL NULL); rows whose y is NaN (the aggregate's NULL y = "prediction row") or that hold a non-finite
 * feature do not train.  d_train_counts (optional, [n_groups]) is the number of training rows the aggregate's
 * "fewer than 2 -> NULL" rule looks at (ols_predict_aggregate.cpp:333); NULL = use the group's row count.
 * d_core receives the fit records as in anofox_hip_fit_batch_device (compute_inference is ignored: the
 * aggregates fit with inference off).
 */
ANOFOX_HIP_API bool anofox_hip_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                         const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                         const double *d_w, const int64_t *d_train_counts, AnofoxHipBatchOptions options,
                                         double *d_core, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                       const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                       const double *w, const int64_t *train_counts, AnofoxHipBatchOptions options,
                                       double *core, double *pred, AnofoxError *out_error);

/*
 * Expanding-window fit + predict: the `*_fit_predict(y, x [, w] [, opts]) OVER (PARTITION BY .. ORDER BY ..
 * ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW)` window functions (src/window_functions/ols_fit_predict.cpp:
 * 110-324, ridge_fit_predict.cpp, wls_fit_predict.cpp).  Partitions = groups, rows already in window order.
 * d_pred[3*e .. 3*e+2] = {yhat, yhat_lower, yhat_upper} of x_e from the fit on rows 0..e of e's partition
 * (rows with NaN y — the window's NULL y — or non-finite features do not train); NaN = SQL NULL (at most
 * p + [intercept] training rows so far, failed fit, or non-finite prediction).  A frame ending at 1 PRECEDING is
 * this output shifted down by one row within the partition.  n_features <= 8 run the in-register window kernels,
 * wider designs the virtual-group path (anofox_hip_fit_predict_frames_*).
 */
ANOFOX_HIP_API bool anofox_hip_fit_predict_expanding_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                             const double *d_w, AnofoxHipBatchOptions options, double *d_pred,
                                             AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_fit_predict_expanding_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                           const double *w, AnofoxHipBatchOptions options, double *pred,
                                           AnofoxError *out_error);

/*
 * The same window functions over any ROWS frame:
 *   ROWS BETWEEN start_preceding PRECEDING AND end_preceding PRECEDING
 * Offsets count rows before the current row; 0 = CURRENT ROW, negative = FOLLOWING (-3 = 3 FOLLOWING);
 * start_preceding = ANOFOX_HIP_FRAME_UNBOUNDED = UNBOUNDED PRECEDING, end_preceding = -ANOFOX_HIP_FRAME_UNBOUNDED =
 * UNBOUNDED FOLLOWING; start_preceding >= end_preceding.  Frames are clipped to the partition, as DuckDB does.
 * The aggregate trains on the frame's rows with non-NULL y and predicts the x of the LAST row of the frame
 * (ols_fit_predict.cpp:157-162), so with end_preceding = b the output of row e uses x of row e - b (or of the
 * partition's last row when the frame reaches past it); rows whose frame is empty are NULL.  Frames that start
 * UNBOUNDED PRECEDING run the one-pass prefix kernel, the others sum each frame directly (O(frame) per row).
 */
#define ANOFOX_HIP_FRAME_UNBOUNDED INT64_MAX
typedef struct {
	int64_t start_preceding;
	int64_t end_preceding;
} AnofoxHipWindowFrame;
ANOFOX_HIP_API bool anofox_hip_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                          const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                          const double *d_w, AnofoxHipWindowFrame frame, AnofoxHipBatchOptions options,
                                          double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                        const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                        const double *w, AnofoxHipWindowFrame frame, AnofoxHipBatchOptions options,
                                        double *pred, AnofoxError *out_error);

/*
 * The same window functions over EXPLICIT frames — RANGE and GROUPS frames, EXCLUDE clauses, anything DuckDB's window
 * executor resolves to a row range per output row (src/window_functions/ols_fit_predict.cpp:110-324 receives the
 * frame's rows whatever the frame type): frame of row e = rows [frame_lo[e], frame_hi[e]) of the (already ordered)
 * input, hi exclusive; an empty frame (hi <= lo) is NULL.  Trains on the frame's rows with non-NULL (non-NaN) y,
 * predicts the x of the frame's LAST row hi - 1, NULL unless MORE than p + [intercept] training rows exist (:257-262).
 * Every frame is fitted as a group of the batch path (its refinement passes included), so any n_features <=
 * anofox_hip_max_features() and any frame shape work; cost O(frame) per output row.  The ROWS entry points above use
 * this path for n_features > 8 and for the frames the in-register kernels flag as ill-conditioned.
 */
ANOFOX_HIP_API bool anofox_hip_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                          const double *const *x_cols, const double *d_w, const int64_t *d_frame_lo,
                                          const int64_t *d_frame_hi, AnofoxHipBatchOptions options, double *d_pred,
                                          AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                        const double *const *x_cols, const double *w, const int64_t *frame_lo,
                                        const int64_t *frame_hi, AnofoxHipBatchOptions options, double *pred,
                                        AnofoxError *out_error);

/*
 * The elastic net window function anofox_stats_elasticnet_fit_predict(y, x [, options]) OVER (... ROWS ...)
 * (src/window_functions/elasticnet_fit_predict.cpp:150-330): per output row, the elastic net fit of the frame's rows with
 * non-NULL y, NULL unless MORE than p + [intercept] such rows exist, predicting the x of the frame's LAST row; frames as
 * anofox_hip_fit_predict_window_* (the expanding window is frame = {ANOFOX_HIP_FRAME_UNBOUNDED, 0}).  For p <= 8 the
 * in-register window kernels solve every frame from its moments; frames whose moment rss cancels or that fail the
 * Cholesky pivot test are refitted through the frames path, which serves p > 8 entirely.
 */
ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                     const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                     AnofoxHipWindowFrame frame, AnofoxHipElasticNetBatchOptions options,
                                                     double confidence_level, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                   const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                   AnofoxHipWindowFrame frame, AnofoxHipElasticNetBatchOptions options,
                                                   double confidence_level, double *pred, AnofoxError *out_error);
/* the same over explicit frames [frame_lo[e], frame_hi[e]) (as anofox_hip_fit_predict_frames_*): every frame a group of the
 * elastic net batch fit */
ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                                     const double *const *x_cols, const int64_t *d_frame_lo, const int64_t *d_frame_hi,
                                                     AnofoxHipElasticNetBatchOptions options, double confidence_level, double *d_pred,
                                                     AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_elasticnet_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                                   const double *const *x_cols, const int64_t *frame_lo, const int64_t *frame_hi,
                                                   AnofoxHipElasticNetBatchOptions options, double confidence_level, double *pred,
                                                   AnofoxError *out_error);

/*
 * Grouped recursive least squares (anofox_stats_rls_fit_agg): per group, the reference's sequential filter over the rows
 * with finite y and x, in row order and in its exact operation order (DESIGN.md §1 "Recursive least squares"), so the
 * coefficients are bit-identical to fit_rls.  Records: core[g] as above (length p + 6) with r_squared, adj_r_squared and
 * residual_std_error NaN; statuses 1 (forgetting_factor outside (0, 1] or initial_p_diagonal <= 0, checked only when some
 * column is not constant), 6, 10, ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS.
 */
typedef struct {
	bool fit_intercept;
	double forgetting_factor;
	double initial_p_diagonal;
} AnofoxHipRlsBatchOptions;

ANOFOX_HIP_API bool anofox_hip_rls_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                     const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                     AnofoxHipRlsBatchOptions options, double *d_core, AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_rls_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                   const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                   AnofoxHipRlsBatchOptions options, double *core, AnofoxError *out_error);

/*
 * RLS fit + predict (anofox_stats_rls_fit_predict_agg, src/aggregate_functions/rls_predict_aggregate.cpp): the fit of
 * anofox_hip_rls_fit_batch_* on each group, then every row gets {yhat, yhat, yhat} (pred, [n_rows x 3], NaN = SQL NULL):
 * anofox_predict_with_interval with sigma = NaN, so the interval is the point and confidence_level has no effect.
 * train_counts (optional) is what the "fewer than 2 training rows -> NULL" rule looks at.  A group whose status is not 0
 * predicts NaN everywhere.
 */
ANOFOX_HIP_API bool anofox_hip_rls_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                             const int64_t *d_train_counts, AnofoxHipRlsBatchOptions options,
                                             double confidence_level, double *d_core, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_rls_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                           const int64_t *train_counts, AnofoxHipRlsBatchOptions options,
                                           double confidence_level, double *core, double *pred, AnofoxError *out_error);

/*
 * The RLS window function anofox_stats_rls_fit_predict(y, x [, options]) OVER (... ROWS ...) (src/window_functions/
 * rls_fit_predict.cpp): per output row, the RLS fit of the frame's rows, NULL unless MORE than p + [intercept] rows with
 * non-NULL y exist (:228), predicting the x of the frame's LAST row; frames as anofox_hip_fit_predict_window_*.  Every frame
 * runs the batch filter over its own rows (one lane per frame for p <= 8, one wavefront above).
 */
ANOFOX_HIP_API bool anofox_hip_rls_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                              const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                              AnofoxHipWindowFrame frame, AnofoxHipRlsBatchOptions options,
                                              double confidence_level, double *d_pred, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_rls_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                            AnofoxHipWindowFrame frame, AnofoxHipRlsBatchOptions options,
                                            double confidence_level, double *pred, AnofoxError *out_error);
/* the same over explicit frames [frame_lo[e], frame_hi[e]) (as anofox_hip_fit_predict_frames_*) */
ANOFOX_HIP_API bool anofox_hip_rls_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                              const double *const *x_cols, const int64_t *d_frame_lo, const int64_t *d_frame_hi,
                                              AnofoxHipRlsBatchOptions options, double confidence_level, double *d_pred,
                                              AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_rls_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                            const double *const *x_cols, const int64_t *frame_lo, const int64_t *frame_hi,
                                            AnofoxHipRlsBatchOptions options, double confidence_level, double *pred,
                                            AnofoxError *out_error);

/*
 * The quantile regression window function: quantile_fit_predict(y, x [, options]) OVER (PARTITION BY .. ORDER BY .. ROWS ..)
 * — rolling medians and rolling quantile bands.  Per output row e the fit above over the frame's rows with finite y and x,
 * predicting the x of the frame's LAST row: pred[3 e] = {yhat, NaN, NaN} (there is no interval).  The row rules are the
 * fit-predict aggregate's, per frame: fewer than 2 rows with a non-NaN y -> ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS, no valid row
 * -> 10, fewer valid rows than p + [intercept] -> 6 (equality interpolates).  pred is NaN (SQL NULL) for an empty frame, a
 * failed rule, a failed fit and a non-finite yhat; tau outside (0, 1) gives status 1 on every row; n_features > 32 fails the
 * call.  quantile (may be NULL) receives [n_rows x (p + 6)] records in the layout of anofox_hip_quantile_fit_batch_*,
 * iterations (may be NULL) the pivots of each frame, negated when max_iterations (per frame) stopped it.
 * Frames: ROWS BETWEEN start_preceding PRECEDING AND end_preceding PRECEDING, clipped to the partition as
 * anofox_hip_fit_predict_window_* clips them; row_offsets must start at 0 and end at n_rows.  The frames entry points take
 * explicit bounds [frame_lo[e], frame_hi[e]) of any shape (hi <= lo: empty).
 * Method (DESIGN.md §1 "Quantile regression", "Window function"): a wavefront walks a run of consecutive output rows of one
 * partition and carries the optimal vertex from frame to frame — rows that leave are masked, rows that enter get their
 * residual from the carried coefficients, and the simplex pivots on from there.  A frame begins afresh when it is the first
 * of its run, when its bounds are not both non-decreasing or it does not overlap the frame before it, when a row of the
 * carried basis left, and after a frame that failed.  Each frame's result is an LP-optimal vertex of that frame's rows with
 * aliased coefficients exactly 0.0; where the optimum is not unique it may be another vertex than a fit of the frame alone
 * returns, with the same loss.  A host-side planner cuts the partitions into runs (about 8192 walkers when partitions are few
 * and long, a whole partition per walker when they are many or the frames start UNBOUNDED PRECEDING); each launched wavefront
 * owns 24 bytes of scratch per row of the longest chain of a run (consecutive frames with non-decreasing, overlapping bounds:
 * last frame's end - first frame's start; unsorted or far-apart explicit frames begin afresh and cost none), 1 GiB in all at
 * most: fewer wavefronts are launched to stay below it, and a single span above it fails the call ("quantile window: frame
 * span .. exceeds the scratch budget").  The device variants copy the offsets / the frame bounds to the host for the planner.
 */
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                   const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                   AnofoxHipWindowFrame frame, AnofoxHipQuantileBatchOptions options, double *d_pred,
                                                   double *d_quantile, int32_t *d_iterations, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                 const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                 AnofoxHipWindowFrame frame, AnofoxHipQuantileBatchOptions options, double *pred,
                                                 double *quantile, int32_t *iterations, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                                   const double *const *x_cols, const int64_t *d_frame_lo, const int64_t *d_frame_hi,
                                                   AnofoxHipQuantileBatchOptions options, double *d_pred, double *d_quantile,
                                                   int32_t *d_iterations, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_quantile_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                                 const double *const *x_cols, const int64_t *frame_lo, const int64_t *frame_hi,
                                                 AnofoxHipQuantileBatchOptions options, double *pred, double *quantile,
                                                 int32_t *iterations, AnofoxError *out_error);
/* The planner alone, on host arrays (no device is touched): run_begin ([capacity], may be NULL) receives the first output row
 * of every walker and one entry past the last, *n_runs their number, *span_rows the scratch rows of one wavefront, *n_waves
 * the wavefronts a launch would use.  run_length / scratch_cap_bytes 0: the library's rule. */
ANOFOX_HIP_API bool anofox_hip_quantile_window_plan(int64_t n_groups, const int64_t *row_offsets, int64_t n_rows, const int64_t *frame_lo,
                                     const int64_t *frame_hi, int64_t run_length, int64_t scratch_cap_bytes, int64_t *run_begin,
                                     int64_t capacity, int64_t *n_runs, int64_t *span_rows, int64_t *n_waves, AnofoxError *out_error);
/* For tests and measurements: the run length and the scratch cap of every later window call of the process (0: the rule). */
ANOFOX_HIP_API void anofox_hip_quantile_window_test_hooks(int64_t run_length, int64_t scratch_cap_bytes);
/* out[6] = {output rows, frames that began afresh, walkers, launched wavefronts, scratch rows per wavefront, restarts = the
 * frames begun afresh right after a fitted frame (a basis row left, or explicit bounds that are not monotone and overlapping)}
 * of the most recent window call on ctx (NULL: the thread's default context); waits for the context's stream.  The record is
 * the context's own: every window call on it resets it, no other call touches it, closing the context frees it. */
ANOFOX_HIP_API bool anofox_hip_quantile_window_stats(AnofoxHipContext *ctx, int64_t *out, AnofoxError *out_error);

/*
 * The window function of the GLM family: poisson_fit_predict / logistic_fit_predict OVER (PARTITION BY .. ORDER BY .. ROWS ..).
 * Output row e gets the fit of its frame's rows: pred[3 e] = {mu, lower, upper} at the x (and offset) of the FRAME'S LAST ROW,
 * and, with glm_records != NULL, the frame's record of p + 11 doubles in anofox_hip_glm_fit_batch_*'s layout.  One wavefront
 * walks a run of consecutive output rows of a partition; a frame whose bounds are both at or after those of the frame before it,
 * that overlaps it, and whose predecessor was fitted with every coefficient estimated starts IRLS from the predecessor's
 * coefficients, every other frame from mustart; a warm-started frame that does not converge or ends with a skipped column is
 * fitted again from mustart.  The answer is the minimiser of deviance + lambda sum b^2 either way.
 *   window  ROWS frames, clipped to the partition as anofox_hip_fit_predict_window_* clips them; row_offsets cover [0, n_rows].
 *   frames  explicit bounds [frame_lo[e], frame_hi[e]) of any shape; frame_hi <= frame_lo is an empty frame.
 * Row rules per frame, those of anofox_hip_glm_fit_predict_batch_* with train_counts = the frame's rows with a non-NaN y: fewer
 * than 2 of them -> ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS (an empty frame too); a finite y outside the support -> status 1, for
 * the frames that contain it; no valid row -> 10; fewer valid rows than fitted columns -> 6.  A failed frame, a non-finite x /
 * offset of the predicted row or a non-finite mu: NaN.  Invalid options: status 1 on every row.  n_features > 32 fails the call.
 * interval_z as in anofox_hip_glm_fit_predict_interval_batch_*: 0 leaves the bounds NaN, > 0 gives the Poisson bounds, > 0 with
 * the binomial family fails the call.  Scratch: 16 bytes per row of the call's longest frame per launched wavefront, from the
 * context's workspace, 1 GiB at most in all (fewer wavefronts are launched to stay below it); a single frame above that fails
 * the call: "glm window: frame of .. rows exceeds the scratch budget".  The device forms copy the offsets / the bounds to the
 * host for the planner (one synchronising copy).
 */
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                              const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                              const double *d_offset, AnofoxHipWindowFrame frame, AnofoxHipGlmBatchOptions options,
                                              double interval_z, double *d_pred, double *d_glm_records, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                            const double *offset, AnofoxHipWindowFrame frame, AnofoxHipGlmBatchOptions options,
                                            double interval_z, double *pred, double *glm_records, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                              const double *const *x_cols, const double *d_offset, const int64_t *d_frame_lo,
                                              const int64_t *d_frame_hi, AnofoxHipGlmBatchOptions options, double interval_z,
                                              double *d_pred, double *d_glm_records, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glm_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                            const double *const *x_cols, const double *offset, const int64_t *frame_lo,
                                            const int64_t *frame_hi, AnofoxHipGlmBatchOptions options, double interval_z,
                                            double *pred, double *glm_records, AnofoxError *out_error);
/*
 * The planner of the GLM window function alone, on host arrays, under the test hooks in force: run_begin (capacity entries, may
 * be NULL with capacity 0) receives the first output row of every walker and one entry past them, *n_runs their number,
 * *span_rows the scratch rows of one wavefront (the longest frame), *n_waves the wavefronts a launch would use.  No device.
 */
ANOFOX_HIP_API bool anofox_hip_glm_window_plan(int64_t n_groups, const int64_t *row_offsets, int64_t n_rows, const int64_t *frame_lo,
                                const int64_t *frame_hi, int64_t *run_begin, int64_t capacity, int64_t *n_runs,
                                int64_t *span_rows, int64_t *n_waves, AnofoxError *out_error);
/*
 * A test's hook: the run length and the scratch cap (0: the library's rule) and whether frames may start warm (1, the default;
 * 0: every frame starts cold, and a frame's record and mu are bit for bit anofox_hip_glm_fit_predict_batch_*'s on a group of
 * exactly the frame's rows) of every later GLM window call of the process.  No environment variable is read.
 */
ANOFOX_HIP_API void anofox_hip_glm_window_test_hooks(int64_t run_length, int64_t scratch_cap_bytes, int warm);
/*
 * What the most recent GLM window call on ctx (NULL: the thread's default context) did: out[8] = {output rows, frames started
 * cold, frames started warm, warm frames refitted cold, IRLS iterations summed over the frames, walkers, launched wavefronts,
 * scratch rows per wavefront}.  Waits for the context's stream.  Per context, reset by every GLM window call on it.
 */
ANOFOX_HIP_API bool anofox_hip_glm_window_stats(AnofoxHipContext *ctx, int64_t *out, AnofoxError *out_error);

/*
 * Grouped accelerated failure time (AFT) survival regression with right censoring (anofox_aft_fit and the aggregate
 * aft_fit_agg): log T = x'beta + sigma W.  Per group, over the rows whose time, event and x are all finite, THE stationary point
 * of the censored log-likelihood in (intercept, beta, log sigma), by the reference's Newton loop with step halving fused into
 * one kernel, one wavefront per group (DESIGN.md §1 "Accelerated failure time models").  event: 1 = the time is an observed
 * event, 0 = the row is right-censored at it.  1 <= n_features <= 32; more fails the call.  dist: ANOFOX_AFT_WEIBULL 0,
 * ANOFOX_AFT_LOGNORMAL 1, ANOFOX_AFT_LOGLOGISTIC 2, ANOFOX_AFT_EXPONENTIAL 3 (Weibull with sigma = 1, not estimated).
 * Records (anofox_hip_aft_record_len(p) = p + 13 doubles):
 *   aft[g] = { coefficients[0..p), intercept (NaN without one), scale (exactly 1 for exponential), log_likelihood,
 *              null_log_likelihood (the intercept-only model; NaN without an intercept or when that fit fails), aic = 2 k - 2 l,
 *              bic = k ln n - 2 l, n_observations, n_events, n_censored, n_params (k), iterations, converged, status }
 * status != 0 => every other field is NaN; statuses 1 (invalid options: every group of the call; or, among the rows that are
 * otherwise finite, a time <= 0 or an event other than 0 / 1; or every row censored), 10 (no valid row), 6 (fewer valid rows
 * than k + 1), 3 (no convergence in max_iterations), checked in this order.
 * inference (may be NULL): [n_groups x (5 p + 2)] = { se[p], z[p], p[p], ci_lower[p], ci_upper[p], intercept_std_error,
 * log_scale_std_error } per group, from the inverse of -H at the mode; NaN when compute_inference is 0, for a failed group and
 * for a parameter that is not fitted.
 * Invalid options: tolerance not finite and positive, max_iterations = 0, an unknown dist, and a confidence_level outside
 * (0, 1) while compute_inference is set.
 */
typedef struct {
	int dist;
	int fit_intercept;
	uint32_t max_iterations;
	double tolerance;
	int compute_inference;
	double confidence_level;
} AnofoxHipAftBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_aft_record_len(size_t n_features);
ANOFOX_HIP_API bool anofox_hip_aft_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                     const int64_t *d_row_offsets, const double *d_time, const double *const *d_x_cols,
                                     const double *d_event, AnofoxHipAftBatchOptions options, double *d_records,
                                     double *d_inference, AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_aft_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                   const int64_t *row_offsets, const double *time, const double *const *x_cols, const double *event,
                                   AnofoxHipAftBatchOptions options, double *records, double *inference, AnofoxError *out_error);
/*
 * A test's hook: the most workgroups a later AFT launch of the process starts (0: the library's rule, one per group up to
 * 2^20), so that a small batch exercises the kernel's stride over the groups.  The records do not depend on it.
 */
ANOFOX_HIP_API void anofox_hip_aft_test_hooks(int64_t max_blocks);

/*
 * AFT fit-predict (the aggregate aft_fit_predict_agg): the fit above and, by the same wavefront right after it, a score for every
 * row of the call.  records and inference are byte for byte those of anofox_hip_aft_fit_batch_* on the same inputs.  A row whose
 * event or time is not finite takes no part in the fit (the fit's own row rule) but is scored: a prediction row is a row with
 * event = NaN.  pred: [n_rows x anofox_hip_aft_pred_len() = 4] doubles, row i of the call at pred[4 i]:
 *   eta            x_i'beta (+ intercept), for a row of the fit the very value its likelihood term was computed from
 *   time_quantile  exp(eta + scale w_q), w_q the `quantile`-quantile of W (the median time at the default the bindings pass, 0.5)
 *   cdf            P(T <= time_i); 0 for a finite time_i <= 0; NaN where time_i is not finite
 *   risk           P(T <= time_i + horizon | T > time_i), from the difference of the two log-survival terms; for a finite
 *                  time_i <= 0 the cdf at time_i + horizon; exactly 0 at horizon = 0; NaN where time_i is not finite or
 *                  horizon is NaN ("risk not asked for")
 * All four are NaN for a row with an x that is not finite and for every row of a group whose status is not 0.  Rows outside
 * [row_offsets[0], row_offsets[n_groups]) are not written.  quantile NaN or outside the open interval (0, 1):
 * ANOFOX_ERROR_INVALID_INPUT, "aft: quantile must be in (0, 1)" (unlike anofox_aft_quantile, nothing is clamped); horizon negative
 * or infinite: "aft: horizon must be finite and >= 0"; pred NULL with n_groups > 0: "pred is NULL" (with no groups nothing is
 * written and NULL is taken, as for the other outputs); all before any device is touched.
 * anofox_hip_aft_test_hooks applies.
 */
typedef struct {
	double quantile;
	double horizon; /* NaN: risk is not asked for */
} AnofoxHipAftPredictOptions;

ANOFOX_HIP_API size_t anofox_hip_aft_pred_len(void);
ANOFOX_HIP_API bool anofox_hip_aft_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_time, const double *const *d_x_cols,
                                             const double *d_event, AnofoxHipAftBatchOptions options,
                                             AnofoxHipAftPredictOptions predict, double *d_records, double *d_inference,
                                             double *d_pred, AnofoxError *out_error);
/* host pointers, synchronous; ctx may be NULL (per-thread default context) */
ANOFOX_HIP_API bool anofox_hip_aft_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *time, const double *const *x_cols,
                                           const double *event, AnofoxHipAftBatchOptions options, AnofoxHipAftPredictOptions predict,
                                           double *records, double *inference, double *pred, AnofoxError *out_error);

/*
 * Empirical-Bayes shrinkage of per-group estimates (anofox_eb_shrink and the aggregate eb_shrink_agg; the reference's
 * crates/anofox-stats-core/src/models/eb_shrink.rs): the DerSimonian-Laird random-effects model, closed form.  A pair
 * (est, se) is usable when est is finite and se is finite and > 0; k = the usable pairs of a set, sums over them only:
 *   w = 1/se^2, Sw = sum w, fixed = sum w est / Sw, Q = sum w (est - fixed)^2 (a second pass about `fixed`), df = k - 1,
 *   C = Sw - sum w^2 / Sw;  tau^2 = options.tau_squared if it is not NaN, else 0 (ANOFOX_TAU_NONE), else
 *   max(0, (Q - df) / C) if C > 0 else 0;  wr = 1/(se^2 + tau^2), mu = sum wr est / sum wr, mu_se = sqrt(1 / sum wr),
 *   I^2 = clamp((Q - df) / Q, 0, 1) if Q > df and Q > 0 else 0.
 * Input: est[g * est_stride + c], se[g * se_stride + c], item g in [0, n_items), column c in [0, n_cols); set_offsets[n_sets + 1]
 * are contiguous item ranges, and a set is (item range s, column c): a call holds n_sets * n_cols sets.  n_cols = 1 with both
 * strides 1 is the plain vector call; n_cols = p, est = a GLM record batch with est_stride = its record length and se = its
 * inference batch with se_stride = 5 p shrinks every coefficient column in place, without a transpose.
 *   out[(g * n_cols + c) * 3]         {shrunken, shrunken_se, weight}; usable pair, tau^2 > 0: weight = (1/se^2) / (1/se^2 + 1/tau^2),
 *                                     shrunken = weight est + (1 - weight) mu, shrunken_se = sqrt(1 / (1/se^2 + 1/tau^2)); tau^2 = 0:
 *                                     {mu, mu_se, 0}; a pair that is not usable: NaN, NaN, NaN.  Items outside every set are not written.
 *   summary[(s * n_cols + c) * 8]     {mu, mu_se, tau_squared, i_squared, q, n_groups (= k), n_input (= the set's items), status}
 * Status per set: 0; ANOFOX_ERROR_INVALID_INPUT 1 for every set of a call whose options are invalid (an unknown method, a
 * tau_squared that is negative or infinite); ANOFOX_ERROR_NO_VALID_DATA 10 for a set without items; ANOFOX_ERROR_INSUFFICIENT_DATA
 * 6 for k < 2.  A status other than 0 makes the other seven summary fields and all the set's outputs NaN.
 * Two paths, chosen from n_sets, n_items and n_cols alone (the average set size): one wavefront per set, or, for few large
 * sets, chunk partials in a scratch added in a fixed order.  No atomics: repeated calls give identical bytes on either path.
 * Argument errors (false before any device is touched): a NULL pointer where there is something to read or write, n_cols = 0,
 * a stride smaller than n_cols, negative counts, and for the host form offsets that are not non-decreasing within [0, n_items].
 * The device form is asynchronous on the context's stream.
 * anofox_hip_eb_shrink_test_hooks (for tests; 0 restores the library's rule): force_path 1 = one wavefront per set, 2 = chunks;
 * chunk_items = the items of a chunk; max_workgroups = the most workgroups a launch starts.
 */
/* the batch entries' options: AnofoxEbShrinkOptions' layout (method: ANOFOX_TAU_DERSIMONIAN_LAIRD 0, ANOFOX_TAU_NONE 1), a type of
 * this header's own so that the batch surface stands next to the reference's header as well */
typedef struct {
	int method;
	double tau_squared; /* NaN: estimate it */
} AnofoxHipEbShrinkOptions;

ANOFOX_HIP_API size_t anofox_hip_eb_shrink_summary_len(void); /* 8 */
ANOFOX_HIP_API bool anofox_hip_eb_shrink_batch_device(AnofoxHipContext *ctx, int64_t n_sets, int64_t n_items, const int64_t *d_set_offsets,
                                       size_t n_cols, const double *d_est, int64_t est_stride, const double *d_se, int64_t se_stride,
                                       AnofoxHipEbShrinkOptions options, double *d_out, double *d_summary, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_eb_shrink_batch_host(AnofoxHipContext *ctx, int64_t n_sets, int64_t n_items, const int64_t *set_offsets,
                                     size_t n_cols, const double *est, int64_t est_stride, const double *se, int64_t se_stride,
                                     AnofoxHipEbShrinkOptions options, double *out, double *summary, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_eb_shrink_test_hooks(int force_path, int64_t chunk_items, int64_t max_workgroups);

/*
 * Grouped Pearson, Spearman and Kendall correlation with the test of no association (pearson_agg, spearman_agg, kendall_agg and
 * the three scalars above): R's cor.test with exact = FALSE in closed form.  The formulas: DESIGN.md §1 "Rank and product-moment
 * correlation" and csrc/rank_cor.h.
 * Input: row_offsets[n_groups + 1], group g owns rows [off[g], off[g + 1]) of x and y (n_rows doubles each).  A row is valid when
 * x and y are both not NaN (infinities stay in); n = a group's valid rows.
 * Output: records[g * 8] = {estimate (r, rho or tau), statistic (t; Kendall: z), p_value, ci_lower, ci_upper, n, s (Kendall's
 * concordant minus discordant pairs, exact; NaN otherwise), status}.
 * Status per group: 0; ANOFOX_ERROR_INSUFFICIENT_DATA 6 for n < 3, which makes every other field but n NaN.  A group whose valid
 * x or y is constant has status 0 with estimate, statistic, p_value and the interval NaN, for all three methods.
 * Pearson: two passes (means, then centred sums); t = r sqrt((n - 2) / (1 - r^2)) under Student's t with n - 2 degrees of
 * freedom, |r| = 1: t = +-inf and p = 0; interval tanh(atanh r -+ z / sqrt(n - 3)), z the normal quantile of
 * (1 + confidence_level) / 2, two-sided whatever the alternative, NaN at n = 3 and for a NaN confidence_level.  Spearman: the same
 * on the midranks.  Kendall: tau-b (default), tau-a or tau-c; z = s / sqrt(var) with R's tie-corrected variance under the normal
 * distribution; no interval.
 * Groups of up to 1462 rows are worked in LDS by one wavefront each; larger ones in the context's workspace (28 bytes per row of
 * the call), Kendall's pairs then spread over the whole device and added as integers.  Both paths give the same n, s and rho to
 * the bit; Pearson streams on one path whatever the size.
 * Argument errors (false before any device is touched): negative counts, a NULL array where there are groups, an unknown
 * method, alternative or tau type, a confidence level outside (0, 1) that is not NaN (all "correlation: ..."), and for the host
 * form offsets that are not non-decreasing within [0, n_rows].  The device form is asynchronous on the context's stream.
 * anofox_hip_cor_test_hooks (for tests): small_cap lowers the rows a group may have on the small path for later calls of the
 * process; 0 restores 1462.
 */
typedef struct {
	int32_t method;      /* 0 Pearson, 1 Spearman, 2 Kendall */
	int32_t alternative; /* AnofoxAlternative */
	int32_t tau_type;    /* AnofoxKendallType; read for every method */
	double confidence_level; /* in (0, 1); NaN: no interval */
} AnofoxHipCorBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_cor_record_len(void); /* 8 */
ANOFOX_HIP_API bool anofox_hip_cor_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                 const double *d_x, const double *d_y, AnofoxHipCorBatchOptions options, double *d_records,
                                 AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_cor_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets,
                               const double *x, const double *y, AnofoxHipCorBatchOptions options, double *records,
                               AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_cor_test_hooks(int64_t small_cap);

/*
 * Grouped rank-based location tests (mann_whitney_u_agg, wilcoxon_signed_rank_agg, kruskal_wallis_agg and the three scalars
 * above): R's wilcox.test(exact = FALSE) and kruskal.test in closed form.  The formulas: DESIGN.md §1 "Rank-based location tests"
 * and csrc/rank_tests.h.
 * Input: row_offsets[n_groups + 1], group g owns rows [off[g], off[g + 1]) of v (n_rows doubles), of y (doubles; Wilcoxon only,
 * otherwise it may be NULL) and of sample (int32; Mann-Whitney and Kruskal-Wallis only, otherwise it may be NULL).  A row is valid
 * when v is not NaN, for Wilcoxon when v - y - mu is not NaN (infinities stay in).  Mann-Whitney's first sample is sample == 0, its
 * second every other id; Kruskal-Wallis' ids are any int32.
 * Output: records[g * 8] = {statistic (W, V or H), z, p_value, df, n, n1, n2, status}: Mann-Whitney df NaN; Wilcoxon df NaN, n the
 * valid pairs, n1 the non-zero differences, n2 the zeros dropped; Kruskal-Wallis df = k - 1, n1 = k, n2 and z NaN.
 * Status per group: 0; ANOFOX_ERROR_INSUFFICIENT_DATA 6 (an empty sample; fewer than 2 valid pairs; N < 3 or k < 2), which makes
 * every field but the counts NaN.  A group without spread (every value tied, no non-zero difference) has status 0 with z (H) and
 * p_value NaN.  W, V and the counts are exact and the same on both size paths.
 * Groups of up to 1462 rows are worked in LDS by one wavefront each; larger ones in the context's workspace (28 bytes per row of
 * the call) by a workgroup of 1024 threads.
 * Argument errors (false before any device is touched): negative counts, an unknown test or alternative, a mu that is not finite,
 * a mu != 0 for Kruskal-Wallis, a NULL array where there are groups, a missing y (Wilcoxon) or sample (the others) (all "rank
 * test: ..."), and for the host form offsets that are not non-decreasing within [0, n_rows].  The device form is asynchronous on
 * the context's stream.
 * anofox_hip_rank_test_hooks (for tests): small_cap lowers the rows a group may have on the small path for later calls of the
 * process; 0 restores 1462.
 */
typedef struct {
	int32_t test;        /* 0 Mann-Whitney, 1 Wilcoxon signed-rank, 2 Kruskal-Wallis */
	int32_t alternative; /* AnofoxAlternative; not read by Kruskal-Wallis */
	int32_t continuity_correction; /* 0: none */
	double mu;           /* the hypothesised shift; 0 for Kruskal-Wallis */
} AnofoxHipRankTestBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_rank_test_record_len(void); /* 8 */
ANOFOX_HIP_API bool anofox_hip_rank_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                       const double *d_v, const double *d_y, const int32_t *d_sample,
                                       AnofoxHipRankTestBatchOptions options, double *d_records, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_rank_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets,
                                     const double *v, const double *y, const int32_t *sample,
                                     AnofoxHipRankTestBatchOptions options, double *records, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_rank_test_hooks(int64_t small_cap);

/*
 * Grouped parametric and studentised-rank tests (t_test_agg, yuen_agg, one_way_anova_agg, brown_forsythe_agg, brunner_munzel_agg and
 * the five scalars above): R's t.test, Yuen's test, oneway.test, the median-centred Levene test and brunner.munzel.test in closed
 * form.  The formulas: DESIGN.md §1 "Parametric and studentised-rank tests" and csrc/sample_tests.h.
 * Input: the layout of the rank tests: row_offsets[n_groups + 1], v (n_rows doubles), y (doubles; the paired t-test only, otherwise
 * it may be NULL) and sample (int32; every other test, NULL for the paired t-test).  A row is valid when v is not NaN, for the
 * paired t-test when v - y - mu is not NaN (infinities stay in).  The two-sample tests (t, Yuen, Brunner-Munzel) take sample == 0
 * as sample 1 and every other id as sample 2; the k-sample tests (ANOVA, Brown-Forsythe) take any int32 ids.
 * Output: records[g * 12] = {statistic, p_value, df, df2, estimate, ci_lower, ci_upper, n, n1, n2, aux, status}.  t-test and Yuen:
 * estimate the difference of the (trimmed) means, aux its standard error; the paired t-test: n = n1 = n2 = the valid pairs.
 * ANOVA and Brown-Forsythe: statistic F on (df, df2), estimate SSB, aux SSW, n1 = k, n2 and the interval NaN.  Brunner-Munzel:
 * estimate phat = P(X1 < X2) + P(X1 = X2) / 2 with its two-sided interval, aux its standard error.
 * Status per group: 0; ANOFOX_ERROR_INSUFFICIENT_DATA 6 (an arm below 2 rows; Yuen: below 4, or fewer than 2 left after trimming;
 * fewer than 2 valid pairs; k < 2), which makes every field but the counts NaN.  A zero standard error has status 0 with statistic,
 * p_value, df and the interval NaN; SSW = 0 gives F = +inf, p = 0 (NaN when SSB = 0 too); complete separation gives Brunner-Munzel's
 * statistic +-inf, p 0 or 1, df NaN and the interval [phat, phat].
 * The t-test streams each group twice by one wavefront and stages nothing; the other tests work groups of up to 1462 rows in LDS
 * by one wavefront each, larger ones in the context's workspace (28 bytes per row of the call) by a workgroup of 1024 threads.
 * Argument errors (false before any device is touched): negative counts, an unknown test, kind or alternative, a mu that is not
 * finite, a mu != 0 for a test other than the t-test, a trim outside [0, 0.5), a confidence level outside (0, 1) that is not NaN
 * (NaN: no interval), a NULL array where there are groups, a missing y (paired) or sample (the others) (all "sample test: ..."), and
 * for the host form offsets that are not non-decreasing within [0, n_rows].  The device form is asynchronous on the context's
 * stream.
 * anofox_hip_sample_test_hooks (for tests): small_cap lowers the rows a group may have on the small path for later calls of this
 * family in the process (the rank test and correlation families keep theirs); 0 restores 1462.
 */
typedef struct {
	int32_t test;        /* 0 t-test, 1 Yuen, 2 one-way ANOVA, 3 Brown-Forsythe, 4 Brunner-Munzel */
	int32_t alternative; /* AnofoxAlternative; not read by ANOVA and Brown-Forsythe */
	int32_t kind;        /* t-test: 0 Welch, 1 Student, 2 paired; ANOVA: 0 Fisher, 1 Welch; otherwise 0 */
	double mu;           /* the t-test's hypothesised difference; 0 otherwise */
	double trim;         /* Yuen's trimming proportion, in [0, 0.5) */
	double confidence_level; /* in (0, 1); NaN: no interval */
} AnofoxHipSampleTestBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_sample_test_record_len(void); /* 12 */
ANOFOX_HIP_API bool anofox_hip_sample_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                         const double *d_v, const double *d_y, const int32_t *d_sample,
                                         AnofoxHipSampleTestBatchOptions options, double *d_records, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_sample_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets,
                                       const double *v, const double *y, const int32_t *sample,
                                       AnofoxHipSampleTestBatchOptions options, double *records, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_sample_test_hooks(int64_t small_cap);

/*
 * Grouped normality tests (shapiro_wilk_agg, dagostino_k2_agg, jarque_bera_agg and the three scalars above): the Shapiro-Wilk test
 * as Royston's Algorithm AS R94 (R's swilk.c, scipy.stats.shapiro), D'Agostino's K2 as scipy.stats.normaltest, and the Jarque-Bera
 * test.  The formulas: DESIGN.md §1 "Normality tests" and csrc/normality_tests.h.
 * Input: row_offsets[n_groups + 1], group g owns rows [off[g], off[g + 1]) of v (n_rows doubles).  A row is valid when v is not NaN;
 * infinities stay in and make the moments (and W) NaN.  n = a group's valid rows.
 * Output: records[g * 8] = {statistic (W, K2 or JB), p_value, skewness, kurtosis (excess), z_skewness, z_kurtosis, n, status}.
 * Shapiro-Wilk defines the first two, Jarque-Bera the first four, K2 all six; a field a test does not define is NaN.
 * Status per group: 0; ANOFOX_ERROR_INSUFFICIENT_DATA 6 (Shapiro-Wilk and Jarque-Bera n < 3, K2 n < 8); ANOFOX_ERROR_INVALID_INPUT 1
 * (Shapiro-Wilk n > 5000; K2 and Jarque-Bera of values that are all equal, m2 <= 0).  Either makes every field but n NaN.
 * Shapiro-Wilk of values that are all equal has status 0 with W = 1 and p = 1.
 * Jarque-Bera and K2 stream each group twice by one wavefront and stage nothing; Shapiro-Wilk works groups of up to 1462 rows in LDS
 * by one wavefront each, larger ones in the context's workspace (28 bytes per row of the call) by a workgroup of 1024 threads,
 * and gives the same W to the bit on both paths.
 * Argument errors (false before any device is touched): negative counts, an unknown test, a NULL array where there are groups
 * (all "normality test: ..."), and for the host form offsets that are not non-decreasing within [0, n_rows].  The device form is
 * asynchronous on the context's stream.
 * anofox_hip_normality_test_hooks (for tests): small_cap lowers the rows a group may have on the small path for later calls of
 * this family in the process (the correlation, rank test and sample test families keep theirs); 0 restores 1462.
 */
typedef struct {
	int32_t test; /* 0 Shapiro-Wilk, 1 D'Agostino K2, 2 Jarque-Bera */
	int32_t reserved; /* padding to 8 bytes; not read */
} AnofoxHipNormalityTestBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_normality_test_record_len(void); /* 8 */
ANOFOX_HIP_API bool anofox_hip_normality_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                            const double *d_v, AnofoxHipNormalityTestBatchOptions options, double *d_records,
                                            AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_normality_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets,
                                          const double *v, AnofoxHipNormalityTestBatchOptions options, double *records,
                                          AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_normality_test_hooks(int64_t small_cap);

/*
 * Grouped categorical tests (chisq_test_agg, g_test_agg, fisher_exact_agg, mcnemar_agg, cramers_v_agg, phi_coefficient_agg,
 * contingency_coef_agg and the scalars above): the chi-square test of independence with Cramer's V, Pearson's C and phi, the
 * G-test, Fisher's exact test of a 2 x 2 table as R's fisher.test, and McNemar's test.  The formulas: DESIGN.md §1 "Categorical
 * tests" and csrc/categorical_tests.h.
 * Input: row_offsets[n_groups + 1], group g owns rows [off[g], off[g + 1]) of the int32 columns a (the row variable) and b (the
 * column variable), n_rows each.  A row is valid unless either entry is INT32_MIN, the NULL of this family; every other int32 is
 * a label.
 * Output: records[g * 12] = {statistic, p_value, df, estimate, ci_lower, ci_upper, n, n_row_levels, n_col_levels, aux, aux2,
 * status}.
 *   test 0, chi-square: X2 (Yates' form with `correction` on a 2 x 2 table, the correction clipped to |O - E|), df = (r - 1)(c - 1),
 *     estimate = Cramer's V, aux = Pearson's C, aux2 = phi (2 x 2 tables, signed by ascending label order; else NaN), all three
 *     from the uncorrected X2.  The table is that of the distinct labels: there are no empty margins.
 *   test 1, G: 2 sum O ln(O/E); estimate, aux, aux2 NaN.
 *   test 2, Fisher: only rows with both labels in {0, 1} are counted.  statistic = the sample odds ratio, p for `alternative`
 *     (two-sided: the probabilities <= the observed one times 1 + 1e-7), estimate = the conditional maximum-likelihood odds ratio,
 *     ci_lower / ci_upper its exact interval at confidence_level (NaN: none; one-sided for a one-sided alternative), df NaN, the
 *     level counts 2.
 *   test 3, McNemar: a label of 0 against every other label; b = n01, c = n10.  (|b - c| - 1)^2/(b + c) with `correction`, else
 *     (b - c)^2/(b + c), df 1; with `exact` the binomial p min(1, 2 P(X <= min(b, c))), statistic and df NaN.  estimate = b/c,
 *     aux = b, aux2 = c, the level counts 2.  b + c = 0: status 0, statistic and p NaN.
 *   The interval fields are NaN but for Fisher.
 * Status per group: 0; ANOFOX_ERROR_INSUFFICIENT_DATA 6 (no valid row; tests 0 and 1: fewer than 2 distinct labels on either
 * side; tests 2 and 3: no counted row), which makes every field but n and the two level counts NaN.
 * Fisher and McNemar stream each group once by one wavefront and stage nothing; the chi-square and the G-test work groups of up to
 * 1462 rows in LDS by one wavefront each, larger ones in the context's workspace (28 bytes per row of the call) by a workgroup of
 * 1024 threads, and give the same record to the bit on both paths.  No dense table is built: the number of labels is bounded by
 * the rows alone.
 * Argument errors (false before any device is touched, all "categorical test: ..."): negative counts, an unknown test or
 * alternative, a confidence level outside (0, 1) that is not NaN, a NULL array where there are groups, and for the host form
 * offsets that are not non-decreasing within [0, n_rows].  The device form is asynchronous on the context's stream.
 * anofox_hip_categorical_test_hooks (for tests): small_cap lowers the rows a group may have on the small path for later calls of
 * this family in the process (the other families keep theirs); 0 restores 1462.
 */
typedef struct {
	int32_t test;        /* 0 chi-square, 1 G, 2 Fisher exact, 3 McNemar */
	int32_t alternative; /* AnofoxAlternative; read by Fisher */
	int32_t correction;  /* != 0: Yates (chi-square, 2 x 2) / Edwards (McNemar) */
	int32_t exact;       /* != 0: McNemar's binomial p */
	double confidence_level; /* Fisher's interval; NaN: none */
} AnofoxHipCategoricalTestBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_categorical_test_record_len(void); /* 12 */
ANOFOX_HIP_API bool anofox_hip_categorical_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                              const int32_t *d_a, const int32_t *d_b, AnofoxHipCategoricalTestBatchOptions options,
                                              double *d_records, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_categorical_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets,
                                            const int32_t *a, const int32_t *b, AnofoxHipCategoricalTestBatchOptions options,
                                            double *records, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_categorical_test_hooks(int64_t small_cap);

/*
 * Grouped permutation tests (energy_distance_agg, mmd_agg, permutation_t_test_agg and the three scalars below): the energy
 * distance test (R's eqdist.etest, the V-statistic), the permutation Welch t-test and the biased Gaussian-kernel MMD^2, each with
 * p = (1 + n_extreme) / (B + 1) over B random relabellings.  The statistics, the permutation stream (a function of seed,
 * permutation and row alone) and the order of every sum: DESIGN.md §1 "Permutation tests" and csrc/perm_tests.h.
 * Input: the layout of the rank tests: row_offsets[n_groups + 1], v (n_rows doubles) and sample (int32).  A row is valid when v is
 * not NaN; sample 1 is sample == 0, sample 2 every other id.
 * Output: records[g * 8] = {statistic, p_value, aux, n_extreme, n, n1, n2, status}: aux is Welch's df of the observed split
 * (t-test), sigma (MMD) or NaN (energy distance); n_extreme the permutations at least as extreme as the observed statistic.
 * n_permutations = 0: the statistic alone, p_value NaN.
 * Status per group: 0; ANOFOX_ERROR_INSUFFICIENT_DATA 6 (n1 < 2, n2 < 2, or an infinity among the values); 7 ("mmd: group too
 * large"): an MMD group of more than 1462 rows, because MMD costs O(N^2) per permutation and is built on the small path only.  A
 * status that is not 0 makes every field but the counts NaN.  An observed t without variance, or a sigma of 0 (more than half of the
 * pairs tied), has status 0 with statistic and p_value NaN.
 * A group's record depends on its rows, the options and the seed alone: not on its place in the call, and, for the energy
 * distance and the t-test, not on the size path (statistic and n_extreme are the same to the bit).
 * Argument errors (false before any device is touched): negative counts, an unknown test or alternative, n_permutations outside
 * [0, 1000000], an infinite sigma, a NULL array where there are groups (all "permutation test: ..."), and for the host form offsets
 * that are not non-decreasing within [0, n_rows].  The device form is asynchronous on the context's stream.
 * anofox_hip_perm_test_hooks (for tests): small_cap lowers the rows a group may have on the small path for later calls of the
 * process; 0 restores 1462.
 */
typedef struct {
	int32_t test;        /* 0 energy distance, 1 permutation t-test, 2 MMD */
	int32_t alternative; /* AnofoxAlternative; read by the t-test alone */
	int64_t n_permutations;
	uint64_t seed;
	double sigma;        /* MMD's kernel width; NaN or <= 0: the median heuristic */
} AnofoxHipPermTestBatchOptions;

ANOFOX_HIP_API size_t anofox_hip_perm_test_record_len(void); /* 8 */
ANOFOX_HIP_API bool anofox_hip_perm_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                       const double *d_v, const int32_t *d_sample, AnofoxHipPermTestBatchOptions options,
                                       double *d_records, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_perm_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets,
                                     const double *v, const int32_t *sample, AnofoxHipPermTestBatchOptions options, double *records,
                                     AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_perm_test_hooks(int64_t small_cap);

/*
 * Grouped Gaussian linear mixed models with one random intercept (glmm_fit_agg): per panel  y_ij = a_ij'beta + b_j + e_ij,
 * b_j ~ N(0, var_group), e ~ N(0, var_residual), fitted by profiled REML or ML.  The contract, the formulas and what is not
 * built: DESIGN.md §1 "Linear mixed models" and csrc/lmm_profile.h.
 * Input: the grouped-columns layout with one more layer of offsets; rows are sorted by (panel, level).
 *   panel_level_offsets[n_panels + 1]  panel g owns levels [plo[g], plo[g + 1]); plo[0] = 0 and plo[n_panels] = n_levels
 *   level_row_offsets[n_levels + 1]    level l owns rows [lro[l], lro[l + 1])
 *   y, x_cols[j]                       n_rows doubles each, NaN = NULL; a row is valid when y and every x are finite
 * Output:
 *   glmm[g * (p + 13)]      { coefficients[p], intercept (NaN without one), var_group, var_residual, icc, log_likelihood, aic, bic,
 *                             deviance (= -2 log_likelihood), n_observations, n_groups (levels with a valid row), iterations
 *                             (evaluations of the search loop), converged, status }
 *   inference[g * (5 p + 1)] { se[p], z[p], p[p], ci_lower[p], ci_upper[p], intercept_std_error }, normal-based; may be NULL
 *   ranef[n_levels]          the BLUP of every level; NaN for a level without a valid row and for a failed panel
 *   level_n[n_levels]        valid rows per level (int64); may be NULL
 * Status per panel: 0; 1 invalid options (every panel of the call: a tolerance that is not finite and positive, max_iterations
 * = 0, a confidence_level outside (0, 1) with inference), fewer than two non-empty levels, or every non-empty level with one
 * row; 10 no valid row; 6 n <= k + 1.  A status other than 0 makes every other field NaN.  theta^ = 0 (the score is not
 * positive at the lower end of the bracket [1e-10, 1e10]): var_group = icc = 0.0, BLUPs 0.0, beta the pooled fit, converged = 1.
 * A search that ends on the upper end: converged = 0, status 0.  A column that is aliased (or constant next to an intercept)
 * is dropped by the pivot rule: NaN coefficient and inference, and k counts the kept columns.
 * Two stages on the context's stream: level statistics (one wavefront per chunk of 64 levels) and the profile search (one
 * workgroup of 1, 4 or 16 wavefronts per panel, by its level count: <= 64, <= 1024, more).  No atomics: repeated calls give
 * identical bytes, and a panel's bytes do not depend on the other panels of the call.
 * Argument errors (false before any device is touched): NULL pointers where there is something to read or write, n_features
 * outside [1, 32], negative counts, a family other than ANOFOX_GLMM_GAUSSIAN ("glmm: ... is not built"), and for the host form
 * offsets that are not non-decreasing or do not cover [0, n_levels] and stay within [0, n_rows].  The device form is
 * asynchronous; x_cols is a host array of device pointers, as in the other families.
 * anofox_hip_glmm_test_hooks (for measurements and tests; 0 restores the library's rule): stats_only != 0 makes a call stop
 * after the level statistics, so that the stage can be timed alone (the outputs are then not written); wave_mask (bit 0, 1, 2:
 * the search launch of 1, 4, 16 wavefronts) keeps the device form from making the other launches, whose workgroups would find
 * no panel of their size: panels of a size that is masked out are then not fitted.
 */
typedef struct {
	int family; /* ANOFOX_GLMM_GAUSSIAN 0 */
	int fit_intercept;
	int reml;
	uint32_t max_iterations;
	double tolerance;
	int compute_inference;
	double confidence_level;
} AnofoxHipGlmmOptions;

ANOFOX_HIP_API size_t anofox_hip_glmm_record_len(size_t n_features);    /* p + 13 */
ANOFOX_HIP_API size_t anofox_hip_glmm_inference_len(size_t n_features); /* 5 p + 1 */
ANOFOX_HIP_API void anofox_hip_glmm_test_hooks(int stats_only, int wave_mask);
ANOFOX_HIP_API bool anofox_hip_glmm_fit_batch_device(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features,
                                      int64_t n_rows, const int64_t *d_panel_level_offsets, const int64_t *d_level_row_offsets,
                                      const double *d_y, const double *const *d_x_cols, AnofoxHipGlmmOptions options, double *d_glmm,
                                      double *d_inference, double *d_ranef, int64_t *d_level_n, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glmm_fit_batch_host(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features,
                                    int64_t n_rows, const int64_t *panel_level_offsets, const int64_t *level_row_offsets,
                                    const double *y, const double *const *x_cols, AnofoxHipGlmmOptions options, double *glmm,
                                    double *inference, double *ranef, int64_t *level_n, AnofoxError *out_error);

/*
 * Mixed-model fit-predict (glmm_fit_predict_agg): the fit above and, in the same call, a score of every row of
 * [lro[0], lro[n_levels]).  glmm, inference, ranef and level_n are byte for byte those of anofox_hip_glmm_fit_batch_* on the
 * same inputs.  A row of level j of a panel with status 0 whose x are all finite is scored whether or not its y is finite (a row
 * with y = NaN is a prediction row; the fit drops it).  With s_j = theta^ lambda_j (0, like the BLUP b^_j, for a level without a
 * valid row), abar_j the level's mean design row, A = X'V^-1 X over the kept columns and s2 = var_residual:
 *   pred[i * 5] = { yhat = yhat_fixed + b^_j,  yhat_fixed = a_i'beta^ (what a new level gets),
 *                   se = sqrt(s2 [c'A^-1 c + theta^ / (1 + n_j theta^)]),  c = a_i - s_j abar_j,  lower, upper }
 * se^2 is the variance of the prediction error (a'beta^ + b^_j) - (a'beta + b_j) at known theta (csrc/lmm_profile.h has the
 * derivation).  interval 0: lower = upper = NaN; 1 (confidence): yhat -+ z se; 2 (prediction): yhat -+ z sqrt(se^2 + s2);
 * z the normal quantile of 1/2 + level / 2.  A column dropped by the pivot rule contributes nothing.  All five values are NaN
 * for a row with an x that is not finite and for every row of a panel whose status is not 0.  Rows outside
 * [lro[0], lro[n_levels]) are not written.
 * Argument errors (false before any device is touched): the fit's own; pred NULL with n_panels > 0 ("pred is NULL"); an
 * interval outside {0, 1, 2} ("glmm: interval must be 0, 1 or 2"); with interval != 0 a level that is NaN or outside the open
 * (0, 1) ("glmm: level must be in (0, 1)").  anofox_hip_glmm_test_hooks applies: after stats_only nothing is scored, and the rows
 * of a panel whose search launch is masked out are NaN.  No atomics; a panel's rows do not depend on the other panels.
 */
typedef struct {
	int interval; /* 0 none, 1 confidence, 2 prediction */
	double level;
} AnofoxHipGlmmPredictOptions;

ANOFOX_HIP_API size_t anofox_hip_glmm_pred_len(void); /* 5: yhat, yhat_fixed, se, lower, upper */
ANOFOX_HIP_API bool anofox_hip_glmm_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features,
                                              int64_t n_rows, const int64_t *d_panel_level_offsets,
                                              const int64_t *d_level_row_offsets, const double *d_y, const double *const *d_x_cols,
                                              AnofoxHipGlmmOptions options, AnofoxHipGlmmPredictOptions predict, double *d_glmm,
                                              double *d_inference, double *d_ranef, int64_t *d_level_n, double *d_pred,
                                              AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_glmm_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features,
                                            int64_t n_rows, const int64_t *panel_level_offsets, const int64_t *level_row_offsets,
                                            const double *y, const double *const *x_cols, AnofoxHipGlmmOptions options,
                                            AnofoxHipGlmmPredictOptions predict, double *glmm, double *inference, double *ranef,
                                            int64_t *level_n, double *pred, AnofoxError *out_error);

/*
 * Grouped variance inflation factors: the Finalize loop of vif_agg (src/aggregate_functions/vif_aggregate.cpp:
 * 144-185) in one call.  x_cols as in the fit entry points (rows of a group contiguous; the aggregate's Update
 * has already dropped NULL rows and NaN values, :67-93).  d_vif[g] = { vif[n_features], status }
 * (anofox_hip_vif_record_len doubles): status 100 = fewer than 3 rows -> SQL NULL (:154), 0 otherwise.
 * n_features <= 8 uses one pass over the rows; up to anofox_hip_vif_max_features() = 129 one grouped fit per feature.
 */
ANOFOX_HIP_API size_t anofox_hip_vif_record_len(size_t n_features);
ANOFOX_HIP_API size_t anofox_hip_vif_max_features(void);
ANOFOX_HIP_API bool anofox_hip_vif_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                 const int64_t *d_row_offsets, const double *const *x_cols, double *d_vif,
                                 AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_vif_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                               const int64_t *row_offsets, const double *const *x_cols, double *vif,
                               AnofoxError *out_error);

/*
 * Grouped residual diagnostics: the Finalize loop of residuals_diagnostics_agg
 * (src/aggregate_functions/residuals_diagnostics_aggregate.cpp:213-286) in one call.  Per row r the record
 * d_out[4 r ..] = { raw, standardized, studentized, leverage } (NaN where the part is absent); per group
 * d_group[2 g ..] = { rows used, ANOFOX_HIP_RESIDUALS_HAS_* flags }.  With drop_nan_rows the rows whose y or
 * y_hat is NaN are left out, as the aggregate's Update does (:154-163; their records are all NaN); the aggregate
 * itself returns NULL for groups with fewer than 3 used rows (:223) and passes no residual standard error (:232),
 * so d_rse (one value per group, NaN = none) may be NULL.  x_cols / n_features may be NULL / 0 (no leverage);
 * n_features <= anofox_hip_residuals_max_features() = 128 (up to 8: one wavefront per group, residuals_narrow.hip;
 * 9 .. 128: one workgroup per group, residuals_wide.hip).
 */
#define ANOFOX_HIP_RESIDUALS_HAS_STANDARDIZED 1
#define ANOFOX_HIP_RESIDUALS_HAS_STUDENTIZED 2
#define ANOFOX_HIP_RESIDUALS_HAS_LEVERAGE 4
ANOFOX_HIP_API size_t anofox_hip_residuals_max_features(void);
ANOFOX_HIP_API bool anofox_hip_residuals_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                       const int64_t *d_row_offsets, const double *d_y, const double *d_y_hat,
                                       const double *const *x_cols, const double *d_rse, bool include_studentized,
                                       bool drop_nan_rows, double *d_out, double *d_group, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_residuals_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                     const int64_t *row_offsets, const double *y, const double *y_hat,
                                     const double *const *x_cols, const double *rse, bool include_studentized,
                                     bool drop_nan_rows, double *out, double *group, AnofoxError *out_error);

/*
 * Streaming aggregate state: the Update / Combine / Finalize callbacks of the three aggregates
 * (src/aggregate_functions/ols_aggregate.cpp:120-186,189-234,249-338; ridge_aggregate.cpp:124-345;
 * wls_aggregate.cpp:122-362) with the state kept on the GPU.  The reference buffers every row of every group on
 * the host until Finalize; here ONE object holds an O(p^2) moment record per "slot" (= one DuckDB aggregate state:
 * the shim's Initialize hands out slot numbers 0, 1, 2, ...) and rows are folded in as they arrive, in any order:
 *
 *   update    n_rows rows in arrival order: slot[i] (state of row i), y[i], x_rowmajor[i * p .. i * p + p) (the LIST
 *             child as DuckDB delivers it), w[i] (WLS), valid[i] (optional; 0 = the row Update skips: NULL y, NULL x
 *             list or NULL weight, ols_aggregate.cpp:150-159, wls_aggregate.cpp:160-166).  NULL list ELEMENTS are
 *             passed as NaN (the row filter of the fit drops such rows, ols.rs:59-66).  n_slots = number of slots
 *             handed out so far (every slot[i] < n_slots; the state grows to it).  The feature count is fixed at
 *             creation — the shim keeps the reference's "Inconsistent feature count" check (ols_aggregate.cpp:165-175).
 *             _host: pageable or pinned host memory (anofox_hip_host_alloc), staged through the GPU in chunks with the
 *             copy of one chunk overlapping the kernels of the previous one; returns when the inputs may be reused.
 *             _device: device pointers, asynchronous on the context's stream.
 *   combine   pairs (source slot, target slot) as Combine receives them: the source's rows count as arriving AFTER
 *             the target's (ols_aggregate.cpp:224-233) and the source is emptied; a slot may take part in one pair
 *             per call.
 *   finalize  fit records of slots [0, n_slots) exactly as anofox_hip_fit_batch_* lays them out (status 100 for
 *             fewer than 2 accumulated rows, ols_aggregate.cpp:263-267).  The rows are gone, so the batch path's
 *             refinement passes (re-reading the rows of ill-conditioned or exactly fitting groups) cannot run
 *             unless a row log is kept (below).  A group that would have taken them — smallest Cholesky pivot ratio
 *             below 1e-3 or rss / tss below 1e-7: its coefficients would carry cond^2 eps and its sigma / r^2 the
 *             cancellation of rss = tss - |z|^2 — is NOT handed out as a number: its record is NaN with status
 *             ANOFOX_HIP_STATUS_UNREFINED (101 -> SQL NULL).  *out_unrefined (optional) is the number of such groups
 *             and out_unrefined_slots (optional, room for n_slots entries) receives their slot numbers, in no
 *             particular order.  Every other record meets the batch entry points' tolerances.
 *   retain_rows(max_bytes)  (optional, before the first update) keeps every chunk in a row log in HBM as well — p + 2 (+ 1
 *             with weights) doubles and 5 bytes per row, up to max_bytes — and Finalize then refits exactly the groups
 *             its solve queued, through the batch path (accumulate, solve, refinement passes) on their logged rows:
 *             *out_unrefined is 0 and every group has the batch entry points' accuracy.  Combine re-labels the source
 *             slots' logged rows.  Exceeding max_bytes (or device memory) is not an error: the log continues in
 *             page-locked host memory up to retain_rows_host's max_host_bytes (the kernels of Finalize read those
 *             slabs over PCIe: 5 bytes per row for the selection, the queued groups' rows for the refit); beyond
 *             both budgets the log is dropped, anofox_hip_agg_state_retaining() turns 0 and Finalize flags the queued
 *             groups as without a log.  finalize_device synchronises the stream once when a log is kept.
 *   log-only  Designs of more than 8 features have no moment record to stream into, and HC standard errors (hc_type
 *             other than none, with inference, OLS / WLS) need a second pass over the rows: such a state keeps ONLY the
 *             row log — the reference's row buffers, in HBM — and Finalize runs the batch path over all of it.  Same
 *             entry points and results as above (*out_unrefined is 0); retain_rows(max_bytes) caps the HBM part of the
 *             log (0 = no cap), retain_rows_host its host part, and an Update that exceeds both (or the memory itself)
 *             FAILS with ANOFOX_ERROR_ALLOCATION_FAILURE.
 *
 *   other families  the elastic net and the bounded / non-negative least squares are finalized from the same state
 *             (anofox_hip_agg_state_finalize_elasticnet_* / _bls_*, below): the state does not depend on their options.
 *
 * A state belongs to one context (device + stream); calls on one state are serialised.  n_features <=
 * anofox_hip_agg_state_max_features() = 128.
 */
typedef struct AnofoxHipAggState AnofoxHipAggState;
ANOFOX_HIP_API size_t anofox_hip_agg_state_max_features(void);
ANOFOX_HIP_API bool anofox_hip_agg_state_create(AnofoxHipContext *ctx, size_t n_features, AnofoxHipBatchOptions options,
                                 int64_t initial_slots, AnofoxHipAggState **out_state, AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_agg_state_destroy(AnofoxHipAggState *state);
ANOFOX_HIP_API bool anofox_hip_agg_state_reserve(AnofoxHipAggState *state, int64_t n_slots, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_retain_rows(AnofoxHipAggState *state, size_t max_bytes, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_retain_rows_host(AnofoxHipAggState *state, size_t max_host_bytes, AnofoxError *out_error);
ANOFOX_HIP_API int anofox_hip_agg_state_retaining(const AnofoxHipAggState *state);          /* 1 while a row log is kept */
ANOFOX_HIP_API size_t anofox_hip_agg_state_retained_bytes(const AnofoxHipAggState *state);  /* HBM held by the log */
ANOFOX_HIP_API size_t anofox_hip_agg_state_retained_host_bytes(const AnofoxHipAggState *state); /* page-locked host memory held by it */
ANOFOX_HIP_API int64_t anofox_hip_agg_state_slots(const AnofoxHipAggState *state);
ANOFOX_HIP_API int64_t anofox_hip_agg_state_rows(const AnofoxHipAggState *state);
ANOFOX_HIP_API bool anofox_hip_agg_state_update_host(AnofoxHipAggState *state, int64_t n_rows, int64_t n_slots, const uint32_t *slot,
                                      const double *y, const double *x_rowmajor, const double *w, const uint8_t *valid,
                                      AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_update_device(AnofoxHipAggState *state, int64_t n_rows, int64_t n_slots, const uint32_t *d_slot,
                                        const double *d_y, const double *d_x_rowmajor, const double *d_w, const uint8_t *d_valid,
                                        AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_combine(AnofoxHipAggState *state, int64_t n_pairs, const uint32_t *source_slots,
                                  const uint32_t *target_slots, AnofoxError *out_error);
/* combine with preserve_sources = true leaves the sources as they are (DuckDB's AggregateCombineType::PRESERVE_INPUT: a
 * window segment tree combines one node into many frames); the same source may then feed several targets of a call.
 * (r4) A row log — and the rows of a log-only state — follow: every target gets its own copies of its sources' logged rows
 * (the reference's Combine copies the row buffers as well, ols_aggregate.cpp:224-233), appended behind the target's own, so
 * that Finalize refits exactly fitting or ill-conditioned frames as it does for a GROUP BY.  More than 2^24 rows to copy in ONE
 * call is not a window frame's Combine: a moment state then gives its log up (flagged groups), a log-only state reports an error. */
ANOFOX_HIP_API bool anofox_hip_agg_state_combine_ex(AnofoxHipAggState *state, int64_t n_pairs, const uint32_t *source_slots,
                                     const uint32_t *target_slots, bool preserve_sources, AnofoxError *out_error);
/* Finalize of the listed (distinct) slots only: record k belongs to slots[k].  Same records as finalize_host. */
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_slots_host(AnofoxHipAggState *state, int64_t n_list, const uint32_t *slots, double *core,
                                              double *inference, int64_t *out_unrefined, AnofoxError *out_error);
/* Destroy of aggregate states (ols_aggregate.cpp:108-118): the listed slots become empty and may be handed out again. */
ANOFOX_HIP_API bool anofox_hip_agg_state_release_slots(AnofoxHipAggState *state, int64_t n_list, const uint32_t *slots, AnofoxError *out_error);
/* (r4) Cross-device Combine of moment states (n_features <= 8, no HC errors): the DuckDB glue shards a query's aggregate states
 * over the node's GPUs by hash, and Combine (ols_aggregate.cpp:189-234) may pair a source on one device with a
 * target on another.  export copies the listed slots' records out as the device keeps them — record_len() doubles and the
 * accepted-row count per slot; import overwrites the listed (distinct) slots of ANOTHER state of the same width and options with
 * them, after which an ordinary combine merges them into their targets.  Rows kept in a row log do not travel: both calls give
 * the state's log up, and a group its moments cannot resolve is then flagged by Finalize (status 101), never handed out.
 * Log-only states (wider designs, HC errors) refuse both: they stay on one device. */
/* (r4) Back to the state as created (every slot empty, the row log released, slots() = 0), device buffers kept: between two
 * executions of a prepared statement whose bind data — and with it the query's device state — DuckDB re-uses. */
ANOFOX_HIP_API bool anofox_hip_agg_state_reset(AnofoxHipAggState *state, AnofoxError *out_error);
ANOFOX_HIP_API size_t anofox_hip_agg_state_record_len(const AnofoxHipAggState *state);
ANOFOX_HIP_API bool anofox_hip_agg_state_export_slots_host(AnofoxHipAggState *state, int64_t n_list, const uint32_t *slots, double *records,
                                            int64_t *counts, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_import_slots_host(AnofoxHipAggState *state, int64_t n_list, const uint32_t *slots, const double *records,
                                            const int64_t *counts, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_host(AnofoxHipAggState *state, int64_t n_slots, double *core, double *inference,
                                        int64_t *out_unrefined, int32_t *out_unrefined_slots, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_device(AnofoxHipAggState *state, int64_t n_slots, double *d_core, double *d_inference,
                                          AnofoxError *out_error);
/*
 * Elastic net and bounded / non-negative least squares from a streaming state.  A state is independent of lambda, l1_ratio and
 * the bounds, so one pass over the rows serves the regression Finalize above and any number of these; each of them is READ-ONLY
 * (moments, row log and slots stay as they are) and two calls with the same options return identical bits.  The state must have
 * been created with model = OLS (no weights), hc_type = none and the fit_intercept of the family's options; anything else is
 * ANOFOX_ERROR_INVALID_INPUT naming the mismatch, and nothing is launched.  Records and iteration counts (iterations may be
 * NULL) as anofox_hip_elasticnet_fit_batch_* (p + 6) / anofox_hip_bls_fit_batch_* (anofox_hip_bls_record_len(p)); status 100
 * for fewer than 2 accumulated rows; unusable BLS bounds give status 1 to every other slot.
 *   n_features <= 8   the family's solve on the moment records.  It flags the slots whose moment-form ssr has cancelled (the
 *                     batch path sums those residuals from the rows): with a row log exactly their logged rows go through the
 *                     batch path and *out_unrefined is 0; without one (or once it was dropped) their records are NaN with status
 *                     ANOFOX_HIP_STATUS_UNREFINED, counted in *out_unrefined and listed (ascending) in out_unrefined_slots
 *                     (optional, room for n_slots entries).
 *   9 .. 128          log-only states: the batch path with the family's solve over the whole log; *out_unrefined is 0.
 * _device: device buffers, asynchronous on the context's stream except that a kept row log synchronises it once.
 * _slots_host: the listed (distinct) slots only, record k belongs to slots[k]; the same bits as those rows of the full call,
 *              except slots refitted from the row log, which agree to rounding (the refit's batch of rows is another one).
 */
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_elasticnet_host(AnofoxHipAggState *state, int64_t n_slots, AnofoxHipElasticNetBatchOptions options,
                                                   double *core, int32_t *iterations, int64_t *out_unrefined, int32_t *out_unrefined_slots,
                                                   AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_elasticnet_device(AnofoxHipAggState *state, int64_t n_slots, AnofoxHipElasticNetBatchOptions options,
                                                     double *d_core, int32_t *d_iterations, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_elasticnet_slots_host(AnofoxHipAggState *state, int64_t n_list, const uint32_t *slots,
                                                         AnofoxHipElasticNetBatchOptions options, double *core, int32_t *iterations,
                                                         int64_t *out_unrefined, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_bls_host(AnofoxHipAggState *state, int64_t n_slots, AnofoxHipBlsBatchOptions options, double *bls,
                                            int32_t *iterations, int64_t *out_unrefined, int32_t *out_unrefined_slots, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_bls_device(AnofoxHipAggState *state, int64_t n_slots, AnofoxHipBlsBatchOptions options, double *d_bls,
                                              int32_t *d_iterations, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_agg_state_finalize_bls_slots_host(AnofoxHipAggState *state, int64_t n_list, const uint32_t *slots,
                                                  AnofoxHipBlsBatchOptions options, double *bls, int32_t *iterations, int64_t *out_unrefined,
                                                  AnofoxError *out_error);
/* Page-locked host memory for the shim's row arenas (copies from it run at the full PCIe rate and asynchronously). */
ANOFOX_HIP_API void *anofox_hip_host_alloc(size_t bytes);
ANOFOX_HIP_API void anofox_hip_host_free(void *ptr);

/* Predictions only, from existing fit records (d_core as produced by the fit entry points). */
ANOFOX_HIP_API bool anofox_hip_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                     const int64_t *d_row_offsets, const double *const *x_cols, const double *d_core,
                                     double confidence_level, double *d_pred, AnofoxError *out_error);

/*
 * Multi-GPU (no reference counterpart): the path shards by GROUP BY key — one process per GPU fits its
 * own keys with no data-path communication — and ONE collective assembles the result: an RCCL all-gather of the
 * fixed-size f64 records over xGMI.  These entry points are that exchange step without Python: rank 0 calls
 * anofox_hip_comm_unique_id and ships the 128 bytes to the other ranks by whatever channel the host has; every rank
 * calls anofox_hip_comm_create on its own context (collective: returns when all ranks have joined); after a fit,
 * anofox_hip_gather_records_device gathers `records_per_rank` records of `record_len` doubles from every rank into
 * d_all[world_size * records_per_rank * record_len] on every rank, rank r's block at r * records_per_rank (shards are
 * padded to the same count; pad records with NaN), stream-ordered behind the fit kernels of the communicator's
 * context.  RCCL is loaded at run time by the first of these calls (dlopen): the library has no link-time dependency
 * on it.
 */
#define ANOFOX_HIP_COMM_ID_BYTES 128
typedef struct AnofoxHipComm AnofoxHipComm;
ANOFOX_HIP_API bool anofox_hip_comm_unique_id(uint8_t *out_id /* [ANOFOX_HIP_COMM_ID_BYTES] */, AnofoxError *out_error);
ANOFOX_HIP_API bool anofox_hip_comm_create(AnofoxHipContext *ctx, int world_size, int rank, const uint8_t *id, AnofoxHipComm **out_comm,
                            AnofoxError *out_error);
ANOFOX_HIP_API void anofox_hip_comm_destroy(AnofoxHipComm *comm);
ANOFOX_HIP_API int anofox_hip_comm_world_size(const AnofoxHipComm *comm);
ANOFOX_HIP_API int anofox_hip_comm_rank(const AnofoxHipComm *comm);
/* ranks RCCL itself counts in the communicator (ncclCommCount): the audit figure of an N-GPU run; 0 = unknown */
ANOFOX_HIP_API int anofox_hip_comm_ranks_seen(const AnofoxHipComm *comm);
ANOFOX_HIP_API bool anofox_hip_gather_records_device(AnofoxHipComm *comm, const double *d_local, int64_t records_per_rank,
                                      size_t record_len, double *d_all, AnofoxError *out_error);

/* Measurement hooks (bench.py): when enabled, every accumulate-kernel launch of this context is
 * bracketed by HIP events on the launch stream. */
typedef struct {
	double accumulate_ms;     /* summed duration of the dominant (HBM-streaming) kernel */
	int64_t accumulate_count; /* launches summed */
	double solve_ms;          /* summed duration of the per-group solve/diagnostics kernels */
	int64_t solve_count;
	double predict_ms;        /* summed duration of the per-row prediction kernel */
	int64_t predict_count;
	double accumulate_ms_min; /* (r4) shortest / longest single launch of the dominant kernel in the interval (0 if none) */
	double accumulate_ms_max;
} AnofoxHipKernelTimes;
ANOFOX_HIP_API bool anofox_hip_context_enable_timing(AnofoxHipContext *ctx, bool enable, AnofoxError *out_error);
/* synchronises, returns the sums since the last call and resets them */
ANOFOX_HIP_API bool anofox_hip_context_collect_timing(AnofoxHipContext *ctx, AnofoxHipKernelTimes *out, AnofoxError *out_error);

/* Diagnostic: how many groups of the context's most recent fit launch (narrow path: the whole batch; wide path:
 * the last slab) were queued for the on-device refinement passes.  Synchronises the context's stream. */
ANOFOX_HIP_API bool anofox_hip_context_last_refine_count(AnofoxHipContext *ctx, int64_t *out_count, AnofoxError *out_error);

/* Diagnostic: output rows of the context's most recent window call (n_features <= 8) whose frame the in-register
 * kernel flagged as ill-conditioned and that were refitted through the virtual-group path with refinement. */
ANOFOX_HIP_API bool anofox_hip_context_last_window_refit_count(AnofoxHipContext *ctx, int64_t *out_count, AnofoxError *out_error);

/* Library / build identification, e.g. "anofox_stats_hip 0.1 gfx950". */
ANOFOX_HIP_API const char *anofox_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ANOFOX_STATS_HIP_H */
