// glm.hip — grouped generalised linear models (Poisson / log, binomial / logit): one wavefront per group runs the whole IRLS
// loop of glm_irls.h, and the entry points anofox_hip_glm_fit_batch_{device,host}, anofox_hip_glm_fit_predict_batch_*,
// anofox_hip_glm_fit_predict_interval_batch_*, anofox_hip_glm_fit_accuracy_batch_*, anofox_poisson_fit / anofox_binomial_fit /
// anofox_logistic_fit / anofox_free_glm_result.
//
// The contract and the method: glm_irls.h and DESIGN.md §1, "Generalised linear models".
//   glm_irls_kernel<EM>: 64 lanes per workgroup = one wavefront per group (grid-stride over the groups).  LDS holds the
//     augmented Gram matrix ((k + 1) x (k + 2 | 1) doubles), the row tile (64 x (k + 2 | 1)) and three vectors:
//     gi_work_doubles(k) * 8 bytes, 28.3 KB at k = 33.  EM = the Gram entries a lane owns at most (1, 4 or 10 by k).  eta and mu
//     of a row sit in a per-call device scratch (2 doubles per row, the context's workspace) that only the row's own lane
//     touches and that the first pass writes before anything reads it.  Nothing returns to the host between iterations; the
//     same wavefront writes the record, the inference and, for fit-predict, mu of every row.
// No atomics: a group is one wavefront's own work in a fixed order, so repeated calls give identical bytes.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "glm_irls.h"
#include "host_math.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::glm;

// shared with glm_window.hip (declared in context.h)
namespace anofox {
namespace host {

bool glm_options_invalid(const AnofoxHipGlmBatchOptions &o) {
	if (o.family != ANOFOX_HIP_GLM_POISSON && o.family != ANOFOX_HIP_GLM_BINOMIAL) return true;
	if (!(o.tolerance > 0.0) || !isfinite(o.tolerance)) return true;
	if (!(o.lambda >= 0.0) || !isfinite(o.lambda)) return true;
	if (o.max_iterations == 0) return true;
	if (o.compute_inference && !(o.confidence_level > 0.0 && o.confidence_level < 1.0)) return true;
	return false;
}

// the interval entry: z = 0 is the plain fit-predict; the bounds are the Poisson family's
bool glm_check_interval(const AnofoxHipGlmBatchOptions &o, double z, AnofoxError *e) {
	if (!(z >= 0.0) || !isfinite(z)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "glm: interval_z must be finite and not negative"); return false; }
	if (z > 0.0 && o.family == ANOFOX_HIP_GLM_BINOMIAL) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "glm: the prediction interval of the binomial family is not built");
		return false;
	}
	return true;
}

} // namespace host
} // namespace anofox

namespace {

struct GlmArgs {
	const int64_t *row_offsets;  // [G + 1]
	const int64_t *train_counts; // [G] or nullptr (fit-predict)
	const double *y;
	const double *x[kGiMaxP];
	const double *offset; // [n_rows] or nullptr
	double *scratch;      // [2 x n_rows]
	int64_t n_rows;
	int64_t n_groups;
	int p;
	int fit_intercept;
	int family;
	int max_iterations;
	double tolerance;
	double lambda;
	int compute_inference;
	double zq;
	int invalid;   // invalid options: every group gets ANOFOX_ERROR_INVALID_INPUT
	int rule;      // 1: the fit-predict rule "fewer than 2 training rows -> NULL"
	double *rec;   // [G x (p + 11)]
	double *inf;   // [G x 5 p] or nullptr
	double *pred;  // [n_rows x 3] or nullptr
	double interval_z; // > 0: the Poisson interval into pred[:, 1:]
	double threshold;  // of the accuracy
	double *accuracy;  // [G] or nullptr
};

// what the interval and accuracy entry points add to a launch; the other entry points pass none
struct GlmExtras {
	double interval_z = 0.0;
	double threshold = 0.5;
	double *accuracy = nullptr; // device: [G]; glm_host: the host array the result is copied to
};

template <int EM>
__global__ __launch_bounds__(64) void glm_irls_kernel(GlmArgs a) {
	extern __shared__ double glm_lds[];
	// the column pointers in LDS: indexing the kernel arguments by a run-time column would make a private copy of them
	__shared__ const double *glm_x[kGiMaxP];
#pragma unroll
	for (int j = 0; j < kGiMaxP; ++j)
		if (threadIdx.x == 0) glm_x[j] = a.x[j];
	__syncthreads();
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		GiProblem P;
		P.y = a.y;
		P.x = glm_x;
		P.offset = a.offset;
		P.p = a.p;
		P.fit_intercept = a.fit_intercept;
		P.family = a.family;
		P.lo = a.row_offsets[g];
		P.hi = a.row_offsets[g + 1];
		P.rule_count = a.rule ? (a.train_counts ? a.train_counts[g] : P.hi - P.lo) : -1;
		P.max_iterations = a.max_iterations;
		P.tolerance = a.tolerance;
		P.lambda = a.lambda;
		P.compute_inference = a.compute_inference;
		P.zq = a.zq;
		P.eta = a.scratch;
		P.mu = a.scratch + a.n_rows;
		P.interval_z = a.interval_z;
		P.threshold = a.threshold;
		P.accuracy = a.accuracy ? a.accuracy + g : nullptr;
		gi_fit<EM>(P, a.invalid != 0, glm_lds, a.rec + g * (int64_t)(a.p + 11), a.inf ? a.inf + g * (int64_t)(5 * a.p) : nullptr, a.pred);
		__syncthreads(); // the next group reuses the LDS
	}
}

using anofox::hostmath::normal_quantile; // (host_math.h: shared with aft.hip)

bool check_glm(int64_t G, size_t p, int64_t n_rows, const void *off, const void *y, const double *const *x_cols, const void *out,
               AnofoxError *e) {
	return check_batch_args(G, p, n_rows, off, y, x_cols, out, kGiMaxP, "glm: n_features > 32 is not built", "row_offsets, y or an output is NULL",
	                        false, e);
}

// the fit of G groups on device-resident inputs, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_glm(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const int64_t *d_off, const double *d_y,
                const double *const *x_cols, const double *d_offset, const int64_t *d_tc, const AnofoxHipGlmBatchOptions &o, int rule,
                double *d_rec, double *d_inf, double *d_pred, AnofoxError *e, const GlmExtras &x = GlmExtras()) {
	if (G == 0) return true;
	const size_t rows = n_rows > 0 ? (size_t)n_rows : 1;
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, 2 * rows * sizeof(double), "glm scratch", e)) return false;
	GlmArgs a;
	memset(&a, 0, sizeof a);
	a.row_offsets = d_off;
	a.train_counts = d_tc;
	a.y = d_y;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.offset = d_offset;
	a.scratch = (double *)ctx->ws;
	a.n_rows = (int64_t)rows;
	a.n_groups = G;
	a.p = (int)p;
	a.fit_intercept = o.fit_intercept ? 1 : 0;
	a.family = o.family;
	a.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	a.tolerance = o.tolerance;
	a.lambda = o.lambda;
	a.invalid = glm_options_invalid(o) ? 1 : 0;
	a.compute_inference = o.compute_inference && d_inf ? 1 : 0;
	a.zq = a.compute_inference && !a.invalid ? normal_quantile(0.5 + o.confidence_level / 2.0) : NAN;
	a.rule = rule;
	a.rec = d_rec;
	a.inf = d_inf;
	a.pred = d_pred;
	a.interval_z = x.interval_z;
	a.threshold = x.threshold;
	a.accuracy = x.accuracy;
	const int k = (int)p + a.fit_intercept;
	const size_t lds = gi_work_doubles(k) * sizeof(double);
	const int64_t max_blocks = 1 << 20;
	const dim3 grid((unsigned)(G < max_blocks ? G : max_blocks)), block(64);
	switch (gi_entry_class(k)) {
	case 1: hipLaunchKernelGGL(glm_irls_kernel<1>, grid, block, lds, ctx->stream, a); break;
	case 4: hipLaunchKernelGGL(glm_irls_kernel<4>, grid, block, lds, ctx->stream, a); break;
	default: hipLaunchKernelGGL(glm_irls_kernel<10>, grid, block, lds, ctx->stream, a); break;
	}
	return !hip_fail(hipGetLastError(), "glm_irls_kernel", e);
}

// host pointers: one staging of the whole call, the kernel, the copies back (fit: pred == nullptr; fit-predict: inf == nullptr)
bool glm_host(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *row_offsets, const double *y,
              const double *const *x_cols, const double *offset, const int64_t *train_counts, const AnofoxHipGlmBatchOptions &o, int rule,
              double *rec, double *inf, double *pred, AnofoxError *e, const GlmExtras &x = GlmExtras()) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups, N = (size_t)n_rows, rec_len = p + 11;
	std::lock_guard<std::mutex> lk(ctx->mu); // one lock over staging, the kernel and the copies back
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off, *d_tc;
	StagedColumns c;
	double *d_rec, *d_inf, *d_pred;
	GlmExtras dx = x;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(row_offsets, G + 1);
		    d_tc = s.put(train_counts, G);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, offset, kPlainColumns);
		    d_rec = s.take<double>(G * rec_len);
		    d_inf = inf ? s.take<double>(G * 5 * p) : nullptr;
		    d_pred = pred ? s.take<double>(3 * N) : nullptr;
		    if (x.accuracy) dx.accuracy = s.take<double>(G);
	    }))
		return false;
	if (!launch_glm(ctx, n_groups, p, n_rows, d_off, c.y, c.x, c.offset, d_tc, o, rule, d_rec, d_inf, d_pred, e, dx)) return false;
	if (x.accuracy && !d2h(x.accuracy, dx.accuracy, G * sizeof(double), st, e)) return false;
	if (!d2h(rec, d_rec, G * rec_len * sizeof(double), st, e)) return false;
	if (inf && !d2h(inf, d_inf, G * 5 * p * sizeof(double), st, e)) return false;
	if (pred && !d2h(pred, d_pred, 3 * N * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

bool check_accuracy(const AnofoxHipGlmBatchOptions &o, double threshold, AnofoxError *e) {
	if (o.family != ANOFOX_HIP_GLM_BINOMIAL) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "glm: the accuracy is the binomial family's"); return false; }
	if (!isfinite(threshold)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "glm: threshold must be finite"); return false; }
	return true;
}

// ---- the one-group entry points ----
void reset_inference(AnofoxFitResultInference *inf) {
	if (!inf) return;
	inf->std_errors = inf->t_values = inf->p_values = inf->ci_lower = inf->ci_upper = nullptr;
	inf->len = 0;
	inf->confidence_level = inf->f_statistic = inf->f_pvalue = NAN;
}

struct ScalarOptions {
	const char *name;
	bool fit_intercept, compute_inference;
	int family, link;
	uint32_t max_iterations;
	double tolerance, confidence_level, lambda;
	const AnofoxPriorSpec *priors;
	int vcov;
	size_t offset_column;
	bool binary_y;    // logistic: y in {0, 1}
	double threshold; // logistic
};

// A batch of one group with anofox_ols_fit's conventions: argument checks first, NULL entries -> NaN, the offset column split
// out of x (design.rs:186-202), the reference's error texts (crates/anofox-stats-core/src/errors.rs), the arrays malloc'ed.
bool scalar_glm_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, const ScalarOptions &so, AnofoxGlmFitResultCore *out_core,
                    AnofoxFitResultInference *out_inference, AnofoxLogisticFitExtras *out_extras, AnofoxError *out_error) {
	reset_error(out_error);
	reset_inference(out_inference); // a failed call leaves no pointer behind in any output
	if (out_extras) out_extras->accuracy = out_extras->threshold = NAN;
	if (!out_core) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_core is NULL"); return false; }
	memset(out_core, 0, sizeof *out_core);
	out_core->intercept = out_core->deviance = out_core->null_deviance = out_core->pseudo_r_squared = out_core->aic = out_core->dispersion = NAN;
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (y.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: y cannot be empty"); return false; }
	if (so.link != 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, std::string("glm: link ") + std::to_string(so.link) + " of " + so.name + " is not built"); return false; }
	if (so.priors) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glm: priors are not built"); return false; }
	if (so.vcov != ANOFOX_VCOV_LAPLACE) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glm: a vcov other than Laplace is not built"); return false; }
	for (size_t j = 0; j < x_count; ++j) {
		if (x[j].len != y.len) {
			set_error(out_error, ANOFOX_ERROR_DIMENSION_MISMATCH,
			          "Dimension mismatch: y has " + std::to_string(y.len) + " elements, X has " + std::to_string(x[j].len) + " rows");
			return false;
		}
	}
	if (so.offset_column > x_count) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT,
		          "Invalid value for offset: offset must be a 1-based index into x (1..=" + std::to_string(x_count) + "), got " + std::to_string(so.offset_column));
		return false;
	}
	if (so.binary_y && !(so.threshold >= 0.0 && so.threshold <= 1.0)) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "threshold must be in [0, 1]");
		return false;
	}
	const size_t n = y.len, p = x_count - (so.offset_column ? 1 : 0);
	if (p == 0) { set_error(out_error, ANOFOX_ERROR_INSUFFICIENT_DATA, "Insufficient data: no feature besides the offset column"); return false; }
	if (p > (size_t)kGiMaxP) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glm: n_features > 32 is not built"); return false; }
	std::vector<double> yv, ov;
	expand_data_array(y, yv);
	std::vector<std::vector<double>> cols(p);
	std::vector<const double *> xp(p);
	for (size_t j = 0, f = 0; j < x_count; ++j) {
		if (so.offset_column && j == so.offset_column - 1) { expand_data_array(x[j], ov); continue; }
		expand_data_array(x[j], cols[f]);
		xp[f] = cols[f].data();
		++f;
	}
	if (so.binary_y)
		for (size_t i = 0; i < n; ++i)
			if (yv[i] == yv[i] && yv[i] != 0.0 && yv[i] != 1.0) {
				set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Invalid value for y: Logistic regression requires binary response values (0.0 or 1.0)");
				return false;
			}
	AnofoxHipGlmBatchOptions o;
	memset(&o, 0, sizeof o);
	o.family = so.family;
	o.fit_intercept = so.fit_intercept;
	o.max_iterations = so.max_iterations;
	o.tolerance = so.tolerance;
	o.lambda = so.lambda;
	o.compute_inference = so.compute_inference && out_inference;
	o.confidence_level = so.confidence_level;
	if (glm_options_invalid(o)) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, std::string("glm: invalid options for ") + so.name); return false; }
	const int64_t off[2] = {0, (int64_t)n};
	std::vector<double> rec(p + 11), inf(5 * p), pred(so.binary_y && out_extras ? 3 * n : 0);
	const bool want_pred = !pred.empty();
	// (the accuracy needs mu of the fitted rows: the fit-predict form without its "fewer than 2 rows" rule)
	if (!glm_host(nullptr, 1, p, (int64_t)n, off, yv.data(), xp.data(), so.offset_column ? ov.data() : nullptr, nullptr, o, 0, rec.data(),
	              o.compute_inference ? inf.data() : nullptr, want_pred ? pred.data() : nullptr, out_error))
		return false;
	const int status = (int)rec[p + 10];
	if (status != ANOFOX_ERROR_SUCCESS) {
		std::string msg;
		switch (status) {
		case ANOFOX_ERROR_NO_VALID_DATA: msg = "All rows filtered due to NULL/NaN values"; break;
		case ANOFOX_ERROR_INSUFFICIENT_DATA: msg = "Insufficient data: fewer valid rows than parameters (" + std::to_string(p) + " features)"; break;
		case ANOFOX_ERROR_CONVERGENCE_FAILURE: msg = "Convergence failure after " + std::to_string(so.max_iterations) + " iterations"; break;
		case ANOFOX_ERROR_INVALID_INPUT: msg = std::string("Invalid value for y: outside the support of ") + so.name; break;
		default: msg = "GLM fit failed on the GPU path"; break;
		}
		set_error(out_error, (AnofoxErrorCode)status, msg);
		return false;
	}
	double *coef = (double *)malloc(p * sizeof(double));
	if (!coef) {
		set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate coefficients");
		return false;
	}
	memcpy(coef, rec.data(), p * sizeof(double));
	out_core->coefficients = coef;
	out_core->coefficients_len = p;
	out_core->intercept = rec[p];
	out_core->deviance = rec[p + 1];
	out_core->null_deviance = rec[p + 2];
	out_core->pseudo_r_squared = rec[p + 3];
	out_core->aic = rec[p + 4];
	out_core->dispersion = rec[p + 5];
	out_core->n_observations = (size_t)rec[p + 6];
	out_core->n_features = p;
	out_core->iterations = (uint32_t)rec[p + 8];
	out_core->converged = rec[p + 9] != 0.0;
	if (o.compute_inference) { // five arrays of their own: anofox_free_result_inference frees each
		double *parts[5];
		bool ok = true;
		for (int b = 0; b < 5; ++b) ok = (parts[b] = (double *)malloc(p * sizeof(double))) && ok;
		if (!ok) {
			for (int b = 0; b < 5; ++b) free(parts[b]);
			free(coef);
			out_core->coefficients = nullptr;
			out_core->coefficients_len = 0;
			set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate inference arrays");
			return false;
		}
		for (int b = 0; b < 5; ++b) memcpy(parts[b], inf.data() + (size_t)b * p, p * sizeof(double));
		out_inference->std_errors = parts[0];
		out_inference->t_values = parts[1];
		out_inference->p_values = parts[2];
		out_inference->ci_lower = parts[3];
		out_inference->ci_upper = parts[4];
		out_inference->len = p;
		out_inference->confidence_level = so.confidence_level;
	}
	if (out_extras) {
		out_extras->threshold = so.threshold;
		out_extras->accuracy = NAN;
		if (want_pred) {
			size_t correct = 0, fitted = 0;
			for (size_t i = 0; i < n; ++i) {
				const double mu = pred[3 * i];
				if (!(yv[i] == yv[i]) || !(mu == mu)) continue; // (a row is fitted when y, x and offset are finite)
				++fitted;
				correct += ((mu >= so.threshold ? 1.0 : 0.0) == yv[i]) ? 1 : 0;
			}
			out_extras->accuracy = (double)correct / (double)(fitted ? fitted : 1);
		}
	}
	return true;
}

} // namespace

extern "C" {

size_t anofox_hip_glm_record_len(size_t p) { return p + 11; }

bool anofox_hip_glm_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows, const int64_t *d_row_offsets,
                                     const double *d_y, const double *const *x_cols, const double *d_offset, AnofoxHipGlmBatchOptions options,
                                     double *d_records, double *d_inference, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glm(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_glm(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_offset, nullptr, options, 0, d_records, d_inference,
	                  nullptr, out_error);
}

bool anofox_hip_glm_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows, const int64_t *row_offsets,
                                   const double *y, const double *const *x_cols, const double *offset, AnofoxHipGlmBatchOptions options,
                                   double *records, double *inference, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glm(n_groups, n_features, n_rows, row_offsets, y, x_cols, records, out_error)) return false;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	return glm_host(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, offset, nullptr, options, 0, records, inference, nullptr,
	                out_error);
}

bool anofox_hip_glm_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                             const double *d_offset, const int64_t *d_train_counts, AnofoxHipGlmBatchOptions options,
                                             double *d_core, double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glm(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_core, out_error)) return false;
	if (n_groups > 0 && !d_pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_glm(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_offset, d_train_counts, options, 1, d_core, nullptr,
	                  d_pred, out_error);
}

bool anofox_hip_glm_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *y, const double *const *x_cols, const double *offset,
                                           const int64_t *train_counts, AnofoxHipGlmBatchOptions options, double *core, double *pred,
                                           AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glm(n_groups, n_features, n_rows, row_offsets, y, x_cols, core, out_error)) return false;
	if (n_groups > 0 && !pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_whole_range(n_groups, n_rows, row_offsets, out_error)) return false;
	return glm_host(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, offset, train_counts, options, 1, core, nullptr, pred, out_error);
}

bool anofox_hip_glm_fit_predict_interval_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                      const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                      const double *d_offset, const int64_t *d_train_counts,
                                                      AnofoxHipGlmBatchOptions options, double interval_z, double *d_core, double *d_pred,
                                                      AnofoxError *out_error) {
	reset_error(out_error);
	if (!glm_check_interval(options, interval_z, out_error)) return false;
	if (!check_glm(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_core, out_error)) return false;
	if (n_groups > 0 && !d_pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	GlmExtras x;
	x.interval_z = interval_z;
	return launch_glm(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_offset, d_train_counts, options, 1, d_core, nullptr,
	                  d_pred, out_error, x);
}

bool anofox_hip_glm_fit_predict_interval_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                    const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                    const double *offset, const int64_t *train_counts, AnofoxHipGlmBatchOptions options,
                                                    double interval_z, double *core, double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!glm_check_interval(options, interval_z, out_error)) return false;
	if (!check_glm(n_groups, n_features, n_rows, row_offsets, y, x_cols, core, out_error)) return false;
	if (n_groups > 0 && !pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_whole_range(n_groups, n_rows, row_offsets, out_error)) return false;
	GlmExtras x;
	x.interval_z = interval_z;
	return glm_host(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, offset, train_counts, options, 1, core, nullptr, pred,
	                out_error, x);
}

bool anofox_hip_glm_fit_accuracy_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                              const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                              const double *d_offset, AnofoxHipGlmBatchOptions options, double threshold, double *d_records,
                                              double *d_inference, double *d_accuracy, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_accuracy(options, threshold, out_error)) return false;
	if (!check_glm(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_records, out_error)) return false;
	if (n_groups > 0 && !d_accuracy) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "accuracy is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	GlmExtras x;
	x.threshold = threshold;
	x.accuracy = d_accuracy;
	return launch_glm(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_offset, nullptr, options, 0, d_records, d_inference,
	                  nullptr, out_error, x);
}

bool anofox_hip_glm_fit_accuracy_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *row_offsets, const double *y, const double *const *x_cols, const double *offset,
                                            AnofoxHipGlmBatchOptions options, double threshold, double *records, double *inference,
                                            double *accuracy, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_accuracy(options, threshold, out_error)) return false;
	if (!check_glm(n_groups, n_features, n_rows, row_offsets, y, x_cols, records, out_error)) return false;
	if (n_groups > 0 && !accuracy) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "accuracy is NULL"); return false; }
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	GlmExtras x;
	x.threshold = threshold;
	x.accuracy = accuracy;
	return glm_host(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, offset, nullptr, options, 0, records, inference, nullptr,
	                out_error, x);
}

bool anofox_poisson_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxPoissonOptions options,
                        AnofoxGlmFitResultCore *out_core, AnofoxFitResultInference *out_inference, AnofoxError *out_error) {
	const ScalarOptions so = {"poisson", options.fit_intercept, options.compute_inference, ANOFOX_HIP_GLM_POISSON, (int)options.link,
	                          options.max_iterations, options.tolerance, options.confidence_level, options.lambda, options.priors,
	                          (int)options.vcov, options.offset_column, false, NAN};
	return scalar_glm_fit(y, x, x_count, so, out_core, out_inference, nullptr, out_error);
}

bool anofox_binomial_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxBinomialOptions options,
                         AnofoxGlmFitResultCore *out_core, AnofoxFitResultInference *out_inference, AnofoxError *out_error) {
	const ScalarOptions so = {"binomial", options.fit_intercept, options.compute_inference, ANOFOX_HIP_GLM_BINOMIAL, (int)options.link,
	                          options.max_iterations, options.tolerance, options.confidence_level, options.lambda, options.priors,
	                          (int)options.vcov, options.offset_column, false, NAN};
	return scalar_glm_fit(y, x, x_count, so, out_core, out_inference, nullptr, out_error);
}

bool anofox_logistic_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxLogisticOptions options,
                         AnofoxGlmFitResultCore *out_result, AnofoxFitResultInference *out_inference, AnofoxLogisticFitExtras *out_extras,
                         AnofoxError *out_error) {
	const ScalarOptions so = {"logistic", options.fit_intercept, options.compute_inference, ANOFOX_HIP_GLM_BINOMIAL, 0,
	                          options.max_iterations, options.tolerance, options.confidence_level, options.lambda, options.priors,
	                          (int)options.vcov, options.offset_column, true, options.threshold};
	return scalar_glm_fit(y, x, x_count, so, out_result, out_inference, out_extras, out_error);
}

void anofox_free_glm_result(AnofoxGlmFitResultCore *result) {
	if (!result) return;
	free(result->coefficients);
	result->coefficients = nullptr;
	result->coefficients_len = 0;
}

} // extern "C"
