// aft.hip — grouped accelerated failure time (AFT) survival regression with right censoring: one wavefront per group runs the
// whole Newton loop of aft_newton.h, and the entry points anofox_hip_aft_fit_batch_{device,host},
// anofox_hip_aft_fit_predict_batch_{device,host}, anofox_aft_fit / anofox_free_aft_result / anofox_free_aft_inference,
// anofox_aft_cdf / anofox_aft_quantile.
//
// The contract and the method: aft_newton.h and DESIGN.md §1, "Accelerated failure time models".
//   aft_newton_kernel<EM>: 64 lanes per workgroup = one wavefront per group (grid-stride over the groups).  LDS holds the
//     augmented matrix ((k + 1) x (k + 1 | 1) doubles), the row tile (64 x (k + 3 | 1)) and five vectors: an_work_doubles(k) * 8
//     bytes, 29.4 KB at k = 34 (p = 32, an intercept and a scale).  EM = the matrix entries a lane owns at most (1, 4 or 10 by
//     k).  log t of a row sits in a per-call device scratch (one double per row, the context's workspace) that only the row's
//     own lane touches and that the first pass writes before anything reads it.  Nothing returns to the host between
//     iterations; the same wavefront writes the record and the inference and fits the intercept-only model.
//   aft_newton_kernel<EM, true>: the fit-predict launch.  The same fit, then an_predict: the wavefront walks its rows once more
//     and writes {eta, time_quantile, cdf, risk} per row, each lane its own rows' 32 bytes.  PRED is a template parameter so
//     that the fit-only kernel's code is the one it was; LDS is the same (beta and sigma are in it).
// No atomics: a group is one wavefront's own work in a fixed order, so repeated calls give identical bytes.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "aft_newton.h"
#include "host_math.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::aft;

namespace {

std::atomic<int64_t> g_max_blocks{0}; // anofox_hip_aft_test_hooks

struct AftArgs {
	const int64_t *row_offsets; // [G + 1]
	const double *time;
	const double *event;
	const double *x[kAnMaxP];
	double *scratch; // [n_rows]
	int64_t n_groups;
	int p;
	int fit_intercept;
	int dist;
	int max_iterations;
	double tolerance;
	int compute_inference;
	double zq;
	int invalid; // invalid options: every group gets ANOFOX_ERROR_INVALID_INPUT
	double *rec; // [G x (p + 13)]
	double *inf; // [G x (5 p + 2)] or nullptr
	// the fit-predict launch
	double *pred;   // [n_rows x 4]
	double wq;      // the predict quantile of W
	double horizon; // NaN: risk is not asked for
};

template <int EM, bool PRED>
__global__ __launch_bounds__(64) void aft_newton_kernel(AftArgs a) {
	extern __shared__ double aft_lds[];
	// the column pointers in LDS: indexing the kernel arguments by a run-time column would make a private copy of them
	__shared__ const double *aft_x[kAnMaxP];
#pragma unroll
	for (int j = 0; j < kAnMaxP; ++j)
		if (threadIdx.x == 0) aft_x[j] = a.x[j];
	__syncthreads();
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		AnProblem P;
		P.time = a.time;
		P.event = a.event;
		P.x = aft_x;
		P.p = a.p;
		P.fit_intercept = a.fit_intercept;
		P.dist = a.dist;
		P.lo = a.row_offsets[g];
		P.hi = a.row_offsets[g + 1];
		P.max_iterations = a.max_iterations;
		P.tolerance = a.tolerance;
		P.compute_inference = a.compute_inference;
		P.zq = a.zq;
		P.logt = a.scratch;
		if (PRED) {
			P.pred = a.pred;
			P.wq = a.wq;
			P.horizon = a.horizon;
		}
		an_fit<EM>(P, a.invalid != 0, aft_lds, a.rec + g * (int64_t)(a.p + 13), a.inf ? a.inf + g * (int64_t)(5 * a.p + 2) : nullptr);
		__syncthreads(); // the next group reuses the LDS
	}
}

double kernel_quantile(int dist, double p);

bool aft_options_invalid(const AnofoxHipAftBatchOptions &o) {
	if (o.dist < ANOFOX_AFT_WEIBULL || o.dist > ANOFOX_AFT_EXPONENTIAL) return true;
	if (!(o.tolerance > 0.0) || !isfinite(o.tolerance)) return true;
	if (o.max_iterations == 0) return true;
	if (o.compute_inference && !(o.confidence_level > 0.0 && o.confidence_level < 1.0)) return true;
	return false;
}

bool check_aft(int64_t G, size_t p, int64_t n_rows, const void *off, const void *time, const double *const *x_cols, const void *event,
               const void *out, AnofoxError *e) {
	if (!check_batch_args(G, p, n_rows, off, time, x_cols, out, kAnMaxP, "aft: n_features > 32 is not built",
	                      "row_offsets, time or an output is NULL", false, e))
		return false;
	if (G > 0 && !event) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "event is NULL"); return false; }
	return true;
}

// the fit of G groups on device-resident inputs, enqueued on the context's stream (ctx->mu held by the caller)
// predict (with d_pred) or neither: the fit-predict launch, which also scores every row
bool launch_aft(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const int64_t *d_off, const double *d_time,
                const double *const *x_cols, const double *d_event, const AnofoxHipAftBatchOptions &o, double *d_rec, double *d_inf,
                AnofoxError *e, const AnofoxHipAftPredictOptions *predict = nullptr, double *d_pred = nullptr) {
	if (G == 0) return true;
	const size_t rows = n_rows > 0 ? (size_t)n_rows : 1;
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, rows * sizeof(double), "aft scratch", e)) return false;
	AftArgs a;
	memset(&a, 0, sizeof a);
	a.row_offsets = d_off;
	a.time = d_time;
	a.event = d_event;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.scratch = (double *)ctx->ws;
	a.n_groups = G;
	a.p = (int)p;
	a.fit_intercept = o.fit_intercept ? 1 : 0;
	a.invalid = aft_options_invalid(o) ? 1 : 0;
	a.dist = a.invalid ? ANOFOX_AFT_WEIBULL : o.dist;
	a.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	a.tolerance = o.tolerance;
	a.compute_inference = o.compute_inference && d_inf ? 1 : 0;
	a.zq = a.compute_inference && !a.invalid ? hostmath::normal_quantile(0.5 + o.confidence_level / 2.0) : NAN;
	a.rec = d_rec;
	a.inf = d_inf;
	a.pred = d_pred;
	a.wq = d_pred ? kernel_quantile(a.dist, predict->quantile) : NAN;
	a.horizon = d_pred ? predict->horizon : NAN;
	const int k = (int)p + a.fit_intercept + (an_scale_is_fixed(a.dist) ? 0 : 1);
	const size_t lds = an_work_doubles(k) * sizeof(double);
	const int64_t hook = g_max_blocks.load(), max_blocks = hook > 0 ? hook : 1 << 20;
	const dim3 grid((unsigned)(G < max_blocks ? G : max_blocks)), block(64);
	switch (an_entry_class(k) + (d_pred ? 100 : 0)) {
	case 1: hipLaunchKernelGGL((aft_newton_kernel<1, false>), grid, block, lds, ctx->stream, a); break;
	case 4: hipLaunchKernelGGL((aft_newton_kernel<4, false>), grid, block, lds, ctx->stream, a); break;
	case 10: hipLaunchKernelGGL((aft_newton_kernel<10, false>), grid, block, lds, ctx->stream, a); break;
	case 101: hipLaunchKernelGGL((aft_newton_kernel<1, true>), grid, block, lds, ctx->stream, a); break;
	case 104: hipLaunchKernelGGL((aft_newton_kernel<4, true>), grid, block, lds, ctx->stream, a); break;
	default: hipLaunchKernelGGL((aft_newton_kernel<10, true>), grid, block, lds, ctx->stream, a); break;
	}
	return !hip_fail(hipGetLastError(), "aft_newton_kernel", e);
}

// the predict options' own rules, answered before any device is touched
bool check_aft_predict(const AnofoxHipAftPredictOptions &q, const void *pred, int64_t G, AnofoxError *e) {
	if (G > 0 && !pred) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!(q.quantile > 0.0 && q.quantile < 1.0)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "aft: quantile must be in (0, 1)"); return false; }
	if (q.horizon == q.horizon && !(q.horizon >= 0.0 && isfinite(q.horizon))) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "aft: horizon must be finite and >= 0");
		return false;
	}
	return true;
}

// host pointers: one staging of the whole call, the kernel, the copies back
bool aft_host(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *row_offsets, const double *time,
              const double *const *x_cols, const double *event, const AnofoxHipAftBatchOptions &o, double *rec, double *inf,
              AnofoxError *e, const AnofoxHipAftPredictOptions *predict = nullptr, double *pred = nullptr) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups, rec_len = p + 13, inf_len = 5 * p + 2;
	std::lock_guard<std::mutex> lk(ctx->mu); // one lock over staging, the kernel and the copies back
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off;
	StagedColumns c;
	double *d_rec, *d_inf, *d_pred = nullptr;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(row_offsets, G + 1);
		    c = s.columns(p, 0, n_rows, x_cols, time, event, nullptr, kPlainColumns); // (the event column in the weight slot)
		    d_rec = s.take<double>(G * rec_len);
		    d_inf = inf ? s.take<double>(G * inf_len) : nullptr;
		    if (pred) d_pred = s.take<double>((size_t)n_rows * 4);
	    }))
		return false;
	if (!launch_aft(ctx, n_groups, p, n_rows, d_off, c.y, c.x, c.w, o, d_rec, d_inf, e, predict, d_pred)) return false;
	if (!d2h(rec, d_rec, G * rec_len * sizeof(double), st, e)) return false;
	if (pred && n_rows > 0 && !d2h(pred, d_pred, (size_t)n_rows * 4 * sizeof(double), st, e)) return false;
	if (inf && !d2h(inf, d_inf, G * inf_len * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

void reset_aft_inference(AnofoxAftInference *inf) {
	if (!inf) return;
	inf->std_errors = inf->z_values = inf->p_values = inf->ci_lower = inf->ci_upper = nullptr;
	inf->len = 0;
	inf->confidence_level = inf->intercept_std_error = inf->log_scale_std_error = NAN;
}

// z of W's distribution function and its inverse (aft_dist.rs): extreme value, normal, logistic
double kernel_cdf(int dist, double z) {
	switch (dist) {
	case ANOFOX_AFT_WEIBULL:
	case ANOFOX_AFT_EXPONENTIAL: return -expm1(-exp(z > kAnZClamp ? kAnZClamp : (z < -kAnZClamp ? -kAnZClamp : z)));
	case ANOFOX_AFT_LOGNORMAL: return 0.5 * erfc(-z * M_SQRT1_2);
	case ANOFOX_AFT_LOGLOGISTIC: {
		const double e = exp(-fabs(z));
		return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
	}
	default: return NAN;
	}
}

double kernel_quantile(int dist, double p) {
	if (!(p == p)) return NAN;
	p = p < 1e-12 ? 1e-12 : (p > 1.0 - 1e-12 ? 1.0 - 1e-12 : p);
	switch (dist) {
	case ANOFOX_AFT_WEIBULL:
	case ANOFOX_AFT_EXPONENTIAL: return log(-log1p(-p));
	case ANOFOX_AFT_LOGNORMAL: return hostmath::normal_quantile(p);
	case ANOFOX_AFT_LOGLOGISTIC: return log(p / (1.0 - p));
	default: return NAN;
	}
}

} // namespace

extern "C" {

size_t anofox_hip_aft_record_len(size_t p) { return p + 13; }

void anofox_hip_aft_test_hooks(int64_t max_blocks) { g_max_blocks.store(max_blocks > 0 ? max_blocks : 0); }

bool anofox_hip_aft_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows, const int64_t *d_row_offsets,
                                     const double *d_time, const double *const *d_x_cols, const double *d_event,
                                     AnofoxHipAftBatchOptions options, double *d_records, double *d_inference, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_aft(n_groups, n_features, n_rows, d_row_offsets, d_time, d_x_cols, d_event, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_aft(ctx, n_groups, n_features, n_rows, d_row_offsets, d_time, d_x_cols, d_event, options, d_records, d_inference, out_error);
}

bool anofox_hip_aft_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows, const int64_t *row_offsets,
                                   const double *time, const double *const *x_cols, const double *event, AnofoxHipAftBatchOptions options,
                                   double *records, double *inference, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_aft(n_groups, n_features, n_rows, row_offsets, time, x_cols, event, records, out_error)) return false;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	return aft_host(ctx, n_groups, n_features, n_rows, row_offsets, time, x_cols, event, options, records, inference, out_error);
}

size_t anofox_hip_aft_pred_len(void) { return 4; }

bool anofox_hip_aft_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_time, const double *const *d_x_cols,
                                             const double *d_event, AnofoxHipAftBatchOptions options, AnofoxHipAftPredictOptions predict,
                                             double *d_records, double *d_inference, double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_aft(n_groups, n_features, n_rows, d_row_offsets, d_time, d_x_cols, d_event, d_records, out_error)) return false;
	if (!check_aft_predict(predict, d_pred, n_groups, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_aft(ctx, n_groups, n_features, n_rows, d_row_offsets, d_time, d_x_cols, d_event, options, d_records, d_inference, out_error,
	                  &predict, d_pred);
}

bool anofox_hip_aft_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *time, const double *const *x_cols, const double *event,
                                           AnofoxHipAftBatchOptions options, AnofoxHipAftPredictOptions predict, double *records,
                                           double *inference, double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_aft(n_groups, n_features, n_rows, row_offsets, time, x_cols, event, records, out_error)) return false;
	if (!check_aft_predict(predict, pred, n_groups, out_error)) return false;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	return aft_host(ctx, n_groups, n_features, n_rows, row_offsets, time, x_cols, event, options, records, inference, out_error, &predict, pred);
}

// A batch of one group with anofox_ols_fit's conventions: argument checks first, NULL entries -> NaN, the arrays malloc'ed.
bool anofox_aft_fit(AnofoxDataArray time, const AnofoxDataArray *x, size_t x_count, AnofoxDataArray event, AnofoxAftOptions options,
                    AnofoxAftFitResultCore *out_core, AnofoxAftInference *out_inference, AnofoxError *out_error) {
	reset_error(out_error);
	reset_aft_inference(out_inference); // a failed call leaves no pointer behind in any output
	if (!out_core) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_core is NULL"); return false; }
	memset(out_core, 0, sizeof *out_core);
	out_core->intercept = out_core->scale = out_core->log_likelihood = out_core->null_log_likelihood = out_core->aic = out_core->bic = NAN;
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (time.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: time cannot be empty"); return false; }
	if (options.priors) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "aft: priors are not built"); return false; }
	if (event.len != time.len) {
		set_error(out_error, ANOFOX_ERROR_DIMENSION_MISMATCH,
		          "Dimension mismatch: time has " + std::to_string(time.len) + " elements, event has " + std::to_string(event.len));
		return false;
	}
	for (size_t j = 0; j < x_count; ++j) {
		if (x[j].len != time.len) {
			set_error(out_error, ANOFOX_ERROR_DIMENSION_MISMATCH,
			          "Dimension mismatch: time has " + std::to_string(time.len) + " elements, X has " + std::to_string(x[j].len) + " rows");
			return false;
		}
	}
	const size_t n = time.len, p = x_count;
	if (p > (size_t)kAnMaxP) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "aft: n_features > 32 is not built"); return false; }
	AnofoxHipAftBatchOptions o;
	memset(&o, 0, sizeof o);
	o.dist = (int)options.dist;
	o.fit_intercept = options.fit_intercept ? 1 : 0;
	o.max_iterations = options.max_iterations;
	o.tolerance = options.tolerance;
	o.compute_inference = options.compute_inference && out_inference ? 1 : 0;
	o.confidence_level = options.confidence_level;
	if (aft_options_invalid(o)) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "aft: invalid options"); return false; }
	std::vector<double> tv, ev;
	expand_data_array(time, tv);
	expand_data_array(event, ev);
	std::vector<std::vector<double>> cols(p);
	std::vector<const double *> xp(p);
	for (size_t j = 0; j < p; ++j) {
		expand_data_array(x[j], cols[j]);
		xp[j] = cols[j].data();
	}
	const int64_t off[2] = {0, (int64_t)n};
	std::vector<double> rec(p + 13), inf(5 * p + 2);
	if (!aft_host(nullptr, 1, p, (int64_t)n, off, tv.data(), xp.data(), ev.data(), o, rec.data(), o.compute_inference ? inf.data() : nullptr,
	              out_error))
		return false;
	const int status = (int)rec[p + 12];
	if (status != ANOFOX_ERROR_SUCCESS) {
		std::string msg;
		switch (status) {
		case ANOFOX_ERROR_NO_VALID_DATA: msg = "All rows filtered due to NULL/NaN values"; break;
		case ANOFOX_ERROR_INSUFFICIENT_DATA: msg = "Insufficient data: fewer valid rows than parameters + 1 (" + std::to_string(p) + " features)"; break;
		case ANOFOX_ERROR_CONVERGENCE_FAILURE: msg = "Convergence failure after " + std::to_string(options.max_iterations) + " iterations"; break;
		case ANOFOX_ERROR_INVALID_INPUT:
			msg = "Invalid value: AFT regression needs strictly positive times, an event indicator of 0 or 1 and at least one observed event";
			break;
		default: msg = "AFT fit failed on the GPU path"; break;
		}
		set_error(out_error, (AnofoxErrorCode)status, msg);
		return false;
	}
	double *coef = (double *)malloc(p * sizeof(double));
	if (!coef) { set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate coefficients"); return false; }
	memcpy(coef, rec.data(), p * sizeof(double));
	if (o.compute_inference) { // five arrays of their own: anofox_free_aft_inference frees each
		double *parts[5];
		bool ok = true;
		for (int b = 0; b < 5; ++b) ok = (parts[b] = (double *)malloc(p * sizeof(double))) && ok;
		if (!ok) {
			for (int b = 0; b < 5; ++b) free(parts[b]);
			free(coef);
			set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate inference arrays");
			return false;
		}
		for (int b = 0; b < 5; ++b) memcpy(parts[b], inf.data() + (size_t)b * p, p * sizeof(double));
		out_inference->std_errors = parts[0];
		out_inference->z_values = parts[1];
		out_inference->p_values = parts[2];
		out_inference->ci_lower = parts[3];
		out_inference->ci_upper = parts[4];
		out_inference->len = p;
		out_inference->confidence_level = options.confidence_level;
		out_inference->intercept_std_error = inf[5 * p];
		out_inference->log_scale_std_error = inf[5 * p + 1];
	}
	out_core->coefficients = coef;
	out_core->coefficients_len = p;
	out_core->intercept = rec[p];
	out_core->scale = rec[p + 1];
	out_core->log_likelihood = rec[p + 2];
	out_core->null_log_likelihood = rec[p + 3];
	out_core->aic = rec[p + 4];
	out_core->bic = rec[p + 5];
	out_core->n_observations = (size_t)rec[p + 6];
	out_core->n_events = (size_t)rec[p + 7];
	out_core->n_censored = (size_t)rec[p + 8];
	out_core->n_features = p;
	out_core->iterations = (uint32_t)rec[p + 10];
	out_core->converged = rec[p + 11] != 0.0;
	return true;
}

void anofox_free_aft_result(AnofoxAftFitResultCore *result) {
	if (!result) return;
	free(result->coefficients);
	result->coefficients = nullptr;
	result->coefficients_len = 0;
}

void anofox_free_aft_inference(AnofoxAftInference *inf) {
	if (!inf) return;
	free(inf->std_errors);
	free(inf->z_values);
	free(inf->p_values);
	free(inf->ci_lower);
	free(inf->ci_upper);
	inf->std_errors = inf->z_values = inf->p_values = inf->ci_lower = inf->ci_upper = nullptr;
	inf->len = 0;
}

double anofox_aft_cdf(double t, double eta, double scale, AnofoxAftDistribution dist) {
	if (t <= 0.0) return 0.0;
	return kernel_cdf((int)dist, (log(t) - eta) / scale);
}

double anofox_aft_quantile(double p, double eta, double scale, AnofoxAftDistribution dist) {
	return exp(eta + scale * kernel_quantile((int)dist, p));
}

} // extern "C"
