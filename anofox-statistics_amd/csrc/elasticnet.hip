// elasticnet.hip — grouped elastic net fits: a batched covariance-mode coordinate-descent solve on the moment records of
// the accumulate kernels, and the entry points anofox_hip_elasticnet_fit_batch_{device,host} / anofox_elasticnet_fit.
//
// Reference: fit_elasticnet (crates/anofox-stats-core/src/models/elasticnet.rs:29-200): alpha / l1_ratio checks, the row
// filter (finite y and x, no weights), the constant-column test |x - x_first| < 1e-10, the intercept-only shortcut and
// NaN coefficients at constant columns.  Per group ("Elastic net") the solve minimises
//     1/2 sum_i (y_i - b0 - x_i'b)^2 + lam (l1 sum |b_j| + (1 - l1)/2 sum b_j^2)
// over the non-constant columns.  With an intercept C / c are the centred X'X / X'y (the records are shifted by the first
// valid row, so centring is exact), without one the raw moments.  Cyclic coordinate descent from b = 0 in column order:
//     b_j <- S(c_j - sum_{k != j} C_jk b_k, lam l1) / (C_jj + lam (1 - l1))
// until a full sweep moves no coefficient by more than tolerance sqrt(S_yy / C_jj), or max_iterations sweeps.
//   narrow (p <= 8): one LANE per group, C, c and b in registers, the sum formed afresh at every step;
//   wide (9 <= p <= 128): one WAVEFRONT per group, C column-major in LDS, lane k owns b_k and the gradient
//     r_k = c_k - (C b)_k (and k + 64): a coordinate step is a broadcast of r_j, b_j and an axpy of column j into r.
// Statistics as the ridge record (solve_narrow.hip): rss = S_yy - 2 b'c + b'C b; where that falls below 1e-7 of the
// total sum of squares it has cancelled, and rows_rss_kernel sums the squared residuals y - b0 - x'b from the rows.
// No atomics: every group is a lane's or a wavefront's own work, so repeated calls give bit-identical records.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "elasticnet_solve.h"

using namespace anofox;

#include "host_stage.h"
#include "moment_solve.h"
#include "scalar_fit.h"

using namespace anofox::host;

namespace {

// ---- narrow: one lane per group ----
template <int P>
__global__ __launch_bounds__(64) void en_solve_narrow_kernel(BatchArgs a, EnParams en) {
	using L = MomentLayout<P>;
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.n_groups) return;
	const bool icpt = a.fit_intercept != 0;
	const double *rec = a.moments + g * (int64_t)L::REC;
	double *core = a.core + g * (int64_t)(P + 6);
	const int64_t nrows = a.rule_counts ? a.rule_counts[g] : group_row_end(a, g) - a.row_offsets[g];
	double out[P + 6];
	const EnSolveInfo s = en_fit_from_moments<P, false>(rec, en, icpt, nrows, out);
#pragma unroll
	for (int k = 0; k < P + 6; ++k) core[k] = out[k];
	a.refine_list[g] = s.cancels ? 1 : 0;
	if (en.iterations) en.iterations[g] = s.converged ? s.sweeps : -s.sweeps;
}

// ---- wide: one wavefront per group, C in LDS ----
// R = rows of C per lane (1: p <= 64, 2: p <= 128)
template <int R>
__global__ __launch_bounds__(64) void en_solve_wide_kernel(WideArgs a, EnParams en) {
	extern __shared__ double en_lds[]; // [p * p] column-major C, then [p] active flags (as doubles)
	const int p = a.p;
	const int lane = threadIdx.x;
	const int64_t gl = blockIdx.x;
	const int64_t g = a.group_base + gl;
	const bool icpt = a.fit_intercept != 0;
	const WideMoments m(a.moments, gl, p);
	const double *sx = m.sx, *sxy = m.sxy, *fx = m.fx, *nonconst = m.nonconst;
	double *core = a.core + g * (int64_t)(p + 6);
	const double sy = m.sy, syy = m.syy, sw = m.sw, cnt = m.cnt, cyy_c = m.cyy_c;
	const int64_t nrows = a.rule_counts ? a.rule_counts[g] : group_row_end(a, g) - a.row_offsets[g];
	const int p_eff = m.p_eff;
	const double ymean = m.ymean(icpt);
	if (lane == 0) a.refine_list[gl] = 0;
	bool shortcut;
	const int status = en_prechecks(en, nrows, cnt, p_eff, icpt, &shortcut); // (uniform: lane 0 writes)
	if (status != 0 || shortcut) {
		if (lane == 0) {
			if (status != 0) en_write_status(core, p, status);
			else en_write_shortcut(core, p, ymean, cyy_c, cnt);
			if (en.iterations) en.iterations[g] = 0;
		}
		return;
	}
	double *Cs = en_lds;
	double *act = en_lds + (size_t)p * p;
	const double inv_sw = 1.0 / sw;
	for (int idx = lane; idx < p * p; idx += 64) {
		const int j = idx / p, k = idx - j * p; // Cs[j * p + k] = C[k][j]
		Cs[idx] = m.c(j < k ? j : k, j < k ? k : j, icpt, inv_sw);
	}
	for (int j = lane; j < p; j += 64) act[j] = nonconst[j] != 0.0 ? 1.0 : 0.0;
	__syncthreads();

	double r[R], b[R], cc[R];
#pragma unroll
	for (int h = 0; h < R; ++h) {
		const int k = lane + 64 * h;
		cc[h] = k < p ? (icpt ? sxy[k] - sx[k] * sy * inv_sw : sxy[k]) : 0.0;
		r[h] = cc[h];
		b[h] = 0.0;
	}
	const double tss = icpt ? cyy_c : syy;
	double pen1, pen2;
	en_penalty(en, cnt, cyy_c, &pen1, &pen2);
	const double thresh = en.tolerance * sqrt(tss);
	int sweeps = 0;
	bool converged = false;
	while (sweeps < en.max_iterations) {
		++sweeps;
		double dmax = 0.0;
		for (int j = 0; j < p; ++j) {
			if (act[j] == 0.0) continue;
			const int owner = j & 63, h = j >> 6;
			const double rsel = (R == 1 || h == 0) ? r[0] : r[R - 1];
			const double bsel = (R == 1 || h == 0) ? b[0] : b[R - 1];
			const double rj = __shfl(rsel, owner, 64), bj = __shfl(bsel, owner, 64);
			const double cjj = Cs[j * p + j];
			const double bn = soft_threshold(rj + cjj * bj, pen1) / (cjj + pen2);
			const double d = bn - bj;
			dmax = fmax(dmax, sqrt(cjj) * fabs(d));
			if (d != 0.0) {
				const double *col = Cs + j * p;
#pragma unroll
				for (int hh = 0; hh < R; ++hh) {
					const int k = lane + 64 * hh;
					if (k < p) r[hh] = fma(-col[k], d, r[hh]);
				}
				if (lane == owner) {
					if (R == 1 || h == 0) b[0] = bn;
					else b[R - 1] = bn;
				}
			}
		}
		if (dmax <= thresh) { converged = true; break; }
	}
	// rss = S_yy - 2 b'c + b'C b = S_yy - b'(c + r), with C b = c - r; intercept from the column means
	double s_bcr = 0.0, s_bx = 0.0;
#pragma unroll
	for (int h = 0; h < R; ++h) {
		const int k = lane + 64 * h;
		if (k < p) {
			s_bcr += b[h] * (cc[h] + r[h]);
			s_bx += b[h] * (fx[k] * (icpt ? 1.0 : 0.0) + sx[k] * inv_sw);
		}
	}
	for (int m = 32; m >= 1; m >>= 1) {
		s_bcr += __shfl_xor(s_bcr, m, 64);
		s_bx += __shfl_xor(s_bx, m, 64);
	}
#pragma unroll
	for (int h = 0; h < R; ++h) {
		const int k = lane + 64 * h;
		if (k < p) core[k] = act[k] != 0.0 ? b[h] : en_nan();
	}
	if (lane == 0) {
		core[p] = icpt ? ymean - s_bx : en_nan();
		en_write_stats(core, p, tss - s_bcr, tss, cnt, p_eff, icpt, &a.refine_list[gl]);
		if (en.iterations) en.iterations[g] = converged ? sweeps : -sweeps;
	}
}

// ---- rss from the rows of the groups whose moment identity cancelled (moment_solve.h) ----
__global__ __launch_bounds__(64) void rows_rss_kernel(RowsArgs a) {
	const int lane = threadIdx.x;
	const int p = a.p;
	for (int64_t gl = blockIdx.x; gl < a.n_groups; gl += gridDim.x) {
		if (a.flag[gl] == 0) continue;
		const int64_t g = a.group_base + gl;
		double *core = a.core + g * (int64_t)(p + 6);
		const double b0 = a.fit_intercept ? core[p] : 0.0;
		int p_eff = 0;
		for (int j = 0; j < p; ++j) p_eff += isnan(core[j]) ? 0 : 1;
		const double rss = rows_ssr(a, g, core, b0, lane);
		if (lane == 0) {
			const bool icpt = a.fit_intercept != 0;
			const double tss = core[p + 1], cnt = core[p + 4]; // tss parked by the solve
			const double df = cnt - (double)(p_eff + (icpt ? 1 : 0));
			const double r2 = 1.0 - rss / tss;
			core[p + 1] = r2;
			core[p + 2] = 1.0 - (1.0 - r2) * (cnt - (icpt ? 1.0 : 0.0)) / df;
			core[p + 3] = sqrt(rss / df);
		}
	}
}

hipError_t launch_en_narrow(const BatchArgs &a, const EnParams &en, hipStream_t st) {
	return dispatch_narrow(a.p, hipErrorInvalidValue, [&](auto P) {
		hipLaunchKernelGGL((en_solve_narrow_kernel<P()>), dim3((unsigned)((a.n_groups + 63) / 64)), dim3(64), 0, st, a, en);
		return hipGetLastError();
	});
}

hipError_t launch_en_wide(const WideArgs &a, const EnParams &en, hipStream_t st) {
	const size_t lds = ((size_t)a.p * a.p + (size_t)a.p) * sizeof(double);
	return launch_wide_r<en_solve_wide_kernel<1>, en_solve_wide_kernel<2>>(a, en, lds, st);
}

hipError_t launch_rows_rss(const RowsArgs &ra, hipStream_t st) {
	hipLaunchKernelGGL(rows_rss_kernel, dim3(rows_grid(ra.n_groups)), dim3(64), 0, st, ra);
	return hipGetLastError();
}

// the solve stages handed to the batch path (host_api.hip: moment_batch_device)
bool en_narrow_stage(AnofoxHipContext *, BatchArgs &a, hipStream_t st, void *user, AnofoxError *e) {
	const EnParams &en = *static_cast<const EnParams *>(user);
	if (hip_fail(launch_en_narrow(a, en, st), "elastic net solve kernel launch", e)) return false;
	if (!a.row_offsets) return true; // the records of a streaming state: no rows here, its Finalize answers the flagged groups
	return !hip_fail(launch_rows_rss(rows_args(a), st), "elastic net rows kernel launch", e);
}

bool en_wide_stage(AnofoxHipContext *, WideArgs &a, hipStream_t st, int64_t, void *user, AnofoxError *e) {
	const EnParams &en = *static_cast<const EnParams *>(user);
	if (hip_fail(launch_en_wide(a, en, st), "elastic net solve kernel launch", e)) return false;
	return !hip_fail(launch_rows_rss(rows_args(a), st), "elastic net rows kernel launch", e);
}

bool validate_elasticnet_options(const AnofoxHipElasticNetBatchOptions &o, AnofoxError *e);
EnParams elasticnet_params(const AnofoxHipElasticNetBatchOptions &o, int32_t *d_iterations);
SolveStages elasticnet_stages(EnParams *en);

bool validate_en(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const void *off, const void *y, const double *const *x_cols,
                 const AnofoxHipElasticNetBatchOptions &o, const void *core, AnofoxError *e) {
	if (!ctx) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	return check_batch_args(G, p, n_rows, off, y, x_cols, core, kWideMaxP, nullptr, "row_offsets, y or core is NULL", false, e) &&
	       validate_elasticnet_options(o, e);
}

bool run_en(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const int64_t *d_off, const double *d_y, const double *const *x_cols,
            const AnofoxHipElasticNetBatchOptions &o, double *d_core, int32_t *d_iterations, AnofoxError *e) {
	if (G == 0) return true;
	EnParams en = elasticnet_params(o, d_iterations);
	const AnofoxHipBatchOptions acc = unweighted_moment_options(o.fit_intercept, 0.95);
	const SolveStages stages = elasticnet_stages(&en);
	// (the stages run before this call returns: `en` is captured by value into the kernel arguments at launch)
	return moment_batch_device(ctx, G, p, n_rows, d_off, d_y, x_cols, acc, stages, d_core, e);
}

bool validate_elasticnet_options(const AnofoxHipElasticNetBatchOptions &o, AnofoxError *e) {
	if (!(o.tolerance >= 0.0)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "tolerance must be >= 0"); return false; }
	if ((int)o.lambda_scaling != ANOFOX_LAMBDA_SCALING_RAW && (int)o.lambda_scaling != ANOFOX_LAMBDA_SCALING_GLMNET) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "unknown lambda_scaling");
		return false;
	}
	return true;
}

EnParams elasticnet_params(const AnofoxHipElasticNetBatchOptions &o, int32_t *d_iterations) {
	EnParams en;
	en.alpha = o.alpha;
	en.l1_ratio = o.l1_ratio;
	en.tolerance = o.tolerance;
	en.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	en.lambda_scaling = (int)o.lambda_scaling;
	en.iterations = d_iterations;
	return en;
}

SolveStages elasticnet_stages(EnParams *en) { return SolveStages{en_narrow_stage, en_wide_stage, en}; }

// the in-register window kernels (window_narrow.hip, ElasticNetFit); ANOFOX_EN_WINDOW_NARROW=0 sends p <= 8 to the frames path
// as well (A/B switch for measurements)
hipError_t en_window_launch(const WindowArgs &a, void *user, hipStream_t st) {
	return launch_window_predict_en(a, *static_cast<const EnParams *>(user), st);
}

WindowSolve elasticnet_window(EnParams *en) {
	static const bool narrow_on = env_on("ANOFOX_EN_WINDOW_NARROW");
	return WindowSolve{elasticnet_stages(en), narrow_on ? en_window_launch : nullptr, en};
}

} // namespace

namespace anofox {
namespace host {
// the solve as a streaming state's Finalize runs it (agg_state_models.hip)
bool elasticnet_state_options(const AnofoxHipElasticNetBatchOptions &o, AnofoxError *e) { return validate_elasticnet_options(o, e); }
EnParams elasticnet_state_params(const AnofoxHipElasticNetBatchOptions &o) { return elasticnet_params(o, nullptr); }
SolveStages elasticnet_state_stages(EnParams *en) { return elasticnet_stages(en); }
} // namespace host
} // namespace anofox

extern "C" {

bool anofox_hip_elasticnet_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                            AnofoxHipElasticNetBatchOptions options, double *d_core, int32_t *d_iterations,
                                            AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_en(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, options, d_core, out_error)) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const bool ok = run_en(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, options, d_core, d_iterations, out_error);
	ctx->gate_wait = ctx->gate_record = nullptr; // the gate never outlives the call it was set for
	return ok;
}

bool anofox_hip_elasticnet_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                          const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                          AnofoxHipElasticNetBatchOptions options, double *core, int32_t *iterations,
                                          AnofoxError *out_error) {
	reset_error(out_error);
	if (!(ctx = host_context(ctx, out_error))) return false;
	if (!validate_en(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, options, core, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features;
	return fit_slabs_host(ctx, n_groups, p, row_offsets, y, x_cols, nullptr, SlabOutputs{core, p + 6, iterations, 1},
	                      SlabLabels{kNamedColumns, "H2D offsets", "D2H core", "D2H iterations", "D2H"}, out_error,
	                      [&](int64_t G, int64_t R, const int64_t *, const int64_t *d_off, const StagedColumns &c, double *d_core, int32_t *d_it, double *) {
		                      return run_en(ctx, G, p, R, d_off, c.y, c.x, options, d_core, d_it, out_error);
	                      });
}

// A batch of one group with fit_single's conventions (host_api.hip): argument checks first, NULL entries -> NaN through the
// validity bitmask, a one-row input padded with an all-NaN row (the batch applies the aggregate's "< 2 rows" rule), the
// reference's error texts (crates/anofox-stats-core/src/errors.rs), the coefficients malloc'ed.
bool anofox_elasticnet_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxElasticNetOptions options,
                           AnofoxFitResultCore *out_core, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_core) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_core is NULL"); return false; }
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (options.alpha < 0.0) { // elasticnet.rs:33-41: alpha, then l1_ratio, then the inputs
		set_error(out_error, ANOFOX_ERROR_INVALID_ALPHA, "Invalid alpha parameter: " + fmt_g(options.alpha) + " (must be >= 0)");
		return false;
	}
	if (options.l1_ratio < 0.0 || options.l1_ratio > 1.0) {
		set_error(out_error, ANOFOX_ERROR_INVALID_L1_RATIO, "Invalid L1 ratio: " + fmt_g(options.l1_ratio) + " (must be in [0, 1])");
		return false;
	}
	if (y.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: y cannot be empty"); return false; }
	if (!check_column_lengths(y.len, x, x_count, out_error)) return false;
	const size_t p = x_count;
	if (p > (size_t)kWideMaxP) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Elastic Net fit: more than " + std::to_string(kWideMaxP) + " features are not supported by the GPU path");
		return false;
	}
	const ScalarFitInput in(y, x, x_count);
	AnofoxHipElasticNetBatchOptions o;
	memset(&o, 0, sizeof o);
	o.fit_intercept = options.fit_intercept;
	o.alpha = options.alpha;
	o.l1_ratio = options.l1_ratio;
	o.max_iterations = options.max_iterations;
	o.tolerance = options.tolerance;
	o.lambda_scaling = options.lambda_scaling;
	std::vector<double> core(p + 6);
	if (!anofox_hip_elasticnet_fit_batch_host(nullptr, 1, p, (int64_t)in.n_pad, in.off, in.yv.data(), in.xp.data(), o, core.data(), nullptr, out_error))
		return false;
	const int status = (int)core[p + 5];
	if (status != ANOFOX_ERROR_SUCCESS) {
		set_scalar_fit_error(status, (AnofoxErrorCode)status, in, "Elastic Net fit failed on the GPU path", out_error);
		return false;
	}
	return fill_scalar_result(core.data(), p, out_core, out_error);
}

// ---- elastic net fit-predict (anofox_stats_elasticnet_fit_predict_agg, anofox_stats_elasticnet_fit_predict): the elastic net
// record has the regression layout (p + 6), so the predict kernels and the frames path's predict apply unchanged ----

bool anofox_hip_elasticnet_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                    const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                    const int64_t *d_train_counts, AnofoxHipElasticNetBatchOptions options,
                                                    double confidence_level, double *d_core, double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_elasticnet_options(options, out_error)) return false;
	EnParams en = elasticnet_params(options, nullptr);
	return model_fit_predict_batch_device(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_train_counts,
	                                      unweighted_moment_options(options.fit_intercept, confidence_level), elasticnet_stages(&en), d_core, d_pred, out_error);
}

bool anofox_hip_elasticnet_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                  const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                  const int64_t *train_counts, AnofoxHipElasticNetBatchOptions options,
                                                  double confidence_level, double *core, double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_elasticnet_options(options, out_error)) return false;
	EnParams en = elasticnet_params(options, nullptr);
	return model_fit_predict_batch_host(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, train_counts,
	                                    unweighted_moment_options(options.fit_intercept, confidence_level), elasticnet_stages(&en), core, pred, out_error);
}

bool anofox_hip_elasticnet_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                     const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                     AnofoxHipWindowFrame frame, AnofoxHipElasticNetBatchOptions options,
                                                     double confidence_level, double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_elasticnet_options(options, out_error)) return false;
	EnParams en = elasticnet_params(options, nullptr);
	return model_fit_predict_window_device(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, frame,
	                                       unweighted_moment_options(options.fit_intercept, confidence_level), elasticnet_window(&en), d_pred, out_error);
}

bool anofox_hip_elasticnet_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                   const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                   AnofoxHipWindowFrame frame, AnofoxHipElasticNetBatchOptions options,
                                                   double confidence_level, double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_elasticnet_options(options, out_error)) return false;
	EnParams en = elasticnet_params(options, nullptr);
	return model_fit_predict_window_host(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, frame,
	                                     unweighted_moment_options(options.fit_intercept, confidence_level), elasticnet_window(&en), pred, out_error);
}

bool anofox_hip_elasticnet_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                                     const double *const *x_cols, const int64_t *d_frame_lo, const int64_t *d_frame_hi,
                                                     AnofoxHipElasticNetBatchOptions options, double confidence_level, double *d_pred,
                                                     AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_elasticnet_options(options, out_error)) return false;
	EnParams en = elasticnet_params(options, nullptr);
	return model_fit_predict_frames_device(ctx, n_rows, n_features, d_y, x_cols, d_frame_lo, d_frame_hi,
	                                       unweighted_moment_options(options.fit_intercept, confidence_level), elasticnet_stages(&en), d_pred, out_error);
}

bool anofox_hip_elasticnet_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                                   const double *const *x_cols, const int64_t *frame_lo, const int64_t *frame_hi,
                                                   AnofoxHipElasticNetBatchOptions options, double confidence_level, double *pred,
                                                   AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_elasticnet_options(options, out_error)) return false;
	EnParams en = elasticnet_params(options, nullptr);
	return model_fit_predict_frames_host(ctx, n_rows, n_features, y, x_cols, frame_lo, frame_hi,
	                                     unweighted_moment_options(options.fit_intercept, confidence_level), elasticnet_stages(&en), pred, out_error);
}

} // extern "C"
