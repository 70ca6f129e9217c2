// quantile.hip — grouped quantile regression: one wavefront per group runs the exact simplex of quantile_solve.h over the
// group's rows, and the entry points anofox_hip_quantile_fit_batch_{device,host}, anofox_hip_quantile_fit_predict_batch_*,
// anofox_quantile_fit / anofox_free_quantile_result, their tau-path siblings (*_path_*) and the window function
// anofox_hip_quantile_fit_predict_{window,frames}_*.
//
// The contract and the method: quantile_solve.h and DESIGN.md §1, "Quantile regression".
//   quantile_fit_kernel: 64 lanes per workgroup = one wavefront per group (grid-stride over the groups).  LDS holds B^-1 and
//     the LU workspace (k x k doubles each, k = p + [intercept] <= 33) and the per-edge vectors: qs_work_doubles(k) * 8 bytes,
//     20.6 KB at k = 33.  Rows are strided over the lanes; residual, z and breakpoint of a row sit in a per-call device
//     scratch (3 doubles per row, the context's workspace) that only the row's own lane touches.
//   quantile_path_kernel: the same wavefront, LDS and scratch for a whole grid of tau (anofox_hip_quantile_fit_path_batch_*,
//     anofox_hip_quantile_fit_predict_path_batch_*, anofox_quantile_fit_path): qs_fit_path begins once and pivots from each
//     tau's vertex to the next; the grid (sorted by the host, at most kQsMaxTaus) travels in the kernel arguments.  With a
//     prediction buffer the wavefront writes pred[i T + t] = a_i'beta_t of its group's rows right after tau_t's record.
//   quantile_window_kernel: the window function (anofox_hip_quantile_fit_predict_{window,frames}_*).  One wavefront per WALKER,
//     grid-stride over the walkers: a walker is a run of consecutive output rows of one partition, and qs_fit_window carries the
//     optimal vertex from each row's frame to the next.  The same LDS; the scratch is a slab of 3 doubles per row of the longest
//     span of any run (last frame's end - first frame's start) that belongs to the LAUNCHED wavefront (blockIdx), indexed by
//     row - origin, so overlapping frames of neighbouring walkers never share a slot.  plan_window below cuts the runs.
//   quantile_nan_bounds_kernel: the fit-predict entry points hand the records (regression layout, sigma = NaN) to the
//     existing predict kernels, which give yhat = lower = upper for a NaN sigma; quantile regression has no interval, so
//     the two bounds are then overwritten with NaN.
// No atomics: a group is one wavefront's own work in a fixed order, so repeated calls give identical bytes.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "quantile_solve.h"

using namespace anofox;

#include "host_stage.h"
#include "scalar_fit.h"
#include "window_plan.h"

using namespace anofox::host;
using namespace anofox::quantile;

namespace {

struct QuantileArgs {
	const int64_t *row_offsets;  // [G + 1]
	const int64_t *train_counts; // [G] or nullptr: what the "fewer than 2 rows -> NULL" rule looks at
	const double *y;
	const double *x[kQsMaxP];
	double *scratch; // [3 x n_rows]
	int64_t n_rows;
	int64_t n_groups;
	int p;
	int fit_intercept;
	double tau;
	int max_iterations;
	int invalid;        // tau outside (0, 1): every group gets ANOFOX_ERROR_INVALID_INPUT
	int predict_layout; // 1: the regression layout for the predict kernels
	double *core;       // [G x (p + 6)]
	int32_t *iterations; // [G] or nullptr
};

__global__ __launch_bounds__(64) void quantile_fit_kernel(QuantileArgs a) {
	extern __shared__ double quantile_lds[];
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		QsProblem P;
		P.y = a.y;
		P.x = a.x;
		P.p = a.p;
		P.fit_intercept = a.fit_intercept;
		P.lo = a.row_offsets[g];
		P.hi = a.row_offsets[g + 1];
		P.rule_count = a.train_counts ? a.train_counts[g] : P.hi - P.lo;
		P.tau = a.tau;
		P.max_iterations = a.max_iterations;
		P.predict_layout = a.predict_layout;
		P.r = a.scratch;
		P.z = a.scratch + a.n_rows;
		P.t = a.scratch + 2 * a.n_rows;
		qs_fit(P, a.invalid != 0, quantile_lds, a.core + g * (int64_t)(a.p + 6), a.iterations ? a.iterations + g : nullptr);
		__syncthreads(); // the next group reuses the LDS
	}
}

struct QuantilePathArgs {
	QuantileArgs q;           // tau, invalid and predict_layout unused; core [G x T x (p + 6)], iterations [G x T] or nullptr
	double *pred;             // [n_rows x T] or nullptr
	int n_taus, n_ok;         // T; the valid tau among them
	double taus[kQsMaxTaus];  // the valid tau ascending (qs_order_taus)
	uint8_t slot[kQsMaxTaus]; // the caller's position of taus[t]; [n_ok, T): the invalid positions
};

__global__ __launch_bounds__(64) void quantile_path_kernel(QuantilePathArgs a) {
	extern __shared__ double quantile_lds[];
	const int64_t T = a.n_taus;
	for (int64_t g = blockIdx.x; g < a.q.n_groups; g += gridDim.x) {
		QsProblem P;
		P.y = a.q.y;
		P.x = a.q.x;
		P.p = a.q.p;
		P.fit_intercept = a.q.fit_intercept;
		P.lo = a.q.row_offsets[g];
		P.hi = a.q.row_offsets[g + 1];
		P.rule_count = a.q.train_counts ? a.q.train_counts[g] : P.hi - P.lo;
		P.tau = NAN;
		P.max_iterations = a.q.max_iterations;
		P.predict_layout = 0;
		P.r = a.q.scratch;
		P.z = a.q.scratch + a.q.n_rows;
		P.t = a.q.scratch + 2 * a.q.n_rows;
		qs_fit_path(P, a.taus, a.slot, a.n_ok, a.n_taus, quantile_lds, a.q.core + g * T * (int64_t)(a.q.p + 6),
		            a.q.iterations ? a.q.iterations + g * T : nullptr, a.pred);
		__syncthreads(); // the next group reuses the LDS
	}
}

struct QuantileWindowArgs {
	const int64_t *lo, *hi;   // [n_rows]: the frame of output row e is rows [lo[e], hi[e])
	const int64_t *run_begin; // [n_runs + 1]: walker w owns the output rows [run_begin[w], run_begin[w + 1])
	const double *y;
	const double *x[kQsMaxP];
	double *scratch; // [gridDim.x x 3 x slab_rows]
	int32_t *cold;   // [n_runs x 2]: the frames of walker w that began afresh, and those of them that followed a fitted frame
	int64_t n_runs;
	int64_t slab_rows;
	int p;
	int fit_intercept;
	double tau;
	int max_iterations;
	int invalid;
	double *pred;        // [n_rows x 3]
	double *rec;         // [n_rows x (p + 6)] or nullptr
	int32_t *iterations; // [n_rows] or nullptr
};

__global__ __launch_bounds__(64) void quantile_window_kernel(QuantileWindowArgs a) {
	extern __shared__ double quantile_lds[];
	double *slab = a.scratch + (int64_t)blockIdx.x * 3 * a.slab_rows; // this wavefront's, whichever walker it runs
	for (int64_t w = blockIdx.x; w < a.n_runs; w += gridDim.x) {
		QsProblem P;
		P.y = a.y;
		P.x = a.x;
		P.p = a.p;
		P.fit_intercept = a.fit_intercept;
		P.lo = P.hi = 0;
		P.rule_count = 0;
		P.tau = a.tau;
		P.max_iterations = a.max_iterations;
		P.predict_layout = 0;
		P.r = slab;
		P.z = slab + a.slab_rows;
		P.t = slab + 2 * a.slab_rows;
		int64_t n_restart = 0;
		const int64_t n_cold = qs_fit_window(P, a.invalid != 0, a.lo, a.hi, a.run_begin[w], a.run_begin[w + 1], a.slab_rows, quantile_lds,
		                                     a.pred, a.rec, a.iterations, nullptr, &n_restart);
		if (threadIdx.x == 0) {
			a.cold[2 * w] = (int32_t)n_cold;
			a.cold[2 * w + 1] = (int32_t)n_restart;
		}
		__syncthreads(); // the next walker reuses the LDS and the slab
	}
}

__global__ __launch_bounds__(256) void quantile_nan_bounds_kernel(double *pred, int64_t n_rows) {
	const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_rows) return;
	pred[3 * r + 1] = NAN;
	pred[3 * r + 2] = NAN;
}

bool tau_invalid(double tau) { return !(tau > 0.0 && tau < 1.0); } // (NaN fails both)

const char *const kOverWidth = "quantile regression: n_features > 32 is not built";

bool check_quantile(int64_t G, size_t p, int64_t n_rows, const void *off, const void *y, const double *const *x_cols, const void *out,
                    AnofoxError *e) {
	return check_batch_args(G, p, n_rows, off, y, x_cols, out, kQsMaxP, kOverWidth, "row_offsets, y or an output is NULL", false, e);
}

void fill_args(QuantileArgs &a, AnofoxHipContext *ctx, int64_t G, size_t p, size_t rows, const int64_t *d_off, const double *d_y,
               const double *const *x_cols, const int64_t *d_tc, const AnofoxHipQuantileBatchOptions &o, int predict_layout, double *d_core,
               int32_t *d_iterations) {
	memset(&a, 0, sizeof a);
	a.row_offsets = d_off;
	a.train_counts = d_tc;
	a.y = d_y;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.scratch = (double *)ctx->ws;
	a.n_rows = (int64_t)rows;
	a.n_groups = G;
	a.p = (int)p;
	a.fit_intercept = o.fit_intercept ? 1 : 0;
	a.tau = o.tau;
	a.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	a.invalid = tau_invalid(o.tau) ? 1 : 0;
	a.predict_layout = predict_layout;
	a.core = d_core;
	a.iterations = d_iterations;
}

// the fit of G groups on device-resident inputs, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_quantile(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const int64_t *d_off, const double *d_y,
                     const double *const *x_cols, const int64_t *d_tc, const AnofoxHipQuantileBatchOptions &o, int predict_layout,
                     double *d_core, int32_t *d_iterations, AnofoxError *e) {
	if (G == 0) return true;
	const size_t rows = n_rows > 0 ? (size_t)n_rows : 1;
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, 3 * rows * sizeof(double), "quantile scratch", e)) return false;
	QuantileArgs a;
	fill_args(a, ctx, G, p, rows, d_off, d_y, x_cols, d_tc, o, predict_layout, d_core, d_iterations);
	const int k = (int)p + a.fit_intercept;
	const size_t lds = qs_work_doubles(k) * sizeof(double);
	const int64_t max_blocks = 1 << 20;
	hipLaunchKernelGGL(quantile_fit_kernel, dim3((unsigned)(G < max_blocks ? G : max_blocks)), dim3(64), lds, ctx->stream, a);
	return !hip_fail(hipGetLastError(), "quantile_fit_kernel", e);
}

bool check_taus(const double *taus, size_t n_taus, AnofoxError *e) {
	if (!taus || n_taus == 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "taus is NULL or empty"); return false; }
	if (n_taus > (size_t)kQsMaxTaus) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "quantile path: n_taus > 64 is not built"); return false; }
	return true;
}

// the tau path of G groups on device-resident inputs (ctx->mu held by the caller); taus: host memory, checked by check_taus;
// d_pred: [n_rows x T] or nullptr.  options.tau is not read.
bool launch_quantile_path(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const int64_t *d_off, const double *d_y,
                          const double *const *x_cols, const int64_t *d_tc, const AnofoxHipQuantileBatchOptions &o, const double *taus,
                          size_t n_taus, double *d_rec, int32_t *d_iterations, double *d_pred, AnofoxError *e) {
	if (G == 0) return true;
	const size_t rows = n_rows > 0 ? (size_t)n_rows : 1;
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, 3 * rows * sizeof(double), "quantile scratch", e)) return false;
	QuantilePathArgs a;
	memset(&a, 0, sizeof a);
	fill_args(a.q, ctx, G, p, rows, d_off, d_y, x_cols, d_tc, o, 0, d_rec, d_iterations);
	a.pred = d_pred;
	a.n_taus = (int)n_taus;
	a.n_ok = qs_order_taus(taus, (int)n_taus, a.taus, a.slot);
	const int k = (int)p + a.q.fit_intercept;
	const size_t lds = qs_work_doubles(k) * sizeof(double);
	const int64_t max_blocks = 1 << 20;
	hipLaunchKernelGGL(quantile_path_kernel, dim3((unsigned)(G < max_blocks ? G : max_blocks)), dim3(64), lds, ctx->stream, a);
	return !hip_fail(hipGetLastError(), "quantile_path_kernel", e);
}

bool launch_nan_bounds(AnofoxHipContext *ctx, int64_t n_rows, double *d_pred, AnofoxError *e) {
	if (n_rows == 0) return true;
	hipLaunchKernelGGL(quantile_nan_bounds_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, d_pred, n_rows);
	return !hip_fail(hipGetLastError(), "quantile_nan_bounds_kernel", e);
}

// ---- the one-group entry points (anofox_quantile_fit, anofox_quantile_fit_path) ----
// a record's status != 0 as the reference's error
void set_quantile_fit_error(int status, const ScalarFitInput &in, AnofoxError *out_error) {
	set_scalar_fit_error(status, status == ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS ? ANOFOX_ERROR_INSUFFICIENT_DATA : (AnofoxErrorCode)status, in,
	                     "Quantile fit failed on the GPU path", out_error);
}

// the malloc'ed result of one record
bool fill_quantile_result(const double *rec, size_t p, AnofoxQuantileFitResultCore *out_core, AnofoxError *out_error) {
	double *coef = copy_coefficients(rec, p, out_error);
	if (!coef) return false;
	out_core->coefficients = coef;
	out_core->coefficients_len = p;
	out_core->intercept = rec[p];
	out_core->tau = rec[p + 1];
	out_core->n_observations = (size_t)rec[p + 4];
	out_core->n_features = p;
	return true;
}

// ---- the window function ----
// The planner.  cut_window_runs (window_plan.h) cuts the partitions into the walkers' runs.  span = the longest
// chain of a run (last hi - first lo of consecutive monotone, overlapping frames); a launched wavefront owns 3 span doubles, and
// waves = min(runs, kQwMaxWaves, cap / (24 span)): the scratch never exceeds the cap (kQwScratchCap unless a test sets
// another), and a span that does not fit once fails the call.
constexpr int64_t kQwMaxWaves = kWalkMaxWaves;
constexpr int64_t kQwScratchCap = kWalkScratchCap;

std::mutex g_qw_mu;
int64_t g_qw_run_length = 0, g_qw_scratch_cap = 0; // anofox_hip_quantile_window_test_hooks (0: the rule above)

struct WindowPlan {
	std::vector<int64_t> run_begin; // walkers + 1
	int64_t span = 0, waves = 0;
};

bool plan_window(int64_t n_parts, const int64_t *off, const int64_t *lo, const int64_t *hi, int64_t run_length, int64_t cap_bytes,
                 WindowPlan &plan, AnofoxError *e) {
	plan.span = plan.waves = 0;
	if (cap_bytes <= 0) cap_bytes = kQwScratchCap;
	cut_window_runs(n_parts, off, lo, hi, run_length, plan.run_begin);
	const int64_t runs = (int64_t)plan.run_begin.size() - 1;
	if (runs == 0) return true;
	// the walk sets its scratch origin wherever it begins afresh, so a slab has to hold the longest CHAIN of a run: consecutive
	// non-empty frames whose bounds are both non-decreasing and that overlap (qs_fit_window's rule; a basis row that leaves or
	// a failed frame only cuts a chain shorter).  Unsorted or far-apart explicit frames therefore cost no scratch.
	for (int64_t w = 0; w < runs; ++w) {
		bool have = false;
		int64_t origin = 0, plo = 0, phi = 0;
		for (int64_t r = plan.run_begin[(size_t)w]; r < plan.run_begin[(size_t)w + 1]; ++r) {
			if (hi[r] <= lo[r]) { have = false; continue; }
			if (!(have && lo[r] >= plo && hi[r] >= phi && lo[r] < phi)) origin = lo[r];
			have = true;
			plo = lo[r];
			phi = hi[r];
			if (phi - origin > plan.span) plan.span = phi - origin;
		}
	}
	if (plan.span < 1) plan.span = 1;
	const int64_t fit = cap_bytes / (3 * (int64_t)sizeof(double)) / plan.span;
	if (fit < 1) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT,
		          "quantile window: frame span " + std::to_string(plan.span) + " exceeds the scratch budget (" + std::to_string(cap_bytes) +
		              " bytes, 24 per row)");
		return false;
	}
	plan.waves = runs < kQwMaxWaves ? runs : kQwMaxWaves;
	if (fit < plan.waves) plan.waves = fit;
	return true;
}

bool check_window_args(int64_t n_rows, size_t p, const void *y, const double *const *x_cols, const void *pred, AnofoxError *e) {
	return check_batch_args(0, p, n_rows, nullptr, y, x_cols, pred, kQsMaxP, kOverWidth, "y or pred is NULL", true, e);
}

// The walk of a planned call on device-resident rows and frames (ctx->mu held by the caller).  The workspace holds the slabs,
// then the run table, which is copied before the launch (the stream is synchronised: the plan is the caller's local).  The
// walkers' cold-start counts go to a buffer of the context that nothing else uses (anofox_hip_quantile_window_stats).
bool launch_quantile_window(AnofoxHipContext *ctx, size_t p, int64_t n_rows, const double *d_y, const double *const *x_cols,
                            const int64_t *d_lo, const int64_t *d_hi, const WindowPlan &plan, const AnofoxHipQuantileBatchOptions &o,
                            double *d_pred, double *d_rec, int32_t *d_iterations, AnofoxError *e) {
	const int64_t runs = (int64_t)plan.run_begin.size() - 1;
	ctx->qw_valid = false;
	if (runs <= 0 || n_rows == 0) return true;
	const size_t slabs = align_up((size_t)plan.waves * 3 * (size_t)plan.span * sizeof(double), 256);
	const size_t table = align_up(((size_t)runs + 1) * sizeof(int64_t), 256);
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, slabs + table, "quantile window scratch", e)) return false;
	if (!ensure_buffer(&ctx->qw_counts, &ctx->qw_counts_bytes, 2 * (size_t)runs * sizeof(int32_t), "quantile window counts", e)) return false;
	QuantileWindowArgs a;
	memset(&a, 0, sizeof a);
	a.lo = d_lo;
	a.hi = d_hi;
	a.run_begin = (const int64_t *)((char *)ctx->ws + slabs);
	a.y = d_y;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.scratch = (double *)ctx->ws;
	a.cold = (int32_t *)ctx->qw_counts;
	a.n_runs = runs;
	a.slab_rows = plan.span;
	a.p = (int)p;
	a.fit_intercept = o.fit_intercept ? 1 : 0;
	a.tau = o.tau;
	a.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	a.invalid = tau_invalid(o.tau) ? 1 : 0;
	a.pred = d_pred;
	a.rec = d_rec;
	a.iterations = d_iterations;
	if (hip_fail(hipMemcpyAsync((void *)a.run_begin, plan.run_begin.data(), ((size_t)runs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream),
	             "H2D", e) ||
	    hip_fail(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize", e))
		return false;
	const int k = (int)p + a.fit_intercept;
	hipLaunchKernelGGL(quantile_window_kernel, dim3((unsigned)plan.waves), dim3(64), qs_work_doubles(k) * sizeof(double), ctx->stream, a);
	if (hip_fail(hipGetLastError(), "quantile_window_kernel", e)) return false;
	ctx->qw_frames = n_rows;
	ctx->qw_walkers = runs;
	ctx->qw_waves = plan.waves;
	ctx->qw_span = plan.span;
	ctx->qw_valid = true;
	return true;
}

void window_hooks(int64_t *run_length, int64_t *cap) {
	std::lock_guard<std::mutex> lk(g_qw_mu);
	*run_length = g_qw_run_length;
	*cap = g_qw_scratch_cap;
}

} // namespace

extern "C" {

size_t anofox_hip_quantile_record_len(size_t p) { return p + 6; }

bool anofox_hip_quantile_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                          const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                          AnofoxHipQuantileBatchOptions options, double *d_quantile, int32_t *d_iterations,
                                          AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_quantile, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_quantile(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, nullptr, options, 0, d_quantile, d_iterations,
	                       out_error);
}

bool anofox_hip_quantile_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                        const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                        AnofoxHipQuantileBatchOptions options, double *quantile, int32_t *iterations,
                                        AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, row_offsets, y, x_cols, quantile, out_error)) return false;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!(ctx = host_context(ctx, out_error))) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features;
	return fit_slabs_host(ctx, n_groups, p, row_offsets, y, x_cols, nullptr, SlabOutputs{quantile, p + 6, iterations, 1}, kPlainSlab, out_error,
	                      [&](int64_t G, int64_t R, const int64_t *, const int64_t *d_off, const StagedColumns &c, double *d_rec, int32_t *d_it, double *) {
		                      return launch_quantile(ctx, G, p, R, d_off, c.y, c.x, nullptr, options, 0, d_rec, d_it, out_error);
	                      });
}

bool anofox_hip_quantile_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                  const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                  const int64_t *d_train_counts, AnofoxHipQuantileBatchOptions options, double *d_core,
                                                  double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_core, out_error)) return false;
	if (n_groups > 0 && !d_pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	if (n_groups == 0) return true;
	std::lock_guard<std::mutex> lk(ctx->mu); // one lock over fit, predict and the bounds: calls on a context are serialised
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_quantile(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_train_counts, options, 1, d_core, nullptr, out_error) &&
	       // the regression predict kernels on the records (sigma = NaN: no interval)
	       predict_records_locked(ctx, n_groups, n_features, n_rows, d_row_offsets, x_cols, d_core, 0.95, d_pred, out_error) &&
	       launch_nan_bounds(ctx, n_rows, d_pred, out_error);
}

bool anofox_hip_quantile_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                const int64_t *train_counts, AnofoxHipQuantileBatchOptions options, double *core,
                                                double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, row_offsets, y, x_cols, core, out_error)) return false;
	if (n_groups > 0 && !pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_whole_range(n_groups, n_rows, row_offsets, out_error)) return false;
	if (!(ctx = host_context(ctx, out_error))) return false;
	const size_t p = n_features, core_len = p + 6, G = (size_t)n_groups, N = (size_t)n_rows;
	std::lock_guard<std::mutex> lk(ctx->mu); // one lock over staging, fit, predict and the copies back
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off, *d_tc;
	StagedColumns c;
	double *d_core, *d_pred;
	if (!stage_call(ctx, out_error, [&](Stage &s) {
		    d_off = s.put(row_offsets, G + 1);
		    d_tc = s.put(train_counts, G);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, nullptr, kPlainColumns);
		    d_core = s.take<double>(G * core_len);
		    d_pred = s.take<double>(3 * N);
	    }))
		return false;
	if (!launch_quantile(ctx, n_groups, p, n_rows, d_off, c.y, c.x, d_tc, options, 1, d_core, nullptr, out_error)) return false;
	if (!predict_records_locked(ctx, n_groups, p, n_rows, d_off, c.x, d_core, 0.95, d_pred, out_error)) return false;
	if (!launch_nan_bounds(ctx, n_rows, d_pred, out_error)) return false;
	if (!d2h(core, d_core, G * core_len * sizeof(double), st, out_error)) return false;
	if (!d2h(pred, d_pred, 3 * N * sizeof(double), st, out_error)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error);
}

bool anofox_hip_quantile_fit_path_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                               const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                               AnofoxHipQuantileBatchOptions options, const double *taus, size_t n_taus,
                                               double *d_quantile, int32_t *d_iterations, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_quantile, out_error)) return false;
	if (!check_taus(taus, n_taus, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_quantile_path(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, nullptr, options, taus, n_taus, d_quantile,
	                            d_iterations, nullptr, out_error);
}

bool anofox_hip_quantile_fit_path_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                             AnofoxHipQuantileBatchOptions options, const double *taus, size_t n_taus, double *quantile,
                                             int32_t *iterations, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, row_offsets, y, x_cols, quantile, out_error)) return false;
	if (!check_taus(taus, n_taus, out_error)) return false;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!(ctx = host_context(ctx, out_error))) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features, T = n_taus;
	return fit_slabs_host(ctx, n_groups, p, row_offsets, y, x_cols, nullptr, SlabOutputs{quantile, T * (p + 6), iterations, T}, kPlainSlab, out_error,
	                      [&](int64_t G, int64_t R, const int64_t *, const int64_t *d_off, const StagedColumns &c, double *d_rec, int32_t *d_it, double *) {
		                      return launch_quantile_path(ctx, G, p, R, d_off, c.y, c.x, nullptr, options, taus, T, d_rec, d_it, nullptr, out_error);
	                      });
}

bool anofox_hip_quantile_fit_predict_path_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                       const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                       const int64_t *d_train_counts, AnofoxHipQuantileBatchOptions options,
                                                       const double *taus, size_t n_taus, double *d_quantile, int32_t *d_iterations,
                                                       double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_quantile, out_error)) return false;
	if (!check_taus(taus, n_taus, out_error)) return false;
	if (n_groups > 0 && !d_pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	if (n_groups == 0) return true;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_quantile_path(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_train_counts, options, taus, n_taus,
	                            d_quantile, d_iterations, d_pred, out_error);
}

bool anofox_hip_quantile_fit_predict_path_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                     const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                     const int64_t *train_counts, AnofoxHipQuantileBatchOptions options, const double *taus,
                                                     size_t n_taus, double *quantile, int32_t *iterations, double *pred,
                                                     AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_quantile(n_groups, n_features, n_rows, row_offsets, y, x_cols, quantile, out_error)) return false;
	if (!check_taus(taus, n_taus, out_error)) return false;
	if (n_groups > 0 && !pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_whole_range(n_groups, n_rows, row_offsets, out_error)) return false; // every row of pred belongs to a group's wavefront
	if (!(ctx = host_context(ctx, out_error))) return false;
	const size_t p = n_features, T = n_taus, rec_len = T * (p + 6), G = (size_t)n_groups, N = (size_t)n_rows;
	std::lock_guard<std::mutex> lk(ctx->mu); // one lock over staging, the kernel and the copies back
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off, *d_tc;
	StagedColumns c;
	double *d_rec, *d_pred;
	int32_t *d_it;
	if (!stage_call(ctx, out_error, [&](Stage &s) {
		    d_off = s.put(row_offsets, G + 1);
		    d_tc = s.put(train_counts, G);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, nullptr, kPlainColumns);
		    d_rec = s.take<double>(G * rec_len);
		    d_it = iterations ? s.take<int32_t>(G * T) : nullptr;
		    d_pred = s.take<double>(N * T);
	    }))
		return false;
	if (!launch_quantile_path(ctx, n_groups, p, n_rows, d_off, c.y, c.x, d_tc, options, taus, T, d_rec, d_it, d_pred, out_error)) return false;
	if (!d2h(quantile, d_rec, G * rec_len * sizeof(double), st, out_error)) return false;
	if (iterations && !d2h(iterations, d_it, G * T * sizeof(int32_t), st, out_error)) return false;
	if (!d2h(pred, d_pred, N * T * sizeof(double), st, out_error)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error);
}

// A batch of one group with anofox_elasticnet_fit's conventions: argument checks first, tau as fit_quantile checks it
// (quantile.rs:35-40, InvalidValue -> InvalidInput), NULL entries -> NaN through the validity bitmask, a one-row input padded
// with an all-NaN row, the reference's error texts (crates/anofox-stats-core/src/errors.rs), the coefficients malloc'ed.
bool anofox_quantile_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxQuantileOptions options,
                         AnofoxQuantileFitResultCore *out_core, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_core) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_core is NULL"); return false; }
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (y.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: y cannot be empty"); return false; }
	if (tau_invalid(options.tau)) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Invalid value for tau: tau must be in (0, 1)"); return false; }
	if (!check_column_lengths(y.len, x, x_count, out_error)) return false;
	const size_t p = x_count;
	if (p > (size_t)kQsMaxP) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, kOverWidth); return false; }
	const ScalarFitInput in(y, x, x_count);
	AnofoxHipQuantileBatchOptions o;
	memset(&o, 0, sizeof o);
	o.tau = options.tau;
	o.fit_intercept = options.fit_intercept;
	o.max_iterations = options.max_iterations;
	o.tolerance = options.tolerance;
	std::vector<double> rec(p + 6);
	if (!anofox_hip_quantile_fit_batch_host(nullptr, 1, p, (int64_t)in.n_pad, in.off, in.yv.data(), in.xp.data(), o, rec.data(), nullptr, out_error))
		return false;
	const int status = (int)rec[p + 5];
	if (status != ANOFOX_ERROR_SUCCESS) {
		set_quantile_fit_error(status, in, out_error);
		return false;
	}
	return fill_quantile_result(rec.data(), p, out_core, out_error);
}

// anofox_quantile_fit at every tau of a grid, through one anofox_hip_quantile_fit_path_batch_host call of one group.  The
// checks, their order and the error texts are anofox_quantile_fit's; any tau outside (0, 1) fails the call.  On failure no
// result holds memory.
bool anofox_quantile_fit_path(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxQuantileOptions options,
                              const double *taus, size_t n_taus, AnofoxQuantileFitResultCore *out_results, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_results) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_results is NULL"); return false; }
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (y.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: y cannot be empty"); return false; }
	if (!check_taus(taus, n_taus, out_error)) return false;
	for (size_t t = 0; t < n_taus; ++t)
		if (tau_invalid(taus[t])) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Invalid value for tau: tau must be in (0, 1)"); return false; }
	if (!check_column_lengths(y.len, x, x_count, out_error)) return false;
	const size_t p = x_count;
	if (p > (size_t)kQsMaxP) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, kOverWidth); return false; }
	const ScalarFitInput in(y, x, x_count);
	AnofoxHipQuantileBatchOptions o;
	memset(&o, 0, sizeof o);
	o.fit_intercept = options.fit_intercept;
	o.max_iterations = options.max_iterations;
	o.tolerance = options.tolerance;
	std::vector<double> rec(n_taus * (p + 6));
	if (!anofox_hip_quantile_fit_path_batch_host(nullptr, 1, p, (int64_t)in.n_pad, in.off, in.yv.data(), in.xp.data(), o, taus, n_taus, rec.data(),
	                                             nullptr, out_error))
		return false;
	for (size_t t = 0; t < n_taus; ++t) {
		const double *r = rec.data() + t * (p + 6);
		const int status = (int)r[p + 5];
		if (status != ANOFOX_ERROR_SUCCESS) set_quantile_fit_error(status, in, out_error);
		if (status != ANOFOX_ERROR_SUCCESS || !fill_quantile_result(r, p, &out_results[t], out_error)) {
			for (size_t u = 0; u < t; ++u) anofox_free_quantile_result(&out_results[u]);
			return false;
		}
	}
	return true;
}

// ---- the window function: anofox_hip_quantile_fit_predict_{window,frames}_{device,host} ----
// The device variants read the partition offsets / the frame bounds back to the host for the planner (one synchronising copy).

bool anofox_hip_quantile_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                   const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                                   AnofoxHipWindowFrame frame, AnofoxHipQuantileBatchOptions options, double *d_pred,
                                                   double *d_quantile, int32_t *d_iterations, AnofoxError *out_error) {
	reset_error(out_error);
	if (n_groups < 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (!check_window_args(n_rows, n_features, d_y, x_cols, d_pred, out_error)) return false;
	if (!check_window_frame(frame, out_error)) return false;
	if (n_groups > 0 && !d_row_offsets) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "row_offsets is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	if (n_groups == 0 || n_rows == 0) return true;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	hipStream_t st = ctx->stream;
	const size_t G = (size_t)n_groups, N = (size_t)n_rows;
	std::vector<int64_t> off(G + 1), lo(N), hi(N);
	if (!d2h(off.data(), d_row_offsets, (G + 1) * sizeof(int64_t), st, out_error)) return false;
	if (hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error)) return false;
	if (!check_window_offsets(n_groups, n_rows, off.data(), out_error)) return false;
	rows_frames(n_groups, off.data(), frame, lo.data(), hi.data());
	int64_t run_length, cap;
	window_hooks(&run_length, &cap);
	WindowPlan plan;
	if (!plan_window(n_groups, off.data(), lo.data(), hi.data(), run_length, cap, plan, out_error)) return false;
	const size_t b = Stage::bytes(N, sizeof(int64_t));
	if (!ensure_buffer(&ctx->frames_buf, &ctx->frames_bytes, 2 * b, "window frames", out_error)) return false;
	int64_t *d_lo = (int64_t *)ctx->frames_buf, *d_hi = (int64_t *)((char *)ctx->frames_buf + b);
	if (!h2d(d_lo, lo.data(), N * sizeof(int64_t), st, out_error) || !h2d(d_hi, hi.data(), N * sizeof(int64_t), st, out_error)) return false;
	return launch_quantile_window(ctx, n_features, n_rows, d_y, x_cols, d_lo, d_hi, plan, options, d_pred, d_quantile, d_iterations, out_error);
}

bool anofox_hip_quantile_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                                   const double *const *x_cols, const int64_t *d_frame_lo, const int64_t *d_frame_hi,
                                                   AnofoxHipQuantileBatchOptions options, double *d_pred, double *d_quantile,
                                                   int32_t *d_iterations, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_window_args(n_rows, n_features, d_y, x_cols, d_pred, out_error)) return false;
	if (n_rows > 0 && (!d_frame_lo || !d_frame_hi)) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "frame_lo or frame_hi is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	if (n_rows == 0) return true;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	hipStream_t st = ctx->stream;
	const size_t N = (size_t)n_rows;
	std::vector<int64_t> lo(N), hi(N);
	if (!d2h(lo.data(), d_frame_lo, N * sizeof(int64_t), st, out_error) || !d2h(hi.data(), d_frame_hi, N * sizeof(int64_t), st, out_error)) return false;
	if (hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error)) return false;
	if (!check_host_frames(n_rows, lo.data(), hi.data(), out_error)) return false;
	const int64_t off[2] = {0, n_rows};
	int64_t run_length, cap;
	window_hooks(&run_length, &cap);
	WindowPlan plan;
	if (!plan_window(1, off, lo.data(), hi.data(), run_length, cap, plan, out_error)) return false;
	return launch_quantile_window(ctx, n_features, n_rows, d_y, x_cols, d_frame_lo, d_frame_hi, plan, options, d_pred, d_quantile, d_iterations,
	                              out_error);
}

namespace {
// both host entry points: the frames are the caller's (frames) or come from the ROWS spec (window); one lock over staging,
// the kernel and the copies back
bool quantile_window_host(AnofoxHipContext *ctx, int64_t n_parts, const int64_t *off, size_t p, int64_t n_rows, const double *y,
                          const double *const *x_cols, const int64_t *lo, const int64_t *hi, const AnofoxHipQuantileBatchOptions &options,
                          double *pred, double *quantile, int32_t *iterations, AnofoxError *out_error) {
	int64_t run_length, cap;
	window_hooks(&run_length, &cap);
	WindowPlan plan;
	if (!plan_window(n_parts, off, lo, hi, run_length, cap, plan, out_error)) return false;
	if (!(ctx = host_context(ctx, out_error))) return false;
	const size_t N = (size_t)n_rows, rec_len = p + 6;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_lo, *d_hi;
	StagedColumns c;
	double *d_pred, *d_rec;
	int32_t *d_it;
	if (!stage_call(ctx, out_error, [&](Stage &s) {
		    d_lo = s.put(lo, N);
		    d_hi = s.put(hi, N);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, nullptr, kPlainColumns);
		    d_pred = s.take<double>(3 * N);
		    d_rec = quantile ? s.take<double>(N * rec_len) : nullptr;
		    d_it = iterations ? s.take<int32_t>(N) : nullptr;
	    }))
		return false;
	if (!launch_quantile_window(ctx, p, n_rows, c.y, c.x, d_lo, d_hi, plan, options, d_pred, d_rec, d_it, out_error)) return false;
	if (!d2h(pred, d_pred, 3 * N * sizeof(double), st, out_error)) return false;
	if (quantile && !d2h(quantile, d_rec, N * rec_len * sizeof(double), st, out_error)) return false;
	if (iterations && !d2h(iterations, d_it, N * sizeof(int32_t), st, out_error)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error);
}
} // namespace

bool anofox_hip_quantile_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                                 const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                                 AnofoxHipWindowFrame frame, AnofoxHipQuantileBatchOptions options, double *pred,
                                                 double *quantile, int32_t *iterations, AnofoxError *out_error) {
	reset_error(out_error);
	if (n_groups < 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (!check_window_args(n_rows, n_features, y, x_cols, pred, out_error)) return false;
	if (!check_window_frame(frame, out_error)) return false;
	if (n_groups > 0 && !row_offsets) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "row_offsets is NULL"); return false; }
	if (n_groups > 0 && !check_window_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0 || n_rows == 0) return true;
	std::vector<int64_t> lo((size_t)n_rows), hi((size_t)n_rows);
	rows_frames(n_groups, row_offsets, frame, lo.data(), hi.data());
	return quantile_window_host(ctx, n_groups, row_offsets, n_features, n_rows, y, x_cols, lo.data(), hi.data(), options, pred, quantile,
	                            iterations, out_error);
}

bool anofox_hip_quantile_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                                 const double *const *x_cols, const int64_t *frame_lo, const int64_t *frame_hi,
                                                 AnofoxHipQuantileBatchOptions options, double *pred, double *quantile, int32_t *iterations,
                                                 AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_window_args(n_rows, n_features, y, x_cols, pred, out_error)) return false;
	if (n_rows > 0 && (!frame_lo || !frame_hi)) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "frame_lo or frame_hi is NULL"); return false; }
	if (!check_host_frames(n_rows, frame_lo, frame_hi, out_error)) return false;
	if (n_rows == 0) return true;
	const int64_t off[2] = {0, n_rows};
	return quantile_window_host(ctx, 1, off, n_features, n_rows, y, x_cols, frame_lo, frame_hi, options, pred, quantile, iterations, out_error);
}

// The planner alone, on host arrays: run_begin (capacity entries, may be NULL with capacity 0) receives the first output row of
// every walker and one entry past them, *n_runs their number, *span_rows the scratch rows of one wavefront, *n_waves the
// wavefronts a launch would use.  run_length / scratch_cap_bytes 0: the rule of the library.
bool anofox_hip_quantile_window_plan(int64_t n_groups, const int64_t *row_offsets, int64_t n_rows, const int64_t *frame_lo,
                                     const int64_t *frame_hi, int64_t run_length, int64_t scratch_cap_bytes, int64_t *run_begin,
                                     int64_t capacity, int64_t *n_runs, int64_t *span_rows, int64_t *n_waves, AnofoxError *out_error) {
	reset_error(out_error);
	if (n_groups < 0 || n_rows < 0 || !n_runs || !span_rows || !n_waves || (n_groups > 0 && !row_offsets) || (n_rows > 0 && (!frame_lo || !frame_hi))) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "quantile window plan: a NULL or negative argument");
		return false;
	}
	if (n_groups > 0 && !check_window_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (!check_host_frames(n_rows, frame_lo, frame_hi, out_error)) return false;
	WindowPlan plan;
	if (!plan_window(n_groups, row_offsets, frame_lo, frame_hi, run_length, scratch_cap_bytes, plan, out_error)) return false;
	*n_runs = (int64_t)plan.run_begin.size() - 1;
	*span_rows = plan.span;
	*n_waves = plan.waves;
	if (run_begin) {
		if (capacity < (int64_t)plan.run_begin.size()) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "quantile window plan: run_begin is too short"); return false; }
		memcpy(run_begin, plan.run_begin.data(), plan.run_begin.size() * sizeof(int64_t));
	}
	return true;
}

// A test's hook: the run length and the scratch cap of every later window call of the process (0: the library's rule).
void anofox_hip_quantile_window_test_hooks(int64_t run_length, int64_t scratch_cap_bytes) {
	std::lock_guard<std::mutex> lk(g_qw_mu);
	g_qw_run_length = run_length > 0 ? run_length : 0;
	g_qw_scratch_cap = scratch_cap_bytes > 0 ? scratch_cap_bytes : 0;
}

// What the most recent window call on `ctx` (NULL: the thread's default context) did: out[6] = {output rows, frames that began
// afresh, walkers, launched wavefronts, scratch rows per wavefront, restarts = the frames begun afresh right after a fitted
// frame}.  Waits for the context's stream.  The record lives in the context and is reset by every window call on it; without one
// (or after one that launched nothing) the call fails.
bool anofox_hip_quantile_window_stats(AnofoxHipContext *ctx, int64_t *out, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out is NULL"); return false; }
	if (!(ctx = host_context(ctx, out_error))) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (!ctx->qw_valid) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "quantile window stats: no window call on this context"); return false; }
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const int64_t walkers = ctx->qw_walkers;
	std::vector<int32_t> cold(2 * (size_t)walkers);
	if (!d2h(cold.data(), ctx->qw_counts, cold.size() * sizeof(int32_t), ctx->stream, out_error)) return false;
	if (hip_fail(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize", out_error)) return false;
	int64_t begun = 0, restarts = 0;
	for (int64_t w = 0; w < walkers; ++w) {
		begun += cold[2 * (size_t)w];
		restarts += cold[2 * (size_t)w + 1];
	}
	out[0] = ctx->qw_frames;
	out[1] = begun;
	out[2] = walkers;
	out[3] = ctx->qw_waves;
	out[4] = ctx->qw_span;
	out[5] = restarts;
	return true;
}

void anofox_free_quantile_result(AnofoxQuantileFitResultCore *result) {
	if (!result) return;
	free(result->coefficients);
	result->coefficients = nullptr;
	result->coefficients_len = 0;
}

} // extern "C"
