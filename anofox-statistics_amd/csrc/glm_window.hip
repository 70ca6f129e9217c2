// glm_window.hip — the window function of the GLM family (Poisson / log, binomial / logit): anofox_hip_glm_fit_predict_window_*
// (ROWS frames), anofox_hip_glm_fit_predict_frames_* (explicit bounds), anofox_hip_glm_window_plan / _stats / _test_hooks.
//
// The contract and the method: gi_fit_window in glm_irls.h and DESIGN.md §1, "Generalised linear models", "Window function".
//   glm_window_kernel<EM>: 64 lanes per workgroup = one wavefront per WALKER (grid-stride over the walkers).  A walker owns a
//     run of consecutive output rows of one partition and fits frame after frame with gi_fit; the coefficients stay in LDS
//     between frames, and a frame whose bounds moved forward from a fitted one starts IRLS from them.  LDS: gi_fit's work
//     memory plus the frame's record and the carried coefficients (gi_window_work_doubles).  eta and mu of the current
//     frame sit in the wavefront's own slab of the context's workspace, 16 bytes per row of the longest frame of the call.
//   The planner (window_plan.h cuts the runs, as the quantile window's) sizes the slabs: waves = min(walkers, kWalkMaxWaves,
//     cap / (16 longest frame)), so the scratch never exceeds the cap (1 GiB unless a test sets another); a frame that does
//     not fit once fails the call.
// No atomics: a walker is one wavefront's own work in a fixed order, so repeated calls give identical bytes.
#include <math.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "glm_irls.h"

using namespace anofox;

#include "host_stage.h"
#include "window_plan.h"

using namespace anofox::host;
using namespace anofox::glm;

namespace {

struct GlmWindowArgs {
	const int64_t *lo, *hi;   // [n_rows]: the frame of output row e is rows [lo[e], hi[e])
	const int64_t *run_begin; // [n_runs + 1]: walker w owns the output rows [run_begin[w], run_begin[w + 1])
	const double *y;
	const double *x[kGiMaxP];
	const double *offset; // [n_rows] or nullptr
	double *scratch;      // [gridDim.x x 2 x slab_rows]
	int64_t *counts;      // [n_runs x 4]: gi_fit_window's counts of walker w
	int64_t n_runs;
	int64_t slab_rows;
	int p;
	int fit_intercept;
	int family;
	int max_iterations;
	double tolerance;
	double lambda;
	int invalid; // invalid options: every row gets ANOFOX_ERROR_INVALID_INPUT
	int warm;    // 0: every frame starts cold
	double interval_z;
	double *pred; // [n_rows x 3]
	double *rec;  // [n_rows x (p + 11)] or nullptr
};

template <int EM>
__global__ __launch_bounds__(64) void glm_window_kernel(GlmWindowArgs a) {
	extern __shared__ double glm_window_lds[];
	// the column pointers in LDS: indexing the kernel arguments by a run-time column would make a private copy of them
	__shared__ const double *glm_window_x[kGiMaxP];
#pragma unroll
	for (int j = 0; j < kGiMaxP; ++j)
		if (threadIdx.x == 0) glm_window_x[j] = a.x[j];
	__syncthreads();
	double *slab = a.scratch + (int64_t)blockIdx.x * 2 * a.slab_rows; // this wavefront's, whichever walker it runs
	for (int64_t w = blockIdx.x; w < a.n_runs; w += gridDim.x) {
		GiProblem P;
		P.y = a.y;
		P.x = glm_window_x;
		P.offset = a.offset;
		P.p = a.p;
		P.fit_intercept = a.fit_intercept;
		P.family = a.family;
		P.lo = P.hi = 0;
		P.rule_count = 0;
		P.max_iterations = a.max_iterations;
		P.tolerance = a.tolerance;
		P.lambda = a.lambda;
		P.compute_inference = 0;
		P.zq = NAN;
		P.eta = slab;
		P.mu = slab + a.slab_rows;
		P.interval_z = a.interval_z;
		int64_t *counts = a.counts + 4 * w;
		if (threadIdx.x == 0) counts[0] = counts[1] = counts[2] = counts[3] = 0;
		gi_fit_window<EM>(P, a.invalid != 0, a.warm != 0, a.lo, a.hi, a.run_begin[w], a.run_begin[w + 1], a.slab_rows, glm_window_lds,
		                  a.pred, a.rec, counts, nullptr);
		__syncthreads(); // the next walker reuses the LDS and the slab
	}
}

std::mutex g_gw_mu;
int64_t g_gw_run_length = 0, g_gw_scratch_cap = 0; // anofox_hip_glm_window_test_hooks (0: the library's rule)
int g_gw_warm = 1;

void window_hooks(int64_t *run_length, int64_t *cap, int *warm) {
	std::lock_guard<std::mutex> lk(g_gw_mu);
	*run_length = g_gw_run_length;
	*cap = g_gw_scratch_cap;
	*warm = g_gw_warm;
}

struct GlmWindowPlan {
	std::vector<int64_t> run_begin; // walkers + 1
	int64_t span = 0, waves = 0;    // the rows of the longest frame; the wavefronts to launch
};

// Unlike the quantile walk, only the current frame's eta / mu are live (every fit recomputes them from beta), so a slab
// holds the longest frame, not the longest chain of frames.
bool plan_glm_window(int64_t n_parts, const int64_t *off, const int64_t *lo, const int64_t *hi, int64_t run_length, int64_t cap_bytes,
                     GlmWindowPlan &plan, AnofoxError *e) {
	plan.span = plan.waves = 0;
	if (cap_bytes <= 0) cap_bytes = kWalkScratchCap;
	cut_window_runs(n_parts, off, lo, hi, run_length, plan.run_begin);
	const int64_t runs = (int64_t)plan.run_begin.size() - 1;
	if (runs == 0) return true;
	for (int64_t r = plan.run_begin.front(); r < plan.run_begin.back(); ++r)
		if (hi[r] - lo[r] > plan.span) plan.span = hi[r] - lo[r];
	if (plan.span < 1) plan.span = 1;
	const int64_t fit = cap_bytes / (2 * (int64_t)sizeof(double)) / plan.span;
	if (fit < 1) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT,
		          "glm window: frame of " + std::to_string(plan.span) + " rows exceeds the scratch budget (" + std::to_string(cap_bytes) +
		              " bytes, 16 per row)");
		return false;
	}
	plan.waves = runs < kWalkMaxWaves ? runs : kWalkMaxWaves;
	if (fit < plan.waves) plan.waves = fit;
	return true;
}

bool check_window_args(int64_t n_rows, size_t p, const void *y, const double *const *x_cols, const void *pred, AnofoxError *e) {
	return check_batch_args(0, p, n_rows, nullptr, y, x_cols, pred, kGiMaxP, "glm: n_features > 32 is not built", "y or pred is NULL", true, e);
}

// The walk of a planned call on device-resident rows and frames (ctx->mu held by the caller).  The workspace holds the slabs,
// then the run table, which is copied before the launch (the stream is synchronised: the plan is the caller's local).  The
// walkers' counts go to a buffer of the context that nothing else uses (anofox_hip_glm_window_stats).
bool launch_glm_window(AnofoxHipContext *ctx, size_t p, int64_t n_rows, const double *d_y, const double *const *x_cols,
                       const double *d_offset, const int64_t *d_lo, const int64_t *d_hi, const GlmWindowPlan &plan, int warm,
                       const AnofoxHipGlmBatchOptions &o, double interval_z, double *d_pred, double *d_rec, AnofoxError *e) {
	const int64_t runs = (int64_t)plan.run_begin.size() - 1;
	ctx->gw_valid = false;
	if (runs <= 0 || n_rows == 0) return true;
	const size_t slabs = align_up((size_t)plan.waves * 2 * (size_t)plan.span * sizeof(double), 256);
	const size_t table = align_up(((size_t)runs + 1) * sizeof(int64_t), 256);
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, slabs + table, "glm window scratch", e)) return false;
	if (!ensure_buffer(&ctx->gw_counts, &ctx->gw_counts_bytes, 4 * (size_t)runs * sizeof(int64_t), "glm window counts", e)) return false;
	GlmWindowArgs a;
	memset(&a, 0, sizeof a);
	a.lo = d_lo;
	a.hi = d_hi;
	a.run_begin = (const int64_t *)((char *)ctx->ws + slabs);
	a.y = d_y;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.offset = d_offset;
	a.scratch = (double *)ctx->ws;
	a.counts = (int64_t *)ctx->gw_counts;
	a.n_runs = runs;
	a.slab_rows = plan.span;
	a.p = (int)p;
	a.fit_intercept = o.fit_intercept ? 1 : 0;
	a.family = o.family;
	a.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	a.tolerance = o.tolerance;
	a.lambda = o.lambda;
	a.invalid = glm_options_invalid(o) ? 1 : 0;
	a.warm = warm;
	a.interval_z = interval_z;
	a.pred = d_pred;
	a.rec = d_rec;
	if (hip_fail(hipMemcpyAsync((void *)a.run_begin, plan.run_begin.data(), ((size_t)runs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream),
	             "H2D", e) ||
	    hip_fail(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize", e))
		return false;
	const int k = (int)p + a.fit_intercept;
	const size_t lds = gi_window_work_doubles((int)p, k) * sizeof(double);
	const dim3 grid((unsigned)plan.waves), block(64);
	switch (gi_entry_class(k)) {
	case 1: hipLaunchKernelGGL(glm_window_kernel<1>, grid, block, lds, ctx->stream, a); break;
	case 4: hipLaunchKernelGGL(glm_window_kernel<4>, grid, block, lds, ctx->stream, a); break;
	default: hipLaunchKernelGGL(glm_window_kernel<10>, grid, block, lds, ctx->stream, a); break;
	}
	if (hip_fail(hipGetLastError(), "glm_window_kernel", e)) return false;
	ctx->gw_frames = n_rows;
	ctx->gw_walkers = runs;
	ctx->gw_waves = plan.waves;
	ctx->gw_span = plan.span;
	ctx->gw_valid = true;
	return true;
}

// both host entry points: the frames are the caller's (frames) or come from the ROWS spec (window); one lock over staging,
// the kernel and the copies back
bool glm_window_host(AnofoxHipContext *ctx, int64_t n_parts, const int64_t *off, size_t p, int64_t n_rows, const double *y,
                     const double *const *x_cols, const double *offset, const int64_t *lo, const int64_t *hi,
                     const AnofoxHipGlmBatchOptions &options, double interval_z, double *pred, double *records, AnofoxError *out_error) {
	int64_t run_length, cap;
	int warm;
	window_hooks(&run_length, &cap, &warm);
	GlmWindowPlan plan;
	if (!plan_glm_window(n_parts, off, lo, hi, run_length, cap, plan, out_error)) return false;
	if (!(ctx = host_context(ctx, out_error))) return false;
	const size_t N = (size_t)n_rows, rec_len = p + 11;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_lo, *d_hi;
	StagedColumns c;
	double *d_pred, *d_rec;
	if (!stage_call(ctx, out_error, [&](Stage &s) {
		    d_lo = s.put(lo, N);
		    d_hi = s.put(hi, N);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, offset, kPlainColumns);
		    d_pred = s.take<double>(3 * N);
		    d_rec = records ? s.take<double>(N * rec_len) : nullptr;
	    }))
		return false;
	if (!launch_glm_window(ctx, p, n_rows, c.y, c.x, c.offset, d_lo, d_hi, plan, warm, options, interval_z, d_pred, d_rec, out_error)) return false;
	if (!d2h(pred, d_pred, 3 * N * sizeof(double), st, out_error)) return false;
	if (records && !d2h(records, d_rec, N * rec_len * sizeof(double), st, out_error)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error);
}

} // namespace

extern "C" {

// ---- the device variants read the partition offsets / the frame bounds back to the host for the planner (one synchronising copy) ----

bool anofox_hip_glm_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                              const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                              const double *d_offset, AnofoxHipWindowFrame frame, AnofoxHipGlmBatchOptions options,
                                              double interval_z, double *d_pred, double *d_glm_records, AnofoxError *out_error) {
	reset_error(out_error);
	if (n_groups < 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (!glm_check_interval(options, interval_z, out_error)) return false;
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
	int warm;
	window_hooks(&run_length, &cap, &warm);
	GlmWindowPlan plan;
	if (!plan_glm_window(n_groups, off.data(), lo.data(), hi.data(), run_length, cap, plan, out_error)) return false;
	const size_t b = Stage::bytes(N, sizeof(int64_t));
	if (!ensure_buffer(&ctx->frames_buf, &ctx->frames_bytes, 2 * b, "window frames", out_error)) return false;
	int64_t *d_lo = (int64_t *)ctx->frames_buf, *d_hi = (int64_t *)((char *)ctx->frames_buf + b);
	if (!h2d(d_lo, lo.data(), N * sizeof(int64_t), st, out_error) || !h2d(d_hi, hi.data(), N * sizeof(int64_t), st, out_error)) return false;
	// (launch_glm_window synchronises the stream before it launches: lo / hi are this call's locals)
	return launch_glm_window(ctx, n_features, n_rows, d_y, x_cols, d_offset, d_lo, d_hi, plan, warm, options, interval_z, d_pred,
	                         d_glm_records, out_error);
}

bool anofox_hip_glm_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                              const double *const *x_cols, const double *d_offset, const int64_t *d_frame_lo,
                                              const int64_t *d_frame_hi, AnofoxHipGlmBatchOptions options, double interval_z,
                                              double *d_pred, double *d_glm_records, AnofoxError *out_error) {
	reset_error(out_error);
	if (!glm_check_interval(options, interval_z, out_error)) return false;
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
	int warm;
	window_hooks(&run_length, &cap, &warm);
	GlmWindowPlan plan;
	if (!plan_glm_window(1, off, lo.data(), hi.data(), run_length, cap, plan, out_error)) return false;
	return launch_glm_window(ctx, n_features, n_rows, d_y, x_cols, d_offset, d_frame_lo, d_frame_hi, plan, warm, options, interval_z, d_pred,
	                         d_glm_records, out_error);
}

bool anofox_hip_glm_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *row_offsets, const double *y, const double *const *x_cols, const double *offset,
                                            AnofoxHipWindowFrame frame, AnofoxHipGlmBatchOptions options, double interval_z, double *pred,
                                            double *glm_records, AnofoxError *out_error) {
	reset_error(out_error);
	if (n_groups < 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (!glm_check_interval(options, interval_z, out_error)) return false;
	if (!check_window_args(n_rows, n_features, y, x_cols, pred, out_error)) return false;
	if (!check_window_frame(frame, out_error)) return false;
	if (n_groups > 0 && !row_offsets) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "row_offsets is NULL"); return false; }
	if (n_groups > 0 && !check_window_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0 || n_rows == 0) return true;
	std::vector<int64_t> lo((size_t)n_rows), hi((size_t)n_rows);
	rows_frames(n_groups, row_offsets, frame, lo.data(), hi.data());
	return glm_window_host(ctx, n_groups, row_offsets, n_features, n_rows, y, x_cols, offset, lo.data(), hi.data(), options, interval_z, pred,
	                       glm_records, out_error);
}

bool anofox_hip_glm_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                            const double *const *x_cols, const double *offset, const int64_t *frame_lo,
                                            const int64_t *frame_hi, AnofoxHipGlmBatchOptions options, double interval_z, double *pred,
                                            double *glm_records, AnofoxError *out_error) {
	reset_error(out_error);
	if (!glm_check_interval(options, interval_z, out_error)) return false;
	if (!check_window_args(n_rows, n_features, y, x_cols, pred, out_error)) return false;
	if (n_rows > 0 && (!frame_lo || !frame_hi)) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "frame_lo or frame_hi is NULL"); return false; }
	if (!check_host_frames(n_rows, frame_lo, frame_hi, out_error)) return false;
	if (n_rows == 0) return true;
	const int64_t off[2] = {0, n_rows};
	return glm_window_host(ctx, 1, off, n_features, n_rows, y, x_cols, offset, frame_lo, frame_hi, options, interval_z, pred, glm_records,
	                       out_error);
}

// The planner alone, on host arrays, under the test hooks in force: run_begin (capacity entries, may be NULL with capacity 0)
// receives the first output row of every walker and one entry past them, *n_runs their number, *span_rows the scratch rows of
// one wavefront (the longest frame), *n_waves the wavefronts a launch would use.
bool anofox_hip_glm_window_plan(int64_t n_groups, const int64_t *row_offsets, int64_t n_rows, const int64_t *frame_lo,
                                const int64_t *frame_hi, int64_t *run_begin, int64_t capacity, int64_t *n_runs, int64_t *span_rows,
                                int64_t *n_waves, AnofoxError *out_error) {
	reset_error(out_error);
	if (n_groups < 0 || n_rows < 0 || !n_runs || !span_rows || !n_waves || (n_groups > 0 && !row_offsets) || (n_rows > 0 && (!frame_lo || !frame_hi))) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glm window plan: a NULL or negative argument");
		return false;
	}
	if (n_groups > 0 && !check_window_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (!check_host_frames(n_rows, frame_lo, frame_hi, out_error)) return false;
	int64_t run_length, cap;
	int warm;
	window_hooks(&run_length, &cap, &warm);
	GlmWindowPlan plan;
	if (!plan_glm_window(n_groups, row_offsets, frame_lo, frame_hi, run_length, cap, plan, out_error)) return false;
	*n_runs = (int64_t)plan.run_begin.size() - 1;
	*span_rows = plan.span;
	*n_waves = plan.waves;
	if (run_begin) {
		if (capacity < (int64_t)plan.run_begin.size()) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glm window plan: run_begin is too short"); return false; }
		memcpy(run_begin, plan.run_begin.data(), plan.run_begin.size() * sizeof(int64_t));
	}
	return true;
}

// A test's hook: the run length, the scratch cap (0: the library's rule) and whether frames may start warm (1, the default; 0:
// every frame starts cold) of every later GLM window call of the process.
void anofox_hip_glm_window_test_hooks(int64_t run_length, int64_t scratch_cap_bytes, int warm) {
	std::lock_guard<std::mutex> lk(g_gw_mu);
	g_gw_run_length = run_length > 0 ? run_length : 0;
	g_gw_scratch_cap = scratch_cap_bytes > 0 ? scratch_cap_bytes : 0;
	g_gw_warm = warm ? 1 : 0;
}

// What the most recent GLM window call on `ctx` (NULL: the thread's default context) did: out[8] = {output rows, frames started
// cold, frames started warm, warm frames refitted cold, IRLS iterations summed over the frames, walkers, launched wavefronts,
// scratch rows per wavefront}.  Waits for the context's stream.  The record lives in the context and is reset by every GLM
// window call on it; without one (or after one that launched nothing) the call fails.
bool anofox_hip_glm_window_stats(AnofoxHipContext *ctx, int64_t *out, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out is NULL"); return false; }
	if (!(ctx = host_context(ctx, out_error))) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (!ctx->gw_valid) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glm window stats: no window call on this context"); return false; }
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const int64_t walkers = ctx->gw_walkers;
	std::vector<int64_t> counts(4 * (size_t)walkers);
	if (!d2h(counts.data(), ctx->gw_counts, counts.size() * sizeof(int64_t), ctx->stream, out_error)) return false;
	if (hip_fail(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize", out_error)) return false;
	int64_t sum[4] = {0, 0, 0, 0};
	for (int64_t w = 0; w < walkers; ++w)
		for (int j = 0; j < 4; ++j) sum[j] += counts[4 * (size_t)w + j];
	out[0] = ctx->gw_frames;
	out[1] = sum[0];
	out[2] = sum[1];
	out[3] = sum[2];
	out[4] = sum[3];
	out[5] = walkers;
	out[6] = ctx->gw_waves;
	out[7] = ctx->gw_span;
	return true;
}

} // extern "C"
