// rls.hip — grouped recursive least squares: the batch fit, the fit-predict batch, the window functions over ROWS and explicit
// frames, and the reference-compatible anofox_rls_fit.
//
// Reference: fit_rls / RlsState::update (crates/anofox-stats-core/src/models/rls.rs) — a sequential filter per group whose
// in-place P update is not textbook RLS, so no moment path applies: every group (and every window frame) runs the filter
// of rls_filter.h over its own rows, in the reference's operation order (DESIGN.md §1 "Recursive least squares").
//   lane kernels (p <= 8): one lane per group / frame, P in registers;
//   wave kernels (9 <= p <= 128, and groups longer than kRlsLongRows at p <= 8): one wavefront per group / frame, P in LDS;
//   the expanding window at p <= 8: one lane per partition, one pass (rls_expanding_range).
// No atomics: every group or frame is one lane's or one wavefront's own work, so repeated calls give identical bytes.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "rls_filter.h"

using namespace anofox;

#include "host_stage.h"
#include "scalar_fit.h"

using namespace anofox::host;
using namespace anofox::rls;

namespace {

// Groups of more rows than this run on a wavefront even at p <= 8, so that one long group does not hold a single lane
// while the rest of the batch has finished (ANOFOX_RLS_LONG_ROWS overrides it for measurements).
constexpr int64_t kRlsLongRows = 1 << 16;
// workgroups of the wave kernel when it only serves the long groups of a p <= 8 batch
constexpr int64_t kRlsWaveBlocks = 1024;

int64_t rls_long_rows() {
	static const int64_t v = env_int("ANOFOX_RLS_LONG_ROWS", kRlsLongRows);
	return v;
}

// ANOFOX_RLS_EXPANDING=0 sends the expanding window at p <= 8 through the frames path as well (A/B switch for measurements)
bool rls_expanding_on() {
	static const bool on = env_on("ANOFOX_RLS_EXPANDING");
	return on;
}

struct RlsArgs {
	const int64_t *row_offsets;  // [G + 1]
	const int64_t *train_counts; // [G] or nullptr: what the "fewer than 2 rows -> NULL" rule looks at
	const double *y;
	const double *x[kWideMaxP];
	int64_t n_groups;
	int p;
	int wave_all;      // the wave kernel fits every group (p > 8)
	int64_t long_rows; // else: the groups of more rows than this
	RlsParams o;
	double *core; // [G x (p + 6)]
};

struct RlsFramesArgs {
	const int64_t *lo, *hi; // frame of output row e: rows [lo[e], hi[e])
	const double *y;
	const double *x[kWideMaxP];
	int64_t n_frames;
	int p;
	RlsParams o;
	double *pred; // [n_frames x 3]
};

__device__ inline int64_t rls_rule_count(const RlsArgs &a, int64_t g, int64_t lo, int64_t hi) {
	return a.train_counts ? a.train_counts[g] : hi - lo;
}

template <int P>
__global__ __launch_bounds__(64) void rls_batch_lane_kernel(RlsArgs a) {
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.n_groups) return;
	const int64_t lo = a.row_offsets[g], hi = a.row_offsets[g + 1];
	double *rec = a.core + g * (P + 6);
	if (rls_rule_count(a, g, lo, hi) < 2) { rls_fail_record(rec, P, kStatusTooFewRows); return; }
	if (hi - lo > a.long_rows) return; // rls_batch_wave_kernel
	rls_fit_range<P>(a.y, a.x, P, lo, hi, a.o, rec);
}

// Groups g = blockIdx.x, blockIdx.x + gridDim.x, ...: with wave_all the grid covers every group once; at p <= 8 a grid of at
// most kRlsWaveBlocks workgroups walks the offsets and fits only the long groups.
__global__ __launch_bounds__(64) void rls_batch_wave_kernel(RlsArgs a) {
	extern __shared__ double rls_lds[];
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		const int64_t lo = a.row_offsets[g], hi = a.row_offsets[g + 1];
		double *rec = a.core + g * (a.p + 6);
		if (rls_rule_count(a, g, lo, hi) < 2) {
			if (a.wave_all && threadIdx.x == 0) rls_fail_record(rec, a.p, kStatusTooFewRows);
			continue;
		}
		if (!a.wave_all && hi - lo <= a.long_rows) continue; // a lane kernel's group
		rls_fit_range_wave(a.y, a.x, a.p, lo, hi, a.o, rec, rls_lds);
		__syncthreads(); // lane 0 has read the LDS record state before the next group overwrites it
	}
}

// The expanding window (frame {UNBOUNDED PRECEDING, CURRENT ROW}), p <= 8: one lane per partition, one pass over its rows
template <int P>
__global__ __launch_bounds__(64) void rls_expanding_lane_kernel(const int64_t *row_offsets, int64_t n_groups, RlsFramesArgs a) {
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= n_groups) return;
	rls_expanding_range<P>(a.y, a.x, P, row_offsets[g], row_offsets[g + 1], a.o, a.pred);
}

// yhat of every row of every group from its record (anofox_predict_with_interval with sigma = NaN: yhat = lower = upper)
__global__ __launch_bounds__(256) void rls_predict_kernel(const int64_t *row_offsets, int64_t n_groups, RlsArgs a, double *pred) {
	const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (g >= n_groups) return;
	const int p = a.p;
	const double *rec = a.core + g * (p + 6);
	const bool ok = rec[p + 5] == 0.0;
	for (int64_t r = row_offsets[g] + (threadIdx.x & 63); r < row_offsets[g + 1]; r += 64) {
		const double yh = ok ? rls_predict_row(rec, p, a.x, r) : NAN;
		pred[3 * r] = yh;
		pred[3 * r + 1] = yh;
		pred[3 * r + 2] = yh;
	}
}

// The window NULL rule (rls_fit_predict.cpp:228): a frame is NULL unless it holds MORE than p + [intercept] rows with non-NULL y.
__device__ inline bool rls_frame_trains(const double *y, int64_t lo, int64_t hi, int64_t need) {
	int64_t n = 0;
	for (int64_t r = lo; r < hi && n <= need; ++r) n += y[r] == y[r];
	return n > need;
}

__device__ inline void rls_store_pred(double *pred, int64_t e, double v) {
	pred[3 * e] = v;
	pred[3 * e + 1] = v;
	pred[3 * e + 2] = v;
}

template <int P>
__global__ __launch_bounds__(64) void rls_frames_lane_kernel(RlsFramesArgs a) {
	const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= a.n_frames) return;
	const int64_t lo = a.lo[e], hi = a.hi[e];
	if (hi <= lo || !rls_frame_trains(a.y, lo, hi, P + (a.o.fit_intercept ? 1 : 0))) { rls_store_pred(a.pred, e, NAN); return; }
	double rec[P + 6];
	rls_fit_range<P>(a.y, a.x, P, lo, hi, a.o, rec);
	rls_store_pred(a.pred, e, rec[P + 5] == 0.0 ? rls_predict_row(rec, P, a.x, hi - 1) : NAN);
}

__global__ __launch_bounds__(64) void rls_frames_wave_kernel(RlsFramesArgs a) {
	extern __shared__ double rls_lds[];
	const int64_t e = blockIdx.x;
	const int64_t lo = a.lo[e], hi = a.hi[e];
	const int p = a.p;
	if (hi <= lo || !rls_frame_trains(a.y, lo, hi, p + (a.o.fit_intercept ? 1 : 0))) {
		if (threadIdx.x == 0) rls_store_pred(a.pred, e, NAN);
		return;
	}
	const int d = p + 1, ld = d | 1;
	double *rec = rls_lds + (size_t)d * ld + 4 * (size_t)d; // the record slot of rls_wave_lds_bytes
	rls_fit_range_wave(a.y, a.x, p, lo, hi, a.o, rec, rls_lds);
	__syncthreads();
	if (threadIdx.x == 0) rls_store_pred(a.pred, e, rec[p + 5] == 0.0 ? rls_predict_row(rec, p, a.x, hi - 1) : NAN);
}

// ---- launches ----

template <class K>
void rls_allow_lds(K kernel) {
	(void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

RlsParams rls_params(const AnofoxHipRlsBatchOptions &o) {
	RlsParams r;
	r.lambda = o.forgetting_factor;
	r.delta = o.initial_p_diagonal;
	r.fit_intercept = o.fit_intercept ? 1 : 0;
	return r;
}

bool launch_rls_batch(AnofoxHipContext *ctx, int64_t G, size_t p, const int64_t *d_off, const double *d_y, const double *const *x_cols,
                      const int64_t *d_tc, const AnofoxHipRlsBatchOptions &o, double *d_core, AnofoxError *e, int64_t max_rows = -1) {
	if (G == 0) return true;
	RlsArgs a;
	memset(&a, 0, sizeof a);
	a.row_offsets = d_off;
	a.train_counts = d_tc;
	a.y = d_y;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.n_groups = G;
	a.p = (int)p;
	a.wave_all = p > (size_t)kNarrowMaxP;
	a.long_rows = rls_long_rows();
	a.o = rls_params(o);
	a.core = d_core;
	hipStream_t st = ctx->stream;
	if (!a.wave_all) {
		const dim3 grid((unsigned)((G + 63) / 64));
		dispatch_narrow((int)p, 0, [&](auto P) { hipLaunchKernelGGL(rls_batch_lane_kernel<P()>, grid, dim3(64), 0, st, a); return 0; });
		if (hip_fail(hipGetLastError(), "rls_batch_lane_kernel", e)) return false;
	}
	if (!a.wave_all && max_rows >= 0 && max_rows <= a.long_rows) return true; // the host knows there is no long group
	static std::once_flag once;
	std::call_once(once, [] { rls_allow_lds(rls_batch_wave_kernel); rls_allow_lds(rls_frames_wave_kernel); });
	const int64_t blocks = a.wave_all ? G : (G < kRlsWaveBlocks ? G : kRlsWaveBlocks);
	hipLaunchKernelGGL(rls_batch_wave_kernel, dim3((unsigned)blocks), dim3(64), rls_wave_lds_bytes((int)p), st, a);
	return !hip_fail(hipGetLastError(), "rls_batch_wave_kernel", e);
}

bool launch_rls_predict(AnofoxHipContext *ctx, int64_t G, size_t p, const int64_t *d_off, const double *const *x_cols,
                        const double *d_core, double *d_pred, AnofoxError *e) {
	if (G == 0) return true;
	RlsArgs a;
	memset(&a, 0, sizeof a);
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.p = (int)p;
	a.core = const_cast<double *>(d_core);
	hipLaunchKernelGGL(rls_predict_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, ctx->stream, d_off, G, a, d_pred);
	return !hip_fail(hipGetLastError(), "rls_predict_kernel", e);
}

bool launch_rls_frames(AnofoxHipContext *ctx, int64_t n_frames, size_t p, const double *d_y, const double *const *x_cols,
                       const int64_t *d_lo, const int64_t *d_hi, const AnofoxHipRlsBatchOptions &o, double *d_pred, AnofoxError *e) {
	if (n_frames == 0) return true;
	RlsFramesArgs a;
	memset(&a, 0, sizeof a);
	a.lo = d_lo;
	a.hi = d_hi;
	a.y = d_y;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	a.n_frames = n_frames;
	a.p = (int)p;
	a.o = rls_params(o);
	a.pred = d_pred;
	hipStream_t st = ctx->stream;
	if (p <= (size_t)kNarrowMaxP) {
		const dim3 grid((unsigned)((n_frames + 63) / 64));
		dispatch_narrow((int)p, 0, [&](auto P) { hipLaunchKernelGGL(rls_frames_lane_kernel<P()>, grid, dim3(64), 0, st, a); return 0; });
		return !hip_fail(hipGetLastError(), "rls_frames_lane_kernel", e);
	}
	static std::once_flag once;
	std::call_once(once, [] { rls_allow_lds(rls_batch_wave_kernel); rls_allow_lds(rls_frames_wave_kernel); });
	hipLaunchKernelGGL(rls_frames_wave_kernel, dim3((unsigned)n_frames), dim3(64), rls_wave_lds_bytes((int)p), st, a);
	return !hip_fail(hipGetLastError(), "rls_frames_wave_kernel", e);
}

// ---- argument checks: before any device use (and before the host forms pick the thread's default context) ----

bool check_common(int64_t G, size_t p, int64_t n_rows, const void *off, const void *y, const double *const *x_cols, const void *out,
                  AnofoxError *e) {
	return check_batch_args(G, p, n_rows, off, y, x_cols, out, kWideMaxP, nullptr, "row_offsets, y or an output is NULL", false, e);
}

bool check_frame(const AnofoxHipWindowFrame &f, AnofoxError *e) {
	if (f.start_preceding < f.end_preceding || f.start_preceding == -ANOFOX_HIP_FRAME_UNBOUNDED || f.end_preceding == ANOFOX_HIP_FRAME_UNBOUNDED) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "window frame must start at or before its end");
		return false;
	}
	return true;
}

bool check_host_frames(int64_t n_rows, const int64_t *lo, const int64_t *hi, AnofoxError *e) {
	for (int64_t r = 0; r < n_rows; ++r) {
		if (hi[r] > lo[r] && (lo[r] < 0 || hi[r] > n_rows)) {
			set_error(e, ANOFOX_ERROR_INVALID_INPUT, "frame bounds must lie within [0, n_rows]");
			return false;
		}
	}
	return true;
}

int64_t max_group_rows(int64_t G, const int64_t *off) {
	int64_t m = 0;
	for (int64_t g = 0; g < G; ++g) m = off[g + 1] - off[g] > m ? off[g + 1] - off[g] : m;
	return m;
}

bool window_frames_device(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const int64_t *d_off, const double *d_y,
                          const double *const *x_cols, const AnofoxHipWindowFrame &frame, const AnofoxHipRlsBatchOptions &o,
                          double *d_pred, AnofoxError *e) {
	if (G == 0 || n_rows == 0) return true;
	if (p <= (size_t)kNarrowMaxP && frame.start_preceding == ANOFOX_HIP_FRAME_UNBOUNDED && frame.end_preceding == 0 && rls_expanding_on()) {
		RlsFramesArgs a;
		memset(&a, 0, sizeof a);
		a.y = d_y;
		for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
		a.p = (int)p;
		a.o = rls_params(o);
		a.pred = d_pred;
		const dim3 grid((unsigned)((G + 63) / 64));
		dispatch_narrow((int)p, 0, [&](auto P) { hipLaunchKernelGGL(rls_expanding_lane_kernel<P()>, grid, dim3(64), 0, ctx->stream, d_off, G, a); return 0; });
		return !hip_fail(hipGetLastError(), "rls_expanding_lane_kernel", e);
	}
	const size_t b = Stage::bytes((size_t)n_rows, sizeof(int64_t));
	if (!ensure_buffer(&ctx->frames_buf, &ctx->frames_bytes, 2 * b, "window frames", e)) return false;
	int64_t *lo = (int64_t *)ctx->frames_buf, *hi = (int64_t *)((char *)ctx->frames_buf + b);
	if (hip_fail(launch_frames_from_rows_spec(d_off, G, n_rows, frame.start_preceding, frame.end_preceding, lo, hi, ctx->stream),
	             "frames_spec_kernel", e))
		return false;
	return launch_rls_frames(ctx, n_rows, p, d_y, x_cols, lo, hi, o, d_pred, e);
}

} // namespace

extern "C" {

bool anofox_hip_rls_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows, const int64_t *d_row_offsets,
                                     const double *d_y, const double *const *x_cols, AnofoxHipRlsBatchOptions options, double *d_core,
                                     AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_core, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_rls_batch(ctx, n_groups, n_features, d_row_offsets, d_y, x_cols, nullptr, options, d_core, out_error);
}

bool anofox_hip_rls_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows, const int64_t *row_offsets,
                                   const double *y, const double *const *x_cols, AnofoxHipRlsBatchOptions options, double *core,
                                   AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_groups, n_features, n_rows, row_offsets, y, x_cols, core, out_error)) return false;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!(ctx = host_context(ctx, out_error))) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features;
	return fit_slabs_host(ctx, n_groups, p, row_offsets, y, x_cols, nullptr, SlabOutputs{core, p + 6}, kPlainSlab, out_error,
	                      [&](int64_t G, int64_t, const int64_t *off, const int64_t *d_off, const StagedColumns &c, double *d_core, int32_t *, double *) {
		                      return launch_rls_batch(ctx, G, p, d_off, c.y, c.x, nullptr, options, d_core, out_error, max_group_rows(G, off));
	                      });
}

bool anofox_hip_rls_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                             const int64_t *d_train_counts, AnofoxHipRlsBatchOptions options, double confidence_level,
                                             double *d_core, double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_core, out_error)) return false;
	if (n_groups > 0 && !d_pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	(void)confidence_level; // sigma is NaN: the interval is the point (anofox_predict_with_interval)
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_rls_batch(ctx, n_groups, n_features, d_row_offsets, d_y, x_cols, d_train_counts, options, d_core, out_error) &&
	       launch_rls_predict(ctx, n_groups, n_features, d_row_offsets, x_cols, d_core, d_pred, out_error);
}

bool anofox_hip_rls_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                           const int64_t *train_counts, AnofoxHipRlsBatchOptions options, double confidence_level,
                                           double *core, double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_groups, n_features, n_rows, row_offsets, y, x_cols, core, out_error)) return false;
	if (n_groups > 0 && !pred) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0) return true;
	if (!(ctx = host_context(ctx, out_error))) return false;
	(void)confidence_level;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features, core_len = p + 6, G = (size_t)n_groups, N = (size_t)n_rows;
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
	if (!launch_rls_batch(ctx, n_groups, p, d_off, c.y, c.x, d_tc, options, d_core, out_error, max_group_rows(n_groups, row_offsets))) return false;
	if (!launch_rls_predict(ctx, n_groups, p, d_off, c.x, d_core, d_pred, out_error)) return false;
	if (!d2h(core, d_core, G * core_len * sizeof(double), st, out_error)) return false;
	if (!d2h(pred, d_pred, 3 * N * sizeof(double), st, out_error)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error);
}

bool anofox_hip_rls_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                              const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                              AnofoxHipWindowFrame frame, AnofoxHipRlsBatchOptions options, double confidence_level,
                                              double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_pred, out_error)) return false;
	if (!check_frame(frame, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	(void)confidence_level;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return window_frames_device(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, frame, options, d_pred, out_error);
}

bool anofox_hip_rls_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                            const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                            AnofoxHipWindowFrame frame, AnofoxHipRlsBatchOptions options, double confidence_level,
                                            double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_groups, n_features, n_rows, row_offsets, y, x_cols, pred, out_error)) return false;
	if (!check_frame(frame, out_error)) return false;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	if (n_groups == 0 || n_rows == 0) return true;
	if (!(ctx = host_context(ctx, out_error))) return false;
	(void)confidence_level;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features, G = (size_t)n_groups, N = (size_t)n_rows;
	hipStream_t st = ctx->stream;
	int64_t *d_off;
	StagedColumns c;
	double *d_pred;
	if (!stage_call(ctx, out_error, [&](Stage &s) {
		    d_off = s.put(row_offsets, G + 1);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, nullptr, kPlainColumns);
		    d_pred = s.take<double>(3 * N);
	    }))
		return false;
	if (!window_frames_device(ctx, n_groups, p, n_rows, d_off, c.y, c.x, frame, options, d_pred, out_error)) return false;
	if (!d2h(pred, d_pred, 3 * N * sizeof(double), st, out_error)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error);
}

bool anofox_hip_rls_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *d_y,
                                              const double *const *x_cols, const int64_t *d_frame_lo, const int64_t *d_frame_hi,
                                              AnofoxHipRlsBatchOptions options, double confidence_level, double *d_pred,
                                              AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_rows, n_features, n_rows, d_frame_lo, d_y, x_cols, d_pred, out_error)) return false;
	if (n_rows > 0 && !d_frame_hi) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "frame_hi is NULL"); return false; }
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	(void)confidence_level;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_rls_frames(ctx, n_rows, n_features, d_y, x_cols, d_frame_lo, d_frame_hi, options, d_pred, out_error);
}

bool anofox_hip_rls_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t n_features, const double *y,
                                            const double *const *x_cols, const int64_t *frame_lo, const int64_t *frame_hi,
                                            AnofoxHipRlsBatchOptions options, double confidence_level, double *pred,
                                            AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_common(n_rows, n_features, n_rows, frame_lo, y, x_cols, pred, out_error)) return false;
	if (n_rows > 0 && !frame_hi) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "frame_hi is NULL"); return false; }
	if (!check_host_frames(n_rows, frame_lo, frame_hi, out_error)) return false;
	if (n_rows == 0) return true;
	if (!(ctx = host_context(ctx, out_error))) return false;
	(void)confidence_level;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features, N = (size_t)n_rows;
	hipStream_t st = ctx->stream;
	int64_t *d_lo, *d_hi;
	StagedColumns c;
	double *d_pred;
	if (!stage_call(ctx, out_error, [&](Stage &s) {
		    d_lo = s.put(frame_lo, N);
		    d_hi = s.put(frame_hi, N);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, nullptr, kPlainColumns);
		    d_pred = s.take<double>(3 * N);
	    }))
		return false;
	if (!launch_rls_frames(ctx, n_rows, p, c.y, c.x, d_lo, d_hi, options, d_pred, out_error)) return false;
	if (!d2h(pred, d_pred, 3 * N * sizeof(double), st, out_error)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", out_error);
}

// One group through anofox_hip_rls_fit_batch_host with anofox_elasticnet_fit's conventions (elasticnet.hip): argument checks
// first, NULL entries -> NaN through the validity bitmask, a one-row input padded with an all-NaN row (the batch applies the
// aggregate's "< 2 rows" rule), the reference's error texts (crates/anofox-stats-core/src/errors.rs), coefficients malloc'ed.
bool anofox_rls_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxRlsOptions options, AnofoxFitResultCore *out_core,
                    AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_core) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_core is NULL"); return false; }
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (x[0].len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: x[0] cannot be empty"); return false; }
	if (y.len != x[0].len) {
		set_dimension_mismatch(y.len, x[0].len, out_error);
		return false;
	}
	const size_t p = x_count;
	if (!check_column_lengths(y.len, x + 1, p - 1, out_error)) return false;
	if (p > (size_t)kWideMaxP) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT,
		          "RLS fit: more than " + std::to_string(kWideMaxP) + " features are not supported by the GPU path");
		return false;
	}
	const ScalarFitInput in(y, x, x_count);
	AnofoxHipRlsBatchOptions o;
	memset(&o, 0, sizeof o);
	o.forgetting_factor = options.forgetting_factor;
	o.fit_intercept = options.fit_intercept;
	o.initial_p_diagonal = options.initial_p_diagonal;
	std::vector<double> core(p + 6);
	if (!anofox_hip_rls_fit_batch_host(nullptr, 1, p, (int64_t)in.n_pad, in.off, in.yv.data(), in.xp.data(), o, core.data(), out_error)) return false;
	const int status = (int)core[p + 5];
	if (status != ANOFOX_ERROR_SUCCESS) { // rls.rs:56-69
		std::string other = "RLS fit failed on the GPU path";
		if (status == ANOFOX_ERROR_INVALID_INPUT)
			other = !(options.forgetting_factor <= 0.0 || options.forgetting_factor > 1.0)
			            ? "Invalid input: initial_p_diagonal must be > 0 (got " + fmt_g(options.initial_p_diagonal) + ")"
			            : "Invalid input: forgetting_factor must be in (0, 1] (got " + fmt_g(options.forgetting_factor) + ")";
		set_scalar_fit_error(status, (AnofoxErrorCode)status, in, other, out_error);
		return false;
	}
	return fill_scalar_result(core.data(), p, out_core, out_error);
}

} // extern "C"
