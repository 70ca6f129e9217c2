// eb_shrink.hip — empirical-Bayes shrinkage of per-group estimates toward their precision-weighted mean (eb_shrink.h): the kernels
// of both paths and the entry points anofox_hip_eb_shrink_batch_{device,host}, anofox_hip_eb_shrink_test_hooks,
// anofox_eb_shrink / anofox_free_eb_shrink_result.
//
// The contract and the method: eb_shrink.h and DESIGN.md §1, "Empirical-Bayes shrinkage".
//   eb_set_kernel: one wavefront per (set, column block of 64), four wavefronts per workgroup, grid-stride over the units.  No
//     LDS and no scratch: the sums of a set live in the wavefront's registers between its four passes.
//   eb_part_kernel<PASS> / eb_comb_kernel<PASS> / eb_write_kernel: the chunk path for few large sets, seven launches on the
//     context's stream: partials of a pass per chunk into the context's workspace, one wavefront per set adds them in a fixed
//     order, the next pass reads what it left in the state.  Chunk numbers need no prefix sum over the sets (eb_chunk_base), so
//     neither form of the entry reads the offsets on the host to size a launch.
//   The path: chunks when n_sets x column blocks <= kEbChunkMaxUnits and the average set holds kEbCrossoverPairs (item, padded
//     column) pairs or more (docs/MEASUREMENTS.md, "eb_shrink").  It depends on n_sets, n_items and n_cols only, so the device and
//     the host form of a call take the same path and give the same bytes.
// No atomics on either path: repeated calls give identical bytes.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "eb_shrink.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::eb;

namespace {

constexpr int64_t kEbCrossoverPairs = 4096; // average (items x padded columns) of a set from which the chunk path is taken
constexpr int64_t kEbChunkMaxUnits = 1024;  // ... when there are no more (set, column block) units than this
constexpr int64_t kEbChunkPairs = 1024;     // a chunk: this many (item, padded column) pairs, 64 items at least
constexpr int64_t kEbMaxWorkgroups = 1 << 16;
constexpr int kWaves = 4; // wavefronts per workgroup

std::atomic<int> g_force_path{0}; // anofox_hip_eb_shrink_test_hooks
std::atomic<int64_t> g_chunk_items{0}, g_max_workgroups{0};

struct EbArgs {
	EbProblem P;
	const int64_t *off; // [n_sets + 1]
	int64_t n_sets;
	int64_t chunk;     // items per chunk
	int64_t n_numbers; // chunk numbers: n_items / chunk + n_sets
	int col_blocks;
	double *state; // [n_sets x n_cols x kEbStateLen]
	double *parts; // [n_numbers x n_cols x kEbPartLen]
};

__device__ __forceinline__ int64_t first_unit() { return (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); }
__device__ __forceinline__ int64_t unit_step() { return (int64_t)gridDim.x * kWaves; }

__global__ __launch_bounds__(64 * kWaves) void eb_set_kernel(EbArgs a) {
	const int64_t units = a.n_sets * a.col_blocks;
	for (int64_t u = first_unit(); u < units; u += unit_step()) {
		const int64_t set = u / a.col_blocks;
		eb_shrink_set(a.P, set, a.off[set], a.off[set + 1], (int)(u % a.col_blocks) * 64);
	}
}

template <int PASS>
__global__ __launch_bounds__(64 * kWaves) void eb_part_kernel(EbArgs a) {
	const int64_t units = a.n_numbers * a.col_blocks;
	for (int64_t u = first_unit(); u < units; u += unit_step())
		eb_chunk_partial<PASS>(a.P, a.off, a.n_sets, a.chunk, u / a.col_blocks, (int)(u % a.col_blocks) * 64, a.state, a.parts);
}

template <int PASS>
__global__ __launch_bounds__(64 * kWaves) void eb_comb_kernel(EbArgs a) {
	const int64_t units = a.n_sets * a.col_blocks;
	for (int64_t u = first_unit(); u < units; u += unit_step())
		eb_chunk_combine<PASS>(a.P, a.off, a.n_numbers, a.chunk, u / a.col_blocks, (int)(u % a.col_blocks) * 64, a.state, a.parts);
}

__global__ __launch_bounds__(64 * kWaves) void eb_write_kernel(EbArgs a) {
	const int64_t units = a.n_numbers * a.col_blocks;
	for (int64_t u = first_unit(); u < units; u += unit_step())
		eb_chunk_write(a.P, a.off, a.n_sets, a.chunk, u / a.col_blocks, (int)(u % a.col_blocks) * 64, a.state);
}

// the extent of a strided matrix: the doubles from its first to its last element
size_t extent(int64_t n_items, int64_t stride, size_t n_cols) { return n_items > 0 ? (size_t)(n_items - 1) * (size_t)stride + n_cols : 0; }

bool check_eb(int64_t n_sets, int64_t n_items, const void *off, size_t n_cols, const void *est, int64_t est_stride, const void *se,
              int64_t se_stride, const void *out, const void *summary, AnofoxError *e) {
	if (n_sets < 0 || n_items < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "negative n_sets or n_items"); return false; }
	if (n_cols == 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "eb_shrink: n_cols is 0"); return false; }
	if (n_cols > 0x7fffffffu) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "eb_shrink: n_cols is too large"); return false; }
	if (est_stride < (int64_t)n_cols || se_stride < (int64_t)n_cols) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "eb_shrink: a stride is smaller than n_cols");
		return false;
	}
	if (n_sets > 0 && (!off || !summary)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "set_offsets or summary is NULL"); return false; }
	if (n_sets > 0 && n_items > 0 && (!est || !se || !out)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "estimate, se or out is NULL"); return false; }
	return true;
}

template <class K>
bool launch(K kernel, const char *name, const EbArgs &a, int64_t units, hipStream_t st, AnofoxError *e) {
	const int64_t hook = g_max_workgroups.load(), cap = hook > 0 ? hook : kEbMaxWorkgroups;
	int64_t blocks = (units + kWaves - 1) / kWaves;
	blocks = blocks < 1 ? 1 : (blocks > cap ? cap : blocks);
	hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64 * kWaves), 0, st, a);
	return !hip_fail(hipGetLastError(), name, e);
}

// the shrinkage of n_sets x n_cols sets on device-resident inputs, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_eb(AnofoxHipContext *ctx, int64_t n_sets, int64_t n_items, const int64_t *d_off, size_t n_cols, const double *d_est,
               int64_t est_stride, const double *d_se, int64_t se_stride, const AnofoxHipEbShrinkOptions &o, double *d_out, double *d_summary,
               AnofoxError *e) {
	if (n_sets == 0) return true;
	EbArgs a;
	memset(&a, 0, sizeof a);
	a.P.est = d_est;
	a.P.se = d_se;
	a.P.est_stride = est_stride;
	a.P.se_stride = se_stride;
	a.P.n_items = n_items;
	a.P.n_cols = (int)n_cols;
	a.P.invalid = eb_options_invalid((int)o.method, o.tau_squared) ? 1 : 0;
	a.P.method = a.P.invalid ? kEbMethodDL : (int)o.method;
	a.P.tau_fixed = a.P.invalid ? NAN : o.tau_squared;
	a.P.out = d_out;
	a.P.summary = d_summary;
	a.off = d_off;
	a.n_sets = n_sets;
	a.col_blocks = eb_col_blocks((int)n_cols);
	const int64_t cp = eb_col_pad((int)n_cols), units = n_sets * a.col_blocks;
	const int force = g_force_path.load();
	const bool chunks = force ? force == 2 : (units <= kEbChunkMaxUnits && n_items / n_sets * cp >= kEbCrossoverPairs);
	hipStream_t st = ctx->stream;
	if (!chunks) return launch(eb_set_kernel, "eb_set_kernel", a, units, st, e);
	const int64_t hook = g_chunk_items.load(), by_pairs = kEbChunkPairs / cp;
	a.chunk = hook > 0 ? hook : (by_pairs < 64 ? 64 : by_pairs);
	a.n_numbers = n_items / a.chunk + n_sets;
	const size_t state = align_up((size_t)n_sets * n_cols * kEbStateLen * sizeof(double), 256);
	const size_t parts = (size_t)a.n_numbers * n_cols * kEbPartLen * sizeof(double);
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, state + parts, "eb_shrink scratch", e)) return false;
	a.state = (double *)ctx->ws;
	a.parts = (double *)((char *)ctx->ws + state);
	const int64_t chunk_units = a.n_numbers * a.col_blocks;
	return launch(eb_part_kernel<1>, "eb_part_kernel<1>", a, chunk_units, st, e) && launch(eb_comb_kernel<1>, "eb_comb_kernel<1>", a, units, st, e) &&
	       launch(eb_part_kernel<2>, "eb_part_kernel<2>", a, chunk_units, st, e) && launch(eb_comb_kernel<2>, "eb_comb_kernel<2>", a, units, st, e) &&
	       launch(eb_part_kernel<3>, "eb_part_kernel<3>", a, chunk_units, st, e) && launch(eb_comb_kernel<3>, "eb_comb_kernel<3>", a, units, st, e) &&
	       launch(eb_write_kernel, "eb_write_kernel", a, chunk_units, st, e);
}

// host pointers: one staging of the whole call, the kernels, the copies back
bool eb_host(AnofoxHipContext *ctx, int64_t n_sets, int64_t n_items, const int64_t *set_offsets, size_t n_cols, const double *est,
             int64_t est_stride, const double *se, int64_t se_stride, const AnofoxHipEbShrinkOptions &o, double *out, double *summary,
             AnofoxError *e) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t S = (size_t)n_sets, n_out = (size_t)n_items * n_cols * kEbOutLen, n_sum = S * n_cols * kEbSummaryLen;
	std::lock_guard<std::mutex> lk(ctx->mu); // one lock over staging, the kernels and the copies back
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off;
	double *d_est, *d_se, *d_out, *d_sum;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(set_offsets, S + 1);
		    d_est = n_items > 0 ? s.put(est, extent(n_items, est_stride, n_cols)) : nullptr;
		    d_se = n_items > 0 ? s.put(se, extent(n_items, se_stride, n_cols)) : nullptr;
		    d_out = s.take<double>(n_out);
		    d_sum = s.take<double>(n_sum);
	    }))
		return false;
	if (!launch_eb(ctx, n_sets, n_items, d_off, n_cols, d_est, est_stride, d_se, se_stride, o, d_out, d_sum, e)) return false;
	// items outside every set are not written by the kernels and keep the caller's values
	const size_t o0 = (size_t)set_offsets[0] * n_cols * kEbOutLen, o1 = (size_t)set_offsets[S] * n_cols * kEbOutLen;
	if (!d2h(out + o0, d_out + o0, (o1 - o0) * sizeof(double), st, e)) return false;
	if (!d2h(summary, d_sum, n_sum * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

void reset_eb_result(AnofoxEbShrinkResult *r) { memset(r, 0, sizeof *r); }

} // namespace

extern "C" {

size_t anofox_hip_eb_shrink_summary_len(void) { return kEbSummaryLen; }

void anofox_hip_eb_shrink_test_hooks(int force_path, int64_t chunk_items, int64_t max_workgroups) {
	g_force_path.store(force_path == 1 || force_path == 2 ? force_path : 0);
	g_chunk_items.store(chunk_items > 0 ? chunk_items : 0);
	g_max_workgroups.store(max_workgroups > 0 ? max_workgroups : 0);
}

bool anofox_hip_eb_shrink_batch_device(AnofoxHipContext *ctx, int64_t n_sets, int64_t n_items, const int64_t *d_set_offsets, size_t n_cols,
                                       const double *d_est, int64_t est_stride, const double *d_se, int64_t se_stride,
                                       AnofoxHipEbShrinkOptions options, double *d_out, double *d_summary, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_eb(n_sets, n_items, d_set_offsets, n_cols, d_est, est_stride, d_se, se_stride, d_out, d_summary, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_eb(ctx, n_sets, n_items, d_set_offsets, n_cols, d_est, est_stride, d_se, se_stride, options, d_out, d_summary, out_error);
}

bool anofox_hip_eb_shrink_batch_host(AnofoxHipContext *ctx, int64_t n_sets, int64_t n_items, const int64_t *set_offsets, size_t n_cols,
                                     const double *est, int64_t est_stride, const double *se, int64_t se_stride,
                                     AnofoxHipEbShrinkOptions options, double *out, double *summary, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_eb(n_sets, n_items, set_offsets, n_cols, est, est_stride, se, se_stride, out, summary, out_error)) return false;
	if (n_sets > 0) {
		for (int64_t s = 0; s < n_sets; ++s) {
			if (set_offsets[s + 1] < set_offsets[s] || set_offsets[s] < 0 || set_offsets[s + 1] > n_items) {
				set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "set_offsets must be non-decreasing and within [0, n_items]");
				return false;
			}
		}
	}
	if (n_sets == 0) return true;
	return eb_host(ctx, n_sets, n_items, set_offsets, n_cols, est, est_stride, se, se_stride, options, out, summary, out_error);
}

// A batch of one set with anofox_ols_fit's conventions: argument checks first, NULL entries -> NaN, the arrays malloc'ed.
bool anofox_eb_shrink(AnofoxDataArray estimate, AnofoxDataArray se, AnofoxEbShrinkOptions options, AnofoxEbShrinkResult *out_result,
                      AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_result) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL"); return false; }
	reset_eb_result(out_result); // a failed call leaves nothing to free
	if (estimate.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: estimate cannot be empty"); return false; }
	if (se.len != estimate.len) {
		set_error(out_error, ANOFOX_ERROR_DIMENSION_MISMATCH,
		          "Dimension mismatch: estimate has " + std::to_string(estimate.len) + " elements, se has " + std::to_string(se.len));
		return false;
	}
	if (eb_options_invalid((int)options.method, options.tau_squared)) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, (int)options.method != kEbMethodDL && (int)options.method != kEbMethodNone
		                                                     ? "Invalid value for 'method': unknown tau method"
		                                                     : "Invalid value for 'tau_squared': tau_squared must be finite and non-negative");
		return false;
	}
	const size_t n = estimate.len;
	std::vector<double> ev, sv, out(n * kEbOutLen), sum(kEbSummaryLen);
	expand_data_array(estimate, ev);
	expand_data_array(se, sv);
	const int64_t off[2] = {0, (int64_t)n};
	const AnofoxHipEbShrinkOptions batch = {(int)options.method, options.tau_squared};
	if (!eb_host(nullptr, 1, (int64_t)n, off, 1, ev.data(), 1, sv.data(), 1, batch, out.data(), sum.data(), out_error)) return false;
	const int status = (int)sum[7];
	if (status != ANOFOX_ERROR_SUCCESS) {
		size_t k = 0;
		for (size_t i = 0; i < n; ++i) k += isfinite(ev[i]) && isfinite(sv[i]) && sv[i] > 0.0;
		set_error(out_error, (AnofoxErrorCode)status,
		          status == ANOFOX_ERROR_INSUFFICIENT_DATA ? "Insufficient data: " + std::to_string(k) + " usable pairs, need at least 2"
		                                                   : std::string("eb_shrink failed on the GPU path"));
		return false;
	}
	double *parts[5];
	bool ok = true;
	for (int b = 0; b < 5; ++b) ok = (parts[b] = (double *)malloc(n * sizeof(double))) && ok;
	if (!ok) {
		for (int b = 0; b < 5; ++b) free(parts[b]);
		set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the result arrays");
		return false;
	}
	for (size_t i = 0; i < n; ++i) {
		parts[0][i] = ev[i];
		parts[1][i] = sv[i];
		for (int b = 0; b < 3; ++b) parts[2 + b][i] = out[i * kEbOutLen + b];
	}
	out_result->mu = sum[0];
	out_result->mu_se = sum[1];
	out_result->tau_squared = sum[2];
	out_result->i_squared = sum[3];
	out_result->q = sum[4];
	out_result->n_groups = (size_t)sum[5];
	out_result->estimate = parts[0];
	out_result->se = parts[1];
	out_result->shrunken = parts[2];
	out_result->shrunken_se = parts[3];
	out_result->weight = parts[4];
	out_result->len = n;
	return true;
}

void anofox_free_eb_shrink_result(AnofoxEbShrinkResult *result) {
	if (!result) return;
	free(result->estimate);
	free(result->se);
	free(result->shrunken);
	free(result->shrunken_se);
	free(result->weight);
	result->estimate = result->se = result->shrunken = result->shrunken_se = result->weight = nullptr;
	result->len = 0;
}

} // extern "C"
