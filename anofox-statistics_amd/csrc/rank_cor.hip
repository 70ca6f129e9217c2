// rank_cor.hip — grouped Pearson, Spearman and Kendall correlation with their tests (rank_cor.h): the family that runs on the
// size-tiered launch driver of rank_launch.h, Kendall's pair kernels, and the entry points anofox_hip_cor_batch_{device,host},
// anofox_hip_cor_record_len, anofox_hip_cor_test_hooks, anofox_pearson_cor / anofox_spearman_cor / anofox_kendall_cor /
// anofox_free_correlation_result.
//
// The contract and the method: rank_cor.h and DESIGN.md §1, "Rank and product-moment correlation".
//   rank_small_kernel<CAP, CorFamily>, rank_large_kernel<CorFamily>: the two size paths (rank_launch.h).  Pearson stages nothing
//     and runs every group, whatever its size, on the first small instance: it streams the rows twice from memory.  On the large
//     path a Kendall group is entered into a list instead of being counted.
//   cor_pairs_kernel: the listed groups' pairs by (i block, j block) tiles of 256 x 256 rows, the j block in LDS, grid-stride over
//     the tiles; a wavefront adds its count into the group's int64 with one atomic add (a vector atomic; integer, so exact and
//     independent of the order).  cor_finish_kernel: a thread per listed group writes the record.
#include <math.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "rank_launch.h"
#include "host_math.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;
using namespace anofox::rank;

namespace {

constexpr int kCorPairWorkgroups = 2048; // 256 CUs x 8 workgroups of 256 threads

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_cor_test_hooks

struct CorFamily {
	static constexpr const char *kSmallKernel = "rank_small_kernel<CorFamily>", *kLargeKernel = "rank_large_kernel<CorFamily>",
	                            *kScratch = "correlation scratch";
	CorProblem P;
	// the large path's Kendall groups: a counter (256 bytes to itself) and the list it fills
	CorLarge *list;
	unsigned long long *count;
	int64_t slots;

	__host__ __device__ bool staged() const { return P.method != kCorPearson; }

	__device__ __forceinline__ void small_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		rc_group(P, g, lo, hi, W, true, threadIdx.x, 64, nullptr);
	}

	__device__ __forceinline__ void large_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		__shared__ long long s_slot;
		CorLarge *large = nullptr;
		if (P.method == kCorKendall) {
			if (threadIdx.x == 0) {
				const unsigned long long k = atomicAdd(count, 1ull);
				s_slot = k < (unsigned long long)slots ? (long long)k : -1; // (a full list: the wavefront counts the pairs itself)
				if (s_slot >= 0) {
					list[s_slot].group = g;
					list[s_slot].n = 0; // until the group is entered
				}
			}
			__syncthreads();
			if (s_slot >= 0) large = list + s_slot;
		}
		rc_group(P, g, lo, hi, W, threadIdx.x < 64, threadIdx.x, kRankLargeThreads, large);
	}

	size_t prefix_bytes(int64_t n) const { return 256 + (size_t)n * sizeof(CorLarge); }

	bool begin_large(char *prefix, int64_t n, hipStream_t st, AnofoxError *e) {
		count = (unsigned long long *)prefix;
		list = (CorLarge *)(prefix + 256);
		slots = n;
		return !hip_fail(hipMemsetAsync(count, 0, 256, st), "hipMemsetAsync", e);
	}

	bool end_large(const RankCall &c, hipStream_t st, AnofoxError *e) const; // Kendall's two kernels
};

__global__ __launch_bounds__(kCorPairTile) void cor_pairs_kernel(CorFamily f, CorWork W) {
	__shared__ double sx[kCorPairTile], sy[kCorPairTile];
	const int64_t listed = (int64_t)(*f.count < (unsigned long long)f.slots ? *f.count : (unsigned long long)f.slots);
	for (int64_t k = 0; k < listed; ++k) {
		const int64_t n = f.list[k].n, lo = f.list[k].lo;
		if (n < 3) continue;
		const double *x = W.x + lo, *y = W.y + lo;
		const int64_t nb = (n + kCorPairTile - 1) / kCorPairTile;
		int64_t s = 0;
		for (int64_t t = blockIdx.x; t < nb * nb; t += gridDim.x) {
			const int64_t ib = t / nb, jb = t % nb;
			if (jb < ib) continue; // pairs i < j only
			const int64_t j0 = jb * kCorPairTile, i = ib * kCorPairTile + threadIdx.x;
			const int64_t jn = n - j0 < kCorPairTile ? n - j0 : kCorPairTile;
			__syncthreads();
			if ((int64_t)threadIdx.x < jn) {
				sx[threadIdx.x] = x[j0 + threadIdx.x];
				sy[threadIdx.x] = y[j0 + threadIdx.x];
			}
			__syncthreads();
			if (i < n) s += rc_pairs_row(x[i], y[i], sx, sy, jb == ib ? (int64_t)threadIdx.x + 1 : 0, jn);
		}
		GiPL<int64_t> v;
		v.v[0] = s;
		const int64_t total = glm::gi_sum_i(v);
		if ((threadIdx.x & 63u) == 0 && total != 0) atomicAdd((unsigned long long *)&f.list[k].s, (unsigned long long)total);
	}
}

__global__ __launch_bounds__(64) void cor_finish_kernel(CorFamily f) {
	const int64_t listed = (int64_t)(*f.count < (unsigned long long)f.slots ? *f.count : (unsigned long long)f.slots);
	for (int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x; k < listed; k += (int64_t)gridDim.x * 64) {
		const CorLarge &L = f.list[k];
		if (L.n >= 3) rc_kendall_record(f.P, L.s, L.n, L.tx, L.ty, f.P.records + L.group * kCorRecordLen);
	}
}

bool CorFamily::end_large(const RankCall &c, hipStream_t st, AnofoxError *e) const {
	if (P.method != kCorKendall) return true;
	return launch(cor_pairs_kernel, "cor_pairs_kernel", kCorPairWorkgroups, kCorPairTile, st, e, *this, c.W) &&
	       launch(cor_finish_kernel, "cor_finish_kernel", (slots + 63) / 64, 64, st, e, *this);
}

const char *options_text(const AnofoxHipCorBatchOptions &o) {
	if (o.method < kCorPearson || o.method > kCorKendall) return "correlation: unknown method";
	if (o.alternative < kCorTwoSided || o.alternative > kCorGreater) return "correlation: unknown alternative";
	if (o.tau_type < kCorTauA || o.tau_type > kCorTauC) return "correlation: unknown tau_type";
	if (rc_options_invalid(o.method, o.alternative, o.tau_type, o.confidence_level)) return "correlation: confidence_level must lie in (0, 1)";
	return nullptr;
}

bool check_cor(int64_t n_groups, int64_t n_rows, const void *off, const double *x, const double *y, const AnofoxHipCorBatchOptions &o,
               const void *records, AnofoxError *e) {
	const double *cols[1] = {x};
	if (!check_batch_args(n_groups, 1, n_rows, off, y, cols, records, 1, nullptr, "correlation: row_offsets, y or records is NULL", false, e))
		return false;
	if (const char *text = options_text(o)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, text); return false; }
	return true;
}

// the correlations of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_cor(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const double *d_x, const double *d_y,
                const AnofoxHipCorBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	CorFamily f;
	memset(&f, 0, sizeof f);
	f.P.x = d_x;
	f.P.y = d_y;
	f.P.n_rows = n_rows;
	f.P.method = o.method;
	f.P.alternative = o.alternative;
	f.P.tau_type = o.tau_type;
	f.P.zq = o.confidence_level == o.confidence_level ? hostmath::normal_quantile(0.5 * (1.0 + o.confidence_level)) : NAN;
	f.P.records = d_rec;
	RankCall c;
	memset(&c, 0, sizeof c);
	c.off = d_off;
	c.n_groups = n_groups;
	c.n_rows = n_rows;
	return launch_tiers(ctx, c, g_small_cap.load(), f, e);
}

// host pointers: one staging of the whole call, the kernels, the records back
bool cor_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *off, const double *x, const double *y,
              const AnofoxHipCorBatchOptions &o, double *records, AnofoxError *e) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off;
	double *d_x, *d_y, *d_rec;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(off, G + 1);
		    d_x = s.put(x, (size_t)n_rows);
		    d_y = s.put(y, (size_t)n_rows);
		    d_rec = s.take<double>(G * kCorRecordLen);
	    }))
		return false;
	if (!launch_cor(ctx, n_groups, n_rows, d_off, d_x, d_y, o, d_rec, e)) return false;
	if (!d2h(records, d_rec, G * kCorRecordLen * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

// One group through the host batch entry with the reference's conventions: argument checks first, NULL entries -> NaN.
bool scalar_cor(const char *name, const char *method_text, AnofoxDataArray x, AnofoxDataArray y, const AnofoxHipCorBatchOptions &o,
                double level_out, AnofoxCorrelationResult *out, AnofoxError *e) {
	reset_error(e);
	if (!out) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL"); return false; }
	memset(out, 0, sizeof *out); // a failed call leaves nothing to free
	if (x.len != y.len) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, std::string(name) + " correlation requires equal length vectors"); return false; }
	if (const char *text = options_text(o)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, text); return false; }
	std::vector<double> xv, yv;
	expand_data_array(x, xv);
	expand_data_array(y, yv);
	size_t valid = 0;
	for (size_t i = 0; i < xv.size(); ++i) valid += xv[i] == xv[i] && yv[i] == yv[i];
	if (valid < 3) { // (answered here: a device is not needed to count)
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, std::string(name) + " correlation requires at least 3 valid pairs");
		return false;
	}
	const int64_t off[2] = {0, (int64_t)xv.size()};
	double rec[kCorRecordLen];
	if (!cor_host(nullptr, 1, off[1], off, xv.data(), yv.data(), o, rec, e)) return false;
	if (rec[7] != 0.0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, std::string(name) + " correlation failed on the GPU path"); return false; }
	char *text = copy_text(method_text);
	if (!text) { set_error(e, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name"); return false; }
	out->r = rec[0];
	out->statistic = rec[1];
	out->p_value = rec[2];
	out->ci_lower = rec[3];
	out->ci_upper = rec[4];
	out->confidence_level = level_out;
	out->n = (size_t)rec[5];
	out->method = text;
	return true;
}

} // namespace

extern "C" {

size_t anofox_hip_cor_record_len(void) { return kCorRecordLen; }

void anofox_hip_cor_test_hooks(int64_t small_cap) { g_small_cap.store(small_cap > 0 ? small_cap : 0); }

bool anofox_hip_cor_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets, const double *d_x,
                                 const double *d_y, AnofoxHipCorBatchOptions options, double *d_records, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_cor(n_groups, n_rows, d_row_offsets, d_x, d_y, options, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_cor(ctx, n_groups, n_rows, d_row_offsets, d_x, d_y, options, d_records, out_error);
}

bool anofox_hip_cor_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets, const double *x,
                               const double *y, AnofoxHipCorBatchOptions options, double *records, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_cor(n_groups, n_rows, row_offsets, x, y, options, records, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	return cor_host(ctx, n_groups, n_rows, row_offsets, x, y, options, records, out_error);
}

bool anofox_pearson_cor(AnofoxDataArray x, AnofoxDataArray y, AnofoxCorrelationOptions options, AnofoxCorrelationResult *out_result,
                        AnofoxError *out_error) {
	const AnofoxHipCorBatchOptions o = {kCorPearson, (int32_t)options.alternative, kCorTauB, options.confidence_level};
	return scalar_cor("Pearson", "Pearson correlation", x, y, o, options.confidence_level == options.confidence_level ? options.confidence_level : 0.95,
	                  out_result, out_error);
}

bool anofox_spearman_cor(AnofoxDataArray x, AnofoxDataArray y, AnofoxCorrelationOptions options, AnofoxCorrelationResult *out_result,
                         AnofoxError *out_error) {
	const AnofoxHipCorBatchOptions o = {kCorSpearman, (int32_t)options.alternative, kCorTauB, options.confidence_level};
	return scalar_cor("Spearman", "Spearman rank correlation", x, y, o, options.confidence_level == options.confidence_level ? options.confidence_level : 0.95,
	                  out_result, out_error);
}

bool anofox_kendall_cor(AnofoxDataArray x, AnofoxDataArray y, AnofoxKendallOptions options, AnofoxCorrelationResult *out_result,
                        AnofoxError *out_error) {
	static const char *const kNames[3] = {"Kendall's TauA", "Kendall's TauB", "Kendall's TauC"};
	const int tau = (int)options.tau_type;
	const AnofoxHipCorBatchOptions o = {kCorKendall, (int32_t)options.alternative, tau, NAN}; // (no interval: the level is not read)
	return scalar_cor("Kendall", tau >= 0 && tau < 3 ? kNames[tau] : "Kendall", x, y, o, NAN, out_result, out_error);
}

void anofox_free_correlation_result(AnofoxCorrelationResult *result) {
	if (!result) return;
	free(result->method);
	result->method = nullptr;
}

} // extern "C"
