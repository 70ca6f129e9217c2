// rank_tests.hip — grouped Mann-Whitney U, Wilcoxon signed-rank and Kruskal-Wallis tests (rank_tests.h): the family that runs on
// the size-tiered launch driver of rank_launch.h and the entry points anofox_hip_rank_test_batch_{device,host},
// anofox_hip_rank_test_record_len, anofox_hip_rank_test_hooks, anofox_mann_whitney_u / anofox_wilcoxon_signed_rank /
// anofox_kruskal_wallis / anofox_free_test_result.
//
// The contract and the method: rank_tests.h and DESIGN.md §1, "Rank-based location tests".
//   rank_small_kernel<CAP, RankTestFamily>, rank_large_kernel<RankTestFamily>: the two size paths (rank_launch.h); every test
//     stages its rows, and nothing follows the large kernel.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "rank_tests.h"
#include "rank_launch.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;
using namespace anofox::ranktest;
using namespace anofox::rank;

namespace {

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_rank_test_hooks

struct RankTestFamily {
	static constexpr const char *kSmallKernel = "rank_small_kernel<RankTestFamily>", *kLargeKernel = "rank_large_kernel<RankTestFamily>",
	                            *kScratch = "rank test scratch";
	RankTestProblem P;

	__host__ __device__ bool staged() const { return true; }

	__device__ __forceinline__ void small_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		rt_group(P, g, lo, hi, W, true, threadIdx.x, 64);
	}

	__device__ __forceinline__ void large_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		rt_group(P, g, lo, hi, W, threadIdx.x < 64, threadIdx.x, kRankLargeThreads);
	}

	// nothing in the workspace but the work arrays, nothing around the large kernel
	size_t prefix_bytes(int64_t) const { return 0; }
	bool begin_large(char *, int64_t, hipStream_t, AnofoxError *) { return true; }
	bool end_large(const RankCall &, hipStream_t, AnofoxError *) const { return true; }
};

bool check_rank_test(int64_t n_groups, int64_t n_rows, const void *off, const double *v, const double *y, const int32_t *sample,
                     const AnofoxHipRankTestBatchOptions &o, const void *records, AnofoxError *e) {
	if (n_groups < 0 || n_rows < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (const char *text = rt_options_text(o.test, o.alternative, o.mu)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, text); return false; }
	if (n_groups == 0) return true;
	if (!off || !v || !records) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "rank test: row_offsets, v or records is NULL"); return false; }
	if (o.test == kRtWilcoxon && !y) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "rank test: the Wilcoxon signed-rank test needs the y column");
		return false;
	}
	if (o.test != kRtWilcoxon && !sample) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "rank test: the Mann-Whitney and Kruskal-Wallis tests need the sample column");
		return false;
	}
	return true;
}

// the tests of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_rank_test(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const double *d_v, const double *d_y,
                      const int32_t *d_sample, const AnofoxHipRankTestBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	RankTestFamily f;
	memset(&f, 0, sizeof f);
	f.P.v = d_v;
	f.P.y = d_y;
	f.P.sample = d_sample;
	f.P.n_rows = n_rows;
	f.P.test = o.test;
	f.P.alternative = o.alternative;
	f.P.correction = o.continuity_correction != 0;
	f.P.mu = o.mu;
	f.P.records = d_rec;
	RankCall c;
	memset(&c, 0, sizeof c);
	c.off = d_off;
	c.n_groups = n_groups;
	c.n_rows = n_rows;
	return launch_tiers(ctx, c, g_small_cap.load(), f, e);
}

// host pointers: one staging of the whole call, the kernels, the records back
bool rank_test_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *off, const double *v, const double *y,
                    const int32_t *sample, const AnofoxHipRankTestBatchOptions &o, double *records, AnofoxError *e) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	const bool paired = o.test == kRtWilcoxon;
	int64_t *d_off;
	double *d_v, *d_y, *d_rec;
	int32_t *d_sample;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(off, G + 1);
		    d_v = s.put(v, (size_t)n_rows);
		    d_y = paired ? s.put(y, (size_t)n_rows) : nullptr;
		    d_sample = paired ? nullptr : s.put(sample, (size_t)n_rows);
		    d_rec = s.take<double>(G * kRtRecordLen);
	    }))
		return false;
	if (!launch_rank_test(ctx, n_groups, n_rows, d_off, d_v, d_y, d_sample, o, d_rec, e)) return false;
	if (!d2h(records, d_rec, G * kRtRecordLen * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

bool fail(AnofoxError *e, const std::string &text) {
	set_error(e, ANOFOX_ERROR_INVALID_INPUT, text);
	return false;
}

bool begin_scalar(AnofoxTestResult *out, AnofoxError *e) {
	reset_error(e);
	if (!out) return fail(e, "out_result is NULL");
	memset(out, 0, sizeof *out); // a failed call leaves nothing to free
	return true;
}

// One group through the host batch entry; the counts of the result are the caller's (the reference's conventions differ by test)
bool scalar_rank_test(const char *method_text, const std::vector<double> &v, const double *y, const int32_t *sample,
                      const AnofoxHipRankTestBatchOptions &o, double level_out, AnofoxTestResult *out, AnofoxError *e) {
	const int64_t off[2] = {0, (int64_t)v.size()};
	double rec[kRtRecordLen];
	if (!rank_test_host(nullptr, 1, off[1], off, v.data(), y, sample, o, rec, e)) return false;
	if (rec[7] != 0.0) return fail(e, std::string(method_text) + " failed on the GPU path");
	char *text = copy_text(method_text);
	if (!text) { set_error(e, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name"); return false; }
	out->statistic = rec[0];
	out->p_value = rec[2];
	out->df = rec[3];
	out->effect_size = NAN; // not built, as in the reference
	out->ci_lower = NAN;    // the Hodges-Lehmann interval is not built
	out->ci_upper = NAN;
	out->confidence_level = level_out;
	out->alternative = (AnofoxAlternative)o.alternative;
	out->method = text;
	return true;
}

// the reference reads a confidence level that is not > 0 as absent and reports 0.95; a NaN mu is absent too
double level_out(double level) { return level > 0.0 ? level : 0.95; }
double mu_in(double mu) { return mu == mu ? mu : 0.0; }

} // namespace

extern "C" {

size_t anofox_hip_rank_test_record_len(void) { return kRtRecordLen; }

void anofox_hip_rank_test_hooks(int64_t small_cap) { g_small_cap.store(small_cap > 0 ? small_cap : 0); }

bool anofox_hip_rank_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets, const double *d_v,
                                       const double *d_y, const int32_t *d_sample, AnofoxHipRankTestBatchOptions options, double *d_records,
                                       AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_rank_test(n_groups, n_rows, d_row_offsets, d_v, d_y, d_sample, options, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_rank_test(ctx, n_groups, n_rows, d_row_offsets, d_v, d_y, d_sample, options, d_records, out_error);
}

bool anofox_hip_rank_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets, const double *v,
                                     const double *y, const int32_t *sample, AnofoxHipRankTestBatchOptions options, double *records,
                                     AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_rank_test(n_groups, n_rows, row_offsets, v, y, sample, options, records, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	return rank_test_host(ctx, n_groups, n_rows, row_offsets, v, y, sample, options, records, out_error);
}

bool anofox_mann_whitney_u(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxMannWhitneyOptions options, AnofoxTestResult *out_result,
                           AnofoxError *out_error) {
	if (!begin_scalar(out_result, out_error)) return false;
	if (options.exact) return fail(out_error, "Mann-Whitney U test: exact p-values are not built");
	const AnofoxHipRankTestBatchOptions o = {kRtMannWhitney, (int32_t)options.alternative, options.continuity_correction ? 1 : 0, mu_in(options.mu)};
	if (const char *text = rt_options_text(o.test, o.alternative, o.mu)) return fail(out_error, text);
	std::vector<double> v, v2;
	expand_data_array(group1, v);
	expand_data_array(group2, v2);
	std::vector<int32_t> sample(v.size() + v2.size(), 1);
	std::fill(sample.begin(), sample.begin() + (ptrdiff_t)v.size(), 0);
	size_t n1 = 0, n2 = 0;
	for (double a : v) n1 += a == a;
	for (double a : v2) n2 += a == a;
	if (n1 < 1 || n2 < 1) return fail(out_error, "Mann-Whitney U test requires at least 1 observation per group");
	v.insert(v.end(), v2.begin(), v2.end());
	if (!scalar_rank_test("Mann-Whitney U test", v, nullptr, sample.data(), o, level_out(options.confidence_level), out_result, out_error)) return false;
	out_result->n = n1 + n2;
	out_result->n1 = n1;
	out_result->n2 = n2;
	return true;
}

bool anofox_wilcoxon_signed_rank(AnofoxDataArray x, AnofoxDataArray y, AnofoxWilcoxonOptions options, AnofoxTestResult *out_result,
                                 AnofoxError *out_error) {
	if (!begin_scalar(out_result, out_error)) return false;
	if (x.len != y.len) return fail(out_error, "Wilcoxon signed-rank test requires equal length samples");
	if (options.exact) return fail(out_error, "Wilcoxon signed-rank test: exact p-values are not built");
	const AnofoxHipRankTestBatchOptions o = {kRtWilcoxon, (int32_t)options.alternative, options.continuity_correction ? 1 : 0, mu_in(options.mu)};
	if (const char *text = rt_options_text(o.test, o.alternative, o.mu)) return fail(out_error, text);
	std::vector<double> xv, yv;
	expand_data_array(x, xv);
	expand_data_array(y, yv);
	size_t valid = 0;
	for (size_t i = 0; i < xv.size(); ++i) {
		const double d = xv[i] - yv[i] - o.mu;
		valid += d == d;
	}
	if (valid < 2) return fail(out_error, "Wilcoxon signed-rank test requires at least 2 valid pairs");
	if (!scalar_rank_test("Wilcoxon signed-rank test", xv, yv.data(), nullptr, o, level_out(options.confidence_level), out_result, out_error))
		return false;
	out_result->n = out_result->n1 = out_result->n2 = valid; // the reference's counts: the valid pairs, three times
	return true;
}

bool anofox_kruskal_wallis(AnofoxDataArray values, AnofoxDataArray groups, AnofoxTestResult *out_result, AnofoxError *out_error) {
	if (!begin_scalar(out_result, out_error)) return false;
	std::vector<double> v, gv;
	expand_data_array(values, v);
	expand_data_array(groups, gv);
	// the reference zips the two arrays and keys a map by the id cast to an integer; a NaN in either drops the row
	const size_t len = v.size() < gv.size() ? v.size() : gv.size();
	v.resize(len);
	std::vector<int32_t> sample(len, 0);
	std::unordered_map<int64_t, int32_t> ids;
	size_t n = 0;
	for (size_t i = 0; i < len; ++i) {
		if (v[i] != v[i] || gv[i] != gv[i]) {
			v[i] = NAN;
			continue;
		}
		const double t = trunc(gv[i]); // Rust's `as i64`: towards zero, saturating
		const int64_t id = t >= 9223372036854775807.0 ? INT64_MAX : (t <= -9223372036854775808.0 ? INT64_MIN : (int64_t)t);
		sample[i] = ids.emplace(id, (int32_t)ids.size()).first->second;
		++n;
	}
	if (ids.size() < 2) return fail(out_error, "Kruskal-Wallis test requires at least 2 groups");
	if (n < 3) return fail(out_error, "Kruskal-Wallis test requires at least 3 observations");
	const AnofoxHipRankTestBatchOptions o = {kRtKruskalWallis, 0, 0, 0.0};
	if (!scalar_rank_test("Kruskal-Wallis H test", v, nullptr, sample.data(), o, NAN, out_result, out_error)) return false;
	out_result->n = n;
	return true;
}

void anofox_free_test_result(AnofoxTestResult *result) {
	if (!result) return;
	free(result->method);
	result->method = nullptr;
}

} // extern "C"
