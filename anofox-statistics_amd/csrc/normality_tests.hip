// normality_tests.hip — grouped Shapiro-Wilk, D'Agostino K2 and Jarque-Bera normality tests (normality_tests.h): the fourth family on
// the size-tiered launch driver of rank_launch.h and the entry points anofox_hip_normality_test_batch_{device,host},
// anofox_hip_normality_test_record_len, anofox_hip_normality_test_hooks, anofox_shapiro_wilk / anofox_dagostino_k2 /
// anofox_jarque_bera.
//
// The contract and the method: normality_tests.h and DESIGN.md §1, "Normality tests".
//   rank_small_kernel<CAP, NormalityFamily>, rank_large_kernel<NormalityFamily>: the two size paths (rank_launch.h).  Jarque-Bera
//     and K2 stage nothing (staged() is false: every group runs on the first small instance); Shapiro-Wilk stages its rows, and
//     nothing follows the large kernel.
#include <math.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "normality_tests.h"
#include "rank_launch.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;
using namespace anofox::normtest;
using namespace anofox::rank;

namespace {

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_normality_test_hooks

struct NormalityFamily {
	static constexpr const char *kSmallKernel = "rank_small_kernel<NormalityFamily>", *kLargeKernel = "rank_large_kernel<NormalityFamily>",
	                            *kScratch = "normality test scratch";
	NormalityProblem P;

	__host__ __device__ bool staged() const { return P.test == kNtShapiroWilk; }

	__device__ __forceinline__ void small_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		nt_group(P, g, lo, hi, W, true, threadIdx.x, 64);
	}

	__device__ __forceinline__ void large_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		nt_group(P, g, lo, hi, W, threadIdx.x < 64, threadIdx.x, kRankLargeThreads);
	}

	// nothing in the workspace but the work arrays, nothing around the large kernel
	size_t prefix_bytes(int64_t) const { return 0; }
	bool begin_large(char *, int64_t, hipStream_t, AnofoxError *) { return true; }
	bool end_large(const RankCall &, hipStream_t, AnofoxError *) const { return true; }
};

bool check_normality_test(int64_t n_groups, int64_t n_rows, const void *off, const double *v, const AnofoxHipNormalityTestBatchOptions &o,
                          const void *records, AnofoxError *e) {
	if (n_groups < 0 || n_rows < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (const char *text = nt_options_text(o.test)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, text);
		return false;
	}
	if (n_groups == 0) return true;
	if (!off || !v || !records) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "normality test: row_offsets, v or records is NULL"); return false; }
	return true;
}

// the tests of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_normality_test(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const double *d_v,
                           const AnofoxHipNormalityTestBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	NormalityFamily f;
	memset(&f, 0, sizeof f);
	f.P.v = d_v;
	f.P.n_rows = n_rows;
	f.P.test = o.test;
	f.P.records = d_rec;
	RankCall c;
	memset(&c, 0, sizeof c);
	c.off = d_off;
	c.n_groups = n_groups;
	c.n_rows = n_rows;
	return launch_tiers(ctx, c, g_small_cap.load(), f, e);
}

// host pointers: one staging of the whole call, the kernels, the records back
bool normality_test_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *off, const double *v,
                         const AnofoxHipNormalityTestBatchOptions &o, double *records, AnofoxError *e) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off;
	double *d_v, *d_rec;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(off, G + 1);
		    d_v = s.put(v, (size_t)n_rows);
		    d_rec = s.take<double>(G * kNtRecordLen);
	    }))
		return false;
	if (!launch_normality_test(ctx, n_groups, n_rows, d_off, d_v, o, d_rec, e)) return false;
	if (!d2h(records, d_rec, G * kNtRecordLen * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

bool fail(AnofoxError *e, AnofoxErrorCode code, const std::string &text) {
	set_error(e, code, text);
	return false;
}

// One scalar: the reference's guards on the number of valid rows (answered before any device is touched), then one group through
// the host batch entry -> its record and the valid rows in n.  `name`: the test's in the reference's texts.
bool scalar_record(int test, const char *name, AnofoxDataArray data, double *rec, size_t &n, AnofoxError *e) {
	std::vector<double> v;
	expand_data_array(data, v);
	n = 0;
	for (double a : v) n += a == a;
	const size_t least = (size_t)nt_min_rows(test);
	if (n < least) return fail(e, ANOFOX_ERROR_INSUFFICIENT_DATA, std::string(name) + " test requires at least " + std::to_string(least) + " observations");
	if (test == kNtShapiroWilk && n > (size_t)kNtShapiroMaxRows) return fail(e, ANOFOX_ERROR_INVALID_INPUT, "Shapiro-Wilk test is limited to n <= 5000");
	const int64_t off[2] = {0, (int64_t)v.size()};
	const AnofoxHipNormalityTestBatchOptions o = {test, 0};
	if (!normality_test_host(nullptr, 1, off[1], off, v.data(), o, rec, e)) return false;
	if (rec[7] != 0.0) return fail(e, ANOFOX_ERROR_INVALID_INPUT, "Data has zero variance");
	return true;
}

bool scalar_test_result(int test, const char *name, const char *method, AnofoxDataArray data, AnofoxTestResult *out, AnofoxError *e) {
	reset_error(e);
	if (!out) return fail(e, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL");
	memset(out, 0, sizeof *out); // a failed call leaves nothing to free
	double rec[kNtRecordLen];
	size_t n;
	if (!scalar_record(test, name, data, rec, n, e)) return false;
	char *text = copy_text(method);
	if (!text) { set_error(e, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name"); return false; }
	out->statistic = rec[0];
	out->p_value = rec[1];
	out->df = test == kNtDagostinoK2 ? 2.0 : NAN;
	out->effect_size = NAN;
	out->ci_lower = NAN;
	out->ci_upper = NAN;
	out->confidence_level = NAN;
	out->n = n;
	out->n1 = 0; // the reference's counts
	out->n2 = 0;
	out->alternative = ANOFOX_ALTERNATIVE_TWO_SIDED;
	out->method = text;
	return true;
}

} // namespace

extern "C" {

size_t anofox_hip_normality_test_record_len(void) { return kNtRecordLen; }

void anofox_hip_normality_test_hooks(int64_t small_cap) { g_small_cap.store(small_cap > 0 ? small_cap : 0); }

bool anofox_hip_normality_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                            const double *d_v, AnofoxHipNormalityTestBatchOptions options, double *d_records,
                                            AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_normality_test(n_groups, n_rows, d_row_offsets, d_v, options, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_normality_test(ctx, n_groups, n_rows, d_row_offsets, d_v, options, d_records, out_error);
}

bool anofox_hip_normality_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets, const double *v,
                                          AnofoxHipNormalityTestBatchOptions options, double *records, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_normality_test(n_groups, n_rows, row_offsets, v, options, records, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	return normality_test_host(ctx, n_groups, n_rows, row_offsets, v, options, records, out_error);
}

bool anofox_shapiro_wilk(AnofoxDataArray data, AnofoxTestResult *out_result, AnofoxError *out_error) {
	return scalar_test_result(kNtShapiroWilk, "Shapiro-Wilk", "Shapiro-Wilk test", data, out_result, out_error);
}

bool anofox_dagostino_k2(AnofoxDataArray data, AnofoxTestResult *out_result, AnofoxError *out_error) {
	return scalar_test_result(kNtDagostinoK2, "D'Agostino K-squared", "D'Agostino K-squared test", data, out_result, out_error);
}

bool anofox_jarque_bera(AnofoxDataArray data, AnofoxJarqueBeraResult *out_result, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_result) return fail(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL");
	memset(out_result, 0, sizeof *out_result);
	double rec[kNtRecordLen];
	size_t n;
	if (!scalar_record(kNtJarqueBera, "Jarque-Bera", data, rec, n, out_error)) return false;
	out_result->statistic = rec[0];
	out_result->p_value = rec[1];
	out_result->skewness = rec[2];
	out_result->kurtosis = rec[3];
	out_result->n = n;
	return true;
}

} // extern "C"
