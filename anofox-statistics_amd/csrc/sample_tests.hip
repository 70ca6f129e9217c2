// sample_tests.hip — grouped t-test, Yuen, one-way ANOVA, Brown-Forsythe and Brunner-Munzel tests (sample_tests.h): the third family
// on the size-tiered launch driver of rank_launch.h and the entry points anofox_hip_sample_test_batch_{device,host},
// anofox_hip_sample_test_record_len, anofox_hip_sample_test_hooks, anofox_t_test / anofox_yuen_test / anofox_brunner_munzel /
// anofox_one_way_anova / anofox_brown_forsythe / anofox_free_anova_result.
//
// The contract and the method: sample_tests.h and DESIGN.md §1, "Parametric and studentised-rank tests".
//   rank_small_kernel<CAP, SampleTestFamily>, rank_large_kernel<SampleTestFamily>: the two size paths (rank_launch.h).  The t-test
//     stages nothing (staged() is false: every group runs on the first small instance); the other tests stage their rows, and
//     nothing follows the large kernel.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "sample_tests.h"
#include "rank_launch.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;
using namespace anofox::sampletest;
using namespace anofox::rank;

namespace {

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_sample_test_hooks

struct SampleTestFamily {
	static constexpr const char *kSmallKernel = "rank_small_kernel<SampleTestFamily>", *kLargeKernel = "rank_large_kernel<SampleTestFamily>",
	                            *kScratch = "sample test scratch";
	SampleTestProblem P;

	__host__ __device__ bool staged() const { return P.test != kStT; }

	__device__ __forceinline__ void small_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		st_group(P, g, lo, hi, W, true, threadIdx.x, 64);
	}

	__device__ __forceinline__ void large_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		st_group(P, g, lo, hi, W, threadIdx.x < 64, threadIdx.x, kRankLargeThreads);
	}

	// nothing in the workspace but the work arrays, nothing around the large kernel
	size_t prefix_bytes(int64_t) const { return 0; }
	bool begin_large(char *, int64_t, hipStream_t, AnofoxError *) { return true; }
	bool end_large(const RankCall &, hipStream_t, AnofoxError *) const { return true; }
};

bool paired(const AnofoxHipSampleTestBatchOptions &o) { return o.test == kStT && o.kind == kStPaired; }

bool check_sample_test(int64_t n_groups, int64_t n_rows, const void *off, const double *v, const double *y, const int32_t *sample,
                       const AnofoxHipSampleTestBatchOptions &o, const void *records, AnofoxError *e) {
	if (n_groups < 0 || n_rows < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (const char *text = st_options_text(o.test, o.alternative, o.kind, o.mu, o.trim, o.confidence_level)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, text);
		return false;
	}
	if (n_groups == 0) return true;
	if (!off || !v || !records) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "sample test: row_offsets, v or records is NULL"); return false; }
	if (paired(o) && !y) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "sample test: the paired t-test needs the y column");
		return false;
	}
	if (!paired(o) && !sample) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "sample test: every test but the paired t-test needs the sample column");
		return false;
	}
	return true;
}

// the tests of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_sample_test(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const double *d_v, const double *d_y,
                        const int32_t *d_sample, const AnofoxHipSampleTestBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	SampleTestFamily f;
	memset(&f, 0, sizeof f);
	f.P.v = d_v;
	f.P.y = d_y;
	f.P.sample = d_sample;
	f.P.n_rows = n_rows;
	f.P.test = o.test;
	f.P.alternative = o.alternative;
	f.P.kind = o.kind;
	f.P.mu = o.mu;
	f.P.trim = o.trim;
	f.P.confidence_level = o.confidence_level;
	f.P.records = d_rec;
	RankCall c;
	memset(&c, 0, sizeof c);
	c.off = d_off;
	c.n_groups = n_groups;
	c.n_rows = n_rows;
	return launch_tiers(ctx, c, g_small_cap.load(), f, e);
}

// host pointers: one staging of the whole call, the kernels, the records back
bool sample_test_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *off, const double *v, const double *y,
                      const int32_t *sample, const AnofoxHipSampleTestBatchOptions &o, double *records, AnofoxError *e) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	const bool pairs = paired(o);
	int64_t *d_off;
	double *d_v, *d_y, *d_rec;
	int32_t *d_sample;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(off, G + 1);
		    d_v = s.put(v, (size_t)n_rows);
		    d_y = pairs ? s.put(y, (size_t)n_rows) : nullptr;
		    d_sample = pairs ? nullptr : s.put(sample, (size_t)n_rows);
		    d_rec = s.take<double>(G * kStRecordLen);
	    }))
		return false;
	if (!launch_sample_test(ctx, n_groups, n_rows, d_off, d_v, d_y, d_sample, o, d_rec, e)) return false;
	if (!d2h(records, d_rec, G * kStRecordLen * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

bool fail(AnofoxError *e, const std::string &text) {
	set_error(e, ANOFOX_ERROR_INVALID_INPUT, text);
	return false;
}

// the reference reads a NaN mu as absent
double mu_in(double mu) { return mu == mu ? mu : 0.0; }

size_t count_valid(const std::vector<double> &v) {
	size_t n = 0;
	for (double a : v) n += a == a;
	return n;
}

// One group through the host batch entry -> its record
bool scalar_record(const std::vector<double> &v, const std::vector<int32_t> &sample, const AnofoxHipSampleTestBatchOptions &o, double *rec,
                   AnofoxError *e) {
	const int64_t off[2] = {0, (int64_t)v.size()};
	return sample_test_host(nullptr, 1, off[1], off, v.data(), nullptr, sample.data(), o, rec, e);
}

// A two-sample scalar: group1 is sample 0, group2 sample 1.  `least`: the rows an arm needs, `name` the test's in the reference's
// texts.
bool scalar_two_sample(const char *name, size_t least, const std::string &method, AnofoxDataArray group1, AnofoxDataArray group2,
                       const AnofoxHipSampleTestBatchOptions &o, AnofoxTestResult *out, AnofoxError *e) {
	reset_error(e);
	if (!out) return fail(e, "out_result is NULL");
	memset(out, 0, sizeof *out); // a failed call leaves nothing to free
	if (const char *text = st_options_text(o.test, o.alternative, o.kind, o.mu, o.trim, o.confidence_level)) return fail(e, text);
	std::vector<double> v, v2;
	expand_data_array(group1, v);
	expand_data_array(group2, v2);
	const size_t n1 = count_valid(v), n2 = count_valid(v2);
	for (int arm = 0; arm < 2; ++arm)
		if ((arm ? n2 : n1) < least)
			return fail(e, std::string(name) + " requires at least " + std::to_string(least) + " observations in group " + std::to_string(arm + 1));
	std::vector<int32_t> sample(v.size() + v2.size(), 1);
	std::fill(sample.begin(), sample.begin() + (ptrdiff_t)v.size(), 0);
	v.insert(v.end(), v2.begin(), v2.end());
	double rec[kStRecordLen];
	if (!scalar_record(v, sample, o, rec, e)) return false;
	if (rec[11] != 0.0) return fail(e, std::string(name) + ": too few observations remain after trimming");
	char *text = copy_text(method.c_str());
	if (!text) { set_error(e, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name"); return false; }
	out->statistic = rec[0];
	out->p_value = rec[1];
	out->df = rec[2];
	out->effect_size = o.test == kStBrunnerMunzel ? rec[4] : NAN;
	out->ci_lower = rec[5];
	out->ci_upper = rec[6];
	out->confidence_level = o.confidence_level;
	out->n = n1 + n2;
	out->n1 = n1;
	out->n2 = n2;
	out->alternative = (AnofoxAlternative)o.alternative;
	out->method = text;
	return true;
}

// The arms of a k-sample scalar: the reference zips the two arrays and keys a map by the id cast to an integer; a NaN in either
// drops the row.  -> the arms; `least`: the rows of the smallest, `small`: its number in the order of first appearance.
size_t scalar_arms(AnofoxDataArray values, AnofoxDataArray groups, std::vector<double> &v, std::vector<int32_t> &sample, size_t &n, size_t &least,
                   size_t &small) {
	std::vector<double> gv;
	expand_data_array(values, v);
	expand_data_array(groups, gv);
	const size_t len = v.size() < gv.size() ? v.size() : gv.size();
	v.resize(len);
	sample.assign(len, 0);
	std::unordered_map<int64_t, int32_t> ids;
	std::vector<size_t> rows;
	n = 0;
	for (size_t i = 0; i < len; ++i) {
		if (v[i] != v[i] || gv[i] != gv[i]) {
			v[i] = NAN;
			continue;
		}
		const double t = trunc(gv[i]); // Rust's `as i64`: towards zero, saturating
		const int64_t id = t >= 9223372036854775807.0 ? INT64_MAX : (t <= -9223372036854775808.0 ? INT64_MIN : (int64_t)t);
		sample[i] = ids.emplace(id, (int32_t)ids.size()).first->second;
		if ((size_t)sample[i] == rows.size()) rows.push_back(0);
		++rows[(size_t)sample[i]];
		++n;
	}
	least = SIZE_MAX;
	small = 0;
	for (size_t j = 0; j < rows.size(); ++j)
		if (rows[j] < least) {
			least = rows[j];
			small = j;
		}
	return rows.size();
}

// the guards of parametric.rs for a k-sample test called `name`
bool check_arms(const char *name, size_t k, size_t least, size_t small, AnofoxError *e) {
	if (k < 2) return fail(e, std::string(name) + " requires at least 2 groups");
	if (least < 2)
		return fail(e, std::string(name) + " requires at least 2 observations per group (group " + std::to_string(small) + " has " +
		                   std::to_string(least) + ")");
	return true;
}

} // namespace

extern "C" {

size_t anofox_hip_sample_test_record_len(void) { return kStRecordLen; }

void anofox_hip_sample_test_hooks(int64_t small_cap) { g_small_cap.store(small_cap > 0 ? small_cap : 0); }

bool anofox_hip_sample_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets, const double *d_v,
                                         const double *d_y, const int32_t *d_sample, AnofoxHipSampleTestBatchOptions options, double *d_records,
                                         AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_sample_test(n_groups, n_rows, d_row_offsets, d_v, d_y, d_sample, options, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_sample_test(ctx, n_groups, n_rows, d_row_offsets, d_v, d_y, d_sample, options, d_records, out_error);
}

bool anofox_hip_sample_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets, const double *v,
                                       const double *y, const int32_t *sample, AnofoxHipSampleTestBatchOptions options, double *records,
                                       AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_sample_test(n_groups, n_rows, row_offsets, v, y, sample, options, records, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	return sample_test_host(ctx, n_groups, n_rows, row_offsets, v, y, sample, options, records, out_error);
}

bool anofox_t_test(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxTTestOptions options, AnofoxTestResult *out_result, AnofoxError *out_error) {
	const AnofoxHipSampleTestBatchOptions o = {kStT, (int32_t)options.alternative, options.var_equal ? kStStudent : kStWelch, mu_in(options.mu), 0.0,
	                                           options.confidence_level};
	return scalar_two_sample("t-test", 2, options.var_equal ? "Student t-test" : "Welch t-test", group1, group2, o, out_result, out_error);
}

bool anofox_yuen_test(AnofoxDataArray group1, AnofoxDataArray group2, double trim, AnofoxAlternative alternative, double confidence_level,
                      AnofoxTestResult *out_result, AnofoxError *out_error) {
	const AnofoxHipSampleTestBatchOptions o = {kStYuen, (int32_t)alternative, 0, 0.0, trim, confidence_level};
	char method[64];
	snprintf(method, sizeof method, "Yuen test (trim=%.2f)", trim);
	return scalar_two_sample("Yuen test", 4, method, group1, group2, o, out_result, out_error);
}

bool anofox_brunner_munzel(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxBrunnerMunzelOptions options, AnofoxTestResult *out_result,
                           AnofoxError *out_error) {
	const AnofoxHipSampleTestBatchOptions o = {kStBrunnerMunzel, (int32_t)options.alternative, 0, 0.0, 0.0, options.confidence_level};
	return scalar_two_sample("Brunner-Munzel test", 2, "Brunner-Munzel test", group1, group2, o, out_result, out_error);
}

bool anofox_one_way_anova(AnofoxDataArray values, AnofoxDataArray groups, AnofoxAnovaResult *out_result, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_result) return fail(out_error, "out_result is NULL");
	memset(out_result, 0, sizeof *out_result);
	std::vector<double> v;
	std::vector<int32_t> sample;
	size_t n, least, small;
	const size_t k = scalar_arms(values, groups, v, sample, n, least, small);
	if (!check_arms("ANOVA", k, least, small, out_error)) return false;
	const AnofoxHipSampleTestBatchOptions o = {kStAnova, 0, kStFisher, 0.0, 0.0, NAN};
	double rec[kStRecordLen];
	if (!scalar_record(v, sample, o, rec, out_error)) return false;
	if (rec[11] != 0.0) return fail(out_error, "ANOVA failed on the GPU path");
	char *text = copy_text("Fisher One-way ANOVA");
	if (!text) { set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name"); return false; }
	out_result->f_statistic = rec[0];
	out_result->p_value = rec[1];
	out_result->df_between = (size_t)rec[2];
	out_result->df_within = (size_t)rec[3];
	out_result->ss_between = rec[4];
	out_result->ss_within = rec[10];
	out_result->n_groups = k;
	out_result->n = n;
	out_result->method = text;
	return true;
}

bool anofox_brown_forsythe(AnofoxDataArray values, AnofoxDataArray groups, AnofoxTestResult *out_result, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_result) return fail(out_error, "out_result is NULL");
	memset(out_result, 0, sizeof *out_result);
	std::vector<double> v;
	std::vector<int32_t> sample;
	size_t n, least, small;
	const size_t k = scalar_arms(values, groups, v, sample, n, least, small);
	if (!check_arms("Brown-Forsythe test", k, least, small, out_error)) return false;
	const AnofoxHipSampleTestBatchOptions o = {kStBrownForsythe, 0, 0, 0.0, 0.0, NAN};
	double rec[kStRecordLen];
	if (!scalar_record(v, sample, o, rec, out_error)) return false;
	if (rec[11] != 0.0) return fail(out_error, "Brown-Forsythe test failed on the GPU path");
	char *text = copy_text("Brown-Forsythe test");
	if (!text) { set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name"); return false; }
	out_result->statistic = rec[0];
	out_result->p_value = rec[1];
	out_result->df = rec[2];
	out_result->effect_size = NAN;
	out_result->ci_lower = NAN;
	out_result->ci_upper = NAN;
	out_result->confidence_level = NAN;
	out_result->n = n;
	out_result->n1 = 0; // the reference's counts
	out_result->n2 = 0;
	out_result->alternative = ANOFOX_ALTERNATIVE_TWO_SIDED;
	out_result->method = text;
	return true;
}

void anofox_free_anova_result(AnofoxAnovaResult *result) {
	if (!result) return;
	free(result->method);
	result->method = nullptr;
}

} // extern "C"
