// perm_tests.hip — grouped energy distance, permutation t- and MMD tests (perm_tests.h): the sixth family on the size-tiered
// launch driver of rank_launch.h and the entry points anofox_hip_perm_test_batch_{device,host}, anofox_hip_perm_test_record_len,
// anofox_hip_perm_test_hooks, anofox_energy_distance / anofox_mmd / anofox_permutation_t_test.
//
// The contract and the method: perm_tests.h and DESIGN.md §1, "Permutation tests".
//   rank_small_kernel<CAP, PermTestFamily>: one wavefront runs every round of its group, the sorted rows in LDS.
//   rank_large_kernel<PermTestFamily>: energy distance and the t-test.  The sixteen wavefronts sort; wavefront w then runs the
//     rounds w, w + 16, ... on the rows in the workspace and adds its count to one LDS counter with an atomic add of integers,
//     which no order changes; the first thread writes the record after a barrier.  An MMD group gets status 7.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <random>
#include <string>
#include <vector>

#include "common.h"
#include "perm_tests.h"
#include "rank_launch.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;
using namespace anofox::permtest;
using namespace anofox::rank;

static_assert(kPtMmdCap == kRankSmallCap, "MMD runs on the small path alone");

namespace {

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_perm_test_hooks

struct PermTestFamily {
	static constexpr const char *kSmallKernel = "rank_small_kernel<PermTestFamily>", *kLargeKernel = "rank_large_kernel<PermTestFamily>",
	                            *kScratch = "permutation test scratch";
	PermTestProblem P;

	__host__ __device__ bool staged() const { return true; }

	__device__ __forceinline__ void small_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		pt_group(P, g, lo, hi, W, threadIdx.x);
	}

	__device__ __forceinline__ void large_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		__shared__ PtInfo info;
		__shared__ unsigned long long count;
		PtInfo I = pt_prepare(P, lo, hi, W, threadIdx.x < 64, threadIdx.x, kRankLargeThreads, false);
		if (threadIdx.x == 0) {
			info = I;
			count = 0;
		}
		__syncthreads();
		I = info;
		double obs = NAN, aux = NAN;
		if (I.status == 0) { // (the same in every thread)
			const int64_t c = pt_rounds(P, I, W, threadIdx.x >> 6, kRankLargeThreads / 64, obs, aux);
			if ((threadIdx.x & 63u) == 0 && c != 0) atomicAdd(&count, (unsigned long long)c);
		}
		__syncthreads();
		if (threadIdx.x == 0) pt_record(P, I, obs, aux, (int64_t)count, P.records + g * kPtRecordLen);
	}

	// nothing in the workspace but the work arrays, nothing around the large kernel
	size_t prefix_bytes(int64_t) const { return 0; }
	bool begin_large(char *, int64_t, hipStream_t, AnofoxError *) { return true; }
	bool end_large(const RankCall &, hipStream_t, AnofoxError *) const { return true; }
};

bool check_perm_test(int64_t n_groups, int64_t n_rows, const void *off, const double *v, const int32_t *sample,
                     const AnofoxHipPermTestBatchOptions &o, const void *records, AnofoxError *e) {
	if (n_groups < 0 || n_rows < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (const char *text = pt_options_text(o.test, o.alternative, o.n_permutations, o.sigma)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, text); return false; }
	if (n_groups == 0) return true;
	if (!off || !v || !sample || !records) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "permutation test: row_offsets, v, sample or records is NULL");
		return false;
	}
	return true;
}

// the tests of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_perm_test(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const double *d_v, const int32_t *d_sample,
                      const AnofoxHipPermTestBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	PermTestFamily f;
	memset(&f, 0, sizeof f);
	f.P.v = d_v;
	f.P.sample = d_sample;
	f.P.n_rows = n_rows;
	f.P.test = o.test;
	f.P.alternative = o.alternative;
	f.P.n_perm = o.n_permutations;
	f.P.seed = o.seed;
	f.P.sigma = o.sigma;
	f.P.records = d_rec;
	RankCall c;
	memset(&c, 0, sizeof c);
	c.off = d_off;
	c.n_groups = n_groups;
	c.n_rows = n_rows;
	return launch_tiers(ctx, c, g_small_cap.load(), f, e);
}

// host pointers: one staging of the whole call, the kernels, the records back
bool perm_test_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *off, const double *v, const int32_t *sample,
                    const AnofoxHipPermTestBatchOptions &o, double *records, AnofoxError *e) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off;
	double *d_v, *d_rec;
	int32_t *d_sample;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(off, G + 1);
		    d_v = s.put(v, (size_t)n_rows);
		    d_sample = s.put(sample, (size_t)n_rows);
		    d_rec = s.take<double>(G * kPtRecordLen);
	    }))
		return false;
	if (!launch_perm_test(ctx, n_groups, n_rows, d_off, d_v, d_sample, o, d_rec, e)) return false;
	if (!d2h(records, d_rec, G * kPtRecordLen * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

bool fail(AnofoxError *e, const std::string &text) {
	set_error(e, ANOFOX_ERROR_INVALID_INPUT, text);
	return false;
}

uint64_t entropy_seed() {
	std::random_device rd;
	return ((uint64_t)rd() << 32) ^ (uint64_t)rd();
}

// A scalar of the reference's layout: group1 is sample 0, group2 sample 1, one group through the host batch entry.  `name`: the
// test's in the reference's texts, `method` its method text up to the permutations.
bool scalar_perm_test(const char *name, const char *method, AnofoxDataArray group1, AnofoxDataArray group2, int32_t test, int32_t alternative,
                      size_t n_permutations, uint64_t seed, bool has_seed, AnofoxTestResult *out, AnofoxError *e) {
	reset_error(e);
	if (!out) return fail(e, "out_result is NULL");
	memset(out, 0, sizeof *out); // a failed call leaves nothing to free
	const AnofoxHipPermTestBatchOptions o = {test, alternative, n_permutations > (size_t)INT64_MAX ? (int64_t)-1 : (int64_t)n_permutations,
	                                         has_seed ? seed : entropy_seed(), NAN};
	if (const char *text = pt_options_text(o.test, o.alternative, o.n_permutations, o.sigma)) return fail(e, text);
	std::vector<double> v, v2;
	expand_data_array(group1, v);
	expand_data_array(group2, v2);
	size_t n1 = 0, n2 = 0;
	bool inf = false;
	for (double a : v) n1 += a == a, inf = inf || isinf(a);
	for (double a : v2) n2 += a == a, inf = inf || isinf(a);
	if (n1 < 2) return fail(e, std::string(name) + " requires at least 2 observations in group 1");
	if (n2 < 2) return fail(e, std::string(name) + " requires at least 2 observations in group 2");
	if (inf) return fail(e, std::string(name) + " is not defined on infinite values");
	if (test == kPtMmd && n1 + n2 > (size_t)kPtMmdCap) return fail(e, "mmd: group too large (more than 1462 observations)");
	// (the NaN rows are dropped here: a group's size path goes by its rows, and MMD's cap is on the observations)
	v.erase(std::remove_if(v.begin(), v.end(), [](double a) { return a != a; }), v.end());
	std::vector<int32_t> sample(n1 + n2, 1);
	std::fill(sample.begin(), sample.begin() + (ptrdiff_t)n1, 0);
	for (double a : v2)
		if (a == a) v.push_back(a);
	const int64_t off[2] = {0, (int64_t)v.size()};
	double rec[kPtRecordLen];
	if (!perm_test_host(nullptr, 1, off[1], off, v.data(), sample.data(), o, rec, e)) return false;
	if (rec[7] != 0.0) return fail(e, std::string(name) + " failed on the GPU path");
	char *text = copy_text((std::string(method) + std::to_string(n_permutations) + " permutations)").c_str());
	if (!text) { set_error(e, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name"); return false; }
	out->statistic = rec[0];
	out->p_value = rec[1];
	out->df = test == kPtTTest ? rec[2] : NAN; // Welch's df of the observed split (the reference leaves it NaN)
	out->effect_size = test == kPtTTest ? NAN : rec[0];
	out->ci_lower = NAN;
	out->ci_upper = NAN;
	out->confidence_level = NAN;
	out->n = n1 + n2;
	out->n1 = n1;
	out->n2 = n2;
	out->alternative = (AnofoxAlternative)alternative;
	out->method = text;
	return true;
}

} // namespace

extern "C" {

size_t anofox_hip_perm_test_record_len(void) { return kPtRecordLen; }

void anofox_hip_perm_test_hooks(int64_t small_cap) { g_small_cap.store(small_cap > 0 ? small_cap : 0); }

bool anofox_hip_perm_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets, const double *d_v,
                                       const int32_t *d_sample, AnofoxHipPermTestBatchOptions options, double *d_records,
                                       AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_perm_test(n_groups, n_rows, d_row_offsets, d_v, d_sample, options, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_perm_test(ctx, n_groups, n_rows, d_row_offsets, d_v, d_sample, options, d_records, out_error);
}

bool anofox_hip_perm_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets, const double *v,
                                     const int32_t *sample, AnofoxHipPermTestBatchOptions options, double *records, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_perm_test(n_groups, n_rows, row_offsets, v, sample, options, records, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	return perm_test_host(ctx, n_groups, n_rows, row_offsets, v, sample, options, records, out_error);
}

bool anofox_energy_distance(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxEnergyDistanceOptions options, AnofoxTestResult *out_result,
                            AnofoxError *out_error) {
	return scalar_perm_test("Energy distance test", "Energy distance test (", group1, group2, kPtEnergy, kCorTwoSided, options.n_permutations,
	                        options.seed, options.has_seed, out_result, out_error);
}

bool anofox_mmd(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxMmdOptions options, AnofoxTestResult *out_result, AnofoxError *out_error) {
	return scalar_perm_test("MMD test", "MMD test (Gaussian kernel, ", group1, group2, kPtMmd, kCorTwoSided, options.n_permutations, options.seed,
	                        options.has_seed, out_result, out_error);
}

bool anofox_permutation_t_test(AnofoxDataArray group1, AnofoxDataArray group2, AnofoxAlternative alternative, size_t n_permutations, uint64_t seed,
                               bool has_seed, AnofoxTestResult *out_result, AnofoxError *out_error) {
	return scalar_perm_test("Permutation t-test", "Permutation t-test (", group1, group2, kPtTTest, (int32_t)alternative, n_permutations, seed,
	                        has_seed, out_result, out_error);
}

} // extern "C"
