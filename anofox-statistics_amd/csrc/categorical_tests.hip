// categorical_tests.hip — grouped chi-square, G, Fisher exact and McNemar tests (categorical_tests.h): the fifth family on the
// size-tiered launch driver of rank_launch.h and the entry points anofox_hip_categorical_test_batch_{device,host},
// anofox_hip_categorical_test_record_len, anofox_hip_categorical_test_hooks, anofox_chisq_test / anofox_g_test / anofox_cramers_v /
// anofox_contingency_coef / anofox_fisher_exact / anofox_mcnemar_test / anofox_phi_coefficient / anofox_free_chisq_result.
//
// The contract and the method: categorical_tests.h and DESIGN.md §1, "Categorical tests".
//   rank_small_kernel<CAP, CategoricalFamily>, rank_large_kernel<CategoricalFamily>: the two size paths (rank_launch.h).  Fisher's
//     and McNemar's tests stage nothing (staged() is false: every group runs on the first small instance); the chi-square and the
//     G-test stage their rows, and nothing follows the large kernel.
//   The scalars that take a table or four cells touch no device: categorical_scalars.cpp runs the header's plain C++ build.
#include <math.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "categorical_scalars.h"
#include "categorical_tests.h"
#include "common.h"
#include "rank_launch.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;
using namespace anofox::cattest;
using namespace anofox::rank;

namespace {

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_categorical_test_hooks

struct CategoricalFamily {
	static constexpr const char *kSmallKernel = "rank_small_kernel<CategoricalFamily>", *kLargeKernel = "rank_large_kernel<CategoricalFamily>",
	                            *kScratch = "categorical test scratch";
	CategoricalProblem P;

	__host__ __device__ bool staged() const { return ct_staged(P.test); }

	__device__ __forceinline__ void small_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		ct_group(P, g, lo, hi, W, true, threadIdx.x, 64);
	}

	__device__ __forceinline__ void large_group(int64_t g, int64_t lo, int64_t hi, const CorWork &W) const {
		ct_group(P, g, lo, hi, W, threadIdx.x < 64, threadIdx.x, kRankLargeThreads);
	}

	// nothing in the workspace but the work arrays, nothing around the large kernel
	size_t prefix_bytes(int64_t) const { return 0; }
	bool begin_large(char *, int64_t, hipStream_t, AnofoxError *) { return true; }
	bool end_large(const RankCall &, hipStream_t, AnofoxError *) const { return true; }
};

bool check_categorical_test(int64_t n_groups, int64_t n_rows, const void *off, const void *a, const void *b,
                            const AnofoxHipCategoricalTestBatchOptions &o, const void *records, AnofoxError *e) {
	if (n_groups < 0 || n_rows < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "categorical test: negative n_groups or n_rows"); return false; }
	if (const char *text = ct_options_text(o.test, o.alternative, o.confidence_level)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, text);
		return false;
	}
	if (n_groups == 0) return true;
	if (!off || !a || !b || !records) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "categorical test: row_offsets, a, b or records is NULL"); return false; }
	return true;
}

// the tests of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_categorical_test(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const int32_t *d_a, const int32_t *d_b,
                             const AnofoxHipCategoricalTestBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	CategoricalFamily f;
	memset(&f, 0, sizeof f);
	f.P.a = d_a;
	f.P.b = d_b;
	f.P.n_rows = n_rows;
	f.P.test = o.test;
	f.P.alternative = o.alternative;
	f.P.correction = o.correction != 0;
	f.P.exact = o.exact != 0;
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
bool categorical_test_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *off, const int32_t *a, const int32_t *b,
                           const AnofoxHipCategoricalTestBatchOptions &o, double *records, AnofoxError *e) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_groups;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_off;
	int32_t *d_a, *d_b;
	double *d_rec;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_off = s.put(off, G + 1);
		    d_a = s.put(a, (size_t)n_rows);
		    d_b = s.put(b, (size_t)n_rows);
		    d_rec = s.take<double>(G * kCtRecordLen);
	    }))
		return false;
	if (!launch_categorical_test(ctx, n_groups, n_rows, d_off, d_a, d_b, o, d_rec, e)) return false;
	if (!d2h(records, d_rec, G * kCtRecordLen * sizeof(double), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

bool fail(AnofoxError *e, AnofoxErrorCode code, const std::string &text) {
	set_error(e, code, text);
	return false;
}

// the reference's cast of a label, `value as usize`: toward zero, negative values to 0; labels beyond int32 meet at its end
int32_t cast_label(double v) {
	if (!(v >= 1.0)) return 0;
	return v >= 2147483647.0 ? INT32_MAX : (int32_t)v;
}

// a chi-square layout result from a record whose status is 0
bool chisq_result(const double *rec, const char *method, AnofoxChiSquareResult *out, AnofoxError *e) {
	char *text = copy_text(method);
	if (!text) return fail(e, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name");
	out->statistic = rec[0];
	out->p_value = rec[1];
	out->df = rec[2] == rec[2] ? (size_t)rec[2] : 0;
	out->method = text;
	return true;
}

bool table_arguments(const size_t *table, const size_t *row_lengths, size_t n_rows, const void *out, AnofoxError *e) {
	reset_error(e);
	if (!out) return fail(e, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL");
	if (!table || !row_lengths || n_rows == 0) return fail(e, ANOFOX_ERROR_INVALID_INPUT, "Invalid table data");
	return true;
}

// one association measure (field `at` of the uncorrected chi-square record) of a table
bool table_measure(const size_t *table, const size_t *row_lengths, size_t n_rows, int at, double *out, AnofoxError *e) {
	if (!table_arguments(table, row_lengths, n_rows, out, e)) return false;
	double rec[kCtRecordLen];
	ct_scalar_table(kCtChiSquare, 0, table, row_lengths, n_rows, rec);
	if (rec[11] != 0.0) return fail(e, ANOFOX_ERROR_INVALID_INPUT, "Contingency table must have at least 2 occupied rows and 2 occupied columns");
	*out = rec[at];
	return true;
}

} // namespace

extern "C" {

size_t anofox_hip_categorical_test_record_len(void) { return kCtRecordLen; }

void anofox_hip_categorical_test_hooks(int64_t small_cap) { g_small_cap.store(small_cap > 0 ? small_cap : 0); }

bool anofox_hip_categorical_test_batch_device(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_row_offsets,
                                              const int32_t *d_a, const int32_t *d_b, AnofoxHipCategoricalTestBatchOptions options,
                                              double *d_records, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_categorical_test(n_groups, n_rows, d_row_offsets, d_a, d_b, options, d_records, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_categorical_test(ctx, n_groups, n_rows, d_row_offsets, d_a, d_b, options, d_records, out_error);
}

bool anofox_hip_categorical_test_batch_host(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *row_offsets,
                                            const int32_t *a, const int32_t *b, AnofoxHipCategoricalTestBatchOptions options, double *records,
                                            AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_categorical_test(n_groups, n_rows, row_offsets, a, b, options, records, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	return categorical_test_host(ctx, n_groups, n_rows, row_offsets, a, b, options, records, out_error);
}

bool anofox_chisq_test(AnofoxDataArray row_var, AnofoxDataArray col_var, AnofoxChiSquareOptions options, AnofoxChiSquareResult *out_result,
                       AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_result) return fail(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL");
	memset(out_result, 0, sizeof *out_result); // a failed call leaves nothing to free
	std::vector<double> r, c;
	expand_data_array(row_var, r);
	expand_data_array(col_var, c);
	const size_t len = r.size() < c.size() ? r.size() : c.size();
	std::vector<int32_t> a, b;
	for (size_t i = 0; i < len; ++i) {
		if (r[i] != r[i] || c[i] != c[i]) continue;
		a.push_back(cast_label(r[i]));
		b.push_back(cast_label(c[i]));
	}
	if (a.empty()) return fail(out_error, ANOFOX_ERROR_INSUFFICIENT_DATA, "No valid data pairs");
	const int64_t off[2] = {0, (int64_t)a.size()};
	const AnofoxHipCategoricalTestBatchOptions o = {kCtChiSquare, ANOFOX_ALTERNATIVE_TWO_SIDED, options.correction ? 1 : 0, 0, NAN};
	double rec[kCtRecordLen];
	if (!categorical_test_host(nullptr, 1, off[1], off, a.data(), b.data(), o, rec, out_error)) return false;
	if (rec[11] != 0.0) return fail(out_error, ANOFOX_ERROR_INVALID_INPUT, "Contingency table must have at least 2 rows and 2 columns");
	return chisq_result(rec, "Pearson's Chi-squared test", out_result, out_error);
}

void anofox_free_chisq_result(AnofoxChiSquareResult *result) {
	if (!result) return;
	free(result->method);
	result->method = nullptr;
}

bool anofox_g_test(const size_t *table, const size_t *row_lengths, size_t n_rows, AnofoxChiSquareResult *out_result, AnofoxError *out_error) {
	reset_error(out_error);
	if (out_result) memset(out_result, 0, sizeof *out_result);
	if (!table_arguments(table, row_lengths, n_rows, out_result, out_error)) return false;
	double rec[kCtRecordLen];
	ct_scalar_table(kCtG, 0, table, row_lengths, n_rows, rec);
	if (rec[11] != 0.0) return fail(out_error, ANOFOX_ERROR_INVALID_INPUT, "Contingency table must have at least 2 occupied rows and 2 occupied columns");
	return chisq_result(rec, "G-test (log-likelihood ratio)", out_result, out_error);
}

bool anofox_cramers_v(const size_t *table, const size_t *row_lengths, size_t n_rows, double *out_result, AnofoxError *out_error) {
	return table_measure(table, row_lengths, n_rows, 3, out_result, out_error);
}

bool anofox_contingency_coef(const size_t *table, const size_t *row_lengths, size_t n_rows, double *out_result, AnofoxError *out_error) {
	return table_measure(table, row_lengths, n_rows, 9, out_result, out_error);
}

bool anofox_phi_coefficient(size_t a, size_t b, size_t c, size_t d, double *out_result, AnofoxError *out_error) {
	const size_t table[4] = {a, b, c, d}, lengths[2] = {2, 2};
	return table_measure(table, lengths, 2, 10, out_result, out_error);
}

bool anofox_fisher_exact(size_t a, size_t b, size_t c, size_t d, AnofoxFisherExactOptions options, AnofoxTestResult *out_result,
                         AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_result) return fail(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL");
	memset(out_result, 0, sizeof *out_result);
	if (const char *text = ct_options_text(kCtFisher, (int)options.alternative, options.confidence_level))
		return fail(out_error, ANOFOX_ERROR_INVALID_INPUT, text);
	double rec[kCtRecordLen];
	ct_scalar_cells(kCtFisher, (int)options.alternative, 0, 0, options.confidence_level, a, b, c, d, rec);
	if (rec[11] != 0.0) return fail(out_error, ANOFOX_ERROR_INSUFFICIENT_DATA, "Fisher's exact test requires at least one observation");
	char *text = copy_text("Fisher's exact test");
	if (!text) return fail(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the method name");
	out_result->statistic = rec[0];
	out_result->p_value = rec[1];
	out_result->df = NAN;
	out_result->effect_size = rec[3];
	out_result->ci_lower = rec[4];
	out_result->ci_upper = rec[5];
	out_result->confidence_level = options.confidence_level;
	out_result->n = a + b + c + d;
	out_result->n1 = 0; // the reference's counts
	out_result->n2 = 0;
	out_result->alternative = options.alternative;
	out_result->method = text;
	return true;
}

bool anofox_mcnemar_test(size_t a, size_t b, size_t c, size_t d, bool correction, bool exact, AnofoxChiSquareResult *out_result,
                         AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_result) return fail(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL");
	memset(out_result, 0, sizeof *out_result);
	double rec[kCtRecordLen];
	ct_scalar_cells(kCtMcNemar, 0, correction, exact, NAN, a, b, c, d, rec);
	if (rec[11] != 0.0) return fail(out_error, ANOFOX_ERROR_INSUFFICIENT_DATA, "McNemar's test requires at least one observation");
	return chisq_result(rec, exact ? "McNemar's exact test" : correction ? "McNemar's Chi-squared test with continuity correction" : "McNemar's Chi-squared test",
	                    out_result, out_error);
}

} // extern "C"
