// rank_tests.hip — grouped Mann-Whitney U, Wilcoxon signed-rank and Kruskal-Wallis tests (rank_tests.h): the kernels of both size
// paths and the entry points anofox_hip_rank_test_batch_{device,host}, anofox_hip_rank_test_record_len, anofox_hip_rank_test_hooks,
// anofox_mann_whitney_u / anofox_wilcoxon_signed_rank / anofox_kruskal_wallis / anofox_free_test_result.
//
// The contract and the method: rank_tests.h and DESIGN.md §1, "Rank-based location tests".
//   rank_test_small_kernel<CAP>: one wavefront per workgroup and group, grid-stride over the groups, the group's work arrays in
//     LDS, in the two instances of cor_small_kernel (rank_cor.hip): groups of at most kRtTierRows rows take 7 KiB, so a CU holds as
//     many wavefronts as its other limits admit; groups up to kRtSmallCap rows take 40 KiB, which keeps a wavefront on every SIMD.
//     A kernel passes over the groups of the other tier.
//   rank_test_large_kernel: a workgroup of 1024 threads per group above the cap, its work arrays in the context's workspace.  All
//     sixteen wavefronts sort; the first runs the other phases with the small path's code, so the midranks and their sums come out
//     bit for bit as on the small path.
//   Neither form of the entry reads the offsets on the host to size a launch; the large path is launched whenever the call has
//     more rows than the cap, and then takes kCorRowBytes of workspace per row of the call.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "rank_tests.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;
using namespace anofox::ranktest;

namespace {

// the caps of rank_cor.hip, for the same footprint: 40960 bytes / kCorRowBytes (28) = 1462 rows keep one wavefront on every SIMD
constexpr int kRtSmallCap = 40960 / kCorRowBytes;
static_assert(kRtSmallCap == 1462, "the cap's derivation");
constexpr int kRtTierRows = 256; // the first instance's groups: 256 x 28 = 7 KiB
constexpr int64_t kRtMaxWorkgroups = 1 << 16;
constexpr int kRtLargeThreads = 1024;
constexpr int kRtLargeWorkgroups = 1024;

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_rank_test_hooks

struct RankTestArgs {
	RankTestProblem P;
	const int64_t *off;
	int64_t n_groups;
	int64_t above, upto; // the kernel's groups: above < rows <= upto
	CorWork W;           // the large path: each n_rows long; a group's part starts at its first row
};

__device__ __forceinline__ void group_rows(const RankTestArgs &a, int64_t g, int64_t &lo, int64_t &hi) {
	lo = a.off[g] < 0 ? 0 : a.off[g];
	hi = a.off[g + 1] > a.P.n_rows ? a.P.n_rows : a.off[g + 1];
	if (hi < lo) hi = lo;
	if (lo > a.P.n_rows) lo = hi = a.P.n_rows;
}

template <int CAP>
__global__ __launch_bounds__(64) void rank_test_small_kernel(RankTestArgs a) {
	__shared__ double sx[CAP], sy[CAP], sk[CAP];
	__shared__ int32_t si[CAP];
	const CorWork W = {sx, sy, sk, si};
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		int64_t lo, hi;
		group_rows(a, g, lo, hi);
		const int64_t m = hi - lo;
		if (m <= a.above || m > a.upto || m > CAP) continue; // (m > CAP never: upto <= CAP)
		rt_group(a.P, g, lo, hi, W, true, threadIdx.x, 64);
		__syncthreads(); // the next group's rows overwrite these
	}
}

__global__ __launch_bounds__(kRtLargeThreads) void rank_test_large_kernel(RankTestArgs a) {
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		int64_t lo, hi;
		group_rows(a, g, lo, hi);
		if (hi - lo <= a.above) continue;
		const CorWork W = {a.W.x + lo, a.W.y + lo, a.W.key + lo, a.W.idx + lo};
		rt_group(a.P, g, lo, hi, W, threadIdx.x < 64, threadIdx.x, kRtLargeThreads);
		__syncthreads();
	}
}

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

template <class K>
bool launch(K kernel, const char *name, const RankTestArgs &a, int64_t blocks, int threads, hipStream_t st, AnofoxError *e) {
	hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(threads), 0, st, a);
	return !hip_fail(hipGetLastError(), name, e);
}

// the tests of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_rank_test(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const double *d_v, const double *d_y,
                      const int32_t *d_sample, const AnofoxHipRankTestBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	RankTestArgs a;
	memset(&a, 0, sizeof a);
	a.P.v = d_v;
	a.P.y = d_y;
	a.P.sample = d_sample;
	a.P.n_rows = n_rows;
	a.P.test = o.test;
	a.P.alternative = o.alternative;
	a.P.correction = o.continuity_correction != 0;
	a.P.mu = o.mu;
	a.P.records = d_rec;
	a.off = d_off;
	a.n_groups = n_groups;
	hipStream_t st = ctx->stream;
	const int64_t blocks = n_groups < kRtMaxWorkgroups ? n_groups : kRtMaxWorkgroups;
	const int64_t hook = g_small_cap.load(), cap = hook > 0 && hook < kRtSmallCap ? hook : kRtSmallCap;
	const int64_t tier = cap < kRtTierRows ? cap : kRtTierRows;
	a.above = -1;
	a.upto = tier;
	if (!launch(rank_test_small_kernel<kRtTierRows>, "rank_test_small_kernel", a, blocks, 64, st, e)) return false;
	if (n_rows <= tier) return true; // no group has more rows than the call
	if (cap > tier) {
		a.above = tier;
		a.upto = cap;
		if (!launch(rank_test_small_kernel<kRtSmallCap>, "rank_test_small_kernel", a, blocks, 64, st, e)) return false;
	}
	if (n_rows <= cap) return true;
	// the large path: the work arrays, each as long as the call
	const size_t N = (size_t)n_rows;
	const size_t col = align_up(N * sizeof(double), 256), total = 3 * col + align_up(N * sizeof(int32_t), 256);
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, total, "rank test scratch", e)) return false;
	char *ws = (char *)ctx->ws;
	a.W.x = (double *)ws;
	a.W.y = (double *)(ws + col);
	a.W.key = (double *)(ws + 2 * col);
	a.W.idx = (int32_t *)(ws + 3 * col);
	a.above = cap;
	a.upto = INT64_MAX;
	const int64_t large_blocks = n_groups < kRtLargeWorkgroups ? n_groups : kRtLargeWorkgroups;
	return launch(rank_test_large_kernel, "rank_test_large_kernel", a, large_blocks, kRtLargeThreads, st, e);
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

char *copy_text(const char *s) {
	char *p = (char *)malloc(strlen(s) + 1);
	if (p) strcpy(p, s);
	return p;
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
