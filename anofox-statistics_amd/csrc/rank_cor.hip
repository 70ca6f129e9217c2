// rank_cor.hip — grouped Pearson, Spearman and Kendall correlation with their tests (rank_cor.h): the kernels of both size paths
// and the entry points anofox_hip_cor_batch_{device,host}, anofox_hip_cor_record_len, anofox_hip_cor_test_hooks,
// anofox_pearson_cor / anofox_spearman_cor / anofox_kendall_cor / anofox_free_correlation_result.
//
// The contract and the method: rank_cor.h and DESIGN.md §1, "Rank and product-moment correlation".
//   cor_small_kernel<CAP>: one wavefront per workgroup and group, grid-stride over the groups, the group's work arrays in LDS.  Two
//     instances share the groups by their row count: up to kCorTierRows rows (7 KiB of LDS, so a CU holds as many wavefronts as
//     its other limits admit) and up to kCorSmallCap.  A kernel passes over the groups of the other tier.  Pearson stages nothing
//     and runs every group, whatever its size, on the first instance: it streams the rows twice from memory.
//   cor_large_kernel: a workgroup of 1024 threads per group above the cap, its work arrays in the context's workspace.  All
//     sixteen wavefronts sort; the first runs the other phases with the small path's code, so a group's midranks and their sums
//     come out bit for bit as on the small path.  A Kendall group is entered into a list instead of being counted.
//   cor_pairs_kernel: the listed groups' pairs by (i block, j block) tiles of 256 x 256 rows, the j block in LDS, grid-stride over
//     the tiles; a wavefront adds its count into the group's int64 with one atomic add (a vector atomic; integer, so exact and
//     independent of the order).  cor_finish_kernel: a thread per listed group writes the record.
//   Neither form of the entry reads the offsets on the host to size a launch; the large path is launched whenever the call has
//     more rows than the cap, and then takes kCorRowBytes of workspace per row of the call.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "common.h"
#include "rank_cor.h"
#include "host_math.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::cor;

namespace {

// The rows of a group that the small path holds.  A workgroup of cor_small_kernel is one wavefront, and a CU has four SIMDs: with
// 160 KiB of LDS per CU (a single workgroup may take all of it), 160 / 4 = 40 KiB per workgroup keeps one wavefront on every
// SIMD.  40960 bytes / kCorRowBytes (28) = 1462 rows.  A larger cap would idle SIMDs; a smaller one sends groups to the large
// path, which costs three launches and global-memory sorts.
constexpr int kCorSmallCap = 40960 / kCorRowBytes;
static_assert(kCorSmallCap == 1462, "the cap's derivation");
constexpr int kCorTierRows = 256; // the first instance's groups: 256 x 28 = 7 KiB
constexpr int64_t kCorMaxWorkgroups = 1 << 16;
constexpr int kCorLargeThreads = 1024;
constexpr int kCorLargeWorkgroups = 1024;
constexpr int kCorPairWorkgroups = 2048; // 256 CUs x 8 workgroups of 256 threads

std::atomic<int64_t> g_small_cap{0}; // anofox_hip_cor_test_hooks

struct CorArgs {
	CorProblem P;
	const int64_t *off;
	int64_t n_groups;
	int64_t above, upto; // the kernel's groups: above < rows <= upto
	// the large path
	CorWork W; // each n_rows long; a group's part starts at its first row
	CorLarge *list;
	unsigned long long *count;
	int64_t slots;
};

__device__ __forceinline__ void group_rows(const CorArgs &a, int64_t g, int64_t &lo, int64_t &hi) {
	lo = a.off[g] < 0 ? 0 : a.off[g];
	hi = a.off[g + 1] > a.P.n_rows ? a.P.n_rows : a.off[g + 1];
	if (hi < lo) hi = lo;
	if (lo > a.P.n_rows) lo = hi = a.P.n_rows;
}

template <int CAP>
__global__ __launch_bounds__(64) void cor_small_kernel(CorArgs a) {
	__shared__ double sx[CAP], sy[CAP], sk[CAP];
	__shared__ int32_t si[CAP];
	const CorWork W = {sx, sy, sk, si};
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		int64_t lo, hi;
		group_rows(a, g, lo, hi);
		const int64_t m = hi - lo;
		if (m <= a.above || m > a.upto) continue;
		if (a.P.method != kCorPearson && m > CAP) continue; // (never: upto <= CAP for the staged methods)
		rc_group(a.P, g, lo, hi, W, true, threadIdx.x, 64, nullptr);
		__syncthreads(); // the next group's rows overwrite these
	}
}

__global__ __launch_bounds__(kCorLargeThreads) void cor_large_kernel(CorArgs a) {
	__shared__ long long s_slot;
	for (int64_t g = blockIdx.x; g < a.n_groups; g += gridDim.x) {
		int64_t lo, hi;
		group_rows(a, g, lo, hi);
		if (hi - lo <= a.above) continue;
		const CorWork W = {a.W.x + lo, a.W.y + lo, a.W.key + lo, a.W.idx + lo};
		CorLarge *large = nullptr;
		if (a.P.method == kCorKendall) {
			if (threadIdx.x == 0) {
				const unsigned long long k = atomicAdd(a.count, 1ull);
				s_slot = k < (unsigned long long)a.slots ? (long long)k : -1; // (a full list: the wavefront counts the pairs itself)
				if (s_slot >= 0) {
					a.list[s_slot].group = g;
					a.list[s_slot].n = 0; // until the group is entered
				}
			}
			__syncthreads();
			if (s_slot >= 0) large = a.list + s_slot;
		}
		rc_group(a.P, g, lo, hi, W, threadIdx.x < 64, threadIdx.x, kCorLargeThreads, large);
		__syncthreads();
	}
}

__global__ __launch_bounds__(kCorPairTile) void cor_pairs_kernel(CorArgs a) {
	__shared__ double sx[kCorPairTile], sy[kCorPairTile];
	const int64_t listed = (int64_t)(*a.count < (unsigned long long)a.slots ? *a.count : (unsigned long long)a.slots);
	for (int64_t k = 0; k < listed; ++k) {
		const int64_t n = a.list[k].n, lo = a.list[k].lo;
		if (n < 3) continue;
		const double *x = a.W.x + lo, *y = a.W.y + lo;
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
		if ((threadIdx.x & 63u) == 0 && total != 0) atomicAdd((unsigned long long *)&a.list[k].s, (unsigned long long)total);
	}
}

__global__ __launch_bounds__(64) void cor_finish_kernel(CorArgs a) {
	const int64_t listed = (int64_t)(*a.count < (unsigned long long)a.slots ? *a.count : (unsigned long long)a.slots);
	for (int64_t k = (int64_t)blockIdx.x * 64 + threadIdx.x; k < listed; k += (int64_t)gridDim.x * 64) {
		const CorLarge &L = a.list[k];
		if (L.n >= 3) rc_kendall_record(a.P, L.s, L.n, L.tx, L.ty, a.P.records + L.group * kCorRecordLen);
	}
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

template <class K>
bool launch(K kernel, const char *name, const CorArgs &a, int64_t blocks, int threads, hipStream_t st, AnofoxError *e) {
	hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(threads), 0, st, a);
	return !hip_fail(hipGetLastError(), name, e);
}

// the correlations of n_groups groups of device-resident rows, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_cor(AnofoxHipContext *ctx, int64_t n_groups, int64_t n_rows, const int64_t *d_off, const double *d_x, const double *d_y,
                const AnofoxHipCorBatchOptions &o, double *d_rec, AnofoxError *e) {
	if (n_groups == 0) return true;
	CorArgs a;
	memset(&a, 0, sizeof a);
	a.P.x = d_x;
	a.P.y = d_y;
	a.P.n_rows = n_rows;
	a.P.method = o.method;
	a.P.alternative = o.alternative;
	a.P.tau_type = o.tau_type;
	a.P.zq = o.confidence_level == o.confidence_level ? hostmath::normal_quantile(0.5 * (1.0 + o.confidence_level)) : NAN;
	a.P.records = d_rec;
	a.off = d_off;
	a.n_groups = n_groups;
	hipStream_t st = ctx->stream;
	const int64_t blocks = n_groups < kCorMaxWorkgroups ? n_groups : kCorMaxWorkgroups;
	if (o.method == kCorPearson) {
		a.above = -1;
		a.upto = INT64_MAX;
		return launch(cor_small_kernel<kCorTierRows>, "cor_small_kernel", a, blocks, 64, st, e);
	}
	const int64_t hook = g_small_cap.load(), cap = hook > 0 && hook < kCorSmallCap ? hook : kCorSmallCap;
	const int64_t tier = cap < kCorTierRows ? cap : kCorTierRows;
	a.above = -1;
	a.upto = tier;
	if (!launch(cor_small_kernel<kCorTierRows>, "cor_small_kernel", a, blocks, 64, st, e)) return false;
	if (n_rows <= tier) return true; // no group has more rows than the call
	if (cap > tier) {
		a.above = tier;
		a.upto = cap;
		if (!launch(cor_small_kernel<kCorSmallCap>, "cor_small_kernel", a, blocks, 64, st, e)) return false;
	}
	if (n_rows <= cap) return true;
	// the large path: a counter, the list (disjoint groups above the cap: n_rows / (cap + 1) at most) and the work arrays
	const size_t N = (size_t)n_rows;
	a.slots = n_rows / (cap + 1) + 1;
	const size_t list_at = 256, x_at = align_up(list_at + (size_t)a.slots * sizeof(CorLarge), 256);
	const size_t col = align_up(N * sizeof(double), 256), total = x_at + 3 * col + align_up(N * sizeof(int32_t), 256);
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, total, "correlation scratch", e)) return false;
	char *ws = (char *)ctx->ws;
	a.count = (unsigned long long *)ws;
	a.list = (CorLarge *)(ws + list_at);
	a.W.x = (double *)(ws + x_at);
	a.W.y = (double *)(ws + x_at + col);
	a.W.key = (double *)(ws + x_at + 2 * col);
	a.W.idx = (int32_t *)(ws + x_at + 3 * col);
	a.above = cap;
	a.upto = INT64_MAX;
	if (hip_fail(hipMemsetAsync(a.count, 0, 256, st), "hipMemsetAsync", e)) return false;
	const int64_t large_blocks = n_groups < kCorLargeWorkgroups ? n_groups : kCorLargeWorkgroups;
	if (!launch(cor_large_kernel, "cor_large_kernel", a, large_blocks, kCorLargeThreads, st, e)) return false;
	if (o.method != kCorKendall) return true;
	return launch(cor_pairs_kernel, "cor_pairs_kernel", a, kCorPairWorkgroups, kCorPairTile, st, e) &&
	       launch(cor_finish_kernel, "cor_finish_kernel", a, (a.slots + 63) / 64, 64, st, e);
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

char *copy_text(const char *s) {
	char *p = (char *)malloc(strlen(s) + 1);
	if (p) strcpy(p, s);
	return p;
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
