// glmm.hip — grouped Gaussian linear mixed models with one random intercept (lmm_profile.h): the three kernels and the entry points
// anofox_hip_glmm_fit_batch_{device,host}, anofox_hip_glmm_fit_predict_batch_{device,host}, anofox_hip_glmm_record_len /
// _inference_len / _pred_len / _test_hooks, anofox_glmm_fit / anofox_free_glmm_result.
//
// The contract and the method: lmm_profile.h and DESIGN.md §1, "Linear mixed models".
//   lm_stats_kernel: 64 lanes per workgroup = one wavefront per chunk of 64 levels of a panel (grid-stride over the chunk
//     numbers).  Writes the level records {n, ybar, abar[k]}, a validity byte per row and the chunk's partial of [W w; w' omega]
//     into the context's workspace.  It passes k + 2 + E times over a chunk's rows; only the first pass is HBM traffic while the
//     chunk fits the caches (lmm_profile.h; docs/MEASUREMENTS.md, "glmm", has the rates).
//   lm_search_kernel<W, KEEP> (KEEP: with the writes a fit-predict needs; a fit runs the kernel compiled without them):
//     one workgroup of W wavefronts per panel; a launch per W in {1, 4, 16}, and a workgroup whose panel
//     belongs to another W leaves at once, so that the wavefront count of a panel depends on its own level count alone and
//     neither form of the entry reads offsets back to size a launch (the host form, which has them, skips the launches that no
//     panel needs).  LDS: lm_work_doubles(k, W) * 8 bytes, 32.6 KB at k = 33, W = 16.
//   lm_predict_kernel<KC> (fit-predict only): one wavefront per tile of 256 rows of a panel, the tiles numbered without a prefix
//     sum (panel g owns the numbers from (its first row - the call's first row) / 256 + g on).  The wavefront stages the panel's
//     {theta, s2, beta, L^-1} from the call's scratch in LDS (4.8 KB at k = 33), then every lane scores its rows: the columns are
//     read once, lanes over rows, and the level of a row is found by bisection of the level offsets between the levels of the
//     tile's first and last row.  KC in {4, 9, 17, 33} is the compiled width (the lane's L^-1 c lives in KC registers).
// No atomics: the partials of a panel are added in a fixed order, so repeated calls give identical bytes.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "lmm_profile.h"
#include "host_math.h"

using namespace anofox;

#include "host_stage.h"

using namespace anofox::host;
using namespace anofox::lmm;

namespace {

std::atomic<int> g_stats_only{0}, g_wave_mask{0}; // anofox_hip_glmm_test_hooks

struct LmArgs {
	LmProblem P; // P.x is set in the kernel
	const double *x[kLmMaxP];
	// fit-predict
	double *pred; // [n_rows x 5]
	int interval;
	double z;
	int64_t n_tiles; // n_rows / kLmPredTile + n_panels
};

constexpr int64_t kLmPredTile = 256;

__device__ __forceinline__ LmProblem lm_problem(const LmArgs &a, const double **lds_x) {
#pragma unroll
	for (int j = 0; j < kLmMaxP; ++j)
		if (threadIdx.x == 0) lds_x[j] = a.x[j];
	__syncthreads();
	LmProblem P = a.P;
	P.x = lds_x;
	return P;
}

__global__ __launch_bounds__(64) void lm_stats_kernel(LmArgs a) {
	// the column pointers in LDS: indexing the kernel arguments by a run-time column would make a private copy of them
	__shared__ const double *lm_x[kLmMaxP];
	const LmProblem P = lm_problem(a, lm_x);
	for (int64_t v = blockIdx.x; v < P.n_numbers; v += gridDim.x) {
		lm_chunk_stats(P, v);
		__syncthreads();
	}
}

template <int W, bool KEEP>
__global__ __launch_bounds__(64 * W) void lm_search_kernel(LmArgs a) {
	extern __shared__ double lm_lds[];
	__shared__ const double *lm_x[kLmMaxP];
	const LmProblem P = lm_problem(a, lm_x);
	for (int64_t g = blockIdx.x; g < P.n_panels; g += gridDim.x) {
		const int64_t l0 = lm_clip(P.plo[g], P.n_levels), l1 = lm_clip(P.plo[g + 1], P.n_levels);
		if (lm_wave_count(l1 > l0 ? l1 - l0 : 0) != W) continue;
		lm_fit_panel<KEEP>(P, g, W, lm_lds);
	}
}

// the first row of panel g (g == n_panels: the end of the last), clipped into the arrays
__device__ __forceinline__ int64_t lm_panel_row(const LmProblem &P, int64_t g) {
	return lm_clip(P.lro[lm_clip(P.plo[g], P.n_levels)], P.n_rows);
}
__device__ __forceinline__ int64_t lm_tile_base(const LmProblem &P, int64_t g) {
	const int64_t d = lm_panel_row(P, g) - lm_panel_row(P, 0);
	return (d > 0 ? d : 0) / kLmPredTile + g;
}

template <int KC>
__global__ __launch_bounds__(64) void lm_predict_kernel(LmArgs a) {
	__shared__ const double *lm_x[kLmMaxP];
	__shared__ double s_keep[2 + KC];
	__shared__ double s_linv[KC * (KC + 1) / 2];
	const LmProblem P = lm_problem(a, lm_x);
	const int k = lm_k(P.p, P.fit_intercept), lane = (int)threadIdx.x, tri = k * (k + 1) / 2;
	for (int64_t v = blockIdx.x; v < a.n_tiles; v += gridDim.x) {
		// the panel of tile number v: the last one whose base is not above v (every lane makes the same search)
		int64_t ga = 0, gb = P.n_panels - 1;
		while (ga < gb) {
			const int64_t mid = ga + (gb - ga + 1) / 2;
			if (lm_tile_base(P, mid) <= v) ga = mid;
			else gb = mid - 1;
		}
		const int64_t g = ga, j = v - lm_tile_base(P, g);
		const int64_t l0 = lm_clip(P.plo[g], P.n_levels);
		int64_t l1 = lm_clip(P.plo[g + 1], P.n_levels);
		if (l1 < l0) l1 = l0;
		const int64_t p0 = lm_clip(P.lro[l0], P.n_rows);
		int64_t p1 = lm_clip(P.lro[l1], P.n_rows);
		if (p1 < p0) p1 = p0;
		if (j < 0 || l1 == l0) continue;
		const int64_t r0 = p0 + j * kLmPredTile;
		if (r0 >= p1) continue;
		const int64_t r1 = r0 + kLmPredTile < p1 ? r0 + kLmPredTile : p1;
		if (!(P.keep_ok[g] == 1.0)) { // a failed panel (or one whose search was masked out)
			for (int64_t i = r0 + lane; i < r1; i += 64)
				for (int q = 0; q < kLmPredLen; ++q) a.pred[i * kLmPredLen + q] = NAN;
			continue;
		}
		const double *kp = P.keep + g * lm_keep_len(k);
		__syncthreads(); // the tile before
		for (int c = lane; c < 2 + k; c += 64) s_keep[c] = kp[c];
		for (int e = lane; e < KC * (KC + 1) / 2; e += 64) s_linv[e] = e < tri ? kp[2 + k + e] : 0.0;
		__syncthreads();
		// the level of a row: the last level of [l0, l1) that starts at or before it (levels without rows are passed over)
		auto level_of = [&](int64_t i, int64_t lo, int64_t hi) {
			while (lo < hi) {
				const int64_t mid = lo + (hi - lo + 1) / 2;
				if (lm_clip(P.lro[mid], P.n_rows) <= i) lo = mid;
				else hi = mid - 1;
			}
			return lo;
		};
		const int64_t la = level_of(r0, l0, l1 - 1), lb = level_of(r1 - 1, la, l1 - 1);
		for (int64_t i = r0 + lane; i < r1; i += 64) {
			const int64_t l = level_of(i, la, lb);
			double out[kLmPredLen];
			// L^-1 is read from LDS for every row: an offset the compiler cannot see through keeps it from moving the KC (KC + 1)
			// / 2 loads, which do not depend on the row, out of this loop into registers (1364 bytes of scratch per lane at KC = 33).
			// To re-check: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-fast-math --cuda-device-only
			// -Rpass-analysis=kernel-resource-usage -c glmm.hip; lm_predict_kernel<4 | 9 | 17 | 33> must report ScratchSize 0
			// (50 / 71 / 101 / 138 VGPRs with ROCm 7's clang).  If a compiler sees through the offset the kernel stays correct and
			// only spills.
			int at = 0;
			asm volatile("" : "+v"(at));
			lm_predict_row<KC>(P, k, i, P.level_pred + l * lm_level_pred_len(k), s_keep[1], s_keep + 2, s_linv + at, a.interval, a.z, out);
			for (int q = 0; q < kLmPredLen; ++q) a.pred[i * kLmPredLen + q] = out[q];
		}
	}
}

bool glmm_options_invalid(const AnofoxHipGlmmOptions &o) {
	if (!(o.tolerance > 0.0) || !isfinite(o.tolerance)) return true;
	if (o.max_iterations == 0) return true;
	if (o.compute_inference && !(o.confidence_level > 0.0 && o.confidence_level < 1.0)) return true;
	return false;
}

const char *family_name(int family) {
	switch (family) {
	case ANOFOX_GLMM_POISSON: return "poisson";
	case ANOFOX_GLMM_BINOMIAL: return "binomial";
	case ANOFOX_GLMM_NEGBINOMIAL: return "negbinomial";
	case ANOFOX_GLMM_GAMMA: return "gamma";
	case ANOFOX_GLMM_TWEEDIE: return "tweedie";
	default: return "this";
	}
}

bool check_glmm(int64_t n_panels, int64_t n_levels, size_t p, int64_t n_rows, const void *plo, const void *lro, const void *y,
                const double *const *x_cols, int family, const void *rec, const void *ranef, AnofoxError *e) {
	if (n_levels < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "negative n_levels"); return false; }
	if (!check_batch_args(n_panels, p, n_rows, plo, y, x_cols, rec, kLmMaxP, "glmm: n_features > 32 is not built",
	                      "panel_level_offsets, y or an output is NULL", false, e))
		return false;
	if (n_panels > 0 && (!lro || !ranef)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "level_row_offsets or ranef is NULL"); return false; }
	if (family != ANOFOX_GLMM_GAUSSIAN) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, std::string("glmm: the ") + family_name(family) + " family is not built");
		return false;
	}
	return true;
}

// which wavefront counts the call's panels need; nullptr offsets (the device form): all of them
struct Classes {
	bool need[3] = {true, true, true};
};

// the fit of n_panels panels on device-resident inputs, enqueued on the context's stream (ctx->mu held by the caller)
bool launch_glmm(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t p, int64_t n_rows, const int64_t *d_plo,
                 const int64_t *d_lro, const double *d_y, const double *const *x_cols, const AnofoxHipGlmmOptions &o, double *d_rec,
                 double *d_inf, double *d_ranef, int64_t *d_level_n, const Classes &cls, AnofoxError *e,
                 const AnofoxHipGlmmPredictOptions *predict = nullptr, double *d_pred = nullptr) {
	if (n_panels == 0) return true;
	LmArgs a;
	memset(&a, 0, sizeof a);
	LmProblem &P = a.P;
	P.fit_intercept = o.fit_intercept ? 1 : 0;
	const int k = lm_k((int)p, P.fit_intercept), E = lm_entries(k);
	P.n_numbers = n_levels / kLmChunkLevels + n_panels;
	const size_t lev = align_up((size_t)(n_levels > 0 ? n_levels : 1) * (k + 2) * sizeof(double), 256);
	const size_t parts = align_up((size_t)P.n_numbers * E * sizeof(double), 256);
	const size_t valid = (size_t)(n_rows > 0 ? n_rows : 1);
	// a fit-predict keeps more in the same scratch, behind what the fit uses: the fit's own bytes and their places do not change
	const size_t valid_al = align_up(valid, 256);
	const size_t keep = predict ? align_up((size_t)n_panels * lm_keep_len(k) * sizeof(double), 256) : 0;
	const size_t keep_ok = predict ? align_up((size_t)n_panels * sizeof(double), 256) : 0;
	const size_t level_pred = predict ? (size_t)(n_levels > 0 ? n_levels : 1) * lm_level_pred_len(k) * sizeof(double) : 0;
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, predict ? lev + parts + valid_al + keep + keep_ok + level_pred : lev + parts + valid,
	                   "glmm scratch", e))
		return false;
	P.y = d_y;
	for (size_t j = 0; j < p; ++j) a.x[j] = x_cols[j];
	P.p = (int)p;
	P.plo = d_plo;
	P.lro = d_lro;
	P.n_panels = n_panels;
	P.n_levels = n_levels;
	P.n_rows = n_rows;
	P.reml = o.reml ? 1 : 0;
	P.invalid = glmm_options_invalid(o) ? 1 : 0;
	P.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	P.tolerance = o.tolerance;
	P.compute_inference = o.compute_inference && d_inf ? 1 : 0;
	P.zq = P.compute_inference && !P.invalid ? hostmath::normal_quantile(0.5 + o.confidence_level / 2.0) : NAN;
	P.lev = (double *)ctx->ws;
	P.parts = (double *)((char *)ctx->ws + lev);
	P.valid = (unsigned char *)ctx->ws + lev + parts;
	P.rec = d_rec;
	P.inf = d_inf;
	P.ranef = d_ranef;
	P.level_n = d_level_n;
	hipStream_t st = ctx->stream;
	if (predict) {
		char *base = (char *)ctx->ws + lev + parts + valid_al;
		P.keep = (double *)base;
		P.keep_ok = (double *)(base + keep);
		P.level_pred = (double *)(base + keep + keep_ok);
		a.pred = d_pred;
		a.interval = predict->interval;
		a.z = predict->interval ? hostmath::normal_quantile(0.5 + predict->level / 2.0) : NAN;
		a.n_tiles = n_rows / kLmPredTile + n_panels;
		if (hip_fail(hipMemsetAsync(P.keep_ok, 0, (size_t)n_panels * sizeof(double), st), "hipMemsetAsync", e)) return false;
	}
	// The search kernels stride over the panels, so a launch needs no more workgroups than fill the device; the caps also keep
	// the launches of the sizes that no panel of a device-form call needs to a few thousand workgroups that only read offsets
	// (100 000 workgroups of 1024 threads cost 7.6 ms, docs/MEASUREMENTS.md).
	const int64_t cap = 1 << 20;
	const dim3 sgrid((unsigned)(P.n_numbers < cap ? P.n_numbers : cap));
	auto pgrid = [&](int64_t most) { return dim3((unsigned)(n_panels < most ? n_panels : most)); };
	hipLaunchKernelGGL(lm_stats_kernel, sgrid, dim3(64), 0, st, a);
	if (hip_fail(hipGetLastError(), "lm_stats_kernel", e)) return false;
	if (g_stats_only.load()) return true;
	const int mask = g_wave_mask.load() ? g_wave_mask.load() : 7;
	if (cls.need[0] && (mask & 1)) {
		if (predict) hipLaunchKernelGGL((lm_search_kernel<1, true>), pgrid(1 << 16), dim3(64), lm_work_doubles(k, 1) * sizeof(double), st, a);
		else hipLaunchKernelGGL((lm_search_kernel<1, false>), pgrid(1 << 16), dim3(64), lm_work_doubles(k, 1) * sizeof(double), st, a);
		if (hip_fail(hipGetLastError(), "lm_search_kernel<1>", e)) return false;
	}
	if (cls.need[1] && (mask & 2)) {
		if (predict) hipLaunchKernelGGL((lm_search_kernel<4, true>), pgrid(1 << 12), dim3(256), lm_work_doubles(k, 4) * sizeof(double), st, a);
		else hipLaunchKernelGGL((lm_search_kernel<4, false>), pgrid(1 << 12), dim3(256), lm_work_doubles(k, 4) * sizeof(double), st, a);
		if (hip_fail(hipGetLastError(), "lm_search_kernel<4>", e)) return false;
	}
	if (cls.need[2] && (mask & 4)) {
		if (predict) hipLaunchKernelGGL((lm_search_kernel<16, true>), pgrid(1 << 10), dim3(1024), lm_work_doubles(k, 16) * sizeof(double), st, a);
		else hipLaunchKernelGGL((lm_search_kernel<16, false>), pgrid(1 << 10), dim3(1024), lm_work_doubles(k, 16) * sizeof(double), st, a);
		if (hip_fail(hipGetLastError(), "lm_search_kernel<16>", e)) return false;
	}
	if (predict) {
		const dim3 tgrid((unsigned)(a.n_tiles < cap ? a.n_tiles : cap));
		if (k <= 4) hipLaunchKernelGGL(lm_predict_kernel<4>, tgrid, dim3(64), 0, st, a);
		else if (k <= 9) hipLaunchKernelGGL(lm_predict_kernel<9>, tgrid, dim3(64), 0, st, a);
		else if (k <= 17) hipLaunchKernelGGL(lm_predict_kernel<17>, tgrid, dim3(64), 0, st, a);
		else hipLaunchKernelGGL(lm_predict_kernel<33>, tgrid, dim3(64), 0, st, a);
		if (hip_fail(hipGetLastError(), "lm_predict_kernel", e)) return false;
	}
	return true;
}

// the predict options' own rules, answered before any device is touched
bool check_glmm_predict(const AnofoxHipGlmmPredictOptions &q, const void *pred, int64_t n_panels, AnofoxError *e) {
	if (n_panels > 0 && !pred) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "pred is NULL"); return false; }
	if (q.interval < 0 || q.interval > 2) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "glmm: interval must be 0, 1 or 2"); return false; }
	if (q.interval != 0 && !(q.level > 0.0 && q.level < 1.0)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "glmm: level must be in (0, 1)");
		return false;
	}
	return true;
}

bool check_glmm_offsets(int64_t n_panels, int64_t n_levels, int64_t n_rows, const int64_t *plo, const int64_t *lro, AnofoxError *e) {
	if (n_panels == 0) return true;
	if (!check_host_offsets(n_panels, n_levels, plo, e) || !check_whole_range(n_panels, n_levels, plo, e)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "panel_level_offsets must be non-decreasing from 0 to n_levels");
		return false;
	}
	if (!check_host_offsets(n_levels, n_rows, lro, e)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "level_row_offsets must be non-decreasing and within [0, n_rows]");
		return false;
	}
	return true;
}

// host pointers: one staging of the whole call, the kernels, the copies back
bool glmm_host(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t p, int64_t n_rows, const int64_t *plo, const int64_t *lro,
               const double *y, const double *const *x_cols, const AnofoxHipGlmmOptions &o, double *rec, double *inf, double *ranef,
               int64_t *level_n, AnofoxError *e, const AnofoxHipGlmmPredictOptions *predict = nullptr, double *pred = nullptr) {
	if (!(ctx = host_context(ctx, e))) return false;
	const size_t G = (size_t)n_panels, L = (size_t)n_levels, rec_len = p + 13, inf_len = 5 * p + 1;
	Classes cls;
	cls.need[0] = cls.need[1] = cls.need[2] = false;
	for (size_t g = 0; g < G; ++g) {
		const int w = lm_wave_count(plo[g + 1] - plo[g]);
		cls.need[w == 1 ? 0 : (w == 4 ? 1 : 2)] = true;
	}
	std::lock_guard<std::mutex> lk(ctx->mu); // one lock over staging, the kernels and the copies back
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	hipStream_t st = ctx->stream;
	int64_t *d_plo, *d_lro, *d_ln;
	StagedColumns c;
	double *d_rec, *d_inf, *d_ranef, *d_pred = nullptr;
	// only the rows of [lro[0], lro[n_levels]) are written, so only they are copied back
	const size_t w0 = predict ? (size_t)lro[0] * kLmPredLen : 0, w1 = predict ? (size_t)lro[L] * kLmPredLen : 0;
	if (!stage_call(ctx, e, [&](Stage &s) {
		    d_plo = s.put(plo, G + 1);
		    d_lro = s.put(lro, L + 1);
		    c = s.columns(p, 0, n_rows, x_cols, y, nullptr, nullptr, kPlainColumns);
		    d_rec = s.take<double>(G * rec_len);
		    d_inf = inf ? s.take<double>(G * inf_len) : nullptr;
		    d_ranef = s.take<double>(L);
		    d_ln = level_n ? s.take<int64_t>(L) : nullptr;
		    if (predict) d_pred = s.take<double>((size_t)n_rows * kLmPredLen);
	    }))
		return false;
	if (!launch_glmm(ctx, n_panels, n_levels, p, n_rows, d_plo, d_lro, c.y, c.x, o, d_rec, d_inf, d_ranef, d_ln, cls, e, predict, d_pred))
		return false;
	if (w1 > w0 && !d2h(pred + w0, d_pred + w0, (w1 - w0) * sizeof(double), st, e)) return false;
	if (!d2h(rec, d_rec, G * rec_len * sizeof(double), st, e)) return false;
	if (inf && !d2h(inf, d_inf, G * inf_len * sizeof(double), st, e)) return false;
	if (!d2h(ranef, d_ranef, L * sizeof(double), st, e)) return false;
	if (level_n && !d2h(level_n, d_ln, L * sizeof(int64_t), st, e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

void free_glmm_arrays(AnofoxGlmmResult *r) {
	free(r->coefficients);
	free(r->std_errors);
	free(r->z_values);
	free(r->p_values);
	free(r->ci_lower);
	free(r->ci_upper);
	free(r->ranef_group);
	free(r->ranef_value);
	free(r->ranef_se);
	free(r->ranef_n);
	free(r->random_cov);
	free(r->ranef_effects);
	free(r->factor_var);
	free(r->factor_n_levels);
}

void reset_glmm_result(AnofoxGlmmResult *r) {
	memset(r, 0, sizeof *r);
	r->intercept = r->intercept_std_error = r->confidence_level = r->var_group = r->var_residual = r->icc = r->log_likelihood = r->aic =
	    r->bic = r->deviance = NAN;
}

template <class T>
bool alloc_array(T **out, size_t n) {
	*out = (T *)malloc((n ? n : 1) * sizeof(T));
	return *out != nullptr;
}

} // namespace

extern "C" {

size_t anofox_hip_glmm_record_len(size_t p) { return p + 13; }
size_t anofox_hip_glmm_inference_len(size_t p) { return 5 * p + 1; }

void anofox_hip_glmm_test_hooks(int stats_only, int wave_mask) {
	g_stats_only.store(stats_only ? 1 : 0);
	g_wave_mask.store(wave_mask & 7);
}

bool anofox_hip_glmm_fit_batch_device(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features, int64_t n_rows,
                                      const int64_t *d_panel_level_offsets, const int64_t *d_level_row_offsets, const double *d_y,
                                      const double *const *d_x_cols, AnofoxHipGlmmOptions options, double *d_glmm, double *d_inference,
                                      double *d_ranef, int64_t *d_level_n, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glmm(n_panels, n_levels, n_features, n_rows, d_panel_level_offsets, d_level_row_offsets, d_y, d_x_cols, options.family, d_glmm,
	                d_ranef, out_error))
		return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_glmm(ctx, n_panels, n_levels, n_features, n_rows, d_panel_level_offsets, d_level_row_offsets, d_y, d_x_cols, options, d_glmm,
	                   d_inference, d_ranef, d_level_n, Classes(), out_error);
}

bool anofox_hip_glmm_fit_batch_host(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features, int64_t n_rows,
                                    const int64_t *panel_level_offsets, const int64_t *level_row_offsets, const double *y,
                                    const double *const *x_cols, AnofoxHipGlmmOptions options, double *glmm, double *inference, double *ranef,
                                    int64_t *level_n, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glmm(n_panels, n_levels, n_features, n_rows, panel_level_offsets, level_row_offsets, y, x_cols, options.family, glmm, ranef,
	                out_error))
		return false;
	if (!check_glmm_offsets(n_panels, n_levels, n_rows, panel_level_offsets, level_row_offsets, out_error)) return false;
	if (n_panels == 0) return true;
	return glmm_host(ctx, n_panels, n_levels, n_features, n_rows, panel_level_offsets, level_row_offsets, y, x_cols, options, glmm, inference,
	                 ranef, level_n, out_error);
}

size_t anofox_hip_glmm_pred_len(void) { return kLmPredLen; }

bool anofox_hip_glmm_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features, int64_t n_rows,
                                              const int64_t *d_panel_level_offsets, const int64_t *d_level_row_offsets, const double *d_y,
                                              const double *const *d_x_cols, AnofoxHipGlmmOptions options,
                                              AnofoxHipGlmmPredictOptions predict, double *d_glmm, double *d_inference, double *d_ranef,
                                              int64_t *d_level_n, double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glmm(n_panels, n_levels, n_features, n_rows, d_panel_level_offsets, d_level_row_offsets, d_y, d_x_cols, options.family, d_glmm,
	                d_ranef, out_error))
		return false;
	if (!check_glmm_predict(predict, d_pred, n_panels, out_error)) return false;
	if (!ctx) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	return launch_glmm(ctx, n_panels, n_levels, n_features, n_rows, d_panel_level_offsets, d_level_row_offsets, d_y, d_x_cols, options, d_glmm,
	                   d_inference, d_ranef, d_level_n, Classes(), out_error, &predict, d_pred);
}

bool anofox_hip_glmm_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_panels, int64_t n_levels, size_t n_features, int64_t n_rows,
                                            const int64_t *panel_level_offsets, const int64_t *level_row_offsets, const double *y,
                                            const double *const *x_cols, AnofoxHipGlmmOptions options, AnofoxHipGlmmPredictOptions predict,
                                            double *glmm, double *inference, double *ranef, int64_t *level_n, double *pred,
                                            AnofoxError *out_error) {
	reset_error(out_error);
	if (!check_glmm(n_panels, n_levels, n_features, n_rows, panel_level_offsets, level_row_offsets, y, x_cols, options.family, glmm, ranef,
	                out_error))
		return false;
	if (!check_glmm_predict(predict, pred, n_panels, out_error)) return false;
	if (!check_glmm_offsets(n_panels, n_levels, n_rows, panel_level_offsets, level_row_offsets, out_error)) return false;
	if (n_panels == 0) return true;
	return glmm_host(ctx, n_panels, n_levels, n_features, n_rows, panel_level_offsets, level_row_offsets, y, x_cols, options, glmm, inference,
	                 ranef, level_n, out_error, &predict, pred);
}

// A batch of one panel with anofox_ols_fit's conventions: argument checks first, NULL entries -> NaN, the arrays malloc'ed.
bool anofox_glmm_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, const int32_t *group_ids, size_t n_obs,
                     const int32_t *const *extra_group_ids, size_t n_extra_factors, AnofoxGlmmOptions options, AnofoxGlmmResult *out_result,
                     AnofoxError *out_error) {
	(void)extra_group_ids;
	reset_error(out_error);
	if (!out_result) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL"); return false; }
	reset_glmm_result(out_result); // a failed call leaves nothing to free
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (y.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: y cannot be empty"); return false; }
	if (!group_ids || n_obs != y.len) {
		set_error(out_error, ANOFOX_ERROR_DIMENSION_MISMATCH,
		          "Dimension mismatch: y has " + std::to_string(y.len) + " elements, group has " + std::to_string(group_ids ? n_obs : 0));
		return false;
	}
	for (size_t j = 0; j < x_count; ++j) {
		if (x[j].len != y.len) {
			set_error(out_error, ANOFOX_ERROR_DIMENSION_MISMATCH,
			          "Dimension mismatch: y has " + std::to_string(y.len) + " elements, X has " + std::to_string(x[j].len) + " rows");
			return false;
		}
	}
	if (options.offset_column != 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glmm: an offset is not built"); return false; }
	if ((int)options.family != ANOFOX_GLMM_GAUSSIAN) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, std::string("glmm: the ") + family_name((int)options.family) + " family is not built");
		return false;
	}
	if (options.random_slopes_len > 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glmm: random slopes are not built"); return false; }
	if (n_extra_factors > 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glmm: crossed factors are not built"); return false; }
	const size_t n = y.len, p = x_count;
	if (p > (size_t)kLmMaxP) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glmm: n_features > 32 is not built"); return false; }
	AnofoxHipGlmmOptions o;
	memset(&o, 0, sizeof o);
	o.family = ANOFOX_GLMM_GAUSSIAN;
	o.fit_intercept = options.fit_intercept ? 1 : 0;
	o.reml = options.reml ? 1 : 0;
	o.max_iterations = options.max_iterations;
	o.tolerance = options.tolerance;
	o.compute_inference = options.compute_inference ? 1 : 0;
	o.confidence_level = options.confidence_level;
	if (glmm_options_invalid(o)) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "glmm: invalid options"); return false; }
	// the levels in first-seen order, rows with an id < 0 dropped; the rows sorted by level (stably)
	std::unordered_map<int32_t, int64_t> seen;
	std::vector<int32_t> labels;
	std::vector<int64_t> level_of(n, -1);
	for (size_t i = 0; i < n; ++i) {
		if (group_ids[i] < 0) continue;
		auto it = seen.find(group_ids[i]);
		if (it == seen.end()) {
			it = seen.emplace(group_ids[i], (int64_t)labels.size()).first;
			labels.push_back(group_ids[i]);
		}
		level_of[i] = it->second;
	}
	const size_t L = labels.size();
	std::vector<int64_t> lro(L + 1, 0);
	for (size_t i = 0; i < n; ++i)
		if (level_of[i] >= 0) ++lro[(size_t)level_of[i] + 1];
	for (size_t l = 0; l < L; ++l) lro[l + 1] += lro[l];
	const size_t R = (size_t)lro[L];
	std::vector<int64_t> at(lro.begin(), lro.end() - 1);
	std::vector<size_t> order(R);
	for (size_t i = 0; i < n; ++i)
		if (level_of[i] >= 0) order[(size_t)at[(size_t)level_of[i]]++] = i;
	std::vector<double> full, yv(R);
	expand_data_array(y, full);
	for (size_t r = 0; r < R; ++r) yv[r] = full[order[r]];
	std::vector<std::vector<double>> cols(p, std::vector<double>(R));
	std::vector<const double *> xp(p);
	for (size_t j = 0; j < p; ++j) {
		expand_data_array(x[j], full);
		for (size_t r = 0; r < R; ++r) cols[j][r] = full[order[r]];
		xp[j] = cols[j].data();
	}
	const int64_t plo[2] = {0, (int64_t)L};
	std::vector<double> rec(p + 13), inf(5 * p + 1), ranef(L ? L : 1);
	std::vector<int64_t> ln(L ? L : 1);
	if (!glmm_host(nullptr, 1, (int64_t)L, p, (int64_t)R, plo, lro.data(), yv.data(), xp.data(), o, rec.data(),
	               o.compute_inference ? inf.data() : nullptr, ranef.data(), ln.data(), out_error))
		return false;
	const int status = (int)rec[p + 12];
	if (status != ANOFOX_ERROR_SUCCESS) {
		set_error(out_error, (AnofoxErrorCode)status,
		          status == ANOFOX_ERROR_NO_VALID_DATA       ? std::string("No valid data: every row has a NULL or non-finite value")
		          : status == ANOFOX_ERROR_INSUFFICIENT_DATA ? std::string("Insufficient data: too few valid rows for the fixed effects")
		                                                     : std::string("glmm: a mixed model needs at least two groups, and one group with more than one row"));
		return false;
	}
	// the levels with a valid row, in first-seen order
	size_t kept = 0;
	for (size_t l = 0; l < L; ++l) kept += ln[l] > 0;
	AnofoxGlmmResult r;
	reset_glmm_result(&r);
	const size_t ni = o.compute_inference ? p : 0;
	bool ok = alloc_array(&r.coefficients, p) && alloc_array(&r.ranef_group, kept) && alloc_array(&r.ranef_value, kept) &&
	          alloc_array(&r.ranef_se, kept) && alloc_array(&r.ranef_n, kept) && alloc_array(&r.random_cov, 1) &&
	          alloc_array(&r.ranef_effects, kept);
	if (ok && ni)
		ok = alloc_array(&r.std_errors, p) && alloc_array(&r.z_values, p) && alloc_array(&r.p_values, p) && alloc_array(&r.ci_lower, p) &&
		     alloc_array(&r.ci_upper, p);
	if (!ok) {
		free_glmm_arrays(&r);
		set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate the result arrays");
		return false;
	}
	for (size_t j = 0; j < p; ++j) {
		r.coefficients[j] = rec[j];
		if (ni) {
			r.std_errors[j] = inf[j];
			r.z_values[j] = inf[p + j];
			r.p_values[j] = inf[2 * p + j];
			r.ci_lower[j] = inf[3 * p + j];
			r.ci_upper[j] = inf[4 * p + j];
		}
	}
	r.coefficients_len = p;
	r.inference_len = ni;
	r.intercept = rec[p];
	r.intercept_std_error = ni ? inf[5 * p] : NAN;
	r.confidence_level = options.confidence_level;
	r.var_group = rec[p + 1];
	r.var_residual = rec[p + 2];
	r.icc = rec[p + 3];
	r.log_likelihood = rec[p + 4];
	r.aic = rec[p + 5];
	r.bic = rec[p + 6];
	r.deviance = rec[p + 7];
	r.n_observations = (size_t)rec[p + 8];
	r.n_groups = (size_t)rec[p + 9];
	r.n_features = p;
	r.iterations = (uint32_t)rec[p + 10];
	r.converged = rec[p + 11] != 0.0;
	size_t w = 0;
	for (size_t l = 0; l < L; ++l) {
		if (ln[l] <= 0) continue;
		r.ranef_group[w] = labels[l];
		r.ranef_value[w] = r.ranef_effects[w] = ranef[l];
		r.ranef_se[w] = NAN;
		r.ranef_n[w] = ln[l];
		++w;
	}
	r.ranef_len = kept;
	r.random_cov[0] = r.var_group;
	r.random_dim = 1;
	*out_result = r;
	return true;
}

void anofox_free_glmm_result(AnofoxGlmmResult *result) {
	if (!result) return;
	free_glmm_arrays(result);
	reset_glmm_result(result);
}

} // extern "C"
