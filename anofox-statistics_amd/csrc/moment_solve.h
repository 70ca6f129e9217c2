// moment_solve.h — what the solvers on the accumulate kernels' moment records (elasticnet.hip, bls.hip) share around their
// own solve: the view of a wide record, the pass over the rows of the groups whose moment identity cancelled, the launch of a
// wide solve kernel and the accumulate options of their moments.  Device and host.
#pragma once
#include "context.h"

namespace anofox {

// A wide record (accumulate_wide_impl.h) as a wide solve kernel reads it: the upper-triangle 16 x 16 tiles of X'X, then the
// per-column vectors and the scalars, shifted by the first valid row when an intercept is fitted.
struct WideMoments {
	const double *rec, *sx, *sxy, *fx, *nonconst;
	int T;
	double sy, syy, sw, cnt, first_y;
	int p_eff;    // the columns that are not constant
	double cyy_c; // the centred S_yy

	__device__ __forceinline__ WideMoments(const double *moments, int64_t gl, int p) {
		T = wide_tiles(p);
		const int P16 = 16 * T, NT = T * (T + 1) / 2;
		rec = moments + gl * (int64_t)wide_record_len(T);
		const double *vec = rec + (int64_t)NT * 256;
		sx = vec, sxy = vec + P16, fx = vec + 2 * P16, nonconst = vec + 3 * P16;
		const double *sc = vec + 4 * P16;
		sy = sc[0], syy = sc[1], sw = sc[2], cnt = sc[3], first_y = sc[4];
		p_eff = 0;
		for (int j = 0; j < p; ++j) p_eff += nonconst[j] != 0.0 ? 1 : 0;
		cyy_c = syy - sy * sy / sw;
	}
	__device__ __forceinline__ double ymean(bool icpt) const { return (icpt ? first_y : 0.0) + sy / sw; }
	// element (lo, hi), lo <= hi, of the X'X the record keeps
	__device__ __forceinline__ double raw(int lo, int hi) const {
		const int I = lo >> 4, J = hi >> 4;
		const int tile = I * T - I * (I - 1) / 2 + (J - I);
		return rec[(int64_t)tile * 256 + (lo & 15) * 16 + (hi & 15)];
	}
	// the same element of C: centred when an intercept is fitted; inv_sw = 1 / sw
	__device__ __forceinline__ double c(int lo, int hi, bool icpt, double inv_sw) const {
		double v = raw(lo, hi);
		if (icpt) v -= sx[lo] * sx[hi] * inv_sw;
		return v;
	}
};

// ---- the statistic from the rows of the groups whose moment identity cancelled (flag[gl] == 1), one wavefront per group ----
struct RowsArgs {
	const int64_t *row_offsets;
	const int64_t *row_ends; // optional: group g owns rows [row_offsets[g], row_ends[g]) (BatchArgs::row_ends)
	const double *y;
	const double *x_table[kWideMaxP];
	double *core;
	const int32_t *flag; // [n_groups] of this launch
	int64_t group_base, n_groups;
	int p;
	int fit_intercept;
};

template <class Args>
inline RowsArgs rows_args_common(const Args &a, int64_t group_base) {
	RowsArgs ra;
	memset(&ra, 0, sizeof ra);
	ra.row_offsets = a.row_offsets;
	ra.row_ends = a.row_ends;
	ra.y = a.y;
	ra.core = a.core;
	ra.flag = a.refine_list;
	ra.group_base = group_base;
	ra.n_groups = a.n_groups;
	ra.p = a.p;
	ra.fit_intercept = a.fit_intercept;
	return ra;
}
inline RowsArgs rows_args(const BatchArgs &a) {
	RowsArgs ra = rows_args_common(a, 0);
	for (int j = 0; j < a.p; ++j) ra.x_table[j] = a.x[j];
	return ra;
}
inline RowsArgs rows_args(const WideArgs &a) {
	RowsArgs ra = rows_args_common(a, a.group_base);
	for (int j = 0; j < a.p; ++j) ra.x_table[j] = a.x_table[j];
	return ra;
}

// a wavefront's sum of squared residuals y - b0 - x'b over the finite rows of group g; b = core[0..p), NaN = not fitted
__device__ __forceinline__ double rows_ssr(const RowsArgs &a, int64_t g, const double *core, double b0, int lane) {
	const int p = a.p;
	double ssr = 0.0;
	const int64_t hi = a.row_ends ? a.row_ends[g] : a.row_offsets[g + 1];
	for (int64_t row = a.row_offsets[g] + lane; row < hi; row += 64) {
		const double yv = a.y[row];
		bool ok = isfinite(yv);
		double fit = b0;
		for (int j = 0; j < p; ++j) {
			const double xv = a.x_table[j][row];
			ok = ok && isfinite(xv);
			const double bj = core[j];
			if (!isnan(bj)) fit = fma(bj, xv, fit);
		}
		const double e = yv - fit;
		if (ok) ssr = fma(e, e, ssr);
	}
	for (int m = 32; m >= 1; m >>= 1) ssr += __shfl_xor(ssr, m, 64);
	return ssr;
}

inline unsigned rows_grid(int64_t n_groups) { return n_groups < 16384 ? (unsigned)n_groups : 16384u; }

// One wavefront per group of a wide solve kernel's two instances (R = 1: p <= 64, R = 2: p <= 128) with `lds` bytes of dynamic
// LDS; the first launch lifts both instances' LDS limit.
template <auto K1, auto K2, class Params>
hipError_t launch_wide_r(const WideArgs &a, const Params &params, size_t lds, hipStream_t st) {
	static const bool attr_set = [] {
		(void)hipFuncSetAttribute(reinterpret_cast<const void *>(K1), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
		(void)hipFuncSetAttribute(reinterpret_cast<const void *>(K2), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
		return true;
	}();
	(void)attr_set;
	if (a.p <= 64) hipLaunchKernelGGL(K1, dim3((unsigned)a.n_groups), dim3(64), lds, st, a, params);
	else hipLaunchKernelGGL(K2, dim3((unsigned)a.n_groups), dim3(64), lds, st, a, params);
	return hipGetLastError();
}

// the accumulate options of a solver's moments: those of an unweighted fit
inline AnofoxHipBatchOptions unweighted_moment_options(bool fit_intercept, double confidence_level) {
	AnofoxHipBatchOptions acc;
	memset(&acc, 0, sizeof acc);
	acc.model = ANOFOX_HIP_MODEL_OLS;
	acc.fit_intercept = fit_intercept;
	acc.confidence_level = confidence_level;
	acc.hc_type = ANOFOX_HC_NONE;
	return acc;
}

} // namespace anofox
