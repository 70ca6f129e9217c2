// elasticnet_solve.h — the per-group elastic net solve on a MomentLayout<P> record, shared by the batch kernels
// (elasticnet.hip) and the in-register window kernels (window_narrow.hip).  DESIGN.md §1, "Elastic net".
//
// Reference: fit_elasticnet (crates/anofox-stats-core/src/models/elasticnet.rs:29-200): alpha / l1_ratio checks, the row
// filter (finite y and x, no weights), the constant-column test |x - x_first| < 1e-10, the intercept-only shortcut and
// NaN coefficients at constant columns.  Per group the solve minimises
//     1/2 sum_i (y_i - b0 - x_i'b)^2 + lam (l1 sum |b_j| + (1 - l1)/2 sum b_j^2)
// over the non-constant columns by cyclic coordinate descent from b = 0 (see elasticnet.hip).
#pragma once

#include "common.h"

namespace anofox {

constexpr double kEnRefineTol = 1e-7;  // rss / tss below this => rss from the rows
constexpr double kEnAliasTol = 1e-11; // the window kernels' aliasing test (window_narrow.hip: kAliasTolX)

__device__ __forceinline__ double en_nan() { return __builtin_nan(""); }
__device__ __forceinline__ double soft_threshold(double z, double t) { return z > t ? z - t : (z < -t ? z + t : 0.0); }

// The checks every group passes before its solve (elasticnet.rs:33-136 and the aggregate's "< 2 rows -> NULL" rule).
// Returns the status; 0 with *shortcut = true is the intercept-only fit (en_write_shortcut).
__device__ __forceinline__ int en_prechecks(const EnParams &en, int64_t nrows, double cnt, int p_eff, bool icpt, bool *shortcut) {
	*shortcut = false;
	if (nrows < 2) return ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS;                            // the aggregate's NULL rule
	if (!(en.alpha >= 0.0)) return ANOFOX_ERROR_INVALID_ALPHA;                             // elasticnet.rs:34-36
	if (!(en.l1_ratio >= 0.0 && en.l1_ratio <= 1.0)) return ANOFOX_ERROR_INVALID_L1_RATIO; // elasticnet.rs:39-41
	if (!(cnt > 0.0)) return ANOFOX_ERROR_NO_VALID_DATA;                                   // elasticnet.rs:77-79
	if (p_eff == 0) {                                                                      // elasticnet.rs:104-128
		if (!icpt) return ANOFOX_ERROR_INSUFFICIENT_DATA;
		*shortcut = true;
		return 0;
	}
	if (cnt < (double)(p_eff + (icpt ? 1 : 0))) return ANOFOX_ERROR_INSUFFICIENT_DATA; // elasticnet.rs:131-136
	return 0;
}

// every column constant, with an intercept: NaN coefficients, the mean, r2 = adj = 0, sd(y) with n - 1 (elasticnet.rs:110-128)
__device__ __forceinline__ void en_write_shortcut(double *core, int p, double ymean, double cyy_c, double cnt) {
	for (int k = 0; k < p; ++k) core[k] = en_nan();
	core[p] = ymean;
	core[p + 1] = 0.0;
	core[p + 2] = 0.0;
	core[p + 3] = sqrt(cyy_c / (cnt - 1.0));
	core[p + 4] = cnt;
	core[p + 5] = 0.0;
}

__device__ __forceinline__ void en_write_status(double *core, int p, int status) {
	for (int k = 0; k < p + 5; ++k) core[k] = en_nan();
	core[p + 5] = (double)status;
}

// penalty: raw lam = alpha; glmnet lam = n alpha / sd_y, sd_y about the mean with or without an intercept (the ridge rule,
// solve_narrow.hip).  The L1 / L2 parts, with 0 where their share is 0 (an infinite lam times 0 is not NaN).
__device__ __forceinline__ void en_penalty(const EnParams &en, double cnt, double cyy_c, double *pen1, double *pen2) {
	const double lam = en.lambda_scaling == ANOFOX_LAMBDA_SCALING_GLMNET ? cnt * en.alpha / sqrt(cyy_c / cnt) : en.alpha;
	*pen1 = en.l1_ratio > 0.0 ? lam * en.l1_ratio : 0.0;
	*pen2 = en.l1_ratio < 1.0 ? lam * (1.0 - en.l1_ratio) : 0.0;
}

// r2 / adj / rse / n of a finished fit (the ridge record's formulas, df from the non-constant columns); groups whose moment
// rss cancelled get their tss parked in the r2 slot and flag 1 (rows_rss_kernel, or a window kernel's refit list)
__device__ __forceinline__ void en_write_stats(double *core, int p, double rss, double tss, double cnt, int p_eff, bool icpt,
                                               int32_t *flag) {
	const double df = cnt - (double)(p_eff + (icpt ? 1 : 0));
	const bool cancels = !(rss > kEnRefineTol * tss);
	const double r2 = 1.0 - rss / tss;
	core[p + 1] = cancels ? tss : r2;
	core[p + 2] = 1.0 - (1.0 - r2) * (cnt - (icpt ? 1.0 : 0.0)) / df;
	core[p + 3] = sqrt(rss / df);
	core[p + 4] = cnt;
	core[p + 5] = 0.0;
	*flag = cancels ? 1 : 0;
}

struct EnSolveInfo {
	int sweeps;       // coordinate-descent sweeps (0: no solve ran)
	bool converged;   // false: max_iterations stopped it
	bool cancels;     // the moment rss cancelled: core[p + 1] holds tss, the rss is to be summed from the rows
	bool small_pivot; // (COND only) some Cholesky pivot of C + pen2 I below 1e-3 of its diagonal entry
};

// The elastic net fit of one group from its moment record `rec` (MomentLayout<P>; a pointer or a register array) into the
// p + 6 record `core`: prechecks, penalty, sweeps, stopping rule and statistics.  nrows = the count the "< 2 rows" rule
// looks at.  COND: afterwards factor C + pen2 I in place for the window kernels' conditioning test (window_narrow.hip).
template <int P, bool COND, typename Rec>
__device__ __forceinline__ EnSolveInfo en_fit_from_moments(const Rec &rec, const EnParams &en, bool icpt, int64_t nrows,
                                                           double (&core)[P + 6]) {
	using L = MomentLayout<P>;
	EnSolveInfo info = {0, true, false, false};
	const double cnt = rec[L::OFF_CNT], sw = rec[L::OFF_SW];
	const unsigned mask = (unsigned)rec[L::OFF_MASK];
	const int p_eff = __popc(mask);
	const double sy = rec[L::OFF_S + P], qyy = rec[L::q_index(P, P)];
	const double cyy_c = qyy - sy * sy / sw;
	const double ymean = (icpt ? rec[L::OFF_FIRST + P] : 0.0) + sy / sw;
	bool shortcut;
	const int status = en_prechecks(en, nrows, cnt, p_eff, icpt, &shortcut);
	if (status != 0 || shortcut) {
		if (status != 0) en_write_status(core, P, status);
		else en_write_shortcut(core, P, ymean, cyy_c, cnt);
		return info;
	}
	double C[P][P], c[P], b[P], xbar[P];
#pragma unroll
	for (int i = 0; i < P; ++i) {
		const double si = rec[L::OFF_S + i];
		xbar[i] = (icpt ? rec[L::OFF_FIRST + i] : 0.0) + si / sw;
#pragma unroll
		for (int j = 0; j <= i; ++j) {
			const double v = rec[L::q_index(j, i)] - (icpt ? si * rec[L::OFF_S + j] / sw : 0.0);
			C[i][j] = v;
			C[j][i] = v;
		}
		c[i] = rec[L::q_index(i, P)] - (icpt ? si * sy / sw : 0.0);
		b[i] = 0.0;
	}
	const double tss = icpt ? cyy_c : qyy;
	double pen1, pen2;
	en_penalty(en, cnt, cyy_c, &pen1, &pen2);
	const double thresh = en.tolerance * sqrt(tss);
	int sweeps = 0;
	bool converged = false;
	while (sweeps < en.max_iterations) {
		++sweeps;
		double dmax = 0.0;
#pragma unroll
		for (int j = 0; j < P; ++j) {
			if (!((mask >> j) & 1u)) continue;
			double z = c[j];
#pragma unroll
			for (int k = 0; k < P; ++k)
				if (k != j) z -= C[j][k] * b[k];
			const double bn = soft_threshold(z, pen1) / (C[j][j] + pen2);
			dmax = fmax(dmax, sqrt(C[j][j]) * fabs(bn - b[j]));
			b[j] = bn;
		}
		if (dmax <= thresh) { converged = true; break; }
	}
	double bc = 0.0, bcb = 0.0, b0 = ymean;
#pragma unroll
	for (int i = 0; i < P; ++i) {
		double cbi = 0.0;
#pragma unroll
		for (int k = 0; k < P; ++k) cbi += C[i][k] * b[k];
		bc += b[i] * c[i];
		bcb += b[i] * cbi;
		b0 -= b[i] * xbar[i];
	}
#pragma unroll
	for (int j = 0; j < P; ++j) core[j] = ((mask >> j) & 1u) ? b[j] : en_nan();
	core[P] = icpt ? b0 : en_nan();
	int32_t flag = 0;
	en_write_stats(core, P, tss - 2.0 * bc + bcb, tss, cnt, p_eff, icpt, &flag);
	info.sweeps = sweeps;
	info.converged = converged;
	info.cancels = flag != 0;
	if (COND) {
		// the window kernels' test (window_narrow.hip, fit_from_moments) on the matrix the sweeps divide by: an active column
		// whose pivot falls below 1e-3 of its diagonal entry (aliased ones included) sends the frame to the frames path
		bool small = false;
#pragma unroll
		for (int j = 0; j < P; ++j) {
			const bool act = (mask >> j) & 1u;
			const double diag0 = C[j][j] + pen2;
			double d = diag0;
#pragma unroll
			for (int k = 0; k < j; ++k) d -= C[j][k] * C[j][k];
			const bool ok = act && (d > kEnAliasTol * diag0) && (d > 0.0);
			small = small || (act && !(d >= 1e-3 * diag0));
			const double inv = ok ? 1.0 / sqrt(d) : 0.0;
#pragma unroll
			for (int i = j + 1; i < P; ++i) {
				double t = C[i][j];
#pragma unroll
				for (int k = 0; k < j; ++k) t -= C[i][k] * C[j][k];
				C[i][j] = t * inv;
			}
		}
		info.small_pivot = small;
	}
	return info;
}

} // namespace anofox
