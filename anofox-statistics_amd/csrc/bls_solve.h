// bls_solve.h — the per-group bounded least squares solve on a MomentLayout<P> record (the lane-per-group kernels of
// bls.hip), and the pieces it shares with the wavefront-per-group kernels there.  DESIGN.md §1, "Bounded least squares".
//
// Reference: fit_bls (crates/anofox-stats-core/src/models/bls.rs:59-243): the row filter (finite y and x, no weights), the
// constant-column test |x - x_first| < 1e-10, the intercept-only shortcut (ssr = NaN), NaN coefficients at constant
// columns, the bound flags |b_j - bound_j| < tolerance with "lower wins".  Per group the solve finds THE minimiser of
//     1/2 sum_i (y_i - b0 - x_i'b)^2   subject to   lo_j <= b_j <= hi_j,   b0 free
// over the non-constant columns: a strictly convex box-constrained quadratic in the centred (with an intercept) or raw
// moments C = X'X, c = X'y.  The method is an active-set one (Lawson-Hanson NNLS with two-sided bounds, i.e. Stark-Parker
// BVLS) in the scaled variables z_j = sqrt(C_jj) b_j, A = D^-1 C D^-1 (unit diagonal), q = D^-1 c:
//   start   every bounded column on a bound (the lower one if finite, else the upper one), unbounded columns free;
//   outer   w = q - A z.  A column on its lower bound with w_j > tau, or on its upper bound with w_j < -tau, violates the
//           KKT conditions; the worst one is freed.  None: done.  tau = kBlsKktTol sqrt(tss).
//   inner   the Newton step on the free set, A_FF d = w_F, by a Cholesky factorisation of the free block (refactorised every
//           pass).  If z + d is inside the box it is taken whole and the outer loop resumes; otherwise the longest feasible
//           fraction of it is taken, the column that stopped it goes onto the bound it hit, and the step is repeated.
// z stays feasible throughout, so the iterate at hand when max_iterations runs out is returned as it is.  A free-block
// pivot below kEnAliasTol (of a unit diagonal) means the free columns are collinear: on the first pass after a column was
// freed that column goes back to its bound and is not chosen again until the free set has changed; on later passes the
// column keeps its value (zero step).  No atomics, no data-dependent order of summation: two calls give the same bits.
#pragma once

#include "common.h"
#include "elasticnet_solve.h"

namespace anofox {

constexpr double kBlsKktTol = 1e-11; // a multiplier below this share of sqrt(tss) (scaled columns) counts as zero
// outer iterations never exceed this many whatever max_iterations says (the CPU sweep behind the design needed <= p)
__host__ __device__ inline int bls_iteration_cap(int p) { return 8 * p + 64; }

__device__ __forceinline__ double bls_inf() { return __builtin_inf(); }

// The checks every group passes before its solve (bls.rs:74-132 and the aggregates' "< 2 rows -> NULL" rule).
__device__ __forceinline__ int bls_prechecks(int invalid, int64_t nrows, double cnt, int p_eff, bool icpt, bool *shortcut) {
	*shortcut = false;
	if (nrows < 2) return ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS;
	if (invalid) return ANOFOX_ERROR_INVALID_INPUT; // unusable bounds: a stated difference
	if (!(cnt > 0.0)) return ANOFOX_ERROR_NO_VALID_DATA; // bls.rs:75-77
	if (p_eff == 0) {                                    // bls.rs:104-125
		if (!icpt) return ANOFOX_ERROR_INSUFFICIENT_DATA;
		*shortcut = true;
		return 0;
	}
	if (cnt < (double)(p_eff + (icpt ? 1 : 0))) return ANOFOX_ERROR_INSUFFICIENT_DATA; // bls.rs:127-132
	return 0;
}

// The reference's sigma of the fit-predict aggregate (bls_fit_predict_aggregate.cpp:391-395): df over ALL columns in
// unsigned 64-bit arithmetic — a quirk kept.
__device__ __forceinline__ double bls_predict_sigma(double ssr, double cnt, int p, bool icpt) {
	const uint64_t df = (uint64_t)cnt - (uint64_t)p - (uint64_t)(icpt ? 1 : 0);
	return (df > 0 && ssr >= 0.0) ? sqrt(ssr / (double)df) : en_nan();
}

// The scalar fields of a finished record.  predict_layout 0: {.., intercept, ssr, r2, n, n_active, status};
// 1: {.., intercept, r2, ssr, sigma, n, status}.  A cancelled ssr (<= kEnRefineTol tss) parks tss in the r2 slot and
// raises *flag: bls_rows_kernel sums it from the rows.
__device__ __forceinline__ void bls_write_stats(double *core, int p, int predict_layout, double ssr, double tss, double cnt,
                                                int n_active, bool icpt, int32_t *flag) {
	const bool cancels = !(ssr > kEnRefineTol * tss);
	const double r2 = cancels ? tss : 1.0 - ssr / tss;
	if (predict_layout) {
		core[p + 1] = r2;
		core[p + 2] = ssr;
		core[p + 3] = bls_predict_sigma(ssr, cnt, p, icpt);
		core[p + 4] = cnt;
	} else {
		core[p + 1] = ssr;
		core[p + 2] = r2;
		core[p + 3] = cnt;
		core[p + 4] = (double)n_active;
	}
	core[p + 5] = 0.0;
	*flag = cancels ? 1 : 0;
}

// every column constant, with an intercept: NaN coefficients, the mean, ssr = NaN, r2 = 0, no active bound (bls.rs:111-124)
__device__ __forceinline__ void bls_write_shortcut(double *core, int p, int predict_layout, double ymean, double cnt) {
	for (int k = 0; k < p; ++k) core[k] = en_nan();
	core[p] = ymean;
	if (predict_layout) {
		core[p + 1] = 0.0;
		core[p + 2] = en_nan();
		core[p + 3] = en_nan();
		core[p + 4] = cnt;
	} else {
		core[p + 1] = en_nan();
		core[p + 2] = 0.0;
		core[p + 3] = cnt;
		core[p + 4] = 0.0;
		for (int k = 0; k < 2 * p; ++k) core[p + 6 + k] = 0.0;
	}
	core[p + 5] = 0.0;
}

__device__ __forceinline__ void bls_write_status(double *core, int p, int predict_layout, int status) {
	const int len = predict_layout ? p + 6 : 3 * p + 6;
	for (int k = 0; k < len; ++k) core[k] = en_nan();
	core[p + 5] = (double)status;
}

// bls.rs:223-229: lower wins
__device__ __forceinline__ int bls_flags(double b, double lo, double hi, double tolerance) {
	if (isfinite(lo) && fabs(b - lo) < tolerance) return 1;
	if (isfinite(hi) && fabs(b - hi) < tolerance) return 2;
	return 0;
}

struct BlsSolveInfo {
	int iterations; // outer iterations (0: no solve ran)
	bool converged; // false: the iteration limit stopped it
	bool cancels;   // the moment ssr cancelled: the r2 slot holds tss, the ssr is to be summed from the rows
};

// The fit of one group from its moment record `rec` (MomentLayout<P>) into `core`: the 3P + 6 record, or its first P + 6
// entries in the regression layout when bp.predict_layout is set.  Everything in registers; every index is a constant after
// unrolling.
template <int P, typename Rec>
__device__ __forceinline__ BlsSolveInfo bls_fit_from_moments(const Rec &rec, const BlsParamsT<kNarrowMaxP> &bp, bool icpt,
                                                             int64_t nrows, double (&core)[3 * P + 6]) {
	using L = MomentLayout<P>;
	BlsSolveInfo info = {0, true, false};
	const int pl = bp.predict_layout;
	const double cnt = rec[L::OFF_CNT], sw = rec[L::OFF_SW];
	const unsigned mask = (unsigned)rec[L::OFF_MASK];
	const int p_eff = __popc(mask);
	const double sy = rec[L::OFF_S + P], qyy = rec[L::q_index(P, P)];
	const double cyy_c = qyy - sy * sy / sw;
	const double ymean = (icpt ? rec[L::OFF_FIRST + P] : 0.0) + sy / sw;
	bool shortcut;
	const int status = bls_prechecks(bp.invalid, nrows, cnt, p_eff, icpt, &shortcut);
	if (status != 0 || shortcut) {
		// (constant trip counts: `core` is a register array here; the kernel stores the entries its layout has)
#pragma unroll
		for (int k = 0; k < 3 * P + 6; ++k) core[k] = (status != 0 || k < P) ? en_nan() : 0.0;
		if (status != 0) {
			core[P + 5] = (double)status;
		} else { // bls.rs:111-124
			core[P] = ymean;
			core[P + 1] = pl ? 0.0 : en_nan();
			core[P + 2] = pl ? en_nan() : 0.0;
			core[P + 3] = pl ? en_nan() : cnt;
			core[P + 4] = pl ? cnt : 0.0;
		}
		return info;
	}
	// scaled moments: A (lower triangle used: A[i][j], j <= i), q; dead columns (constant) carry an identity row
	double A[P][P], q[P], z[P], w[P], dsc[P], xbar[P], lo[P], hi[P];
	unsigned freeM = 0, lowM = 0, upM = 0, liveM = 0;
#pragma unroll
	for (int i = 0; i < P; ++i) {
		const double si = rec[L::OFF_S + i];
		xbar[i] = (icpt ? rec[L::OFF_FIRST + i] : 0.0) + si / sw;
		const double cii = rec[L::q_index(i, i)] - (icpt ? si * si / sw : 0.0);
		const bool live = ((mask >> i) & 1u) && cii > 0.0;
		dsc[i] = live ? sqrt(cii) : 1.0;
		if (live) liveM |= 1u << i;
	}
#pragma unroll
	for (int i = 0; i < P; ++i) {
		const double si = rec[L::OFF_S + i];
		const bool li = (liveM >> i) & 1u;
#pragma unroll
		for (int j = 0; j < i; ++j) {
			const double v = rec[L::q_index(j, i)] - (icpt ? si * rec[L::OFF_S + j] / sw : 0.0);
			A[i][j] = (li && ((liveM >> j) & 1u)) ? v / (dsc[i] * dsc[j]) : 0.0;
		}
		A[i][i] = 1.0;
		const double ci = rec[L::q_index(i, P)] - (icpt ? si * sy / sw : 0.0);
		q[i] = li ? ci / dsc[i] : 0.0;
		lo[i] = bp.lo[i] * dsc[i]; // (+-inf stay themselves: dsc > 0)
		hi[i] = bp.hi[i] * dsc[i];
		z[i] = 0.0;
		if (li) {
			if (isfinite(bp.lo[i])) { z[i] = lo[i]; lowM |= 1u << i; }
			else if (isfinite(bp.hi[i])) { z[i] = hi[i]; upM |= 1u << i; }
			else freeM |= 1u << i;
		}
	}
	const double tss = icpt ? cyy_c : qyy;
	const double tau = kBlsKktTol * sqrt(tss);
	const int cap = bls_iteration_cap(P);
	const int max_it = bp.max_iterations < cap ? bp.max_iterations : cap;
	int iters = 0, passes = 0, jstar = -1;
	bool converged = false, inner = freeM != 0, first = false, star_low = false;
	unsigned blocked = 0;
	for (;;) {
#pragma unroll
		for (int i = 0; i < P; ++i) {
			double s = q[i];
#pragma unroll
			for (int j = 0; j < P; ++j) {
				if (j == i) s -= z[j];
				else s -= (j < i ? A[i][j] : A[j][i]) * z[j];
			}
			w[i] = ((liveM >> i) & 1u) ? s : 0.0;
		}
		if (!inner) {
			int best = -1;
			double bestv = tau;
#pragma unroll
			for (int j = 0; j < P; ++j) {
				const unsigned bit = 1u << j;
				if (blocked & bit) continue;
				const double v = (lowM & bit) ? w[j] : ((upM & bit) ? -w[j] : 0.0);
				if (v > bestv) { bestv = v; best = j; }
			}
			if (best < 0) { converged = true; break; }
			if (iters >= max_it) break;
			++iters;
			jstar = best;
			star_low = (lowM >> best) & 1u;
			freeM |= 1u << best;
			lowM &= ~(1u << best);
			upM &= ~(1u << best);
			inner = true;
			first = true;
			passes = 0;
		}
		// Cholesky of the free block (others: identity), inverse pivots on the diagonal of Lc
		double Lc[P][P], dl[P];
		bool bad = false;
#pragma unroll
		for (int j = 0; j < P; ++j) {
			const bool fj = (freeM >> j) & 1u;
			double dj = 1.0;
#pragma unroll
			for (int k = 0; k < j; ++k) dj -= Lc[j][k] * Lc[j][k];
			const bool ok = dj > kEnAliasTol;
			bad = bad || (fj && !ok);
			const double inv = ok ? 1.0 / sqrt(dj) : 0.0;
			Lc[j][j] = inv;
#pragma unroll
			for (int i = j + 1; i < P; ++i) {
				double t = (fj && ((freeM >> i) & 1u)) ? A[i][j] : 0.0;
#pragma unroll
				for (int k = 0; k < j; ++k) t -= Lc[i][k] * Lc[j][k];
				Lc[i][j] = t * inv;
			}
		}
		if (bad && first && jstar >= 0) { // collinear with the free columns: back to its bound, not chosen again for now
			const unsigned bit = 1u << jstar;
			freeM &= ~bit;
			if (star_low) lowM |= bit;
			else upM |= bit;
			blocked |= bit;
			inner = false;
			continue;
		}
#pragma unroll
		for (int j = 0; j < P; ++j) {
			double t = ((freeM >> j) & 1u) ? w[j] : 0.0;
#pragma unroll
			for (int k = 0; k < j; ++k) t -= Lc[j][k] * dl[k];
			dl[j] = t * Lc[j][j];
		}
#pragma unroll
		for (int j = P - 1; j >= 0; --j) {
			double t = dl[j];
#pragma unroll
			for (int i = j + 1; i < P; ++i) t -= Lc[i][j] * dl[i];
			dl[j] = t * Lc[j][j];
		}
		// the longest feasible fraction of the step
		double alpha = 1.0;
		int kmin = -1;
		bool kmin_low = false;
#pragma unroll
		for (int k = 0; k < P; ++k) {
			if (!((freeM >> k) & 1u)) continue;
			const double s = z[k] + dl[k];
			if (s < lo[k]) {
				const double a = fmax((lo[k] - z[k]) / dl[k], 0.0);
				if (a < alpha) { alpha = a; kmin = k; kmin_low = true; }
			} else if (s > hi[k]) {
				const double a = fmax((hi[k] - z[k]) / dl[k], 0.0);
				if (a < alpha) { alpha = a; kmin = k; kmin_low = false; }
			}
		}
#pragma unroll
		for (int k = 0; k < P; ++k) {
			const unsigned bit = 1u << k;
			if (!(freeM & bit)) continue;
			double zk = kmin < 0 ? z[k] + dl[k] : fma(alpha, dl[k], z[k]);
			const bool to_low = (k == kmin && kmin_low) || zk < lo[k];
			const bool to_up = !to_low && ((k == kmin && !kmin_low) || zk > hi[k]);
			if (to_low) { zk = lo[k]; freeM &= ~bit; lowM |= bit; }
			if (to_up) { zk = hi[k]; freeM &= ~bit; upM |= bit; }
			z[k] = zk;
		}
		first = false;
		++passes;
		if (kmin < 0 || passes > P) {
			inner = false;
			// a column that came straight back to the bound it left is not chosen again until the free set has changed
			const bool back = jstar >= 0 && (star_low ? ((lowM >> jstar) & 1u) : ((upM >> jstar) & 1u));
			blocked = back ? (blocked | (1u << jstar)) : 0u;
		}
	}
	// b = z / d, a held column exactly its bound; ssr = tss - z'(q + w) with w = q - A z of the final z
	double szqw = 0.0, b0 = ymean;
	int n_active = 0;
#pragma unroll
	for (int j = 0; j < P; ++j) {
		const unsigned bit = 1u << j;
		const bool live = liveM & bit;
		const double bj = (lowM & bit) ? bp.lo[j] : ((upM & bit) ? bp.hi[j] : z[j] / dsc[j]);
		szqw += z[j] * (q[j] + w[j]);
		if (live) b0 -= bj * xbar[j];
		const int f = live ? bls_flags(bj, bp.lo[j], bp.hi[j], bp.tolerance) : 0;
		n_active += f != 0 ? 1 : 0;
		core[j] = live ? bj : en_nan();
		if (!pl) {
			core[P + 6 + j] = f == 1 ? 1.0 : 0.0;
			core[2 * P + 6 + j] = f == 2 ? 1.0 : 0.0;
		}
	}
	core[P] = icpt ? b0 : en_nan();
	int32_t flag = 0;
	bls_write_stats(core, P, pl, tss - szqw, tss, cnt, n_active, icpt, &flag);
	info.iterations = iters;
	info.converged = converged;
	info.cancels = flag != 0;
	return info;
}

} // namespace anofox
