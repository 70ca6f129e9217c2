// solve_narrow_impl.h — the per-group solve of the narrow path (p <= 8), one lane per group.
//
// Shared by solve_narrow.hip (the solve kernels over moment records in HBM, and the refinement passes) and
// accumulate_narrow.hip (the fused accumulate + solve kernel, whose records sit in LDS).  The record and the core
// record are parameters: a global pointer for the kernels of solve_narrow.hip, an LDS pointer in the fused kernel.
// Both translation units compile it with the same flags and no fp-contract pragma, so the two instantiations round
// identically (tests/test_gpu_narrow_fused.py compares them bit for bit).
#pragma once

#include "common.h"
#include "device_math.h"

namespace anofox {
namespace {

constexpr double kAliasTol = 1e-11;   // pivot / original diagonal below this => column aliased (collinear)
constexpr double kAliasBand = 1e-13;  // ... and above this: not rounding noise — the refit applies the reference's rule
constexpr double kRefineTol = 1e-7;   // RSS / TSS below this => recompute RSS from residuals
constexpr double kPivotWarn = 1e-3;   // smallest pivot ratio below this => iterative refinement

__device__ __forceinline__ double nan64() { return __builtin_nan(""); }

enum { MODE_PRIMARY = 0, MODE_UPDATE = 1, MODE_FINAL = 2 };

// Group g from its moment record `rec` (MomentLayout<P>) into its core record `core` (p + 6 doubles); the inference
// record, the refinement vector and the refinement queue stay in HBM.  Returns whether the primary solve queued g.
// INF = false compiles the inference statistics out (the caller guarantees compute_inference is off): their special
// functions take ~245 registers at every p, more than a kernel that keeps two waves per SIMD can give them.
template <int P, int MODE, bool INF = true>
__device__ bool solve_one(const BatchArgs &args, int64_t g, const double *rec, double *core) {
	using L = MomentLayout<P>;
	constexpr int Z = L::Z;
	const int p = P;
	const bool icpt = args.fit_intercept != 0;
	const int model = args.model;

	double *inf = (INF && args.inference && args.compute_inference) ? args.inference + g * (int64_t)(5 * p + 2) : nullptr;
	const double *rv = args.refine_vec + g * (int64_t)refine_vec_len(p); // [rss, sum w r, X'Wr, centred yy] from residual_grad_wave

	int status = ANOFOX_ERROR_SUCCESS;
	double coef[P];
#pragma unroll
	for (int j = 0; j < P; ++j) coef[j] = nan64();
	double intercept = nan64(), r2 = nan64(), adj = nan64(), rse = nan64(), fstat = nan64(), fp = nan64();
	double nobs = nan64();
	bool has_inf = false;
	bool refine = false;

	const int64_t nrows = args.rule_counts ? args.rule_counts[g] : args.row_offsets[g + 1] - args.row_offsets[g];

	do {
		if (nrows < 2) { status = ANOFOX_HIP_STATUS_NULL_TOO_FEW_ROWS; break; }           // ols_aggregate.cpp:263-267
		if (model == ANOFOX_HIP_MODEL_RIDGE && args.alpha < 0.0) { status = ANOFOX_ERROR_INVALID_ALPHA; break; } // ridge.rs:38-40
		const double cnt = rec[L::OFF_CNT];
		if (!(cnt > 0.0)) { status = ANOFOX_ERROR_NO_VALID_DATA; break; }                 // ols.rs:68-70
		const double sw = rec[L::OFF_SW];
		const unsigned mask = (unsigned)rec[L::OFF_MASK];
		const int p_eff = __popc(mask);

		double s[Z], first[Z];
#pragma unroll
		for (int a = 0; a < Z; ++a) { s[a] = rec[L::OFF_S + a]; first[a] = rec[L::OFF_FIRST + a]; }
		const double qyy = rec[L::q_index(P, P)];
		// centred second moment of y about its (weighted) mean; the accumulate kernel shifts only when an
		// intercept is fitted, the identity holds either way
		const double cyy_centred = qyy - s[P] * s[P] / sw;
		const double ymean = (icpt ? first[P] : 0.0) + s[P] / sw;

		if (p_eff == 0) { // ols.rs:101-130, wls.rs:119-150
			if (!icpt) { status = ANOFOX_ERROR_INSUFFICIENT_DATA; break; }
			intercept = ymean;
			r2 = 0.0;
			adj = 0.0;
			rse = (model == ANOFOX_HIP_MODEL_WLS) ? sqrt(cyy_centred / sw) : sqrt(cyy_centred / (cnt - 1.0));
			nobs = cnt;
			break; // inference: None
		}
		if (cnt < (double)(p_eff + (icpt ? 1 : 0))) { status = ANOFOX_ERROR_INSUFFICIENT_DATA; break; } // ols.rs:132-139

		// moment matrix of the kept columns: centred when an intercept is fitted, raw otherwise
		double A[P][P]; // lower triangle used
		double c[P];
		bool active[P];
#pragma unroll
		for (int i = 0; i < P; ++i) {
			active[i] = (mask >> i) & 1u;
#pragma unroll
			for (int j = 0; j <= i; ++j) {
				const double qij = rec[L::q_index(j, i)];
				A[i][j] = icpt ? qij - s[i] * s[j] / sw : qij;
			}
			const double qiy = rec[L::q_index(i, P)];
			c[i] = icpt ? qiy - s[i] * s[P] / sw : qiy;
		}
		const double tss = icpt ? cyy_centred : qyy;

		double lam = 0.0, lam_rows = 0.0; // the penalty in the factor / the penalty the refinement aims at
		bool glmnet_cancels = false;
		if (model == ANOFOX_HIP_MODEL_RIDGE) {
			lam = args.alpha;
			if (args.lambda_scaling == ANOFOX_LAMBDA_SCALING_GLMNET) {
				// sd_y from the moments; a queued group's passes over the rows re-sum it about the mean (uncentred moments of
				// a nearly constant y cancel), and the refinement modes factor with and aim at that lambda (the standard errors
				// come from the same matrix: two nearly equal y values gave a lambda 3e-5 off and standard errors 1.6e-5 off)
				lam = cnt * args.alpha / sqrt(cyy_centred / cnt);
				glmnet_cancels = !icpt && !(cyy_centred * kGlmnetCancelRatio > qyy);
				if (MODE != MODE_PRIMARY && !icpt) lam_rows = cnt * args.alpha / sqrt(rv[p + 2] / cnt);
				else lam_rows = lam;
			} else {
				lam_rows = lam;
			}
#pragma unroll
			for (int i = 0; i < P; ++i) A[i][i] += (MODE == MODE_PRIMARY) ? lam : lam_rows; // the refinement modes factor with the re-summed lambda
		}

		// Cholesky (left-looking, in place), deactivating constant and aliased columns
		double diag0[P];
#pragma unroll
		for (int j = 0; j < P; ++j) diag0[j] = A[j][j];
		double min_ratio = 1.0;
		// (r4) a non-constant column dropped with a pivot above the rounding noise of the moments (1e-13 .. 1e-11 of the diagonal: sin of
		// its angle to the earlier columns 3e-7 .. 3e-6) may be one the reference's rule (remaining norm >= 1e-7 of the column's norm)
		// keeps: the group is queued, and the double-double refit decides with that rule (refit_dd.hip).  Exact copies and dummy-variable
		// traps leave a pivot of rounding noise (1e-16 .. 1e-13 of the diagonal) and are NOT queued: a batch in which every group carries
		// one must not pay the refinement passes for it (tests/test_gpu_parity.py::test_exactly_aliased_columns_are_not_queued).
		bool band = false;
#pragma unroll
		for (int j = 0; j < P; ++j) {
			double d = A[j][j];
#pragma unroll
			for (int k = 0; k < j; ++k) d -= A[j][k] * A[j][k];
			const bool ok = active[j] && (d > kAliasTol * diag0[j]) && (d > 0.0);
			band = band || (active[j] && !ok && d > kAliasBand * diag0[j]);
			active[j] = ok;
			if (ok) min_ratio = fmin(min_ratio, d / diag0[j]);
			const double ljj = ok ? sqrt(d) : 1.0;
			A[j][j] = ljj;
			const double inv = 1.0 / ljj;
#pragma unroll
			for (int i = j + 1; i < P; ++i) {
				double t = A[i][j];
#pragma unroll
				for (int k = 0; k < j; ++k) t -= A[i][k] * A[j][k];
				A[i][j] = ok ? t * inv : 0.0;
			}
			if (!ok) {
#pragma unroll
				for (int k = 0; k < j; ++k) A[j][k] = 0.0;
			}
		}
		int rank = 0;
#pragma unroll
		for (int j = 0; j < P; ++j) rank += active[j] ? 1 : 0;

		// L zf = rhs, L' x = zf
		auto solve_llt = [&](const double (&rhs)[P], double (&zf)[P], double (&x)[P]) {
#pragma unroll
			for (int i = 0; i < P; ++i) {
				double t = rhs[i];
#pragma unroll
				for (int k = 0; k < i; ++k) t -= A[i][k] * zf[k];
				zf[i] = active[i] ? t / A[i][i] : 0.0;
			}
#pragma unroll
			for (int i = P - 1; i >= 0; --i) {
				double t = zf[i];
#pragma unroll
				for (int k = i + 1; k < P; ++k) t -= A[k][i] * x[k];
				x[i] = active[i] ? t / A[i][i] : 0.0;
			}
		};

		double beta[P];
		double rss;
		if (MODE == MODE_PRIMARY) {
			double zf[P];
			solve_llt(c, zf, beta);
			double zz = 0.0, bc = 0.0, bb = 0.0;
#pragma unroll
			for (int i = 0; i < P; ++i) { zz += zf[i] * zf[i]; bc += beta[i] * c[i]; bb += beta[i] * beta[i]; }
			rss = (model == ANOFOX_HIP_MODEL_RIDGE) ? tss - bc - lam * bb : tss - zz;
			refine = !(rss > kRefineTol * tss) || (min_ratio < kPivotWarn) || glmnet_cancels || band;
			double bmax = 0.0;
#pragma unroll
			for (int i = 0; i < P; ++i) bmax = fmax(bmax, active[i] ? fabs(beta[i]) : 0.0);
#pragma unroll
			for (int i = 0; i < P; ++i) refine = refine || (active[i] && coef_bound_weak(beta[i], bmax, diag0[i], tss, min_ratio));
		} else {
			// current coefficients come from the record; residual_grad_wave used exactly these
#pragma unroll
			for (int i = 0; i < P; ++i) {
				const double b = core[i];
				beta[i] = active[i] ? b : 0.0;
			}
			rss = rv[0];
		}

		if (MODE == MODE_UPDATE) {
			// gradient of the (penalised) objective at beta, in centred coordinates
			const double gs = rv[1];
			double gc[P], u[P], delta[P];
#pragma unroll
			for (int i = 0; i < P; ++i) {
				double gi = rv[2 + i];
				if (icpt) gi -= (s[i] / sw) * gs;
				gc[i] = active[i] ? gi - lam_rows * beta[i] : 0.0;
			}
			solve_llt(gc, u, delta);
#pragma unroll
			for (int i = 0; i < P; ++i) beta[i] += delta[i];
		}

		const int n_par = rank + (icpt ? 1 : 0);
		const double df = cnt - (double)n_par;
		const double dfm = (double)rank;

		double b0 = 0.0;
		if (icpt) {
			b0 = ymean;
#pragma unroll
			for (int i = 0; i < P; ++i) b0 -= beta[i] * (first[i] + s[i] / sw);
			intercept = b0;
		}
#pragma unroll
		for (int i = 0; i < P; ++i) coef[i] = active[i] ? beta[i] : nan64();
		if (MODE == MODE_UPDATE) { // only the coefficients change in this pass
#pragma unroll
			for (int j = 0; j < P; ++j) core[j] = coef[j];
			core[p] = intercept;
			return false;
		}
		r2 = 1.0 - rss / tss;
		adj = 1.0 - (1.0 - r2) * (cnt - (icpt ? 1.0 : 0.0)) / df;
		rse = sqrt(rss / df);
		nobs = cnt;
		fstat = ((tss - rss) / dfm) / (rss / df);

		if (inf) {
			has_inf = true;
			fp = dm_f_sf(fstat, dfm, df);
			const double sigma2 = rss / df;
			const double tcrit = dm_tcrit_cached(static_cast<TcritSlot *>(args.tcrit_table), 0.5 * (1.0 + args.confidence_level), df);
			// diag of (L L')^-1 through the columns of L^-1
#pragma unroll
			for (int j = 0; j < P; ++j) {
				double wcol[P];
				double dj = 0.0;
#pragma unroll
				for (int i = j; i < P; ++i) {
					double t = (i == j) ? 1.0 : 0.0;
#pragma unroll
					for (int k = j; k < i; ++k) t -= A[i][k] * wcol[k];
					wcol[i] = active[i] ? t / A[i][i] : 0.0;
					dj += wcol[i] * wcol[i];
				}
				// (written as they come: five arrays of P held to the end took 80 registers, and the fused accumulate kernel
				// that inlines this solve has 256 in all)
				double se = nan64(), tv = nan64(), pv = nan64(), cl = nan64(), cu = nan64();
				if (active[j]) {
					se = sqrt(sigma2 * dj);
					tv = beta[j] / se;
					pv = dm_t_two_sided_p(tv, df);
					cl = beta[j] - tcrit * se;
					cu = beta[j] + tcrit * se;
				}
				inf[j] = se;
				inf[p + j] = tv;
				inf[2 * p + j] = pv;
				inf[3 * p + j] = cl;
				inf[4 * p + j] = cu;
			}
			inf[5 * p] = fstat;
			inf[5 * p + 1] = fp;
		}
	} while (false);

	if (MODE == MODE_UPDATE) return false; // queued groups always have status 0; nothing else to write

	if (status != ANOFOX_ERROR_SUCCESS) {
#pragma unroll
		for (int j = 0; j < P; ++j) coef[j] = nan64();
		intercept = r2 = adj = rse = nobs = nan64();
	}
#pragma unroll
	for (int j = 0; j < P; ++j) core[j] = coef[j];
	core[p] = intercept;
	core[p + 1] = r2;
	core[p + 2] = adj;
	core[p + 3] = rse;
	core[p + 4] = nobs;
	core[p + 5] = (double)status;
	if (inf && !has_inf) {
#pragma unroll
		for (int k = 0; k < 5 * P + 2; ++k) inf[k] = nan64();
	}
	if (MODE == MODE_PRIMARY && refine && status == ANOFOX_ERROR_SUCCESS) {
		const int slot = atomicAdd(args.refine_count, 1);
		args.refine_list[slot] = (int32_t)g;
		return true;
	}
	return false;
}

} // namespace
} // namespace anofox
