// aft_newton.h — the accelerated failure time (AFT) fit of one group of rows with right censoring: Newton's iteration on the
// censored log-likelihood in theta = (intercept?, beta[p], log sigma?), the loop of the reference's newton()
// (crates/anofox-stats-core/src/models/aft.rs) restated.  DESIGN.md §1, "Accelerated failure time models".
//
//     log T = a'beta + sigma W,   z_i = (log t_i - a_i'beta) / sigma,   a_i = (1, x_i) or x_i,
//     l(theta) = sum_{event} [log f_W(z_i) - log sigma - log t_i] + sum_{censored} log S_W(z_i),
//     k = p + [intercept] + [scale estimated] <= 34;  W: extreme value (Weibull; exponential with sigma = 1), normal, logistic.
//
// One source for both builds, with the lanes, the reductions, the Cholesky factorisation and the back substitution of
// glm_irls.h: under hipcc device code run by ONE WAVEFRONT, under a plain C++ compiler a loop over 64 lanes that adds every sum
// in the same order (tests/tools/aft_host.cpp).
//
//   rows       strided over the lanes.  log t of a row sits in a scratch of one double per row that only the lane that owns
//              the row touches; NaN marks a row that is not valid.  The first pass writes it before anything reads it.
//   start      beta = the least-squares fit of log t on the design (normal equations, Cholesky in LDS; an aliased column
//              starts at 0), log sigma = ln sqrt(max(RSS / max(n - k_beta, 1), 1e-8)); exponential: log sigma = 0, no parameter.
//   iteration  one pass over the rows gives l, the gradient g and -H.  With u, v the first and second derivative of a row's
//              term in z and b_i = (a_i / sigma, z_i):  g = sum -u b (- the events, log sigma),  -H = sum (-v) b b' - the u terms
//              of the log sigma row and column, which are g's own sums (-H[beta, s] += g[beta], -H[s, s] += sum -u z).  The
//              sums are the lower triangle of an augmented matrix whose last row is g, (k + 1)(k + 2) / 2 of them (630 at
//              k = 34), by LANES OVER MATRIX ENTRIES ON A ROW TILE STAGED IN LDS as glm_irls.h has it: a lane owns up to EM
//              entries in registers; with 64 entries or fewer the lanes split into row slices that meet in a butterfly.
//   solve      (-H) s = g by Cholesky in LDS, g carried as row k.  -H not positive definite (a pivot not above 1e-10 of its
//              diagonal entry), g's <= 0 or not finite: the Levenberg ladder, diagonal d + damping max(|d|, 1), damping 1e-3,
//              x 10 per rung, 20 rungs at most (-H is kept in the tile's memory meanwhile); then s = g / max|g|.
//   stopping   g's / 2 < tolerance (1 + |l|): converged; the step s just solved for is still taken when l(theta + s) >= l - 1e-12
//              (one more likelihood pass: the distance to the mode squared).  Otherwise theta + f s, f = 1, 1/2, .. (30 halvings at
//              most, one likelihood-only pass each), the first trial with l_trial >= l - 1e-12 is taken; a full step that
//              moves l by less than tolerance (1 + |l_trial|) converges; an exhausted search stops with converged =
//              (max|g| < 1e-4).  l is summed lane by lane and through the same butterfly in both passes: equal theta, equal bits.
//   clamps     extreme value: exp(z) with z clamped to [-700, 700].  logistic: exp(-|z|) only.  normal: log S and the hazard
//              from erfc(z / sqrt 2); where that falls below 1e-300 the Mills-ratio expansion (z + 1/z - 2/z^3).
//   finish     the same wavefront writes the record, inverts -H at the mode for the standard errors (lane j solves L v = e_j)
//              and fits the intercept-only model for null_log_likelihood.
//   predict    (P.pred given) after all that, one more walk over the group's rows, strided over the lanes as in the likelihood
//              pass: per row four doubles {eta, time_quantile, cdf, risk} at pred[4 i], from beta and sigma still in the work
//              memory (an_predict).  A row is scored whether or not it was in the fit; only its x must be finite.
#pragma once
#include "glm_irls.h"

namespace anofox {
namespace aft {

using namespace anofox::glm;

constexpr int kAnMaxP = 32; // features at most (k <= 34)
constexpr int kAnWeibull = 0, kAnLogNormal = 1, kAnLogLogistic = 2, kAnExponential = 3;
constexpr int kAnMaxHalvings = 30;
constexpr int kAnMaxRungs = 20;
constexpr double kAnZClamp = 700.0;
constexpr double kAnSurvivalFloor = 1e-300; // below it the normal kernel takes the Mills-ratio expansion

GI_HD int an_aug_ld(int k) { return (k + 1) | 1; }
GI_HD int an_tile_ld(int k) { return (k + 3) | 1; } // b[k], 1, -v, -u
// doubles of work memory (LDS on the device): the augmented matrix, the row tile (which also keeps -H during the damping
// ladder and the columns of the inverse), theta / step / gradient / trial / diag
GI_HD size_t an_work_doubles(int k) { return (size_t)(k + 1) * an_aug_ld(k) + 64 * (size_t)an_tile_ld(k) + 5 * (size_t)(k + 1); }
GI_HD int an_entries_per_lane(int k) { return ((k + 1) * (k + 2) / 2 + 63) / 64; }
// the template parameter a fit of k parameters needs: 1 (k <= 9), 4 (k <= 21) or 10
GI_HD int an_entry_class(int k) {
	const int e = an_entries_per_lane(k);
	return e <= 1 ? 1 : (e <= 4 ? 4 : 10);
}
GI_HD bool an_scale_is_fixed(int dist) { return dist == kAnExponential; }

struct AnProblem {
	const double *time;
	const double *event;
	const double *const *x; // p column pointers
	int p;
	int fit_intercept;
	int dist;
	int64_t lo, hi; // rows [lo, hi) of the columns
	int max_iterations;
	double tolerance;
	int compute_inference;
	double zq;    // the normal quantile of the confidence level
	double *logt; // scratch, one double per row, indexed by the row number
	// measurements (tests/tools/aft_host.cpp): Newton iterations that entered the damping ladder, main and null fit together
	int *ladder_entries = nullptr;
	// the prediction pass (an_predict); pred == nullptr: no pass
	double *pred = nullptr; // four doubles per row, indexed by the row number
	double wq = NAN;        // the quantile of W that time_quantile is taken at
	double horizon = NAN;   // NaN: risk is not asked for
};

// a model the loop fits: the group's own (the design a_i) or the intercept-only one (the design 1)
struct AnModel {
	int kb;    // coefficients
	int fs;    // 1: log sigma is the last parameter
	bool null; // the intercept-only model
};

GI_DEV double an_elem(const AnProblem &P, const AnModel &M, int c, int64_t i) {
	if (M.null) return 1.0;
	if (P.fit_intercept) return c == 0 ? 1.0 : P.x[c - 1][i];
	return P.x[c][i];
}

GI_DEV double an_eta(const AnProblem &P, const AnModel &M, const double *theta, int64_t i) {
	double eta = 0.0;
	GI_NOUNROLL
	for (int c = 0; c < M.kb; ++c) eta += an_elem(P, M, c, i) * theta[c];
	return eta;
}

GI_DEV double an_safe_exp(double z) { return exp(z > kAnZClamp ? kAnZClamp : (z < -kAnZClamp ? -kAnZClamp : z)); }

// A row's term in z: c = log f_W(z) (event) or log S_W(z) (censored), u = dc/dz, v = d2c/dz2 (v <= 0: the kernels are log-concave)
GI_DEV void an_row_terms(int dist, bool event, double z, double &c, double &u, double &v) {
	if (dist == kAnLogNormal) {
		if (event) {
			c = -0.5 * z * z - 0.91893853320467274178; // log sqrt(2 pi)
			u = -z;
			v = -1.0;
			return;
		}
		const double s = 0.5 * erfc(z * 0.70710678118654752440);
		double r; // the hazard phi / S
		if (s > kAnSurvivalFloor) {
			c = log(s);
			r = exp(-0.5 * z * z) * 0.39894228040143267794 / s;
		} else {
			c = -0.5 * z * z - log(z * 2.50662827463100050242);
			r = z + 1.0 / z - 2.0 / (z * z * z);
		}
		u = -r;
		v = r * (z - r);
		return;
	}
	if (dist == kAnLogLogistic) {
		const double e = exp(-fabs(z)), d = 1.0 + e, l1 = log1p(e);
		const double big = 1.0 / d, small = e / d;
		const bool pos = z >= 0.0;
		const double pr = pos ? big : small, q = pos ? small : big; // logistic(z) and 1 - logistic(z)
		const double sp = pos ? z + l1 : l1;                         // log(1 + e^z)
		if (event) {
			c = z - 2.0 * sp;
			u = q - pr; // 1 - 2 logistic(z)
			v = -2.0 * pr * q;
		} else {
			c = -sp;
			u = -pr;
			v = -pr * q;
		}
		return;
	}
	const double e = an_safe_exp(z); // Weibull and exponential: the extreme value kernel
	if (event) {
		c = z - e;
		u = 1.0 - e;
	} else {
		c = -e;
		u = -e;
	}
	v = -e;
}

GI_DEV void an_fail(double *rec, double *inf, int p, int status) {
	GI_LANES_BEGIN(lane)
	for (int j = lane; j < p + 12; j += 64) rec[j] = NAN;
	if (lane == 0) rec[p + 12] = (double)status;
	if (inf)
		for (int j = lane; j < 5 * p + 2; j += 64) inf[j] = NAN;
	GI_LANES_END
}

// l(theta) over the valid rows; -inf when sigma is not a positive finite number
GI_DEV double an_loglik(const AnProblem &P, const AnModel &M, const double *theta) {
	const double logsig = M.fs ? theta[M.kb] : 0.0, sigma = exp(logsig);
	if (!(gi_finite(sigma) && sigma > 0.0)) return -INFINITY;
	GiPL<double> part;
	GI_LANES_BEGIN(lane)
	double s = 0.0;
	for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
		const double lt = P.logt[i];
		if (!(lt == lt)) continue;
		const double z = (lt - an_eta(P, M, theta, i)) / sigma;
		const bool ev = P.event[i] == 1.0;
		double c, u, v;
		an_row_terms(P.dist, ev, z, c, u, v);
		s += ev ? c - logsig - lt : c;
	}
	part.v[GI_AT(lane)] = s;
	GI_LANES_END
	return gi_sum(part);
}

// which entries (a >= b) of the augmented matrix of kk parameters each lane owns; S row slices of Tp lanes
template <int EM>
GI_DEV void an_map(int kk, GiPL<GiEntries<EM>> &map, int &S, int &Tp) {
	const int T = (kk + 1) * (kk + 2) / 2;
	Tp = 64;
	S = 1;
	if (T <= 64 && EM == 1) {
		Tp = 1;
		while (Tp < T) Tp <<= 1;
		S = 64 / Tp;
	}
	GI_LANES_BEGIN(lane)
	GiEntries<EM> &m = map.v[GI_AT(lane)];
	for (int j = 0; j < EM; ++j) {
		const int e = (S > 1 ? (lane & (Tp - 1)) : lane) + 64 * j;
		if (e < T && (S == 1 || j == 0)) {
			int a = 0;
			while ((a + 1) * (a + 2) / 2 <= e) ++a;
			m.a[j] = a;
			m.b[j] = e - a * (a + 1) / 2;
		} else {
			m.a[j] = -1;
			m.b[j] = 0;
		}
	}
	GI_LANES_END
}

constexpr int kAnSumsNewton = 0, kAnSumsStart = 1;

// One pass over the rows -> the augmented matrix in aug (lower triangle; row kk = the right-hand side).
//   kAnSumsNewton: -H and g of l at theta; returns l (non-finite when sigma is not a positive finite number).
//   kAnSumsStart:  the normal equations of log t on the design (the log sigma slot zero); returns 0.
template <int EM>
GI_DEV double an_sums(const AnProblem &P, const AnModel &M, int what, const double *theta, int64_t n_events, double *aug, double *tile,
                      GiPL<GiEntries<EM>> &map, int S, int Tp) {
	const int kb = M.kb, kk = kb + M.fs, ld = an_aug_ld(kk), tl = an_tile_ld(kk);
	const bool newton = what == kAnSumsNewton;
	const double logsig = newton && M.fs ? theta[kb] : 0.0, sigma = exp(logsig), rs = 1.0 / sigma;
	if (newton && !(gi_finite(sigma) && sigma > 0.0 && gi_finite(rs))) return -INFINITY;
	GiPL<GiAcc<EM>> acc;
	GiPL<double> llp;
	GI_LANES_BEGIN(lane)
	(void)lane;
	for (int j = 0; j < EM; ++j) acc.v[GI_AT(lane)].v[j] = 0.0;
	llp.v[GI_AT(lane)] = 0.0;
	GI_LANES_END
	for (int64_t base = P.lo; base < P.hi; base += 64) {
		const int nr = P.hi - base < 64 ? (int)(P.hi - base) : 64;
		GI_LANES_BEGIN(lane)
		const int64_t i = base + lane;
		double *row = tile + lane * tl;
		const double lt = lane < nr ? P.logt[i] : NAN;
		if (lt == lt) {
			if (newton) {
				const double z = (lt - an_eta(P, M, theta, i)) / sigma;
				const bool ev = P.event[i] == 1.0;
				double c, u, v;
				an_row_terms(P.dist, ev, z, c, u, v);
				llp.v[GI_AT(lane)] += ev ? c - logsig - lt : c;
				GI_NOUNROLL
				for (int cc = 0; cc < kb; ++cc) row[cc] = an_elem(P, M, cc, i) * rs;
				if (M.fs) row[kb] = z;
				row[kk + 1] = -v;
				row[kk + 2] = -u;
			} else {
				GI_NOUNROLL
				for (int cc = 0; cc < kb; ++cc) row[cc] = an_elem(P, M, cc, i);
				if (M.fs) row[kb] = 0.0;
				row[kk + 1] = 1.0;
				row[kk + 2] = lt;
			}
			row[kk] = 1.0;
		} else {
			GI_NOUNROLL
			for (int cc = 0; cc < kk + 3; ++cc) row[cc] = 0.0;
		}
		GI_LANES_END
		gi_sync();
		GI_LANES_BEGIN(lane)
		const GiEntries<EM> &m = map.v[GI_AT(lane)];
		GiAcc<EM> &s = acc.v[GI_AT(lane)];
		for (int r = S > 1 ? lane / Tp : 0; r < nr; r += S) {
			const double *row = tile + r * tl;
			const double wh = row[kk + 1], wg = row[kk + 2];
GI_UNROLL
			for (int j = 0; j < EM; ++j) s.v[j] += (m.a[j] == kk ? wg : wh) * row[m.a[j] < 0 ? 0 : m.a[j]] * row[m.b[j]];
		}
		GI_LANES_END
		gi_sync();
	}
	double total = 0.0;
	if (EM == 1 && S > 1) { // the slices' partial sums meet over the lane bits >= Tp
		GiPL<double> part;
		GI_LANES_BEGIN(lane)
		(void)lane;
		part.v[GI_AT(lane)] = acc.v[GI_AT(lane)].v[0];
		GI_LANES_END
#if defined(__HIPCC__)
		total = gi_sum(part, Tp);
#else
		(void)total;
		gi_sum(part, Tp);
		for (int lane = 0; lane < 64; ++lane) acc.v[lane].v[0] = part.v[lane];
#endif
	}
	GI_LANES_BEGIN(lane)
	const GiEntries<EM> &m = map.v[GI_AT(lane)];
	if (S == 1 || lane < Tp) {
		for (int j = 0; j < EM; ++j) {
			const int a = m.a[j], b = m.b[j];
			if (a < 0) continue;
#if defined(__HIPCC__)
			const double v = (EM == 1 && S > 1) ? total : acc.v[0].v[j];
#else
			const double v = acc.v[lane].v[j];
#endif
			aug[a * ld + b] = v;
		}
	}
	GI_LANES_END
	gi_sync();
	if (newton && M.fs) { // the u terms of the log sigma row are the gradient's own sums; then the events leave g[log sigma]
		GI_LANES_BEGIN(lane)
		if (lane <= kb) aug[kb * ld + lane] += aug[kk * ld + lane];
		GI_LANES_END
		gi_sync();
		GI_LANES_BEGIN(lane)
		if (lane == 0) aug[kk * ld + kb] -= (double)n_events;
		GI_LANES_END
		gi_sync();
	}
	return newton ? gi_sum(llp) : 0.0;
}

// (-H + damping) s = g from the copy of the augmented matrix in `keep` -> g's, NaN when the matrix is not positive definite
GI_DEV double an_solve(double *aug, const double *keep, int ld, int kk, double damping, double *diag0, double *step) {
	GI_LANES_BEGIN(lane)
	for (int e = lane; e < (kk + 1) * ld; e += 64) {
		const int r = e / ld, c = e - r * ld;
		double v = keep[e];
		if (r == c && r < kk && damping > 0.0) v += damping * (fabs(v) > 1.0 ? fabs(v) : 1.0);
		aug[e] = v;
	}
	GI_LANES_END
	gi_sync();
	if (gi_cholesky(aug, ld, kk, kk + 1, 0, diag0) != 0) return NAN;
	gi_back_substitute(aug, ld, kk, 0, step);
	double d = 0.0;
	for (int j = 0; j < kk; ++j) d += keep[kk * ld + j] * step[j];
	return d;
}

// The Newton loop of one model.  -> 0 and theta (kk values in work's theta slot), l, the iterations; or a status.
template <int EM>
GI_DEV int an_newton(const AnProblem &P, const AnModel &M, int64_t n_valid, int64_t n_events, double *work, int k_main, double &ll_out,
                     int &iterations_out) {
	const int kb = M.kb, kk = kb + M.fs, ld = an_aug_ld(kk);
	double *aug = work, *tile = aug + (size_t)(k_main + 1) * an_aug_ld(k_main), *theta = tile + 64 * (size_t)an_tile_ld(k_main),
	       *step = theta + (k_main + 1), *grad = step + (k_main + 1), *trial = grad + (k_main + 1), *diag0 = trial + (k_main + 1);
	GiPL<GiEntries<EM>> map;
	int S, Tp;
	an_map<EM>(kk, map, S, Tp);
	// (theta is written at [0, kk) only, here and at every accepted step: an_fit's prediction pass relies on that when it saves
	// and restores what the intercept-only fit, kk <= 2, overwrites)
	// ---- the start: least squares of log t, then log sigma from its residuals ----
	an_sums<EM>(P, M, kAnSumsStart, theta, n_events, aug, tile, map, S, Tp);
	{
		const uint64_t alias = gi_cholesky(aug, ld, kk, kk + 1, M.fs ? 1ull << kb : 0ull, diag0);
		gi_back_substitute(aug, ld, kk, alias, theta);
	}
	if (M.fs) {
		GiPL<double> part;
		GI_LANES_BEGIN(lane)
		double s = 0.0;
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			const double lt = P.logt[i];
			if (!(lt == lt)) continue;
			const double r = lt - an_eta(P, M, theta, i);
			s += r * r;
		}
		part.v[GI_AT(lane)] = s;
		GI_LANES_END
		const double rss = gi_sum(part), df = (double)(n_valid - kb > 1 ? n_valid - kb : 1), var = rss / df;
		gi_sync();
		GI_LANES_BEGIN(lane)
		if (lane == 0) theta[kb] = log(sqrt(var > 1e-8 ? var : 1e-8));
		GI_LANES_END
		gi_sync();
	}
	// ---- the loop ----
	bool converged = false;
	int iterations = 0;
	double ll = -INFINITY;
	for (int it = 0; it < P.max_iterations && !converged; ++it) {
		iterations = it + 1;
		const double cur = an_sums<EM>(P, M, kAnSumsNewton, theta, n_events, aug, tile, map, S, Tp);
		if (!gi_finite(cur)) return kGiStatusConvergence;
		double gmax = 0.0;
		GI_LANES_BEGIN(lane)
		for (int e = lane; e < (kk + 1) * ld; e += 64) tile[e] = aug[e];
		if (lane < kk) grad[lane] = aug[kk * ld + lane];
		GI_LANES_END
		gi_sync();
		for (int j = 0; j < kk; ++j)
			if (!(fabs(grad[j]) <= gmax)) gmax = fabs(grad[j]); // (a NaN sticks)
		double dec = an_solve(aug, tile, ld, kk, 0.0, diag0, step);
		if (!(gi_finite(dec) && dec > 0.0)) {
			if (P.ladder_entries) {
				GI_LANES_BEGIN(lane)
				if (lane == 0) ++*P.ladder_entries;
				GI_LANES_END
			}
			double damping = 1e-3;
			for (int rung = 0; rung < kAnMaxRungs; ++rung) {
				dec = an_solve(aug, tile, ld, kk, damping, diag0, step);
				if (gi_finite(dec) && dec > 0.0) break;
				damping *= 10.0;
			}
			if (!(gi_finite(dec) && dec > 0.0)) { // no ascent direction under any damping: normalised steepest ascent
				const double gnorm = gmax > 1e-300 ? gmax : 1e-300;
				gi_sync();
				GI_LANES_BEGIN(lane)
				if (lane < kk) step[lane] = grad[lane] / gnorm;
				GI_LANES_END
				gi_sync();
				dec = 0.0;
				for (int j = 0; j < kk; ++j) dec += grad[j] * step[j];
			}
		}
		if (gi_finite(dec) && 0.5 * fabs(dec) < P.tolerance * (1.0 + fabs(cur))) {
			// converged where it stands.  The step the test has just paid for is still taken when it passes the line search's
			// own acceptance: it squares the distance to the mode at the price of one likelihood pass
			ll = cur;
			converged = true;
			gi_sync();
			GI_LANES_BEGIN(lane)
			if (lane < kk) trial[lane] = theta[lane] + step[lane];
			GI_LANES_END
			gi_sync();
			const double tll = an_loglik(P, M, trial);
			if (gi_finite(tll) && tll >= cur - 1e-12) {
				gi_sync();
				GI_LANES_BEGIN(lane)
				if (lane < kk) theta[lane] = trial[lane];
				GI_LANES_END
				gi_sync();
				ll = tll;
			}
			break;
		}
		double factor = 1.0;
		bool accepted = false;
		for (int h = 0; h < kAnMaxHalvings; ++h) {
			gi_sync();
			GI_LANES_BEGIN(lane)
			if (lane < kk) trial[lane] = theta[lane] + factor * step[lane];
			GI_LANES_END
			gi_sync();
			const double tll = an_loglik(P, M, trial);
			if (gi_finite(tll) && tll >= cur - 1e-12) {
				gi_sync();
				GI_LANES_BEGIN(lane)
				if (lane < kk) theta[lane] = trial[lane];
				GI_LANES_END
				gi_sync();
				ll = tll;
				accepted = true;
				if (factor == 1.0 && fabs(tll - cur) / (1.0 + fabs(tll)) < P.tolerance) converged = true;
				break;
			}
			factor *= 0.5;
		}
		if (!accepted) {
			ll = cur;
			converged = gmax < 1e-4;
			break;
		}
	}
	if (!converged) return kGiStatusConvergence;
	ll_out = ll;
	iterations_out = iterations;
	return 0;
}

// P(W <= z) with the clamps of an_row_terms
GI_DEV double an_kernel_cdf(int dist, double z) {
	if (dist == kAnLogNormal) return 0.5 * erfc(-z * 0.70710678118654752440);
	if (dist == kAnLogLogistic) {
		const double e = exp(-fabs(z));
		return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
	}
	return -expm1(-an_safe_exp(z));
}

// The prediction pass of one group: pred[4 i ..] = {eta, time_quantile, cdf, risk} of every row i of [lo, hi), all NaN when the
// fit failed (status != 0) or an x of the row is not finite.  theta: the fitted parameters.  A lane writes its own rows only.
//   eta            a_i'beta by an_eta: for a row of the fit, the bits the last likelihood pass saw
//   time_quantile  exp(eta + sigma wq)
//   cdf            P(T <= t_i): 0 for a finite t_i <= 0, NaN for a t_i that is not finite
//   risk           P(T <= t_i + h | T > t_i) = -expm1(log S(z(t_i + h)) - log S(z(t_i))), the log-survival terms being those of a
//                  censored row (an_row_terms), so a survival that underflows still gives its ratio; t_i <= 0: the cdf at
//                  t_i + h; NaN without a horizon or for a t_i that is not finite
GI_DEV void an_predict(const AnProblem &P, int status, const double *theta) {
	const int p = P.p, kb = p + (P.fit_intercept ? 1 : 0), fs = an_scale_is_fixed(P.dist) ? 0 : 1;
	const AnModel M = {kb, fs, false};
	const double sigma = status == 0 && fs ? exp(theta[kb]) : 1.0; // (the record's scale)
	const bool ask_risk = P.horizon == P.horizon;
	GI_LANES_BEGIN(lane)
	for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
		double *out = P.pred + 4 * i;
		bool ok = status == 0;
		GI_NOUNROLL
		for (int j = 0; ok && j < p; ++j) ok = gi_finite(P.x[j][i]);
		double eta = NAN, tq = NAN, cdf = NAN, risk = NAN;
		if (ok) {
			eta = an_eta(P, M, theta, i);
			tq = exp(eta + sigma * P.wq);
			const double t = P.time[i];
			if (gi_finite(t)) {
				const double t2 = t + P.horizon;
				if (t > 0.0) {
					const double z = (log(t) - eta) / sigma;
					cdf = an_kernel_cdf(P.dist, z);
					if (ask_risk) {
						double c1, c2, u, v;
						an_row_terms(P.dist, false, z, c1, u, v);
						an_row_terms(P.dist, false, (log(t2) - eta) / sigma, c2, u, v);
						risk = 0.0 - expm1(c2 - c1);
					}
				} else {
					cdf = 0.0;
					if (ask_risk) risk = t2 > 0.0 ? an_kernel_cdf(P.dist, (log(t2) - eta) / sigma) : 0.0;
				}
			}
		}
		out[0] = eta;
		out[1] = tq;
		out[2] = cdf;
		out[3] = risk;
	}
	GI_LANES_END
}

// The fit of one group.  rec: p + 13 doubles {b[p], intercept, scale, log_likelihood, null_log_likelihood, aic, bic,
// n_observations, n_events, n_censored, n_params, iterations, converged, status}; inf (optional): 5 p + 2 doubles {se[p], z[p],
// p[p], ci_lower[p], ci_upper[p], intercept_std_error, log_scale_std_error}.
template <int EM>
GI_DEV void an_fit(const AnProblem &P, bool invalid, double *work, double *rec, double *inf) {
	const int p = P.p, ic = P.fit_intercept ? 1 : 0, fs = an_scale_is_fixed(P.dist) ? 0 : 1, kb = p + ic, k = kb + fs;
	if (invalid) {
		an_fail(rec, inf, p, kGiStatusInvalidInput);
		if (P.pred) an_predict(P, kGiStatusInvalidInput, nullptr);
		return;
	}
	// ---- first pass: the row mask, log t, the counts ----
	int64_t n_valid, n_events, n_bad;
	{
		GiPL<int64_t> cnt, evs, bad;
		GI_LANES_BEGIN(lane)
		int64_t c = 0, e = 0, b = 0;
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			const double t = P.time[i], d = P.event[i];
			bool ok = gi_finite(t) && gi_finite(d);
			GI_NOUNROLL
			for (int j = 0; ok && j < p; ++j) ok = gi_finite(P.x[j][i]);
			if (ok && (!(t > 0.0) || (d != 0.0 && d != 1.0))) {
				++b;
				ok = false;
			}
			P.logt[i] = ok ? log(t) : NAN;
			if (ok) {
				++c;
				e += d == 1.0 ? 1 : 0;
			}
		}
		cnt.v[GI_AT(lane)] = c;
		evs.v[GI_AT(lane)] = e;
		bad.v[GI_AT(lane)] = b;
		GI_LANES_END
		n_valid = gi_sum_i(cnt);
		n_events = gi_sum_i(evs);
		n_bad = gi_sum_i(bad);
	}
	int status = 0;
	if (n_bad > 0) status = kGiStatusInvalidInput;
	else if (n_valid == 0) status = kGiStatusNoValidData;
	else if (n_events == 0) status = kGiStatusInvalidInput; // every row censored: the model is not identified
	else if (n_valid < k + 1) status = kGiStatusInsufficientData;
	double ll = NAN;
	int iterations = 0;
	if (!status) {
		const AnModel M = {kb, fs, false};
		status = an_newton<EM>(P, M, n_valid, n_events, work, k, ll, iterations);
	}
	if (status) {
		an_fail(rec, inf, p, status);
		if (P.pred) an_predict(P, status, nullptr);
		return;
	}
	const int ld = an_aug_ld(k), tl = an_tile_ld(k);
	double *aug = work, *tile = aug + (size_t)(k + 1) * ld, *theta = tile + 64 * (size_t)tl, *diag0 = theta + 4 * (k + 1);
	// ---- inference: the diagonal of (-H)^-1 at the mode ----
	if (inf) {
		uint64_t alias = 0;
		if (P.compute_inference) {
			GiPL<GiEntries<EM>> map;
			int S, Tp;
			an_map<EM>(k, map, S, Tp);
			const AnModel M = {kb, fs, false};
			an_sums<EM>(P, M, kAnSumsNewton, theta, n_events, aug, tile, map, S, Tp);
			alias = gi_cholesky(aug, ld, k, k, 0, diag0);
		}
		GI_LANES_BEGIN(lane)
		if (lane < k) { // lane j: parameter j
			const int j = lane;
			double se = NAN;
			if (P.compute_inference && !((alias >> j) & 1)) {
				double *v = tile + lane * tl, ss = 0.0;
				for (int i = j; i < k; ++i) {
					if ((alias >> i) & 1) { v[i] = 0.0; continue; }
					double a = i == j ? 1.0 : 0.0;
					for (int c = j; c < i; ++c)
						if (!((alias >> c) & 1)) a -= aug[i * ld + c] * v[c];
					v[i] = a / aug[i * ld + i];
					ss += v[i] * v[i];
				}
				se = gi_finite(ss) && ss >= 0.0 ? sqrt(ss) : NAN;
			}
			if (j >= ic && j < kb) {
				const int f = j - ic;
				const double b = theta[j], z = b / se;
				inf[f] = se;
				inf[p + f] = z;
				inf[2 * p + f] = erfc(fabs(z) * 0.70710678118654752440);
				inf[3 * p + f] = b - P.zq * se;
				inf[4 * p + f] = b + P.zq * se;
			}
			if (ic && j == 0) inf[5 * p] = se;
			if (fs && j == kb) inf[5 * p + 1] = se;
		}
		if (lane == 0) {
			if (!ic) inf[5 * p] = NAN;
			if (!fs) inf[5 * p + 1] = NAN;
		}
		GI_LANES_END
		gi_sync();
	}
	// ---- the record (null_log_likelihood after the intercept-only fit) ----
	GI_LANES_BEGIN(lane)
	if (lane < p) rec[lane] = theta[lane + ic];
	if (lane == 0) {
		rec[p] = ic ? theta[0] : NAN;
		rec[p + 1] = fs ? exp(theta[kb]) : 1.0;
		rec[p + 2] = ll;
		rec[p + 4] = 2.0 * (double)k - 2.0 * ll;
		rec[p + 5] = (double)k * log((double)n_valid) - 2.0 * ll;
		rec[p + 6] = (double)n_valid;
		rec[p + 7] = (double)n_events;
		rec[p + 8] = (double)(n_valid - n_events);
		rec[p + 9] = (double)k;
		rec[p + 10] = (double)iterations;
		rec[p + 11] = 1.0;
		rec[p + 12] = 0.0;
	}
	GI_LANES_END
	gi_sync();
	double null_ll = NAN;
	if (ic) {
		// the intercept-only fit runs in the same work memory and leaves its own parameters in theta[0], theta[1]: the
		// prediction pass gets the group's back
		const double keep0 = P.pred ? theta[0] : 0.0, keep1 = P.pred ? theta[1] : 0.0;
		const AnModel M0 = {1, fs, true};
		int it0 = 0;
		if (an_newton<EM>(P, M0, n_valid, n_events, work, k, null_ll, it0) != 0) null_ll = NAN;
		if (P.pred) {
			gi_sync();
			GI_LANES_BEGIN(lane)
			if (lane == 0) {
				theta[0] = keep0;
				theta[1] = keep1;
			}
			GI_LANES_END
			gi_sync();
		}
	}
	GI_LANES_BEGIN(lane)
	if (lane == 0) rec[p + 3] = null_ll;
	GI_LANES_END
	gi_sync();
	if (P.pred) an_predict(P, 0, theta);
}

} // namespace aft
} // namespace anofox
