// rank_cor.h — Pearson, Spearman and Kendall correlation of one group of (x, y) rows with the test of rho = 0 / tau = 0: R's
// cor.test with exact = FALSE in closed form (the reference's pearson / spearman / kendall, crates/anofox-stats-core/src/tests/
// correlation.rs, are wrappers around a crate that is not restated here).  DESIGN.md §1, "Rank and product-moment correlation".
//
//     valid row: x and y both not NaN (infinities stay in);  n = the valid rows of a group
//     record {estimate, statistic, p_value, ci_lower, ci_upper, n, s, status};  status != 0: every field but n is NaN
//     status: n < 3 -> 6 (InsufficientData).  A constant x or y (zero variance; for Kendall every pair tied): status 0 with
//             estimate, statistic, p_value and the interval NaN (R's NA), for all three methods and on both size paths.
//     Pearson   TWO PASSES over the rows: the means, then the centred sums Sxx, Syy, Sxy;  r = Sxy / sqrt(Sxx Syy), clamped to
//               [-1, 1];  t = r sqrt((n - 2) / (1 - r^2)), Student's t with n - 2 degrees of freedom;  |r| = 1: t = +-inf, p = 0;
//               interval tanh(atanh r -+ zq / sqrt(n - 3)), two-sided whatever the alternative, NaN at n = 3 or zq NaN;  s = NaN.
//     Spearman  the same on the midranks (ties get the mean of the ranks they span).
//     Kendall   s = sum over pairs i < j of sign(x_i - x_j) sign(y_i - y_j), each sign by comparison (equal infinities tie, no
//               product under- or overflows);  n0 = n(n - 1)/2, n1 = sum t(t - 1)/2 over the tie groups of x, n2 over y;
//               tau-b = s / sqrt((n0 - n1)(n0 - n2)), tau-a = s / n0, tau-c = 2 s / (n^2 (m - 1)/m), m = min(distinct x, distinct y);
//               z = s / sqrt(var), R's tie-corrected variance (rc_kendall_record);  p from the normal distribution;  no interval.
//               s and the tie sums are int64 to the end (exact while 2 n^3 < 2^63, n < 1.6e6): the result does not depend on how
//               the pairs were split.
//
// One source for both builds, by the lanes of glm_irls.h: under hipcc device code, under a plain C++ compiler a wavefront is a loop
// over 64 lanes and the butterfly runs over an array of 64 partials (tests/tools/cor_host.cpp), so both add every sum in the same
// order.  Contraction of a * b + c is switched off in every body.
//
//   work      per row of a group: the compacted valid x and y (8 + 8 bytes), a sort key and its row index (8 + 4): kCorRowBytes.
//             LDS for a group of at most the cap's rows (one wavefront per group), the context's workspace above it.
//   compact   valid rows keep their order (a ballot per 64 rows), so every later sum runs in the same order on both paths.
//   moments   lanes stride over the rows, the butterfly adds the 64 partials; Pearson reads the caller's rows (NaN rows skipped in
//             place, nothing staged), Spearman the ranks in the work arrays.
//   sort      the bitonic network in its all-ascending form (the first step of a merge mirrors, partners past n are skipped: the
//             network of the next power of two with +inf behind the data) on (key, row index), a total order.  The only phase that
//             any number of threads of the workgroup share: the large path runs it with the whole workgroup.
//   runs      a lane that finds the first element of a run of equal keys walks to its end, gives every member the midrank and
//             adds the run's tie terms.
//   pairs     small path: lanes stride over i and walk j > i.  Large path: the group goes to a list (CorLarge), a second kernel
//             counts (i block, j block) tiles on as many wavefronts as there are and adds into CorLarge::s, a third writes the
//             record.
#pragma once
#include "glm_irls.h"

#if defined(__clang__)
#define RC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RC_NO_CONTRACT
#endif

// the distribution functions and the records are calls, not inline text: they run once per group, on one lane
#if defined(__HIPCC__)
#define RC_CALL static __device__ __attribute__((noinline))
#else
#define RC_CALL inline
#endif

namespace anofox {
namespace cor {

using glm::GiPL;

constexpr int kCorRecordLen = 8; // {estimate, statistic, p_value, ci_lower, ci_upper, n, s, status}
constexpr int kCorPearson = 0, kCorSpearman = 1, kCorKendall = 2;
constexpr int kCorTwoSided = 0, kCorLess = 1, kCorGreater = 2; // the reference's AnofoxAlternative
constexpr int kCorTauA = 0, kCorTauB = 1, kCorTauC = 2;        // the reference's AnofoxKendallType
constexpr int kCorStatusInsufficientData = 6;
constexpr int kCorRowBytes = 28; // work memory per row: x, y, key (doubles) and the row index (int32)
constexpr int kCorPairTile = 256; // the large path's pair tiles: this many i rows x this many j rows

struct CorProblem {
	const double *x, *y;
	int64_t n_rows; // row ranges are clipped to [0, n_rows)
	int method, alternative, tau_type;
	double zq; // the normal quantile of (1 + confidence_level) / 2; NaN: no interval
	double *records;
};

// the work arrays of one group, each as long as the group has rows
struct CorWork {
	double *x, *y, *key;
	int32_t *idx;
};

// the tie terms of one column's sorted order: sum t(t - 1), sum t(t - 1)(2t + 5), sum t(t - 1)(t - 2), the distinct values
struct CorTies {
	int64_t t1, t2, t3, m;
};

// a Kendall group of the large path between its kernels
struct CorLarge {
	int64_t group, lo, n, s;
	CorTies tx, ty;
};

GI_HD bool rc_options_invalid(int method, int alternative, int tau_type, double confidence_level) {
	if (method < kCorPearson || method > kCorKendall || alternative < kCorTwoSided || alternative > kCorGreater) return true;
	if (tau_type < kCorTauA || tau_type > kCorTauC) return true;
	return confidence_level == confidence_level && !(confidence_level > 0.0 && confidence_level < 1.0);
}

// ---- the distributions ----

// the continued fraction of the incomplete beta function (device_math.h's recurrence, in a text both builds share)
GI_DEV double rc_betacf(double a, double b, double x) {
	RC_NO_CONTRACT
	const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
	double am = 1.0, bm = 1.0, az = 1.0, bz = 1.0 - qab * x / qap;
	const int cap = 3000 + (int)(4.0 * sqrt(a > b ? a : b));
	GI_NOUNROLL
	for (int m = 1; m <= cap; ++m) {
		const double em = (double)m, tem = em + em;
		double d = em * (b - em) * x / ((qam + tem) * (a + tem));
		const double ap = az + d * am, bp = bz + d * bm;
		d = -(a + em) * (qab + em) * x / ((a + tem) * (qap + tem));
		const double app = ap + d * az, bpp = bp + d * bz, aold = az;
		am = ap / bpp;
		bm = bp / bpp;
		az = app / bpp;
		bz = 1.0;
		if (fabs(az - aold) <= 4e-16 * fabs(az)) break;
	}
	return az;
}

// I_x(a, b) with y = 1 - x given by the caller, who has it without the cancellation
RC_CALL double rc_betainc(double a, double b, double x, double y) {
	RC_NO_CONTRACT
	if (!(x > 0.0)) return 0.0;
	if (!(y > 0.0)) return 1.0;
	const double lbt = lgamma(a + b) - lgamma(a) - lgamma(b) + a * log(x) + b * log(y);
	if (x < (a + 1.0) / (a + b + 2.0)) return exp(lbt) * rc_betacf(a, b, x) / a;
	return 1.0 - exp(lbt) * rc_betacf(b, a, y) / b;
}

// the p-value of t under Student's t with df degrees of freedom
GI_DEV double rc_t_p(double t, double df, int alternative) {
	RC_NO_CONTRACT
	if (t != t) return NAN;
	double two = 0.0; // 2 P(T > |t|)
	if (glm::gi_finite(t)) {
		const double t2 = t * t, d = df + t2;
		two = glm::gi_finite(t2) ? rc_betainc(0.5 * df, 0.5, df / d, t2 / d) : 0.0;
	}
	if (alternative == kCorTwoSided) return two;
	const bool tail = alternative == kCorLess ? t < 0.0 : t > 0.0; // the alternative's side is the side t lies on
	return tail ? 0.5 * two : 1.0 - 0.5 * two;
}

// the p-value of z under the standard normal
GI_DEV double rc_z_p(double z, int alternative) {
	RC_NO_CONTRACT
	if (z != z) return NAN;
	if (alternative == kCorTwoSided) return erfc(fabs(z) * 0.70710678118654752440);
	return 0.5 * erfc((alternative == kCorLess ? -z : z) * 0.70710678118654752440);
}

// ---- the records ----

GI_DEV void rc_write_failed(double *rec, int64_t n, int status) {
	for (int j = 0; j < kCorRecordLen; ++j) rec[j] = NAN;
	rec[5] = (double)n;
	rec[7] = (double)status;
}

// Pearson's and Spearman's record from r (NaN: a constant column)
RC_CALL void rc_moment_record(const CorProblem &P, double r, int64_t n, double *rec) {
	RC_NO_CONTRACT
	if (n < 3) {
		rc_write_failed(rec, n, kCorStatusInsufficientData);
		return;
	}
	const double df = (double)(n - 2);
	double t = NAN, lo = NAN, hi = NAN;
	if (r == r) {
		t = fabs(r) >= 1.0 ? (r > 0.0 ? INFINITY : -INFINITY) : r * sqrt(df / (1.0 - r * r));
		if (n > 3 && P.zq == P.zq) {
			const double z = atanh(r), h = P.zq / sqrt((double)(n - 3));
			lo = tanh(z - h);
			hi = tanh(z + h);
		}
	}
	rec[0] = r;
	rec[1] = t;
	rec[2] = rc_t_p(t, df, P.alternative);
	rec[3] = lo;
	rec[4] = hi;
	rec[5] = (double)n;
	rec[6] = NAN;
	rec[7] = 0.0;
}

// Kendall's record from the pair count and the tie terms of the two sorted orders
RC_CALL void rc_kendall_record(const CorProblem &P, int64_t s, int64_t n, const CorTies &tx, const CorTies &ty, double *rec) {
	RC_NO_CONTRACT
	if (n < 3) {
		rc_write_failed(rec, n, kCorStatusInsufficientData);
		return;
	}
	const double dn = (double)n, ds = (double)s;
	const int64_t n0 = n * (n - 1) / 2;
	double tau = NAN, z = NAN;
	if (tx.m > 1 && ty.m > 1) {
		if (P.tau_type == kCorTauA) tau = ds / (double)n0;
		else if (P.tau_type == kCorTauB) tau = ds / sqrt((double)(n0 - tx.t1 / 2) * (double)(n0 - ty.t1 / 2));
		else {
			const double m = (double)(tx.m < ty.m ? tx.m : ty.m);
			tau = 2.0 * ds / (dn * dn * (m - 1.0) / m);
		}
		const double v0 = dn * (dn - 1.0) * (2.0 * dn + 5.0);
		const double var = (v0 - (double)tx.t2 - (double)ty.t2) / 18.0 + (double)tx.t1 * (double)ty.t1 / (2.0 * dn * (dn - 1.0)) +
		                   (double)tx.t3 * (double)ty.t3 / (9.0 * dn * (dn - 1.0) * (dn - 2.0));
		z = ds / sqrt(var);
	}
	rec[0] = tau;
	rec[1] = z;
	rec[2] = rc_z_p(z, P.alternative);
	rec[3] = NAN;
	rec[4] = NAN;
	rec[5] = dn;
	rec[6] = ds;
	rec[7] = 0.0;
}

// ---- the phases of one wavefront ----

// the valid rows of [lo, hi) to W.x, W.y in their order -> their number
GI_DEV int64_t rc_compact(const CorProblem &P, int64_t lo, int64_t hi, const CorWork &W) {
	int64_t n = 0;
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	for (int64_t base = lo; base < hi; base += 64) {
		const int64_t i = base + lane;
		double xi = NAN, yi = NAN;
		if (i < hi) {
			xi = P.x[i];
			yi = P.y[i];
		}
		const bool valid = xi == xi && yi == yi;
		const unsigned long long mask = __ballot(valid);
		if (valid) {
			const int64_t at = n + __popcll(mask & ((1ull << lane) - 1ull));
			W.x[at] = xi;
			W.y[at] = yi;
		}
		n += __popcll(mask);
	}
#else
	for (int64_t i = lo; i < hi; ++i) {
		if (P.x[i] != P.x[i] || P.y[i] != P.y[i]) continue;
		W.x[n] = P.x[i];
		W.y[n] = P.y[i];
		++n;
	}
#endif
	return n;
}

// r of the m rows (a, b), rows with a NaN skipped -> their number in n.  Two passes: the means, then the centred sums.
GI_DEV double rc_moments(const double *a, const double *b, int64_t m, int64_t &n) {
	RC_NO_CONTRACT
	GiPL<double> s0, s1, s2;
	GiPL<int64_t> cnt;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane);
	double sa = 0.0, sb = 0.0;
	int64_t c = 0;
	for (int64_t i = lane; i < m; i += 64) {
		const double ai = a[i], bi = b[i];
		if (ai != ai || bi != bi) continue;
		sa += ai;
		sb += bi;
		++c;
	}
	s0.v[L] = sa;
	s1.v[L] = sb;
	cnt.v[L] = c;
	GI_LANES_END
	n = glm::gi_sum_i(cnt);
	const double ma = glm::gi_sum(s0) / (double)n, mb = glm::gi_sum(s1) / (double)n;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane);
	double saa = 0.0, sbb = 0.0, sab = 0.0;
	for (int64_t i = lane; i < m; i += 64) {
		const double ai = a[i], bi = b[i];
		if (ai != ai || bi != bi) continue;
		const double da = ai - ma, db = bi - mb;
		saa += da * da;
		sbb += db * db;
		sab += da * db;
	}
	s0.v[L] = saa;
	s1.v[L] = sbb;
	s2.v[L] = sab;
	GI_LANES_END
	const double saa = glm::gi_sum(s0), sbb = glm::gi_sum(s1), sab = glm::gi_sum(s2);
	if (!(saa > 0.0) || !(sbb > 0.0)) return NAN; // a constant column (or nothing finite to centre on)
	const double r = sab / sqrt(saa * sbb);
	return r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
}

// (key[i], i) for the n compacted values v
GI_DEV void rc_fill_keys(const double *v, int64_t n, const CorWork &W) {
	GI_LANES_BEGIN(lane)
	for (int64_t i = lane; i < n; i += 64) {
		W.key[i] = v[i];
		W.idx[i] = (int32_t)i;
	}
	GI_LANES_END
}

GI_DEV void rc_compare_exchange(const CorWork &W, int64_t l, int64_t p) {
	const double kl = W.key[l], kp = W.key[p];
	const int32_t il = W.idx[l], ip = W.idx[p];
	if (kl > kp || (kl == kp && il > ip)) {
		W.key[l] = kp;
		W.key[p] = kl;
		W.idx[l] = ip;
		W.idx[p] = il;
	}
}

// Sorts (key, idx) ascending.  Run by `threads` threads of one workgroup together (tid = this thread's number); on the host by
// the 64 lanes of the loop.  Every step's compare-exchanges touch disjoint pairs; gi_sync() separates the steps.
#if defined(__HIPCC__)
#define RC_THREADS_BEGIN(t, tid) { const int64_t t = (tid);
#else
#define RC_THREADS_BEGIN(t, tid) for (int64_t t = 0; t < threads; ++t) {
#endif
GI_DEV void rc_sort(const CorWork &W, int64_t n, int64_t tid, int64_t threads) {
	(void)tid;
	int64_t pad = 1;
	while (pad < n) pad <<= 1;
	glm::gi_sync();
	for (int64_t k = 2; k <= pad; k <<= 1) {
		const int64_t half = k >> 1;
		RC_THREADS_BEGIN(t, tid)
		for (int64_t u = t; u < pad / 2; u += threads) { // the mirror step: l and its reflection in the block of k
			const int64_t b = u / half * k, o = u % half, p = b + k - 1 - o;
			if (p < n) rc_compare_exchange(W, b + o, p);
		}
		GI_LANES_END
		glm::gi_sync();
		for (int64_t j = half >> 1; j > 0; j >>= 1) {
			RC_THREADS_BEGIN(t, tid)
			for (int64_t u = t; u < pad / 2; u += threads) {
				const int64_t l = 2 * u - (u & (j - 1)), p = l + j;
				if (p < n) rc_compare_exchange(W, l, p);
			}
			GI_LANES_END
			glm::gi_sync();
		}
	}
}

// The runs of equal keys of the sorted order: the tie terms, and with `rank` the midrank of every member at its row's place.
GI_DEV CorTies rc_runs(const CorWork &W, int64_t n, double *rank) {
	GiPL<int64_t> t1, t2, t3, m;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane);
	int64_t a1 = 0, a2 = 0, a3 = 0, am = 0;
	for (int64_t i = lane; i < n; i += 64) {
		const double k = W.key[i];
		if (i > 0 && W.key[i - 1] == k) continue; // not the first of its run
		int64_t e = i + 1;
		while (e < n && W.key[e] == k) ++e;
		const int64_t t = e - i;
		a1 += t * (t - 1);
		a2 += t * (t - 1) * (2 * t + 5);
		a3 += t * (t - 1) * (t - 2);
		++am;
		if (rank) {
			const double mid = 0.5 * (double)(i + e + 1); // the mean of the ranks i + 1 .. e
			for (int64_t q = i; q < e; ++q) rank[W.idx[q]] = mid;
		}
	}
	t1.v[L] = a1;
	t2.v[L] = a2;
	t3.v[L] = a3;
	m.v[L] = am;
	GI_LANES_END
	CorTies T;
	T.t1 = glm::gi_sum_i(t1);
	T.t2 = glm::gi_sum_i(t2);
	T.t3 = glm::gi_sum_i(t3);
	T.m = glm::gi_sum_i(m);
	return T;
}

// sum over j in [j0, j1) of sign(xi - xj[j]) sign(yi - yj[j])
GI_DEV int64_t rc_pairs_row(double xi, double yi, const double *xj, const double *yj, int64_t j0, int64_t j1) {
	int64_t s = 0;
	for (int64_t j = j0; j < j1; ++j) {
		const double a = xj[j], b = yj[j];
		s += ((xi > a) - (xi < a)) * ((yi > b) - (yi < b));
	}
	return s;
}

// the pair count of n compacted rows by one wavefront
GI_DEV int64_t rc_pairs(const double *x, const double *y, int64_t n) {
	GiPL<int64_t> s;
	GI_LANES_BEGIN(lane)
	int64_t a = 0;
	for (int64_t i = lane; i < n; i += 64) a += rc_pairs_row(x[i], y[i], x, y, i + 1, n);
	s.v[GI_AT(lane)] = a;
	GI_LANES_END
	return glm::gi_sum_i(s);
}

// ---- one group ----
// Rows [lo, hi) of group g, W as long as the group.  `lead`: this thread belongs to the wavefront that runs every phase but the
// sort (the only wavefront of the small path); tid / threads: the sort's.  large == nullptr: the record is written.  Otherwise
// (the large path) a Kendall group leaves its pair count to the tile kernel: the lead fills *large and the record waits.
GI_DEV void rc_group(const CorProblem &P, int64_t g, int64_t lo, int64_t hi, const CorWork &W, bool lead, int64_t tid, int64_t threads,
                     CorLarge *large) {
	double *rec = P.records + g * kCorRecordLen;
	if (P.method == kCorPearson) {
		if (!lead) return;
		int64_t n;
		const double r = rc_moments(P.x + lo, P.y + lo, hi - lo, n);
		GI_LANES_BEGIN(lane)
		if (lane == 0) rc_moment_record(P, r, n, rec);
		GI_LANES_END
		return;
	}
	int64_t n = 0;
	if (lead) n = rc_compact(P, lo, hi, W);
#if defined(__HIPCC__)
	if (threads > 64) { // the other wavefronts of the workgroup learn n through the first key slot's index
		if (lead && (threadIdx.x & 63u) == 0 && hi > lo) W.idx[0] = (int32_t)n;
		glm::gi_sync();
		if (hi > lo) n = W.idx[0];
		glm::gi_sync();
	}
#endif
	CorTies tx = {0, 0, 0, 0}, ty = {0, 0, 0, 0};
	const bool ranks = P.method == kCorSpearman;
	if (n >= 3) { // (n is the same in every thread: the barriers of the sort are met by all)
		if (lead) rc_fill_keys(W.x, n, W);
		rc_sort(W, n, tid, threads);
		if (lead) tx = rc_runs(W, n, ranks ? W.x : nullptr);
		glm::gi_sync();
		if (lead) rc_fill_keys(W.y, n, W);
		rc_sort(W, n, tid, threads);
		if (lead) ty = rc_runs(W, n, ranks ? W.y : nullptr);
		glm::gi_sync();
	}
	if (!lead) return;
	if (ranks) {
		int64_t k;
		const double r = n >= 3 ? rc_moments(W.x, W.y, n, k) : NAN;
		GI_LANES_BEGIN(lane)
		if (lane == 0) rc_moment_record(P, r, n, rec);
		GI_LANES_END
		return;
	}
	if (large && n >= 3) {
		GI_LANES_BEGIN(lane)
		if (lane == 0) {
			large->group = g;
			large->lo = lo;
			large->n = n;
			large->s = 0;
			large->tx = tx;
			large->ty = ty;
		}
		GI_LANES_END
		return;
	}
	const int64_t s = n >= 3 ? rc_pairs(W.x, W.y, n) : 0;
	GI_LANES_BEGIN(lane)
	if (lane == 0) rc_kendall_record(P, s, n, tx, ty, rec);
	GI_LANES_END
}

} // namespace cor
} // namespace anofox
