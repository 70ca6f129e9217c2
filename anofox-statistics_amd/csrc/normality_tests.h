// normality_tests.h — the normality tests of one group of rows: the Shapiro-Wilk test (Royston's Algorithm AS R94, as R's swilk.c
// and scipy.stats.shapiro compute it), D'Agostino's K2 (scipy.stats.normaltest: the D'Agostino 1970 skewness transform and the
// Anscombe-Glynn kurtosis transform) and the Jarque-Bera test (the reference's jarque_bera,
// crates/anofox-stats-core/src/diagnostics/jarque_bera.rs; its shapiro_wilk and dagostino_k_squared, tests/distributional.rs, are
// wrappers around a crate that is not restated here).  DESIGN.md §1, "Normality tests".
//
//     input: one value column v;  valid row: v not NaN (infinities stay in and make the moments NaN);  n = the valid rows
//     record {statistic, p_value, skewness, kurtosis, z_skewness, z_kurtosis, n, status}; a field a test does not define is NaN
//     status 6: too few rows (Shapiro-Wilk n < 3, K2 n < 8, Jarque-Bera n < 3);  status 1 (invalid input): Shapiro-Wilk n > 5000,
//           K2 and Jarque-Bera with m2 <= 0 (all valid values equal).  Every field but n and the status is NaN in both.
//     moments   the mean, then the biased central moments m2, m3, m4 about it, in TWO PASSES;  skewness = m3 / sd^3 with
//           sd = sqrt(m2), kurtosis = m4 / m2^2 - 3 (excess)
//     Jarque-Bera (2)  JB = n/6 (S^2 + K^2/4), p = exp(-JB/2)
//     K2 (1)    Zs = delta asinh(y / alpha), y = S sqrt((n+1)(n+3) / (6(n-2))) (a y of exactly 0 is replaced by 1, scipy's rule);
//           Zk = (1 - 2/(9A) - cbrt((1 - 2/A) / |d|) sign d) / sqrt(2/(9A)), d = 1 + x sqrt(2/(A-4)) (d = 0: NaN), x the
//           standardised b2 = K + 3;  K2 = Zs^2 + Zk^2, p = exp(-K2/2)
//     Shapiro-Wilk (0)  the sorted values x_(1..n), scores m_i = Phi^-1((i - 3/8)/(n + 1/4)), coefficients a_i = m_i / sqrt(phi) but
//           for the polynomial-corrected a_n (and a_(n-1) when n > 5); n = 3: a = sqrt(1/2).  The a are antisymmetric: only the
//           upper half u_i = -m_i > 0, i = 1 .. n/2, is evaluated, and the numerator is a sum over the pairs x_(n+1-i) - x_(i).
//           With xi = (x - x_(n/2+1)) / range (the centre only keeps the sums small; scipy subtracts the same element):
//           ssa = 2 sum a_i^2, ssx = sum (xi - mean xi)^2, sax = sum a_i (xi_(n+1-i) - xi_(i)), ssassx = sqrt(ssa ssx),
//           1 - W = (ssassx - sax)(ssassx + sax) / (ssa ssx): swilk's form, which does not lose 1 - W to cancellation as
//           (sum a x)^2 / sum (x - mean)^2 does.  p: n = 3 exactly, 6/pi (asin sqrt W - asin sqrt 3/4), floored at 0; otherwise
//           the upper normal tail of (-log(gamma - log(1 - W)) - m)/s for 4 <= n <= 11 and of (log(1 - W) - m)/s for n >= 12,
//           Royston's polynomials in n and in log n.  A range of 0 (all valid values equal): W = 1, p = 1, status 0.
//
// One source for both builds, as sample_tests.h: under hipcc device code, under a plain C++ compiler a wavefront is a loop over 64
// lanes (tests/tools/normality_test_host.cpp).  Contraction of a * b + c is switched off in every body.
//
//   Jarque-Bera, K2  nothing is staged: the group's wavefront streams the rows twice (count and mean, then the centred sums).
//   Shapiro-Wilk     the valid rows are compacted to W.x and sorted as (key, idx).  Lane l evaluates the scores of i = l, l + 64, ..
//             into W.y and reads them back itself in the second walk, so no lane reads another's write; every lane evaluates
//             the first two scores for itself (the corrected coefficients need them).  The quantile (two erfc and two exp per
//             element) is this test's arithmetic.
//   record    lane 0, from a function per test.
#pragma once
#include "sample_tests.h"

namespace anofox {
namespace normtest {

using cor::CorWork;
using glm::GiPL;

constexpr int kNtRecordLen = 8; // {statistic, p_value, skewness, kurtosis, z_skewness, z_kurtosis, n, status}
constexpr int kNtShapiroWilk = 0, kNtDagostinoK2 = 1, kNtJarqueBera = 2;
constexpr int kNtStatusInvalidInput = 1; // ANOFOX_ERROR_INVALID_INPUT
constexpr int kNtStatusInsufficientData = sampletest::kStStatusInsufficientData;
constexpr int64_t kNtShapiroMaxRows = 5000;

struct NormalityProblem {
	const double *v;
	int64_t n_rows; // row ranges are clipped to [0, n_rows)
	int test;
	double *records;
};

// nullptr, or what is wrong with the options
GI_HD const char *nt_options_text(int test) {
	if (test < kNtShapiroWilk || test > kNtJarqueBera) return "normality test: unknown test";
	return nullptr;
}

GI_HD int64_t nt_min_rows(int test) { return test == kNtDagostinoK2 ? 8 : 3; }

// ---- the records ----

GI_DEV void nt_write_failed(double *rec, int64_t n, int status) {
	for (int j = 0; j < kNtRecordLen; ++j) rec[j] = NAN;
	rec[6] = (double)n;
	rec[7] = (double)status;
}

// the counts and the centred power sums of the valid rows
struct NtMoments {
	int64_t n;
	double s2, s3, s4; // sum d^2, sum d^3, sum d^4, d = v - mean
};

// D'Agostino's (1970) transform of the skewness s at n >= 8 rows
GI_DEV double nt_skew_z(double s, double n) {
	RC_NO_CONTRACT
	double y = s * sqrt((n + 1.0) * (n + 3.0) / (6.0 * (n - 2.0)));
	const double beta2 = 3.0 * (n * n + 27.0 * n - 70.0) * (n + 1.0) * (n + 3.0) / ((n - 2.0) * (n + 5.0) * (n + 7.0) * (n + 9.0));
	const double w2 = -1.0 + sqrt(2.0 * (beta2 - 1.0));
	const double delta = 1.0 / sqrt(0.5 * log(w2)), alpha = sqrt(2.0 / (w2 - 1.0));
	if (y == 0.0) y = 1.0;
	return delta * asinh(y / alpha);
}

// Anscombe and Glynn's (1983) transform of the excess kurtosis k at n >= 8 rows
GI_DEV double nt_kurtosis_z(double k, double n) {
	RC_NO_CONTRACT
	const double b2 = k + 3.0;
	const double e = 3.0 * (n - 1.0) / (n + 1.0);
	const double var = 24.0 * n * (n - 2.0) * (n - 3.0) / ((n + 1.0) * (n + 1.0) * (n + 3.0) * (n + 5.0));
	const double x = (b2 - e) / sqrt(var);
	const double sb1 = 6.0 * (n * n - 5.0 * n + 2.0) / ((n + 7.0) * (n + 9.0)) * sqrt(6.0 * (n + 3.0) * (n + 5.0) / (n * (n - 2.0) * (n - 3.0)));
	const double a = 6.0 + 8.0 / sb1 * (2.0 / sb1 + sqrt(1.0 + 4.0 / (sb1 * sb1)));
	const double term1 = 1.0 - 2.0 / (9.0 * a);
	const double denom = 1.0 + x * sqrt(2.0 / (a - 4.0));
	if (denom == 0.0) return NAN;
	const double root = cbrt((1.0 - 2.0 / a) / fabs(denom)); // (the cube root takes the sign of its denominator)
	return (term1 - (denom < 0.0 ? -root : root)) / sqrt(2.0 / (9.0 * a));
}

// Jarque-Bera's and K2's record
RC_CALL void nt_moment_record(int test, const NtMoments &M, double *rec) {
	RC_NO_CONTRACT
	if (M.n < nt_min_rows(test)) {
		nt_write_failed(rec, M.n, kNtStatusInsufficientData);
		return;
	}
	const double n = (double)M.n, m2 = M.s2 / n, m3 = M.s3 / n, m4 = M.s4 / n;
	if (m2 <= 0.0) {
		nt_write_failed(rec, M.n, kNtStatusInvalidInput);
		return;
	}
	const double sd = sqrt(m2), s = m3 / (sd * sd * sd), k = m4 / (m2 * m2) - 3.0;
	double stat, zs = NAN, zk = NAN;
	if (test == kNtJarqueBera) {
		stat = n / 6.0 * (s * s + k * k / 4.0);
	} else {
		zs = nt_skew_z(s, n);
		zk = nt_kurtosis_z(k, n);
		stat = zs * zs + zk * zk;
	}
	rec[0] = stat;
	rec[1] = exp(-stat / 2.0);
	rec[2] = s;
	rec[3] = k;
	rec[4] = zs;
	rec[5] = zk;
	rec[6] = n;
	rec[7] = 0.0;
}

// c[0] + c[1] x + .. + c[N - 1] x^(N - 1)
template <int N>
GI_DEV double nt_poly(const double (&c)[N], double x) {
	RC_NO_CONTRACT
	double r = c[N - 1];
	for (int j = N - 2; j >= 0; --j) r = r * x + c[j];
	return r;
}

// what the coefficients of n > 3 rows need besides the scores: the corrected a_n and a_(n-1) and the divisor of the others
struct NtShapiroHead {
	double a1, a2, fac;
};

// u1, u2: the first two upper scores; summ2 = 2 sum u_i^2
GI_DEV NtShapiroHead nt_shapiro_head(int64_t n, double u1, double u2, double summ2) {
	RC_NO_CONTRACT
	const double c1[6] = {0.0, 0.221157, -0.147981, -2.07119, 4.434685, -2.706056};
	const double c2[6] = {0.0, 0.042981, -0.293762, -1.752461, 5.682633, -3.582633};
	const double ssumm2 = sqrt(summ2), rsn = 1.0 / sqrt((double)n);
	NtShapiroHead H;
	H.a1 = nt_poly(c1, rsn) + u1 / ssumm2;
	if (n > 5) {
		H.a2 = u2 / ssumm2 + nt_poly(c2, rsn);
		H.fac = sqrt((summ2 - 2.0 * (u1 * u1) - 2.0 * (u2 * u2)) / (1.0 - 2.0 * (H.a1 * H.a1) - 2.0 * (H.a2 * H.a2)));
	} else {
		H.a2 = NAN;
		H.fac = sqrt((summ2 - 2.0 * (u1 * u1)) / (1.0 - 2.0 * (H.a1 * H.a1)));
	}
	return H;
}

// The Shapiro-Wilk record of n in [3, 5000] rows from w1 = 1 - W
RC_CALL void nt_shapiro_record(int64_t n, double w1, double *rec) {
	RC_NO_CONTRACT
	const double w = 1.0 - w1;
	double p;
	if (n == 3) {
		const double c = w > 1.0 ? 1.0 : w;
		p = 1.90985931710274380949 * (asin(sqrt(c)) - 1.04719755119659774615); // 6/pi, asin(sqrt(3/4)) = pi/3
		if (p < 0.0) p = 0.0;
	} else if (!(w1 > 0.0)) {
		p = w1 <= 0.0 ? 1.0 : NAN; // (W at or, by rounding, past 1: the limit of the tail)
	} else {
		const double g[2] = {-2.273, 0.459};
		const double c3[4] = {0.544, -0.39978, 0.025054, -6.714e-4}, c4[4] = {1.3822, -0.77857, 0.062767, -0.0020322};
		const double c5[4] = {-1.5861, -0.31082, -0.083751, 0.0038915}, c6[3] = {-0.4803, -0.082676, 0.0030302};
		double y = log(w1), m, s;
		bool far = false;
		if (n <= 11) {
			const double dn = (double)n, gamma = nt_poly(g, dn);
			far = y >= gamma;
			y = -log(gamma - y);
			m = nt_poly(c3, dn);
			s = exp(nt_poly(c4, dn));
		} else {
			const double xx = log((double)n);
			m = nt_poly(c5, xx);
			s = exp(nt_poly(c6, xx));
		}
		p = far ? 1e-99 : 0.5 * erfc((y - m) / s * 0.70710678118654752440); // (1e-99: swilk's value for a W off the low end)
	}
	rec[0] = w;
	rec[1] = p;
	rec[2] = NAN;
	rec[3] = NAN;
	rec[4] = NAN;
	rec[5] = NAN;
	rec[6] = (double)n;
	rec[7] = 0.0;
}

// ---- the phases of one wavefront ----

// The two streaming passes over rows [lo, hi): the count and the mean, then the centred power sums
GI_DEV NtMoments nt_moments(const NormalityProblem &P, int64_t lo, int64_t hi) {
	RC_NO_CONTRACT
	GiPL<double> s2, s3, s4;
	GiPL<int64_t> c;
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	int64_t k = 0;
	for (int64_t i = lo + lane; i < hi; i += 64) {
		const double v = P.v[i];
		if (v != v) continue;
		a += v;
		++k;
	}
	s2.v[GI_AT(lane)] = a;
	c.v[GI_AT(lane)] = k;
	GI_LANES_END
	NtMoments M;
	M.n = glm::gi_sum_i(c);
	const double mean = glm::gi_sum(s2) / (double)M.n;
	GI_LANES_BEGIN(lane)
	double a2 = 0.0, a3 = 0.0, a4 = 0.0;
	for (int64_t i = lo + lane; i < hi; i += 64) {
		const double v = P.v[i];
		if (v != v) continue;
		const double d = v - mean, d2 = d * d;
		a2 += d2;
		a3 += d2 * d;
		a4 += d2 * d2;
	}
	s2.v[GI_AT(lane)] = a2;
	s3.v[GI_AT(lane)] = a3;
	s4.v[GI_AT(lane)] = a4;
	GI_LANES_END
	M.s2 = glm::gi_sum(s2);
	M.s3 = glm::gi_sum(s3);
	M.s4 = glm::gi_sum(s4);
	return M;
}

// the valid rows of [lo, hi) to W.x in their order -> their number
GI_DEV int64_t nt_compact(const NormalityProblem &P, int64_t lo, int64_t hi, const CorWork &W) {
	int64_t n = 0;
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	for (int64_t base = lo; base < hi; base += 64) {
		const int64_t i = base + lane;
		double v = NAN;
		if (i < hi) v = P.v[i];
		const bool ok = v == v;
		const unsigned long long mask = __ballot(ok);
		if (ok) W.x[n + __popcll(mask & ((1ull << lane) - 1ull))] = v;
		n += __popcll(mask);
	}
#else
	for (int64_t i = lo; i < hi; ++i) {
		if (P.v[i] != P.v[i]) continue;
		W.x[n++] = P.v[i];
	}
#endif
	return n;
}

// the upper score u_(i + 1) = -Phi^-1((i + 1 - 3/8) / (n + 1/4)) > 0, i < n / 2 (zero based)
GI_DEV double nt_score(int64_t i, int64_t n) {
	RC_NO_CONTRACT
	return sampletest::st_normal_upper_quantile(((double)(i + 1) - 0.375) / ((double)n + 0.25));
}

// 1 - W of the n in [3, 5000] sorted keys of W (range > 0 or NaN); W.y takes the upper scores
GI_DEV double nt_shapiro_w1(const CorWork &W, int64_t n) {
	RC_NO_CONTRACT
	const int64_t half = n / 2;
	const double *x = W.key;
	const double range = x[n - 1] - x[0], centre = x[half];
	GiPL<double> s0, s1, s2;
	NtShapiroHead H = {0.7071067811865475244, NAN, 1.0};
	if (n > 3) {
		GI_LANES_BEGIN(lane)
		double a = 0.0;
		for (int64_t i = lane; i < half; i += 64) {
			const double u = nt_score(i, n);
			W.y[i] = u;
			a += u * u;
		}
		s0.v[GI_AT(lane)] = a;
		GI_LANES_END
		const double summ2 = 2.0 * glm::gi_sum(s0);
		H = nt_shapiro_head(n, nt_score(0, n), nt_score(1, n), summ2); // (n >= 4: there is a second score)
	}
	GI_LANES_BEGIN(lane)
	double aa = 0.0, ax = 0.0, sx = 0.0;
	for (int64_t i = lane; i < half; i += 64) {
		const double a = n == 3 ? H.a1 : (i == 0 ? H.a1 : (i == 1 && n > 5 ? H.a2 : W.y[i] / H.fac));
		aa += a * a;
		ax += a * ((x[n - 1 - i] - centre) / range - (x[i] - centre) / range);
	}
	for (int64_t i = lane; i < n; i += 64) sx += (x[i] - centre) / range;
	s0.v[GI_AT(lane)] = aa;
	s1.v[GI_AT(lane)] = ax;
	s2.v[GI_AT(lane)] = sx;
	GI_LANES_END
	const double ssa = 2.0 * glm::gi_sum(s0), sax = glm::gi_sum(s1), mx = glm::gi_sum(s2) / (double)n;
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	for (int64_t i = lane; i < n; i += 64) {
		const double d = (x[i] - centre) / range - mx;
		a += d * d;
	}
	s0.v[GI_AT(lane)] = a;
	GI_LANES_END
	const double ssx = glm::gi_sum(s0), ssassx = sqrt(ssa * ssx);
	return (ssassx - sax) * (ssassx + sax) / (ssa * ssx);
}

// ---- one group ----
// Rows [lo, hi) of group g, W as long as the group (Jarque-Bera and K2 do not touch it).  `lead`: this thread belongs to the
// wavefront that runs every phase but the sort (the only wavefront of the small path); tid / threads: the sort's.
GI_DEV void nt_group(const NormalityProblem &P, int64_t g, int64_t lo, int64_t hi, const CorWork &W, bool lead, int64_t tid, int64_t threads) {
	double *rec = P.records + g * kNtRecordLen;
	if (P.test != kNtShapiroWilk) {
		if (!lead) return;
		const NtMoments M = nt_moments(P, lo, hi);
		GI_LANES_BEGIN(lane)
		if (lane == 0) nt_moment_record(P.test, M, rec);
		GI_LANES_END
		return;
	}
	int64_t n = 0;
	if (lead) n = nt_compact(P, lo, hi, W);
#if defined(__HIPCC__)
	if (threads > 64) { // the other wavefronts of the workgroup learn n through the first index slot
		if (lead && (threadIdx.x & 63u) == 0 && hi > lo) W.idx[0] = (int32_t)n;
		glm::gi_sync();
		if (hi > lo) n = W.idx[0];
		glm::gi_sync();
	}
#endif
	const bool runs = n >= 3 && n <= kNtShapiroMaxRows; // (n is the same in every thread: the barriers of the sort are met by all)
	if (runs) {
		if (lead) cor::rc_fill_keys(W.x, n, W);
		cor::rc_sort(W, n, tid, threads);
	}
	if (!lead) return;
	double w1 = NAN;
	bool flat = false;
	if (runs) {
		flat = W.key[n - 1] - W.key[0] == 0.0;
		if (!flat) w1 = nt_shapiro_w1(W, n);
	}
	GI_LANES_BEGIN(lane)
	if (lane == 0) {
		if (!runs) nt_write_failed(rec, n, n < 3 ? kNtStatusInsufficientData : kNtStatusInvalidInput);
		else if (flat) {
			nt_write_failed(rec, n, 0);
			rec[0] = rec[1] = 1.0;
		} else nt_shapiro_record(n, w1, rec);
	}
	GI_LANES_END
}

} // namespace normtest
} // namespace anofox
