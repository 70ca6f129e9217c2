// rank_tests.h — the rank-based location tests of one group of rows: Mann-Whitney U, Wilcoxon signed-rank and Kruskal-Wallis in
// closed form, as R's wilcox.test(exact = FALSE) and kruskal.test compute them (the reference's mann_whitney_u, wilcoxon_signed_rank
// and kruskal_wallis, crates/anofox-stats-core/src/tests/nonparametric.rs, are wrappers around a crate that is not restated here).
// DESIGN.md §1, "Rank-based location tests".
//
//     input: a value column v, a second column y (Wilcoxon) and an int32 sample column (Mann-Whitney, Kruskal-Wallis)
//     valid row: v not NaN (infinities stay in); Wilcoxon: v - y - mu not NaN, that is v and y not NaN and not the same infinity
//     record {statistic, z, p_value, df, n, n1, n2, status};  status != 0: every field but the counts is NaN
//     Mann-Whitney (test 0)   sample 1 = the rows with sample == 0, sample 2 = every other id;  r = midranks of c(v1 - mu, v2);
//               W = sum r[sample 1] - n1(n1 + 1)/2;  z = (W - n1 n2 / 2 - c) / sigma,
//               sigma^2 = n1 n2 / 12 ((N + 1) - sum(t^3 - t) / (N (N - 1))), N = n1 + n2;  c = 0 without the continuity correction,
//               else sign(W - n1 n2 / 2) / 2 two-sided, +1/2 greater, -1/2 less;  p from the normal distribution.
//               n1 < 1 or n2 < 1 -> status 6;  sigma = 0 (every value tied): status 0, W kept, z and p NaN.  df = NaN.
//     Wilcoxon (test 1)       d = v - y - mu over the valid pairs, zero differences dropped: m left;  r = midranks of |d|;
//               V = sum r[d > 0];  z = (V - m(m + 1)/4 - c) / sigma,  sigma^2 = m(m + 1)(2m + 1)/24 - sum(t^3 - t)/48;  c, p as above.
//               fewer than 2 valid pairs -> status 6;  m = 0: status 0, V = 0, z and p NaN.
//               n = the valid pairs with the zeros, n1 = m, n2 = the zeros dropped, df = NaN.
//     Kruskal-Wallis (test 2) r = midranks of the valid values, k = the distinct sample ids (any int32) among them;
//               H = (12 / (N (N + 1)) sum_j R_j^2 / n_j - 3 (N + 1)) / (1 - sum(t^3 - t) / (N^3 - N));  df = k - 1;
//               p = Q(df / 2, H / 2), the upper tail of chi-square.  N < 3 or k < 2 -> status 6;  every value equal: status 0 with H
//               and p NaN.  n1 = k, n2 = NaN, z = NaN.
//     Midranks are multiples of 1/2, so W, V and every R_j are exact in double and do not depend on the order of a sum or on the
//     size path; the tie sum is int64, sum(t^3 - t) = t3 + 3 t1 of CorTies.  Only sigma, the division, H's last arithmetic and the
//     distribution function round.
//     Not built: exact small-sample p-values, the Hodges-Lehmann estimate and its interval.
//
// One source for both builds, as rank_cor.h, whose work layout (CorWork, 28 bytes per row), sort, runs and butterfly sums these
// tests use: under hipcc device code, under a plain C++ compiler a wavefront is a loop over 64 lanes (tests/tools/
// rank_test_host.cpp).  Contraction of a * b + c is switched off in every body.
//
//   compact   valid rows keep their order (a ballot per 64 rows).  W.x: the value to rank (v - mu for sample 1, v otherwise; |d|),
//             W.y: the second datum (the sample id as a double, exact for int32; sign(d)).
//   rank      rc_fill_keys(W.x), rc_sort, rc_runs with rank = W.x: the midranks replace the values, the tie terms come back.
//   sums      Mann-Whitney, Wilcoxon: lanes stride over the rows and add the ranks that W.y selects (exact, any order).
//             Kruskal-Wallis: a second sort, by sample id; the lane that finds the first element of a run of equal ids walks the
//             run, adds its ranks and contributes R^2 / t and 1 (to k); the partials meet in the fixed-order butterfly.
//   record    lane 0, from a function per test.
#pragma once
#include "rank_cor.h"

namespace anofox {
namespace ranktest {

using cor::CorTies;
using cor::CorWork;
using glm::GiPL;

constexpr int kRtRecordLen = 8; // {statistic, z, p_value, df, n, n1, n2, status}
constexpr int kRtMannWhitney = 0, kRtWilcoxon = 1, kRtKruskalWallis = 2;
constexpr int kRtStatusInsufficientData = 6;

struct RankTestProblem {
	const double *v, *y;   // y: Wilcoxon only
	const int32_t *sample; // Mann-Whitney and Kruskal-Wallis only
	int64_t n_rows;        // row ranges are clipped to [0, n_rows)
	int test, alternative, correction;
	double mu;
	double *records;
};

// nullptr, or what is wrong with the options
GI_HD const char *rt_options_text(int test, int alternative, double mu) {
	if (test < kRtMannWhitney || test > kRtKruskalWallis) return "rank test: unknown test";
	if (alternative < cor::kCorTwoSided || alternative > cor::kCorGreater) return "rank test: unknown alternative";
	if (!(fabs(mu) <= DBL_MAX)) return "rank test: mu must be finite";
	if (test == kRtKruskalWallis && mu != 0.0) return "rank test: the Kruskal-Wallis test takes no mu";
	return nullptr;
}

// ---- the chi-square tail ----

// Q(a, x), the regularised upper incomplete gamma function: the series of P below a + 1, Lentz's continued fraction of Q above
RC_CALL double rt_gamma_q(double a, double x) {
	RC_NO_CONTRACT
	if (x != x || a != a) return NAN;
	if (!(x > 0.0)) return 1.0;
	if (!glm::gi_finite(x)) return 0.0;
	const double pre = exp(a * log(x) - x - lgamma(a));
	const int cap = 3000 + (int)(8.0 * sqrt(a > x ? a : x));
	if (x < a + 1.0) {
		double term = 1.0 / a, sum = term;
		GI_NOUNROLL
		for (int n = 1; n <= cap; ++n) {
			term *= x / (a + (double)n);
			sum += term;
			if (term <= 1e-17 * sum) break;
		}
		return 1.0 - pre * sum;
	}
	const double tiny = 1e-300;
	double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
	GI_NOUNROLL
	for (int i = 1; i <= cap; ++i) {
		const double an = -(double)i * ((double)i - a);
		b += 2.0;
		d = an * d + b;
		if (fabs(d) < tiny) d = tiny;
		c = b + an / c;
		if (fabs(c) < tiny) c = tiny;
		d = 1.0 / d;
		const double del = d * c;
		h *= del;
		if (fabs(del - 1.0) <= 2e-16) break;
	}
	return pre * h;
}

// ---- the records ----

GI_DEV void rt_write_failed(double *rec, double n, double n1, double n2) {
	for (int j = 0; j < kRtRecordLen; ++j) rec[j] = NAN;
	rec[4] = n;
	rec[5] = n1;
	rec[6] = n2;
	rec[7] = (double)kRtStatusInsufficientData;
}

// the continuity correction of a statistic whose distance from its mean is `num`
GI_DEV double rt_correction(const RankTestProblem &P, double num) {
	if (!P.correction) return 0.0;
	if (P.alternative == cor::kCorGreater) return 0.5;
	if (P.alternative == cor::kCorLess) return -0.5;
	return num > 0.0 ? 0.5 : (num < 0.0 ? -0.5 : 0.0);
}

GI_DEV void rt_write_z(const RankTestProblem &P, double stat, double num, double var, double n, double n1, double n2, double *rec) {
	RC_NO_CONTRACT
	const double z = var > 0.0 ? (num - rt_correction(P, num)) / sqrt(var) : NAN;
	rec[0] = stat;
	rec[1] = z;
	rec[2] = cor::rc_z_p(z, P.alternative);
	rec[3] = NAN;
	rec[4] = n;
	rec[5] = n1;
	rec[6] = n2;
	rec[7] = 0.0;
}

// Mann-Whitney's record from the rank sum of sample 1, the two counts and the tie terms of the pooled order
RC_CALL void rt_mann_whitney_record(const RankTestProblem &P, double rank_sum, int64_t n1, int64_t n2, const CorTies &T, double *rec) {
	RC_NO_CONTRACT
	const double d1 = (double)n1, d2 = (double)n2, dn = d1 + d2;
	if (n1 < 1 || n2 < 1) {
		rt_write_failed(rec, dn, d1, d2);
		return;
	}
	const double w = rank_sum - d1 * (d1 + 1.0) / 2.0;
	const double ties = (double)(T.t3 + 3 * T.t1);
	const double var = T.m > 1 ? d1 * d2 / 12.0 * ((dn + 1.0) - ties / (dn * (dn - 1.0))) : 0.0;
	rt_write_z(P, w, w - d1 * d2 / 2.0, var, dn, d1, d2, rec);
}

// Wilcoxon's record from the rank sum of the positive differences, the m non-zero differences and the valid pairs
RC_CALL void rt_wilcoxon_record(const RankTestProblem &P, double rank_sum, int64_t m, int64_t valid, const CorTies &T, double *rec) {
	RC_NO_CONTRACT
	const double dm = (double)m, dn = (double)valid, zeros = (double)(valid - m);
	if (valid < 2) {
		rt_write_failed(rec, dn, dm, zeros);
		return;
	}
	const double ties = (double)(T.t3 + 3 * T.t1);
	const double var = m > 0 ? dm * (dm + 1.0) * (2.0 * dm + 1.0) / 24.0 - ties / 48.0 : 0.0;
	rt_write_z(P, rank_sum, rank_sum - dm * (dm + 1.0) / 4.0, var, dn, dm, zeros, rec);
}

// Kruskal-Wallis' record from sum_j R_j^2 / n_j, the k samples, the N valid rows and the tie terms
RC_CALL void rt_kruskal_record(const RankTestProblem &, double sum_r2, int64_t k, int64_t n, const CorTies &T, double *rec) {
	RC_NO_CONTRACT
	const double dn = (double)n, dk = (double)k;
	if (n < 3 || k < 2) {
		rt_write_failed(rec, dn, dk, NAN);
		return;
	}
	double h = NAN, p = NAN;
	if (T.m > 1) {
		const double ties = (double)(T.t3 + 3 * T.t1);
		h = (12.0 / (dn * (dn + 1.0)) * sum_r2 - 3.0 * (dn + 1.0)) / (1.0 - ties / (dn * dn * dn - dn));
		p = rt_gamma_q(0.5 * (dk - 1.0), 0.5 * h);
	}
	rec[0] = h;
	rec[1] = NAN;
	rec[2] = p;
	rec[3] = dk - 1.0;
	rec[4] = dn;
	rec[5] = dk;
	rec[6] = NAN;
	rec[7] = 0.0;
}

// ---- the phases of one wavefront ----

// One row's datum: the value to rank in a, the second datum in b -> the row is valid; keep: it is ranked (not a zero difference)
GI_DEV bool rt_row(const RankTestProblem &P, int64_t i, double &a, double &b, bool &keep) {
	RC_NO_CONTRACT
	const double v = P.v[i];
	if (P.test == kRtWilcoxon) {
		const double d = v - P.y[i] - P.mu;
		a = fabs(d);
		b = d > 0.0 ? 1.0 : -1.0;
		keep = d == d && d != 0.0;
		return d == d;
	}
	const int32_t s = P.sample[i];
	a = P.test == kRtMannWhitney && s == 0 ? v - P.mu : v;
	b = (double)s;
	keep = v == v;
	return keep;
}

// the ranked rows of [lo, hi) to W.x, W.y in their order -> their number; valid: the valid rows (Wilcoxon: with the zeros)
GI_DEV int64_t rt_compact(const RankTestProblem &P, int64_t lo, int64_t hi, const CorWork &W, int64_t &valid) {
	int64_t n = 0;
	valid = 0;
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	for (int64_t base = lo; base < hi; base += 64) {
		const int64_t i = base + lane;
		double a = NAN, b = NAN;
		bool keep = false, ok = false;
		if (i < hi) ok = rt_row(P, i, a, b, keep);
		const unsigned long long mask = __ballot(keep);
		if (keep) {
			const int64_t at = n + __popcll(mask & ((1ull << lane) - 1ull));
			W.x[at] = a;
			W.y[at] = b;
		}
		n += __popcll(mask);
		valid += __popcll(__ballot(ok));
	}
#else
	for (int64_t i = lo; i < hi; ++i) {
		double a, b;
		bool keep;
		if (rt_row(P, i, a, b, keep)) ++valid;
		if (!keep) continue;
		W.x[n] = a;
		W.y[n] = b;
		++n;
	}
#endif
	return n;
}

// the sum of the ranks W.x whose W.y equals `pick`, and in `count` how many they are
GI_DEV double rt_rank_sum(const CorWork &W, int64_t n, double pick, int64_t &count) {
	RC_NO_CONTRACT
	GiPL<double> s;
	GiPL<int64_t> c;
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	int64_t k = 0;
	for (int64_t i = lane; i < n; i += 64) {
		if (W.y[i] != pick) continue;
		a += W.x[i];
		++k;
	}
	s.v[GI_AT(lane)] = a;
	c.v[GI_AT(lane)] = k;
	GI_LANES_END
	count = glm::gi_sum_i(c);
	return glm::gi_sum(s);
}

// (key, idx) sorted by sample id, the ranks in W.x: sum over the samples of R^2 / t, and in k the samples
GI_DEV double rt_sample_sums(const CorWork &W, int64_t n, int64_t &k) {
	RC_NO_CONTRACT
	GiPL<double> s;
	GiPL<int64_t> c;
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	int64_t m = 0;
	for (int64_t i = lane; i < n; i += 64) {
		const double id = W.key[i];
		if (i > 0 && W.key[i - 1] == id) continue; // not the first of its run
		double r = 0.0;
		int64_t e = i;
		for (; e < n && W.key[e] == id; ++e) r += W.x[W.idx[e]];
		a += r * r / (double)(e - i);
		++m;
	}
	s.v[GI_AT(lane)] = a;
	c.v[GI_AT(lane)] = m;
	GI_LANES_END
	k = glm::gi_sum_i(c);
	return glm::gi_sum(s);
}

// ---- one group ----
// Rows [lo, hi) of group g, W as long as the group.  `lead`: this thread belongs to the wavefront that runs every phase but the
// sorts (the only wavefront of the small path); tid / threads: the sorts'.
GI_DEV void rt_group(const RankTestProblem &P, int64_t g, int64_t lo, int64_t hi, const CorWork &W, bool lead, int64_t tid, int64_t threads) {
	double *rec = P.records + g * kRtRecordLen;
	int64_t n = 0, valid = 0;
	if (lead) n = rt_compact(P, lo, hi, W, valid);
#if defined(__HIPCC__)
	if (threads > 64) { // the other wavefronts of the workgroup learn n through the first key slot's index
		if (lead && (threadIdx.x & 63u) == 0 && hi > lo) W.idx[0] = (int32_t)n;
		glm::gi_sync();
		if (hi > lo) n = W.idx[0];
		glm::gi_sync();
	}
#endif
	CorTies T = {0, 0, 0, 0};
	// (n is the same in every thread: the barriers of the sorts are met by all)
	if (lead) cor::rc_fill_keys(W.x, n, W);
	cor::rc_sort(W, n, tid, threads);
	if (lead) T = cor::rc_runs(W, n, W.x);
	glm::gi_sync();
	if (P.test == kRtKruskalWallis) {
		if (lead) cor::rc_fill_keys(W.y, n, W);
		cor::rc_sort(W, n, tid, threads);
		if (!lead) return;
		int64_t k;
		const double sum_r2 = rt_sample_sums(W, n, k);
		GI_LANES_BEGIN(lane)
		if (lane == 0) rt_kruskal_record(P, sum_r2, k, n, T, rec);
		GI_LANES_END
		return;
	}
	if (!lead) return;
	int64_t n1;
	const double rank_sum = rt_rank_sum(W, n, P.test == kRtMannWhitney ? 0.0 : 1.0, n1);
	GI_LANES_BEGIN(lane)
	if (lane == 0) {
		if (P.test == kRtMannWhitney) rt_mann_whitney_record(P, rank_sum, n1, n - n1, T, rec);
		else rt_wilcoxon_record(P, rank_sum, n, valid, T, rec);
	}
	GI_LANES_END
}

} // namespace ranktest
} // namespace anofox
