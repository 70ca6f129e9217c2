// sample_tests.h — the parametric and studentised-rank tests of one group of rows: the t-test (Welch, Student, paired), Yuen's
// trimmed-mean test, one-way ANOVA (Fisher, Welch), the Brown-Forsythe test and the Brunner-Munzel test in closed form, as R's
// t.test, oneway.test, the median-centred Levene test, Yuen's test and brunner.munzel.test compute them (the reference's t_test,
// yuen_test, one_way_anova, brown_forsythe and brunner_munzel, crates/anofox-stats-core/src/tests/{parametric,nonparametric}.rs,
// are wrappers around a crate that is not restated here).  DESIGN.md §1, "Parametric and studentised-rank tests".
//
//     input: a value column v, a second column y (the paired t-test) and an int32 sample column (every other test)
//     valid row: v not NaN (infinities stay in); paired: v - y - mu not NaN
//     arms: two-sample tests (t, Yuen, Brunner-Munzel): sample 1 = the rows with sample == 0, sample 2 = every other id;
//           k-sample tests (ANOVA, Brown-Forsythe): any int32 ids
//     record {statistic, p_value, df, df2, estimate, ci_lower, ci_upper, n, n1, n2, aux, status};  status 6: every field but the
//           counts is NaN.  aux: the standard error of the estimate (t, Yuen, Brunner-Munzel), SSW (ANOVA, Brown-Forsythe).
//     per arm n_j, mean m_j, S_j = sum (v - m_j)^2 in TWO PASSES (the means, then the centred sums), s_j^2 = S_j / (n_j - 1)
//     t-test (0)   n1 < 2 or n2 < 2 (paired: fewer than 2 valid pairs) -> 6.  estimate = m1 - m2 (paired: the mean of d = v - y);
//           t = (estimate - mu) / se.  Welch se^2 = s1^2/n1 + s2^2/n2, df Welch-Satterthwaite; Student the pooled variance,
//           df = n1 + n2 - 2; paired the one-sample form on d, df = n - 1 (n = n1 = n2 = the valid pairs).  p from Student's t;
//           interval estimate -+ q se, q the t quantile of (1 + cl)/2; one-sided: q of cl and the open side +-inf (R's rule).
//           se = 0 (or NaN): status 0 with statistic, p, df and the interval NaN.  A NaN confidence level: no interval.
//     Yuen (1)     an arm below 4 rows, or h = n - 2 g < 2 with g = floor(trim n) -> 6.  tm = the mean of the order statistics
//           g .. n-g-1, sw^2 the winsorised sample variance, d = (n - 1) sw^2 / (h (h - 1));  t = (tm1 - tm2) / sqrt(d1 + d2),
//           df = (d1 + d2)^2 / (d1^2/(h1-1) + d2^2/(h2-1));  estimate = tm1 - tm2;  p and the interval as the t-test.
//     ANOVA (2)    k < 2 or an arm below 2 rows -> 6.  Fisher F = (SSB/(k-1)) / (SSW/(N-k)), df = k-1, df2 = N-k.  Welch: R's
//           oneway.test(var.equal = FALSE).  estimate = SSB, aux = SSW, n1 = k, n2 = NaN.  p = the upper tail of F.
//           SSW = 0: F = +inf, p = 0 when SSB > 0, both NaN when SSB = 0.  Welch with an s_j^2 = 0: F, df2 and p NaN.
//     Brown-Forsythe (3)  Fisher's F of z = |v - median_j| (an even arm's median: the mean of its two middle values).
//     Brunner-Munzel (4)  n1 < 2 or n2 < 2 -> 6.  R the pooled midranks, r the midranks within the row's arm, Rbar_j the arm means
//           of R, S_j^2 = sum (R - r - Rbar_j + (n_j+1)/2)^2 / (n_j - 1);  W = n1 n2 (Rbar2 - Rbar1) / ((n1+n2) sqrt(n1 S1^2 + n2 S2^2)),
//           Satterthwaite's df, p from Student's t (`greater`: the lower tail of W, scipy's and lawstat's reading);
//           estimate = phat = (Rbar2 - (n2+1)/2) / n1, not clamped;  interval phat -+ q sqrt(S1^2/(n1 n2^2) + S2^2/(n2 n1^2)),
//           two-sided whatever the alternative.  S1^2 + S2^2 = 0: W = +-inf by the sign of phat - 1/2 (NaN at 1/2), df NaN, the
//           interval [phat, phat].  R, r and their arm sums are multiples of 1/2: exact, whatever the order of a sum.
//
// One source for both builds, as rank_tests.h: under hipcc device code, under a plain C++ compiler a wavefront is a loop over 64
// lanes (tests/tools/sample_test_host.cpp).  Contraction of a * b + c is switched off in every body.
//
//   t-test    nothing is staged: the group's wavefront streams the rows twice (counts and means, then centred sums).
//   two-sample sorted (Yuen, Brunner-Munzel)  a count pass gives n1; the ordered compaction writes sample 1 to [0, n1) and sample
//             2 to [n1, n) of W.x, so the arm is the position.  Each arm is a sub-view W + 0, W + n1 of the work arrays that
//             rc_fill_keys / rc_sort / rc_runs take as they take a whole group (rc_sort addresses its view by element only:
//             any base, any length).  Brunner-Munzel ranks the pooled view into W.y, then each sub-view over W.x.
//   k-sample  the sort by id makes the arms runs; the lane that finds a run's first element walks it (mean, centred sum) and
//             leaves both in W.y for the second walk (SSB; Welch's weights), which needs the grand mean.  Brown-Forsythe sorts
//             by value first, regathers x and the ids in that order, and sorts by id: the index tie-break keeps value order
//             within an arm, so a run's median is its middle one or two elements.
//   record    lane 0, from a function per test.
#pragma once
#include "rank_cor.h"

namespace anofox {
namespace sampletest {

using cor::CorWork;
using glm::GiPL;

constexpr int kStRecordLen = 12; // {statistic, p_value, df, df2, estimate, ci_lower, ci_upper, n, n1, n2, aux, status}
constexpr int kStT = 0, kStYuen = 1, kStAnova = 2, kStBrownForsythe = 3, kStBrunnerMunzel = 4;
constexpr int kStWelch = 0, kStStudent = 1, kStPaired = 2; // the t-test's kinds
constexpr int kStFisher = 0, kStWelchAnova = 1;            // ANOVA's kinds
constexpr int kStStatusInsufficientData = 6;

struct SampleTestProblem {
	const double *v, *y;   // y: the paired t-test only
	const int32_t *sample; // every test but the paired t-test
	int64_t n_rows;        // row ranges are clipped to [0, n_rows)
	int test, alternative, kind;
	double mu, trim, confidence_level; // confidence_level NaN: no interval
	double *records;
};

// nullptr, or what is wrong with the options
GI_HD const char *st_options_text(int test, int alternative, int kind, double mu, double trim, double confidence_level) {
	if (test < kStT || test > kStBrunnerMunzel) return "sample test: unknown test";
	if (alternative < cor::kCorTwoSided || alternative > cor::kCorGreater) return "sample test: unknown alternative";
	const int kinds = test == kStT ? 3 : (test == kStAnova ? 2 : 1);
	if (kind < 0 || kind >= kinds) return "sample test: unknown kind";
	if (!(fabs(mu) <= DBL_MAX)) return "sample test: mu must be finite";
	if (test != kStT && mu != 0.0) return "sample test: only the t-test takes a mu";
	if (!(trim >= 0.0 && trim < 0.5)) return "sample test: trim must lie in [0, 0.5)";
	if (confidence_level == confidence_level && !(confidence_level > 0.0 && confidence_level < 1.0))
		return "sample test: confidence_level must lie in (0, 1)";
	return nullptr;
}

GI_HD bool st_paired(const SampleTestProblem &P) { return P.test == kStT && P.kind == kStPaired; }
GI_HD bool st_two_sample(int test) { return test == kStT || test == kStYuen || test == kStBrunnerMunzel; }

// ---- the t quantile ----

// P(T > t) of Student's t with df degrees of freedom, t >= 0
GI_DEV double st_t_upper(double t, double df) {
	RC_NO_CONTRACT
	const double t2 = t * t, d = df + t2;
	if (!glm::gi_finite(t2)) return 0.0;
	return 0.5 * cor::rc_betainc(0.5 * df, 0.5, df / d, t2 / d);
}

// z with P(Z > z) = tail, 0 < tail <= 1/2, of the standard normal: Acklam's rational approximation, then two Halley steps on erfc
// (host_math.h's normal_quantile in a text both builds share)
GI_DEV double st_normal_upper_quantile(double tail) {
	RC_NO_CONTRACT
	double x;
	if (tail < 0.02425) {
		const double q = sqrt(-2.0 * log(tail));
		x = -(((((-7.784894002430293e-03 * q - 3.223964580411365e-01) * q - 2.400758277161838e+00) * q - 2.549732539343734e+00) * q +
		       4.374664141464968e+00) * q + 2.938163982698783e+00) /
		    ((((7.784695709041462e-03 * q + 3.224671290700398e-01) * q + 2.445134137142996e+00) * q + 3.754408661907416e+00) * q + 1.0);
	} else {
		const double q = 0.5 - tail, r = q * q;
		x = (((((-3.969683028665376e+01 * r + 2.209460984245205e+02) * r - 2.759285104469687e+02) * r + 1.383577518672690e+02) * r -
		      3.066479806614716e+01) * r + 2.506628277459239e+00) * q /
		    (((((-5.447609879822406e+01 * r + 1.615858368580409e+02) * r - 1.556989798598866e+02) * r + 6.680131188771972e+01) * r -
		      1.328068155288572e+01) * r + 1.0);
	}
	for (int it = 0; it < 2; ++it) {
		const double e = tail - 0.5 * erfc(x * 0.70710678118654752440), u = e * 2.50662827463100050242 * exp(0.5 * x * x);
		x = x - u / (1.0 + 0.5 * x * u);
	}
	return x;
}

// t with P(T > t) = tail, 0 < tail < 1, for any df > 0.  The start is the Cornish-Fisher series around the normal quantile
// (Abramowitz & Stegun 26.7.5), which above df = 1e5 is the answer; below, Newton steps on the tail, kept inside a bracket that
// every evaluation narrows (a step that leaves it is replaced by the bracket's middle, or by doubling while there is no upper
// end), until a Newton step is below 1e-8 relative: the tail is convex, the steps converge quadratically, so the step after that one
// would be below 1e-15.
RC_CALL double st_t_quantile(double tail, double df) {
	RC_NO_CONTRACT
	if (!(tail > 0.0 && tail < 1.0) || !(df > 0.0)) return NAN;
	if (tail == 0.5) return 0.0;
	const double sign = tail > 0.5 ? -1.0 : 1.0; // the lower half by symmetry
	if (tail > 0.5) tail = 1.0 - tail;
	const double z = st_normal_upper_quantile(tail), z2 = z * z, r = 1.0 / df;
	const double g1 = z * (z2 + 1.0) * 0.25;
	const double g2 = z * ((5.0 * z2 + 16.0) * z2 + 3.0) * (1.0 / 96.0);
	const double g3 = z * (((3.0 * z2 + 19.0) * z2 + 17.0) * z2 - 15.0) * (1.0 / 384.0);
	const double g4 = z * ((((79.0 * z2 + 776.0) * z2 + 1482.0) * z2 - 1920.0) * z2 - 945.0) * (1.0 / 92160.0);
	double t = z + r * (g1 + r * (g2 + r * (g3 + r * g4)));
	if (df > 1e5) return sign * t;
	if (!(t > 0.0) || !glm::gi_finite(t)) t = 1.0; // (the series is no use at a small df and a far tail)
	const double lnc = lgamma(0.5 * (df + 1.0)) - lgamma(0.5 * df) - 0.5 * log(df * 3.14159265358979323846);
	double lo = 0.0, hi = INFINITY;
	GI_NOUNROLL
	for (int it = 0; it < 1200; ++it) {
		const double u = st_t_upper(t, df);
		if (u > tail) lo = t;
		else hi = t;
		const double pdf = exp(lnc - 0.5 * (df + 1.0) * log1p(t * t / df));
		const double tn = t + (u - tail) / pdf;
		// only a Newton step ends the search.  At the root the step rounds to 0 and tn is the end of the bracket that t has just
		// become: the bracket is closed here, or the converged t would be given up for the bracket's middle, which within 2e-8
		// of the start passed for a small step and was returned 1e-8 off.
		if (tn >= lo && tn <= hi && fabs(tn - t) <= 1e-8 * fabs(tn)) return sign * tn;
		t = tn > lo && tn < hi ? tn : (glm::gi_finite(hi) ? 0.5 * (lo + hi) : 2.0 * t);
	}
	return sign * t;
}

// ---- the records ----

GI_DEV void st_write_failed(double *rec, double n, double n1, double n2) {
	for (int j = 0; j < kStRecordLen; ++j) rec[j] = NAN;
	rec[7] = n;
	rec[8] = n1;
	rec[9] = n2;
	rec[11] = (double)kStStatusInsufficientData;
}

// The record of a studentised estimate: t = num / se on df degrees of freedom, the interval around `est` (R's rule: a one-sided
// alternative leaves its far side open).  se not > 0: statistic, p, df and the interval are NaN.
GI_DEV void st_write_t(const SampleTestProblem &P, double est, double num, double se, double df, double n, double n1, double n2, double *rec) {
	RC_NO_CONTRACT
	double t = NAN, p = NAN, lo = NAN, hi = NAN;
	if (se > 0.0) {
		t = num / se;
		p = cor::rc_t_p(t, df, P.alternative);
		const double cl = P.confidence_level;
		if (cl == cl) {
			if (P.alternative == cor::kCorTwoSided) {
				const double q = st_t_quantile(0.5 * (1.0 - cl), df);
				lo = est - q * se;
				hi = est + q * se;
			} else {
				const double q = st_t_quantile(1.0 - cl, df);
				lo = P.alternative == cor::kCorLess ? -INFINITY : est - q * se;
				hi = P.alternative == cor::kCorLess ? est + q * se : INFINITY;
			}
		}
	} else {
		df = NAN;
	}
	rec[0] = t;
	rec[1] = p;
	rec[2] = df;
	rec[3] = NAN;
	rec[4] = est;
	rec[5] = lo;
	rec[6] = hi;
	rec[7] = n;
	rec[8] = n1;
	rec[9] = n2;
	rec[10] = se;
	rec[11] = 0.0;
}

// the counts, means and centred sums of the two arms (the paired t-test: of d = v - y, in arm 1)
struct StArms {
	int64_t n1, n2;
	double m1, m2, s1, s2;
};

RC_CALL void st_t_record(const SampleTestProblem &P, const StArms &A, double *rec) {
	RC_NO_CONTRACT
	const double d1 = (double)A.n1, d2 = (double)A.n2;
	if (P.kind == kStPaired) {
		if (A.n1 < 2) {
			st_write_failed(rec, d1, d1, d1);
			return;
		}
		const double se = sqrt(A.s1 / (d1 - 1.0) / d1);
		st_write_t(P, A.m1, A.m1 - P.mu, se, d1 - 1.0, d1, d1, d1, rec);
		return;
	}
	if (A.n1 < 2 || A.n2 < 2) {
		st_write_failed(rec, d1 + d2, d1, d2);
		return;
	}
	const double est = A.m1 - A.m2;
	double se, df;
	if (P.kind == kStStudent) {
		df = d1 + d2 - 2.0;
		se = sqrt((A.s1 + A.s2) / df * (1.0 / d1 + 1.0 / d2));
	} else {
		const double a = A.s1 / (d1 - 1.0) / d1, b = A.s2 / (d2 - 1.0) / d2;
		se = sqrt(a + b);
		df = (a + b) * (a + b) / (a * a / (d1 - 1.0) + b * b / (d2 - 1.0));
	}
	st_write_t(P, est, est - P.mu, se, df, d1 + d2, d1, d2, rec);
}

// g = floor(trim n) rows leave each tail of an arm of n rows; h = n - 2 g stay
GI_DEV int64_t st_trim_count(double trim, int64_t n) {
	RC_NO_CONTRACT
	return (int64_t)floor(trim * (double)n);
}

GI_DEV bool st_yuen_insufficient(double trim, int64_t n1, int64_t n2) {
	return n1 < 4 || n2 < 4 || n1 - 2 * st_trim_count(trim, n1) < 2 || n2 - 2 * st_trim_count(trim, n2) < 2;
}

// Yuen's record from each arm's trimmed mean tm and winsorised centred sum sw (sum (w - mean w)^2)
RC_CALL void st_yuen_record(const SampleTestProblem &P, int64_t n1, int64_t n2, double tm1, double sw1, double tm2, double sw2, double *rec) {
	RC_NO_CONTRACT
	const double c1 = (double)n1, c2 = (double)n2;
	if (st_yuen_insufficient(P.trim, n1, n2)) {
		st_write_failed(rec, c1 + c2, c1, c2);
		return;
	}
	const double h1 = (double)(n1 - 2 * st_trim_count(P.trim, n1)), h2 = (double)(n2 - 2 * st_trim_count(P.trim, n2));
	const double d1 = sw1 / (h1 * (h1 - 1.0)), d2 = sw2 / (h2 * (h2 - 1.0)); // (n - 1) sw^2 = the centred sum
	const double est = tm1 - tm2, se = sqrt(d1 + d2);
	const double df = (d1 + d2) * (d1 + d2) / (d1 * d1 / (h1 - 1.0) + d2 * d2 / (h2 - 1.0));
	st_write_t(P, est, est, se, df, c1 + c2, c1, c2, rec);
}

// the sums of the k arms of a k-sample test
struct StAnova {
	int64_t k, n, min_arm; // min_arm: the rows of the smallest arm
	double ssb, ssw;
	double wnum, wtmp;     // Welch: sum w_j (m_j - mtilde)^2 and sum (1 - w_j / sum w)^2 / (n_j - 1)
	int64_t flat;          // Welch: the arms whose variance is not > 0
};

// the upper tail of F(df, df2)
GI_DEV double st_f_p(double f, double df, double df2) {
	RC_NO_CONTRACT
	if (f != f || df2 != df2) return NAN;
	if (!glm::gi_finite(f)) return f > 0.0 ? 0.0 : 1.0;
	const double d = df2 + df * f;
	return cor::rc_betainc(0.5 * df2, 0.5 * df, df2 / d, df * f / d);
}

RC_CALL void st_anova_record(const SampleTestProblem &P, const StAnova &A, double *rec) {
	RC_NO_CONTRACT
	const double dk = (double)A.k, dn = (double)A.n;
	if (A.k < 2 || A.min_arm < 2) {
		st_write_failed(rec, dn, dk, NAN);
		return;
	}
	const double df = dk - 1.0;
	double f, df2, p;
	if (P.test == kStAnova && P.kind == kStWelchAnova) {
		if (A.flat > 0) {
			f = df2 = p = NAN;
		} else {
			const double tmp = A.wtmp / (dk * dk - 1.0);
			f = A.wnum / (df * (1.0 + 2.0 * (dk - 2.0) * tmp));
			df2 = 1.0 / (3.0 * tmp);
			p = st_f_p(f, df, df2);
		}
	} else {
		df2 = dn - dk;
		if (A.ssw > 0.0 || A.ssw != A.ssw) {
			f = (A.ssb / df) / (A.ssw / df2);
			p = st_f_p(f, df, df2);
		} else if (A.ssb > 0.0) {
			f = INFINITY;
			p = 0.0;
		} else {
			f = p = NAN;
		}
	}
	rec[0] = f;
	rec[1] = p;
	rec[2] = df;
	rec[3] = df2;
	rec[4] = A.ssb;
	rec[5] = NAN;
	rec[6] = NAN;
	rec[7] = dn;
	rec[8] = dk;
	rec[9] = NAN;
	rec[10] = A.ssw;
	rec[11] = 0.0;
}

// Brunner-Munzel's record from the arm sums r1, r2 of the pooled midranks and the centred placement sums q1, q2
RC_CALL void st_brunner_munzel_record(const SampleTestProblem &P, int64_t n1, int64_t n2, double r1, double r2, double q1, double q2, double *rec) {
	RC_NO_CONTRACT
	const double d1 = (double)n1, d2 = (double)n2;
	if (n1 < 2 || n2 < 2) {
		st_write_failed(rec, d1 + d2, d1, d2);
		return;
	}
	const double v1 = q1 / (d1 - 1.0), v2 = q2 / (d2 - 1.0);
	const double phat = (r2 / d2 - (d2 + 1.0) / 2.0) / d1;
	const double a = d1 * v1, b = d2 * v2;
	const double se = sqrt(v1 / (d1 * d2 * d2) + v2 / (d2 * d1 * d1));
	// (`greater`, sample 1 stochastically greater, is the lower tail of W, whose sign is sample 2's)
	const int tail = P.alternative == cor::kCorTwoSided ? cor::kCorTwoSided : (P.alternative == cor::kCorLess ? cor::kCorGreater : cor::kCorLess);
	double w, df = NAN, lo = phat, hi = phat;
	if (a + b > 0.0 || a + b != a + b) {
		w = d1 * d2 * (r2 / d2 - r1 / d1) / ((d1 + d2) * sqrt(a + b));
		df = (a + b) * (a + b) / (a * a / (d1 - 1.0) + b * b / (d2 - 1.0));
		if (P.confidence_level == P.confidence_level) {
			const double q = st_t_quantile(0.5 * (1.0 - P.confidence_level), df);
			lo = phat - q * se;
			hi = phat + q * se;
		} else {
			lo = hi = NAN;
		}
	} else {
		w = phat > 0.5 ? INFINITY : (phat < 0.5 ? -INFINITY : NAN);
		if (P.confidence_level != P.confidence_level) lo = hi = NAN;
	}
	rec[0] = w;
	rec[1] = cor::rc_t_p(w, df, tail);
	rec[2] = df;
	rec[3] = NAN;
	rec[4] = phat;
	rec[5] = lo;
	rec[6] = hi;
	rec[7] = d1 + d2;
	rec[8] = d1;
	rec[9] = d2;
	rec[10] = se;
	rec[11] = 0.0;
}

// ---- the phases of one wavefront ----

// One row of the unstaged t-test: its datum in a, its arm (0 or 1) -> the row is valid
GI_DEV bool st_t_row(const SampleTestProblem &P, int64_t i, double &a, int &arm) {
	RC_NO_CONTRACT
	const double v = P.v[i];
	if (P.kind == kStPaired) {
		const double d = v - P.y[i];
		a = d;
		arm = 0;
		return d - P.mu == d - P.mu;
	}
	a = v;
	arm = P.sample[i] == 0 ? 0 : 1;
	return v == v;
}

// The t-test's two streaming passes over rows [lo, hi): counts and means, then centred sums
GI_DEV StArms st_t_moments(const SampleTestProblem &P, int64_t lo, int64_t hi) {
	RC_NO_CONTRACT
	GiPL<double> s1, s2;
	GiPL<int64_t> c1, c2;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane);
	double a1 = 0.0, a2 = 0.0;
	int64_t k1 = 0, k2 = 0;
	for (int64_t i = lo + lane; i < hi; i += 64) {
		double a;
		int arm;
		if (!st_t_row(P, i, a, arm)) continue;
		if (arm == 0) {
			a1 += a;
			++k1;
		} else {
			a2 += a;
			++k2;
		}
	}
	s1.v[L] = a1;
	s2.v[L] = a2;
	c1.v[L] = k1;
	c2.v[L] = k2;
	GI_LANES_END
	StArms A;
	A.n1 = glm::gi_sum_i(c1);
	A.n2 = glm::gi_sum_i(c2);
	A.m1 = glm::gi_sum(s1) / (double)A.n1;
	A.m2 = glm::gi_sum(s2) / (double)A.n2;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane);
	double a1 = 0.0, a2 = 0.0;
	for (int64_t i = lo + lane; i < hi; i += 64) {
		double a;
		int arm;
		if (!st_t_row(P, i, a, arm)) continue;
		const double d = a - (arm == 0 ? A.m1 : A.m2);
		if (arm == 0) a1 += d * d;
		else a2 += d * d;
	}
	s1.v[L] = a1;
	s2.v[L] = a2;
	GI_LANES_END
	A.s1 = glm::gi_sum(s1);
	A.s2 = glm::gi_sum(s2);
	return A;
}

// the valid rows of [lo, hi) that belong to sample 1
GI_DEV int64_t st_count_first(const SampleTestProblem &P, int64_t lo, int64_t hi) {
	GiPL<int64_t> c;
	GI_LANES_BEGIN(lane)
	int64_t k = 0;
	for (int64_t i = lo + lane; i < hi; i += 64) k += P.v[i] == P.v[i] && P.sample[i] == 0;
	c.v[GI_AT(lane)] = k;
	GI_LANES_END
	return glm::gi_sum_i(c);
}

// The valid rows of [lo, hi) to W.x in their order, sample 1 (n1 rows) to [0, n1) and sample 2 behind it -> their number
GI_DEV int64_t st_compact_two(const SampleTestProblem &P, int64_t lo, int64_t hi, const CorWork &W, int64_t n1) {
	int64_t a = 0, b = n1;
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	const unsigned long long below = (1ull << lane) - 1ull;
	for (int64_t base = lo; base < hi; base += 64) {
		const int64_t i = base + lane;
		double v = NAN;
		bool first = false;
		if (i < hi) {
			v = P.v[i];
			first = P.sample[i] == 0;
		}
		const bool ok = v == v;
		const unsigned long long m1 = __ballot(ok && first), m2 = __ballot(ok && !first);
		if (ok) W.x[first ? a + __popcll(m1 & below) : b + __popcll(m2 & below)] = v;
		a += __popcll(m1);
		b += __popcll(m2);
	}
#else
	for (int64_t i = lo; i < hi; ++i) {
		const double v = P.v[i];
		if (v != v) continue;
		if (P.sample[i] == 0) W.x[a++] = v;
		else W.x[b++] = v;
	}
#endif
	return b;
}

// the valid rows of [lo, hi) to W.x, their sample ids (as doubles, exact for int32) to W.y, in their order -> their number
GI_DEV int64_t st_compact_ids(const SampleTestProblem &P, int64_t lo, int64_t hi, const CorWork &W) {
	int64_t n = 0;
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	for (int64_t base = lo; base < hi; base += 64) {
		const int64_t i = base + lane;
		double v = NAN;
		int32_t s = 0;
		if (i < hi) {
			v = P.v[i];
			s = P.sample[i];
		}
		const bool ok = v == v;
		const unsigned long long mask = __ballot(ok);
		if (ok) {
			const int64_t at = n + __popcll(mask & ((1ull << lane) - 1ull));
			W.x[at] = v;
			W.y[at] = (double)s;
		}
		n += __popcll(mask);
	}
#else
	for (int64_t i = lo; i < hi; ++i) {
		if (P.v[i] != P.v[i]) continue;
		W.x[n] = P.v[i];
		W.y[n] = (double)P.sample[i];
		++n;
	}
#endif
	return n;
}

// One arm of Yuen's test from its n sorted values: the trimmed mean in tm -> the centred sum of the winsorised values
GI_DEV double st_yuen_arm(const double *key, int64_t n, double trim, double &tm) {
	RC_NO_CONTRACT
	const int64_t g = st_trim_count(trim, n), top = n - g - 1;
	GiPL<double> s0, s1;
	GI_LANES_BEGIN(lane)
	double a = 0.0, b = 0.0;
	for (int64_t i = lane; i < n; i += 64) {
		const double w = key[i < g ? g : (i > top ? top : i)];
		a += w;
		if (i >= g && i <= top) b += w;
	}
	s0.v[GI_AT(lane)] = a;
	s1.v[GI_AT(lane)] = b;
	GI_LANES_END
	const double mw = glm::gi_sum(s0) / (double)n;
	tm = glm::gi_sum(s1) / (double)(n - 2 * g);
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	for (int64_t i = lane; i < n; i += 64) {
		const double d = key[i < g ? g : (i > top ? top : i)] - mw;
		a += d * d;
	}
	s0.v[GI_AT(lane)] = a;
	GI_LANES_END
	return glm::gi_sum(s0);
}

// One arm of Brunner-Munzel's test, n rows with the pooled midranks in R and the arm's own in r: the sum of R in sum_r -> the
// sum of (R - r - Rbar + (n + 1)/2)^2
GI_DEV double st_placement_arm(const double *R, const double *r, int64_t n, double &sum_r) {
	RC_NO_CONTRACT
	GiPL<double> s;
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	for (int64_t i = lane; i < n; i += 64) a += R[i];
	s.v[GI_AT(lane)] = a;
	GI_LANES_END
	sum_r = glm::gi_sum(s);
	const double shift = ((double)n + 1.0) / 2.0 - sum_r / (double)n;
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	for (int64_t i = lane; i < n; i += 64) {
		const double d = R[i] - r[i] + shift;
		a += d * d;
	}
	s.v[GI_AT(lane)] = a;
	GI_LANES_END
	return glm::gi_sum(s);
}

// (key, idx) sorted by value: x and the ids regathered in that order (x from the keys, the ids through idx into key), idx reset:
// what rc_fill_keys would leave for a group whose rows came in value order
GI_DEV void st_regather(const CorWork &W, int64_t n) {
	GI_LANES_BEGIN(lane)
	for (int64_t i = lane; i < n; i += 64) {
		const int32_t from = W.idx[i];
		W.x[i] = W.key[i];
		W.key[i] = W.y[from]; // (W.y is only read here: no lane's write is another's read)
		W.idx[i] = (int32_t)i;
	}
	GI_LANES_END
}

// the datum of sorted position e of a run: the value, or for Brown-Forsythe its distance from the run's median
GI_DEV double st_arm_datum(const CorWork &W, int64_t e, bool spread, double med) {
	RC_NO_CONTRACT
	const double v = W.x[W.idx[e]];
	return spread ? fabs(v - med) : v;
}

// (key, idx) sorted by sample id (Brown-Forsythe: by id, then value): the sums of the arms.  The lane that finds the first element
// of a run walks it; W.y (free once the ids are keys) keeps the run's mean and centred sum at the run's first two places.
GI_DEV StAnova st_arm_sums(const CorWork &W, int64_t n, bool spread, bool welch) {
	RC_NO_CONTRACT
	GiPL<double> s0, s1, s2, s3;
	GiPL<int64_t> c0, c1, c2;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane);
	double tot = 0.0, ssw = 0.0, sw = 0.0, swm = 0.0;
	int64_t k = 0, least = INT64_MAX, flat = 0;
	for (int64_t i = lane; i < n; i += 64) {
		const double id = W.key[i];
		if (i > 0 && W.key[i - 1] == id) continue; // not the first of its run
		int64_t e = i + 1;
		while (e < n && W.key[e] == id) ++e;
		const int64_t t = e - i;
		double med = 0.0;
		if (spread) med = (t & 1) ? W.x[W.idx[i + t / 2]] : 0.5 * (W.x[W.idx[i + t / 2 - 1]] + W.x[W.idx[i + t / 2]]);
		double sum = 0.0, cs = 0.0;
		for (int64_t q = i; q < e; ++q) sum += st_arm_datum(W, q, spread, med);
		const double m = sum / (double)t;
		for (int64_t q = i; q < e; ++q) {
			const double d = st_arm_datum(W, q, spread, med) - m;
			cs += d * d;
		}
		W.y[i] = m;
		if (t >= 2) W.y[i + 1] = cs;
		tot += sum;
		ssw += cs;
		++k;
		if (t < least) least = t;
		if (welch && t >= 2) {
			const double var = cs / (double)(t - 1);
			if (var > 0.0) {
				const double w = (double)t / var;
				sw += w;
				swm += w * m;
			} else {
				++flat;
			}
		}
	}
	s0.v[L] = tot;
	s1.v[L] = ssw;
	s2.v[L] = sw;
	s3.v[L] = swm;
	c0.v[L] = k;
	c1.v[L] = least;
	c2.v[L] = flat;
	GI_LANES_END
	StAnova A;
	A.n = n;
	A.k = glm::gi_sum_i(c0);
	A.min_arm = glm::gi_min_i(c1);
	A.flat = glm::gi_sum_i(c2);
	A.ssw = glm::gi_sum(s1);
	A.ssb = A.wnum = A.wtmp = NAN;
	const double grand = glm::gi_sum(s0) / (double)n, wsum = glm::gi_sum(s2), wmean = glm::gi_sum(s3) / wsum;
	if (A.k < 2 || A.min_arm < 2) return A;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane);
	double ssb = 0.0, num = 0.0, tmp = 0.0;
	for (int64_t i = lane; i < n; i += 64) {
		const double id = W.key[i];
		if (i > 0 && W.key[i - 1] == id) continue;
		int64_t e = i + 1;
		while (e < n && W.key[e] == id) ++e;
		const double t = (double)(e - i), m = W.y[i], cs = W.y[i + 1]; // (every run has two rows here)
		ssb += t * ((m - grand) * (m - grand));
		if (welch && A.flat == 0) {
			const double w = t / (cs / (t - 1.0)), r = 1.0 - w / wsum;
			num += w * ((m - wmean) * (m - wmean));
			tmp += r * r / (t - 1.0);
		}
	}
	s0.v[L] = ssb;
	s1.v[L] = num;
	s2.v[L] = tmp;
	GI_LANES_END
	A.ssb = glm::gi_sum(s0);
	A.wnum = glm::gi_sum(s1);
	A.wtmp = glm::gi_sum(s2);
	return A;
}

// ---- one group ----
// Rows [lo, hi) of group g, W as long as the group (the t-test does not touch it).  `lead`: this thread belongs to the wavefront
// that runs every phase but the sorts (the only wavefront of the small path); tid / threads: the sorts'.
GI_DEV void st_group(const SampleTestProblem &P, int64_t g, int64_t lo, int64_t hi, const CorWork &W, bool lead, int64_t tid, int64_t threads) {
	double *rec = P.records + g * kStRecordLen;
	if (P.test == kStT) {
		if (!lead) return;
		const StArms A = st_t_moments(P, lo, hi);
		GI_LANES_BEGIN(lane)
		if (lane == 0) st_t_record(P, A, rec);
		GI_LANES_END
		return;
	}
	const bool two = st_two_sample(P.test);
	int64_t n = 0, n1 = 0;
	if (lead) {
		if (two) {
			n1 = st_count_first(P, lo, hi);
			n = st_compact_two(P, lo, hi, W, n1);
		} else {
			n = st_compact_ids(P, lo, hi, W);
		}
	}
#if defined(__HIPCC__)
	if (threads > 64) { // the other wavefronts of the workgroup learn n and n1 through the first two index slots (a group of the
		                // large path has more rows than a cap of at least one)
		const bool room = hi - lo >= 2;
		if (lead && (threadIdx.x & 63u) == 0 && room) {
			W.idx[0] = (int32_t)n;
			W.idx[1] = (int32_t)n1;
		}
		glm::gi_sync();
		if (room) {
			n = W.idx[0];
			n1 = W.idx[1];
		}
		glm::gi_sync();
	}
#endif
	// (n and n1 are the same in every thread: the barriers of the sorts are met by all)
	if (two) {
		const int64_t n2 = n - n1;
		const CorWork A = {W.x, W.y, W.key, W.idx}, B = {W.x + n1, W.y + n1, W.key + n1, W.idx + n1};
		if (P.test == kStBrunnerMunzel) { // the pooled midranks to W.y, before the arms' own replace the values
			if (lead) cor::rc_fill_keys(W.x, n, W);
			cor::rc_sort(W, n, tid, threads);
			if (lead) cor::rc_runs(W, n, W.y);
			glm::gi_sync();
		}
		if (lead) cor::rc_fill_keys(A.x, n1, A);
		cor::rc_sort(A, n1, tid, threads);
		if (lead && P.test == kStBrunnerMunzel) cor::rc_runs(A, n1, A.x);
		glm::gi_sync();
		if (lead) cor::rc_fill_keys(B.x, n2, B);
		cor::rc_sort(B, n2, tid, threads);
		if (lead && P.test == kStBrunnerMunzel) cor::rc_runs(B, n2, B.x);
		glm::gi_sync();
		if (!lead) return;
		if (P.test == kStYuen) {
			double tm1 = NAN, tm2 = NAN, sw1 = NAN, sw2 = NAN;
			if (!st_yuen_insufficient(P.trim, n1, n2)) {
				sw1 = st_yuen_arm(A.key, n1, P.trim, tm1);
				sw2 = st_yuen_arm(B.key, n2, P.trim, tm2);
			}
			GI_LANES_BEGIN(lane)
			if (lane == 0) st_yuen_record(P, n1, n2, tm1, sw1, tm2, sw2, rec);
			GI_LANES_END
			return;
		}
		double r1 = 0.0, r2 = 0.0;
		const double q1 = st_placement_arm(A.y, A.x, n1, r1), q2 = st_placement_arm(B.y, B.x, n2, r2);
		GI_LANES_BEGIN(lane)
		if (lane == 0) st_brunner_munzel_record(P, n1, n2, r1, r2, q1, q2, rec);
		GI_LANES_END
		return;
	}
	const bool spread = P.test == kStBrownForsythe;
	if (spread) {
		if (lead) cor::rc_fill_keys(W.x, n, W);
		cor::rc_sort(W, n, tid, threads);
		if (lead) st_regather(W, n);
	} else if (lead) {
		cor::rc_fill_keys(W.y, n, W);
	}
	cor::rc_sort(W, n, tid, threads);
	if (!lead) return;
	const StAnova S = st_arm_sums(W, n, spread, P.test == kStAnova && P.kind == kStWelchAnova);
	GI_LANES_BEGIN(lane)
	if (lane == 0) st_anova_record(P, S, rec);
	GI_LANES_END
}

} // namespace sampletest
} // namespace anofox
