// categorical_tests.h — the categorical tests of one group of rows of two int32 label columns: the chi-square test of independence
// with Cramer's V, Pearson's contingency coefficient and phi (R's chisq.test, scipy's chi2_contingency and contingency.association),
// the G-test, Fisher's exact test of a 2 x 2 table (R's fisher.test: the hypergeometric p-values, the conditional maximum-likelihood
// odds ratio and its exact interval) and McNemar's test.  The reference's chisq_test, g_test, fisher_exact and mcnemar_test are
// wrappers around a crate that is not restated here; the codings of the 2 x 2 tests are its aggregates'.  DESIGN.md §1,
// "Categorical tests".
//
//     input: two int32 columns a (the row variable) and b (the column variable);  valid row: neither entry is INT32_MIN (the NULL
//           of this family); every other int32 is a label
//     record {statistic, p_value, df, estimate, ci_lower, ci_upper, n, n_row_levels, n_col_levels, aux, aux2, status}
//     status 6: no valid row; tests 0 and 1 fewer than 2 distinct labels on either side; tests 2 and 3 no counted row.  Every field
//           but n and the two level counts is NaN.
//     chi-square (0)  the table of the r distinct labels of a by the c distinct labels of b (coded densely in ascending order: no
//           empty margin).  X2 = n (sum O^2/(R C) - 1), evaluated without the cancellation as
//           (sum over the occupied cells of (O n - R C)^2 / (R C) + n^2 - sum over the occupied cells of R C) / n: the integers are
//           exact, every term is >= 0, an independent table gives 0.  correction on a 2 x 2 table: Yates' form with the correction
//           clipped to min(1/2, |O - E|), (|O - E| - y)^2 n^3 / (R1 R2 C1 C2), |O - E| = |n11 n22 - n12 n21| / n in all four cells.
//           df = (r - 1)(c - 1), p = Q(df/2, X2/2) (rank_tests.h).  estimate = V = sqrt(X2/(n min(r - 1, c - 1))), aux = C =
//           sqrt(X2/(X2 + n)), aux2 = phi = (n11 n22 - n12 n21)/sqrt(R1 R2 C1 C2) on a 2 x 2 table (else NaN); all three from the
//           uncorrected X2.
//     G (1)     G = 2 sum O ln(O n/(R C)) over the occupied cells, df and p as above; estimate, aux, aux2 NaN.
//     Fisher (2)  only rows with both labels in {0, 1} are counted: n11 = (0, 0), n12 = (0, 1), n21 = (1, 0), n22 = (1, 1), n their
//           number.  With m = R1, k = C1 and the support lo = max(0, R1 - C2) .. hi = min(R1, C1) of x = n11:
//           log dc(s) = -(lgamma(s + 1) + lgamma(m - s + 1) + lgamma(k - s + 1) + lgamma(R2 - k + s + 1)) (up to a constant),
//           P_theta(s) proportional to exp(log dc(s) + theta s), theta the log odds ratio; the weights are scaled by their maximum
//           before they are summed.  p at theta = 0: less P(X <= x), greater P(X >= x), two-sided the sum of the P(s) <= P(x)
//           (1 + 1e-7), compared as log P(s) <= log P(x) + log(1 + 1e-7).  statistic = n11 n22/(n12 n21) (0/0: NaN).  estimate = the
//           conditional MLE: x = lo: 0, x = hi: +inf, else exp of the root of E_theta X = x.  Interval at confidence_level (NaN:
//           none): two-sided alpha = (1 - level)/2, lower = the root of P_theta(X >= x) = alpha (x = lo: 0), upper = the root of
//           P_theta(X <= x) = alpha (x = hi: +inf); less [0, upper at 1 - level]; greater [lower at 1 - level, +inf].  The roots: a
//           bracket grown from theta = 0 by doubling steps, then the Illinois false position.  df NaN, level counts 2.
//     McNemar (3)  a label of 0 is "0", every other label "1";  b = n01, c = n10.  exact == 0: (|b - c| - 1)^2/(b + c) with
//           correction, else (b - c)^2/(b + c), chi-square with 1 df.  exact != 0: p = min(1, 2 P(X <= min(b, c))), X ~ Bin(b + c,
//           1/2), statistic and df NaN.  b + c = 0: status 0 with statistic and p NaN.  estimate = b/c, aux = b, aux2 = c.
//
// One source for both builds, as normality_tests.h: under hipcc device code, under a plain C++ compiler a wavefront is a loop over 64
// lanes (tests/tools/categorical_test_host.cpp).  Contraction of a * b + c is switched off in every body.
//
//   tests 2, 3  nothing is staged: the group's wavefront streams the rows once and counts four cells.
//   tests 0, 1  no dense table is built.  The valid rows are compacted (W.x = a, W.y = b) and sorted by b.  Row q of that order
//           finds the first row of its column by bisection: W.y[q] = the column's start, a dense-enough code that ascends with b.
//           The keys become a in the order by b with idx = q, W.x[start] takes the column's count, and the second sort, by a with
//           ties by q, puts every cell's rows side by side.  The lane that holds a cell's first row finds the ends of its row and
//           of the cell by bisection (within a row the column starts ascend) and adds the cell's term; the partials meet in the
//           fixed-order butterfly.  Every count is an integer.  No walk is longer than log2 n steps.
//   record    lane 0, from a function per test family; the functions take counts and sums and also serve the table- and
//           cell-taking scalars, which touch no device.
#pragma once
#include "rank_tests.h"

namespace anofox {
namespace cattest {

using cor::CorWork;
using glm::GiPL;

constexpr int kCtRecordLen = 12; // {statistic, p_value, df, estimate, ci_lower, ci_upper, n, n_row_levels, n_col_levels, aux, aux2, status}
constexpr int kCtChiSquare = 0, kCtG = 1, kCtFisher = 2, kCtMcNemar = 3;
constexpr int kCtStatusInsufficientData = 6; // ANOFOX_ERROR_INSUFFICIENT_DATA
constexpr int32_t kCtNull = INT32_MIN;
constexpr double kCtTieSlack = 9.9999995000000333e-8; // log(1 + 1e-7): R's relative slack of the two-sided Fisher p
constexpr int kCtRootSteps = 200;

struct CategoricalProblem {
	const int32_t *a, *b;
	int64_t n_rows; // row ranges are clipped to [0, n_rows)
	int test, alternative, correction, exact;
	double confidence_level; // NaN: no interval
	double *records;
};

// nullptr, or what is wrong with the options
GI_HD const char *ct_options_text(int test, int alternative, double confidence_level) {
	if (test < kCtChiSquare || test > kCtMcNemar) return "categorical test: unknown test";
	if (alternative < cor::kCorTwoSided || alternative > cor::kCorGreater) return "categorical test: unknown alternative";
	if (confidence_level == confidence_level && !(confidence_level > 0.0 && confidence_level < 1.0))
		return "categorical test: confidence_level must lie in (0, 1) or be NaN";
	return nullptr;
}

GI_HD bool ct_staged(int test) { return test == kCtChiSquare || test == kCtG; }

// ---- the records ----

GI_DEV void ct_write_failed(double *rec, double n, double r, double c) {
	for (int j = 0; j < kCtRecordLen; ++j) rec[j] = NAN;
	rec[6] = n;
	rec[7] = r;
	rec[8] = c;
	rec[11] = (double)kCtStatusInsufficientData;
}

// what the walks of a table leave: the counts, the two sums over the occupied cells, and of a 2 x 2 table the first cell and margins
struct CtTable {
	int64_t n, r, c;
	double sum;     // chi-square: sum (O n - R C)^2 / (R C);  G: sum O ln(O n / (R C))
	int64_t sum_rc; // sum R C
	int64_t n11, r1, c1; // the cell of the smallest labels, its row's and its column's totals (read when r = c = 2)
};

// one occupied cell's term of CtTable::sum
GI_DEV double ct_cell_term(int test, int64_t o, int64_t r, int64_t c, int64_t n) {
	RC_NO_CONTRACT
	const double rc = (double)r * (double)c;
	if (test == kCtG) return (double)o * log((double)o * (double)n / rc);
	const double d = (double)(o * n - r * c);
	return d * d / rc;
}

// the chi-square and the G record
RC_CALL void ct_table_record(int test, int correction, const CtTable &T, double *rec) {
	RC_NO_CONTRACT
	const double n = (double)T.n;
	if (T.n < 1 || T.r < 2 || T.c < 2) {
		ct_write_failed(rec, n, (double)T.r, (double)T.c);
		return;
	}
	const double df = (double)(T.r - 1) * (double)(T.c - 1);
	double stat, v = NAN, cc = NAN, phi = NAN;
	if (test == kCtG) {
		stat = 2.0 * T.sum;
	} else {
		const double x2 = (T.sum + (double)(T.n * T.n - T.sum_rc)) / n;
		stat = x2;
		const int64_t least = T.r < T.c ? T.r - 1 : T.c - 1;
		v = sqrt(x2 / (n * (double)least));
		cc = sqrt(x2 / (x2 + n));
		if (T.r == 2 && T.c == 2) {
			const int64_t n12 = T.r1 - T.n11, n21 = T.c1 - T.n11, n22 = T.n - T.r1 - T.c1 + T.n11;
			const double det = (double)(T.n11 * n22 - n12 * n21);
			const double margins = (double)T.r1 * (double)(T.n - T.r1) * (double)T.c1 * (double)(T.n - T.c1);
			phi = det / sqrt(margins);
			if (correction) {
				const double d = fabs(det) / n, y = d < 0.5 ? d : 0.5;
				stat = (d - y) * (d - y) * n * n * n / margins;
			}
		}
	}
	rec[0] = stat;
	rec[1] = ranktest::rt_gamma_q(0.5 * df, 0.5 * stat);
	rec[2] = df;
	rec[3] = v;
	rec[4] = NAN;
	rec[5] = NAN;
	rec[6] = n;
	rec[7] = (double)T.r;
	rec[8] = (double)T.c;
	rec[9] = cc;
	rec[10] = phi;
	rec[11] = 0.0;
}

// McNemar's record from the four cells (n00, b = n01, c = n10, n11)
RC_CALL void ct_mcnemar_record(int correction, int exact, int64_t n00, int64_t b, int64_t c, int64_t n11, double *rec) {
	RC_NO_CONTRACT
	const int64_t n = n00 + b + c + n11, d = b + c;
	if (n < 1) {
		ct_write_failed(rec, 0.0, 2.0, 2.0);
		return;
	}
	double stat = NAN, p = NAN;
	if (d > 0 && exact) {
		const int64_t k = b < c ? b : c; // (k <= d/2 < d)
		p = 2.0 * cor::rc_betainc((double)(d - k), (double)(k + 1), 0.5, 0.5);
		if (p > 1.0) p = 1.0;
	} else if (d > 0) {
		double num = fabs((double)(b - c));
		if (correction) num -= 1.0;
		stat = num * num / (double)d;
		p = ranktest::rt_gamma_q(0.5, 0.5 * stat);
	}
	rec[0] = stat;
	rec[1] = p;
	rec[2] = exact ? NAN : 1.0;
	rec[3] = (double)b / (double)c;
	rec[4] = NAN;
	rec[5] = NAN;
	rec[6] = (double)n;
	rec[7] = 2.0;
	rec[8] = 2.0;
	rec[9] = (double)b;
	rec[10] = (double)c;
	rec[11] = 0.0;
}

// ---- Fisher's exact test: the noncentral hypergeometric distribution over the lanes ----

struct CtHyper {
	int64_t m, n2, k, lo, hi, x; // R1, R2, C1, the support, the observed n11
};

GI_DEV CtHyper ct_hyper(int64_t n11, int64_t n12, int64_t n21, int64_t n22) {
	CtHyper H;
	H.m = n11 + n12;
	H.n2 = n21 + n22;
	H.k = n11 + n21;
	H.lo = H.k - H.n2 > 0 ? H.k - H.n2 : 0;
	H.hi = H.k < H.m ? H.k : H.m;
	H.x = n11;
	return H;
}

GI_DEV double ct_log_dc(const CtHyper &H, int64_t s) {
	RC_NO_CONTRACT
	return -(lgamma((double)(s + 1)) + lgamma((double)(H.m - s + 1)) + lgamma((double)(H.k - s + 1)) + lgamma((double)(H.n2 - H.k + s + 1)));
}

constexpr int kCtLower = 0, kCtUpper = 1, kCtMean = 2, kCtTwoSided = 3;

// At the log odds ratio theta: P(X <= x) (kCtLower), P(X >= x) (kCtUpper), E X - x (kCtMean), or the sum of the P(s) that do not
// exceed P(x) by more than the slack (kCtTwoSided).  One pass: every lane scales its weights by the largest exponent it has met,
// the lanes then by the largest of all.
GI_DEV double ct_hyper_eval(const CtHyper &H, double theta, int what) {
	RC_NO_CONTRACT
	GiPL<double> top, num, den;
	const double at_x = ct_log_dc(H, H.x);
	GI_LANES_BEGIN(lane)
	double mx = -INFINITY, sn = 0.0, sd = 0.0;
	for (int64_t s = H.lo + lane; s <= H.hi; s += 64) {
		const double off = (double)(s - H.x);
		const double d = ct_log_dc(H, s) + theta * off;
		if (d > mx) {
			const double scale = exp(mx - d); // (the first: exp(-inf) = 0 times 0)
			sn *= scale;
			sd *= scale;
			mx = d;
		}
		const double w = exp(d - mx);
		sd += w;
		if (what == kCtMean) sn += off * w;
		else if (what == kCtLower ? s <= H.x : what == kCtUpper ? s >= H.x : d <= at_x + kCtTieSlack) sn += w;
	}
	top.v[GI_AT(lane)] = mx;
	num.v[GI_AT(lane)] = sn;
	den.v[GI_AT(lane)] = sd;
	GI_LANES_END
	GiPL<double> t2;
	GI_LANES_BEGIN(lane)
	(void)lane;
	t2.v[GI_AT(lane)] = top.v[GI_AT(lane)];
	GI_LANES_END
	const double all = glm::gi_max(t2);
	GI_LANES_BEGIN(lane)
	(void)lane;
	const double mx = top.v[GI_AT(lane)];
	const double scale = mx == -INFINITY ? 0.0 : exp(mx - all); // (a lane without a support point)
	num.v[GI_AT(lane)] *= scale;
	den.v[GI_AT(lane)] *= scale;
	GI_LANES_END
	const double n = glm::gi_sum(num), d = glm::gi_sum(den);
	return n / d;
}

// exp(theta) for the theta at which ct_hyper_eval(what) = target; the function ascends in theta but for kCtLower
GI_DEV double ct_hyper_root(const CtHyper &H, int what, double target) {
	RC_NO_CONTRACT
	const double slope = what == kCtLower ? -1.0 : 1.0;
	double t0 = 0.0, g0 = ct_hyper_eval(H, 0.0, what) - target;
	if (g0 == 0.0) return 1.0;
	if (g0 != g0) return NAN;
	double step = slope * g0 < 0.0 ? 1.0 : -1.0, t1 = 0.0, g1 = g0;
	bool found = false;
	GI_NOUNROLL
	for (int it = 0; it < 64 && !found; ++it) {
		t1 = t0 + step;
		g1 = ct_hyper_eval(H, t1, what) - target;
		if (g1 == 0.0) return exp(t1);
		if (g1 != g1) return NAN;
		if ((g1 < 0.0) != (g0 < 0.0)) {
			found = true;
		} else {
			t0 = t1;
			g0 = g1;
			step *= 2.0;
		}
	}
	if (!found) return step > 0.0 ? INFINITY : 0.0;
	double t = t1;
	GI_NOUNROLL
	for (int it = 0; it < kCtRootSteps; ++it) {
		const double lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
		double next = t1 - g1 * (t1 - t0) / (g1 - g0);
		if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
		if (next == t0 || next == t1) break; // the bracket has no double inside
		const double g = ct_hyper_eval(H, next, what) - target;
		const double moved = fabs(next - t);
		t = next;
		if (g == 0.0 || g != g) break;
		if ((g < 0.0) != (g1 < 0.0)) {
			t0 = t1;
			g0 = g1;
		} else {
			g0 *= 0.5; // Illinois: the end that stays loses half its weight
		}
		t1 = next;
		g1 = g;
		if (moved <= 4e-16 * (fabs(t) > 1.0 ? fabs(t) : 1.0)) break;
	}
	return exp(t);
}

// what the wavefront leaves to lane 0
struct CtFisher {
	double p, mle, lower, upper;
};

GI_DEV CtFisher ct_fisher(const CtHyper &H, int alternative, double level) {
	RC_NO_CONTRACT
	CtFisher F;
	F.p = ct_hyper_eval(H, 0.0, alternative == cor::kCorLess ? kCtLower : alternative == cor::kCorGreater ? kCtUpper : kCtTwoSided);
	if (F.p > 1.0) F.p = 1.0;
	F.mle = H.x == H.lo ? 0.0 : H.x == H.hi ? INFINITY : ct_hyper_root(H, kCtMean, 0.0);
	F.lower = F.upper = NAN;
	if (level == level) {
		const double alpha = alternative == cor::kCorTwoSided ? 0.5 * (1.0 - level) : 1.0 - level;
		F.lower = alternative == cor::kCorLess || H.x == H.lo ? 0.0 : ct_hyper_root(H, kCtUpper, alpha);
		F.upper = alternative == cor::kCorGreater || H.x == H.hi ? INFINITY : ct_hyper_root(H, kCtLower, alpha);
	}
	return F;
}

GI_DEV void ct_fisher_record(int64_t n11, int64_t n12, int64_t n21, int64_t n22, const CtFisher &F, double *rec) {
	RC_NO_CONTRACT
	rec[0] = (double)n11 * (double)n22 / ((double)n12 * (double)n21);
	rec[1] = F.p;
	rec[2] = NAN;
	rec[3] = F.mle;
	rec[4] = F.lower;
	rec[5] = F.upper;
	rec[6] = (double)(n11 + n12 + n21 + n22);
	rec[7] = 2.0;
	rec[8] = 2.0;
	rec[9] = NAN;
	rec[10] = NAN;
	rec[11] = 0.0;
}

// ---- the phases of one wavefront ----

// The four cells of rows [lo, hi) in one pass: Fisher counts the rows with both labels in {0, 1}, McNemar every valid row with a
// label of 0 against every other label.  cell[2 i + j]: a in class i, b in class j.
GI_DEV void ct_count_cells(const CategoricalProblem &P, int64_t lo, int64_t hi, int64_t (&cell)[4]) {
	GiPL<int64_t> c0, c1, c2, c3;
	GI_LANES_BEGIN(lane)
	int64_t k[4] = {0, 0, 0, 0};
	for (int64_t i = lo + lane; i < hi; i += 64) {
		const int32_t a = P.a[i], b = P.b[i];
		if (a == kCtNull || b == kCtNull) continue;
		if (P.test == kCtFisher) {
			if ((a == 0 || a == 1) && (b == 0 || b == 1)) ++k[2 * a + b];
		} else {
			++k[2 * (a != 0) + (b != 0)];
		}
	}
	c0.v[GI_AT(lane)] = k[0];
	c1.v[GI_AT(lane)] = k[1];
	c2.v[GI_AT(lane)] = k[2];
	c3.v[GI_AT(lane)] = k[3];
	GI_LANES_END
	cell[0] = glm::gi_sum_i(c0);
	cell[1] = glm::gi_sum_i(c1);
	cell[2] = glm::gi_sum_i(c2);
	cell[3] = glm::gi_sum_i(c3);
}

// the valid rows of [lo, hi) to W.x (a) and W.y (b) in their order -> their number
GI_DEV int64_t ct_compact(const CategoricalProblem &P, int64_t lo, int64_t hi, const CorWork &W) {
	int64_t n = 0;
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	for (int64_t base = lo; base < hi; base += 64) {
		const int64_t i = base + lane;
		int32_t a = kCtNull, b = kCtNull;
		if (i < hi) {
			a = P.a[i];
			b = P.b[i];
		}
		const bool ok = a != kCtNull && b != kCtNull;
		const unsigned long long mask = __ballot(ok);
		if (ok) {
			const int64_t at = n + __popcll(mask & ((1ull << lane) - 1ull));
			W.x[at] = (double)a;
			W.y[at] = (double)b;
		}
		n += __popcll(mask);
	}
#else
	for (int64_t i = lo; i < hi; ++i) {
		if (P.a[i] == kCtNull || P.b[i] == kCtNull) continue;
		W.x[n] = (double)P.a[i];
		W.y[n] = (double)P.b[i];
		++n;
	}
#endif
	return n;
}

// the first index of the ascending v[lo, hi) whose element is not below `value`
GI_DEV int64_t ct_lower_bound(const double *v, int64_t lo, int64_t hi, double value) {
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (v[mid] < value) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// the first index of the ascending v[lo, hi) whose element is above `value`
GI_DEV int64_t ct_upper_bound(const double *v, int64_t lo, int64_t hi, double value) {
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (v[mid] <= value) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// the keys sorted by b: W.y[q] = the first place of q's column in this order
GI_DEV void ct_column_starts(const CorWork &W, int64_t n) {
	GI_LANES_BEGIN(lane)
	for (int64_t q = lane; q < n; q += 64) W.y[q] = (double)ct_lower_bound(W.key, 0, q, W.key[q]);
	GI_LANES_END
}

// the second sort's input: a in the order by b, ties to be broken by the place in that order
GI_DEV void ct_rekey(const CorWork &W, int64_t n) {
	GI_LANES_BEGIN(lane)
	for (int64_t q = lane; q < n; q += 64) {
		W.key[q] = W.x[W.idx[q]];
		W.idx[q] = (int32_t)q;
	}
	GI_LANES_END
}

// W.x[start] = the column's count, for every column start -> the columns
GI_DEV int64_t ct_column_counts(const CorWork &W, int64_t n) {
	GiPL<int64_t> c;
	GI_LANES_BEGIN(lane)
	int64_t k = 0;
	for (int64_t q = lane; q < n; q += 64) {
		if (W.y[q] != (double)q) continue;
		W.x[q] = (double)(ct_upper_bound(W.y, q + 1, n, (double)q) - q);
		++k;
	}
	c.v[GI_AT(lane)] = k;
	GI_LANES_END
	return glm::gi_sum_i(c);
}

// the column start of the row at place p of the order by (a, column)
GI_DEV double ct_column_of(const CorWork &W, int64_t p) { return W.y[W.idx[p]]; }

// the first place of [lo, hi) (one row of the table, its column starts ascending) whose column start is above `col`
GI_DEV int64_t ct_cell_end(const CorWork &W, int64_t lo, int64_t hi, double col) {
	while (lo < hi) {
		const int64_t mid = lo + (hi - lo) / 2;
		if (ct_column_of(W, mid) <= col) lo = mid + 1;
		else hi = mid;
	}
	return lo;
}

// the cells of the n rows sorted by (a, column): every occupied cell once, from the lane that holds its first row
GI_DEV CtTable ct_cells(int test, const CorWork &W, int64_t n, int64_t columns) {
	RC_NO_CONTRACT
	GiPL<double> s;
	GiPL<int64_t> rc, rows, first, first_row;
	GI_LANES_BEGIN(lane)
	double a = 0.0;
	int64_t arc = 0, ar = 0, a11 = 0, ar1 = 0;
	for (int64_t p = lane; p < n; p += 64) {
		const double label = W.key[p], col = ct_column_of(W, p);
		if (p > 0 && W.key[p - 1] == label && ct_column_of(W, p - 1) == col) continue; // not the first row of its cell
		const int64_t row_lo = ct_lower_bound(W.key, 0, p, label), row_hi = ct_upper_bound(W.key, p + 1, n, label);
		const int64_t o = ct_cell_end(W, p + 1, row_hi, col) - p, r = row_hi - row_lo, c = (int64_t)W.x[(int64_t)col];
		a += ct_cell_term(test, o, r, c, n);
		arc += r * c;
		if (row_lo == p) ++ar;
		if (p == 0) {
			ar1 = r;
			a11 = col == 0.0 ? o : 0;
		}
	}
	s.v[GI_AT(lane)] = a;
	rc.v[GI_AT(lane)] = arc;
	rows.v[GI_AT(lane)] = ar;
	first.v[GI_AT(lane)] = a11;
	first_row.v[GI_AT(lane)] = ar1;
	GI_LANES_END
	CtTable T;
	T.n = n;
	T.c = columns;
	T.sum = glm::gi_sum(s);
	T.sum_rc = glm::gi_sum_i(rc);
	T.r = glm::gi_sum_i(rows);
	T.n11 = glm::gi_sum_i(first);
	T.r1 = glm::gi_sum_i(first_row);
	T.c1 = (int64_t)W.x[0];
	return T;
}

// ---- one group ----
// Rows [lo, hi) of group g, W as long as the group (Fisher and McNemar do not touch it).  `lead`: this thread belongs to the
// wavefront that runs every phase but the sorts (the only wavefront of the small path); tid / threads: the sorts'.
GI_DEV void ct_group(const CategoricalProblem &P, int64_t g, int64_t lo, int64_t hi, const CorWork &W, bool lead, int64_t tid, int64_t threads) {
	double *rec = P.records + g * kCtRecordLen;
	if (!ct_staged(P.test)) {
		if (!lead) return;
		int64_t cell[4];
		ct_count_cells(P, lo, hi, cell);
		if (P.test == kCtMcNemar) {
			GI_LANES_BEGIN(lane)
			if (lane == 0) ct_mcnemar_record(P.correction, P.exact, cell[0], cell[1], cell[2], cell[3], rec);
			GI_LANES_END
			return;
		}
		const bool counted = cell[0] + cell[1] + cell[2] + cell[3] > 0;
		CtFisher F = {NAN, NAN, NAN, NAN};
		if (counted) F = ct_fisher(ct_hyper(cell[0], cell[1], cell[2], cell[3]), P.alternative, P.confidence_level);
		GI_LANES_BEGIN(lane)
		if (lane == 0) {
			if (counted) ct_fisher_record(cell[0], cell[1], cell[2], cell[3], F, rec);
			else ct_write_failed(rec, 0.0, 2.0, 2.0);
		}
		GI_LANES_END
		return;
	}
	int64_t n = 0;
	if (lead) n = ct_compact(P, lo, hi, W);
#if defined(__HIPCC__)
	if (threads > 64) { // the other wavefronts of the workgroup learn n through the first index slot
		if (lead && (threadIdx.x & 63u) == 0 && hi > lo) W.idx[0] = (int32_t)n;
		glm::gi_sync();
		if (hi > lo) n = W.idx[0];
		glm::gi_sync();
	}
#endif
	CtTable T = {0, 0, 0, 0.0, 0, 0, 0, 0};
	if (n > 0) { // (n is the same in every thread: the barriers below are met by all)
		if (lead) cor::rc_fill_keys(W.y, n, W);
		cor::rc_sort(W, n, tid, threads);
		if (lead) ct_column_starts(W, n);
		glm::gi_sync();
		if (lead) ct_rekey(W, n);
		glm::gi_sync();
		int64_t columns = 0;
		if (lead) columns = ct_column_counts(W, n);
		cor::rc_sort(W, n, tid, threads);
		if (!lead) return;
		T = ct_cells(P.test, W, n, columns);
	}
	if (!lead) return;
	GI_LANES_BEGIN(lane)
	if (lane == 0) ct_table_record(P.test, P.correction, T, rec);
	GI_LANES_END
}

} // namespace cattest
} // namespace anofox
