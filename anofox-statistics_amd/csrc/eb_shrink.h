// eb_shrink.h — empirical-Bayes shrinkage of (estimate, standard error) pairs toward their precision-weighted mean: the
// DerSimonian-Laird random-effects model of the reference's eb_shrink (crates/anofox-stats-core/src/models/eb_shrink.rs)
// restated for one wavefront.  DESIGN.md §1, "Empirical-Bayes shrinkage".
//
//     usable pair: est finite, se finite and > 0;  k = the usable pairs of a set;  sums over usable pairs only
//     w = 1/se^2   Sw = sum w   fixed = sum w est / Sw   Q = sum w (est - fixed)^2  (a second pass, about `fixed`)
//     df = k - 1   C = Sw - sum w^2 / Sw
//     tau^2 = the options' value if it is not NaN | 0 (method none) | max(0, (Q - df) / C) if C > 0 else 0 (DerSimonian-Laird)
//     wr = 1/(se^2 + tau^2)   mu = sum wr est / sum wr   mu_se = sqrt(1 / sum wr)
//     I^2 = clamp((Q - df) / Q, 0, 1) if Q > df and Q > 0 else 0
//     usable pair:  tau^2 > 0: weight = (1/se^2) / (1/se^2 + 1/tau^2), shrunken = weight est + (1 - weight) mu,
//                              shrunken_se = sqrt(1 / (1/se^2 + 1/tau^2));   tau^2 = 0: shrunken = mu, shrunken_se = mu_se, weight = 0
//     other pairs:  NaN, NaN, NaN (the pair keeps its place)
//     status: invalid options 1 (every set) | no items 10 | k < 2: 6;  a status != 0 makes the summary and the set's outputs NaN
//
// Input: est[g est_stride + c], se[g se_stride + c], g an item, c a column in [0, n_cols); a set is (a contiguous item range,
// a column).  One source for both builds, by the lanes of glm_irls.h: under hipcc the functions are device code run by ONE
// WAVEFRONT, under a plain C++ compiler a wavefront is a loop over 64 lanes and the butterfly runs over an array of 64
// partials, so both builds add every sum in the same order.  Contraction of a * b + c is switched off in every body.
//
//   lanes     cp = n_cols rounded up to a power of two (64 at most; wider calls go by column blocks of 64).  Lane l works
//             on column c0 + (l & (cp - 1)) and starts at item l / cp, 64 / cp items per step: neighbouring lanes read
//             neighbouring doubles of one item's record, whatever the stride between items.  A lane keeps the sums of its own
//             column only; the butterfly over the lane bits >= cp (gi_sum's m_lo) adds the 64 / cp lanes of a column.
//   one wave  eb_shrink_set: three reduction passes over the items (Sw, Sw est, Sw^2, k | Q | Swr, Swr est) and one write pass.
//   chunks    eb_chunk_partial / eb_chunk_combine / eb_chunk_write: the same passes over chunks of `chunk` items.  A pass is a
//             grid of chunk partials written to a scratch, then one wavefront per (set, column block) adds a set's partials with
//             the lanes striding over the chunks and the same butterfly.  The order depends on `chunk` only.  Chunks are
//             numbered without a prefix sum over the sets: set s owns the numbers from V(s) = (off[s] - off[0]) / chunk + s on;
//             V(s + 1) - V(s) >= ceil(m_s / chunk), numbers past a set's last chunk are idle.
#pragma once
#include "glm_irls.h"

#if defined(__clang__)
#define EB_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EB_NO_CONTRACT
#endif
#if defined(__HIPCC__)
#define EB_UNROLL4 _Pragma("unroll 4")
#else
#define EB_UNROLL4
#endif

namespace anofox {
namespace eb {

using glm::GiPL;

constexpr int kEbSummaryLen = 8; // {mu, mu_se, tau_squared, i_squared, q, n_groups, n_input, status}
constexpr int kEbOutLen = 3;     // {shrunken, shrunken_se, weight}
constexpr int kEbPartLen = 4;    // the sums of one pass, per chunk and column
constexpr int kEbMethodDL = 0;
constexpr int kEbMethodNone = 1;
constexpr int kEbStatusInvalidInput = 1;
constexpr int kEbStatusInsufficientData = 6;
constexpr int kEbStatusNoValidData = 10;

// what the chunk path carries per (set, column) between its passes
enum { kEbSw = 0, kEbSwy, kEbSw2, kEbK, kEbFixed, kEbQ, kEbTau2, kEbMu, kEbMuSe, kEbFailed, kEbStateLen };

struct EbProblem {
	const double *est, *se;
	int64_t est_stride, se_stride;
	int64_t n_items; // item ranges are clipped to [0, n_items)
	int n_cols;
	int method;
	double tau_fixed; // NaN: estimate it
	int invalid;      // invalid options: every set gets status 1
	double *out;      // [n_items x n_cols x 3]
	double *summary;  // [n_sets x n_cols x 8]
};

GI_HD int eb_col_pad(int n_cols) {
	int cp = 1;
	while (cp < n_cols && cp < 64) cp <<= 1;
	return cp;
}
GI_HD int eb_col_blocks(int n_cols) { return (n_cols + 63) / 64; }
GI_HD bool eb_options_invalid(int method, double tau_fixed) {
	if (method != kEbMethodDL && method != kEbMethodNone) return true;
	return tau_fixed == tau_fixed && !(tau_fixed >= 0.0 && tau_fixed <= DBL_MAX);
}
// the first chunk number of set s (s == n_sets: the count of numbers)
GI_HD int64_t eb_chunk_base(const int64_t *off, int64_t s, int64_t chunk) { return (off[s] - off[0]) / chunk + s; }

GI_DEV bool eb_usable(double est, double se) { return glm::gi_finite(est) && glm::gi_finite(se) && se > 0.0; }

// the butterfly over the lane bits >= cp; afterwards every lane holds its own column's total
GI_DEV void eb_reduce(GiPL<double> &s, int cp) {
#if defined(__HIPCC__)
	s.v[0] = glm::gi_sum(s, cp);
#else
	glm::gi_sum(s, cp);
#endif
}

struct EbSums {
	GiPL<double> a[kEbPartLen];
};

// One pass over items [lo, hi) of column block c0: PASS 1 -> {Sw, Sw est, Sw^2, k}, PASS 2 -> {Q} about prm = fixed,
// PASS 3 -> {Swr, Swr est} with prm = tau^2; per lane, not yet reduced.
template <int PASS>
GI_DEV void eb_accumulate(const EbProblem &P, int64_t lo, int64_t hi, int c0, int cp, const GiPL<double> &prm, EbSums &S) {
	EB_NO_CONTRACT
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane), col = c0 + (lane & (cp - 1)), per = 64 / cp;
	double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
	if (col < P.n_cols) {
		const double v = prm.v[L];
		const double *e = P.est + col, *s = P.se + col;
		EB_UNROLL4
		for (int64_t i = lo + lane / cp; i < hi; i += per) {
			const double ei = e[i * P.est_stride], si = s[i * P.se_stride];
			if (!eb_usable(ei, si)) continue;
			if (PASS == 1) {
				const double w = 1.0 / (si * si);
				a0 += w;
				a1 += w * ei;
				a2 += w * w;
				a3 += 1.0;
			} else if (PASS == 2) {
				const double w = 1.0 / (si * si), d = ei - v;
				a0 += w * (d * d);
			} else {
				const double wr = 1.0 / (si * si + v);
				a0 += wr;
				a1 += wr * ei;
			}
		}
	}
	S.a[0].v[L] = a0;
	S.a[1].v[L] = a1;
	S.a[2].v[L] = a2;
	S.a[3].v[L] = a3;
	GI_LANES_END
}

GI_DEV double eb_fixed_mean(double sw, double swy) { return swy / sw; }

GI_DEV double eb_tau_squared(const EbProblem &P, double sw, double sw2, double k, double q) {
	EB_NO_CONTRACT
	if (P.tau_fixed == P.tau_fixed) return P.tau_fixed;
	if (P.method == kEbMethodNone) return 0.0;
	const double c = sw - sw2 / sw, t = (q - (k - 1.0)) / c;
	return c > 0.0 && t > 0.0 ? t : 0.0; // (a NaN t: 0, as f64::max)
}

GI_DEV int eb_status(const EbProblem &P, int64_t m, double k) {
	if (P.invalid) return kEbStatusInvalidInput;
	if (m <= 0) return kEbStatusNoValidData;
	return k < 2.0 ? kEbStatusInsufficientData : 0;
}

// the 8 doubles of one set's summary; mu and mu_se come back for the write pass (NaN for a failed set)
GI_DEV void eb_write_summary(double *sum, int status, int64_t m, double k, double q, double tau2, double swr, double swry, double &mu,
                             double &mu_se) {
	EB_NO_CONTRACT
	if (status != 0) {
		for (int j = 0; j < kEbSummaryLen - 1; ++j) sum[j] = NAN;
		sum[7] = (double)status;
		mu = mu_se = NAN;
		return;
	}
	const double df = k - 1.0;
	mu = swry / swr;
	mu_se = sqrt(1.0 / swr);
	double i2 = 0.0;
	if (q > df && q > 0.0) {
		i2 = (q - df) / q;
		i2 = i2 < 0.0 ? 0.0 : (i2 > 1.0 ? 1.0 : i2);
	}
	sum[0] = mu;
	sum[1] = mu_se;
	sum[2] = tau2;
	sum[3] = i2;
	sum[4] = q;
	sum[5] = k;
	sum[6] = (double)m;
	sum[7] = 0.0;
}

// The write pass over items [lo, hi) of column block c0; a lane's mu, mu_se and tau^2 are its column's, NaN mu: a failed set.
GI_DEV void eb_write_items(const EbProblem &P, int64_t lo, int64_t hi, int c0, int cp, const GiPL<double> &mu, const GiPL<double> &mu_se,
                           const GiPL<double> &tau2, const GiPL<int> &failed) {
	EB_NO_CONTRACT
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane), col = c0 + (lane & (cp - 1)), per = 64 / cp;
	if (col < P.n_cols) {
		const double m = mu.v[L], ms = mu_se.v[L], t2 = tau2.v[L];
		const bool bad = failed.v[L] != 0;
		const double *e = P.est + col, *s = P.se + col;
		for (int64_t i = lo + lane / cp; i < hi; i += per) {
			const double ei = e[i * P.est_stride], si = s[i * P.se_stride];
			double sh = NAN, sh_se = NAN, wt = NAN;
			if (!bad && eb_usable(ei, si)) {
				if (t2 > 0.0) {
					const double pw = 1.0 / (si * si), pb = 1.0 / t2, pp = pw + pb;
					wt = pw / pp;
					sh = wt * ei + (1.0 - wt) * m;
					sh_se = sqrt(1.0 / pp);
				} else {
					sh = m;
					sh_se = ms;
					wt = 0.0;
				}
			}
			double *o = P.out + (i * (int64_t)P.n_cols + col) * kEbOutLen;
			o[0] = sh;
			o[1] = sh_se;
			o[2] = wt;
		}
	}
	GI_LANES_END
}

// ---- one wavefront per (set, column block): the whole set in four passes ----
GI_DEV void eb_shrink_set(const EbProblem &P, int64_t set, int64_t lo, int64_t hi, int c0) {
	lo = lo < 0 ? 0 : lo;
	hi = hi > P.n_items ? P.n_items : hi;
	if (hi < lo) hi = lo;
	const int cp = eb_col_pad(P.n_cols - c0);
	const int64_t m = hi - lo;
	EbSums S1, S2;
	GiPL<double> prm, mu, mu_se;
	GiPL<int> failed;
	GI_LANES_BEGIN(lane)
	(void)lane;
	prm.v[GI_AT(lane)] = 0.0;
	GI_LANES_END
	eb_accumulate<1>(P, lo, hi, c0, cp, prm, S1);
	for (int j = 0; j < kEbPartLen; ++j) eb_reduce(S1.a[j], cp);
	GI_LANES_BEGIN(lane)
	(void)lane;
	const int L = GI_AT(lane);
	prm.v[L] = eb_fixed_mean(S1.a[kEbSw].v[L], S1.a[kEbSwy].v[L]);
	GI_LANES_END
	eb_accumulate<2>(P, lo, hi, c0, cp, prm, S2);
	eb_reduce(S2.a[0], cp);
	GiPL<double> q;
	GI_LANES_BEGIN(lane)
	(void)lane;
	const int L = GI_AT(lane);
	q.v[L] = S2.a[0].v[L];
	prm.v[L] = eb_tau_squared(P, S1.a[kEbSw].v[L], S1.a[kEbSw2].v[L], S1.a[kEbK].v[L], q.v[L]);
	GI_LANES_END
	eb_accumulate<3>(P, lo, hi, c0, cp, prm, S2);
	eb_reduce(S2.a[0], cp);
	eb_reduce(S2.a[1], cp);
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane), col = c0 + (lane & (cp - 1));
	const int status = eb_status(P, m, S1.a[kEbK].v[L]);
	failed.v[L] = status != 0;
	double sum[kEbSummaryLen];
	eb_write_summary(sum, status, m, S1.a[kEbK].v[L], q.v[L], prm.v[L], S2.a[0].v[L], S2.a[1].v[L], mu.v[L], mu_se.v[L]);
	if (lane < cp && col < P.n_cols) { // the first lane of a column writes its summary
		double *o = P.summary + (set * (int64_t)P.n_cols + col) * kEbSummaryLen;
		for (int j = 0; j < kEbSummaryLen; ++j) o[j] = sum[j];
	}
	GI_LANES_END
	eb_write_items(P, lo, hi, c0, cp, mu, mu_se, prm, failed);
}

// ---- the chunk path ----
// parts: [n_numbers x n_cols x 4] chunk partials of the running pass, n_numbers = n_items / chunk + n_sets >= V(n_sets);  state: [n_sets x n_cols x kEbStateLen]

// the set of chunk number v: the largest s with V(s) <= v
GI_DEV int64_t eb_chunk_set(const int64_t *off, int64_t n_sets, int64_t chunk, int64_t v) {
	int64_t a = 0, b = n_sets - 1;
	while (a < b) {
		const int64_t mid = a + (b - a + 1) / 2;
		if (eb_chunk_base(off, mid, chunk) <= v) a = mid;
		else b = mid - 1;
	}
	return a;
}

// The items of chunk number v -> [lo, hi) (empty for an idle number) and its set; false: nothing to do, not even a summary.
GI_DEV bool eb_chunk_range(const EbProblem &P, const int64_t *off, int64_t n_sets, int64_t chunk, int64_t v, int64_t &set, int64_t &lo,
                           int64_t &hi) {
	set = eb_chunk_set(off, n_sets, chunk, v);
	const int64_t j = v - eb_chunk_base(off, set, chunk);
	int64_t s_lo = off[set] < 0 ? 0 : off[set], s_hi = off[set + 1] > P.n_items ? P.n_items : off[set + 1];
	if (s_hi < s_lo) s_hi = s_lo;
	lo = s_lo + j * chunk;
	if (lo > s_hi) lo = s_hi;
	hi = lo + chunk < s_hi ? lo + chunk : s_hi;
	return j == 0 || lo < hi;
}

// One wavefront, chunk number v, column block c0: the partial sums of pass PASS into parts.
template <int PASS>
GI_DEV void eb_chunk_partial(const EbProblem &P, const int64_t *off, int64_t n_sets, int64_t chunk, int64_t v, int c0, const double *state,
                             double *parts) {
	int64_t set, lo, hi;
	if (!eb_chunk_range(P, off, n_sets, chunk, v, set, lo, hi)) return;
	const int cp = eb_col_pad(P.n_cols - c0);
	GiPL<double> prm;
	EbSums S;
	GI_LANES_BEGIN(lane)
	const int col = c0 + (lane & (cp - 1));
	double x = 0.0;
	if (PASS > 1 && col < P.n_cols) x = state[(set * (int64_t)P.n_cols + col) * kEbStateLen + (PASS == 2 ? kEbFixed : kEbTau2)];
	prm.v[GI_AT(lane)] = x;
	GI_LANES_END
	eb_accumulate<PASS>(P, lo, hi, c0, cp, prm, S);
	constexpr int n = PASS == 1 ? 4 : (PASS == 2 ? 1 : 2);
	for (int j = 0; j < n; ++j) eb_reduce(S.a[j], cp);
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane), col = c0 + (lane & (cp - 1));
	if (lane < cp && col < P.n_cols)
		for (int j = 0; j < n; ++j) parts[(v * (int64_t)P.n_cols + col) * kEbPartLen + j] = S.a[j].v[L];
	GI_LANES_END
}

// One wavefront, one set, column block c0: adds the set's chunk partials of pass PASS (lanes stride over the chunks of a
// column, then the butterfly) and writes what the next pass needs into the state; after pass 3 also the summary.
template <int PASS>
GI_DEV void eb_chunk_combine(const EbProblem &P, const int64_t *off, int64_t n_numbers, int64_t chunk, int64_t set, int c0, double *state,
                             const double *parts) {
	EB_NO_CONTRACT
	const int cp = eb_col_pad(P.n_cols - c0);
	int64_t s_lo = off[set] < 0 ? 0 : off[set], s_hi = off[set + 1] > P.n_items ? P.n_items : off[set + 1];
	if (s_hi < s_lo) s_hi = s_lo;
	const int64_t m = s_hi - s_lo, v0 = eb_chunk_base(off, set, chunk), n_chunks = m > 0 ? (m + chunk - 1) / chunk : 1;
	constexpr int n = PASS == 1 ? 4 : (PASS == 2 ? 1 : 2);
	EbSums S;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane), col = c0 + (lane & (cp - 1)), per = 64 / cp;
	double a[kEbPartLen] = {0.0, 0.0, 0.0, 0.0};
	if (col < P.n_cols)
		for (int64_t j = lane / cp; j < n_chunks && v0 + j >= 0 && v0 + j < n_numbers; j += per) // (the bound: offsets never lead outside parts)
			for (int t = 0; t < n; ++t) a[t] += parts[((v0 + j) * (int64_t)P.n_cols + col) * kEbPartLen + t];
	for (int t = 0; t < kEbPartLen; ++t) S.a[t].v[L] = a[t];
	GI_LANES_END
	for (int j = 0; j < n; ++j) eb_reduce(S.a[j], cp);
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane), col = c0 + (lane & (cp - 1));
	if (lane < cp && col < P.n_cols) {
		double *st = state + (set * (int64_t)P.n_cols + col) * kEbStateLen;
		if (PASS == 1) {
			st[kEbSw] = S.a[0].v[L];
			st[kEbSwy] = S.a[1].v[L];
			st[kEbSw2] = S.a[2].v[L];
			st[kEbK] = S.a[3].v[L];
			st[kEbFixed] = eb_fixed_mean(S.a[0].v[L], S.a[1].v[L]);
		} else if (PASS == 2) {
			st[kEbQ] = S.a[0].v[L];
			st[kEbTau2] = eb_tau_squared(P, st[kEbSw], st[kEbSw2], st[kEbK], S.a[0].v[L]);
		} else {
			double mu, mu_se;
			const int status = eb_status(P, m, st[kEbK]);
			eb_write_summary(P.summary + (set * (int64_t)P.n_cols + col) * kEbSummaryLen, status, m, st[kEbK], st[kEbQ], st[kEbTau2],
			                 S.a[0].v[L], S.a[1].v[L], mu, mu_se);
			st[kEbMu] = mu;
			st[kEbMuSe] = mu_se;
			st[kEbFailed] = status != 0 ? 1.0 : 0.0;
		}
	}
	GI_LANES_END
}

// One wavefront, chunk number v, column block c0: the write pass of the chunk's items.
GI_DEV void eb_chunk_write(const EbProblem &P, const int64_t *off, int64_t n_sets, int64_t chunk, int64_t v, int c0, const double *state) {
	int64_t set, lo, hi;
	if (!eb_chunk_range(P, off, n_sets, chunk, v, set, lo, hi)) return;
	const int cp = eb_col_pad(P.n_cols - c0);
	GiPL<double> mu, mu_se, tau2;
	GiPL<int> failed;
	GI_LANES_BEGIN(lane)
	const int L = GI_AT(lane), col = c0 + (lane & (cp - 1));
	const double *st = state + (set * (int64_t)P.n_cols + (col < P.n_cols ? col : c0)) * kEbStateLen;
	mu.v[L] = st[kEbMu];
	mu_se.v[L] = st[kEbMuSe];
	tau2.v[L] = st[kEbTau2];
	failed.v[L] = st[kEbFailed] != 0.0;
	GI_LANES_END
	eb_write_items(P, lo, hi, c0, cp, mu, mu_se, tau2, failed);
}

} // namespace eb
} // namespace anofox
