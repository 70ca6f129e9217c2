// perm_tests.h — the resampling two-sample tests of one group of rows: the energy distance test, the permutation (Welch) t-test
// and the Gaussian-kernel MMD test, each with a permutation p-value.  The reference's energy_distance_test, mmd_test and
// permutation_t_test (crates/anofox-stats-core/src/tests/modern.rs, resampling.rs) are wrappers around a crate that is not
// restated here, and its permutation stream is not specified; the contract below is this project's own.
// DESIGN.md §1, "Permutation tests".
//
//     input: a value column v and an int32 sample column;  sample 1 = the rows with sample == 0, sample 2 = every other id
//     valid row: v not NaN.  A group that holds an infinity: status 6 (the statistics are undefined there)
//     record {statistic, p_value, aux, n_extreme, n, n1, n2, status};  status != 0: every field but the counts is NaN
//     status: n1 < 2 or n2 < 2 or an infinity -> 6 (InsufficientData);  MMD on a group above the small path's cap (kPtMmdCap =
//             1462 rows, the rows one wavefront holds in LDS) -> 7 ("mmd: group too large"): MMD costs O(N^2) per permutation
//             and is built on the small path only
//     after the sort: z_k the k-th smallest valid value (ties in their original order: rc_sort orders (key, idx)), l_k its
//             observed label, c_k = z_k - z_[N/2] (an element pick, no sum), d_k = z_(k+1) - z_k
//     stream  permutation b (0 <= b < B): state = seed ^ ((b + 1) * 0xD1B54A32D192ED03);  row step k = 0 .. N - 1:
//             state += 0x9E3779B97F4A7C15, z = splitmix64's finaliser of state, r = z >> 32;  row k joins sample 1 iff
//             (r * (N - k)) >> 32 < n1 - taken (Knuth's selection sampling: a uniformly random n1-subset, the bias of a draw at
//             most N / 2^32).  The stream depends on (seed, b, k) alone, not on the group's index.
//     lanes   one lane = one permutation: round r covers the permutations 64 r .. 64 r + 63, a lane with b >= B does nothing and is
//             not counted.  A lane accumulates sequentially in k, with no cross-lane sum.  The observed statistic comes from the
//             same lane routine fed the labels l_k, so `permuted >= observed` compares numbers of identical arithmetic.
//             n_extreme (int64) = the permutations with T*_b >= T;  p = (1 + n_extreme) / (B + 1);  B = 0: p NaN.
//     Energy distance (test 0)   a_k, b_k = the rows of sample 1 / 2 among the first k + 1;  per lane
//               sxx += d_k a_k (n1 - a_k), syy += d_k b_k (n2 - b_k), sxy += d_k (a_k (n2 - b_k) + b_k (n1 - a_k)) (the integer
//               products exact);  E = n1 n2 / N (2 sxy / (n1 n2) - (2 sxx / n1^2 + 2 syy / n2^2)): R's eqdist.etest, the
//               V-statistic; scipy's energy_distance^2 n1 n2 / N.  Swapping the samples gives the same bits.  O(N) per permutation.
//     Permutation t-test (test 1)   per lane the sums of c_k and c_k^2 over its sample 1 and over its sample 2, Welch's t from the
//               four;  two-sided counts |t*| >= |t|, greater t* >= t, less t* <= t;  a permutation whose variance term is 0 gives NaN
//               and is not counted.  Observed variance 0: status 0, statistic and p NaN.  aux = Welch's df of the observed split.
//     MMD (test 2)   k(a, b) = exp(-(a - b)^2 / (2 sigma^2));  sigma from the options, or when that is NaN or <= 0 the median
//               heuristic: the ceil(M / 2)-th smallest of the M = N (N - 1) / 2 pairwise distances, found exactly by bisection over
//               the bit pattern of a double, the pairs within t counted by a binary search per row.  sigma = 0: status 0, statistic
//               and p NaN.  The labels of a round's 64 permutations are bit l of a 64-bit word per row (over W.x).  For each i the
//               lanes write the kernel values K(i, j0 + lane) of a block of 64 columns to a row buffer (over W.y) and every lane
//               walks the buffer: the pair order is i ascending; blocks j0 = 64 [i / 64], + 64, ... ascending; within a block j from
//               j0 + 63 down to j0, keeping i < j < N.  A lane adds K to its sxx, syy or sxy by its two bits; the diagonal is added
//               in closed form: MMD^2 = ((n1 + 2 sxx) / n1^2 + (n2 + 2 syy) / n2^2) - 2 sxy / (n1 n2), the biased estimate.
//               aux = sigma.  O(N^2) per permutation.
//     Not built: distance correlation, TOST, multivariate samples, MMD above kPtMmdCap rows.
//
// One source for both builds, as rank_tests.h: under hipcc device code, under a plain C++ compiler a wavefront is a loop over 64
// lanes (tests/tools/perm_test_host.cpp).  Contraction of a * b + c is switched off in every body.
//
//   compact   valid rows keep their order.  W.x: the value, W.y: 1.0 for sample 1, 0.0 for sample 2.
//   sort      rc_fill_keys(W.x), rc_sort: W.key = z.  Then W.x[k] = l_k and W.y[k] = d_k (energy) or c_k (t-test).
//   rounds    pt_rounds (energy, t-test): wavefront `wave` of `waves` runs the rounds wave, wave + waves, ...; its count is a sum
//             of integers, so the split does not change n_extreme.  pt_mmd_rounds: the one wavefront of the small path.
//   record    lane 0.
#pragma once
#include <string.h>

#include "rank_cor.h"

namespace anofox {
namespace permtest {

using cor::CorWork;
using glm::GiPL;

constexpr int kPtRecordLen = 8; // {statistic, p_value, aux, n_extreme, n, n1, n2, status}
constexpr int kPtEnergy = 0, kPtTTest = 1, kPtMmd = 2;
constexpr int kPtStatusInsufficientData = 6, kPtStatusTooLarge = 7;
constexpr int64_t kPtMaxPermutations = 1000000;
constexpr int kPtMmdCap = 1462; // the small path's cap (rank_launch.h)

typedef uint64_t __attribute__((may_alias)) pt_word; // a row's label word, stored where a double was

struct PermTestProblem {
	const double *v;
	const int32_t *sample;
	int64_t n_rows; // row ranges are clipped to [0, n_rows)
	int test, alternative;
	int64_t n_perm;
	uint64_t seed;
	double sigma; // MMD; NaN or <= 0: the median heuristic
	double *records;
};

// what the phases after the sort need of a group
struct PtInfo {
	int64_t n, n1;
	int status;
};

// nullptr, or what is wrong with the options
GI_HD const char *pt_options_text(int test, int alternative, int64_t n_permutations, double sigma) {
	if (test < kPtEnergy || test > kPtMmd) return "permutation test: unknown test";
	if (alternative < cor::kCorTwoSided || alternative > cor::kCorGreater) return "permutation test: unknown alternative";
	if (n_permutations < 0 || n_permutations > kPtMaxPermutations) return "permutation test: n_permutations must be within [0, 1000000]";
	if (sigma == sigma && !(fabs(sigma) <= DBL_MAX)) return "permutation test: sigma must be finite";
	return nullptr;
}

// ---- the permutation stream ----

GI_HD uint64_t pt_stream_start(uint64_t seed, int64_t b) { return seed ^ ((uint64_t)(b + 1) * 0xD1B54A32D192ED03ull); }

// row step: does the row join sample 1, of which `need` rows are still to take among the `left` rows from this one on
GI_HD bool pt_draw(uint64_t &state, int64_t left, int64_t need) {
	state += 0x9E3779B97F4A7C15ull;
	uint64_t z = state;
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	z ^= z >> 31;
	return (((z >> 32) * (uint64_t)left) >> 32) < (uint64_t)need;
}

// ---- the lane routines: one labelling of the sorted rows, sequentially in k ----

// E of the labelling.  W.y: the gaps d_k.  observed: the labels are W.x, else drawn from `state`.
GI_DEV double pt_energy_walk(const CorWork &W, int64_t n, int64_t n1, bool observed, uint64_t state) {
	RC_NO_CONTRACT
	const double dn1 = (double)n1, dn2 = (double)(n - n1), dn = (double)n;
	double a = 0.0, b = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
	int64_t taken = 0;
	for (int64_t k = 0; k + 1 < n; ++k) {
		const bool join = observed ? W.x[k] != 0.0 : pt_draw(state, n - k, n1 - taken);
		taken += join;
		a += join ? 1.0 : 0.0;
		b += join ? 0.0 : 1.0;
		const double d = W.y[k], ra = dn1 - a, rb = dn2 - b;
		sxx += d * (a * ra);
		syy += d * (b * rb);
		sxy += d * (a * rb + b * ra);
	}
	return (dn1 * dn2 / dn) * (2.0 * sxy / (dn1 * dn2) - (2.0 * sxx / (dn1 * dn1) + 2.0 * syy / (dn2 * dn2)));
}

// Welch's t of the labelling (NaN: no variance), its df in `df`.  W.y: the centred values c_k.
GI_DEV double pt_t_walk(const CorWork &W, int64_t n, int64_t n1, bool observed, uint64_t state, double &df) {
	RC_NO_CONTRACT
	const double dn1 = (double)n1, dn2 = (double)(n - n1);
	double s1 = 0.0, q1 = 0.0, s2 = 0.0, q2 = 0.0;
	int64_t taken = 0;
	for (int64_t k = 0; k < n; ++k) {
		const bool join = observed ? W.x[k] != 0.0 : pt_draw(state, n - k, n1 - taken);
		taken += join;
		const double c = W.y[k], cc = c * c;
		s1 += join ? c : 0.0;
		q1 += join ? cc : 0.0;
		s2 += join ? 0.0 : c;
		q2 += join ? 0.0 : cc;
	}
	const double m1 = s1 / dn1, m2 = s2 / dn2;
	const double e1 = (q1 - s1 * m1) / (dn1 - 1.0) / dn1, e2 = (q2 - s2 * m2) / (dn2 - 1.0) / dn2;
	const double se2 = e1 + e2;
	df = NAN;
	if (!(se2 > 0.0)) return NAN;
	df = se2 * se2 / (e1 * e1 / (dn1 - 1.0) + e2 * e2 / (dn2 - 1.0));
	return (m1 - m2) / sqrt(se2);
}

// does the permuted statistic count against the observed one
GI_DEV bool pt_hit(const PermTestProblem &P, double t, double obs) {
	if (P.test != kPtTTest || P.alternative == cor::kCorGreater) return t >= obs;
	if (P.alternative == cor::kCorLess) return t <= obs;
	return fabs(t) >= fabs(obs);
}

// ---- the phases of one wavefront ----

// the valid rows of [lo, hi) to W.x (value) and W.y (label) in their order; status 6 for a group the tests are not defined on
GI_DEV PtInfo pt_compact(const PermTestProblem &P, int64_t lo, int64_t hi, const CorWork &W) {
	PtInfo I = {0, 0, 0};
	bool inf = false;
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	for (int64_t base = lo; base < hi; base += 64) {
		const int64_t i = base + lane;
		double v = NAN;
		int32_t s = 1;
		if (i < hi) {
			v = P.v[i];
			s = P.sample[i];
		}
		const bool valid = v == v;
		const unsigned long long mask = __ballot(valid);
		if (valid) {
			const int64_t at = I.n + __popcll(mask & ((1ull << lane) - 1ull));
			W.x[at] = v;
			W.y[at] = s == 0 ? 1.0 : 0.0;
		}
		I.n += __popcll(mask);
		I.n1 += __popcll(__ballot(valid && s == 0));
		inf = inf || __ballot(valid && !glm::gi_finite(v)) != 0ull;
	}
#else
	for (int64_t i = lo; i < hi; ++i) {
		const double v = P.v[i];
		if (v != v) continue;
		W.x[I.n] = v;
		W.y[I.n] = P.sample[i] == 0 ? 1.0 : 0.0;
		++I.n;
		I.n1 += P.sample[i] == 0;
		inf = inf || !glm::gi_finite(v);
	}
#endif
	if (inf || I.n1 < 2 || I.n - I.n1 < 2) I.status = kPtStatusInsufficientData;
	return I;
}

// Compaction, the sort and the sorted columns.  Every thread of the workgroup calls it (the barriers are met by all); the
// result is the lead wavefront's.  mmd_fits: the group may run MMD (the small path).  A group whose status is not 0 is not sorted.
GI_DEV PtInfo pt_prepare(const PermTestProblem &P, int64_t lo, int64_t hi, const CorWork &W, bool lead, int64_t tid, int64_t threads,
                         bool mmd_fits) {
	PtInfo I = {0, 0, 0};
	if (lead) {
		I = pt_compact(P, lo, hi, W);
		if (I.status == 0 && P.test == kPtMmd && !mmd_fits) I.status = kPtStatusTooLarge;
	}
	int64_t n = I.status == 0 ? I.n : 0; // what is sorted
#if defined(__HIPCC__)
	if (threads > 64) { // the other wavefronts of the workgroup learn n through the first key slot's index
		if (lead && (threadIdx.x & 63u) == 0 && hi > lo) W.idx[0] = (int32_t)n;
		glm::gi_sync();
		if (hi > lo) n = W.idx[0];
		glm::gi_sync();
	}
#endif
	if (n == 0) return I;
	if (lead) cor::rc_fill_keys(W.x, n, W);
	cor::rc_sort(W, n, tid, threads);
	if (lead) {
		GI_LANES_BEGIN(lane)
		for (int64_t k = lane; k < n; k += 64) W.x[k] = W.y[W.idx[k]];
		GI_LANES_END
	}
	glm::gi_sync();
	if (lead && P.test != kPtMmd) {
		RC_NO_CONTRACT
		const double mid = W.key[n / 2];
		GI_LANES_BEGIN(lane)
		for (int64_t k = lane; k < n; k += 64) {
			if (P.test == kPtTTest) W.y[k] = W.key[k] - mid;
			else W.y[k] = k + 1 < n ? W.key[k + 1] - W.key[k] : 0.0;
		}
		GI_LANES_END
	}
	glm::gi_sync();
	return I;
}

// Energy distance and t-test: the observed statistic (with aux) and this wavefront's count over the rounds wave, wave + waves, ...
GI_DEV int64_t pt_rounds(const PermTestProblem &P, const PtInfo &I, const CorWork &W, int64_t wave, int64_t waves, double &obs, double &aux) {
	GiPL<double> t0, a0;
	GI_LANES_BEGIN(lane)
	(void)lane;
	double df = NAN;
	t0.v[GI_AT(lane)] = P.test == kPtTTest ? pt_t_walk(W, I.n, I.n1, true, 0, df) : pt_energy_walk(W, I.n, I.n1, true, 0);
	a0.v[GI_AT(lane)] = df;
	GI_LANES_END
	obs = t0.v[0];
	aux = a0.v[0];
	GiPL<int64_t> cnt;
	GI_LANES_BEGIN(lane)
	int64_t c = 0;
	if (obs == obs) {
		for (int64_t r = wave; r * 64 < P.n_perm; r += waves) {
			const int64_t b = r * 64 + lane;
			if (b >= P.n_perm) continue;
			double df;
			const uint64_t state = pt_stream_start(P.seed, b);
			const double t = P.test == kPtTTest ? pt_t_walk(W, I.n, I.n1, false, state, df) : pt_energy_walk(W, I.n, I.n1, false, state);
			c += pt_hit(P, t, obs);
		}
	}
	cnt.v[GI_AT(lane)] = c;
	GI_LANES_END
	return glm::gi_sum_i(cnt);
}

// ---- MMD ----

// the pairs i < j of the sorted z with z_j - z_i <= t (the difference as computed: rounding keeps it monotone in j)
GI_DEV int64_t pt_pairs_within(const double *z, int64_t n, double t) {
	RC_NO_CONTRACT
	GiPL<int64_t> s;
	GI_LANES_BEGIN(lane)
	int64_t c = 0;
	for (int64_t i = lane; i < n; i += 64) {
		int64_t l = i, h = n; // z[l] - z[i] <= t (l = i: 0), z[h] - z[i] > t (h = n: past the end)
		while (h - l > 1) {
			const int64_t m = l + (h - l) / 2;
			if (z[m] - z[i] <= t) l = m;
			else h = m;
		}
		c += l - i;
	}
	s.v[GI_AT(lane)] = c;
	GI_LANES_END
	return glm::gi_sum_i(s);
}

GI_DEV double pt_from_bits(uint64_t u) {
	double d;
	memcpy(&d, &u, sizeof d);
	return d;
}

// the lower median of the pairwise distances of the sorted z (n >= 4): the smallest t, by its bit pattern, with at least
// ceil(M / 2) pairs within it
GI_DEV double pt_mmd_sigma(const double *z, int64_t n) {
	RC_NO_CONTRACT
	const int64_t pairs = n * (n - 1) / 2, want = (pairs + 1) / 2;
	if (pt_pairs_within(z, n, 0.0) >= want) return 0.0;
	const double top = z[n - 1] - z[0];
	uint64_t lo = 0, hi;
	memcpy(&hi, &top, sizeof hi);
	while (hi - lo > 1) { // fewer than `want` pairs within lo, at least `want` within hi
		const uint64_t mid = lo + (hi - lo) / 2;
		if (pt_pairs_within(z, n, pt_from_bits(mid)) >= want) hi = mid;
		else lo = mid;
	}
	return pt_from_bits(hi);
}

// the label words of the round that starts at permutation b0: bit l of words[k] = lane l's label of row k
GI_DEV void pt_draw_words(const PermTestProblem &P, pt_word *words, int64_t n, int64_t n1, int64_t b0) {
#if defined(__HIPCC__)
	const int lane = (int)(threadIdx.x & 63u);
	const int64_t b = b0 + lane;
	uint64_t state = pt_stream_start(P.seed, b);
	int64_t taken = 0;
	for (int64_t k = 0; k < n; ++k) {
		const bool join = b < P.n_perm && pt_draw(state, n - k, n1 - taken);
		taken += join;
		const unsigned long long w = __ballot(join);
		if (lane == 0) words[k] = w;
	}
#else
	for (int64_t k = 0; k < n; ++k) words[k] = 0;
	for (int lane = 0; lane < 64 && b0 + lane < P.n_perm; ++lane) {
		uint64_t state = pt_stream_start(P.seed, b0 + lane);
		int64_t taken = 0;
		for (int64_t k = 0; k < n; ++k) {
			const bool join = pt_draw(state, n - k, n1 - taken);
			taken += join;
			words[k] |= (uint64_t)join << lane;
		}
	}
#endif
}

// MMD^2 of the 64 labellings in `words`, one per lane, in the pair order of the head of this file.  buf: min(64, n) doubles.
GI_DEV void pt_mmd_pass(const double *z, const pt_word *words, double *buf, int64_t n, int64_t n1, double den, GiPL<double> &stat) {
	RC_NO_CONTRACT
	GiPL<double> axx, ayy, axy;
	GI_LANES_BEGIN(lane)
	(void)lane;
	axx.v[GI_AT(lane)] = ayy.v[GI_AT(lane)] = axy.v[GI_AT(lane)] = 0.0;
	GI_LANES_END
	for (int64_t i = 0; i + 1 < n; ++i) {
		const double zi = z[i];
		const uint64_t wi = words[i];
		for (int64_t j0 = i / 64 * 64; j0 < n; j0 += 64) {
			GI_LANES_BEGIN(lane)
			if (j0 + lane < n) {
				const double d = zi - z[j0 + lane];
				buf[lane] = exp(-(d * d) / den);
			}
			GI_LANES_END
			glm::gi_sync();
			const int l_hi = n - 1 - j0 < 63 ? (int)(n - 1 - j0) : 63, l_lo = i + 1 > j0 ? (int)(i + 1 - j0) : 0;
			GI_LANES_BEGIN(lane)
			const bool bi = (wi >> lane) & 1u;
			double sxx = axx.v[GI_AT(lane)], syy = ayy.v[GI_AT(lane)], sxy = axy.v[GI_AT(lane)];
			for (int l = l_hi; l >= l_lo; --l) {
				const double kv = buf[l];
				const bool bj = (words[j0 + l] >> lane) & 1u;
				sxx += bi && bj ? kv : 0.0;
				syy += !bi && !bj ? kv : 0.0;
				sxy += bi != bj ? kv : 0.0;
			}
			axx.v[GI_AT(lane)] = sxx;
			ayy.v[GI_AT(lane)] = syy;
			axy.v[GI_AT(lane)] = sxy;
			GI_LANES_END
			glm::gi_sync();
		}
	}
	const double dn1 = (double)n1, dn2 = (double)(n - n1);
	GI_LANES_BEGIN(lane)
	(void)lane;
	const double sxx = axx.v[GI_AT(lane)], syy = ayy.v[GI_AT(lane)], sxy = axy.v[GI_AT(lane)];
	stat.v[GI_AT(lane)] = ((dn1 + 2.0 * sxx) / (dn1 * dn1) + (dn2 + 2.0 * syy) / (dn2 * dn2)) - 2.0 * sxy / (dn1 * dn2);
	GI_LANES_END
}

// MMD by the one wavefront of the small path: sigma (in aux), the observed statistic and the count over every round.
// W.key: z, W.x: the observed labels on entry, then the label words; W.y: the row buffer.
GI_DEV int64_t pt_mmd_rounds(const PermTestProblem &P, const PtInfo &I, const CorWork &W, double &obs, double &aux) {
	RC_NO_CONTRACT
	const int64_t n = I.n;
	const double sigma = P.sigma > 0.0 ? P.sigma : pt_mmd_sigma(W.key, n);
	aux = sigma;
	obs = NAN;
	if (!(sigma > 0.0)) return 0;
	const double den = 2.0 * sigma * sigma;
	pt_word *words = (pt_word *)W.x;
	GI_LANES_BEGIN(lane)
	for (int64_t k = lane; k < n; k += 64) {
		const bool one = W.x[k] != 0.0;
		words[k] = one ? ~0ull : 0ull;
	}
	GI_LANES_END
	glm::gi_sync();
	GiPL<double> stat;
	pt_mmd_pass(W.key, words, W.y, n, I.n1, den, stat);
	obs = stat.v[0];
	GiPL<int64_t> cnt;
	GI_LANES_BEGIN(lane)
	(void)lane;
	cnt.v[GI_AT(lane)] = 0;
	GI_LANES_END
	if (obs == obs) {
		for (int64_t b0 = 0; b0 < P.n_perm; b0 += 64) {
			pt_draw_words(P, words, n, I.n1, b0);
			glm::gi_sync();
			pt_mmd_pass(W.key, words, W.y, n, I.n1, den, stat);
			GI_LANES_BEGIN(lane)
			if (b0 + lane < P.n_perm) cnt.v[GI_AT(lane)] += stat.v[GI_AT(lane)] >= obs;
			GI_LANES_END
		}
	}
	return glm::gi_sum_i(cnt);
}

// ---- the record ----

RC_CALL void pt_record(const PermTestProblem &P, const PtInfo &I, double obs, double aux, int64_t n_extreme, double *rec) {
	RC_NO_CONTRACT
	for (int j = 0; j < kPtRecordLen; ++j) rec[j] = NAN;
	rec[4] = (double)I.n;
	rec[5] = (double)I.n1;
	rec[6] = (double)(I.n - I.n1);
	rec[7] = (double)I.status;
	if (I.status != 0) return;
	rec[0] = obs;
	rec[2] = aux;
	rec[3] = (double)n_extreme;
	if (obs == obs && P.n_perm > 0) rec[1] = (1.0 + (double)n_extreme) / ((double)P.n_perm + 1.0);
}

// ---- one group on one wavefront (the small path; the host build's large path adds pt_rounds over the waves itself) ----
// tid: the lane, for the sort
GI_DEV void pt_group(const PermTestProblem &P, int64_t g, int64_t lo, int64_t hi, const CorWork &W, int64_t tid) {
	const PtInfo I = pt_prepare(P, lo, hi, W, true, tid, 64, true);
	double obs = NAN, aux = NAN;
	int64_t count = 0;
	if (I.status == 0) count = P.test == kPtMmd ? pt_mmd_rounds(P, I, W, obs, aux) : pt_rounds(P, I, W, 0, 1, obs, aux);
	GI_LANES_BEGIN(lane)
	if (lane == 0) pt_record(P, I, obs, aux, count, P.records + g * kPtRecordLen);
	GI_LANES_END
}

} // namespace permtest
} // namespace anofox
