// lmm_profile.h — the Gaussian linear mixed model with one random intercept, fitted by profiled (restricted) maximum
// likelihood from per-level means and a within-level scatter.  DESIGN.md §1, "Linear mixed models".
//
//     y_ij = a_ij'beta + b_j + e_ij,   b_j ~ N(0, sb2),   e ~ N(0, s2),   theta = sb2 / s2,   k = p + [intercept] <= 33
//     per level j (valid rows only):  n_j, abar_j, ybar_j
//     per panel:  W = sum_j sum_i (a - abar_j)(a - abar_j)',  w = sum (a - abar_j)(y - ybar_j),  omega = sum (y - ybar_j)^2
//     lambda_j = n_j / (1 + n_j theta)
//     A = W + sum lambda_j abar_j abar_j'   c = w + sum lambda_j abar_j ybar_j   beta = A^-1 c (Cholesky)
//     RSS = (omega - 2 w'beta + beta'W beta) + sum lambda_j r_j^2,  r_j = ybar_j - abar_j'beta   (= q - c'beta at the minimiser;
//           this form is a within part, floored at 0, plus a sum of squares, so it cannot turn negative by cancellation)
//     m = n - k (REML) | n (ML)    s2 = RSS / m
//     l = -1/2 [ m log(2 pi s2) + sum log(1 + n_j theta) + m + (REML) log det A ]
//     dl/dtheta = -1/2 [ sum lambda_j - (m / RSS) sum lambda_j^2 r_j^2 - (REML) sum lambda_j^2 abar_j'A^-1 abar_j ]
//     theta^ : the root of u -> theta dl/dtheta, u = log theta, on [log 1e-10, log 1e10] (lm_fit_panel)
//     BLUP b_j = theta lambda_j r_j
//
// Fit-predict ("Mixed-model fit-predict").  A row a of level j is scored with
//     yhat_fixed = a'beta^      yhat = yhat_fixed + b^_j      s_j = theta^ lambda_j  (0, like b^_j, for a level without a valid row)
//     se^2 = s2 [ c'A^-1 c + theta^ / (1 + n_j theta^) ],   c = a - s_j abar_j
// the variance of the prediction error (a'beta^ + b^_j) - (a'beta + b_j) at known theta.  Derivation: at known beta the BLUP is
// b~_j = s_j (ybar_j - abar_j'beta), and b~_j - b_j has variance s2 theta / (1 + n_j theta) (the posterior variance of b_j given
// the level's mean: sb2 - sb2^2 / (sb2 + s2 / n_j)).  With beta^ in place of beta, b^_j = b~_j - s_j abar_j'(beta^ - beta), so the
// error is  c'(beta^ - beta) + (b~_j - b_j).  b~_j - b_j is the error of a conditional mean given y and hence uncorrelated with
// every linear function of y, beta^ - beta (GLS, variance s2 A^-1) among them: the two variances add.  n_j = 0: c = a and the
// variance is s2 (a'A^-1 a + theta^), an unseen level.  theta^ = 0: the OLS confidence variance s2 a'(X'X)^-1 a.
// c'A^-1 c = |L^-1 c|^2 with A = L L': a forward substitution against the factor's inverse, which the last evaluation of the
// search has already formed, and not the expanded a'Ma - 2 a'(M s_j abar_j) + s_j^2 abar_j'M abar_j: for a level with many rows
// s_j -> 1 and c = a - abar_j is small against a, so the expanded form loses what the difference cancels and may turn negative,
// while the sum of squares cannot; it also needs no k x k product per level.  A column dropped by the pivot rule has a zero row
// and column in L^-1 and a zero coefficient, so it contributes nothing.
//
// One source for both builds (the lanes of glm_irls.h).  Two stages:
//   lm_chunk_stats  ONE WAVEFRONT per chunk of 64 levels of a panel.  Sweep A: per level the valid rows (a byte per row in a
//                   scratch that only the row's own lane touches), n_j and the means, into the level record {n, ybar, abar[k]}.
//                   When no level of the chunk has more than 32 rows, four levels share the wavefront (lane = 4 r + sub:
//                   sub the level, r the row), else a level has all 64 lanes.  Sweep B: per entry (a >= b) of the augmented
//                   scatter [W w; w' omega] every lane adds its own rows of all the chunk's levels, centred at the level's mean,
//                   and one butterfly gives the chunk's partial.  That is k + 2 + E passes over the chunk's rows (E = (k + 1)
//                   (k + 2) / 2, 16 + 2 at p = 3, 596 + 2 at p = 32): the first comes from HBM, the others from the caches only
//                   while the chunk's rows fit there (64 levels x 15 rows x 4 columns are 30 KB; a chunk of large levels or
//                   many columns is re-read from L2 or HBM).  Lanes over matrix entries on a row tile in LDS, as glm_irls.h
//                   forms its Gram matrix, would read every row once at any size; it is not built (docs/MEASUREMENTS.md has
//                   what this costs).  Chunks are numbered without a prefix sum (eb_shrink.h):
//                   panel g owns the numbers from (plo[g] - plo[0]) / 64 + g on.
//   lm_fit_panel    ONE WORKGROUP of W wavefronts (1, 4 or 16 by the panel's level count, lm_wave_count) per panel.  Threads own
//                   matrix entries: with E = (k + 1)(k + 2) / 2 entries and T = 64 W threads, T / E slices of the levels each
//                   add all E entries (or, E > T, every thread owns several entries of one slice), and the slices are added
//                   in their order.  The five scalar sums of an evaluation go through the wavefronts' butterflies and then over
//                   the wavefronts in their order.  Cholesky, back substitution and L^-1 are the first wavefront's; the control
//                   flow is the same in every thread.  The order of every sum depends on (k, W, the panel's levels) only.
#pragma once
#include "glm_irls.h"

#if defined(__HIPCC__)
#define LM_WAVES_BEGIN(w, W) { const int w = (int)(threadIdx.x >> 6);
#define LM_WAVE0_BEGIN(lane) if (threadIdx.x < 64u) { const int lane = (int)threadIdx.x;
#define LM_SYNC() __syncthreads()
#else
#define LM_WAVES_BEGIN(w, W) for (int w = 0; w < (W); ++w) {
#define LM_WAVE0_BEGIN(lane) for (int lane = 0; lane < 64; ++lane) {
#define LM_SYNC()
#endif
#define LM_WAVES_END }
#define LM_WAVE0_END }

namespace anofox {
namespace lmm {

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

using glm::GiPL;
using glm::gi_finite;

constexpr int kLmMaxP = 32;
constexpr double kLmThetaLo = 1e-10, kLmThetaHi = 1e10; // the bracket of the search (a decision of ours)
constexpr int64_t kLmChunkLevels = 64;
constexpr int64_t kLmSharedRows = 32; // a chunk whose levels all have this many rows at most: four levels per wavefront
constexpr double kLmRankTol = 1e-10;  // the pivot rule of glm_irls.h
constexpr int kLmStatusInvalidInput = 1;
constexpr int kLmStatusInsufficientData = 6;
constexpr int kLmStatusNoValidData = 10;

struct LmProblem {
	const double *y;
	const double *const *x; // p column pointers
	int p;
	int fit_intercept;
	const int64_t *plo; // [n_panels + 1]
	const int64_t *lro; // [n_levels + 1]
	int64_t n_panels, n_levels, n_rows;
	int reml;
	int max_iterations;
	double tolerance;
	int compute_inference;
	double zq;   // the normal quantile of the confidence level
	int invalid; // invalid options: every panel gets status 1
	// the workspace
	double *lev;          // [n_levels x (k + 2)]: {n_j, ybar_j, abar_j[k]}
	unsigned char *valid; // [n_rows]
	double *parts;        // [n_numbers x E]
	int64_t n_numbers;    // n_levels / 64 + n_panels
	// the outputs
	double *rec;      // [n_panels x (p + 13)]
	double *inf;      // [n_panels x (5 p + 1)] or nullptr
	double *ranef;    // [n_levels]
	int64_t *level_n; // [n_levels] or nullptr
	// fit-predict only (nullptr for a fit): what the search keeps for the prediction pass, in the call's scratch
	double *keep;       // [n_panels x lm_keep_len(k)]: {theta, s2, beta[k] (0 for a dropped column), L^-1 packed lower (lm_idx)}
	double *keep_ok;    // [n_panels]: 1.0 once the panel's record above is written (the entry zeroes it before the launches)
	double *level_pred; // [n_levels x (k + 3)]: {s_j, b_j, theta / (1 + n_j theta), s_j abar_j[k]}
};

GI_HD int lm_k(int p, int fit_intercept) { return p + (fit_intercept ? 1 : 0); }
GI_HD int lm_entries(int k) { return (k + 1) * (k + 2) / 2; }
GI_HD int lm_idx(int a, int b) { return a * (a + 1) / 2 + b; } // a >= b
GI_HD int lm_record_len(int p) { return p + 13; }
GI_HD int lm_inference_len(int p) { return 5 * p + 1; }
GI_HD int lm_wave_count(int64_t levels) { return levels <= 64 ? 1 : (levels <= 1024 ? 4 : 16); }
GI_HD int lm_red_doubles(int k, int W) {
	const int E = lm_entries(k), T = 64 * W;
	return E > T ? E : T;
}
// doubles of work memory (LDS on the device): aug, base, linv, beta, diag0, red
GI_HD size_t lm_work_doubles(int k, int W) {
	return 2 * (size_t)(k + 1) * glm::gi_aug_ld(k) + (size_t)lm_entries(k) + 2 * (size_t)(k + 1) + (size_t)lm_red_doubles(k, W);
}
GI_HD int lm_keep_len(int k) { return 2 + k + k * (k + 1) / 2; }
GI_HD int lm_level_pred_len(int k) { return k + 3; }
constexpr int kLmPredLen = 5; // yhat, yhat_fixed, se, lower, upper
GI_HD int64_t lm_clip(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// the first chunk number of panel g (g == n_panels: the count of numbers is at most this)
GI_HD int64_t lm_chunk_base(const int64_t *plo, int64_t g) { return (plo[g] - plo[0]) / kLmChunkLevels + g; }

GI_DEV void lm_entry(int e, int &a, int &b) {
	a = 0;
	while ((a + 1) * (a + 2) / 2 <= e) ++a;
	b = e - a * (a + 1) / 2;
}

// element c of the row's design vector; c == k: y
GI_DEV double lm_elem(const LmProblem &P, int k, int c, int64_t i) {
	if (c == k) return P.y[i];
	if (P.fit_intercept) return c == 0 ? 1.0 : P.x[c - 1][i];
	return P.x[c][i];
}

GI_DEV void lm_reduce(GiPL<double> &s, int m_lo) {
#if defined(__HIPCC__)
	s.v[0] = glm::gi_sum(s, m_lo);
#else
	glm::gi_sum(s, m_lo);
#endif
}

// ---- stage 1: the level statistics of one chunk, by one wavefront ----

// the levels [l0, l1) of chunk number v and its panel; false: an idle number
GI_DEV bool lm_chunk_range(const LmProblem &P, int64_t v, int64_t &l0, int64_t &l1) {
	int64_t a = 0, b = P.n_panels - 1;
	while (a < b) {
		const int64_t mid = a + (b - a + 1) / 2;
		if (lm_chunk_base(P.plo, mid) <= v) a = mid;
		else b = mid - 1;
	}
	const int64_t j = v - lm_chunk_base(P.plo, a);
	const int64_t p0 = lm_clip(P.plo[a], P.n_levels);
	int64_t p1 = lm_clip(P.plo[a + 1], P.n_levels);
	if (p1 < p0) p1 = p0;
	if (j < 0) return false;
	l0 = p0 + j * kLmChunkLevels;
	if (l0 >= p1) return false;
	l1 = l0 + kLmChunkLevels < p1 ? l0 + kLmChunkLevels : p1;
	return true;
}

// the rows of level l, clipped into the arrays
GI_DEV void lm_level_rows(const LmProblem &P, int64_t l, int64_t &lo, int64_t &hi) {
	lo = lm_clip(P.lro[l], P.n_rows);
	hi = lm_clip(P.lro[l + 1], P.n_rows);
	if (hi < lo) hi = lo;
}

GI_DEV void lm_chunk_stats(const LmProblem &P, int64_t v) {
	int64_t l0, l1;
	if (v < 0 || v >= P.n_numbers || !lm_chunk_range(P, v, l0, l1)) return;
	const int k = lm_k(P.p, P.fit_intercept), E = lm_entries(k), rl = k + 2;
	GiPL<double> s;
	GI_LANES_BEGIN(lane)
	double m = 0.0;
	if (l0 + lane < l1) {
		int64_t lo, hi;
		lm_level_rows(P, l0 + lane, lo, hi);
		m = (double)(hi - lo);
	}
	s.v[GI_AT(lane)] = m;
	GI_LANES_END
	const int nsub = glm::gi_max(s) <= (double)kLmSharedRows ? 4 : 1, stride = 64 / nsub;
	const int64_t steps = (l1 - l0 + nsub - 1) / nsub;
	// sweep A: validity, counts, means
	for (int64_t st = 0; st < steps; ++st) {
		GiPL<double> cnt;
		GI_LANES_BEGIN(lane)
		const int64_t l = l0 + st * nsub + (lane & (nsub - 1));
		double c = 0.0;
		if (l < l1) {
			int64_t lo, hi;
			lm_level_rows(P, l, lo, hi);
			for (int64_t i = lo + lane / nsub; i < hi; i += stride) {
				bool ok = gi_finite(P.y[i]);
				for (int j = 0; j < P.p; ++j) ok = ok && gi_finite(P.x[j][i]);
				P.valid[i] = ok ? 1 : 0;
				c += ok ? 1.0 : 0.0;
			}
		}
		cnt.v[GI_AT(lane)] = c;
		GI_LANES_END
		lm_reduce(cnt, nsub);
		for (int c = 0; c <= k; ++c) {
			GI_LANES_BEGIN(lane)
			const int64_t l = l0 + st * nsub + (lane & (nsub - 1));
			double a = 0.0;
			if (l < l1) {
				int64_t lo, hi;
				lm_level_rows(P, l, lo, hi);
				for (int64_t i = lo + lane / nsub; i < hi; i += stride)
					if (P.valid[i]) a += lm_elem(P, k, c, i);
			}
			s.v[GI_AT(lane)] = a;
			GI_LANES_END
			lm_reduce(s, nsub);
			GI_LANES_BEGIN(lane)
			const int L = GI_AT(lane);
			const int64_t l = l0 + st * nsub + (lane & (nsub - 1));
			if (l < l1 && lane < nsub) { // the first lane of a level writes its record
				const double n = cnt.v[L];
				double *r = P.lev + l * rl;
				r[0] = n;
				r[c == k ? 1 : 2 + c] = n > 0.0 ? s.v[L] / n : 0.0;
				if (c == 0 && P.level_n) P.level_n[l] = (int64_t)n;
			}
			GI_LANES_END
		}
	}
	glm::gi_sync(); // the records are read by other lanes than wrote them
	// sweep B: the chunk's partial of every entry of [W w; w' omega]
	for (int e = 0; e < E; ++e) {
		int ea, eb;
		lm_entry(e, ea, eb);
		const bool zero = P.fit_intercept && eb == 0; // the centred intercept column is 0
		GI_LANES_BEGIN(lane)
		double acc = 0.0;
		if (!zero) {
			for (int64_t st = 0; st < steps; ++st) {
				const int64_t l = l0 + st * nsub + (lane & (nsub - 1));
				if (l >= l1) continue;
				int64_t lo, hi;
				lm_level_rows(P, l, lo, hi);
				const double *r = P.lev + l * rl;
				const double ma = r[ea == k ? 1 : 2 + ea], mb = r[eb == k ? 1 : 2 + eb];
				for (int64_t i = lo + lane / nsub; i < hi; i += stride)
					if (P.valid[i]) acc += (lm_elem(P, k, ea, i) - ma) * (lm_elem(P, k, eb, i) - mb);
			}
		}
		s.v[GI_AT(lane)] = acc;
		GI_LANES_END
		lm_reduce(s, 1);
		GI_LANES_BEGIN(lane)
		if (lane == 0) P.parts[v * E + e] = s.v[GI_AT(lane)];
		GI_LANES_END
	}
}

// ---- stage 2: the profile search of one panel, by one workgroup of W wavefronts ----

struct LmWork {
	double *aug;   // (k + 1) x ld: A with [c q] as row k, then its Cholesky factor
	double *linv;  // (k + 1) x ld: L^-1 (lower)
	double *base;  // E: [W w; w' omega]
	double *beta;  // k + 1
	double *diag0; // k + 1
	double *red;   // lm_red_doubles
	int ld;
};

GI_DEV LmWork lm_work(double *mem, int k) {
	LmWork w;
	w.ld = glm::gi_aug_ld(k);
	w.aug = mem;
	w.linv = w.aug + (size_t)(k + 1) * w.ld;
	w.base = w.linv + (size_t)(k + 1) * w.ld;
	w.beta = w.base + lm_entries(k);
	w.diag0 = w.beta + (k + 1);
	w.red = w.diag0 + (k + 1);
	return w;
}

// out(e, a, b, sum over j < N of f(j, e, a, b)) for every entry e, the sum in slices of j added in their order
template <class F, class O>
GI_DEV void lm_accumulate(int W, int E, int64_t N, double *red, F f, O out) {
	const int T = 64 * W, S = T / E < 1 ? 1 : T / E;
	LM_WAVES_BEGIN(w, W)
	GI_LANES_BEGIN(lane)
	const int t = w * 64 + lane;
	if (S > 1) {
		if (t < S * E) {
			const int e = t % E, sl = t / E;
			int a, b;
			lm_entry(e, a, b);
			double acc = 0.0;
			for (int64_t j = sl; j < N; j += S) acc += f(j, e, a, b);
			red[sl * E + e] = acc;
		}
	} else {
		for (int e = t; e < E; e += T) {
			int a, b;
			lm_entry(e, a, b);
			double acc = 0.0;
			for (int64_t j = 0; j < N; ++j) acc += f(j, e, a, b);
			red[e] = acc;
		}
	}
	GI_LANES_END
	LM_WAVES_END
	LM_SYNC();
	LM_WAVES_BEGIN(w, W)
	GI_LANES_BEGIN(lane)
	for (int e = w * 64 + lane; e < E; e += T) {
		int a, b;
		lm_entry(e, a, b);
		double sum = 0.0;
		for (int sl = 0; sl < S; ++sl) sum += red[sl * E + e];
		out(e, a, b, sum);
	}
	GI_LANES_END
	LM_WAVES_END
	LM_SYNC();
}

struct LmSums {
	double v[5];
};

// five sums over the levels: f(j, s) adds level j into s; every thread gets the totals
template <class F>
GI_DEV LmSums lm_sums(int W, int64_t N, double *red, F f) {
	const int T = 64 * W;
	LM_WAVES_BEGIN(w, W)
	GiPL<double> pl[5];
	GI_LANES_BEGIN(lane)
	double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
	for (int64_t j = w * 64 + lane; j < N; j += T) f(j, s);
	for (int q = 0; q < 5; ++q) pl[q].v[GI_AT(lane)] = s[q];
	GI_LANES_END
	for (int q = 0; q < 5; ++q) lm_reduce(pl[q], 1);
	GI_LANES_BEGIN(lane)
	if (lane == 0)
		for (int q = 0; q < 5; ++q) red[q * W + w] = pl[q].v[GI_AT(lane)];
	GI_LANES_END
	LM_WAVES_END
	LM_SYNC();
	LmSums r;
	for (int q = 0; q < 5; ++q) {
		double a = 0.0;
		for (int w = 0; w < W; ++w) a += red[q * W + w];
		r.v[q] = a;
	}
	LM_SYNC();
	return r;
}

// Cholesky of the leading k x k block of aug in place (lower), row k carried along -> the mask of the skipped columns
GI_DEV uint64_t lm_cholesky(const LmWork &M, int k) {
	const int ld = M.ld;
	LM_WAVE0_BEGIN(lane)
	if (lane < k) M.diag0[lane] = M.aug[lane * ld + lane];
	LM_WAVE0_END
	LM_SYNC();
	uint64_t alias = 0;
	for (int j = 0; j < k; ++j) {
		const double piv = M.aug[j * ld + j];
		if (!(piv > kLmRankTol * M.diag0[j]) || !(piv > 0.0)) {
			alias |= 1ull << j;
			continue;
		}
		const double l = sqrt(piv);
		LM_SYNC();
		LM_WAVE0_BEGIN(lane)
		const int i = j + lane;
		if (lane == 0) M.aug[j * ld + j] = l;
		else if (i <= k) M.aug[i * ld + j] /= l;
		LM_WAVE0_END
		LM_SYNC();
		LM_WAVE0_BEGIN(lane)
		const int i = j + 1 + lane;
		if (i <= k) {
			const double lij = M.aug[i * ld + j];
			const int ce = i < k ? i : k - 1;
			for (int c = j + 1; c <= ce; ++c) M.aug[i * ld + c] -= lij * M.aug[c * ld + j];
		}
		LM_WAVE0_END
		LM_SYNC();
	}
	return alias;
}

GI_DEV void lm_back_substitute(const LmWork &M, int k, uint64_t alias) {
	const int ld = M.ld;
	for (int j = k - 1; j >= 0; --j) {
		const bool skip = (alias >> j) & 1;
		const double bj = skip ? 0.0 : M.aug[k * ld + j] / M.aug[j * ld + j];
		LM_SYNC();
		LM_WAVE0_BEGIN(lane)
		if (lane == 0) M.beta[j] = bj;
		if (!skip && lane < j && !((alias >> lane) & 1)) M.aug[k * ld + lane] -= M.aug[j * ld + lane] * bj;
		LM_WAVE0_END
		LM_SYNC();
	}
}

// L^-1 into linv (lower; the rows and columns of skipped columns are 0): lane j solves L v = e_j
GI_DEV void lm_invert_factor(const LmWork &M, int k, uint64_t alias) {
	const int ld = M.ld;
	LM_WAVE0_BEGIN(lane)
	if (lane < k) {
		const int j = lane;
		const bool dead = (alias >> j) & 1;
		for (int i = 0; i < k; ++i) {
			double v = 0.0;
			if (!dead && i >= j && !((alias >> i) & 1)) {
				double s = i == j ? 1.0 : 0.0;
				for (int c = j; c < i; ++c)
					if (!((alias >> c) & 1)) s -= M.aug[i * ld + c] * M.linv[c * ld + j];
				v = s / M.aug[i * ld + i];
			}
			M.linv[i * ld + j] = v;
		}
	}
	LM_WAVE0_END
	LM_SYNC();
}

struct LmEval {
	double ell, score; // the log-likelihood and d ell / d theta
	double sigma2, rss;
	uint64_t alias;
	int kept;
};

GI_DEV int lm_popcount(uint64_t m) {
	int c = 0;
	for (; m; m &= m - 1) ++c;
	return c;
}

// one evaluation of the profiled likelihood at theta; afterwards beta is in M.beta, the factor in M.aug, L^-1 in M.linv (when
// `invert` or REML)
GI_DEV LmEval lm_eval(const LmProblem &P, const LmWork &M, const double *lev, int64_t N, int W, int k, double theta, double n, bool invert) {
	const int rl = k + 2, ld = M.ld;
	lm_accumulate(
	    W, lm_entries(k), N, M.red,
	    [&](int64_t j, int, int a, int b) {
		    const double *r = lev + j * rl;
		    const double nj = r[0], lam = nj / (1.0 + nj * theta);
		    return lam * (r[a == k ? 1 : 2 + a] * r[b == k ? 1 : 2 + b]);
	    },
	    [&](int e, int a, int b, double sum) { M.aug[a * ld + b] = M.base[e] + sum; });
	LmEval R;
	R.alias = lm_cholesky(M, k);
	R.kept = k - lm_popcount(R.alias);
	double logdet = 0.0;
	for (int j = 0; j < k; ++j)
		if (!((R.alias >> j) & 1)) logdet += 2.0 * log(M.aug[j * ld + j]);
	lm_back_substitute(M, k, R.alias);
	const bool reml = P.reml != 0;
	if (reml || invert) lm_invert_factor(M, k, R.alias);
	const LmSums S = lm_sums(W, N, M.red, [&](int64_t j, double *s) {
		const double *r = lev + j * rl;
		const double nj = r[0];
		if (!(nj > 0.0)) return;
		const double lam = nj / (1.0 + nj * theta);
		double res = r[1];
		for (int c = 0; c < k; ++c) res -= r[2 + c] * M.beta[c];
		s[0] += lam;
		s[1] += lam * (res * res);
		s[2] += (lam * lam) * (res * res);
		s[3] += log1p(nj * theta);
		if (reml) {
			double quad = 0.0;
			for (int i = 0; i < k; ++i) {
				double d = 0.0;
				for (int c = 0; c <= i; ++c) d += M.linv[i * ld + c] * r[2 + c];
				quad += d * d;
			}
			s[4] += (lam * lam) * quad;
		}
	});
	double within = M.base[lm_idx(k, k)];
	for (int a = 0; a < k; ++a) {
		double row = 0.0;
		for (int b = 0; b < k; ++b) row += M.base[a >= b ? lm_idx(a, b) : lm_idx(b, a)] * M.beta[b];
		within += M.beta[a] * (row - 2.0 * M.base[lm_idx(k, a)]);
	}
	R.rss = (within > 0.0 ? within : 0.0) + S.v[1];
	const double m = n - (reml ? (double)R.kept : 0.0);
	R.sigma2 = R.rss / m;
	R.ell = -0.5 * (m * log(6.283185307179586477 * R.sigma2) + S.v[3] + m + (reml ? logdet : 0.0));
	R.score = -0.5 * (S.v[0] - (m / R.rss) * S.v[2] - (reml ? S.v[4] : 0.0));
	return R;
}

GI_DEV void lm_fail_panel(const LmProblem &P, int64_t g, int64_t l0, int64_t N, int W, int status) {
	const int rlen = lm_record_len(P.p), ilen = lm_inference_len(P.p), T = 64 * W;
	LM_WAVES_BEGIN(w, W)
	GI_LANES_BEGIN(lane)
	const int t = w * 64 + lane;
	for (int j = t; j < rlen; j += T) P.rec[g * rlen + j] = j == rlen - 1 ? (double)status : NAN;
	if (P.inf)
		for (int j = t; j < ilen; j += T) P.inf[g * ilen + j] = NAN;
	for (int64_t j = t; j < N; j += T) P.ranef[l0 + j] = NAN;
	GI_LANES_END
	LM_WAVES_END
}

// The fit of panel g by a workgroup of W wavefronts on `mem` (lm_work_doubles(k, W) doubles).  KEEP false: a fit that is compiled
// without the writes of a fit-predict (P.keep and P.level_pred are then not looked at), so a fit runs the code it always ran.
template <bool KEEP = true>
GI_DEV void lm_fit_panel(const LmProblem &P, int64_t g, int W, double *mem) {
	const int k = lm_k(P.p, P.fit_intercept), E = lm_entries(k), rl = k + 2, p = P.p, T = 64 * W;
	const LmWork M = lm_work(mem, k);
	const int ld = M.ld;
	const int64_t l0 = lm_clip(P.plo[g], P.n_levels);
	int64_t l1 = lm_clip(P.plo[g + 1], P.n_levels);
	if (l1 < l0) l1 = l0;
	const int64_t N = l1 - l0;
	const double *lev = P.lev + l0 * rl;
	LM_SYNC(); // the work memory of the panel before
	if (P.invalid) {
		lm_fail_panel(P, g, l0, N, W, kLmStatusInvalidInput);
		return;
	}
	// [W w; w' omega]: the panel's chunk partials in their order
	const int64_t v0 = lm_chunk_base(P.plo, g), n_chunks = (N + kLmChunkLevels - 1) / kLmChunkLevels;
	lm_accumulate(
	    W, E, n_chunks, M.red,
	    [&](int64_t j, int e, int, int) { return v0 + j >= 0 && v0 + j < P.n_numbers ? P.parts[(v0 + j) * E + e] : 0.0; },
	    [&](int e, int, int, double sum) { M.base[e] = sum; });
	const LmSums C = lm_sums(W, N, M.red, [&](int64_t j, double *s) {
		const double *r = lev + j * rl;
		if (!(r[0] > 0.0)) return;
		s[0] += 1.0;
		s[1] += r[0];
		s[2] += r[0] * r[0];
		s[3] += r[0] * r[1];
	});
	const double J = C.v[0], n = C.v[1];
	int status = 0;
	if (!(n > 0.0)) status = kLmStatusNoValidData;
	else if (J < 2.0) status = kLmStatusInvalidInput;
	else if (n <= (double)(k + 1)) status = kLmStatusInsufficientData;
	else if (n == J) status = kLmStatusInvalidInput;
	if (status) {
		lm_fail_panel(P, g, l0, N, W, status);
		return;
	}
	// the start: the ANOVA moment estimate of theta
	const double ybar = C.v[3] / n;
	const LmSums B = lm_sums(W, N, M.red, [&](int64_t j, double *s) {
		const double *r = lev + j * rl;
		if (r[0] > 0.0) s[0] += r[0] * ((r[1] - ybar) * (r[1] - ybar));
	});
	const double sw2 = M.base[lm_idx(k, k)] / (n - J), msb = B.v[0] / (J - 1.0), n0 = (n - C.v[2] / n) / (J - 1.0);
	double t0 = ((msb - sw2) / n0) / sw2;
	if (!(t0 == t0) || t0 > kLmThetaHi) t0 = kLmThetaHi;
	if (t0 < kLmThetaLo) t0 = kLmThetaLo;

	double theta = 0.0;
	int iterations = 0, converged = 1;
	LmEval ev = lm_eval(P, M, lev, N, W, k, kLmThetaLo, n, false);
	if (ev.score > 0.0) {
		double a = log(kLmThetaLo);
		ev = lm_eval(P, M, lev, N, W, k, kLmThetaHi, n, false);
		if (!(ev.score < 0.0)) { // the likelihood still rises at the upper end
			theta = kLmThetaHi;
			converged = 0;
		} else {
			double b = log(kLmThetaHi);
			double u = log(t0), up = 0.0, fp = 0.0;
			bool have = false;
			if (!(u > a && u < b)) u = 0.5 * (a + b);
			converged = 0;
			while (iterations < P.max_iterations) {
				++iterations;
				const double th = exp(u);
				ev = lm_eval(P, M, lev, N, W, k, th, n, false);
				const double f = th * ev.score;
				if (f > 0.0) a = u;
				else if (f < 0.0) b = u;
				else if (f == 0.0) { converged = 1; break; }
				else break; // a NaN score: the last iterate, not converged
				double un;
				const double d = have ? (f - fp) / (u - up) : 0.0;
				if (have && d < 0.0) un = u - f / d; // Newton's step on the secant slope of the last two iterates
				else un = u + (f > 0.0 ? 1.0 : -1.0);
				if (!(un > a && un < b)) un = 0.5 * (a + b);
				const double du = un - u;
				up = u;
				fp = f;
				have = true;
				u = un;
				if (fabs(du) <= P.tolerance || b - a <= P.tolerance) { converged = 1; break; }
			}
			theta = exp(u);
		}
	}
	ev = lm_eval(P, M, lev, N, W, k, theta, n, true);
	const double K = (double)ev.kept + 2.0;
	// the record and the inference
	LM_WAVE0_BEGIN(lane)
	double *rec = P.rec + g * lm_record_len(p);
	const int c0 = P.fit_intercept ? 1 : 0;
	if (lane < p) rec[lane] = ((ev.alias >> (lane + c0)) & 1) ? NAN : M.beta[lane + c0];
	if (lane == 0) {
		double *r = rec + p;
		r[0] = P.fit_intercept ? ((ev.alias & 1) ? NAN : M.beta[0]) : NAN;
		r[1] = theta > 0.0 ? theta * ev.sigma2 : 0.0;
		r[2] = ev.sigma2;
		r[3] = theta > 0.0 ? theta / (1.0 + theta) : 0.0;
		r[4] = ev.ell;
		r[5] = 2.0 * K - 2.0 * ev.ell;
		r[6] = K * log(n) - 2.0 * ev.ell;
		r[7] = -2.0 * ev.ell;
		r[8] = n;
		r[9] = J;
		r[10] = (double)iterations;
		r[11] = (double)converged;
		r[12] = 0.0;
	}
	if (P.inf) {
		double *inf = P.inf + g * lm_inference_len(p);
		if (lane < k) {
			const int c = lane;
			double se = NAN;
			if (P.compute_inference && !((ev.alias >> c) & 1)) {
				double d = 0.0;
				for (int i = c; i < k; ++i) d += M.linv[i * ld + c] * M.linv[i * ld + c];
				se = sqrt(ev.sigma2 * d);
			}
			if (c >= c0) {
				const int f = c - c0;
				const double bta = M.beta[c], z = bta / se;
				inf[f] = se;
				inf[p + f] = z;
				inf[2 * p + f] = erfc(fabs(z) * 0.70710678118654752440);
				inf[3 * p + f] = bta - P.zq * se;
				inf[4 * p + f] = bta + P.zq * se;
			} else {
				inf[5 * p] = se;
			}
		}
		if (lane == 0 && !P.fit_intercept) inf[5 * p] = NAN;
	}
	LM_WAVE0_END
	// the BLUPs, and for a fit-predict the prologue of every level
	LM_WAVES_BEGIN(w, W)
	GI_LANES_BEGIN(lane)
	for (int64_t j = w * 64 + lane; j < N; j += T) {
		const double *r = lev + j * rl;
		const double nj = r[0];
		double bl = NAN;
		if (nj > 0.0) {
			double res = r[1];
			for (int c = 0; c < k; ++c) res -= r[2 + c] * M.beta[c];
			bl = theta > 0.0 ? theta * (nj / (1.0 + nj * theta)) * res : 0.0;
		}
		P.ranef[l0 + j] = bl;
		if (KEEP && P.level_pred) {
			double *lp = P.level_pred + (l0 + j) * lm_level_pred_len(k);
			const double sj = nj > 0.0 && theta > 0.0 ? theta * (nj / (1.0 + nj * theta)) : 0.0;
			lp[0] = sj;
			lp[1] = nj > 0.0 ? bl : 0.0;
			lp[2] = nj > 0.0 ? theta / (1.0 + nj * theta) : theta;
			for (int c = 0; c < k; ++c) lp[3 + c] = sj * r[2 + c];
		}
	}
	GI_LANES_END
	LM_WAVES_END
	// what the prediction pass needs of the panel: M.beta and M.linv are those of the last evaluation
	if (KEEP && P.keep) {
		double *kp = P.keep + g * lm_keep_len(k);
		const int tri = k * (k + 1) / 2;
		LM_WAVES_BEGIN(w, W)
		GI_LANES_BEGIN(lane)
		const int t = w * 64 + lane;
		if (t == 0) {
			kp[0] = theta;
			kp[1] = ev.sigma2;
			P.keep_ok[g] = 1.0;
		}
		for (int c = t; c < k; c += T) kp[2 + c] = M.beta[c];
		for (int e = t; e < tri; e += T) {
			int a, b;
			lm_entry(e, a, b);
			kp[2 + k + e] = M.linv[a * ld + b];
		}
		GI_LANES_END
		LM_WAVES_END
	}
}

// ---- the prediction pass: one row, by one lane ----

// The five values of row i of a fitted panel into out.  KC >= k is the compiled width: `beta` holds k coefficients and `linv` the
// packed L^-1 padded with zeros to KC (KC + 1) / 2 entries (both staged per workgroup), `lp` is the level's prologue record.
template <int KC>
GI_DEV void lm_predict_row(const LmProblem &P, int k, int64_t i, const double *lp, double s2, const double *beta, const double *linv,
                           int interval, double z, double *out) {
	double u[KC];
	GI_UNROLL
	for (int r = 0; r < KC; ++r) u[r] = 0.0;
	double fixed = 0.0;
	bool ok = true;
	GI_UNROLL
	for (int c = 0; c < KC; ++c) {
		if (c < k) {
			const double a = lm_elem(P, k, c, i);
			ok = ok && gi_finite(a);
			fixed += a * beta[c];
			const double cc = a - lp[3 + c];
			GI_UNROLL
			for (int r = c; r < KC; ++r) u[r] += linv[lm_idx(r, c)] * cc;
		}
	}
	double quad = 0.0;
	GI_UNROLL
	for (int r = 0; r < KC; ++r) quad += u[r] * u[r];
	const double se2 = s2 * (quad + lp[2]), yhat = fixed + lp[1];
	double lower = NAN, upper = NAN;
	if (interval != 0) {
		const double half = z * sqrt(interval == 2 ? se2 + s2 : se2);
		lower = yhat - half;
		upper = yhat + half;
	}
	out[0] = ok ? yhat : NAN;
	out[1] = ok ? fixed : NAN;
	out[2] = ok ? sqrt(se2) : NAN;
	out[3] = ok ? lower : NAN;
	out[4] = ok ? upper : NAN;
}

} // namespace lmm
} // namespace anofox
