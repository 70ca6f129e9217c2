// glm_irls.h — the generalised linear model fit of one group of rows: Poisson / log and binomial / logit by penalised
// iteratively reweighted least squares, the loop of the reference's fit_irls (crates/anofox-stats-core/src/models/
// glm_engine/irls.rs) restated.  DESIGN.md §1, "Generalised linear models".
//
//     minimise  deviance(beta) + lambda sum_j beta_j^2   (the intercept not penalised),   eta_i = a_i'beta + offset_i,
//     a_i = (1, x_i) or x_i,   k = p + [intercept] <= 33;   the minimiser solves  X'(y - mu) = lambda beta.
//
// One source for both builds: under hipcc the functions are device code run by ONE WAVEFRONT (64 lanes); under a plain C++
// compiler a wavefront is a loop over 64 lanes (GI_LANES_BEGIN / GI_LANES_END) and a cross-lane reduction is the same
// butterfly over an array of 64 partials, so both builds add every sum in the same order (tests/tools/glm_host.cpp).
//
//   rows       strided over the lanes.  eta and mu of a row sit in a scratch of 2 doubles per row that only the lane that
//              owns the row touches; mu = NaN marks a row that is not valid.  Both are written (first pass) before they are read.
//   start      R's mustart: mu = y + 0.1 (Poisson), (y + 0.5) / 2 (binomial); eta = link(mu); beta = 0.
//   iteration  w = mu (Poisson), mu (1 - mu) (binomial);  z = eta - offset + (y - mu) / w;  solve (X'WX + lambda I') beta = X'Wz;
//              eta, mu and the objective at the new beta;  converged when |obj - obj_old| / (0.1 + |obj|) < tolerance or
//              max|delta beta| < tolerance (tested before step halving and again after it);  from the second iteration on, up
//              to 10 halvings of the step while obj > obj_old + 1e-7 |obj_old| + eps (max(scale, 1) + 8 (n + sum y)),
//              scale = |null deviance|, the last term the rounding of the deviance's own sum (the first iteration's obj_old
//              is the deviance at mustart, which no beta attains: nothing to halve against).
//   warm start P.start = k carried coefficients: the first pass takes eta = a_i'start + offset and mu from it instead of mustart,
//              obj_old of the first iteration is the objective at `start`, and the step may be halved from the first iteration.
//              The minimiser is the problem's, so the start changes the path and not the answer (gi_fit_window).
//   Gram       the augmented matrix [X z]'W[X z], (k + 1)(k + 2) / 2 sums (595 at k = 33), by LANES OVER MATRIX ENTRIES ON A
//              ROW TILE STAGED IN LDS: the 64 lanes stage 64 rows {a_i, z_i, w_i} (each lane its own row), then every lane
//              adds the tile's rows, in row order, into the entries it owns, which stay in registers (ceil(595 / 64) = 10 at
//              most, template parameter EM).  With 64 entries or fewer the lanes split into 64 / T' row slices (T' = the next
//              power of two) whose partial sums meet in a butterfly over the lane bits above T'.  No atomics, a fixed order.
//   solve      Cholesky of the k x k block in LDS with the right-hand side as row k (the forward solve for free), then the back
//              substitution.  A pivot not above 1e-10 of its own diagonal entry marks the column aliased: it is skipped
//              (coefficient NaN in the record, 0 in eta) and the rest are solved without it.  A column constant over the valid
//              rows (|x - x_first| < 1e-10) is dropped the same way when there is an intercept.
//   clamps     Poisson: eta is clamped to [-700, 700] before exp.  Binomial: log mu and log(1 - mu) are floored at log 1e-15,
//              mu and 1 - mu at 1e-15.  Neither is active while |eta| <= 30.
//   finish     weights at the mode -> X'WX + lambda I' -> its Cholesky -> the diagonal of the inverse (lane j solves L v = e_j);
//              deviance, log-likelihood and Pearson chi^2 in one pass; then mu of every row for fit-predict.
//   extras     interval_z > 0 (Poisson): the lane that writes mu of a row also writes the reference's bounds
//              exp(eta -+ interval_z sqrt(dispersion) / max(mu, 0.001)), the lower one floored at 0.  accuracy
//              (binomial): the share of the fitted rows with (mu >= threshold) == y, mu by the prediction pass's own expression
//              (gi_row_mu) so that it equals a count over pred[:, 0]; two integer sums through the butterfly, lane 0 writes.
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GI_DEV __device__ __forceinline__
#define GI_STORE 1 // per-lane variables: one per thread
#define GI_LANES_BEGIN(lane) { const int lane = (int)(threadIdx.x & 63u);
#define GI_LANES_END }
#define GI_AT(lane) 0
#define GI_NOUNROLL _Pragma("unroll 1")
#define GI_UNROLL _Pragma("unroll")
#else
#define GI_NOUNROLL
#define GI_UNROLL
#define GI_DEV inline
#define GI_STORE 64 // per-lane variables: an array over the lanes
#define GI_LANES_BEGIN(lane) for (int lane = 0; lane < 64; ++lane) {
#define GI_LANES_END }
#define GI_AT(lane) (lane)
#endif

namespace anofox {
namespace glm {

constexpr int kGiMaxP = 32;             // features at most (k <= 33)
constexpr int kGiFamilyPoisson = 0;     // log link
constexpr int kGiFamilyBinomial = 1;    // logit link
constexpr double kGiRankTol = 1e-10;    // the reference's rank_tolerance
constexpr double kGiConstTol = 1e-10;   // design.rs: a column within this of its first value is constant
constexpr int kGiMaxHalvings = 10;
constexpr double kGiEtaClamp = 700.0;   // Poisson: exp(eta) stays finite
constexpr double kGiMuFloor = 1e-15;    // binomial: mu and 1 - mu stay above this
constexpr double kGiLogMuFloor = -34.538776394910684; // log(1e-15)

constexpr int kGiStatusInvalidInput = 1;
constexpr int kGiStatusConvergence = 3;
constexpr int kGiStatusInsufficientData = 6;
constexpr int kGiStatusNoValidData = 10;
constexpr int kGiStatusTooFewRows = 100;

#if defined(__HIPCC__)
#define GI_HD __host__ __device__ inline
#else
#define GI_HD inline
#endif
GI_HD int gi_aug_ld(int k) { return (k + 1) | 1; }
GI_HD int gi_tile_ld(int k) { return (k + 2) | 1; }
// doubles of work memory (LDS on the device): the augmented matrix, the row tile, beta / beta_old / diag
GI_HD size_t gi_work_doubles(int k) { return (size_t)(k + 1) * gi_aug_ld(k) + 64 * (size_t)gi_tile_ld(k) + 3 * (size_t)(k + 1); }
// entries of the augmented Gram matrix a lane owns at most
GI_HD int gi_entries_per_lane(int k) { return ((k + 1) * (k + 2) / 2 + 63) / 64; }

struct GiProblem {
	const double *y;
	const double *const *x; // p column pointers
	const double *offset;   // or nullptr
	int p;
	int fit_intercept;
	int family;
	int64_t lo, hi;     // rows [lo, hi) of the columns
	int64_t rule_count; // fit-predict: fewer than 2 -> kGiStatusTooFewRows; < 0: no such rule
	int max_iterations;
	double tolerance;
	double lambda;
	int compute_inference;
	double zq;         // the normal quantile of the confidence level
	double *eta, *mu;  // scratch, one double per row each, indexed by the row number
	// the extras; a caller that does not set them gets none
	double interval_z = 0.0;    // fit-predict, Poisson: > 0 fills pred[3 i + 1], pred[3 i + 2] with the bounds; 0: they stay NaN
	double threshold = 0.5;     // accuracy: a row is classified 1 when mu >= threshold
	double *accuracy = nullptr; // binomial: where the group's training accuracy goes (NaN for a failed group), or nullptr
	// a warm start (gi_fit_window): k carried coefficients in the order of a_i, all finite; nullptr: the cold start at mustart
	const double *start = nullptr;
};

template <class T>
struct GiPL { // a variable every lane has its own copy of
	T v[GI_STORE];
};

// ---- the lanes of the wavefront ----
#if defined(__HIPCC__)
GI_DEV void gi_sync() { __syncthreads(); } // one wavefront per workgroup: orders its LDS traffic
// The value lane (l ^ M) holds, by the butterfly's two instructions: ds_swizzle in its bit-mask mode within a half
// (M <= 16: and 0x1f, or 0, xor M), v_permlane32_swap across the halves (M = 32).
template <int M>
GI_DEV uint32_t gi_xor_lane_u32(uint32_t v) {
	if (M == 32) {
		const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false); // r[0] = the low half's value, r[1] = the high half's
		return (threadIdx.x & 32u) ? (uint32_t)r[0] : (uint32_t)r[1];
	}
	return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, ((M & 0x1f) << 10) | 0x1f);
}
template <int M>
GI_DEV uint64_t gi_xor_lane_u64(uint64_t v) {
	return ((uint64_t)gi_xor_lane_u32<M>((uint32_t)(v >> 32)) << 32) | gi_xor_lane_u32<M>((uint32_t)v);
}
template <int M>
GI_DEV double gi_xor_lane(double v) { return __longlong_as_double((long long)gi_xor_lane_u64<M>((uint64_t)__double_as_longlong(v))); }
template <int M>
GI_DEV int64_t gi_xor_lane(int64_t v) { return (int64_t)gi_xor_lane_u64<M>((uint64_t)v); }
template <int M>
GI_DEV uint32_t gi_xor_lane(uint32_t v) { return gi_xor_lane_u32<M>(v); }
#define GI_STEP(M, T, EXPR)                                                  \
	if (M >= m_lo) {                                                  \
		const T b = gi_xor_lane<M>(a);                                \
		a = (EXPR);                                                   \
	}
#define GI_REDUCE(NAME, T, ST, EXPR)                                  \
	GI_DEV T NAME(GiPL<T> &s, int m_lo = 1) {                         \
		T a = s.v[0];                                                 \
		GI_STEP(32, T, EXPR) GI_STEP(16, T, EXPR) GI_STEP(8, T, EXPR)   \
		GI_STEP(4, T, EXPR) GI_STEP(2, T, EXPR) GI_STEP(1, T, EXPR)      \
		return a;                                                     \
	}
#else
GI_DEV void gi_sync() {}
#define GI_REDUCE(NAME, T, ST, EXPR)                                  \
	GI_DEV T NAME(GiPL<T> &s, int m_lo = 1) {                         \
		T t[64];                                                      \
		for (int m = 32; m >= m_lo; m >>= 1) {                        \
			for (int l = 0; l < 64; ++l) {                            \
				const T a = s.v[l], b = s.v[l ^ m];                   \
				t[l] = (EXPR);                                        \
			}                                                         \
			for (int l = 0; l < 64; ++l) s.v[l] = t[l];               \
		}                                                             \
		return s.v[0];                                                \
	}
#endif
// (a + b is commutative bit for bit, so after every butterfly step the two partners hold the same value; with m_lo > 1 the
// result is the sum over the lanes that differ from the caller's in the bits >= m_lo only: lane 0's on the host)
GI_REDUCE(gi_sum, double, double, a + b)
GI_REDUCE(gi_sum_i, int64_t, long long, a + b)
GI_REDUCE(gi_min_i, int64_t, long long, b < a ? b : a)
GI_REDUCE(gi_or_u, uint32_t, unsigned, a | b)
GI_REDUCE(gi_max, double, double, b > a ? b : a)

GI_DEV bool gi_finite(double v) { return fabs(v) <= DBL_MAX; } // false for NaN

// element c of a_i
GI_DEV double gi_elem(const GiProblem &P, int c, int64_t i) {
	if (P.fit_intercept) return c == 0 ? 1.0 : P.x[c - 1][i];
	return P.x[c][i];
}

GI_DEV bool gi_in_support(int family, double y) { return family == kGiFamilyPoisson ? y >= 0.0 : (y >= 0.0 && y <= 1.0); }

// mu, q = 1 - mu (binomial; 1 for Poisson), log mu and log(1 - mu) from eta, with the clamps; a NaN eta stays NaN
GI_DEV void gi_inverse_link(int family, double eta, double &mu, double &q, double &lmu, double &lq) {
	if (family == kGiFamilyPoisson) {
		const double ec = eta > kGiEtaClamp ? kGiEtaClamp : (eta < -kGiEtaClamp ? -kGiEtaClamp : eta);
		mu = exp(ec);
		q = 1.0;
		lmu = ec;
		lq = 0.0;
		return;
	}
	const double e = exp(-fabs(eta)), d = 1.0 + e, l1 = log1p(e);
	const bool pos = eta >= 0.0;
	double big = 1.0 / d, small = e / d; // (big >= 1/2: only the small one can reach the floor)
	if (small < kGiMuFloor) {
		small = kGiMuFloor;
		big = 1.0 - kGiMuFloor;
	}
	mu = pos ? big : small;
	q = pos ? small : big;
	lmu = pos ? -l1 : eta - l1;
	lq = pos ? -eta - l1 : -l1;
	if (lmu < kGiLogMuFloor) lmu = kGiLogMuFloor;
	if (lq < kGiLogMuFloor) lq = kGiLogMuFloor;
}

// log Gamma(x), x >= 1 (the Poisson term log y!): the argument is shifted up to x >= 10, then Stirling's series to x^-13
// (its first omitted term is below 1e-17 there).  One text for both builds, and far fewer registers than the library's.
GI_DEV double gi_lgamma(double x) {
	double shift = 1.0;
	GI_NOUNROLL
	while (x < 10.0) {
		shift *= x;
		x += 1.0;
	}
	const double r = 1.0 / x, r2 = r * r;
	const double series = r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0 + r2 * (1.0 / 1188.0 +
	                      r2 * (-691.0 / 360360.0 + r2 * (1.0 / 156.0)))))));
	return (x - 0.5) * log(x) - x + 0.91893853320467274178 + series - log(shift);
}

GI_DEV double gi_xlogx(double v) { return v > 0.0 ? v * log(v) : 0.0; }

// the unit deviance from log mu / log(1 - mu)
GI_DEV double gi_unit_deviance(int family, double y, double mu, double lmu, double lq) {
	if (family == kGiFamilyPoisson) return 2.0 * ((y > 0.0 ? y * (log(y) - lmu) : 0.0) - (y - mu));
	return 2.0 * (gi_xlogx(y) + gi_xlogx(1.0 - y) - y * lmu - (1.0 - y) * lq);
}

GI_DEV void gi_fail(double *rec, double *inf, int p, int status) {
	GI_LANES_BEGIN(lane)
	for (int j = lane; j < p + 10; j += 64) rec[j] = NAN;
	if (lane == 0) rec[p + 10] = (double)status;
	if (inf)
		for (int j = lane; j < 5 * p; j += 64) inf[j] = NAN;
	GI_LANES_END
}

GI_DEV void gi_nan_pred(const GiProblem &P, double *pred) {
	if (!pred) return;
	GI_LANES_BEGIN(lane)
	for (int64_t i = P.lo + lane; i < P.hi; i += 64) pred[3 * i] = pred[3 * i + 1] = pred[3 * i + 2] = NAN;
	GI_LANES_END
}

GI_DEV void gi_nan_accuracy(const GiProblem &P) {
	if (!P.accuracy) return;
	GI_LANES_BEGIN(lane)
	if (lane == 0) *P.accuracy = NAN;
	GI_LANES_END
}

// eta (the full linear predictor, the offset included) and mu of row i at beta; a non-finite eta gives mu = NaN
GI_DEV double gi_row_mu(const GiProblem &P, int k, const double *beta, int64_t i, double &eta) {
	eta = P.offset ? P.offset[i] : 0.0;
	GI_NOUNROLL
	for (int c = 0; c < k; ++c) eta += gi_elem(P, c, i) * beta[c];
	double mu = NAN, q, lmu, lq;
	if (gi_finite(eta)) gi_inverse_link(P.family, eta, mu, q, lmu, lq);
	return mu;
}

template <int EM>
struct GiEntries { // the entries (a >= b) of the augmented Gram matrix a lane owns; a < 0: none
	int a[EM], b[EM];
};
template <int EM>
struct GiAcc {
	double v[EM];
};

// The augmented Gram matrix [X z]'W[X z] (lower triangle, row k = the right-hand side) at the scratch's eta / mu into aug, lambda
// on the penalised diagonal.  map: which entries each lane owns; S row slices of Tp lanes (S = 1: every lane sees every row).
template <int EM>
GI_DEV void gi_gram(const GiProblem &P, int k, double *aug, double *tile, GiPL<GiEntries<EM>> &map, int S, int Tp) {
	const int ld = gi_aug_ld(k), tl = gi_tile_ld(k);
	GiPL<GiAcc<EM>> acc;
	GI_LANES_BEGIN(lane)
	(void)lane;
	for (int j = 0; j < EM; ++j) acc.v[GI_AT(lane)].v[j] = 0.0;
	GI_LANES_END
	for (int64_t base = P.lo; base < P.hi; base += 64) {
		const int nr = P.hi - base < 64 ? (int)(P.hi - base) : 64;
		GI_LANES_BEGIN(lane)
		const int64_t i = base + lane;
		double *row = tile + lane * tl;
		double mu = lane < nr ? P.mu[i] : NAN;
		if (mu == mu) {
			const double eta = P.eta[i], y = P.y[i], off = P.offset ? P.offset[i] : 0.0;
			double w = mu;
			if (P.family == kGiFamilyBinomial) {
				double q, lmu, lq;
				gi_inverse_link(P.family, eta, mu, q, lmu, lq);
				w = mu * q;
			}
			GI_NOUNROLL
			for (int c = 0; c < k; ++c) row[c] = gi_elem(P, c, i);
			row[k] = eta - off + (y - mu) / w;
			row[k + 1] = w;
		} else {
			GI_NOUNROLL
			for (int c = 0; c < k + 2; ++c) row[c] = 0.0;
		}
		GI_LANES_END
		gi_sync();
		GI_LANES_BEGIN(lane)
		const GiEntries<EM> &m = map.v[GI_AT(lane)];
		GiAcc<EM> &s = acc.v[GI_AT(lane)];
		for (int r = S > 1 ? lane / Tp : 0; r < nr; r += S) {
			const double *row = tile + r * tl;
			const double w = row[k + 1];
GI_UNROLL
			for (int j = 0; j < EM; ++j) s.v[j] += w * row[m.a[j] < 0 ? 0 : m.a[j]] * row[m.b[j]];
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
			double v = (EM == 1 && S > 1) ? total : acc.v[0].v[j];
#else
			double v = acc.v[lane].v[j];
#endif
			if (a == b && a < k && !(P.fit_intercept && a == 0)) v += P.lambda;
			aug[a * ld + b] = v;
		}
	}
	GI_LANES_END
	gi_sync();
}

// Cholesky of the leading k x k block of aug in place (lower triangle), rows [k, rows) carried along (the right-hand side).
// -> the mask of the columns skipped: those of `dropped` and those whose pivot is not above kGiRankTol of diag0[j].
GI_DEV uint64_t gi_cholesky(double *aug, int ld, int k, int rows, uint64_t dropped, double *diag0) {
	GI_LANES_BEGIN(lane)
	if (lane < k) diag0[lane] = aug[lane * ld + lane];
	GI_LANES_END
	uint64_t alias = dropped;
	for (int j = 0; j < k; ++j) {
		gi_sync();
		const double piv = aug[j * ld + j];
		if (((dropped >> j) & 1) || !(piv > kGiRankTol * diag0[j])) {
			alias |= 1ull << j;
			continue;
		}
		const double l = sqrt(piv);
		GI_LANES_BEGIN(lane)
		const int i = j + 1 + lane;
		if (i < rows) aug[i * ld + j] /= l;
		GI_LANES_END
		gi_sync();
		GI_LANES_BEGIN(lane)
		if (lane == 0) aug[j * ld + j] = l;
		const int i = j + 1 + lane;
		if (i < rows) {
			const double lij = aug[i * ld + j];
			const int ce = i < k ? i : k - 1;
			for (int c = j + 1; c <= ce; ++c) aug[i * ld + c] -= lij * aug[c * ld + j];
		}
		GI_LANES_END
	}
	gi_sync();
	return alias;
}

// beta from the factor and the forward-solved right-hand side in row k (which it overwrites); a skipped column gets 0
GI_DEV void gi_back_substitute(double *aug, int ld, int k, uint64_t alias, double *beta) {
	for (int j = k - 1; j >= 0; --j) {
		gi_sync();
		const bool skip = (alias >> j) & 1;
		const double bj = skip ? 0.0 : aug[k * ld + j] / aug[j * ld + j];
		GI_LANES_BEGIN(lane)
		if (lane == 0) beta[j] = bj;
		if (!skip && lane < j && !((alias >> lane) & 1)) aug[k * ld + lane] -= aug[j * ld + lane] * bj;
		GI_LANES_END
	}
	gi_sync();
}

// eta and mu of the valid rows at beta into the scratch -> the deviance (its sum is non-finite when an eta is)
GI_DEV double gi_update(const GiProblem &P, int k, const double *beta) {
	GiPL<double> part;
	GI_LANES_BEGIN(lane)
	double s = 0.0;
	for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
		if (!(P.mu[i] == P.mu[i])) continue;
		double eta = P.offset ? P.offset[i] : 0.0;
		GI_NOUNROLL
		for (int c = 0; c < k; ++c) eta += gi_elem(P, c, i) * beta[c];
		double mu, q, lmu, lq;
		gi_inverse_link(P.family, eta, mu, q, lmu, lq);
		s += gi_unit_deviance(P.family, P.y[i], mu, lmu, lq);
		P.eta[i] = eta;
		// a NaN mu would unmask the row: keep the row valid, the NaN deviance ends the fit (no convergence)
		P.mu[i] = mu == mu ? mu : 1.0;
	}
	part.v[GI_AT(lane)] = s;
	GI_LANES_END
	return gi_sum(part);
}

GI_DEV double gi_penalty(const GiProblem &P, int k, const double *beta) {
	if (!(P.lambda > 0.0)) return 0.0;
	double s = 0.0;
	for (int c = P.fit_intercept ? 1 : 0; c < k; ++c) s += beta[c] * beta[c];
	return P.lambda * s;
}

// The fit of one group.  rec: p + 11 doubles {b[p], intercept, deviance, null_deviance, pseudo_r_squared, aic, dispersion,
// n_observations, n_params, iterations, converged, status}; inf (optional): 5 p doubles {se[p], z[p], p[p], ci_lower[p],
// ci_upper[p]}; pred (optional): [.. x 3] indexed by the row number, {mu, NaN, NaN} for every row of [lo, hi), or {mu, lower,
// upper} with P.interval_z > 0 (Poisson).
template <int EM>
GI_DEV void gi_fit(const GiProblem &P, bool invalid, double *work, double *rec, double *inf, double *pred) {
	const int p = P.p, k = p + (P.fit_intercept ? 1 : 0), ld = gi_aug_ld(k), tl = gi_tile_ld(k), ic = P.fit_intercept ? 1 : 0;
	double *aug = work, *tile = aug + (size_t)(k + 1) * ld, *beta = tile + 64 * (size_t)tl, *beta_old = beta + (k + 1), *diag0 = beta_old + (k + 1);
	int status = 0;
	if (invalid) status = kGiStatusInvalidInput;
	else if (P.rule_count >= 0 && P.rule_count < 2) status = kGiStatusTooFewRows;
	if (status) {
		gi_fail(rec, inf, p, status);
		gi_nan_pred(P, pred);
		gi_nan_accuracy(P);
		return;
	}
	// ---- first pass: the row mask, the start values, sum y, the first valid row ----
	int64_t n_valid, first;
	double ybar, sum_y;
	{
		GiPL<int64_t> cnt, bad, fst;
		GiPL<double> sy;
		GI_LANES_BEGIN(lane)
		int64_t c = 0, b = 0, f = INT64_MAX;
		double s = 0.0;
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			const double y = P.y[i];
			bool ok = gi_finite(y);
			if (ok && !gi_in_support(P.family, y)) ++b;
			GI_NOUNROLL
			for (int j = 0; ok && j < p; ++j) ok = gi_finite(P.x[j][i]);
			if (ok && P.offset) ok = gi_finite(P.offset[i]);
			if (ok) {
				if (P.start) { // eta and mu at the carried coefficients, as gi_update writes them
					double eta = P.offset ? P.offset[i] : 0.0, mu, q, lmu, lq;
					GI_NOUNROLL
					for (int cc = 0; cc < k; ++cc) eta += gi_elem(P, cc, i) * P.start[cc];
					gi_inverse_link(P.family, eta, mu, q, lmu, lq);
					P.eta[i] = eta;
					P.mu[i] = mu == mu ? mu : 1.0;
				} else {
					const double m0 = P.family == kGiFamilyPoisson ? y + 0.1 : (y + 0.5) / 2.0;
					P.mu[i] = m0;
					P.eta[i] = P.family == kGiFamilyPoisson ? log(m0) : log(m0 / (1.0 - m0));
				}
				++c;
				s += y;
				if (i < f) f = i;
			} else {
				P.mu[i] = NAN;
				P.eta[i] = NAN;
			}
		}
		cnt.v[GI_AT(lane)] = c;
		bad.v[GI_AT(lane)] = b;
		fst.v[GI_AT(lane)] = f;
		sy.v[GI_AT(lane)] = s;
		GI_LANES_END
		n_valid = gi_sum_i(cnt);
		const int64_t n_bad = gi_sum_i(bad);
		first = gi_min_i(fst);
		sum_y = gi_sum(sy);
		ybar = sum_y / (double)(n_valid > 0 ? n_valid : 1);
		if (n_bad > 0) status = kGiStatusInvalidInput;
		else if (n_valid == 0) status = kGiStatusNoValidData;
	}
	// ---- the columns constant over the valid rows (dropped when there is an intercept) ----
	uint64_t dropped = 0;
	if (!status && P.fit_intercept) {
		GiPL<uint32_t> varies;
		GI_LANES_BEGIN(lane)
		uint32_t m = 0;
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			if (!(P.mu[i] == P.mu[i])) continue;
			GI_NOUNROLL
			for (int j = 0; j < p; ++j)
				if (!(fabs(P.x[j][i] - P.x[j][first]) < kGiConstTol)) m |= 1u << j;
		}
		varies.v[GI_AT(lane)] = m;
		GI_LANES_END
		const uint32_t v = gi_or_u(varies);
		for (int j = 0; j < p; ++j)
			if (!((v >> j) & 1)) dropped |= 1ull << (j + 1);
	}
	int k_eff = k;
	for (int c = 0; c < k; ++c) k_eff -= (int)((dropped >> c) & 1);
	if (!status && n_valid < (k_eff > 1 ? k_eff : 1)) status = kGiStatusInsufficientData;
	if (status) {
		gi_fail(rec, inf, p, status);
		gi_nan_pred(P, pred);
		gi_nan_accuracy(P);
		return;
	}
	// ---- the start: objective at mustart (beta = 0) or at the carried coefficients, the null deviance at mu = ybar ----
	double obj, null_dev;
	{
		GiPL<double> d0, dn;
		double nmu, nq, nlmu, nlq;
		if (P.family == kGiFamilyPoisson) {
			nmu = ybar;
			nq = 1.0;
			nlmu = ybar > 0.0 ? log(ybar) : 0.0;
			nlq = 0.0;
		} else {
			// (ybar = 0 or 1: every y sits on that boundary, its unit deviance there is exactly 0 and the logs are not used)
			nmu = ybar;
			nq = 1.0 - ybar;
			nlmu = ybar > 0.0 ? log(ybar) : 0.0;
			nlq = ybar < 1.0 ? log(1.0 - ybar) : 0.0;
		}
		(void)nq;
		GI_LANES_BEGIN(lane)
		double s0 = 0.0, sn = 0.0;
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			if (!(P.mu[i] == P.mu[i])) continue;
			double mu, q, lmu, lq;
			gi_inverse_link(P.family, P.eta[i], mu, q, lmu, lq);
			s0 += gi_unit_deviance(P.family, P.y[i], mu, lmu, lq);
			sn += gi_unit_deviance(P.family, P.y[i], nmu, nlmu, nlq);
		}
		d0.v[GI_AT(lane)] = s0;
		dn.v[GI_AT(lane)] = sn;
		GI_LANES_END
		obj = gi_sum(d0);
		null_dev = gi_sum(dn);
		if (P.start) obj += gi_penalty(P, k, P.start);
	}
	// ---- which entries of the augmented Gram matrix each lane owns ----
	const int T = (k + 1) * (k + 2) / 2;
	int Tp = 64, S = 1;
	if (T <= 64 && EM == 1) {
		Tp = 1;
		while (Tp < T) Tp <<= 1;
		S = 64 / Tp;
	}
	GiPL<GiEntries<EM>> map;
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
	GI_LANES_BEGIN(lane)
	if (lane <= k) beta[lane] = beta_old[lane] = P.start && lane < k ? P.start[lane] : 0.0;
	GI_LANES_END
	gi_sync();
	// ---- the loop ----
	// (a unit deviance is rounded to a few eps (y + mu), mostly exp's ulp: an increase below 8 eps (n + sum y) is not one.  It
	// decides only where the deviance itself is that small: a saturated fit of large counts, whose step it otherwise halves on noise)
	const double scale = fabs(null_dev), floor_ = DBL_EPSILON * ((scale > 1.0 ? scale : 1.0) + 8.0 * ((double)n_valid + sum_y));
	bool converged = false;
	int iterations = 0;
	uint64_t alias = dropped;
	for (int it = 0; it < P.max_iterations && !converged; ++it) {
		iterations = it + 1;
		const double obj_old = obj;
		gi_gram<EM>(P, k, aug, tile, map, S, Tp);
		alias = gi_cholesky(aug, ld, k, k + 1, dropped, diag0);
		GI_LANES_BEGIN(lane)
		if (lane < k) beta_old[lane] = beta[lane];
		GI_LANES_END
		gi_back_substitute(aug, ld, k, alias, beta);
		double max_change = 0.0;
		for (int c = 0; c < k; ++c) {
			const double d = fabs(beta[c] - beta_old[c]);
			if (!(d <= max_change)) max_change = d; // (a NaN sticks)
		}
		obj = gi_update(P, k, beta) + gi_penalty(P, k, beta);
		const bool coef_ok = max_change < P.tolerance;
		if (gi_finite(obj) && (fabs(obj - obj_old) / (0.1 + fabs(obj)) < P.tolerance || coef_ok)) {
			converged = true;
			break;
		}
		// (not on the first iteration: its obj_old is the deviance at mustart, nearly the saturated fit, which no beta attains;
		// every first step is "worse" than it, and ten halvings towards beta = 0 strand a fit with large counts)
		// (a warm start's obj_old is the objective at the carried coefficients, which a beta attains: it halves from the first step)
		if ((it > 0 || P.start) && gi_finite(obj) && gi_finite(obj_old)) {
			int halvings = 0;
			while (obj > obj_old + 1e-7 * fabs(obj_old) + floor_ && halvings < kGiMaxHalvings) {
				++halvings;
				gi_sync();
				GI_LANES_BEGIN(lane)
				if (lane < k) beta[lane] = (beta[lane] + beta_old[lane]) / 2.0;
				GI_LANES_END
				gi_sync();
				obj = gi_update(P, k, beta) + gi_penalty(P, k, beta);
			}
			if (gi_finite(obj) && (fabs(obj - obj_old) / (0.1 + fabs(obj)) < P.tolerance || coef_ok)) converged = true;
		}
	}
	if (!converged) {
		gi_fail(rec, inf, p, kGiStatusConvergence);
		gi_nan_pred(P, pred);
		gi_nan_accuracy(P);
		return;
	}
	// ---- the finish: deviance, log-likelihood, Pearson chi^2 at the mode ----
	double dev, loglik, chi2;
	{
		GiPL<double> sd, sl, sc;
		GI_LANES_BEGIN(lane)
		double d = 0.0, l = 0.0, c2 = 0.0;
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			if (!(P.mu[i] == P.mu[i])) continue;
			double mu, q, lmu, lq;
			const double y = P.y[i];
			gi_inverse_link(P.family, P.eta[i], mu, q, lmu, lq);
			d += gi_unit_deviance(P.family, y, mu, lmu, lq);
			if (P.family == kGiFamilyPoisson) {
				l += y * lmu - mu - gi_lgamma(y + 1.0);
				c2 += (y - mu) * (y - mu) / mu;
			} else {
				l += y * lmu + (1.0 - y) * lq;
			}
		}
		sd.v[GI_AT(lane)] = d;
		sl.v[GI_AT(lane)] = l;
		sc.v[GI_AT(lane)] = c2;
		GI_LANES_END
		dev = gi_sum(sd);
		loglik = gi_sum(sl);
		chi2 = gi_sum(sc);
	}
	int n_params = k;
	for (int c = 0; c < k; ++c) n_params -= (int)((alias >> c) & 1);
	double dispersion = 1.0;
	if (P.family == kGiFamilyPoisson && n_valid > n_params) {
		dispersion = chi2 / (double)(n_valid - n_params);
		if (!(dispersion > 1.0)) dispersion = 1.0;
	}
	// ---- inference: the diagonal of (X'WX + lambda I')^-1 with the weights at the mode ----
	if (inf) {
		uint64_t ialias = alias;
		if (P.compute_inference) {
			gi_gram<EM>(P, k, aug, tile, map, S, Tp);
			ialias = alias | gi_cholesky(aug, ld, k, k, dropped, diag0);
		}
		GI_LANES_BEGIN(lane)
		const int j = lane + ic; // lane f: feature f
		if (lane < p) {
			double se = NAN;
			if (P.compute_inference && !((ialias >> j) & 1)) {
				double *v = tile + lane * tl, ss = 0.0;
				for (int i = j; i < k; ++i) {
					if ((ialias >> i) & 1) { v[i] = 0.0; continue; }
					double acc = i == j ? 1.0 : 0.0;
					for (int c = j; c < i; ++c)
						if (!((ialias >> c) & 1)) acc -= aug[i * ld + c] * v[c];
					v[i] = acc / aug[i * ld + i];
					ss += v[i] * v[i];
				}
				se = sqrt(dispersion * ss);
			}
			const double b = beta[j], z = b / se;
			inf[lane] = se;
			inf[p + lane] = z;
			inf[2 * p + lane] = erfc(fabs(z) * 0.70710678118654752440);
			inf[3 * p + lane] = b - P.zq * se;
			inf[4 * p + lane] = b + P.zq * se;
		}
		GI_LANES_END
		gi_sync();
	}
	// ---- the record ----
	GI_LANES_BEGIN(lane)
	if (lane < p) rec[lane] = ((alias >> (lane + ic)) & 1) ? NAN : beta[lane + ic];
	if (lane == 0) {
		rec[p] = P.fit_intercept ? ((alias & 1) ? NAN : beta[0]) : NAN;
		rec[p + 1] = dev;
		rec[p + 2] = null_dev;
		rec[p + 3] = null_dev > 0.0 ? 1.0 - dev / null_dev : 0.0;
		rec[p + 4] = -2.0 * loglik + 2.0 * (double)n_params;
		rec[p + 5] = dispersion;
		rec[p + 6] = (double)n_valid;
		rec[p + 7] = (double)n_params;
		rec[p + 8] = (double)iterations;
		rec[p + 9] = 1.0;
		rec[p + 10] = 0.0;
	}
	GI_LANES_END
	// ---- fit-predict: mu of every row of the group ----
	if (pred) {
		const bool interval = P.interval_z > 0.0 && P.family == kGiFamilyPoisson;
		const double zs = interval ? P.interval_z * sqrt(dispersion) : 0.0;
		GI_LANES_BEGIN(lane)
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			double eta;
			const double mu = gi_row_mu(P, k, beta, i, eta);
			double lower = NAN, upper = NAN;
			if (interval && gi_finite(mu)) { // the reference's bounds, kept as they stand
				const double h = zs / (mu > 0.001 ? mu : 0.001);
				lower = exp(eta - h);
				upper = exp(eta + h);
				if (!(lower > 0.0)) lower = 0.0;
			}
			pred[3 * i] = mu;
			pred[3 * i + 1] = lower;
			pred[3 * i + 2] = upper;
		}
		GI_LANES_END
	}
	// ---- the training accuracy at the threshold: over the rows the fit used, mu as the prediction pass computes it ----
	if (P.accuracy) {
		GiPL<int64_t> hit, cnt;
		GI_LANES_BEGIN(lane)
		int64_t h = 0, c = 0;
		for (int64_t i = P.lo + lane; i < P.hi; i += 64) {
			if (!(P.mu[i] == P.mu[i])) continue;
			double eta;
			const double mu = gi_row_mu(P, k, beta, i, eta);
			if (!(mu == mu)) continue;
			++c;
			h += ((mu >= P.threshold ? 1.0 : 0.0) == P.y[i]) ? 1 : 0;
		}
		hit.v[GI_AT(lane)] = h;
		cnt.v[GI_AT(lane)] = c;
		GI_LANES_END
		// a group that reaches this point converged on at least max(k, 1) >= 1 valid rows, so fitted >= 1; the guard only keeps a 0 / 0
		// out of the division should a row's recomputed mu ever be NaN where the scratch mu was not
		const int64_t hits = gi_sum_i(hit), fitted = gi_sum_i(cnt);
		GI_LANES_BEGIN(lane)
		if (lane == 0) *P.accuracy = (double)hits / (double)(fitted > 0 ? fitted : 1);
		GI_LANES_END
	}
	gi_sync();
}

// the template parameter a fit of k parameters needs: 1 (k <= 9), 4 (k <= 21) or 10
GI_HD int gi_entry_class(int k) {
	const int e = gi_entries_per_lane(k);
	return e <= 1 ? 1 : (e <= 4 ? 4 : 10);
}

// ---- the window walk: one wavefront fits the frames of a run of consecutive output rows, one after the other ----
// doubles of work memory of a walk: gi_fit's, then the frame's record (p + 11) and the carried coefficients (k + 1)
GI_HD size_t gi_window_work_doubles(int p, int k) { return gi_work_doubles(k) + (size_t)(p + 11) + (size_t)(k + 1); }

// the largest |eta| of a fit whose coefficients are carried, and of a warm-started fit that is kept: beyond it the clamps of
// gi_inverse_link come into play, the objective is flat, and a start there can "converge" where it stands
constexpr double kGiWarmEtaMax = 30.0;

// max |eta| over the valid rows of the scratch (after a fit that converged: every one of them is finite)
GI_DEV double gi_max_abs_eta(const GiProblem &P) {
	GiPL<double> part;
	GI_LANES_BEGIN(lane)
	double m = 0.0;
	for (int64_t i = P.lo + lane; i < P.hi; i += 64)
		if (P.mu[i] == P.mu[i] && !(fabs(P.eta[i]) <= m)) m = fabs(P.eta[i]);
	part.v[GI_AT(lane)] = m;
	GI_LANES_END
	return gi_max(part);
}

constexpr int kGiStartCold = 0, kGiStartWarm = 1, kGiStartRefit = 2; // how a frame was started (gi_fit_window's `started`)

// The frames [flo[e], fhi[e]) of the output rows e = e0 .. e1 - 1 (fhi <= flo: an empty frame).  P: the columns, the options
// and a slab of 2 x slab_rows doubles in P.eta (eta of the frame's row i sits in slot i - lo, mu slab_rows further on; only
// the current frame's are live, every fit writes them before it reads them).  Per output row: pred[3 e] = {mu, lower, upper}
// at the frame's last row (the bounds as gi_fit's, with P.interval_z), and, with `records`, the frame's record.
//   cold   a frame is fitted by gi_fit from mustart when `warm` is off, when it is the first of the run, when the previous
//          frame failed, was empty, left a NaN (dropped or aliased) coefficient or an |eta| above kGiWarmEtaMax (a fit near
//          separation), when a bound is below the previous frame's, or when it does not overlap the previous frame;
//   warm   every other frame starts from the previous frame's coefficients (P.start);
//   refit  a warm-started frame that ends without convergence, with a NaN coefficient or with an |eta| above kGiWarmEtaMax is
//          fitted again cold: a record with a failure, a skipped column or a saturated row is always the cold fit's, so a warm
//          start never makes a NULL of its own, and never stops in the flat part of the objective where it began.
// counts (lane 0's, added to): {frames started cold, started warm, warm frames refitted cold, IRLS iterations (a fit that
// did not converge counts max_iterations)}.  started (optional): per output row one of kGiStart*.
template <int EM>
GI_DEV void gi_fit_window(GiProblem P, bool invalid, bool warm, const int64_t *flo, const int64_t *fhi, int64_t e0, int64_t e1,
                          int64_t slab_rows, double *work, double *pred, double *records, int64_t *counts, int32_t *started) {
	const int p = P.p, k = p + (P.fit_intercept ? 1 : 0), ic = P.fit_intercept ? 1 : 0;
	const double *beta = work + (size_t)(k + 1) * gi_aug_ld(k) + 64 * (size_t)gi_tile_ld(k); // where gi_fit leaves its coefficients
	double *rec = work + gi_work_doubles(k), *carry = rec + (p + 11);
	double *slab = P.eta;
	bool have = false; // carry holds the coefficients of the frame [plo, phi), all of them finite
	int64_t plo = 0, phi = 0, n_cold = 0, n_warm = 0, n_refit = 0, n_iter = 0;
	for (int64_t e = e0; e < e1; ++e) {
		int64_t lo = flo[e], hi = fhi[e];
		if (hi <= lo) lo = hi = 0; // an empty frame, whatever its bounds are
		const bool fits = hi - lo <= slab_rows; // (the planner sizes the slab by the longest frame: always true)
		const bool use = warm && have && fits && hi > lo && lo >= plo && hi >= phi && lo < phi;
		GiPL<int64_t> rule;
		GI_LANES_BEGIN(lane)
		int64_t c = 0;
		for (int64_t i = lo + lane; i < hi; i += 64) c += P.y[i] == P.y[i] ? 1 : 0;
		rule.v[GI_AT(lane)] = c;
		GI_LANES_END
		P.lo = lo;
		P.hi = hi;
		P.rule_count = gi_sum_i(rule);
		P.eta = slab - lo;
		P.mu = slab + slab_rows - lo;
		P.start = use ? carry : nullptr;
		int kind = use ? kGiStartWarm : kGiStartCold;
		gi_fit<EM>(P, invalid || !fits, work, rec, nullptr, nullptr);
		gi_sync(); // (a failed fit returns right after it has written the record)
		bool nan_coef = false;
		for (int j = 0; j < p + ic; ++j) nan_coef = nan_coef || !(rec[j] == rec[j]);
		int status = (int)rec[p + 10];
		double eta_max = status == 0 ? gi_max_abs_eta(P) : 0.0;
		if (use) {
			n_iter += status == 0 ? (int64_t)rec[p + 8] : (status == kGiStatusConvergence ? P.max_iterations : 0);
			if (status == kGiStatusConvergence || (status == 0 && (nan_coef || !(eta_max <= kGiWarmEtaMax)))) {
				kind = kGiStartRefit;
				P.start = nullptr;
				gi_sync();
				gi_fit<EM>(P, invalid, work, rec, nullptr, nullptr);
				gi_sync();
				nan_coef = false;
				for (int j = 0; j < p + ic; ++j) nan_coef = nan_coef || !(rec[j] == rec[j]);
				status = (int)rec[p + 10];
				eta_max = status == 0 ? gi_max_abs_eta(P) : 0.0;
			}
		}
		if (kind != kGiStartWarm) n_iter += status == 0 ? (int64_t)rec[p + 8] : (status == kGiStatusConvergence ? P.max_iterations : 0);
		n_cold += kind == kGiStartCold;
		n_warm += kind != kGiStartCold;
		n_refit += kind == kGiStartRefit;
		have = status == 0 && !nan_coef && eta_max <= kGiWarmEtaMax;
		plo = lo;
		phi = hi;
		GI_LANES_BEGIN(lane)
		if (have && lane < k) carry[lane] = beta[lane];
		if (records)
			for (int j = lane; j < p + 11; j += 64) records[e * (int64_t)(p + 11) + j] = rec[j];
		if (lane == 0) {
			double mu = NAN, lower = NAN, upper = NAN;
			if (status == 0) {
				double eta;
				mu = gi_row_mu(P, k, beta, hi - 1, eta);
				if (P.interval_z > 0.0 && P.family == kGiFamilyPoisson && gi_finite(mu)) { // gi_fit's bounds
					const double h = P.interval_z * sqrt(rec[p + 5]) / (mu > 0.001 ? mu : 0.001);
					lower = exp(eta - h);
					upper = exp(eta + h);
					if (!(lower > 0.0)) lower = 0.0;
				}
			}
			pred[3 * e] = mu;
			pred[3 * e + 1] = lower;
			pred[3 * e + 2] = upper;
			if (started) started[e] = kind;
		}
		GI_LANES_END
		gi_sync(); // the next frame's fit overwrites the record and the coefficients
	}
	GI_LANES_BEGIN(lane)
	if (lane == 0) {
		counts[0] += n_cold;
		counts[1] += n_warm;
		counts[2] += n_refit;
		counts[3] += n_iter;
	}
	GI_LANES_END
}

} // namespace glm
} // namespace anofox
