// quantile_solve.h — the quantile regression fit of one group of rows: the exact vertex of the linear program
//     minimise  sum_i rho_tau(y_i - a_i'beta),   rho_tau(r) = r (tau - [r < 0]),   a_i = (1, x_i) or x_i,  k = p + [intercept]
// by the Barrodale-Roberts / Koenker-d'Orey simplex over the rows.  DESIGN.md §1, "Quantile regression".
//
// One source for both builds: under hipcc the functions are device code run by ONE WAVEFRONT (64 lanes, rows strided over
// the lanes, one lane per basis direction, the small matrices in LDS); under a plain C++ compiler the same text runs with
// one "lane" (tests/tools/quantile_solve_host.cpp), which is where the algorithm is debugged.
//
// Basis: k elements, element j either a row whose residual is held at zero or the artificial "beta_j = 0".  It starts
// with all k artificials (B^-1 = I, beta = 0).  Column j of B^-1 is the edge d_j: moving along it changes only element j.
//   optimality  s = sum over the non-basis rows with r != 0 of psi(r_i) a_i (psi = tau for r > 0, tau - 1 for r < 0),
//               u = B^-T s.  The one-sided derivatives along +d_j / -d_j are
//                   g+_j = -u_j + (1 - tau) [row]  + sum over non-basis rows with r = 0 of (z > 0 ? (1 - tau) z : tau |z|)
//                   g-_j = +u_j + tau [row]        + sum over non-basis rows with r = 0 of (z > 0 ? tau z : (1 - tau) |z|)
//               (z = a_i'd_j), i.e. a row element needs -tau <= u_j <= 1 - tau, an artificial u_j = 0.  An edge is violated
//               when g < -kQsDualTol * sum_c (sum_i |a_ic|) |d_jc| (the size u_j could have).
//   pivot       leave along the most violated edge (the lowest violated one once a step has stalled: Bland); z_i = a_i'd;
//               breakpoints t_i = r_i / z_i > 0 with weights |z_i|; the entering row is the weighted quantile where the
//               derivative turns non-negative: the smallest t with sum_{t_i <= t} |z_i| >= -g, found by bisection over the
//               bit pattern of the positive double t (one reduction per bit), ties to the lowest row.  B^-1 by the rank-one
//               formula, r_i -= t z_i, the entering row's residual exactly 0; |r| <= kQsSnapTol max|y| is snapped to 0.
//   finish      when no edge is violated: B is rebuilt from the basis rows, factorised by LU with partial pivoting, beta and a
//               fresh B^-1 come from that factorisation, the residuals from the rows, and the optimality test runs again;
//               if it fails the pivots go on (at most kQsMaxRestarts times).
//   degeneracy  when no edge descends but rows sit on their kink off the basis, the vertex is degenerate and another basis of it
//               may still have a descending edge.  Each such row carries a side (the sign of its zero: the multiplier bound it
//               is counted at); with the sides fixed the test is the plain simplex one, u within its bounds.  No violation: the
//               multipliers are a certificate, the vertex is optimal.  Else a pivot of length zero: the most violated element
//               leaves; the kink rows the move would push across their side block it at t = 0, in index order those whose
//               weights |z_i| stay below -g change side and the next one enters (the line search's rule at t = 0); the leaving
//               row takes the side it leaves towards; the test above runs on the new basis.  After kQsBlandAfter such pivots
//               at one tau: Bland's rule (the violated element and the first blocking row of lowest index, no side changes),
//               which cannot cycle; at most kQsMaxExchanges in all.
//   tau path    a vertex is feasible for every tau (only the optimality test and the line search read it): qs_fit_path begins once
//               and pivots from the vertex each tau's finish rebuilt to the optimum of the next (qs_fit = begin, pivot, record).
//   window      a vertex also stays feasible when rows join or leave the data set as long as its k basis rows remain: qs_fit_window
//               walks consecutive frames of a partition and pivots from each frame's optimum to the next's.
// Pivots are bounded by min(max_iterations, qs_iteration_ceiling(k)); when the bound stops a fit the last vertex is
// returned (status 0) and the pivot count is reported negated.  No atomics, a fixed order of every sum: two calls give the
// same bytes.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QS_DEV __device__ inline
#define QS_LANES 64
#else
#define QS_DEV inline
#define QS_LANES 1
#endif

namespace anofox {
namespace quantile {

constexpr int kQsMaxP = 32;           // features at most (k <= 33)
constexpr double kQsDualTol = 1e-10;  // a derivative below this share of its scale counts as zero
constexpr double kQsPivotTol = 1e-11; // |z_i| below this share of sum_c max_i|a_ic| |d_c| is no breakpoint
constexpr double kQsSnapTol = 1e-12;  // |r_i| <= this share of max|y| is a zero residual
constexpr double kQsStallTol = 1e-14; // a step that lowers the loss by less than this share of max|y|: Bland's rule from here on
constexpr int kQsMaxRestarts = 3;     // failed optimality tests after a refactorisation that may resume the pivots
#ifndef QS_MAX_EXCHANGES // (a test builds the host program with 256 to show that a fit needs the pivots under Bland's rule)
#define QS_MAX_EXCHANGES 1024
#endif
constexpr int kQsMaxExchanges = QS_MAX_EXCHANGES; // zero-length pivots at degenerate vertices, per tau (then the count is reported negated)
constexpr int kQsBlandAfter = 256;    // of them before Bland's rule takes over

constexpr int kQsStatusInvalidInput = 1;
constexpr int kQsStatusInsufficientData = 6;
constexpr int kQsStatusNoValidData = 10;
constexpr int kQsStatusTooFewRows = 100;

#if defined(__HIPCC__)
__host__ __device__
#endif
inline int qs_iteration_ceiling(int k) { return 1000 + 50 * k; }

// doubles of work memory (LDS on the device) for k basis elements
#if defined(__HIPCC__)
__host__ __device__
#endif
inline size_t qs_work_doubles(int k) { return 2 * (size_t)k * (size_t)(k | 1) + 12 * (size_t)k; }

struct QsProblem {
	const double *y;
	const double *const *x; // p column pointers
	int p;
	int fit_intercept;
	int64_t lo, hi;     // rows [lo, hi) of the columns
	int64_t rule_count; // what the "fewer than 2 rows" rule looks at
	double tau;
	int max_iterations;
	int predict_layout; // 0: {b, intercept, tau, loss, n_basis_rows, n, status}; 1: {b, intercept, NaN, NaN, NaN, n, status}
	double *r, *z, *t;  // scratch, one double per row each: row i sits in slot i - origin
	int64_t origin = 0; // 0: indexed by the row number (the fit and the tau path); the window walk keeps a slab of its own
};

// ---- the lanes of the wavefront (one lane in the host build) ----
#if defined(__HIPCC__)
QS_DEV int qs_lane() { return (int)(threadIdx.x & 63u); }
QS_DEV void qs_sync() { __syncthreads(); } // one wavefront per workgroup: orders its LDS traffic
QS_DEV double qs_sum(double v) {
	for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
	return v;
}
QS_DEV double qs_max(double v) {
	for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
	return v;
}
QS_DEV int64_t qs_sum_i(int64_t v) {
	for (int m = 32; m >= 1; m >>= 1) v += (int64_t)__shfl_xor((long long)v, m, 64);
	return v;
}
QS_DEV int64_t qs_min_i(int64_t v) {
	for (int m = 32; m >= 1; m >>= 1) {
		const int64_t o = (int64_t)__shfl_xor((long long)v, m, 64);
		v = o < v ? o : v;
	}
	return v;
}
QS_DEV uint64_t qs_min_u(uint64_t v) {
	for (int m = 32; m >= 1; m >>= 1) {
		const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, m, 64);
		v = o < v ? o : v;
	}
	return v;
}
QS_DEV uint64_t qs_max_u(uint64_t v) {
	for (int m = 32; m >= 1; m >>= 1) {
		const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, m, 64);
		v = o > v ? o : v;
	}
	return v;
}
// the largest v and its index, the lowest index on ties; j < 0 = no candidate on this lane
QS_DEV void qs_argmax(double &v, int &j) {
	for (int m = 32; m >= 1; m >>= 1) {
		const double ov = __shfl_xor(v, m, 64);
		const int oj = __shfl_xor(j, m, 64);
		if (oj >= 0 && (j < 0 || ov > v || (ov == v && oj < j))) { v = ov; j = oj; }
	}
}
QS_DEV uint64_t qs_ballot(bool b) { return (uint64_t)__ballot(b); }
#else
QS_DEV int qs_lane() { return 0; }
QS_DEV void qs_sync() {}
QS_DEV double qs_sum(double v) { return v; }
QS_DEV double qs_max(double v) { return v; }
QS_DEV int64_t qs_sum_i(int64_t v) { return v; }
QS_DEV int64_t qs_min_i(int64_t v) { return v; }
QS_DEV uint64_t qs_min_u(uint64_t v) { return v; }
QS_DEV uint64_t qs_max_u(uint64_t v) { return v; }
QS_DEV void qs_argmax(double &, int &) {}
QS_DEV uint64_t qs_ballot(bool b) { return b ? 1ull : 0ull; }
#endif

QS_DEV uint64_t qs_bits(double v) {
	uint64_t b;
	memcpy(&b, &v, sizeof b);
	return b;
}
QS_DEV double qs_from_bits(uint64_t b) {
	double v;
	memcpy(&v, &b, sizeof v);
	return v;
}

// element c of a_i
QS_DEV double qs_elem(const QsProblem &P, int c, int64_t i) {
	if (P.fit_intercept) return c == 0 ? 1.0 : P.x[c - 1][i];
	return P.x[c][i];
}

QS_DEV bool qs_in_basis(const int64_t *basis, int k, int64_t i) {
	for (int j = 0; j < k; ++j)
		if (basis[j] == i) return true;
	return false;
}

QS_DEV void qs_fail_record(double *rec, int p, int status, int32_t *iterations) {
	if (qs_lane() != 0) return;
	for (int j = 0; j < p + 5; ++j) rec[j] = NAN;
	rec[p + 5] = (double)status;
	if (iterations) *iterations = 0;
}

// B from the basis, P B = L U with partial pivoting, beta = B^-1 v and a fresh B^-1 from the factors, the residuals of all
// rows from beta.  false: B is singular to working precision (a zero pivot).
QS_DEV bool qs_refactor(const QsProblem &P, int k, int ld, double *M, double *Binv, double *beta, double *v, const int64_t *basis,
                        int64_t *perm, double snap) {
	const int lane = qs_lane();
	for (int r = lane; r < k; r += QS_LANES) {
		const int64_t b = basis[r];
		for (int c = 0; c < k; ++c) M[r * ld + c] = b >= 0 ? qs_elem(P, c, b) : (c == r ? 1.0 : 0.0);
		v[r] = b >= 0 ? P.y[b] : 0.0;
		perm[r] = r;
	}
	qs_sync();
	for (int c = 0; c < k; ++c) {
		double best = -1.0;
		int br = -1;
		for (int r = c + lane; r < k; r += QS_LANES) {
			const double a = fabs(M[r * ld + c]);
			if (a > best) { best = a; br = r; }
		}
		qs_argmax(best, br);
		if (br < 0 || !(best > 0.0)) return false; // (the same on every lane)
		qs_sync();
		if (br != c) {
			for (int cc = lane; cc < k; cc += QS_LANES) {
				const double tmp = M[c * ld + cc];
				M[c * ld + cc] = M[br * ld + cc];
				M[br * ld + cc] = tmp;
			}
			if (lane == 0) {
				const double tv = v[c];
				v[c] = v[br];
				v[br] = tv;
				const int64_t tp = perm[c];
				perm[c] = perm[br];
				perm[br] = tp;
			}
		}
		qs_sync();
		const double piv = M[c * ld + c];
		for (int r = c + 1 + lane; r < k; r += QS_LANES) {
			const double f = M[r * ld + c] / piv;
			M[r * ld + c] = f;
			for (int cc = c + 1; cc < k; ++cc) M[r * ld + cc] -= f * M[c * ld + cc];
		}
		qs_sync();
	}
	// lane j solves for column j of B^-1 (right-hand side P e_j); j == k: beta (right-hand side P v)
	for (int j = lane; j <= k; j += QS_LANES) {
		double *out = j < k ? Binv + j * ld : beta;
		for (int r = 0; r < k; ++r) {
			double acc = j < k ? (perm[r] == j ? 1.0 : 0.0) : v[r];
			for (int c = 0; c < r; ++c) acc -= M[r * ld + c] * out[c];
			out[r] = acc;
		}
		for (int r = k - 1; r >= 0; --r) {
			double acc = out[r];
			for (int c = r + 1; c < k; ++c) acc -= M[r * ld + c] * out[c];
			out[r] = acc / M[r * ld + r];
		}
	}
	qs_sync();
	for (int j = lane; j < k; j += QS_LANES)
		if (basis[j] < 0) beta[j] = 0.0; // an artificial pins its coefficient: exactly 0
	qs_sync();
	for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
		if (!(P.r[i - P.origin] == P.r[i - P.origin])) continue; // masked at the first pass
		double fit = 0.0;
		for (int c = 0; c < k; ++c) fit += qs_elem(P, c, i) * beta[c];
		const double old = P.r[i - P.origin];
		double rr = P.y[i] - fit;
		if (fabs(rr) <= snap || qs_in_basis(basis, k, i)) rr = old == 0.0 ? old : copysign(0.0, rr); // a kink row keeps its side
		P.r[i - P.origin] = rr;
	}
	return true;
}

// B^-1 when row `enter` takes the place of element bj (the rank-one formula), and the basis entry.
QS_DEV void qs_replace(const QsProblem &P, int k, int ld, double *Binv, double *wrow, int64_t *basis, int bj, int64_t enter) {
	const int lane = qs_lane();
	for (int l = lane; l < k; l += QS_LANES) {
		double acc = 0.0;
		for (int c = 0; c < k; ++c) acc += qs_elem(P, c, enter) * Binv[l * ld + c];
		wrow[l] = acc;
	}
	qs_sync();
	const double wj = wrow[bj];
	qs_sync();
	for (int c = lane; c < k; c += QS_LANES) Binv[bj * ld + c] /= wj;
	qs_sync();
	for (int l = lane; l < k; l += QS_LANES) {
		if (l == bj) continue;
		const double wl = wrow[l];
		for (int c = 0; c < k; ++c) Binv[l * ld + c] -= wl * Binv[bj * ld + c];
	}
	if (lane == 0) basis[bj] = enter;
	qs_sync();
}

// What begin leaves for the pivots and the record of every tau of the group: the sizes, the scales and the slices of `work`.
struct QsState {
	int k, ld, max_it;
	int64_t n_valid;
	double ymax, snap;
	double *Binv, *M, *s, *dvec, *beta, *v, *amax, *asum, *wrow, *gp, *gm, *thr;
	int64_t *basis, *perm;
};

// The column sizes max_i |a_ic| and sum_i |a_ic| over the valid rows of [P.lo, P.hi) (the rows whose r is not NaN): the scales
// of the thresholds.  Begin computes them once per group, the window walk once per frame.
QS_DEV void qs_column_sizes(const QsProblem &P, int k, double *amax, double *asum) {
	const int lane = qs_lane();
	for (int c = 0; c < k; ++c) {
		double mx = 0.0, sm = 0.0;
		for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
			if (!(P.r[i - P.origin] == P.r[i - P.origin])) continue;
			const double a = fabs(qs_elem(P, c, i));
			mx = fmax(mx, a);
			sm += a;
		}
		mx = qs_max(mx);
		sm = qs_sum(sm);
		if (lane == 0) { amax[c] = mx; asum[c] = sm; }
	}
}

// Begin: the row rules, the first pass, the column sizes and the all-artificial basis (B^-1 = I, beta = 0, r = y).  Nothing
// here reads tau.  -> 0, or the status that fails the group (100, 10, 6) at every tau.
QS_DEV int qs_begin(const QsProblem &P, double *work, QsState &S) {
	const int lane = qs_lane();
	const int p = P.p, k = p + (P.fit_intercept ? 1 : 0), ld = k | 1;
	if (P.rule_count < 2) return kQsStatusTooFewRows;
	// ---- first pass: the row mask, r = y (beta = 0), max|y| ----
	int64_t n_valid = 0;
	double ymax = 0.0;
	for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
		const double yv = P.y[i];
		bool ok = isfinite(yv);
		for (int j = 0; j < p; ++j) ok = ok && isfinite(P.x[j][i]);
		P.r[i - P.origin] = ok ? yv : NAN;
		P.z[i - P.origin] = 0.0;      // a masked row is never a breakpoint: the line search reads these slots of EVERY row, and the
		P.t[i - P.origin] = INFINITY; // scratch arrives with whatever an earlier call left in it
		if (ok) {
			++n_valid;
			ymax = fmax(ymax, fabs(yv));
		}
	}
	n_valid = qs_sum_i(n_valid);
	ymax = qs_max(ymax);
	if (n_valid == 0) return kQsStatusNoValidData;
	if (n_valid < k) return kQsStatusInsufficientData;
	const double snap = kQsSnapTol * ymax;

	double *Binv = work, *M = Binv + (size_t)k * ld;
	double *s = M + (size_t)k * ld, *dvec = s + k, *beta = dvec + k, *v = beta + k, *amax = v + k, *asum = amax + k;
	double *wrow = asum + k, *gp = wrow + k, *gm = gp + k, *thr = gm + k;
	int64_t *basis = reinterpret_cast<int64_t *>(thr + k), *perm = basis + k;

	qs_column_sizes(P, k, amax, asum);
	for (int j = lane; j < k; j += QS_LANES) {
		for (int c = 0; c < k; ++c) Binv[j * ld + c] = c == j ? 1.0 : 0.0;
		basis[j] = -1 - (int64_t)j;
		beta[j] = 0.0;
	}
	qs_sync();
	// rows that are zero from the start (y_i = 0) are snapped like every later residual
	for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES)
		if (fabs(P.r[i - P.origin]) <= snap) P.r[i - P.origin] = 0.0;

	const int ceiling = qs_iteration_ceiling(k);
	S.k = k;
	S.ld = ld;
	S.max_it = P.max_iterations < ceiling ? P.max_iterations : ceiling;
	S.n_valid = n_valid;
	S.ymax = ymax;
	S.snap = snap;
	S.Binv = Binv; S.M = M; S.s = s; S.dvec = dvec; S.beta = beta; S.v = v; S.amax = amax; S.asum = asum;
	S.wrow = wrow; S.gp = gp; S.gm = gm; S.thr = thr;
	S.basis = basis; S.perm = perm;
	return 0;
}

// Pivot to the optimum of one tau from the vertex the state holds (begin's, or the one an earlier tau's finish rebuilt: a
// vertex is feasible for every tau), through the finish and the re-test.  The pivot budget, the restarts, Bland's rule and
// the rested edges start afresh.  -> false: the finish met a singular basis; else beta, B^-1 and r are those of the
// refactorised last basis.  *pivots: the count; *converged: the optimality test passed after a finish.
QS_DEV bool qs_pivot_to_optimum(const QsProblem &P, const QsState &S, const double tau, int *pivots_out, bool *converged_out) {
	const int lane = qs_lane();
	const int k = S.k, ld = S.ld, max_it = S.max_it;
	const double ymax = S.ymax, snap = S.snap;
	double *Binv = S.Binv, *M = S.M, *s = S.s, *dvec = S.dvec, *beta = S.beta, *v = S.v, *amax = S.amax, *asum = S.asum;
	double *wrow = S.wrow, *gp = S.gp, *gm = S.gm, *thr = S.thr;
	int64_t *basis = S.basis, *perm = S.perm;
	int pivots = 0, restarts = 0;
	bool fresh = false, converged = false, bland = false, singular = false;
	uint64_t blocked = 0; // edges whose line search found no breakpoint since the last pivot
	int zero_pivots = 0;  // pivots of length zero at degenerate vertices (not part of the pivot count)

	for (;;) {
		// ---- s over the non-basis rows off their kink (basis rows have r = 0) ----
		for (int c = 0; c < k; ++c) {
			double acc = 0.0;
			for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
				const double ri = P.r[i - P.origin];
				if (ri > 0.0) acc += tau * qs_elem(P, c, i);
				else if (ri < 0.0) acc += (tau - 1.0) * qs_elem(P, c, i);
			}
			acc = qs_sum(acc);
			if (lane == 0) s[c] = acc;
		}
		qs_sync();
		// ---- the one-sided derivatives of every edge ----
		for (int j = lane; j < k; j += QS_LANES) {
			double u = 0.0, sc = 0.0;
			for (int c = 0; c < k; ++c) {
				const double d = Binv[j * ld + c];
				u += s[c] * d;
				sc += asum[c] * fabs(d);
			}
			const bool row = basis[j] >= 0;
			gp[j] = -u + (row ? 1.0 - tau : 0.0);
			gm[j] = u + (row ? tau : 0.0);
			thr[j] = kQsDualTol * sc;
		}
		for (int64_t c0 = P.lo; c0 < P.hi; c0 += QS_LANES) { // non-basis rows on their kink: each side pays its own slope
			const int64_t i = c0 + lane;
			uint64_t m = qs_ballot(i < P.hi && P.r[i - P.origin] == 0.0 && !qs_in_basis(basis, k, i));
			while (m) {
				const int bit = __builtin_ctzll(m);
				m &= m - 1;
				const int64_t ii = c0 + bit;
				for (int j = lane; j < k; j += QS_LANES) {
					double zz = 0.0;
					for (int c = 0; c < k; ++c) zz += qs_elem(P, c, ii) * Binv[j * ld + c];
					if (zz > 0.0) { gp[j] += (1.0 - tau) * zz; gm[j] += tau * zz; }
					else { gp[j] -= tau * zz; gm[j] -= (1.0 - tau) * zz; }
				}
			}
		}
		// ---- the leaving edge ----
		double bestv = -1.0;
		int bj = -1;
		for (int j = lane; j < k; j += QS_LANES) {
			if ((blocked >> j) & 1ull) continue;
			const double g = gp[j] < gm[j] ? gp[j] : gm[j];
			if (g < -thr[j]) {
				const double val = bland ? (double)(k - j) : -g;
				if (bj < 0 || val > bestv) { bestv = val; bj = j; }
			}
		}
		qs_argmax(bestv, bj);
		qs_sync(); // (gp / gm / thr are read below by every lane)
		if (bj < 0) {
			if (!fresh) {
				if (!qs_refactor(P, k, ld, M, Binv, beta, v, basis, perm, snap)) { singular = true; break; }
				fresh = true;
				blocked = 0;
				continue;
			}
			// ---- no edge of this basis descends.  With rows on their kink off the basis the vertex is degenerate: another
			// basis of it may have an edge that does.  Count every such row at the multiplier bound of its side (the sign of
			// its zero): u of the plain simplex test.  Without such rows this is the test above over again. ----
			for (int j = lane; j < k; j += QS_LANES) {
				double u = 0.0;
				for (int c = 0; c < k; ++c) u += s[c] * Binv[j * ld + c];
				const bool row = basis[j] >= 0;
				gp[j] = -u + (row ? 1.0 - tau : 0.0);
				gm[j] = u + (row ? tau : 0.0);
			}
			for (int64_t c0 = P.lo; c0 < P.hi; c0 += QS_LANES) {
				const int64_t i = c0 + lane;
				uint64_t m = qs_ballot(i < P.hi && P.r[i - P.origin] == 0.0 && !qs_in_basis(basis, k, i));
				while (m) {
					const int bit = __builtin_ctzll(m);
					m &= m - 1;
					const int64_t ii = c0 + bit;
					const double psi = __builtin_signbit(P.r[ii - P.origin]) ? tau - 1.0 : tau;
					for (int j = lane; j < k; j += QS_LANES) {
						double zz = 0.0;
						for (int c = 0; c < k; ++c) zz += qs_elem(P, c, ii) * Binv[j * ld + c];
						gp[j] -= psi * zz;
						gm[j] += psi * zz;
					}
				}
			}
			// the most violated element; under Bland's rule the one of lowest index, artificials before rows
			const bool zbland = zero_pivots >= kQsBlandAfter;
			bestv = -1.0;
			bj = -1;
			for (int j = lane; j < k; j += QS_LANES) {
				if ((blocked >> j) & 1ull) continue;
				const double g = gp[j] < gm[j] ? gp[j] : gm[j];
				if (g < -thr[j]) {
					const double val = !zbland ? -g : -(basis[j] >= 0 ? (double)k + (double)(basis[j] - P.lo) : (double)(-1 - basis[j]));
					if (bj < 0 || val > bestv) { bestv = val; bj = j; }
				}
			}
			qs_argmax(bestv, bj);
			qs_sync();
			if (bj < 0) { converged = true; break; } // the multipliers lie within their bounds: a certificate
			if (zero_pivots >= kQsMaxExchanges) break;
			const double sg = gp[bj] < gm[bj] ? 1.0 : -1.0;
			for (int c = lane; c < k; c += QS_LANES) dvec[c] = sg * Binv[bj * ld + c];
			qs_sync();
			double zs = 0.0;
			for (int c = 0; c < k; ++c) zs += amax[c] * fabs(dvec[c]);
			const double zt = kQsPivotTol * zs;
			// the kink rows that the move would push across their side block it at length zero, with weight |z_i|
			const double need0 = -(gp[bj] < gm[bj] ? gp[bj] : gm[bj]);
			double w0 = 0.0;
			int64_t first0 = INT64_MAX;
			for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
				const double ri = P.r[i - P.origin];
				double wz = 0.0;
				if (ri == 0.0 && !qs_in_basis(basis, k, i)) {
					double zi = 0.0;
					for (int c = 0; c < k; ++c) zi += qs_elem(P, c, i) * dvec[c];
					if (fabs(zi) > zt && (__builtin_signbit(ri) ? zi < 0.0 : zi > 0.0)) wz = fabs(zi);
				}
				P.z[i - P.origin] = wz;
				if (wz > 0.0) {
					w0 += wz;
					if (i < first0) first0 = i;
				}
			}
			w0 = qs_sum(w0);
			first0 = qs_min_i(first0);
			if (first0 == INT64_MAX) { // nothing blocks: rounding in g; the edge rests until a pivot
				blocked |= 1ull << bj;
				continue;
			}
			int64_t enter0 = first0;
			if (!zbland) {
				// the first row, in index order, at which the weights sum to -g (all of them when rounding leaves less): by
				// bisection over the row index, one reduction per bit
				const double target = need0 < w0 ? need0 : w0;
				int64_t ilo = P.lo - 1, ihi = P.hi - 1; // prefix(ilo) = 0 < target <= prefix(ihi)
				while (ihi - ilo > 1) {
					const int64_t mid = ilo + (ihi - ilo) / 2;
					double pre = 0.0;
					for (int64_t i = P.lo + lane; i <= mid; i += QS_LANES) pre += P.z[i - P.origin];
					pre = qs_sum(pre);
					if (pre >= target) ihi = mid;
					else ilo = mid;
				}
				int64_t last = -1; // the last blocking row at or below ihi enters, those before it change side
				for (int64_t i = P.lo + lane; i <= ihi; i += QS_LANES)
					if (P.z[i - P.origin] > 0.0 && i > last) last = i;
				enter0 = -qs_min_i(-last);
				if (enter0 < first0) enter0 = first0;
				for (int64_t i = P.lo + lane; i < enter0; i += QS_LANES)
					if (P.z[i - P.origin] > 0.0) P.r[i - P.origin] = -P.r[i - P.origin];
			}
			const int64_t out = basis[bj];
			if (out >= 0 && (out - P.lo) % QS_LANES == lane) P.r[out - P.origin] = sg > 0.0 ? -0.0 : 0.0; // r = -t sg along the move
			qs_replace(P, k, ld, Binv, wrow, basis, bj, enter0);
			++zero_pivots;
			fresh = false;
			blocked = 0;
			continue;
		}
		if (pivots >= max_it || (fresh && restarts >= kQsMaxRestarts)) {
			if (!fresh && !qs_refactor(P, k, ld, M, Binv, beta, v, basis, perm, snap)) singular = true;
			break;
		}
		if (fresh) ++restarts;
		const double sigma = gp[bj] < gm[bj] ? 1.0 : -1.0;
		const double need = -(gp[bj] < gm[bj] ? gp[bj] : gm[bj]);
		const int64_t leaving = basis[bj];
		for (int c = lane; c < k; c += QS_LANES) dvec[c] = sigma * Binv[bj * ld + c];
		qs_sync();
		double zscale = 0.0;
		for (int c = 0; c < k; ++c) zscale += amax[c] * fabs(dvec[c]);
		const double ztol = kQsPivotTol * zscale;
		// ---- z, the breakpoints, their range ----
		uint64_t tmin = ~0ull, tmax = 0ull;
		double wall = 0.0;
		for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
			const double ri = P.r[i - P.origin];
			if (!(ri == ri)) continue;
			double zi = 0.0;
			for (int c = 0; c < k; ++c) zi += qs_elem(P, c, i) * dvec[c];
			if (ri == 0.0 && i != leaving && qs_in_basis(basis, k, i)) zi = 0.0; // the other basis rows stay on their kink
			double ti = INFINITY;
			if (ri != 0.0 && fabs(zi) > ztol && (ri > 0.0) == (zi > 0.0)) ti = ri / zi;
			if (!(ti > 0.0)) ti = INFINITY;
			P.z[i - P.origin] = zi;
			P.t[i - P.origin] = ti;
			if (ti < INFINITY) {
				const uint64_t tb = qs_bits(ti);
				tmin = tb < tmin ? tb : tmin;
				tmax = tb > tmax ? tb : tmax;
				wall += fabs(zi);
			}
		}
		tmin = qs_min_u(tmin);
		tmax = qs_max_u(tmax);
		wall = qs_sum(wall);
		if (tmax == 0ull || !(wall >= need)) { // no breakpoint turns the derivative: rounding in g; the edge rests until a pivot
			blocked |= 1ull << bj;
			continue;
		}
		// ---- the weighted quantile of the breakpoints, by bisection over the bits of t ----
		uint64_t blo = tmin - 1, bhi = tmax; // W(blo) = 0 < need <= W(bhi)
		while (bhi - blo > 1) {
			const uint64_t mid = blo + (bhi - blo) / 2;
			double wsum = 0.0;
			for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
				const double ti = P.t[i - P.origin]; // (+inf for masked rows, set at the first pass)
				if (ti < INFINITY && qs_bits(ti) <= mid) wsum += fabs(P.z[i - P.origin]);
			}
			wsum = qs_sum(wsum);
			if (wsum >= need) bhi = mid;
			else blo = mid;
		}
		int64_t enter = INT64_MAX;
		for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
			const double ti = P.t[i - P.origin];
			if (ti < INFINITY && qs_bits(ti) == bhi && i < enter) enter = i;
		}
		enter = qs_min_i(enter);
		if (enter == INT64_MAX) { // (cannot happen: bhi is a breakpoint) — rest the edge rather than loop
			blocked |= 1ull << bj;
			continue;
		}
		const double tstar = qs_from_bits(bhi);
		if (tstar * need <= kQsStallTol * ymax) bland = true;
		// ---- the step ----
		for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
			const double ri = P.r[i - P.origin];
			if (!(ri == ri)) continue;
			const double zi = P.z[i - P.origin];
			double rn = zi != 0.0 ? ri - tstar * zi : ri;
			if (fabs(rn) <= snap) rn = 0.0;
			if (i == enter) rn = 0.0;
			P.r[i - P.origin] = rn;
		}
		qs_replace(P, k, ld, Binv, wrow, basis, bj, enter);
		++pivots;
		fresh = false;
		blocked = 0;
	}
	*pivots_out = pivots;
	*converged_out = converged;
	return !singular;
}

// Record: the coefficients of the refactorised basis, the loss of tau from the rows, the pivot count.
QS_DEV void qs_record(const QsProblem &P, const QsState &S, const double tau, int pivots, bool converged, double *rec,
                      int32_t *iterations) {
	const int lane = qs_lane();
	const int p = P.p, k = S.k;
	const double *beta = S.beta;
	const int64_t *basis = S.basis;
	double loss = 0.0;
	for (int64_t i = P.lo + lane; i < P.hi; i += QS_LANES) {
		const double ri = P.r[i - P.origin];
		if (ri > 0.0) loss += tau * ri;
		else if (ri < 0.0) loss += (tau - 1.0) * ri;
	}
	loss = qs_sum(loss);
	if (lane == 0) {
		const int ic = P.fit_intercept ? 1 : 0;
		int n_rows_in = 0;
		for (int j = 0; j < k; ++j) n_rows_in += basis[j] >= 0 ? 1 : 0;
		for (int j = 0; j < p; ++j) rec[j] = beta[ic + j];
		rec[p] = ic ? beta[0] : NAN;
		rec[p + 1] = P.predict_layout ? NAN : tau;
		rec[p + 2] = P.predict_layout ? NAN : loss;
		rec[p + 3] = P.predict_layout ? NAN : (double)n_rows_in;
		rec[p + 4] = (double)S.n_valid;
		rec[p + 5] = 0.0;
		if (iterations) *iterations = converged ? pivots : -pivots;
	}
}

// The fit of one group at P.tau.  `work`: qs_work_doubles(k) doubles (LDS); rec: p + 6 doubles, written by lane 0;
// *iterations (optional): the pivots, negated when the bound stopped the fit.  `invalid`: tau is unusable (status 1).
QS_DEV void qs_fit(const QsProblem &P, bool invalid, double *work, double *rec, int32_t *iterations) {
	if (invalid) { qs_fail_record(rec, P.p, kQsStatusInvalidInput, iterations); return; }
	QsState S;
	const int status = qs_begin(P, work, S);
	if (status != 0) { qs_fail_record(rec, P.p, status, iterations); return; }
	int pivots;
	bool converged;
	if (!qs_pivot_to_optimum(P, S, P.tau, &pivots, &converged)) {
		qs_fail_record(rec, P.p, 2 /* ANOFOX_ERROR_SINGULAR_MATRIX */, iterations);
		return;
	}
	qs_record(P, S, P.tau, pivots, converged, rec, iterations);
}

// ---- the tau path ----
constexpr int kQsMaxTaus = 64; // quantiles of one call at most (the grid travels in the kernel arguments)

// The order the path walks a caller's grid in: the valid tau (inside (0, 1)) ascending, ties in the caller's order, so that
// neighbouring vertices are close and the result does not depend on the caller's order.  sorted[0 .. n_ok) and their
// positions slot[0 .. n_ok); slot[n_ok .. n_taus) are the positions of the invalid ones.  -> n_ok.
inline int qs_order_taus(const double *taus, int n_taus, double *sorted, uint8_t *slot) {
	int n_ok = 0;
	for (int t = 0; t < n_taus; ++t) {
		if (!(taus[t] > 0.0 && taus[t] < 1.0)) continue; // (NaN fails both)
		int at = n_ok++;
		for (; at > 0 && sorted[at - 1] > taus[t]; --at) { // insertion: stable
			sorted[at] = sorted[at - 1];
			slot[at] = slot[at - 1];
		}
		sorted[at] = taus[t];
		slot[at] = (uint8_t)t;
	}
	int n_bad = 0;
	for (int t = 0; t < n_taus; ++t)
		if (!(taus[t] > 0.0 && taus[t] < 1.0)) slot[n_ok + n_bad++] = (uint8_t)t;
	return n_ok;
}

// The predictions of one tau: pred[i * n_taus + slot] = a_i'beta for EVERY row of the group, the prediction rows (y NaN)
// included; NaN where an x of the row is not finite, or on all rows when beta is nullptr (a failed fit).  Rows strided over
// the lanes, each element written once by its row's lane.
QS_DEV void qs_predict_rows(const QsProblem &P, int k, const double *beta, double *pred, int n_taus, int slot) {
	for (int64_t i = P.lo + qs_lane(); i < P.hi; i += QS_LANES) {
		double fit = NAN;
		if (beta) {
			bool ok = true;
			for (int j = 0; j < P.p; ++j) ok = ok && isfinite(P.x[j][i]);
			if (ok) {
				fit = 0.0;
				for (int c = 0; c < k; ++c) fit += qs_elem(P, c, i) * beta[c];
			}
		}
		pred[i * (int64_t)n_taus + slot] = fit;
	}
}

// The fits of one group at every tau of a grid: begin once, then per tau (taus[0 .. n_ok), as qs_order_taus sorts them)
// pivot from the vertex the tau before left and record.  rec: n_taus records of p + 6 doubles, iterations (optional): n_taus
// counts, pred (optional): the call's [n_rows x n_taus] predictions — all indexed by the caller's position slot[t].  A
// status of begin fails every valid tau alike; a singular finish fails its tau and every later one (there is no
// trustworthy vertex to go on from); the invalid positions slot[n_ok .. n_taus) get status 1.  P.tau is not read.
QS_DEV void qs_fit_path(const QsProblem &P, const double *taus, const uint8_t *slot, int n_ok, int n_taus, double *work, double *rec,
                        int32_t *iterations, double *pred) {
	const int p = P.p;
	for (int t = n_ok; t < n_taus; ++t) {
		qs_fail_record(rec + (size_t)slot[t] * (p + 6), p, kQsStatusInvalidInput, iterations ? iterations + slot[t] : nullptr);
		if (pred) qs_predict_rows(P, 0, nullptr, pred, n_taus, slot[t]);
	}
	if (n_ok == 0) return;
	QsState S;
	int status = qs_begin(P, work, S);
	for (int t = 0; t < n_ok; ++t) {
		double *rec_t = rec + (size_t)slot[t] * (p + 6);
		int32_t *it_t = iterations ? iterations + slot[t] : nullptr;
		int pivots = 0;
		bool converged = false;
		if (status == 0 && !qs_pivot_to_optimum(P, S, taus[t], &pivots, &converged)) status = 2; // ANOFOX_ERROR_SINGULAR_MATRIX
		if (status != 0) {
			qs_fail_record(rec_t, p, status, it_t);
			if (pred) qs_predict_rows(P, 0, nullptr, pred, n_taus, slot[t]);
			continue;
		}
		qs_record(P, S, taus[t], pivots, converged, rec_t, it_t);
		if (pred) qs_predict_rows(P, S.k, S.beta, pred, n_taus, slot[t]);
	}
}

// ---- the window walk ----
// One row of the window function's output: pred[3 e] = {yhat, NaN, NaN}, yhat = a_q'beta with qs_predict_rows' arithmetic
// for the prediction row q (NaN where an x of q is not finite, beta is nullptr or the sum is not finite).  Lane 0 writes.
QS_DEV void qs_window_predict(const QsProblem &P, int k, const double *beta, int64_t q, double *pred_e) {
	if (qs_lane() != 0) return;
	double fit = NAN;
	if (beta) {
		bool ok = true;
		for (int j = 0; j < P.p; ++j) ok = ok && isfinite(P.x[j][q]);
		if (ok) {
			fit = 0.0;
			for (int c = 0; c < k; ++c) fit += qs_elem(P, c, q) * beta[c];
			if (!isfinite(fit)) fit = NAN;
		}
	}
	pred_e[0] = fit;
	pred_e[1] = NAN;
	pred_e[2] = NAN;
}

// The fits of the consecutive output rows [e0, e1) of ONE partition, each over its frame [flo[e], fhi[e]) and predicting the
// x of the frame's last row.  The first frame is a cold fit (begin, pivot: qs_fit).  A later frame whose bounds are both
// non-decreasing, that overlaps the frame before it and loses none of the basis rows keeps the vertex: the rows that left
// are masked, the rows that entered get r = y - a'beta of the carried beta (on their kink: the side of the rounding, as the
// refactorisation assigns it), n_valid, max|y|, the snap and the column sizes are those a begin on this frame computes, and
// the pivots go on from the carried basis with a fresh budget (as the tau path does per tau).  Every other transition, a frame
// after one that failed, and a frame from which a basis row left begin afresh.
//   P        y, x, p, fit_intercept, tau, max_iterations; r / z / t: a slab of slab_rows slots each that belongs to the caller
//            (lo, hi, rule_count and origin are set here per frame: rule_count = the frame's rows whose y is not NaN)
//   pred     [.. x 3], rec [.. x (p + 6)] (optional, the quantile layout), iterations (optional), cold (optional: 1 where
//            the frame ran begin) — all indexed by the output row e
// A frame longer than the slab gets status 2 (the planner never launches one).  -> the frames that ran begin; *restarts
// (optional): those of them that followed a fitted frame (a basis row left, or the bounds were not monotone and overlapping)
// — the first frame of the run and the frames after a failed one are not restarts.
QS_DEV int64_t qs_fit_window(QsProblem &P, bool invalid, const int64_t *flo, const int64_t *fhi, int64_t e0, int64_t e1,
                             int64_t slab_rows, double *work, double *pred, double *rec, int32_t *iterations, uint8_t *cold,
                             int64_t *restarts) {
	const int lane = qs_lane();
	const int p = P.p, k = p + (P.fit_intercept ? 1 : 0);
	QsState S;
	bool have = false; // S holds the optimal vertex of the frame [plo, phi)
	int64_t plo = 0, phi = 0, n_cold = 0, n_restart = 0;
	P.predict_layout = 0;
	for (int64_t e = e0; e < e1; ++e) {
		const int64_t lo = flo[e], hi = fhi[e];
		double *rec_e = rec ? rec + e * (int64_t)(p + 6) : nullptr;
		int32_t *it_e = iterations ? iterations + e : nullptr;
		if (cold && lane == 0) cold[e] = 0;
		int status = 0;
		bool began = false;
		if (invalid) status = kQsStatusInvalidInput;
		else if (hi <= lo) status = kQsStatusTooFewRows; // an empty frame
		else if (hi - lo > slab_rows) status = 2;
		if (status == 0) {
			bool warm = have && lo >= plo && hi >= phi && lo < phi && hi - P.origin <= slab_rows;
			if (warm) // a basis row among the rows that leave: this vertex does not exist on the new frame
				for (int j = 0; j < k; ++j) warm = warm && !(S.basis[j] >= plo && S.basis[j] < lo);
			int64_t rule = 0;
			for (int64_t i = lo + lane; i < hi; i += QS_LANES) rule += P.y[i] == P.y[i] ? 1 : 0;
			P.rule_count = qs_sum_i(rule);
			P.lo = lo;
			P.hi = hi;
			qs_sync(); // (the basis was read above; begin writes it)
			if (!warm) {
				P.origin = lo;
				began = true;
				status = qs_begin(P, work, S);
			} else if (P.rule_count < 2) {
				status = kQsStatusTooFewRows;
			} else {
				for (int64_t i = plo + lane; i < lo; i += QS_LANES) { // the rows that left: as begin masks an invalid row
					P.r[i - P.origin] = NAN;
					P.z[i - P.origin] = 0.0;
					P.t[i - P.origin] = INFINITY;
				}
				int64_t n_valid = 0;
				double ymax = 0.0;
				for (int64_t i = lo + lane; i < hi; i += QS_LANES) {
					const double yv = P.y[i];
					bool ok = isfinite(yv);
					for (int j = 0; j < p; ++j) ok = ok && isfinite(P.x[j][i]);
					if (ok) {
						++n_valid;
						ymax = fmax(ymax, fabs(yv));
					}
				}
				n_valid = qs_sum_i(n_valid);
				ymax = qs_max(ymax);
				const double snap = kQsSnapTol * ymax;
				if (n_valid == 0) status = kQsStatusNoValidData;
				else if (n_valid < k) status = kQsStatusInsufficientData;
				else {
					for (int64_t i = phi + lane; i < hi; i += QS_LANES) { // the rows that entered
						const double yv = P.y[i];
						bool ok = isfinite(yv);
						for (int j = 0; j < p; ++j) ok = ok && isfinite(P.x[j][i]);
						double rr = NAN;
						if (ok) {
							double fit = 0.0;
							for (int c = 0; c < k; ++c) fit += qs_elem(P, c, i) * S.beta[c];
							rr = yv - fit;
							if (fabs(rr) <= snap) rr = copysign(0.0, rr);
						}
						P.r[i - P.origin] = rr;
						P.z[i - P.origin] = 0.0;
						P.t[i - P.origin] = INFINITY;
					}
					qs_column_sizes(P, k, S.amax, S.asum);
					S.n_valid = n_valid;
					S.ymax = ymax;
					S.snap = snap;
					qs_sync();
				}
			}
		}
		int pivots = 0;
		bool converged = false;
		if (status == 0 && !qs_pivot_to_optimum(P, S, P.tau, &pivots, &converged)) status = 2; // ANOFOX_ERROR_SINGULAR_MATRIX
		if (began) {
			++n_cold;
			n_restart += have ? 1 : 0;
			if (cold && lane == 0) cold[e] = 1;
		}
		if (status != 0) {
			if (rec_e) qs_fail_record(rec_e, p, status, it_e);
			else if (it_e && lane == 0) *it_e = 0;
			qs_window_predict(P, 0, nullptr, 0, pred + 3 * e);
			have = false;
			continue;
		}
		if (rec) qs_record(P, S, P.tau, pivots, converged, rec_e, it_e);
		else if (it_e && lane == 0) *it_e = converged ? pivots : -pivots;
		qs_window_predict(P, k, S.beta, hi - 1, pred + 3 * e);
		have = true;
		plo = lo;
		phi = hi;
	}
	if (restarts) *restarts = n_restart;
	return n_cold;
}

} // namespace quantile
} // namespace anofox
