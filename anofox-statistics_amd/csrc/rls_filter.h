// rls_filter.h — the recursive least squares fit of one range of rows, in the reference's operation order
// (fit_rls / RlsState::update, crates/anofox-stats-core/src/models/rls.rs).  DESIGN.md §1 "Recursive least squares".
//
// The reference's filter is chaotic for some inputs (lambda < 1: coefficients of 1e11 that move by 45x their size when
// one input moves by an ulp), so the contract is its exact operation order, which gives bit-identical coefficients
// under IEEE binary64 without contraction.  hipcc contracts a*b + c by default for HIP; every function here switches
// contraction off for its own body.  The quirk of the reference that is kept: P is updated in place, row by row, so
// row i of the update reads the rows l < i that this step already rewrote.
//
// rls_fit_range: one lane, P in registers (the lane kernels of rls.hip instantiate PMAX = p <= 8; the host tests
// instantiate PMAX = 128).  rls_fit_range_wave: one wavefront, P column-major in LDS, lane j owns column j of the update
// (a column's update reads only that column, so the in-place order needs no barrier inside it).  Both give the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RLS_HD __host__ __device__ __forceinline__
#else
#define RLS_HD inline
#endif

namespace anofox {
namespace rls {

// status words of the record (an AnofoxErrorCode, or the aggregate's "fewer than 2 rows" NULL)
constexpr int kStatusInvalidInput = 1;
constexpr int kStatusInsufficientData = 6;
constexpr int kStatusNoValidData = 10;
constexpr int kStatusTooFewRows = 100;

// Rust's f64 Sum folds from -0.0 (the exact additive identity): the iterator sums of update() and fit_rls start there,
// the explicit `+=` loops (P x and k x' P) from 0.0.
constexpr double kSumStart = -0.0;

struct RlsParams {
	double lambda; // forgetting factor
	double delta;  // initial P diagonal
	int fit_intercept;
};

// record of a failed range: every field NaN, the status last (length p + 6)
RLS_HD void rls_fail_record(double *rec, int p, int status) {
	for (int j = 0; j < p + 5; ++j) rec[j] = NAN;
	rec[p + 5] = (double)status;
}

RLS_HD bool rls_row_valid(const double *y, const double *const *x, int p, int64_t r) {
	if (!isfinite(y[r])) return false;
	for (int j = 0; j < p; ++j)
		if (!isfinite(x[j][r])) return false;
	return true;
}

// sum of the valid rows' y in row order (the intercept-only shortcut's mean)
RLS_HD double rls_valid_y_sum(const double *y, const double *const *x, int p, int64_t lo, int64_t hi) {
#pragma clang fp contract(off)
	double s = kSumStart;
	for (int64_t r = lo; r < hi; ++r)
		if (rls_row_valid(y, x, p, r)) s += y[r];
	return s;
}

// One row of RlsState::update on the slots of `act` (D = PMAX + 1; slot 0 the intercept, u[0] == 1): the reference's order.
template <int PMAX>
RLS_HD void rls_step(const double *y, const double *const *x, int p, int64_t r, double lam, const bool *act, double (*P)[PMAX + 1],
                     double *b, double *u) {
#pragma clang fp contract(off)
	constexpr int D = PMAX + 1;
	const int dn = p + 1 < D ? p + 1 : D;
	double px[D], k[D];
#pragma unroll
	for (int j = 0; j < p; ++j)
		u[1 + j] = x[j][r];
	double yhat = kSumStart;
#pragma unroll
	for (int i = 0; i < dn; ++i)
		if (act[i]) yhat += u[i] * b[i];
	const double e = y[r] - yhat;
#pragma unroll
	for (int i = 0; i < dn; ++i) {
		double s = 0.0;
#pragma unroll
		for (int j = 0; j < dn; ++j)
			if (act[j]) s += P[i][j] * u[j];
		px[i] = s;
	}
	double xpx = kSumStart;
#pragma unroll
	for (int i = 0; i < dn; ++i)
		if (act[i]) xpx += u[i] * px[i];
	const double den = lam + xpx;
#pragma unroll
	for (int i = 0; i < dn; ++i) {
		k[i] = px[i] / den;
		b[i] += k[i] * e;
	}
	// P <- (P - k x' P) / lambda, in place: row i reads the rows l < i already rewritten
#pragma unroll
	for (int i = 0; i < dn; ++i) {
		if (!act[i]) continue;
#pragma unroll
		for (int j = 0; j < dn; ++j) {
			if (!act[j]) continue;
			double s = 0.0;
#pragma unroll
			for (int l = 0; l < dn; ++l)
				if (act[l]) s += (k[i] * u[l]) * P[l][j];
			P[i][j] = (P[i][j] - s) / lam;
		}
	}
}

// The fit of rows [lo, hi) of columns y, x[0..p) into rec (length p + 6): coefficients, intercept, r2 / adj r2 / sigma
// (NaN, as the reference's FFI), n_obs, status.  PMAX >= p; slot 0 of the filter is the intercept, slot 1 + j column j;
// inactive slots (no intercept, constant columns) are skipped, never added as zeros, so the sums are those of the
// reduced-dimension filter.
template <int PMAX>
RLS_HD void rls_fit_range(const double *y, const double *const *x, int p, int64_t lo, int64_t hi, RlsParams o, double *rec) {
#pragma clang fp contract(off)
	constexpr int D = PMAX + 1;
	const int dn = p + 1 < D ? p + 1 : D; // slots in use
	double x0[PMAX > 0 ? PMAX : 1];
	bool act[D];
	int64_t first = -1, n_valid = 0;
	for (int j = 0; j < D; ++j) act[j] = false;
	for (int64_t r = lo; r < hi; ++r) {
		if (!rls_row_valid(y, x, p, r)) continue;
		++n_valid;
		if (first < 0) {
			first = r;
#pragma unroll
			for (int j = 0; j < p; ++j)
				x0[j] = x[j][r];
			continue;
		}
#pragma unroll
		for (int j = 0; j < p; ++j)
			if (!(fabs(x[j][r] - x0[j]) < 1e-10)) act[1 + j] = true;
	}
	if (n_valid == 0) { rls_fail_record(rec, p, kStatusNoValidData); return; }
	int n_active = 0;
	for (int j = 0; j < p; ++j) n_active += act[1 + j];
	if (n_active == 0) { // intercept-only model: no option checks (it never reaches RlsState::new)
		if (!o.fit_intercept) { rls_fail_record(rec, p, kStatusInsufficientData); return; }
		const double s = rls_valid_y_sum(y, x, p, first, hi);
		for (int j = 0; j < p; ++j) rec[j] = NAN;
		rec[p] = s / (double)n_valid;
		rec[p + 1] = rec[p + 2] = rec[p + 3] = NAN;
		rec[p + 4] = (double)n_valid;
		rec[p + 5] = 0.0;
		return;
	}
	if (o.lambda <= 0.0 || o.lambda > 1.0 || o.delta <= 0.0) { rls_fail_record(rec, p, kStatusInvalidInput); return; }
	act[0] = o.fit_intercept != 0;
	double P[D][D], b[D], u[D];
#pragma unroll
	for (int i = 0; i < dn; ++i) {
		b[i] = 0.0;
#pragma unroll
		for (int j = 0; j < dn; ++j) P[i][j] = i == j ? o.delta : 0.0;
	}
	u[0] = 1.0;
	for (int64_t r = first; r < hi; ++r) {
		if (!rls_row_valid(y, x, p, r)) continue;
		rls_step<PMAX>(y, x, p, r, o.lambda, act, P, b, u);
	}
	for (int j = 0; j < p; ++j) rec[j] = act[1 + j] ? b[1 + j] : NAN;
	rec[p] = o.fit_intercept ? b[0] : NAN;
	rec[p + 1] = rec[p + 2] = rec[p + 3] = NAN;
	rec[p + 4] = (double)n_valid;
	rec[p + 5] = 0.0;
}

// anofox_predict_with_interval's yhat (ffi lib.rs:2292-2300): intercept (0 when NaN) + sum of coef_j x_j in index order
// over the coefficients that are not NaN.  Contraction off, so yhat is bit-identical too.
RLS_HD double rls_predict_row(const double *rec, int p, const double *const *x, int64_t r) {
#pragma clang fp contract(off)
	double yhat = isnan(rec[p]) ? 0.0 : rec[p];
	for (int j = 0; j < p; ++j)
		if (!isnan(rec[j])) yhat += rec[j] * x[j][r];
	return yhat;
}


// The expanding window of one partition, rows [lo, hi) in window order, in ONE pass: pred[r] (r in [lo, hi)) = the value of
// the frame [lo, r + 1) exactly as rls_fit_range over that frame followed by rls_predict_row of row r gives it (NaN = NULL):
// the filter state after a prefix IS the prefix's fit.  The constant-column set of a prefix only shrinks (a column that
// varied keeps varying); when it changes at row r the filter restarts over the prefix with the new set — at most p times.
// The intercept-only shortcut uses the running sum of y in row order; invalid options null a frame only once some column
// varies.  NULL rule of the window: MORE than p + [intercept] rows with non-NULL y in the frame.
template <int PMAX>
RLS_HD void rls_expanding_range(const double *y, const double *const *x, int p, int64_t lo, int64_t hi, RlsParams o, double *pred) {
#pragma clang fp contract(off)
	constexpr int D = PMAX + 1;
	const int dn = p + 1 < D ? p + 1 : D;
	const int64_t need = p + (o.fit_intercept ? 1 : 0);
	const bool bad_opts = o.lambda <= 0.0 || o.lambda > 1.0 || o.delta <= 0.0;
	double x0[PMAX > 0 ? PMAX : 1], P[D][D], b[D], u[D];
	bool act[D];
	for (int j = 0; j < D; ++j) act[j] = false;
	act[0] = o.fit_intercept != 0;
	u[0] = 1.0;
	int64_t first = -1, n_valid = 0, n_y = 0;
	int n_active = 0;
	double ysum = kSumStart;
	for (int64_t r = lo; r < hi; ++r) {
		n_y += y[r] == y[r];
		if (rls_row_valid(y, x, p, r)) {
			++n_valid;
			ysum += y[r];
			bool grew = false;
			if (first < 0) {
				first = r;
#pragma unroll
				for (int j = 0; j < p; ++j)
					x0[j] = x[j][r];
			} else {
#pragma unroll
				for (int j = 0; j < p; ++j)
					if (!act[1 + j] && !(fabs(x[j][r] - x0[j]) < 1e-10)) {
						act[1 + j] = true;
						++n_active;
						grew = true;
					}
			}
			if (n_active > 0 && !bad_opts) {
				if (grew) { // restart over the prefix with the new column set
#pragma unroll
					for (int i = 0; i < dn; ++i) {
						b[i] = 0.0;
#pragma unroll
						for (int j = 0; j < dn; ++j) P[i][j] = i == j ? o.delta : 0.0;
					}
					for (int64_t q = first; q <= r; ++q)
						if (rls_row_valid(y, x, p, q)) rls_step<PMAX>(y, x, p, q, o.lambda, act, P, b, u);
				} else {
					rls_step<PMAX>(y, x, p, r, o.lambda, act, P, b, u);
				}
			}
		}
		double v = NAN;
		if (n_y > need && n_valid > 0) {
			double rec[(PMAX > 0 ? PMAX : 1) + 6];
			if (n_active == 0) {
				if (o.fit_intercept) {
					for (int j = 0; j < p; ++j) rec[j] = NAN;
					rec[p] = ysum / (double)n_valid;
					v = rls_predict_row(rec, p, x, r);
				}
			} else if (!bad_opts) {
				for (int j = 0; j < p; ++j) rec[j] = act[1 + j] ? b[1 + j] : NAN;
				rec[p] = o.fit_intercept ? b[0] : NAN;
				v = rls_predict_row(rec, p, x, r);
			}
		}
		pred[3 * r] = v;
		pred[3 * r + 1] = v;
		pred[3 * r + 2] = v;
	}
}

#if defined(__HIPCC__)
// LDS of rls_fit_range_wave for p features: P (d x ld, ld = d | 1), u, b, px, k (d each), the active slot list, the record
__host__ __device__ inline size_t rls_wave_lds_bytes(int p) {
	const int d = p + 1, ld = d | 1;
	return ((size_t)d * ld + 4 * (size_t)d + (size_t)p + 6) * sizeof(double) + (size_t)d * sizeof(int);
}

// The same fit by one wavefront of 64 lanes (blockDim.x == 64), P in `lds` (rls_wave_lds_bytes(p)).  The row pass is
// uniform across the wave; the per-row sums that are sequential in the reference (yhat, x'Px) are formed by every lane
// in slot order from LDS.  rec is written by lane 0.
__device__ inline void rls_fit_range_wave(const double *y, const double *const *x, int p, int64_t lo, int64_t hi, RlsParams o,
                                          double *rec, double *lds) {
#pragma clang fp contract(off)
	const int lane = threadIdx.x;
	const int dmax = p + 1, ld = dmax | 1;
	double *Pc = lds;                   // column-major: P[i][j] at Pc[j * ld + i]
	double *u = Pc + (size_t)dmax * ld; // current row, slots in reduced order
	double *b = u + dmax;
	double *px = b + dmax;
	double *kk = px + dmax;
	double *srec = kk + dmax;           // p + 6
	int *slot = (int *)(srec + p + 6);  // reduced slot -> column (-1 = intercept)
	// the first valid row
	int64_t first = -1;
	for (int64_t c = lo; c < hi && first < 0; c += 64) {
		const int64_t r = c + lane;
		const unsigned long long m = __ballot(r < hi && rls_row_valid(y, x, p, r));
		if (m) first = c + (int64_t)__ffsll((long long)m) - 1;
	}
	if (first < 0) {
		if (lane == 0) rls_fail_record(rec, p, kStatusNoValidData);
		return;
	}
	// valid rows and the constant-column test (lane-local, reduced across the wave at the end)
	int64_t n_valid = 0;
	unsigned long long nc[2] = {0ull, 0ull};
	for (int64_t r = first + lane; r < hi; r += 64) {
		if (!rls_row_valid(y, x, p, r)) continue;
		++n_valid;
		for (int j = 0; j < p; ++j)
			if (!(fabs(x[j][r] - x[j][first]) < 1e-10)) nc[j >> 6] |= 1ull << (j & 63);
	}
	for (int s = 32; s > 0; s >>= 1) {
		n_valid += __shfl_xor(n_valid, s);
		nc[0] |= __shfl_xor(nc[0], s);
		nc[1] |= __shfl_xor(nc[1], s);
	}
	const int n_active = __popcll(nc[0]) + __popcll(nc[1]);
	if (n_active == 0) {
		if (!o.fit_intercept) {
			if (lane == 0) rls_fail_record(rec, p, kStatusInsufficientData);
			return;
		}
		// the mean of y: a sequential sum in row order, the same adds on every lane
		double s = kSumStart;
		for (int64_t c = first; c < hi; c += 64) {
			const int64_t r = c + lane;
			const bool v = r < hi && rls_row_valid(y, x, p, r);
			const double yv = v ? y[r] : 0.0;
			unsigned long long m = __ballot(v);
			while (m) {
				const int bit = __ffsll((long long)m) - 1;
				m &= m - 1;
				s += __shfl(yv, bit);
			}
		}
		if (lane == 0) {
			for (int j = 0; j < p; ++j) rec[j] = NAN;
			rec[p] = s / (double)n_valid;
			rec[p + 1] = rec[p + 2] = rec[p + 3] = NAN;
			rec[p + 4] = (double)n_valid;
			rec[p + 5] = 0.0;
		}
		return;
	}
	if (o.lambda <= 0.0 || o.lambda > 1.0 || o.delta <= 0.0) {
		if (lane == 0) rls_fail_record(rec, p, kStatusInvalidInput);
		return;
	}
	const int icpt = o.fit_intercept ? 1 : 0;
	const int d = icpt + n_active;
	if (lane == 0) {
		int k = 0;
		if (icpt) slot[k++] = -1;
		for (int j = 0; j < p; ++j)
			if ((nc[j >> 6] >> (j & 63)) & 1ull) slot[k++] = j;
	}
	for (int i = lane; i < d; i += 64) {
		b[i] = 0.0;
		for (int l = 0; l < d; ++l) Pc[(size_t)i * ld + l] = l == i ? o.delta : 0.0;
	}
	__syncthreads();
	const double lam = o.lambda;
	for (int64_t c = first; c < hi; c += 64) {
		const int64_t rr = c + lane;
		unsigned long long m = __ballot(rr < hi && rls_row_valid(y, x, p, rr));
		while (m) {
			const int64_t r = c + __ffsll((long long)m) - 1;
			m &= m - 1;
			for (int i = lane; i < d; i += 64) u[i] = slot[i] < 0 ? 1.0 : x[slot[i]][r];
			__syncthreads();
			for (int i = lane; i < d; i += 64) {
				double s = 0.0;
				for (int j = 0; j < d; ++j) s += Pc[(size_t)j * ld + i] * u[j];
				px[i] = s;
			}
			__syncthreads();
			double yhat = kSumStart, xpx = kSumStart;
			for (int i = 0; i < d; ++i) yhat += u[i] * b[i];
			for (int i = 0; i < d; ++i) xpx += u[i] * px[i];
			const double e = y[r] - yhat, den = lam + xpx;
			__syncthreads();
			for (int i = lane; i < d; i += 64) {
				kk[i] = px[i] / den;
				b[i] += kk[i] * e;
			}
			__syncthreads();
			for (int j = lane; j < d; j += 64) {
				double *col = Pc + (size_t)j * ld;
				for (int i = 0; i < d; ++i) {
					const double ki = kk[i];
					double s = 0.0;
					for (int l = 0; l < d; ++l) s += (ki * u[l]) * col[l];
					col[i] = (col[i] - s) / lam;
				}
			}
			__syncthreads();
		}
	}
	if (lane == 0) {
		for (int j = 0; j < p; ++j) rec[j] = NAN;
		for (int i = 0; i < d; ++i) {
			if (slot[i] < 0) rec[p] = b[i];
			else rec[slot[i]] = b[i];
		}
		if (!icpt) rec[p] = NAN;
		rec[p + 1] = rec[p + 2] = rec[p + 3] = NAN;
		rec[p + 4] = (double)n_valid;
		rec[p + 5] = 0.0;
	}
	(void)srec;
}
#endif

} // namespace rls
} // namespace anofox
