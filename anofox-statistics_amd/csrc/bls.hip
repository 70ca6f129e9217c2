// bls.hip — grouped bounded / non-negative least squares fits: a batched active-set solve on the moment records of the
// accumulate kernels, and the entry points anofox_hip_bls_fit_batch_{device,host}, anofox_hip_bls_fit_predict_batch_*,
// anofox_bls_fit / anofox_nnls_fit / anofox_free_bls_result.
//
// The contract and the method: bls_solve.h and DESIGN.md §1, "Bounded least squares".
//   narrow (p <= 8): one LANE per group, the scaled moments, the iterate, the free-set mask and the Cholesky factor of the
//     free block in registers (bls_fit_from_moments);
//   wide (9 <= p <= 128): one WAVEFRONT per group.  LDS holds the lower triangles of the scaled matrix A and of the factor
//     of the current free block (p (p + 1) doubles together) and the per-column vectors; lane k owns column k (and k + 64).
//     The free columns are compacted (ballot + prefix count) and the m x m block is factorised column by column, lane a
//     owning row a; the triangular solves keep the right-hand side in registers and broadcast one component per step.
// Statistics: ssr = tss - z'(q + w); where that falls below 1e-7 of tss it has cancelled and bls_rows_kernel sums the
// squared residuals from the rows (the elastic net's rule).  No atomics: repeated calls give bit-identical records.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "bls_solve.h"

using namespace anofox;

#include "host_stage.h"
#include "moment_solve.h"
#include "scalar_fit.h"

using namespace anofox::host;

namespace {

typedef BlsParamsT<kNarrowMaxP> BlsNarrowParams;
typedef BlsParamsT<kWideMaxP> BlsWideParams;

// ---- narrow: one lane per group ----
template <int P>
__global__ __launch_bounds__(64) void bls_solve_narrow_kernel(BatchArgs a, BlsNarrowParams bp) {
	using L = MomentLayout<P>;
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.n_groups) return;
	const bool icpt = a.fit_intercept != 0;
	const double *rec = a.moments + g * (int64_t)L::REC;
	const int len = bp.predict_layout ? P + 6 : 3 * P + 6;
	double *core = a.core + g * (int64_t)len;
	const int64_t nrows = a.rule_counts ? a.rule_counts[g] : group_row_end(a, g) - a.row_offsets[g];
	double out[3 * P + 6];
	const BlsSolveInfo s = bls_fit_from_moments<P>(rec, bp, icpt, nrows, out);
#pragma unroll
	for (int k = 0; k < 3 * P + 6; ++k)
		if (k < len) core[k] = out[k];
	a.refine_list[g] = s.cancels ? 1 : 0;
	if (bp.iterations) bp.iterations[g] = s.converged ? s.iterations : -s.iterations;
}

// ---- wide: one wavefront per group ----
__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; } // j <= i

// R = columns per lane (1: p <= 64, 2: p <= 128)
template <int R>
__global__ __launch_bounds__(64) void bls_solve_wide_kernel(WideArgs a, BlsWideParams bp) {
	extern __shared__ double bls_lds[];
	const int p = a.p;
	const int ntri = p * (p + 1) / 2;
	const int lane = threadIdx.x;
	const int64_t gl = blockIdx.x;
	const int64_t g = a.group_base + gl;
	const bool icpt = a.fit_intercept != 0;
	const int pl = bp.predict_layout;
	const WideMoments m(a.moments, gl, p);
	const double *sx = m.sx, *sxy = m.sxy, *fx = m.fx, *nonconst = m.nonconst;
	double *core = a.core + g * (int64_t)(pl ? p + 6 : 3 * p + 6);
	const double sy = m.sy, syy = m.syy, sw = m.sw, cnt = m.cnt, cyy_c = m.cyy_c;
	const int64_t nrows = a.rule_counts ? a.rule_counts[g] : group_row_end(a, g) - a.row_offsets[g];
	const int p_eff = m.p_eff;
	const double ymean = m.ymean(icpt);
	if (lane == 0) a.refine_list[gl] = 0;
	bool shortcut;
	const int status = bls_prechecks(bp.invalid, nrows, cnt, p_eff, icpt, &shortcut); // (uniform: lane 0 writes)
	if (status != 0 || shortcut) {
		if (lane == 0) {
			if (status != 0) bls_write_status(core, p, pl, status);
			else bls_write_shortcut(core, p, pl, ymean, cnt);
			if (bp.iterations) bp.iterations[g] = 0;
		}
		return;
	}
	// LDS: At | Lt (lower triangles, row-major) | zs | ws | los | his | dsc | st, idxF, blk (int)
	double *At = bls_lds, *Lt = At + ntri;
	double *zs = Lt + ntri, *ws = zs + p, *los = ws + p, *his = los + p, *dsc = his + p;
	int *st = reinterpret_cast<int *>(dsc + p), *idxF = st + p, *blk = idxF + p; // state: 0 dead, 1 free, 2 lower, 3 upper
	const double inv_sw = 1.0 / sw;
	double qv[R];
#pragma unroll
	for (int h = 0; h < R; ++h) {
		const int k = lane + 64 * h;
		qv[h] = 0.0;
		if (k < p) {
			const double cii = m.raw(k, k) - (icpt ? sx[k] * sx[k] * inv_sw : 0.0);
			const bool live = nonconst[k] != 0.0 && cii > 0.0;
			const double d = live ? sqrt(cii) : 1.0;
			const double blo = bp.lo[k], bhi = bp.hi[k];
			dsc[k] = d;
			los[k] = blo * d;
			his[k] = bhi * d;
			qv[h] = live ? (icpt ? sxy[k] - sx[k] * sy * inv_sw : sxy[k]) / d : 0.0;
			int s = 0;
			double z0 = 0.0;
			if (live) {
				if (isfinite(blo)) { s = 2; z0 = blo * d; }
				else if (isfinite(bhi)) { s = 3; z0 = bhi * d; }
				else s = 1;
			}
			st[k] = s;
			zs[k] = z0;
			blk[k] = 0;
		}
	}
	__syncthreads();
	for (int i = 0; i < p; ++i) {
		const bool li = st[i] != 0;
		for (int j = lane; j <= i; j += 64) {
			double v = m.c(j, i, icpt, inv_sw); // j <= i: element (j, i) of the upper triangle the record keeps
			v = (li && st[j] != 0) ? v / (dsc[i] * dsc[j]) : 0.0;
			At[tri(i, j)] = i == j ? 1.0 : v;
		}
	}
	__syncthreads();

	const double tss = icpt ? cyy_c : syy;
	const double tau = kBlsKktTol * sqrt(tss);
	const int cap = bls_iteration_cap(p);
	const int max_it = bp.max_iterations < cap ? bp.max_iterations : cap;
	int iters = 0, passes = 0, jstar = -1;
	bool converged = false, first = false, star_low = false;
	// (everything that steers the loop is wavefront-uniform: the barriers below are reached by all lanes together)
	bool inner;
	{
		bool fr = false;
#pragma unroll
		for (int h = 0; h < R; ++h) {
			const int k = lane + 64 * h;
			fr = fr || (k < p && st[k] == 1);
		}
		inner = __ballot(fr) != 0ull;
	}
	double wv[R];
	for (;;) {
		// w = q - A z
#pragma unroll
		for (int h = 0; h < R; ++h) {
			const int k = lane + 64 * h;
			wv[h] = 0.0;
			if (k < p) {
				double s = qv[h];
				for (int j = 0; j < p; ++j) s -= At[j <= k ? tri(k, j) : tri(j, k)] * zs[j];
				wv[h] = st[k] != 0 ? s : 0.0;
				ws[k] = wv[h];
			}
		}
		__syncthreads();
		if (!inner) {
			double bestv = tau;
			int best = -1;
#pragma unroll
			for (int h = 0; h < R; ++h) {
				const int k = lane + 64 * h;
				if (k < p && !blk[k]) {
					const int s = st[k];
					const double v = s == 2 ? wv[h] : (s == 3 ? -wv[h] : 0.0);
					if (v > bestv) { bestv = v; best = k; }
				}
			}
			for (int m = 32; m >= 1; m >>= 1) { // the largest violation, the lowest column on ties
				const double ov = __shfl_xor(bestv, m, 64);
				const int oi = __shfl_xor(best, m, 64);
				if (oi >= 0 && (ov > bestv || (ov == bestv && (best < 0 || oi < best)))) { bestv = ov; best = oi; }
			}
			if (best < 0) { converged = true; break; }
			if (iters >= max_it) break;
			++iters;
			jstar = best;
			star_low = st[best] == 2;
			__syncthreads(); // (every lane has read st[best])
			if (lane == 0) st[best] = 1;
			inner = true;
			first = true;
			passes = 0;
			__syncthreads();
		}
		// the free columns, compacted in column order
		int m = 0;
#pragma unroll
		for (int h = 0; h < R; ++h) {
			const int k = lane + 64 * h;
			const bool fr = k < p && st[k] == 1;
			const unsigned long long b = __ballot(fr);
			if (fr) idxF[m + __popcll(b & ((1ull << lane) - 1ull))] = k;
			m += __popcll(b);
		}
		__syncthreads();
		// Cholesky of the free block: Lt[tri(r, c)], c < r, and the INVERSE pivots on the diagonal
		bool bad = false;
		for (int jc = 0; jc < m; ++jc) {
			const int cj = idxF[jc];
			double t[R];
#pragma unroll
			for (int h = 0; h < R; ++h) {
				const int r = lane + 64 * h;
				t[h] = 0.0;
				if (r >= jc && r < m) {
					double s = r == jc ? 1.0 : At[tri(idxF[r], cj)];
					const double *lr = Lt + tri(r, 0), *lj = Lt + tri(jc, 0);
					for (int k = 0; k < jc; ++k) s -= lr[k] * lj[k];
					t[h] = s;
				}
			}
			const double dj = __shfl((R == 1 || jc < 64) ? t[0] : t[R - 1], jc & 63, 64);
			const bool ok = dj > kEnAliasTol;
			bad = bad || !ok;
			const double inv = ok ? 1.0 / sqrt(dj) : 0.0;
#pragma unroll
			for (int h = 0; h < R; ++h) {
				const int r = lane + 64 * h;
				if (r >= jc && r < m) Lt[tri(r, jc)] = r == jc ? inv : t[h] * inv;
			}
			__syncthreads();
		}
		if (bad && first && jstar >= 0) { // collinear with the free columns: back to its bound, not chosen again for now
			if (lane == 0) {
				st[jstar] = star_low ? 2 : 3;
				blk[jstar] = 1;
			}
			inner = false;
			__syncthreads();
			continue;
		}
		// L L' d = w_F: lane r keeps component r of the right-hand side, one component is broadcast per step
		double rv[R];
		int col[R];
#pragma unroll
		for (int h = 0; h < R; ++h) {
			const int r = lane + 64 * h;
			col[h] = r < m ? idxF[r] : -1;
			rv[h] = r < m ? ws[col[h]] : 0.0;
		}
		for (int jc = 0; jc < m; ++jc) {
			const double mine = ((R == 1 || jc < 64) ? rv[0] : rv[R - 1]) * Lt[tri(jc, jc)];
			const double vj = __shfl(mine, jc & 63, 64);
#pragma unroll
			for (int h = 0; h < R; ++h) {
				const int r = lane + 64 * h;
				if (r == jc) rv[h] = vj;
				else if (r > jc && r < m) rv[h] -= Lt[tri(r, jc)] * vj;
			}
		}
		for (int jc = m - 1; jc >= 0; --jc) {
			const double mine = ((R == 1 || jc < 64) ? rv[0] : rv[R - 1]) * Lt[tri(jc, jc)];
			const double vj = __shfl(mine, jc & 63, 64);
#pragma unroll
			for (int h = 0; h < R; ++h) {
				const int r = lane + 64 * h;
				if (r == jc) rv[h] = vj;
				else if (r < jc) rv[h] -= Lt[tri(jc, r)] * vj;
			}
		}
		// the longest feasible fraction of the step; ties go to the lowest compacted index
		double alpha = 1.0;
		int kmin = 0x7fffffff, kside = 0;
		double zk[R];
#pragma unroll
		for (int h = 0; h < R; ++h) {
			const int r = lane + 64 * h;
			zk[h] = 0.0;
			if (r < m) {
				zk[h] = zs[col[h]];
				const double s = zk[h] + rv[h];
				const double l = los[col[h]], u = his[col[h]];
				if (s < l) {
					const double al = fmax((l - zk[h]) / rv[h], 0.0);
					if (al < alpha) { alpha = al; kmin = r; kside = 2; }
				} else if (s > u) {
					const double al = fmax((u - zk[h]) / rv[h], 0.0);
					if (al < alpha) { alpha = al; kmin = r; kside = 3; }
				}
			}
		}
		for (int mm = 32; mm >= 1; mm >>= 1) {
			const double oa = __shfl_xor(alpha, mm, 64);
			const int oi = __shfl_xor(kmin, mm, 64), os = __shfl_xor(kside, mm, 64);
			if (oa < alpha || (oa == alpha && oi < kmin)) { alpha = oa; kmin = oi; kside = os; }
		}
		const bool whole = kmin == 0x7fffffff;
#pragma unroll
		for (int h = 0; h < R; ++h) {
			const int r = lane + 64 * h;
			if (r < m) {
				const double l = los[col[h]], u = his[col[h]];
				double zn = whole ? zk[h] + rv[h] : fma(alpha, rv[h], zk[h]);
				const bool to_low = (r == kmin && kside == 2) || zn < l;
				const bool to_up = !to_low && ((r == kmin && kside == 3) || zn > u);
				if (to_low) { zn = l; st[col[h]] = 2; }
				if (to_up) { zn = u; st[col[h]] = 3; }
				zs[col[h]] = zn;
			}
		}
		first = false;
		++passes;
		__syncthreads();
		if (whole || passes > p) {
			inner = false;
			// a column that came straight back to the bound it left is not chosen again until the free set has changed
			const bool back = jstar >= 0 && st[jstar] == (star_low ? 2 : 3);
			__syncthreads();
			if (back) {
				if (lane == 0) blk[jstar] = 1;
			} else {
#pragma unroll
				for (int h = 0; h < R; ++h) {
					const int k = lane + 64 * h;
					if (k < p) blk[k] = 0;
				}
			}
			__syncthreads();
		}
	}
	// b = z / d, a held column exactly its bound; ssr = tss - z'(q + w); intercept from the column means
	double s_zqw = 0.0, s_bx = 0.0;
	int n_active = 0;
#pragma unroll
	for (int h = 0; h < R; ++h) {
		const int k = lane + 64 * h;
		if (k < p) {
			const int s = st[k];
			const double bj = s == 2 ? bp.lo[k] : (s == 3 ? bp.hi[k] : zs[k] / dsc[k]);
			s_zqw += zs[k] * (qv[h] + wv[h]);
			const int f = s != 0 ? bls_flags(bj, bp.lo[k], bp.hi[k], bp.tolerance) : 0;
			if (s != 0) s_bx += bj * ((icpt ? fx[k] : 0.0) + sx[k] * inv_sw);
			n_active += f != 0 ? 1 : 0;
			core[k] = s != 0 ? bj : en_nan();
			if (!pl) {
				core[p + 6 + k] = f == 1 ? 1.0 : 0.0;
				core[2 * p + 6 + k] = f == 2 ? 1.0 : 0.0;
			}
		}
	}
	for (int m = 32; m >= 1; m >>= 1) {
		s_zqw += __shfl_xor(s_zqw, m, 64);
		s_bx += __shfl_xor(s_bx, m, 64);
		n_active += __shfl_xor(n_active, m, 64);
	}
	if (lane == 0) {
		core[p] = icpt ? ymean - s_bx : en_nan();
		bls_write_stats(core, p, pl, tss - s_zqw, tss, cnt, n_active, icpt, &a.refine_list[gl]);
		if (bp.iterations) bp.iterations[g] = converged ? iters : -iters;
	}
}

// ---- ssr from the rows of the groups whose moment identity cancelled (moment_solve.h) ----
__global__ __launch_bounds__(64) void bls_rows_kernel(RowsArgs a, int pl) {
	const int lane = threadIdx.x;
	const int p = a.p;
	for (int64_t gl = blockIdx.x; gl < a.n_groups; gl += gridDim.x) {
		if (a.flag[gl] == 0) continue;
		const int64_t g = a.group_base + gl;
		double *core = a.core + g * (int64_t)(pl ? p + 6 : 3 * p + 6);
		const double b0 = a.fit_intercept ? core[p] : 0.0;
		const double ssr = rows_ssr(a, g, core, b0, lane);
		if (lane == 0) {
			if (pl) {
				const double tss = core[p + 1]; // parked by the solve
				core[p + 1] = 1.0 - ssr / tss;
				core[p + 2] = ssr;
				core[p + 3] = bls_predict_sigma(ssr, core[p + 4], p, a.fit_intercept != 0);
			} else {
				const double tss = core[p + 2];
				core[p + 1] = ssr;
				core[p + 2] = 1.0 - ssr / tss;
			}
		}
	}
}

hipError_t launch_bls_narrow(const BatchArgs &a, const BlsNarrowParams &bp, hipStream_t st) {
	return dispatch_narrow(a.p, hipErrorInvalidValue, [&](auto P) {
		hipLaunchKernelGGL((bls_solve_narrow_kernel<P()>), dim3((unsigned)((a.n_groups + 63) / 64)), dim3(64), 0, st, a, bp);
		return hipGetLastError();
	});
}

size_t bls_wide_lds_bytes(int p) { return ((size_t)p * (p + 1) + 7 * (size_t)p) * sizeof(double); }

hipError_t launch_bls_wide(const WideArgs &a, const BlsWideParams &bp, hipStream_t st) {
	// (139 264 bytes of LDS at p = 128)
	return launch_wide_r<bls_solve_wide_kernel<1>, bls_solve_wide_kernel<2>>(a, bp, bls_wide_lds_bytes(a.p), st);
}

hipError_t launch_bls_rows(const RowsArgs &ra, int predict_layout, hipStream_t st) {
	hipLaunchKernelGGL(bls_rows_kernel, dim3(rows_grid(ra.n_groups)), dim3(64), 0, st, ra, predict_layout);
	return hipGetLastError();
}

// the solve stages handed to the batch path (host_api.hip: moment_batch_device)
bool bls_narrow_stage(AnofoxHipContext *, BatchArgs &a, hipStream_t st, void *user, AnofoxError *e) {
	const BlsWideParams &bw = *static_cast<const BlsWideParams *>(user);
	BlsNarrowParams bp;
	for (int j = 0; j < kNarrowMaxP; ++j) {
		bp.lo[j] = bw.lo[j];
		bp.hi[j] = bw.hi[j];
	}
	bp.tolerance = bw.tolerance;
	bp.max_iterations = bw.max_iterations;
	bp.invalid = bw.invalid;
	bp.predict_layout = bw.predict_layout;
	bp.iterations = bw.iterations;
	if (hip_fail(launch_bls_narrow(a, bp, st), "bounded least squares solve kernel launch", e)) return false;
	if (!a.row_offsets) return true; // the records of a streaming state: no rows here, its Finalize answers the flagged groups
	return !hip_fail(launch_bls_rows(rows_args(a), bw.predict_layout, st), "bounded least squares rows kernel launch", e);
}

bool bls_wide_stage(AnofoxHipContext *, WideArgs &a, hipStream_t st, int64_t, void *user, AnofoxError *e) {
	const BlsWideParams &bw = *static_cast<const BlsWideParams *>(user);
	if (hip_fail(launch_bls_wide(a, bw, st), "bounded least squares solve kernel launch", e)) return false;
	return !hip_fail(launch_bls_rows(rows_args(a), bw.predict_layout, st), "bounded least squares rows kernel launch", e);
}

SolveStages bls_stages(BlsWideParams *bp) { return SolveStages{bls_narrow_stage, bls_wide_stage, bp}; }

// The bounds of a call per ORIGINAL column (bls.rs:148-186, 209-221): both sides absent = NNLS; otherwise an absent side is
// unbounded, one value applies to every column.  Another length, a NaN bound or lo > hi: `invalid` (status 1 everywhere).
BlsWideParams bls_params(const AnofoxHipBlsBatchOptions &o, size_t p, int predict_layout, int32_t *d_iterations) {
	BlsWideParams bp;
	memset(&bp, 0, sizeof bp);
	const bool has_lo = o.lower_bounds && o.lower_bounds_len != 0, has_hi = o.upper_bounds && o.upper_bounds_len != 0;
	bp.invalid = (has_lo && o.lower_bounds_len != 1 && o.lower_bounds_len != p) || (has_hi && o.upper_bounds_len != 1 && o.upper_bounds_len != p) ||
	             (!o.lower_bounds && o.lower_bounds_len != 0) || (!o.upper_bounds && o.upper_bounds_len != 0);
	for (size_t j = 0; j < (size_t)kWideMaxP; ++j) {
		double lo = has_lo ? -INFINITY : (has_hi ? -INFINITY : 0.0), hi = INFINITY;
		if (!bp.invalid && j < p) {
			if (has_lo) lo = o.lower_bounds_len == 1 ? o.lower_bounds[0] : o.lower_bounds[j];
			if (has_hi) hi = o.upper_bounds_len == 1 ? o.upper_bounds[0] : o.upper_bounds[j];
			if (isnan(lo) || isnan(hi) || lo > hi) bp.invalid = 1;
		}
		bp.lo[j] = lo;
		bp.hi[j] = hi;
	}
	bp.tolerance = o.tolerance;
	bp.max_iterations = o.max_iterations > 0x7fffffffu ? 0x7fffffff : (int)o.max_iterations;
	bp.predict_layout = predict_layout;
	bp.iterations = d_iterations;
	return bp;
}

bool validate_bls(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const void *off, const void *y, const double *const *x_cols,
                  const AnofoxHipBlsBatchOptions &o, const void *core, AnofoxError *e) {
	if (!ctx) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "context is NULL"); return false; }
	if (!check_batch_args(G, p, n_rows, off, y, x_cols, core, kWideMaxP, nullptr,
	                      "row_offsets, y or the record buffer is NULL", false, e))
		return false;
	if (!(o.tolerance >= 0.0)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "tolerance must be >= 0"); return false; }
	return true;
}

bool run_bls(AnofoxHipContext *ctx, int64_t G, size_t p, int64_t n_rows, const int64_t *d_off, const double *d_y, const double *const *x_cols,
             const AnofoxHipBlsBatchOptions &o, double *d_bls, int32_t *d_iterations, AnofoxError *e) {
	if (G == 0) return true;
	BlsWideParams bp = bls_params(o, p, 0, d_iterations);
	// (the stages run before this call returns: `bp` is captured by value into the kernel arguments at launch)
	return moment_batch_device(ctx, G, p, n_rows, d_off, d_y, x_cols, unweighted_moment_options(o.fit_intercept, 0.95), bls_stages(&bp), d_bls, e);
}

} // namespace

namespace anofox {
namespace host {
// the solve as a streaming state's Finalize runs it (agg_state_models.hip)
bool bls_state_options(const AnofoxHipBlsBatchOptions &o, AnofoxError *e) {
	if (!(o.tolerance >= 0.0)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "tolerance must be >= 0"); return false; }
	return true;
}
BlsParamsT<kWideMaxP> bls_state_params(const AnofoxHipBlsBatchOptions &o, size_t p) { return bls_params(o, p, 0, nullptr); }
SolveStages bls_state_stages(BlsParamsT<kWideMaxP> *bp) { return bls_stages(bp); }
} // namespace host
} // namespace anofox

extern "C" {

size_t anofox_hip_bls_record_len(size_t p) { return 3 * p + 6; }

bool anofox_hip_bls_fit_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                     const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                     AnofoxHipBlsBatchOptions options, double *d_bls, int32_t *d_iterations, AnofoxError *out_error) {
	reset_error(out_error);
	if (!validate_bls(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, options, d_bls, out_error)) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const bool ok = run_bls(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, options, d_bls, d_iterations, out_error);
	ctx->gate_wait = ctx->gate_record = nullptr; // the gate never outlives the call it was set for
	return ok;
}

bool anofox_hip_bls_fit_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                   const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                   AnofoxHipBlsBatchOptions options, double *bls, int32_t *iterations, AnofoxError *out_error) {
	reset_error(out_error);
	if (!(ctx = host_context(ctx, out_error))) return false;
	if (!validate_bls(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, options, bls, out_error)) return false;
	if (n_groups == 0) return true;
	if (!check_host_offsets(n_groups, n_rows, row_offsets, out_error)) return false;
	std::lock_guard<std::mutex> lk(ctx->mu);
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", out_error)) return false;
	const size_t p = n_features;
	return fit_slabs_host(ctx, n_groups, p, row_offsets, y, x_cols, nullptr, SlabOutputs{bls, 3 * p + 6, iterations, 1},
	                      SlabLabels{kNamedColumns, "H2D offsets", "D2H records", "D2H iterations", "D2H"}, out_error,
	                      [&](int64_t G, int64_t R, const int64_t *, const int64_t *d_off, const StagedColumns &c, double *d_rec, int32_t *d_it, double *) {
		                      return run_bls(ctx, G, p, R, d_off, c.y, c.x, options, d_rec, d_it, out_error);
	                      });
}

// A batch of one group with anofox_elasticnet_fit's conventions: argument checks first (lib.rs:3510-3522), NULL entries ->
// NaN through the validity bitmask, a one-row input padded with an all-NaN row, the reference's error texts
// (crates/anofox-stats-core/src/errors.rs), the three arrays malloc'ed.  Nothing is allocated on `false`.
bool anofox_bls_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxBlsOptions options,
                    AnofoxBlsFitResultCore *out_core, AnofoxError *out_error) {
	reset_error(out_error);
	if (!out_core) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "out_result is NULL"); return false; }
	if (!x || x_count == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (y.len == 0) { set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "Empty input: y cannot be empty"); return false; }
	if (!check_column_lengths(y.len, x, x_count, out_error)) return false;
	const size_t p = x_count;
	if (p > (size_t)kWideMaxP) {
		set_error(out_error, ANOFOX_ERROR_INVALID_INPUT, "BLS fit: more than " + std::to_string(kWideMaxP) + " features are not supported by the GPU path");
		return false;
	}
	const ScalarFitInput in(y, x, x_count);
	AnofoxHipBlsBatchOptions o;
	memset(&o, 0, sizeof o);
	o.fit_intercept = options.fit_intercept;
	o.lower_bounds = options.lower_bounds;
	o.lower_bounds_len = options.lower_bounds ? options.lower_bounds_len : 0; // lib.rs:3529: a NULL pointer is "no bounds"
	o.upper_bounds = options.upper_bounds;
	o.upper_bounds_len = options.upper_bounds ? options.upper_bounds_len : 0;
	o.max_iterations = options.max_iterations;
	o.tolerance = options.tolerance;
	std::vector<double> rec(3 * p + 6);
	if (!anofox_hip_bls_fit_batch_host(nullptr, 1, p, (int64_t)in.n_pad, in.off, in.yv.data(), in.xp.data(), o, rec.data(), nullptr, out_error)) return false;
	const int status = (int)rec[p + 5];
	if (status != ANOFOX_ERROR_SUCCESS) {
		set_scalar_fit_error(status, (AnofoxErrorCode)status, in,
		                     status == ANOFOX_ERROR_INVALID_INPUT ? "Invalid bounds: each side takes 0, 1 or n_features values, none NaN, lower <= upper"
		                                                          : "BLS fit failed on the GPU path",
		                     out_error);
		return false;
	}
	double *coef = (double *)malloc(p * sizeof(double));
	bool *at_lo = (bool *)malloc(p * sizeof(bool)), *at_hi = (bool *)malloc(p * sizeof(bool));
	if (!coef || !at_lo || !at_hi) {
		free(coef);
		free(at_lo);
		free(at_hi);
		set_error(out_error, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate coefficients");
		return false;
	}
	memcpy(coef, rec.data(), p * sizeof(double));
	for (size_t j = 0; j < p; ++j) {
		at_lo[j] = rec[p + 6 + j] != 0.0;
		at_hi[j] = rec[2 * p + 6 + j] != 0.0;
	}
	out_core->coefficients = coef;
	out_core->coefficients_len = p;
	out_core->intercept = rec[p];
	out_core->ssr = rec[p + 1];
	out_core->r_squared = rec[p + 2];
	out_core->n_observations = (size_t)rec[p + 3];
	out_core->n_features = p;
	out_core->n_active_constraints = (size_t)rec[p + 4];
	out_core->at_lower_bound = at_lo;
	out_core->at_upper_bound = at_hi;
	return true;
}

// lib.rs:3620-3640: BlsOptions::nnls() — no intercept, 1000 iterations, tolerance 1e-10, no bound arrays
bool anofox_nnls_fit(AnofoxDataArray y, const AnofoxDataArray *x, size_t x_count, AnofoxBlsFitResultCore *out_core, AnofoxError *out_error) {
	AnofoxBlsOptions o;
	memset(&o, 0, sizeof o);
	o.fit_intercept = false;
	o.max_iterations = 1000;
	o.tolerance = 1e-10;
	return anofox_bls_fit(y, x, x_count, o, out_core, out_error);
}

void anofox_free_bls_result(AnofoxBlsFitResultCore *result) {
	if (!result) return;
	free(result->coefficients);
	free(result->at_lower_bound);
	free(result->at_upper_bound);
	result->coefficients = nullptr;
	result->at_lower_bound = result->at_upper_bound = nullptr;
	result->coefficients_len = 0;
}

// ---- fit-predict (anofox_stats_bls_fit_predict_agg): the solve writes the regression layout with the reference's sigma, so
// the predict kernels apply unchanged ----

bool anofox_hip_bls_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                             const int64_t *d_row_offsets, const double *d_y, const double *const *x_cols,
                                             const int64_t *d_train_counts, AnofoxHipBlsBatchOptions options,
                                             double confidence_level, double *d_core, double *d_pred, AnofoxError *out_error) {
	reset_error(out_error);
	// (the fit entry points' argument checks and texts)
	if (!validate_bls(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, options, d_core, out_error)) return false;
	BlsWideParams bp = bls_params(options, n_features, 1, nullptr);
	return model_fit_predict_batch_device(ctx, n_groups, n_features, n_rows, d_row_offsets, d_y, x_cols, d_train_counts,
	                                      unweighted_moment_options(options.fit_intercept, confidence_level), bls_stages(&bp), d_core, d_pred, out_error);
}

bool anofox_hip_bls_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t n_features, int64_t n_rows,
                                           const int64_t *row_offsets, const double *y, const double *const *x_cols,
                                           const int64_t *train_counts, AnofoxHipBlsBatchOptions options,
                                           double confidence_level, double *core, double *pred, AnofoxError *out_error) {
	reset_error(out_error);
	if (!(ctx = host_context(ctx, out_error))) return false;
	if (!validate_bls(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, options, core, out_error)) return false;
	BlsWideParams bp = bls_params(options, n_features, 1, nullptr);
	return model_fit_predict_batch_host(ctx, n_groups, n_features, n_rows, row_offsets, y, x_cols, train_counts,
	                                    unweighted_moment_options(options.fit_intercept, confidence_level), bls_stages(&bp), core, pred, out_error);
}

} // extern "C"
