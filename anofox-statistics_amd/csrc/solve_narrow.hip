// solve_narrow.hip — per-group solve and diagnostics (p <= 8), one lane per group.
//
// Consumes the moment records of accumulate_narrow.hip and produces the reference's result STRUCT fields
// (src/aggregate_functions/ols_aggregate.cpp:74-96) as dense records.  Restates, per group:
//   - the model's pre-checks and shortcuts: crates/anofox-stats-core/src/models/ols.rs:68-139,
//     ridge.rs:38-40,104-146, wls.rs:119-157
//   - the regressor (anofox-regression OlsRegressor / RidgeRegressor / WlsRegressor, call sites
//     ols.rs:155-161, ridge.rs:156-164, wls.rs:174-182): here a Cholesky factorisation of the centred
//     (shifted) moment matrix with aliased-pivot detection, two triangular solves, and the closed forms for
//     R^2, adjusted R^2, sigma, SE, t, p, CI and F
//   - NaN re-expansion at dropped columns: ols.rs:167-171,191-206
//
// Normal equations square the condition number, and RSS = Syy - b'Sxy cancels when R^2 -> 1.  Groups where
// either matters (smallest Cholesky pivot ratio < 1e-3, or RSS/TSS < 1e-7) are queued on the device; for
// those groups only, refine_fused_kernel re-reads the rows (one wavefront per queued group) and forms the
// residuals r = y - b0 - x'b, their weighted sum of squares and the gradient X'Wr directly from the data, and
// the solve runs again in
//   MODE 1: one step of iterative refinement  b += (X'WX)^-1 X'Wr   (twice), then
//   MODE 2: final statistics from the directly summed RSS.
// This restores the accuracy of a QR on the design (the reference's algorithm class) for the queued groups.
#include "common.h"
#include "device_math.h"
#include "dd_arith.h"
#include "solve_narrow_impl.h"

namespace anofox {

static_assert(sizeof(TcritSlot) * kTcritSlots == kTcritTableBytes, "t memo does not fill its workspace slice");

namespace {

template <int P>
__global__ __launch_bounds__(64) void solve_narrow_kernel(BatchArgs args) {
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= args.n_groups) return;
	solve_one<P, MODE_PRIMARY>(args, g, args.moments + g * (int64_t)MomentLayout<P>::REC, args.core + g * (int64_t)(P + 6));
}

// One wavefront per queued group, straight from the data with the record's current coefficients:
//   refine_vec[g] = { sum w r^2, sum w r, sum w r (x_j - shift_j) ..., sum w (y - ybar)^2 },  r = y - b0 - x'b
// over the valid rows (same row filter as the accumulate kernel); shift = first valid row when an intercept
// is fitted (the shift of the moment record), 0 otherwise.  The residual and the gradient sums are formed in
// double-double arithmetic (dd_arith.h), as on the wide path: with the residual in working precision the update stalls
// at cond(X) eps — designs without an intercept whose columns sit far from zero reach cond 1e7 at p <= 8 (3 of 240 000
// cases of the deep narrow sweep were 1.5 .. 2.5e-9 off).  Only queued groups pay for it.
__device__ __forceinline__ void residual_grad_wave(const BatchArgs &args, int64_t g, int lane) {
#pragma clang fp contract(off)
	const int p = args.p;
	const bool weighted = args.model == ANOFOX_HIP_MODEL_WLS;
	const int Z = p + 1;
	const int off_first = Z + Z * (Z + 1) / 2 + 1;
	const int rec_len = moment_record_len(p);
	const double *core = args.core + g * (int64_t)(p + 6);
	const double *rec = args.moments + g * (int64_t)rec_len;
	// acc: [0] sum w r, [1 + j] sum w r (x_j - shift_j), as (hi, lo) pairs; rss and the centred yy in working precision
	double b[kNarrowMaxP], sh[kNarrowMaxP], acc_h[kNarrowMaxP + 1], acc_l[kNarrowMaxP + 1];
	// mean of y over the valid rows, from the record (sum / weight, plus the shift an intercept fit accumulates about)
	const double ybar = rec[p] / rec[Z + Z * (Z + 1) / 2] + (args.fit_intercept ? rec[off_first + p] : 0.0);
#pragma unroll
	for (int j = 0; j < kNarrowMaxP; ++j) {
		b[j] = sh[j] = 0.0;
		if (j < p) {
			const double bj = core[j];
			b[j] = isnan(bj) ? 0.0 : bj; // dropped / aliased columns do not enter the fit
			sh[j] = args.fit_intercept ? rec[off_first + j] : 0.0;
		}
	}
#pragma unroll
	for (int k = 0; k < kNarrowMaxP + 1; ++k) acc_h[k] = acc_l[k] = 0.0;
	double rss = 0.0, cyy = 0.0;
	const double b0 = args.fit_intercept ? core[p] : 0.0;
	const int64_t lo = args.row_offsets[g], hi = group_row_end(args, g);
	for (int64_t r = lo + lane; r < hi; r += 64) {
		const double yv = args.y[r];
		bool ok = isfinite(yv);
		double fh = b0, fl = 0.0; // fit = fh + fl
		double xv[kNarrowMaxP];
#pragma unroll
		for (int j = 0; j < kNarrowMaxP; ++j) {
			xv[j] = 0.0;
			if (j < p) {
				xv[j] = args.x[j][r];
				ok = ok && isfinite(xv[j]);
				dd_fit_term(fh, fl, b[j], xv[j]);
			}
		}
		double wv = 1.0;
		if (weighted) {
			wv = args.w[r];
			ok = ok && (wv > 0.0) && isfinite(wv);
		}
		if (ok) {
			double e, wh, wl;
			dd_weighted_residual(yv, fh, fl, wv, e, wh, wl); // wh + wl = w (y - fit) to twice the working precision
			rss = fma(wh, e, rss);
			dd_add(acc_h[0], acc_l[0], wh, wl);
#pragma unroll
			for (int j = 0; j < kNarrowMaxP; ++j)
				if (j < p) dd_add_scaled_diff(acc_h[1 + j], acc_l[1 + j], wh, wl, xv[j], sh[j]);
			const double dy = yv - ybar;
			cyy = fma(wv * dy, dy, cyy);
		}
	}
	for (int m = 32; m >= 1; m >>= 1) {
		rss += __shfl_xor(rss, m, 64);
		cyy += __shfl_xor(cyy, m, 64);
#pragma unroll
		for (int k = 0; k < kNarrowMaxP + 1; ++k)
			if (k < p + 1) dd_add(acc_h[k], acc_l[k], __shfl_xor(acc_h[k], m, 64), __shfl_xor(acc_l[k], m, 64));
	}
	double *out = args.refine_vec + g * (int64_t)refine_vec_len(p);
	double mine = rss;
#pragma unroll
	for (int k = 0; k < kNarrowMaxP + 1; ++k) mine = (lane == 1 + k) ? acc_h[k] + acc_l[k] : mine;
	if (lane == p + 2) mine = cyy;
	if (lane < p + 3) out[lane] = mine;
}

// The whole refinement of the queued groups in ONE launch: a wavefront takes a queued group through
//   kRefineSteps x (residual + gradient pass over its rows, iterative-refinement update)  and the final
//   residual pass + statistics,
// the row passes on all 64 lanes, the small solves on lane 0.  Groups are independent, so nothing has to be
// synchronised across waves; six dependent launches (~35 us of dispatch latency each on an otherwise empty
// queue) become one.
template <int P>
__global__ __launch_bounds__(64) void refine_fused_kernel(BatchArgs args, int steps) {
	const int lane = threadIdx.x & 63;
	const int n = *args.refine_count;
	for (int i = blockIdx.x; i < n; i += gridDim.x) {
		const int64_t g = args.refine_list[i];
		for (int it = 0; it <= steps; ++it) {
			// Producer and consumer are lanes of the SAME wavefront: a workgroup-scope fence orders the stores before the
			// loads without the agent-scope L2 write-back / invalidate of __threadfence(), which costs microseconds when
			// the L2 is full of another kernel's dirty lines (7 801 queued window frames: 0.89 ms -> measured below)
			residual_grad_wave(args, g, lane);
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); // refine_vec[g] written by lanes 0..p+2, read by lane 0
			if (lane == 0) {
				const double *rec = args.moments + g * (int64_t)MomentLayout<P>::REC;
				double *core = args.core + g * (int64_t)(P + 6);
				if (it < steps) solve_one<P, MODE_UPDATE>(args, g, rec, core);
				else solve_one<P, MODE_FINAL>(args, g, rec, core);
			}
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); // the record's coefficients written by lane 0, read by every lane in the next pass
		}
	}
}

template <int P>
hipError_t launch_solve_p(const BatchArgs &a, hipStream_t stream) {
	const unsigned grid = (unsigned)((a.n_groups + 63) / 64);
	hipLaunchKernelGGL((solve_narrow_kernel<P>), dim3(grid), dim3(64), 0, stream, a);
	return hipGetLastError();
}

} // namespace

hipError_t launch_solve_narrow(const BatchArgs &a, hipStream_t stream) {
	if (a.n_groups <= 0) return hipSuccess;
	return dispatch_narrow(a.p, hipErrorInvalidValue, [&](auto P) { return launch_solve_p<P()>(a, stream); });
}

template <int P>
hipError_t launch_refine_p(const BatchArgs &a, int steps, hipStream_t stream) {
	// one wavefront per queued group and trip: the grid covers small batches entirely (the refits of flagged window
	// frames queue nearly every group of theirs: 7 801 groups on 1 024 wavefronts took 0.9 ms, eight groups in a row each)
	const unsigned grid = a.n_groups < 1024 ? 1024u : (a.n_groups > 16384 ? 16384u : (unsigned)a.n_groups);
	hipLaunchKernelGGL((refine_fused_kernel<P>), dim3(grid), dim3(64), 0, stream, a, steps);
	return hipGetLastError();
}

hipError_t launch_refine_fused_narrow(const BatchArgs &a, int steps, hipStream_t stream) {
	if (a.n_groups <= 0) return hipSuccess;
	return dispatch_narrow(a.p, hipErrorInvalidValue, [&](auto P) { return launch_refine_p<P()>(a, steps, stream); });
}

} // namespace anofox
