// The one-group scaffolding (csrc/scalar_fit.h) and the batch argument check (csrc/context.h) as a program of its own:
// tests/test_scalar_fit_cpu.py compiles it with g++ under ASan / UBSan (no device code, no GPU) and reads what it prints.
#include <stdio.h>

#include "../../anofox-statistics_amd/csrc/scalar_fit.h"

using namespace anofox::host;

int main() {
	AnofoxError e;
	// three rows, the second y NULL through the validity mask, a NaN in the second column; then a one-row input (padded)
	double yd[3] = {1.0, 2.0, 3.0}, x0[3] = {0.5, 1.5, 2.5}, x1[3] = {4.0, 5.0, NAN}, wd[3] = {1.0, 0.0, 2.0};
	uint8_t yvalid = 0x5;
	AnofoxDataArray y{yd, &yvalid, 3}, xs[2] = {{x0, nullptr, 3}, {x1, nullptr, 3}}, w{wd, nullptr, 3};
	const ScalarFitInput in(y, xs, 2);
	printf("input %zu %zu %zu %lld %lld nan=%d valid=%zu w=%d\n", in.p, in.n, in.n_pad, (long long)in.off[0], (long long)in.off[1],
	       (int)isnan(in.yv[1]), in.n_valid(), in.w() != nullptr);
	const ScalarFitInput inw(y, xs, 2, &w);
	printf("weighted valid=%zu w=%d\n", inw.n_valid(), inw.w() != nullptr);
	AnofoxDataArray y1{yd, nullptr, 1}, xs1[1] = {{x0, nullptr, 1}};
	const ScalarFitInput one(y1, xs1, 1);
	printf("one %zu %zu %lld len=%zu pad_nan=%d %d xp=%d\n", one.n, one.n_pad, (long long)one.off[1], one.yv.size(), (int)isnan(one.yv[1]),
	       (int)isnan(one.cols[0][1]), one.xp[0] == one.cols[0].data());
	for (int status : {ANOFOX_ERROR_NO_VALID_DATA, ANOFOX_ERROR_INSUFFICIENT_DATA, ANOFOX_ERROR_INVALID_INPUT}) {
		reset_error(&e);
		set_scalar_fit_error(status, (AnofoxErrorCode)status, in, "Some fit failed on the GPU path", &e);
		printf("status %d -> %d %s\n", status, (int)e.code, e.message);
	}
	AnofoxDataArray bad[2] = {{x0, nullptr, 3}, {x1, nullptr, 2}};
	reset_error(&e);
	const bool same = check_column_lengths(3, xs, 2, &e), shorter = check_column_lengths(3, bad, 2, &e);
	printf("lengths %d %d -> %d %s\n", (int)same, (int)shorter, (int)e.code, e.message);
	double core[8] = {0.25, -0.5, 1.0, 0.9, 0.8, 0.1, 3.0, 0.0};
	AnofoxFitResultCore r;
	if (!fill_scalar_result(core, 2, &r, &e)) return 1;
	printf("result %g %g %zu %g %g %g %g %zu %zu\n", r.coefficients[0], r.coefficients[1], r.coefficients_len, r.intercept, r.r_squared,
	       r.adj_r_squared, r.residual_std_error, r.n_observations, r.n_features);
	free(r.coefficients);
	// check_batch_args: the order of the checks, both forms
	const double *cols[2] = {x0, nullptr};
	const int64_t off[2] = {0, 3};
	struct { int64_t G; size_t p; int64_t n; const void *off, *y; const double *const *x; const void *out; bool by_rows; } calls[] = {
	    {-1, 0, 3, off, yd, cols, yd, false}, {1, 0, 3, nullptr, yd, cols, yd, false}, {1, 3, 3, nullptr, yd, cols, yd, false},
	    {1, 2, 3, nullptr, yd, cols, yd, false}, {1, 2, 3, off, yd, cols, yd, false}, {0, 2, 3, nullptr, nullptr, cols, nullptr, false},
	    {-1, 2, 3, nullptr, yd, cols, yd, true}, {-1, 2, 3, nullptr, yd, cols, nullptr, true}, {-1, 2, 0, nullptr, nullptr, cols, nullptr, true},
	    {0, 2, -1, nullptr, nullptr, cols, nullptr, true}};
	for (const auto &c : calls) {
		reset_error(&e);
		const bool ok = check_batch_args(c.G, c.p, c.n, c.off, c.y, c.x, c.out, 2, nullptr, "an array is NULL", c.by_rows, &e);
		printf("args %d %d %s\n", (int)ok, (int)e.code, e.message);
	}
	printf("fmt %s %s\n", fmt_g(-1.0).c_str(), fmt_g(1.5).c_str());
	return 0;
}
