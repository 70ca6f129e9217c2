// Host build of rls_filter.h (tests/test_rls_cpu.py): reads cases from a binary file, fits each with rls_fit_range<128>, writes
// the records.  Compiled with -ffp-contract=off, so the host arithmetic is the filter's IEEE operation order.
// Input, per case: int32 p, int32 fit_intercept, int64 n, double lambda, double delta, y[n], x[p][n] (column-major).
// Output, per case: the record (p + 6 doubles).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rls_filter.h"

int main(int argc, char **argv) {
	if (argc != 3) return 2;
	FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
	if (!in || !out) return 2;
	for (;;) {
		int32_t p, icpt;
		int64_t n;
		double lam, delta;
		if (fread(&p, 4, 1, in) != 1) break;
		if (fread(&icpt, 4, 1, in) != 1 || fread(&n, 8, 1, in) != 1 || fread(&lam, 8, 1, in) != 1 || fread(&delta, 8, 1, in) != 1) return 3;
		if (p < 1 || p > 128 || n < 0) return 4;
		std::vector<double> y((size_t)n), x((size_t)n * p);
		if (fread(y.data(), 8, (size_t)n, in) != (size_t)n || fread(x.data(), 8, (size_t)n * p, in) != (size_t)n * p) return 3;
		std::vector<const double *> cols((size_t)p);
		for (int j = 0; j < p; ++j) cols[(size_t)j] = x.data() + (size_t)j * n;
		std::vector<double> rec((size_t)p + 6);
		anofox::rls::RlsParams o{lam, delta, icpt};
		anofox::rls::rls_fit_range<128>(y.data(), cols.data(), p, 0, n, o, rec.data());
		fwrite(rec.data(), 8, rec.size(), out);
	}
	fclose(out);
	fclose(in);
	printf("ok\n");
	return 0;
}
