// glm_host.cpp — the GLM solver header (csrc/glm_irls.h) in its host build, where a wavefront is a loop over 64 lanes: a
// stand-alone program that tests/test_glm_cpu.py compiles under ASan / UBSan and feeds cases on stdin.
//
// stdin:  raw doubles (native byte order): n_cases, then per case
//           family fit_intercept max_iterations tolerance lambda compute_inference zq p n has_offset predict rule_count
//           n rows of  y x_1 .. x_p [offset]
// stdout: per case one line: the record (p + 11), the inference (5 p) and, with predict, mu of the n rows.
// The rows sit at an offset inside larger arrays whose other slots hold a poison value, so a read or write outside the
// group's rows shows (the scratch is checked to be untouched outside [lo, hi)).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/glm_irls.h"

using namespace anofox::glm;

static double read_double() {
	double v;
	if (fread(&v, sizeof v, 1, stdin) != 1) {
		fprintf(stderr, "ERROR: short input\n");
		exit(2);
	}
	return v;
}

int main() {
	const int n_cases = (int)read_double();
	const int64_t pad = 5;
	const double poison = -12345.678;
	for (int cs = 0; cs < n_cases; ++cs) {
		GiProblem P;
		P.family = (int)read_double();
		P.fit_intercept = (int)read_double();
		P.max_iterations = (int)read_double();
		P.tolerance = read_double();
		P.lambda = read_double();
		P.compute_inference = (int)read_double();
		P.zq = read_double();
		const int p = (int)read_double();
		const int64_t n = (int64_t)read_double();
		const int has_offset = (int)read_double(), predict = (int)read_double();
		P.rule_count = (int64_t)read_double();
		if (p < 1 || p > kGiMaxP || n < 0) {
			fprintf(stderr, "ERROR: bad case header\n");
			return 2;
		}
		const size_t N = (size_t)(n + 2 * pad);
		std::vector<double> y(N, poison), off(N, poison), eta(N, poison), mu(N, poison), pred(3 * N, poison);
		std::vector<std::vector<double>> cols((size_t)p, std::vector<double>(N, poison));
		for (int64_t i = 0; i < n; ++i) {
			y[(size_t)(pad + i)] = read_double();
			for (int j = 0; j < p; ++j) cols[(size_t)j][(size_t)(pad + i)] = read_double();
			if (has_offset) off[(size_t)(pad + i)] = read_double();
		}
		std::vector<const double *> xp((size_t)p);
		for (int j = 0; j < p; ++j) xp[(size_t)j] = cols[(size_t)j].data();
		P.y = y.data();
		P.x = xp.data();
		P.offset = has_offset ? off.data() : nullptr;
		P.p = p;
		P.lo = pad;
		P.hi = pad + n;
		P.eta = eta.data();
		P.mu = mu.data();
		const int k = p + (P.fit_intercept ? 1 : 0);
		std::vector<double> work(gi_work_doubles(k), poison), rec((size_t)p + 11, poison), inf(5 * (size_t)p, poison);
		const bool invalid = !(P.tolerance > 0.0) || !(P.tolerance <= DBL_MAX) || !(P.lambda >= 0.0) || !(P.lambda <= DBL_MAX) ||
		                     P.max_iterations <= 0 || (P.family != kGiFamilyPoisson && P.family != kGiFamilyBinomial);
		switch (gi_entry_class(k)) {
		case 1: gi_fit<1>(P, invalid, work.data(), rec.data(), inf.data(), predict ? pred.data() : nullptr); break;
		case 4: gi_fit<4>(P, invalid, work.data(), rec.data(), inf.data(), predict ? pred.data() : nullptr); break;
		default: gi_fit<10>(P, invalid, work.data(), rec.data(), inf.data(), predict ? pred.data() : nullptr); break;
		}
		for (int64_t i = 0; i < (int64_t)N; ++i) {
			const bool inside = i >= pad && i < pad + n;
			if (!inside && (eta[(size_t)i] != poison || mu[(size_t)i] != poison || pred[3 * (size_t)i] != poison)) {
				fprintf(stderr, "ERROR: a slot outside the group's rows was written (case %d, slot %lld)\n", cs, (long long)i);
				return 3;
			}
		}
		for (double v : rec) printf("%.17g ", v);
		for (double v : inf) printf("%.17g ", v);
		if (predict)
			for (int64_t i = 0; i < n; ++i) {
				if (pred[3 * (size_t)(pad + i) + 1] == pred[3 * (size_t)(pad + i) + 1] || pred[3 * (size_t)(pad + i) + 2] == pred[3 * (size_t)(pad + i) + 2]) {
					fprintf(stderr, "ERROR: an interval bound is not NaN (case %d)\n", cs);
					return 3;
				}
				printf("%.17g ", pred[3 * (size_t)(pad + i)]);
			}
		printf("\n");
	}
	return 0;
}
