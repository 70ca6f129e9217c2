// glm_extras_host.cpp — the interval and the accuracy of the GLM solver header (csrc/glm_irls.h) in its host build, where a
// wavefront is a loop over 64 lanes: a stand-alone program that tests/test_glm_extras_cpu.py compiles under ASan / UBSan and
// feeds cases on stdin (tests/glm_extras_cases.py writes them).
//
// stdin:  raw doubles (native byte order): n_cases, then per case
//           family fit_intercept max_iterations tolerance lambda p n has_offset predict rule_count interval_z threshold want_accuracy
//           n rows of  y x_1 .. x_p [offset]
// stdout: per case one line: the record (p + 11), the accuracy (nan when it was not asked for) and, with predict, the n rows of
//         pred = {mu, lower, upper}.
// The rows sit at an offset inside larger arrays whose other slots hold a poison value, and the accuracy between two poisoned
// neighbours, so a write outside the group's own slots shows.
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
		P.compute_inference = 0;
		P.zq = NAN;
		const int p = (int)read_double();
		const int64_t n = (int64_t)read_double();
		const int has_offset = (int)read_double(), predict = (int)read_double();
		P.rule_count = (int64_t)read_double();
		P.interval_z = read_double();
		P.threshold = read_double();
		const int want_accuracy = (int)read_double();
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
		double acc[3] = {poison, poison, poison};
		P.y = y.data();
		P.x = xp.data();
		P.offset = has_offset ? off.data() : nullptr;
		P.p = p;
		P.lo = pad;
		P.hi = pad + n;
		P.eta = eta.data();
		P.mu = mu.data();
		P.accuracy = want_accuracy ? &acc[1] : nullptr;
		const int k = p + (P.fit_intercept ? 1 : 0);
		std::vector<double> work(gi_work_doubles(k), poison), rec((size_t)p + 11, poison);
		const bool invalid = !(P.tolerance > 0.0) || !(P.tolerance <= DBL_MAX) || !(P.lambda >= 0.0) || !(P.lambda <= DBL_MAX) ||
		                     P.max_iterations <= 0 || (P.family != kGiFamilyPoisson && P.family != kGiFamilyBinomial);
		switch (gi_entry_class(k)) {
		case 1: gi_fit<1>(P, invalid, work.data(), rec.data(), nullptr, predict ? pred.data() : nullptr); break;
		case 4: gi_fit<4>(P, invalid, work.data(), rec.data(), nullptr, predict ? pred.data() : nullptr); break;
		default: gi_fit<10>(P, invalid, work.data(), rec.data(), nullptr, predict ? pred.data() : nullptr); break;
		}
		for (int64_t i = 0; i < (int64_t)N; ++i) {
			const bool inside = i >= pad && i < pad + n;
			const size_t s = (size_t)i;
			if (!inside && (eta[s] != poison || mu[s] != poison || pred[3 * s] != poison || pred[3 * s + 1] != poison || pred[3 * s + 2] != poison)) {
				fprintf(stderr, "ERROR: a slot outside the group's rows was written (case %d, slot %lld)\n", cs, (long long)i);
				return 3;
			}
		}
		if (acc[0] != poison || acc[2] != poison || (!want_accuracy && acc[1] != poison)) {
			fprintf(stderr, "ERROR: the accuracy was written outside its slot (case %d)\n", cs);
			return 3;
		}
		for (double v : rec) printf("%.17g ", v);
		printf("%.17g ", want_accuracy ? acc[1] : (double)NAN);
		if (predict)
			for (int64_t i = 0; i < 3 * n; ++i) printf("%.17g ", pred[3 * (size_t)pad + (size_t)i]);
		printf("\n");
	}
	return 0;
}
