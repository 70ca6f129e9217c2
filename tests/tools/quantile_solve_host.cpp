// quantile_solve_host.cpp — csrc/quantile_solve.h compiled as plain C++ (one "lane") behind a main(): reads cases on stdin,
// prints one record per case.  Built by tests/test_quantile_cpu.py with -fsanitize=address,undefined; never loaded into python.
//
// stdin, per case:   p fit_intercept tau n max_iterations rule_count
//                    n lines of:  y x_1 .. x_p      (nan / inf as strtod reads them)
// stdout, per case:  the p + 6 record values (%.17g) and the signed pivot count, on one line.  Every case is fitted twice, the
//                    second time on scratch filled with stale values; differing bytes end the program with status 3.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/quantile_solve.h"

using namespace anofox::quantile;

int main() {
	int p, icpt, max_it;
	long long n, rule;
	double tau;
	while (scanf("%d %d %lf %lld %d %lld", &p, &icpt, &tau, &n, &max_it, &rule) == 6) {
		if (p < 1 || n < 0) return 2;
		std::vector<double> y((size_t)n);
		std::vector<std::vector<double>> cols((size_t)p, std::vector<double>((size_t)n));
		for (long long i = 0; i < n; ++i) {
			if (scanf("%lf", &y[(size_t)i]) != 1) return 2;
			for (int j = 0; j < p; ++j)
				if (scanf("%lf", &cols[(size_t)j][(size_t)i]) != 1) return 2;
		}
		std::vector<const double *> xp((size_t)p);
		for (int j = 0; j < p; ++j) xp[(size_t)j] = cols[(size_t)j].data();
		std::vector<double> r((size_t)n), z((size_t)n), t((size_t)n), rec((size_t)p + 6), rec2((size_t)p + 6);
		int32_t its = 0, its2 = 0;
		if (p > kQsMaxP) {
			printf("error: n_features > 32\n");
			continue;
		}
		const int k = p + (icpt ? 1 : 0);
		std::vector<double> work(qs_work_doubles(k));
		QsProblem P;
		P.y = y.data();
		P.x = xp.data();
		P.p = p;
		P.fit_intercept = icpt;
		P.lo = 0;
		P.hi = n;
		P.rule_count = rule;
		P.tau = tau;
		P.max_iterations = max_it;
		P.predict_layout = 0;
		P.r = r.data();
		P.z = z.data();
		P.t = t.data();
		const bool invalid = !(tau > 0.0 && tau < 1.0);
		qs_fit(P, invalid, work.data(), rec.data(), &its);
		// again with the scratch and the work memory as an earlier call of any kind may have left them (positive values look
		// like breakpoints): the record and the pivot count must come back with the same bytes
		for (long long i = 0; i < n; ++i) {
			r[(size_t)i] = 1.0 + (double)(i % 7);
			z[(size_t)i] = 0.5 + (double)(i % 3);
			t[(size_t)i] = 1e-3 * (double)(1 + i % 5);
		}
		for (double &w : work) w = 3.25;
		qs_fit(P, invalid, work.data(), rec2.data(), &its2);
		if (its != its2 || memcmp(rec.data(), rec2.data(), rec.size() * sizeof(double)) != 0) {
			fprintf(stderr, "ERROR: the fit depends on the contents of its scratch (pivots %d vs %d)\n", its, its2);
			return 3;
		}
		for (int j = 0; j < p + 6; ++j) printf("%.17g ", rec[(size_t)j]);
		printf("%d\n", its);
	}
	return 0;
}
