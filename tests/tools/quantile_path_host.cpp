// quantile_path_host.cpp — the tau path of csrc/quantile_solve.h (qs_order_taus + qs_fit_path) compiled as plain C++ (one
// "lane") behind a main(): reads cases on stdin, prints one line per tau of each case.  Built by
// tests/test_quantile_path_cpu.py with -fsanitize=address,undefined; never loaded into python.
//
// stdin, per case:   p fit_intercept n_taus n max_iterations rule_count
//                    one line of the n_taus values of tau, in the caller's order (nan / inf as strtod reads them)
//                    n lines of:  y x_1 .. x_p
// stdout, per case:  n_taus lines in the caller's order: the p + 6 record values (%.17g), the signed pivot count, then the n
//                    fused predictions of that tau.  Every case is fitted twice, the second time on scratch filled with stale
//                    values; differing bytes end the program with status 3.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/quantile_solve.h"

using namespace anofox::quantile;

int main() {
	int p, icpt, n_taus, max_it;
	long long n, rule;
	while (scanf("%d %d %d %lld %d %lld", &p, &icpt, &n_taus, &n, &max_it, &rule) == 6) {
		if (p < 1 || n < 0 || n_taus < 0) return 2;
		std::vector<double> taus((size_t)n_taus);
		for (int t = 0; t < n_taus; ++t)
			if (scanf("%lf", &taus[(size_t)t]) != 1) return 2;
		std::vector<double> y((size_t)n);
		std::vector<std::vector<double>> cols((size_t)p, std::vector<double>((size_t)n));
		for (long long i = 0; i < n; ++i) {
			if (scanf("%lf", &y[(size_t)i]) != 1) return 2;
			for (int j = 0; j < p; ++j)
				if (scanf("%lf", &cols[(size_t)j][(size_t)i]) != 1) return 2;
		}
		if (p > kQsMaxP) {
			printf("error: n_features > 32\n");
			continue;
		}
		if (n_taus < 1 || n_taus > kQsMaxTaus) {
			printf("error: n_taus outside 1 .. 64\n");
			continue;
		}
		std::vector<const double *> xp((size_t)p);
		for (int j = 0; j < p; ++j) xp[(size_t)j] = cols[(size_t)j].data();
		const size_t T = (size_t)n_taus, len = (size_t)p + 6;
		std::vector<double> r((size_t)n), z((size_t)n), t((size_t)n);
		std::vector<double> rec(T * len), rec2(T * len), pred((size_t)n * T), pred2((size_t)n * T);
		std::vector<int32_t> its(T), its2(T);
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
		P.tau = NAN; // not read by the path
		P.max_iterations = max_it;
		P.predict_layout = 0;
		P.r = r.data();
		P.z = z.data();
		P.t = t.data();
		double sorted[kQsMaxTaus];
		uint8_t slot[kQsMaxTaus];
		const int n_ok = qs_order_taus(taus.data(), n_taus, sorted, slot);
		qs_fit_path(P, sorted, slot, n_ok, n_taus, work.data(), rec.data(), its.data(), pred.data());
		// again with the scratch and the work memory as an earlier call of any kind may have left them
		for (long long i = 0; i < n; ++i) {
			r[(size_t)i] = 1.0 + (double)(i % 7);
			z[(size_t)i] = 0.5 + (double)(i % 3);
			t[(size_t)i] = 1e-3 * (double)(1 + i % 5);
		}
		for (double &w : work) w = 3.25;
		qs_fit_path(P, sorted, slot, n_ok, n_taus, work.data(), rec2.data(), its2.data(), pred2.data());
		if (memcmp(its.data(), its2.data(), T * sizeof(int32_t)) != 0 || memcmp(rec.data(), rec2.data(), rec.size() * sizeof(double)) != 0 ||
		    (!pred.empty() && memcmp(pred.data(), pred2.data(), pred.size() * sizeof(double)) != 0)) { // (a group of no rows: no bytes)
			fprintf(stderr, "ERROR: the path depends on the contents of its scratch\n");
			return 3;
		}
		for (size_t tt = 0; tt < T; ++tt) {
			for (size_t j = 0; j < len; ++j) printf("%.17g ", rec[tt * len + j]);
			printf("%d", its[tt]);
			for (long long i = 0; i < n; ++i) printf(" %.17g", pred[(size_t)i * T + tt]);
			printf("\n");
		}
	}
	return 0;
}
