// quantile_window_host.cpp — qs_fit_window of csrc/quantile_solve.h compiled as plain C++ (one "lane") behind a main(): reads
// partitions with their frames on stdin, prints one line per output row.  Built by tests/test_quantile_window_cpu.py with
// -fsanitize=address,undefined; never loaded into python.
//
// stdin, per case:   p fit_intercept tau n max_iterations run_length      (run_length 0: the partition is one run)
//                    n lines of:  lo hi y x_1 .. x_p                      (the frame [lo, hi) of the row; nan / inf as strtod reads them)
// stdout, per row:   the walk's p + 6 record values (%.17g), its signed pivot count, 1 if the frame ran begin (plus twice the run's
//                    restart count on the first row of a run), yhat; then the
//                    p + 6 record values and the signed pivot count of a cold qs_fit of the same frame.
// The partition is cut into runs of run_length output rows.  Every run gets a slab of exactly the rows the planner's bound
// gives it (the longest chain of consecutive frames with non-decreasing, overlapping bounds), filled with stale values, so that a slot outside the bound is an
// address error and a read of a stale slot changes the output.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/quantile_solve.h"

using namespace anofox::quantile;

int main() {
	int p, icpt, max_it;
	long long n, run_length;
	double tau;
	while (scanf("%d %d %lf %lld %d %lld", &p, &icpt, &tau, &n, &max_it, &run_length) == 6) {
		if (p < 1 || p > kQsMaxP || n < 0 || run_length < 0) return 2;
		std::vector<int64_t> lo((size_t)n), hi((size_t)n);
		std::vector<double> y((size_t)n);
		std::vector<std::vector<double>> cols((size_t)p, std::vector<double>((size_t)n));
		for (long long i = 0; i < n; ++i) {
			long long a, b;
			if (scanf("%lld %lld %lf", &a, &b, &y[(size_t)i]) != 3) return 2;
			if (b > a && (a < 0 || b > n)) return 2;
			lo[(size_t)i] = a;
			hi[(size_t)i] = b;
			for (int j = 0; j < p; ++j)
				if (scanf("%lf", &cols[(size_t)j][(size_t)i]) != 1) return 2;
		}
		std::vector<const double *> xp((size_t)p);
		for (int j = 0; j < p; ++j) xp[(size_t)j] = cols[(size_t)j].data();
		const int k = p + (icpt ? 1 : 0);
		const bool invalid = !(tau > 0.0 && tau < 1.0);
		std::vector<double> work(qs_work_doubles(k)), pred(3 * (size_t)n), rec((size_t)n * (p + 6));
		std::vector<int32_t> its((size_t)n);
		std::vector<uint8_t> cold((size_t)n);
		const long long L = run_length > 0 ? run_length : (n > 0 ? n : 1);
		std::vector<int64_t> restarts((size_t)(n / L + 1), 0);
		for (long long e0 = 0; e0 < n; e0 += L) {
			const long long e1 = e0 + L < n ? e0 + L : n;
			int64_t slab = 0, origin = 0, plo = 0, phi = 0; // the planner's bound: the longest chain of monotone, overlapping frames
			bool have = false;
			for (long long e = e0; e < e1; ++e) {
				const int64_t a = lo[(size_t)e], b = hi[(size_t)e];
				if (b <= a) { have = false; continue; }
				if (!(have && a >= plo && b >= phi && a < phi)) origin = a;
				have = true;
				plo = a;
				phi = b;
				slab = phi - origin > slab ? phi - origin : slab;
			}
			std::vector<double> r((size_t)slab), z((size_t)slab), t((size_t)slab);
			for (int64_t i = 0; i < slab; ++i) {
				r[(size_t)i] = 1.0 + (double)(i % 7);
				z[(size_t)i] = 0.5 + (double)(i % 3);
				t[(size_t)i] = 1e-3 * (double)(1 + i % 5);
			}
			for (double &w : work) w = 3.25;
			QsProblem P;
			P.y = y.data();
			P.x = xp.data();
			P.p = p;
			P.fit_intercept = icpt;
			P.lo = P.hi = 0;
			P.rule_count = 0;
			P.tau = tau;
			P.max_iterations = max_it;
			P.predict_layout = 0;
			P.r = r.data();
			P.z = z.data();
			P.t = t.data();
			qs_fit_window(P, invalid, lo.data(), hi.data(), e0, e1, slab, work.data(), pred.data(), rec.data(), its.data(), cold.data(), &restarts[(size_t)(e0 / L)]);
		}
		// the cold fit of every frame, on scratch indexed by the row number (origin 0)
		std::vector<double> r((size_t)n), z((size_t)n), t((size_t)n), crec((size_t)p + 6);
		for (long long e = 0; e < n; ++e) {
			for (int j = 0; j < p + 6; ++j) printf("%.17g ", rec[(size_t)e * (p + 6) + j]);
			printf("%d %d %.17g ", its[(size_t)e], (int)cold[(size_t)e] + (e % L == 0 ? 2 * (int)restarts[(size_t)(e / L)] : 0), pred[3 * (size_t)e]);
			if (!(pred[3 * (size_t)e + 1] != pred[3 * (size_t)e + 1]) || !(pred[3 * (size_t)e + 2] != pred[3 * (size_t)e + 2])) {
				fprintf(stderr, "ERROR: the bounds of row %lld are not NaN\n", e);
				return 3;
			}
			QsProblem P;
			P.y = y.data();
			P.x = xp.data();
			P.p = p;
			P.fit_intercept = icpt;
			P.lo = lo[(size_t)e];
			P.hi = hi[(size_t)e] > lo[(size_t)e] ? hi[(size_t)e] : lo[(size_t)e];
			P.rule_count = 0;
			for (int64_t i = P.lo; i < P.hi; ++i) P.rule_count += y[(size_t)i] == y[(size_t)i] ? 1 : 0;
			P.tau = tau;
			P.max_iterations = max_it;
			P.predict_layout = 0;
			P.r = r.data();
			P.z = z.data();
			P.t = t.data();
			int32_t cits = 0;
			qs_fit(P, invalid, work.data(), crec.data(), &cits);
			for (int j = 0; j < p + 6; ++j) printf("%.17g ", crec[(size_t)j]);
			printf("%d\n", cits);
		}
	}
	return 0;
}
