// aft_predict_host.cpp — the AFT solver header (csrc/aft_newton.h) in its host build WITH the prediction pass (an_predict): a
// stand-alone program that tests/test_aft_predict_cpu.py compiles under ASan / UBSan and feeds cases on stdin.
//
// stdin:  raw doubles (native byte order): n_cases, then per case
//           dist fit_intercept max_iterations tolerance compute_inference zq wq horizon p n
//           n rows of  time event x_1 .. x_p
// stdout: per case one line: the record (p + 13), the inference (5 p + 2), the same two from a run of the same case WITHOUT the
//         pass (P.pred == nullptr), and the n x 4 predictions.
// The rows sit at an offset inside larger arrays whose other slots hold a poison value: the program fails when the pass wrote a
// prediction slot outside the group's rows or left one of the group's own unwritten.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/aft_newton.h"

using namespace anofox::aft;

static double read_double() {
	double v;
	if (fread(&v, sizeof v, 1, stdin) != 1) {
		fprintf(stderr, "ERROR: short input\n");
		exit(2);
	}
	return v;
}

static void fit(const AnProblem &P, bool invalid, int k, double *work, double *rec, double *inf) {
	switch (an_entry_class(k)) {
	case 1: an_fit<1>(P, invalid, work, rec, inf); break;
	case 4: an_fit<4>(P, invalid, work, rec, inf); break;
	default: an_fit<10>(P, invalid, work, rec, inf); break;
	}
}

int main() {
	const int n_cases = (int)read_double();
	const int64_t pad = 5;
	const double poison = -12345.678;
	for (int cs = 0; cs < n_cases; ++cs) {
		AnProblem P;
		P.dist = (int)read_double();
		P.fit_intercept = (int)read_double();
		P.max_iterations = (int)read_double();
		P.tolerance = read_double();
		P.compute_inference = (int)read_double();
		P.zq = read_double();
		const double wq = read_double(), horizon = read_double();
		const int p = (int)read_double();
		const int64_t n = (int64_t)read_double();
		if (p < 1 || p > kAnMaxP || n < 0) {
			fprintf(stderr, "ERROR: bad case header\n");
			return 2;
		}
		const size_t N = (size_t)(n + 2 * pad);
		std::vector<double> time(N, poison), event(N, poison), logt(N, poison), pred(4 * N, poison);
		std::vector<std::vector<double>> cols((size_t)p, std::vector<double>(N, poison));
		for (int64_t i = 0; i < n; ++i) {
			time[(size_t)(pad + i)] = read_double();
			event[(size_t)(pad + i)] = read_double();
			for (int j = 0; j < p; ++j) cols[(size_t)j][(size_t)(pad + i)] = read_double();
		}
		std::vector<const double *> xp((size_t)p);
		for (int j = 0; j < p; ++j) xp[(size_t)j] = cols[(size_t)j].data();
		P.time = time.data();
		P.event = event.data();
		P.x = xp.data();
		P.p = p;
		P.lo = pad;
		P.hi = pad + n;
		P.logt = logt.data();
		const bool invalid = !(P.tolerance > 0.0) || !(P.tolerance <= DBL_MAX) || P.max_iterations <= 0 || P.dist < 0 || P.dist > 3;
		if (invalid) P.dist = 0;
		const int k = p + (P.fit_intercept ? 1 : 0) + (an_scale_is_fixed(P.dist) ? 0 : 1);
		std::vector<double> work(an_work_doubles(k), poison), rec((size_t)p + 13, poison), inf(5 * (size_t)p + 2, poison);
		std::vector<double> rec0(rec), inf0(inf);
		fit(P, invalid, k, work.data(), rec0.data(), inf0.data()); // the fit alone
		std::fill(work.begin(), work.end(), poison);
		std::fill(logt.begin(), logt.end(), poison);
		P.pred = pred.data();
		P.wq = wq;
		P.horizon = horizon;
		fit(P, invalid, k, work.data(), rec.data(), inf.data());
		for (int64_t i = 0; i < (int64_t)N; ++i) {
			const bool inside = i >= pad && i < pad + n;
			for (int s = 0; s < 4; ++s) {
				const double v = pred[(size_t)(4 * i + s)];
				if (inside != (memcmp(&v, &poison, sizeof v) != 0)) {
					fprintf(stderr, "ERROR: prediction slot %d of row %lld %s (case %d)\n", s, (long long)(i - pad),
					        inside ? "was not written" : "lies outside the group and was written", cs);
					return 3;
				}
			}
			if (!inside && logt[(size_t)i] != poison) {
				fprintf(stderr, "ERROR: a scratch slot outside the group's rows was written (case %d, slot %lld)\n", cs, (long long)i);
				return 3;
			}
		}
		for (double v : rec) printf("%.17g ", v);
		for (double v : inf) printf("%.17g ", v);
		for (double v : rec0) printf("%.17g ", v);
		for (double v : inf0) printf("%.17g ", v);
		for (int64_t i = 0; i < 4 * n; ++i) printf("%.17g ", pred[(size_t)(4 * pad + i)]);
		printf("\n");
	}
	return 0;
}
