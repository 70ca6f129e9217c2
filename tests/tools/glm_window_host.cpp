// glm_window_host.cpp — the window walk of the GLM solver header (csrc/glm_irls.h, gi_fit_window) in its host build, where a
// wavefront is a loop over 64 lanes: a stand-alone program that tests/test_glm_window_cpu.py compiles under ASan / UBSan and
// feeds one call on stdin.
//
// stdin:  raw doubles (native byte order):
//           family fit_intercept max_iterations tolerance lambda p n has_offset warm interval_z check_plain n_runs
//           run_begin[n_runs + 1]   lo[n]   hi[n]   n rows of  y x_1 .. x_p [offset]
// stdout: per output row one line: the record (p + 11), pred (3), how the frame was started (0 cold, 1 warm, 2 warm and
//         refitted cold); then one line with the walk's counts {cold, warm, refitted, iterations}.
// Every run is walked on a slab of exactly 2 x (the longest frame of the call) doubles, the planner's bound, allocated on
// its own (a slot past it is ASan's) and pre-filled with a stale value before every run.
// check_plain (for warm = 0): every frame is also fitted by a plain gi_fit on a gathered copy of its rows, as the batch entry
// fits a group; the record and mu of the last row have to be the same bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

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

template <int EM>
static void walk(const GiProblem &P, bool invalid, bool warm, const int64_t *lo, const int64_t *hi, int64_t e0, int64_t e1, int64_t slab_rows,
                 double *work, double *pred, double *rec, int64_t *counts, int32_t *started) {
	gi_fit_window<EM>(P, invalid, warm, lo, hi, e0, e1, slab_rows, work, pred, rec, counts, started);
}

template <int EM>
static void plain(const GiProblem &P, bool invalid, double *work, double *rec, double *pred) {
	gi_fit<EM>(P, invalid, work, rec, nullptr, pred);
}

int main() {
	GiProblem P;
	P.family = (int)read_double();
	P.fit_intercept = (int)read_double();
	P.max_iterations = (int)read_double();
	P.tolerance = read_double();
	P.lambda = read_double();
	const int p = (int)read_double();
	const int64_t n = (int64_t)read_double();
	const int has_offset = (int)read_double(), warm = (int)read_double();
	P.interval_z = read_double();
	const int check_plain = (int)read_double();
	const int64_t n_runs = (int64_t)read_double();
	if (p < 1 || p > kGiMaxP || n < 0 || n_runs < 0) {
		fprintf(stderr, "ERROR: bad header\n");
		return 2;
	}
	const size_t N = (size_t)n, R = (size_t)(p + 11);
	std::vector<int64_t> run_begin((size_t)n_runs + 1), lo(N), hi(N);
	for (auto &v : run_begin) v = (int64_t)read_double();
	for (auto &v : lo) v = (int64_t)read_double();
	for (auto &v : hi) v = (int64_t)read_double();
	std::vector<double> y(N), off(N);
	std::vector<std::vector<double>> cols((size_t)p, std::vector<double>(N));
	for (size_t i = 0; i < N; ++i) {
		y[i] = read_double();
		for (int j = 0; j < p; ++j) cols[(size_t)j][i] = read_double();
		if (has_offset) off[i] = read_double();
	}
	std::vector<const double *> xp((size_t)p);
	for (int j = 0; j < p; ++j) xp[(size_t)j] = cols[(size_t)j].data();
	P.y = y.data();
	P.x = xp.data();
	P.offset = has_offset ? off.data() : nullptr;
	P.p = p;
	P.lo = P.hi = 0;
	P.rule_count = 0;
	P.compute_inference = 0;
	P.zq = NAN;
	const int k = p + (P.fit_intercept ? 1 : 0);
	const bool invalid = !(P.tolerance > 0.0) || !(P.tolerance <= DBL_MAX) || !(P.lambda >= 0.0) || !(P.lambda <= DBL_MAX) ||
	                     P.max_iterations <= 0 || (P.family != kGiFamilyPoisson && P.family != kGiFamilyBinomial);
	int64_t span = 1;
	for (size_t e = 0; e < N; ++e)
		if (hi[e] - lo[e] > span) span = hi[e] - lo[e];
	const double stale = -12345.678;
	std::vector<double> slab(2 * (size_t)span), work(gi_window_work_doubles(p, k), stale), pred(3 * N, stale), rec(N * R, stale);
	std::vector<int32_t> started(N, -1);
	int64_t counts[4] = {0, 0, 0, 0};
	P.eta = slab.data();
	P.mu = slab.data() + span;
	const int em = gi_entry_class(k);
	for (int64_t w = 0; w < n_runs; ++w) {
		for (auto &v : slab) v = stale;
		const int64_t e0 = run_begin[(size_t)w], e1 = run_begin[(size_t)w + 1];
		if (em == 1) walk<1>(P, invalid, warm != 0, lo.data(), hi.data(), e0, e1, span, work.data(), pred.data(), rec.data(), counts, started.data());
		else if (em == 4) walk<4>(P, invalid, warm != 0, lo.data(), hi.data(), e0, e1, span, work.data(), pred.data(), rec.data(), counts, started.data());
		else walk<10>(P, invalid, warm != 0, lo.data(), hi.data(), e0, e1, span, work.data(), pred.data(), rec.data(), counts, started.data());
	}
	if (check_plain) {
		std::vector<double> pwork(gi_work_doubles(k)), prec(R);
		for (size_t e = 0; e < N; ++e) {
			const int64_t a = hi[e] > lo[e] ? lo[e] : 0, b = hi[e] > lo[e] ? hi[e] : 0;
			const size_t m = (size_t)(b - a);
			std::vector<double> gy(y.begin() + a, y.begin() + b), goff(off.begin() + a, off.begin() + b), geta(m, stale), gmu(m, stale), gpred(3 * m, stale);
			std::vector<std::vector<double>> gcols((size_t)p);
			std::vector<const double *> gxp((size_t)p);
			for (int j = 0; j < p; ++j) {
				gcols[(size_t)j].assign(cols[(size_t)j].begin() + a, cols[(size_t)j].begin() + b);
				gxp[(size_t)j] = gcols[(size_t)j].data();
			}
			GiProblem Q = P;
			Q.y = gy.data();
			Q.x = gxp.data();
			Q.offset = has_offset ? goff.data() : nullptr;
			Q.lo = 0;
			Q.hi = (int64_t)m;
			Q.rule_count = 0;
			for (double v : gy) Q.rule_count += v == v ? 1 : 0;
			Q.eta = geta.data();
			Q.mu = gmu.data();
			Q.start = nullptr;
			for (auto &v : pwork) v = stale;
			if (em == 1) plain<1>(Q, invalid, pwork.data(), prec.data(), gpred.data());
			else if (em == 4) plain<4>(Q, invalid, pwork.data(), prec.data(), gpred.data());
			else plain<10>(Q, invalid, pwork.data(), prec.data(), gpred.data());
			const double nan3[3] = {NAN, NAN, NAN};
			const double *want = m ? &gpred[3 * (m - 1)] : nan3;
			if (memcmp(prec.data(), &rec[e * R], R * sizeof(double)) != 0 || memcmp(want, &pred[3 * e], 3 * sizeof(double)) != 0) {
				fprintf(stderr, "ERROR: frame %zu [%lld, %lld) differs from the plain fit of its rows\n", e, (long long)a, (long long)b);
				return 3;
			}
		}
	}
	for (size_t e = 0; e < N; ++e) {
		for (size_t j = 0; j < R; ++j) printf("%.17g ", rec[e * R + j]);
		printf("%.17g %.17g %.17g %d\n", pred[3 * e], pred[3 * e + 1], pred[3 * e + 2], (int)started[e]);
	}
	printf("%lld %lld %lld %lld\n", (long long)counts[0], (long long)counts[1], (long long)counts[2], (long long)counts[3]);
	return 0;
}
