// cor_host.cpp — the correlation header (csrc/rank_cor.h) in its host build, where a wavefront is a loop over 64 lanes: a
// stand-alone program that tests/test_cor_restate_cpu.py compiles under ASan / UBSan and feeds one call on stdin.
//
// stdin:  raw doubles (native byte order): method alternative tau_type confidence_level small_cap n_groups n_rows, then the
//         n_groups + 1 offsets, x[n_rows], y[n_rows]
// stdout: one line, the records (n_groups x 8), %.17g.
// A group of at most small_cap rows goes the small path; a larger one the large path: its work arrays are a slice of one
// workspace as long as the call, and a Kendall group's pairs are counted by tiles as the pair kernel counts them.  The work arrays
// of the small path are exactly as long as the group, so a read or write outside them is the sanitizer's to report; the records
// start out as a poison value and every element has to be written.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/rank_cor.h"

using namespace anofox::cor;

static double read_double() {
	double v;
	if (fread(&v, sizeof v, 1, stdin) != 1) {
		fprintf(stderr, "ERROR: short input\n");
		exit(2);
	}
	return v;
}

// the standard normal quantile by bisection on erfc (the library takes it from host_math.h)
static double normal_quantile(double prob) {
	double lo = -40.0, hi = 40.0;
	for (int i = 0; i < 200; ++i) {
		const double mid = 0.5 * (lo + hi);
		if (0.5 * erfc(-mid * 0.70710678118654752440) < prob) lo = mid;
		else hi = mid;
	}
	return 0.5 * (lo + hi);
}

int main() {
	const int method = (int)read_double(), alternative = (int)read_double(), tau_type = (int)read_double();
	const double level = read_double();
	const int64_t cap = (int64_t)read_double(), n_groups = (int64_t)read_double(), n_rows = (int64_t)read_double();
	if (n_groups < 0 || n_rows < 0 || rc_options_invalid(method, alternative, tau_type, level)) {
		fprintf(stderr, "ERROR: bad header\n");
		return 2;
	}
	std::vector<int64_t> off((size_t)n_groups + 1);
	for (auto &o : off) o = (int64_t)read_double();
	std::vector<double> x((size_t)n_rows), y((size_t)n_rows);
	for (auto &v : x) v = read_double();
	for (auto &v : y) v = read_double();
	const double poison = -12345.678;
	std::vector<double> rec((size_t)n_groups * kCorRecordLen, poison);
	CorProblem P;
	P.x = x.data();
	P.y = y.data();
	P.n_rows = n_rows;
	P.method = method;
	P.alternative = alternative;
	P.tau_type = tau_type;
	P.zq = level == level ? normal_quantile(0.5 * (1.0 + level)) : NAN;
	P.records = rec.data();
	std::vector<double> wx((size_t)n_rows), wy((size_t)n_rows), wk((size_t)n_rows);
	std::vector<int32_t> wi((size_t)n_rows);
	for (int64_t g = 0; g < n_groups; ++g) {
		const int64_t lo = off[(size_t)g], hi = off[(size_t)g + 1], m = hi - lo;
		if (lo < 0 || hi < lo || hi > n_rows) {
			fprintf(stderr, "ERROR: bad offsets\n");
			return 2;
		}
		if (m <= cap) {
			std::vector<double> sx((size_t)m), sy((size_t)m), sk((size_t)m);
			std::vector<int32_t> si((size_t)m);
			rc_group(P, g, lo, hi, CorWork {sx.data(), sy.data(), sk.data(), si.data()}, true, 0, 64, nullptr);
			continue;
		}
		CorLarge L;
		L.n = 0;
		const CorWork W = {wx.data() + lo, wy.data() + lo, wk.data() + lo, wi.data() + lo};
		rc_group(P, g, lo, hi, W, true, 0, 64, &L);
		if (method != kCorKendall || L.n < 3) continue;
		const int64_t nb = (L.n + kCorPairTile - 1) / kCorPairTile;
		for (int64_t t = nb * nb - 1; t >= 0; --t) { // (any order of the tiles)
			const int64_t ib = t / nb, jb = t % nb;
			if (jb < ib) continue;
			const int64_t j0 = jb * kCorPairTile, jn = L.n - j0 < kCorPairTile ? L.n - j0 : kCorPairTile;
			for (int64_t i = ib * kCorPairTile; i < (ib + 1) * kCorPairTile && i < L.n; ++i)
				L.s += rc_pairs_row(W.x[i], W.y[i], W.x + j0, W.y + j0, jb == ib ? i - j0 + 1 : 0, jn);
		}
		rc_kendall_record(P, L.s, L.n, L.tx, L.ty, rec.data() + L.group * kCorRecordLen);
	}
	for (double v : rec) {
		if (v == poison) {
			fprintf(stderr, "ERROR: a record element was not written\n");
			return 3;
		}
		printf("%.17g ", v);
	}
	printf("\n");
	return 0;
}
