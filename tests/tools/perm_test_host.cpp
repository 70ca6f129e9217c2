// perm_test_host.cpp — the permutation test header (csrc/perm_tests.h) in its host build, where a wavefront is a loop over 64
// lanes: a stand-alone program that tests/test_perm_test_restate_cpu.py compiles under ASan / UBSan and feeds one call on stdin.
//
// stdin:  raw doubles (native byte order): test alternative n_permutations seed_high32 seed_low32 sigma small_cap n_groups n_rows,
//         then the n_groups + 1 offsets, v[n_rows], sample[n_rows] (the ids as doubles)
// stdout: one line, the records (n_groups x 8), %.17g.
// A group of at most small_cap rows goes the small path; a larger one the large path: its work arrays are a slice of one
// workspace as long as the call, sixteen wavefronts share the rounds and their counts are added, and MMD gets status 7.  The work
// arrays of the small path are exactly as long as the group, so a read or write outside them is the sanitizer's to report; the
// records start out as a poison value and every element has to be written.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/perm_tests.h"

using namespace anofox::cor;
using namespace anofox::permtest;

static double read_double() {
	double v;
	if (fread(&v, sizeof v, 1, stdin) != 1) {
		fprintf(stderr, "ERROR: short input\n");
		exit(2);
	}
	return v;
}

int main() {
	const int test = (int)read_double(), alternative = (int)read_double();
	const int64_t n_perm = (int64_t)read_double();
	const uint64_t seed_high = (uint64_t)read_double(), seed_low = (uint64_t)read_double();
	const double sigma = read_double();
	const int64_t cap = (int64_t)read_double(), n_groups = (int64_t)read_double(), n_rows = (int64_t)read_double();
	if (n_groups < 0 || n_rows < 0 || pt_options_text(test, alternative, n_perm, sigma)) {
		fprintf(stderr, "ERROR: bad header\n");
		return 2;
	}
	std::vector<int64_t> off((size_t)n_groups + 1);
	for (auto &o : off) o = (int64_t)read_double();
	std::vector<double> v((size_t)n_rows);
	std::vector<int32_t> sample((size_t)n_rows);
	for (auto &a : v) a = read_double();
	for (auto &a : sample) a = (int32_t)read_double();
	const double poison = -12345.678;
	std::vector<double> rec((size_t)n_groups * kPtRecordLen, poison);
	PermTestProblem P;
	P.v = v.data();
	P.sample = sample.data();
	P.n_rows = n_rows;
	P.test = test;
	P.alternative = alternative;
	P.n_perm = n_perm;
	P.seed = seed_high << 32 | seed_low;
	P.sigma = sigma;
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
			pt_group(P, g, lo, hi, CorWork {sx.data(), sy.data(), sk.data(), si.data()}, 0);
			continue;
		}
		const CorWork W = {wx.data() + lo, wy.data() + lo, wk.data() + lo, wi.data() + lo};
		const PtInfo I = pt_prepare(P, lo, hi, W, true, 0, 64, false);
		double obs = NAN, aux = NAN;
		int64_t count = 0;
		if (I.status == 0)
			for (int wave = 0; wave < 16; ++wave) count += pt_rounds(P, I, W, wave, 16, obs, aux);
		pt_record(P, I, obs, aux, count, rec.data() + g * kPtRecordLen);
	}
	for (double a : rec) {
		if (a == poison) {
			fprintf(stderr, "ERROR: a record element was not written\n");
			return 3;
		}
		printf("%.17g ", a);
	}
	printf("\n");
	return 0;
}
