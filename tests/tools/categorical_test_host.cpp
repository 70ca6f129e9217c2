// categorical_test_host.cpp — the categorical test header (csrc/categorical_tests.h) in its host build, where a wavefront is a loop
// over 64 lanes: a stand-alone program that tests/test_categorical_test_abi_cpu.py compiles under ASan / UBSan and feeds one call on
// stdin.
//
// stdin:  raw doubles (native byte order): test alternative correction exact confidence_level small_cap n_groups n_rows, then the
//         n_groups + 1 offsets, a[n_rows] and b[n_rows] (labels as doubles, exact for int32).
// stdout: one line, the records (n_groups x 12), %.17g.
// A group of at most small_cap rows goes the small path; a larger one the large path: its work arrays are a slice of one
// workspace as long as the call.  The work arrays of the small path are exactly as long as the group, so a read or write outside
// them is the sanitizer's to report; Fisher and McNemar get no work arrays at all.  The records start out as a poison value and
// every element has to be written.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/categorical_tests.h"

using namespace anofox::cor;
using namespace anofox::cattest;

static double read_double() {
	double v;
	if (fread(&v, sizeof v, 1, stdin) != 1) {
		fprintf(stderr, "ERROR: short input\n");
		exit(2);
	}
	return v;
}

int main() {
	CategoricalProblem P;
	P.test = (int)read_double();
	P.alternative = (int)read_double();
	P.correction = (int)read_double();
	P.exact = (int)read_double();
	P.confidence_level = read_double();
	const int64_t cap = (int64_t)read_double(), n_groups = (int64_t)read_double(), n_rows = (int64_t)read_double();
	if (n_groups < 0 || n_rows < 0 || ct_options_text(P.test, P.alternative, P.confidence_level)) {
		fprintf(stderr, "ERROR: bad header\n");
		return 2;
	}
	std::vector<int64_t> off((size_t)n_groups + 1);
	for (auto &o : off) o = (int64_t)read_double();
	std::vector<int32_t> a((size_t)n_rows), b((size_t)n_rows);
	for (auto &v : a) v = (int32_t)read_double();
	for (auto &v : b) v = (int32_t)read_double();
	const double poison = -12345.678;
	std::vector<double> rec((size_t)n_groups * kCtRecordLen, poison);
	P.a = a.data();
	P.b = b.data();
	P.n_rows = n_rows;
	P.records = rec.data();
	std::vector<double> wx((size_t)n_rows), wy((size_t)n_rows), wk((size_t)n_rows);
	std::vector<int32_t> wi((size_t)n_rows);
	for (int64_t g = 0; g < n_groups; ++g) {
		const int64_t lo = off[(size_t)g], hi = off[(size_t)g + 1], m = hi - lo;
		if (lo < 0 || hi < lo || hi > n_rows) {
			fprintf(stderr, "ERROR: bad offsets\n");
			return 2;
		}
		if (!ct_staged(P.test)) { // not staged: no work arrays at all
			ct_group(P, g, lo, hi, CorWork {nullptr, nullptr, nullptr, nullptr}, true, 0, 64);
			continue;
		}
		if (m <= cap) {
			std::vector<double> sx((size_t)m), sy((size_t)m), sk((size_t)m);
			std::vector<int32_t> si((size_t)m);
			ct_group(P, g, lo, hi, CorWork {sx.data(), sy.data(), sk.data(), si.data()}, true, 0, 64);
			continue;
		}
		ct_group(P, g, lo, hi, CorWork {wx.data() + lo, wy.data() + lo, wk.data() + lo, wi.data() + lo}, true, 0, 64);
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
