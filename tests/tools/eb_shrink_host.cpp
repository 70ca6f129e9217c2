// eb_shrink_host.cpp — the shrinkage header (csrc/eb_shrink.h) in its host build, where a wavefront is a loop over 64 lanes: a
// stand-alone program that tests/test_eb_shrink_cpu.py compiles under ASan / UBSan and feeds one call on stdin.
//
// stdin:  raw doubles (native byte order): path (1: one wavefront per set, 2: chunks) chunk_items method tau_squared n_sets
//         n_items n_cols est_stride se_stride est_len se_len, then the n_sets + 1 offsets, est[est_len], se[se_len]
// stdout: two lines: the summary (n_sets x n_cols x 8) and the outputs (n_items x n_cols x 3), %.17g.
// The arrays are exactly as long as the call says, so a read or write outside them is the sanitizer's to report; the outputs
// start out as a poison value and every element has to be written.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../anofox-statistics_amd/csrc/eb_shrink.h"

using namespace anofox::eb;

static double read_double() {
	double v;
	if (fread(&v, sizeof v, 1, stdin) != 1) {
		fprintf(stderr, "ERROR: short input\n");
		exit(2);
	}
	return v;
}

int main() {
	const int path = (int)read_double();
	const int64_t chunk_in = (int64_t)read_double();
	const int method = (int)read_double();
	const double tau = read_double();
	const int64_t n_sets = (int64_t)read_double(), n_items = (int64_t)read_double();
	const int n_cols = (int)read_double();
	const int64_t est_stride = (int64_t)read_double(), se_stride = (int64_t)read_double();
	const int64_t est_len = (int64_t)read_double(), se_len = (int64_t)read_double();
	if (n_sets < 1 || n_items < 0 || n_cols < 1 || est_stride < n_cols || se_stride < n_cols || est_len < 0 || se_len < 0) {
		fprintf(stderr, "ERROR: bad header\n");
		return 2;
	}
	std::vector<int64_t> off((size_t)n_sets + 1);
	for (auto &o : off) o = (int64_t)read_double();
	std::vector<double> est((size_t)est_len), se((size_t)se_len);
	for (auto &v : est) v = read_double();
	for (auto &v : se) v = read_double();
	const double poison = -12345.678;
	std::vector<double> out((size_t)n_items * n_cols * kEbOutLen, poison), summary((size_t)n_sets * n_cols * kEbSummaryLen, poison);
	EbProblem P;
	P.est = est.data();
	P.se = se.data();
	P.est_stride = est_stride;
	P.se_stride = se_stride;
	P.n_items = n_items;
	P.n_cols = n_cols;
	P.invalid = eb_options_invalid(method, tau) ? 1 : 0;
	P.method = P.invalid ? kEbMethodDL : method;
	P.tau_fixed = P.invalid ? NAN : tau;
	P.out = out.data();
	P.summary = summary.data();
	const int blocks = eb_col_blocks(n_cols);
	if (path == 1) {
		for (int64_t s = 0; s < n_sets; ++s)
			for (int b = 0; b < blocks; ++b) eb_shrink_set(P, s, off[(size_t)s], off[(size_t)s + 1], b * 64);
	} else {
		const int64_t by_pairs = 1024 / eb_col_pad(n_cols), chunk = chunk_in > 0 ? chunk_in : (by_pairs < 64 ? 64 : by_pairs);
		const int64_t numbers = n_items / chunk + n_sets;
		std::vector<double> state((size_t)n_sets * n_cols * kEbStateLen, poison), parts((size_t)numbers * n_cols * kEbPartLen, poison);
		const int64_t *o = off.data();
#define EACH_NUMBER(CALL)                     \
	for (int64_t v = 0; v < numbers; ++v)     \
		for (int b = 0; b < blocks; ++b) CALL;
#define EACH_SET(CALL)                        \
	for (int64_t s = 0; s < n_sets; ++s)      \
		for (int b = 0; b < blocks; ++b) CALL;
		EACH_NUMBER(eb_chunk_partial<1>(P, o, n_sets, chunk, v, b * 64, state.data(), parts.data()))
		EACH_SET(eb_chunk_combine<1>(P, o, numbers, chunk, s, b * 64, state.data(), parts.data()))
		EACH_NUMBER(eb_chunk_partial<2>(P, o, n_sets, chunk, v, b * 64, state.data(), parts.data()))
		EACH_SET(eb_chunk_combine<2>(P, o, numbers, chunk, s, b * 64, state.data(), parts.data()))
		EACH_NUMBER(eb_chunk_partial<3>(P, o, n_sets, chunk, v, b * 64, state.data(), parts.data()))
		EACH_SET(eb_chunk_combine<3>(P, o, numbers, chunk, s, b * 64, state.data(), parts.data()))
		EACH_NUMBER(eb_chunk_write(P, o, n_sets, chunk, v, b * 64, state.data()))
	}
	for (double v : summary) {
		if (v == poison) {
			fprintf(stderr, "ERROR: a summary element was not written\n");
			return 3;
		}
		printf("%.17g ", v);
	}
	printf("\n");
	for (double v : out) {
		if (v == poison) {
			fprintf(stderr, "ERROR: an output element was not written\n");
			return 3;
		}
		printf("%.17g ", v);
	}
	printf("\n");
	return 0;
}
