// bls_glue_sanitize.cpp — duckdb_shim/bls_family_hip.cpp and its test driver (bls_family_capi.cpp) linked with a MOCK of the
// three C ABI symbols they call, for an ASan / UBSan build on a machine without a GPU (tests/test_bls_cpu.py): registration,
// bind, Update from several threads, Combine, Finalize by vectors (LIST children reserved before they are written), NULL
// results, Destroy.  The mock "fits" b_j = j + 1 at the first column's lower flag and predicts yhat = y's row index.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "anofox_stats_hip.h"

extern "C" {
size_t anofox_hip_max_features(void) { return 128; }
bool anofox_hip_bls_fit_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t, const int64_t *off, const double *, const double *const *,
                                   AnofoxHipBlsBatchOptions, double *rec, int32_t *, AnofoxError *) {
	for (int64_t g = 0; g < G; ++g) {
		double *r = rec + g * (3 * p + 6);
		for (size_t k = 0; k < 3 * p + 6; ++k) r[k] = 0.0;
		for (size_t j = 0; j < p; ++j) r[j] = j == 1 ? NAN : (double)(j + 1);
		r[p] = NAN;
		r[p + 3] = (double)(off[g + 1] - off[g]);
		r[p + 4] = 1.0;
		r[p + 5] = (g % 5 == 4) ? 6.0 : 0.0; // every fifth group fails
		r[p + 6] = 1.0;
	}
	return true;
}
bool anofox_hip_bls_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *, const double *, const double *const *,
                                           const int64_t *, AnofoxHipBlsBatchOptions, double, double *core, double *pred, AnofoxError *) {
	for (int64_t g = 0; g < G; ++g) {
		for (size_t k = 0; k < p + 6; ++k) core[g * (p + 6) + k] = 0.0;
		core[g * (p + 6) + p + 5] = (g % 4 == 3) ? 6.0 : 0.0;
	}
	for (int64_t r = 0; r < n; ++r) {
		pred[3 * r] = (r % 7 == 6) ? NAN : (double)r;
		pred[3 * r + 1] = pred[3 * r] - 1.0;
		pred[3 * r + 2] = pred[3 * r] + 1.0;
	}
	return true;
}

void *blsf_open(const char *, const char *, int, char *);
void blsf_close(void *);
int blsf_group_by(void *, size_t, size_t, const uint32_t *, size_t, const double *, const double *, const uint8_t *, const uint8_t *, const uint8_t *, int,
                  size_t, double *, uint8_t *, char *);
void *blsp_open(const char *, const char *, int, int, char *);
void blsp_close(void *);
int64_t blsp_group_by(void *, size_t, size_t, const uint32_t *, size_t, const double *, const double *, const uint8_t *, const uint8_t *, const uint8_t *,
                      const uint8_t *, int, size_t, int64_t *, double *, uint8_t *, uint8_t *, char *);
void blsp_feature_count_errors(void *, char *, char *);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "bls_glue_sanitize: %s failed at line %d: %s\n", #c, __LINE__, msg); return 1; } } while (0)

int main() {
	char msg[512] = "";
	const size_t n = 5000, p = 3, K = 37;
	std::vector<double> y(n), x(n * p);
	std::vector<uint32_t> key(n);
	std::vector<uint8_t> y_null(n, 0), x_null(n, 0), xe_null(n * p, 0);
	for (size_t i = 0; i < n; ++i) {
		y[i] = (double)i;
		key[i] = (uint32_t)((i * 7) % K);
		for (size_t j = 0; j < p; ++j) x[i * p + j] = (double)(i + j);
		y_null[i] = i % 11 == 0;
		x_null[i] = i % 13 == 0;
		xe_null[i * p + 1] = i % 17 == 0;
	}
	for (const char *fn : {"anofox_stats_bls_fit_agg", "bls_fit_agg", "anofox_stats_nnls_fit_agg", "nnls_fit_agg"}) {
		for (const char *spec : {(const char *)nullptr, "lower=-1;upper=2;fit_intercept=true"}) {
			void *q = blsf_open(fn, spec, spec != nullptr, msg);
			CHECK(q != nullptr);
			std::vector<double> out(K * (3 * p + 6));
			std::vector<uint8_t> is_null(K);
			CHECK(blsf_group_by(q, n, p, key.data(), K, y.data(), x.data(), y_null.data(), x_null.data(), xe_null.data(), 4, 64, out.data(), is_null.data(), msg) == 0);
			for (size_t k = 0; k < K; ++k) {
				const double *r = &out[k * (3 * p + 6)];
				if (is_null[k]) continue;
				CHECK(r[0] == 1.0 && isnan(r[1]) && r[2] == 3.0 && isnan(r[p]) && r[p + 4] == 1.0 && r[p + 6] == 1.0 && r[p + 7] == 0.0);
			}
			size_t nulls = 0;
			for (auto v : is_null) nulls += v;
			CHECK(nulls > 0 && nulls < K);
			blsf_close(q);
		}
	}
	CHECK(blsf_open("bls_fit_agg", "null_policy=bogus", 0, msg) == nullptr);
	for (int split = 0; split < 2; ++split) {
		void *q = blsp_open("bls_fit_predict_agg", "lower=0;confidence_level=0.9", 0, split, msg);
		CHECK(q != nullptr);
		std::vector<int64_t> off(K + 1);
		std::vector<double> vals(n * 4);
		std::vector<uint8_t> flags(n), is_null(K), sp(n);
		for (size_t i = 0; i < n; ++i) sp[i] = (uint8_t)(i % 3 == 0 ? 2 : 1);
		const int64_t rows = blsp_group_by(q, n, p, key.data(), K, y.data(), x.data(), y_null.data(), x_null.data(), xe_null.data(), split ? sp.data() : nullptr,
		                                   3, 128, off.data(), vals.data(), flags.data(), is_null.data(), msg);
		CHECK(rows > 0 && rows <= (int64_t)n && off[K] == rows);
		// one state given a 2-feature row and then a 3-feature row; a 2-feature state combined into a 3-feature state: the texts of
		// bls_fit_predict_aggregate.cpp, without the counts
		char combine_msg[512];
		blsp_feature_count_errors(q, msg, combine_msg);
		CHECK(strcmp(msg, "Inconsistent feature count") == 0);
		memcpy(msg, combine_msg, sizeof msg);
		CHECK(strcmp(msg, "Cannot combine states with different feature counts") == 0);
		blsp_close(q);
	}
	printf("bls_glue_sanitize: all scenarios passed\n");
	return 0;
}
