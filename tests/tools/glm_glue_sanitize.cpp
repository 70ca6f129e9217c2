// glm_glue_sanitize.cpp — duckdb_shim/glm_family_hip.cpp and its test driver (glm_family_capi.cpp) linked with a MOCK of the
// C ABI symbols they call, for an ASan / UBSan build on a machine without a GPU (tests/test_glm_glue_cpu.py): registration,
// bind, Update from several threads with dictionary vectors, Combine, Finalize by vectors of several sizes (LIST children
// reserved before they are written), two feature counts in one Finalize vector, NULL results, the offset column, a bad offset,
// a failing call, Destroy.
//
// The mock "fits" nothing: a record holds sums over the group's rows and echoes of the options, a prediction the sum of its
// row's x plus its group's train count.  Every input is a small integer, so each value is exact and says which rows, which
// columns and which options reached the call: routing is checked with ==.  The mock counts its calls: exactly one per
// Finalize vector and feature count.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "duckdb.hpp"

#include "anofox_stats_hip.h"
#include "glm_family_hip.hpp"

static int g_calls = 0;
static bool g_fail = false;

// record: coefficients[j] = sum of feature column j, intercept = sum of y, deviance = sum of the offset column (0 without one),
// null_deviance = lambda, pseudo_r_squared = max_iterations, aic = family, dispersion = confidence_level, n_observations = rows,
// n_params = q + 1, iterations = 7, converged = 1, status = 1 for a group with a negative y; inference[k][j] = coefficient + k + 1
static bool mock_fit(int64_t G, size_t q, int64_t n, const int64_t *off, const double *y, const double *const *cols, const double *offset,
                     AnofoxHipGlmBatchOptions o, double *rec, double *inf, AnofoxError *err) {
	++g_calls;
	if (g_fail || !(G > 0 && q > 0 && off && y && cols && rec && off[0] == 0 && off[G] == n)) {
		err->code = ANOFOX_ERROR_INVALID_INPUT;
		snprintf(err->message, sizeof err->message, "%s", g_fail ? "mock: the batched call was told to fail" : "mock: malformed batch");
		return false;
	}
	for (int64_t g = 0; g < G; ++g) {
		double *r = rec + (size_t)g * (q + 11);
		for (size_t k = 0; k < q + 11; ++k) r[k] = 0.0;
		bool negative = false;
		for (int64_t i = off[g]; i < off[g + 1]; ++i) {
			for (size_t j = 0; j < q; ++j) r[j] += cols[j][i];
			if (!isnan(y[i])) r[q] += y[i];
			negative = negative || y[i] < 0.0;
			r[q + 1] += offset ? offset[i] : 0.0;
		}
		r[q + 2] = o.lambda;
		r[q + 3] = (double)o.max_iterations;
		r[q + 4] = (double)o.family;
		r[q + 5] = o.confidence_level;
		r[q + 6] = (double)(off[g + 1] - off[g]);
		r[q + 7] = (double)q + 1.0;
		r[q + 8] = 7.0;
		r[q + 9] = 1.0;
		r[q + 10] = negative ? 1.0 : 0.0;
		if (inf)
			for (size_t k = 0; k < 5; ++k)
				for (size_t j = 0; j < q; ++j) inf[((size_t)g * 5 + k) * q + j] = r[j] + (double)k + 1.0;
	}
	return true;
}

extern "C" {
bool anofox_hip_glm_fit_batch_host(AnofoxHipContext *, int64_t G, size_t q, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                   const double *offset, AnofoxHipGlmBatchOptions o, double *rec, double *inf, AnofoxError *err) {
	return mock_fit(G, q, n, off, y, cols, offset, o, rec, o.compute_inference ? inf : nullptr, err);
}
// accuracy = threshold + the group's rows
bool anofox_hip_glm_fit_accuracy_batch_host(AnofoxHipContext *, int64_t G, size_t q, int64_t n, const int64_t *off, const double *y,
                                            const double *const *cols, const double *offset, AnofoxHipGlmBatchOptions o, double threshold, double *rec,
                                            double *inf, double *accuracy, AnofoxError *err) {
	if (!mock_fit(G, q, n, off, y, cols, offset, o, rec, o.compute_inference ? inf : nullptr, err)) return false;
	for (int64_t g = 0; g < G; ++g) accuracy[g] = threshold + (double)(off[g + 1] - off[g]);
	return true;
}
// pred = {sum of the row's x + train_counts[g], interval_z, the count of the group's rows with a y}; three NaN where the sum is NaN
bool anofox_hip_glm_fit_predict_interval_batch_host(AnofoxHipContext *, int64_t G, size_t q, int64_t n, const int64_t *off, const double *y,
                                                    const double *const *cols, const double *offset, const int64_t *train_counts,
                                                    AnofoxHipGlmBatchOptions o, double z, double *core, double *pred, AnofoxError *err) {
	if (!mock_fit(G, q, n, off, y, cols, offset, o, core, nullptr, err)) return false;
	for (int64_t g = 0; g < G; ++g) {
		double with_y = 0.0;
		for (int64_t i = off[g]; i < off[g + 1]; ++i) with_y += !isnan(y[i]);
		for (int64_t i = off[g]; i < off[g + 1]; ++i) {
			double s = 0.0;
			for (size_t j = 0; j < q; ++j) s += cols[j][i];
			pred[3 * i] = isnan(s) ? NAN : s + (double)train_counts[g];
			pred[3 * i + 1] = isnan(s) ? NAN : z;
			pred[3 * i + 2] = isnan(s) ? NAN : with_y;
		}
	}
	return true;
}

void *gg_open(const char *, const char *, int, int, int, char *);
void gg_close(void *);
int64_t gg_group_by(void *, size_t, size_t, const uint32_t *, size_t, const double *, const double *, const uint8_t *, const uint8_t *, const uint8_t *,
                    const uint32_t *, const uint8_t *, int, size_t, int, size_t, int64_t *, double *, uint8_t *, uint8_t *, size_t *, char *);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "glm_glue_sanitize: %s failed at line %d: %s\n", #c, __LINE__, msg); return 1; } } while (0)

namespace {
char msg[512] = "";

struct Data {
	size_t n = 1500, p = 3, K = 37; // key K - 1 never occurs: its global state is never initialised
	std::vector<double> y, x;
	std::vector<uint32_t> key, x_len;
	std::vector<uint8_t> y_null, x_null, xe_null, split;
	Data() : y(n), x(n * p), key(n), x_len(n), y_null(n, 0), x_null(n, 0), xe_null(n * p, 0), split(n) {
		for (size_t i = 0; i < n; ++i) {
			y[i] = (double)(i % 50);
			key[i] = (uint32_t)((i * 11) % (K - 2)); // keys 0 .. K - 3
			for (size_t j = 0; j < p; ++j) x[i * p + j] = (double)((i + 3 * j) % 101);
			y_null[i] = i % 11 == 0;
			x_null[i] = i % 13 == 0;
			split[i] = (uint8_t)(i % 7); // every spelling of the driver's table, and NULL
		}
		xe_null[40 * p + 1] = 1;            // a NULL list element: NaN in its column, no prediction for the row
		key[n - 1] = (uint32_t)(K - 2);     // a group of one row
		y_null[n - 1] = x_null[n - 1] = 0;
		for (size_t i = 0; i < n; ++i)
			if (key[i] == 5 && !y_null[i] && !x_null[i]) {
				y[i] = -1.0;                    // the mock fails group 5
				break;
			}
		for (size_t i = 0; i < n; ++i) x_len[i] = (uint32_t)(key[i] % 2 ? p - 1 : p); // odd keys: two features
	}
	bool Trains(size_t i, bool with_split, bool drop_zero) const {
		static const bool split_trains[] = {false, true, true, false, true, false, true};
		bool t = !y_null[i] && (!with_split || split_trains[split[i]]);
		if (drop_zero)
			for (size_t j = 0; j < p; ++j) t = t && !(x[i * p + j] == 0.0 && !xe_null[i * p + j]);
		return t;
	}
};

struct Run {
	std::vector<int64_t> offsets;
	std::vector<double> vals;
	std::vector<uint8_t> flags, is_null;
	size_t q = 0;
	int64_t rc = 0;
};

Run GroupBy(void *h, const Data &d, bool ragged, bool with_split, int threads, size_t vsize, bool dictionary) {
	Run r;
	r.offsets.assign(d.K + 1, 0);
	r.vals.assign(std::max(d.n * 4, d.K * (6 * d.p + 11)), 0.0);
	r.flags.assign(d.n, 0);
	r.is_null.assign(d.K, 0);
	r.rc = gg_group_by(h, d.n, d.p, d.key.data(), d.K, d.y.data(), d.x.data(), d.y_null.data(), d.x_null.data(), d.xe_null.data(),
	                   ragged ? d.x_len.data() : nullptr, with_split ? d.split.data() : nullptr, threads, vsize, dictionary, r.vals.size(), r.offsets.data(),
	                   r.vals.data(), r.flags.data(), r.is_null.data(), &r.q, msg);
	return r;
}

// a fit aggregate over the data: every field of every group against the mock's definition
int CheckFit(const char *fn, const char *spec, bool as_map, bool ragged, size_t offset_column, bool inference, bool logistic, double lambda,
             double max_iterations, double family, double f6, int threads, size_t vsize, bool dictionary, int want_calls) {
	Data d;
	void *h = gg_open(fn, spec, as_map, 0, 1, msg);
	CHECK(h);
	g_calls = 0;
	Run r = GroupBy(h, d, ragged, false, threads, vsize, dictionary);
	gg_close(h);
	CHECK(r.rc == 0);
	CHECK(g_calls == want_calls);
	const size_t qmax = d.p - (offset_column ? 1 : 0), width = qmax + 11 + (inference ? 5 * qmax : 0);
	CHECK(r.q == qmax);
	for (uint32_t g = 0; g < d.K; ++g) {
		const size_t pg = ragged && g % 2 ? d.p - 1 : d.p, q = pg - (offset_column ? 1 : 0);
		std::vector<double> sum(pg, 0.0);
		double sum_y = 0.0, rows = 0.0;
		bool negative = false;
		for (size_t i = 0; i < d.n; ++i) {
			if (d.key[i] != g || d.y_null[i] || d.x_null[i]) continue;
			rows += 1.0;
			sum_y += d.y[i];
			negative = negative || d.y[i] < 0.0;
			for (size_t j = 0; j < pg; ++j) sum[j] += d.xe_null[i * d.p + j] ? NAN : d.x[i * d.p + j];
		}
		CHECK(r.is_null[g] == (rows < 2.0 || negative));
		if (r.is_null[g]) continue;
		const double *c = &r.vals[g * width];
		std::vector<double> coef;
		for (size_t j = 0; j < pg; ++j)
			if (j + 1 != offset_column) coef.push_back(sum[j]);
		for (size_t j = 0; j < q; ++j) CHECK(c[j] == coef[j] || (isnan(c[j]) && isnan(coef[j])));
		const double want[] = {sum_y, offset_column ? sum[offset_column - 1] : 0.0, lambda, max_iterations, family, f6};
		for (size_t k = 0; k < (logistic ? 5u : 6u); ++k) CHECK(c[qmax + k] == want[k] || (isnan(c[qmax + k]) && isnan(want[k])));
		CHECK(logistic ? c[qmax + 5] == f6 + rows && c[qmax + 6] == f6 : isnan(c[qmax + 6])); // accuracy = threshold + rows, then the threshold
		CHECK(c[qmax + 7] == rows && c[qmax + 8] == (double)q && c[qmax + 9] == 7.0 && c[qmax + 10] == 1.0);
		if (inference)
			for (size_t k = 0; k < 5; ++k)
				for (size_t j = 0; j < q; ++j) {
					const double v = c[qmax + 11 + k * qmax + j];
					CHECK(v == coef[j] + (double)k + 1.0 || (isnan(v) && isnan(coef[j])));
				}
	}
	return 0;
}

int CheckPredict(const char *fn, const char *spec, bool with_split, bool drop_zero, double z, int threads, size_t vsize, bool dictionary) {
	Data d;
	void *h = gg_open(fn, spec, 0, with_split, 1, msg);
	CHECK(h);
	Run r = GroupBy(h, d, false, with_split, threads, vsize, dictionary);
	gg_close(h);
	CHECK(r.rc >= 0);
	for (uint32_t g = 0; g < d.K; ++g) {
		std::vector<size_t> rows;
		double training = 0.0, with_y = 0.0;
		for (size_t i = 0; i < d.n; ++i) {
			if (d.key[i] != g || d.x_null[i]) continue;
			rows.push_back(i);
			training += d.Trains(i, with_split, drop_zero);
		}
		bool negative = false;
		for (size_t i : rows) {
			const bool t = d.Trains(i, with_split, drop_zero);
			with_y += t;
			negative = negative || (t && d.y[i] < 0.0);
		}
		CHECK(r.is_null[g] == (training < 2.0 || negative));
		if (r.is_null[g]) {
			CHECK(r.offsets[g + 1] == r.offsets[g]);
			continue;
		}
		CHECK((size_t)(r.offsets[g + 1] - r.offsets[g]) == rows.size());
		// the entries are the group's rows in some order of arrival: match each by (y, yhat), both exact
		std::vector<bool> used(rows.size(), false);
		for (int64_t e = r.offsets[g]; e < r.offsets[g + 1]; ++e) {
			const double *v = &r.vals[(size_t)e * 4];
			const uint8_t fl = r.flags[(size_t)e];
			bool found = false;
			for (size_t k = 0; k < rows.size() && !found; ++k) {
				const size_t i = rows[k];
				if (used[k]) continue;
				double s = 0.0;
				for (size_t j = 0; j < d.p; ++j) s += d.xe_null[i * d.p + j] ? NAN : d.x[i * d.p + j];
				const bool y_ok = d.y_null[i] ? (fl & 1) != 0 : (!(fl & 1) && v[0] == d.y[i]);
				const bool yhat_ok = isnan(s) ? (fl & 14) == 14 : (!(fl & 14) && v[1] == s + training && v[2] == z && v[3] == with_y);
				if (y_ok && yhat_ok && ((fl & 16) != 0) == d.Trains(i, with_split, drop_zero)) used[k] = found = true;
			}
			CHECK(found);
		}
	}
	return 0;
}

int Fails(const char *fn, const char *spec, bool ragged, const char *want) {
	Data d;
	void *h = gg_open(fn, spec, 0, 0, 1, msg);
	CHECK(h);
	Run r = GroupBy(h, d, ragged, false, 3, 64, true);
	gg_close(h);
	CHECK(r.rc == -1 && strstr(msg, want));
	msg[0] = 0;
	return 0;
}
} // namespace

int main() {
	// K = 37 states: 3 Finalize vectors of 16, 1 of 2048; ragged: two feature counts, so two calls per vector that holds both
	if (CheckFit("poisson_fit_agg", nullptr, false, false, 0, false, false, 0.0, 100.0, 0.0, 0.95, 1, 2048, false, 1)) return 1;
	if (CheckFit("anofox_stats_poisson_fit_agg", "offset=2;inference=true;glm_lambda=0.5;max_iter=9;confidence=0.5", false, false, 2, true, false, 0.5, 9.0,
	             0.0, 0.5, 3, 16, true, 3))
		return 1;
	if (CheckFit("binomial_fit_agg", "compute_inference=1;binomial_link=logit;unknown_key=3", false, true, 0, true, false, 0.0, 100.0, 1.0, 0.95, 4, 16, true, 6))
		return 1;
	if (CheckFit("binomial_fit_agg", "offset=1", true, true, 1, false, false, 0.0, 100.0, 1.0, 0.95, 2, 2048, false, 2)) return 1;
	if (CheckFit("logistic_fit_agg", "threshold=0.25;glm_lambda=2", true, false, 0, false, true, 2.0, 100.0, 1.0, 0.25, 3, 7, true, 5)) return 1; // the last vector of 7 holds only NULL groups: no call
	if (CheckFit("anofox_stats_logistic_fit_agg", "threshold=0.75;inference=true", false, false, 0, true, true, 0.0, 100.0, 1.0, 0.75, 2, 2048, true, 1)) return 1;
	if (CheckPredict("poisson_fit_predict_agg", nullptr, false, false, 1.96, 3, 16, true)) return 1;
	if (CheckPredict("poisson_fit_predict_agg", "confidence_level=0.99;offset=2;inference=true", false, false, 2.576, 1, 2048, false)) return 1;
	if (CheckPredict("anofox_stats_poisson_fit_predict_agg", nullptr, true, false, 1.96, 4, 5, true)) return 1;
	if (CheckPredict("poisson_fit_predict_agg", "confidence=0.9;null_policy=drop_y_zero_x", true, true, 1.645, 2, 64, false)) return 1;
	if (CheckPredict("poisson_fit_predict_agg", "confidence=0.8", false, false, 1.96, 2, 64, false)) return 1;
	// errors leave nothing behind: a bad offset (Finalize), a failing call, an inconsistent feature count inside a group (Update)
	if (Fails("poisson_fit_agg", "offset=4", false, "offset must be a 1-based index into x (1..=3), got 4")) return 1;
	if (Fails("logistic_fit_agg", "offset=3", true, "offset must be a 1-based index into x (1..=2), got 3")) return 1;
	g_fail = true;
	if (Fails("binomial_fit_agg", "intercept=false", false, "anofox_stats (HIP): mock: the batched call was told to fail")) return 1;
	g_fail = false;
	{
		Data d;
		for (size_t i = 0; i < d.n; ++i) d.x_len[i] = (uint32_t)(i % 2 ? d.p : d.p - 1);
		void *h = gg_open("poisson_fit_agg", nullptr, 0, 0, 1, msg);
		CHECK(h);
		Run r = GroupBy(h, d, true, false, 2, 64, false);
		gg_close(h);
		CHECK(r.rc == -1 && strstr(msg, "Inconsistent feature count: expected"));
	}
	printf("all scenarios passed\n");
	return 0;
}
