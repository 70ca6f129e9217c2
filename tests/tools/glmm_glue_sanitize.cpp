// glmm_glue_sanitize.cpp — duckdb_shim/glmm_family_hip.cpp and its test driver (glmm_family_capi.cpp) linked with a MOCK of the
// two C ABI symbols they call, for an ASan / UBSan build on a machine without a GPU (tests/test_glmm_glue_cpu.py): registration,
// bind, Update from several threads with dictionary vectors and its NULL rules for both aggregates and the three group types,
// Combine's renumbering of the levels, Finalize by vectors of several sizes, two feature counts in one Finalize vector, NULL
// results, a failed panel, a failing call, Destroy.
//
// The mock "fits" nothing: a record holds sums over the panel's rows and echoes of the options, a BLUP is the sum of its level's
// y, a prediction echoes its row.  Every input is a small integer, so each value is exact and says which rows reached which
// level of which panel: routing is checked with ==.  The mock counts its calls: one per Finalize vector and feature count.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <vector>

#include "anofox_stats_hip.h"

static int g_calls = 0;
static bool g_fail = false;

// record: coefficients[j] = sum of column j, intercept = sum of the finite y, var_group = number of levels, var_residual = reml,
// icc = fit_intercept, log_likelihood = max_iterations, aic = interval (-1 for a fit), bic = level, deviance = confidence_level,
// n_observations = rows with a finite y, n_groups = levels with one, iterations 7, converged 1, status 1 for a panel with a
// negative y.  ranef[l] = sum of the level's finite y (NaN without one), level_n[l] = their count.
// pred[i] = {sum of the row's x, the row's level within its panel, 0, interval ? -1 : NaN, interval ? y or -2 : NaN}.
static bool mock(int64_t G, int64_t L, size_t p, int64_t n, const int64_t *plo, const int64_t *lro, const double *y, const double *const *cols,
                 AnofoxHipGlmmOptions o, const AnofoxHipGlmmPredictOptions *q, double *rec, double *inf, double *ranef, int64_t *level_n, double *pred,
                 AnofoxError *err) {
	++g_calls;
	bool ok = !g_fail && G > 0 && p > 0 && plo && lro && y && cols && rec && ranef && plo[0] == 0 && plo[G] == L && lro[0] == 0 && lro[L] == n;
	for (int64_t l = 0; ok && l < L; ++l) ok = lro[l] < lro[l + 1]; // the glue makes no level without a row
	if (!ok) {
		err->code = ANOFOX_ERROR_INVALID_INPUT;
		snprintf(err->message, sizeof err->message, "%s", g_fail ? "mock: the batched call was told to fail" : "mock: malformed batch");
		return false;
	}
	for (int64_t g = 0; g < G; ++g) {
		double *r = rec + (size_t)g * (p + 13);
		for (size_t k = 0; k < p + 13; ++k) r[k] = 0.0;
		bool negative = false;
		for (int64_t l = plo[g]; l < plo[g + 1]; ++l) {
			double s = 0.0;
			int64_t c = 0;
			for (int64_t i = lro[l]; i < lro[l + 1]; ++i) {
				for (size_t j = 0; j < p; ++j)
					if (!isnan(cols[j][i])) r[j] += cols[j][i];
				if (!isnan(y[i])) {
					s += y[i];
					++c;
					negative = negative || y[i] < 0.0;
				}
				if (pred) {
					double sx = 0.0;
					for (size_t j = 0; j < p; ++j) sx += cols[j][i];
					double *out = pred + 5 * i;
					out[0] = sx;
					out[1] = (double)(l - plo[g]);
					out[2] = 0.0;
					out[3] = q->interval ? -1.0 : NAN;
					out[4] = q->interval ? (isnan(y[i]) ? -2.0 : y[i]) : NAN;
				}
			}
			ranef[l] = c ? s : NAN;
			if (level_n) level_n[l] = c;
			r[p] += s;
			r[p + 8] += (double)c;
			r[p + 9] += c ? 1.0 : 0.0;
		}
		r[p + 1] = (double)(plo[g + 1] - plo[g]);
		r[p + 2] = (double)o.reml;
		r[p + 3] = (double)o.fit_intercept;
		r[p + 4] = (double)o.max_iterations;
		r[p + 5] = q ? (double)q->interval : -1.0;
		r[p + 6] = q ? q->level : 0.0;
		r[p + 7] = o.confidence_level;
		r[p + 10] = 7.0;
		r[p + 11] = 1.0;
		r[p + 12] = negative ? 1.0 : 0.0;
		if (inf)
			for (size_t k = 0; k < 5 * p + 1; ++k) inf[(size_t)g * (5 * p + 1) + k] = (double)k + 100.0;
	}
	return true;
}

extern "C" {
bool anofox_hip_glmm_fit_batch_host(AnofoxHipContext *, int64_t G, int64_t L, size_t p, int64_t n, const int64_t *plo, const int64_t *lro, const double *y,
                                    const double *const *cols, AnofoxHipGlmmOptions o, double *rec, double *inf, double *ranef, int64_t *level_n,
                                    AnofoxError *err) {
	return mock(G, L, p, n, plo, lro, y, cols, o, nullptr, rec, inf, ranef, level_n, nullptr, err);
}
bool anofox_hip_glmm_fit_predict_batch_host(AnofoxHipContext *, int64_t G, int64_t L, size_t p, int64_t n, const int64_t *plo, const int64_t *lro,
                                            const double *y, const double *const *cols, AnofoxHipGlmmOptions o, AnofoxHipGlmmPredictOptions q, double *rec,
                                            double *inf, double *ranef, int64_t *level_n, double *pred, AnofoxError *err) {
	return pred ? mock(G, L, p, n, plo, lro, y, cols, o, &q, rec, inf, ranef, level_n, pred, err) : false;
}
size_t anofox_hip_max_features(void) { return 128; }

// the driver's entry points (glmm_family_capi.cpp)
void *ag_open(const char *fn_name, const char *options_spec, int as_map, int foldable, int group_kind, int with_split, char *msg);
void ag_close(void *q);
int ag_registered_count(void *q);
int64_t ag_group_by(void *q, size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *y, const double *x, const int64_t *group,
                    const uint8_t *y_null, const uint8_t *x_null, const uint8_t *xe_null, const uint8_t *group_null, const uint8_t *split_train,
                    const uint8_t *split_null, const uint32_t *x_len, int n_threads, size_t vector_size, int dictionary, size_t capacity,
                    int64_t *out_offsets, double *out_vals, uint8_t *out_flags, uint8_t *is_null, size_t *out_q, size_t ranef_capacity, double *out_ranef,
                    char *msg);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "glmm_glue_sanitize: %s failed at line %d: %s\n", #c, __LINE__, msg); return 1; } } while (0)

namespace {
char msg[512] = "";

struct Data {
	size_t n = 1200, p = 2, K = 9; // key K - 1 never occurs: its global state is never initialised; key K - 2 has three features
	std::vector<double> y, x;
	std::vector<int64_t> group;
	std::vector<uint32_t> key, x_len;
	std::vector<uint8_t> y_null, x_null, group_null, split_train;
	Data() : y(n), x(n * p), group(n), key(n), x_len(n, 2), y_null(n, 0), x_null(n, 0), group_null(n, 0), split_train(n, 1) {
		for (size_t i = 0; i < n; ++i) {
			y[i] = (double)(i + 1); // the row's name: the fit-predict aggregate echoes it, which shows the arrival order
			key[i] = (uint32_t)((i * 5) % (K - 2));
			group[i] = (int64_t)(100 + (i * 7) % 13); // thirteen levels, met in another order by every key and thread
			for (size_t j = 0; j < p; ++j) x[i * p + j] = (double)((i + 3 * j) % 11);
			y_null[i] = i % 11 == 0;
			x_null[i] = i % 13 == 0;
			group_null[i] = i % 17 == 0;
			split_train[i] = i % 3 != 0;
		}
		for (size_t i = 0; i < n; ++i)
			if (key[i] == 3 && !y_null[i] && !x_null[i] && !group_null[i] && split_train[i]) {
				y[i] = -1.0; // the mock fails key 3
				break;
			}
		for (size_t i = n - 40; i < n; ++i) { // a key with three features (the third is 0)
			key[i] = (uint32_t)(K - 2);
			x_len[i] = 3;
		}
	}
};

struct Out {
	std::vector<int64_t> offsets;
	std::vector<double> vals, ranef;
	std::vector<uint8_t> flags, is_null;
	size_t q = 0;
	int64_t r = 0;
};

Out run(void *q, const Data &d, bool split, int threads, size_t vs, bool dict) {
	Out o;
	const size_t cap = d.n * 8 + 64;
	o.offsets.assign(d.K + 1, 0);
	o.vals.assign(cap * 5, NAN);
	o.ranef.assign((d.n + 1) * 4, NAN);
	o.flags.assign(cap, 0);
	o.is_null.assign(d.K, 0);
	o.r = ag_group_by(q, d.n, d.p, d.key.data(), d.K, d.y.data(), d.x.data(), d.group.data(), d.y_null.data(), d.x_null.data(), nullptr,
	                  d.group_null.data(), split ? d.split_train.data() : nullptr, nullptr, d.x_len.data(), threads, vs, dict, cap, o.offsets.data(),
	                  o.vals.data(), o.flags.data(), o.is_null.data(), &o.q, d.n + 1, o.ranef.data(), msg);
	return o;
}
} // namespace

int main() {
	Data d;
	for (int kind = 0; kind < 3; ++kind) {
		// ---- glmm_fit_agg ----
		void *q = ag_open(kind ? "glmm_fit_agg" : "anofox_stats_glmm_fit_agg", "compute_inference=true;reml=false;max_iter=50", kind == 1, 1, kind, 0, msg);
		CHECK(q);
		CHECK(ag_registered_count(q) == 4);
		const size_t vs = kind == 0 ? 3 : (kind == 1 ? 64 : 2048);
		g_calls = 0;
		Out o = run(q, d, false, kind + 1, vs, kind != 1);
		CHECK(o.r == 0 && o.q == 3);
		CHECK(g_calls >= 1 && g_calls <= (int)((d.K + vs - 1) / vs) + 1); // one call per Finalize vector and feature count (one key has three)
		const size_t width = o.q + 17 + 5 * o.q + 1;
		for (size_t k = 0; k < d.K; ++k) {
			CHECK(o.is_null[k] == (k == 3 || k == d.K - 1));
			if (o.is_null[k]) continue;
			// what the rows of key k add up to, by the fit aggregate's NULL rule, and the levels in first-seen order
			double sum_y = 0.0, cnt = 0.0, sx0 = 0.0;
			std::vector<int64_t> seen;
			std::map<int64_t, double> level_sum;
			for (size_t i = 0; i < d.n; ++i) {
				if (d.key[i] != k || d.y_null[i] || d.x_null[i] || d.group_null[i]) continue;
				sum_y += d.y[i];
				cnt += 1.0;
				sx0 += d.x[i * d.p];
				if (!level_sum.count(d.group[i])) seen.push_back(d.group[i]);
				level_sum[d.group[i]] += d.y[i];
			}
			const double *c = &o.vals[k * width];
			CHECK(c[0] == sx0 && c[o.q] == sum_y && c[o.q + 8] == cnt && c[o.q + 1] == (double)seen.size() && c[o.q + 9] == (double)seen.size());
			CHECK(c[o.q + 2] == 0.0 && c[o.q + 4] == 50.0 && c[o.q + 5] == -1.0 && c[o.q + 10] == (k == d.K - 2 ? 3.0 : 2.0) && c[o.q + 11] == 7.0);
			CHECK(c[o.q + 13] == c[o.q + 1] && c[o.q + 14] == 1.0 && c[o.q + 15] == 1.0 && c[o.q + 16] == 0.0 && c[o.q + 17] == 100.0);
			CHECK((size_t)(o.offsets[k + 1] - o.offsets[k]) == seen.size());
			if (kind + 1 == 1) // one thread: arrival order is row order, so the levels come in the order the rows first name them
				for (size_t j = 0; j < seen.size(); ++j) CHECK(o.ranef[4 * (o.offsets[k] + j)] == (double)seen[j]);
			for (int64_t e = o.offsets[k]; e < o.offsets[k + 1]; ++e) {
				const int64_t id = (int64_t)o.ranef[4 * e];
				CHECK(level_sum.count(id) && o.ranef[4 * e + 1] == level_sum[id] && isnan(o.ranef[4 * e + 2]) && o.ranef[4 * e + 3] > 0.0);
			}
		}
		ag_close(q);
		// ---- glmm_fit_predict_agg, with and without the split column ----
		for (int split = 0; split < 2; ++split) {
			q = ag_open(kind ? "glmm_fit_predict_agg" : "anofox_stats_glmm_fit_predict_agg", split ? "interval=confidence;level=0.9" : nullptr, 0, 1, kind, split, msg);
			CHECK(q);
			o = run(q, d, split != 0, 3, vs, split != 0);
			CHECK(o.r > 0);
			for (size_t k = 0; k < d.K; ++k) {
				CHECK(o.is_null[k] == (k == 3 || k == d.K - 1));
				if (o.is_null[k]) continue;
				size_t rows = 0;
				for (size_t i = 0; i < d.n; ++i) rows += d.key[i] == k && !d.x_null[i] && !d.group_null[i];
				CHECK((size_t)(o.offsets[k + 1] - o.offsets[k]) == rows);
			}
			// every entry echoes a row: its y names it, its prediction is its own x, its training flag its own rule
			for (int64_t e = 0; e < o.r; ++e) {
				const double *v = &o.vals[5 * e];
				const uint8_t fl = o.flags[e];
				if (fl & 1) { // a NULL y: a prediction row
					CHECK(!(fl & 64) && (split ? v[4] == -2.0 : (fl & 16)));
					continue;
				}
				const size_t i = (size_t)v[0] - 1;
				CHECK(i < d.n && !d.y_null[i] && v[1] == d.x[i * d.p] + d.x[i * d.p + 1]);
				CHECK(((fl & 64) != 0) == (split ? d.split_train[i] != 0 : true));
				if (split) CHECK(v[3] == -1.0 && v[4] == ((fl & 64) ? d.y[i] : -2.0));
				else CHECK((fl & 8) && (fl & 16));
			}
			ag_close(q);
		}
	}
	// a failing call raises with the library's text; what is not built raises at bind
	void *q = ag_open("glmm_fit_agg", nullptr, 0, 1, 1, 0, msg);
	CHECK(q);
	g_fail = true;
	Out o = run(q, d, false, 2, 64, false);
	CHECK(o.r == -1 && strstr(msg, "mock: the batched call was told to fail"));
	g_fail = false;
	ag_close(q);
	CHECK(!ag_open("glmm_fit_agg", "family=poisson", 0, 1, 0, 0, msg) && !strcmp(msg, "glmm: the poisson family is not built"));
	printf("glmm_glue_sanitize: ok\n");
	return 0;
}
