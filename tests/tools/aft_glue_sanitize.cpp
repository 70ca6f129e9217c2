// aft_glue_sanitize.cpp — duckdb_shim/aft_family_hip.cpp and its test driver (aft_family_capi.cpp) linked with a MOCK of the
// two C ABI symbols they call, for an ASan / UBSan build on a machine without a GPU (tests/test_aft_glue_cpu.py): registration,
// bind, every option key spelling, Update from several threads with dictionary vectors and its NULL rules for both aggregates,
// Combine order, Finalize by vectors of several sizes (LIST children reserved before they are written), two feature counts in
// one Finalize vector, NULL results, a failed group, a failing call, Destroy.
//
// The mock "fits" nothing: a record holds sums over the group's rows and echoes of the options, a prediction echoes its row.
// Every input is a small integer, so each value is exact and says which rows, which columns and which options reached the
// call: routing is checked with ==.  The mock counts its calls: exactly one per Finalize vector and feature count.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "anofox_stats_hip.h"

static int g_calls = 0;
static bool g_fail = false;

// record: coefficients[j] = sum of column j (NaN entries left out), intercept = sum of the finite times, scale = sum of the
// finite events, log_likelihood = dist, null_log_likelihood = max_iterations, aic = fit_intercept, bic = confidence_level,
// n_observations = rows, n_events = rows with a NaN event, n_censored = rows with a NaN time, n_params = p + 1, iterations = 7
// (tolerance 1e-9) or 8, converged = 1, status = 1 for a group with a negative time; inference[k][j] = coefficient + k + 1,
// then 100 and 200.  pred[i] = {sum of the row's x, quantile, horizon, time}, NaN throughout for a failed group.
static bool mock(int64_t G, size_t p, int64_t n, const int64_t *off, const double *time, const double *const *cols, const double *event,
                 AnofoxHipAftBatchOptions o, const AnofoxHipAftPredictOptions *q, double *rec, double *inf, double *pred, AnofoxError *err) {
	++g_calls;
	if (g_fail || !(G > 0 && p > 0 && off && time && cols && event && rec && off[0] == 0 && off[G] == n)) {
		err->code = ANOFOX_ERROR_INVALID_INPUT;
		snprintf(err->message, sizeof err->message, "%s", g_fail ? "mock: the batched call was told to fail" : "mock: malformed batch");
		return false;
	}
	for (int64_t g = 0; g < G; ++g) {
		double *r = rec + (size_t)g * (p + 13);
		for (size_t k = 0; k < p + 13; ++k) r[k] = 0.0;
		bool negative = false;
		for (int64_t i = off[g]; i < off[g + 1]; ++i) {
			for (size_t j = 0; j < p; ++j)
				if (!isnan(cols[j][i])) r[j] += cols[j][i];
			if (!isnan(time[i])) r[p] += time[i];
			else r[p + 8] += 1.0;
			if (!isnan(event[i])) r[p + 1] += event[i];
			else r[p + 7] += 1.0;
			negative = negative || time[i] < 0.0;
		}
		r[p + 2] = (double)o.dist;
		r[p + 3] = (double)o.max_iterations;
		r[p + 4] = (double)o.fit_intercept;
		r[p + 5] = o.confidence_level;
		r[p + 6] = (double)(off[g + 1] - off[g]);
		r[p + 9] = (double)p + 1.0;
		r[p + 10] = o.tolerance == 1e-9 ? 7.0 : 8.0;
		r[p + 11] = 1.0;
		r[p + 12] = negative ? 1.0 : 0.0;
		if (inf) {
			double *f = inf + (size_t)g * (5 * p + 2);
			for (size_t k = 0; k < 5; ++k)
				for (size_t j = 0; j < p; ++j) f[k * p + j] = r[j] + (double)k + 1.0;
			f[5 * p] = 100.0;
			f[5 * p + 1] = 200.0;
		}
		if (pred)
			for (int64_t i = off[g]; i < off[g + 1]; ++i) {
				double s = 0.0;
				for (size_t j = 0; j < p; ++j) s += cols[j][i];
				double *out = pred + 4 * i;
				out[0] = negative ? NAN : s;
				out[1] = negative ? NAN : q->quantile;
				out[2] = negative ? NAN : q->horizon;
				out[3] = negative ? NAN : time[i];
			}
	}
	return true;
}

extern "C" {
bool anofox_hip_aft_fit_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *time, const double *const *cols,
                                   const double *event, AnofoxHipAftBatchOptions o, double *rec, double *inf, AnofoxError *err) {
	return mock(G, p, n, off, time, cols, event, o, nullptr, rec, inf, nullptr, err);
}
bool anofox_hip_aft_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *time,
                                           const double *const *cols, const double *event, AnofoxHipAftBatchOptions o, AnofoxHipAftPredictOptions q,
                                           double *rec, double *inf, double *pred, AnofoxError *err) {
	return pred ? mock(G, p, n, off, time, cols, event, o, &q, rec, inf, pred, err) : false;
}
size_t anofox_hip_max_features(void) { return 128; }

// the driver's entry points (aft_family_capi.cpp)
void *ag_open(const char *fn_name, const char *options_spec, int as_map, int foldable, char *msg);
void ag_close(void *q);
int ag_registered(void *q, const char *name);
int ag_registered_count(void *q);
int ag_overloads(void *q, const char *name, int *out);
int ag_result_fields(void *q, int *kinds, int *is_list, char *names);
int64_t ag_group_by(void *q, size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *time, const double *x, const double *event,
                    const uint8_t *time_null, const uint8_t *x_null, const uint8_t *xe_null, const uint8_t *event_null, const uint32_t *x_len, int n_threads,
                    size_t vector_size, int dictionary, size_t capacity, int64_t *out_offsets, double *out_vals, uint8_t *out_flags, uint8_t *is_null,
                    size_t *out_q, char *msg);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "aft_glue_sanitize: %s failed at line %d: %s\n", #c, __LINE__, msg); return 1; } } while (0)

namespace {
char msg[512] = "";

struct Data {
	size_t n = 1500, p = 3, K = 37; // key K - 1 never occurs: its global state is never initialised
	std::vector<double> time, x, event;
	std::vector<uint32_t> key, x_len;
	std::vector<uint8_t> time_null, x_null, xe_null, event_null;
	Data() : time(n), x(n * p), event(n), key(n), x_len(n), time_null(n, 0), x_null(n, 0), xe_null(n * p, 0), event_null(n, 0) {
		for (size_t i = 0; i < n; ++i) {
			time[i] = (double)(i + 1); // the row's name: the fit-predict aggregate echoes it, which shows the arrival order
			event[i] = (double)(i % 2);
			key[i] = (uint32_t)((i * 11) % (K - 2)); // keys 0 .. K - 3
			for (size_t j = 0; j < p; ++j) x[i * p + j] = (double)((i + 3 * j) % 101);
			time_null[i] = i % 11 == 0;
			x_null[i] = i % 13 == 0;
			event_null[i] = i % 7 == 0;
		}
		xe_null[40 * p + 1] = 1;        // a NULL list element: NaN in its column
		key[n - 1] = (uint32_t)(K - 2); // a group of one row
		time_null[n - 1] = x_null[n - 1] = event_null[n - 1] = 0;
		for (size_t i = 0; i < n; ++i)
			if (key[i] == 5 && !time_null[i] && !x_null[i] && !event_null[i]) {
				time[i] = -1.0; // the mock fails group 5
				break;
			}
		for (size_t i = 0; i < n; ++i) x_len[i] = (uint32_t)(key[i] % 2 ? p - 1 : p); // odd keys: two features
	}
	bool Kept(size_t i, bool predict) const { return !x_null[i] && (predict || (!time_null[i] && !event_null[i])); }
	// the rows of group g in the order the driver makes them arrive: thread by thread (Combine), vector by vector, row by row
	std::vector<size_t> Arrival(uint32_t g, bool predict, int threads, size_t vsize) const {
		std::vector<size_t> rows;
		for (int t = 0; t < threads; ++t)
			for (size_t i = 0; i < n; ++i)
				if (key[i] == g && Kept(i, predict) && (int)((i / vsize) % (size_t)threads) == t) rows.push_back(i);
		return rows;
	}
};

struct Run {
	std::vector<int64_t> offsets;
	std::vector<double> vals;
	std::vector<uint8_t> flags, is_null;
	size_t q = 0;
	int64_t rc = 0;
};

Run GroupBy(void *h, const Data &d, bool ragged, int threads, size_t vsize, bool dictionary) {
	Run r;
	r.offsets.assign(d.K + 1, 0);
	r.vals.assign(std::max(d.n * 6, d.K * (6 * d.p + 14)), 0.0);
	r.flags.assign(d.n, 0);
	r.is_null.assign(d.K, 0);
	r.rc = ag_group_by(h, d.n, d.p, d.key.data(), d.K, d.time.data(), d.x.data(), d.event.data(), d.time_null.data(), d.x_null.data(), d.xe_null.data(),
	                   d.event_null.data(), ragged ? d.x_len.data() : nullptr, threads, vsize, dictionary, r.vals.size(), r.offsets.data(), r.vals.data(),
	                   r.flags.data(), r.is_null.data(), &r.q, msg);
	return r;
}

size_t Vectors(size_t K, size_t vsize) { return (K + vsize - 1) / vsize; }

// aft_fit_agg over the data: every field of every group against the mock's definition
int CheckFit(const char *fn, const char *spec, bool as_map, bool ragged, bool inference, double dist, double max_iterations, double fit_intercept,
             double confidence, double iterations, int threads, size_t vsize, bool dictionary) {
	Data d;
	void *h = ag_open(fn, spec, as_map, 1, msg);
	CHECK(h);
	g_calls = 0;
	Run r = GroupBy(h, d, ragged, threads, vsize, dictionary);
	ag_close(h);
	CHECK(r.rc == 0);
	if (!ragged) CHECK(g_calls == (int)Vectors(d.K, vsize)); // one call per Finalize vector (the last vector holds a fitted state: key K - 2)
	else CHECK(g_calls > (int)Vectors(d.K, vsize) && g_calls <= 2 * (int)Vectors(d.K, vsize));
	const size_t width = d.p + 12 + (inference ? 5 * d.p + 2 : 0);
	CHECK(r.q == d.p);
	for (uint32_t g = 0; g < d.K; ++g) {
		const size_t pg = ragged && g % 2 ? d.p - 1 : d.p;
		const std::vector<size_t> rows = d.Arrival(g, false, 1, vsize);
		bool negative = false;
		std::vector<double> sum(pg, 0.0);
		double st = 0.0, se = 0.0;
		for (size_t i : rows) {
			for (size_t j = 0; j < pg; ++j)
				if (!d.xe_null[i * d.p + j]) sum[j] += d.x[i * d.p + j];
			st += d.time[i];
			se += d.event[i];
			negative = negative || d.time[i] < 0.0;
		}
		CHECK(r.is_null[g] == (rows.empty() || negative));
		const double *c = &r.vals[g * width];
		if (r.is_null[g]) {
			for (size_t k = 0; k < width; ++k) CHECK(isnan(c[k]));
			continue;
		}
		for (size_t j = 0; j < pg; ++j) CHECK(c[j] == sum[j]);
		for (size_t j = pg; j < d.p; ++j) CHECK(isnan(c[j]));
		const size_t q = d.p;
		CHECK(c[q] == st && c[q + 1] == se && c[q + 2] == dist && c[q + 3] == max_iterations && c[q + 4] == fit_intercept && c[q + 5] == confidence);
		CHECK(c[q + 6] == (double)rows.size() && c[q + 7] == 0.0 && c[q + 8] == 0.0); // no NaN time or event reaches the fit aggregate
		CHECK(c[q + 9] == (double)pg && c[q + 10] == iterations && c[q + 11] == 1.0);
		if (inference) {
			for (size_t k = 0; k < 5; ++k)
				for (size_t j = 0; j < pg; ++j) CHECK(c[q + 12 + k * q + j] == sum[j] + (double)k + 1.0);
			CHECK(c[6 * q + 12] == 100.0 && c[6 * q + 13] == 200.0);
		}
	}
	return 0;
}

// aft_fit_predict_agg: list length, arrival order, NULL mapping, is_training, the options' route
int CheckPredict(const char *fn, const char *spec, bool ragged, double quantile, double horizon, int threads, size_t vsize, bool dictionary) {
	Data d;
	void *h = ag_open(fn, spec, 0, 1, msg);
	CHECK(h);
	g_calls = 0;
	Run r = GroupBy(h, d, ragged, threads, vsize, dictionary);
	ag_close(h);
	CHECK(r.rc >= 0);
	CHECK(g_calls >= (int)Vectors(d.K, vsize) && g_calls <= (ragged ? 2 : 1) * (int)Vectors(d.K, vsize));
	int64_t total = 0;
	for (uint32_t g = 0; g < d.K; ++g) {
		const size_t pg = ragged && g % 2 ? d.p - 1 : d.p;
		const std::vector<size_t> rows = d.Arrival(g, true, threads, vsize);
		CHECK(r.is_null[g] == rows.empty());
		CHECK(r.offsets[g + 1] - r.offsets[g] == (int64_t)rows.size());
		bool negative = false;
		for (size_t i : rows) negative = negative || (!d.time_null[i] && d.time[i] < 0.0);
		for (size_t k = 0; k < rows.size(); ++k) {
			const size_t i = rows[k], at = (size_t)r.offsets[g] + k;
			const double *v = &r.vals[at * 6];
			const uint8_t fl = r.flags[at];
			CHECK(((fl & 1) != 0) == (d.time_null[i] != 0) && ((fl & 2) != 0) == (d.event_null[i] != 0));
			if (!d.time_null[i]) CHECK(v[0] == d.time[i]);
			if (!d.event_null[i]) CHECK(v[1] == d.event[i]);
			CHECK(((fl & 64) != 0) == (!d.time_null[i] && !d.event_null[i]));
			bool x_nan = false;
			double s = 0.0;
			for (size_t j = 0; j < pg; ++j) {
				x_nan = x_nan || d.xe_null[i * d.p + j];
				s += d.x[i * d.p + j];
			}
			if (negative) {
				CHECK((fl & 60) == 60); // a failed group: the rows with four NULL predictions
				continue;
			}
			CHECK(((fl & 4) != 0) == x_nan);
			if (!x_nan) CHECK(v[2] == s);
			CHECK(!(fl & 8) && v[3] == quantile);
			CHECK(((fl & 16) != 0) == (bool)isnan(horizon));
			if (!isnan(horizon)) CHECK(v[4] == horizon);
			CHECK(((fl & 32) != 0) == (d.time_null[i] != 0)); // the mock's risk slot echoes the time the library saw: NaN where it was NULL
			if (!d.time_null[i]) CHECK(v[5] == d.time[i]);
		}
		total += (int64_t)rows.size();
	}
	CHECK(r.rc == total);
	return 0;
}

// one option spelling: the record field at `slot` (from the coefficients' end) of a two-row group must be `want`
int CheckOption(const char *spec, bool as_map, size_t slot, double want) {
	const double time[2] = {1, 2}, x[2] = {3, 4}, event[2] = {1, 0};
	const uint32_t key[2] = {0, 0};
	void *h = ag_open("aft_fit_agg", spec, as_map, 1, msg);
	CHECK(h);
	double vals[32];
	int64_t offs[2];
	uint8_t flags[2], is_null[1];
	size_t q = 0;
	const int64_t rc = ag_group_by(h, 2, 1, key, 1, time, x, event, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 8, 0, 32, offs, vals, flags, is_null, &q, msg);
	ag_close(h);
	CHECK(rc == 0 && q == 1 && !is_null[0]);
	snprintf(msg, sizeof msg, "%s: field %zu is %g, want %g", spec, slot, vals[1 + slot], want);
	CHECK(vals[1 + slot] == want);
	msg[0] = 0;
	return 0;
}

} // namespace

int main() {
	// registration: the two names and their aliases, (time, x, event) and (time, x, event, options), nothing else
	void *h = ag_open("anofox_stats_aft_fit_agg", nullptr, 0, 1, msg);
	CHECK(h);
	CHECK(ag_registered_count(h) == 4);
	for (const char *name : {"anofox_stats_aft_fit_agg", "aft_fit_agg", "anofox_stats_aft_fit_predict_agg", "aft_fit_predict_agg"}) {
		int counts[8];
		CHECK(ag_registered(h, name) == 1);
		CHECK(ag_overloads(h, name, counts) == 2 && counts[0] == 3 && counts[1] == 4);
	}
	ag_close(h);
	// every key spelling (slots: 2 dist, 3 max_iterations, 4 fit_intercept, 5 confidence_level, 10 iterations = 8 when tolerance is not 1e-9)
	struct { const char *spec; bool as_map; size_t slot; double want; } options[] = {
	    {"dist=weibull", false, 2, 0}, {"dist=lognormal", false, 2, 1}, {"dist=log_normal", true, 2, 1}, {"DIST=Log-Normal", false, 2, 1},
	    {"dist=loglogistic", false, 2, 2}, {"distribution=log_logistic", false, 2, 2}, {"dist=log-logistic", true, 2, 2},
	    {"dist=exponential", false, 2, 3}, {"dist=exp", false, 2, 3}, {"dist=cauchy", false, 2, 0}, {"dist=null", false, 2, 0},
	    {"fit_intercept=false", false, 4, 0}, {"intercept=false", false, 4, 0}, {"intercept=0", true, 4, 0}, {"max_iterations=17", false, 3, 17},
	    {"max_iter=18", true, 3, 18}, {"confidence_level=0.5", false, 5, 0.5}, {"confidence=0.25", true, 5, 0.25}, {"tolerance=0.5", false, 10, 8},
	    {"tol=0.5", true, 10, 8}, {"tolerance=null", false, 10, 7}, {"vcov=sandwich;something_else=3", false, 10, 7}, {"quantile=0.9;horizon=3", false, 10, 7},
	    {"prior=null;priors=null", false, 10, 7}};
	for (auto &o : options)
		if (CheckOption(o.spec, o.as_map, o.slot, o.want)) return 1;
	// compute_inference / inference set the result type at bind
	for (const char *spec : {"compute_inference=true", "inference=true", "Inference=1"}) {
		int kinds[24], is_list = -1;
		char names[512];
		h = ag_open("aft_fit_agg", spec, 0, 1, msg);
		CHECK(h);
		CHECK(ag_result_fields(h, kinds, &is_list, names) == 20 && !is_list);
		ag_close(h);
	}
	// priors raise at bind with the library's text, for both aggregates and both spellings
	for (const char *fn : {"aft_fit_agg", "anofox_stats_aft_fit_predict_agg"})
		for (const char *spec : {"prior=normal", "priors=1"}) {
			msg[0] = 0;
			CHECK(!ag_open(fn, spec, 0, 1, msg) && std::string(msg) == "aft: priors are not built");
		}
	msg[0] = 0;
	// aft_fit_agg: Update's NULL rules, Combine, Finalize vectors, two feature counts, the failed group, NULL states
	if (CheckFit("anofox_stats_aft_fit_agg", nullptr, false, false, false, 0, 100, 1, 0.95, 7, 1, 2048, false)) return 1;
	if (CheckFit("aft_fit_agg", "dist=exp;max_iter=9;intercept=false;confidence=0.5;tol=0.125", false, true, false, 3, 9, 0, 0.5, 8, 3, 5, true)) return 1;
	if (CheckFit("aft_fit_agg", "inference=true;dist=log_logistic", false, true, true, 2, 100, 1, 0.95, 7, 2, 16, false)) return 1;
	if (CheckFit("aft_fit_agg", "compute_inference=1", true, false, true, 0, 100, 1, 0.95, 7, 4, 7, true)) return 1;
	// a NULL constant and options that are not constant keep the defaults; a scalar is the option visitor's error
	h = ag_open("aft_fit_agg", "<null>", 0, 1, msg);
	CHECK(h);
	ag_close(h);
	CHECK(!ag_open("aft_fit_agg", "<scalar>", 0, 1, msg) && std::string(msg).find("Options must be a MAP or STRUCT") == 0);
	msg[0] = 0;
	h = ag_open("aft_fit_agg", "prior=normal;inference=true", 0, 0, msg); // not foldable: not parsed
	CHECK(h);
	ag_close(h);
	// aft_fit_predict_agg
	if (CheckPredict("anofox_stats_aft_fit_predict_agg", nullptr, false, 0.5, NAN, 1, 2048, false)) return 1;
	if (CheckPredict("aft_fit_predict_agg", "quantile=0.25;horizon=3", true, 0.25, 3.0, 3, 5, true)) return 1;
	if (CheckPredict("aft_fit_predict_agg", "Quantile=0.75;HORIZON=0;inference=true", false, 0.75, 0.0, 2, 16, false)) return 1;
	// an inconsistent feature count inside one group raises the reference's text; a failing call raises the library's message
	{
		Data d;
		d.x_len[1] = 1; // (row 1 has an x list: one feature where its group's other rows have two)
		h = ag_open("aft_fit_predict_agg", nullptr, 0, 1, msg);
		CHECK(h);
		Run r = GroupBy(h, d, true, 1, 64, false);
		ag_close(h);
		CHECK(r.rc == -1 && std::string(msg).find("Inconsistent feature count: expected") != std::string::npos);
		msg[0] = 0;
		Data e;
		g_fail = true;
		h = ag_open("aft_fit_agg", nullptr, 0, 1, msg);
		CHECK(h);
		r = GroupBy(h, e, false, 2, 64, false);
		ag_close(h);
		g_fail = false;
		CHECK(r.rc == -1 && std::string(msg) == "anofox_stats (HIP): mock: the batched call was told to fail");
		msg[0] = 0;
	}
	printf("aft_glue_sanitize: ok\n");
	return 0;
}
