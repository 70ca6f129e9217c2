// eb_shrink_glue_sanitize.cpp — duckdb_shim/eb_shrink_hip.cpp and its test driver (eb_shrink_capi.cpp) linked with a MOCK of
// the C ABI symbols they call, for an ASan / UBSan build on a machine without a GPU (tests/test_eb_shrink_glue_cpu.py):
// registration, bind, the result type, every option spelling, Update from several threads with dictionary vectors and its NULL
// rule, Combine order, Finalize by vectors of several sizes (the LIST child reserved before it is written), NULL results, a
// failed set, a failing call, Destroy.
//
// The mock shrinks nothing: a summary holds sums over the set's pairs and echoes of the options, an output row echoes its pair.
// Every input is a small integer, so each value is exact and says which pairs and which options reached the call: routing is
// checked with ==.  The mock counts its calls: exactly one per Finalize vector that holds a state to fit.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "anofox_stats_hip.h"

static int g_calls = 0;
static bool g_fail = false;

extern "C" {
// summary = {sum est, sum se, method, tau_squared (-1 for NaN), 7, m, m, status}: status 6 for a set with a negative estimate;
// out = {est + 1, se + 2, the pair's place in its set}
bool anofox_hip_eb_shrink_batch_host(AnofoxHipContext *, int64_t S, int64_t n, const int64_t *off, size_t n_cols, const double *est, int64_t es,
                                     const double *se, int64_t ss, AnofoxHipEbShrinkOptions o, double *out, double *summary, AnofoxError *err) {
	++g_calls;
	if (g_fail || !(S > 0 && n_cols == 1 && es == 1 && ss == 1 && off && est && se && out && summary && off[0] == 0 && off[S] == n)) {
		err->code = ANOFOX_ERROR_INVALID_INPUT;
		snprintf(err->message, sizeof err->message, "%s", g_fail ? "mock: the batched call was told to fail" : "mock: malformed batch");
		return false;
	}
	for (int64_t s = 0; s < S; ++s) {
		double *r = summary + 8 * s;
		for (int k = 0; k < 8; ++k) r[k] = 0.0;
		bool negative = false;
		if (off[s + 1] - off[s] < 2) { // the glue never sends a state with fewer than 2 pairs
			err->code = ANOFOX_ERROR_INVALID_INPUT;
			snprintf(err->message, sizeof err->message, "mock: a set of fewer than 2 pairs");
			return false;
		}
		for (int64_t i = off[s]; i < off[s + 1]; ++i) {
			r[0] += est[i];
			r[1] += se[i];
			negative = negative || est[i] < 0.0;
			out[3 * i] = est[i] + 1.0;
			out[3 * i + 1] = se[i] + 2.0;
			out[3 * i + 2] = (double)(i - off[s]);
		}
		r[2] = (double)o.method;
		r[3] = isnan(o.tau_squared) ? -1.0 : o.tau_squared;
		r[4] = 7.0;
		r[5] = r[6] = (double)(off[s + 1] - off[s]);
		r[7] = negative ? 6.0 : 0.0;
	}
	return true;
}
size_t anofox_hip_eb_shrink_summary_len(void) { return 8; }
size_t anofox_hip_max_features(void) { return 128; }

// the driver's entry points (eb_shrink_capi.cpp)
void *eg_open(const char *fn_name, const char *options_spec, int as_map, int foldable, char *msg);
void eg_close(void *q);
int eg_registered(void *q, const char *name);
int eg_registered_count(void *q);
int eg_overloads(void *q, const char *name, int *out);
void eg_result_type(void *q, char *text);
int64_t eg_group_by(void *q, size_t n, const uint32_t *key, size_t n_keys, const double *est, const double *se, const uint8_t *est_null,
                    const uint8_t *se_null, int n_threads, size_t vector_size, int dictionary, size_t capacity, uint8_t *is_null, double *out_summary,
                    int64_t *out_offsets, double *out_rows, char *msg);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "eb_shrink_glue_sanitize: %s failed at line %d: %s\n", #c, __LINE__, msg); return 1; } } while (0)

namespace {
char msg[512] = "";

struct Data {
	size_t n = 1500, K = 37; // key K - 1 never occurs: its global state is never initialised
	std::vector<double> est, se;
	std::vector<uint32_t> key;
	std::vector<uint8_t> est_null, se_null;
	Data() : est(n), se(n), key(n), est_null(n, 0), se_null(n, 0) {
		for (size_t i = 0; i < n; ++i) {
			est[i] = (double)(i + 1); // the pair's name: the output echoes it, which shows the arrival order
			se[i] = (double)(i % 5 + 1);
			key[i] = (uint32_t)((i * 11) % (K - 3)); // keys 0 .. K - 4
			est_null[i] = i % 11 == 0;
			se_null[i] = i % 7 == 0;
		}
		key[n - 1] = (uint32_t)(K - 3); // a set of one pair: NULL without a call
		est_null[n - 1] = se_null[n - 1] = 0;
		key[n - 2] = key[n - 3] = (uint32_t)(K - 2); // a set of two pairs in the last Finalize vector
		est_null[n - 2] = se_null[n - 2] = est_null[n - 3] = se_null[n - 3] = 0;
		for (size_t i = 0; i < n; ++i)
			if (key[i] == 5 && !est_null[i] && !se_null[i]) {
				est[i] = -1.0; // the mock fails set 5
				break;
			}
	}
	// the pairs of set g in the order the driver makes them arrive: thread by thread (Combine), vector by vector, row by row
	std::vector<size_t> Arrival(uint32_t g, int threads, size_t vsize) const {
		std::vector<size_t> rows;
		for (int t = 0; t < threads; ++t)
			for (size_t i = 0; i < n; ++i)
				if (key[i] == g && !est_null[i] && !se_null[i] && (int)((i / vsize) % (size_t)threads) == t) rows.push_back(i);
		return rows;
	}
};

int CheckGroupBy(const char *fn, const char *spec, bool as_map, double method, double tau, int threads, size_t vsize, bool dictionary) {
	Data d;
	void *h = eg_open(fn, spec, as_map, 1, msg);
	CHECK(h);
	std::vector<uint8_t> is_null(d.K);
	std::vector<double> summary(d.K * 6), rows(d.n * 5);
	std::vector<int64_t> offsets(d.K + 1);
	g_calls = 0;
	const int64_t rc = eg_group_by(h, d.n, d.key.data(), d.K, d.est.data(), d.se.data(), d.est_null.data(), d.se_null.data(), threads, vsize, dictionary, d.n,
	                               is_null.data(), summary.data(), offsets.data(), rows.data(), msg);
	eg_close(h);
	CHECK(rc >= 0);
	CHECK(g_calls == (int)((d.K + vsize - 1) / vsize)); // one call per Finalize vector (the last vector holds a fitted state: key K - 2)
	int64_t total = 0;
	for (uint32_t g = 0; g < d.K; ++g) {
		const std::vector<size_t> pairs = d.Arrival(g, threads, vsize);
		bool negative = false;
		double se_sum = 0.0, est_sum = 0.0;
		for (size_t i : pairs) {
			negative = negative || d.est[i] < 0.0;
			est_sum += d.est[i];
			se_sum += d.se[i];
		}
		CHECK(is_null[g] == (pairs.size() < 2 || negative));
		const double *s = &summary[g * 6];
		if (is_null[g]) {
			for (int k = 0; k < 6; ++k) CHECK(isnan(s[k]));
			CHECK(offsets[g + 1] == offsets[g]);
			continue;
		}
		CHECK(s[0] == est_sum && s[1] == se_sum && s[2] == method && s[3] == tau && s[4] == 7.0 && s[5] == (double)pairs.size());
		CHECK(offsets[g + 1] - offsets[g] == (int64_t)pairs.size());
		for (size_t k = 0; k < pairs.size(); ++k) {
			const double *v = &rows[((size_t)offsets[g] + k) * 5];
			const size_t i = pairs[k];
			CHECK(v[0] == d.est[i] && v[1] == d.se[i] && v[2] == d.est[i] + 1.0 && v[3] == d.se[i] + 2.0 && v[4] == (double)k);
		}
		total += (int64_t)pairs.size();
	}
	CHECK(rc == total);
	return 0;
}

// one option spelling on a set of two pairs: summary slot 2 (method) and slot 3 (tau_squared, -1 when unset)
int CheckOption(const char *spec, bool as_map, bool foldable, double method, double tau) {
	const double est[2] = {1, 2}, se[2] = {3, 4};
	const uint32_t key[2] = {0, 0};
	void *h = eg_open("eb_shrink_agg", spec, as_map, foldable, msg);
	CHECK(h);
	uint8_t is_null[1];
	double summary[6], rows[10];
	int64_t offs[2];
	const int64_t rc = eg_group_by(h, 2, key, 1, est, se, nullptr, nullptr, 1, 8, 0, 2, is_null, summary, offs, rows, msg);
	eg_close(h);
	CHECK(rc == 2 && !is_null[0]);
	snprintf(msg, sizeof msg, "%s: method %g tau %g, want %g %g", spec, summary[2], summary[3], method, tau);
	CHECK(summary[2] == method && summary[3] == tau);
	msg[0] = 0;
	return 0;
}

} // namespace

int main() {
	// registration: the name and its alias, (estimate, se) and (estimate, se, options), nothing else; the result type
	void *h = eg_open("anofox_stats_eb_shrink_agg", nullptr, 0, 1, msg);
	CHECK(h);
	CHECK(eg_registered_count(h) == 2);
	for (const char *name : {"anofox_stats_eb_shrink_agg", "eb_shrink_agg"}) {
		int counts[8];
		CHECK(eg_registered(h, name) == 1);
		CHECK(eg_overloads(h, name, counts) == 2 && counts[0] == 2 && counts[1] == 3);
	}
	char text[512];
	eg_result_type(h, text);
	CHECK(std::string(text) == "mu:DOUBLE,mu_se:DOUBLE,tau_squared:DOUBLE,i_squared:DOUBLE,q:DOUBLE,n_groups:BIGINT,shrunken:LIST[estimate:DOUBLE,"
	                           "se:DOUBLE,shrunken:DOUBLE,shrunken_se:DOUBLE,weight:DOUBLE]");
	eg_close(h);
	// every spelling of the options
	struct { const char *spec; bool as_map, foldable; double method, tau; } options[] = {
	    {"tau_method=dl", false, true, 0, -1}, {"tau_method=dersimonian_laird", false, true, 0, -1}, {"shrinkage=dersimonian-laird", true, true, 0, -1},
	    {"TAU_METHOD=DL", false, true, 0, -1}, {"tau_method=none", false, true, 1, -1}, {"shrinkage=pooled", false, true, 1, -1},
	    {"Shrinkage=Complete", true, true, 1, -1}, {"tau_squared=0.25", false, true, 0, 0.25}, {"tau2=2", true, true, 0, 2}, {"TAU2=0.5;tau_method=none", false, true, 1, 0.5},
	    {"tau_squared=null", false, true, 0, -1}, {"something_else=3;compute_inference=true", false, true, 0, -1}, {"tau_squared=-1", false, true, 0, -1.0},
	    {"tau_method=none;tau2=3", false, false, 0, -1}, {"<null>", false, true, 0, -1}}; // (not foldable: not parsed)
	for (auto &o : options)
		if (CheckOption(o.spec, o.as_map, o.foldable, o.method, o.tau)) return 1;
	for (const char *spec : {"tau_method=reml", "shrinkage=null"}) {
		msg[0] = 0;
		CHECK(!eg_open("eb_shrink_agg", spec, 0, 1, msg));
		CHECK(std::string(msg) == (std::string(spec) == "tau_method=reml" ? "Unknown tau_method 'reml'. Expected 'dl' or 'none'." : "Unknown tau_method ''. Expected 'dl' or 'none'."));
	}
	msg[0] = 0;
	CHECK(!eg_open("eb_shrink_agg", "<scalar>", 0, 1, msg) && std::string(msg).find("Options must be a MAP or STRUCT") == 0);
	msg[0] = 0;
	h = eg_open("eb_shrink_agg", "tau_method=reml", 0, 0, msg); // not foldable: not parsed, no error
	CHECK(h);
	eg_close(h);
	// Update's NULL rule, Combine, Finalize vectors, the failed set, NULL states
	if (CheckGroupBy("anofox_stats_eb_shrink_agg", nullptr, false, 0, -1, 1, 2048, false)) return 1;
	if (CheckGroupBy("eb_shrink_agg", "tau_method=pooled;tau2=4", false, 1, 4, 3, 5, true)) return 1;
	if (CheckGroupBy("eb_shrink_agg", "shrinkage=dl", true, 0, -1, 2, 16, false)) return 1;
	if (CheckGroupBy("eb_shrink_agg", "tau2=0.5", true, 0, 0.5, 4, 7, true)) return 1;
	// a Finalize vector without a state to fit makes no call; a failing call raises the library's message
	{
		const double est[3] = {1, 2, 3}, se[3] = {1, 1, 1};
		const uint32_t key[3] = {0, 1, 2};
		uint8_t is_null[4];
		double summary[24], rows[20];
		int64_t offs[5];
		h = eg_open("eb_shrink_agg", nullptr, 0, 1, msg);
		CHECK(h);
		g_calls = 0;
		const int64_t rc = eg_group_by(h, 3, key, 4, est, se, nullptr, nullptr, 1, 8, 0, 4, is_null, summary, offs, rows, msg);
		eg_close(h);
		CHECK(rc == 0 && g_calls == 0 && is_null[0] && is_null[1] && is_null[2] && is_null[3]);
		Data d;
		std::vector<uint8_t> nul(d.K);
		std::vector<double> sm(d.K * 6), rw(d.n * 5);
		std::vector<int64_t> of(d.K + 1);
		g_fail = true;
		h = eg_open("eb_shrink_agg", nullptr, 0, 1, msg);
		CHECK(h);
		const int64_t rf = eg_group_by(h, d.n, d.key.data(), d.K, d.est.data(), d.se.data(), d.est_null.data(), d.se_null.data(), 2, 64, 0, d.n, nul.data(),
		                               sm.data(), of.data(), rw.data(), msg);
		eg_close(h);
		g_fail = false;
		CHECK(rf == -1 && std::string(msg) == "anofox_stats (HIP): mock: the batched call was told to fail");
		msg[0] = 0;
	}
	printf("eb_shrink_glue_sanitize: ok\n");
	return 0;
}
