// quantile_glue_sanitize.cpp — duckdb_shim/quantile_family_hip.cpp and its test driver (quantile_family_capi.cpp) linked with
// a MOCK of the C ABI symbols they call, for an ASan / UBSan build on a machine without a GPU (tests/test_quantile_glue_cpu.py):
// registration, bind, Update from several threads with dictionary vectors, Combine both ways, Finalize by vectors of several
// sizes (LIST children reserved before they are written), two feature counts in one Finalize vector, NULL results, a failing
// call, Destroy, the window aggregate under the naive and the tree aggregator.
//
// The mock "fits" nothing: yhat of a row = (the sum of its x) + (its group's count of training rows), plus tau on the path.
// Every input is a small integer (tau a dyadic fraction), so the value is exact and says which row and which group a prediction
// came from: row routing is checked with ==.  The mock counts its calls: exactly one per Finalize vector and feature count.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <set>
#include <string>
#include <vector>

#include "duckdb.hpp"

#include "anofox_stats_hip.h"
#include "quantile_family_hip.hpp"

static int g_calls = 0;
static bool g_fail = false;
static AnofoxHipQuantileBatchOptions g_options; // what the last call was given
static const char *const kMockFailure = "mock: the batched call was told to fail";

static bool mock_check(int64_t G, size_t p, int64_t n, const int64_t *off, const double *y, const double *const *x_cols, const int64_t *train_counts,
                       AnofoxError *err) {
	++g_calls;
	if (g_fail) {
		err->code = ANOFOX_ERROR_INVALID_INPUT;
		snprintf(err->message, sizeof err->message, "%s", kMockFailure);
		return false;
	}
	bool ok = G > 0 && p > 0 && off && y && x_cols && train_counts && off[0] == 0 && off[G] == n;
	for (int64_t g = 0; ok && g < G; ++g) {
		int64_t training = 0;
		for (int64_t r = off[g]; r < off[g + 1]; ++r) training += !isnan(y[r]);
		ok = off[g + 1] > off[g] && train_counts[g] >= 2 && training <= train_counts[g];
	}
	if (!ok) {
		err->code = ANOFOX_ERROR_INVALID_INPUT;
		snprintf(err->message, sizeof err->message, "mock: malformed batch");
	}
	return ok;
}

extern "C" {
bool anofox_hip_context_create(int, AnofoxHipContext **out_ctx, AnofoxError *) {
	*out_ctx = nullptr;
	return true;
}
void anofox_hip_context_destroy(AnofoxHipContext *) {}
bool anofox_hip_context_synchronize(AnofoxHipContext *, AnofoxError *) { return true; }

bool anofox_hip_quantile_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y,
                                                const double *const *x_cols, const int64_t *train_counts, AnofoxHipQuantileBatchOptions options,
                                                double *core, double *pred, AnofoxError *err) {
	g_options = options;
	if (!mock_check(G, p, n, off, y, x_cols, train_counts, err)) return false;
	for (int64_t g = 0; g < G; ++g) {
		for (size_t k = 0; k < p + 6; ++k) core[g * (p + 6) + k] = 0.0;
		for (int64_t r = off[g]; r < off[g + 1]; ++r) {
			double s = 0.0;
			for (size_t j = 0; j < p; ++j) s += x_cols[j][r];
			pred[3 * r] = s + (double)train_counts[g];
			pred[3 * r + 1] = pred[3 * r + 2] = NAN;
		}
	}
	return true;
}
bool anofox_hip_quantile_fit_predict_path_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y,
                                                     const double *const *x_cols, const int64_t *train_counts, AnofoxHipQuantileBatchOptions options,
                                                     const double *taus, size_t T, double *rec, int32_t *, double *pred, AnofoxError *err) {
	g_options = options;
	if (!mock_check(G, p, n, off, y, x_cols, train_counts, err)) return false;
	for (int64_t g = 0; g < G; ++g) {
		for (size_t t = 0; t < T; ++t) {
			const bool valid = taus[t] > 0.0 && taus[t] < 1.0;
			double *r = rec + ((size_t)g * T + t) * (p + 6);
			for (size_t k = 0; k < p + 6; ++k) r[k] = valid ? 0.0 : NAN;
			r[p + 5] = valid ? 0.0 : 1.0;
			for (int64_t i = off[g]; i < off[g + 1]; ++i) {
				double s = 0.0;
				for (size_t j = 0; j < p; ++j) s += x_cols[j][i];
				pred[(size_t)i * T + t] = valid ? s + (double)train_counts[g] + taus[t] : NAN;
			}
		}
	}
	return true;
}

void *qg_open(int, const char *, const char *, int, int, int, char *);
void qg_close(void *);
int64_t qg_group_by(void *, size_t, size_t, const uint32_t *, size_t, const double *, const double *, const uint8_t *, const uint8_t *, const uint8_t *,
                    const uint32_t *, const uint8_t *, int, size_t, int, size_t, int64_t *, double *, uint8_t *, uint8_t *, char *);
int qg_window(void *, size_t, size_t, const double *, const double *, const uint8_t *, const uint8_t *, const uint8_t *, size_t, size_t, size_t, size_t,
              double *, uint8_t *, uint8_t *, char *);
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "quantile_glue_sanitize: %s failed at line %d: %s\n", #c, __LINE__, msg); return 1; } } while (0)

namespace {
char msg[512] = "";

struct Data {
	size_t n = 1500, p = 3, K = 37; // key K - 1 never occurs: its global state is never initialised
	std::vector<double> y, x;
	std::vector<uint32_t> key;
	std::vector<uint8_t> y_null, x_null, xe_null, split;
	Data() : y(n), x(n * p), key(n), y_null(n, 0), x_null(n, 0), xe_null(n * p, 0), split(n) {
		for (size_t i = 0; i < n; ++i) {
			y[i] = (double)(i % 50);
			key[i] = (uint32_t)((i * 11) % (K - 2)); // keys 0 .. K - 3
			for (size_t j = 0; j < p; ++j) x[i * p + j] = (double)((i + 3 * j) % 101);
			y_null[i] = i % 11 == 0;
			x_null[i] = i % 13 == 0;
			xe_null[i * p + 1] = i % 17 == 0; // a NULL list element: yhat is not finite
			split[i] = (uint8_t)(i % 7);       // every spelling of family_driver.hpp's table, and NULL
		}
		x[5 * p] = x[5 * p + 1] = 1e308;          // the sum overflows: a non-finite yhat
		key[n - 1] = (uint32_t)(K - 2);          // a group of one training row
		y_null[n - 1] = x_null[n - 1] = 0;
	}
	bool Trains(size_t i, bool with_split) const {
		static const bool split_trains[] = {false, true, true, false, true, false, true};
		return !y_null[i] && (!with_split || split_trains[split[i]]);
	}
	double SumX(size_t i) const { // NaN for a NULL element
		double s = 0.0;
		for (size_t j = 0; j < p; ++j) s += xe_null[i * p + j] ? NAN : x[i * p + j];
		return s;
	}
	// a group's buffered rows in the order the driver's threads and Combine leave them
	std::vector<size_t> Order(uint32_t g, size_t n_threads, size_t vsize) const {
		std::vector<size_t> out;
		for (size_t t = 0; t < n_threads; ++t)
			for (size_t i = 0; i < n; ++i)
				if (key[i] == g && (i / vsize) % n_threads == t && !x_null[i]) out.push_back(i);
		return out;
	}
};

// kind 0 / 1 as a threaded GROUP BY; taus: the path's grid
int GroupByScenario(const Data &d, int kind, bool with_split, bool as_map, size_t vsize, const std::vector<double> &taus) {
	const char *fn = kind == 0 ? (with_split ? "quantile_fit_predict_agg" : "anofox_stats_quantile_fit_predict_agg")
	                           : (with_split ? "anofox_stats_quantile_path_fit_predict_agg" : "quantile_path_fit_predict_agg");
	const char *spec = kind == 0 ? (as_map ? "TAU=0.25;quantile=0.9" : nullptr) : (as_map ? "taus=[0.75,0.25,null,1.5,0.25]" : "Intercept=false;taus=[0.75,0.25,null,1.5,0.25]");
	void *q = qg_open(kind, fn, spec, as_map, with_split, 1, msg);
	CHECK(q != nullptr);
	const size_t T = kind == 0 ? 1 : taus.size(), F = kind == 0 ? 2 : 3, n_threads = 4;
	std::vector<int64_t> off(d.K + 1);
	std::vector<double> vals(d.n * T * F);
	std::vector<uint8_t> flags(d.n * T), is_null(d.K);
	g_calls = 0;
	const int64_t entries = qg_group_by(q, d.n, d.p, d.key.data(), d.K, d.y.data(), d.x.data(), d.y_null.data(), d.x_null.data(), d.xe_null.data(), nullptr,
	                                    with_split ? d.split.data() : nullptr, (int)n_threads, vsize, 1, d.n * T, off.data(), vals.data(), flags.data(),
	                                    is_null.data(), msg);
	qg_close(q);
	CHECK(entries >= 0 && off[d.K] == entries);
	std::set<size_t> fitted_vectors;
	size_t fitted = 0, null_yhat = 0;
	for (uint32_t g = 0; g < d.K; ++g) {
		const std::vector<size_t> rows = d.Order(g, n_threads, vsize);
		size_t n_train = 0;
		for (size_t i : rows) n_train += d.Trains(i, with_split);
		if (n_train < 2) {
			CHECK(is_null[g] && off[g + 1] == off[g]);
			continue;
		}
		++fitted;
		fitted_vectors.insert(g / vsize);
		CHECK(!is_null[g] && (size_t)(off[g + 1] - off[g]) == rows.size() * T);
		for (size_t k = 0; k < rows.size(); ++k) {
			const size_t i = rows[k];
			for (size_t t = 0; t < T; ++t) {
				const size_t at = (size_t)off[g] + k * T + t;
				const double *v = &vals[at * F];
				const uint8_t fl = flags[at];
				CHECK(((fl & 16) != 0) == d.Trains(i, with_split));
				CHECK(((fl & 1) != 0) == (d.y_null[i] != 0) && (d.y_null[i] || v[0] == d.y[i]));
				double want = d.SumX(i) + (double)n_train;
				if (kind == 1) {
					const bool tau_null = isnan(taus[t]);
					CHECK(((fl & 2) != 0) == tau_null && (tau_null || v[1] == taus[t]));
					want = taus[t] > 0.0 && taus[t] < 1.0 ? want + taus[t] : NAN;
				}
				const uint8_t yhat_bit = kind == 0 ? 2 : 4;
				CHECK(((fl & yhat_bit) != 0) == !isfinite(want) && (!isfinite(want) || v[F - 1] == want));
				null_yhat += !isfinite(want);
			}
		}
	}
	CHECK(is_null[d.K - 1] && is_null[d.K - 2]); // never initialised; one training row
	CHECK(fitted > 0 && null_yhat > 0);
	CHECK(g_calls == (int)fitted_vectors.size()); // ONE batched call per Finalize vector (every group has p features)
	return 0;
}

// the options a call receives: the defaults, the aliases in any case, MAP and STRUCT; `quantile` (the key of the reference's own
// example) is ignored, so the call is given what a query without options gives it
int OptionsScenario(const Data &d) {
	struct Case {
		const char *spec;
		int as_map;
		double tau;
		bool fit_intercept;
		uint32_t max_iterations;
		double tolerance;
	};
	const Case cases[] = {{nullptr, 0, 0.5, true, 1000, 1e-6},
	                      {"quantile=0.9", 0, 0.5, true, 1000, 1e-6},
	                      {"quantile=0.9", 1, 0.5, true, 1000, 1e-6},
	                      {"TAU=0.25;Intercept=false;max_iter=7;tol=0.5", 0, 0.25, false, 7, 0.5},
	                      {"tau=1.5;fit_intercept=0;max_iterations=9;tolerance=0.25", 1, 1.5, false, 9, 0.25}};
	for (int kind : {0, 2}) {
		for (const Case &c : cases) {
			void *q = qg_open(kind, kind == 0 ? "quantile_fit_predict_agg" : "quantile_fit_predict", c.spec, c.as_map, 0, 1, msg);
			CHECK(q != nullptr);
			const size_t n = 64;
			std::vector<uint32_t> key(n, 0);
			std::vector<int64_t> off(2);
			std::vector<double> vals(n * 3);
			std::vector<uint8_t> flags(n), is_null(n);
			memset(&g_options, 0, sizeof g_options);
			if (kind == 0)
				CHECK(qg_group_by(q, n, d.p, key.data(), 1, d.y.data(), d.x.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 1, 16, 0, n, off.data(),
				                  vals.data(), flags.data(), is_null.data(), msg) == (int64_t)n);
			else
				CHECK(qg_window(q, n, d.p, d.y.data(), d.x.data(), nullptr, nullptr, nullptr, 4, 0, 0, 16, vals.data(), flags.data(), is_null.data(), msg) == 0);
			qg_close(q);
			CHECK(g_options.tau == c.tau && g_options.fit_intercept == c.fit_intercept && g_options.max_iterations == c.max_iterations &&
			      g_options.tolerance == c.tolerance);
		}
	}
	return 0;
}

int FailureScenario(const Data &d) {
	for (int kind = 0; kind < 2; ++kind) {
		void *q = qg_open(kind, kind == 0 ? "quantile_fit_predict_agg" : "quantile_path_fit_predict_agg", kind == 0 ? nullptr : "taus=[0.5]", 0, 0, 1, msg);
		CHECK(q != nullptr);
		std::vector<int64_t> off(d.K + 1);
		std::vector<double> vals(d.n * 3);
		std::vector<uint8_t> flags(d.n), is_null(d.K);
		g_fail = true;
		const int64_t entries = qg_group_by(q, d.n, d.p, d.key.data(), d.K, d.y.data(), d.x.data(), d.y_null.data(), d.x_null.data(), d.xe_null.data(),
		                                    nullptr, nullptr, 2, 64, 0, d.n, off.data(), vals.data(), flags.data(), is_null.data(), msg);
		g_fail = false;
		qg_close(q);
		CHECK(entries == -1 && strstr(msg, kMockFailure) != nullptr); // the exception carries the library's message
	}
	return 0;
}

int WindowScenario(const Data &d) {
	for (const char *fn : {"anofox_stats_quantile_fit_predict", "quantile_fit_predict"}) {
		const bool with_options = fn[0] == 'q';
		void *q = qg_open(2, fn, with_options ? "tau=0.75;max_iter=50" : nullptr, 0, 0, 1, msg);
		CHECK(q != nullptr);
		const size_t n = 300, preceding = 6, vsize = 32;
		std::vector<double> out(n * 3);
		std::vector<uint8_t> flags(n), is_null(n);
		g_calls = 0;
		CHECK(qg_window(q, n, d.p, d.y.data(), d.x.data(), d.y_null.data(), d.x_null.data(), d.xe_null.data(), preceding, 0, 0, vsize, out.data(), flags.data(),
		                is_null.data(), msg) == 0);
		std::set<size_t> fitted_vectors;
		size_t nulls = 0;
		for (size_t o = 0; o < n; ++o) {
			size_t n_train = 0;
			for (size_t r = o >= preceding ? o - preceding : 0; r <= o; ++r) n_train += !d.x_null[r] && !d.y_null[r];
			const bool fit = n_train >= 2 && !d.x_null[o];
			if (fit) fitted_vectors.insert(o / vsize);
			const double want = fit ? d.SumX(o) + (double)n_train : NAN;
			CHECK((is_null[o] != 0) == !isfinite(want));
			nulls += is_null[o];
			if (!is_null[o]) CHECK(out[3 * o] == want && flags[o] == 6); // both bounds are always NULL
		}
		CHECK(nulls > 0 && nulls < n && is_null[0]);
		CHECK(g_calls == (int)fitted_vectors.size());
		// the segment tree: leaves of 8 rows combined (PRESERVE_INPUT) into frames of 3 leaves, each leaf feeding up to 3 frames
		const size_t leaf = 8, back = 2, n_leaves = (n + leaf - 1) / leaf;
		std::vector<double> tout(n_leaves * 3);
		std::vector<uint8_t> tflags(n_leaves), tnull(n_leaves);
		g_calls = 0;
		CHECK(qg_window(q, n, d.p, d.y.data(), d.x.data(), d.y_null.data(), d.x_null.data(), d.xe_null.data(), 0, leaf, back, 16, tout.data(), tflags.data(),
		                tnull.data(), msg) == 0);
		qg_close(q);
		for (size_t o = 0; o < n_leaves; ++o) {
			const size_t lo = (o >= back ? o - back : 0) * leaf, hi = std::min(n, (o + 1) * leaf);
			// Combine keeps the current row of the latest leaf whose last row has an x (rls_family_hip.cpp's rule)
			size_t n_train = 0, last = SIZE_MAX;
			for (size_t r = lo; r < hi; ++r) n_train += !d.x_null[r] && !d.y_null[r];
			for (size_t l = lo / leaf; l * leaf < hi; ++l) {
				const size_t end = std::min(n, (l + 1) * leaf) - 1;
				if (!d.x_null[end]) last = end;
			}
			const double want = n_train >= 2 && last != SIZE_MAX ? d.SumX(last) + (double)n_train : NAN;
			CHECK((tnull[o] != 0) == !isfinite(want));
			if (!tnull[o]) CHECK(tout[3 * o] == want && tflags[o] == 6);
		}
		CHECK(g_calls == (int)((n_leaves + 15) / 16));
	}
	return 0;
}

// states of two feature counts (and one never initialised) in ONE Finalize vector, from Update vectors built here
int MixedWidthScenario() {
	using namespace duckdb;
	ExtensionLoader loader;
	RegisterHipQuantileFitPredictAggregateFunction(loader);
	auto &set = loader.registered.at("anofox_stats_quantile_fit_predict_agg").functions.functions;
	const AggregateFunction *pick = nullptr;
	for (auto &f : set)
		if (f.arguments.size() == 2) pick = &f;
	CHECK(pick != nullptr);
	AggregateFunction fn(*pick);
	ClientContext context;
	vector<unique_ptr<Expression>> args;
	args.push_back(make_uniq<Expression>(Value(), false));
	args.push_back(make_uniq<Expression>(Value(), false));
	auto bind = fn.bind(context, fn, args);
	ArenaAllocator alloc;
	AggregateInputData aid(bind.get(), alloc);
	const size_t n_states = 5, widths[n_states] = {2, 3, 2, 0, 3}; // state 3 sees no row
	std::vector<std::vector<data_t>> storage(n_states, std::vector<data_t>(fn.state_size(fn)));
	std::vector<data_ptr_t> states(n_states);
	for (size_t s = 0; s < n_states; ++s) {
		states[s] = storage[s].data();
		fn.initialize(fn, states[s]);
	}
	auto pointers = [&](const std::vector<data_ptr_t> &ptrs) {
		Vector v(LogicalType(LogicalType::POINTER), ptrs.size());
		memcpy(FlatVector::GetData<data_ptr_t>(v), ptrs.data(), ptrs.size() * sizeof(data_ptr_t));
		return v;
	};
	// rows r = 0 .. 11 go to state r % 5 (never 3); row r's x = {r, r + 1, ...} as wide as its state
	std::vector<size_t> row_state;
	for (size_t r = 0; r < 15; ++r)
		if (r % n_states != 3) row_state.push_back(r % n_states);
	const size_t cnt = row_state.size();
	auto update = [&](const std::vector<size_t> &lens) {
		std::vector<Vector> inputs;
		inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
		inputs.emplace_back(LogicalType::LIST(LogicalType::DOUBLE), cnt);
		size_t total = 0;
		for (size_t len : lens) total += len;
		ListVector::Reserve(inputs[1], total);
		size_t off = 0;
		std::vector<data_ptr_t> sp(cnt);
		for (size_t i = 0; i < cnt; ++i) {
			FlatVector::GetData<double>(inputs[0])[i] = (double)i;
			ListVector::GetData(inputs[1])[i] = list_entry_t {off, lens[i]};
			for (size_t j = 0; j < lens[i]; ++j) FlatVector::GetData<double>(ListVector::GetEntry(inputs[1]))[off + j] = (double)(i + j);
			off += lens[i];
			sp[i] = states[row_state[i]];
		}
		ListVector::SetListSize(inputs[1], total);
		Vector sv = pointers(sp);
		fn.update(inputs.data(), aid, inputs.size(), sv, cnt);
	};
	std::vector<size_t> lens(cnt);
	for (size_t i = 0; i < cnt; ++i) lens[i] = widths[row_state[i]];
	update(lens);
	Vector result(fn.return_type, n_states);
	Vector sv = pointers(states);
	g_calls = 0;
	fn.finalize(sv, aid, result, n_states, 0);
	CHECK(g_calls == 2); // one call per distinct feature count of the vector
	auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
	for (size_t s = 0; s < n_states; ++s) {
		const bool valid = FlatVector::Validity(result).RowIsValid(s);
		CHECK(valid == (s != 3));
		if (!valid) continue;
		const list_entry_t e = ListVector::GetData(result)[s];
		CHECK(e.length == 3 && e.offset + e.length <= ListVector::GetListCapacity(result));
		size_t k = 0;
		for (size_t i = 0; i < cnt; ++i) {
			if (row_state[i] != s) continue;
			double want = 3.0; // the group's three training rows
			for (size_t j = 0; j < widths[s]; ++j) want += (double)(i + j);
			CHECK(FlatVector::GetData<double>(*fields[0])[e.offset + k] == (double)i && FlatVector::GetData<double>(*fields[1])[e.offset + k] == want &&
			      FlatVector::GetData<bool>(*fields[2])[e.offset + k]);
			++k;
		}
	}
	// a state that sees another feature count: the reference's error text
	bool threw = false;
	try {
		std::vector<size_t> wrong(lens);
		wrong[0] = widths[row_state[0]] + 1;
		update(wrong);
	} catch (const std::exception &e) {
		threw = true;
		snprintf(msg, sizeof msg, "%s", e.what());
	}
	CHECK(threw && strcmp(msg, "Inconsistent feature count: expected 2, got 3") == 0);
	// a 2-feature state combined into a 3-feature state: the reference's text, without the counts
	threw = false;
	try {
		Vector source = pointers({states[0]}), target = pointers({states[1]});
		fn.combine(source, target, aid, 1);
	} catch (const std::exception &e) {
		threw = true;
		snprintf(msg, sizeof msg, "%s", e.what());
	}
	CHECK(threw && strcmp(msg, "Cannot combine states with different feature counts") == 0);
	fn.destructor(sv, aid, n_states);
	return 0;
}
} // namespace

int main() {
	const Data d;
	const std::vector<double> taus = {0.75, 0.25, NAN, 1.5, 0.25};
	for (int kind = 0; kind < 2; ++kind)
		for (int with_split = 0; with_split < 2; ++with_split)
			for (size_t vsize : {(size_t)5, (size_t)16, (size_t)64})
				if (GroupByScenario(d, kind, with_split != 0, vsize == 16, vsize, taus)) return 1;
	if (OptionsScenario(d) || FailureScenario(d) || WindowScenario(d) || MixedWidthScenario()) return 1;
	printf("quantile_glue_sanitize: all scenarios passed\n");
	return 0;
}
