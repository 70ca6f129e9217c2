// aft_family_hip.cpp — DuckDB glue of the accelerated failure time (AFT) family over the batched C ABI:
//
//   anofox_stats_aft_fit_agg(time, x, event[, options])          src/aggregate_functions/aft_aggregate.cpp (bind data :56-82,
//                                                                result type :86-112, Update :140-190, Finalize :246-330)
//   anofox_stats_aft_fit_predict_agg(time, x, event[, options])  NO COUNTERPART in the reference, which stops at the fit and the
//                                                                two scalars: the fit and a score for every buffered row
//
// As the other glue files: the DuckDB state buffers the group's rows on the host in arrival order (time in RowBuffer::y, the
// event column in RowBuffer::w), Combine appends the source's rows after the target's, and Finalize turns the whole vector of
// states into ONE batched call per feature count where the reference makes one anofox_aft_fit call per group:
// anofox_hip_aft_fit_batch_host and anofox_hip_aft_fit_predict_batch_host.  The glue adds no arithmetic.
//
// Options (RegressionMapOptions::ParseFromValue), STRUCT or MAP literal, keys case-insensitive, unknown keys ignored, options
// that are not constant keep the defaults: dist / distribution (weibull, lognormal / log_normal / log-normal, loglogistic /
// log_logistic / log-logistic, exponential / exp; a name that is none of them is left unread, map_options_parser.cpp:420-423,
// 694-701), fit_intercept / intercept, compute_inference / inference, confidence_level / confidence, max_iterations / max_iter,
// tolerance / tol; the fit-predict aggregate also reads quantile and horizon.  A non-NULL prior / priors raises at bind with the
// library's "aft: priors are not built".  vcov is accepted and ignored: without priors every vcov is one matrix.
//
// NULL rules.  aft_fit_agg skips a row when time, x or event is NULL (:160-163).  aft_fit_predict_agg keeps a row whose event or
// time is NULL: it reaches the library as NaN, which the fit's own row rule leaves out and the prediction pass scores, and it is
// NULL again in the output; only a NULL x list drops the row.  Combine's text on two feature counts is row_glue.hpp's, not the
// reference's ("Inconsistent feature count during combine", :221).
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU with
// the real library (tests/test_gpu_aft_glue.py through tests/tools/aft_family_capi.cpp).
#include <math.h>
#include <string.h>

#include "duckdb.hpp"
#include "duckdb/common/types/data_chunk.hpp"
#include "duckdb/execution/expression_executor.hpp"
#include "duckdb/function/aggregate_function.hpp"
#include "duckdb/main/extension/extension_loader.hpp"
#include "duckdb/parser/parsed_data/create_aggregate_function_info.hpp"

#include "anofox_stats_hip.h"
#include "aft_family_hip.hpp"
#include "hip_options.hpp"
#include "row_shapes.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "survival"};
constexpr uint8_t kEventNull = 4; // beside row_glue.hpp's kYNull (the time) and kTraining

enum class AftKind : uint8_t { FIT, PREDICT };

struct HipAftOptions {
	int dist = ANOFOX_AFT_WEIBULL;  // aft_aggregate.cpp:58
	bool fit_intercept = true;      // :59
	uint32_t max_iterations = 100;  // :60
	double tolerance = 1e-9;        // :61
	bool compute_inference = false; // :62
	double confidence_level = 0.95; // :63
	double quantile = 0.5;          // the fit-predict aggregate
	double horizon = NAN;           // NaN: risk is not asked for
	bool operator==(const HipAftOptions &o) const {
		return dist == o.dist && fit_intercept == o.fit_intercept && max_iterations == o.max_iterations && tolerance == o.tolerance &&
		       compute_inference == o.compute_inference && confidence_level == o.confidence_level && quantile == o.quantile &&
		       ((isnan(horizon) && isnan(o.horizon)) || horizon == o.horizon);
	}
	AnofoxHipAftBatchOptions Batch() const {
		AnofoxHipAftBatchOptions b;
		memset(&b, 0, sizeof b);
		b.dist = dist;
		b.fit_intercept = fit_intercept;
		b.max_iterations = max_iterations;
		b.tolerance = tolerance;
		b.compute_inference = compute_inference;
		b.confidence_level = confidence_level;
		return b;
	}
};

// IsAftDistName / ParseAftDist (map_options_parser.cpp:405-423): false for a name that is no AFT distribution
bool ParseAftDist(const string &v, int &dist) {
	if (v == "weibull") dist = ANOFOX_AFT_WEIBULL;
	else if (v == "lognormal" || v == "log_normal" || v == "log-normal") dist = ANOFOX_AFT_LOGNORMAL;
	else if (v == "loglogistic" || v == "log_logistic" || v == "log-logistic") dist = ANOFOX_AFT_LOGLOGISTIC;
	else if (v == "exponential" || v == "exp") dist = ANOFOX_AFT_EXPONENTIAL;
	else return false;
	return true;
}

void ParseHipAftOptions(const Value &v, AftKind kind, HipAftOptions &o) {
	if (v.IsNull()) return;
	bool has_prior = false;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (val.IsNull()) return;
		if (key == "dist" || key == "distribution") ParseAftDist(OptionString(val), o.dist);
		else if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(val);
		else if (key == "compute_inference" || key == "inference") o.compute_inference = ExtractBool(val);
		else if (key == "confidence_level" || key == "confidence") o.confidence_level = val.GetValue<double>();
		else if (key == "max_iterations" || key == "max_iter") o.max_iterations = ExtractUInteger(val);
		else if (key == "tolerance" || key == "tol") o.tolerance = val.GetValue<double>();
		else if (key == "quantile") {
			if (kind == AftKind::PREDICT) o.quantile = val.GetValue<double>();
		} else if (key == "horizon") {
			if (kind == AftKind::PREDICT) o.horizon = val.GetValue<double>();
		} else if (key == "prior" || key == "priors") has_prior = true;
		// vcov and every other key: ignored
	});
	if (has_prior) throw InvalidInputException("aft: priors are not built");
}

using HipAftBindData = RowsBindData<HipAftOptions, AftKind>;

// Update, (time, x, event[, options]): the event column is read where row_shapes.hpp reads a weights column.  KEEP_NULLS: the
// fit-predict aggregate, which drops a row only for a NULL x list.
template <bool KEEP_NULLS>
void AftUpdate(Vector inputs[], AggregateInputData &, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 3) ThrowTooFewArguments("aft aggregates");
	RowsInput in(inputs, count, state_vector, true, 0);
	for (idx_t i = 0; i < count; i++) {
		double time = NAN, event = NAN;
		const bool time_valid = in.Y(i, time), event_valid = in.W(i, event);
		const list_entry_t *entry = in.X(i);
		if (!entry || (!KEEP_NULLS && (!time_valid || !event_valid))) continue;
		auto &rows = RowsOf(in.State(i), entry->length, true); // aft_aggregate.cpp:175: the text with the two counts
		in.AppendX(*entry, rows.x);
		PushRow(rows, time_valid ? time : NAN, time_valid, time_valid && event_valid);
		if (!event_valid) rows.flags.back() |= kEventNull;
		rows.w.push_back(event_valid ? event : NAN);
	}
}

// the states of one Finalize vector as one batch per feature count; time and event go as they were buffered (NaN where NULL)
struct AftBatch : RowBatch {
	vector<double> records, inference, pred;
	int64_t n = 0;
	void StageRows() {
		for (auto *b : buffers) {
			n += (int64_t)b->Rows();
			offsets.push_back(n);
		}
		y.resize((size_t)n);
		w.resize((size_t)n);
		cols.resize((size_t)n * p);
		int64_t at = 0;
		for (auto *b : buffers) {
			const idx_t rows = b->Rows();
			for (idx_t r = 0; r < rows; r++) {
				y[at + r] = b->y[r];
				w[at + r] = b->w[r];
				for (idx_t j = 0; j < p; j++) cols[j * (size_t)n + at + r] = b->x[r * p + j];
			}
			at += (int64_t)rows;
		}
		col_ptrs.resize(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * (size_t)n;
		records.resize(Groups() * (p + 13));
	}
	void Run(const HipAftBindData &bind) {
		StageRows();
		if (bind.opts.compute_inference) inference.resize(Groups() * (5 * p + 2));
		double *inf = bind.opts.compute_inference ? inference.data() : nullptr;
		AnofoxError err;
		memset(&err, 0, sizeof err);
		bool ok;
		if (bind.kind == AftKind::PREDICT) {
			pred.resize((size_t)n * 4);
			AnofoxHipAftPredictOptions q;
			q.quantile = bind.opts.quantile;
			q.horizon = bind.opts.horizon;
			ok = anofox_hip_aft_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), w.data(),
			                                           bind.opts.Batch(), q, records.data(), inf, pred.data(), &err);
		} else {
			ok = anofox_hip_aft_fit_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), w.data(), bind.opts.Batch(),
			                                   records.data(), inf, &err);
		}
		if (!ok) ThrowAbi(err);
	}
	const double *Record(idx_t g) const { return &records[g * (p + 13)]; }
	bool Failed(idx_t g) const { return Record(g)[p + 12] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_aft_fit_agg(time, x, event[, options]) -> STRUCT
// =====================================================================================================================
LogicalType GetHipAftAggResultType(bool compute_inference) { // GetAftAggResultType, aft_aggregate.cpp:86-112
	child_list_t<LogicalType> children;
	children.push_back(make_pair("coefficients", LogicalType::LIST(LogicalType::DOUBLE)));
	for (auto *name : {"intercept", "scale", "log_likelihood", "null_log_likelihood", "aic", "bic"}) children.push_back(make_pair(string(name), LogicalType(LogicalType::DOUBLE)));
	for (auto *name : {"n_observations", "n_events", "n_censored", "n_features"}) children.push_back(make_pair(string(name), LogicalType(LogicalType::BIGINT)));
	children.push_back(make_pair("iterations", LogicalType::INTEGER));
	children.push_back(make_pair("converged", LogicalType::BOOLEAN));
	if (compute_inference) {
		for (auto *name : {"std_errors", "z_values", "p_values", "ci_lower", "ci_upper"})
			children.push_back(make_pair(string(name), LogicalType::LIST(LogicalType::DOUBLE)));
		children.push_back(make_pair("intercept_std_error", LogicalType::DOUBLE));
		children.push_back(make_pair("log_scale_std_error", LogicalType::DOUBLE));
	}
	return LogicalType::STRUCT(std::move(children));
}

// Finalize (:246-330): NULL for a state no row reached and for a group whose status is not 0; otherwise the record's fields
void HipAftAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipAftBindData>();
	auto batches = CollectBatches<AftBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 1; });
	for (auto &kv : batches) kv.second.Run(bind);
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		const idx_t p = b.p;
		for (idx_t g = 0; g < b.Groups(); g++) {
			const idx_t r = b.result_rows[g];
			if (b.Failed(g)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const double *rec = b.Record(g); // b[p], intercept, scale, ll, null ll, aic, bic, n_obs, n_events, n_censored, n_params, iterations, converged
			idx_t f = 0;
			AppendList(*fields[f++], r, rec, p);
			for (idx_t k = 0; k < 6; k++) SetDoubleOrNull(*fields[f++], r, rec[p + k], false);
			for (idx_t k = 0; k < 3; k++) FlatVector::GetData<int64_t>(*fields[f++])[r] = (int64_t)rec[p + 6 + k];
			FlatVector::GetData<int64_t>(*fields[f++])[r] = (int64_t)p;
			FlatVector::GetData<int32_t>(*fields[f++])[r] = (int32_t)rec[p + 10];
			FlatVector::GetData<bool>(*fields[f++])[r] = rec[p + 11] != 0.0;
			if (bind.opts.compute_inference) {
				const double *inf = &b.inference[g * (5 * p + 2)];
				for (idx_t k = 0; k < 5; k++) AppendList(*fields[f++], r, inf + k * p, p);
				FlatVector::GetData<double>(*fields[f++])[r] = inf[5 * p];
				FlatVector::GetData<double>(*fields[f++])[r] = inf[5 * p + 1];
			}
		}
	}
}

// =====================================================================================================================
// anofox_stats_aft_fit_predict_agg(time, x, event[, options])
//   -> LIST(STRUCT(time, event, eta, time_quantile, cdf, risk, is_training))
// =====================================================================================================================
LogicalType AftPredictResultType() {
	child_list_t<LogicalType> row;
	for (auto *name : {"time", "event", "eta", "time_quantile", "cdf", "risk"}) row.push_back(make_pair(string(name), LogicalType(LogicalType::DOUBLE)));
	row.push_back(make_pair("is_training", LogicalType::BOOLEAN));
	return LogicalType::LIST(LogicalType::STRUCT(std::move(row)));
}

// Finalize: every buffered row in arrival order; time / event NULL where the input was, a slot that is not finite NULL (all
// four for a failed group, as AppendPredictRows has it for the other families); NULL for a state no row reached
void HipAftPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipAftBindData>();
	auto batches = CollectBatches<AftBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 1; });
	for (auto &kv : batches) kv.second.Run(bind);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			const RowBuffer &rows = *b.buffers[g];
			const idx_t n_rows = rows.Rows(), list_offset = AppendListEntry(result, b.result_rows[g], n_rows);
			auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
			const double *pred = &b.pred[(size_t)b.offsets[g] * 4];
			for (idx_t r = 0; r < n_rows; r++) {
				const idx_t at = list_offset + r;
				SetDoubleOrNull(*fields[0], at, rows.y[r], (rows.flags[r] & kYNull) != 0);
				SetDoubleOrNull(*fields[1], at, rows.w[r], (rows.flags[r] & kEventNull) != 0);
				for (idx_t k = 0; k < 4; k++) SetDoubleOrNull(*fields[2 + k], at, pred[r * 4 + k], !isfinite(pred[r * 4 + k]));
				FlatVector::GetData<bool>(*fields[6])[at] = (rows.flags[r] & kTraining) != 0;
			}
		}
	}
}

template <AftKind KIND>
unique_ptr<FunctionData> HipAftBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipAftOptions>(
	    context, function, arguments, 3, false, [](const Value &v, HipAftOptions &o) { ParseHipAftOptions(v, KIND, o); },
	    [](const HipAftOptions &o) { return KIND == AftKind::PREDICT ? AftPredictResultType() : GetHipAftAggResultType(o.compute_inference); }, KIND);
}

template <AftKind KIND>
void RegisterHipAftAgg(ExtensionLoader &loader, const char *name, const char *alias, const char *what, const char *example_options) {
	RowsFunctionNames f {name, alias, {}, what, kCategories};
	f.base = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::DOUBLE};
	f.base_names = {"time", "x", "event"};
	RegisterWithOptions(loader, f, example_options, [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, AftUpdate<KIND == AftKind::PREDICT>, RowsCombine<false, true>,
		                    KIND == AftKind::PREDICT ? HipAftPredictAggFinalize : HipAftAggFinalize, HipAftBind<KIND>);
	});
}

} // namespace

void RegisterAftFamilyHip(ExtensionLoader &loader) {
	RegisterHipAftAgg<AftKind::FIT>(loader, "anofox_stats_aft_fit_agg", "aft_fit_agg",
	                                "Fits an accelerated failure time model with right censoring per group (event: 1 observed, 0 censored).",
	                                "{'dist': 'weibull', 'compute_inference': true}");
	RegisterHipAftAgg<AftKind::PREDICT>(loader, "anofox_stats_aft_fit_predict_agg", "aft_fit_predict_agg",
	                                    "Fits an accelerated failure time model per group and scores every row: the linear predictor, a quantile of "
	                                    "the time, P(T <= time) and the chance of failing within a horizon given survival so far.",
	                                    "{'dist': 'weibull', 'quantile': 0.5, 'horizon': 30.0}");
}

} // namespace duckdb
