// quantile_family_hip.cpp — DuckDB glue of quantile regression over the batched C ABI:
//
//   anofox_stats_quantile_fit_predict_agg        src/aggregate_functions/quantile_fit_predict_aggregate.cpp (state :19-49, bind
//                                                data :54-72, result type :77-85, Update :115-211, Combine :213-257, Finalize
//                                                :259-354, binds :359-398, registration :403-484)
//   anofox_stats_quantile_path_fit_predict_agg   no counterpart in the reference: the SQL face of aggregate.py's
//                                                quantile_path_fit_predict_agg (the tau path, one fit per group for a grid of tau)
//   anofox_stats_quantile_fit_predict            no counterpart in the reference: the SQL face of aggregate.py's
//                                                quantile_fit_predict (window aggregate; mechanics of rls_family_hip.cpp's,
//                                                src/window_functions/rls_fit_predict.cpp)
//
// As the other glue files: the DuckDB state buffers the group's rows on the host in arrival order, Combine appends the
// source's rows after the target's, and Finalize turns the whole vector of states into ONE batched call per feature count
// (anofox_hip_quantile_fit_predict_batch_host / anofox_hip_quantile_fit_predict_path_batch_host) where the reference makes one
// anofox_quantile_fit call per group (:298): states = groups, columns concatenated, NaN y = "does not train".  LIST children
// are reserved before they are written.  The glue adds no arithmetic: every yhat is the library's.
//
// Options (the keys options.parse_quantile_options reads; the reference's bind reads tau and fit_intercept, :363-371):
// tau, fit_intercept / intercept, max_iterations / max_iter, tolerance / tol; the path reads taus (a LIST of numbers) in
// place of tau.  Every other key is ignored — `quantile` included, which the reference's own example passes (:449) and
// its aggregate never reads.  tau is not range-checked at bind: the fit reports it (status 1) and every group is NULL.
//
// The window aggregate fits every frame cold.  DuckDB hands an aggregate without a window callback a materialised frame per
// output row — Update calls for the frame's rows (the naive aggregator) or a Combine of segment-tree states — and never the
// consecutive frame bounds of a partition, which is what the sliding simplex needs to pivot from one frame's vertex to the
// next's.  anofox_hip_quantile_fit_predict_window_* / _frames_* therefore stay reachable from the C ABI and Python only; an
// aggregate_window_t callback over the partition is the follow-up that would reach them.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU
// with the real library (tests/test_gpu_quantile_glue.py through tests/tools/quantile_family_capi.cpp).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <memory>

#include "duckdb.hpp"
#include "duckdb/common/types/data_chunk.hpp"
#include "duckdb/execution/expression_executor.hpp"
#include "duckdb/function/aggregate_function.hpp"
#include "duckdb/main/extension/extension_loader.hpp"
#include "duckdb/parser/parsed_data/create_aggregate_function_info.hpp"

#include "anofox_stats_hip.h"
#include "quantile_family_hip.hpp"
#include "hip_options.hpp"
#include "row_shapes.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "quantile"};

// ---- options ----
constexpr idx_t kMaxTaus = 64; // the library's grid limit (anofox_hip_quantile_fit_predict_path_batch_host)
const char *const kTausMissing = "the quantile path needs the option 'taus': a non-empty list of quantiles";
const char *const kTauGiven = "the quantile path takes a list of quantiles in 'taus', not 'tau'";
const char *const kNotConstant = "Options parameter must be a constant expression";

struct HipQuantileOptions {
	double tau = 0.5;                // quantile_fit_predict_aggregate.cpp:55
	bool fit_intercept = true;       // :56
	uint32_t max_iterations = 1000;  // :292
	double tolerance = 1e-6;         // :293
	vector<double> taus;             // the path only, in the caller's order; NaN = a NULL element
	bool operator==(const HipQuantileOptions &o) const {
		return memcmp(&tau, &o.tau, sizeof tau) == 0 && fit_intercept == o.fit_intercept && max_iterations == o.max_iterations &&
		       tolerance == o.tolerance && taus.size() == o.taus.size() &&
		       (taus.empty() || memcmp(taus.data(), o.taus.data(), taus.size() * sizeof(double)) == 0);
	}
	AnofoxHipQuantileBatchOptions Batch() const {
		AnofoxHipQuantileBatchOptions b;
		memset(&b, 0, sizeof b);
		b.tau = tau;
		b.fit_intercept = fit_intercept;
		b.max_iterations = max_iterations;
		b.tolerance = tolerance;
		return b;
	}
};

void ApplyQuantileOption(const string &key, const Value &v, HipQuantileOptions &o) { // key lower-cased
	if (v.IsNull()) return;
	if (key == "tau") o.tau = v.GetValue<double>();
	else if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(v);
	else if (key == "max_iterations" || key == "max_iter") o.max_iterations = ExtractUInteger(v);
	else if (key == "tolerance" || key == "tol") o.tolerance = v.GetValue<double>();
	// every other key: ignored, as in the reference ({'quantile': 0.5} of its example binds and changes nothing)
}

void ParseHipQuantileOptions(const Value &v, HipQuantileOptions &o) {
	if (v.IsNull()) return;
	VisitOptionEntries(v, [&](const string &key, const Value &val) { ApplyQuantileOption(key, val, o); });
}

// options.parse_quantile_path_options: `tau` is rejected whatever its value, `taus` must be a non-empty LIST; a NULL element
// is kept as NaN and an out-of-range one as it is (the fit reports both at their position: status 1, NULL predictions)
void ParseHipQuantilePathOptions(const Value &v, HipQuantileOptions &o) {
	if (v.IsNull()) throw InvalidInputException("%s", kTausMissing);
	VisitOptionEntries(v, [&](const string &key, const Value &) {
		if (key == "tau") throw InvalidInputException("%s", kTauGiven);
	});
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (key != "taus") {
			ApplyQuantileOption(key, val, o);
			return;
		}
		o.taus.clear();
		if (val.IsNull() || val.type().id() != LogicalTypeId::LIST) return;
		for (auto &e : ListValue::GetChildren(val)) o.taus.push_back(e.IsNull() ? NAN : e.GetValue<double>());
	});
	if (o.taus.empty()) throw InvalidInputException("%s", kTausMissing);
	if (o.taus.size() > kMaxTaus) throw InvalidInputException("quantile path: n_taus > 64 is not built");
}

using HipQuantileBindData = RowsBindData<HipQuantileOptions>;

// Update (quantile_fit_predict_aggregate.cpp:115-211): the width is not checked (the library's call reports it), RowsOf's text
// has the counts (:162-164), null_policy is never read, and a NaN y that is not NULL counts as a training row (:204-209; the
// fit's row filter drops it).  The window buffers every row with its flags, the last one also as the row to predict; it binds
// no split column.  Both shapes go by one name in "too few arguments".
struct QuantileTraits : RowTraits {
	using Bind = HipQuantileBindData;
	static constexpr const char *kName = "quantile_fit_predict";
	static constexpr bool kCheckMaxFeatures = false;
	static constexpr bool kCountsInError = true;
	static constexpr bool kBuffersEveryRow = true;
	static bool DropYZeroX(const Bind &) { return false; }
};

// the states of one Finalize vector as one batch per feature count (RowBatch) through the family's two ABI calls; rows that
// do not train reach the ABI with y = NaN
struct QuantileBatch : RowBatch {
	vector<double> records, pred;
	// records [G x (p + 6)] in the regression layout, pred [n x 3] = {yhat, NaN, NaN}: the two NaN bounds are dropped by the callers
	void Run(const HipQuantileOptions &opts, bool extra_row) {
		const int64_t n = Stage(false, extra_row);
		records.resize(Groups() * (p + 6));
		pred.resize((size_t)n * 3);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_quantile_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                                opts.Batch(), records.data(), pred.data(), &err))
			ThrowAbi(err);
	}
	// records [G x T x (p + 6)] in the quantile layout, pred [n x T]
	void RunPath(const HipQuantileOptions &opts) {
		const int64_t n = Stage(false, false);
		const size_t T = opts.taus.size();
		records.resize(Groups() * T * (p + 6));
		pred.resize((size_t)n * T);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_quantile_fit_predict_path_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                                     opts.Batch(), opts.taus.data(), T, records.data(), nullptr, pred.data(), &err))
			ThrowAbi(err);
	}
	bool Failed(idx_t g, idx_t T = 1, idx_t t = 0) const { return records[(g * T + t) * (p + 6) + p + 5] != 0.0; }
};

// the states of a Finalize vector that are fitted, by feature count; the others are NULL (:269: never initialised or fewer
// than 2 training rows; WINDOW: no current row either)
template <bool WINDOW>
std::map<idx_t, QuantileBatch> CollectQuantileBatches(Vector &state_vector, Vector &result, idx_t count, idx_t offset) {
	return CollectBatches<QuantileBatch>(state_vector, result, count, offset,
	                                     [](const RowBuffer &rows) { return rows.n_training >= 2 && (!WINDOW || rows.has_current_x); });
}

// =====================================================================================================================
// anofox_stats_quantile_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, is_training))
// =====================================================================================================================
LogicalType GetHipQuantilePredictAggResultType() { // :77-85
	child_list_t<LogicalType> row_children;
	row_children.push_back(make_pair("y", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	row_children.push_back(make_pair("is_training", LogicalType::BOOLEAN));
	return LogicalType::LIST(LogicalType::STRUCT(std::move(row_children)));
}

// Finalize (:259-354): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with its prediction
// (a non-finite yhat is NULL :341-346, y is NULL where the input was :326-330)
void HipQuantilePredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipQuantileBindData>();
	auto batches = CollectQuantileBatches<false>(state_vector, result, count, offset);
	for (auto &kv : batches) kv.second.Run(bind.opts, false);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.buffers.size(); g++) {
			const idx_t r = b.result_rows[g];
			if (b.Failed(g)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const RowBuffer &rows = *b.buffers[g];
			const idx_t n_rows = rows.Rows();
			const idx_t list_offset = AppendListEntry(result, r, n_rows);
			auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
			const double *pred = &b.pred[(size_t)b.offsets[g] * 3];
			for (idx_t row = 0; row < n_rows; row++) {
				const idx_t at = list_offset + row;
				SetDoubleOrNull(*fields[0], at, rows.y[row], (rows.flags[row] & kYNull) != 0);
				SetDoubleOrNull(*fields[1], at, pred[row * 3], !isfinite(pred[row * 3]));
				FlatVector::GetData<bool>(*fields[2])[at] = (rows.flags[row] & kTraining) != 0;
			}
		}
	}
}

template <bool SPLIT, LogicalType (*TYPE)()>
unique_ptr<FunctionData> HipQuantileBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipQuantileOptions>(context, function, arguments, SPLIT ? 3 : 2, SPLIT, ParseHipQuantileOptions, [](const HipQuantileOptions &) { return TYPE(); });
}

// =====================================================================================================================
// anofox_stats_quantile_path_fit_predict_agg(y, x[, split_col], options) -> LIST(STRUCT(y, tau, yhat, is_training))
// long format: for each buffered row in arrival order one entry per tau in the caller's order (row-major)
// =====================================================================================================================
LogicalType GetHipQuantilePathAggResultType() {
	child_list_t<LogicalType> row_children;
	row_children.push_back(make_pair("y", LogicalType::DOUBLE));
	row_children.push_back(make_pair("tau", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	row_children.push_back(make_pair("is_training", LogicalType::BOOLEAN));
	return LogicalType::LIST(LogicalType::STRUCT(std::move(row_children)));
}

// Finalize: the group is NULL by the row rules or when every tau failed; a single failed or invalid tau NULLs its own yhat
// entries only (the library writes NaN there)
void HipQuantilePathAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipQuantileBindData>();
	const auto &taus = bind.opts.taus;
	const idx_t T = taus.size();
	auto batches = CollectQuantileBatches<false>(state_vector, result, count, offset);
	for (auto &kv : batches) kv.second.RunPath(bind.opts);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.buffers.size(); g++) {
			const idx_t r = b.result_rows[g];
			bool any_fitted = false;
			for (idx_t t = 0; t < T; t++) any_fitted = any_fitted || !b.Failed(g, T, t);
			if (!any_fitted) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const RowBuffer &rows = *b.buffers[g];
			const idx_t n_rows = rows.Rows();
			const idx_t list_offset = AppendListEntry(result, r, n_rows * T);
			auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
			const double *pred = &b.pred[(size_t)b.offsets[g] * T];
			for (idx_t row = 0; row < n_rows; row++) {
				for (idx_t t = 0; t < T; t++) {
					const idx_t at = list_offset + row * T + t;
					const double yhat = pred[row * T + t];
					SetDoubleOrNull(*fields[0], at, rows.y[row], (rows.flags[row] & kYNull) != 0);
					SetDoubleOrNull(*fields[1], at, taus[t], isnan(taus[t]));
					SetDoubleOrNull(*fields[2], at, yhat, b.Failed(g, T, t) || !isfinite(yhat));
					FlatVector::GetData<bool>(*fields[3])[at] = (rows.flags[row] & kTraining) != 0;
				}
			}
		}
	}
}

template <bool SPLIT>
unique_ptr<FunctionData> HipQuantilePathAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipQuantileOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() <= opt_idx) throw InvalidInputException("%s", kTausMissing);
	if (!arguments[opt_idx]->IsFoldable()) throw InvalidInputException("%s", kNotConstant);
	ParseHipQuantilePathOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts);
	function.return_type = GetHipQuantilePathAggResultType();
	return make_uniq<HipQuantileBindData>(opts, SPLIT);
}

// =====================================================================================================================
// anofox_stats_quantile_fit_predict(y, x[, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// the result type of the *_fit_predict family, so the name can be swapped into an ols_fit_predict query; there is no interval:
// both bounds are always NULL
// =====================================================================================================================
// Finalize: the frame's rows plus the current x as a last row that does not train, whose yhat is the result.  NULL: a state
// never initialised, no current row, fewer than 2 training rows in the frame, a failed fit, a non-finite yhat.
void HipQuantileFitPredictFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipQuantileBindData>();
	auto batches = CollectQuantileBatches<true>(state_vector, result, count, offset);
	for (auto &kv : batches) kv.second.Run(bind.opts, true);
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.buffers.size(); g++) {
			const idx_t r = b.result_rows[g];
			const double yhat = b.pred[((size_t)b.offsets[g + 1] - 1) * 3];
			if (b.Failed(g) || !isfinite(yhat)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			FlatVector::GetData<double>(*fields[0])[r] = yhat;
			FlatVector::SetNull(*fields[1], r, true);
			FlatVector::SetNull(*fields[2], r, true);
		}
	}
}

} // namespace

void RegisterHipQuantileFitPredictAggregateFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_quantile_fit_predict_agg", "quantile_fit_predict_agg", {},
	                           "Fits a quantile regression model over a partition and returns per-row predictions.", kCategories};
	RegisterWithSplitAndOptions(loader, f, "{'tau': 0.5}", "{'tau': 0.5}", [](const string &fname, const vector<LogicalType> &args, bool split) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsPredictAggUpdate<QuantileTraits>, RowsCombine<false>, HipQuantilePredictAggFinalize,
		                    split ? HipQuantileBind<true, GetHipQuantilePredictAggResultType> : HipQuantileBind<false, GetHipQuantilePredictAggResultType>);
	});
}

void RegisterHipQuantilePathFitPredictAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_quantile_path_fit_predict_agg";
	const char *what = "Fits quantile regression at every quantile of a grid from one fit per partition and returns per-row, per-quantile predictions.";
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	const vector<LogicalType> split_map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR, LogicalType::ANY};
	auto make = [](const string &fname, const vector<LogicalType> &args, bool split) {
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>,
		                         RowsInitialize, RowsPredictAggUpdate<QuantileTraits>, RowsCombine<false>, HipQuantilePathAggFinalize,
		                         nullptr, split ? HipQuantilePathAggBind<true> : HipQuantilePathAggBind<false>, RowsDestroy);
	};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		set.AddFunction(make(fname, map_args, false));       // (y, x, options)
		set.AddFunction(make(fname, split_map_args, true));  // (y, x, split_col, options)
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	const string head = string(name) + "(y, x";
	info.descriptions.push_back(Describe(what, head + ", {'taus': [0.1, 0.5, 0.9]})", {"y", "x", "options"}, map_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'taus': [0.1, 0.5, 0.9]})", {"y", "x", "split_col", "options"}, split_map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("quantile_path_fit_predict_agg"));
}

void RegisterHipQuantileFitPredictFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_quantile_fit_predict", "quantile_fit_predict", {},
	                           "Fits a quantile regression model over a window frame and returns the prediction of the current row.", kCategories};
	RegisterWithOptions(loader, f, "{'tau': 0.9}", [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, FitPredictResultType(), RowsWindowUpdate<QuantileTraits>, RowsCombine<true>, HipQuantileFitPredictFinalize,
		                    HipQuantileBind<false, FitPredictResultType>);
	});
}

} // namespace duckdb
