// elasticnet_family_hip.cpp — DuckDB glue of the elastic net's fit-predict functions over the batched C ABI:
//
//   anofox_stats_elasticnet_fit_predict_agg   src/aggregate_functions/elasticnet_predict_aggregate.cpp (state :20-58, bind data
//                                             :60-92, result type :94-106, Update :150-245, Combine :255-296, Finalize :299-395,
//                                             Bind :400-475, registration :480-591)
//   anofox_stats_elasticnet_fit_predict       src/window_functions/elasticnet_fit_predict.cpp (state :20-50, Update :110-180,
//                                             Combine :190-230, Finalize :235-290, Bind :295-320, registration :330-378)
//
// As family_agg_hip.cpp does for ols / ridge / wls: the DuckDB state buffers the group's rows on the host (the aggregate
// returns every row in arrival order; the window aggregate's frame rows arrive one state at a time), and Finalize turns the
// whole vector of states into ONE anofox_hip_elasticnet_fit_predict_batch_host call per feature count: states = groups,
// columns concatenated, NaN y = "does not train".  The window aggregate appends its current x as a last row that does not
// train and reads that row's prediction.
//
// Options: the elastic net keys of hip_options.hpp plus confidence_level / confidence and null_policy.  Reference quirk kept:
// the aggregate's bind reads opts.alpha only (elasticnet_predict_aggregate.cpp:405-431), so there a `lambda` key is ignored;
// the window function's bind uses GetRegularizationStrength() (elasticnet_fit_predict.cpp:307), where alpha wins over lambda.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU
// with the real library (tests/test_gpu_elasticnet_family_glue.py through tests/tools/elasticnet_family_capi.cpp).
#include <math.h>
#include <stdlib.h>

#include <map>
#include <memory>

#include "duckdb.hpp"
#include "duckdb/common/types/data_chunk.hpp"
#include "duckdb/execution/expression_executor.hpp"
#include "duckdb/function/aggregate_function.hpp"
#include "duckdb/main/extension/extension_loader.hpp"
#include "duckdb/parser/parsed_data/create_aggregate_function_info.hpp"

#include "anofox_stats_hip.h"
#include "elasticnet_family_hip.hpp"
#include "hip_options.hpp"
#include "row_glue.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "prediction"};

// ---- options: the elastic net's plus the interval's confidence level and the null policy ----
struct HipEnPredictOptions {
	HipElasticNetOptions en;
	double confidence_level = 0.95;
	bool drop_y_zero_x = false;
	bool operator==(const HipEnPredictOptions &o) const {
		return en == o.en && confidence_level == o.confidence_level && drop_y_zero_x == o.drop_y_zero_x;
	}
};

// use_lambda = false: the aggregate's bind (alpha only); true: the window function's (alpha, else lambda)
void ParseHipEnPredictOptions(const Value &v, HipEnPredictOptions &o, bool use_lambda) {
	if (v.IsNull()) return;
	AlphaOrLambda strength;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (val.IsNull()) return;
		if (key == "confidence_level" || key == "confidence") o.confidence_level = val.GetValue<double>();
		else if (key == "null_policy") o.drop_y_zero_x = ExtractNullPolicy(val);
		else ApplyElasticNetOption(key, val, o.en, strength);
	});
	strength.Store(o.en.alpha, use_lambda);
}

struct HipEnFamilyBindData : public FunctionData {
	HipEnFamilyBindData(const HipEnPredictOptions &opts_p, bool use_split_col_p) : opts(opts_p), use_split_col(use_split_col_p) {}
	HipEnPredictOptions opts;
	bool use_split_col;
	unique_ptr<FunctionData> Copy() const override { return make_uniq<HipEnFamilyBindData>(opts, use_split_col); }
	bool Equals(const FunctionData &other_p) const override {
		auto &other = other_p.Cast<HipEnFamilyBindData>();
		return opts == other.opts && use_split_col == other.use_split_col;
	}
};

// the states of one Finalize vector as one batch per feature count (RowBatch) through the fit-predict call
struct EnBatch : RowBatch {
	vector<double> core, pred;
	void Run(const HipEnPredictOptions &opts, bool extra_row) {
		const int64_t n = Stage(false, extra_row);
		core.resize(Groups() * (p + 6));
		pred.resize((size_t)n * 3);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_elasticnet_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                                  opts.en.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			ThrowAbi(err);
	}
	bool Failed(idx_t g) const { return core[g * (p + 6) + p + 5] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_elasticnet_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Update (:150-245): every row with a non-NULL x list is kept for the output; it trains iff y is not NULL (and the split column
// says train), and under null_policy = 'drop_y_zero_x' no feature is exactly 0.  A NULL list element is NaN: the row is handed
// to the fit, whose row filter drops it.
void HipEnPredictAggUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<HipEnFamilyBindData>();
	if (input_count < 2) throw InvalidInputException("anofox_stats elasticnet_fit_predict_agg (HIP): too few arguments");
	UnifiedVectorFormat y_data, x_data, split_data, sdata;
	inputs[0].ToUnifiedFormat(count, y_data);
	inputs[1].ToUnifiedFormat(count, x_data);
	auto y_values = UnifiedVectorFormat::GetData<double>(y_data);
	auto x_list = UnifiedVectorFormat::GetData<list_entry_t>(x_data);
	auto &x_child = ListVector::GetEntry(inputs[1]);
	auto x_child_data = FlatVector::GetData<double>(x_child);
	auto &x_child_validity = FlatVector::Validity(x_child);
	const string_t *split_values = nullptr;
	if (bind.use_split_col && input_count > 2) {
		inputs[2].ToUnifiedFormat(count, split_data);
		split_values = UnifiedVectorFormat::GetData<string_t>(split_data);
	}
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (RowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		CheckMaxFeatures("elasticnet_fit_predict_agg", entry.length, max_features);
		auto &rows = RowsOf(state, entry.length, false);
		const size_t at = rows.x.size();
		rows.x.resize(at + entry.length);
		const bool has_zero = ReadListRow(entry, x_child_data, x_child_validity, rows.x.data() + at).has_zero;
		auto y_idx = y_data.sel->get_index(i);
		const bool y_valid = y_data.validity.RowIsValid(y_idx);
		bool training = y_valid;
		if (bind.use_split_col && split_values) {
			auto s_idx = split_data.sel->get_index(i);
			training = split_data.validity.RowIsValid(s_idx) && IsSplitTraining(split_values[s_idx]) && y_valid;
		}
		if (training && bind.opts.drop_y_zero_x && has_zero) training = false;
		rows.y.push_back(y_valid ? y_values[y_idx] : NAN);
		rows.flags.push_back((uint8_t)((y_valid ? 0 : kYNull) | (training ? kTraining : 0)));
		rows.n_training += training ? 1 : 0;
	}
}

// Finalize (:299-395): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with its prediction
void HipEnPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipEnFamilyBindData>();
	auto batches = CollectBatches<EnBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; });
	for (auto &kv : batches) kv.second.Run(bind.opts, false);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			if (b.Failed(g)) FlatVector::SetNull(result, b.result_rows[g], true);
			else AppendPredictRows(result, b.result_rows[g], *b.buffers[g], &b.pred[(size_t)b.offsets[g] * 3]);
		}
	}
}

template <bool SPLIT>
unique_ptr<FunctionData> HipEnPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipEnPredictOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable())
		ParseHipEnPredictOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts, false);
	function.return_type = PredictAggResultType();
	return make_uniq<HipEnFamilyBindData>(opts, SPLIT);
}

// =====================================================================================================================
// anofox_stats_elasticnet_fit_predict(y, x[, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// =====================================================================================================================
// Update (elasticnet_fit_predict.cpp:110-180): the last row with a non-NULL x list is the row to predict; every row with a
// non-NULL y trains (not under drop_y_zero_x when a feature is 0).  Only training rows are buffered.
void HipEnFitPredictUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<HipEnFamilyBindData>();
	if (input_count < 2) throw InvalidInputException("anofox_stats elasticnet_fit_predict (HIP): too few arguments");
	UnifiedVectorFormat y_data, x_data, sdata;
	inputs[0].ToUnifiedFormat(count, y_data);
	inputs[1].ToUnifiedFormat(count, x_data);
	auto y_values = UnifiedVectorFormat::GetData<double>(y_data);
	auto x_list = UnifiedVectorFormat::GetData<list_entry_t>(x_data);
	auto &x_child = ListVector::GetEntry(inputs[1]);
	auto x_child_data = FlatVector::GetData<double>(x_child);
	auto &x_child_validity = FlatVector::Validity(x_child);
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (RowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) {
			if (state.rows) state.rows->has_current_x = false; // :134-137
			continue;
		}
		const auto entry = x_list[x_idx];
		CheckMaxFeatures("elasticnet_fit_predict", entry.length, max_features);
		auto &rows = RowsOf(state, entry.length, false);
		rows.current_x.resize(entry.length);
		const bool has_zero = ReadListRow(entry, x_child_data, x_child_validity, rows.current_x.data()).has_zero;
		rows.has_current_x = true;
		auto y_idx = y_data.sel->get_index(i);
		bool training = y_data.validity.RowIsValid(y_idx);
		if (training && bind.opts.drop_y_zero_x && has_zero) training = false; // :162-169
		if (!training) continue;
		rows.y.push_back(y_values[y_idx]);
		rows.x.insert(rows.x.end(), rows.current_x.begin(), rows.current_x.end());
		rows.flags.push_back(kTraining);
		rows.n_training++;
	}
}

// Finalize (:235-290): NULL without a current row or with at most p + [intercept] training rows, or when the fit fails
void HipEnFitPredictFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipEnFamilyBindData>();
	const idx_t intercept = bind.opts.en.fit_intercept ? 1 : 0;
	auto batches = CollectBatches<EnBatch>(state_vector, result, count, offset, [&](const RowBuffer &rows) {
		return rows.has_current_x && rows.n_training > rows.n_features + intercept;
	});
	for (auto &kv : batches) kv.second.Run(bind.opts, true);
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.buffers.size(); g++) {
			const idx_t r = b.result_rows[g];
			const double *pred = &b.pred[((size_t)b.offsets[g + 1] - 1) * 3];
			if (b.Failed(g) || !isfinite(pred[0])) { // :270-286: a failed fit or prediction is NULL
				FlatVector::SetNull(result, r, true);
				continue;
			}
			for (idx_t k = 0; k < 3; k++) FlatVector::GetData<double>(*fields[k])[r] = pred[k];
		}
	}
}

unique_ptr<FunctionData> HipEnFitPredictBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipEnPredictOptions opts;
	if (arguments.size() > 2 && arguments[2]->IsFoldable()) ParseHipEnPredictOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), opts, true);
	function.return_type = FitPredictResultType();
	return make_uniq<HipEnFamilyBindData>(opts, false);
}

} // namespace

void RegisterHipElasticNetFitPredictAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_elasticnet_fit_predict_agg";
	const char *what = "Fits Elastic Net regression over a partition and returns per-row predictions with confidence intervals.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	const vector<LogicalType> split_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR};
	const vector<LogicalType> split_map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR, LogicalType::ANY};
	auto make = [](const string &fname, const vector<LogicalType> &args, bool split) {
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>, RowsInitialize,
		                         HipEnPredictAggUpdate, RowsCombine<false>, HipEnPredictAggFinalize, nullptr,
		                         split ? HipEnPredictAggBind<true> : HipEnPredictAggBind<false>, RowsDestroy);
	};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		set.AddFunction(make(fname, basic, false));          // (y, x)
		set.AddFunction(make(fname, map_args, false));       // (y, x, options)
		set.AddFunction(make(fname, split_args, true));      // (y, x, split_col)
		set.AddFunction(make(fname, split_map_args, true));  // (y, x, split_col, options)
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	const string head = string(name) + "(y, x";
	info.descriptions.push_back(Describe(what, head + ")", {"y", "x"}, basic, kCategories));
	info.descriptions.push_back(Describe(what, head + ", {'alpha': 1.0, 'l1_ratio': 0.5})", {"y", "x", "options"}, map_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col)", {"y", "x", "split_col"}, split_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'alpha': 1.0})", {"y", "x", "split_col", "options"}, split_map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("elasticnet_fit_predict_agg"));
	for (const char *alias : {"elasticnet_predict_agg", "anofox_stats_elasticnet_predict_agg"}) RegisterAlias(loader, name, fill(alias)); // the deprecated names
}

void RegisterHipElasticNetFitPredictFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_elasticnet_fit_predict";
	const char *what = "Fits an ElasticNet regression model over a window partition and returns predictions with confidence intervals.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, FitPredictResultType(), AggregateFunction::StateSize<RowsState>, RowsInitialize,
			                                  HipEnFitPredictUpdate, RowsCombine<true>, HipEnFitPredictFinalize, nullptr, HipEnFitPredictBind,
			                                  RowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic, kCategories));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'null_policy': 'drop'})", {"y", "x", "options"}, map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("elasticnet_fit_predict"));
}

} // namespace duckdb
