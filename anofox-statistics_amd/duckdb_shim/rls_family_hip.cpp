// rls_family_hip.cpp — DuckDB glue of recursive least squares over the batched C ABI:
//
//   anofox_stats_rls_fit_agg              src/aggregate_functions/rls_aggregate.cpp
//   anofox_stats_rls_fit_predict_agg      src/aggregate_functions/rls_predict_aggregate.cpp
//   anofox_stats_rls_fit_predict          src/window_functions/rls_fit_predict.cpp (state :20-60, Update :100-163,
//                                         Combine :165-210, Finalize :212-271, Bind :273-294, registration :296-)
//
// RLS depends on row order, so it cannot use the moment arena: the DuckDB state buffers the group's rows in arrival order,
// Combine appends the source's rows after the target's (as the reference does), and Finalize turns the whole vector of
// states into ONE anofox_hip_rls_fit_batch_host / anofox_hip_rls_fit_predict_batch_host call per feature count.  The window
// aggregate appends its current x as a last row that does not train and reads that row's prediction.
//
// Options (map_options_parser.cpp:637-681): forgetting_factor, initial_p_diagonal / p_diagonal, fit_intercept / intercept,
// confidence_level / confidence and null_policy are read.  Every other key is ignored — `lambda` included (the reference's
// test_scalar_functions.test passes {'lambda': 0.99}, which its parser stores as a regularisation strength) — but a value the
// shared parser cannot convert is still a bind error, whichever key it sits under.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU
// with the real library (tests/test_gpu_rls_glue.py through tests/tools/rls_family_capi.cpp).
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
#include "rls_family_hip.hpp"
#include "hip_options.hpp"
#include "row_glue.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "prediction"};

// ---- options ----
struct HipRlsOptions {
	double forgetting_factor = 1.0;
	double initial_p_diagonal = 100.0;
	bool fit_intercept = true;
	double confidence_level = 0.95;
	bool drop_y_zero_x = false;
	bool operator==(const HipRlsOptions &o) const {
		return forgetting_factor == o.forgetting_factor && initial_p_diagonal == o.initial_p_diagonal && fit_intercept == o.fit_intercept &&
		       confidence_level == o.confidence_level && drop_y_zero_x == o.drop_y_zero_x;
	}
	AnofoxHipRlsBatchOptions Batch() const {
		AnofoxHipRlsBatchOptions b;
		memset(&b, 0, sizeof b);
		b.fit_intercept = fit_intercept;
		b.forgetting_factor = forgetting_factor;
		b.initial_p_diagonal = initial_p_diagonal;
		return b;
	}
};

void ParseHipRlsOptions(const Value &v, HipRlsOptions &o) {
	if (v.IsNull()) return;
	HipElasticNetOptions ignored;
	AlphaOrLambda ignored_strength;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (val.IsNull()) return;
		if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(val);
		else if (key == "forgetting_factor") o.forgetting_factor = val.GetValue<double>();
		else if (key == "initial_p_diagonal" || key == "p_diagonal") o.initial_p_diagonal = val.GetValue<double>();
		else if (key == "confidence_level" || key == "confidence") o.confidence_level = val.GetValue<double>();
		else if (key == "compute_inference" || key == "inference") (void)ExtractBool(val);
		else if (key == "null_policy") o.drop_y_zero_x = ExtractNullPolicy(val);
		else ApplyElasticNetOption(key, val, ignored, ignored_strength); // parsed by the shared parser, not read by RLS: only its conversion errors matter
	});
}

struct HipRlsFamilyBindData : public FunctionData {
	HipRlsFamilyBindData(const HipRlsOptions &opts_p, bool use_split_col_p) : opts(opts_p), use_split_col(use_split_col_p) {}
	HipRlsOptions opts;
	bool use_split_col;
	unique_ptr<FunctionData> Copy() const override { return make_uniq<HipRlsFamilyBindData>(opts, use_split_col); }
	bool Equals(const FunctionData &other_p) const override {
		auto &other = other_p.Cast<HipRlsFamilyBindData>();
		return opts == other.opts && use_split_col == other.use_split_col;
	}
};

// the states of one Finalize vector as one batch per feature count (RowBatch) through the fit-predict call
struct RlsBatch : RowBatch {
	vector<double> core, pred;
	void Run(const HipRlsOptions &opts, bool extra_row) {
		const int64_t n = Stage(false, extra_row);
		core.resize(Groups() * (p + 6));
		pred.resize((size_t)n * 3);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_rls_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                           opts.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			ThrowAbi(err);
	}
	bool Failed(idx_t g) const { return core[g * (p + 6) + p + 5] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_rls_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Update (:150-245): every row with a non-NULL x list is kept for the output; it trains iff y is not NULL (and the split column
// says train), and under null_policy = 'drop_y_zero_x' no feature is exactly 0.  A NULL list element is NaN: the row is handed
// to the fit, whose row filter drops it.
void HipRlsPredictAggUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	if (input_count < 2) throw InvalidInputException("anofox_stats rls_fit_predict_agg (HIP): too few arguments");
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
		CheckMaxFeatures("rls_fit_predict_agg", entry.length, max_features);
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
void HipRlsPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	auto batches = CollectBatches<RlsBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; });
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
unique_ptr<FunctionData> HipRlsPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipRlsOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable())
		ParseHipRlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts);
	function.return_type = PredictAggResultType();
	return make_uniq<HipRlsFamilyBindData>(opts, SPLIT);
}

// =====================================================================================================================
// anofox_stats_rls_fit_predict(y, x[, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// =====================================================================================================================
// Update (rls_fit_predict.cpp:110-180): the last row with a non-NULL x list is the row to predict; every row with a
// non-NULL y trains (not under drop_y_zero_x when a feature is 0).  Only training rows are buffered.
void HipRlsFitPredictUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	if (input_count < 2) throw InvalidInputException("anofox_stats rls_fit_predict (HIP): too few arguments");
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
		CheckMaxFeatures("rls_fit_predict", entry.length, max_features);
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
void HipRlsFitPredictFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	const idx_t intercept = bind.opts.fit_intercept ? 1 : 0;
	auto batches = CollectBatches<RlsBatch>(state_vector, result, count, offset, [&](const RowBuffer &rows) {
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

unique_ptr<FunctionData> HipRlsFitPredictBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipRlsOptions opts;
	if (arguments.size() > 2 && arguments[2]->IsFoldable()) ParseHipRlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), opts);
	function.return_type = FitPredictResultType();
	return make_uniq<HipRlsFamilyBindData>(opts, false);
}

// =====================================================================================================================
// anofox_stats_rls_fit_agg(y, x[, options]) -> STRUCT(coefficients, intercept, r_squared, adj_r_squared, residual_std_error,
// n_observations, n_features)
// =====================================================================================================================
LogicalType GetHipRlsFitAggResultType() { // rls_aggregate.cpp, the regression fit STRUCT
	child_list_t<LogicalType> children;
	children.push_back(make_pair("coefficients", LogicalType::LIST(LogicalType::DOUBLE)));
	children.push_back(make_pair("intercept", LogicalType::DOUBLE));
	children.push_back(make_pair("r_squared", LogicalType::DOUBLE));
	children.push_back(make_pair("adj_r_squared", LogicalType::DOUBLE));
	children.push_back(make_pair("residual_std_error", LogicalType::DOUBLE));
	children.push_back(make_pair("n_observations", LogicalType::BIGINT));
	children.push_back(make_pair("n_features", LogicalType::BIGINT));
	return LogicalType::STRUCT(std::move(children));
}

// Update: every row with a non-NULL x list and a non-NULL y is buffered in arrival order (a NULL list element is NaN: the
// fit's row filter drops that row)
void HipRlsFitAggUpdate(Vector inputs[], AggregateInputData &, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 2) throw InvalidInputException("anofox_stats rls_fit_agg (HIP): too few arguments");
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
		auto x_idx = x_data.sel->get_index(i), y_idx = y_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx) || !y_data.validity.RowIsValid(y_idx)) continue;
		const auto entry = x_list[x_idx];
		CheckMaxFeatures("rls_fit_agg", entry.length, max_features);
		auto &rows = RowsOf(state, entry.length, false);
		const size_t at = rows.x.size();
		rows.x.resize(at + entry.length);
		ReadListRow(entry, x_child_data, x_child_validity, rows.x.data() + at);
		rows.y.push_back(y_values[y_idx]);
		rows.flags.push_back(kTraining);
		rows.n_training++;
	}
}

// Finalize: NULL with fewer than 2 rows or a failed fit; the vector's other states in ONE batched call per feature count
void HipRlsFitAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	auto batches = CollectBatches<RowBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 2; });
	auto &entries = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		const idx_t p = kv.first;
		auto &b = kv.second;
		const int64_t n = b.Stage(false, false); // (every buffered row trains)
		const size_t rec = anofox_hip_core_record_len(p);
		vector<double> core(b.Groups() * rec);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_rls_fit_batch_host(nullptr, (int64_t)b.Groups(), p, n, b.offsets.data(), b.y.data(), b.col_ptrs.data(), bind.opts.Batch(), core.data(),
		                                   &err))
			ThrowAbi(err);
		for (idx_t g = 0; g < b.Groups(); g++) {
			const idx_t r = b.result_rows[g];
			const double *c = core.data() + g * rec;
			if (c[p + 5] != 0.0) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			AppendList(*entries[0], r, c, p);
			for (idx_t k = 0; k < 4; k++) FlatVector::GetData<double>(*entries[1 + k])[r] = c[p + k];
			FlatVector::GetData<int64_t>(*entries[5])[r] = (int64_t)c[p + 4];
			FlatVector::GetData<int64_t>(*entries[6])[r] = (int64_t)p;
		}
	}
}

unique_ptr<FunctionData> HipRlsFitAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipRlsOptions opts;
	if (arguments.size() > 2 && arguments[2]->IsFoldable()) ParseHipRlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), opts);
	function.return_type = GetHipRlsFitAggResultType();
	return make_uniq<HipRlsFamilyBindData>(opts, false);
}

} // namespace

void RegisterHipRlsAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_rls_fit_agg";
	const char *what = "Fits a Recursive Least Squares model over the group's rows in order and returns coefficients as a struct.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>,
			                                  RowsInitialize, HipRlsFitAggUpdate, RowsCombine<false>, HipRlsFitAggFinalize, nullptr,
			                                  HipRlsFitAggBind, RowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic, kCategories));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'forgetting_factor': 0.99})", {"y", "x", "options"}, map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("rls_fit_agg"));
}

void RegisterHipRlsFitPredictAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_rls_fit_predict_agg";
	const char *what = "Fits Recursive Least Squares over a partition and returns per-row predictions.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	const vector<LogicalType> split_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR};
	const vector<LogicalType> split_map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR, LogicalType::ANY};
	auto make = [](const string &fname, const vector<LogicalType> &args, bool split) {
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>, RowsInitialize,
		                         HipRlsPredictAggUpdate, RowsCombine<false>, HipRlsPredictAggFinalize, nullptr,
		                         split ? HipRlsPredictAggBind<true> : HipRlsPredictAggBind<false>, RowsDestroy);
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
	info.descriptions.push_back(Describe(what, head + ", {'forgetting_factor': 0.99})", {"y", "x", "options"}, map_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col)", {"y", "x", "split_col"}, split_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'forgetting_factor': 0.99})", {"y", "x", "split_col", "options"}, split_map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("rls_fit_predict_agg"));
	for (const char *alias : {"rls_predict_agg", "anofox_stats_rls_predict_agg"}) RegisterAlias(loader, name, fill(alias)); // the deprecated names
}

void RegisterHipRlsFitPredictFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_rls_fit_predict";
	const char *what = "Fits a Recursive Least Squares model over a window partition and returns predictions.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, FitPredictResultType(), AggregateFunction::StateSize<RowsState>, RowsInitialize,
			                                  HipRlsFitPredictUpdate, RowsCombine<true>, HipRlsFitPredictFinalize, nullptr, HipRlsFitPredictBind,
			                                  RowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic, kCategories));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'null_policy': 'drop'})", {"y", "x", "options"}, map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("rls_fit_predict"));
}

} // namespace duckdb
