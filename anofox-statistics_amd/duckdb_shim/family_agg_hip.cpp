// family_agg_hip.cpp — DuckDB glue of the rest of the regression family over the batched C ABI:
//
//   {ols,ridge,wls}_fit_predict_agg   src/aggregate_functions/ols_predict_aggregate.cpp   (state :21-58, bind data :63-88,
//                                     result type :93-104, Update :134-268, Combine :271-327, Finalize :330-425, Bind
//                                     :430-492, registration :497-603), ridge_predict_aggregate.cpp, wls_predict_aggregate.cpp
//   {ols,ridge,wls}_fit_predict       src/window_functions/ols_fit_predict.cpp (state :21-52, Update :110-193, Combine
//                                     :196-243, Finalize :246-324, Bind :329-355, registration :360-409),
//                                     ridge_fit_predict.cpp, wls_fit_predict.cpp — aggregates DuckDB's window operator drives
//   vif_agg                           src/aggregate_functions/vif_aggregate.cpp (Update :50-95, Combine :97-129, Finalize
//                                     :144-185, registration :201-232)
//
// The reference fits ONE state per FFI call inside its Finalize loop.  Here the DuckDB state still buffers the group's
// rows on the host (these aggregates return every row, in arrival order, so the rows must be kept whatever fits them) and
// Finalize turns the whole vector of states (up to 2048) into ONE call of anofox_hip_fit_predict_batch_host /
// anofox_hip_vif_batch_host per feature count: states = groups, columns concatenated, NaN y = "does not train".
// The SQL surface is the reference's: names, aliases and deprecated aliases, the overloads with and without the split column
// and the constant options argument, LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training)) / STRUCT(yhat, yhat_lower,
// yhat_upper) / LIST(DOUBLE), NULL where the reference returns NULL.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub) with a mock of
// the C ABI under ASan / UBSan, and on the GPU with the real library against the oracle (tests/test_gpu_glue.py).
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <memory>

#include "duckdb.hpp"
#include "duckdb/common/types/data_chunk.hpp"
#include "duckdb/execution/expression_executor.hpp"
#include "duckdb/function/aggregate_function.hpp"
#include "duckdb/main/extension/extension_loader.hpp"
#include "duckdb/parser/parsed_data/create_aggregate_function_info.hpp"

#include "anofox_stats_hip.h"
#include "family_agg_hip.hpp"
#include "hip_options.hpp"
#include "row_shapes.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "prediction"};

// ---- bind data of the predict aggregate and the window aggregate: the parsed options and the model ----
using HipFamilyBindData = RowsBindData<HipFitOptions, HipModel>;

AnofoxHipBatchOptions BatchOptions(const HipFamilyBindData &bind) {
	HipFitOptions o = bind.opts;
	o.compute_inference = false; // both aggregates fit with inference off (ols_predict_aggregate.cpp:356, ols_fit_predict.cpp:283)
	return MakeHipOptions(bind.kind, o);
}

// ---- the states of one Finalize vector as one batch per feature count through the family's ABI call ----
struct FamilyBatch : PredictBatch {
	// extra_row: the window aggregate appends its current x as a row that does not train
	void Run(const AnofoxHipBatchOptions &options, bool weighted, bool extra_row) {
		const int64_t n = StagePredict(weighted, extra_row);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), weighted ? w.data() : nullptr,
		                                       train_counts.data(), options, core.data(), pred.data(), &err))
			ThrowAbi(err);
	}
};

// What differs between the three models' Updates.  RowsOf's text has the counts in ols_predict_aggregate.cpp / ols_fit_predict.cpp
// and is bare in the ridge / wls files.  A NULL feature: the OLS file clears the training flag (ols_predict_aggregate.cpp:236-239);
// the ridge / wls files keep it — the row is handed to the fit, whose row filter drops it — and so does the is_training column
// of their output.  Weights: wls_predict_aggregate.cpp:160-240, wls_fit_predict.cpp:150-154.
template <HipModel MODEL, bool WINDOW>
struct FamilyTraits : RowTraits {
	using Bind = HipFamilyBindData;
	static constexpr const char *kName = WINDOW ? "fit_predict" : "fit_predict_agg";
	static constexpr bool kCountsInError = MODEL == HipModel::OLS;
	static constexpr bool kWeighted = MODEL == HipModel::WLS;
	static constexpr bool kNullElementStopsTraining = MODEL == HipModel::OLS; // (the predict aggregate; the window never looks)
	static bool DropYZeroX(const Bind &bind) { return bind.opts.drop_y_zero_x; }
};

constexpr idx_t FirstOptional(HipModel model) { return model == HipModel::WLS ? 3 : 2; } // after y, x[, weights]

// =====================================================================================================================
// *_fit_predict_agg(y, x[, weights][, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
void HipPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipFamilyBindData>();
	const auto options = BatchOptions(bind);
	// fewer than 2 training rows -> NULL (ols_predict_aggregate.cpp:343-346)
	FinalizePredictRows<FamilyBatch>(
	    state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; },
	    [&](FamilyBatch &b) { b.Run(options, bind.kind == HipModel::WLS, false); });
}

template <HipModel MODEL, bool SPLIT>
unique_ptr<FunctionData> HipPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipFitOptions>(context, function, arguments, FirstOptional(MODEL) + (SPLIT ? 1 : 0) /* ols_predict_aggregate.cpp:435 / :466 */, SPLIT,
	                               ParseHipFitOptions, [](const HipFitOptions &) { return PredictAggResultType(); }, MODEL);
}

template <HipModel MODEL>
void RegisterHipPredictAggregate(ExtensionLoader &loader, const string &model_name, const char *what) {
	RowsFunctionNames f {"anofox_stats_" + model_name + "_fit_predict_agg", model_name + "_fit_predict_agg",
	                     // the two deprecated names (ols_predict_aggregate.cpp:563-602)
	                     {model_name + "_predict_agg", "anofox_stats_" + model_name + "_predict_agg"}, what, kCategories};
	if (MODEL == HipModel::WLS) {
		f.base.push_back(LogicalType::DOUBLE);
		f.base_names.push_back("weights");
	}
	RegisterWithSplitAndOptions(loader, f, "{'null_policy': 'drop'}", "{'null_policy': 'drop'}", [](const string &fname, const vector<LogicalType> &args, bool split) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsPredictAggUpdate<FamilyTraits<MODEL, false>>, RowsCombine<false, true>,
		                    HipPredictAggFinalize, split ? HipPredictAggBind<MODEL, true> : HipPredictAggBind<MODEL, false>);
	});
}

// =====================================================================================================================
// *_fit_predict(y, x[, weight][, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// =====================================================================================================================
void HipFitPredictFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipFamilyBindData>();
	const auto options = BatchOptions(bind);
	FinalizeWindowRows<FamilyBatch, false>(state_vector, result, count, offset, bind.opts.fit_intercept,
	                                       [&](FamilyBatch &b) { b.Run(options, bind.kind == HipModel::WLS, true); });
}

template <HipModel MODEL>
unique_ptr<FunctionData> HipFitPredictBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipFitOptions>(context, function, arguments, FirstOptional(MODEL) /* ols_fit_predict.cpp:333 */, false, ParseHipFitOptions,
	                               [](const HipFitOptions &) { return FitPredictResultType(); }, MODEL);
}

template <HipModel MODEL>
void RegisterHipFitPredict(ExtensionLoader &loader, const string &model_name, const char *what) {
	RowsFunctionNames f {"anofox_stats_" + model_name + "_fit_predict", model_name + "_fit_predict", {}, what, kCategories};
	if (MODEL == HipModel::WLS) {
		f.base.push_back(LogicalType::DOUBLE);
		f.base_names.push_back("weight");
	}
	RegisterWithOptions(loader, f, "{'null_policy': 'drop'}", [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, FitPredictResultType(), RowsWindowUpdate<FamilyTraits<MODEL, true>>, RowsCombine<true>, HipFitPredictFinalize,
		                    HipFitPredictBind<MODEL>);
	});
}

// =====================================================================================================================
// vif_agg(x LIST(DOUBLE)) -> LIST(DOUBLE)
// =====================================================================================================================
// the state: one column of values per feature — Update appends every non-NaN value to ITS column (vif_aggregate.cpp:86-92),
// so a NaN shortens that column only and Finalize meets columns of unequal length (-> NULL, vif.rs:40-51)
struct VifColumns {
	vector<vector<double>> columns;
};
struct HipVifState {
	VifColumns *cols;
};

void HipVifInitialize(const AggregateFunction &, data_ptr_t state_p) { reinterpret_cast<HipVifState *>(state_p)->cols = nullptr; }

void HipVifDestroy(Vector &state_vector, AggregateInputData &, idx_t count) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipVifState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		delete state.cols;
		state.cols = nullptr;
	}
}

void HipVifUpdate(Vector inputs[], AggregateInputData &, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 1) throw InvalidInputException("anofox_stats vif_agg (HIP): too few arguments");
	UnifiedVectorFormat x_data, sdata;
	inputs[0].ToUnifiedFormat(count, x_data);
	auto x_list = UnifiedVectorFormat::GetData<list_entry_t>(x_data);
	auto &x_child = ListVector::GetEntry(inputs[0]);
	auto x_child_data = FlatVector::GetData<double>(x_child);
	auto &x_child_validity = FlatVector::Validity(x_child);
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipVifState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		if (!state.cols) {
			state.cols = new VifColumns();
			state.cols->columns.resize(entry.length);
		}
		auto &columns = state.cols->columns;
		if (entry.length != columns.size())
			throw InvalidInputException("Inconsistent feature count: expected %llu, got %llu", (unsigned long long)columns.size(),
			                            (unsigned long long)entry.length);
		for (idx_t j = 0; j < entry.length; j++) {
			const idx_t pos = entry.offset + j;
			if (!x_child_validity.RowIsValid(pos)) continue; // (a NULL element: as a NaN — the reference reads the slot as it is)
			const double v = x_child_data[pos];
			if (!std::isnan(v)) columns[j].push_back(v);
		}
	}
}

void HipVifCombine(Vector &source_vector, Vector &target_vector, AggregateInputData &aggr_input_data, idx_t count) {
	UnifiedVectorFormat source_data, target_data;
	source_vector.ToUnifiedFormat(count, source_data);
	target_vector.ToUnifiedFormat(count, target_data);
	auto sources = (HipVifState **)source_data.data;
	auto targets = (HipVifState **)target_data.data;
	const bool preserve = aggr_input_data.combine_type == AggregateCombineType::PRESERVE_INPUT;
	for (idx_t i = 0; i < count; i++) {
		auto &source = *sources[source_data.sel->get_index(i)];
		auto &target = *targets[target_data.sel->get_index(i)];
		if (!source.cols || &source == &target) continue;
		if (!target.cols) {
			if (preserve) {
				target.cols = new VifColumns(*source.cols);
			} else {
				target.cols = source.cols;
				source.cols = nullptr;
			}
			continue;
		}
		if (source.cols->columns.size() != target.cols->columns.size())
			throw InvalidInputException("Cannot combine states with different feature counts: %llu vs %llu", (unsigned long long)source.cols->columns.size(),
			                            (unsigned long long)target.cols->columns.size());
		for (idx_t j = 0; j < target.cols->columns.size(); j++)
			target.cols->columns[j].insert(target.cols->columns[j].end(), source.cols->columns[j].begin(), source.cols->columns[j].end());
	}
}

// Finalize (vif_aggregate.cpp:144-185): NULL without rows, with fewer than 2 features or fewer than 3 values in the first
// column, and when the columns differ in length; every other state of the vector goes into one batched call per feature count
void HipVifFinalize(Vector &state_vector, AggregateInputData &, Vector &result, idx_t count, idx_t offset) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipVifState **)sdata.data;
	struct Batch {
		vector<idx_t> result_rows;
		vector<VifColumns *> cols;
	};
	std::map<idx_t, Batch> batches;
	const idx_t max_features = anofox_hip_vif_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		bool usable = state.cols && state.cols->columns.size() >= 2 && state.cols->columns[0].size() >= 3;
		if (usable)
			for (auto &c : state.cols->columns) usable = usable && c.size() == state.cols->columns[0].size();
		if (!usable) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		CheckMaxFeatures("vif_agg", state.cols->columns.size(), max_features);
		auto &b = batches[state.cols->columns.size()];
		b.result_rows.push_back(i + offset);
		b.cols.push_back(state.cols);
	}
	for (auto &kv : batches) {
		const idx_t p = kv.first;
		auto &b = kv.second;
		vector<int64_t> offsets {0};
		for (auto *c : b.cols) offsets.push_back(offsets.back() + (int64_t)c->columns[0].size());
		const size_t n = (size_t)offsets.back();
		vector<double> cols(n * p);
		for (idx_t g = 0; g < b.cols.size(); g++)
			for (idx_t j = 0; j < p; j++) std::copy(b.cols[g]->columns[j].begin(), b.cols[g]->columns[j].end(), cols.begin() + j * n + (size_t)offsets[g]);
		vector<const double *> col_ptrs(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * n;
		const size_t rec = anofox_hip_vif_record_len(p);
		vector<double> vif(b.cols.size() * rec);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_vif_batch_host(nullptr, (int64_t)b.cols.size(), p, (int64_t)n, offsets.data(), col_ptrs.data(), vif.data(), &err)) ThrowAbi(err);
		for (idx_t g = 0; g < b.cols.size(); g++) {
			const idx_t r = b.result_rows[g];
			if (vif[g * rec + p] != 0.0) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			AppendList(result, r, &vif[g * rec], p); // (reserved first: the reference's SetListInResult omits that, vif_aggregate.cpp:132-141)
		}
	}
}

unique_ptr<FunctionData> HipVifBind(ClientContext &, AggregateFunction &function, vector<unique_ptr<Expression>> &) {
	function.return_type = LogicalType::LIST(LogicalType::DOUBLE);
	return nullptr; // no options, no bind data (vif_aggregate.cpp:190-195)
}

} // namespace

void RegisterHipOlsFitPredictAggregateFunction(ExtensionLoader &loader) {
	RegisterHipPredictAggregate<HipModel::OLS>(loader, "ols", "Fits OLS regression over a partition and returns per-row predictions with confidence intervals.");
}
void RegisterHipRidgeFitPredictAggregateFunction(ExtensionLoader &loader) {
	RegisterHipPredictAggregate<HipModel::RIDGE>(loader, "ridge", "Fits Ridge regression over a partition and returns per-row predictions with confidence intervals.");
}
void RegisterHipWlsFitPredictAggregateFunction(ExtensionLoader &loader) {
	RegisterHipPredictAggregate<HipModel::WLS>(loader, "wls", "Fits WLS regression over a partition using weights and returns per-row predictions.");
}
void RegisterHipOlsFitPredictFunction(ExtensionLoader &loader) {
	RegisterHipFitPredict<HipModel::OLS>(loader, "ols", "Fits an OLS model over a window partition and returns predictions for each row, including confidence intervals.");
}
void RegisterHipRidgeFitPredictFunction(ExtensionLoader &loader) {
	RegisterHipFitPredict<HipModel::RIDGE>(loader, "ridge", "Fits a Ridge regression model over a window partition and returns predictions for each row.");
}
void RegisterHipWlsFitPredictFunction(ExtensionLoader &loader) {
	RegisterHipFitPredict<HipModel::WLS>(loader, "wls", "Fits a WLS regression model over a window partition using per-row weights and returns predictions.");
}
void RegisterHipVifAggregateFunction(ExtensionLoader &loader) {
	auto make = [](const string &fname) {
		return AggregateFunction(fname, {LogicalType::LIST(LogicalType::DOUBLE)}, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<HipVifState>,
		                         HipVifInitialize, HipVifUpdate, HipVifCombine, HipVifFinalize, nullptr, HipVifBind, HipVifDestroy);
	};
	AggregateFunctionSet func_set("anofox_stats_vif_agg");
	func_set.AddFunction(make("anofox_stats_vif_agg"));
	CreateAggregateFunctionInfo info(std::move(func_set));
	info.descriptions.push_back(Describe("Aggregate version of VIF: computes Variance Inflation Factor for each feature from a column of feature vectors.",
	                                     "anofox_stats_vif_agg(x)", {"x"}, {LogicalType::LIST(LogicalType::DOUBLE)}, {"regression-diagnostics"}));
	AggregateFunctionSet alias_set("vif_agg");
	alias_set.AddFunction(make("vif_agg"));
	RegisterWithAlias(loader, std::move(info), std::move(alias_set));
}

} // namespace duckdb
