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
#include "row_shapes.hpp"

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

using HipEnFamilyBindData = RowsBindData<HipEnPredictOptions>;

// the states of one Finalize vector as one batch per feature count through the fit-predict call
struct EnBatch : PredictBatch {
	void Run(const HipEnPredictOptions &opts, bool extra_row) {
		const int64_t n = StagePredict(false, extra_row);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_elasticnet_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                                  opts.en.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			ThrowAbi(err);
	}
};

// Update: elasticnet_predict_aggregate.cpp:150-245 (RowsOf's bare text :190-192), elasticnet_fit_predict.cpp:110-180 (drop_y_zero_x :162-169)
template <bool WINDOW>
struct EnTraits : RowTraits {
	using Bind = HipEnFamilyBindData;
	static constexpr const char *kName = WINDOW ? "elasticnet_fit_predict" : "elasticnet_fit_predict_agg";
	static bool DropYZeroX(const Bind &bind) { return bind.opts.drop_y_zero_x; }
};

// =====================================================================================================================
// anofox_stats_elasticnet_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Finalize (:299-395): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with its prediction
void HipEnPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipEnFamilyBindData>();
	FinalizePredictRows<EnBatch>(
	    state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; }, [&](EnBatch &b) { b.Run(bind.opts, false); });
}

// use_lambda = false: the aggregate's bind (alpha only)
template <bool SPLIT>
unique_ptr<FunctionData> HipEnPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipEnPredictOptions>(
	    context, function, arguments, SPLIT ? 3 : 2, SPLIT, [](const Value &v, HipEnPredictOptions &o) { ParseHipEnPredictOptions(v, o, false); },
	    [](const HipEnPredictOptions &) { return PredictAggResultType(); });
}

// =====================================================================================================================
// anofox_stats_elasticnet_fit_predict(y, x[, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// =====================================================================================================================
// Finalize (elasticnet_fit_predict.cpp:235-290): NULL without a current row or with at most p + [intercept] training rows, or when
// the fit or the prediction fails (:270-286)
void HipEnFitPredictFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipEnFamilyBindData>();
	FinalizeWindowRows<EnBatch, true>(state_vector, result, count, offset, bind.opts.en.fit_intercept, [&](EnBatch &b) { b.Run(bind.opts, true); });
}

unique_ptr<FunctionData> HipEnFitPredictBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipEnPredictOptions>(
	    context, function, arguments, 2, false, [](const Value &v, HipEnPredictOptions &o) { ParseHipEnPredictOptions(v, o, true); },
	    [](const HipEnPredictOptions &) { return FitPredictResultType(); });
}

} // namespace

void RegisterHipElasticNetFitPredictAggregateFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_elasticnet_fit_predict_agg", "elasticnet_fit_predict_agg",
	                           {"elasticnet_predict_agg", "anofox_stats_elasticnet_predict_agg"}, // the deprecated names
	                           "Fits Elastic Net regression over a partition and returns per-row predictions with confidence intervals.", kCategories};
	RegisterWithSplitAndOptions(loader, f, "{'alpha': 1.0, 'l1_ratio': 0.5}", "{'alpha': 1.0}", [](const string &fname, const vector<LogicalType> &args, bool split) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsPredictAggUpdate<EnTraits<false>>, RowsCombine<false>, HipEnPredictAggFinalize,
		                    split ? HipEnPredictAggBind<true> : HipEnPredictAggBind<false>);
	});
}

void RegisterHipElasticNetFitPredictFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_elasticnet_fit_predict", "elasticnet_fit_predict", {},
	                           "Fits an ElasticNet regression model over a window partition and returns predictions with confidence intervals.", kCategories};
	RegisterWithOptions(loader, f, "{'null_policy': 'drop'}", [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, FitPredictResultType(), RowsWindowUpdate<EnTraits<true>>, RowsCombine<true>, HipEnFitPredictFinalize, HipEnFitPredictBind);
	});
}

} // namespace duckdb
