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
#include "row_shapes.hpp"

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

using HipRlsFamilyBindData = RowsBindData<HipRlsOptions>;

// the states of one Finalize vector as one batch per feature count through the fit-predict call
struct RlsBatch : PredictBatch {
	void Run(const HipRlsOptions &opts, bool extra_row) {
		const int64_t n = StagePredict(false, extra_row);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_rls_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                           opts.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			ThrowAbi(err);
	}
};

// Update: rls_predict_aggregate.cpp:150-245 (RowsOf's bare text :190-192), rls_fit_predict.cpp:100-163 (a NULL x list :134-137,
// drop_y_zero_x :162-169); the fit aggregate buffers every row with a non-NULL y and x list
struct RlsTraits : RowTraits {
	using Bind = HipRlsFamilyBindData;
	static bool DropYZeroX(const Bind &bind) { return bind.opts.drop_y_zero_x; }
};
struct RlsPredictAggTraits : RlsTraits { static constexpr const char *kName = "rls_fit_predict_agg"; };
struct RlsWindowTraits : RlsTraits { static constexpr const char *kName = "rls_fit_predict"; };
struct RlsFitAggTraits : RlsTraits { static constexpr const char *kName = "rls_fit_agg"; };

// =====================================================================================================================
// anofox_stats_rls_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Finalize (:299-395): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with its prediction
void HipRlsPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	FinalizePredictRows<RlsBatch>(
	    state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; }, [&](RlsBatch &b) { b.Run(bind.opts, false); });
}

// =====================================================================================================================
// anofox_stats_rls_fit_predict(y, x[, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// =====================================================================================================================
// Finalize (rls_fit_predict.cpp:212-271): NULL without a current row or with at most p + [intercept] training rows, or when the
// fit or the prediction fails
void HipRlsFitPredictFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	FinalizeWindowRows<RlsBatch, true>(state_vector, result, count, offset, bind.opts.fit_intercept, [&](RlsBatch &b) { b.Run(bind.opts, true); });
}

// every function of the family binds the same options; OPT_IDX: 2, or 3 behind a split column
template <idx_t OPT_IDX, LogicalType (*TYPE)()>
unique_ptr<FunctionData> HipRlsBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipRlsOptions>(context, function, arguments, OPT_IDX, OPT_IDX == 3, ParseHipRlsOptions, [](const HipRlsOptions &) { return TYPE(); });
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

} // namespace

void RegisterHipRlsAggregateFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_rls_fit_agg", "rls_fit_agg", {},
	                           "Fits a Recursive Least Squares model over the group's rows in order and returns coefficients as a struct.", kCategories};
	RegisterWithOptions(loader, f, "{'forgetting_factor': 0.99}", [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsFitAggUpdate<RlsFitAggTraits>, RowsCombine<false>, HipRlsFitAggFinalize,
		                    HipRlsBind<2, GetHipRlsFitAggResultType>);
	});
}

void RegisterHipRlsFitPredictAggregateFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_rls_fit_predict_agg", "rls_fit_predict_agg", {"rls_predict_agg", "anofox_stats_rls_predict_agg"}, // the deprecated names
	                           "Fits Recursive Least Squares over a partition and returns per-row predictions.", kCategories};
	RegisterWithSplitAndOptions(loader, f, "{'forgetting_factor': 0.99}", "{'forgetting_factor': 0.99}", [](const string &fname, const vector<LogicalType> &args, bool split) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsPredictAggUpdate<RlsPredictAggTraits>, RowsCombine<false>, HipRlsPredictAggFinalize,
		                    split ? HipRlsBind<3, PredictAggResultType> : HipRlsBind<2, PredictAggResultType>);
	});
}

void RegisterHipRlsFitPredictFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_rls_fit_predict", "rls_fit_predict", {},
	                           "Fits a Recursive Least Squares model over a window partition and returns predictions.", kCategories};
	RegisterWithOptions(loader, f, "{'null_policy': 'drop'}", [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, FitPredictResultType(), RowsWindowUpdate<RlsWindowTraits>, RowsCombine<true>, HipRlsFitPredictFinalize,
		                    HipRlsBind<2, FitPredictResultType>);
	});
}

} // namespace duckdb
