// bls_family_hip.cpp — DuckDB glue of the bounded least squares aggregates over the batched C ABI:
//
//   anofox_stats_bls_fit_agg, anofox_stats_nnls_fit_agg   src/aggregate_functions/bls_aggregate.cpp (state :19-45, bind data :48-79,
//                                                         result type :83-96, Update :118-180, Combine, Finalize :249-330, binds
//                                                         :335-396, registration)
//   anofox_stats_bls_fit_predict_agg                      src/aggregate_functions/bls_fit_predict_aggregate.cpp (Update :146-265,
//                                                         Combine :268-323, Finalize :326-452)
//
// As the other glue files: the DuckDB state buffers the group's rows on the host, and Finalize turns the whole vector of
// states into ONE batched call per feature count (anofox_hip_bls_fit_batch_host / anofox_hip_bls_fit_predict_batch_host):
// states = groups, columns concatenated, NaN y = "does not train".  LIST children are reserved before they are written.
//
// Options (map_options_parser.cpp:637-721): fit_intercept / intercept (default FALSE), lower_bound / lower, upper_bound /
// upper (one number for every column), max_iterations / max_iter, tolerance / tol; the fit-predict aggregate also reads
// confidence_level / confidence and null_policy.  nnls_fit_agg's bind reads fit_intercept, max_iterations and tolerance only
// (bls_aggregate.cpp:370-396): bound keys are silently ignored there.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU
// with the real library (tests/test_gpu_bls_glue.py through tests/tools/bls_family_capi.cpp).
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
#include "bls_family_hip.hpp"
#include "hip_options.hpp"
#include "row_shapes.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression"};

struct HipBlsOptions {
	bool fit_intercept = false; // bls_aggregate.cpp:49
	bool has_lower = false, has_upper = false;
	double lower = 0.0, upper = 0.0;
	uint32_t max_iterations = 1000;
	double tolerance = 1e-10;
	double confidence_level = 0.95;
	bool drop_y_zero_x = false;
	bool operator==(const HipBlsOptions &o) const {
		return fit_intercept == o.fit_intercept && has_lower == o.has_lower && has_upper == o.has_upper && lower == o.lower && upper == o.upper &&
		       max_iterations == o.max_iterations && tolerance == o.tolerance && confidence_level == o.confidence_level &&
		       drop_y_zero_x == o.drop_y_zero_x;
	}
	// (the bound pointers point into this object: it outlives the call it is passed to)
	AnofoxHipBlsBatchOptions Batch() const {
		AnofoxHipBlsBatchOptions b;
		memset(&b, 0, sizeof b);
		b.fit_intercept = fit_intercept;
		b.lower_bounds = has_lower ? &lower : nullptr;
		b.lower_bounds_len = has_lower ? 1 : 0;
		b.upper_bounds = has_upper ? &upper : nullptr;
		b.upper_bounds_len = has_upper ? 1 : 0;
		b.max_iterations = max_iterations;
		b.tolerance = tolerance;
		return b;
	}
};

// bounds = false: nnls_fit_agg's bind; predict = true: the fit-predict aggregate's.  A key this bind does not read is still
// converted (parsed by the shared parser whoever reads it).
void ParseHipBlsOptions(const Value &v, HipBlsOptions &o, bool bounds, bool predict) {
	if (v.IsNull()) return;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (val.IsNull()) return;
		if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(val);
		else if (key == "max_iterations" || key == "max_iter") o.max_iterations = ExtractUInteger(val);
		else if (key == "tolerance" || key == "tol") o.tolerance = val.GetValue<double>();
		else if (key == "lower_bound" || key == "lower") {
			const double b = val.GetValue<double>();
			if (bounds) { o.lower = b; o.has_lower = true; }
		} else if (key == "upper_bound" || key == "upper") {
			const double b = val.GetValue<double>();
			if (bounds) { o.upper = b; o.has_upper = true; }
		} else if (key == "confidence_level" || key == "confidence") {
			const double c = val.GetValue<double>();
			if (predict) o.confidence_level = c;
		} else if (key == "null_policy") {
			const bool drop_y_zero_x = ExtractNullPolicy(val);
			if (predict) o.drop_y_zero_x = drop_y_zero_x;
		}
		// every other key: ignored, as in the reference
	});
}

using HipBlsBindData = RowsBindData<HipBlsOptions>;

// the states of one Finalize vector as one batch per feature count through the fit-predict call
struct BlsPredictBatch : PredictBatch {
	void Run(const HipBlsOptions &opts) {
		const int64_t n = StagePredict(false, false);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_bls_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                           opts.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			ThrowAbi(err);
	}
};

// Update: bls_fit_predict_aggregate.cpp:146-265 (RowsOf's bare text :204-207); bls_aggregate.cpp:118-180 for both fit aggregates,
// nnls_fit_agg under the name of bls_fit_agg
struct BlsPredictAggTraits : RowTraits {
	using Bind = HipBlsBindData;
	static constexpr const char *kName = "bls_fit_predict_agg";
	static bool DropYZeroX(const Bind &bind) { return bind.opts.drop_y_zero_x; }
};
struct BlsFitAggTraits : RowTraits { static constexpr const char *kName = "bls_fit_agg"; };

// bounds = false: nnls_fit_agg's bind; predict = true: the fit-predict aggregate's
template <bool BOUNDS, bool PREDICT, bool SPLIT, LogicalType (*TYPE)()>
unique_ptr<FunctionData> HipBlsBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipBlsOptions>(
	    context, function, arguments, SPLIT ? 3 : 2, SPLIT, [](const Value &v, HipBlsOptions &o) { ParseHipBlsOptions(v, o, BOUNDS, PREDICT); },
	    [](const HipBlsOptions &) { return TYPE(); });
}

// =====================================================================================================================
// anofox_stats_bls_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Finalize (bls_fit_predict_aggregate.cpp:326-452): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with its prediction
void HipBlsPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipBlsBindData>();
	FinalizePredictRows<BlsPredictBatch>(
	    state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; }, [&](BlsPredictBatch &b) { b.Run(bind.opts); });
}

// =====================================================================================================================
// anofox_stats_bls_fit_agg / anofox_stats_nnls_fit_agg (y, x[, options]) -> STRUCT(coefficients, intercept, ssr, r_squared,
// n_observations, n_features, n_active_constraints, at_lower_bound, at_upper_bound)
// =====================================================================================================================
LogicalType GetHipBlsAggResultType() { // bls_aggregate.cpp:83-96
	child_list_t<LogicalType> children;
	children.push_back(make_pair("coefficients", LogicalType::LIST(LogicalType::DOUBLE)));
	children.push_back(make_pair("intercept", LogicalType::DOUBLE));
	children.push_back(make_pair("ssr", LogicalType::DOUBLE));
	children.push_back(make_pair("r_squared", LogicalType::DOUBLE));
	children.push_back(make_pair("n_observations", LogicalType::BIGINT));
	children.push_back(make_pair("n_features", LogicalType::BIGINT));
	children.push_back(make_pair("n_active_constraints", LogicalType::BIGINT));
	children.push_back(make_pair("at_lower_bound", LogicalType::LIST(LogicalType::BOOLEAN)));
	children.push_back(make_pair("at_upper_bound", LogicalType::LIST(LogicalType::BOOLEAN)));
	return LogicalType::STRUCT(std::move(children));
}

// Finalize (bls_aggregate.cpp:249-330): NULL with fewer than 2 buffered rows or a failed fit; ONE batched call per feature count
void HipBlsAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipBlsBindData>();
	auto batches = CollectBatches<RowBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 2; });
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		const idx_t p = b.p, G = b.Groups(), rec_len = 3 * p + 6;
		const int64_t n = b.Stage(false, false); // (every buffered row trains)
		vector<double> rec(G * rec_len);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_bls_fit_batch_host(nullptr, (int64_t)G, p, n, b.offsets.data(), b.y.data(), b.col_ptrs.data(), bind.opts.Batch(), rec.data(), nullptr,
		                                   &err))
			ThrowAbi(err);
		for (idx_t g = 0; g < G; g++) {
			const idx_t r = b.result_rows[g];
			const double *rc = &rec[g * rec_len];
			if (rc[p + 5] != 0.0) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			// the three LIST children: reserved before they are written
			Vector *lists[3] = {fields[0].get(), fields[7].get(), fields[8].get()};
			for (int l = 0; l < 3; l++) {
				Vector &lv = *lists[l];
				const idx_t lo = AppendListEntry(lv, r, p);
				Vector &child = ListVector::GetEntry(lv);
				for (idx_t j = 0; j < p; j++) {
					if (l == 0) {
						if (isnan(rc[j])) FlatVector::SetNull(child, lo + j, true); // SetListInResult: NaN -> NULL
						else FlatVector::GetData<double>(child)[lo + j] = rc[j];
					} else {
						FlatVector::GetData<bool>(child)[lo + j] = rc[(l == 1 ? p + 6 : 2 * p + 6) + j] != 0.0;
					}
				}
			}
			if (isnan(rc[p])) FlatVector::SetNull(*fields[1], r, true);
			else FlatVector::GetData<double>(*fields[1])[r] = rc[p];
			FlatVector::GetData<double>(*fields[2])[r] = rc[p + 1];
			FlatVector::GetData<double>(*fields[3])[r] = rc[p + 2];
			FlatVector::GetData<int64_t>(*fields[4])[r] = (int64_t)rc[p + 3];
			FlatVector::GetData<int64_t>(*fields[5])[r] = (int64_t)p;
			FlatVector::GetData<int64_t>(*fields[6])[r] = (int64_t)rc[p + 4];
		}
	}
}

template <bool NNLS>
void RegisterFit(ExtensionLoader &loader, const char *name, const char *alias, const char *what) {
	const RowsFunctionNames f {name, alias, {}, what, kCategories};
	RegisterWithOptions(loader, f, "{'fit_intercept': true}", [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, GetHipBlsAggResultType(), RowsFitAggUpdate<BlsFitAggTraits>, RowsCombine<false>, HipBlsAggFinalize,
		                    HipBlsBind<!NNLS, false, false, GetHipBlsAggResultType>);
	});
}

} // namespace

void RegisterHipBlsAggregateFunction(ExtensionLoader &loader) {
	RegisterFit<false>(loader, "anofox_stats_bls_fit_agg", "bls_fit_agg", "Fits a bounded least squares regression per group.");
}

void RegisterHipBlsNnlsAggregateFunction(ExtensionLoader &loader) {
	RegisterFit<true>(loader, "anofox_stats_nnls_fit_agg", "nnls_fit_agg", "Fits a non-negative least squares regression per group.");
}

void RegisterHipBlsFitPredictAggregateFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_bls_fit_predict_agg", "bls_fit_predict_agg", {},
	                           "Fits bounded least squares over a partition and returns per-row predictions with confidence intervals.", kCategories};
	RegisterWithSplitAndOptions(loader, f, "{'lower_bound': 0.0}", "{'upper_bound': 1.0}", [](const string &fname, const vector<LogicalType> &args, bool split) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsPredictAggUpdate<BlsPredictAggTraits>, RowsCombine<false>, HipBlsPredictAggFinalize,
		                    split ? HipBlsBind<true, true, true, PredictAggResultType> : HipBlsBind<true, true, false, PredictAggResultType>);
	});
}

} // namespace duckdb
