// elasticnet_agg_hip.cpp — DuckDB glue of anofox_stats_elasticnet_fit_agg / elasticnet_fit_agg over the batched C ABI.
//
// Reference: src/aggregate_functions/elasticnet_aggregate.cpp (state, bind data, the 7-field result STRUCT, Update, Combine,
// Finalize, Bind, registration).  The state buffers the group's rows on the host as the reference's does; Finalize turns the
// whole vector of states into ONE anofox_hip_elasticnet_fit_batch_host call per feature count (states = groups, columns
// concatenated) instead of one anofox_elasticnet_fit call per state.  NULL where the reference returns NULL: fewer than 2
// buffered rows, or a failing fit (status != 0).
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU
// with the real library (tests/test_gpu_elasticnet_glue.py through tests/tools/elasticnet_glue_capi.cpp).
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
#include "elasticnet_agg_hip.hpp"
#include "hip_options.hpp"
#include "row_shapes.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

using HipElasticNetBindData = RowsBindData<HipElasticNetOptions>;

// Update (elasticnet_aggregate.cpp Update): the feature count is fixed by the first accepted row and RowsOf's text has the
// counts; the width is checked in Finalize, of what is about to be fitted
struct EnFitAggTraits : RowTraits {
	static constexpr const char *kName = "elasticnet_fit_agg";
	static constexpr bool kCheckMaxFeatures = false;
	static constexpr bool kCountsInError = true;
};

LogicalType GetElasticNetResultType() { // elasticnet_aggregate.cpp:78-90
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

// Finalize: NULL without rows or with fewer than 2 (the reference's check before its FFI call); every other state of the
// vector goes into one batched call per feature count; a group whose fit failed (status != 0) is NULL, as upstream
void HipEnFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	const auto &opts = aggr_input_data.bind_data->Cast<HipElasticNetBindData>().opts;
	const idx_t max_features = anofox_hip_max_features();
	auto batches = CollectBatches<RowBatch>(state_vector, result, count, offset, [&](const RowBuffer &rows) {
		if (rows.Rows() < 2) return false;
		CheckMaxFeatures("elasticnet_fit_agg", rows.n_features, max_features); // (this aggregate checks the width of what it is about to fit)
		return true;
	});
	auto &entries = StructVector::GetEntries(result);
	const AnofoxHipElasticNetBatchOptions batch_opts = opts.Batch();
	for (auto &kv : batches) {
		const idx_t p = kv.first;
		auto &b = kv.second;
		const int64_t n = b.Stage(false, false); // (every buffered row trains)
		const size_t rec = anofox_hip_core_record_len(p);
		vector<double> core(b.Groups() * rec);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_elasticnet_fit_batch_host(nullptr, (int64_t)b.Groups(), p, n, b.offsets.data(), b.y.data(), b.col_ptrs.data(), batch_opts, core.data(),
		                                          nullptr, &err))
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

// Bind: the options argument is read when it folds to a constant (elasticnet_aggregate.cpp Bind)
unique_ptr<FunctionData> HipEnBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipElasticNetOptions>(context, function, arguments, 2, false, ParseHipElasticNetOptions,
	                                      [](const HipElasticNetOptions &) { return GetElasticNetResultType(); });
}

} // namespace

void RegisterHipElasticNetAggregateFunction(ExtensionLoader &loader) {
	const RowsFunctionNames f {"anofox_stats_elasticnet_fit_agg", "elasticnet_fit_agg", {},
	                           "Fits an Elastic Net regression model (L1 + L2) and returns coefficients and fit statistics as a struct.", {"regression"}};
	RegisterWithOptions(
	    loader, f, "{'alpha': 1.0, 'l1_ratio': 0.5}",
	    [](const string &fname, const vector<LogicalType> &args) {
		    return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsFitAggUpdate<EnFitAggTraits>, RowsCombine<false, true>, HipEnFinalize, HipEnBind);
	    },
	    true /* the overload with options is described first */);
}

} // namespace duckdb
