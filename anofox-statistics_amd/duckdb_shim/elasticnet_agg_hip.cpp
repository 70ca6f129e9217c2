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
#include "row_glue.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

struct HipElasticNetBindData : public FunctionData {
	explicit HipElasticNetBindData(const HipElasticNetOptions &opts_p) : opts(opts_p) {}
	HipElasticNetOptions opts;
	unique_ptr<FunctionData> Copy() const override { return make_uniq<HipElasticNetBindData>(opts); }
	bool Equals(const FunctionData &other_p) const override { return opts == other_p.Cast<HipElasticNetBindData>().opts; }
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

// Update (elasticnet_aggregate.cpp Update): rows with a NULL y or a NULL x list are skipped; the feature count is fixed by
// the first accepted row
void HipEnUpdate(Vector inputs[], AggregateInputData &, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 2) throw InvalidInputException("anofox_stats elasticnet_fit_agg (HIP): too few arguments");
	UnifiedVectorFormat y_data, x_data, sdata;
	inputs[0].ToUnifiedFormat(count, y_data);
	inputs[1].ToUnifiedFormat(count, x_data);
	auto y_vals = UnifiedVectorFormat::GetData<double>(y_data);
	auto x_list = UnifiedVectorFormat::GetData<list_entry_t>(x_data);
	auto &x_child = ListVector::GetEntry(inputs[1]);
	auto x_child_data = FlatVector::GetData<double>(x_child);
	auto &x_child_validity = FlatVector::Validity(x_child);
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (RowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		const auto y_idx = y_data.sel->get_index(i), x_idx = x_data.sel->get_index(i);
		if (!y_data.validity.RowIsValid(y_idx) || !x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		auto &rows = RowsOf(state, entry.length, true);
		const size_t at = rows.x.size();
		rows.x.resize(at + entry.length);
		ReadListRow(entry, x_child_data, x_child_validity, rows.x.data() + at); // (a NULL list element is NaN, which the row filter drops)
		rows.y.push_back(y_vals[y_idx]);
		rows.flags.push_back(kTraining);
		rows.n_training++;
	}
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
	HipElasticNetOptions opts;
	if (arguments.size() >= 3 && arguments[2]->IsFoldable()) ParseHipElasticNetOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), opts);
	function.return_type = GetElasticNetResultType();
	return make_uniq<HipElasticNetBindData>(opts);
}

} // namespace

void RegisterHipElasticNetAggregateFunction(ExtensionLoader &loader) {
	const vector<LogicalType> basic_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto make = [](const string &fname, const vector<LogicalType> &args) {
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>, RowsInitialize, HipEnUpdate,
		                         RowsCombine<false, true>, HipEnFinalize, nullptr, HipEnBind, RowsDestroy);
	};
	const char *name = "anofox_stats_elasticnet_fit_agg";
	const char *what = "Fits an Elastic Net regression model (L1 + L2) and returns coefficients and fit statistics as a struct.";
	AggregateFunctionSet func_set(name);
	func_set.AddFunction(make(name, basic_args));
	func_set.AddFunction(make(name, map_args));
	CreateAggregateFunctionInfo info(std::move(func_set));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'alpha': 1.0, 'l1_ratio': 0.5})", {"y", "x", "options"}, map_args, {"regression"}));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic_args, {"regression"}));
	AggregateFunctionSet alias_set("elasticnet_fit_agg");
	alias_set.AddFunction(make("elasticnet_fit_agg", basic_args));
	alias_set.AddFunction(make("elasticnet_fit_agg", map_args));
	RegisterWithAlias(loader, std::move(info), std::move(alias_set));
}

} // namespace duckdb
