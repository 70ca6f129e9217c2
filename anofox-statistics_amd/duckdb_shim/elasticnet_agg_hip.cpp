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

namespace duckdb {

namespace {
using namespace hip_glue;

struct HipElasticNetBindData : public FunctionData {
	explicit HipElasticNetBindData(const HipElasticNetOptions &opts_p) : opts(opts_p) {}
	HipElasticNetOptions opts;
	unique_ptr<FunctionData> Copy() const override { return make_uniq<HipElasticNetBindData>(opts); }
	bool Equals(const FunctionData &other_p) const override { return opts == other_p.Cast<HipElasticNetBindData>().opts; }
};

// the rows Update accepted: y and one column per feature (a NULL list element is NaN, which the row filter drops)
struct EnRows {
	idx_t n_features = 0;
	vector<double> y;
	vector<vector<double>> x;
};
struct HipElasticNetState {
	EnRows *rows;
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

void HipEnInitialize(const AggregateFunction &, data_ptr_t state_p) { reinterpret_cast<HipElasticNetState *>(state_p)->rows = nullptr; }

void HipEnDestroy(Vector &state_vector, AggregateInputData &, idx_t count) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipElasticNetState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		delete state.rows;
		state.rows = nullptr;
	}
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
	auto states = (HipElasticNetState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		const auto y_idx = y_data.sel->get_index(i), x_idx = x_data.sel->get_index(i);
		if (!y_data.validity.RowIsValid(y_idx) || !x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		if (!state.rows) {
			state.rows = new EnRows();
			state.rows->n_features = entry.length;
			state.rows->x.resize(entry.length);
		}
		auto &r = *state.rows;
		if (entry.length != r.n_features)
			throw InvalidInputException("Inconsistent feature count: expected %llu, got %llu", (unsigned long long)r.n_features,
			                            (unsigned long long)entry.length);
		r.y.push_back(y_vals[y_idx]);
		for (idx_t j = 0; j < entry.length; j++) {
			const idx_t pos = entry.offset + j;
			r.x[j].push_back(x_child_validity.RowIsValid(pos) ? x_child_data[pos] : NAN);
		}
	}
}

void HipEnCombine(Vector &source_vector, Vector &target_vector, AggregateInputData &aggr_input_data, idx_t count) {
	UnifiedVectorFormat source_data, target_data;
	source_vector.ToUnifiedFormat(count, source_data);
	target_vector.ToUnifiedFormat(count, target_data);
	auto sources = (HipElasticNetState **)source_data.data;
	auto targets = (HipElasticNetState **)target_data.data;
	const bool preserve = aggr_input_data.combine_type == AggregateCombineType::PRESERVE_INPUT;
	for (idx_t i = 0; i < count; i++) {
		auto &source = *sources[source_data.sel->get_index(i)];
		auto &target = *targets[target_data.sel->get_index(i)];
		if (!source.rows || &source == &target) continue;
		if (!target.rows) {
			if (preserve) {
				target.rows = new EnRows(*source.rows);
			} else {
				target.rows = source.rows;
				source.rows = nullptr;
			}
			continue;
		}
		if (source.rows->n_features != target.rows->n_features)
			throw InvalidInputException("Cannot combine states with different feature counts: %llu vs %llu", (unsigned long long)source.rows->n_features,
			                            (unsigned long long)target.rows->n_features);
		target.rows->y.insert(target.rows->y.end(), source.rows->y.begin(), source.rows->y.end());
		for (idx_t j = 0; j < target.rows->n_features; j++)
			target.rows->x[j].insert(target.rows->x[j].end(), source.rows->x[j].begin(), source.rows->x[j].end());
	}
}

void AppendList(Vector &list_vec, idx_t row, const double *src, idx_t n) {
	auto entries = ListVector::GetData(list_vec);
	auto offset = ListVector::GetListSize(list_vec);
	ListVector::Reserve(list_vec, offset + n);
	auto child = FlatVector::GetData<double>(ListVector::GetEntry(list_vec));
	for (idx_t k = 0; k < n; k++) child[offset + k] = src[k];
	entries[row].offset = offset;
	entries[row].length = n;
	ListVector::SetListSize(list_vec, offset + n);
}

// Finalize: NULL without rows or with fewer than 2 (the reference's check before its FFI call); every other state of the
// vector goes into one batched call per feature count; a group whose fit failed (status != 0) is NULL, as upstream
void HipEnFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	const auto &opts = aggr_input_data.bind_data->Cast<HipElasticNetBindData>().opts;
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipElasticNetState **)sdata.data;
	struct Batch {
		vector<idx_t> result_rows;
		vector<EnRows *> rows;
	};
	std::map<idx_t, Batch> batches;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		if (!state.rows || state.rows->y.size() < 2 || state.rows->n_features == 0) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		if (state.rows->n_features > max_features)
			throw InvalidInputException("anofox_stats elasticnet_fit_agg (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)state.rows->n_features);
		auto &b = batches[state.rows->n_features];
		b.result_rows.push_back(i + offset);
		b.rows.push_back(state.rows);
	}
	auto &entries = StructVector::GetEntries(result);
	const AnofoxHipElasticNetBatchOptions batch_opts = opts.Batch();
	for (auto &kv : batches) {
		const idx_t p = kv.first;
		auto &b = kv.second;
		vector<int64_t> offsets {0};
		for (auto *r : b.rows) offsets.push_back(offsets.back() + (int64_t)r->y.size());
		const size_t n = (size_t)offsets.back();
		vector<double> y(n), cols(n * p);
		for (idx_t g = 0; g < b.rows.size(); g++) {
			std::copy(b.rows[g]->y.begin(), b.rows[g]->y.end(), y.begin() + offsets[g]);
			for (idx_t j = 0; j < p; j++) std::copy(b.rows[g]->x[j].begin(), b.rows[g]->x[j].end(), cols.begin() + j * n + (size_t)offsets[g]);
		}
		vector<const double *> col_ptrs(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * n;
		const size_t rec = anofox_hip_core_record_len(p);
		vector<double> core(b.rows.size() * rec);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_elasticnet_fit_batch_host(nullptr, (int64_t)b.rows.size(), p, (int64_t)n, offsets.data(), y.data(), col_ptrs.data(), batch_opts,
		                                          core.data(), nullptr, &err))
			throw InvalidInputException("anofox_stats (HIP): %s", err.message[0] ? err.message : "the batched call failed");
		for (idx_t g = 0; g < b.rows.size(); g++) {
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
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<HipElasticNetState>, HipEnInitialize,
		                         HipEnUpdate, HipEnCombine, HipEnFinalize, nullptr, HipEnBind, HipEnDestroy);
	};
	const char *name = "anofox_stats_elasticnet_fit_agg";
	const char *what = "Fits an Elastic Net regression model (L1 + L2) and returns coefficients and fit statistics as a struct.";
	AggregateFunctionSet func_set(name);
	func_set.AddFunction(make(name, basic_args));
	func_set.AddFunction(make(name, map_args));
	CreateAggregateFunctionInfo info(std::move(func_set));
	info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	FunctionDescription d1;
	d1.description = what;
	d1.examples = {string(name) + "(y, x, {'alpha': 1.0, 'l1_ratio': 0.5})"};
	d1.categories = {"regression"};
	d1.parameter_names = {"y", "x", "options"};
	d1.parameter_types = map_args;
	info.descriptions.push_back(std::move(d1));
	FunctionDescription d2;
	d2.description = what;
	d2.examples = {string(name) + "(y, x)"};
	d2.categories = {"regression"};
	d2.parameter_names = {"y", "x"};
	d2.parameter_types = basic_args;
	info.descriptions.push_back(std::move(d2));
	loader.RegisterFunction(std::move(info));
	AggregateFunctionSet alias_set("elasticnet_fit_agg");
	alias_set.AddFunction(make("elasticnet_fit_agg", basic_args));
	alias_set.AddFunction(make("elasticnet_fit_agg", map_args));
	CreateAggregateFunctionInfo alias_info(std::move(alias_set));
	alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	alias_info.alias_of = name;
	loader.RegisterFunction(std::move(alias_info));
}

} // namespace duckdb
