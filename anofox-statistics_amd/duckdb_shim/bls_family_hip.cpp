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
#include "row_glue.hpp"

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

struct HipBlsBindData : public FunctionData {
	HipBlsBindData(const HipBlsOptions &opts_p, bool use_split_col_p) : opts(opts_p), use_split_col(use_split_col_p) {}
	HipBlsOptions opts;
	bool use_split_col;
	unique_ptr<FunctionData> Copy() const override { return make_uniq<HipBlsBindData>(opts, use_split_col); }
	bool Equals(const FunctionData &other_p) const override {
		auto &other = other_p.Cast<HipBlsBindData>();
		return opts == other.opts && use_split_col == other.use_split_col;
	}
};

// the states of one Finalize vector as one batch per feature count (RowBatch) through the fit-predict call
struct BlsPredictBatch : RowBatch {
	vector<double> core, pred;
	void Run(const HipBlsOptions &opts) {
		const int64_t n = Stage(false, false);
		core.resize(Groups() * (p + 6));
		pred.resize((size_t)n * 3);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_bls_fit_predict_batch_host(nullptr, (int64_t)Groups(), p, n, offsets.data(), y.data(), col_ptrs.data(), train_counts.data(),
		                                           opts.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			ThrowAbi(err);
	}
	bool Failed(idx_t g) const { return core[g * (p + 6) + p + 5] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_bls_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Update (bls_fit_predict_aggregate.cpp:146-265): every row with a non-NULL x list is kept for the output; it trains iff y is not NULL (and the split column
// says train), and under null_policy = 'drop_y_zero_x' no feature is exactly 0.  A NULL list element is NaN: the row is handed
// to the fit, whose row filter drops it.
void HipBlsPredictAggUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<HipBlsBindData>();
	if (input_count < 2) throw InvalidInputException("anofox_stats bls_fit_predict_agg (HIP): too few arguments");
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
		CheckMaxFeatures("bls_fit_predict_agg", entry.length, max_features);
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

// Finalize (bls_fit_predict_aggregate.cpp:326-452): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with its prediction
void HipBlsPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipBlsBindData>();
	auto batches = CollectBatches<BlsPredictBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; });
	for (auto &kv : batches) kv.second.Run(bind.opts);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			if (b.Failed(g)) FlatVector::SetNull(result, b.result_rows[g], true);
			else AppendPredictRows(result, b.result_rows[g], *b.buffers[g], &b.pred[(size_t)b.offsets[g] * 3]);
		}
	}
}

template <bool SPLIT>
unique_ptr<FunctionData> HipBlsPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipBlsOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable())
		ParseHipBlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts, true, true);
	function.return_type = PredictAggResultType();
	return make_uniq<HipBlsBindData>(opts, SPLIT);
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

// Update (bls_aggregate.cpp:118-180): rows with a NULL y or a NULL x list are skipped; a NULL list element is NaN here (the
// reference reads the slot unchecked), so the fit's row filter drops the row
void HipBlsAggUpdate(Vector inputs[], AggregateInputData &, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 2) throw InvalidInputException("anofox_stats bls_fit_agg (HIP): too few arguments");
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
		auto y_idx = y_data.sel->get_index(i);
		if (!y_data.validity.RowIsValid(y_idx)) continue;
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		CheckMaxFeatures("bls_fit_agg", entry.length, max_features);
		auto &rows = RowsOf(state, entry.length, false);
		const size_t at = rows.x.size();
		rows.x.resize(at + entry.length);
		ReadListRow(entry, x_child_data, x_child_validity, rows.x.data() + at);
		rows.y.push_back(y_values[y_idx]);
		rows.flags.push_back(kTraining);
		rows.n_training++;
	}
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
unique_ptr<FunctionData> HipBlsAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipBlsOptions opts;
	if (arguments.size() > 2 && arguments[2]->IsFoldable()) ParseHipBlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), opts, !NNLS, false);
	function.return_type = GetHipBlsAggResultType();
	return make_uniq<HipBlsBindData>(opts, false);
}

template <bool NNLS>
void RegisterFit(ExtensionLoader &loader, const char *name, const char *alias, const char *what) {
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, GetHipBlsAggResultType(), AggregateFunction::StateSize<RowsState>, RowsInitialize,
			                                  HipBlsAggUpdate, RowsCombine<false>, HipBlsAggFinalize, nullptr, HipBlsAggBind<NNLS>, RowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic, kCategories));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'fit_intercept': true})", {"y", "x", "options"}, map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill(alias));
}

} // namespace

void RegisterHipBlsAggregateFunction(ExtensionLoader &loader) {
	RegisterFit<false>(loader, "anofox_stats_bls_fit_agg", "bls_fit_agg", "Fits a bounded least squares regression per group.");
}

void RegisterHipBlsNnlsAggregateFunction(ExtensionLoader &loader) {
	RegisterFit<true>(loader, "anofox_stats_nnls_fit_agg", "nnls_fit_agg", "Fits a non-negative least squares regression per group.");
}

void RegisterHipBlsFitPredictAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_bls_fit_predict_agg";
	const char *what = "Fits bounded least squares over a partition and returns per-row predictions with confidence intervals.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	const vector<LogicalType> split_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR};
	const vector<LogicalType> split_map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR, LogicalType::ANY};
	auto make = [](const string &fname, const vector<LogicalType> &args, bool split) {
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>, RowsInitialize,
		                         HipBlsPredictAggUpdate, RowsCombine<false>, HipBlsPredictAggFinalize, nullptr,
		                         split ? HipBlsPredictAggBind<true> : HipBlsPredictAggBind<false>, RowsDestroy);
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
	info.descriptions.push_back(Describe(what, head + ", {'lower_bound': 0.0})", {"y", "x", "options"}, map_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col)", {"y", "x", "split_col"}, split_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'upper_bound': 1.0})", {"y", "x", "split_col", "options"}, split_map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("bls_fit_predict_agg"));
}

} // namespace duckdb
