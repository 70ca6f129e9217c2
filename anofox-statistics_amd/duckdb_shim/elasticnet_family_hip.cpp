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

namespace duckdb {

namespace {
using namespace hip_glue;

// ---- options: the elastic net's plus the interval's confidence level and the null policy ----
struct HipEnPredictOptions {
	HipElasticNetOptions en;
	double confidence_level = 0.95;
	bool drop_y_zero_x = false;
	bool operator==(const HipEnPredictOptions &o) const {
		return en == o.en && confidence_level == o.confidence_level && drop_y_zero_x == o.drop_y_zero_x;
	}
};

void ApplyEnPredictOption(const string &raw_key, const Value &v, HipEnPredictOptions &o, bool &has_alpha, double &alpha, bool &has_lambda, double &lambda) {
	if (v.IsNull()) return;
	const string key = Lower(raw_key);
	if (key == "confidence_level" || key == "confidence") o.confidence_level = v.GetValue<double>();
	else if (key == "null_policy") {
		const string s = Lower(v.type().id() == LogicalTypeId::VARCHAR ? StringValue::Get(v) : v.ToString());
		if (s == "drop") o.drop_y_zero_x = false;
		else if (s == "drop_y_zero_x") o.drop_y_zero_x = true;
		else throw InvalidInputException("Invalid null_policy: '%s'. Valid values are 'drop', 'drop_y_zero_x'", s.c_str());
	} else ApplyElasticNetOption(raw_key, v, o.en, has_alpha, alpha, has_lambda, lambda);
}

// use_lambda = false: the aggregate's bind (alpha only); true: the window function's (alpha, else lambda)
void ParseHipEnPredictOptions(const Value &v, HipEnPredictOptions &o, bool use_lambda) {
	if (v.IsNull()) return;
	bool has_alpha = false, has_lambda = false;
	double alpha = 0.0, lambda = 0.0;
	if (v.type().id() == LogicalTypeId::STRUCT) {
		auto &kids = StructValue::GetChildren(v);
		for (idx_t i = 0; i < kids.size(); i++) ApplyEnPredictOption(StructType::GetChildName(v.type(), i), kids[i], o, has_alpha, alpha, has_lambda, lambda);
	} else if (v.type().id() == LogicalTypeId::MAP) {
		for (auto &entry : MapValue::GetChildren(v)) {
			auto &kv = StructValue::GetChildren(entry);
			if (kv.size() != 2 || kv[0].IsNull()) continue;
			ApplyEnPredictOption(kv[0].type().id() == LogicalTypeId::VARCHAR ? StringValue::Get(kv[0]) : kv[0].ToString(), kv[1], o, has_alpha, alpha,
			                     has_lambda, lambda);
		}
	} else {
		throw InvalidInputException("Options must be a MAP or STRUCT, got %s", v.type().ToString().c_str());
	}
	if (has_alpha) o.en.alpha = alpha;
	else if (has_lambda && use_lambda) o.en.alpha = lambda;
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

// ---- the row buffer behind a DuckDB state (the layout of family_agg_hip.cpp's) ----
constexpr uint8_t kYNull = 1, kTraining = 2;
struct EnRowBuffer {
	idx_t n_features = 0;
	vector<double> y;      // NaN where y was NULL
	vector<double> x;      // row-major; a NULL list element is NaN
	vector<uint8_t> flags; // kYNull | kTraining
	idx_t n_training = 0;
	vector<double> current_x; // the window aggregate: x of the last row Update saw
	bool has_current_x = false;
	idx_t Rows() const { return y.size(); }
};
struct HipEnRowsState {
	EnRowBuffer *rows;
};

void HipEnRowsInitialize(const AggregateFunction &, data_ptr_t state_p) { reinterpret_cast<HipEnRowsState *>(state_p)->rows = nullptr; }

void HipEnRowsDestroy(Vector &state_vector, AggregateInputData &, idx_t count) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipEnRowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		delete state.rows;
		state.rows = nullptr;
	}
}

EnRowBuffer &EnRows(HipEnRowsState &state, idx_t n_features) {
	if (!state.rows) {
		state.rows = new EnRowBuffer();
		state.rows->n_features = n_features;
	}
	if (state.rows->n_features != n_features) throw InvalidInputException("Inconsistent feature count"); // elasticnet_predict_aggregate.cpp:190-192
	return *state.rows;
}

bool IsEnSplitTraining(const string_t &split) { // ElasticNetIsSplitTraining: 'train' / 'training', any case
	string v = split.GetString();
	for (auto &c : v) c = (char)std::tolower((unsigned char)c);
	return v == "train" || v == "training";
}

template <bool WINDOW>
void HipEnRowsCombine(Vector &source_vector, Vector &target_vector, AggregateInputData &aggr_input_data, idx_t count) {
	UnifiedVectorFormat source_data, target_data;
	source_vector.ToUnifiedFormat(count, source_data);
	target_vector.ToUnifiedFormat(count, target_data);
	auto sources = (HipEnRowsState **)source_data.data;
	auto targets = (HipEnRowsState **)target_data.data;
	const bool preserve = aggr_input_data.combine_type == AggregateCombineType::PRESERVE_INPUT;
	for (idx_t i = 0; i < count; i++) {
		auto &source = *sources[source_data.sel->get_index(i)];
		auto &target = *targets[target_data.sel->get_index(i)];
		if (!source.rows || &source == &target) continue;
		if (!target.rows) {
			if (preserve) {
				target.rows = new EnRowBuffer(*source.rows);
			} else {
				target.rows = source.rows;
				source.rows = nullptr;
			}
			continue;
		}
		if (source.rows->n_features != target.rows->n_features) throw InvalidInputException("Cannot combine states with different feature counts");
		auto &t = *target.rows;
		const auto &s = *source.rows;
		t.y.insert(t.y.end(), s.y.begin(), s.y.end());
		t.x.insert(t.x.end(), s.x.begin(), s.x.end());
		t.flags.insert(t.flags.end(), s.flags.begin(), s.flags.end());
		t.n_training += s.n_training;
		if (WINDOW && s.has_current_x) { // the later state's row is the frame's last (elasticnet_fit_predict.cpp:224-227)
			t.current_x = s.current_x;
			t.has_current_x = true;
		}
	}
}

// the states of one Finalize vector as one batch per feature count
struct EnBatch {
	idx_t p = 0;
	vector<idx_t> result_rows;
	vector<EnRowBuffer *> buffers;
	vector<int64_t> offsets {0};
	vector<int64_t> train_counts;
	vector<double> y, cols, core, pred;
	void Run(const HipEnPredictOptions &opts, bool extra_row) {
		int64_t n = 0;
		for (auto *b : buffers) {
			n += (int64_t)b->Rows() + (extra_row ? 1 : 0);
			offsets.push_back(n);
			train_counts.push_back((int64_t)b->n_training);
		}
		y.resize((size_t)n);
		cols.resize((size_t)n * p);
		int64_t at = 0;
		for (auto *b : buffers) {
			const idx_t rows = b->Rows();
			for (idx_t r = 0; r < rows; r++) {
				y[at + r] = (b->flags[r] & kTraining) ? b->y[r] : NAN;
				for (idx_t j = 0; j < p; j++) cols[j * (size_t)n + at + r] = b->x[r * p + j];
			}
			at += (int64_t)rows;
			if (extra_row) {
				y[at] = NAN;
				for (idx_t j = 0; j < p; j++) cols[j * (size_t)n + at] = b->current_x[j];
				at++;
			}
		}
		vector<const double *> col_ptrs(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * (size_t)n;
		core.resize(buffers.size() * (p + 6));
		pred.resize((size_t)n * 3);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_elasticnet_fit_predict_batch_host(nullptr, (int64_t)buffers.size(), p, n, offsets.data(), y.data(), col_ptrs.data(),
		                                                  train_counts.data(), opts.en.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			throw InvalidInputException("anofox_stats (HIP): %s", err.message[0] ? err.message : "the batched call failed");
	}
	bool Failed(idx_t g) const { return core[g * (p + 6) + p + 5] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_elasticnet_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
LogicalType GetHipEnPredictAggResultType() { // elasticnet_predict_aggregate.cpp:94-106
	child_list_t<LogicalType> row_children;
	row_children.push_back(make_pair("y", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat_lower", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat_upper", LogicalType::DOUBLE));
	row_children.push_back(make_pair("is_training", LogicalType::BOOLEAN));
	return LogicalType::LIST(LogicalType::STRUCT(std::move(row_children)));
}

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
	auto states = (HipEnRowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		if (entry.length > max_features)
			throw InvalidInputException("anofox_stats elasticnet_fit_predict_agg (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)entry.length);
		auto &rows = EnRows(state, entry.length);
		bool has_zero = false;
		const size_t at = rows.x.size();
		rows.x.resize(at + entry.length);
		for (idx_t j = 0; j < entry.length; j++) {
			const idx_t pos = entry.offset + j;
			rows.x[at + j] = x_child_validity.RowIsValid(pos) ? x_child_data[pos] : NAN; // never read the slot of a NULL
			has_zero = has_zero || rows.x[at + j] == 0.0;
		}
		auto y_idx = y_data.sel->get_index(i);
		const bool y_valid = y_data.validity.RowIsValid(y_idx);
		bool training = y_valid;
		if (bind.use_split_col && split_values) {
			auto s_idx = split_data.sel->get_index(i);
			training = split_data.validity.RowIsValid(s_idx) && IsEnSplitTraining(split_values[s_idx]) && y_valid;
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
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipEnRowsState **)sdata.data;
	std::map<idx_t, EnBatch> batches;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		if (!state.rows || state.rows->n_training < 2 || state.rows->n_features == 0) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		auto &b = batches[state.rows->n_features];
		b.p = state.rows->n_features;
		b.result_rows.push_back(i + offset);
		b.buffers.push_back(state.rows);
	}
	for (auto &kv : batches) kv.second.Run(bind.opts, false);
	auto list_data = ListVector::GetData(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.buffers.size(); g++) {
			const idx_t r = b.result_rows[g];
			if (b.Failed(g)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const EnRowBuffer &rows = *b.buffers[g];
			const idx_t n_rows = rows.Rows();
			const idx_t list_offset = ListVector::GetListSize(result);
			ListVector::Reserve(result, list_offset + n_rows);
			ListVector::SetListSize(result, list_offset + n_rows);
			list_data[r].offset = list_offset;
			list_data[r].length = n_rows;
			auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
			const double *pred = &b.pred[(size_t)b.offsets[g] * 3];
			for (idx_t row = 0; row < n_rows; row++) {
				const idx_t at = list_offset + row;
				if (rows.flags[row] & kYNull) FlatVector::SetNull(*fields[0], at, true);
				else FlatVector::GetData<double>(*fields[0])[at] = rows.y[row];
				if (isfinite(pred[row * 3])) {
					for (idx_t k = 0; k < 3; k++) FlatVector::GetData<double>(*fields[1 + k])[at] = pred[row * 3 + k];
				} else {
					for (idx_t k = 0; k < 3; k++) FlatVector::SetNull(*fields[1 + k], at, true);
				}
				FlatVector::GetData<bool>(*fields[4])[at] = (rows.flags[row] & kTraining) != 0;
			}
		}
	}
}

template <bool SPLIT>
unique_ptr<FunctionData> HipEnPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipEnPredictOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable())
		ParseHipEnPredictOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts, false);
	function.return_type = GetHipEnPredictAggResultType();
	return make_uniq<HipEnFamilyBindData>(opts, SPLIT);
}

// =====================================================================================================================
// anofox_stats_elasticnet_fit_predict(y, x[, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// =====================================================================================================================
LogicalType GetHipEnFitPredictResultType() {
	child_list_t<LogicalType> children;
	children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	children.push_back(make_pair("yhat_lower", LogicalType::DOUBLE));
	children.push_back(make_pair("yhat_upper", LogicalType::DOUBLE));
	return LogicalType::STRUCT(std::move(children));
}

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
	auto states = (HipEnRowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) {
			if (state.rows) state.rows->has_current_x = false; // :134-137
			continue;
		}
		const auto entry = x_list[x_idx];
		if (entry.length > max_features)
			throw InvalidInputException("anofox_stats elasticnet_fit_predict (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)entry.length);
		auto &rows = EnRows(state, entry.length);
		rows.current_x.resize(entry.length);
		bool has_zero = false;
		for (idx_t j = 0; j < entry.length; j++) {
			const idx_t pos = entry.offset + j;
			rows.current_x[j] = x_child_validity.RowIsValid(pos) ? x_child_data[pos] : NAN;
			has_zero = has_zero || rows.current_x[j] == 0.0;
		}
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
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipEnRowsState **)sdata.data;
	std::map<idx_t, EnBatch> batches;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		if (!state.rows || !state.rows->has_current_x || state.rows->n_features == 0) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		const idx_t min_obs = state.rows->n_features + (bind.opts.en.fit_intercept ? 1 : 0);
		if (state.rows->n_training <= min_obs) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		auto &b = batches[state.rows->n_features];
		b.p = state.rows->n_features;
		b.result_rows.push_back(i + offset);
		b.buffers.push_back(state.rows);
	}
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
	function.return_type = GetHipEnFitPredictResultType();
	return make_uniq<HipEnFamilyBindData>(opts, false);
}

FunctionDescription Describe(const char *what, const string &example, vector<string> names, const vector<LogicalType> &types) {
	FunctionDescription d;
	d.description = what;
	d.examples = {example};
	d.categories = {"regression", "prediction"};
	d.parameter_names = std::move(names);
	d.parameter_types = types;
	return d;
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
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<HipEnRowsState>, HipEnRowsInitialize,
		                         HipEnPredictAggUpdate, HipEnRowsCombine<false>, HipEnPredictAggFinalize, nullptr,
		                         split ? HipEnPredictAggBind<true> : HipEnPredictAggBind<false>, HipEnRowsDestroy);
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
	info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	const string head = string(name) + "(y, x";
	info.descriptions.push_back(Describe(what, head + ")", {"y", "x"}, basic));
	info.descriptions.push_back(Describe(what, head + ", {'alpha': 1.0, 'l1_ratio': 0.5})", {"y", "x", "options"}, map_args));
	info.descriptions.push_back(Describe(what, head + ", split_col)", {"y", "x", "split_col"}, split_args));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'alpha': 1.0})", {"y", "x", "split_col", "options"}, split_map_args));
	loader.RegisterFunction(std::move(info));
	for (const char *alias : {"elasticnet_fit_predict_agg", "elasticnet_predict_agg", "anofox_stats_elasticnet_predict_agg"}) {
		CreateAggregateFunctionInfo alias_info(fill(alias));
		alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
		alias_info.alias_of = name;
		loader.RegisterFunction(std::move(alias_info));
	}
}

void RegisterHipElasticNetFitPredictFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_elasticnet_fit_predict";
	const char *what = "Fits an ElasticNet regression model over a window partition and returns predictions with confidence intervals.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, GetHipEnFitPredictResultType(), AggregateFunction::StateSize<HipEnRowsState>, HipEnRowsInitialize,
			                                  HipEnFitPredictUpdate, HipEnRowsCombine<true>, HipEnFitPredictFinalize, nullptr, HipEnFitPredictBind,
			                                  HipEnRowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'null_policy': 'drop'})", {"y", "x", "options"}, map_args));
	loader.RegisterFunction(std::move(info));
	CreateAggregateFunctionInfo alias_info(fill("elasticnet_fit_predict"));
	alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	alias_info.alias_of = name;
	loader.RegisterFunction(std::move(alias_info));
}

} // namespace duckdb
