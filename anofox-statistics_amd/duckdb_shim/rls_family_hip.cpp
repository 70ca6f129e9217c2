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

namespace duckdb {

namespace {
using namespace hip_glue;

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

void ApplyRlsOption(const string &raw_key, const Value &v, HipRlsOptions &o) {
	if (v.IsNull()) return;
	const string key = Lower(raw_key);
	if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(v);
	else if (key == "forgetting_factor") o.forgetting_factor = v.GetValue<double>();
	else if (key == "initial_p_diagonal" || key == "p_diagonal") o.initial_p_diagonal = v.GetValue<double>();
	else if (key == "confidence_level" || key == "confidence") o.confidence_level = v.GetValue<double>();
	else if (key == "compute_inference" || key == "inference") (void)ExtractBool(v);
	else if (key == "null_policy") {
		const string s = Lower(v.type().id() == LogicalTypeId::VARCHAR ? StringValue::Get(v) : v.ToString());
		if (s == "drop") o.drop_y_zero_x = false;
		else if (s == "drop_y_zero_x") o.drop_y_zero_x = true;
		else throw InvalidInputException("Invalid null_policy: '%s'. Valid values are 'drop', 'drop_y_zero_x'", s.c_str());
	} else { // parsed by the shared parser, not read by RLS: only its conversion errors matter
		HipElasticNetOptions ignored;
		bool has_alpha = false, has_lambda = false;
		double alpha = 0.0, lambda = 0.0;
		ApplyElasticNetOption(raw_key, v, ignored, has_alpha, alpha, has_lambda, lambda);
	}
}

void ParseHipRlsOptions(const Value &v, HipRlsOptions &o) {
	if (v.IsNull()) return;
	if (v.type().id() == LogicalTypeId::STRUCT) {
		auto &kids = StructValue::GetChildren(v);
		for (idx_t i = 0; i < kids.size(); i++) ApplyRlsOption(StructType::GetChildName(v.type(), i), kids[i], o);
	} else if (v.type().id() == LogicalTypeId::MAP) {
		for (auto &entry : MapValue::GetChildren(v)) {
			auto &kv = StructValue::GetChildren(entry);
			if (kv.size() != 2 || kv[0].IsNull()) continue;
			ApplyRlsOption(kv[0].type().id() == LogicalTypeId::VARCHAR ? StringValue::Get(kv[0]) : kv[0].ToString(), kv[1], o);
		}
	} else {
		throw InvalidInputException("Options must be a MAP or STRUCT, got %s", v.type().ToString().c_str());
	}
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

// ---- the row buffer behind a DuckDB state (the layout of family_agg_hip.cpp's) ----
constexpr uint8_t kYNull = 1, kTraining = 2;
struct RlsRowBuffer {
	idx_t n_features = 0;
	vector<double> y;      // NaN where y was NULL
	vector<double> x;      // row-major; a NULL list element is NaN
	vector<uint8_t> flags; // kYNull | kTraining
	idx_t n_training = 0;
	vector<double> current_x; // the window aggregate: x of the last row Update saw
	bool has_current_x = false;
	idx_t Rows() const { return y.size(); }
};
struct HipRlsRowsState {
	RlsRowBuffer *rows;
};

void HipRlsRowsInitialize(const AggregateFunction &, data_ptr_t state_p) { reinterpret_cast<HipRlsRowsState *>(state_p)->rows = nullptr; }

void HipRlsRowsDestroy(Vector &state_vector, AggregateInputData &, idx_t count) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipRlsRowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		delete state.rows;
		state.rows = nullptr;
	}
}

RlsRowBuffer &RlsRows(HipRlsRowsState &state, idx_t n_features) {
	if (!state.rows) {
		state.rows = new RlsRowBuffer();
		state.rows->n_features = n_features;
	}
	if (state.rows->n_features != n_features) throw InvalidInputException("Inconsistent feature count"); // rls_predict_aggregate.cpp:190-192
	return *state.rows;
}

bool IsRlsSplitTraining(const string_t &split) { // IsSplitTraining: 'train' / 'training', any case
	string v = split.GetString();
	for (auto &c : v) c = (char)std::tolower((unsigned char)c);
	return v == "train" || v == "training";
}

template <bool WINDOW>
void HipRlsRowsCombine(Vector &source_vector, Vector &target_vector, AggregateInputData &aggr_input_data, idx_t count) {
	UnifiedVectorFormat source_data, target_data;
	source_vector.ToUnifiedFormat(count, source_data);
	target_vector.ToUnifiedFormat(count, target_data);
	auto sources = (HipRlsRowsState **)source_data.data;
	auto targets = (HipRlsRowsState **)target_data.data;
	const bool preserve = aggr_input_data.combine_type == AggregateCombineType::PRESERVE_INPUT;
	for (idx_t i = 0; i < count; i++) {
		auto &source = *sources[source_data.sel->get_index(i)];
		auto &target = *targets[target_data.sel->get_index(i)];
		if (!source.rows || &source == &target) continue;
		if (!target.rows) {
			if (preserve) {
				target.rows = new RlsRowBuffer(*source.rows);
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
		if (WINDOW && s.has_current_x) { // the later state's row is the frame's last (rls_fit_predict.cpp:224-227)
			t.current_x = s.current_x;
			t.has_current_x = true;
		}
	}
}

// the states of one Finalize vector as one batch per feature count
struct RlsBatch {
	idx_t p = 0;
	vector<idx_t> result_rows;
	vector<RlsRowBuffer *> buffers;
	vector<int64_t> offsets {0};
	vector<int64_t> train_counts;
	vector<double> y, cols, core, pred;
	void Run(const HipRlsOptions &opts, bool extra_row) {
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
		if (!anofox_hip_rls_fit_predict_batch_host(nullptr, (int64_t)buffers.size(), p, n, offsets.data(), y.data(), col_ptrs.data(),
		                                           train_counts.data(), opts.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			throw InvalidInputException("anofox_stats (HIP): %s", err.message[0] ? err.message : "the batched call failed");
	}
	bool Failed(idx_t g) const { return core[g * (p + 6) + p + 5] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_rls_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
LogicalType GetHipRlsPredictAggResultType() { // rls_predict_aggregate.cpp:94-106
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
	auto states = (HipRlsRowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		if (entry.length > max_features)
			throw InvalidInputException("anofox_stats rls_fit_predict_agg (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)entry.length);
		auto &rows = RlsRows(state, entry.length);
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
			training = split_data.validity.RowIsValid(s_idx) && IsRlsSplitTraining(split_values[s_idx]) && y_valid;
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
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipRlsRowsState **)sdata.data;
	std::map<idx_t, RlsBatch> batches;
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
			const RlsRowBuffer &rows = *b.buffers[g];
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
unique_ptr<FunctionData> HipRlsPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipRlsOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable())
		ParseHipRlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts);
	function.return_type = GetHipRlsPredictAggResultType();
	return make_uniq<HipRlsFamilyBindData>(opts, SPLIT);
}

// =====================================================================================================================
// anofox_stats_rls_fit_predict(y, x[, options]) OVER (...) -> STRUCT(yhat, yhat_lower, yhat_upper)
// =====================================================================================================================
LogicalType GetHipRlsFitPredictResultType() {
	child_list_t<LogicalType> children;
	children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	children.push_back(make_pair("yhat_lower", LogicalType::DOUBLE));
	children.push_back(make_pair("yhat_upper", LogicalType::DOUBLE));
	return LogicalType::STRUCT(std::move(children));
}

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
	auto states = (HipRlsRowsState **)sdata.data;
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
			throw InvalidInputException("anofox_stats rls_fit_predict (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)entry.length);
		auto &rows = RlsRows(state, entry.length);
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
void HipRlsFitPredictFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipRlsRowsState **)sdata.data;
	std::map<idx_t, RlsBatch> batches;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		if (!state.rows || !state.rows->has_current_x || state.rows->n_features == 0) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		const idx_t min_obs = state.rows->n_features + (bind.opts.fit_intercept ? 1 : 0);
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

unique_ptr<FunctionData> HipRlsFitPredictBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipRlsOptions opts;
	if (arguments.size() > 2 && arguments[2]->IsFoldable()) ParseHipRlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), opts);
	function.return_type = GetHipRlsFitPredictResultType();
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
	auto states = (HipRlsRowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i), y_idx = y_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx) || !y_data.validity.RowIsValid(y_idx)) continue;
		const auto entry = x_list[x_idx];
		if (entry.length > max_features)
			throw InvalidInputException("anofox_stats rls_fit_agg (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)entry.length);
		auto &rows = RlsRows(state, entry.length);
		for (idx_t j = 0; j < entry.length; j++) {
			const idx_t pos = entry.offset + j;
			rows.x.push_back(x_child_validity.RowIsValid(pos) ? x_child_data[pos] : NAN);
		}
		rows.y.push_back(y_values[y_idx]);
		rows.flags.push_back(kTraining);
		rows.n_training++;
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

// Finalize: NULL with fewer than 2 rows or a failed fit; the vector's other states in ONE batched call per feature count
void HipRlsFitAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipRlsFamilyBindData>();
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipRlsRowsState **)sdata.data;
	struct Batch {
		vector<idx_t> result_rows;
		vector<RlsRowBuffer *> rows;
	};
	std::map<idx_t, Batch> batches;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		if (!state.rows || state.rows->Rows() < 2 || state.rows->n_features == 0) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		auto &b = batches[state.rows->n_features];
		b.result_rows.push_back(i + offset);
		b.rows.push_back(state.rows);
	}
	auto &entries = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		const idx_t p = kv.first;
		auto &b = kv.second;
		vector<int64_t> offsets {0};
		for (auto *r : b.rows) offsets.push_back(offsets.back() + (int64_t)r->Rows());
		const size_t n = (size_t)offsets.back();
		vector<double> y(n), cols(n * p);
		for (idx_t g = 0; g < b.rows.size(); g++) {
			const RlsRowBuffer &r = *b.rows[g];
			for (idx_t row = 0; row < r.Rows(); row++) {
				y[(size_t)offsets[g] + row] = r.y[row];
				for (idx_t j = 0; j < p; j++) cols[j * n + (size_t)offsets[g] + row] = r.x[row * p + j];
			}
		}
		vector<const double *> col_ptrs(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * n;
		const size_t rec = anofox_hip_core_record_len(p);
		vector<double> core(b.rows.size() * rec);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_rls_fit_batch_host(nullptr, (int64_t)b.rows.size(), p, (int64_t)n, offsets.data(), y.data(), col_ptrs.data(), bind.opts.Batch(),
		                                   core.data(), &err))
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

unique_ptr<FunctionData> HipRlsFitAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipRlsOptions opts;
	if (arguments.size() > 2 && arguments[2]->IsFoldable()) ParseHipRlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), opts);
	function.return_type = GetHipRlsFitAggResultType();
	return make_uniq<HipRlsFamilyBindData>(opts, false);
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

void RegisterHipRlsAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_rls_fit_agg";
	const char *what = "Fits a Recursive Least Squares model over the group's rows in order and returns coefficients as a struct.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<HipRlsRowsState>,
			                                  HipRlsRowsInitialize, HipRlsFitAggUpdate, HipRlsRowsCombine<false>, HipRlsFitAggFinalize, nullptr,
			                                  HipRlsFitAggBind, HipRlsRowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'forgetting_factor': 0.99})", {"y", "x", "options"}, map_args));
	loader.RegisterFunction(std::move(info));
	CreateAggregateFunctionInfo alias_info(fill("rls_fit_agg"));
	alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	alias_info.alias_of = name;
	loader.RegisterFunction(std::move(alias_info));
}

void RegisterHipRlsFitPredictAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_rls_fit_predict_agg";
	const char *what = "Fits Recursive Least Squares over a partition and returns per-row predictions.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	const vector<LogicalType> split_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR};
	const vector<LogicalType> split_map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR, LogicalType::ANY};
	auto make = [](const string &fname, const vector<LogicalType> &args, bool split) {
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<HipRlsRowsState>, HipRlsRowsInitialize,
		                         HipRlsPredictAggUpdate, HipRlsRowsCombine<false>, HipRlsPredictAggFinalize, nullptr,
		                         split ? HipRlsPredictAggBind<true> : HipRlsPredictAggBind<false>, HipRlsRowsDestroy);
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
	info.descriptions.push_back(Describe(what, head + ", {'forgetting_factor': 0.99})", {"y", "x", "options"}, map_args));
	info.descriptions.push_back(Describe(what, head + ", split_col)", {"y", "x", "split_col"}, split_args));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'forgetting_factor': 0.99})", {"y", "x", "split_col", "options"}, split_map_args));
	loader.RegisterFunction(std::move(info));
	for (const char *alias : {"rls_fit_predict_agg", "rls_predict_agg", "anofox_stats_rls_predict_agg"}) {
		CreateAggregateFunctionInfo alias_info(fill(alias));
		alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
		alias_info.alias_of = name;
		loader.RegisterFunction(std::move(alias_info));
	}
}

void RegisterHipRlsFitPredictFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_rls_fit_predict";
	const char *what = "Fits a Recursive Least Squares model over a window partition and returns predictions.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, GetHipRlsFitPredictResultType(), AggregateFunction::StateSize<HipRlsRowsState>, HipRlsRowsInitialize,
			                                  HipRlsFitPredictUpdate, HipRlsRowsCombine<true>, HipRlsFitPredictFinalize, nullptr, HipRlsFitPredictBind,
			                                  HipRlsRowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'null_policy': 'drop'})", {"y", "x", "options"}, map_args));
	loader.RegisterFunction(std::move(info));
	CreateAggregateFunctionInfo alias_info(fill("rls_fit_predict"));
	alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	alias_info.alias_of = name;
	loader.RegisterFunction(std::move(alias_info));
}

} // namespace duckdb
