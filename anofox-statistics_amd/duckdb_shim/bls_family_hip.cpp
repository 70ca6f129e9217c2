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

namespace duckdb {

namespace {
using namespace hip_glue;

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

// bounds = false: nnls_fit_agg's bind; predict = true: the fit-predict aggregate's
void ApplyBlsOption(const string &raw_key, const Value &v, HipBlsOptions &o, bool bounds, bool predict) {
	if (v.IsNull()) return;
	const string key = Lower(raw_key);
	if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(v);
	else if (key == "max_iterations" || key == "max_iter") {
		const double it = v.GetValue<double>();
		if (!(it >= 0.0 && it <= 4294967295.0)) throw InvalidInputException("Value %s is out of range for UINTEGER", v.ToString().c_str());
		o.max_iterations = (uint32_t)it;
	} else if (key == "tolerance" || key == "tol") o.tolerance = v.GetValue<double>();
	else if (key == "lower_bound" || key == "lower") {
		const double b = v.GetValue<double>(); // (parsed by the shared parser whoever reads it)
		if (bounds) { o.lower = b; o.has_lower = true; }
	} else if (key == "upper_bound" || key == "upper") {
		const double b = v.GetValue<double>();
		if (bounds) { o.upper = b; o.has_upper = true; }
	} else if (key == "confidence_level" || key == "confidence") {
		const double c = v.GetValue<double>();
		if (predict) o.confidence_level = c;
	} else if (key == "null_policy") {
		const string s = Lower(v.type().id() == LogicalTypeId::VARCHAR ? StringValue::Get(v) : v.ToString());
		if (s != "drop" && s != "drop_y_zero_x") throw InvalidInputException("Invalid null_policy: '%s'. Valid values are 'drop', 'drop_y_zero_x'", s.c_str());
		if (predict) o.drop_y_zero_x = s == "drop_y_zero_x";
	}
	// every other key: ignored, as in the reference
}

void ParseHipBlsOptions(const Value &v, HipBlsOptions &o, bool bounds, bool predict) {
	if (v.IsNull()) return;
	if (v.type().id() == LogicalTypeId::STRUCT) {
		auto &kids = StructValue::GetChildren(v);
		for (idx_t i = 0; i < kids.size(); i++) ApplyBlsOption(StructType::GetChildName(v.type(), i), kids[i], o, bounds, predict);
	} else if (v.type().id() == LogicalTypeId::MAP) {
		for (auto &entry : MapValue::GetChildren(v)) {
			auto &kv = StructValue::GetChildren(entry);
			if (kv.size() != 2 || kv[0].IsNull()) continue;
			ApplyBlsOption(kv[0].type().id() == LogicalTypeId::VARCHAR ? StringValue::Get(kv[0]) : kv[0].ToString(), kv[1], o, bounds, predict);
		}
	} else {
		throw InvalidInputException("Options must be a MAP or STRUCT, got %s", v.type().ToString().c_str());
	}
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

// ---- the row buffer behind a DuckDB state (the layout of family_agg_hip.cpp's) ----
constexpr uint8_t kYNull = 1, kTraining = 2;
struct BlsRowBuffer {
	idx_t n_features = 0;
	vector<double> y;      // NaN where y was NULL
	vector<double> x;      // row-major; a NULL list element is NaN
	vector<uint8_t> flags; // kYNull | kTraining
	idx_t n_training = 0;
	idx_t Rows() const { return y.size(); }
};
struct HipBlsRowsState {
	BlsRowBuffer *rows;
};

void HipBlsRowsInitialize(const AggregateFunction &, data_ptr_t state_p) { reinterpret_cast<HipBlsRowsState *>(state_p)->rows = nullptr; }

void HipBlsRowsDestroy(Vector &state_vector, AggregateInputData &, idx_t count) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipBlsRowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		delete state.rows;
		state.rows = nullptr;
	}
}

BlsRowBuffer &BlsRows(HipBlsRowsState &state, idx_t n_features) {
	if (!state.rows) {
		state.rows = new BlsRowBuffer();
		state.rows->n_features = n_features;
	}
	if (state.rows->n_features != n_features) throw InvalidInputException("Inconsistent feature count"); // bls_fit_predict_aggregate.cpp:204-207
	return *state.rows;
}

bool IsBlsSplitTraining(const string_t &split) { // BlsIsSplitTraining: 'train' / 'training', any case
	string v = split.GetString();
	for (auto &c : v) c = (char)std::tolower((unsigned char)c);
	return v == "train" || v == "training";
}

void HipBlsRowsCombine(Vector &source_vector, Vector &target_vector, AggregateInputData &aggr_input_data, idx_t count) {
	UnifiedVectorFormat source_data, target_data;
	source_vector.ToUnifiedFormat(count, source_data);
	target_vector.ToUnifiedFormat(count, target_data);
	auto sources = (HipBlsRowsState **)source_data.data;
	auto targets = (HipBlsRowsState **)target_data.data;
	const bool preserve = aggr_input_data.combine_type == AggregateCombineType::PRESERVE_INPUT;
	for (idx_t i = 0; i < count; i++) {
		auto &source = *sources[source_data.sel->get_index(i)];
		auto &target = *targets[target_data.sel->get_index(i)];
		if (!source.rows || &source == &target) continue;
		if (!target.rows) {
			if (preserve) {
				target.rows = new BlsRowBuffer(*source.rows);
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
	}
}

// the states of one Finalize vector as one batch per feature count
struct BlsPredictBatch {
	idx_t p = 0;
	vector<idx_t> result_rows;
	vector<BlsRowBuffer *> buffers;
	vector<int64_t> offsets {0};
	vector<int64_t> train_counts;
	vector<double> y, cols, core, pred;
	void Run(const HipBlsOptions &opts) {
		int64_t n = 0;
		for (auto *b : buffers) {
			n += (int64_t)b->Rows();
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
		}
		vector<const double *> col_ptrs(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * (size_t)n;
		core.resize(buffers.size() * (p + 6));
		pred.resize((size_t)n * 3);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_bls_fit_predict_batch_host(nullptr, (int64_t)buffers.size(), p, n, offsets.data(), y.data(), col_ptrs.data(),
		                                           train_counts.data(), opts.Batch(), opts.confidence_level, core.data(), pred.data(), &err))
			throw InvalidInputException("anofox_stats (HIP): %s", err.message[0] ? err.message : "the batched call failed");
	}
	bool Failed(idx_t g) const { return core[g * (p + 6) + p + 5] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_bls_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
LogicalType GetHipBlsPredictAggResultType() { // bls_fit_predict_aggregate.cpp:106-116
	child_list_t<LogicalType> row_children;
	row_children.push_back(make_pair("y", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat_lower", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat_upper", LogicalType::DOUBLE));
	row_children.push_back(make_pair("is_training", LogicalType::BOOLEAN));
	return LogicalType::LIST(LogicalType::STRUCT(std::move(row_children)));
}

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
	auto states = (HipBlsRowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		if (entry.length > max_features)
			throw InvalidInputException("anofox_stats bls_fit_predict_agg (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)entry.length);
		auto &rows = BlsRows(state, entry.length);
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
			training = split_data.validity.RowIsValid(s_idx) && IsBlsSplitTraining(split_values[s_idx]) && y_valid;
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
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipBlsRowsState **)sdata.data;
	std::map<idx_t, BlsPredictBatch> batches;
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
	for (auto &kv : batches) kv.second.Run(bind.opts);
	auto list_data = ListVector::GetData(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.buffers.size(); g++) {
			const idx_t r = b.result_rows[g];
			if (b.Failed(g)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const BlsRowBuffer &rows = *b.buffers[g];
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
unique_ptr<FunctionData> HipBlsPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipBlsOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable())
		ParseHipBlsOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts, true, true);
	function.return_type = GetHipBlsPredictAggResultType();
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
	auto states = (HipBlsRowsState **)sdata.data;
	const idx_t max_features = anofox_hip_max_features();
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto y_idx = y_data.sel->get_index(i);
		if (!y_data.validity.RowIsValid(y_idx)) continue;
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		if (entry.length > max_features)
			throw InvalidInputException("anofox_stats bls_fit_agg (HIP): at most %llu features are supported, got %llu",
			                            (unsigned long long)max_features, (unsigned long long)entry.length);
		auto &rows = BlsRows(state, entry.length);
		const size_t at = rows.x.size();
		rows.x.resize(at + entry.length);
		for (idx_t j = 0; j < entry.length; j++) {
			const idx_t pos = entry.offset + j;
			rows.x[at + j] = x_child_validity.RowIsValid(pos) ? x_child_data[pos] : NAN; // never read the slot of a NULL
		}
		rows.y.push_back(y_values[y_idx]);
		rows.flags.push_back(kTraining);
		rows.n_training++;
	}
}

// Finalize (bls_aggregate.cpp:249-330): NULL with fewer than 2 buffered rows or a failed fit; ONE batched call per feature count
void HipBlsAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipBlsBindData>();
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (HipBlsRowsState **)sdata.data;
	struct FitBatch {
		idx_t p = 0;
		vector<idx_t> result_rows;
		vector<BlsRowBuffer *> buffers;
	};
	std::map<idx_t, FitBatch> batches;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		if (!state.rows || state.rows->Rows() < 2 || state.rows->n_features == 0) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		auto &b = batches[state.rows->n_features];
		b.p = state.rows->n_features;
		b.result_rows.push_back(i + offset);
		b.buffers.push_back(state.rows);
	}
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		const idx_t p = b.p, G = b.buffers.size(), rec_len = 3 * p + 6;
		vector<int64_t> offsets {0};
		int64_t n = 0;
		for (auto *buf : b.buffers) {
			n += (int64_t)buf->Rows();
			offsets.push_back(n);
		}
		vector<double> y((size_t)n), cols((size_t)n * p), rec(G * rec_len);
		int64_t at = 0;
		for (auto *buf : b.buffers) {
			const idx_t rows = buf->Rows();
			for (idx_t r = 0; r < rows; r++) {
				y[at + r] = buf->y[r];
				for (idx_t j = 0; j < p; j++) cols[j * (size_t)n + at + r] = buf->x[r * p + j];
			}
			at += (int64_t)rows;
		}
		vector<const double *> col_ptrs(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * (size_t)n;
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_bls_fit_batch_host(nullptr, (int64_t)G, p, n, offsets.data(), y.data(), col_ptrs.data(), bind.opts.Batch(), rec.data(), nullptr, &err))
			throw InvalidInputException("anofox_stats (HIP): %s", err.message[0] ? err.message : "the batched call failed");
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
				const idx_t lo = ListVector::GetListSize(lv);
				ListVector::Reserve(lv, lo + p);
				ListVector::SetListSize(lv, lo + p);
				ListVector::GetData(lv)[r].offset = lo;
				ListVector::GetData(lv)[r].length = p;
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

FunctionDescription Describe(const char *what, const string &example, vector<string> names, const vector<LogicalType> &types) {
	FunctionDescription d;
	d.description = what;
	d.examples = {example};
	d.categories = {"regression"};
	d.parameter_names = std::move(names);
	d.parameter_types = types;
	return d;
}

template <bool NNLS>
void RegisterFit(ExtensionLoader &loader, const char *name, const char *alias, const char *what) {
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, GetHipBlsAggResultType(), AggregateFunction::StateSize<HipBlsRowsState>, HipBlsRowsInitialize,
			                                  HipBlsAggUpdate, HipBlsRowsCombine, HipBlsAggFinalize, nullptr, HipBlsAggBind<NNLS>, HipBlsRowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, {'fit_intercept': true})", {"y", "x", "options"}, map_args));
	loader.RegisterFunction(std::move(info));
	CreateAggregateFunctionInfo alias_info(fill(alias));
	alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	alias_info.alias_of = name;
	loader.RegisterFunction(std::move(alias_info));
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
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<HipBlsRowsState>, HipBlsRowsInitialize,
		                         HipBlsPredictAggUpdate, HipBlsRowsCombine, HipBlsPredictAggFinalize, nullptr,
		                         split ? HipBlsPredictAggBind<true> : HipBlsPredictAggBind<false>, HipBlsRowsDestroy);
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
	info.descriptions.push_back(Describe(what, head + ", {'lower_bound': 0.0})", {"y", "x", "options"}, map_args));
	info.descriptions.push_back(Describe(what, head + ", split_col)", {"y", "x", "split_col"}, split_args));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'upper_bound': 1.0})", {"y", "x", "split_col", "options"}, split_map_args));
	loader.RegisterFunction(std::move(info));
	CreateAggregateFunctionInfo alias_info(fill("bls_fit_predict_agg"));
	alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	alias_info.alias_of = name;
	loader.RegisterFunction(std::move(alias_info));
}

} // namespace duckdb
