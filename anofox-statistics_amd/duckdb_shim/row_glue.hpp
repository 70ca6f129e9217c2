// row_glue.hpp — what the row-buffering DuckDB glue files of this directory share (family_agg_hip.cpp, elasticnet_agg_hip.cpp,
// elasticnet_family_hip.cpp, rls_family_hip.cpp, bls_family_hip.cpp, quantile_family_hip.cpp, glm_family_hip.cpp;
// fit_agg_hip.cpp takes the small pieces at the end): the host-side row buffer behind a one-pointer DuckDB state, its
// Initialize / Destroy / Combine, the Finalize vector as one batch per feature count staged for the batched C ABI, and the
// helpers that write results and register function sets.  row_shapes.hpp builds the callbacks that come in a few shapes on
// top of it: Update, Bind, the Finalize tails of the prediction rows and the overload blocks of a registration.
// Everything is inline or a template: several of these .cpp files are linked into one extension.
//
// Each family keeps what is its own: its options and their parser, which rows train (its traits for row_shapes.hpp's Update),
// which states are fitted (the keep predicate of CollectBatches), its one ABI call (Run) and its record layout and result types.
#pragma once
#include <math.h>
#include <string.h>

#include <cctype>
#include <map>
#include <utility>

#include "duckdb.hpp"
#include "duckdb/function/aggregate_function.hpp"
#include "duckdb/main/extension/extension_loader.hpp"
#include "duckdb/parser/parsed_data/create_aggregate_function_info.hpp"

#include "anofox_stats_hip.h"

namespace duckdb {
namespace hip_glue {

[[noreturn]] inline void ThrowAbi(const AnofoxError &err) {
	throw InvalidInputException("anofox_stats (HIP): %s", err.message[0] ? err.message : "the batched call failed");
}

// the per-function prefix of the library's width limit (anofox_hip_max_features)
inline void CheckMaxFeatures(const char *function, idx_t n_features, idx_t max_features) {
	if (n_features > max_features)
		throw InvalidInputException("anofox_stats %s (HIP): at most %llu features are supported, got %llu", function, (unsigned long long)max_features,
		                            (unsigned long long)n_features);
}

// ---- the row buffer behind a DuckDB state: everything Update accepted, in arrival order ----
struct RowBuffer {
	idx_t n_features = 0;
	vector<double> y;        // NaN where y was NULL
	vector<double> x;        // row-major, n_features per row; a NULL list element is NaN
	vector<double> w;        // weighted models only
	vector<uint8_t> flags;   // per row: kYNull | kTraining
	idx_t n_training = 0;
	// the window aggregates: x of the last row Update saw (ols_fit_predict.cpp:29-31)
	vector<double> current_x;
	bool has_current_x = false;
	idx_t Rows() const { return y.size(); }
	void Append(const RowBuffer &o) {
		y.insert(y.end(), o.y.begin(), o.y.end());
		x.insert(x.end(), o.x.begin(), o.x.end());
		w.insert(w.end(), o.w.begin(), o.w.end());
		flags.insert(flags.end(), o.flags.begin(), o.flags.end());
		n_training += o.n_training;
	}
};
constexpr uint8_t kYNull = 1, kTraining = 2;

// The DuckDB-side state is one pointer: Initialize has nothing to construct and an untouched state costs no allocation
// (a window query makes a state per output row).
struct RowsState {
	RowBuffer *rows;
};

inline void RowsInitialize(const AggregateFunction &, data_ptr_t state_p) { reinterpret_cast<RowsState *>(state_p)->rows = nullptr; }

inline void RowsDestroy(Vector &state_vector, AggregateInputData &, idx_t count) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (RowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		delete state.rows;
		state.rows = nullptr;
	}
}

// The state's buffer; the first row with a non-NULL x list fixes the feature count (ols_predict_aggregate.cpp:182-187).
// with_counts: the text of ols_predict_aggregate.cpp / ols_fit_predict.cpp, quantile_fit_predict_aggregate.cpp:162-164 and
// elasticnet_aggregate.cpp; bare: the text of the ridge / wls files, rls_predict_aggregate.cpp:190-192,
// bls_fit_predict_aggregate.cpp:204-207 and elasticnet_predict_aggregate.cpp:190-192
inline RowBuffer &RowsOf(RowsState &state, idx_t n_features, bool with_counts) {
	if (!state.rows) {
		state.rows = new RowBuffer();
		state.rows->n_features = n_features;
	}
	if (state.rows->n_features != n_features) {
		if (with_counts)
			throw InvalidInputException("Inconsistent feature count: expected %llu, got %llu", (unsigned long long)state.rows->n_features,
			                            (unsigned long long)n_features);
		throw InvalidInputException("Inconsistent feature count");
	}
	return *state.rows;
}

inline bool IsSplitTraining(const string_t &split) { // 'train' / 'training', any case (ols_predict_aggregate.cpp:125-132)
	string v = split.GetString();
	for (auto &c : v) c = (char)std::tolower((unsigned char)c);
	return v == "train" || v == "training";
}

// One x list row into dst: a NULL element is NaN — never read the slot of a NULL (upstream issue #95)
struct ListRowFlags {
	bool has_null = false; // a NULL element
	bool has_zero = false; // an element that is exactly 0 (null_policy = 'drop_y_zero_x')
};
inline ListRowFlags ReadListRow(const list_entry_t &entry, const double *child_data, const ValidityMask &child_validity, double *dst) {
	ListRowFlags f;
	for (idx_t j = 0; j < entry.length; j++) {
		const idx_t pos = entry.offset + j;
		if (child_validity.RowIsValid(pos)) {
			dst[j] = child_data[pos];
			f.has_zero = f.has_zero || dst[j] == 0.0;
		} else {
			dst[j] = NAN;
			f.has_null = true;
		}
	}
	return f;
}

// Combine: an initialised source is appended to the target; an uninitialised target takes the source's buffer (moved when the
// source may be consumed, copied under PRESERVE_INPUT — the window segment tree).  WINDOW: the later state's current row is
// the frame's last (ols_fit_predict.cpp:238-241, rls_fit_predict.cpp:224-227, elasticnet_fit_predict.cpp:224-227).
// WITH_COUNTS: the error text of the non-window ols / ridge / wls aggregates and of elasticnet_aggregate.cpp.
template <bool WINDOW, bool WITH_COUNTS = false>
void RowsCombine(Vector &source_vector, Vector &target_vector, AggregateInputData &aggr_input_data, idx_t count) {
	UnifiedVectorFormat source_data, target_data;
	source_vector.ToUnifiedFormat(count, source_data);
	target_vector.ToUnifiedFormat(count, target_data);
	auto sources = (RowsState **)source_data.data;
	auto targets = (RowsState **)target_data.data;
	const bool preserve = aggr_input_data.combine_type == AggregateCombineType::PRESERVE_INPUT;
	for (idx_t i = 0; i < count; i++) {
		auto &source = *sources[source_data.sel->get_index(i)];
		auto &target = *targets[target_data.sel->get_index(i)];
		if (!source.rows || &source == &target) continue;
		if (!target.rows) {
			if (preserve) {
				target.rows = new RowBuffer(*source.rows);
			} else {
				target.rows = source.rows;
				source.rows = nullptr;
			}
			continue;
		}
		if (source.rows->n_features != target.rows->n_features) {
			if (WITH_COUNTS)
				throw InvalidInputException("Cannot combine states with different feature counts: %llu vs %llu", (unsigned long long)source.rows->n_features,
				                            (unsigned long long)target.rows->n_features);
			throw InvalidInputException("Cannot combine states with different feature counts");
		}
		target.rows->Append(*source.rows);
		if (WINDOW && source.rows->has_current_x) {
			target.rows->current_x = source.rows->current_x;
			target.rows->has_current_x = true;
		}
	}
}

// ---- the states of one Finalize vector as one batch per feature count ----
struct RowBatch {
	idx_t p = 0;
	vector<idx_t> result_rows;     // where each group of the batch goes
	vector<RowBuffer *> buffers;
	vector<int64_t> offsets {0};
	vector<int64_t> train_counts;
	vector<double> y, w, cols;     // cols: p columns of n rows, one after the other
	vector<const double *> col_ptrs;
	idx_t Groups() const { return buffers.size(); }
	// The batch as the ABI takes it: states = groups, columns concatenated, y = NaN for a row that does not train (its weight
	// 1).  extra_row: the window aggregates append their current x as a last row that does not train.  Returns the row count.
	int64_t Stage(bool weighted, bool extra_row) {
		int64_t n = 0;
		for (auto *b : buffers) {
			n += (int64_t)b->Rows() + (extra_row ? 1 : 0);
			offsets.push_back(n);
			train_counts.push_back((int64_t)b->n_training);
		}
		y.resize((size_t)n);
		cols.resize((size_t)n * p);
		if (weighted) w.resize((size_t)n);
		int64_t at = 0;
		for (auto *b : buffers) {
			const idx_t rows = b->Rows();
			for (idx_t r = 0; r < rows; r++) {
				const bool train = b->flags[r] & kTraining;
				y[at + r] = train ? b->y[r] : NAN;
				if (weighted) w[at + r] = train ? b->w[r] : 1.0;
				for (idx_t j = 0; j < p; j++) cols[j * (size_t)n + at + r] = b->x[r * p + j];
			}
			at += (int64_t)rows;
			if (extra_row) {
				y[at] = NAN;
				if (weighted) w[at] = 1.0;
				for (idx_t j = 0; j < p; j++) cols[j * (size_t)n + at] = b->current_x[j];
				at++;
			}
		}
		col_ptrs.resize(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * (size_t)n;
		return n;
	}
};

// The states of a Finalize vector that are fitted, by feature count; the others are NULL: a state no row reached, an empty x
// list (the FFI refuses it), and whatever the family's keep(const RowBuffer &) turns down.  BATCH: RowBatch or the family's own.
template <class BATCH, class KEEP>
std::map<idx_t, BATCH> CollectBatches(Vector &state_vector, Vector &result, idx_t count, idx_t offset, KEEP &&keep) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (RowsState **)sdata.data;
	std::map<idx_t, BATCH> batches;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		if (!state.rows || state.rows->n_features == 0 || !keep(*state.rows)) {
			FlatVector::SetNull(result, i + offset, true);
			continue;
		}
		auto &b = batches[state.rows->n_features];
		b.p = state.rows->n_features;
		b.result_rows.push_back(i + offset);
		b.buffers.push_back(state.rows);
	}
	return batches;
}

// ---- writing results ----
// a LIST entry of `length` rows at the end of the list's child, reserved before it is written (the reference's SetListInResult
// omits the Reserve, ols_aggregate.cpp:237-246); returns the entry's offset in the child
inline idx_t AppendListEntry(Vector &list_vec, idx_t row, idx_t length) {
	const idx_t list_offset = ListVector::GetListSize(list_vec);
	ListVector::Reserve(list_vec, list_offset + length);
	ListVector::SetListSize(list_vec, list_offset + length);
	auto entries = ListVector::GetData(list_vec);
	entries[row].offset = list_offset;
	entries[row].length = length;
	return list_offset;
}

inline void AppendList(Vector &list_vec, idx_t row, const double *src, idx_t n) {
	const idx_t list_offset = AppendListEntry(list_vec, row, n);
	auto child = FlatVector::GetData<double>(ListVector::GetEntry(list_vec));
	for (idx_t k = 0; k < n; k++) child[list_offset + k] = src[k];
}

inline void SetDoubleOrNull(Vector &field, idx_t at, double v, bool is_null) {
	if (is_null) FlatVector::SetNull(field, at, true);
	else FlatVector::GetData<double>(field)[at] = v;
}

inline LogicalType PredictAggResultType() { // ols_predict_aggregate.cpp:93-104 and its rls / bls / elastic net twins
	child_list_t<LogicalType> row_children;
	row_children.push_back(make_pair("y", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat_lower", LogicalType::DOUBLE));
	row_children.push_back(make_pair("yhat_upper", LogicalType::DOUBLE));
	row_children.push_back(make_pair("is_training", LogicalType::BOOLEAN));
	return LogicalType::LIST(LogicalType::STRUCT(std::move(row_children)));
}

inline LogicalType FitPredictResultType() { // ols_fit_predict.cpp:84-90
	child_list_t<LogicalType> children;
	children.push_back(make_pair("yhat", LogicalType::DOUBLE));
	children.push_back(make_pair("yhat_lower", LogicalType::DOUBLE));
	children.push_back(make_pair("yhat_upper", LogicalType::DOUBLE));
	return LogicalType::STRUCT(std::move(children));
}

// One group of a predict aggregate into its PredictAggResultType() row: every buffered row with its prediction, pred = the
// group's [rows x 3] {yhat, yhat_lower, yhat_upper}.  y is NULL where the input was; a non-finite prediction is three NULLs
// (ols_predict_aggregate.cpp:404-413).
inline void AppendPredictRows(Vector &result, idx_t row, const RowBuffer &rows, const double *pred) {
	const idx_t n_rows = rows.Rows();
	const idx_t list_offset = AppendListEntry(result, row, n_rows);
	auto &fields = StructVector::GetEntries(ListVector::GetEntry(result)); // [y, yhat, yhat_lower, yhat_upper, is_training]
	for (idx_t r = 0; r < n_rows; r++) {
		const idx_t at = list_offset + r;
		SetDoubleOrNull(*fields[0], at, rows.y[r], (rows.flags[r] & kYNull) != 0);
		const bool no_prediction = !isfinite(pred[r * 3]);
		for (idx_t k = 0; k < 3; k++) SetDoubleOrNull(*fields[1 + k], at, pred[r * 3 + k], no_prediction);
		FlatVector::GetData<bool>(*fields[4])[at] = (rows.flags[r] & kTraining) != 0;
	}
}

// ---- registration ----
inline FunctionDescription Describe(const char *what, const string &example, vector<string> names, const vector<LogicalType> &types,
                                    vector<string> categories) {
	FunctionDescription d;
	d.description = what;
	d.examples = {example};
	d.categories = std::move(categories);
	d.parameter_names = std::move(names);
	d.parameter_types = types;
	return d;
}

inline void RegisterAlias(ExtensionLoader &loader, const string &name, AggregateFunctionSet alias_set) {
	CreateAggregateFunctionInfo alias_info(std::move(alias_set));
	alias_info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	alias_info.alias_of = name;
	loader.RegisterFunction(std::move(alias_info));
}

// a function set with its descriptions, then the same set under its alias
inline void RegisterWithAlias(ExtensionLoader &loader, CreateAggregateFunctionInfo info, AggregateFunctionSet alias_set) {
	const string name = info.functions.name;
	info.on_conflict = OnCreateConflict::ALTER_ON_CONFLICT;
	loader.RegisterFunction(std::move(info));
	RegisterAlias(loader, name, std::move(alias_set));
}

} // namespace hip_glue
} // namespace duckdb
