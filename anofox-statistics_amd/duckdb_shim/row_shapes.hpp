// row_shapes.hpp — the callbacks of the row-buffering glue files that come in a few shapes only, written once on top of
// row_glue.hpp: the reader of an Update vector, Update for the three shapes (predict aggregate, window aggregate, fit
// aggregate), the bind data and Bind, the Finalize tails that write prediction rows, and the registration of the
// (y, x) / (y, x, options) [/ (y, x, split_col) / (y, x, split_col, options)] overload blocks.
//
// A family names what is its own in a traits struct of static constexpr members (RowTraits holds the defaults) that the
// templates read at compile time; the per-row paths carry no run-time switch that the copies they replace did not have.
// The table of what differs today, each with the place in the reference that it follows, stands at the traits:
//
//                        name in messages            width checked  counts in RowsOf's text  weights  NULL element  drop_y_zero_x
//   ols   predict/window fit_predict_agg/fit_predict yes            yes                      -        stops train.  read
//   ridge predict/window fit_predict_agg/fit_predict yes            no                       -        kept          read
//   wls   predict/window fit_predict_agg/fit_predict yes            no                       yes      kept          read
//   elastic net p / w    elasticnet_fit_predict[_agg] yes           no                       -        kept          read
//   rls   predict/window rls_fit_predict[_agg]       yes            no                       -        kept          read
//   bls   predict        bls_fit_predict_agg         yes            no                       -        kept          read
//   glm   predict        glm aggregates              no             yes                      -        kept          read
//   quantile p / w       quantile_fit_predict        no             yes                      -        kept          never
//   fit aggregates       rls_fit_agg, bls_fit_agg (nnls too): checked, bare; glm aggregates, elasticnet_fit_agg: not checked
//                        in Update (the elastic net checks what it is about to fit, in Finalize), with counts
#pragma once
#include "duckdb/execution/expression_executor.hpp"

#include "row_glue.hpp"

namespace duckdb {
namespace hip_glue {

// ---- bind data: the parsed options, whether a split column is bound, and the family's kind where it has one ----
struct NoKind {
	bool operator==(const NoKind &) const { return true; }
};
template <class OPTS, class KIND = NoKind>
struct RowsBindData : public FunctionData {
	RowsBindData(const OPTS &opts_p, bool use_split_col_p, KIND kind_p = KIND()) : opts(opts_p), use_split_col(use_split_col_p), kind(kind_p) {}
	OPTS opts;
	bool use_split_col;
	KIND kind;
	unique_ptr<FunctionData> Copy() const override { return make_uniq<RowsBindData>(opts, use_split_col, kind); }
	bool Equals(const FunctionData &other_p) const override {
		auto &other = other_p.Cast<RowsBindData>();
		return kind == other.kind && opts == other.opts && use_split_col == other.use_split_col;
	}
};

// Bind: the options argument at opt_idx is parsed when it is there and folds to a constant — options that are not constant
// keep the defaults (ols_predict_aggregate.cpp:435-447) — then return_type(opts) is the function's type.
template <class OPTS, class KIND = NoKind, class PARSE, class TYPE>
unique_ptr<FunctionData> BindRows(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments, idx_t opt_idx,
                                  bool use_split_col, PARSE &&parse, TYPE &&return_type, KIND kind = KIND()) {
	OPTS opts;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable()) parse(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), opts);
	function.return_type = return_type(opts);
	return make_uniq<RowsBindData<OPTS, KIND>>(opts, use_split_col, kind);
}

// ---- one Update vector: y, x[, weights at 2][, split column at split_at], and the states ----
struct RowsInput {
	RowsInput(Vector inputs[], idx_t count, Vector &state_vector, bool weighted, idx_t split_at /* 0: none */)
	    : x_child_data(FlatVector::GetData<double>(ListVector::GetEntry(inputs[1]))), x_child_validity(FlatVector::Validity(ListVector::GetEntry(inputs[1]))) {
		inputs[0].ToUnifiedFormat(count, y_data);
		inputs[1].ToUnifiedFormat(count, x_data);
		if (weighted) inputs[2].ToUnifiedFormat(count, w_data);
		if (split_at) inputs[split_at].ToUnifiedFormat(count, split_data);
		state_vector.ToUnifiedFormat(count, sdata);
	}
	RowsInput(const RowsInput &) = delete; // (a unified format may point into itself)
	RowsState &State(idx_t i) const { return *((RowsState **)sdata.data)[sdata.sel->get_index(i)]; }
	// the row's x list, nullptr where it is NULL
	const list_entry_t *X(idx_t i) const {
		const auto idx = x_data.sel->get_index(i);
		return x_data.validity.RowIsValid(idx) ? UnifiedVectorFormat::GetData<list_entry_t>(x_data) + idx : nullptr;
	}
	// false where the value is NULL; v is then left as it is
	bool Y(idx_t i, double &v) const { return Read(y_data, i, v); }
	bool W(idx_t i, double &v) const { return Read(w_data, i, v); }
	bool SplitTrains(idx_t i) const { // a NULL split value does not train (ols_predict_aggregate.cpp:217-226)
		const auto idx = split_data.sel->get_index(i);
		return split_data.validity.RowIsValid(idx) && IsSplitTraining(UnifiedVectorFormat::GetData<string_t>(split_data)[idx]);
	}
	ListRowFlags ReadX(const list_entry_t &entry, double *dst) const { return ReadListRow(entry, x_child_data, x_child_validity, dst); }
	ListRowFlags AppendX(const list_entry_t &entry, vector<double> &x) const {
		const size_t at = x.size();
		x.resize(at + entry.length);
		return ReadX(entry, x.data() + at);
	}

private:
	static bool Read(const UnifiedVectorFormat &data, idx_t i, double &v) {
		const auto idx = data.sel->get_index(i);
		if (!data.validity.RowIsValid(idx)) return false;
		v = UnifiedVectorFormat::GetData<double>(data)[idx];
		return true;
	}
	UnifiedVectorFormat y_data, x_data, w_data, split_data, sdata;
	const double *x_child_data;
	const ValidityMask &x_child_validity;
};

// ---- what a family says about its Update; the defaults are the most common choice ----
struct RowTraits {
	// kName: the function's name in "too few arguments" and in the width limit's text — each family declares its own
	static constexpr bool kCheckMaxFeatures = true;         // anofox_hip_max_features() per row, under kName
	static constexpr bool kCountsInError = false;           // RowsOf's text: bare, or with the two counts
	static constexpr bool kWeighted = false;                // a weights column at argument 2
	static constexpr bool kNullElementStopsTraining = false; // a NULL list element: kept (the fit's row filter drops the row), or not training
	static constexpr bool kBuffersEveryRow = false;         // the window shape: training rows only, or every row with its flags
	// static bool DropYZeroX(const Bind &): null_policy = 'drop_y_zero_x' of the bound options; constant false where it is never read
};

[[noreturn]] inline void ThrowTooFewArguments(const char *function) {
	throw InvalidInputException("anofox_stats %s (HIP): too few arguments", function);
}

inline void PushRow(RowBuffer &rows, double y, bool y_valid, bool training) {
	rows.y.push_back(y);
	rows.flags.push_back((uint8_t)((y_valid ? 0 : kYNull) | (training ? kTraining : 0)));
	rows.n_training += training ? 1 : 0;
}

// Predict aggregate, (y, x[, weights][, split_col][, options]): every row with a non-NULL x list (and, weighted, a non-NULL
// weight) is kept for the output; it trains iff y is not NULL — with a split column: iff the split value says train AND y is
// not NULL — and the traits' further conditions hold (ols_predict_aggregate.cpp:134-268 and its twins).
template <class T>
void RowsPredictAggUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<typename T::Bind>();
	constexpr idx_t kSplitAt = T::kWeighted ? 3 : 2;
	if (input_count < kSplitAt) ThrowTooFewArguments(T::kName);
	const bool split = bind.use_split_col && input_count > kSplitAt;
	RowsInput in(inputs, count, state_vector, T::kWeighted, split ? kSplitAt : 0);
	const bool drop_y_zero_x = T::DropYZeroX(bind);
	const idx_t max_features = T::kCheckMaxFeatures ? anofox_hip_max_features() : 0;
	for (idx_t i = 0; i < count; i++) {
		const list_entry_t *entry = in.X(i);
		if (!entry) continue; // a NULL x list: the row does not exist for this aggregate
		double weight = 1.0;
		if (T::kWeighted && !in.W(i, weight)) continue;
		if (T::kCheckMaxFeatures) CheckMaxFeatures(T::kName, entry->length, max_features);
		auto &rows = RowsOf(in.State(i), entry->length, T::kCountsInError);
		const ListRowFlags x_flags = in.AppendX(*entry, rows.x);
		double y = NAN;
		const bool y_valid = in.Y(i, y);
		bool training = y_valid;
		if (split) training = in.SplitTrains(i) && y_valid;
		// wls_predict_aggregate.cpp:212-217 (`weight <= 0`; a NaN weight trains upstream and fails the fit there — here it does not train)
		if (T::kWeighted && !(weight > 0)) training = false;
		if (T::kNullElementStopsTraining && x_flags.has_null) training = false;
		if (training && drop_y_zero_x && x_flags.has_zero) training = false;
		PushRow(rows, y, y_valid, training);
		if (T::kWeighted) rows.w.push_back(weight);
	}
}

// Window aggregate, (y, x[, weight][, options]) OVER (...): the frame's rows arrive one by one; the last one with a non-NULL x
// list is the row to predict (a NULL x list there: nothing to predict), every one with a non-NULL y (and weight) trains
// (ols_fit_predict.cpp:110-193).  A NULL list element is NaN — the reference reads the slot as it is.
template <class T>
void RowsWindowUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<typename T::Bind>();
	if (input_count < (T::kWeighted ? 3u : 2u)) ThrowTooFewArguments(T::kName);
	RowsInput in(inputs, count, state_vector, T::kWeighted, 0);
	const bool drop_y_zero_x = T::DropYZeroX(bind);
	const idx_t max_features = T::kCheckMaxFeatures ? anofox_hip_max_features() : 0;
	for (idx_t i = 0; i < count; i++) {
		auto &state = in.State(i);
		const list_entry_t *entry = in.X(i);
		if (!entry) {
			if (state.rows) state.rows->has_current_x = false; // ols_fit_predict.cpp:141-144
			continue;
		}
		if (T::kCheckMaxFeatures) CheckMaxFeatures(T::kName, entry->length, max_features);
		auto &rows = RowsOf(state, entry->length, T::kCountsInError);
		double y = NAN;
		if (T::kBuffersEveryRow) { // the row is buffered with its flags and copied into current_x
			in.AppendX(*entry, rows.x);
			rows.current_x.assign(rows.x.end() - (ptrdiff_t)entry->length, rows.x.end());
			rows.has_current_x = true;
			const bool y_valid = in.Y(i, y);
			PushRow(rows, y, y_valid, y_valid);
			continue;
		}
		rows.current_x.resize(entry->length);
		const bool has_zero = in.ReadX(*entry, rows.current_x.data()).has_zero;
		rows.has_current_x = true;
		bool training = in.Y(i, y);
		double weight = 1.0;
		if (T::kWeighted) training = training && in.W(i, weight); // wls_fit_predict.cpp:150-154: the row's x is still the current x
		if (training && drop_y_zero_x && has_zero) training = false;
		if (!training) continue;
		rows.x.insert(rows.x.end(), rows.current_x.begin(), rows.current_x.end());
		PushRow(rows, y, true, true);
		if (T::kWeighted) rows.w.push_back(weight);
	}
}

// Fit aggregate, (y, x[, options]): a row with a NULL y or a NULL x list is skipped before anything about it is checked, every
// other row is buffered in arrival order; a NULL list element is NaN, so the fit's row filter drops that row
// (bls_aggregate.cpp:118-180, poisson_aggregate.cpp:149-218)
template <class T>
void RowsFitAggUpdate(Vector inputs[], AggregateInputData &, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 2) ThrowTooFewArguments(T::kName);
	RowsInput in(inputs, count, state_vector, false, 0);
	const idx_t max_features = T::kCheckMaxFeatures ? anofox_hip_max_features() : 0;
	for (idx_t i = 0; i < count; i++) {
		double y = NAN;
		if (!in.Y(i, y)) continue;
		const list_entry_t *entry = in.X(i);
		if (!entry) continue;
		if (T::kCheckMaxFeatures) CheckMaxFeatures(T::kName, entry->length, max_features);
		auto &rows = RowsOf(in.State(i), entry->length, T::kCountsInError);
		in.AppendX(*entry, rows.x);
		PushRow(rows, y, true, true);
	}
}

// ---- Finalize ----
// a RowBatch with the outputs of a fit-predict call: core [G x (p + 6)] with the status last, pred [n x 3]
struct PredictBatch : RowBatch {
	vector<double> core, pred;
	int64_t StagePredict(bool weighted, bool extra_row) {
		const int64_t n = Stage(weighted, extra_row);
		core.resize(Groups() * (p + 6));
		pred.resize((size_t)n * 3);
		return n;
	}
	bool Failed(idx_t g) const { return core[g * (p + 6) + p + 5] != 0.0; }
};

// Predict aggregate: the states keep() accepts go through run(batch), one call per feature count; a group whose fit failed
// is NULL (ols_predict_aggregate.cpp:366-369), every other one gets its buffered rows with their predictions.
// BATCH: pred [n x 3], Failed(g).  (The reference's state.Reset() after a fit: Destroy frees the buffers here.)
template <class BATCH, class KEEP, class RUN>
void FinalizePredictRows(Vector &state_vector, Vector &result, idx_t count, idx_t offset, KEEP &&keep, RUN &&run) {
	auto batches = CollectBatches<BATCH>(state_vector, result, count, offset, keep);
	for (auto &kv : batches) run(kv.second);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			if (b.Failed(g)) FlatVector::SetNull(result, b.result_rows[g], true);
			else AppendPredictRows(result, b.result_rows[g], *b.buffers[g], &b.pred[(size_t)b.offsets[g] * 3]);
		}
	}
}

// Window aggregate: NULL without a current row or with at most p + [intercept] training rows (ols_fit_predict.cpp:246-324);
// otherwise the state's training rows plus its current row — the group's last, which run() appends — form one group, and the
// prediction of that last row goes into FitPredictResultType().  NULL_NON_FINITE: a prediction that is not finite is NULL
// (elasticnet_fit_predict.cpp:270-286, rls_fit_predict.cpp), or stays what the library made of it, as the reference writes
// whatever anofox_predict_with_interval returned (ols_fit_predict.cpp:311-318).
template <class BATCH, bool NULL_NON_FINITE, class RUN>
void FinalizeWindowRows(Vector &state_vector, Vector &result, idx_t count, idx_t offset, bool fit_intercept, RUN &&run) {
	const idx_t intercept = fit_intercept ? 1 : 0;
	auto batches = CollectBatches<BATCH>(state_vector, result, count, offset, [&](const RowBuffer &rows) {
		return rows.has_current_x && rows.n_training > rows.n_features + intercept;
	});
	for (auto &kv : batches) run(kv.second);
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			const idx_t r = b.result_rows[g];
			const double *pred = &b.pred[((size_t)b.offsets[g + 1] - 1) * 3];
			if (b.Failed(g) || (NULL_NON_FINITE && !isfinite(pred[0]))) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			for (idx_t k = 0; k < 3; k++) FlatVector::GetData<double>(*fields[k])[r] = pred[k];
		}
	}
}

// ---- registration ----
// what the overload blocks of one function share: its names, its description, and the arguments before split_col / options
struct RowsFunctionNames {
	string name, alias;
	vector<string> deprecated; // further aliases: the reference's older names
	const char *what;
	vector<string> categories;
	vector<LogicalType> base = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	vector<string> base_names = {"y", "x"};
	string Head() const {
		string head = name + "(";
		for (size_t k = 0; k < base_names.size(); k++) head += (k ? ", " : "") + base_names[k];
		return head;
	}
};

template <class T>
vector<T> Plus(vector<T> v, std::initializer_list<T> more) {
	v.insert(v.end(), more);
	return v;
}

// (y, x) and (y, x, options), make(fname, args) being the function; then the same set under the alias.  options_first: the
// description of the overload with options stands before the other one (elasticnet_aggregate.cpp's order)
template <class MAKE>
void RegisterWithOptions(ExtensionLoader &loader, const RowsFunctionNames &f, const string &options_example, MAKE &&make, bool options_first = false) {
	const vector<LogicalType> map_args = Plus<LogicalType>(f.base, {LogicalType::ANY});
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		set.AddFunction(make(fname, f.base));    // (y, x)
		set.AddFunction(make(fname, map_args));  // (y, x, options)
		return set;
	};
	CreateAggregateFunctionInfo info(fill(f.name));
	info.descriptions.push_back(Describe(f.what, f.Head() + ")", f.base_names, f.base, f.categories));
	info.descriptions.push_back(Describe(f.what, f.Head() + ", " + options_example + ")", Plus<string>(f.base_names, {"options"}), map_args, f.categories));
	if (options_first) std::swap(info.descriptions[0], info.descriptions[1]);
	RegisterWithAlias(loader, std::move(info), fill(f.alias));
	for (const string &alias : f.deprecated) RegisterAlias(loader, f.name, fill(alias));
}

// (y, x), (y, x, options), (y, x, split_col), (y, x, split_col, options) of a predict aggregate, make(fname, args, split) being
// the function (ols_predict_aggregate.cpp:497-603); then the same set under the alias and under the deprecated names
template <class MAKE>
void RegisterWithSplitAndOptions(ExtensionLoader &loader, const RowsFunctionNames &f, const string &options_example, const string &split_options_example,
                                 MAKE &&make) {
	const vector<LogicalType> map_args = Plus<LogicalType>(f.base, {LogicalType::ANY}), split_args = Plus<LogicalType>(f.base, {LogicalType::VARCHAR}),
	                          split_map_args = Plus<LogicalType>(f.base, {LogicalType::VARCHAR, LogicalType::ANY});
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		set.AddFunction(make(fname, f.base, false));         // (y, x)
		set.AddFunction(make(fname, map_args, false));       // (y, x, options)
		set.AddFunction(make(fname, split_args, true));      // (y, x, split_col)
		set.AddFunction(make(fname, split_map_args, true));  // (y, x, split_col, options)
		return set;
	};
	CreateAggregateFunctionInfo info(fill(f.name));
	auto describe = [&](const string &tail, std::initializer_list<string> names, const vector<LogicalType> &types) {
		info.descriptions.push_back(Describe(f.what, f.Head() + tail, Plus<string>(f.base_names, names), types, f.categories));
	};
	describe(")", {}, f.base);
	describe(", " + options_example + ")", {"options"}, map_args);
	describe(", split_col)", {"split_col"}, split_args);
	describe(", split_col, " + split_options_example + ")", {"split_col", "options"}, split_map_args);
	RegisterWithAlias(loader, std::move(info), fill(f.alias));
	for (const string &alias : f.deprecated) RegisterAlias(loader, f.name, fill(alias));
}

// the AggregateFunction of a row-buffering aggregate: RowsState behind it, RowsInitialize / RowsDestroy around it
inline AggregateFunction RowsFunction(const string &fname, const vector<LogicalType> &args, const LogicalType &return_type, aggregate_update_t update,
                                      aggregate_combine_t combine, aggregate_finalize_t finalize, bind_aggregate_function_t bind) {
	return AggregateFunction(fname, args, return_type, AggregateFunction::StateSize<RowsState>, RowsInitialize, update, combine, finalize, nullptr, bind,
	                         RowsDestroy);
}

} // namespace hip_glue
} // namespace duckdb
