// glmm_family_hip.cpp — DuckDB glue of the mixed-model family (Gaussian, one random intercept) over the batched C ABI:
//
//   anofox_stats_glmm_fit_agg(y, x, group[, options])                  src/aggregate_functions/glmm_aggregate.cpp (result type
//                                                                      :156-199, Finalize :429-498)
//   anofox_stats_glmm_fit_predict_agg(y, x, group[, split][, options]) NO COUNTERPART in the reference: the fit and a score of
//                                                                      every buffered row
//
// As the other glue files: the DuckDB state buffers the key's rows on the host in arrival order, Combine appends the source's
// rows after the target's, and Finalize turns the whole vector of states into ONE batched call per feature count
// (anofox_hip_glmm_fit_batch_host / anofox_hip_glmm_fit_predict_batch_host) where the reference calls anofox_glmm_fit once per
// state.  The glue adds no arithmetic.  What is its own: the group column.  Its value is taken as VARCHAR, BIGINT or INTEGER and
// rendered to VARCHAR; a state numbers its labels in first-seen order (the code of a row's level rides in RowBuffer::w), Combine
// renumbers the source's codes into the target's, and Finalize sorts a state's rows by level (stably) into the library's
// (panel, level) layout and scatters the predictions back to arrival order.
//
// Options, STRUCT or MAP literal, keys case-insensitive, unknown keys ignored, options that are not constant keep the defaults:
// family (gaussian | normal | lmm), fit_intercept | intercept, reml, max_iterations | max_iter, tolerance | tol,
// compute_inference, confidence_level; the fit-predict aggregate also reads interval ('none' | 'confidence' | 'prediction';
// true: prediction, false: none) and level (default: confidence_level).  What is not built raises at bind with the library's
// texts: another family, an offset, random_slopes.
//
// NULL rules.  glmm_fit_agg skips a row whose y, x list or group is NULL.  glmm_fit_predict_agg skips a row whose x list or group
// is NULL; a row whose y is NULL (or, with a split column, whose split value does not say train) is a prediction row: it
// reaches the library with y = NaN, which the fit's row rule drops and the prediction pass scores.  A panel whose status is not 0
// gives a NULL row.  The fit's fields are written as the library gives them (the reference's Finalize maps nothing); in the
// fit-predict list a value that is not finite is NULL, and yhat_lower / yhat_upper are NULL unless the options carry interval.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU with
// the real library (tests/test_gpu_glmm_glue.py through tests/tools/glmm_family_capi.cpp).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <unordered_map>

#include "duckdb.hpp"
#include "duckdb/common/types/data_chunk.hpp"
#include "duckdb/execution/expression_executor.hpp"
#include "duckdb/function/aggregate_function.hpp"
#include "duckdb/main/extension/extension_loader.hpp"
#include "duckdb/parser/parsed_data/create_aggregate_function_info.hpp"

#include "anofox_stats_hip.h"
#include "glmm_family_hip.hpp"
#include "hip_options.hpp"
#include "row_shapes.hpp"

namespace duckdb {

struct StringVector; // DuckDB's; the stand-in has Vector::AddString in its place (AddLabel below takes whichever there is)

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "mixed_models"};

enum class GlmmKind : uint8_t { FIT, PREDICT };

struct HipGlmmOptions {
	bool fit_intercept = true;
	bool reml = true;
	uint32_t max_iterations = 100;
	double tolerance = 1e-8;
	bool compute_inference = false;
	double confidence_level = 0.95;
	int interval = 0;   // the fit-predict aggregate: 0 none, 1 confidence, 2 prediction
	double level = NAN; // NaN: confidence_level
	bool operator==(const HipGlmmOptions &o) const {
		return fit_intercept == o.fit_intercept && reml == o.reml && max_iterations == o.max_iterations && tolerance == o.tolerance &&
		       compute_inference == o.compute_inference && confidence_level == o.confidence_level && interval == o.interval &&
		       ((isnan(level) && isnan(o.level)) || level == o.level);
	}
	AnofoxHipGlmmOptions Batch() const {
		AnofoxHipGlmmOptions b;
		memset(&b, 0, sizeof b);
		b.family = ANOFOX_GLMM_GAUSSIAN;
		b.fit_intercept = fit_intercept;
		b.reml = reml;
		b.max_iterations = max_iterations;
		b.tolerance = tolerance;
		b.compute_inference = compute_inference;
		b.confidence_level = confidence_level;
		return b;
	}
	AnofoxHipGlmmPredictOptions Predict() const {
		AnofoxHipGlmmPredictOptions q;
		memset(&q, 0, sizeof q);
		q.interval = interval;
		q.level = isnan(level) ? confidence_level : level;
		return q;
	}
};

int ParseInterval(const Value &val) {
	if (val.type().id() == LogicalTypeId::BOOLEAN) return BooleanValue::Get(val) ? 2 : 0;
	const string s = OptionString(val);
	if (s == "none") return 0;
	if (s == "confidence") return 1;
	if (s == "prediction") return 2;
	throw InvalidInputException("Unknown interval '%s'. Expected 'none', 'confidence' or 'prediction'.", s.c_str());
}

void ParseHipGlmmOptions(const Value &v, GlmmKind kind, HipGlmmOptions &o) {
	if (v.IsNull()) return;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (val.IsNull()) return;
		if (key == "family") {
			const string name = OptionString(val);
			for (auto *other : {"poisson", "binomial", "logistic", "negbinomial", "gamma", "tweedie"})
				if (name == other) throw InvalidInputException("glmm: the %s family is not built", name.c_str());
			if (name != "gaussian" && name != "normal" && name != "lmm")
				throw InvalidInputException("Unknown GLMM family '%s'. Expected 'gaussian'.", name.c_str());
		} else if (key == "offset" || key == "offset_column") throw InvalidInputException("glmm: an offset is not built");
		else if (key == "random_slopes") throw InvalidInputException("glmm: random slopes are not built");
		else if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(val);
		else if (key == "reml") o.reml = ExtractBool(val);
		else if (key == "max_iterations" || key == "max_iter") o.max_iterations = ExtractUInteger(val);
		else if (key == "tolerance" || key == "tol") o.tolerance = val.GetValue<double>();
		else if (key == "compute_inference") o.compute_inference = ExtractBool(val);
		else if (key == "confidence_level") o.confidence_level = val.GetValue<double>();
		else if (key == "interval") {
			if (kind == GlmmKind::PREDICT) o.interval = ParseInterval(val);
		} else if (key == "level") {
			if (kind == GlmmKind::PREDICT) o.level = val.GetValue<double>();
		}
	});
}

using HipGlmmBindData = RowsBindData<HipGlmmOptions, GlmmKind>;

// ---- the state: row_glue.hpp's buffer and the key's group labels in first-seen order; RowBuffer::w holds each row's code ----
struct GlmmRows : RowBuffer {
	vector<string> labels;
	std::unordered_map<string, uint32_t> index;
	uint32_t Code(const string &label) {
		auto it = index.find(label);
		if (it != index.end()) return it->second;
		const uint32_t code = (uint32_t)labels.size();
		labels.push_back(label);
		index.emplace(label, code);
		return code;
	}
};

GlmmRows &GlmmRowsOf(RowsState &state, idx_t n_features) {
	if (!state.rows) {
		state.rows = new GlmmRows();
		state.rows->n_features = n_features;
	}
	if (state.rows->n_features != n_features)
		throw InvalidInputException("Inconsistent feature count: expected %llu, got %llu", (unsigned long long)state.rows->n_features,
		                            (unsigned long long)n_features);
	return *static_cast<GlmmRows *>(state.rows);
}

void GlmmDestroy(Vector &state_vector, AggregateInputData &, idx_t count) {
	UnifiedVectorFormat sdata;
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (RowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		delete static_cast<GlmmRows *>(state.rows); // (every buffer of this family is a GlmmRows)
		state.rows = nullptr;
	}
}

// Combine: the source's rows after the target's, the source's level codes renumbered into the target's labels
void GlmmCombine(Vector &source_vector, Vector &target_vector, AggregateInputData &aggr_input_data, idx_t count) {
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
		auto *src = static_cast<GlmmRows *>(source.rows);
		if (!target.rows) {
			if (preserve) {
				target.rows = new GlmmRows(*src);
			} else {
				target.rows = source.rows;
				source.rows = nullptr;
			}
			continue;
		}
		auto *dst = static_cast<GlmmRows *>(target.rows);
		if (src->n_features != dst->n_features)
			throw InvalidInputException("Cannot combine states with different feature counts: %llu vs %llu", (unsigned long long)src->n_features,
			                            (unsigned long long)dst->n_features);
		const size_t at = dst->w.size();
		dst->Append(*src);
		for (size_t r = at; r < dst->w.size(); r++) dst->w[r] = (double)dst->Code(src->labels[(size_t)dst->w[r]]);
	}
}

// the group value of row i rendered to VARCHAR; false where it is NULL
struct GroupInput {
	GroupInput(Vector &v, idx_t count) : id(v.GetType().id()) {
		if (id != LogicalTypeId::VARCHAR && id != LogicalTypeId::BIGINT && id != LogicalTypeId::INTEGER)
			throw InvalidInputException("glmm: the group column must be VARCHAR, BIGINT or INTEGER, got %s", v.GetType().ToString().c_str());
		v.ToUnifiedFormat(count, data);
	}
	GroupInput(const GroupInput &) = delete;
	bool Read(idx_t i, string &label) const {
		const auto idx = data.sel->get_index(i);
		if (!data.validity.RowIsValid(idx)) return false;
		if (id == LogicalTypeId::VARCHAR) label = UnifiedVectorFormat::GetData<string_t>(data)[idx].GetString();
		else if (id == LogicalTypeId::BIGINT) label = std::to_string((long long)UnifiedVectorFormat::GetData<int64_t>(data)[idx]);
		else label = std::to_string((long long)UnifiedVectorFormat::GetData<int32_t>(data)[idx]);
		return true;
	}
	LogicalTypeId id;
	UnifiedVectorFormat data;
};

// Update, (y, x, group[, split][, options]).  PREDICT: a NULL y is a prediction row and a split column decides who trains.
template <bool PREDICT>
void GlmmUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 3) ThrowTooFewArguments("glmm aggregates");
	auto &bind = aggr_input_data.bind_data->Cast<HipGlmmBindData>();
	const bool split = PREDICT && bind.use_split_col && input_count > 3;
	RowsInput in(inputs, count, state_vector, false, split ? 3 : 0);
	GroupInput groups(inputs[2], count);
	string label;
	for (idx_t i = 0; i < count; i++) {
		double y = NAN;
		const bool y_valid = in.Y(i, y);
		const list_entry_t *entry = in.X(i);
		if (!entry || (!PREDICT && !y_valid) || !groups.Read(i, label)) continue;
		auto &rows = GlmmRowsOf(in.State(i), entry->length);
		in.AppendX(*entry, rows.x);
		PushRow(rows, y_valid ? y : NAN, y_valid, split ? in.SplitTrains(i) && y_valid : y_valid);
		rows.w.push_back((double)rows.Code(label));
	}
}

// the states of one Finalize vector as panels of one call per feature count: a state's rows sorted by level (stably)
struct GlmmBatch : RowBatch {
	vector<int64_t> plo {0}, lro {0}, level_n;
	vector<size_t> order; // order[sorted row] = the row's place in its buffer; offsets[g] is the panel's first sorted row
	vector<double> records, inference, ranef, pred;
	int64_t n = 0;
	void Run(const HipGlmmBindData &bind) {
		for (auto *b : buffers) n += (int64_t)b->Rows();
		y.resize((size_t)n);
		cols.resize((size_t)n * p);
		order.resize((size_t)n);
		int64_t at = 0;
		for (auto *b : buffers) {
			auto &rows = *static_cast<GlmmRows *>(b);
			const size_t m = rows.Rows(), L = rows.labels.size();
			vector<int64_t> first(L + 1, 0);
			for (size_t r = 0; r < m; r++) first[(size_t)rows.w[r] + 1]++;
			for (size_t l = 0; l < L; l++) first[l + 1] += first[l];
			for (size_t l = 0; l < L; l++) lro.push_back(at + first[l + 1]);
			vector<int64_t> next(first.begin(), first.end() - 1);
			for (size_t r = 0; r < m; r++) {
				const size_t to = (size_t)(at + next[(size_t)rows.w[r]]++);
				order[to] = r;
				y[to] = (rows.flags[r] & kTraining) ? rows.y[r] : NAN;
				for (idx_t j = 0; j < p; j++) cols[j * (size_t)n + to] = rows.x[r * p + j];
			}
			at += (int64_t)m;
			offsets.push_back(at);
			plo.push_back((int64_t)lro.size() - 1);
		}
		col_ptrs.resize(p);
		for (idx_t j = 0; j < p; j++) col_ptrs[j] = cols.data() + j * (size_t)n;
		const size_t G = Groups(), L = lro.size() - 1;
		records.resize(G * (p + 13));
		ranef.resize(L ? L : 1);
		level_n.resize(L ? L : 1);
		if (bind.opts.compute_inference) inference.resize(G * (5 * p + 1));
		double *inf = bind.opts.compute_inference ? inference.data() : nullptr;
		AnofoxError err;
		memset(&err, 0, sizeof err);
		bool ok;
		if (bind.kind == GlmmKind::PREDICT) {
			pred.resize((size_t)n * 5);
			ok = anofox_hip_glmm_fit_predict_batch_host(nullptr, (int64_t)G, (int64_t)L, p, n, plo.data(), lro.data(), y.data(), col_ptrs.data(),
			                                            bind.opts.Batch(), bind.opts.Predict(), records.data(), inf, ranef.data(), level_n.data(),
			                                            pred.data(), &err);
		} else {
			ok = anofox_hip_glmm_fit_batch_host(nullptr, (int64_t)G, (int64_t)L, p, n, plo.data(), lro.data(), y.data(), col_ptrs.data(),
			                                    bind.opts.Batch(), records.data(), inf, ranef.data(), level_n.data(), &err);
		}
		if (!ok) ThrowAbi(err);
	}
	const double *Record(idx_t g) const { return &records[g * (p + 13)]; }
	bool Failed(idx_t g) const { return Record(g)[p + 12] != 0.0; }
};

// a label into a VARCHAR vector: DuckDB's StringVector::AddString, or the stand-in's Vector::AddString
template <class V>
auto AddLabel(V &v, const string &s, int) -> decltype(v.AddString(s)) {
	return v.AddString(s);
}
template <class V, class SV = StringVector>
string_t AddLabel(V &v, const string &s, long) {
	return SV::AddString(v, s);
}

// =====================================================================================================================
// anofox_stats_glmm_fit_agg(y, x, group[, options]) -> STRUCT
// =====================================================================================================================
LogicalType GetHipGlmmResultType(bool compute_inference) { // the names, order and types of GetGlmmResultType, glmm_aggregate.cpp:156-199
	child_list_t<LogicalType> ranef;
	ranef.push_back(make_pair("group", LogicalType::VARCHAR));
	ranef.push_back(make_pair("intercept", LogicalType::DOUBLE));
	ranef.push_back(make_pair("se", LogicalType::DOUBLE));
	ranef.push_back(make_pair("n", LogicalType::BIGINT));
	child_list_t<LogicalType> children;
	children.push_back(make_pair("coefficients", LogicalType::LIST(LogicalType::DOUBLE)));
	for (auto *name : {"intercept", "var_group", "var_residual", "icc", "log_likelihood", "aic", "bic", "deviance"})
		children.push_back(make_pair(string(name), LogicalType(LogicalType::DOUBLE)));
	for (auto *name : {"n_observations", "n_groups", "n_features"}) children.push_back(make_pair(string(name), LogicalType(LogicalType::BIGINT)));
	children.push_back(make_pair("iterations", LogicalType::INTEGER));
	children.push_back(make_pair("converged", LogicalType::BOOLEAN));
	children.push_back(make_pair("random_cov", LogicalType::LIST(LogicalType::DOUBLE)));
	children.push_back(make_pair("random_dim", LogicalType::INTEGER));
	child_list_t<LogicalType> factor;
	factor.push_back(make_pair("n_levels", LogicalType::BIGINT));
	factor.push_back(make_pair("var", LogicalType::DOUBLE));
	children.push_back(make_pair("factors", LogicalType::LIST(LogicalType::STRUCT(std::move(factor)))));
	if (compute_inference) {
		for (auto *name : {"std_errors", "z_values", "p_values", "ci_lower", "ci_upper"})
			children.push_back(make_pair(string(name), LogicalType::LIST(LogicalType::DOUBLE)));
		children.push_back(make_pair("intercept_std_error", LogicalType::DOUBLE));
	}
	children.push_back(make_pair("ranef", LogicalType::LIST(LogicalType::STRUCT(std::move(ranef)))));
	return LogicalType::STRUCT(std::move(children));
}

void HipGlmmAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipGlmmBindData>();
	auto batches = CollectBatches<GlmmBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 1; });
	for (auto &kv : batches) kv.second.Run(bind);
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		const idx_t p = b.p;
		for (idx_t g = 0; g < b.Groups(); g++) {
			const idx_t r = b.result_rows[g];
			if (b.Failed(g)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const double *rec = b.Record(g); // b[p], intercept, var_group, var_residual, icc, ll, aic, bic, deviance, n, J, iterations, converged
			idx_t f = 0;
			AppendList(*fields[f++], r, rec, p);
			for (idx_t k = 0; k < 8; k++) FlatVector::GetData<double>(*fields[f++])[r] = rec[p + k];
			FlatVector::GetData<int64_t>(*fields[f++])[r] = (int64_t)rec[p + 8];
			FlatVector::GetData<int64_t>(*fields[f++])[r] = (int64_t)rec[p + 9];
			FlatVector::GetData<int64_t>(*fields[f++])[r] = (int64_t)p;
			FlatVector::GetData<int32_t>(*fields[f++])[r] = (int32_t)rec[p + 10];
			FlatVector::GetData<bool>(*fields[f++])[r] = rec[p + 11] != 0.0;
			AppendList(*fields[f++], r, rec + p + 1, 1); // random_cov = [var_group]
			FlatVector::GetData<int32_t>(*fields[f++])[r] = 1;
			AppendListEntry(*fields[f++], r, 0); // factors: none
			if (bind.opts.compute_inference) {
				const double *inf = &b.inference[g * (5 * p + 1)];
				for (idx_t k = 0; k < 5; k++) AppendList(*fields[f++], r, inf + k * p, p);
				FlatVector::GetData<double>(*fields[f++])[r] = inf[5 * p];
			}
			// ranef: the levels with a valid row, in first-seen order
			const auto &rows = *static_cast<const GlmmRows *>(b.buffers[g]);
			const int64_t l0 = b.plo[g], l1 = b.plo[g + 1];
			idx_t kept = 0;
			for (int64_t l = l0; l < l1; l++) kept += b.level_n[(size_t)l] > 0;
			Vector &ranef = *fields[f];
			idx_t at = AppendListEntry(ranef, r, kept);
			auto &rf = StructVector::GetEntries(ListVector::GetEntry(ranef));
			for (int64_t l = l0; l < l1; l++) {
				if (b.level_n[(size_t)l] <= 0) continue;
				FlatVector::GetData<string_t>(*rf[0])[at] = AddLabel(*rf[0], rows.labels[(size_t)(l - l0)], 0);
				FlatVector::GetData<double>(*rf[1])[at] = b.ranef[(size_t)l];
				FlatVector::GetData<double>(*rf[2])[at] = NAN; // ranef_se is not built
				FlatVector::GetData<int64_t>(*rf[3])[at] = b.level_n[(size_t)l];
				at++;
			}
		}
	}
}

// =====================================================================================================================
// anofox_stats_glmm_fit_predict_agg(y, x, group[, split][, options])
//   -> LIST(STRUCT(y, yhat, yhat_fixed, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
LogicalType GlmmPredictResultType() {
	child_list_t<LogicalType> row;
	for (auto *name : {"y", "yhat", "yhat_fixed", "yhat_lower", "yhat_upper"}) row.push_back(make_pair(string(name), LogicalType(LogicalType::DOUBLE)));
	row.push_back(make_pair("is_training", LogicalType::BOOLEAN));
	return LogicalType::LIST(LogicalType::STRUCT(std::move(row)));
}

void HipGlmmPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipGlmmBindData>();
	auto batches = CollectBatches<GlmmBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 1; });
	for (auto &kv : batches) kv.second.Run(bind);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			if (b.Failed(g)) {
				FlatVector::SetNull(result, b.result_rows[g], true);
				continue;
			}
			const RowBuffer &rows = *b.buffers[g];
			const idx_t n_rows = rows.Rows(), list_offset = AppendListEntry(result, b.result_rows[g], n_rows);
			auto &fields = StructVector::GetEntries(ListVector::GetEntry(result));
			for (idx_t s = 0; s < n_rows; s++) { // s: the sorted place; the row goes back to its arrival place
				const size_t from = (size_t)b.offsets[g] + s;
				const idx_t r = b.order[from], at = list_offset + r;
				const double *pred = &b.pred[from * 5]; // yhat, yhat_fixed, se, lower, upper
				SetDoubleOrNull(*fields[0], at, rows.y[r], (rows.flags[r] & kYNull) != 0);
				SetDoubleOrNull(*fields[1], at, pred[0], !isfinite(pred[0]));
				SetDoubleOrNull(*fields[2], at, pred[1], !isfinite(pred[1]));
				SetDoubleOrNull(*fields[3], at, pred[3], !isfinite(pred[3]));
				SetDoubleOrNull(*fields[4], at, pred[4], !isfinite(pred[4]));
				FlatVector::GetData<bool>(*fields[5])[at] = (rows.flags[r] & kTraining) != 0;
			}
		}
	}
}

template <GlmmKind KIND, bool SPLIT>
unique_ptr<FunctionData> HipGlmmBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipGlmmOptions>(
	    context, function, arguments, SPLIT ? 4 : 3, SPLIT, [](const Value &v, HipGlmmOptions &o) { ParseHipGlmmOptions(v, KIND, o); },
	    [](const HipGlmmOptions &o) { return KIND == GlmmKind::PREDICT ? GlmmPredictResultType() : GetHipGlmmResultType(o.compute_inference); }, KIND);
}

AggregateFunction GlmmFunction(const string &fname, const vector<LogicalType> &args, aggregate_update_t update, aggregate_finalize_t finalize,
                               bind_aggregate_function_t bind) {
	return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>, RowsInitialize, update, GlmmCombine,
	                         finalize, nullptr, bind, GlmmDestroy);
}

} // namespace

void RegisterGlmmFamilyHip(ExtensionLoader &loader) {
	RowsFunctionNames fit {"anofox_stats_glmm_fit_agg", "glmm_fit_agg", {},
	                       "Fits a Gaussian linear mixed model with one random intercept per group level, by profiled REML or ML.", kCategories};
	fit.base = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	fit.base_names = {"y", "x", "group"};
	RegisterWithOptions(loader, fit, "{'reml': true, 'compute_inference': true}", [](const string &fname, const vector<LogicalType> &args) {
		return GlmmFunction(fname, args, GlmmUpdate<false>, HipGlmmAggFinalize, HipGlmmBind<GlmmKind::FIT, false>);
	});
	RowsFunctionNames predict {"anofox_stats_glmm_fit_predict_agg", "glmm_fit_predict_agg", {},
	                           "Fits a Gaussian random-intercept mixed model and scores every row: the prediction with the level's BLUP, the "
	                           "population prediction and a confidence or prediction interval.",
	                           kCategories};
	predict.base = fit.base;
	predict.base_names = fit.base_names;
	RegisterWithSplitAndOptions(loader, predict, "{'interval': 'prediction', 'level': 0.9}", "{'interval': 'prediction', 'level': 0.9}",
	                            [](const string &fname, const vector<LogicalType> &args, bool split) {
		                            return GlmmFunction(fname, args, GlmmUpdate<true>, HipGlmmPredictAggFinalize,
		                                                split ? HipGlmmBind<GlmmKind::PREDICT, true> : HipGlmmBind<GlmmKind::PREDICT, false>);
	                            });
}

} // namespace duckdb
