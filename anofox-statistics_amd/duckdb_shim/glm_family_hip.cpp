// glm_family_hip.cpp — DuckDB glue of the generalised linear models over the batched C ABI:
//
//   anofox_stats_poisson_fit_agg          src/aggregate_functions/poisson_aggregate.cpp (bind data :54-86, result type :91-115,
//                                         Update :149-218, Combine :220-267, Finalize :280-367, bind :372-409)
//   anofox_stats_binomial_fit_agg         src/aggregate_functions/binomial_aggregate.cpp (result type :101-118, the same mechanics)
//   anofox_stats_logistic_fit_agg         src/aggregate_functions/logistic_aggregate.cpp (result type :89-107: accuracy and
//                                         threshold in place of dispersion; bind :350-387)
//   anofox_stats_poisson_fit_predict_agg  src/aggregate_functions/poisson_fit_predict_aggregate.cpp (bind data :63-93, result type
//                                         :98-108, GetTCritical :140-164, Update :186-306, Finalize :365-517, binds :522-590)
//
// As the other glue files: the DuckDB state buffers the group's rows on the host in arrival order, Combine appends the
// source's rows after the target's, and Finalize turns the whole vector of states into ONE batched call per feature count
// where the reference makes one anofox_*_fit call per group: anofox_hip_glm_fit_batch_host (poisson, binomial),
// anofox_hip_glm_fit_accuracy_batch_host (logistic: the wavefront that fitted the group counts its accuracy, no per-row
// prediction crosses the bus) and anofox_hip_glm_fit_predict_interval_batch_host (fit-predict: mu and the reference's
// interval from the lane that holds the row).  The glue adds no arithmetic: every number of a result is the library's.
//
// Options (RegressionMapOptions::ParseFromValue, map_options_parser.cpp:637-780), STRUCT or MAP literal, keys case-insensitive,
// unknown keys ignored, options that are not constant keep the defaults: fit_intercept / intercept, compute_inference /
// inference, confidence_level / confidence, link / poisson_link, binomial_link, max_iterations / max_iter, tolerance / tol,
// glm_lambda, threshold, offset, null_policy, prior / priors.  Each function reads what its reference bind reads:
//   poisson_fit_agg          all but binomial_link, threshold, null_policy
//   binomial_fit_agg         all but link / poisson_link, threshold, null_policy
//   logistic_fit_agg         all but both links and null_policy; threshold
//   poisson_fit_predict_agg  fit_intercept, link, max_iterations, tolerance, confidence_level, glm_lambda, null_policy — NOT
//                            offset, compute_inference or priors, which its reference bind does not read either (:527-550)
// A link that the library does not fit (anything but log / logit) and any prior raise at bind with the library's "glm: ... is
// not built" text in the functions that read them; a silent NULL would hide that the model asked for was not the one fitted.
// offset = j takes the 1-based x column j out of the features and passes it as the offset; n_features in the result is the
// number of columns handed to the fit.  An out-of-range j raises the reference's text (glm_engine/design.rs:192) from
// Finalize, where the feature count is known.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU
// with the real library (tests/test_gpu_glm_glue.py through tests/tools/glm_family_capi.cpp).
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
#include "glm_family_hip.hpp"
#include "hip_options.hpp"
#include "row_glue.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "glm"};

enum class GlmKind : uint8_t { POISSON, BINOMIAL, LOGISTIC, POISSON_PREDICT };

// ---- options ----
struct HipGlmOptions {
	bool fit_intercept = true;       // poisson_aggregate.cpp:56
	uint32_t max_iterations = 100;   // :58
	double tolerance = 1e-8;         // :59
	bool compute_inference = false;  // :60
	double confidence_level = 0.95;  // :61
	double glm_lambda = 0.0;         // :62
	idx_t offset_column = 0;         // :63, 1-based, 0 = none
	double threshold = 0.5;          // logistic_aggregate.cpp:56
	bool drop_y_zero_x = false;      // poisson_fit_predict_aggregate.cpp:70
	bool operator==(const HipGlmOptions &o) const {
		return fit_intercept == o.fit_intercept && max_iterations == o.max_iterations && tolerance == o.tolerance &&
		       compute_inference == o.compute_inference && confidence_level == o.confidence_level && glm_lambda == o.glm_lambda &&
		       offset_column == o.offset_column && threshold == o.threshold && drop_y_zero_x == o.drop_y_zero_x;
	}
	AnofoxHipGlmBatchOptions Batch(GlmKind kind) const {
		AnofoxHipGlmBatchOptions b;
		memset(&b, 0, sizeof b);
		b.family = kind == GlmKind::POISSON || kind == GlmKind::POISSON_PREDICT ? ANOFOX_HIP_GLM_POISSON : ANOFOX_HIP_GLM_BINOMIAL;
		b.fit_intercept = fit_intercept;
		b.max_iterations = max_iterations;
		b.tolerance = tolerance;
		b.lambda = glm_lambda;
		b.compute_inference = compute_inference;
		b.confidence_level = confidence_level;
		return b;
	}
};

// ExtractPoissonLink / ExtractBinomialLink (map_options_parser.cpp:96-127): an unknown name is the parser's error whichever
// function is bound; returns the lower-cased name
string ExtractLink(const Value &v, const char *family, std::initializer_list<const char *> valid, const char *valid_text) {
	const string s = OptionString(v);
	for (auto *name : valid)
		if (s == name) return s;
	throw InvalidInputException("Invalid %s link: '%s'. Valid values are %s", family, s.c_str(), valid_text);
}

void ParseHipGlmOptions(const Value &v, GlmKind kind, HipGlmOptions &o) {
	if (v.IsNull()) return;
	const bool predict = kind == GlmKind::POISSON_PREDICT;
	string poisson_link = "log", binomial_link = "logit";
	bool has_prior = false;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (val.IsNull()) return;
		if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(val);
		else if (key == "compute_inference" || key == "inference") {
			const bool b = ExtractBool(val);
			if (!predict) o.compute_inference = b;
		} else if (key == "confidence_level" || key == "confidence") o.confidence_level = val.GetValue<double>();
		else if (key == "max_iterations" || key == "max_iter") o.max_iterations = ExtractUInteger(val);
		else if (key == "tolerance" || key == "tol") o.tolerance = val.GetValue<double>();
		else if (key == "glm_lambda") o.glm_lambda = val.GetValue<double>();
		else if (key == "threshold") {
			const double t = val.GetValue<double>();
			if (kind == GlmKind::LOGISTIC) o.threshold = t;
		} else if (key == "offset") {
			const uint32_t j = ExtractUInteger(val);
			if (!predict) o.offset_column = j;
		} else if (key == "null_policy") {
			const bool drop = ExtractNullPolicy(val);
			if (predict) o.drop_y_zero_x = drop;
		} else if (key == "link" || key == "poisson_link") poisson_link = ExtractLink(val, "poisson", {"log", "identity", "sqrt"}, "'log', 'identity', 'sqrt'");
		else if (key == "binomial_link") binomial_link = ExtractLink(val, "binomial", {"logit", "probit", "cloglog"}, "'logit', 'probit', 'cloglog'");
		else if (key == "prior" || key == "priors") has_prior = true;
		// every other key: ignored, as upstream (:798)
	});
	if ((kind == GlmKind::POISSON || predict) && poisson_link != "log") throw InvalidInputException("glm: link %s is not built", poisson_link.c_str());
	if (kind == GlmKind::BINOMIAL && binomial_link != "logit") throw InvalidInputException("glm: link %s is not built", binomial_link.c_str());
	if (!predict && has_prior) throw InvalidInputException("glm: priors are not built");
}

// GetTCritical (poisson_fit_predict_aggregate.cpp:140-164): a three-entry table of normal quantiles, 1.96 for anything else
double IntervalZ(double confidence_level) {
	if (fabs(confidence_level - 0.95) < 0.001) return 1.96;
	if (fabs(confidence_level - 0.99) < 0.001) return 2.576;
	if (fabs(confidence_level - 0.90) < 0.001) return 1.645;
	return 1.96;
}

struct HipGlmBindData : public FunctionData {
	HipGlmBindData(GlmKind kind_p, const HipGlmOptions &opts_p, bool use_split_col_p) : kind(kind_p), opts(opts_p), use_split_col(use_split_col_p) {}
	GlmKind kind;
	HipGlmOptions opts;
	bool use_split_col;
	unique_ptr<FunctionData> Copy() const override { return make_uniq<HipGlmBindData>(kind, opts, use_split_col); }
	bool Equals(const FunctionData &other_p) const override {
		auto &other = other_p.Cast<HipGlmBindData>();
		return kind == other.kind && opts == other.opts && use_split_col == other.use_split_col;
	}
};

// Update.  PREDICT = false (poisson_aggregate.cpp:149-218 and its twins): a row with a NULL y or a NULL x list is skipped, every
// other row is buffered, a NULL list element as NaN.  PREDICT = true (poisson_fit_predict_aggregate.cpp:186-306): every row with
// a non-NULL x list is kept for the output; it trains iff its y is not NULL — and, with a split column, its split value is not
// NULL and says train — and, under null_policy = 'drop_y_zero_x', no x element is exactly 0 (:283-290).
template <bool PREDICT>
void HipGlmRowsUpdate(Vector inputs[], AggregateInputData &aggr_input_data, idx_t input_count, Vector &state_vector, idx_t count) {
	auto &bind = aggr_input_data.bind_data->Cast<HipGlmBindData>();
	if (input_count < 2) throw InvalidInputException("anofox_stats glm aggregates (HIP): too few arguments");
	UnifiedVectorFormat y_data, x_data, split_data, sdata;
	inputs[0].ToUnifiedFormat(count, y_data);
	inputs[1].ToUnifiedFormat(count, x_data);
	auto y_values = UnifiedVectorFormat::GetData<double>(y_data);
	auto x_list = UnifiedVectorFormat::GetData<list_entry_t>(x_data);
	auto &x_child = ListVector::GetEntry(inputs[1]);
	auto x_child_data = FlatVector::GetData<double>(x_child);
	auto &x_child_validity = FlatVector::Validity(x_child);
	const string_t *split_values = nullptr;
	if (PREDICT && bind.use_split_col && input_count > 2) {
		inputs[2].ToUnifiedFormat(count, split_data);
		split_values = UnifiedVectorFormat::GetData<string_t>(split_data);
	}
	state_vector.ToUnifiedFormat(count, sdata);
	auto states = (RowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		auto &state = *states[sdata.sel->get_index(i)];
		auto y_idx = y_data.sel->get_index(i);
		const bool y_valid = y_data.validity.RowIsValid(y_idx);
		if (!PREDICT && !y_valid) continue;
		auto x_idx = x_data.sel->get_index(i);
		if (!x_data.validity.RowIsValid(x_idx)) continue;
		const auto entry = x_list[x_idx];
		auto &rows = RowsOf(state, entry.length, true);
		const size_t at = rows.x.size();
		rows.x.resize(at + entry.length);
		const ListRowFlags f = ReadListRow(entry, x_child_data, x_child_validity, rows.x.data() + at); // never reads the slot of a NULL
		bool training = y_valid;
		if (split_values) {
			auto s_idx = split_data.sel->get_index(i);
			training = split_data.validity.RowIsValid(s_idx) && IsSplitTraining(split_values[s_idx]) && y_valid;
		}
		if (PREDICT && bind.opts.drop_y_zero_x && f.has_zero) training = false;
		rows.y.push_back(y_valid ? y_values[y_idx] : NAN);
		rows.flags.push_back((uint8_t)((y_valid ? 0 : kYNull) | (training ? kTraining : 0)));
		rows.n_training += training ? 1 : 0;
	}
}

// the states of one Finalize vector as one batch per feature count (RowBatch) through the family's ABI calls
struct GlmBatch : RowBatch {
	vector<double> records, inference, accuracy, pred;
	vector<const double *> features; // the columns handed to the fit: all of them, or all but the offset column
	idx_t q = 0;                     // their count: n_features of the result
	const double *offset = nullptr;
	int64_t n = 0;
	// offset_column: 1-based into the x list (0 = none); out of range: the reference's text (glm_engine/design.rs:192)
	void StageFit(idx_t offset_column) {
		if (offset_column > p)
			throw InvalidInputException("offset must be a 1-based index into x (1..=%llu), got %llu", (unsigned long long)p, (unsigned long long)offset_column);
		n = Stage(false, false);
		for (idx_t j = 0; j < p; j++) {
			if (j + 1 == offset_column) offset = col_ptrs[j];
			else features.push_back(col_ptrs[j]);
		}
		q = features.size();
		records.resize(Groups() * (q + 11));
	}
	// records [G x (q + 11)], inference [G x 5 q] with compute_inference, accuracy [G] for the logistic fit
	void RunFit(const HipGlmBindData &bind) {
		StageFit(bind.opts.offset_column);
		if (bind.opts.compute_inference) inference.resize(Groups() * 5 * q);
		double *inf = bind.opts.compute_inference ? inference.data() : nullptr;
		AnofoxError err;
		memset(&err, 0, sizeof err);
		bool ok;
		if (bind.kind == GlmKind::LOGISTIC) {
			accuracy.resize(Groups());
			ok = anofox_hip_glm_fit_accuracy_batch_host(nullptr, (int64_t)Groups(), q, n, offsets.data(), y.data(), features.data(), offset,
			                                            bind.opts.Batch(bind.kind), bind.opts.threshold, records.data(), inf, accuracy.data(), &err);
		} else {
			ok = anofox_hip_glm_fit_batch_host(nullptr, (int64_t)Groups(), q, n, offsets.data(), y.data(), features.data(), offset,
			                                   bind.opts.Batch(bind.kind), records.data(), inf, &err);
		}
		if (!ok) ThrowAbi(err);
	}
	// records as above, pred [n x 3] = {mu, lower, upper}; rows that do not train reach the ABI with y = NaN, and the count of
	// the rows that train (a NaN y that is not NULL included, :376) goes as train_counts so that the reference's rule decides
	void RunPredict(const HipGlmBindData &bind) {
		StageFit(0);
		pred.resize((size_t)n * 3);
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_glm_fit_predict_interval_batch_host(nullptr, (int64_t)Groups(), q, n, offsets.data(), y.data(), features.data(), nullptr,
		                                                    train_counts.data(), bind.opts.Batch(bind.kind), IntervalZ(bind.opts.confidence_level),
		                                                    records.data(), pred.data(), &err))
			ThrowAbi(err);
	}
	const double *Record(idx_t g) const { return &records[g * (q + 11)]; }
	bool Failed(idx_t g) const { return Record(g)[q + 10] != 0.0; }
};

// =====================================================================================================================
// anofox_stats_{poisson,binomial,logistic}_fit_agg(y, x[, options]) -> STRUCT
// =====================================================================================================================
LogicalType GetHipGlmAggResultType(GlmKind kind, bool compute_inference) { // poisson :91-115, binomial :101-118, logistic :89-107
	child_list_t<LogicalType> children;
	children.push_back(make_pair("coefficients", LogicalType::LIST(LogicalType::DOUBLE)));
	children.push_back(make_pair("intercept", LogicalType::DOUBLE));
	children.push_back(make_pair("deviance", LogicalType::DOUBLE));
	children.push_back(make_pair("null_deviance", LogicalType::DOUBLE));
	children.push_back(make_pair("pseudo_r_squared", LogicalType::DOUBLE));
	children.push_back(make_pair("aic", LogicalType::DOUBLE));
	if (kind == GlmKind::LOGISTIC) {
		children.push_back(make_pair("accuracy", LogicalType::DOUBLE));
		children.push_back(make_pair("threshold", LogicalType::DOUBLE));
	} else {
		children.push_back(make_pair("dispersion", LogicalType::DOUBLE));
	}
	children.push_back(make_pair("n_observations", LogicalType::BIGINT));
	children.push_back(make_pair("n_features", LogicalType::BIGINT));
	children.push_back(make_pair("iterations", LogicalType::INTEGER));
	children.push_back(make_pair("converged", LogicalType::BOOLEAN));
	if (compute_inference) {
		children.push_back(make_pair("std_errors", LogicalType::LIST(LogicalType::DOUBLE)));
		children.push_back(make_pair("z_values", LogicalType::LIST(LogicalType::DOUBLE)));
		children.push_back(make_pair("p_values", LogicalType::LIST(LogicalType::DOUBLE)));
		children.push_back(make_pair("ci_lower", LogicalType::LIST(LogicalType::DOUBLE)));
		children.push_back(make_pair("ci_upper", LogicalType::LIST(LogicalType::DOUBLE)));
	}
	return LogicalType::STRUCT(std::move(children));
}

// Finalize (:280-367): NULL for a state no row reached, fewer than 2 buffered rows (:292 counts rows, not finite rows) or a
// failed fit (:331-334); otherwise the record's fields in the result type's order
void HipGlmAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipGlmBindData>();
	auto batches = CollectBatches<GlmBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 2; });
	for (auto &kv : batches) kv.second.RunFit(bind);
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		const idx_t q = b.q;
		for (idx_t g = 0; g < b.Groups(); g++) {
			const idx_t r = b.result_rows[g];
			if (b.Failed(g)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const double *rec = b.Record(g); // coefficients[q], intercept, deviance, null_deviance, pseudo_r_squared, aic, dispersion, n_observations, ...
			idx_t f = 0;
			AppendList(*fields[f++], r, rec, q);
			for (idx_t k = 0; k < 5; k++) FlatVector::GetData<double>(*fields[f++])[r] = rec[q + k];
			if (bind.kind == GlmKind::LOGISTIC) {
				FlatVector::GetData<double>(*fields[f++])[r] = b.accuracy[g];
				FlatVector::GetData<double>(*fields[f++])[r] = bind.opts.threshold;
			} else {
				FlatVector::GetData<double>(*fields[f++])[r] = rec[q + 5];
			}
			FlatVector::GetData<int64_t>(*fields[f++])[r] = (int64_t)rec[q + 6];
			FlatVector::GetData<int64_t>(*fields[f++])[r] = (int64_t)q;
			FlatVector::GetData<int32_t>(*fields[f++])[r] = (int32_t)rec[q + 8];
			FlatVector::GetData<bool>(*fields[f++])[r] = rec[q + 9] != 0.0;
			if (bind.opts.compute_inference)
				for (idx_t k = 0; k < 5; k++) AppendList(*fields[f++], r, &b.inference[(g * 5 + k) * q], q);
		}
	}
}

template <GlmKind KIND>
unique_ptr<FunctionData> HipGlmAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipGlmOptions opts;
	if (arguments.size() > 2 && arguments[2]->IsFoldable()) ParseHipGlmOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[2]), KIND, opts);
	function.return_type = GetHipGlmAggResultType(KIND, opts.compute_inference);
	return make_uniq<HipGlmBindData>(KIND, opts, false);
}

template <GlmKind KIND>
void RegisterHipGlmAgg(ExtensionLoader &loader, const char *name, const char *alias, const char *what, const char *example_options) {
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	auto fill = [&](const string &fname) {
		AggregateFunctionSet set(fname);
		for (auto *args : {&basic, &map_args})
			set.AddFunction(AggregateFunction(fname, *args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>, RowsInitialize,
			                                  HipGlmRowsUpdate<false>, RowsCombine<false, true>, HipGlmAggFinalize, nullptr, HipGlmAggBind<KIND>, RowsDestroy));
		return set;
	};
	CreateAggregateFunctionInfo info(fill(name));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x)", {"y", "x"}, basic, kCategories));
	info.descriptions.push_back(Describe(what, string(name) + "(y, x, " + example_options + ")", {"y", "x", "options"}, map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill(alias));
}

// =====================================================================================================================
// anofox_stats_poisson_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Finalize (:365-517): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with mu and the
// interval (three NULLs where mu is not finite :498-508, y NULL where the input was :447-451)
void HipGlmPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipGlmBindData>();
	auto batches = CollectBatches<GlmBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; });
	for (auto &kv : batches) kv.second.RunPredict(bind);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			if (b.Failed(g)) FlatVector::SetNull(result, b.result_rows[g], true);
			else AppendPredictRows(result, b.result_rows[g], *b.buffers[g], &b.pred[(size_t)b.offsets[g] * 3]);
		}
	}
}

template <bool SPLIT>
unique_ptr<FunctionData> HipGlmPredictAggBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	HipGlmOptions opts;
	const idx_t opt_idx = SPLIT ? 3 : 2;
	if (arguments.size() > opt_idx && arguments[opt_idx]->IsFoldable())
		ParseHipGlmOptions(ExpressionExecutor::EvaluateScalar(context, *arguments[opt_idx]), GlmKind::POISSON_PREDICT, opts);
	function.return_type = PredictAggResultType();
	return make_uniq<HipGlmBindData>(GlmKind::POISSON_PREDICT, opts, SPLIT);
}

} // namespace

void RegisterHipPoissonAggregateFunction(ExtensionLoader &loader) {
	RegisterHipGlmAgg<GlmKind::POISSON>(loader, "anofox_stats_poisson_fit_agg", "poisson_fit_agg",
	                                    "Fits a Poisson regression (log link) per group for count data.", "{'fit_intercept': true, 'offset': 2}");
}

void RegisterHipBinomialAggregateFunction(ExtensionLoader &loader) {
	RegisterHipGlmAgg<GlmKind::BINOMIAL>(loader, "anofox_stats_binomial_fit_agg", "binomial_fit_agg",
	                                     "Fits a binomial regression (logit link) per group for a response in [0, 1].",
	                                     "{'binomial_link': 'logit', 'fit_intercept': true}");
}

void RegisterHipLogisticAggregateFunction(ExtensionLoader &loader) {
	RegisterHipGlmAgg<GlmKind::LOGISTIC>(loader, "anofox_stats_logistic_fit_agg", "logistic_fit_agg",
	                                     "Fits a logistic regression per group for a 0 / 1 response, with the training accuracy at the threshold.",
	                                     "{'glm_lambda': 0.1, 'threshold': 0.5}");
}

void RegisterHipPoissonFitPredictAggregateFunction(ExtensionLoader &loader) {
	const char *name = "anofox_stats_poisson_fit_predict_agg";
	const char *what = "Fits a Poisson regression over a partition and returns per-row predictions with an interval.";
	const vector<LogicalType> basic = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
	const vector<LogicalType> map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
	const vector<LogicalType> split_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR};
	const vector<LogicalType> split_map_args = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::VARCHAR, LogicalType::ANY};
	auto make = [](const string &fname, const vector<LogicalType> &args, bool split) {
		return AggregateFunction(fname, args, LogicalType::ANY /* set in bind */, AggregateFunction::StateSize<RowsState>, RowsInitialize,
		                         HipGlmRowsUpdate<true>, RowsCombine<false, true>, HipGlmPredictAggFinalize, nullptr,
		                         split ? HipGlmPredictAggBind<true> : HipGlmPredictAggBind<false>, RowsDestroy);
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
	info.descriptions.push_back(Describe(what, head + ", {'confidence_level': 0.99})", {"y", "x", "options"}, map_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col)", {"y", "x", "split_col"}, split_args, kCategories));
	info.descriptions.push_back(Describe(what, head + ", split_col, {'confidence_level': 0.99})", {"y", "x", "split_col", "options"}, split_map_args, kCategories));
	RegisterWithAlias(loader, std::move(info), fill("poisson_fit_predict_agg"));
}

} // namespace duckdb
