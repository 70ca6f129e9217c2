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
#include "row_shapes.hpp"

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

using HipGlmBindData = RowsBindData<HipGlmOptions, GlmKind>;

// Update.  The fit aggregates: poisson_aggregate.cpp:149-218 and its twins.  The predict aggregate: poisson_fit_predict_aggregate.cpp
// :186-306, drop_y_zero_x :283-290.  Neither checks the width (the library's call reports it), RowsOf's text has the counts, and
// every function of the family goes by one name in "too few arguments".
struct GlmTraits : RowTraits {
	using Bind = HipGlmBindData;
	static constexpr const char *kName = "glm aggregates";
	static constexpr bool kCheckMaxFeatures = false;
	static constexpr bool kCountsInError = true;
	static bool DropYZeroX(const Bind &bind) { return bind.opts.drop_y_zero_x; } // (the predict aggregate; the fit aggregates never read it)
};

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

// the fit aggregates' result type depends on compute_inference; SPLIT: the predict aggregate behind a split column
template <GlmKind KIND, bool SPLIT>
unique_ptr<FunctionData> HipGlmBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipGlmOptions>(
	    context, function, arguments, SPLIT ? 3 : 2, SPLIT, [](const Value &v, HipGlmOptions &o) { ParseHipGlmOptions(v, KIND, o); },
	    [](const HipGlmOptions &o) { return KIND == GlmKind::POISSON_PREDICT ? PredictAggResultType() : GetHipGlmAggResultType(KIND, o.compute_inference); }, KIND);
}

template <GlmKind KIND>
void RegisterHipGlmAgg(ExtensionLoader &loader, const char *name, const char *alias, const char *what, const char *example_options) {
	const RowsFunctionNames f {name, alias, {}, what, kCategories};
	RegisterWithOptions(loader, f, example_options, [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsFitAggUpdate<GlmTraits>, RowsCombine<false, true>, HipGlmAggFinalize,
		                    HipGlmBind<KIND, false>);
	});
}

// =====================================================================================================================
// anofox_stats_poisson_fit_predict_agg(y, x[, split_col][, options]) -> LIST(STRUCT(y, yhat, yhat_lower, yhat_upper, is_training))
// =====================================================================================================================
// Finalize (:365-517): NULL with fewer than 2 training rows or a failed fit; otherwise every buffered row with mu and the
// interval (three NULLs where mu is not finite :498-508, y NULL where the input was :447-451)
void HipGlmPredictAggFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipGlmBindData>();
	FinalizePredictRows<GlmBatch>(
	    state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.n_training >= 2; }, [&](GlmBatch &b) { b.RunPredict(bind); });
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
	const RowsFunctionNames f {"anofox_stats_poisson_fit_predict_agg", "poisson_fit_predict_agg", {},
	                           "Fits a Poisson regression over a partition and returns per-row predictions with an interval.", kCategories};
	RegisterWithSplitAndOptions(loader, f, "{'confidence_level': 0.99}", "{'confidence_level': 0.99}", [](const string &fname, const vector<LogicalType> &args, bool split) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, RowsPredictAggUpdate<GlmTraits>, RowsCombine<false, true>, HipGlmPredictAggFinalize,
		                    split ? HipGlmBind<GlmKind::POISSON_PREDICT, true> : HipGlmBind<GlmKind::POISSON_PREDICT, false>);
	});
}

} // namespace duckdb
