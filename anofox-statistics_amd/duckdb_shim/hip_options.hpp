// hip_options.hpp — the options argument of the regression aggregates as the reference's parser reads it, shared by every
// DuckDB glue file of this directory: the STRUCT / MAP walk, the value converters with the reference's error texts, and the
// option sets more than one file reads (ols / ridge / wls: fit_agg_hip.cpp, family_agg_hip.cpp; the elastic net:
// elasticnet_agg_hip.cpp, elasticnet_family_hip.cpp, and rls_family_hip.cpp for the keys it converts and ignores).
// bls_family_hip.cpp and quantile_family_hip.cpp keep their own option sets and parse them with the same pieces.
#pragma once
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cctype>
#include <initializer_list>
#include <utility>

#include "duckdb.hpp"

#include "anofox_stats_hip.h"

namespace duckdb {
namespace hip_glue {

enum class HipModel : uint8_t { OLS, RIDGE, WLS };

// ---- options: the keys, aliases, defaults and error texts of the reference's parser ----
// (RegressionMapOptions::ParseFromValue src/include/map_options_parser.cpp:637-750, ExtractBool :21-45,
//  ExtractSolverType / ExtractHcType / ExtractLambdaScaling :222-266, VisitOptionEntries :343-373 — STRUCT and MAP
//  literals, lower-cased keys, unknown keys ignored :798 — GetRegularizationStrength map_options_parser.hpp:265-270;
//  defaults ols_aggregate.cpp:48-52, ridge_aggregate.cpp:49-54, wls_aggregate.cpp:49-54)
struct HipFitOptions {
	bool fit_intercept = true;
	bool compute_inference = false;
	double confidence_level = 0.95;
	AnofoxSolverType solver = ANOFOX_SOLVER_SVD; // accepted; the GPU path has one solver (results agree within 1e-10)
	AnofoxHcType hc_type = ANOFOX_HC_NONE;
	double alpha = 1.0;
	AnofoxLambdaScaling lambda_scaling = ANOFOX_LAMBDA_SCALING_RAW;
	bool drop_y_zero_x = false; // null_policy = 'drop_y_zero_x': read by the predict aggregates only (ols_predict_aggregate.cpp:241-249)
	bool operator==(const HipFitOptions &o) const {
		return fit_intercept == o.fit_intercept && compute_inference == o.compute_inference && confidence_level == o.confidence_level &&
		       solver == o.solver && hc_type == o.hc_type && alpha == o.alpha && lambda_scaling == o.lambda_scaling && drop_y_zero_x == o.drop_y_zero_x;
	}
};

inline string Lower(string s) {
	std::transform(s.begin(), s.end(), s.begin(), [](unsigned char c) { return (char)std::tolower(c); });
	return s;
}

inline bool ExtractBool(const Value &v) {
	switch (v.type().id()) {
	case LogicalTypeId::BOOLEAN: return BooleanValue::Get(v);
	case LogicalTypeId::INTEGER:
	case LogicalTypeId::BIGINT: return v.GetValue<int64_t>() != 0;
	case LogicalTypeId::DOUBLE: return v.GetValue<double>() != 0.0;
	default: throw InvalidInputException("Cannot convert value of type %s to boolean", v.type().ToString().c_str());
	}
}

inline string OptionString(const Value &v) { return Lower(v.type().id() == LogicalTypeId::VARCHAR ? StringValue::Get(v) : v.ToString()); }

template <class ENUM>
ENUM ExtractEnum(const Value &v, const char *what, const char *valid, std::initializer_list<std::pair<const char *, ENUM>> table) {
	const string s = OptionString(v);
	for (auto &e : table)
		if (s == e.first) return e.second;
	throw InvalidInputException("Invalid %s: '%s'. Valid values are %s", what, s.c_str(), valid);
}

inline AnofoxLambdaScaling ExtractLambdaScaling(const Value &v) {
	return ExtractEnum<AnofoxLambdaScaling>(v, "lambda_scaling", "'raw', 'glmnet'", {{"raw", ANOFOX_LAMBDA_SCALING_RAW}, {"glmnet", ANOFOX_LAMBDA_SCALING_GLMNET}});
}

inline uint32_t ExtractUInteger(const Value &v) { // max_iterations: the reference's cast to UINTEGER
	const double d = v.GetValue<double>();
	if (!(d >= 0.0 && d <= 4294967295.0)) throw InvalidInputException("Value %s is out of range for UINTEGER", v.ToString().c_str());
	return (uint32_t)d;
}

// null_policy (ExtractNullPolicy map_options_parser.cpp:80-93): true for 'drop_y_zero_x', false for 'drop'; every aggregate
// validates it, the predict ones use it
inline bool ExtractNullPolicy(const Value &v) {
	const string s = OptionString(v);
	if (s != "drop" && s != "drop_y_zero_x") throw InvalidInputException("Invalid null_policy: '%s'. Valid values are 'drop', 'drop_y_zero_x'", s.c_str());
	return s == "drop_y_zero_x";
}

// The entries of a STRUCT or MAP literal as visit(lower-cased key, value), in the literal's order (VisitOptionEntries
// map_options_parser.cpp:343-373).  A NULL value is handed on: most keys ignore it, the quantile path's `tau` does not.
template <class F>
void VisitOptionEntries(const Value &v, F &&visit) {
	if (v.type().id() == LogicalTypeId::STRUCT) {
		auto &kids = StructValue::GetChildren(v);
		for (idx_t i = 0; i < kids.size(); i++) visit(Lower(StructType::GetChildName(v.type(), i)), kids[i]);
	} else if (v.type().id() == LogicalTypeId::MAP) {
		for (auto &entry : MapValue::GetChildren(v)) { // a list of {key, value} structs
			auto &kv = StructValue::GetChildren(entry);
			if (kv.size() != 2 || kv[0].IsNull()) continue;
			visit(OptionString(kv[0]), kv[1]);
		}
	} else {
		throw InvalidInputException("Options must be a MAP or STRUCT, got %s", v.type().ToString().c_str());
	}
}

// `alpha` and its alias `lambda`: alpha wins wherever both stand in the literal (GetRegularizationStrength
// map_options_parser.hpp:265-270)
struct AlphaOrLambda {
	bool has_alpha = false, has_lambda = false;
	double alpha = 0.0, lambda = 0.0;
	bool Read(const string &key, const Value &v) {
		if (key == "alpha") { has_alpha = true; alpha = v.GetValue<double>(); }
		else if (key == "lambda") { has_lambda = true; lambda = v.GetValue<double>(); }
		else return false;
		return true;
	}
	void Store(double &strength, bool use_lambda = true) const {
		if (has_alpha) strength = alpha;
		else if (has_lambda && use_lambda) strength = lambda;
	}
};

inline void ParseHipFitOptions(const Value &v, HipFitOptions &o) {
	if (v.IsNull()) return;
	AlphaOrLambda strength;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (val.IsNull() || strength.Read(key, val)) return;
		if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(val);
		else if (key == "compute_inference" || key == "inference") o.compute_inference = ExtractBool(val);
		else if (key == "confidence_level" || key == "confidence") o.confidence_level = val.GetValue<double>(); // no range check upstream
		else if (key == "solver")
			o.solver = ExtractEnum<AnofoxSolverType>(val, "solver", "'qr', 'svd', 'cholesky'",
			                                         {{"qr", ANOFOX_SOLVER_QR}, {"svd", ANOFOX_SOLVER_SVD}, {"cholesky", ANOFOX_SOLVER_CHOLESKY}});
		else if (key == "hc_type")
			o.hc_type = ExtractEnum<AnofoxHcType>(val, "hc_type", "'none', 'hc0', 'hc1', 'hc2', 'hc3'",
			                                      {{"none", ANOFOX_HC_NONE}, {"hc0", ANOFOX_HC_HC0}, {"hc1", ANOFOX_HC_HC1}, {"hc2", ANOFOX_HC_HC2}, {"hc3", ANOFOX_HC_HC3}});
		else if (key == "lambda_scaling") o.lambda_scaling = ExtractLambdaScaling(val);
		else if (key == "null_policy") o.drop_y_zero_x = ExtractNullPolicy(val);
		// every other key: ignored, as upstream (the legacy {'full_output': true} of the reference's examples must bind)
	});
	strength.Store(o.alpha);
}

inline AnofoxHipBatchOptions MakeHipOptions(HipModel model, const HipFitOptions &o) {
	AnofoxHipBatchOptions b;
	memset(&b, 0, sizeof b);
	b.model = model == HipModel::OLS ? ANOFOX_HIP_MODEL_OLS : (model == HipModel::RIDGE ? ANOFOX_HIP_MODEL_RIDGE : ANOFOX_HIP_MODEL_WLS);
	b.fit_intercept = o.fit_intercept;
	b.compute_inference = o.compute_inference;
	b.confidence_level = o.confidence_level;
	b.solver = o.solver;
	// ridge: alpha and its scaling, no HC branch (ridge.rs:36-229); ols / wls: HC standard errors (ols.rs:209-245)
	b.alpha = model == HipModel::RIDGE ? o.alpha : 0.0;
	b.lambda_scaling = model == HipModel::RIDGE ? o.lambda_scaling : ANOFOX_LAMBDA_SCALING_RAW;
	b.hc_type = model == HipModel::RIDGE ? ANOFOX_HC_NONE : o.hc_type;
	return b;
}

// ---- the elastic net's options (elasticnet_aggregate.cpp bind data; keys map_options_parser.cpp:637-750 with :651-656) ----
struct HipElasticNetOptions {
	double alpha = 1.0;
	double l1_ratio = 0.5;
	bool fit_intercept = true;
	uint32_t max_iterations = 1000;
	double tolerance = 1e-6;
	AnofoxLambdaScaling lambda_scaling = ANOFOX_LAMBDA_SCALING_RAW;
	bool operator==(const HipElasticNetOptions &o) const {
		return alpha == o.alpha && l1_ratio == o.l1_ratio && fit_intercept == o.fit_intercept && max_iterations == o.max_iterations &&
		       tolerance == o.tolerance && lambda_scaling == o.lambda_scaling;
	}
	AnofoxHipElasticNetBatchOptions Batch() const {
		AnofoxHipElasticNetBatchOptions b;
		memset(&b, 0, sizeof b);
		b.fit_intercept = fit_intercept;
		b.alpha = alpha;
		b.l1_ratio = l1_ratio;
		b.max_iterations = max_iterations;
		b.tolerance = tolerance;
		b.lambda_scaling = lambda_scaling;
		return b;
	}
};

// one entry of the elastic net's options; key lower-cased (also what rls_family_hip.cpp converts and does not read)
inline void ApplyElasticNetOption(const string &key, const Value &v, HipElasticNetOptions &o, AlphaOrLambda &strength) {
	if (v.IsNull() || strength.Read(key, v)) return;
	if (key == "fit_intercept" || key == "intercept") o.fit_intercept = ExtractBool(v);
	else if (key == "l1_ratio") o.l1_ratio = v.GetValue<double>();
	else if (key == "max_iterations" || key == "max_iter") o.max_iterations = ExtractUInteger(v);
	else if (key == "tolerance" || key == "tol") o.tolerance = v.GetValue<double>();
	else if (key == "lambda_scaling") o.lambda_scaling = ExtractLambdaScaling(v);
	// every other key: ignored, as upstream
}

// STRUCT or MAP literal, keys case-insensitive, alpha wins over lambda (GetRegularizationStrength)
inline void ParseHipElasticNetOptions(const Value &v, HipElasticNetOptions &o) {
	if (v.IsNull()) return;
	AlphaOrLambda strength;
	VisitOptionEntries(v, [&](const string &key, const Value &val) { ApplyElasticNetOption(key, val, o, strength); });
	strength.Store(o.alpha);
}

} // namespace hip_glue
} // namespace duckdb
