// glue_transcript.cpp — every DuckDB glue file of duckdb_shim/ linked with a recording MOCK of the C ABI, as one stand-alone
// program that prints what the glue does: a transcript (tests/test_glue_transcript_cpu.py compares it byte for byte with
// tests/golden/glue_transcript.txt, which was recorded from the glue as it stood before its Update / Bind / registration code
// was folded into row_shapes.hpp).  The program uses the public Register...Function entry points and the stand-in DuckDB API of
// tests/tools/duckdb_stub only, so the same source compiles against the glue before and after a refactor.
//
//   (a) registration  per Register...Function (each into a fresh loader, names in the loader's — alphabetical — order): alias_of,
//                     every overload's argument types and whether an alias shares its primary's callbacks, every description
//   (b) binds         per name and overload: the bound return type without, with and with a non-constant options argument, with
//                     the options argument missing, and the error text of one bad option
//   (c) updates       per primary name and overload: Update -> Combine -> Finalize -> Destroy over one small input holding every
//                     kind of row, in variants (flat / dictionary vectors, one / two source states per group, ALLOW_DESTRUCTIVE /
//                     PRESERVE_INPUT), every ABI call the glue makes with all it passes, the result vector, and the error texts
//
// The mock fills its outputs with a fixed function of its inputs; a group holding y = -7 gets a non-zero status and a row
// whose first feature is 13 a non-finite prediction.  Whatever repeats (an array staged for a call, a call's options, a call, what one
// variant of a pass did, a group's result, a type, the outcomes of an overload's binds, a pass's error texts) is printed in
// full where it first occurs and by letter and number afterwards; an alias that registers and binds as its primary says so.  Doubles print as hexadecimal floats, NaN as its 64-bit
// pattern, so that NaN and -0 compare exactly.  The calls of the moment arena behind {ols,ridge,wls}_fit_agg are not recorded
// (tests/tools/mock_abi.hpp serves them); their results are.
//
//   glue_transcript          the transcript on stdout
//   glue_transcript --time   rows per second through four Update functions against the mock (docs/MEASUREMENTS.md)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "duckdb.hpp"

#include "anofox_stats_hip.h"
// mock_abi.hpp serves the arena's entries; the two batched entries it also defines are recorded here instead
#define anofox_hip_fit_predict_batch_host mock_abi_unrecorded_fit_predict
#define anofox_hip_vif_batch_host mock_abi_unrecorded_vif
#include "mock_abi.hpp"
#undef anofox_hip_fit_predict_batch_host
#undef anofox_hip_vif_batch_host

#include "bls_family_hip.hpp"
#include "elasticnet_agg_hip.hpp"
#include "elasticnet_family_hip.hpp"
#include "family_agg_hip.hpp"
#include "fit_agg_hip.hpp"
#include "glm_family_hip.hpp"
#include "quantile_family_hip.hpp"
#include "rls_family_hip.hpp"

using namespace duckdb;

namespace {

bool g_quiet = false;         // --time: the mock records nothing
std::string *g_calls = nullptr; // where the mock writes its calls: what one variant of a pass did

std::string Hex(double v) {
	char buf[40];
	if (isnan(v)) {
		uint64_t bits;
		memcpy(&bits, &v, sizeof bits);
		snprintf(buf, sizeof buf, "#%016llx", (unsigned long long)bits);
	} else {
		snprintf(buf, sizeof buf, "%a", v);
	}
	return buf;
}

// a long value in full where it first occurs, by number afterwards
std::string Interned(const char *kind, const std::string &text) {
	static std::map<std::string, std::map<std::string, size_t>> seen;
	auto &table = seen[kind];
	auto it = table.find(text);
	if (it != table.end()) return std::string(kind) + std::to_string(it->second);
	const size_t id = table.size();
	table.emplace(text, id);
	if (!g_quiet) printf("  %s%zu := %s\n", kind, id, text.c_str());
	return std::string(kind) + std::to_string(id);
}

std::string Doubles(const double *v, size_t n) {
	if (!v) return "null";
	std::string s = "[";
	for (size_t i = 0; i < n; ++i) s += (i ? " " : "") + Hex(v[i]);
	return s + "]";
}
std::string Ints(const int64_t *v, size_t n) {
	if (!v) return "null";
	std::string s = "[";
	for (size_t i = 0; i < n; ++i) s += (i ? " " : "") + std::to_string(v[i]);
	return s + "]";
}

// ---- the recording mock ----
void LogCall(const char *entry, int64_t G, size_t p, int64_t n, const int64_t *off, const int64_t *tc, const double *y, const double *const *cols,
             const double *w, const double *offset, const std::string &scalars) {
	if (g_quiet) return;
	auto array = [&](const double *v) { return v ? Interned("A", Doubles(v, (size_t)n)) : std::string("null"); };
	std::string call = std::string(entry) + " G=" + std::to_string(G) + " p=" + std::to_string(p) + " n=" + std::to_string(n) + " " +
	                   (scalars.empty() ? scalars : Interned("O", scalars)) + " offsets=" + Ints(off, (size_t)G + 1) + " train_counts=" + Ints(tc, (size_t)G) +
	                   " y=" + array(y);
	for (size_t j = 0; j < p; ++j) call += " x" + std::to_string(j) + "=" + array(cols[j]);
	if (w) call += " w=" + array(w);
	if (offset) call += " offset=" + array(offset);
	if (g_calls) *g_calls += Interned("C", call) + "; ";
}

// a group's record: coefficient j = the sum of column j over the rows that train (y not NaN), then {sum of their y, rows, training rows,
// 0.25, training rows}, padded with zeros up to `status_at`, where the status stands: 1 for a group holding y = -7
void FillRecord(int64_t g, size_t p, const int64_t *off, const double *y, const double *const *cols, double *rec, size_t len, size_t status_at) {
	for (size_t k = 0; k < len; ++k) rec[k] = 0.0;
	double sum_y = 0.0, n_train = 0.0;
	bool fails = false;
	for (int64_t r = off[g]; r < off[g + 1]; ++r) {
		if (isnan(y[r])) continue;
		for (size_t j = 0; j < p; ++j) rec[j] += cols[j][r];
		sum_y += y[r];
		n_train += 1.0;
		fails = fails || y[r] == -7.0;
	}
	const double tail[5] = {sum_y, (double)(off[g + 1] - off[g]), n_train, 0.25, n_train};
	for (size_t k = 0; k < 5 && p + k < status_at; ++k) rec[p + k] = tail[k];
	rec[status_at] = fails ? 1.0 : 0.0;
}

// row r: {v, v - 1, v + 1} with v = the sum of the row's features + its group's train count; NaN where the first feature is 13
void FillPred(int64_t G, size_t p, const int64_t *off, const double *const *cols, const int64_t *tc, double *pred) {
	for (int64_t g = 0; g < G; ++g)
		for (int64_t r = off[g]; r < off[g + 1]; ++r) {
			double v = tc ? (double)tc[g] : 0.0;
			for (size_t j = 0; j < p; ++j) v += cols[j][r];
			if (cols[0][r] == 13.0) v = NAN;
			pred[3 * r] = v;
			pred[3 * r + 1] = v - 1.0;
			pred[3 * r + 2] = v + 1.0;
		}
}

std::string EnOpts(AnofoxHipElasticNetBatchOptions o) {
	return "en{intercept=" + std::to_string(o.fit_intercept) + " alpha=" + Hex(o.alpha) + " l1_ratio=" + Hex(o.l1_ratio) + " max_iter=" +
	       std::to_string(o.max_iterations) + " tol=" + Hex(o.tolerance) + " scaling=" + std::to_string((int)o.lambda_scaling) + "}";
}
std::string RlsOpts(AnofoxHipRlsBatchOptions o) {
	return "rls{intercept=" + std::to_string(o.fit_intercept) + " forgetting=" + Hex(o.forgetting_factor) + " p_diagonal=" + Hex(o.initial_p_diagonal) + "}";
}
std::string BlsOpts(AnofoxHipBlsBatchOptions o) {
	return "bls{intercept=" + std::to_string(o.fit_intercept) + " lower=" + Doubles(o.lower_bounds, o.lower_bounds_len) + " upper=" +
	       Doubles(o.upper_bounds, o.upper_bounds_len) + " max_iter=" + std::to_string(o.max_iterations) + " tol=" + Hex(o.tolerance) + "}";
}
std::string QuantileOpts(AnofoxHipQuantileBatchOptions o) {
	return "quantile{tau=" + Hex(o.tau) + " intercept=" + std::to_string(o.fit_intercept) + " max_iter=" + std::to_string(o.max_iterations) + " tol=" +
	       Hex(o.tolerance) + "}";
}
std::string GlmOpts(AnofoxHipGlmBatchOptions o) {
	return "glm{family=" + std::to_string(o.family) + " intercept=" + std::to_string(o.fit_intercept) + " max_iter=" + std::to_string(o.max_iterations) +
	       " tol=" + Hex(o.tolerance) + " lambda=" + Hex(o.lambda) + " inference=" + std::to_string(o.compute_inference) + " confidence=" +
	       Hex(o.confidence_level) + "}";
}
std::string FitOpts(AnofoxHipBatchOptions o) {
	return "fit{model=" + std::to_string((int)o.model) + " intercept=" + std::to_string(o.fit_intercept) + " inference=" + std::to_string(o.compute_inference) +
	       " confidence=" + Hex(o.confidence_level) + " alpha=" + Hex(o.alpha) + " solver=" + std::to_string((int)o.solver) + " scaling=" +
	       std::to_string((int)o.lambda_scaling) + " hc=" + std::to_string((int)o.hc_type) + "}";
}

} // namespace

extern "C" {
size_t anofox_hip_core_record_len(size_t p) { return p + 6; }

bool anofox_hip_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                       const double *w, const int64_t *tc, AnofoxHipBatchOptions o, double *core, double *pred, AnofoxError *) {
	LogCall("fit_predict", G, p, n, off, tc, y, cols, w, nullptr, FitOpts(o));
	for (int64_t g = 0; g < G; ++g) FillRecord(g, p, off, y, cols, core + (size_t)g * (p + 6), p + 6, p + 5);
	FillPred(G, p, off, cols, tc, pred);
	return true;
}
// the VIF of feature j: the sum over the group's rows of (k + 1) x_j[k]; status 1 for a group whose first value is -7
bool anofox_hip_vif_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *const *cols, double *vif, AnofoxError *) {
	std::vector<double> no_y((size_t)n, 0.0);
	LogCall("vif", G, p, n, off, nullptr, no_y.data(), cols, nullptr, nullptr, "");
	for (int64_t g = 0; g < G; ++g) {
		for (size_t j = 0; j < p; ++j) {
			double s = 0.0;
			for (int64_t r = off[g]; r < off[g + 1]; ++r) s += (double)(r - off[g] + 1) * cols[j][r];
			vif[(size_t)g * (p + 1) + j] = s;
		}
		vif[(size_t)g * (p + 1) + p] = cols[0][off[g]] == -7.0 ? 1.0 : 0.0;
	}
	return true;
}
bool anofox_hip_elasticnet_fit_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                          AnofoxHipElasticNetBatchOptions o, double *core, int32_t *, AnofoxError *) {
	LogCall("elasticnet_fit", G, p, n, off, nullptr, y, cols, nullptr, nullptr, EnOpts(o));
	for (int64_t g = 0; g < G; ++g) FillRecord(g, p, off, y, cols, core + (size_t)g * (p + 6), p + 6, p + 5);
	return true;
}
bool anofox_hip_elasticnet_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y,
                                                  const double *const *cols, const int64_t *tc, AnofoxHipElasticNetBatchOptions o, double confidence,
                                                  double *core, double *pred, AnofoxError *) {
	LogCall("elasticnet_fit_predict", G, p, n, off, tc, y, cols, nullptr, nullptr, EnOpts(o) + " confidence=" + Hex(confidence));
	for (int64_t g = 0; g < G; ++g) FillRecord(g, p, off, y, cols, core + (size_t)g * (p + 6), p + 6, p + 5);
	FillPred(G, p, off, cols, tc, pred);
	return true;
}
bool anofox_hip_rls_fit_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                   AnofoxHipRlsBatchOptions o, double *core, AnofoxError *) {
	LogCall("rls_fit", G, p, n, off, nullptr, y, cols, nullptr, nullptr, RlsOpts(o));
	for (int64_t g = 0; g < G; ++g) FillRecord(g, p, off, y, cols, core + (size_t)g * (p + 6), p + 6, p + 5);
	return true;
}
bool anofox_hip_rls_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                           const int64_t *tc, AnofoxHipRlsBatchOptions o, double confidence, double *core, double *pred, AnofoxError *) {
	LogCall("rls_fit_predict", G, p, n, off, tc, y, cols, nullptr, nullptr, RlsOpts(o) + " confidence=" + Hex(confidence));
	for (int64_t g = 0; g < G; ++g) FillRecord(g, p, off, y, cols, core + (size_t)g * (p + 6), p + 6, p + 5);
	FillPred(G, p, off, cols, tc, pred);
	return true;
}
// the bls record [3 p + 6]: coefficients (the second one NaN in odd groups), intercept (NaN without one), ..., status at p + 5, then
// the at-lower flags (feature j of group g: (g + j) odd) and the at-upper flags (their complement)
bool anofox_hip_bls_fit_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                   AnofoxHipBlsBatchOptions o, double *bls, int32_t *, AnofoxError *) {
	LogCall("bls_fit", G, p, n, off, nullptr, y, cols, nullptr, nullptr, BlsOpts(o));
	for (int64_t g = 0; g < G; ++g) {
		double *rec = bls + (size_t)g * (3 * p + 6);
		FillRecord(g, p, off, y, cols, rec, 3 * p + 6, p + 5);
		if (g % 2 && p > 1) rec[1] = NAN;
		if (!o.fit_intercept) rec[p] = NAN;
		for (size_t j = 0; j < p; ++j) {
			rec[p + 6 + j] = (double)(((size_t)g + j) % 2);
			rec[2 * p + 6 + j] = 1.0 - rec[p + 6 + j];
		}
	}
	return true;
}
bool anofox_hip_bls_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                           const int64_t *tc, AnofoxHipBlsBatchOptions o, double confidence, double *core, double *pred, AnofoxError *) {
	LogCall("bls_fit_predict", G, p, n, off, tc, y, cols, nullptr, nullptr, BlsOpts(o) + " confidence=" + Hex(confidence));
	for (int64_t g = 0; g < G; ++g) FillRecord(g, p, off, y, cols, core + (size_t)g * (p + 6), p + 6, p + 5);
	FillPred(G, p, off, cols, tc, pred);
	return true;
}
bool anofox_hip_quantile_fit_predict_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y,
                                                const double *const *cols, const int64_t *tc, AnofoxHipQuantileBatchOptions o, double *core, double *pred,
                                                AnofoxError *) {
	LogCall("quantile_fit_predict", G, p, n, off, tc, y, cols, nullptr, nullptr, QuantileOpts(o));
	for (int64_t g = 0; g < G; ++g) FillRecord(g, p, off, y, cols, core + (size_t)g * (p + 6), p + 6, p + 5);
	FillPred(G, p, off, cols, tc, pred);
	for (int64_t r = 0; r < n; ++r) pred[3 * r + 1] = pred[3 * r + 2] = NAN;
	return true;
}
// tau t of a group: status 1 and NaN predictions where the tau is NaN or outside (0, 1), or the group holds y = -7; yhat = tau + the row's v
bool anofox_hip_quantile_fit_predict_path_batch_host(AnofoxHipContext *, int64_t G, size_t p, int64_t n, const int64_t *off, const double *y,
                                                     const double *const *cols, const int64_t *tc, AnofoxHipQuantileBatchOptions o, const double *taus,
                                                     size_t T, double *quantile, int32_t *, double *pred, AnofoxError *) {
	LogCall("quantile_path", G, p, n, off, tc, y, cols, nullptr, nullptr, QuantileOpts(o) + " taus=" + Doubles(taus, T));
	std::vector<double> one((size_t)n * 3);
	FillPred(G, p, off, cols, tc, one.data());
	for (int64_t g = 0; g < G; ++g)
		for (size_t t = 0; t < T; ++t) {
			double *rec = quantile + ((size_t)g * T + t) * (p + 6);
			FillRecord(g, p, off, y, cols, rec, p + 6, p + 5);
			if (!(taus[t] > 0.0 && taus[t] < 1.0)) rec[p + 5] = 1.0;
			for (int64_t r = off[g]; r < off[g + 1]; ++r) pred[(size_t)r * T + t] = rec[p + 5] != 0.0 ? NAN : taus[t] + one[3 * (size_t)r];
		}
	return true;
}
// the glm record [q + 11]: as FillRecord, then iterations = 7 at q + 8, converged at q + 9, status at q + 10; inference[k][j] = coefficient + k + 1
static void MockGlm(int64_t G, size_t q, const int64_t *off, const double *y, const double *const *cols, bool with_inference, double *rec, double *inf) {
	for (int64_t g = 0; g < G; ++g) {
		double *r = rec + (size_t)g * (q + 11);
		FillRecord(g, q, off, y, cols, r, q + 11, q + 10);
		r[q + 5] = 1.5;
		r[q + 6] = (double)(off[g + 1] - off[g]);
		r[q + 8] = 7.0;
		r[q + 9] = (double)(g % 2);
		if (with_inference && inf)
			for (size_t k = 0; k < 5; ++k)
				for (size_t j = 0; j < q; ++j) inf[((size_t)g * 5 + k) * q + j] = r[j] + (double)k + 1.0;
	}
}
bool anofox_hip_glm_fit_batch_host(AnofoxHipContext *, int64_t G, size_t q, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                   const double *offset, AnofoxHipGlmBatchOptions o, double *rec, double *inf, AnofoxError *) {
	LogCall("glm_fit", G, q, n, off, nullptr, y, cols, nullptr, offset, GlmOpts(o) + " inference_out=" + std::to_string(inf != nullptr));
	MockGlm(G, q, off, y, cols, o.compute_inference, rec, inf);
	return true;
}
bool anofox_hip_glm_fit_accuracy_batch_host(AnofoxHipContext *, int64_t G, size_t q, int64_t n, const int64_t *off, const double *y, const double *const *cols,
                                            const double *offset, AnofoxHipGlmBatchOptions o, double threshold, double *rec, double *inf, double *accuracy,
                                            AnofoxError *) {
	LogCall("glm_fit_accuracy", G, q, n, off, nullptr, y, cols, nullptr, offset,
	        GlmOpts(o) + " threshold=" + Hex(threshold) + " inference_out=" + std::to_string(inf != nullptr));
	MockGlm(G, q, off, y, cols, o.compute_inference, rec, inf);
	for (int64_t g = 0; g < G; ++g) accuracy[g] = threshold + (double)(off[g + 1] - off[g]);
	return true;
}
bool anofox_hip_glm_fit_predict_interval_batch_host(AnofoxHipContext *, int64_t G, size_t q, int64_t n, const int64_t *off, const double *y,
                                                    const double *const *cols, const double *offset, const int64_t *tc, AnofoxHipGlmBatchOptions o, double z,
                                                    double *core, double *pred, AnofoxError *) {
	LogCall("glm_fit_predict_interval", G, q, n, off, tc, y, cols, nullptr, offset, GlmOpts(o) + " z=" + Hex(z));
	MockGlm(G, q, off, y, cols, false, core, nullptr);
	FillPred(G, q, off, cols, tc, pred);
	return true;
}
}

namespace {

// ---- the functions ----
struct Registration {
	const char *symbol;
	void (*reg)(ExtensionLoader &);
};
#define REG(f) {#f, f}
const Registration kRegistrations[] = {
    REG(RegisterHipOlsAggregateFunction), REG(RegisterHipRidgeAggregateFunction), REG(RegisterHipWlsAggregateFunction),
    REG(RegisterHipOlsFitPredictAggregateFunction), REG(RegisterHipRidgeFitPredictAggregateFunction), REG(RegisterHipWlsFitPredictAggregateFunction),
    REG(RegisterHipOlsFitPredictFunction), REG(RegisterHipRidgeFitPredictFunction), REG(RegisterHipWlsFitPredictFunction),
    REG(RegisterHipVifAggregateFunction), REG(RegisterHipElasticNetAggregateFunction), REG(RegisterHipElasticNetFitPredictAggregateFunction),
    REG(RegisterHipElasticNetFitPredictFunction), REG(RegisterHipRlsAggregateFunction), REG(RegisterHipRlsFitPredictAggregateFunction),
    REG(RegisterHipRlsFitPredictFunction), REG(RegisterHipBlsAggregateFunction), REG(RegisterHipBlsNnlsAggregateFunction),
    REG(RegisterHipBlsFitPredictAggregateFunction), REG(RegisterHipQuantileFitPredictAggregateFunction),
    REG(RegisterHipQuantilePathFitPredictAggregateFunction), REG(RegisterHipQuantileFitPredictFunction), REG(RegisterHipPoissonAggregateFunction),
    REG(RegisterHipBinomialAggregateFunction), REG(RegisterHipLogisticAggregateFunction), REG(RegisterHipPoissonFitPredictAggregateFunction)};
#undef REG

std::string Types(const vector<LogicalType> &types) {
	std::string s = "(";
	for (size_t i = 0; i < types.size(); ++i) s += (i ? ", " : "") + types[i].ToString();
	return s + ")";
}
std::string Strings(const vector<string> &v) {
	std::string s = "[";
	for (size_t i = 0; i < v.size(); ++i) s += (i ? " | " : "") + v[i];
	return s + "]";
}
bool SameCallbacks(const AggregateFunction &a, const AggregateFunction &b) {
	return a.state_size == b.state_size && a.initialize == b.initialize && a.update == b.update && a.combine == b.combine && a.finalize == b.finalize &&
	       a.simple_update == b.simple_update && a.bind == b.bind && a.destructor == b.destructor;
}
const CreateAggregateFunctionInfo *PrimaryOf(const ExtensionLoader &loader) {
	for (auto &kv : loader.registered)
		if (kv.second.alias_of.empty()) return &kv.second;
	return nullptr;
}

void PrintRegistration(const Registration &r) {
	ExtensionLoader loader;
	r.reg(loader);
	printf("%s\n", r.symbol);
	const CreateAggregateFunctionInfo *primary = PrimaryOf(loader);
	for (auto &kv : loader.registered) {
		const auto &info = kv.second;
		printf(" name %s set=%s alias_of=%s on_conflict=%d\n", kv.first.c_str(), info.functions.name.c_str(), info.alias_of.empty() ? "-" : info.alias_of.c_str(),
		       (int)info.on_conflict);
		const auto &fs = info.functions.functions;
		bool as_primary = &info != primary && primary && fs.size() == primary->functions.functions.size();
		for (size_t k = 0; as_primary && k < fs.size(); ++k) {
			const auto &pf = primary->functions.functions[k];
			as_primary = fs[k].name == kv.first && fs[k].arguments == pf.arguments && fs[k].return_type == pf.return_type && SameCallbacks(fs[k], pf);
		}
		if (as_primary) printf("  overloads: the primary's %zu, in its order, with its callbacks, under this name\n", fs.size());
		for (size_t k = 0; !as_primary && k < fs.size(); ++k)
			printf("  overload %zu %s%s declared=%s\n", k, fs[k].name.c_str(), Types(fs[k].arguments).c_str(), fs[k].return_type.ToString().c_str());
		for (auto &d : info.descriptions)
			printf("  description text=%s examples=%s names=%s types=%s categories=%s\n", Interned("W", d.description).c_str(), Strings(d.examples).c_str(),
			       Strings(d.parameter_names).c_str(), Types(d.parameter_types).c_str(), Strings(d.categories).c_str());
	}
}

// ---- constants for the options argument ----
template <class Tag, typename Tag::type Member>
struct MemberAccess {
	friend typename Tag::type Access(Tag) { return Member; }
};
struct ValueTypeTag {
	typedef LogicalType Value::*type;
	friend type Access(ValueTypeTag);
};
template struct MemberAccess<ValueTypeTag, &Value::type_>; // (the stand-in's Value has no LIST factory: a STRUCT constant retyped)

Value ListOf(std::initializer_list<double> values, bool with_null) {
	child_list_t<Value> kids;
	for (double v : values) kids.push_back({std::to_string(kids.size()), Value::DOUBLE(v)});
	if (with_null) kids.push_back({std::to_string(kids.size()), Value(LogicalType(LogicalType::DOUBLE))});
	Value v = Value::STRUCT(std::move(kids));
	v.*Access(ValueTypeTag()) = LogicalType::LIST(LogicalType::DOUBLE);
	return v;
}

// the option literals of the passes: every family finds its own keys in them and ignores the others
Value Options(bool drop_y_zero_x, bool inference) {
	child_list_t<Value> kids;
	kids.push_back({"Fit_Intercept", Value::BOOLEAN(false)});
	kids.push_back({"null_policy", Value(std::string(drop_y_zero_x ? "DROP_Y_ZERO_X" : "drop"))});
	kids.push_back({"compute_inference", Value::BOOLEAN(inference)});
	kids.push_back({"confidence_level", Value::DOUBLE(0.99)});
	kids.push_back({"alpha", Value::DOUBLE(0.5)});
	kids.push_back({"lambda", Value::DOUBLE(0.25)});
	kids.push_back({"l1_ratio", Value::DOUBLE(0.75)});
	kids.push_back({"forgetting_factor", Value::DOUBLE(0.875)});
	kids.push_back({"lower_bound", Value::DOUBLE(-1.0)});
	kids.push_back({"upper", Value::INTEGER(3)});
	kids.push_back({"max_iter", Value::INTEGER(17)});
	kids.push_back({"taus", ListOf({0.5, 0.125, 1.5}, true)});
	kids.push_back({"threshold", Value::DOUBLE(0.75)});
	kids.push_back({"offset", Value::INTEGER(2)});
	kids.push_back({"glm_lambda", Value::DOUBLE(0.125)});
	kids.push_back({"unknown_key", Value(std::string("x"))});
	return Value::STRUCT(std::move(kids));
}
Value BadOptions() { return Value::STRUCT({{"taus", ListOf({0.5}, false)}, {"fit_intercept", Value(std::string("maybe"))}}); }

bool TakesOptions(const AggregateFunction &f) { return !f.arguments.empty() && f.arguments.back().id() == LogicalTypeId::ANY; }

// bind a copy of the overload: the column arguments are not foldable; options: nullptr = the argument is missing
std::string Bind(const AggregateFunction &f, const Value *options, bool foldable, unique_ptr<FunctionData> *bind_out = nullptr,
                 AggregateFunction *bound_out = nullptr) {
	AggregateFunction fn(f);
	ClientContext context;
	vector<unique_ptr<Expression>> args;
	const size_t columns = f.arguments.size() - (TakesOptions(f) ? 1 : 0);
	for (size_t k = 0; k < columns; ++k) args.push_back(make_uniq<Expression>(Value(), false));
	if (options) args.push_back(make_uniq<Expression>(*options, foldable));
	try {
		auto bind = fn.bind(context, fn, args);
		if (bind) {
			auto copy = bind->Copy();
			if (!bind->Equals(*copy) || !copy->Equals(*bind)) return "error: a copy of the bind data does not equal it";
		}
		if (bind_out) *bind_out = std::move(bind);
		if (bound_out) *bound_out = fn;
		return Interned("T", fn.return_type.ToString());
	} catch (const std::exception &e) {
		return std::string("error: ") + e.what();
	}
}

void PrintBinds(const Registration &r) {
	ExtensionLoader loader;
	r.reg(loader);
	printf("%s\n", r.symbol);
	const Value plain = Options(false, false), inference = Options(false, true), bad = BadOptions();
	auto outcomes = [&](const CreateAggregateFunctionInfo &info) { // per overload: its argument types and what its binds give
		std::vector<std::string> out;
		for (auto &f : info.functions.functions) {
			std::string o = Bind(f, nullptr, true);
			if (TakesOptions(f))
				o = "options -> " + Bind(f, &plain, true) + " | inference -> " + Bind(f, &inference, true) + " | not constant -> " + Bind(f, &plain, false) +
				    " | missing -> " + o + " | bad option -> " + Bind(f, &bad, true);
			out.push_back(Types(f.arguments) + " " + Interned("B", o));
		}
		return out;
	};
	const CreateAggregateFunctionInfo *primary = PrimaryOf(loader);
	if (!primary) return;
	const std::vector<std::string> of_primary = outcomes(*primary);
	for (auto &kv : loader.registered) {
		const std::vector<std::string> mine = &kv.second == primary ? of_primary : outcomes(kv.second);
		if (&kv.second != primary && mine == of_primary) {
			printf(" bind %s: every overload as the primary's\n", kv.first.c_str());
			continue;
		}
		for (auto &o : mine) printf(" bind %s%s\n", kv.first.c_str(), o.c_str());
	}
}

// ---- the input of the passes ----
struct InRow {
	int group;
	bool y_null;
	double y;
	bool x_null;
	std::vector<double> x;
	std::vector<uint8_t> xe_null;
	bool w_null;
	double w;
	int split; // a code into kSplit
};
const char *const kSplit[] = {nullptr, "train", "Training", "test", "TRAIN", "a-validation-partition-name", "training"}; // family_driver.hpp's kSplitStrings
constexpr int kGroups = 6;

// group 0: every kind of row among enough plain ones; group 1: holds y = -7 (the mock fails it); group 2: one training row;
// group 3: no row; group 4: two features, its last row without a finite prediction; group 5: plain rows only, all of them training
std::vector<InRow> MakeRows() {
	std::vector<InRow> rows;
	auto plain = [&](int group, int i, size_t p) {
		InRow r {group, false, (double)(i + 1) * 0.5, false, {}, {}, false, 1.0 + 0.25 * (double)i, 1 + (i % 2)};
		for (size_t j = 0; j < p; ++j) r.x.push_back((double)(1 + (i * (int)(j + 2)) % 7) + 0.5 * (double)j);
		r.xe_null.assign(p, 0);
		rows.push_back(r);
		return rows.size() - 1;
	};
	for (int i = 0; i < 16; ++i) {
		const size_t at = plain(0, i, 3);
		rows[at].split = i % 7; // every split string, NULL included
	}
	rows[1].y_null = true;                      // NULL y
	rows[2].x_null = true;                      // NULL x list
	rows[3].xe_null[1] = 1;                     // a NULL list element
	rows[4].x[2] = 0.0;                         // a zero feature
	rows[5].w_null = true;                      // NULL / zero / negative / NaN weights
	rows[6].w = 0.0;
	rows[8].w = -2.0;
	rows[9].w = NAN;
	rows[11].y = NAN;                           // a NaN y that is not NULL
	rows[12].x[0] = 13.0;                       // no finite prediction for this row
	rows[13].x[0] = -0.0;                       // (a zero feature that is a negative zero)
	rows[15].y_null = rows[15].x_null = true;
	for (int i = 0; i < 6; ++i) plain(1, i, 3);
	rows[16 + 4].y = -7.0;
	plain(2, 0, 3);
	rows[plain(2, 1, 3)].y_null = true;
	for (int i = 0; i < 6; ++i) plain(4, i, 2);
	rows.back().x[0] = 13.0;
	for (int i = 0; i < 6; ++i) rows[plain(5, i, 3)].split = 1;
	return rows;
}

struct Variant {
	const char *name;
	bool dictionary;
	int sources;
	AggregateCombineType combine_type;
};
const Variant kVariants[] = {{"flat, 1 source, ALLOW_DESTRUCTIVE", false, 1, AggregateCombineType::ALLOW_DESTRUCTIVE},
                             {"dictionary, 2 sources, ALLOW_DESTRUCTIVE", true, 2, AggregateCombineType::ALLOW_DESTRUCTIVE},
                             {"flat, 2 sources, PRESERVE_INPUT", false, 2, AggregateCombineType::PRESERVE_INPUT}};

struct Shape { // which inputs an overload takes
	bool has_y = true, weighted = false, split = false, options = false;
	explicit Shape(const AggregateFunction &f) {
		has_y = f.arguments[0].id() == LogicalTypeId::DOUBLE;
		options = TakesOptions(f);
		for (size_t k = has_y ? 2 : 1; k < f.arguments.size(); ++k) {
			weighted = weighted || f.arguments[k].id() == LogicalTypeId::DOUBLE;
			split = split || f.arguments[k].id() == LogicalTypeId::VARCHAR;
		}
	}
};

Vector PointerVector(std::vector<data_ptr_t> &ptrs) {
	Vector v(LogicalType(LogicalType::POINTER), ptrs.size() ? ptrs.size() : 1);
	if (!ptrs.empty()) memcpy(FlatVector::GetData<data_ptr_t>(v), ptrs.data(), ptrs.size() * sizeof(data_ptr_t));
	return v;
}

// the rows as the input vectors of one Update call (dictionary: the physical order is the reverse of the logical one)
std::vector<Vector> InputVectors(const Shape &shape, const std::vector<const InRow *> &rows, bool dictionary) {
	const size_t cnt = rows.size();
	std::vector<uint32_t> sel(cnt);
	for (size_t i = 0; i < cnt; ++i) sel[i] = (uint32_t)(dictionary ? cnt - 1 - i : i);
	std::vector<Vector> inputs;
	if (shape.has_y) inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
	const size_t x_at = inputs.size();
	inputs.emplace_back(LogicalType::LIST(LogicalType::DOUBLE), cnt);
	const size_t w_at = inputs.size();
	if (shape.weighted) inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
	const size_t s_at = inputs.size();
	if (shape.split) inputs.emplace_back(LogicalType(LogicalType::VARCHAR), cnt);
	const size_t data_inputs = inputs.size();
	if (shape.options) inputs.emplace_back(LogicalType(LogicalType::BIGINT), cnt);
	size_t total = 0;
	for (auto *r : rows) total += r->x.size();
	ListVector::Reserve(inputs[x_at], total ? total : 1);
	list_entry_t *entries = ListVector::GetData(inputs[x_at]);
	Vector &child = ListVector::GetEntry(inputs[x_at]);
	double *child_values = FlatVector::GetData<double>(child);
	size_t off = 0;
	for (size_t i = 0; i < cnt; ++i) {
		const InRow &r = *rows[i];
		const size_t phys = sel[i];
		if (shape.has_y) {
			FlatVector::GetData<double>(inputs[0])[phys] = r.y_null ? 1e300 : r.y;
			if (r.y_null) FlatVector::SetNull(inputs[0], phys, true);
		}
		entries[phys].offset = off;
		entries[phys].length = r.x.size();
		for (size_t j = 0; j < r.x.size(); ++j) {
			child_values[off + j] = r.xe_null[j] ? 1e300 : r.x[j]; // (the slot of a NULL holds whatever it holds: the glue must not read it)
			if (r.xe_null[j]) FlatVector::Validity(child).SetInvalid(off + j);
		}
		off += r.x.size();
		if (r.x_null) FlatVector::SetNull(inputs[x_at], phys, true);
		if (shape.weighted) {
			FlatVector::GetData<double>(inputs[w_at])[phys] = r.w_null ? 1e300 : r.w;
			if (r.w_null) FlatVector::SetNull(inputs[w_at], phys, true);
		}
		if (shape.split) {
			if (!kSplit[r.split]) FlatVector::SetNull(inputs[s_at], phys, true);
			else FlatVector::GetData<string_t>(inputs[s_at])[phys] = inputs[s_at].AddString(kSplit[r.split]);
		}
	}
	ListVector::SetListSize(inputs[x_at], total);
	if (dictionary)
		for (size_t k = 0; k < data_inputs; ++k) inputs[k].MakeDictionary(sel);
	if (inputs.size() > data_inputs) inputs.back().MakeConstant();
	return inputs;
}

void Dump(Vector &v, idx_t i, std::string &out) {
	if (!FlatVector::Validity(v).RowIsValid(i)) {
		out += "NULL";
		return;
	}
	switch (v.GetType().id()) {
	case LogicalTypeId::DOUBLE: out += Hex(FlatVector::GetData<double>(v)[i]); break;
	case LogicalTypeId::BIGINT: out += std::to_string(FlatVector::GetData<int64_t>(v)[i]); break;
	case LogicalTypeId::INTEGER: out += std::to_string(FlatVector::GetData<int32_t>(v)[i]); break;
	case LogicalTypeId::BOOLEAN: out += FlatVector::GetData<bool>(v)[i] ? "true" : "false"; break;
	case LogicalTypeId::LIST: {
		const list_entry_t e = ListVector::GetData(v)[i];
		if (e.offset + e.length > ListVector::GetListSize(v)) {
			out += "BAD LIST ENTRY";
			break;
		}
		out += "[";
		for (idx_t k = 0; k < e.length; ++k) {
			if (k) out += " ";
			Dump(ListVector::GetEntry(v), e.offset + k, out);
		}
		out += "]";
		break;
	}
	case LogicalTypeId::STRUCT: {
		out += "{";
		auto &fields = StructVector::GetEntries(v);
		for (size_t c = 0; c < fields.size(); ++c) {
			if (c) out += " ";
			Dump(*fields[c], i, out);
		}
		out += "}";
		break;
	}
	default: out += "?";
	}
}

// the states of one pass, destroyed and freed whatever happens
struct States {
	States(AggregateFunction &fn_p, AggregateInputData &aid_p) : fn(fn_p), aid(aid_p) {}
	~States() {
		if (!all.empty() && fn.destructor) {
			Vector sv = PointerVector(all);
			fn.destructor(sv, aid, all.size());
		}
		for (auto s : all) delete[] s;
	}
	data_ptr_t New() {
		data_ptr_t s = new data_t[fn.state_size(fn)];
		fn.initialize(fn, s);
		all.push_back(s);
		return s;
	}
	AggregateFunction &fn;
	AggregateInputData &aid;
	std::vector<data_ptr_t> all;
};

void Update(AggregateFunction &fn, AggregateInputData &aid, const Shape &shape, const std::vector<const InRow *> &rows, std::vector<data_ptr_t> &states,
            bool dictionary, idx_t input_count_override = (idx_t)-1) {
	std::vector<Vector> inputs = InputVectors(shape, rows, dictionary);
	Vector sv = PointerVector(states);
	fn.update(inputs.data(), aid, input_count_override == (idx_t)-1 ? inputs.size() : input_count_override, sv, rows.size());
}

std::string RunPass(const AggregateFunction &bound, FunctionData *bind, const std::vector<InRow> &rows, const Variant &variant) {
	AggregateFunction fn(bound);
	const Shape shape(fn);
	ArenaAllocator alloc;
	AggregateInputData aid(bind, alloc, variant.combine_type);
	std::string did;
	g_calls = &did;
	try {
		States states(fn, aid);
		std::vector<std::vector<data_ptr_t>> sources(variant.sources);
		std::vector<data_ptr_t> targets;
		for (auto &s : sources)
			for (int g = 0; g < kGroups; ++g) s.push_back(states.New());
		for (int g = 0; g < kGroups; ++g) targets.push_back(states.New());
		std::vector<size_t> group_rows(kGroups, 0), seen(kGroups, 0);
		for (auto &r : rows) group_rows[r.group]++;
		std::vector<const InRow *> in;
		std::vector<data_ptr_t> row_states;
		for (auto &r : rows) {
			const size_t k = seen[r.group]++;
			in.push_back(&r);
			row_states.push_back(sources[variant.sources == 2 && k >= group_rows[r.group] / 2 ? 1 : 0][r.group]); // the later half: the second source
		}
		Update(fn, aid, shape, in, row_states, variant.dictionary);
		for (auto &s : sources) {
			Vector sv = PointerVector(s), tv = PointerVector(targets);
			fn.combine(sv, tv, aid, kGroups);
		}
		Vector result(fn.return_type, kGroups + 2);
		Vector tv = PointerVector(targets);
		fn.finalize(tv, aid, result, kGroups, 2); // (at an offset, as DuckDB finalizes into a slice)
		did += "result";
		for (int g = 0; g < kGroups; ++g) {
			std::string value;
			Dump(result, (idx_t)g + 2, value);
			did += " g" + std::to_string(g) + "=" + (value.size() > 8 ? Interned("R", value) : value);
		}
	} catch (const std::exception &e) {
		did += std::string("error: ") + e.what();
	}
	g_calls = nullptr;
	return Interned("V", did);
}

// one state, the given rows in one Update call: the error text, or "none"
void RunErrorCase(std::string &texts, const char *what, const AggregateFunction &bound, FunctionData *bind, const std::vector<InRow> &rows,
                  idx_t input_count_override) {
	AggregateFunction fn(bound);
	const Shape shape(fn);
	ArenaAllocator alloc;
	AggregateInputData aid(bind, alloc);
	std::string text = "none";
	try {
		States states(fn, aid);
		data_ptr_t s = states.New();
		std::vector<const InRow *> in;
		for (auto &r : rows) in.push_back(&r);
		std::vector<data_ptr_t> row_states(rows.size(), s);
		Update(fn, aid, shape, in, row_states, false, input_count_override);
	} catch (const std::exception &e) {
		text = e.what();
	}
	texts += std::string(what) + ": " + text + " | ";
}

// a source state of `from` features combined into a target of `into`: the error text
void RunCombineError(std::string &texts, const AggregateFunction &bound, FunctionData *bind, size_t from, size_t into) {
	AggregateFunction fn(bound);
	const Shape shape(fn);
	ArenaAllocator alloc;
	AggregateInputData aid(bind, alloc, AggregateCombineType::ALLOW_DESTRUCTIVE);
	std::string text = "none";
	try {
		States states(fn, aid);
		std::vector<data_ptr_t> source {states.New()}, target {states.New()};
		InRow a {0, false, 1.0, false, std::vector<double>(from, 1.0), std::vector<uint8_t>(from, 0), false, 1.0, 1};
		InRow b {0, false, 2.0, false, std::vector<double>(into, 2.0), std::vector<uint8_t>(into, 0), false, 1.0, 1};
		std::vector<const InRow *> in {&a, &b};
		std::vector<data_ptr_t> row_states {source[0], target[0]};
		Update(fn, aid, shape, in, row_states, false);
		Vector sv = PointerVector(source), tv = PointerVector(target);
		fn.combine(sv, tv, aid, 1);
	} catch (const std::exception &e) {
		text = e.what();
	}
	texts += "3: " + text + " | ";
}

void PrintUpdates(const Registration &r) {
	ExtensionLoader loader;
	r.reg(loader);
	printf("%s\n", r.symbol);
	const CreateAggregateFunctionInfo *primary = PrimaryOf(loader);
	if (!primary) return;
	const std::vector<InRow> rows = MakeRows();
	const bool window = primary->functions.name.find("_agg") == std::string::npos;
	for (auto &f : primary->functions.functions) {
		for (int drop = 0; drop < (TakesOptions(f) ? 2 : 1); ++drop) {
			const Value options = Options(drop != 0, false);
			unique_ptr<FunctionData> bind;
			AggregateFunction bound(f);
			const std::string t = Bind(f, TakesOptions(f) ? &options : nullptr, true, &bind, &bound);
			printf(" pass %s%s%s -> %s\n", f.name.c_str(), Types(f.arguments).c_str(),
			       !TakesOptions(f) ? "" : (drop ? " null_policy=drop_y_zero_x" : " null_policy=drop"), t.c_str());
			if (t.compare(0, 6, "error:") == 0) continue;
			std::string variants; // in kVariants' order; PRESERVE_INPUT is the window functions' segment tree
			for (auto &variant : kVariants)
				if (window || variant.combine_type != AggregateCombineType::PRESERVE_INPUT) variants += " " + RunPass(bound, bind.get(), rows, variant);
			printf("  variants%s\n", variants.c_str());
			if (drop) continue;
			std::string texts;
			InRow two {0, false, 1.0, false, {1.0, 2.0}, {0, 0}, false, 1.0, 1}, three {0, false, 2.0, false, {1.0, 2.0, 3.0}, {0, 0, 0}, false, 1.0, 1};
			RunErrorCase(texts, "1", bound, bind.get(), {two, three}, (idx_t)-1);
			InRow null_y_three = three;
			null_y_three.y_null = true;
			RunErrorCase(texts, "2", bound, bind.get(), {two, null_y_three}, (idx_t)-1);
			RunCombineError(texts, bound, bind.get(), 2, 3);
			InRow wide {0, false, 1.0, false, std::vector<double>(129, 1.0), std::vector<uint8_t>(129, 0), false, 1.0, 1};
			RunErrorCase(texts, "4", bound, bind.get(), {wide}, (idx_t)-1);
			InRow wide_null_y = wide;
			wide_null_y.y_null = true;
			RunErrorCase(texts, "5", bound, bind.get(), {wide_null_y}, (idx_t)-1);
			RunErrorCase(texts, "6", bound, bind.get(), {two}, Shape(f).has_y ? 1 : 0);
			printf("  errors %s\n", Interned("E", texts).c_str());
		}
	}
}

// ---- --time: rows per second through Update ----
void TimeUpdate(const char *label, void (*reg)(ExtensionLoader &), const char *name, bool with_split) {
	ExtensionLoader loader;
	reg(loader);
	const AggregateFunction *pick = nullptr;
	for (auto &f : loader.registered.at(name).functions.functions) {
		const Shape s(f);
		if (!s.options && s.split == with_split) pick = &f;
	}
	if (!pick) throw std::runtime_error(std::string("no overload of ") + name);
	unique_ptr<FunctionData> bind;
	AggregateFunction fn(*pick);
	Bind(*pick, nullptr, true, &bind, &fn);
	const Shape shape(fn);
	ArenaAllocator alloc;
	AggregateInputData aid(bind.get(), alloc);
	constexpr size_t kRows = 1000000, kVector = 2048, kStates = 64, kP = 4;
	// the vectors are built once and fed again and again: only Update is timed
	std::vector<InRow> rows(kVector);
	for (size_t i = 0; i < kVector; ++i) {
		rows[i] = InRow {0, i % 97 == 0, (double)(i % 13), false, {}, std::vector<uint8_t>(kP, 0), false, 1.0 + (double)(i % 3), 1 + (int)(i % 3)};
		for (size_t j = 0; j < kP; ++j) rows[i].x.push_back((double)((i + 3 * j) % 11) + 1.0);
	}
	std::vector<const InRow *> in;
	for (auto &r : rows) in.push_back(&r);
	std::vector<Vector> inputs = InputVectors(shape, in, false);
	States states(fn, aid);
	std::vector<data_ptr_t> pool, row_states(kVector);
	for (size_t k = 0; k < kStates; ++k) pool.push_back(states.New());
	for (size_t i = 0; i < kVector; ++i) row_states[i] = pool[i % kStates];
	Vector sv = PointerVector(row_states);
	const auto t0 = std::chrono::steady_clock::now();
	size_t fed = 0;
	while (fed < kRows) {
		const size_t cnt = std::min(kVector, kRows - fed);
		fn.update(inputs.data(), aid, inputs.size(), sv, cnt);
		fed += cnt;
	}
	const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	printf("%s %.0f\n", label, (double)fed / seconds);
}

} // namespace

int main(int argc, char **argv) {
	unsetenv("ANOFOX_HIP_DEVICES"); // (the moment arena reads them)
	unsetenv("ANOFOX_HIP_UNREFINED");
	try {
		if (argc > 1 && std::string(argv[1]) == "--time") {
			g_quiet = true;
			TimeUpdate("ols_fit_predict_agg", RegisterHipOlsFitPredictAggregateFunction, "anofox_stats_ols_fit_predict_agg", true);
			TimeUpdate("wls_fit_predict_agg", RegisterHipWlsFitPredictAggregateFunction, "anofox_stats_wls_fit_predict_agg", true);
			TimeUpdate("rls_fit_predict_agg", RegisterHipRlsFitPredictAggregateFunction, "anofox_stats_rls_fit_predict_agg", true);
			TimeUpdate("ols_fit_predict", RegisterHipOlsFitPredictFunction, "anofox_stats_ols_fit_predict", false);
			return 0;
		}
		printf("== (a) registration ==\n");
		for (auto &r : kRegistrations) PrintRegistration(r);
		printf("== (b) binds ==\n");
		for (auto &r : kRegistrations) PrintBinds(r);
		printf("== (c) updates ==\n");
		printf("variants of a pass, in order: %s | %s | %s (the window functions only)\n", kVariants[0].name, kVariants[1].name, kVariants[2].name);
		printf("errors of a pass, one state each: 1 a later row of another feature count | 2 the same, its y NULL | 3 combining a state of 2 features into one "
		       "of 3 | 4 a row of 129 features | 5 the same, its y NULL | 6 fewer input arguments than the function takes\n");
		for (auto &r : kRegistrations) PrintUpdates(r);
	} catch (const std::exception &e) {
		printf("glue_transcript: unexpected exception: %s\n", e.what());
		return 1;
	}
	return 0;
}
