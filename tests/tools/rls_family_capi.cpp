// rls_family_capi.cpp — C entry points for tests/test_gpu_rls_glue.py and tests/test_rls_cpu.py: drives
// duckdb_shim/rls_family_hip.cpp (compiled against the stand-in of DuckDB's headers) on top of the REAL library through
// family_driver.hpp's FamilyQuery — GroupBy (parallel hash aggregate: thread-local states, Combine, Finalize per vector),
// Window (the naive window aggregator) and TreeWindow (a segment tree's PRESERVE_INPUT Combine).
//
// FamilyQuery registers the regression family through the Register* functions of family_agg_hip.hpp.  This library does not
// link family_agg_hip.cpp: it defines those functions here so that the predict-aggregate slot registers the RLS's
// fit-predict aggregate and the window slot its window function (the driver picks the kind by name: "_agg" = aggregate); the
// vif slot registers the fit aggregate, so that its names, overloads and result type bind through the same loader.
// Test infrastructure; builds into anofox-statistics_amd/duckdb_shim/libanofox_rls_family_capi.so (duckdb_shim/Makefile).
#include "family_driver.hpp"

#include "../../anofox-statistics_amd/duckdb_shim/rls_family_hip.hpp"

namespace duckdb {
void RegisterHipOlsFitPredictAggregateFunction(ExtensionLoader &loader) { RegisterHipRlsFitPredictAggregateFunction(loader); }
void RegisterHipRidgeFitPredictAggregateFunction(ExtensionLoader &) {}
void RegisterHipWlsFitPredictAggregateFunction(ExtensionLoader &) {}
void RegisterHipOlsFitPredictFunction(ExtensionLoader &loader) { RegisterHipRlsFitPredictFunction(loader); }
void RegisterHipRidgeFitPredictFunction(ExtensionLoader &) {}
void RegisterHipWlsFitPredictFunction(ExtensionLoader &) {}
void RegisterHipVifAggregateFunction(ExtensionLoader &loader) { RegisterHipRlsAggregateFunction(loader); }
} // namespace duckdb

using namespace glue_driver;

extern "C" {
#define ENF_API __attribute__((visibility("default")))

static int enf_fail(char *msg, const std::exception &e) {
	if (msg) {
		strncpy(msg, e.what(), 511);
		msg[511] = 0;
	}
	return -1;
}

static Inputs enf_inputs(size_t n, size_t p, const double *y, const double *x, const uint8_t *y_null, const uint8_t *x_null, const uint8_t *xe_null) {
	Inputs in;
	in.n = n;
	in.p = p;
	in.y = y;
	in.x = x;
	in.y_null = y_null;
	in.x_null = x_null;
	in.xe_null = xe_null;
	return in;
}

ENF_API void *enf_open(const char *fn_name, const char *options_spec, int as_map, int with_split, char *msg) {
	try {
		return new FamilyQuery(fn_name, options_spec, as_map != 0, with_split != 0);
	} catch (const std::exception &e) {
		enf_fail(msg, e);
		return nullptr;
	}
}
ENF_API void enf_close(void *q) { delete static_cast<FamilyQuery *>(q); }
ENF_API int enf_registered(void *q, const char *name) { return (int)static_cast<FamilyQuery *>(q)->Loader().registered.count(name); }
// the overloads of a registered name: their argument counts in out[] (at most 8); returns how many
ENF_API int enf_overloads(void *q, const char *name, int *out) {
	auto &reg = static_cast<FamilyQuery *>(q)->Loader().registered;
	auto it = reg.find(name);
	if (it == reg.end()) return -1;
	int k = 0;
	for (auto &f : it->second.functions.functions)
		if (k < 8) out[k++] = (int)f.arguments.size();
	return k;
}
// 0 = LIST(STRUCT) of the aggregate, 1 = STRUCT of the window aggregate; fields = the STRUCT's field count
ENF_API int enf_result_shape(void *q, int *fields) {
	auto *fq = static_cast<FamilyQuery *>(q);
	const LogicalType &t = fq->ReturnType();
	*fields = fq->kind() == FamilyQuery::Kind::PREDICT_AGG ? (int)t.children()[0].second.children().size() : (int)t.children().size();
	return (int)fq->kind();
}
// GROUP BY key: out_offsets [n_keys + 1], out_vals [n x 4] = {y, yhat, yhat_lower, yhat_upper}, out_flags [n] (1 y NULL,
// 2 / 4 / 8 yhat / lower / upper NULL, 16 is_training), is_null [n_keys]; returns the number of output rows
ENF_API int64_t enf_group_by(void *q, size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *y, const double *x, const uint8_t *y_null,
                             const uint8_t *xe_null, const uint8_t *split, int n_threads, size_t vector_size, int64_t *out_offsets, double *out_vals,
                             uint8_t *out_flags, uint8_t *is_null, char *msg) {
	try {
		FamilyOut r = static_cast<FamilyQuery *>(q)->GroupBy(enf_inputs(n, p, y, x, y_null, nullptr, xe_null), split, key, n_keys, n_threads, vector_size, false);
		if (r.flags.size() > n) throw std::runtime_error("more output rows than input rows");
		memcpy(out_offsets, r.offsets.data(), (n_keys + 1) * sizeof(int64_t));
		memcpy(is_null, r.is_null.data(), n_keys);
		if (!r.flags.empty()) {
			memcpy(out_vals, r.vals.data(), r.vals.size() * sizeof(double));
			memcpy(out_flags, r.flags.data(), r.flags.size());
		}
		return (int64_t)r.flags.size();
	} catch (const std::exception &e) {
		return enf_fail(msg, e);
	}
}
// OVER (ROWS BETWEEN preceding PRECEDING AND CURRENT ROW) (leaf = 0), or a segment tree of `leaf`-row leaves with frames of
// back + 1 leaves (one output row per leaf): out [rows x 3], is_null [rows]
ENF_API int enf_window(void *q, size_t n, size_t p, const double *y, const double *x, const uint8_t *y_null, const uint8_t *x_null, size_t preceding,
                       size_t leaf, size_t back, size_t vector_size, double *out, uint8_t *is_null, char *msg) {
	try {
		auto *fq = static_cast<FamilyQuery *>(q);
		const Inputs in = enf_inputs(n, p, y, x, y_null, x_null, nullptr);
		FamilyOut r = leaf ? fq->TreeWindow(in, leaf, back, vector_size) : fq->Window(in, preceding, vector_size);
		memcpy(out, r.vals.data(), r.vals.size() * sizeof(double));
		memcpy(is_null, r.is_null.data(), r.is_null.size());
		return 0;
	} catch (const std::exception &e) {
		return enf_fail(msg, e);
	}
}

// the texts of the two feature-count errors at their smallest (FamilyQuery::FeatureCountErrors): update_msg, combine_msg [512]
ENF_API void enf_feature_count_errors(void *q, char *update_msg, char *combine_msg) {
	std::string update, combine;
	static_cast<FamilyQuery *>(q)->FeatureCountErrors(update, combine);
	strncpy(update_msg, update.c_str(), 511);
	update_msg[511] = 0;
	strncpy(combine_msg, combine.c_str(), 511);
	combine_msg[511] = 0;
}

} // extern "C"
