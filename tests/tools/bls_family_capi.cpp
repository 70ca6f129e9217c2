// bls_family_capi.cpp — C entry points for tests/test_gpu_bls_glue.py and tests/test_bls_cpu.py: drives
// duckdb_shim/bls_family_hip.cpp (compiled against the stand-in of DuckDB's headers) on top of the REAL library.
//
// The fit-predict aggregate runs through family_driver.hpp's FamilyQuery (parallel hash aggregate: thread-local states,
// Combine, Finalize per vector): this library defines the regression family's Register* functions so that the
// predict-aggregate slot registers it.  The two fit aggregates return a STRUCT with LIST children, which FamilyQuery does not
// decode: BlsFitQuery below is the same hash aggregate for them (blsf_*).
// Test infrastructure; builds into anofox-statistics_amd/duckdb_shim/libanofox_bls_family_capi.so (duckdb_shim/Makefile).
#include "family_driver.hpp"

#include "../../anofox-statistics_amd/duckdb_shim/bls_family_hip.hpp"

namespace duckdb {
void RegisterHipOlsFitPredictAggregateFunction(ExtensionLoader &loader) { RegisterHipBlsFitPredictAggregateFunction(loader); }
void RegisterHipRidgeFitPredictAggregateFunction(ExtensionLoader &) {}
void RegisterHipWlsFitPredictAggregateFunction(ExtensionLoader &) {}
void RegisterHipOlsFitPredictFunction(ExtensionLoader &) {}
void RegisterHipRidgeFitPredictFunction(ExtensionLoader &) {}
void RegisterHipWlsFitPredictFunction(ExtensionLoader &) {}
void RegisterHipVifAggregateFunction(ExtensionLoader &) {}
} // namespace duckdb

using namespace glue_driver;

namespace {

// bls_fit_agg / nnls_fit_agg as a parallel hash aggregate; out: per key a 3p + 6 record in the library's layout
// (status 0, or NaN with status 100 for a NULL result)
class BlsFitQuery {
public:
	BlsFitQuery(const std::string &fn_name, const char *options_spec, bool as_map) {
		RegisterHipBlsAggregateFunction(loader_);
		RegisterHipBlsNnlsAggregateFunction(loader_);
		auto it = loader_.registered.find(fn_name);
		if (it == loader_.registered.end()) throw std::runtime_error("no such function: " + fn_name);
		vector<LogicalType> want = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE)};
		if (options_spec) want.push_back(LogicalType::ANY);
		const AggregateFunction *pick = nullptr;
		for (auto &f : it->second.functions.functions)
			if (f.arguments == want) pick = &f;
		if (!pick) throw std::runtime_error("no overload with these argument types");
		fn_.reset(new AggregateFunction(*pick));
		vector<unique_ptr<Expression>> args;
		args.push_back(make_uniq<Expression>(Value(), false));
		args.push_back(make_uniq<Expression>(Value(), false));
		if (options_spec) args.push_back(make_uniq<Expression>(ParseOptionSpec(options_spec, as_map), true));
		bind_ = fn_->bind(context_, *fn_, args);
		if (fn_->return_type.id() != LogicalTypeId::STRUCT) throw std::runtime_error("bind did not set a STRUCT return type");
	}
	const ExtensionLoader &Loader() const { return loader_; }
	const LogicalType &ReturnType() const { return fn_->return_type; }

	void GroupBy(const Inputs &in, const uint32_t *key, size_t n_keys, int n_threads, size_t vector_size, double *out, uint8_t *is_null) {
		if (n_threads < 1) n_threads = 1;
		std::vector<std::vector<data_ptr_t>> local(n_threads, std::vector<data_ptr_t>(n_keys, nullptr));
		std::vector<std::string> errors(n_threads);
		std::vector<std::unique_ptr<FunctionData>> binds;
		for (int t = 0; t < n_threads; ++t) binds.push_back(bind_->Copy());
		auto worker = [&](int t) {
			try {
				ArenaAllocator alloc;
				AggregateInputData aid(binds[t].get(), alloc);
				size_t v = 0;
				for (size_t r0 = 0; r0 < in.n; r0 += vector_size, ++v) {
					if ((int)(v % (size_t)n_threads) != t) continue;
					const size_t cnt = std::min(vector_size, in.n - r0);
					std::vector<data_ptr_t> sp(cnt);
					for (size_t i = 0; i < cnt; ++i) {
						data_ptr_t &st = local[t][key[r0 + i]];
						if (!st) st = NewState();
						sp[i] = st;
					}
					Update(aid, in, r0, cnt, sp);
				}
			} catch (const std::exception &e) {
				errors[t] = e.what();
			}
		};
		std::vector<std::thread> th;
		for (int t = 0; t < n_threads; ++t) th.emplace_back(worker, t);
		for (auto &t : th) t.join();
		ArenaAllocator alloc;
		AggregateInputData aid(bind_.get(), alloc, AggregateCombineType::ALLOW_DESTRUCTIVE);
		std::vector<data_ptr_t> global(n_keys, nullptr);
		for (size_t k = 0; k < n_keys; ++k) global[k] = NewState();
		auto cleanup = [&] {
			for (auto &l : local) Destroy(aid, l, vector_size);
			Destroy(aid, global, vector_size);
		};
		try {
			for (auto &e : errors)
				if (!e.empty()) throw std::runtime_error(e);
			for (int t = 0; t < n_threads; ++t) {
				std::vector<data_ptr_t> s, d;
				for (size_t k = 0; k < n_keys; ++k)
					if (local[t][k]) {
						s.push_back(local[t][k]);
						d.push_back(global[k]);
					}
				for (size_t c0 = 0; c0 < s.size(); c0 += vector_size) {
					const size_t cnt = std::min(vector_size, s.size() - c0);
					Vector sv = Pointers(s.data() + c0, cnt), dv = Pointers(d.data() + c0, cnt);
					fn_->combine(sv, dv, aid, cnt);
				}
			}
			Finalize(aid, global, vector_size, in.p, out, is_null);
		} catch (...) {
			cleanup();
			throw;
		}
		cleanup();
	}

private:
	data_ptr_t NewState() {
		data_ptr_t s = new data_t[fn_->state_size(*fn_)];
		fn_->initialize(*fn_, s);
		return s;
	}
	static Vector Pointers(data_ptr_t *ptrs, size_t cnt) {
		Vector v(LogicalType(LogicalType::POINTER), cnt);
		memcpy(FlatVector::GetData<data_ptr_t>(v), ptrs, cnt * sizeof(data_ptr_t));
		return v;
	}
	void Destroy(AggregateInputData &aid, std::vector<data_ptr_t> &states, size_t vector_size) {
		std::vector<data_ptr_t> live;
		for (auto s : states)
			if (s) live.push_back(s);
		for (size_t c0 = 0; c0 < live.size(); c0 += vector_size) {
			const size_t cnt = std::min(vector_size, live.size() - c0);
			Vector sv = Pointers(live.data() + c0, cnt);
			fn_->destructor(sv, aid, cnt);
		}
		for (auto &s : states) {
			delete[] s;
			s = nullptr;
		}
	}
	void Update(AggregateInputData &aid, const Inputs &in, size_t r0, size_t cnt, std::vector<data_ptr_t> &states) {
		std::vector<Vector> inputs;
		inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
		inputs.emplace_back(LogicalType::LIST(LogicalType::DOUBLE), cnt);
		if (fn_->arguments.size() > 2) inputs.emplace_back(LogicalType(LogicalType::BIGINT), cnt); // the options constant
		list_entry_t *le = ListVector::GetData(inputs[1]);
		ListVector::Reserve(inputs[1], cnt * in.p + 1);
		Vector &child = ListVector::GetEntry(inputs[1]);
		double *cv = FlatVector::GetData<double>(child);
		for (size_t i = 0; i < cnt; ++i) {
			const size_t r = r0 + i;
			FlatVector::GetData<double>(inputs[0])[i] = in.y[r];
			if (in.y_null && in.y_null[r]) FlatVector::SetNull(inputs[0], i, true);
			le[i].offset = i * in.p;
			le[i].length = in.p;
			for (size_t j = 0; j < in.p; ++j) {
				cv[i * in.p + j] = in.x[r * in.p + j];
				if (in.xe_null && in.xe_null[r * in.p + j]) {
					FlatVector::Validity(child).SetInvalid(i * in.p + j);
					cv[i * in.p + j] = 1e300; // the slot of a NULL holds whatever it holds: the glue must not read it
				}
			}
			if (in.x_null && in.x_null[r]) FlatVector::SetNull(inputs[1], i, true);
		}
		ListVector::SetListSize(inputs[1], cnt * in.p);
		if (inputs.size() > 2) inputs.back().MakeConstant();
		Vector sv = Pointers(states.data(), cnt);
		fn_->update(inputs.data(), aid, inputs.size(), sv, cnt);
	}
	void Finalize(AggregateInputData &aid, std::vector<data_ptr_t> &states, size_t vector_size, size_t p, double *out, uint8_t *is_null) {
		const size_t n = states.size(), len = 3 * p + 6;
		Vector result(fn_->return_type, n ? n : 1);
		for (size_t c0 = 0; c0 < n; c0 += vector_size) {
			const size_t cnt = std::min(vector_size, n - c0);
			Vector sv = Pointers(states.data() + c0, cnt);
			fn_->finalize(sv, aid, result, cnt, c0);
		}
		auto &f = StructVector::GetEntries(result);
		for (size_t r = 0; r < n; ++r) {
			double *rec = out + r * len;
			for (size_t k = 0; k < len; ++k) rec[k] = NAN;
			is_null[r] = !FlatVector::Validity(result).RowIsValid(r);
			rec[p + 5] = is_null[r] ? 100.0 : 0.0;
			if (is_null[r]) continue;
			const size_t at[3] = {0, p + 6, 2 * p + 6};
			Vector *lists[3] = {f[0].get(), f[7].get(), f[8].get()};
			for (int l = 0; l < 3; ++l) {
				const list_entry_t e = ListVector::GetData(*lists[l])[r];
				if (e.length != p || e.offset + e.length > ListVector::GetListSize(*lists[l])) throw std::runtime_error("finalize wrote a bad LIST entry");
				if (ListVector::GetListCapacity(*lists[l]) < e.offset + e.length) throw std::runtime_error("LIST child written beyond its reservation");
				Vector &child = ListVector::GetEntry(*lists[l]);
				for (size_t j = 0; j < p; ++j) {
					if (l == 0) rec[j] = FlatVector::Validity(child).RowIsValid(e.offset + j) ? FlatVector::GetData<double>(child)[e.offset + j] : NAN;
					else rec[at[l] + j] = FlatVector::GetData<bool>(child)[e.offset + j] ? 1.0 : 0.0;
				}
			}
			rec[p] = FlatVector::Validity(*f[1]).RowIsValid(r) ? FlatVector::GetData<double>(*f[1])[r] : NAN;
			rec[p + 1] = FlatVector::GetData<double>(*f[2])[r];
			rec[p + 2] = FlatVector::GetData<double>(*f[3])[r];
			rec[p + 3] = (double)FlatVector::GetData<int64_t>(*f[4])[r];
			if ((size_t)FlatVector::GetData<int64_t>(*f[5])[r] != p) throw std::runtime_error("n_features differs from the feature count");
			rec[p + 4] = (double)FlatVector::GetData<int64_t>(*f[6])[r];
		}
	}

	ExtensionLoader loader_;
	ClientContext context_;
	std::unique_ptr<AggregateFunction> fn_;
	unique_ptr<FunctionData> bind_;
};

} // namespace

extern "C" {
#define BLS_API __attribute__((visibility("default")))

static int bls_fail(char *msg, const std::exception &e) {
	if (msg) {
		strncpy(msg, e.what(), 511);
		msg[511] = 0;
	}
	return -1;
}

static Inputs bls_inputs(size_t n, size_t p, const double *y, const double *x, const uint8_t *y_null, const uint8_t *x_null, const uint8_t *xe_null) {
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

// ---- the fit aggregates ----
BLS_API void *blsf_open(const char *fn_name, const char *options_spec, int as_map, char *msg) {
	try {
		return new BlsFitQuery(fn_name, options_spec, as_map != 0);
	} catch (const std::exception &e) {
		bls_fail(msg, e);
		return nullptr;
	}
}
BLS_API void blsf_close(void *q) { delete static_cast<BlsFitQuery *>(q); }
BLS_API int blsf_registered(void *q, const char *name) { return (int)static_cast<BlsFitQuery *>(q)->Loader().registered.count(name); }
BLS_API int blsf_overloads(void *q, const char *name, int *out) {
	auto &reg = static_cast<BlsFitQuery *>(q)->Loader().registered;
	auto it = reg.find(name);
	if (it == reg.end()) return -1;
	int k = 0;
	for (auto &f : it->second.functions.functions)
		if (k < 8) out[k++] = (int)f.arguments.size();
	return k;
}
// the result STRUCT: its field count; kinds[k] = 0 DOUBLE, 1 BIGINT, 2 LIST(DOUBLE), 3 LIST(BOOLEAN), -1 anything else
BLS_API int blsf_result_fields(void *q, int *kinds) {
	const LogicalType &t = static_cast<BlsFitQuery *>(q)->ReturnType();
	int k = 0;
	for (auto &c : t.children()) {
		int kind = -1;
		if (c.second == LogicalType(LogicalType::DOUBLE)) kind = 0;
		else if (c.second == LogicalType(LogicalType::BIGINT)) kind = 1;
		else if (c.second == LogicalType::LIST(LogicalType::DOUBLE)) kind = 2;
		else if (c.second == LogicalType::LIST(LogicalType::BOOLEAN)) kind = 3;
		if (k < 16) kinds[k] = kind;
		++k;
	}
	return k;
}
// GROUP BY key: out [n_keys x (3p + 6)] records, is_null [n_keys]
BLS_API int blsf_group_by(void *q, size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *y, const double *x, const uint8_t *y_null,
                          const uint8_t *x_null, const uint8_t *xe_null, int n_threads, size_t vector_size, double *out, uint8_t *is_null, char *msg) {
	try {
		static_cast<BlsFitQuery *>(q)->GroupBy(bls_inputs(n, p, y, x, y_null, x_null, xe_null), key, n_keys, n_threads, vector_size, out, is_null);
		return 0;
	} catch (const std::exception &e) {
		return bls_fail(msg, e);
	}
}

// ---- the fit-predict aggregate (as elasticnet_family_capi.cpp's enf_*) ----
BLS_API void *blsp_open(const char *fn_name, const char *options_spec, int as_map, int with_split, char *msg) {
	try {
		return new FamilyQuery(fn_name, options_spec, as_map != 0, with_split != 0);
	} catch (const std::exception &e) {
		bls_fail(msg, e);
		return nullptr;
	}
}
BLS_API void blsp_close(void *q) { delete static_cast<FamilyQuery *>(q); }
BLS_API int blsp_registered(void *q, const char *name) { return (int)static_cast<FamilyQuery *>(q)->Loader().registered.count(name); }
BLS_API int blsp_overloads(void *q, const char *name, int *out) {
	auto &reg = static_cast<FamilyQuery *>(q)->Loader().registered;
	auto it = reg.find(name);
	if (it == reg.end()) return -1;
	int k = 0;
	for (auto &f : it->second.functions.functions)
		if (k < 8) out[k++] = (int)f.arguments.size();
	return k;
}
BLS_API int blsp_result_fields(void *q) { return (int)static_cast<FamilyQuery *>(q)->ReturnType().children()[0].second.children().size(); }
// GROUP BY key: out_offsets [n_keys + 1], out_vals [n x 4] = {y, yhat, yhat_lower, yhat_upper}, out_flags [n] (1 y NULL,
// 2 / 4 / 8 yhat / lower / upper NULL, 16 is_training), is_null [n_keys]; returns the number of output rows
BLS_API int64_t blsp_group_by(void *q, size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *y, const double *x, const uint8_t *y_null,
                              const uint8_t *x_null, const uint8_t *xe_null, const uint8_t *split, int n_threads, size_t vector_size, int64_t *out_offsets,
                              double *out_vals, uint8_t *out_flags, uint8_t *is_null, char *msg) {
	try {
		FamilyOut r = static_cast<FamilyQuery *>(q)->GroupBy(bls_inputs(n, p, y, x, y_null, x_null, xe_null), split, key, n_keys, n_threads, vector_size, false);
		if (r.flags.size() > n) throw std::runtime_error("more output rows than input rows");
		memcpy(out_offsets, r.offsets.data(), (n_keys + 1) * sizeof(int64_t));
		memcpy(is_null, r.is_null.data(), n_keys);
		if (!r.flags.empty()) {
			memcpy(out_vals, r.vals.data(), r.vals.size() * sizeof(double));
			memcpy(out_flags, r.flags.data(), r.flags.size());
		}
		return (int64_t)r.flags.size();
	} catch (const std::exception &e) {
		return bls_fail(msg, e);
	}
}

// the texts of the two feature-count errors at their smallest (FamilyQuery::FeatureCountErrors): update_msg, combine_msg [512]
BLS_API void blsp_feature_count_errors(void *q, char *update_msg, char *combine_msg) {
	std::string update, combine;
	static_cast<FamilyQuery *>(q)->FeatureCountErrors(update, combine);
	strncpy(update_msg, update.c_str(), 511);
	update_msg[511] = 0;
	strncpy(combine_msg, combine.c_str(), 511);
	combine_msg[511] = 0;
}

} // extern "C"
