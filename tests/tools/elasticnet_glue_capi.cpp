// elasticnet_glue_capi.cpp — C entry points for tests/test_gpu_elasticnet_glue.py: drives duckdb_shim/elasticnet_agg_hip.cpp
// (compiled against the stand-in of DuckDB's headers) on top of the REAL library as DuckDB's parallel hash aggregate does —
// worker threads with thread-local states fed by Update vectors, Combine (ALLOW_DESTRUCTIVE) into the global states,
// Finalize vector by vector with a result offset, Destroy.  The option literals are built as glue_driver.hpp builds them.
// Test infrastructure; builds into anofox-statistics_amd/duckdb_shim/libanofox_elasticnet_glue_capi.so (duckdb_shim/Makefile).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "duckdb.hpp"
#include "duckdb/function/aggregate_function.hpp"

#include "../../anofox-statistics_amd/duckdb_shim/elasticnet_agg_hip.hpp"

namespace {
using namespace duckdb;

// "key=value;key=value" -> a STRUCT literal or, as_map, a MAP(VARCHAR, DOUBLE) literal (numbers and booleans)
Value ParseOptionSpec(const std::string &spec, bool as_map) {
	child_list_t<Value> kids;
	size_t at = 0;
	while (at < spec.size()) {
		size_t end = spec.find(';', at);
		if (end == std::string::npos) end = spec.size();
		const std::string item = spec.substr(at, end - at);
		at = end + 1;
		const size_t eq = item.find('=');
		if (eq == std::string::npos) continue;
		const std::string k = item.substr(0, eq), v = item.substr(eq + 1);
		char *e = nullptr;
		const double dv = strtod(v.c_str(), &e);
		if (v == "true" || v == "false") kids.push_back({k, Value::BOOLEAN(v == "true")});
		else if (!v.empty() && e && *e == 0) kids.push_back({k, Value::DOUBLE(dv)});
		else kids.push_back({k, Value(v)});
	}
	if (!as_map) return Value::STRUCT(std::move(kids));
	vector<Value> keys, vals;
	for (auto &k : kids) {
		keys.push_back(Value(k.first));
		vals.push_back(k.second.type().id() == LogicalTypeId::VARCHAR ? k.second : Value::DOUBLE(k.second.GetValue<double>()));
	}
	return Value::MAP(LogicalType::VARCHAR, LogicalType::DOUBLE, keys, vals);
}

class EnQuery {
public:
	EnQuery(const std::string &fn_name, const char *options_spec, bool as_map) {
		RegisterHipElasticNetAggregateFunction(loader_);
		auto it = loader_.registered.find(fn_name);
		if (it == loader_.registered.end()) throw std::runtime_error("no such function: " + fn_name);
		const size_t n_args = options_spec ? 3 : 2;
		const AggregateFunction *pick = nullptr;
		for (auto &f : it->second.functions.functions)
			if (f.arguments.size() == n_args) pick = &f;
		if (!pick) throw std::runtime_error("no overload with that many arguments");
		fn_.reset(new AggregateFunction(*pick));
		vector<unique_ptr<Expression>> args;
		args.push_back(make_uniq<Expression>(Value(), false));
		args.push_back(make_uniq<Expression>(Value(), false));
		if (options_spec) args.push_back(make_uniq<Expression>(ParseOptionSpec(options_spec, as_map), true));
		bind_ = fn_->bind(context_, *fn_, args);
		if (fn_->return_type.id() != LogicalTypeId::STRUCT || fn_->return_type.children().size() != 7)
			throw std::runtime_error("bind did not set the 7-field STRUCT");
	}
	size_t Registered(const char *name) const { return loader_.registered.count(name); }

	// rows r with key[r]; y_null / x_null per row (may be NULL); out_core [n_keys x (p + 6)], last column = n_features
	// x_len: optional LIST length per row (<= p; default p)
	void GroupBy(size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *y, const double *x, const uint8_t *y_null, const uint8_t *x_null,
	             int n_threads, size_t vector_size, double *out_core, uint8_t *is_null, const uint32_t *x_len = nullptr) {
		if (n_threads < 1) n_threads = 1;
		std::vector<std::vector<data_ptr_t>> local(n_threads, std::vector<data_ptr_t>(n_keys, nullptr));
		std::vector<std::string> errors(n_threads);
		std::vector<unique_ptr<FunctionData>> binds;
		for (int t = 0; t < n_threads; ++t) binds.push_back(bind_->Copy());
		auto worker = [&](int t) {
			try {
				ArenaAllocator alloc;
				AggregateInputData aid(binds[t].get(), alloc);
				size_t v = 0;
				for (size_t r0 = 0; r0 < n; r0 += vector_size, ++v) {
					if ((int)(v % (size_t)n_threads) != t) continue;
					const size_t cnt = std::min(vector_size, n - r0);
					std::vector<data_ptr_t> sp(cnt);
					for (size_t i = 0; i < cnt; ++i) {
						data_ptr_t &st = local[t][key[r0 + i]];
						if (!st) st = NewState();
						sp[i] = st;
					}
					Update(aid, r0, cnt, p, y, x, y_null, x_null, x_len, sp);
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
		for (auto &g : global) g = NewState();
		std::string err;
		for (auto &e : errors)
			if (!e.empty()) err = e;
		try {
			if (!err.empty()) throw std::runtime_error(err);
			for (int t = 0; t < n_threads; ++t) {
				std::vector<data_ptr_t> s, d;
				for (size_t k = 0; k < n_keys; ++k)
					if (local[t][k]) {
						s.push_back(local[t][k]);
						d.push_back(global[k]);
					}
				for (size_t c0 = 0; c0 < s.size(); c0 += vector_size) {
					const size_t cnt = std::min(vector_size, s.size() - c0);
					Vector sv = PointerVector(s.data() + c0, cnt), dv = PointerVector(d.data() + c0, cnt);
					fn_->combine(sv, dv, aid, cnt);
				}
			}
			Finalize(aid, global, p, vector_size, out_core, is_null);
		} catch (...) {
			for (auto &l : local) Destroy(aid, l, vector_size);
			Destroy(aid, global, vector_size);
			throw;
		}
		for (auto &l : local) Destroy(aid, l, vector_size);
		Destroy(aid, global, vector_size);
	}

private:
	data_ptr_t NewState() {
		data_ptr_t s = new data_t[fn_->state_size(*fn_)];
		fn_->initialize(*fn_, s);
		return s;
	}
	static Vector PointerVector(data_ptr_t *ptrs, size_t cnt) {
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
			Vector sv = PointerVector(live.data() + c0, cnt);
			fn_->destructor(sv, aid, cnt);
		}
		for (auto &s : states) {
			delete[] s;
			s = nullptr;
		}
	}
	void Update(AggregateInputData &aid, size_t r0, size_t cnt, size_t p, const double *y, const double *x, const uint8_t *y_null, const uint8_t *x_null,
	            const uint32_t *x_len, std::vector<data_ptr_t> &states) {
		std::vector<Vector> inputs;
		inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
		inputs.emplace_back(LogicalType::LIST(LogicalType::DOUBLE), cnt);
		if (fn_->arguments.size() > 2) inputs.emplace_back(LogicalType(LogicalType::BIGINT), cnt);
		double *yv = FlatVector::GetData<double>(inputs[0]);
		list_entry_t *le = ListVector::GetData(inputs[1]);
		ListVector::Reserve(inputs[1], std::max<size_t>(cnt * p, 1));
		double *cv = FlatVector::GetData<double>(ListVector::GetEntry(inputs[1]));
		for (size_t i = 0; i < cnt; ++i) {
			const size_t r = r0 + i;
			yv[i] = y[r];
			if (y_null && y_null[r]) FlatVector::SetNull(inputs[0], i, true);
			le[i].offset = i * p;
			le[i].length = x_len ? x_len[r] : p;
			for (size_t j = 0; j < p; ++j) cv[i * p + j] = x[r * p + j];
			if (x_null && x_null[r]) FlatVector::SetNull(inputs[1], i, true);
		}
		ListVector::SetListSize(inputs[1], cnt * p);
		if (inputs.size() > 2) inputs.back().MakeConstant();
		Vector sv = PointerVector(states.data(), cnt);
		fn_->update(inputs.data(), aid, inputs.size(), sv, cnt);
	}
	void Finalize(AggregateInputData &aid, std::vector<data_ptr_t> &states, size_t p, size_t vector_size, double *out_core, uint8_t *is_null) {
		const size_t n = states.size();
		Vector result(fn_->return_type, n ? n : 1);
		for (size_t c0 = 0; c0 < n; c0 += vector_size) {
			const size_t cnt = std::min(vector_size, n - c0);
			Vector sv = PointerVector(states.data() + c0, cnt);
			fn_->finalize(sv, aid, result, cnt, c0);
		}
		auto &entries = StructVector::GetEntries(result);
		for (size_t r = 0; r < n; ++r) {
			is_null[r] = FlatVector::Validity(result).RowIsValid(r) ? 0 : 1;
			if (is_null[r]) continue;
			double *c = out_core + r * (p + 6);
			const list_entry_t e = ListVector::GetData(*entries[0])[r];
			if (e.length != p || e.offset + e.length > ListVector::GetListSize(*entries[0])) throw std::runtime_error("finalize wrote a bad LIST entry");
			memcpy(c, FlatVector::GetData<double>(ListVector::GetEntry(*entries[0])) + e.offset, p * sizeof(double));
			for (int k = 0; k < 4; ++k) c[p + k] = FlatVector::GetData<double>(*entries[1 + k])[r];
			c[p + 4] = (double)FlatVector::GetData<int64_t>(*entries[5])[r];
			c[p + 5] = (double)FlatVector::GetData<int64_t>(*entries[6])[r];
		}
	}

	ExtensionLoader loader_;
	ClientContext context_;
	std::unique_ptr<AggregateFunction> fn_;
	unique_ptr<FunctionData> bind_;
};

} // namespace

extern "C" {
#define EN_API __attribute__((visibility("default")))

EN_API void *en_open(const char *fn_name, const char *options_spec, int as_map, char *msg) {
	try {
		return new EnQuery(fn_name, options_spec, as_map != 0);
	} catch (const std::exception &e) {
		if (msg) { strncpy(msg, e.what(), 511); msg[511] = 0; }
		return nullptr;
	}
}
EN_API void en_close(void *q) { delete static_cast<EnQuery *>(q); }
EN_API int en_registered(void *q, const char *name) { return (int)static_cast<EnQuery *>(q)->Registered(name); }
EN_API int en_group_by(void *q, size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *y, const double *x, const uint8_t *y_null,
                       const uint8_t *x_null, int n_threads, size_t vector_size, double *out_core, uint8_t *is_null, char *msg) {
	try {
		static_cast<EnQuery *>(q)->GroupBy(n, p, key, n_keys, y, x, y_null, x_null, n_threads, vector_size, out_core, is_null);
		return 0;
	} catch (const std::exception &e) {
		if (msg) { strncpy(msg, e.what(), 511); msg[511] = 0; }
		return -1;
	}
}

// the texts of the two feature-count errors at their smallest: one state given a 2-feature row and then a 3-feature row
// (update_msg), and a 2-feature state combined into a 3-feature state (combine_msg: two worker threads' states of one group);
// both [512].  Both are thrown before Finalize, so no fit is made and no device is needed.
EN_API void en_feature_count_errors(void *q, char *update_msg, char *combine_msg) {
	const double y[2] = {1.0, 2.0}, x[6] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0};
	const uint32_t key[2] = {0, 0};
	double core[3 + 6];
	uint8_t is_null[1];
	auto run = [&](uint32_t first, uint32_t second, bool combining, char *msg) {
		const uint32_t len[2] = {first, second};
		msg[0] = 0;
		try {
			static_cast<EnQuery *>(q)->GroupBy(2, 3, key, 1, y, x, nullptr, nullptr, combining ? 2 : 1, combining ? 1 : 2048, core, is_null, len);
		} catch (const std::exception &e) {
			strncpy(msg, e.what(), 511);
			msg[511] = 0;
		}
	};
	run(2, 3, false, update_msg);
	run(3, 2, true, combine_msg); // the second row's state (2 features) is the source, the first row's (3 features) the target
}

} // extern "C"
