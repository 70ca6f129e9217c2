// eb_shrink_capi.cpp — C entry points for tests/test_gpu_eb_shrink_glue.py and tests/test_eb_shrink_glue_cpu.py: drives
// duckdb_shim/eb_shrink_hip.cpp (compiled against the stand-in of DuckDB's headers) on top of the REAL library, the way
// DuckDB's parallel hash aggregate drives an aggregate function (glue_driver.hpp describes it): thread-local states fed by
// Update vectors (optionally dictionary vectors), Combine (ALLOW_DESTRUCTIVE) into the global states, Finalize vector by
// vector with a result offset, Destroy.
//
// ParseOptionSpec and the stand-in's loader come from glue_driver.hpp; the two DOUBLE inputs (estimate, se) and the result
// STRUCT(mu, mu_se, tau_squared, i_squared, q, n_groups, shrunken LIST(STRUCT(...))) are handled here.
// Test infrastructure; builds into anofox-statistics_amd/duckdb_shim/libanofox_eb_shrink_capi.so (duckdb_shim/Makefile).
#include "glue_driver.hpp"

#include "../../anofox-statistics_amd/duckdb_shim/eb_shrink_hip.hpp"

using namespace glue_driver;

namespace {

struct EbOut {
	std::vector<uint8_t> is_null; // per group
	std::vector<double> summary;  // [groups x 6]: mu, mu_se, tau_squared, i_squared, q, n_groups; NaN for a NULL group
	std::vector<int64_t> offsets; // per group its slice of the rows
	std::vector<double> rows;     // [entries x 5]: estimate, se, shrunken, shrunken_se, weight
};

class EbQuery {
public:
	EbQuery(const std::string &fn_name, const char *options_spec, bool as_map, bool foldable) {
		RegisterEbShrinkHip(loader_);
		auto it = loader_.registered.find(fn_name);
		if (it == loader_.registered.end()) throw std::runtime_error("no such function: " + fn_name);
		vector<LogicalType> want = {LogicalType::DOUBLE, LogicalType::DOUBLE};
		if (options_spec) want.push_back(LogicalType::ANY);
		const AggregateFunction *pick = nullptr;
		for (auto &f : it->second.functions.functions)
			if (f.arguments == want) pick = &f;
		if (!pick) throw std::runtime_error("no overload with these argument types");
		fn_.reset(new AggregateFunction(*pick));
		vector<unique_ptr<Expression>> args;
		for (size_t k = 0; k < 2; ++k) args.push_back(make_uniq<Expression>(Value(), false)); // column references
		if (options_spec) {
			const std::string spec = options_spec;
			Value v = spec == "<scalar>" ? Value::DOUBLE(1.0) : (spec == "<null>" ? Value() : ParseOptionSpec(spec, as_map));
			args.push_back(make_uniq<Expression>(v, foldable));
		}
		bind_ = fn_->bind(context_, *fn_, args);
		const LogicalType &t = fn_->return_type;
		if (t.id() != LogicalTypeId::STRUCT || t.children().size() != 7) throw std::runtime_error("bind did not set the result STRUCT");
		const LogicalType &l = t.children()[6].second;
		if (l.id() != LogicalTypeId::LIST || l.children()[0].second.id() != LogicalTypeId::STRUCT || l.children()[0].second.children().size() != 5)
			throw std::runtime_error("the result's last field is not a LIST of five-field STRUCTs");
	}
	const ExtensionLoader &Loader() const { return loader_; }
	const LogicalType &ReturnType() const { return fn_->return_type; }

	EbOut GroupBy(const Inputs &in, const uint32_t *key, size_t n_keys, int n_threads, size_t vector_size, bool dictionary) {
		if (n_threads < 1) n_threads = 1;
		std::vector<std::vector<data_ptr_t>> local(n_threads, std::vector<data_ptr_t>(n_keys, nullptr));
		std::vector<std::string> errors(n_threads);
		std::vector<std::unique_ptr<FunctionData>> binds;
		for (int t = 0; t < n_threads; ++t) binds.push_back(bind_->Copy()); // every thread works with a copy of the bind data
		auto worker = [&](int t) {
			try {
				ArenaAllocator alloc;
				AggregateInputData aid(binds[t].get(), alloc);
				size_t v = 0;
				for (size_t r0 = 0; r0 < in.n; r0 += vector_size, ++v) {
					if ((int)(v % (size_t)n_threads) != t) continue;
					const size_t cnt = std::min(vector_size, in.n - r0);
					std::vector<size_t> rows(cnt);
					std::vector<data_ptr_t> sp(cnt);
					for (size_t i = 0; i < cnt; ++i) {
						rows[i] = r0 + i;
						data_ptr_t &st = local[t][key[r0 + i]];
						if (!st) st = NewState();
						sp[i] = st;
					}
					UpdateRows(aid, in, rows, sp, dictionary);
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
		for (auto &e : errors)
			if (!e.empty()) { // (a failing query still destroys its states)
				for (auto &l : local) DestroyStates(aid, l, vector_size);
				throw std::runtime_error(e);
			}
		std::vector<data_ptr_t> global(n_keys, nullptr);
		for (size_t k = 0; k < n_keys; ++k) global[k] = NewState();
		EbOut out;
		try {
			for (int t = 0; t < n_threads; ++t) { // thread 0's rows first, then thread 1's ..: the order the tests rebuild
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
			out = FinalizeStates(aid, global, vector_size);
		} catch (...) {
			for (auto &l : local) DestroyStates(aid, l, vector_size);
			DestroyStates(aid, global, vector_size);
			throw;
		}
		for (auto &l : local) DestroyStates(aid, l, vector_size);
		DestroyStates(aid, global, vector_size);
		return out;
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
	void DestroyStates(AggregateInputData &aid, std::vector<data_ptr_t> &states, size_t vector_size) {
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
	// one Update call over the given input rows; dictionary: the inputs arrive as dictionary vectors over reversed data
	void UpdateRows(AggregateInputData &aid, const Inputs &in, const std::vector<size_t> &rows, std::vector<data_ptr_t> &states, bool dictionary) {
		const size_t cnt = rows.size();
		if (cnt == 0) return;
		std::vector<uint32_t> sel(cnt);
		for (size_t i = 0; i < cnt; ++i) sel[i] = (uint32_t)(dictionary ? cnt - 1 - i : i);
		std::vector<Vector> inputs;
		inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
		inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
		const size_t data_inputs = inputs.size();
		if (fn_->arguments.size() > data_inputs) inputs.emplace_back(LogicalType(LogicalType::BIGINT), cnt); // the options constant
		for (size_t i = 0; i < cnt; ++i) {
			const size_t r = rows[i], phys = sel[i];
			FlatVector::GetData<double>(inputs[0])[phys] = in.y[r];
			if (in.y_null && in.y_null[r]) {
				FlatVector::SetNull(inputs[0], phys, true);
				FlatVector::GetData<double>(inputs[0])[phys] = 1e300; // the slot of a NULL holds whatever it holds: the glue must not read it
			}
			FlatVector::GetData<double>(inputs[1])[phys] = in.w[r];
			if (in.w_null && in.w_null[r]) {
				FlatVector::SetNull(inputs[1], phys, true);
				FlatVector::GetData<double>(inputs[1])[phys] = 1e300;
			}
		}
		if (dictionary)
			for (size_t k = 0; k < data_inputs; ++k) inputs[k].MakeDictionary(sel);
		if (inputs.size() > data_inputs) inputs.back().MakeConstant();
		Vector sv = PointerVector(states.data(), cnt);
		fn_->update(inputs.data(), aid, inputs.size(), sv, cnt);
	}
	EbOut FinalizeStates(AggregateInputData &aid, std::vector<data_ptr_t> &states, size_t vector_size) {
		const size_t n = states.size();
		Vector result(fn_->return_type, n ? n : 1);
		for (size_t c0 = 0; c0 < n; c0 += vector_size) {
			const size_t cnt = std::min(vector_size, n - c0);
			Vector sv = PointerVector(states.data() + c0, cnt);
			fn_->finalize(sv, aid, result, cnt, c0);
		}
		EbOut out;
		out.is_null.assign(n, 0);
		out.summary.assign(n * 6, NAN);
		out.offsets.assign(n + 1, 0);
		auto &f = StructVector::GetEntries(result);
		Vector &lv = *f[6];
		auto &rf = StructVector::GetEntries(ListVector::GetEntry(lv));
		for (size_t r = 0; r < n; ++r) {
			out.is_null[r] = !FlatVector::Validity(result).RowIsValid(r);
			out.offsets[r + 1] = out.offsets[r];
			if (out.is_null[r]) continue;
			for (size_t k = 0; k < 5; ++k) out.summary[r * 6 + k] = FlatVector::GetData<double>(*f[k])[r];
			out.summary[r * 6 + 5] = (double)FlatVector::GetData<int64_t>(*f[5])[r];
			const list_entry_t e = ListVector::GetData(lv)[r];
			if (e.offset + e.length > ListVector::GetListSize(lv)) throw std::runtime_error("finalize wrote a bad LIST entry");
			if (ListVector::GetListCapacity(lv) < e.offset + e.length) throw std::runtime_error("LIST child written beyond its reservation");
			out.offsets[r + 1] += (int64_t)e.length;
			for (size_t k = 0; k < e.length; ++k)
				for (size_t c = 0; c < 5; ++c) {
					if (!FlatVector::Validity(*rf[c]).RowIsValid(e.offset + k)) throw std::runtime_error("a row field is NULL");
					out.rows.push_back(FlatVector::GetData<double>(*rf[c])[e.offset + k]);
				}
		}
		return out;
	}

	ExtensionLoader loader_;
	ClientContext context_;
	std::unique_ptr<AggregateFunction> fn_;
	unique_ptr<FunctionData> bind_;
};

} // namespace

extern "C" {
#define EG_API __attribute__((visibility("default")))

static int eg_fail(char *msg, const std::exception &e) {
	if (msg) {
		strncpy(msg, e.what(), 511);
		msg[511] = 0;
	}
	return -1;
}

// options_spec == NULL: the overload without the options argument; "<scalar>": a DOUBLE constant; "<null>": a NULL constant;
// foldable = 0: the options argument is not a constant
EG_API void *eg_open(const char *fn_name, const char *options_spec, int as_map, int foldable, char *msg) {
	try {
		return new EbQuery(fn_name, options_spec, as_map != 0, foldable != 0);
	} catch (const std::exception &e) {
		eg_fail(msg, e);
		return nullptr;
	}
}
EG_API void eg_close(void *q) { delete static_cast<EbQuery *>(q); }
EG_API int eg_registered(void *q, const char *name) { return (int)static_cast<EbQuery *>(q)->Loader().registered.count(name); }
EG_API int eg_registered_count(void *q) { return (int)static_cast<EbQuery *>(q)->Loader().registered.size(); }
// the overloads of a registered name: their argument counts in out[] (at most 8); returns how many
EG_API int eg_overloads(void *q, const char *name, int *out) {
	auto &reg = static_cast<EbQuery *>(q)->Loader().registered;
	auto it = reg.find(name);
	if (it == reg.end()) return -1;
	int k = 0;
	for (auto &f : it->second.functions.functions)
		if (k < 8) out[k++] = (int)f.arguments.size();
	return k;
}
// The result type as text: "name:KIND,..." for the STRUCT's fields, the LIST's row struct in brackets after `shrunken`
// (KIND: DOUBLE, BIGINT, LIST, OTHER); at most 511 bytes.
EG_API void eg_result_type(void *q, char *text) {
	auto kind = [](const LogicalType &t) -> std::string {
		if (t == LogicalType(LogicalType::DOUBLE)) return "DOUBLE";
		if (t == LogicalType(LogicalType::BIGINT)) return "BIGINT";
		if (t.id() == LogicalTypeId::LIST) return "LIST";
		return "OTHER";
	};
	std::string s;
	for (auto &c : static_cast<EbQuery *>(q)->ReturnType().children()) {
		s += (s.empty() ? "" : ",") + c.first + ":" + kind(c.second);
		if (c.second.id() == LogicalTypeId::LIST) {
			s += "[";
			bool first = true;
			for (auto &r : c.second.children()[0].second.children()) {
				s += (first ? "" : ",") + r.first + ":" + kind(r.second);
				first = false;
			}
			s += "]";
		}
	}
	strncpy(text, s.c_str(), 511);
	text[511] = 0;
}
// GROUP BY key over rows (estimate, se): is_null [n_keys], out_summary [n_keys x 6], out_offsets [n_keys + 1], out_rows
// [capacity x 5]; returns the number of output rows, -1 with msg on an error.
EG_API int64_t eg_group_by(void *q, size_t n, const uint32_t *key, size_t n_keys, const double *est, const double *se, const uint8_t *est_null,
                           const uint8_t *se_null, int n_threads, size_t vector_size, int dictionary, size_t capacity, uint8_t *is_null,
                           double *out_summary, int64_t *out_offsets, double *out_rows, char *msg) {
	try {
		Inputs in;
		in.n = n;
		in.y = est;
		in.w = se;
		in.y_null = est_null;
		in.w_null = se_null;
		EbOut r = static_cast<EbQuery *>(q)->GroupBy(in, key, n_keys, n_threads, vector_size, dictionary != 0);
		if (r.rows.size() > capacity * 5) throw std::runtime_error("more output rows than the caller's capacity");
		memcpy(is_null, r.is_null.data(), n_keys);
		memcpy(out_summary, r.summary.data(), n_keys * 6 * sizeof(double));
		memcpy(out_offsets, r.offsets.data(), (n_keys + 1) * sizeof(int64_t));
		if (!r.rows.empty()) memcpy(out_rows, r.rows.data(), r.rows.size() * sizeof(double));
		return (int64_t)(r.rows.size() / 5);
	} catch (const std::exception &e) {
		return eg_fail(msg, e);
	}
}

} // extern "C"
