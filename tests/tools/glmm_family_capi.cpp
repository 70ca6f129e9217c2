// glmm_family_capi.cpp — C entry points for tests/test_gpu_glmm_glue.py and tests/test_glmm_glue_cpu.py: drives
// duckdb_shim/glmm_family_hip.cpp (compiled against the stand-in of DuckDB's headers) on top of the REAL library, the way
// DuckDB's parallel hash aggregate drives an aggregate function (glue_driver.hpp describes it): thread-local states fed by
// Update vectors (optionally dictionary vectors), Combine (ALLOW_DESTRUCTIVE) into the global states, Finalize vector by
// vector with a result offset, Destroy.
//
// Inputs, ParseOptionSpec and the stand-in's loader come from glue_driver.hpp; what (y, x, group[, split]) needs is here: the
// group column is an id per row that the driver hands over as VARCHAR ("level_number_<id>", longer than an inlined string),
// BIGINT or INTEGER, the split column 'train' / 'TRAINING' / 'test'.  The two result shapes of the family are decoded here:
// glmm_fit_agg's STRUCT (one row of doubles per key and its ranef list) and glmm_fit_predict_agg's LIST of six-field row structs.
// Test infrastructure; builds into anofox-statistics_amd/duckdb_shim/libanofox_glmm_family_capi.so (duckdb_shim/Makefile).
#include "glue_driver.hpp"

#include "../../anofox-statistics_amd/duckdb_shim/glmm_family_hip.hpp"

using namespace glue_driver;

namespace {

enum GroupKind { GROUP_VARCHAR = 0, GROUP_BIGINT = 1, GROUP_INTEGER = 2 };

std::string RenderGroup(int kind, int64_t id) { return (kind == GROUP_VARCHAR ? "level_number_" : "") + std::to_string((long long)id); }

struct GlmmIn {
	const int64_t *group = nullptr;
	const uint8_t *group_null = nullptr, *split_train = nullptr, *split_null = nullptr;
};

struct GlmmOut {
	std::vector<uint8_t> is_null; // per key
	// glmm_fit_agg: `width` doubles per key, NaN for a NULL key: coefficients[q], intercept, var_group, var_residual, icc,
	//   log_likelihood, aic, bic, deviance, n_observations, n_groups, n_features, iterations, converged, random_cov[0], its length,
	//   random_dim, the length of factors, then with inference std_errors[q] .. ci_upper[q], intercept_std_error;  q = the widest
	//   key's coefficient count.  ranef: per key its slice [r_offsets] of {group id (-1: the label is not the driver's rendering
	//   of an id), intercept, se (NaN where NULL or NaN), n}
	size_t q = 0, width = 0;
	std::vector<double> vals;
	std::vector<int64_t> r_offsets;
	std::vector<double> r_vals;
	// glmm_fit_predict_agg: per key its slice of the entries; per entry {y, yhat, yhat_fixed, yhat_lower, yhat_upper} and flags
	// (bit c: field c is NULL; 64 = is_training)
	std::vector<int64_t> offsets;
	std::vector<uint8_t> flags;
};

class GlmmQuery {
public:
	GlmmQuery(const std::string &fn_name, const char *options_spec, bool as_map, bool foldable, int group_kind, bool with_split)
	    : group_kind_(group_kind), with_split_(with_split) {
		RegisterGlmmFamilyHip(loader_);
		auto it = loader_.registered.find(fn_name);
		if (it == loader_.registered.end()) throw std::runtime_error("no such function: " + fn_name);
		vector<LogicalType> want = {LogicalType::DOUBLE, LogicalType::LIST(LogicalType::DOUBLE), LogicalType::ANY};
		if (with_split) want.push_back(LogicalType::VARCHAR);
		if (options_spec) want.push_back(LogicalType::ANY);
		const AggregateFunction *pick = nullptr;
		for (auto &f : it->second.functions.functions)
			if (f.arguments == want) pick = &f;
		if (!pick) throw std::runtime_error("no overload with these argument types");
		fn_.reset(new AggregateFunction(*pick));
		vector<unique_ptr<Expression>> args;
		for (size_t k = 0; k < (with_split ? 4u : 3u); ++k) args.push_back(make_uniq<Expression>(Value(), false)); // column references
		if (options_spec) {
			const std::string spec = options_spec;
			Value v = spec == "<scalar>" ? Value::DOUBLE(1.0) : (spec == "<null>" ? Value() : ParseOptionSpec(spec, as_map));
			args.push_back(make_uniq<Expression>(v, foldable));
		}
		bind_ = fn_->bind(context_, *fn_, args);
		const LogicalType &t = fn_->return_type;
		predict_ = t.id() == LogicalTypeId::LIST;
		if (predict_) {
			if (t.children()[0].second.id() != LogicalTypeId::STRUCT || t.children()[0].second.children().size() != 6)
				throw std::runtime_error("bind did not set fit-predict's LIST(STRUCT) return type");
		} else {
			if (t.id() != LogicalTypeId::STRUCT) throw std::runtime_error("bind did not set a STRUCT return type");
			const size_t n = t.children().size();
			inference_ = n == 24;
			if (!inference_ && n != 18) throw std::runtime_error("the result STRUCT's field count fits neither shape of glmm_fit_agg");
		}
	}
	const ExtensionLoader &Loader() const { return loader_; }
	const LogicalType &ReturnType() const { return fn_->return_type; }

	GlmmOut GroupBy(const Inputs &in, const GlmmIn &gin, const uint32_t *key, size_t n_keys, int n_threads, size_t vector_size, bool dictionary) {
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
					UpdateRows(aid, in, gin, rows, sp, dictionary);
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
		GlmmOut out;
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
	void UpdateRows(AggregateInputData &aid, const Inputs &in, const GlmmIn &gin, const std::vector<size_t> &rows, std::vector<data_ptr_t> &states, bool dictionary) {
		const size_t cnt = rows.size();
		if (cnt == 0) return;
		std::vector<uint32_t> sel(cnt);
		for (size_t i = 0; i < cnt; ++i) sel[i] = (uint32_t)(dictionary ? cnt - 1 - i : i);
		std::vector<Vector> inputs;
		inputs.emplace_back(LogicalType(LogicalType::DOUBLE), cnt);
		inputs.emplace_back(LogicalType::LIST(LogicalType::DOUBLE), cnt);
		inputs.emplace_back(LogicalType(group_kind_ == GROUP_VARCHAR ? LogicalType::VARCHAR : (group_kind_ == GROUP_BIGINT ? LogicalType::BIGINT : LogicalType::INTEGER)), cnt);
		if (with_split_) inputs.emplace_back(LogicalType(LogicalType::VARCHAR), cnt);
		const size_t data_inputs = inputs.size();
		if (fn_->arguments.size() > data_inputs) inputs.emplace_back(LogicalType(LogicalType::BIGINT), cnt); // the options constant
		list_entry_t *le = ListVector::GetData(inputs[1]);
		Vector &child = ListVector::GetEntry(inputs[1]);
		size_t total = 0;
		for (size_t i = 0; i < cnt; ++i) total += in.x_len ? in.x_len[rows[i]] : in.p;
		ListVector::Reserve(inputs[1], total ? total : 1);
		double *cv = FlatVector::GetData<double>(child);
		size_t off = 0;
		for (size_t i = 0; i < cnt; ++i) {
			const size_t r = rows[i], phys = sel[i];
			FlatVector::GetData<double>(inputs[0])[phys] = in.y[r];
			if (in.y_null && in.y_null[r]) {
				FlatVector::SetNull(inputs[0], phys, true);
				FlatVector::GetData<double>(inputs[0])[phys] = 1e300; // the slot of a NULL holds whatever it holds: the glue must not read it
			}
			const bool g_null = gin.group_null && gin.group_null[r]; // (the slot of a NULL holds a value that is no row's)
			const int64_t gid = g_null ? 987654321 : gin.group[r];
			if (group_kind_ == GROUP_VARCHAR) FlatVector::GetData<string_t>(inputs[2])[phys] = inputs[2].AddString(RenderGroup(group_kind_, gid));
			else if (group_kind_ == GROUP_BIGINT) FlatVector::GetData<int64_t>(inputs[2])[phys] = gid;
			else FlatVector::GetData<int32_t>(inputs[2])[phys] = (int32_t)gid;
			if (g_null) FlatVector::SetNull(inputs[2], phys, true);
			if (with_split_) {
				FlatVector::GetData<string_t>(inputs[3])[phys] = inputs[3].AddString(gin.split_train[r] ? (r % 2 ? "train" : "TRAINING") : "test");
				if (gin.split_null && gin.split_null[r]) FlatVector::SetNull(inputs[3], phys, true);
			}
			const size_t len = in.x_len ? in.x_len[r] : in.p;
			le[phys].offset = off;
			le[phys].length = len;
			for (size_t j = 0; j < len; ++j) {
				cv[off + j] = j < in.p ? in.x[r * in.p + j] : 0.0;
				if (in.xe_null && j < in.p && in.xe_null[r * in.p + j]) {
					FlatVector::Validity(child).SetInvalid(off + j);
					cv[off + j] = 1e300;
				}
			}
			off += len;
			if (in.x_null && in.x_null[r]) FlatVector::SetNull(inputs[1], phys, true);
		}
		ListVector::SetListSize(inputs[1], total);
		if (dictionary)
			for (size_t k = 0; k < data_inputs; ++k) inputs[k].MakeDictionary(sel);
		if (inputs.size() > data_inputs) inputs.back().MakeConstant();
		Vector sv = PointerVector(states.data(), cnt);
		fn_->update(inputs.data(), aid, inputs.size(), sv, cnt);
	}
	static list_entry_t CheckedEntry(Vector &lv, size_t r) {
		const list_entry_t e = ListVector::GetData(lv)[r];
		if (e.offset + e.length > ListVector::GetListSize(lv)) throw std::runtime_error("finalize wrote a bad LIST entry");
		if (ListVector::GetListCapacity(lv) < e.offset + e.length) throw std::runtime_error("LIST child written beyond its reservation");
		return e;
	}
	GlmmOut FinalizeStates(AggregateInputData &aid, std::vector<data_ptr_t> &states, size_t vector_size) {
		const size_t n = states.size();
		Vector result(fn_->return_type, n ? n : 1);
		for (size_t c0 = 0; c0 < n; c0 += vector_size) {
			const size_t cnt = std::min(vector_size, n - c0);
			Vector sv = PointerVector(states.data() + c0, cnt);
			fn_->finalize(sv, aid, result, cnt, c0);
		}
		GlmmOut out;
		out.is_null.assign(n, 0);
		for (size_t r = 0; r < n; ++r) out.is_null[r] = !FlatVector::Validity(result).RowIsValid(r);
		if (predict_) {
			out.offsets.assign(n + 1, 0);
			auto &f = StructVector::GetEntries(ListVector::GetEntry(result));
			for (size_t r = 0; r < n; ++r) {
				out.offsets[r + 1] = out.offsets[r];
				if (out.is_null[r]) continue;
				const list_entry_t e = CheckedEntry(result, r);
				out.offsets[r + 1] += (int64_t)e.length;
				for (size_t k = 0; k < e.length; ++k) {
					const size_t at = e.offset + k;
					uint8_t fl = 0;
					for (size_t c = 0; c < 5; ++c) {
						const bool ok = FlatVector::Validity(*f[c]).RowIsValid(at);
						if (!ok) fl |= (uint8_t)(1u << c);
						out.vals.push_back(ok ? FlatVector::GetData<double>(*f[c])[at] : NAN);
					}
					if (FlatVector::GetData<bool>(*f[5])[at]) fl |= 64;
					out.flags.push_back(fl);
				}
			}
			return out;
		}
		auto &f = StructVector::GetEntries(result);
		size_t q = 0;
		for (size_t r = 0; r < n; ++r)
			if (!out.is_null[r]) q = std::max<size_t>(q, ListVector::GetData(*f[0])[r].length);
		out.q = q;
		out.width = q + 17 + (inference_ ? 5 * q + 1 : 0);
		out.vals.assign(n * out.width, NAN);
		out.r_offsets.assign(n + 1, 0);
		for (size_t r = 0; r < n; ++r) {
			out.r_offsets[r + 1] = out.r_offsets[r];
			if (out.is_null[r]) continue;
			double *c = &out.vals[r * out.width];
			auto copy_list = [&](Vector &lv, double *dst, size_t most) {
				const list_entry_t e = CheckedEntry(lv, r);
				if (e.length > most) throw std::runtime_error("finalize wrote a bad LIST entry");
				if (e.length) memcpy(dst, FlatVector::GetData<double>(ListVector::GetEntry(lv)) + e.offset, e.length * sizeof(double));
				return (double)e.length;
			};
			size_t k = 0;
			copy_list(*f[k++], c, q);
			for (size_t d = 0; d < 8; ++d) c[q + d] = FlatVector::GetData<double>(*f[k++])[r]; // intercept .. deviance
			for (size_t d = 0; d < 3; ++d) c[q + 8 + d] = (double)FlatVector::GetData<int64_t>(*f[k++])[r];
			c[q + 11] = (double)FlatVector::GetData<int32_t>(*f[k++])[r];
			c[q + 12] = FlatVector::GetData<bool>(*f[k++])[r] ? 1.0 : 0.0;
			c[q + 14] = copy_list(*f[k++], c + q + 13, 1); // random_cov and its length
			c[q + 15] = (double)FlatVector::GetData<int32_t>(*f[k++])[r];
			c[q + 16] = (double)CheckedEntry(*f[k++], r).length; // factors
			if (inference_) {
				for (size_t d = 0; d < 5; ++d) copy_list(*f[k++], c + q + 17 + d * q, q);
				c[6 * q + 17] = FlatVector::GetData<double>(*f[k++])[r];
			}
			Vector &ranef = *f[k];
			const list_entry_t e = CheckedEntry(ranef, r);
			auto &rf = StructVector::GetEntries(ListVector::GetEntry(ranef));
			out.r_offsets[r + 1] += (int64_t)e.length;
			const std::string prefix = group_kind_ == GROUP_VARCHAR ? "level_number_" : "";
			for (size_t j = 0; j < e.length; ++j) {
				const size_t at = e.offset + j;
				const std::string label = FlatVector::GetData<string_t>(*rf[0])[at].GetString();
				int64_t id = -1;
				if (label.size() > prefix.size()) {
					const long long v = atoll(label.c_str() + prefix.size());
					if (RenderGroup(group_kind_, v) == label) id = v;
				}
				out.r_vals.push_back((double)id);
				out.r_vals.push_back(FlatVector::GetData<double>(*rf[1])[at]);
				out.r_vals.push_back(FlatVector::Validity(*rf[2]).RowIsValid(at) ? FlatVector::GetData<double>(*rf[2])[at] : NAN);
				out.r_vals.push_back((double)FlatVector::GetData<int64_t>(*rf[3])[at]);
			}
		}
		return out;
	}

	ExtensionLoader loader_;
	ClientContext context_;
	std::unique_ptr<AggregateFunction> fn_;
	unique_ptr<FunctionData> bind_;
	bool predict_ = false, inference_ = false;
	int group_kind_;
	bool with_split_;
};

} // namespace

extern "C" {
#define AG_API __attribute__((visibility("default")))

static int ag_fail(char *msg, const std::exception &e) {
	if (msg) {
		strncpy(msg, e.what(), 511);
		msg[511] = 0;
	}
	return -1;
}

// options_spec == NULL: the overload without the options argument; "<scalar>": a DOUBLE constant; "<null>": a NULL constant;
// foldable = 0: the options argument is not a constant
// group_kind: 0 VARCHAR, 1 BIGINT, 2 INTEGER; with_split: the overload with the split column
AG_API void *ag_open(const char *fn_name, const char *options_spec, int as_map, int foldable, int group_kind, int with_split, char *msg) {
	try {
		return new GlmmQuery(fn_name, options_spec, as_map != 0, foldable != 0, group_kind, with_split != 0);
	} catch (const std::exception &e) {
		ag_fail(msg, e);
		return nullptr;
	}
}
AG_API void ag_close(void *q) { delete static_cast<GlmmQuery *>(q); }
AG_API int ag_registered(void *q, const char *name) { return (int)static_cast<GlmmQuery *>(q)->Loader().registered.count(name); }
AG_API int ag_registered_count(void *q) { return (int)static_cast<GlmmQuery *>(q)->Loader().registered.size(); }
// the overloads of a registered name: their argument counts in out[] (at most 8; + 100 where argument 3 is VARCHAR, the split
// column); returns how many
AG_API int ag_overloads(void *q, const char *name, int *out) {
	auto &reg = static_cast<GlmmQuery *>(q)->Loader().registered;
	auto it = reg.find(name);
	if (it == reg.end()) return -1;
	int k = 0;
	for (auto &f : it->second.functions.functions)
		if (k < 8) out[k++] = (int)f.arguments.size() + (f.arguments.size() > 3 && f.arguments[3] == LogicalType(LogicalType::VARCHAR) ? 100 : 0);
	return k;
}
// the result's STRUCT (the LIST's row struct, *is_list = 1, or aft_fit_agg's own): its field count; kinds[k] = 0 DOUBLE,
// 1 BOOLEAN, 2 BIGINT, 3 INTEGER, 4 LIST(DOUBLE), 5 LIST(STRUCT(n_levels BIGINT, var DOUBLE)), 6 LIST(STRUCT(group VARCHAR,
// intercept DOUBLE, se DOUBLE, n BIGINT)), -1 anything else; names: the field names joined by ',' (at most 24 / 511 bytes)
AG_API int ag_result_fields(void *q, int *kinds, int *is_list, char *names) {
	const LogicalType &t = static_cast<GlmmQuery *>(q)->ReturnType();
	*is_list = t.id() == LogicalTypeId::LIST;
	const LogicalType &s = *is_list ? t.children()[0].second : t;
	int k = 0;
	std::string joined;
	for (auto &c : s.children()) {
		int kind = -1;
		if (c.second == LogicalType(LogicalType::DOUBLE)) kind = 0;
		else if (c.second == LogicalType(LogicalType::BOOLEAN)) kind = 1;
		else if (c.second == LogicalType(LogicalType::BIGINT)) kind = 2;
		else if (c.second == LogicalType(LogicalType::INTEGER)) kind = 3;
		else if (c.second == LogicalType::LIST(LogicalType::DOUBLE)) kind = 4;
			else if (c.second == LogicalType::LIST(LogicalType::STRUCT({{"n_levels", LogicalType(LogicalTypeId::BIGINT)}, {"var", LogicalType(LogicalTypeId::DOUBLE)}}))) kind = 5;
			else if (c.second == LogicalType::LIST(LogicalType::STRUCT({{"group", LogicalType(LogicalTypeId::VARCHAR)}, {"intercept", LogicalType(LogicalTypeId::DOUBLE)}, {"se", LogicalType(LogicalTypeId::DOUBLE)}, {"n", LogicalType(LogicalTypeId::BIGINT)}}))) kind = 6;
		if (k < 24) kinds[k] = kind;
		joined += (k ? "," : "") + c.first;
		++k;
	}
	strncpy(names, joined.c_str(), 511);
	names[511] = 0;
	return k;
}
// GROUP BY key over rows (y, x[p], group[, split]).  glmm_fit_agg: out_vals [n_keys x width] with width = q + 17 (+ 5 q + 1 with
// inference) <= capacity / n_keys, *out_q = q, out_offsets [n_keys + 1] the keys' slices of out_ranef [.. x 4] (at most
// ranef_capacity entries); returns 0.  glmm_fit_predict_agg: out_offsets [n_keys + 1], out_vals [capacity x 5], out_flags
// [capacity]; returns the number of output entries.  is_null [n_keys].  -1 with msg on an error.
AG_API int64_t ag_group_by(void *q, size_t n, size_t p, const uint32_t *key, size_t n_keys, const double *y, const double *x, const int64_t *group,
                           const uint8_t *y_null, const uint8_t *x_null, const uint8_t *xe_null, const uint8_t *group_null, const uint8_t *split_train,
                           const uint8_t *split_null, const uint32_t *x_len, int n_threads, size_t vector_size, int dictionary, size_t capacity,
                           int64_t *out_offsets, double *out_vals, uint8_t *out_flags, uint8_t *is_null, size_t *out_q, size_t ranef_capacity,
                           double *out_ranef, char *msg) {
	try {
		Inputs in;
		in.n = n;
		in.p = p;
		in.y = y;
		in.x = x;
		in.y_null = y_null;
		in.x_null = x_null;
		in.xe_null = xe_null;
		in.x_len = x_len;
		GlmmIn gin;
		gin.group = group;
		gin.group_null = group_null;
		gin.split_train = split_train;
		gin.split_null = split_null;
		GlmmOut r = static_cast<GlmmQuery *>(q)->GroupBy(in, gin, key, n_keys, n_threads, vector_size, dictionary != 0);
		memcpy(is_null, r.is_null.data(), n_keys);
		if (r.offsets.empty()) {
			if (r.vals.size() > capacity) throw std::runtime_error("more output values than the caller's capacity");
			if (r.r_vals.size() > 4 * ranef_capacity) throw std::runtime_error("more ranef entries than the caller's capacity");
			*out_q = r.q;
			if (!r.vals.empty()) memcpy(out_vals, r.vals.data(), r.vals.size() * sizeof(double));
			memcpy(out_offsets, r.r_offsets.data(), (n_keys + 1) * sizeof(int64_t));
			if (!r.r_vals.empty()) memcpy(out_ranef, r.r_vals.data(), r.r_vals.size() * sizeof(double));
			return 0;
		}
		if (r.flags.size() > capacity) throw std::runtime_error("more output entries than the caller's capacity");
		memcpy(out_offsets, r.offsets.data(), (n_keys + 1) * sizeof(int64_t));
		if (!r.flags.empty()) {
			memcpy(out_vals, r.vals.data(), r.vals.size() * sizeof(double));
			memcpy(out_flags, r.flags.data(), r.flags.size());
		}
		return (int64_t)r.flags.size();
	} catch (const std::exception &e) {
		return ag_fail(msg, e);
	}
}

} // extern "C"
