// eb_shrink_hip.cpp — DuckDB glue of empirical-Bayes shrinkage over the batched C ABI:
//
//   anofox_stats_eb_shrink_agg(estimate, se[, options])   src/aggregate_functions/eb_shrink_aggregate.cpp (bind data :41-58,
//                                                         result type :60-78, Update :93-120, Combine :122-143, Finalize :145-210)
//
// As the other glue files: the DuckDB state buffers the set's pairs on the host in arrival order (row_glue.hpp's RowBuffer with
// a feature count of 1 that stands for nothing: the estimate in RowBuffer::y, the standard error in RowBuffer::w), Combine
// appends the source's pairs after the target's, and Finalize turns the whole vector of states into ONE call of
// anofox_hip_eb_shrink_batch_host (the states as item ranges, n_cols = 1, strides 1) where the reference makes one
// anofox_eb_shrink call per state.  The glue adds no arithmetic.
//
// Options (RegressionMapOptions::ParseFromValue, map_options_parser.cpp:782-792), STRUCT or MAP literal, keys case-insensitive,
// unknown keys ignored, read only when the argument folds to a constant: tau_squared / tau2 (a NULL value leaves it unset),
// tau_method / shrinkage = dl | dersimonian_laird | dersimonian-laird, none | pooled | complete; any other value, a NULL among
// them, raises the reference's "Unknown tau_method '...'. Expected 'dl' or 'none'.".  The value of tau_squared is not checked
// here: an invalid one gives every set status 1, which is NULL.
//
// NULL rules.  Update skips a row whose estimate or se is NULL (:114-116).  A state with fewer than 2 buffered pairs is NULL
// (:155-158) and never reaches the library; a set whose status is not 0 (fewer than 2 usable pairs, invalid options) is NULL
// (:169-173).  The estimate and se of the output rows are the buffered values as they came.
//
// Compiled and driven in this repository against the stand-in of DuckDB's headers (tests/tools/duckdb_stub), on the GPU with
// the real library (tests/test_gpu_eb_shrink_glue.py through tests/tools/eb_shrink_capi.cpp).
#include <math.h>
#include <string.h>

#include "duckdb.hpp"
#include "duckdb/common/types/data_chunk.hpp"
#include "duckdb/execution/expression_executor.hpp"
#include "duckdb/function/aggregate_function.hpp"
#include "duckdb/main/extension/extension_loader.hpp"
#include "duckdb/parser/parsed_data/create_aggregate_function_info.hpp"

#include "anofox_stats_hip.h"
#include "eb_shrink_hip.hpp"
#include "hip_options.hpp"
#include "row_shapes.hpp"

namespace duckdb {

namespace {
using namespace hip_glue;

const vector<string> kCategories = {"regression", "shrinkage"};

struct HipEbShrinkOptions {
	int method = 0;           // ANOFOX_TAU_DERSIMONIAN_LAIRD, eb_shrink_aggregate.cpp:42
	double tau_squared = NAN; // NaN: estimate it, :43
	bool operator==(const HipEbShrinkOptions &o) const {
		return method == o.method && ((isnan(tau_squared) && isnan(o.tau_squared)) || tau_squared == o.tau_squared); // :55
	}
};

void ParseHipEbShrinkOptions(const Value &v, HipEbShrinkOptions &o) {
	if (v.IsNull()) return;
	VisitOptionEntries(v, [&](const string &key, const Value &val) {
		if (key == "tau_squared" || key == "tau2") {
			if (!val.IsNull()) o.tau_squared = val.GetValue<double>();
		} else if (key == "tau_method" || key == "shrinkage") {
			const string m = val.IsNull() ? string() : OptionString(val);
			if (m == "dl" || m == "dersimonian_laird" || m == "dersimonian-laird") o.method = 0;
			else if (m == "none" || m == "pooled" || m == "complete") o.method = 1;
			else throw InvalidInputException("Unknown tau_method '%s'. Expected 'dl' or 'none'.", m.c_str());
		}
		// every other key: ignored
	});
}

using HipEbShrinkBindData = RowsBindData<HipEbShrinkOptions>;

// Update, (estimate, se[, options]): a pair with a NULL on either side is skipped, every other one is buffered as it is
void EbShrinkUpdate(Vector inputs[], AggregateInputData &, idx_t input_count, Vector &state_vector, idx_t count) {
	if (input_count < 2) ThrowTooFewArguments("eb_shrink_agg");
	UnifiedVectorFormat est_data, se_data, sdata;
	inputs[0].ToUnifiedFormat(count, est_data);
	inputs[1].ToUnifiedFormat(count, se_data);
	state_vector.ToUnifiedFormat(count, sdata);
	auto est = UnifiedVectorFormat::GetData<double>(est_data), se = UnifiedVectorFormat::GetData<double>(se_data);
	auto states = (RowsState **)sdata.data;
	for (idx_t i = 0; i < count; i++) {
		const auto e = est_data.sel->get_index(i), s = se_data.sel->get_index(i);
		if (!est_data.validity.RowIsValid(e) || !se_data.validity.RowIsValid(s)) continue;
		auto &rows = RowsOf(*states[sdata.sel->get_index(i)], 1, false);
		PushRow(rows, est[e], true, true);
		rows.w.push_back(se[s]);
	}
}

// the states of one Finalize vector as the item ranges of one call
struct EbShrinkBatch : RowBatch {
	vector<double> out, summary;
	void Run(const HipEbShrinkBindData &bind) {
		int64_t n = 0;
		for (auto *b : buffers) {
			n += (int64_t)b->Rows();
			offsets.push_back(n);
		}
		y.reserve((size_t)n);
		w.reserve((size_t)n);
		for (auto *b : buffers) {
			y.insert(y.end(), b->y.begin(), b->y.end());
			w.insert(w.end(), b->w.begin(), b->w.end());
		}
		out.resize((size_t)n * 3);
		summary.resize(Groups() * anofox_hip_eb_shrink_summary_len());
		AnofoxHipEbShrinkOptions o;
		memset(&o, 0, sizeof o);
		o.method = bind.opts.method;
		o.tau_squared = bind.opts.tau_squared;
		AnofoxError err;
		memset(&err, 0, sizeof err);
		if (!anofox_hip_eb_shrink_batch_host(nullptr, (int64_t)Groups(), n, offsets.data(), 1, y.data(), 1, w.data(), 1, o, out.data(), summary.data(), &err))
			ThrowAbi(err);
	}
	const double *Summary(idx_t g) const { return &summary[g * 8]; }
	bool Failed(idx_t g) const { return Summary(g)[7] != 0.0; }
};

LogicalType EbShrinkResultType() { // GetEbShrinkResultType, eb_shrink_aggregate.cpp:60-78
	child_list_t<LogicalType> row;
	for (auto *name : {"estimate", "se", "shrunken", "shrunken_se", "weight"}) row.push_back(make_pair(string(name), LogicalType(LogicalType::DOUBLE)));
	child_list_t<LogicalType> children;
	for (auto *name : {"mu", "mu_se", "tau_squared", "i_squared", "q"}) children.push_back(make_pair(string(name), LogicalType(LogicalType::DOUBLE)));
	children.push_back(make_pair("n_groups", LogicalType::BIGINT));
	children.push_back(make_pair("shrunken", LogicalType::LIST(LogicalType::STRUCT(std::move(row)))));
	return LogicalType::STRUCT(std::move(children));
}

// Finalize (:145-210): NULL for a state with fewer than 2 pairs and for a set whose status is not 0; otherwise the summary's
// fields and one row per buffered pair in arrival order
void EbShrinkFinalize(Vector &state_vector, AggregateInputData &aggr_input_data, Vector &result, idx_t count, idx_t offset) {
	auto &bind = aggr_input_data.bind_data->Cast<HipEbShrinkBindData>();
	auto batches = CollectBatches<EbShrinkBatch>(state_vector, result, count, offset, [](const RowBuffer &rows) { return rows.Rows() >= 2; });
	for (auto &kv : batches) kv.second.Run(bind);
	auto &fields = StructVector::GetEntries(result);
	for (auto &kv : batches) {
		auto &b = kv.second;
		for (idx_t g = 0; g < b.Groups(); g++) {
			const idx_t r = b.result_rows[g];
			if (b.Failed(g)) {
				FlatVector::SetNull(result, r, true);
				continue;
			}
			const double *sum = b.Summary(g);
			for (idx_t k = 0; k < 5; k++) FlatVector::GetData<double>(*fields[k])[r] = sum[k];
			FlatVector::GetData<int64_t>(*fields[5])[r] = (int64_t)sum[5];
			const RowBuffer &rows = *b.buffers[g];
			const idx_t n_rows = rows.Rows(), list_offset = AppendListEntry(*fields[6], r, n_rows);
			auto &row_fields = StructVector::GetEntries(ListVector::GetEntry(*fields[6]));
			const double *out = &b.out[(size_t)b.offsets[g] * 3];
			for (idx_t i = 0; i < n_rows; i++) {
				const idx_t at = list_offset + i;
				FlatVector::GetData<double>(*row_fields[0])[at] = rows.y[i];
				FlatVector::GetData<double>(*row_fields[1])[at] = rows.w[i];
				for (idx_t k = 0; k < 3; k++) FlatVector::GetData<double>(*row_fields[2 + k])[at] = out[i * 3 + k];
			}
		}
	}
}

unique_ptr<FunctionData> EbShrinkBind(ClientContext &context, AggregateFunction &function, vector<unique_ptr<Expression>> &arguments) {
	return BindRows<HipEbShrinkOptions>(context, function, arguments, 2, false, ParseHipEbShrinkOptions,
	                                    [](const HipEbShrinkOptions &) { return EbShrinkResultType(); });
}

} // namespace

void RegisterEbShrinkHip(ExtensionLoader &loader) {
	RowsFunctionNames f {"anofox_stats_eb_shrink_agg", "eb_shrink_agg", {}, "Shrinks per-group estimates toward their precision-weighted mean (DerSimonian-Laird).",
	                     kCategories};
	f.base = {LogicalType::DOUBLE, LogicalType::DOUBLE};
	f.base_names = {"estimate", "se"};
	RegisterWithOptions(loader, f, "{'tau_method': 'dl'}", [](const string &fname, const vector<LogicalType> &args) {
		return RowsFunction(fname, args, LogicalType::ANY /* set in bind */, EbShrinkUpdate, RowsCombine<false>, EbShrinkFinalize, EbShrinkBind);
	});
}

} // namespace duckdb
