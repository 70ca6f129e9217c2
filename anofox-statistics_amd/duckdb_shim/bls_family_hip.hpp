// bls_family_hip.hpp — registration of the bounded least squares aggregates over the batched C ABI (bls_family_hip.cpp).
// The extension entry point calls these instead of
//   RegisterBlsAggregateFunction / RegisterNnlsAggregateFunction   (src/aggregate_functions/bls_aggregate.cpp)
//   RegisterBlsFitPredictAggregateFunction                         (src/aggregate_functions/bls_fit_predict_aggregate.cpp)
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_bls_fit_agg, bls_fit_agg
void RegisterHipBlsAggregateFunction(ExtensionLoader &loader);
// anofox_stats_nnls_fit_agg, nnls_fit_agg
void RegisterHipBlsNnlsAggregateFunction(ExtensionLoader &loader);
// anofox_stats_bls_fit_predict_agg, bls_fit_predict_agg
void RegisterHipBlsFitPredictAggregateFunction(ExtensionLoader &loader);
} // namespace duckdb
