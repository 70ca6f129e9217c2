// rls_family_hip.hpp — registration of the recursive least squares functions over the batched C ABI (rls_family_hip.cpp).
// The extension entry point calls these instead of
//   RegisterRlsAggregateFunction              (src/aggregate_functions/rls_aggregate.cpp)
//   RegisterRlsFitPredictAggregateFunction    (src/aggregate_functions/rls_predict_aggregate.cpp)
//   RegisterRlsFitPredictFunction             (src/window_functions/rls_fit_predict.cpp)
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_rls_fit_agg, rls_fit_agg
void RegisterHipRlsAggregateFunction(ExtensionLoader &loader);
// anofox_stats_rls_fit_predict_agg, rls_fit_predict_agg, rls_predict_agg, anofox_stats_rls_predict_agg
void RegisterHipRlsFitPredictAggregateFunction(ExtensionLoader &loader);
// anofox_stats_rls_fit_predict, rls_fit_predict (window aggregate)
void RegisterHipRlsFitPredictFunction(ExtensionLoader &loader);
} // namespace duckdb
