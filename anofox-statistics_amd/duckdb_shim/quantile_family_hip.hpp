// quantile_family_hip.hpp — registration of the quantile regression functions over the batched C ABI (quantile_family_hip.cpp).
// The extension entry point calls the first instead of
//   RegisterQuantileFitPredictAggregateFunction   (src/aggregate_functions/quantile_fit_predict_aggregate.cpp)
// and the other two next to it: the tau path and the window aggregate are this project's own functions.
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_quantile_fit_predict_agg, quantile_fit_predict_agg
void RegisterHipQuantileFitPredictAggregateFunction(ExtensionLoader &loader);
// anofox_stats_quantile_path_fit_predict_agg, quantile_path_fit_predict_agg (the tau path, long format)
void RegisterHipQuantilePathFitPredictAggregateFunction(ExtensionLoader &loader);
// anofox_stats_quantile_fit_predict, quantile_fit_predict (window aggregate)
void RegisterHipQuantileFitPredictFunction(ExtensionLoader &loader);
} // namespace duckdb
