// elasticnet_family_hip.hpp — registration of the elastic net's fit-predict functions over the batched C ABI
// (elasticnet_family_hip.cpp).  The extension entry point calls these instead of
//   RegisterElasticNetFitPredictAggregateFunction   (src/aggregate_functions/elasticnet_predict_aggregate.cpp)
//   RegisterElasticNetFitPredictFunction            (src/window_functions/elasticnet_fit_predict.cpp)
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_elasticnet_fit_predict_agg, elasticnet_fit_predict_agg, elasticnet_predict_agg, anofox_stats_elasticnet_predict_agg
void RegisterHipElasticNetFitPredictAggregateFunction(ExtensionLoader &loader);
// anofox_stats_elasticnet_fit_predict, elasticnet_fit_predict (window aggregate)
void RegisterHipElasticNetFitPredictFunction(ExtensionLoader &loader);
} // namespace duckdb
