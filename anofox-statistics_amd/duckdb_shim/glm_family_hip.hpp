// glm_family_hip.hpp — registration of the generalised linear model aggregates over the batched C ABI (glm_family_hip.cpp).
// The extension entry point calls them instead of
//   RegisterPoissonAggregateFunction            (src/aggregate_functions/poisson_aggregate.cpp)
//   RegisterBinomialAggregateFunction           (src/aggregate_functions/binomial_aggregate.cpp)
//   RegisterLogisticAggregateFunction           (src/aggregate_functions/logistic_aggregate.cpp)
//   RegisterPoissonFitPredictAggregateFunction  (src/aggregate_functions/poisson_fit_predict_aggregate.cpp)
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_poisson_fit_agg, poisson_fit_agg
void RegisterHipPoissonAggregateFunction(ExtensionLoader &loader);
// anofox_stats_binomial_fit_agg, binomial_fit_agg
void RegisterHipBinomialAggregateFunction(ExtensionLoader &loader);
// anofox_stats_logistic_fit_agg, logistic_fit_agg (the binomial fit plus accuracy and threshold)
void RegisterHipLogisticAggregateFunction(ExtensionLoader &loader);
// anofox_stats_poisson_fit_predict_agg, poisson_fit_predict_agg (per-row mu with the reference's interval)
void RegisterHipPoissonFitPredictAggregateFunction(ExtensionLoader &loader);
} // namespace duckdb
