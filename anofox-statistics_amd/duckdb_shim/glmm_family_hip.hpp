// glmm_family_hip.hpp — registration of the mixed-model aggregates over the batched C ABI (glmm_family_hip.cpp).  The extension
// entry point calls it instead of
//   RegisterGlmmAggregateFunction  (src/aggregate_functions/glmm_aggregate.cpp)
// and gains anofox_stats_glmm_fit_predict_agg, which the reference does not have.
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_glmm_fit_agg, glmm_fit_agg; anofox_stats_glmm_fit_predict_agg, glmm_fit_predict_agg
void RegisterGlmmFamilyHip(ExtensionLoader &loader);
} // namespace duckdb
