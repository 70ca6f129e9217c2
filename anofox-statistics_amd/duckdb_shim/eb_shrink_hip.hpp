// eb_shrink_hip.hpp — registration of the empirical-Bayes shrinkage aggregate over the batched C ABI (eb_shrink_hip.cpp).
// The extension entry point calls it instead of
//   RegisterEbShrinkAggregateFunction  (src/aggregate_functions/eb_shrink_aggregate.cpp)
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_eb_shrink_agg, eb_shrink_agg
void RegisterEbShrinkHip(ExtensionLoader &loader);
} // namespace duckdb
