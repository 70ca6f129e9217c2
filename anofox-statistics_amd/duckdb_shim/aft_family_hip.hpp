// aft_family_hip.hpp — registration of the accelerated failure time (AFT) aggregates over the batched C ABI
// (aft_family_hip.cpp).  The extension entry point calls it instead of
//   RegisterAftAggregateFunction  (src/aggregate_functions/aft_aggregate.cpp)
// and gains anofox_stats_aft_fit_predict_agg, which the reference does not have.
#pragma once

namespace duckdb {
class ExtensionLoader;
// anofox_stats_aft_fit_agg, aft_fit_agg; anofox_stats_aft_fit_predict_agg, aft_fit_predict_agg
void RegisterAftFamilyHip(ExtensionLoader &loader);
} // namespace duckdb
