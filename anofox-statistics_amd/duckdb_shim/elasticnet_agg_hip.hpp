// elasticnet_agg_hip.hpp — registration of the elastic net aggregate over the batched C ABI (elasticnet_agg_hip.cpp).  The
// extension entry point calls this instead of RegisterElasticNetAggregateFunction
// (src/aggregate_functions/elasticnet_aggregate.cpp in the reference).
#pragma once

namespace duckdb {
class ExtensionLoader;
void RegisterHipElasticNetAggregateFunction(ExtensionLoader &loader); // anofox_stats_elasticnet_fit_agg, elasticnet_fit_agg
} // namespace duckdb
