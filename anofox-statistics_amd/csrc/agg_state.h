// agg_state.h — the streaming aggregate state object (agg_state.hip) and what the other Finalize families
// (agg_state_models.hip: elastic net, bounded least squares) share with the regression Finalize.  Internal: nothing here
// is exported.
#pragma once
#include <mutex>
#include <vector>

#include "context.h"

struct AnofoxHipAggState {
	AnofoxHipContext *ctx = nullptr;
	size_t p = 0;
	AnofoxHipBatchOptions opt{};
	std::mutex mu;
	// per-slot state
	double *moments = nullptr;
	int64_t *n_accum = nullptr;
	int32_t *run_start = nullptr, *run_end = nullptr;
	int64_t capacity = 0; // slots allocated
	int64_t n_slots = 0;  // slots in use (largest count announced by the caller)
	int64_t rows = 0;     // rows passed to update so far
	// per-pass scratch (one set: the passes of one state are serialised on the context's stream)
	void *scratch = nullptr;
	size_t scratch_bytes = 0;
	size_t sort_temp_bytes = 0;
	int32_t *counters = nullptr; // [0] runs of the current pass, [1] sticky out-of-range flag (own small allocation)
	// staging of host chunks
	struct Stage {
		void *buf = nullptr;
		size_t bytes = 0;
		hipEvent_t copied = nullptr, done = nullptr;
	} stage[2];
	int next_stage = 0;
	hipStream_t copy_stream = nullptr;
	void *pair_buf = nullptr; // combine: src | dst
	size_t pair_bytes = 0;
	// optional row log (anofox_hip_agg_state_retain_rows): slabs in arrival order
	bool log_only = false;     // p > 8 or HC errors: no moments, the row log IS the state
	bool retain = false;       // asked for
	bool log_dropped = false;  // ... and given up because the budget was exceeded
	size_t log_budget = 0, log_bytes = 0;            // HBM part of the log
	size_t log_host_budget = 0, log_host_bytes = 0;  // page-locked host part (the spill beyond the HBM budget)
	int64_t log_rows = 0;
	std::vector<anofox::RowLogSlab> slabs;
	void *refit_idx = nullptr, *refit_rows = nullptr; // Finalize's refit scratch
	size_t refit_idx_bytes = 0, refit_rows_bytes = 0;
	void *remap_buf = nullptr;
	size_t remap_bytes = 0;
};

namespace anofox {
namespace host {
// Another family's Finalize on a state's logged rows (refit_from_log): its solve stages after the accumulate kernels of an
// unweighted fit, its record length, and where its iteration counts go.  `iterations_field` is the `iterations` member of the
// parameter block behind stages.user: the refit points it at the buffer its own launch writes.
struct ModelRefit {
	SolveStages stages;
	int rec_len;
	int32_t **iterations_field;
	int32_t *d_iterations; // one per row of the records, or nullptr
	int64_t n_records;     // rows of the record buffer the refit writes into
	// the family's record scatter (agg_state_models.hip): record k of src (k_n records of `len` doubles, with src_it[k] when both
	// iteration arrays are given) goes to row rows[k] of dst — or pos[rows[k]] — when that row is in [0, n_dst)
	hipError_t (*scatter)(const double *src, const int32_t *src_it, const int32_t *rows, int64_t k_n, int len, double *dst, int32_t *dst_it,
	                      const int32_t *pos, int64_t n_dst, hipStream_t st);
};
// agg_state.hip (the regression Finalize's helpers, shared)
bool agg_state_attached(AnofoxHipAggState *s, AnofoxError *e);
bool agg_state_reserve_slots(AnofoxHipAggState *s, int64_t n_slots, AnofoxError *e);
bool agg_state_check_slot_flag(AnofoxHipAggState *s, AnofoxError *e); // synchronises the stream
bool agg_state_refit_from_log(AnofoxHipAggState *s, int64_t n, int64_t K, const int32_t *d_list, double *d_records, const int32_t *d_pos,
                              const ModelRefit &model, AnofoxError *e);
} // namespace host
} // namespace anofox
