// context.h — the context object and the small host-side helpers shared by the translation units that implement
// the C ABI (host_api.hip, agg_state.hip, the model families).  Internal: nothing here is exported.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "common.h"

struct AnofoxHipContext {
	int device = 0;
	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr;
	std::mutex mu;
	// device workspace (moments, refine queue, direct RSS)
	void *ws = nullptr;
	size_t ws_bytes = 0;
	// device staging for the host-pointer entry points
	void *stage = nullptr;
	size_t stage_bytes = 0;
	// small auxiliary device buffer (t-quantile memo of the predict kernel)
	void *aux = nullptr;
	size_t aux_bytes = 0;
	// run_wide_batch with several slabs of groups: the solve / refinement kernels of slab k run on this stream while the
	// main stream accumulates slab k + 1 (two moment buffers); events per buffer parity
	hipStream_t solve_stream = nullptr;
	hipEvent_t slab_acc_done[2] = {nullptr, nullptr}, slab_solve_done[2] = {nullptr, nullptr};
	const int32_t *last_refine_count = nullptr; // device address of the most recent launch's queue counter
	hipEvent_t gate_wait = nullptr, gate_record = nullptr; // anofox_hip_context_set_accumulate_gate
	// set around a fit call by the window-frame path (frames.hip): group g owns rows [row_offsets[g], frame_ends[g])
	const int64_t *frame_ends = nullptr;
	bool frame_prefix = false; // (r4) the frames of this call extend one another (UNBOUNDED PRECEDING): accumulate_prefix.hip writes their records
	int64_t last_window_flagged = 0; // frames of the last in-register window call that were refitted with refinement
	void *frames_buf = nullptr; // scratch of that path (prefix counts, rule counts, records of one slab of frames)
	size_t frames_bytes = 0;
	// Student-t critical values for df = 1..kWindowTcritCap at the confidence level of the last window call
	void *wtab = nullptr;
	size_t wtab_bytes = 0;
	double wtab_conf = -1.0;
	// the quantile window function's last launch on this context (quantile.hip): per walker {frames begun afresh, of them after
	// a fitted frame} in a buffer of its own, so that no other call overwrites it; reset by every window call
	void *qw_counts = nullptr;
	size_t qw_counts_bytes = 0;
	int64_t qw_frames = 0, qw_walkers = 0, qw_waves = 0, qw_span = 0;
	bool qw_valid = false;
	// the GLM window function's last launch on this context (glm_window.hip): per walker {frames started cold, started warm,
	// warm frames refitted cold, IRLS iterations} as int64 in a buffer of its own; reset by every GLM window call
	void *gw_counts = nullptr;
	size_t gw_counts_bytes = 0;
	int64_t gw_frames = 0, gw_walkers = 0, gw_waves = 0, gw_span = 0;
	bool gw_valid = false;
	// timing
	bool timing = false;
	std::vector<hipEvent_t> free_events;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> acc_events, solve_events, predict_events;
	// streaming aggregate states created on this context (agg_state.hip); destroying the context releases their
	// device memory and leaves them detached (every later call on them fails, destroy still frees the object)
	std::vector<struct AnofoxHipAggState *> agg_states;
};

namespace anofox {
// The ANOFOX_* environment switches ("switches").  Every reader caches its value in a function-local
// `static const`: a switch is read once per process.
inline long long env_int(const char *name, long long dflt) { // the variable's integer value; `dflt` when it is unset
	const char *v = getenv(name);
	return v ? atoll(v) : dflt;
}
inline bool env_is(const char *name, int value) { return getenv(name) && env_int(name, 0) == value; } // set, and to `value`
inline bool env_on(const char *name) { return !env_is(name, 0); } // on unless set to 0 (the A/B switches of shipped choices)

namespace host {
void agg_state_detach(struct AnofoxHipAggState *s); // agg_state.hip
// host_api.hip: the device batch path (accumulate -> solve -> refine) on device-resident inputs, enqueued on the
// context's stream; used by agg_state.hip to refit the queued groups of a state from its row log
bool refit_groups_device(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *d_row_offsets,
                         const double *d_y, const double *const *x_cols, const double *d_w, const AnofoxHipBatchOptions &opt,
                         double *d_core, double *d_inf, AnofoxError *e);
// What follows the accumulate kernels of one launch of the batch path (host_api.hip): the regression models' solve and
// refinement chain, or another model's solve on the same moment records (elasticnet.hip).  `narrow` runs once on the
// narrow records (p <= 8, the context's stream), `wide` once per slab of wide records on the solve stream `st`; `slab`
// is the call's largest slab.
struct SolveStages {
	bool (*narrow)(AnofoxHipContext *ctx, BatchArgs &a, hipStream_t st, void *user, AnofoxError *e);
	bool (*wide)(AnofoxHipContext *ctx, WideArgs &a, hipStream_t st, int64_t slab, void *user, AnofoxError *e);
	void *user;
};
// host_api.hip: the device batch path with the accumulate dispatch of an unweighted fit (opt.model, fit_intercept) and
// `stages` after it; enqueued on the context's stream
bool moment_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *d_row_offsets,
                         const double *d_y, const double *const *x_cols, const AnofoxHipBatchOptions &opt, const SolveStages &stages,
                         double *d_core, AnofoxError *e);
// elasticnet.hip / bls.hip: the two families' option checks, solve parameters (iterations unset) and stages, for the Finalize of
// a streaming state (agg_state_models.hip).  Their narrow stage takes records without rows (BatchArgs::row_offsets == nullptr):
// it then leaves the groups it flags in refine_list[g] to the caller.
bool elasticnet_state_options(const AnofoxHipElasticNetBatchOptions &o, AnofoxError *e);
EnParams elasticnet_state_params(const AnofoxHipElasticNetBatchOptions &o);
SolveStages elasticnet_state_stages(EnParams *en);
bool bls_state_options(const AnofoxHipBlsBatchOptions &o, AnofoxError *e);
BlsParamsT<kWideMaxP> bls_state_params(const AnofoxHipBlsBatchOptions &o, size_t p);
SolveStages bls_state_stages(BlsParamsT<kWideMaxP> *bp);
// glm.hip: the GLM family's option and interval checks, for its window function (glm_window.hip)
bool glm_options_invalid(const AnofoxHipGlmBatchOptions &o);
bool glm_check_interval(const AnofoxHipGlmBatchOptions &o, double z, AnofoxError *e);
// host_api.hip: the predict kernels on fit records in the regression layout, enqueued on the context's stream; the caller
// holds ctx->mu (a family that fits outside the moment path — quantile.hip — keeps one lock over fit and predict)
bool predict_records_locked(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *d_row_offsets,
                            const double *const *x_cols, const double *d_core, double confidence_level, double *d_pred, AnofoxError *e);
// host_api.hip: the context of a host entry point: `ctx`, or for ctx == NULL the calling thread's default context on the
// current device (created on first use; nullptr and `e` set when that fails)
AnofoxHipContext *host_context(AnofoxHipContext *ctx, AnofoxError *e);
// The window path of another model (the elastic net): its solve stages for the frames path, and its in-register window kernels
// for p <= 8 (launch == nullptr: every frame through the frames path)
struct WindowSolve {
	SolveStages stages;
	hipError_t (*launch)(const WindowArgs &a, void *user, hipStream_t st);
	void *user;
};
// host_api.hip: the fit-predict entry points (batch / ROWS window / explicit frames) with another model's solve; `opt` = the
// accumulate options of its moments (an unweighted fit) with the interval's confidence level.  Argument checks first; the
// host forms take ctx == NULL as the thread's default context.
bool model_fit_predict_batch_device(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *d_row_offsets,
                                    const double *d_y, const double *const *x_cols, const int64_t *d_train_counts,
                                    const AnofoxHipBatchOptions &opt, const SolveStages &stages, double *d_core, double *d_pred, AnofoxError *e);
bool model_fit_predict_batch_host(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *row_offsets,
                                  const double *y, const double *const *x_cols, const int64_t *train_counts, const AnofoxHipBatchOptions &opt,
                                  const SolveStages &stages, double *core, double *pred, AnofoxError *e);
bool model_fit_predict_window_device(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *d_row_offsets,
                                     const double *d_y, const double *const *x_cols, const AnofoxHipWindowFrame &frame,
                                     const AnofoxHipBatchOptions &opt, const WindowSolve &ws, double *d_pred, AnofoxError *e);
bool model_fit_predict_window_host(AnofoxHipContext *ctx, int64_t n_groups, size_t p, int64_t n_rows, const int64_t *row_offsets,
                                   const double *y, const double *const *x_cols, const AnofoxHipWindowFrame &frame,
                                   const AnofoxHipBatchOptions &opt, const WindowSolve &ws, double *pred, AnofoxError *e);
bool model_fit_predict_frames_device(AnofoxHipContext *ctx, int64_t n_rows, size_t p, const double *d_y, const double *const *x_cols,
                                     const int64_t *d_frame_lo, const int64_t *d_frame_hi, const AnofoxHipBatchOptions &opt,
                                     const SolveStages &stages, double *d_pred, AnofoxError *e);
bool model_fit_predict_frames_host(AnofoxHipContext *ctx, int64_t n_rows, size_t p, const double *y, const double *const *x_cols,
                                   const int64_t *frame_lo, const int64_t *frame_hi, const AnofoxHipBatchOptions &opt,
                                   const SolveStages &stages, double *pred, AnofoxError *e);
}
}

namespace anofox {
namespace host {


inline void set_error(AnofoxError *e, AnofoxErrorCode code, const std::string &msg) {
	if (!e) return;
	e->code = code;
	const size_t n = msg.size() < 255 ? msg.size() : 255;
	memcpy(e->message, msg.data(), n);
	e->message[n] = 0;
}

inline void reset_error(AnofoxError *e) {
	if (!e) return;
	e->code = ANOFOX_ERROR_SUCCESS;
	memset(e->message, 0, sizeof e->message);
}

inline bool hip_fail(hipError_t rc, const char *what, AnofoxError *e) {
	if (rc == hipSuccess) return false;
	set_error(e, ANOFOX_ERROR_INTERNAL, std::string("HIP error in ") + what + ": " + hipGetErrorString(rc));
	return true;
}

constexpr int kRefineSteps = 2; // iterative-refinement updates applied to queued groups

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline bool ensure_buffer(void **buf, size_t *cap, size_t need, const char *what, AnofoxError *e) {
	if (need <= *cap) return true;
	if (*buf) {
		if (hip_fail(hipFree(*buf), "hipFree", e)) return false; // hipFree synchronises the device
		*buf = nullptr;
		*cap = 0;
	}
	const size_t want = align_up(need + need / 8, 1 << 20);
	if (hipMalloc(buf, want) != hipSuccess) {
		(void)hipGetLastError();
		*buf = nullptr;
		set_error(e, ANOFOX_ERROR_ALLOCATION_FAILURE, std::string("hipMalloc failed for ") + what);
		return false;
	}
	*cap = want;
	return true;
}

// ---- argument checks and input conversion shared by the host entry points ----

inline std::string fmt_g(double v) {
	char buf[64];
	snprintf(buf, sizeof buf, "%g", v);
	return buf;
}

// The argument checks that every batch entry point makes, in their order: the signs, x, the width, the NULL arrays
// (`null_text`), the NULL columns.  Above `max_p` the text is `over_text`, or for nullptr "n_features = <p> exceeds the supported
// maximum of <max_p>", built only then.  by_rows == false: the arrays are needed when G > 0 (the fit entries); true: when
// n_rows > 0, and neither G nor `off` is looked at (the window entries, one output per row).  The context is not checked here:
// every entry keeps its own place for that step and for its family's options.
inline bool check_batch_args(int64_t G, size_t p, int64_t n_rows, const void *off, const void *y, const double *const *x_cols,
                             const void *out, size_t max_p, const char *over_text, const char *null_text, bool by_rows, AnofoxError *e) {
	if ((!by_rows && G < 0) || n_rows < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "negative n_groups or n_rows"); return false; }
	if (p == 0 || !x_cols) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "x is NULL or empty"); return false; }
	if (p > max_p) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT,
		          over_text ? std::string(over_text)
		                    : "n_features = " + std::to_string(p) + " exceeds the supported maximum of " + std::to_string(max_p));
		return false;
	}
	const bool need = by_rows ? n_rows > 0 : G > 0;
	if (need && ((!by_rows && !off) || !y || !out)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, null_text); return false; }
	for (size_t j = 0; j < p; ++j)
		if (need && !x_cols[j]) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "x column pointer is NULL"); return false; }
	return true;
}

// the offsets of a host batch: group g owns rows [off[g], off[g + 1]) of the n_rows that the caller's arrays hold
inline bool check_host_offsets(int64_t G, int64_t n_rows, const int64_t *off, AnofoxError *e) {
	for (int64_t g = 0; g < G; ++g) {
		if (off[g + 1] < off[g] || off[g] < 0 || off[g + 1] > n_rows) {
			set_error(e, ANOFOX_ERROR_INVALID_INPUT, "row_offsets must be non-decreasing and within [0, n_rows]");
			return false;
		}
	}
	return true;
}

// entries with one output per row: every row belongs to a group
inline bool check_whole_range(int64_t G, int64_t n_rows, const int64_t *off, AnofoxError *e) {
	if (G > 0 && (off[0] != 0 || off[G] != n_rows)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "row_offsets must start at 0 and end at n_rows");
		return false;
	}
	return true;
}

// DataArray::to_vec (types.rs:79-89): NULL entries -> NaN through the validity bitmask; rows past a.len, up to len, are NaN
inline void expand_data_array(const AnofoxDataArray &a, std::vector<double> &out, size_t len = 0) {
	out.assign(len > a.len ? len : a.len, NAN);
	for (size_t i = 0; i < a.len; ++i) {
		const bool valid = !a.validity || ((a.validity[i / 8] >> (i % 8)) & 1);
		out[i] = valid ? a.data[i] : NAN;
	}
}

// a malloc'd copy of a result's text (the reference's results own theirs; anofox_free_* frees it); nullptr: no memory
inline char *copy_text(const char *s) {
	char *p = (char *)malloc(strlen(s) + 1);
	if (p) strcpy(p, s);
	return p;
}

inline hipEvent_t get_event(AnofoxHipContext *ctx) {
	if (!ctx->free_events.empty()) {
		hipEvent_t ev = ctx->free_events.back();
		ctx->free_events.pop_back();
		return ev;
	}
	hipEvent_t ev = nullptr;
	(void)hipEventCreate(&ev);
	return ev;
}

} // namespace host
} // namespace anofox
