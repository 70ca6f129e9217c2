// agg_state_models.hip — anofox_hip_agg_state_finalize_{elasticnet,bls}_*: the elastic net and the bounded / non-negative
// least squares fits finalized from a streaming aggregate state (agg_state.hip).
//
// A state is independent of lambda, l1_ratio and the bounds: its moment records (p <= 8) or its row log (9 <= p <= 128) serve
// the regression Finalize and any number of these, and none of them changes it.  Per call:
//   moment state   the family's narrow stage (elasticnet.hip / bls.hip: one lane per record) on the state's records — or on the
//                  gathered records of the listed slots — with the state's n_accum as the "< 2 rows" rule.  The stage flags the
//                  records whose moment-form ssr has cancelled (refine_list[g] = 1); the batch path answers those from the rows:
//                    compact   the flag array -> the ascending list of flagged slots (one workgroup, prefix counts: the order
//                              is the slot order whatever the scheduling — no atomic queue)
//                    with a row log: the existing log-gather on exactly those slots, the batch path with the family's stages
//                              on their rows, and the records (and iteration counts) scattered back;
//                    without:  the flagged records become NaN with status ANOFOX_HIP_STATUS_UNREFINED, listed and counted.
//   log-only state the batch path with the family's stages over the whole log (or the listed slots' rows).
// No atomics in anything here, and every buffer written is the call's own staging: two calls with the same options give the
// same bits.
#include <algorithm>
#include <string>
#include <vector>

#include "agg_state.h"

using namespace anofox;
using namespace anofox::host;

namespace anofox {
namespace {

constexpr int kCompactBlock = 1024; // 16 wavefronts, each owning one contiguous range of the flags
constexpr int kCompactWaves = kCompactBlock / 64;
constexpr int kScatterBlock = 256;

// flags[0 .. n) -> out_pos[0 .. *count): the indices i with flags[i] != 0, ascending; out_slot[k] = sel[out_pos[k]] when a
// selection is given (the flags of listed slots: positions in, slot numbers out).  ONE workgroup: wavefront w counts the flags of
// its range (coalesced, 4 loads in flight), the 16 counts are prefix-summed through LDS, and the wavefronts that have any write
// theirs behind those of the ranges before them.  The output arrays have room for n entries.
__global__ __launch_bounds__(kCompactBlock) void state_compact_flags_kernel(const int32_t *flags, int64_t n, const uint32_t *sel, int32_t *out_pos,
                                                                            int32_t *out_slot, int32_t *count) {
	__shared__ int s_cnt[kCompactWaves];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int64_t per = ((n + kCompactWaves - 1) / kCompactWaves + 63) / 64 * 64;
	const int64_t lo = (int64_t)wave * per, hi = lo + per < n ? lo + per : n;
	int mine = 0; // (uniform over the wavefront)
	for (int64_t i0 = lo; i0 < hi; i0 += 256) {
		int f[4];
#pragma unroll
		for (int u = 0; u < 4; ++u) {
			const int64_t i = i0 + u * 64 + lane;
			f[u] = i < hi ? flags[i] : 0;
		}
#pragma unroll
		for (int u = 0; u < 4; ++u) mine += __popcll(__ballot(f[u] != 0));
	}
	if (lane == 0) s_cnt[wave] = mine;
	__syncthreads();
	int at = 0, total = 0;
	for (int w = 0; w < kCompactWaves; ++w) {
		const int c = s_cnt[w];
		if (w < wave) at += c;
		total += c;
	}
	if (threadIdx.x == 0) *count = total;
	if (mine == 0) return;
	for (int64_t i0 = lo; i0 < hi; i0 += 64) {
		const int64_t i = i0 + lane;
		const bool on = i < hi && flags[i] != 0;
		const unsigned long long m = __ballot(on);
		if (on) {
			const int k = at + __popcll(m & ((1ull << lane) - 1ull));
			out_pos[k] = (int32_t)i;
			if (sel) out_slot[k] = (int32_t)sel[i];
		}
		at += __popcll(m);
	}
}

// Records of any length to the rows a list names (grid-stride, one element per thread and step).  Record k goes to row rows[k],
// or pos[rows[k]] with a position map; rows outside [0, n_dst) are skipped.  src == nullptr: the record becomes NaN with
// ANOFOX_HIP_STATUS_UNREFINED at [status_at] instead.  The number of records is k_n, or *count (device) when that is given.
__global__ __launch_bounds__(kScatterBlock) void state_scatter_records_kernel(const double *src, const int32_t *src_it, const int32_t *rows,
                                                                              const int32_t *count, int64_t k_n, int len, int status_at, double *dst,
                                                                              int32_t *dst_it, const int32_t *pos, int64_t n_dst) {
	if (count) {
		const int64_t c = *count;
		k_n = c < k_n ? c : k_n;
	}
	const int64_t total = k_n * len;
	for (int64_t t = (int64_t)blockIdx.x * kScatterBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kScatterBlock) {
		const int64_t k = t / len;
		const int j = (int)(t - k * len);
		int64_t row = rows[k];
		if (pos) row = (row >= 0) ? pos[row] : -1;
		if (row < 0 || row >= n_dst) continue;
		double v;
		if (src) v = src[t];
		else v = (j == status_at) ? (double)ANOFOX_HIP_STATUS_UNREFINED : __builtin_nan("");
		dst[(size_t)row * (size_t)len + (size_t)j] = v;
		if (j == 0 && src_it && dst_it) dst_it[row] = src_it[k];
	}
}

unsigned scatter_grid(int64_t elems) {
	int64_t g = (elems + kScatterBlock - 1) / kScatterBlock;
	if (g < 1) g = 1;
	if (g > 4096) g = 4096;
	return (unsigned)g;
}

hipError_t launch_state_compact_flags(const int32_t *flags, int64_t n, const uint32_t *sel, int32_t *out_pos, int32_t *out_slot, int32_t *count,
                                      hipStream_t st) {
	state_compact_flags_kernel<<<1, kCompactBlock, 0, st>>>(flags, n, sel, out_pos, out_slot, count);
	return hipGetLastError();
}

// the flagged records of a state without a log; `count` stays on the device
hipError_t launch_state_flag_unrefined(const int32_t *rows, const int32_t *count, int64_t n, int len, int status_at, double *dst, hipStream_t st) {
	// (how many there are is not known here: a grid for a few thousand records, striding over more)
	state_scatter_records_kernel<<<scatter_grid(std::min<int64_t>(n, 4096) * len), kScatterBlock, 0, st>>>(nullptr, nullptr, rows, count, n, len, status_at,
	                                                                                                      dst, nullptr, nullptr, n);
	return hipGetLastError();
}

hipError_t launch_state_scatter_records(const double *src, const int32_t *src_it, const int32_t *rows, int64_t k_n, int len, double *dst,
                                        int32_t *dst_it, const int32_t *pos, int64_t n_dst, hipStream_t st) {
	if (k_n <= 0) return hipSuccess;
	state_scatter_records_kernel<<<scatter_grid(k_n * len), kScatterBlock, 0, st>>>(src, src_it, rows, nullptr, k_n, len, -1, dst, dst_it, pos, n_dst);
	return hipGetLastError();
}

} // namespace
} // namespace anofox

namespace {

// one family of a call: its stages (whose parameter block the caller owns), record layout and option values
struct Family {
	const char *name;
	SolveStages stages;
	int32_t **iterations_field;
	int rec_len;
	bool fit_intercept;
};

// The state must hold the moments (or rows) of the unweighted fit the family's batch call would accumulate.
bool check_state(AnofoxHipAggState *s, const Family &f, AnofoxError *e) {
	if (s->opt.model != ANOFOX_HIP_MODEL_OLS) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT,
		          std::string(f.name) + " finalize: the state was created with model " + (s->opt.model == ANOFOX_HIP_MODEL_WLS ? "WLS (weights)" : "ridge") +
		              ", it needs the unweighted OLS moments");
		return false;
	}
	if (s->opt.hc_type != ANOFOX_HC_NONE) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, std::string(f.name) + " finalize: the state was created with an hc_type other than none");
		return false;
	}
	if ((s->opt.fit_intercept ? 1 : 0) != (f.fit_intercept ? 1 : 0)) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT,
		          std::string(f.name) + " finalize: fit_intercept of the options differs from the fit_intercept the state was created with");
		return false;
	}
	return true;
}

// staging of one call (the context's staging buffer): records | iterations | flagged positions | flagged slots | counter |
// and for listed slots: list | position map | gathered records | gathered counts
struct Staging {
	double *rec = nullptr;
	int32_t *it = nullptr, *flag_pos = nullptr, *flag_slot = nullptr, *count = nullptr;
	uint32_t *sel = nullptr;
	int32_t *pos = nullptr;
	double *mom = nullptr;
	int64_t *cnt = nullptr;
};

bool carve_staging(AnofoxHipAggState *s, int64_t n, const Family &f, bool listed, Staging *o, AnofoxError *e) {
	AnofoxHipContext *ctx = s->ctx;
	const size_t N = (size_t)n, rec = s->log_only ? 0 : (size_t)moment_record_len((int)s->p);
	const size_t b_rec = align_up(N * (size_t)f.rec_len * sizeof(double), 256), b_i = align_up(N * sizeof(int32_t), 256);
	const size_t b_pos = listed ? align_up((size_t)s->n_slots * sizeof(int32_t), 256) : 0;
	const size_t b_mom = listed ? align_up(N * rec * sizeof(double), 256) : 0, b_cnt = listed ? align_up(N * sizeof(int64_t), 256) : 0;
	if (!ensure_buffer(&ctx->stage, &ctx->stage_bytes, b_rec + 3 * b_i + 256 + (listed ? b_i : 0) + b_pos + b_mom + b_cnt, "staging", e)) return false;
	char *c = (char *)ctx->stage;
	o->rec = (double *)c; c += b_rec;
	o->it = (int32_t *)c; c += b_i;
	o->flag_pos = (int32_t *)c; c += b_i;
	o->flag_slot = (int32_t *)c; c += b_i;
	o->count = (int32_t *)c; c += 256;
	if (listed) {
		o->sel = (uint32_t *)c; c += b_i;
		o->pos = (int32_t *)c; c += b_pos;
		o->mom = (double *)c; c += b_mom;
		o->cnt = (int64_t *)c;
	}
	return true;
}

// The family's narrow stage on n moment records and the compaction of its flags.  d_sel: the listed slots the records were
// gathered from (nullptr: record g is slot g).  Afterwards flag_pos / flag_slot / count (device) describe the flagged records.
bool solve_records(AnofoxHipAggState *s, int64_t n, double *d_mom, const int64_t *d_counts, const uint32_t *d_sel, const Family &f, double *d_rec,
                   int32_t *d_it, const Staging &sg, AnofoxError *e) {
	AnofoxHipContext *ctx = s->ctx;
	hipStream_t st = ctx->stream;
	// workspace: one flag per record | the counters the stages' argument block points at
	const size_t b_flag = align_up((size_t)n * sizeof(int32_t), 256);
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, b_flag + 256, "workspace", e)) return false;
	char *base = (char *)ctx->ws;
	BatchArgs a;
	memset(&a, 0, sizeof a); // (row_offsets == nullptr: records without rows)
	a.n_groups = n;
	a.p = (int)s->p;
	a.model = ANOFOX_HIP_MODEL_OLS;
	a.fit_intercept = f.fit_intercept ? 1 : 0;
	a.hc_type = ANOFOX_HC_NONE;
	a.confidence_level = 0.95;
	a.moments = d_mom;
	a.core = d_rec;
	a.refine_list = (int32_t *)base;
	a.refine_count = (int32_t *)(base + b_flag);
	a.rule_counts = d_counts; // the aggregate's "< 2 accumulated rows -> NULL"
	ctx->last_refine_count = a.refine_count;
	if (hip_fail(hipMemsetAsync(a.refine_count, 0, 256, st), "hipMemsetAsync", e)) return false;
	*f.iterations_field = d_it;
	if (!f.stages.narrow(ctx, a, st, f.stages.user, e)) return false;
	return !hip_fail(launch_state_compact_flags(a.refine_list, n, d_sel, sg.flag_pos, d_sel ? sg.flag_slot : nullptr, sg.count, st),
	                 "flag compaction kernel launch", e);
}

bool has_log(const AnofoxHipAggState *s) { return s->retain && !s->log_dropped && s->log_rows > 0; }

// After solve_records, with the number of flagged records on the host (the stream is synchronised): their refit from the row
// log, or their NaN records.  *unrefined = the records flagged and not refitted.
bool answer_flagged(AnofoxHipAggState *s, int64_t n, int32_t flagged, const Family &f, double *d_rec, int32_t *d_it, const Staging &sg, bool listed,
                    int64_t *unrefined, AnofoxError *e) {
	*unrefined = 0;
	if (flagged <= 0) return true;
	if (flagged > n) flagged = (int32_t)n;
	if (has_log(s)) {
		// (the refit's own batch call reuses the workspace the flags were in: they are compacted into the staging already)
		ModelRefit m{f.stages, f.rec_len, f.iterations_field, d_it, n, launch_state_scatter_records};
		return listed ? agg_state_refit_from_log(s, s->n_slots, flagged, sg.flag_slot, d_rec, sg.pos, m, e)
		              : agg_state_refit_from_log(s, n, flagged, sg.flag_pos, d_rec, nullptr, m, e);
	}
	*unrefined = flagged;
	return !hip_fail(launch_state_flag_unrefined(sg.flag_pos, sg.count, n, f.rec_len, (int)s->p + 5, d_rec, s->ctx->stream), "flag kernel launch", e);
}

bool read_flagged(AnofoxHipAggState *s, const Staging &sg, int32_t *flagged, AnofoxError *e) {
	hipStream_t st = s->ctx->stream;
	if (hip_fail(hipMemcpyAsync(flagged, sg.count, sizeof *flagged, hipMemcpyDeviceToHost, st), "D2H", e)) return false;
	return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
}

bool check_args(AnofoxHipAggState *s, int64_t n, const void *rec, AnofoxError *e) {
	if (!s) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "state is NULL"); return false; }
	if (n < 0 || n > s->n_slots) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "n_slots exceeds the slots in use"); return false; }
	if (n > 0 && !rec) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "the record buffer is NULL"); return false; }
	return true;
}

// ---- the three forms, for either family ----

bool finalize_device(AnofoxHipAggState *s, int64_t n, const Family &f, double *d_rec, int32_t *d_it, AnofoxError *e) {
	if (!check_args(s, n, d_rec, e)) return false;
	std::lock_guard<std::mutex> lk0(s->mu);
	if (!agg_state_attached(s, e)) return false;
	if (!check_state(s, f, e)) return false;
	if (n == 0) return true;
	std::lock_guard<std::mutex> lk(s->ctx->mu);
	if (hip_fail(hipSetDevice(s->ctx->device), "hipSetDevice", e)) return false;
	if (s->log_only) {
		ModelRefit m{f.stages, f.rec_len, f.iterations_field, d_it, n, launch_state_scatter_records};
		return agg_state_refit_from_log(s, n, n, nullptr, d_rec, nullptr, m, e);
	}
	if (!agg_state_reserve_slots(s, s->n_slots, e)) return false; // slots handed out but never updated
	Staging sg;
	if (!carve_staging(s, n, f, false, &sg, e)) return false;
	if (!solve_records(s, n, s->moments, s->n_accum, nullptr, f, d_rec, d_it, sg, e)) return false;
	if (!has_log(s)) // nothing to refit and no reason to synchronise: the flagged records are marked from the device-side count
		return !hip_fail(launch_state_flag_unrefined(sg.flag_pos, sg.count, n, f.rec_len, (int)s->p + 5, d_rec, s->ctx->stream), "flag kernel launch", e);
	int32_t flagged = 0;
	int64_t unrefined = 0;
	if (!read_flagged(s, sg, &flagged, e)) return false;
	if (!answer_flagged(s, n, flagged, f, d_rec, d_it, sg, false, &unrefined, e)) return false;
	return agg_state_check_slot_flag(s, e);
}

bool finalize_host(AnofoxHipAggState *s, int64_t n, const Family &f, double *rec, int32_t *iterations, int64_t *out_unrefined,
                   int32_t *out_unrefined_slots, AnofoxError *e) {
	if (out_unrefined) *out_unrefined = 0;
	if (!check_args(s, n, rec, e)) return false;
	std::lock_guard<std::mutex> lk0(s->mu);
	if (!agg_state_attached(s, e)) return false;
	if (!check_state(s, f, e)) return false;
	if (n == 0) return true;
	std::lock_guard<std::mutex> lk(s->ctx->mu);
	AnofoxHipContext *ctx = s->ctx;
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	if (!s->log_only && !agg_state_reserve_slots(s, s->n_slots, e)) return false;
	Staging sg;
	if (!carve_staging(s, n, f, false, &sg, e)) return false;
	hipStream_t st = ctx->stream;
	int64_t unrefined = 0;
	if (s->log_only) {
		ModelRefit m{f.stages, f.rec_len, f.iterations_field, iterations ? sg.it : nullptr, n, launch_state_scatter_records};
		if (!agg_state_refit_from_log(s, n, n, nullptr, sg.rec, nullptr, m, e)) return false;
	} else {
		int32_t flagged = 0;
		if (!solve_records(s, n, s->moments, s->n_accum, nullptr, f, sg.rec, iterations ? sg.it : nullptr, sg, e)) return false;
		if (!read_flagged(s, sg, &flagged, e)) return false;
		if (!answer_flagged(s, n, flagged, f, sg.rec, iterations ? sg.it : nullptr, sg, false, &unrefined, e)) return false;
	}
	if (hip_fail(hipMemcpyAsync(rec, sg.rec, (size_t)n * (size_t)f.rec_len * sizeof(double), hipMemcpyDeviceToHost, st), "D2H records", e)) return false;
	if (iterations && hip_fail(hipMemcpyAsync(iterations, sg.it, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st), "D2H iterations", e)) return false;
	if (out_unrefined_slots && unrefined > 0 &&
	    hip_fail(hipMemcpyAsync(out_unrefined_slots, sg.flag_pos, (size_t)unrefined * sizeof(int32_t), hipMemcpyDeviceToHost, st), "D2H", e))
		return false;
	if (!agg_state_check_slot_flag(s, e)) return false; // (synchronises the stream)
	if (out_unrefined) *out_unrefined = unrefined;
	return true;
}

bool finalize_slots_host(AnofoxHipAggState *s, int64_t n_list, const uint32_t *slots, const Family &f, double *rec, int32_t *iterations,
                         int64_t *out_unrefined, AnofoxError *e) {
	if (out_unrefined) *out_unrefined = 0;
	if (!s || n_list < 0) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "state is NULL or n_list negative"); return false; }
	if (n_list > 0 && (!slots || !rec)) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "slots or the record buffer is NULL"); return false; }
	std::lock_guard<std::mutex> lk0(s->mu);
	if (!agg_state_attached(s, e)) return false;
	if (!check_state(s, f, e)) return false;
	if (n_list == 0) return true;
	for (int64_t k = 0; k < n_list; ++k)
		if ((int64_t)slots[k] >= s->n_slots) { set_error(e, ANOFOX_ERROR_INVALID_INPUT, "finalize: slot index out of range"); return false; }
	{
		// record k belongs to slots[k]: a slot listed twice would leave one of its two rows unwritten
		std::vector<uint32_t> sorted(slots, slots + n_list);
		std::sort(sorted.begin(), sorted.end());
		if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) {
			set_error(e, ANOFOX_ERROR_INVALID_INPUT, "finalize: a slot is listed twice");
			return false;
		}
	}
	std::lock_guard<std::mutex> lk(s->ctx->mu);
	AnofoxHipContext *ctx = s->ctx;
	if (hip_fail(hipSetDevice(ctx->device), "hipSetDevice", e)) return false;
	if (!s->log_only && !agg_state_reserve_slots(s, s->n_slots, e)) return false;
	Staging sg;
	if (!carve_staging(s, n_list, f, true, &sg, e)) return false;
	hipStream_t st = ctx->stream;
	bool bad = hip_fail(hipMemcpyAsync(sg.sel, slots, (size_t)n_list * sizeof(uint32_t), hipMemcpyHostToDevice, st), "H2D", e);
	bad = bad || hip_fail(launch_rowlog_positions(sg.sel, n_list, sg.pos, s->n_slots, st), "positions kernel launch", e);
	if (bad) return false;
	int64_t unrefined = 0;
	int32_t *d_it = iterations ? sg.it : nullptr;
	if (s->log_only) {
		ModelRefit m{f.stages, f.rec_len, f.iterations_field, d_it, n_list, launch_state_scatter_records};
		if (!agg_state_refit_from_log(s, s->n_slots, n_list, (const int32_t *)sg.sel, sg.rec, sg.pos, m, e)) return false;
	} else {
		if (hip_fail(launch_ingest_gather_slots(s->moments, s->n_accum, sg.sel, n_list, (int)s->p, sg.mom, sg.cnt, st), "gather kernel launch", e))
			return false;
		int32_t flagged = 0;
		if (!solve_records(s, n_list, sg.mom, sg.cnt, sg.sel, f, sg.rec, d_it, sg, e)) return false;
		if (!read_flagged(s, sg, &flagged, e)) return false;
		if (!answer_flagged(s, n_list, flagged, f, sg.rec, d_it, sg, true, &unrefined, e)) return false;
	}
	if (hip_fail(hipMemcpyAsync(rec, sg.rec, (size_t)n_list * (size_t)f.rec_len * sizeof(double), hipMemcpyDeviceToHost, st), "D2H records", e)) return false;
	if (iterations && hip_fail(hipMemcpyAsync(iterations, sg.it, (size_t)n_list * sizeof(int32_t), hipMemcpyDeviceToHost, st), "D2H iterations", e)) return false;
	if (!agg_state_check_slot_flag(s, e)) return false; // (synchronises the stream; the slot list is pageable host memory)
	if (out_unrefined) *out_unrefined = unrefined;
	return true;
}

// the parameter blocks live in the entry point's frame: the stages capture them by value at every launch
struct EnCall {
	EnParams en;
	Family f;
	bool init(AnofoxHipAggState *s, const AnofoxHipElasticNetBatchOptions &o, AnofoxError *e) {
		reset_error(e);
		if (!elasticnet_state_options(o, e)) return false;
		en = elasticnet_state_params(o);
		f = Family{"elastic net", elasticnet_state_stages(&en), &en.iterations, s ? (int)s->p + 6 : 0, o.fit_intercept};
		return true;
	}
};

struct BlsCall {
	BlsParamsT<kWideMaxP> bp;
	Family f;
	bool init(AnofoxHipAggState *s, const AnofoxHipBlsBatchOptions &o, AnofoxError *e) {
		reset_error(e);
		if (!bls_state_options(o, e)) return false;
		bp = bls_state_params(o, s ? s->p : 1);
		f = Family{"bounded least squares", bls_state_stages(&bp), &bp.iterations, s ? 3 * (int)s->p + 6 : 0, o.fit_intercept};
		return true;
	}
};

} // namespace

extern "C" {

bool anofox_hip_agg_state_finalize_elasticnet_host(AnofoxHipAggState *s, int64_t n_slots, AnofoxHipElasticNetBatchOptions options, double *core,
                                                   int32_t *iterations, int64_t *out_unrefined, int32_t *out_unrefined_slots, AnofoxError *out_error) {
	EnCall c;
	if (out_unrefined) *out_unrefined = 0;
	return c.init(s, options, out_error) && finalize_host(s, n_slots, c.f, core, iterations, out_unrefined, out_unrefined_slots, out_error);
}

bool anofox_hip_agg_state_finalize_elasticnet_device(AnofoxHipAggState *s, int64_t n_slots, AnofoxHipElasticNetBatchOptions options, double *d_core,
                                                     int32_t *d_iterations, AnofoxError *out_error) {
	EnCall c;
	return c.init(s, options, out_error) && finalize_device(s, n_slots, c.f, d_core, d_iterations, out_error);
}

bool anofox_hip_agg_state_finalize_elasticnet_slots_host(AnofoxHipAggState *s, int64_t n_list, const uint32_t *slots,
                                                         AnofoxHipElasticNetBatchOptions options, double *core, int32_t *iterations,
                                                         int64_t *out_unrefined, AnofoxError *out_error) {
	EnCall c;
	if (out_unrefined) *out_unrefined = 0;
	return c.init(s, options, out_error) && finalize_slots_host(s, n_list, slots, c.f, core, iterations, out_unrefined, out_error);
}

bool anofox_hip_agg_state_finalize_bls_host(AnofoxHipAggState *s, int64_t n_slots, AnofoxHipBlsBatchOptions options, double *bls, int32_t *iterations,
                                            int64_t *out_unrefined, int32_t *out_unrefined_slots, AnofoxError *out_error) {
	BlsCall c;
	if (out_unrefined) *out_unrefined = 0;
	return c.init(s, options, out_error) && finalize_host(s, n_slots, c.f, bls, iterations, out_unrefined, out_unrefined_slots, out_error);
}

bool anofox_hip_agg_state_finalize_bls_device(AnofoxHipAggState *s, int64_t n_slots, AnofoxHipBlsBatchOptions options, double *d_bls,
                                              int32_t *d_iterations, AnofoxError *out_error) {
	BlsCall c;
	return c.init(s, options, out_error) && finalize_device(s, n_slots, c.f, d_bls, d_iterations, out_error);
}

bool anofox_hip_agg_state_finalize_bls_slots_host(AnofoxHipAggState *s, int64_t n_list, const uint32_t *slots, AnofoxHipBlsBatchOptions options,
                                                  double *bls, int32_t *iterations, int64_t *out_unrefined, AnofoxError *out_error) {
	BlsCall c;
	if (out_unrefined) *out_unrefined = 0;
	return c.init(s, options, out_error) && finalize_slots_host(s, n_list, slots, c.f, bls, iterations, out_unrefined, out_error);
}

} // extern "C"
