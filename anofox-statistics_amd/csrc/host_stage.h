// host_stage.h — the staging of one host-pointer call in the context's device buffer (ctx->stage), shared by every *_host
// entry point.  A call describes its device layout once, as a function of a Stage; stage_call() runs that description twice:
// first with no buffer, which only adds up the size, then, after ensure_buffer() with that size, on the buffer, which places
// the arrays and enqueues the copies to the device.  The size and the placement cannot disagree: they are the same code.
#pragma once
#include "context.h"
#include "row_slabs.h"

namespace anofox {
namespace host {

inline bool h2d(void *dst, const void *src, size_t bytes, hipStream_t st, AnofoxError *e, const char *what = "H2D") {
	return bytes == 0 || !hip_fail(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), what, e);
}

inline bool d2h(void *dst, const void *src, size_t bytes, hipStream_t st, AnofoxError *e, const char *what = "D2H") {
	return bytes == 0 || !hip_fail(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), what, e);
}

// the labels of the copies that Stage::columns enqueues, as they appear in a HIP error's text
struct ColumnLabels {
	const char *x, *y, *w, *offset;
};
constexpr ColumnLabels kNamedColumns = {"H2D x", "H2D y", "H2D w", "H2D offset"};
constexpr ColumnLabels kPlainColumns = {"H2D", "H2D", "H2D", "H2D"};

// the device addresses of the staged rows of one call (a NULL host pointer stays a NULL device pointer)
struct StagedColumns {
	const double *x[kWideMaxP + 1]; // (the VIF entry takes one column more than a fit)
	const double *y, *w, *offset;
};

struct Stage {
	char *base; // nullptr: the sizing pass
	hipStream_t st;
	AnofoxError *e;
	size_t used = 0;
	bool ok = true; // false after the first failed copy; what follows it in the layout is placed but not copied

	// n elements, 256-byte aligned, with 16 readable bytes after the last one
	template <class T>
	T *take(size_t n) {
		T *p = base ? (T *)(base + used) : nullptr;
		used += bytes(n, sizeof(T));
		return p;
	}
	static size_t bytes(size_t n, size_t elem) { return align_up(n * elem + 16, 256); }
	// take(n) filled from host memory; src == nullptr: nothing is taken and the device pointer is NULL too
	template <class T>
	T *put(const T *src, size_t n, const char *what = "H2D") {
		if (!src) return nullptr;
		T *p = take<T>(n);
		if (base && ok) ok = h2d(p, src, n * sizeof(T), st, e, what);
		return p;
	}
	// One column of rows [r0, r0 + R).  Every staged column keeps two doubles of readable slack after its last row, on top of
	// take()'s 16 bytes: the narrow predict kernel loads rows in pairs.
	const double *column(const double *src, int64_t r0, int64_t R, const char *what = "H2D") {
		if (!src) return nullptr;
		double *p = take<double>((size_t)R + 2);
		if (base && ok) ok = h2d(p, src + r0, (size_t)R * sizeof(double), st, e, what);
		return p;
	}
	// the p columns, y and the optional w / offset of rows [r0, r0 + R)
	StagedColumns columns(size_t p, int64_t r0, int64_t R, const double *const *x_cols, const double *y, const double *w = nullptr,
	                      const double *offset = nullptr, const ColumnLabels &l = kNamedColumns) {
		StagedColumns c;
		for (size_t j = 0; j < p; ++j) c.x[j] = column(x_cols[j], r0, R, l.x);
		c.y = column(y, r0, R, l.y);
		c.w = column(w, r0, R, l.w);
		c.offset = column(offset, r0, R, l.offset);
		return c;
	}
};

// Sizes ctx->stage by `layout`, then places it and enqueues its copies on the context's stream (ctx->mu held by the caller).
template <class Layout>
bool stage_call(AnofoxHipContext *ctx, AnofoxError *e, Layout &&layout) {
	Stage size{nullptr, ctx->stream, e};
	layout(size);
	if (!ensure_buffer(&ctx->stage, &ctx->stage_bytes, size.used, "staging", e)) return false;
	Stage s{(char *)ctx->stage, ctx->stream, e};
	layout(s);
	return s.ok;
}

// ---- the host form of a batch fit: slab by slab (row_slabs.h) through the staging buffer ----

// what a host fit returns per group: the records, and optionally int32 iteration counts and a second block of doubles (the
// inference of the regression models); a NULL pointer is an output the call does not ask for
struct SlabOutputs {
	double *rec;
	size_t rec_len;
	int32_t *iterations = nullptr;
	size_t it_len = 0;
	double *extra = nullptr;
	size_t extra_len = 0;
};

// the labels of a slab's copies, as they appear in a HIP error's text
struct SlabLabels {
	ColumnLabels columns;
	const char *offsets, *rec, *iterations, *extra;
};
constexpr SlabLabels kPlainSlab = {kPlainColumns, "H2D", "D2H", "D2H", "D2H"};

// Stages each slab's rebased offsets, columns and output blocks, calls run(G, R, off, d_off, columns, d_rec, d_iterations,
// d_extra) — `off` the slab's offsets on the host, the rest device addresses — which enqueues the family's fit of the slab's
// G groups and R rows on the context's stream, copies the outputs back to their place in the caller's arrays and synchronises.
// ctx->mu is held by the caller.
template <class Run>
bool fit_slabs_host(AnofoxHipContext *ctx, int64_t n_groups, size_t p, const int64_t *row_offsets, const double *y,
                    const double *const *x_cols, const double *w, const SlabOutputs &out, const SlabLabels &l, AnofoxError *e, Run &&run) {
	hipStream_t st = ctx->stream;
	return for_each_row_slab(row_offsets, n_groups, kHostSlabRows, [&](int64_t g0, int64_t G, int64_t r0, int64_t R, const int64_t *off) {
		const size_t n = (size_t)G, at = (size_t)g0;
		int64_t *d_off;
		StagedColumns c;
		double *d_rec, *d_extra;
		int32_t *d_it;
		if (!stage_call(ctx, e, [&](Stage &s) {
			    d_off = s.put(off, n + 1, l.offsets);
			    c = s.columns(p, r0, R, x_cols, y, w, nullptr, l.columns);
			    d_rec = s.take<double>(n * out.rec_len);
			    d_it = out.iterations ? s.take<int32_t>(n * out.it_len) : nullptr;
			    d_extra = out.extra ? s.take<double>(n * out.extra_len) : nullptr;
		    }))
			return false;
		if (!run(G, R, off, (const int64_t *)d_off, (const StagedColumns &)c, d_rec, d_it, d_extra)) return false;
		if (!d2h(out.rec + at * out.rec_len, d_rec, n * out.rec_len * sizeof(double), st, e, l.rec)) return false;
		if (d_it && !d2h(out.iterations + at * out.it_len, d_it, n * out.it_len * sizeof(int32_t), st, e, l.iterations)) return false;
		if (d_extra && !d2h(out.extra + at * out.extra_len, d_extra, n * out.extra_len * sizeof(double), st, e, l.extra)) return false;
		return !hip_fail(hipStreamSynchronize(st), "hipStreamSynchronize", e);
	});
}

} // namespace host
} // namespace anofox
