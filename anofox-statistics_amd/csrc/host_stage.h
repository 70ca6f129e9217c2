// host_stage.h — the staging of one host-pointer call in the context's device buffer (ctx->stage), shared by every *_host
// entry point.  A call describes its device layout once, as a function of a Stage; stage_call() runs that description twice:
// first with no buffer, which only adds up the size, then, after ensure_buffer() with that size, on the buffer, which places
// the arrays and enqueues the copies to the device.  The size and the placement cannot disagree: they are the same code.
#pragma once
#include "context.h"

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

} // namespace host
} // namespace anofox
