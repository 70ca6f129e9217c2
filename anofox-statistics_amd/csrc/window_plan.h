// window_plan.h — what the window functions that WALK their frames share on the host (quantile.hip, glm_window.hip): the
// frames of a ROWS spec, the argument checks of frames and partitions, and the cut of the partitions into the runs of
// consecutive output rows that one wavefront walks.  How much scratch a run needs is the family's own rule.
#pragma once
#include <vector>

#include "context.h"

namespace anofox {
namespace host {

// Walkers: every partition is cut into runs of consecutive output rows, min(ceil(n_g / L), n_g / kWalkMinRun) of them (at
// least one) of equal length (the last one shorter), L = ceil(n_rows / kWalkTargetWalkers): with many partitions a run is a
// whole partition, with few long ones there are about kWalkTargetWalkers walkers, and no run is shorter than kWalkMinRun rows
// unless its partition is (every run begins with a cold fit, which the rows after it have to pay for).  A partition all of
// whose frames start at the same row (UNBOUNDED PRECEDING) is one run: every run of it would span the partition anyway.
// run_length > 0 (a test's hook): runs of exactly that many rows, neither rule applied.
constexpr int64_t kWalkMinRun = 64;
constexpr int64_t kWalkTargetWalkers = 8192;
constexpr int64_t kWalkMaxWaves = 8192;
constexpr int64_t kWalkScratchCap = 1ll << 30;

// -> run_begin: the first output row of every run, then off[n_parts] (runs + 1 entries; a run ends where the next begins
// or at its partition's end: the runs are contiguous over the partitions' rows, and an empty partition owns none)
inline void cut_window_runs(int64_t n_parts, const int64_t *off, const int64_t *lo, const int64_t *hi, int64_t run_length,
                            std::vector<int64_t> &run_begin) {
	run_begin.clear();
	const int64_t N = n_parts > 0 ? off[n_parts] - off[0] : 0;
	int64_t L = run_length;
	if (L <= 0) {
		L = (N + kWalkTargetWalkers - 1) / kWalkTargetWalkers;
		if (L < 1) L = 1;
	}
	for (int64_t g = 0; g < n_parts; ++g) {
		const int64_t b = off[g], n = off[g + 1] - b;
		if (n <= 0) continue;
		int64_t pieces = (n + L - 1) / L;
		if (run_length <= 0 && pieces > n / kWalkMinRun) pieces = n / kWalkMinRun > 0 ? n / kWalkMinRun : 1; // no run below kWalkMinRun rows
		if (run_length <= 0 && pieces > 1) { // frames that all start at one row: one walker
			int64_t first = -1;
			bool same = true;
			for (int64_t r = b; r < b + n && same; ++r) {
				if (hi[r] <= lo[r]) continue;
				if (first < 0) first = lo[r];
				same = lo[r] == first;
			}
			if (same) pieces = 1;
		}
		const int64_t len = (n + pieces - 1) / pieces;
		for (int64_t r = b; r < b + n; r += len) run_begin.push_back(r);
	}
	run_begin.push_back(n_parts > 0 ? off[n_parts] : 0);
}

// the frames of ROWS BETWEEN start PRECEDING AND end PRECEDING, clipped to the partition: frames_spec_kernel's arithmetic
inline void rows_frames(int64_t G, const int64_t *off, const AnofoxHipWindowFrame &f, int64_t *lo, int64_t *hi) {
	for (int64_t g = 0; g < G; ++g) {
		const int64_t plo = off[g], phi = off[g + 1];
		for (int64_t r = plo; r < phi; ++r) {
			int64_t first = f.start_preceding == ANOFOX_HIP_FRAME_UNBOUNDED ? plo : r - f.start_preceding;
			int64_t last = f.end_preceding == -ANOFOX_HIP_FRAME_UNBOUNDED ? phi - 1 : r - f.end_preceding;
			if (first < plo) first = plo;
			if (last > phi - 1) last = phi - 1;
			const bool empty = last < first;
			lo[r] = empty ? r : first;
			hi[r] = empty ? r : last + 1;
		}
	}
}

inline bool check_window_frame(const AnofoxHipWindowFrame &f, AnofoxError *e) {
	if (f.start_preceding < f.end_preceding || f.start_preceding == -ANOFOX_HIP_FRAME_UNBOUNDED || f.end_preceding == ANOFOX_HIP_FRAME_UNBOUNDED) {
		set_error(e, ANOFOX_ERROR_INVALID_INPUT, "window frame must start at or before its end");
		return false;
	}
	return true;
}

inline bool check_window_offsets(int64_t G, int64_t n_rows, const int64_t *off, AnofoxError *e) {
	// (the whole range: every output row belongs to a partition's walker)
	return check_host_offsets(G, n_rows, off, e) && check_whole_range(G, n_rows, off, e);
}

inline bool check_host_frames(int64_t n_rows, const int64_t *lo, const int64_t *hi, AnofoxError *e) {
	for (int64_t r = 0; r < n_rows; ++r) {
		if (hi[r] > lo[r] && (lo[r] < 0 || hi[r] > n_rows)) {
			set_error(e, ANOFOX_ERROR_INVALID_INPUT, "frame bounds must lie within [0, n_rows]");
			return false;
		}
	}
	return true;
}

} // namespace host
} // namespace anofox
