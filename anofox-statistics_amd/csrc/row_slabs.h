// row_slabs.h — how a host batch of groups is cut into slabs that pass through the GPU one after another.  Plain C++17, no
// HIP: the cut is a pure function of the offsets and is tested on its own (tests/tools/row_slabs_host.cpp).
#pragma once
#include <stdint.h>

#include <vector>

namespace anofox {
namespace host {

constexpr int64_t kHostSlabRows = 32ll << 20; // the host fit entries stage at most ~32M rows at a time

// The slab that begins at group g0 < n_groups: the longest run of groups [g0, g1) whose rows span at most slab_rows, never
// empty (a single group larger than slab_rows is a slab of its own).  Returns g1; `rebased` receives the g1 - g0 + 1 offsets
// of the slab's groups counted from its first row, row_offsets[g0 + g] - row_offsets[g0].
inline int64_t next_row_slab(const int64_t *row_offsets, int64_t n_groups, int64_t g0, int64_t slab_rows, std::vector<int64_t> &rebased) {
	int64_t g1 = g0 + 1;
	while (g1 < n_groups && row_offsets[g1 + 1] - row_offsets[g0] <= slab_rows) ++g1;
	rebased.resize((size_t)(g1 - g0) + 1);
	for (int64_t g = g0; g <= g1; ++g) rebased[(size_t)(g - g0)] = row_offsets[g] - row_offsets[g0];
	return g1;
}

// The slabs of a batch in order: fn(g0, G, r0, R, rebased) for the G groups from g0, whose R rows begin at row r0 of the
// caller's arrays; `rebased` points at the slab's G + 1 offsets.  Stops at the first `false` and returns it.
template <class Fn>
bool for_each_row_slab(const int64_t *row_offsets, int64_t n_groups, int64_t slab_rows, Fn &&fn) {
	std::vector<int64_t> off;
	for (int64_t g0 = 0, g1; g0 < n_groups; g0 = g1) {
		g1 = next_row_slab(row_offsets, n_groups, g0, slab_rows, off);
		if (!fn(g0, g1 - g0, row_offsets[g0], off[(size_t)(g1 - g0)], (const int64_t *)off.data())) return false;
	}
	return true;
}

} // namespace host
} // namespace anofox
