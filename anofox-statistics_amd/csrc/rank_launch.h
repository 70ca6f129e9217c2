// rank_launch.h — the size-tiered launch driver of a rank family (rank_cor.hip, rank_tests.hip): the caps, the view of a call,
// the two kernel frames and the host-side ladder that launches them.  HIP only; the per-group mathematics (rank_cor.h,
// rank_tests.h) also compiles as plain C++ and does not include this.  DESIGN.md §1, "Rank and product-moment correlation".
//
//   rank_small_kernel<CAP, Family>: one wavefront per workgroup and group, grid-stride over the groups, the group's work arrays in
//     LDS.  Two instances share the groups by their row count: up to kRankTierRows rows (7 KiB of LDS, so a CU holds as many
//     wavefronts as its other limits admit) and up to kRankSmallCap.  A kernel passes over the groups of the other tier.
//   rank_large_kernel<Family>: a workgroup of 1024 threads per group above the cap, its work arrays in the context's workspace.
//     All sixteen wavefronts sort; the first runs the other phases with the small path's code, so a group's midranks and their
//     sums come out bit for bit as on the small path.
//   Neither form of an entry reads the offsets on the host to size a launch; the large path is launched whenever the call has
//     more rows than the cap, and then takes kCorRowBytes of workspace per row of the call.
//
// A family is a small trivially-copyable struct that holds its problem and is passed by value to the kernels:
//   static const char *const kSmallKernel, kLargeKernel, kScratch   the texts of a HIP error and of a failed allocation
//   bool staged() const                       false: the groups' rows are not staged in the work arrays, so every group runs on
//                                             the first small instance whatever its size and nothing else is launched
//   __device__ void small_group(g, lo, hi, W) rows [lo, hi) of group g by the one wavefront of the workgroup, W in LDS
//   __device__ void large_group(g, lo, hi, W) the same by a workgroup of kRankLargeThreads threads, W in the workspace
//   size_t prefix_bytes(slots) const          what the family keeps in the workspace ahead of the work arrays for a call that
//                                             has at most `slots` groups on the large path
//   bool begin_large(prefix, slots, st, e)    enqueued before the large kernel (the family may keep addresses inside `prefix`)
//   bool end_large(call, st, e) const         enqueued after it
#pragma once
#include "common.h"
#include "context.h"
#include "rank_cor.h"

namespace anofox {
namespace rank {

// The rows of a group that the small path holds.  A workgroup of rank_small_kernel is one wavefront, and a CU has four SIMDs: with
// 160 KiB of LDS per CU (a single workgroup may take all of it), 160 / 4 = 40 KiB per workgroup keeps one wavefront on every
// SIMD.  40960 bytes / kCorRowBytes (28) = 1462 rows.  A larger cap would idle SIMDs; a smaller one sends groups to the large
// path, which costs further launches and global-memory sorts.
constexpr int kRankSmallCap = 40960 / cor::kCorRowBytes;
static_assert(kRankSmallCap == 1462, "the cap's derivation");
constexpr int kRankTierRows = 256; // the first instance's groups: 256 x 28 = 7 KiB
constexpr int64_t kRankMaxWorkgroups = 1 << 16;
constexpr int kRankLargeThreads = 1024;
constexpr int kRankLargeWorkgroups = 1024;

// what every kernel of either family needs of a call
struct RankCall {
	const int64_t *off;
	int64_t n_groups;
	int64_t above, upto; // the kernel's groups: above < rows <= upto
	cor::CorWork W;      // the large path: each n_rows long; a group's part starts at its first row
	int64_t n_rows;      // row ranges are clipped to [0, n_rows]
};

__device__ __forceinline__ void group_rows(const RankCall &c, int64_t g, int64_t &lo, int64_t &hi) {
	lo = c.off[g] < 0 ? 0 : c.off[g];
	hi = c.off[g + 1] > c.n_rows ? c.n_rows : c.off[g + 1];
	if (hi < lo) hi = lo;
	if (lo > c.n_rows) lo = hi = c.n_rows;
}

template <int CAP, class Family>
__global__ __launch_bounds__(64) void rank_small_kernel(Family f, RankCall c) {
	__shared__ double sx[CAP], sy[CAP], sk[CAP];
	__shared__ int32_t si[CAP];
	const cor::CorWork W = {sx, sy, sk, si};
	const int64_t upto = f.staged() && c.upto > CAP ? CAP : c.upto; // (CAP never: upto <= CAP for a staged family)
	for (int64_t g = blockIdx.x; g < c.n_groups; g += gridDim.x) {
		int64_t lo, hi;
		group_rows(c, g, lo, hi);
		const int64_t m = hi - lo;
		if (m <= c.above || m > upto) continue;
		f.small_group(g, lo, hi, W);
		__syncthreads(); // the next group's rows overwrite these
	}
}

template <class Family>
__global__ __launch_bounds__(kRankLargeThreads) void rank_large_kernel(Family f, RankCall c) {
	for (int64_t g = blockIdx.x; g < c.n_groups; g += gridDim.x) {
		int64_t lo, hi;
		group_rows(c, g, lo, hi);
		if (hi - lo <= c.above) continue;
		const cor::CorWork W = {c.W.x + lo, c.W.y + lo, c.W.key + lo, c.W.idx + lo};
		f.large_group(g, lo, hi, W);
		__syncthreads();
	}
}

template <class K, class... Args>
bool launch(K kernel, const char *name, int64_t blocks, int threads, hipStream_t st, AnofoxError *e, const Args &...args) {
	hipLaunchKernelGGL(kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(threads), 0, st, args...);
	return !host::hip_fail(hipGetLastError(), name, e);
}

// The groups of the call `c` (off, n_groups, n_rows; n_groups > 0) by their tiers, enqueued on the context's stream (ctx->mu held by
// the caller).  `hook`: a family's test hook, a cap below kRankSmallCap, or 0.
template <class Family>
bool launch_tiers(AnofoxHipContext *ctx, RankCall c, int64_t hook, Family f, AnofoxError *e) {
	using namespace host;
	hipStream_t st = ctx->stream;
	const int64_t blocks = c.n_groups < kRankMaxWorkgroups ? c.n_groups : kRankMaxWorkgroups;
	const int64_t cap = hook > 0 && hook < kRankSmallCap ? hook : kRankSmallCap;
	const int64_t tier = cap < kRankTierRows ? cap : kRankTierRows;
	c.above = -1;
	c.upto = f.staged() ? tier : INT64_MAX;
	if (!launch(rank_small_kernel<kRankTierRows, Family>, Family::kSmallKernel, blocks, 64, st, e, f, c)) return false;
	if (!f.staged() || c.n_rows <= tier) return true; // no group has more rows than the call
	if (cap > tier) {
		c.above = tier;
		c.upto = cap;
		if (!launch(rank_small_kernel<kRankSmallCap, Family>, Family::kSmallKernel, blocks, 64, st, e, f, c)) return false;
	}
	if (c.n_rows <= cap) return true;
	// the large path: the family's prefix (disjoint groups above the cap: n_rows / (cap + 1) at most) and the work arrays, each as
	// long as the call
	const size_t N = (size_t)c.n_rows;
	const int64_t slots = c.n_rows / (cap + 1) + 1;
	const size_t x_at = align_up(f.prefix_bytes(slots), 256), col = align_up(N * sizeof(double), 256);
	if (!ensure_buffer(&ctx->ws, &ctx->ws_bytes, x_at + 3 * col + align_up(N * sizeof(int32_t), 256), Family::kScratch, e)) return false;
	char *ws = (char *)ctx->ws;
	c.W.x = (double *)(ws + x_at);
	c.W.y = (double *)(ws + x_at + col);
	c.W.key = (double *)(ws + x_at + 2 * col);
	c.W.idx = (int32_t *)(ws + x_at + 3 * col);
	c.above = cap;
	c.upto = INT64_MAX;
	if (!f.begin_large(ws, slots, st, e)) return false;
	const int64_t large_blocks = c.n_groups < kRankLargeWorkgroups ? c.n_groups : kRankLargeWorkgroups;
	return launch(rank_large_kernel<Family>, Family::kLargeKernel, large_blocks, kRankLargeThreads, st, e, f, c) && f.end_large(c, st, e);
}

} // namespace rank
} // namespace anofox
