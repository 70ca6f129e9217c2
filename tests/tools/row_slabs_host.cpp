// The slab cut of the host fit entries (csrc/row_slabs.h) as a program of its own: tests/test_row_slabs_cpu.py compiles it under
// ASan / UBSan and compares what it prints with a restatement of the loop.
// stdin: "slab_rows n_groups" and the n_groups + 1 offsets of a case, any number of cases.
// stdout: per slab "g0 g1 rebased offsets..." on one line; then the walk of for_each_row_slab, per slab
// "each g0 G r0 R rebased offsets...", and the same walk told to stop after its second slab, per slab "stop g0"; a line "end"
// after each case.
#include <stdio.h>

#include "../../anofox-statistics_amd/csrc/row_slabs.h"

int main() {
	long long slab_rows, n_groups;
	while (scanf("%lld %lld", &slab_rows, &n_groups) == 2) {
		std::vector<int64_t> offsets((size_t)n_groups + 1), rebased;
		for (auto &o : offsets) {
			long long v;
			if (scanf("%lld", &v) != 1) return 1;
			o = v;
		}
		for (int64_t g0 = 0, g1; g0 < n_groups; g0 = g1) {
			g1 = anofox::host::next_row_slab(offsets.data(), n_groups, g0, slab_rows, rebased);
			printf("%lld %lld", (long long)g0, (long long)g1);
			for (int64_t o : rebased) printf(" %lld", (long long)o);
			printf("\n");
		}
		using anofox::host::for_each_row_slab;
		const bool all = for_each_row_slab(offsets.data(), n_groups, slab_rows, [](int64_t g0, int64_t G, int64_t r0, int64_t R, const int64_t *off) {
			printf("each %lld %lld %lld %lld", (long long)g0, (long long)G, (long long)r0, (long long)R);
			for (int64_t g = 0; g <= G; ++g) printf(" %lld", (long long)off[g]);
			printf("\n");
			return true;
		});
		int seen = 0;
		const bool stopped = !for_each_row_slab(offsets.data(), n_groups, slab_rows, [&](int64_t g0, int64_t, int64_t, int64_t, const int64_t *) {
			printf("stop %lld\n", (long long)g0);
			return ++seen < 2;
		});
		if (!all || stopped != (seen == 2)) return 2;
		printf("end\n");
	}
	return 0;
}
