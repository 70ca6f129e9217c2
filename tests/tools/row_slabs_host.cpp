// The slab cut of the host fit entries (csrc/row_slabs.h) as a program of its own: tests/test_row_slabs_cpu.py compiles it under
// ASan / UBSan and compares what it prints with a restatement of the loop.
// stdin: "slab_rows n_groups" and the n_groups + 1 offsets of a case, any number of cases.
// stdout: per slab "g0 g1 rebased offsets..." on one line; a line "end" after each case.
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
		printf("end\n");
	}
	return 0;
}
