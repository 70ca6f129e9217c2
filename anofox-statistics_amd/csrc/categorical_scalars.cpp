// categorical_scalars.cpp — categorical_tests.h in its plain C++ build inside the library: the records of the scalars that take a
// table or four cells (categorical_scalars.h).  Compiled as C++, not as HIP: no device code, no device call.
#include "categorical_scalars.h"

#include <vector>

#include "categorical_tests.h"

namespace anofox {
namespace cattest {

void ct_scalar_table(int test, int correction, const size_t *table, const size_t *row_lengths, size_t n_rows, double *rec) {
	size_t width = 0;
	for (size_t i = 0; i < n_rows; ++i) width = row_lengths[i] > width ? row_lengths[i] : width;
	std::vector<int64_t> cells(n_rows * width, 0), row_total(n_rows, 0), col_total(width, 0);
	CtTable T = {0, 0, 0, 0.0, 0, 0, 0, 0};
	size_t at = 0;
	for (size_t i = 0; i < n_rows; ++i) {
		for (size_t j = 0; j < row_lengths[i]; ++j) {
			const int64_t o = (int64_t)table[at++];
			cells[i * width + j] = o;
			row_total[i] += o;
			col_total[j] += o;
			T.n += o;
		}
	}
	for (size_t j = 0; j < width; ++j) T.c += col_total[j] > 0;
	size_t first_col = 0;
	while (first_col < width && col_total[first_col] == 0) ++first_col;
	for (size_t i = 0; i < n_rows; ++i) {
		if (row_total[i] == 0) continue;
		if (T.r++ == 0) { // the first occupied row and column: the 2 x 2 table's n11 and margins
			T.r1 = row_total[i];
			T.c1 = col_total[first_col];
			T.n11 = cells[i * width + first_col];
		}
		for (size_t j = 0; j < width; ++j) {
			const int64_t o = cells[i * width + j];
			if (o == 0) continue;
			T.sum += ct_cell_term(test, o, row_total[i], col_total[j], T.n);
			T.sum_rc += row_total[i] * col_total[j];
		}
	}
	ct_table_record(test, correction, T, rec);
}

void ct_scalar_cells(int test, int alternative, int correction, int exact, double confidence_level, size_t n11, size_t n12, size_t n21,
                     size_t n22, double *rec) {
	const int64_t a = (int64_t)n11, b = (int64_t)n12, c = (int64_t)n21, d = (int64_t)n22;
	if (test == kCtMcNemar) {
		ct_mcnemar_record(correction, exact, a, b, c, d, rec);
		return;
	}
	if (a + b + c + d < 1) {
		ct_write_failed(rec, 0.0, 2.0, 2.0);
		return;
	}
	ct_fisher_record(a, b, c, d, ct_fisher(ct_hyper(a, b, c, d), alternative, confidence_level), rec);
}

} // namespace cattest
} // namespace anofox
