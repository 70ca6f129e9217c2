// categorical_scalars.h — the records of the categorical tests from counts, for the table- and cell-taking scalars
// (anofox_g_test, anofox_cramers_v, anofox_contingency_coef, anofox_fisher_exact, anofox_mcnemar_test, anofox_phi_coefficient).
// categorical_scalars.cpp compiles categorical_tests.h as plain C++, where a wavefront is a loop over 64 lanes: the same text the
// kernels run, on the host, with no device touched.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace anofox {
namespace cattest {

// rec[12] of the chi-square (0) or G (1) test of a table flattened row by row, row i having row_lengths[i] cells (a short row's
// missing cells are 0).  Empty rows and columns are dropped, as the dense coding of the grouped entries drops them.
void ct_scalar_table(int test, int correction, const size_t *table, const size_t *row_lengths, size_t n_rows, double *rec);

// rec[12] of Fisher's (2) or McNemar's (3) test of the cells [[n11, n12], [n21, n22]]
void ct_scalar_cells(int test, int alternative, int correction, int exact, double confidence_level, size_t n11, size_t n12, size_t n21,
                     size_t n22, double *rec);

} // namespace cattest
} // namespace anofox
