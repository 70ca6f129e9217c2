// scalar_fit.h — what the one-group entry points (anofox_*_fit) share around their family's host batch call of one group: the
// expansion of the inputs, the reference's error text of a record's status, the malloc'ed coefficients.  Host only.  Every
// entry keeps its own leading checks in its own order, its extra status texts and its result struct.
#pragma once
#include <stdlib.h>

#include "context.h"

namespace anofox {
namespace host {

inline void set_dimension_mismatch(size_t y_len, size_t x_len, AnofoxError *e) {
	set_error(e, ANOFOX_ERROR_DIMENSION_MISMATCH,
	          "Dimension mismatch: y has " + std::to_string(y_len) + " elements, X has " + std::to_string(x_len) + " rows");
}

// every column as long as y (the first that is not names itself)
inline bool check_column_lengths(size_t y_len, const AnofoxDataArray *x, size_t x_count, AnofoxError *e) {
	for (size_t j = 0; j < x_count; ++j)
		if (x[j].len != y_len) { set_dimension_mismatch(y_len, x[j].len, e); return false; }
	return true;
}

// The rows of a one-group call as a host batch takes them: NULL entries -> NaN through the validity bitmask.  The kernels
// apply the aggregate's "< 2 rows -> NULL" rule from row_offsets; a single-group call has no such rule (ols.rs accepts
// n == 1), so a one-row input is padded with one all-NaN row, which the row filter drops again.
struct ScalarFitInput {
	size_t p, n, n_pad;
	std::vector<std::vector<double>> cols;
	std::vector<double> yv, wv;
	std::vector<const double *> xp;
	int64_t off[2];

	ScalarFitInput(const AnofoxDataArray &y, const AnofoxDataArray *x, size_t x_count, const AnofoxDataArray *weights = nullptr)
	    : p(x_count), n(y.len), n_pad(y.len < 2 ? 2 : y.len), cols(x_count), xp(x_count), off{0, (int64_t)(y.len < 2 ? 2 : y.len)} {
		expand_data_array(y, yv, n_pad);
		for (size_t j = 0; j < p; ++j) {
			expand_data_array(x[j], cols[j], n_pad);
			xp[j] = cols[j].data();
		}
		if (weights) expand_data_array(*weights, wv, n_pad);
	}
	const double *w() const { return wv.empty() ? nullptr : wv.data(); }
	// the rows the fit keeps: finite y and x, and a finite weight > 0 where the call has weights
	size_t n_valid() const {
		size_t k = 0;
		for (size_t i = 0; i < n; ++i) {
			bool ok = isfinite(yv[i]);
			for (size_t j = 0; ok && j < p; ++j) ok = isfinite(cols[j][i]);
			if (ok && !wv.empty()) ok = wv[i] > 0.0 && isfinite(wv[i]);
			k += ok;
		}
		return k;
	}
};

// A record's status != 0 as the reference's error (crates/anofox-stats-core/src/errors.rs) under `code`: the two texts every
// family shares, `other` for any other status.
inline void set_scalar_fit_error(int status, AnofoxErrorCode code, const ScalarFitInput &in, const std::string &other, AnofoxError *e) {
	std::string msg;
	switch (status) {
	case ANOFOX_ERROR_NO_VALID_DATA: msg = "All rows filtered due to NULL/NaN values"; break;
	case ANOFOX_ERROR_INSUFFICIENT_DATA:
		msg = "Insufficient data: " + std::to_string(in.n_valid()) + " rows, " + std::to_string(in.p) + " features (need rows > features)";
		break;
	default: msg = other; break;
	}
	set_error(e, code, msg);
}

// the malloc'ed coefficients of one record (nullptr with `e` set when the allocation fails)
inline double *copy_coefficients(const double *rec, size_t p, AnofoxError *e) {
	double *coef = (double *)malloc(p * sizeof(double));
	if (!coef) { set_error(e, ANOFOX_ERROR_ALLOCATION_FAILURE, "Failed to allocate coefficients"); return nullptr; }
	memcpy(coef, rec, p * sizeof(double));
	return coef;
}

// the result of one record in the regression layout (p + 6)
inline bool fill_scalar_result(const double *core, size_t p, AnofoxFitResultCore *out_core, AnofoxError *e) {
	double *coef = copy_coefficients(core, p, e);
	if (!coef) return false;
	out_core->coefficients = coef;
	out_core->coefficients_len = p;
	out_core->intercept = core[p];
	out_core->r_squared = core[p + 1];
	out_core->adj_r_squared = core[p + 2];
	out_core->residual_std_error = core[p + 3];
	out_core->n_observations = (size_t)core[p + 4];
	out_core->n_features = p;
	return true;
}

} // namespace host
} // namespace anofox
