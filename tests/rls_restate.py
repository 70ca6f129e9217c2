"""NumPy restatement of the reference's recursive least squares (fit_rls / RlsState::update,
crates/anofox-stats-core/src/models/rls.rs) in its exact operation order.

Every summation runs in a Python loop along its summation index; only independent indices are vectorised, so every
rounding is the reference's (NumPy never fuses a multiply with an add).  Rust's f64 `Sum` folds from -0.0; the explicit
`+=` loops of the reference (P x, k x' P) start from 0.0.  The P update is done in place, row by row, as the reference
does it: row i reads the rows l < i that this step already rewrote.

A record has the library's layout: coefficients[p], intercept, r2, adj r2, sigma (NaN), n_obs, status.
"""
import numpy as np

STATUS_INVALID_INPUT = 1
STATUS_INSUFFICIENT_DATA = 6
STATUS_NO_VALID_DATA = 10
STATUS_TOO_FEW_ROWS = 100


def fail_record(p, status):
    rec = np.full(p + 6, np.nan)
    rec[p + 5] = status
    return rec


def _filter(rows_y, rows_x, lam, delta, textbook=False):
    """The filter over the reduced design rows_x (n x d, slot order), from b = 0 and P = delta I."""
    n, d = rows_x.shape
    b = np.zeros(d)
    P = np.zeros((d, d))
    for i in range(d):
        P[i, i] = delta
    for t in range(n):
        u = rows_x[t]
        yhat = -0.0
        for i in range(d):
            yhat = yhat + u[i] * b[i]
        e = rows_y[t] - yhat
        px = np.zeros(d)
        for j in range(d):          # px_i += P_ij u_j in j order, vectorised over i
            px = px + P[:, j] * u[j]
        xpx = -0.0
        for i in range(d):
            xpx = xpx + u[i] * px[i]
        den = lam + xpx
        k = px / den
        b = b + k * e
        src = P.copy() if textbook else P   # textbook RLS reads the old P throughout
        for i in range(d):                  # in place: row i sees the rows l < i of this step
            s = np.zeros(d)
            for l in range(d):              # vectorised over j
                s = s + (k[i] * u[l]) * src[l, :]
            P[i, :] = (P[i, :] - s) / lam
    return b


def rls_fit(y, X, forgetting_factor=1.0, initial_p_diagonal=100.0, fit_intercept=True, textbook=False):
    """fit_rls of one group: y (n,), X (n, p).  Returns the record (p + 6)."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64).reshape(len(y), -1)
    p = X.shape[1]
    valid = np.isfinite(y) & np.all(np.isfinite(X), axis=1)
    idx = np.nonzero(valid)[0]
    if len(idx) == 0:
        return fail_record(p, STATUS_NO_VALID_DATA)
    first = X[idx[0]]
    const = np.array([bool(np.all(np.abs(X[idx, j] - first[j]) < 1e-10)) for j in range(p)], dtype=bool)
    active = np.nonzero(~const)[0]
    rec = np.full(p + 6, np.nan)
    rec[p + 4] = len(idx)
    rec[p + 5] = 0
    if len(active) == 0:
        if not fit_intercept:
            return fail_record(p, STATUS_INSUFFICIENT_DATA)
        s = -0.0
        for i in idx:
            s = s + y[i]
        rec[p] = s / float(len(idx))
        return rec
    if forgetting_factor <= 0.0 or forgetting_factor > 1.0 or initial_p_diagonal <= 0.0:
        return fail_record(p, STATUS_INVALID_INPUT)
    cols = [X[idx, j] for j in active]
    if fit_intercept:
        cols = [np.ones(len(idx))] + cols
    b = _filter(y[idx], np.stack(cols, axis=1), float(forgetting_factor), float(initial_p_diagonal), textbook)
    off = 1 if fit_intercept else 0
    for k, j in enumerate(active):
        rec[j] = b[off + k]
    if fit_intercept:
        rec[p] = b[0]
    return rec


def predict(rec, x):
    """anofox_predict_with_interval's yhat (ffi lib.rs:2292-2300): intercept (0 when NaN) + sum of the non-NaN coef_j x_j."""
    p = len(rec) - 6
    yhat = 0.0 if np.isnan(rec[p]) else rec[p]
    for j in range(p):
        if not np.isnan(rec[j]):
            yhat = yhat + rec[j] * x[j]
    return yhat


def batch(row_offsets, y, x_cols, train_counts=None, **opts):
    """Records of every group, with the aggregates' "fewer than 2 rows -> NULL" rule (status 100)."""
    X = np.stack([np.asarray(c, dtype=np.float64) for c in x_cols], axis=1)
    p = X.shape[1]
    out = []
    for g in range(len(row_offsets) - 1):
        lo, hi = int(row_offsets[g]), int(row_offsets[g + 1])
        cnt = hi - lo if train_counts is None else int(train_counts[g])
        out.append(fail_record(p, STATUS_TOO_FEW_ROWS) if cnt < 2 else rls_fit(y[lo:hi], X[lo:hi], **opts))
    return np.array(out).reshape(len(row_offsets) - 1, p + 6)


def frame_prediction(y, X, lo, hi, fit_intercept=True, **opts):
    """The window function's value for the frame [lo, hi): NaN unless MORE than p + [intercept] rows with non-NULL y."""
    p = X.shape[1]
    if hi <= lo:
        return np.nan
    if int(np.sum(~np.isnan(y[lo:hi]))) <= p + (1 if fit_intercept else 0):
        return np.nan
    rec = rls_fit(y[lo:hi], X[lo:hi], fit_intercept=fit_intercept, **opts)
    return predict(rec, X[hi - 1]) if rec[p + 5] == 0 else np.nan
