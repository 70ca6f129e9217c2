"""Quantile regression restated in numpy: the pinball loss, a certificate of optimality for a candidate solution, and the
row and option rules of DESIGN.md §1 "Quantile regression".  No solver here: the answer is defined by its optimality
conditions, and any candidate is checked with one k x k solve.

The linear program  min sum_i rho_tau(y_i - b0 - x_i'b),  rho_tau(r) = r (tau - [r < 0]),  has a vertex optimum: k = p +
[intercept] rows with zero residual (the set Z) whose multipliers a, A_Z' a = -sum_{i not in Z} psi(r_i) a_i with psi = tau
for r > 0 and tau - 1 for r < 0, lie in [tau - 1, tau].  Strictly inside: the optimum is unique."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantile", "cases.json")

STATUS_INVALID_INPUT = 1
STATUS_INSUFFICIENT_DATA = 6
STATUS_NO_VALID_DATA = 10
STATUS_TOO_FEW_ROWS = 100


def design(X, fit_intercept):
    X = np.asarray(X, dtype=np.float64)
    return np.column_stack([np.ones(len(X)), X]) if fit_intercept else X


def valid_rows(X, y):
    X = np.asarray(X, dtype=np.float64)
    return np.isfinite(np.asarray(y, dtype=np.float64)) & np.isfinite(X).all(axis=1)


def pinball_loss(X, y, tau, b, b0):
    """sum over the valid rows of rho_tau(y - b0 - x'b); b0 None or NaN = no intercept."""
    ok = valid_rows(X, y)
    X, y = np.asarray(X, dtype=np.float64)[ok], np.asarray(y, dtype=np.float64)[ok]
    r = y - X @ np.asarray(b, dtype=np.float64) - (0.0 if b0 is None or np.isnan(b0) else b0)
    return float(np.sum(np.where(r >= 0, tau * r, (tau - 1.0) * r)))


def certify(X, y, tau, fit_intercept, b, b0):
    """-> dict(n_zero, k, decided, optimal, strict).  decided: |Z| == k and A_Z is non-singular, so the multipliers exist
    and are unique; optimal: they lie in [tau - 1, tau] (1e-9 slack for the solve's rounding); strict: inside by 1e-7."""
    ok = valid_rows(X, y)
    A = design(np.asarray(X, dtype=np.float64)[ok], fit_intercept)
    yv = np.asarray(y, dtype=np.float64)[ok]
    beta = np.concatenate([[b0], b]) if fit_intercept else np.asarray(b, dtype=np.float64)
    k = A.shape[1]
    r = yv - A @ beta
    zero = np.abs(r) <= 1e-9 * np.max(np.abs(yv))
    out = dict(n_zero=int(zero.sum()), k=k, decided=False, optimal=False, strict=False)
    if out["n_zero"] != k:
        return out
    AZ = A[zero]
    if np.linalg.matrix_rank(AZ) < k:
        return out
    psi = np.where(r > 0, tau, tau - 1.0)
    rhs = -(A[~zero] * psi[~zero][:, None]).sum(axis=0)
    a = np.linalg.solve(AZ.T, rhs)
    out["decided"] = True
    out["optimal"] = bool((a >= tau - 1.0 - 1e-9).all() and (a <= tau + 1e-9).all())
    out["strict"] = bool((a >= tau - 1.0 + 1e-7).all() and (a <= tau - 1e-7).all())
    return out


def rule_status(X, y, tau, fit_intercept, rule_count=None):
    """The status a group gets before any solve (0: it is fitted)."""
    X = np.asarray(X, dtype=np.float64)
    if not (0.0 < tau < 1.0):                      # NaN fails both comparisons
        return STATUS_INVALID_INPUT
    if (len(y) if rule_count is None else rule_count) < 2:
        return STATUS_TOO_FEW_ROWS
    n_valid = int(valid_rows(X, y).sum())
    if n_valid == 0:
        return STATUS_NO_VALID_DATA
    if n_valid < X.shape[1] + (1 if fit_intercept else 0):
        return STATUS_INSUFFICIENT_DATA
    return 0


def reference_tables():
    """The integer tables of the reference's test/sql/fit_predict_agg/test_quantile_fit_predict_agg.test, as (y, X) with
    None-free floats; y is NaN on the rows the SQL leaves NULL (prediction rows)."""
    i = np.arange(1, 11, dtype=np.float64)
    t = {"test_data": (np.where(i <= 7, 2.0 * i + 1.0 + (i % 3) - 1.0, np.nan), np.column_stack([i, 0.5 * i]))}
    i = np.arange(1, 26, dtype=np.float64)
    t["high_dim"] = (np.where(i <= 20, 1.5 * i + (i % 4), np.nan), np.column_stack([i, 2 * i, 3 * i, 4 * i, 5 * i]))
    i = np.arange(1, 101, dtype=np.float64)
    t["large_data"] = (np.where(i <= 80, 2.0 * i + 1.0 + (i % 7), np.nan), np.column_stack([i, 0.5 * i]))
    i = np.arange(1, 11, dtype=np.float64)
    t["outlier_data"] = (np.where(i == 5, 1000.0, np.where(i <= 8, 2.0 * i, np.nan)), i[:, None].copy())
    return t


def load_cases():
    """-> list of dict(name, X, y, tau, fit_intercept, b, b0, loss, unique) from tests/golden/quantile/cases.json."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    base = np.array(doc["x_base"], dtype=np.float64).reshape(130, 32)      # a data set without an X of its own: the first p columns
    data = [(np.array(d["y"], dtype=np.float64),
             np.array(d["X"], dtype=np.float64).reshape(len(d["y"]), d["p"]) if "X" in d else np.ascontiguousarray(base[:, :d["p"]]))
            for d in doc["datasets"]]
    out = []
    for c in doc["cases"]:
        y, X = data[c["dataset"]]
        y, X = y[:c["n"]], X[:c["n"]]                # a case fits the first n rows of its data set
        name = (f"gauss p={X.shape[1]} icpt={int(c['fit_intercept'])} n={c['n']} tau={c['tau']}" if c["table"] == "gauss"
                else f"{c['table']} icpt={int(c['fit_intercept'])} tau={c['tau']}")
        out.append(dict(name=name, X=X, y=y, tau=c["tau"], fit_intercept=bool(c["fit_intercept"]),
                        b=np.array(c["b"], dtype=np.float64), b0=c["b0"] if c["b0"] is not None else float("nan"),
                        loss=c["loss"], unique=bool(c["unique"])))
    return out
