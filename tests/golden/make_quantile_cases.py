"""Writes tests/golden/quantile/cases.json: quantile regression inputs with the optimum scipy's HiGHS dual simplex finds for
the standard linear program
    min tau 1'u+ + (1 - tau) 1'u-   s.t.   A beta + u+ - u- = y,   u+, u- >= 0,   beta free.
Where the optimum is a single vertex (k zero residuals, non-singular) the coefficients are re-solved from those k rows, so
they carry numpy's LU accuracy rather than the solver's feasibility tolerance.  Inputs are rounded to 3 decimals to keep the
file small; one 130 x 32 matrix serves every width (its first p columns, each width with a y of its own), every n (the first n rows), both
intercept settings and the three tau values.

Run from the repository root:  python tests/golden/make_quantile_cases.py   (needs scipy; the tests do not)"""
import json
import os
import sys

import numpy as np
from scipy.optimize import linprog

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import quantile_restate as qr  # noqa: E402

TAUS = (0.1, 0.5, 0.9)


def solve_lp(X, y, tau, fit_intercept):
    A = qr.design(X, fit_intercept)
    n, k = A.shape
    c = np.concatenate([np.zeros(k), np.full(n, tau), np.full(n, 1.0 - tau)])
    Aeq = np.hstack([A, np.eye(n), -np.eye(n)])
    res = linprog(c, A_eq=Aeq, b_eq=y, bounds=[(None, None)] * k + [(0, None)] * (2 * n), method="highs-ds")
    assert res.status == 0, res.message
    beta = res.x[:k]
    r = y - A @ beta
    zero = np.abs(r) <= 1e-9 * np.max(np.abs(y))
    if zero.sum() == k and np.linalg.matrix_rank(A[zero]) == k:
        beta = np.linalg.solve(A[zero], y[zero])
    b0 = float(beta[0]) if fit_intercept else None
    b = beta[1:] if fit_intercept else beta
    cert = qr.certify(X, y, tau, fit_intercept, b, b0 if fit_intercept else float("nan"))
    loss = qr.pinball_loss(X, y, tau, b, b0)
    assert loss <= res.fun * (1 + 1e-9) + 1e-12, (loss, res.fun)
    return dict(b=[float(v) for v in b], b0=b0, loss=loss, unique=bool(cert["decided"] and cert["strict"]))


def main():
    rng = np.random.default_rng(20240611)
    datasets, cases = [], []
    scale = rng.uniform(0.5, 4.0, size=32)
    shift = rng.uniform(-3.0, 3.0, size=32)
    base = np.round(rng.normal(size=(130, 32)) * scale + shift, 3)
    for p in (1, 2, 8, 9, 32):                       # width p: the first p columns of the 130 x 32 base, a y of its own;
        X = base[:, :p]                              # a case fits the first n rows
        beta = rng.uniform(-2.0, 2.0, size=p)
        y = np.round(X @ beta + 1.5 + rng.standard_t(3, size=130), 3)
        datasets.append(dict(p=p, y=y.tolist()))
        for icpt in (False, True):
            k = p + (1 if icpt else 0)
            for n in (k, k + 1, 63, 64, 65, 130):
                for tau in TAUS:
                    sol = solve_lp(X[:n], y[:n], tau, icpt)
                    cases.append(dict(table="gauss", dataset=len(datasets) - 1, n=n, tau=tau,
                                      fit_intercept=icpt, **sol))
    for name, (y, X) in qr.reference_tables().items():
        ok = np.isfinite(y)
        datasets.append(dict(p=X.shape[1], y=y[ok].tolist(), X=X[ok].ravel().tolist()))
        for icpt in (True, False):
            for tau in TAUS:
                sol = solve_lp(X[ok], y[ok], tau, icpt)
                cases.append(dict(table=name, dataset=len(datasets) - 1, n=int(ok.sum()), tau=tau,
                                  fit_intercept=icpt, **sol))
    out = os.path.join(HERE, "quantile", "cases.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    dump = lambda v: json.dumps(v, separators=(",", ":"))  # noqa: E731
    with open(out, "w") as f:                        # one data set, one case per line
        f.write('{"x_base":' + dump(base.ravel().tolist()) + ',\n"datasets":[\n' + ",\n".join(dump(d) for d in datasets) + '\n],"cases":[\n' + ",\n".join(dump(c) for c in cases) + "\n]}\n")
    n_unique = sum(c["unique"] for c in cases)
    print(f"{len(cases)} cases, {n_unique} unique, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
