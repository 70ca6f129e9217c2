"""A row-based, extended-precision restatement of the elastic net contract ("Elastic net"): the yardstick of
the family sweeps.  It shares no code with the library or with test_elasticnet_cpu.en_reference.

Per group: the row filter, the constant-column rule, the statuses and the intercept-only shortcut; the centred moments
(raw without an intercept) summed from the rows in np.longdouble (x86: 64-bit mantissa, eps 1.08e-19); then THE minimiser,
found independently of any sweep order: coordinate descent in extended precision proposes a support and its signs, the
stationarity system  (C_AA + lambda (1 - l1) I) b_A = c_A - lambda l1 sign(b_A)  is solved directly by a Cholesky
factorisation written here in extended precision, and the result is accepted only when it satisfies the KKT conditions
of the problem in extended precision (signs as assumed, |g_j| <= lambda l1 off the support).  The problem is convex and,
under the input conditions below, strictly so: a point that satisfies its KKT conditions is the minimiser whatever
proposed it.  The statistics are summed from the residuals of the rows.

Also here: the conditions the sweeps put on generated inputs (on this module's output; a list of violations)."""
import numpy as np

LD = np.longdouble
if not np.finfo(LD).eps < 1e-18:          # pragma: no cover  (platforms whose long double is binary64)
    raise ImportError("elasticnet_restate needs an extended-precision np.longdouble (eps < 1e-18)")

STATUS_ALPHA, STATUS_L1, STATUS_INSUFFICIENT, STATUS_NO_VALID, STATUS_TOO_FEW_ROWS = 4, 5, 6, 10, 100
KKT_TOL = LD(1e-15)                       # extended-precision residual of an accepted stationarity system / sign test


def cholesky_solve(A, r):
    """x with A x = r for a symmetric positive definite longdouble A (lower Cholesky, column by column); None when a pivot
    is not positive."""
    k = len(r)
    L = np.zeros((k, k), dtype=LD)
    for j in range(k):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            return None
        L[j:, j] = col / np.sqrt(col[0])
    z = np.zeros(k, dtype=LD)
    for j in range(k):                    # L z = r
        z[j] = (r[j] - L[j, :j] @ z[:j]) / L[j, j]
    x = np.zeros(k, dtype=LD)
    for j in range(k - 1, -1, -1):        # L' x = z
        x[j] = (z[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def _sweeps(Cm, c, b, pen1, pen2, count):
    """`count` cyclic coordinate-descent sweeps on b (in place); returns the largest coordinate change of the last one."""
    g = c - Cm @ b
    d = np.diag(Cm)
    dmax = LD(0)
    for _ in range(count):
        dmax = LD(0)
        for j in range(len(c)):
            z = g[j] + d[j] * b[j]
            bn = (z - pen1 if z > pen1 else (z + pen1 if z < -pen1 else LD(0))) / (d[j] + pen2)
            delta = bn - b[j]
            if delta != 0:
                g -= Cm[:, j] * delta
                b[j] = bn
                dmax = max(dmax, abs(delta) * np.sqrt(d[j]))
    return dmax


def _certified(Cm, c, b, pen1, pen2):
    """The direct solve on the support and signs of b; the solution when it passes the KKT conditions, else None."""
    A = np.nonzero(b != 0)[0]
    out = np.zeros(len(c), dtype=LD)
    scale = max(pen1, np.max(np.abs(c))) if len(c) else LD(1)
    if len(A):
        s = np.sign(b[A])
        sol = cholesky_solve(Cm[np.ix_(A, A)] + pen2 * np.eye(len(A), dtype=LD), c[A] - pen1 * s)
        if sol is None or np.any(np.sign(sol) != s):
            return None
        out[A] = sol
    g = c - Cm @ out
    if len(A) and np.max(np.abs(g[A] - pen2 * out[A] - pen1 * np.sign(out[A]))) > KKT_TOL * scale * len(c):
        return None
    off = np.ones(len(c), dtype=bool)
    off[A] = False
    if off.any() and np.max(np.abs(g[off])) > pen1:
        return None
    return out


def minimise(Cm, c, lam, l1, max_sweeps=2_000_000):
    """(b, g = c - C b) of the minimiser of  1/2 b'Cb - c'b + lam (l1 |b|_1 + (1 - l1)/2 |b|^2)  in extended precision."""
    pen1, pen2 = LD(lam) * LD(l1), LD(lam) * (LD(1) - LD(l1))
    b = np.zeros(len(c), dtype=LD)
    block, done = 8, 0
    while True:
        dmax = _sweeps(Cm, c, b, pen1, pen2, block)
        done += block
        sol = _certified(Cm, c, b, pen1, pen2)
        if sol is not None:
            return sol, c - Cm @ sol
        if dmax == 0 or done >= max_sweeps:
            raise ArithmeticError("elasticnet_restate: no support passes the KKT conditions (degenerate or singular problem)")
        block = min(2 * block, 4096)


def fit_en(y, X, alpha=1.0, l1_ratio=0.5, fit_intercept=True, lambda_scaling="raw", rule_count=None, lambda_factor=1.0):
    """One group.  Returns a dict: status, p and, for status 0, the record's fields plus what the input conditions need
    (valid rows, constant mask, lam, the gradient g on the non-constant columns, c, q_yy, c_yy).  `lambda_factor` multiplies
    the penalty (the pinned test beyond the glmnet boundary brackets a perturbed lambda with it)."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    X = X if X.ndim == 2 else X.reshape(len(y), -1)
    p = X.shape[1]
    out = {"status": 0, "p": p}
    if (len(y) if rule_count is None else rule_count) < 2:
        out["status"] = STATUS_TOO_FEW_ROWS
    elif not alpha >= 0:
        out["status"] = STATUS_ALPHA
    elif not 0 <= l1_ratio <= 1:
        out["status"] = STATUS_L1
    if out["status"]:
        return out
    ok = np.isfinite(y) & np.isfinite(X).all(axis=1)
    if not ok.any():
        out["status"] = STATUS_NO_VALID
        return out
    yv, Xv = y[ok], X[ok]
    n = len(yv)
    const = (np.abs(Xv - Xv[0]) < 1e-10).all(axis=0)
    k = int((~const).sum())
    icpt = 1 if fit_intercept else 0
    yl = yv.astype(LD)
    ybar = yl.sum() / n
    cyy = ((yl - ybar) ** 2).sum()
    qyy = (yl * yl).sum()
    nanp = np.full(p, np.nan)
    if k == 0:
        if not fit_intercept:
            out["status"] = STATUS_INSUFFICIENT
            return out
        with np.errstate(all="ignore"):
            sd = float(np.sqrt(cyy / LD(n - 1)))
        out.update(coefficients=nanp, intercept=float(ybar), r_squared=0.0, adj_r_squared=0.0, residual_std_error=sd,
                   n_observations=n, valid=ok, const=const, shortcut=True, df=n - 1)
        return out
    if n < k + icpt:
        out["status"] = STATUS_INSUFFICIENT
        return out
    Xl = Xv[:, ~const].astype(LD)
    xbar = Xl.sum(axis=0) / n if fit_intercept else np.zeros(k, dtype=LD)
    Xc, yc = Xl - xbar, yl - (ybar if fit_intercept else LD(0))
    Cm, c, syy = Xc.T @ Xc, Xc.T @ yc, (yc * yc).sum()
    lam = LD(alpha) * LD(lambda_factor)
    if lambda_scaling == "glmnet":
        lam = LD(n) * lam / np.sqrt(cyy / LD(n))
    b, g = minimise(Cm, c, lam, l1_ratio)
    b0 = ybar - xbar @ b if fit_intercept else LD(0)
    r = yl - b0 - Xl @ b
    rss = (r * r).sum()
    df = n - (k + icpt)
    with np.errstate(all="ignore"):
        r2 = LD(1) - rss / syy
        adj = LD(1) - (LD(1) - r2) * LD(n - icpt) / LD(df)
        rse = np.sqrt(rss / LD(df))
    coef = nanp.copy()
    coef[~const] = b.astype(np.float64)
    out.update(coefficients=coef, intercept=(float(b0) if fit_intercept else np.nan), r_squared=float(r2),
               adj_r_squared=float(adj), residual_std_error=float(rse), n_observations=n, valid=ok, const=const, shortcut=False,
               df=df, lam=float(lam), l1_ratio=float(l1_ratio), g=g.astype(np.float64), c=c.astype(np.float64),
               q_yy=float(qyy), c_yy=float(cyy), fit_intercept=bool(fit_intercept), lambda_scaling=lambda_scaling)
    return out


def record(res):
    """The library's p + 6 core record of a restated fit."""
    p = res["p"]
    rec = np.full(p + 6, np.nan)
    rec[p + 5] = res["status"]
    if res["status"] != 0:
        return rec
    rec[:p] = res["coefficients"]
    rec[p:p + 5] = [res["intercept"], res["r_squared"], res["adj_r_squared"], res["residual_std_error"], res["n_observations"]]
    return rec


def kappa_bound(p):
    """The largest condition number a moment-based solve of p columns may meet: it loses about p kappa^2 2^-53, which the
    bound holds at a tenth of the 1e-9 coefficient tolerance."""
    return float(np.sqrt(1e-10 / (p * 2.0 ** -53)))


def design_kappa(D):
    """Condition number of the design D (penalty rows already appended) after its columns are scaled to unit norm."""
    if D.shape[1] == 0:
        return 1.0
    nrm = np.linalg.norm(D, axis=0)
    if not np.all(nrm > 0):
        return np.inf
    sv = np.linalg.svd(D / nrm, compute_uv=False)
    return float(sv[0] / sv[-1]) if sv[-1] > 0 else np.inf


def input_conditions(res, y, X):
    """The conditions the sweeps put on a generated case, evaluated on the restatement's output; a list of violations."""
    bad = []
    if res["status"] != 0 or res["shortcut"]:
        return bad
    ok, const = res["valid"], res["const"]
    Xv = np.asarray(X, dtype=np.float64)[ok][:, ~const]
    b, g, c = res["coefficients"][~const], res["g"], res["c"]
    pen1, pen2 = res["lam"] * res["l1_ratio"], res["lam"] * (1.0 - res["l1_ratio"])
    act = b != 0
    scale = max(pen1, float(np.max(np.abs(c))))
    if (~act).any() and (np.abs(np.abs(g[~act]) - pen1) < 1e-6 * scale).any():
        bad.append("an inactive column's gradient lies within 1e-6 of the threshold (degenerate support)")
    if act.any() and (np.abs(b[act]) < 1e-6 * np.max(np.abs(b[act]))).any():
        bad.append("an active coefficient is below 1e-6 of the largest one")
    n, ka = Xv.shape[0], int(act.sum())
    cols = ([np.ones((n, 1))] if res["fit_intercept"] else []) + [Xv[:, act]]
    D = np.concatenate(cols, axis=1)
    if pen2 > 0 and ka:
        pad = np.zeros((ka, D.shape[1]))
        pad[:, D.shape[1] - ka:] = np.sqrt(pen2) * np.eye(ka)
        D = np.concatenate([D, pad], axis=0)
    kap = design_kappa(D)
    res["kappa"] = kap
    if not res["p"] * kap * kap * 2.0 ** -53 <= 1e-10:
        bad.append(f"p kappa^2 2^-53 above 1e-10 (kappa {kap:.3g}, bound {kappa_bound(res['p']):.3g})")
    if res["lambda_scaling"] == "glmnet" and not res["fit_intercept"] and not res["q_yy"] < 1e4 * res["c_yy"]:
        bad.append("glmnet scaling without an intercept with q_yy >= 1e4 c_yy")
    return bad
