"""The yardstick of the GLM tests: Poisson / log and binomial / logit maximum (penalised) likelihood in numpy, sharing
neither the loop nor the solve with csrc/glm_irls.h.

Newton's method on  deviance(beta) + lambda sum_j beta_j^2  (the intercept not penalised) from its own start (beta = 0, the
intercept at link(mean y)), with backtracking on the objective, every step by `lstsq` on the sqrt(w)-scaled rows (no normal
equations), until  ||X'(y - mu) - lambda beta||_inf <= 1e-12 max(1, ||X'y||_inf);  the last steps evaluate the score in
np.longdouble.  Besides the fit it returns what the tests condition on: `kappa` (the condition number of the column-scaled,
sqrt(w)-scaled design at the optimum), `max_abs_eta`, and `separated` (not converged, or max_abs_eta > 30).

Row rules and statuses are DESIGN.md §1 "Generalised linear models": 1 a finite y outside the support, 10 no valid row,
6 fewer valid rows than max(k, 1)."""
import math

import numpy as np

POISSON, BINOMIAL = 0, 1
_lgamma = np.vectorize(math.lgamma, otypes=[float])


def _mu(family, eta):
    if family == POISSON:
        return np.exp(eta)
    return 1.0 / (1.0 + np.exp(-eta))


def _xlogy(a, b):
    out = np.zeros_like(a)
    m = a > 0
    out[m] = a[m] * np.log(b[m])
    return out


def deviance(family, y, mu):
    if family == POISSON:
        return float(2.0 * np.sum(_xlogy(y, y / np.where(y > 0, mu, 1.0)) - (y - mu)))
    return float(2.0 * np.sum(_xlogy(y, y / np.where(y > 0, mu, 1.0)) + _xlogy(1.0 - y, (1.0 - y) / np.where(y < 1, 1.0 - mu, 1.0))))


def loglik(family, y, mu):
    if family == POISSON:
        return float(np.sum(_xlogy(y, mu) - mu - _lgamma(y + 1.0)))
    return float(np.sum(_xlogy(y, mu) + _xlogy(1.0 - y, 1.0 - mu)))


def _failed(status, n_rows):
    return dict(status=status, separated=False, kappa=np.inf, max_abs_eta=np.nan, mu_all=np.full(n_rows, np.nan))


def fit(family, y, x, offset=None, fit_intercept=True, lam=0.0, max_newton=200):
    """x: [n, p].  -> dict(status, coef[p] (NaN: dropped), intercept, deviance, null_deviance, aic, dispersion, n_obs, n_params,
    se[p], mu_all[n] (every row), kappa, max_abs_eta, separated, converged, dropped[p])."""
    y = np.asarray(y, float)
    x = np.asarray(x, float)
    x = x.reshape(len(y), x.shape[-1] if x.ndim == 2 else 1)
    n_rows, p = x.shape
    off = np.zeros(n_rows) if offset is None else np.asarray(offset, float)
    fin_y = np.isfinite(y)
    bad = fin_y & ((y < 0) if family == POISSON else ((y < 0) | (y > 1)))
    if bad.any():
        return _failed(1, n_rows)
    valid = fin_y & np.isfinite(x).all(axis=1) & np.isfinite(off)
    if not valid.any():
        return _failed(10, n_rows)
    yv, xv, ov = y[valid], x[valid], off[valid]
    n = len(yv)
    dropped = np.zeros(p, bool)
    if fit_intercept:
        dropped = (np.abs(xv - xv[0]) < 1e-10).all(axis=0)
    keep = np.flatnonzero(~dropped)
    k = len(keep) + (1 if fit_intercept else 0)
    if n < max(k, 1):
        return _failed(6, n_rows)
    A = np.hstack([np.ones((n, 1)), xv[:, keep]]) if fit_intercept else xv[:, keep]
    pen = np.full(k, lam)
    if fit_intercept:
        pen[0] = 0.0
    ybar = yv.mean()
    beta = np.zeros(k)
    if fit_intercept:
        beta[0] = math.log(max(ybar, 1e-8)) if family == POISSON else math.log(min(max(ybar, 1e-8), 1 - 1e-8) / (1 - min(max(ybar, 1e-8), 1 - 1e-8)))

    def objective(b):
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            return deviance(family, yv, _mu(family, A @ b + ov)) + float(np.sum(pen * b * b))

    Al, yl, ol, pl = A.astype(np.longdouble), yv.astype(np.longdouble), ov.astype(np.longdouble), pen.astype(np.longdouble)

    def score(b):  # in double far from the optimum, in long double for the final polish
        with np.errstate(over="ignore", invalid="ignore"):
            g = A.T @ (yv - _mu(family, A @ b + ov)) - pen * b
        if not np.all(np.isfinite(g)) or float(np.max(np.abs(g))) > 1e4 * goal:
            return g
        bl = b.astype(np.longdouble)
        eta = Al @ bl + ol
        mu = np.exp(eta) if family == POISSON else 1 / (1 + np.exp(-eta))
        return Al.T @ (yl - mu) - pl * bl

    goal = 1e-12 * max(1.0, float(np.max(np.abs(A.T @ yv))))
    sq_pen = np.diag(np.sqrt(pen))[pen > 0]
    converged = False
    obj = objective(beta)
    for _ in range(max_newton):
        g = score(beta)
        if float(np.max(np.abs(g))) <= goal:
            converged = True
            break
        with np.errstate(over="ignore"):
            mu = _mu(family, A @ beta + ov)
        w = mu if family == POISSON else mu * (1 - mu)
        if not np.all(np.isfinite(w)) or not np.any(w > 0):
            break
        sw = np.sqrt(w)
        # the Newton step: min || sqrt(w) (A d) - g-equivalent ||: solve the weighted least squares for d with right-hand side
        # r = (y - mu) / w - pen-part, through the stacked rows [sqrt(w) A; sqrt(pen)] d = [sqrt(w) (y - mu) / w; -sqrt(pen) beta]
        rows = np.vstack([A * sw[:, None], sq_pen]) if len(sq_pen) else A * sw[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            rhs_top = np.where(w > 0, (yv - mu) / sw, 0.0)
        rhs = np.concatenate([rhs_top, -(np.sqrt(pen) * beta)[pen > 0]]) if len(sq_pen) else rhs_top
        d = np.linalg.lstsq(rows, rhs, rcond=1e-12)[0]
        polish = float(np.max(np.abs(g))) <= 1e4 * goal  # the objective no longer resolves the step: take it whole
        t, accepted = 1.0, polish
        cand, o = beta + d, obj
        for _ in range(0 if polish else 40):
            cand = beta + t * d
            o = objective(cand)
            if np.isfinite(o) and o <= obj + 1e-14 * abs(obj):
                accepted = True
                break
            t /= 2
        if not accepted:
            break
        beta, obj = cand, o
    eta = A @ beta + ov
    max_abs_eta = float(np.max(np.abs(eta)))
    separated = (not converged) or max_abs_eta > 30
    with np.errstate(over="ignore"):
        mu = _mu(family, eta)
    w = mu if family == POISSON else mu * (1 - mu)
    S = A * np.sqrt(w)[:, None]
    norms = np.linalg.norm(S, axis=0)
    Sp = np.vstack([S, sq_pen]) if len(sq_pen) else S  # (a ridge term makes aliased columns estimable: it counts)
    norms = np.linalg.norm(Sp, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sv = np.linalg.svd(Sp / np.where(norms > 0, norms, 1.0), compute_uv=False) if np.all(np.isfinite(Sp)) else np.array([np.nan])
    rank = int(np.sum(sv > 1e-6 * sv[0])) if np.all(np.isfinite(sv)) else 0
    kappa = float(sv[0] / sv[-1]) if rank == k and sv[-1] > 0 else np.inf
    out = dict(status=0, separated=bool(separated), converged=bool(converged), kappa=kappa, max_abs_eta=max_abs_eta, n_obs=n,
               n_params=rank, dropped=dropped, k=k, sum_y=float(np.sum(yv)))
    coef = np.full(p, np.nan)
    coef[keep] = beta[1:] if fit_intercept else beta
    out["coef"] = coef
    out["intercept"] = float(beta[0]) if fit_intercept else np.nan
    dev = deviance(family, yv, mu)
    mu0 = np.full(n, ybar)
    null_dev = deviance(family, yv, mu0) if 0 < ybar and (family == POISSON or ybar < 1) else 0.0
    out["deviance"], out["null_deviance"] = dev, null_dev
    out["aic"] = -2.0 * loglik(family, yv, mu) + 2.0 * rank
    disp = 1.0
    if family == POISSON and n > rank:
        with np.errstate(divide="ignore", invalid="ignore"):
            disp = max(1.0, float(np.sum((yv - mu) ** 2 / mu)) / (n - rank))
    out["dispersion"] = disp
    se = np.full(p, np.nan)
    if rank == k and np.isfinite(kappa):
        info = S.T @ S + np.diag(pen)
        d = np.sqrt(disp * np.diag(np.linalg.inv(info)))
        se[keep] = d[1:] if fit_intercept else d
    out["se"] = se
    # mu of every row (training or not): NaN where x or the offset is not finite
    b_all = np.where(np.isnan(coef), 0.0, coef)
    with np.errstate(invalid="ignore", over="ignore"):
        eta_all = x @ b_all + off + (beta[0] if fit_intercept else 0.0)
        out["mu_all"] = np.where(np.isfinite(eta_all), _mu(family, eta_all), np.nan)
    return out
