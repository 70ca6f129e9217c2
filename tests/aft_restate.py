"""The yardstick of the AFT tests: the censored maximum likelihood fit of  log T = a'beta + sigma W  in numpy, row based, written
from the formulas of DESIGN.md §1 "Accelerated failure time models" and sharing neither the loop nor the solve with
csrc/aft_newton.h.

    l(theta) = sum_{event} [log f_W(z) - log sigma - log t] + sum_{censored} log S_W(z),   z = (log t - a'beta) / sigma,
    theta = (intercept?, beta[p], log sigma?);   W: extreme value (Weibull, exponential with sigma = 1), normal, logistic.

Newton's method from the least-squares fit of log t (by `lstsq`), every step by `numpy.linalg.solve` on -H (shifted to positive
definite by its smallest eigenvalue when it is not), with backtracking on l, until the score is at rounding level:
||g||_inf <= 1e-12 max(1, ||A' log t||_inf).  The normal kernel takes log S and the hazard from erfc(z / sqrt 2).  Besides the fit
it returns what the tests condition on: `max_abs_z` over the rows and `kappa`, the condition number of the information.

Row rules and statuses: a row is valid when time, event and every x are finite; 1 a valid row's time <= 0 or event not in {0, 1},
or every valid row censored; 10 no valid row; 6 fewer valid rows than k + 1; 3 the score never reached rounding level."""
import math

import numpy as np
from scipy.special import erfc, ndtri

WEIBULL, LOGNORMAL, LOGLOGISTIC, EXPONENTIAL = 0, 1, 2, 3
NAMES = {WEIBULL: "weibull", LOGNORMAL: "lognormal", LOGLOGISTIC: "loglogistic", EXPONENTIAL: "exponential"}
_LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


def scale_is_fixed(dist):
    return dist == EXPONENTIAL


def terms(dist, event, z):
    """Per row: c = log f_W(z) (event) or log S_W(z) (censored), u = dc/dz, v = d2c/dz2."""
    z = np.asarray(z, float)
    ev = np.asarray(event, bool)
    if dist in (WEIBULL, EXPONENTIAL):
        e = np.exp(np.clip(z, -700.0, 700.0))
        return np.where(ev, z - e, -e), np.where(ev, 1.0 - e, -e), -e
    if dist == LOGLOGISTIC:
        s = np.logaddexp(0.0, z)                      # log(1 + e^z)
        pr = np.exp(z - s)                            # logistic(z)
        q = np.exp(-s)                                # 1 - logistic(z)
        return np.where(ev, z - 2.0 * s, -s), np.where(ev, q - pr, -pr), np.where(ev, -2.0 * pr * q, -pr * q)
    if dist == LOGNORMAL:
        surv = 0.5 * erfc(z / math.sqrt(2.0))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            tail = surv <= 1e-300
            zt = np.where(tail, z, 1.0)
            log_s = np.where(tail, -0.5 * z * z - np.log(zt * math.sqrt(2.0 * math.pi)), np.log(np.where(tail, 1.0, surv)))
            r = np.where(tail, zt + 1.0 / zt - 2.0 / zt ** 3, np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi) / np.where(tail, 1.0, surv))
        return np.where(ev, -0.5 * z * z - _LOG_SQRT_2PI, log_s), np.where(ev, -z, -r), np.where(ev, -1.0, r * (z - r))
    raise ValueError("unknown distribution %r" % (dist,))


def kernel_cdf(dist, z):
    if dist in (WEIBULL, EXPONENTIAL):
        return -math.expm1(-math.exp(min(max(z, -700.0), 700.0)))
    if dist == LOGNORMAL:
        return 0.5 * math.erfc(-z / math.sqrt(2.0))
    e = math.exp(-abs(z))
    return 1.0 / (1.0 + e) if z >= 0 else e / (1.0 + e)


def kernel_quantile(dist, p):
    p = min(max(p, 1e-12), 1.0 - 1e-12)
    if dist in (WEIBULL, EXPONENTIAL):
        return math.log(-math.log1p(-p))
    if dist == LOGNORMAL:
        return float(ndtri(p))
    return math.log(p / (1.0 - p))


def cdf_time(dist, t, eta, scale):
    """P(T <= t); 0 for t <= 0."""
    return 0.0 if t <= 0.0 else kernel_cdf(dist, (math.log(t) - eta) / scale)


def quantile_time(dist, p, eta, scale):
    return math.exp(eta + scale * kernel_quantile(dist, p))


def loglik(dist, A, logt, delta, theta, fit_scale):
    kb = A.shape[1]
    ls = theta[kb] if fit_scale else 0.0
    z = (logt - A @ theta[:kb]) / math.exp(ls)
    c, _, _ = terms(dist, delta == 1.0, z)
    return float(np.sum(np.where(delta == 1.0, c - ls - logt, c)))


def derivatives(dist, A, logt, delta, theta, fit_scale):
    """-> (l, gradient[k], Hessian[k, k]) of the log-likelihood at theta = (beta, log sigma?) on the design A."""
    n, kb = A.shape
    ls = theta[kb] if fit_scale else 0.0
    k = kb + int(fit_scale)
    g, H = np.zeros(k), np.zeros((k, k))
    with np.errstate(all="ignore"):  # (a trial step far out gives infinities: the caller backtracks on a non-finite l)
        sigma = math.exp(min(ls, 700.0))
        z = (logt - A @ theta[:kb]) / sigma
        ev = delta == 1.0
        c, u, v = terms(dist, ev, z)
        ll = float(np.sum(np.where(ev, c - ls - logt, c)))
        g[:kb] = -(A.T @ u) / sigma
        H[:kb, :kb] = (A.T * v) @ A / (sigma * sigma)
        if fit_scale:
            g[kb] = float(np.sum(-u * z - delta))
            cross = A.T @ (v * z + u) / sigma
            H[:kb, kb] = H[kb, :kb] = cross
            H[kb, kb] = float(np.sum(v * z * z + u * z))
    return ll, g, H


def _newton(dist, A, logt, delta, fit_scale, max_newton):
    """-> (theta, l, converged): Newton's iteration to a score at rounding level."""
    n, kb = A.shape
    beta = np.linalg.lstsq(A, logt, rcond=None)[0]
    theta = beta
    if fit_scale:
        rss = float(np.sum((logt - A @ beta) ** 2))
        theta = np.append(beta, math.log(math.sqrt(max(rss / max(n - kb, 1), 1e-8))))
    bound = 1e-12 * max(1.0, float(np.max(np.abs(A.T @ logt))))
    ll, g, H = derivatives(dist, A, logt, delta, theta, fit_scale)
    for _ in range(max_newton):
        if not np.isfinite(ll) or not np.all(np.isfinite(g)) or not np.all(np.isfinite(H)):
            return theta, ll, False
        if np.max(np.abs(g)) <= bound:
            return theta, ll, True
        info = -H
        lam_min = float(np.min(np.linalg.eigvalsh(info)))
        floor = 1e-8 * max(1.0, float(np.max(np.abs(np.diag(info)))))
        if lam_min < floor:
            info = info + (floor - lam_min) * np.eye(len(g))
        step = np.linalg.solve(info, g)
        f, moved = 1.0, False
        for _ in range(60):
            trial = theta + f * step
            tl, tg, tH = derivatives(dist, A, logt, delta, trial, fit_scale)
            # near the mode l is flat to rounding: there a step is taken when it shrinks the score
            if np.isfinite(tl) and (tl > ll or (tl >= ll - 1e-9 * (1.0 + abs(ll)) and np.max(np.abs(tg)) < np.max(np.abs(g)))):
                theta, ll, g, H, moved = trial, tl, tg, tH, True
                break
            f *= 0.5
        if not moved:
            return theta, ll, False
    return theta, ll, bool(np.max(np.abs(g)) <= bound)


def _failed(status):
    return dict(status=status)


def prepare(time, x, event, fit_intercept):
    """The valid rows: -> (status, A[n, kb], log t[n], delta[n]); status 1 / 10 as the row rules say, else 0."""
    time, event = np.asarray(time, float), np.asarray(event, float)
    x = np.asarray(x, float).reshape(len(time), -1)
    ok = np.isfinite(time) & np.isfinite(event) & np.all(np.isfinite(x), axis=1)
    t, d, xv = time[ok], event[ok], x[ok]
    if np.any(t <= 0.0) or np.any((d != 0.0) & (d != 1.0)):
        return 1, None, None, None
    if len(t) == 0:
        return 10, None, None, None
    A = np.column_stack([np.ones(len(t)), xv]) if fit_intercept else xv
    return 0, A, np.log(t), d


def fit(dist, time, x, event, fit_intercept=True, max_newton=200):
    """x: [n, p].  -> dict(status, theta[k] (intercept?, beta, log sigma?), coef[p], intercept, log_sigma, scale, ll, null_ll, aic,
    bic, n_obs, n_events, n_censored, n_params, information[k, k], vcov[k, k], se[k], max_abs_z, kappa)."""
    status, A, logt, delta = prepare(time, x, event, fit_intercept)
    if status:
        return _failed(status)
    n, kb = A.shape
    fs = not scale_is_fixed(dist)
    k = kb + int(fs)
    n_events = int(np.sum(delta == 1.0))
    if n_events == 0:
        return _failed(1)
    if n < k + 1:
        return _failed(6)
    theta, ll, converged = _newton(dist, A, logt, delta, fs, max_newton)
    if not converged:
        return _failed(3)
    ll, g, H = derivatives(dist, A, logt, delta, theta, fs)
    info = -H
    try:
        vcov = np.linalg.inv(info)
    except np.linalg.LinAlgError:
        return _failed(3)
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.diag(vcov))
    null_ll = float("nan")
    if fit_intercept:
        th0, l0, ok0 = _newton(dist, np.ones((n, 1)), logt, delta, fs, max_newton)
        null_ll = l0 if ok0 else float("nan")
    ic = int(fit_intercept)
    ls = theta[kb] if fs else 0.0
    z = (logt - A @ theta[:kb]) / math.exp(ls)
    return dict(status=0, theta=theta, coef=theta[ic:kb].copy(), intercept=theta[0] if ic else float("nan"), log_sigma=ls,
                scale=math.exp(ls) if fs else 1.0, ll=ll, null_ll=null_ll, aic=2.0 * k - 2.0 * ll, bic=k * math.log(n) - 2.0 * ll,
                n_obs=n, n_events=n_events, n_censored=n - n_events, n_params=k, information=info, vcov=vcov, se=se, score=g,
                max_abs_z=float(np.max(np.abs(z))), max_abs_logt=float(np.max(np.abs(logt))), kappa=float(np.linalg.cond(info)))


def evaluate(dist, time, x, event, fit_intercept, theta):
    """l, the gradient and the information of the valid rows at a given theta (the certificate of a returned fit)."""
    status, A, logt, delta = prepare(time, x, event, fit_intercept)
    assert status == 0
    ll, g, H = derivatives(dist, A, logt, delta, np.asarray(theta, float), not scale_is_fixed(dist))
    return ll, g, -H
