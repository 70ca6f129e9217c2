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


# ---- a solver that shares nothing with csrc/quantile_solve.h: interior point on the dual, then a crossover ----------------
# Frisch-Newton (Portnoy & Koenker 1997, "The Gaussian hare and the Laplacian tortoise"): the dual of the linear program,
#     max y'a   s.t.  A'a = (1 - tau) A'1,  0 <= a <= 1,
# by a primal-dual log-barrier iteration with Mehrotra's predictor-corrector step.  No basis, no pivot rule, no tolerance of
# the kernel's: the iterate is an interior point, its duality gap bounds the distance of its loss from the optimum.

def _step_bound(v, dv):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(dv < 0, -v / dv, 1e20)


def _frisch_newton(U, y, tau):
    """U: n x r, orthonormal columns spanning the design's column space.  -> (g, primal, dual): the fit is U g, primal its
    pinball loss, dual the objective of the feasible dual point a (a lower bound of the optimal loss).  The iteration starts
    from a = (1 - tau) 1, which at tau near 0 or 1 and thousands of rows lies close to the boundary, where a predictor-corrector
    step can jam; how far inside the multipliers start decides it, so a start that does not close the gap gives way to the
    next one.  The gap is a certificate: whichever start closes it has found the optimum."""
    best = None
    for start in (0.1, 1.0, 10.0, 0.01, 100.0):
        got = _frisch_newton_from(U, y, tau, start)
        if best is None or got[1] - got[2] < best[1] - best[2]:
            best = got
        if best[1] - best[2] <= 1e-12 * max(best[1], 1e-300):
            break
    return best


def _frisch_newton_from(U, y, tau, start, max_it=200):
    n, r = U.shape
    c = -y
    x = np.full(n, 1.0 - tau)
    s = 1.0 - x
    b = U.T @ x
    yv = U.T @ c
    res = c - U @ yv
    eps = start * float(np.mean(np.abs(res))) + 1e-300      # both multipliers start positive; z - w = res stays exact to rounding
    z = np.maximum(res, 0.0) + eps
    w = np.maximum(-res, 0.0) + eps
    const = (1.0 - tau) * float(np.sum(y))

    def objectives(yv, x):
        rr = y + U @ yv                                  # y - U g with g = -yv
        primal = float(np.sum(np.where(rr >= 0, tau * rr, (tau - 1.0) * rr)))
        # the dual point projected back onto U'a = b (rounding drifts off it), then pulled towards the centre (1 - tau) 1 of
        # the box, which lies on U'a = b, by as much as the projection left the box: a feasible point, hence a lower bound
        a = x - U @ (U.T @ x - b)
        viol = max(float(np.max(-a)), float(np.max(a - 1.0)), 0.0)
        if viol > 0.0:
            a = (1.0 - tau) + (1.0 - viol / (viol + min(tau, 1.0 - tau))) * (a - (1.0 - tau))
        return primal, float(y @ a) - const

    best = (-yv, *objectives(yv, x))
    stall = 0
    for _ in range(max_it):
        primal, dual = best[1], best[2]
        if primal - dual <= 1e-14 * max(primal, 1e-300):
            break
        with np.errstate(all="ignore"):
            q = 1.0 / (z / x + w / s)
            rz = c - U @ yv                              # = z - w up to the drift of rounding, which this takes back
            UQ = U * q[:, None]
            M = U.T @ UQ
            rhs = UQ.T @ rz + (b - U.T @ x)
            if not np.isfinite(M).all():
                break
            solve = lambda v: np.linalg.lstsq(M, v, rcond=None)[0]  # noqa: E731  (q spans many decades near the optimum)
            dy = solve(rhs)
            dx = q * (U @ dy - rz)
            ds = -dx
            dz = -z * (1.0 + dx / x)
            dw = -w * (1.0 + ds / s)
            fp = min(0.9995 * min(_step_bound(x, dx).min(), _step_bound(s, ds).min()), 1.0)
            fd = min(0.9995 * min(_step_bound(w, dw).min(), _step_bound(z, dz).min()), 1.0)
            if min(fp, fd) < 1.0:
                mu = float(z @ x + w @ s)
                g = float((z + fd * dz) @ (x + fp * dx) + (w + fd * dw) @ (s + fp * ds))
                mu = mu * (g / mu) ** 3 / (2.0 * n)
                xinv, sinv = 1.0 / x, 1.0 / s
                # the second-order terms of x z = mu and s w = mu; a predictor that could move less than a tenth of its length
                # says nothing about them (they would jam the iterate at the boundary): a pure centring step then
                so = 1.0 if min(fp, fd) >= 0.1 else 0.0
                dxdz, dsdw = so * dx * dz * xinv, so * ds * dw * sinv
                xi = mu * (xinv - sinv)
                dy = solve(rhs + U.T @ (q * (dxdz - dsdw - xi)))
                dx = q * (U @ dy + xi - rz - dxdz + dsdw)
                ds = -dx
                dz = mu * xinv - z - xinv * z * dx - dxdz
                dw = mu * sinv - w - sinv * w * ds - dsdw
                frac = 0.9995 if so else 0.5                    # (and stays well inside after a centring step)
                fp = min(frac * min(_step_bound(x, dx).min(), _step_bound(s, ds).min()), 1.0)
                fd = min(frac * min(_step_bound(w, dw).min(), _step_bound(z, dz).min()), 1.0)
            x2, s2, yv2, w2, z2 = x + fp * dx, s + fp * ds, yv + fd * dy, w + fd * dw, z + fd * dz
        if not (np.isfinite(x2).all() and np.isfinite(yv2).all() and np.isfinite(w2).all() and np.isfinite(z2).all()
                and (x2 > 0).all() and (s2 > 0).all() and (w2 > 0).all() and (z2 > 0).all()):
            break
        x, s, yv, w, z = x2, s2, yv2, w2, z2
        p2, d2 = objectives(yv, x)
        if p2 - d2 < best[1] - best[2]:
            best, stall = (-yv, p2, d2), 0
        else:
            stall += 1
            if stall >= 4:
                break
    return best


def _vertex(AZ, yZ):
    """The k x k solve A_Z beta = y_Z in double, and once more with one step of iterative refinement in extended precision."""
    beta = np.linalg.solve(AZ, yZ)
    res = (yZ.astype(np.longdouble) - (AZ.astype(np.longdouble) * beta.astype(np.longdouble)).sum(axis=1)).astype(np.float64)
    refined = (beta.astype(np.longdouble) + np.linalg.solve(AZ, res).astype(np.longdouble)).astype(np.float64)
    return beta, refined


def _certified_vertex(A, yv, X, y, tau, fit_intercept, beta_guess, s):
    """The crossover from an approximate solution: the k rows of smallest |residual|, the vertex they define, its certificate.
    -> dict of the vertex, or None where the rows are singular or the certificate is not decided, optimal and strict."""
    k = A.shape[1]
    if len(yv) < k:
        return None
    r = np.abs(yv - A @ beta_guess)
    Z = np.sort(np.argsort(r, kind="stable")[:k])
    AZ = A[Z]
    if np.linalg.matrix_rank(AZ / s) < k:
        return None
    try:
        dbl, ref = _vertex(AZ, yv[Z])
    except np.linalg.LinAlgError:
        return None
    b, b0 = (ref[1:], float(ref[0])) if fit_intercept else (ref, float("nan"))
    cert = certify(X, y, tau, fit_intercept, b, b0)
    if not (cert["decided"] and cert["optimal"] and cert["strict"]):
        return None
    off = np.ones(len(yv), dtype=bool)
    off[Z] = False
    rv = np.abs(yv - A @ ref)[off]
    rv = rv[rv > 0]
    return dict(beta=ref, beta_double=dbl, kappa=float(np.linalg.cond(AZ / s)),
                rmin=float(rv.min() / np.max(np.abs(yv))) if rv.size else float("inf"))


def solve(X, y, tau, fit_intercept, warm=None):
    """The quantile regression fit of one group in numpy alone (the rows with finite y and x; k <= their number).
    -> dict(b, b0 (NaN without an intercept), loss, unique, kappa, gap, rmin, b_double, b0_double, rank):
      unique   the crossover found a vertex whose certificate is decided and strict; then b, b0 are that vertex (solved in
               double, refined once in extended precision; b_double / b0_double: the double solve alone), loss its loss,
               kappa the 2-norm condition number of A_Z with the columns scaled to unit max-abs over the valid rows, rmin the
               smallest non-zero |r| at the vertex over max|y|;
      else     b, b0, loss are the interior-point iterate's (for an aliased design the minimum-norm coefficients), kappa = inf,
               rmin = nan;
      gap      (primal - dual) / primal of the interior-point iterate, less the rounding of evaluating the primal: its loss is
               within that share of the optimum.  0.0 where the fit interpolates (loss <= 1e-12 max|y|: a loss cannot be negative) and where no iteration ran.
    `warm` (optional, (b, b0)): a candidate tried first — the optimum of a neighbouring tau is often the optimum of this one;
    it is accepted only with a decided, strict certificate at THIS tau, so the answer does not depend on it."""
    ok = valid_rows(X, y)
    Xv, yv = np.asarray(X, dtype=np.float64)[ok], np.asarray(y, dtype=np.float64)[ok]
    A = design(Xv, fit_intercept)
    n, k = A.shape
    ymax = float(np.max(np.abs(yv)))
    s = np.max(np.abs(A), axis=0)
    s = np.where(s > 0, s, 1.0)

    def result(v, gap, rank):
        beta, dbl = v["beta"], v["beta_double"]
        b, b0 = (beta[1:], float(beta[0])) if fit_intercept else (beta, float("nan"))
        bd, b0d = (dbl[1:], float(dbl[0])) if fit_intercept else (dbl, float("nan"))
        return dict(b=b, b0=b0, loss=pinball_loss(Xv, yv, tau, b, b0), unique=True, kappa=v["kappa"], gap=gap, rmin=v["rmin"],
                    b_double=bd, b0_double=b0d, rank=rank)

    if warm is not None and np.isfinite(warm[0]).all():
        guess = np.concatenate([[warm[1]], warm[0]]) if fit_intercept else np.asarray(warm[0], dtype=np.float64)
        v = _certified_vertex(A, yv, Xv, yv, tau, fit_intercept, guess, s)
        if v is not None:
            return result(v, 0.0, k)
    Uf, sv, Vt = np.linalg.svd(A / s, full_matrices=False)
    rank = int((sv > 1e-10 * sv[0]).sum()) if sv[0] > 0 else 0
    U = Uf[:, :rank]
    if ymax == 0.0 or rank == 0:
        g, primal, dual = np.zeros(rank), float(np.sum(np.where(yv >= 0, tau * yv, (tau - 1.0) * yv))), 0.0
        dual = primal if rank == 0 else dual
    elif n == rank or np.max(np.abs(yv - U @ (U.T @ yv))) <= 1e-13 * ymax:      # y lies in the column space: the loss is 0
        g = U.T @ yv
        primal = dual = 0.0
    else:
        g, primal, dual = _frisch_newton(U, yv / ymax, tau)
        g, primal, dual = g * ymax, primal * ymax, dual * ymax
    beta = (Vt[:rank].T @ (g / sv[:rank])) / s                                   # minimum norm in the scaled columns
    b, b0 = (beta[1:], float(beta[0])) if fit_intercept else (beta, float("nan"))
    loss = pinball_loss(Xv, yv, tau, b, b0)
    # the loss of any beta is evaluated from residuals that carry (k + 2) 2^-52 (|y_i| + |a_i|'|beta|) of rounding each: a gap
    # below that is not there (it matters where the fit nearly interpolates, the loss a 1e-6 of max|y|)
    noise = (k + 2) * 2.0 ** -52 * float(np.sum(np.abs(yv) + np.abs(A) @ np.abs(beta)))
    gap = 0.0 if loss <= 1e-12 * ymax else max(0.0, loss - dual - noise) / loss
    if rank == k:
        v = _certified_vertex(A, yv, Xv, yv, tau, fit_intercept, beta, s)
        if v is not None:
            return result(v, gap, rank)
    return dict(b=b, b0=b0, loss=loss, unique=False, kappa=float("inf"), gap=gap, rmin=float("nan"), b_double=b, b0_double=b0,
                rank=rank)
