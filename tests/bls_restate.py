"""A NumPy restatement of the bounded least squares contract ("Bounded least squares") that works on the
ROWS: the reference's row filter, constant-column rule, shortcut and statuses, then an active-set solve whose free set is
fitted by `lstsq` on the free columns (an intercept as a column of ones), flags and the ssr summed from residuals.  It is the
yardstick of the BLS tests and shares no code with the library: the library sees only moments, this sees only rows.

Also here: the conditions the tests put on generated inputs (conditions on the INPUT, asserted on this module's output) and
the comparison of a library record with a restated one at the project's tolerances."""
import numpy as np

STATUS_INVALID_INPUT, STATUS_INSUFFICIENT, STATUS_NO_VALID, STATUS_TOO_FEW_ROWS = 1, 6, 10, 100


def resolve_bounds(p, lower, upper):
    """(lo[p], hi[p]) per original column, or None when the bounds are unusable (status 1).  Both absent = NNLS."""
    def side(b, default):
        if b is None:
            return np.full(p, default)
        b = np.atleast_1d(np.asarray(b, dtype=np.float64))
        if len(b) == 0:
            return np.full(p, default)
        if len(b) == 1:
            return np.full(p, b[0])
        if len(b) != p:
            return None
        return b.copy()
    absent = lambda b: b is None or len(np.atleast_1d(b)) == 0  # noqa: E731
    if absent(lower) and absent(upper):
        return np.zeros(p), np.full(p, np.inf)
    lo, hi = side(lower, -np.inf), side(upper, np.inf)
    if lo is None or hi is None or np.isnan(lo).any() or np.isnan(hi).any() or (lo > hi).any():
        return None
    return lo, hi


def _solve_free(Xs, y, free, b, icpt):
    """lstsq of y - X_B b_B on the free columns (and a column of ones): the free coefficients and the intercept."""
    n = len(y)
    rhs = y - Xs[:, ~free] @ b[~free]
    cols = [np.ones((n, 1))] if icpt else []
    cols.append(Xs[:, free])
    A = np.concatenate(cols, axis=1)
    if A.shape[1] == 0:
        return np.empty(0), 0.0
    sol = np.linalg.lstsq(A, rhs, rcond=None)[0]
    return (sol[1:], sol[0]) if icpt else (sol, 0.0)


def active_set_rows(X, y, lo, hi, icpt, max_iterations=1000):
    """The minimiser of ||y - b0 - X b||^2 over lo <= b <= hi from the rows.  Columns are scaled to unit norm for the
    solve (bounds scaled with them).  Returns (b, b0, on_lower, on_upper, outer iterations)."""
    n, p = X.shape
    nrm = np.linalg.norm(X - (X.mean(axis=0) if icpt else 0.0), axis=0)
    Xs = X / nrm
    los, his = lo * nrm, hi * nrm
    on_lo = np.isfinite(lo)
    on_hi = ~on_lo & np.isfinite(hi)
    free = ~(on_lo | on_hi)
    z = np.where(on_lo, los, np.where(on_hi, his, 0.0))
    z0 = 0.0
    ynorm = np.linalg.norm(y - (y.mean() if icpt else 0.0))
    tau = 1e-12 * max(ynorm, 1e-300)
    blocked = np.zeros(p, dtype=bool)
    iters = 0
    pending = free.any() or icpt
    jstar, star_side = -1, 0
    while True:
        if not pending:
            r = y - z0 - Xs @ z
            w = Xs.T @ r
            viol = np.where(on_lo, w, np.where(on_hi, -w, 0.0))
            viol[blocked] = 0.0
            j = int(np.argmax(viol))
            if not viol[j] > tau or iters >= max_iterations:
                break
            iters += 1
            jstar, star_side = j, (1 if on_lo[j] else 2)
            free[j], on_lo[j], on_hi[j] = True, False, False
        pending = False
        for _ in range(p + 1):
            s, s0 = _solve_free(Xs, y, free, z, icpt)
            zf = z[free]
            d = s - zf
            lf, hf = los[free], his[free]
            below, above = s < lf, s > hf
            if not (below.any() or above.any()):
                z[free], z0 = s, s0
                break
            with np.errstate(divide="ignore", invalid="ignore"):
                a = np.where(below, (lf - zf) / d, np.where(above, (hf - zf) / d, np.inf))
            a = np.clip(a, 0.0, None)
            k = int(np.argmin(a))
            alpha = min(a[k], 1.0)
            zn = zf + alpha * d
            idx = np.nonzero(free)[0]
            hit_lo = (zn < lf) | ((np.arange(len(idx)) == k) & below)
            hit_hi = ~hit_lo & ((zn > hf) | ((np.arange(len(idx)) == k) & above))
            zn = np.where(hit_lo, lf, np.where(hit_hi, hf, zn))
            z[idx] = zn
            on_lo[idx[hit_lo]] = True
            on_hi[idx[hit_hi]] = True
            free[idx[hit_lo | hit_hi]] = False
            if icpt:                                   # the intercept of the point moved to
                z0 = float(np.mean(y - Xs @ z))
        back = jstar >= 0 and ((star_side == 1 and on_lo[jstar]) or (star_side == 2 and on_hi[jstar]))
        if back:
            blocked[jstar] = True
        else:
            blocked[:] = False
    b = np.where(on_lo, lo, np.where(on_hi, hi, z / nrm))
    b0 = float(np.mean(y - X @ b)) if icpt else 0.0
    return b, b0, on_lo, on_hi, iters


def fit_bls(y, X, fit_intercept=False, lower=None, upper=None, max_iterations=1000, tolerance=1e-10, rule_count=None):
    """One group.  X is [n, p].  Returns a dict: status and, for status 0, coefficients[p] (NaN at constant columns),
    intercept (NaN without one), ssr, r_squared, n_observations, n_active_constraints, at_lower_bound[p], at_upper_bound[p];
    plus held_lower / held_upper (columns the solve holds on a bound), multipliers g = x_j'r, iterations and the valid rows."""
    y = np.asarray(y, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    X = X if X.ndim == 2 else X.reshape(len(y), -1)
    n, p = X.shape
    out = {"status": 0, "p": p}
    if (n if rule_count is None else rule_count) < 2:
        out["status"] = STATUS_TOO_FEW_ROWS
        return out
    bounds = resolve_bounds(p, lower, upper)
    if bounds is None:
        out["status"] = STATUS_INVALID_INPUT
        return out
    lo, hi = bounds
    ok = np.isfinite(y) & np.isfinite(X).all(axis=1)
    if not ok.any():
        out["status"] = STATUS_NO_VALID
        return out
    yv, Xv = y[ok], X[ok]
    nv = len(yv)
    const = (np.abs(Xv - Xv[0]) < 1e-10).all(axis=0)
    k = int((~const).sum())
    nanp = np.full(p, np.nan)
    if k == 0:
        if not fit_intercept:
            out["status"] = STATUS_INSUFFICIENT
            return out
        out.update(coefficients=nanp, intercept=float(yv.mean()), ssr=np.nan, r_squared=0.0, n_observations=nv,
                   n_active_constraints=0, at_lower_bound=np.zeros(p, bool), at_upper_bound=np.zeros(p, bool),
                   held_lower=np.zeros(p, bool), held_upper=np.zeros(p, bool), g=np.zeros(p), iterations=0, valid=ok,
                   lo=lo, hi=hi, const=const)
        return out
    if nv < k + (1 if fit_intercept else 0):
        out["status"] = STATUS_INSUFFICIENT
        return out
    Xr = Xv[:, ~const]
    b, b0, on_lo, on_hi, iters = active_set_rows(Xr, yv, lo[~const], hi[~const], fit_intercept, max_iterations)
    r = yv - b0 - Xr @ b
    ssr = float(r @ r)
    tss = float(((yv - yv.mean()) ** 2).sum()) if fit_intercept else float(yv @ yv)
    coef = nanp.copy()
    coef[~const] = b
    at_lo, at_hi = np.zeros(p, bool), np.zeros(p, bool)
    for j in np.nonzero(~const)[0]:
        if np.isfinite(lo[j]) and abs(coef[j] - lo[j]) < tolerance:
            at_lo[j] = True
        elif np.isfinite(hi[j]) and abs(coef[j] - hi[j]) < tolerance:
            at_hi[j] = True
    held_lo, held_hi, g = np.zeros(p, bool), np.zeros(p, bool), np.zeros(p)
    held_lo[~const], held_hi[~const] = on_lo, on_hi
    g[~const] = Xr.T @ r
    out.update(coefficients=coef, intercept=(b0 if fit_intercept else np.nan), ssr=ssr, r_squared=1.0 - ssr / tss,
               n_observations=nv, n_active_constraints=int(at_lo.sum() + at_hi.sum()), at_lower_bound=at_lo,
               at_upper_bound=at_hi, held_lower=held_lo, held_upper=held_hi, g=g, iterations=iters, valid=ok, lo=lo, hi=hi,
               const=const)
    return out


def record(res):
    """The library's 3p + 6 record of a restated fit."""
    p = res["p"]
    rec = np.full(3 * p + 6, np.nan)
    rec[p + 5] = res["status"]
    if res["status"] != 0:
        return rec
    rec[:p] = res["coefficients"]
    rec[p] = res["intercept"]
    rec[p + 1], rec[p + 2], rec[p + 3], rec[p + 4] = res["ssr"], res["r_squared"], res["n_observations"], res["n_active_constraints"]
    rec[p + 6:2 * p + 6] = res["at_lower_bound"]
    rec[2 * p + 6:] = res["at_upper_bound"]
    return rec


def kkt_residuals(res, y, X, fit_intercept):
    """(worst free |g|, worst wrong-signed multiplier) / (||x_j|| ||y||) over the non-constant columns."""
    ok, const = res["valid"], res["const"]
    yv, Xv = np.asarray(y)[ok], np.asarray(X)[ok]
    scale = np.linalg.norm(Xv, axis=0) * np.linalg.norm(yv)
    g = res["g"]
    free = ~const & ~res["held_lower"] & ~res["held_upper"]
    worst_free = float(np.max(np.abs(g[free]) / scale[free])) if free.any() else 0.0
    wrong = 0.0
    if res["held_lower"].any():   # at a lower bound the objective must not fall when b_j grows: x_j'r <= 0
        wrong = max(wrong, float(np.max(g[res["held_lower"]] / scale[res["held_lower"]])))
    if res["held_upper"].any():
        wrong = max(wrong, float(np.max(-g[res["held_upper"]] / scale[res["held_upper"]])))
    return worst_free, wrong


def input_conditions(res, y, X, fit_intercept, tolerance=1e-10):
    """The conditions the GPU tests put on a generated case (on the restatement's output); a list of violations."""
    bad = []
    if res["status"] != 0 or np.isnan(res.get("ssr", np.nan)):
        return bad
    ok, const = res["valid"], res["const"]
    yv, Xv = np.asarray(y)[ok], np.asarray(X)[ok][:, ~const]
    b, lo, hi = res["coefficients"][~const], res["lo"][~const], res["hi"][~const]
    for bound in (lo, hi):
        d = np.abs(b - bound)
        d = d[np.isfinite(d)]
        if ((d > tolerance / 10) & (d < 10 * tolerance)).any():
            bad.append("a coefficient lies within (tolerance / 10, 10 tolerance) of a bound")
    held = (res["held_lower"] | res["held_upper"])[~const]
    scale = np.linalg.norm(Xv, axis=0) * np.linalg.norm(yv)
    if held.any() and (np.abs(res["g"][~const][held]) < 1e-6 * scale[held]).any():
        bad.append("a held bound has a multiplier below 1e-6 ||x_j|| ||y|| (degenerate vertex)")
    D = np.concatenate([np.ones((len(yv), 1)), Xv], axis=1) if fit_intercept else Xv
    sv = np.linalg.svd(D / np.linalg.norm(D, axis=0), compute_uv=False)
    if sv[0] > 1e6 * sv[-1]:
        bad.append("column-scaled design condition number above 1e6")
    return bad


def moment_conditions(res, y, X, fit_intercept, tolerance=1e-10):
    """input_conditions with the bound on the design that a solver of MOMENTS can be held to: it loses about
    p kappa^2 2^-53, so 1e-9 on the coefficients needs  p kappa^2 2^-53 <= 1e-10  (kappa <= 335 at p = 8, 84 at p = 128) of the
    column-scaled design of the non-constant columns (with the ones column when there is an intercept) — far inside
    input_conditions' 1e6.  The randomised family sweeps assert this variant."""
    bad = input_conditions(res, y, X, fit_intercept, tolerance)
    if res["status"] != 0 or np.isnan(res.get("ssr", np.nan)):
        return bad
    ok, const = res["valid"], res["const"]
    Xv = np.asarray(X)[ok][:, ~const]
    D = np.concatenate([np.ones((len(Xv), 1)), Xv], axis=1) if fit_intercept else Xv
    sv = np.linalg.svd(D / np.linalg.norm(D, axis=0), compute_uv=False)
    kappa = sv[0] / sv[-1] if sv[-1] > 0 else np.inf
    res["kappa"] = float(kappa)
    if not res["p"] * kappa * kappa * 2.0 ** -53 <= 1e-10:
        bad.append(f"p kappa^2 2^-53 above 1e-10 (kappa {kappa:.3g})")
    return bad


def assert_record_matches(rec, ref, p, xbar=None, what="", coef_rtol=1e-9, diag_rtol=1e-6):
    """A library record against a restated one: coefficients within coef_rtol max(|ref_j|, 1e-3 max_k |ref_k|), the
    intercept with its sum |xbar_j| tol_j allowance, ssr and r2 within diag_rtol relative / 1e-12 absolute, n, flags,
    n_active and the status exactly (the rules of conftest.assert_records_match)."""
    rec, ref = np.asarray(rec), np.asarray(ref)
    assert rec.shape == ref.shape == (3 * p + 6,), what
    assert rec[p + 5] == ref[p + 5], f"{what}: status {rec[p + 5]} vs {ref[p + 5]}"
    if ref[p + 5] != 0:
        return
    c, rc = rec[:p], ref[:p]
    assert np.array_equal(np.isnan(c), np.isnan(rc)), f"{what}: NaN pattern of coefficients differs"
    with np.errstate(all="ignore"):
        scale = np.nanmax(np.abs(np.concatenate([rc, ref[p:p + 1]])))
    scale = scale if np.isfinite(scale) else 0.0
    tol = coef_rtol * np.maximum(np.abs(rc), 1e-3 * scale)
    m = ~np.isnan(rc)
    if m.any():
        worst = np.max(np.abs(c - rc)[m] / np.maximum(tol[m], 1e-300))
        assert worst <= 1.0, f"{what}: coefficients off by {worst:.3g} x tolerance"
    assert np.isnan(rec[p]) == np.isnan(ref[p]), f"{what}: intercept NaN pattern differs"
    if not np.isnan(ref[p]):
        itol = coef_rtol * max(abs(ref[p]), 1e-3 * scale)
        if xbar is not None:
            itol += float(np.nansum(np.abs(xbar) * np.where(m, tol, 0.0)))
        assert abs(rec[p] - ref[p]) <= itol, f"{what}: intercept off by {abs(rec[p] - ref[p]) / itol:.3g} x tolerance"
    for k, name in ((1, "ssr"), (2, "r_squared")):
        g, r = rec[p + k], ref[p + k]
        assert np.isnan(g) == np.isnan(r), f"{what}: NaN pattern of {name} differs"
        if not np.isnan(r):
            assert abs(g - r) <= diag_rtol * abs(r) + 1e-12, f"{what}: {name} {g!r} vs {r!r}"
    assert rec[p + 3] == ref[p + 3], f"{what}: n_observations {rec[p + 3]} vs {ref[p + 3]}"
    assert rec[p + 4] == ref[p + 4], f"{what}: n_active_constraints {rec[p + 4]} vs {ref[p + 4]}"
    assert np.array_equal(rec[p + 6:], ref[p + 6:]), f"{what}: bound flags differ"


def make_case(rng, n, p, offsets=True, noise=1.0):
    """The generator of the design study: uniform(-10, 10) columns with offsets, Gaussian beta and noise."""
    X = rng.uniform(-10.0, 10.0, size=(n, p)) + (rng.normal(size=p) * 3.0 if offsets else 0.0)
    beta = rng.normal(size=p)
    y = X @ beta + 0.7 + noise * rng.normal(size=n)
    return y, X


def pivot_table():
    """The table of the reference's test/sql/regression/test_bls_nnls_pivot.test (12 rows, y = 7 c0 + 2 c1 + 0.5 c2)."""
    i = np.arange(12)
    c0 = (i % 4) * 0.001 + 0.001
    c1 = ((i * 3) % 5) * 1000.0 + 5.0
    c2 = ((i * 7) % 6) * 10.0 + 1.0
    X = np.stack([c0, c1, c2], axis=1)
    return 7.0 * c0 + 2.0 * c1 + 0.5 * c2, X
