"""Empirical-Bayes shrinkage restated from its formulas ("Empirical-Bayes shrinkage"), for the tests: numpy with
np.longdouble sums, nothing shared with csrc/eb_shrink.h.

    usable pair: est finite, se finite and > 0;  k usable pairs;  sums over usable pairs only
    w = 1/se^2, Sw = sum w, fixed = sum w est / Sw, Q = sum w (est - fixed)^2, df = k - 1, C = Sw - sum w^2 / Sw
    tau^2 = the fixed value | 0 (none) | max(0, (Q - df) / C) if C > 0 else 0
    wr = 1/(se^2 + tau^2), mu = sum wr est / sum wr, mu_se = sqrt(1 / sum wr), I^2 = clamp((Q - df)/Q, 0, 1) if Q > df and Q > 0 else 0
"""
import math

import numpy as np

LD = np.longdouble
DL, NONE = 0, 1
SUMMARY = ("mu", "mu_se", "tau_squared", "i_squared", "q", "n_groups", "n_input", "status")


def options_invalid(method, tau_squared):
    if method not in (DL, NONE):
        return True
    t = float("nan") if tau_squared is None else float(tau_squared)
    return not math.isnan(t) and not (t >= 0.0 and math.isfinite(t))


def shrink_set(est, se, method=DL, tau_squared=None):
    """One set -> (summary[8], out[m, 3], q_minus_df): the summary in float64 of values computed in long double; q_minus_df
    (a float, NaN for a failed set) is what decides the clamp of tau^2 and I^2."""
    est, se = np.asarray(est, np.float64), np.asarray(se, np.float64)
    m = len(est)
    out = np.full((m, 3), np.nan)
    fail = np.full(8, np.nan)
    ok = np.isfinite(est) & np.isfinite(se) & (se > 0)
    k = int(ok.sum())
    status = 1 if options_invalid(method, tau_squared) else 10 if m == 0 else 6 if k < 2 else 0
    if status:
        fail[7] = status
        return fail, out, float("nan")
    e, s = est[ok].astype(LD), se[ok].astype(LD)
    w = 1 / (s * s)
    sw = w.sum()
    fixed = (w * e).sum() / sw
    q = (w * (e - fixed) ** 2).sum()
    df = LD(k - 1)
    if tau_squared is not None and not math.isnan(tau_squared):
        tau2 = LD(tau_squared)
    elif method == NONE:
        tau2 = LD(0)
    else:
        c = sw - (w * w).sum() / sw
        tau2 = max(LD(0), (q - df) / c) if c > 0 else LD(0)
    wr = 1 / (s * s + tau2)
    swr = wr.sum()
    mu = (wr * e).sum() / swr
    mu_se = np.sqrt(1 / swr)
    i2 = min(max((q - df) / q, LD(0)), LD(1)) if q > df and q > 0 else LD(0)
    if tau2 > 0:
        pw, pb = w, 1 / tau2
        wt = pw / (pw + pb)
        out[ok, 0] = (wt * e + (1 - wt) * mu).astype(np.float64)
        out[ok, 1] = np.sqrt(1 / (pw + pb)).astype(np.float64)
        out[ok, 2] = wt.astype(np.float64)
    else:
        out[ok, 0], out[ok, 1], out[ok, 2] = float(mu), float(mu_se), 0.0
    return np.array([mu, mu_se, tau2, i2, q, k, m, 0], dtype=np.float64), out, float(q - df)


def shrink_batch(set_offsets, n_cols, est, est_stride, se, se_stride, method=DL, tau_squared=None):
    """The matrix form: -> (out[n_items, n_cols, 3], summary[n_sets, n_cols, 8], q_minus_df[n_sets, n_cols]); items outside
    every set stay NaN."""
    off = np.asarray(set_offsets, np.int64)
    n_sets = len(off) - 1
    n_items = int(off[-1]) if n_sets >= 0 else 0
    est, se = np.asarray(est, np.float64).ravel(), np.asarray(se, np.float64).ravel()
    out = np.full((n_items, n_cols, 3), np.nan)
    summary = np.full((max(n_sets, 0), n_cols, 8), np.nan)
    qd = np.full((max(n_sets, 0), n_cols), np.nan)
    for s in range(n_sets):
        g = np.arange(off[s], off[s + 1])
        for c in range(n_cols):
            summary[s, c], out[off[s]:off[s + 1], c], qd[s, c] = shrink_set(est[g * est_stride + c], se[g * se_stride + c], method,
                                                                            tau_squared)
    return out, summary, qd
