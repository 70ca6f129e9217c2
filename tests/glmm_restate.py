"""A restatement of the Gaussian random-intercept mixed model for the tests: row-based and dense, in numpy / scipy, sharing
nothing with csrc/lmm_profile.h.  Per panel it builds V = I + theta ZZ' over the valid rows and evaluates the profiled
log-likelihood and its score through P = V^-1 - V^-1 X (X'V^-1 X)^-1 X'V^-1; theta^ is brentq's root of the score in log theta
on [1e-10, 1e10], 0 when the score is not positive at the lower end, and the upper end when it is not negative there."""
import numpy as np
from scipy.optimize import brentq

THETA_LO, THETA_HI = 1e-10, 1e10


class Dense:
    def __init__(self, y, X, levels, reml):
        self.y, self.X, self.reml = np.asarray(y, float), np.asarray(X, float), bool(reml)
        self.n, self.k = self.X.shape
        uniq, inv = np.unique(levels, return_inverse=True)
        self.Z = np.zeros((self.n, len(uniq)))
        self.Z[np.arange(self.n), inv] = 1.0
        self.ZZ = self.Z @ self.Z.T
        self.m = self.n - self.k if self.reml else self.n

    def parts(self, theta):
        Vi = np.linalg.inv(np.eye(self.n) + theta * self.ZZ)
        XtVi = self.X.T @ Vi
        A = XtVi @ self.X
        Ai = np.linalg.inv(A)
        P = Vi - XtVi.T @ Ai @ XtVi
        return Vi, A, Ai, P

    def ell_score(self, theta):
        Vi, A, Ai, P = self.parts(theta)
        rss = float(self.y @ P @ self.y)
        s2 = rss / self.m
        logdet_v = -np.linalg.slogdet(Vi)[1]
        ell = -0.5 * (self.m * np.log(2 * np.pi * s2) + logdet_v + self.m + (np.linalg.slogdet(A)[1] if self.reml else 0.0))
        Py = P @ self.y
        tr = np.sum(P * self.ZZ) if self.reml else np.sum(Vi * self.ZZ)
        score = -0.5 * (tr - (self.m / rss) * float(Py @ self.ZZ @ Py))
        return ell, score

    def fit(self):
        g = lambda u: np.exp(u) * self.ell_score(np.exp(u))[1]   # noqa: E731
        converged = True
        if not g(np.log(THETA_LO)) > 0.0:
            theta = 0.0
        elif not g(np.log(THETA_HI)) < 0.0:
            theta, converged = THETA_HI, False
        else:
            theta = float(np.exp(brentq(g, np.log(THETA_LO), np.log(THETA_HI), xtol=1e-13, rtol=1e-15)))
        Vi, A, Ai, P = self.parts(theta)
        beta = Ai @ (self.X.T @ Vi @ self.y)
        ell = self.ell_score(theta)[0]
        s2 = float(self.y @ P @ self.y) / self.m
        res = self.y - self.X @ beta
        blup = theta * (self.Z.T @ (Vi @ res))
        curvature = np.nan
        if theta > 0.0 and converged:
            h, u = 1e-3, np.log(theta)
            curvature = -(g(u + h) - g(u - h)) / (2 * h)   # - d^2 ell / du^2 at the root
        return dict(theta=theta, beta=beta, sigma2=s2, var_group=theta * s2, icc=theta / (1 + theta), ell=ell,
                    se=np.sqrt(s2 * np.diag(Ai)), blup=blup, cond=float(np.linalg.cond(A)), curvature=float(curvature),
                    converged=converged, n=self.n, n_groups=self.Z.shape[1], K=self.k + 2)


def fit_panel(y, x_cols, levels, fit_intercept=True, reml=True):
    """The valid rows of one panel -> Dense.fit(), or the status (10, 1, 6) of a panel that cannot be fitted.  blup comes back
    per sorted unique level among the valid rows."""
    y = np.asarray(y, float)
    X = np.column_stack([np.asarray(c, float) for c in x_cols])
    ok = np.isfinite(y) & np.all(np.isfinite(X), axis=1)
    levels = np.asarray(levels)[ok]
    y, X = y[ok], X[ok]
    if fit_intercept:
        X = np.column_stack([np.ones(len(y)), X])
    n, k = X.shape
    if n == 0:
        return 10
    uniq = np.unique(levels)
    if len(uniq) < 2:
        return 1
    if n <= k + 1:
        return 6
    if n == len(uniq):
        return 1
    out = Dense(y, X, levels, reml).fit()
    out["levels"] = uniq
    return out
