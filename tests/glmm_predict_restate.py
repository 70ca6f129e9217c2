"""A dense restatement of the mixed model's prediction-error variance for the tests, sharing nothing with csrc/lmm_profile.h:
Henderson's mixed-model equations at a given theta = var_group / var_residual,

    C = [ X'X   X'Z           ]      var( [beta^ - beta; b^ - b] ) = s2 C^-1
        [ Z'X   Z'Z + I/theta ]

over the valid rows, with one column of Z per level of the panel whether or not it has a valid row (an unseen level has a zero
column and the diagonal 1 / theta alone).  A row with design a in level j then has the prediction-error variance
s2 [a; e_j]' C^-1 [a; e_j] and the prediction [a; e_j]' C^-1 [X'y; Z'y].  theta = 0 has b = 0 and is the ordinary least-squares
fit.  A dropped column is left out of X and of a.  closed_form() is section "Mixed-model fit-predict" of DESIGN.md §1 in numpy,
from the level means."""
import numpy as np


def design(x_cols, fit_intercept, keep=None):
    X = np.column_stack([np.asarray(c, float) for c in x_cols])
    if fit_intercept:
        X = np.column_stack([np.ones(len(X)), X])
    return X if keep is None else X[:, np.asarray(keep, bool)]


def henderson(y, X, levels, n_levels, theta, s2, A_new, levels_new):
    """y, X, levels: the valid rows.  -> (yhat, yhat_fixed, var) of the rows (A_new, levels_new)."""
    y, X, A_new = np.asarray(y, float), np.asarray(X, float), np.asarray(A_new, float)
    k = X.shape[1]
    if theta == 0.0:
        Ci = np.linalg.inv(X.T @ X)
        beta = Ci @ (X.T @ y)
        fixed = A_new @ beta
        return fixed, fixed, s2 * np.einsum("ij,jk,ik->i", A_new, Ci, A_new)
    Z = np.zeros((len(y), n_levels))
    Z[np.arange(len(y)), np.asarray(levels)] = 1.0
    C = np.block([[X.T @ X, X.T @ Z], [Z.T @ X, Z.T @ Z + np.eye(n_levels) / theta]])
    Ci = np.linalg.inv(C)
    sol = Ci @ np.concatenate([X.T @ y, Z.T @ y])
    T = np.zeros((len(A_new), k + n_levels))
    T[:, :k] = A_new
    T[np.arange(len(A_new)), k + np.asarray(levels_new)] = 1.0
    return T @ sol, A_new @ sol[:k], s2 * np.einsum("ij,jk,ik->i", T, Ci, T)


def closed_form(y, X, levels, n_levels, theta, s2, A_new, levels_new):
    """The same three through the level means: se^2 = s2 [c'A^-1 c + theta / (1 + n_j theta)], c = a - s_j abar_j."""
    y, X, A_new = np.asarray(y, float), np.asarray(X, float), np.asarray(A_new, float)
    levels, levels_new = np.asarray(levels), np.asarray(levels_new)
    k = X.shape[1]
    n = np.bincount(levels, minlength=n_levels).astype(float)
    abar, ybar = np.zeros((n_levels, k)), np.zeros(n_levels)
    for j in range(n_levels):
        if n[j] > 0:
            abar[j], ybar[j] = X[levels == j].mean(axis=0), y[levels == j].mean()
    lam = n / (1.0 + n * theta)
    Xc, yc = X - abar[levels], y - ybar[levels]
    A = Xc.T @ Xc + (abar * lam[:, None]).T @ abar
    beta = np.linalg.solve(A, Xc.T @ yc + abar.T @ (lam * ybar))
    s = theta * lam
    blup = s * (ybar - abar @ beta)
    fixed = A_new @ beta
    c = A_new - s[levels_new, None] * abar[levels_new]
    var = s2 * (np.einsum("ij,jk,ik->i", c, np.linalg.inv(A), c) + theta / (1.0 + n[levels_new] * theta))
    return fixed + blup[levels_new], fixed, var


def panel_reference(y, x_cols, levels, n_levels, fit_intercept, theta, s2, keep=None):
    """Every row of one panel (levels: 0-based within the panel) scored by the Henderson form fitted on the panel's valid rows at
    the given theta and s2; rows with an x that is not finite come back NaN.  -> (yhat, yhat_fixed, se)"""
    y = np.asarray(y, float)
    X = design(x_cols, fit_intercept, keep)
    levels = np.asarray(levels)
    xok = np.all(np.isfinite(X), axis=1)
    ok = xok & np.isfinite(y)
    out = np.full((3, len(y)), np.nan)
    yh, yf, var = henderson(y[ok], X[ok], levels[ok], n_levels, theta, s2, X[xok], levels[xok])
    out[0, xok], out[1, xok], out[2, xok] = yh, yf, np.sqrt(var)
    return out
